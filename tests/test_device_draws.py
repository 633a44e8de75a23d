"""The draws a training iteration makes on the device (csrc/dn_rng.h: Philox-4x32-10 uniforms, Box-Muller normals, the Feistel pixel
permutation, the drawn view, the iteration counter) against oracle/exact_rng.py, a numpy restatement in integer arithmetic that shares no
code with the library - and the numbers the sampling / compositing kernels draw themselves against dn_rng_fill at ragged shapes.

Everything is integer arithmetic or an exact fp32 product, so every comparison is assert_array_equal; only the Box-Muller normals carry
a gate, measured against torch's own fp32 evaluation of the same formula on the device.

CPU part: the restatement reproduces the Random123 known-answer vectors, is a permutation at every size used below, and re-derives the
two planted records (a word whose top 24 bits are all ones / all zeros: the largest uniform and u1 == 1; uniform 0 and the smallest u1)."""
import numpy as np
import pytest
import torch

F = np.float32
U32 = 0xFFFFFFFF

SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 0xDEADBEEFCAFEF00D)
FIRST_ITERATIONS = (0, 1, 2 ** 31, 2 ** 32 - 1)
FILL_SIZES = (1, 255, 256, 257, 65537)     # the edges of dn_rng_fill's 256-thread block, and more than one 16-bit index range

# n = 4^k - 1, 4^k, 4^k + 1 for k = 1..6: just above 4^k the Feistel domain is almost 4 n and the cycle walk at its longest
IMAGE_SIZES = ((1, 1), (1, 2), (2, 2), (1, 5), (4, 4), (1, 17), (8, 8), (5, 13), (16, 16), (257, 1), (32, 32), (25, 41), (64, 64),
               (17, 241), (37, 29),
               (1, 3), (3, 5), (7, 9), (15, 17), (31, 33), (63, 65))      # 4^k - 1: the whole domain but one value
PAIR_SHAPES = ((3, 5, 7), (4, 8, 8), (5, 41, 5), (1, 37, 29))     # (V, H, W)
DRAW_SEEDS = (11, 0xDEADBEEFCAFEF00D)
DRAW_ITERATIONS = (0, 3, 2 ** 32 - 1)

# (seed, iteration, stream, index, word 0): found once by a search over index < 65536 (about 2^24 trials each)
PLANT_ONES = (7, 1131, 0, 23249, 0xFFFFFFF0)      # w0 >> 8 == 0xFFFFFF: uniform 1 - 2^-24, u1 == 1
PLANT_ZEROS = (7, 1215, 1, 17555, 0x00000038)     # w0 >> 8 == 0: uniform 0, u1 == 2^-24

Z_MAX = 5.7681      # sqrt(-2 ln 2^-24) = sqrt(48 ln 2): the largest |z| Box-Muller can return on 24-bit uniforms


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU: the yardstick -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_restated_philox_reproduces_the_random123_known_answers(counter, key, want):
    """The three philox4x32_10 vectors of the Random123 distribution (kat_vectors), through philox4x32_10 and through rng_words' layout
    key = (seed_lo, seed_hi), counter = (index_lo, index_hi, stream, iteration) - the only cover of a non-zero high index word."""
    from oracle import exact_rng as ex
    assert tuple(int(w) for w in ex.philox4x32_10(*key, *counter)) == want
    seed, index = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
    assert tuple(int(w) for w in ex.rng_words(seed, counter[3], counter[2], index)) == want
    got = ex.rng_words(seed, counter[3], counter[2], np.array([index, index], dtype=np.uint64))
    assert all(w.shape == (2,) and int(w[0]) == int(w[1]) == x for w, x in zip(got, want))


def test_restated_uniform_and_view_on_the_anchor_word():
    from oracle import exact_rng as ex
    u = ex.uniform(0, 0, 0, np.arange(3))
    assert u.dtype == F and u[0] == F(0x6627e8) / F(2 ** 24) and 0.0 <= float(u.min()) and float(u.max()) < 1.0
    w0 = int(ex.rng_words(9, 4, 5, 0)[0])
    assert [ex.drawn_view(9, 4, v) for v in (1, 2, 5, 7)] == [w0 % v for v in (1, 2, 5, 7)]


def test_restated_feistel_is_a_permutation_at_every_size_drawn_below():
    """sorted(perm(arange(n))) == arange(n) for every image and pair size of the GPU tests, two seeds (one with a high word), two
    iterations; the bit count is the smallest even one covering n, so n = 4^k + 1 walks a domain of 4^(k+1)."""
    from oracle import exact_rng as ex
    sizes = sorted({h * w for h, w in IMAGE_SIZES} | {v * h * w for v, h, w in PAIR_SHAPES})
    for k in range(1, 7):
        assert {4 ** k - 1, 4 ** k, 4 ** k + 1} <= set(sizes)
        assert ex.feistel_bits(4 ** k) == 2 * k and ex.feistel_bits(4 ** k + 1) == 2 * k + 2 and ex.feistel_bits(4 ** k - 1) == 2 * k
    assert ex.feistel_bits(1) == ex.feistel_bits(2) == ex.feistel_bits(3) == 2
    for n in sizes:
        for seed in DRAW_SEEDS:
            for iteration in (0, 2 ** 32 - 1):
                perm = ex.feistel_permute(np.arange(n), n, seed, iteration)
                assert perm.dtype == np.int64
                np.testing.assert_array_equal(np.sort(perm), np.arange(n), err_msg=f"n={n} seed={seed:#x} iteration={iteration}")
    a, b = ex.feistel_permute(np.arange(1073), 1073, 11, 0), ex.feistel_permute(np.arange(1073), 1073, 11, 1)
    assert not np.array_equal(a, b)
    np.testing.assert_array_equal(ex.feistel_permute(np.arange(7), 1073, 11, 0), a[:7])


def test_planted_records_hold_the_extreme_words():
    from oracle import exact_rng as ex
    seed, iteration, stream, index, word = PLANT_ONES
    assert int(ex.rng_words(seed, iteration, stream, index)[0]) == word and word >> 8 == 0xFFFFFF and index < 65536
    assert ex.uniform(seed, iteration, stream, index) == F(1.0) - F(2.0 ** -24)
    z, u1, _ = ex.normal_f64(seed, iteration, stream, index)
    assert u1 == F(1.0) and z == 0.0
    seed, iteration, stream, index, word = PLANT_ZEROS
    assert int(ex.rng_words(seed, iteration, stream, index)[0]) == word and word >> 8 == 0 and index < 65536
    assert ex.uniform(seed, iteration, stream, index) == F(0.0)
    z, u1, _ = ex.normal_f64(seed, iteration, stream, index)
    assert u1 == F(2.0 ** -24) and np.isfinite(z) and abs(z) <= Z_MAX
    assert abs(np.sqrt(48.0 * np.log(2.0)) - Z_MAX) < 1e-4


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(hiplib):
    assert torch.cuda.is_available()
    import nerf
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


def C(t):
    return t.detach().cpu().numpy()


def words(state):
    """The four words of an RNG state record as unsigned integers."""
    return [w & U32 for w in state.tolist()]


def _record_measurement(key, values):
    from test_hip_parity import _record_measurement as record      # the suite's measurement record
    record(key, values)


@pytest.mark.gpu
def test_rng_fill_uniforms_bit_equal_to_the_restatement(dev):
    """dn_rng_fill, uniforms: every seed x every stream, the first iteration and the size rotating so that every value of both appears
    with every stream and every stream meets three non-zero iterations (exchanged counter words cannot agree); the anchor literal; the
    two planted records."""
    from nerf import _ops
    from oracle import exact_rng as ex
    seen = set()
    for si, seed in enumerate(SEEDS):
        for stream in range(6):
            iteration = FIRST_ITERATIONS[(si + stream) % 4]
            n = FILL_SIZES[(si + 2 * stream) % 5]
            seen |= {("it", stream, iteration), ("n", n)}
            got = C(_ops.rng_fill(_ops.new_rng_state(seed, dev, iteration), stream, (n,)))
            assert got.dtype == F
            np.testing.assert_array_equal(got, ex.uniform(seed, iteration, stream, np.arange(n)),
                                          err_msg=f"seed={seed:#x} iteration={iteration} stream={stream} n={n}")
    assert all(("n", n) in seen for n in FILL_SIZES) and all(any(("it", s, it) in seen for s in range(6)) for it in FIRST_ITERATIONS)
    assert all(sum(("it", s, it) in seen for it in FIRST_ITERATIONS[1:]) >= 3 for s in range(6))
    assert float(_ops.rng_fill(_ops.new_rng_state(0, dev), 0, (1,))[0]) == 0x6627e8 / 2 ** 24
    for (seed, iteration, stream, index, _), want in ((PLANT_ONES, 1.0 - 2.0 ** -24), (PLANT_ZEROS, 0.0)):
        got = C(_ops.rng_fill(_ops.new_rng_state(seed, dev, iteration), stream, (index + 1,)))
        assert float(got[index]) == want
        np.testing.assert_array_equal(got, ex.uniform(seed, iteration, stream, np.arange(index + 1)))


@pytest.mark.gpu
def test_rng_fill_normals_against_float64_box_muller(dev):
    """dn_rng_fill, normals, 65,537 elements for two seeds on the two noise streams: the worst absolute error against Box-Muller in
    float64 on the same fp32 u1 and angle is at most max(2 x the worst error of torch's fp32 sqrt(-2 log(u1)) cos(angle) on the device,
    fed the same u1 and angle, 4 fp32 ulps of [4, 8) = 1.9e-6); no non-finite value; at the planted records u1 == 1 gives 0 and
    u1 == 2^-24 a finite |z| <= sqrt(48 ln 2)."""
    from nerf import _ops
    from oracle import exact_rng as ex
    n = 65537
    floor = 4.0 * 2.0 ** -21
    worst_lib = worst_torch = 0.0
    for seed, iteration, stream in ((SEEDS[4], 2 ** 31, 1), (SEEDS[3], 5, 3)):
        z, u1, u2 = ex.normal_f64(seed, iteration, stream, np.arange(n))
        got = C(_ops.rng_fill(_ops.new_rng_state(seed, dev, iteration), stream, (n,), normal=True)).astype(np.float64)
        assert np.isfinite(got).all()
        u1_d, angle_d = torch.tensor(u1, device=dev), torch.tensor(ex.TWO_PI_F32 * u2, device=dev)
        assert u1_d.dtype == torch.float32 and angle_d.dtype == torch.float32
        yard = C(torch.sqrt(-2.0 * torch.log(u1_d)) * torch.cos(angle_d)).astype(np.float64)
        worst_lib = max(worst_lib, float(np.abs(got - z).max()))
        worst_torch = max(worst_torch, float(np.abs(yard - z).max()))
    gate = max(2.0 * worst_torch, floor)
    print(f"normal draws: worst |z - z64| library {worst_lib:.3e}, torch fp32 {worst_torch:.3e}, gate {gate:.3e}")
    _record_measurement("device_normal_draws", dict(library=worst_lib, torch_fp32=worst_torch, gate=gate))
    assert worst_lib <= gate, (worst_lib, worst_torch, gate)
    seed, iteration, stream, index, _ = PLANT_ONES
    got = C(_ops.rng_fill(_ops.new_rng_state(seed, dev, iteration), stream, (index + 1,), normal=True))
    assert np.isfinite(got).all() and float(got[index]) == 0.0
    seed, iteration, stream, index, _ = PLANT_ZEROS
    got = C(_ops.rng_fill(_ops.new_rng_state(seed, dev, iteration), stream, (index + 1,), normal=True))
    assert np.isfinite(got).all() and abs(float(got[index])) <= Z_MAX
    z = ex.normal_f64(seed, iteration, stream, index)[0]
    assert abs(float(got[index]) - float(z)) <= gate


def identity_cameras(n_views, dev):
    """Identity rotations, focal length 50, principal point (3, 2); the camera position's first coordinate names the view."""
    cams = torch.zeros(n_views, 16, device=dev)
    cams[:, 0] = cams[:, 4] = cams[:, 8] = 1.0
    cams[:, 12], cams[:, 13], cams[:, 14] = 50.0, 3.0, 2.0
    cams[:, 9] = torch.arange(n_views, device=dev, dtype=torch.float32)
    return cams


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", IMAGE_SIZES, ids=[f"{h}x{w}" for h, w in IMAGE_SIZES])
def test_pixel_draw_bit_equal_to_the_restated_feistel_walk(dev, h, w):
    """dn_select_rays_draw: the full H W draw equals feistel_permute(arange(H W), H W, seed, iteration) and a 7-ray draw (H W rays where
    the image has fewer) its head, for a seed with and one without a high word and first iterations 0, 3 and 2^32 - 1; the state after a
    draw is (iteration, iteration).  37 x 29 also through the NDC entry: the same pixels."""
    from nerf import _ops
    from oracle import exact_rng as ex
    cams = identity_cameras(2, dev)
    view = torch.zeros((), dtype=torch.int32, device=dev)
    n = h * w
    head = min(7, n)
    for seed in DRAW_SEEDS:
        for iteration in DRAW_ITERATIONS:
            want = ex.feistel_permute(np.arange(n), n, seed, iteration)
            what = f"{h}x{w} seed={seed:#x} iteration={iteration}"
            st = _ops.new_rng_state(seed, dev, iteration)
            pix = _ops.select_rays_draw(h, w, cams, view, 2.0, 6.0, st, n, want_pixels=True)[2]
            assert pix.dtype == torch.int64
            np.testing.assert_array_equal(C(pix), want, err_msg=what)
            assert words(st)[2:] == [iteration, iteration]
            short = _ops.select_rays_draw(h, w, cams, view, 2.0, 6.0, _ops.new_rng_state(seed, dev, iteration), head, want_pixels=True)[2]
            np.testing.assert_array_equal(C(short), want[:head], err_msg=what + " prefix")
            if (h, w) == (37, 29):
                ndc = _ops.select_rays_draw(h, w, cams, view, 2.0, 6.0, _ops.new_rng_state(seed, dev, iteration), n, want_pixels=True,
                                            ndc_focal=50.0)[2]
                np.testing.assert_array_equal(C(ndc), want, err_msg=what + " NDC")


@pytest.mark.gpu
@pytest.mark.parametrize("n_views,first", [(1, 0), (2, 2 ** 31), (5, 2 ** 32 - 8), (7, 0)])
def test_drawn_view_equals_the_restated_modulo(dev, n_views, first):
    """view=None: over 16 iterations advanced by dn_mse2_loss (one run crossing the wrap of the 32-bit counter) every ray of a draw
    comes from view w0 % V of stream 5, index 0, and its pixels are that iteration's permutation."""
    from nerf import _ops
    from oracle import exact_rng as ex
    h, w, n, seed = 5, 13, 16, 9
    cams = identity_cameras(n_views, dev)
    dummy = torch.zeros(n, 3, device=dev)
    st = _ops.new_rng_state(seed, dev, first)
    for k in range(16):
        iteration = (first + k) & U32
        rows, _, pix = _ops.select_rays_draw(h, w, cams, None, 2.0, 6.0, st, n, want_pixels=True)
        np.testing.assert_array_equal(C(rows[:, 0]), np.full(n, float(ex.drawn_view(seed, iteration, n_views)), F), err_msg=f"V={n_views} k={k}")
        np.testing.assert_array_equal(C(pix), ex.feistel_permute(np.arange(n), h * w, seed, iteration), err_msg=f"V={n_views} k={k}")
        _ops.mse2_loss(dummy, dummy, dummy, rng_state=st)
        assert words(st)[2:] == [iteration, (iteration + 1) & U32]


@pytest.mark.gpu
@pytest.mark.parametrize("n_views,h,w", PAIR_SHAPES)
def test_drawn_pairs_equal_the_restated_walk_over_all_views(dev, n_views, h, w):
    """dn_select_rays_draw_views: (view, pixel) of ray i == divmod(feistel_permute(i, V H W), H W), the full draw and a 7-pair head,
    and the row's camera is the view's; with one view it is the single-view draw of the same state."""
    from nerf import _ops
    from oracle import exact_rng as ex
    cams = identity_cameras(n_views, dev)
    n = n_views * h * w
    for seed, iteration in ((DRAW_SEEDS[0], 3), (DRAW_SEEDS[1], 2 ** 32 - 1)):
        want_v, want_p = np.divmod(ex.feistel_permute(np.arange(n), n, seed, iteration), h * w)
        for count in (n, 7):
            rows, _, pix, views = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, _ops.new_rng_state(seed, dev, iteration), count, want_pixels=True)
            what = f"V={n_views} {h}x{w} seed={seed:#x} iteration={iteration} count={count}"
            np.testing.assert_array_equal(C(views), want_v[:count], err_msg=what)
            np.testing.assert_array_equal(C(pix), want_p[:count], err_msg=what)
            np.testing.assert_array_equal(C(rows[:, 0]), want_v[:count].astype(F), err_msg=what)
        if n_views == 1:
            view = torch.zeros((), dtype=torch.int32, device=dev)
            one_rows, _, one_pix = _ops.select_rays_draw(h, w, cams, view, 2.0, 6.0, _ops.new_rng_state(seed, dev, iteration), 7, want_pixels=True)
            assert torch.equal(one_pix, pix) and torch.equal(one_rows, rows)


@pytest.mark.gpu
def test_iteration_counter_protocol_and_its_wrap_around(dev):
    """A draw publishes nxt as cur and leaves nxt; each loss head (dn_mse2_loss, dn_render_loss, dn_render_loss_exposure) writes
    nxt = cur + 1; from first iteration 2^32 - 1 the next nxt is 0 and the draw after it is the restatement's at iteration 0."""
    from nerf import _ops
    from oracle import exact_rng as ex
    h, w, n, seed = 5, 13, 16, 0x0123456789ABCDEF
    cams = identity_cameras(1, dev)
    view = torch.zeros((), dtype=torch.int32, device=dev)
    rgb = torch.rand(n, 3, device=dev)
    eps = torch.zeros(1, 1, device=dev)

    def draw(st, iteration):
        pix = _ops.select_rays_draw(h, w, cams, view, 2.0, 6.0, st, n, want_pixels=True)[2]
        np.testing.assert_array_equal(C(pix), ex.feistel_permute(np.arange(n), h * w, seed, iteration), err_msg=f"iteration {iteration}")

    heads = (lambda st: _ops.mse2_loss(rgb, rgb, rgb, rng_state=st),
             lambda st: _ops.render_loss(rgb, rgb, rgb, rng_state=st),
             lambda st: _ops.render_loss_exposure(rgb, rgb, rgb, eps, rng_state=st))
    st = _ops.new_rng_state(seed, dev, 41)
    assert words(st) == [0x89ABCDEF, 0x01234567, 41, 41]
    iteration = 41
    for head in heads:
        draw(st, iteration)
        assert words(st)[2:] == [iteration, iteration]
        head(st)
        assert words(st)[2:] == [iteration, iteration + 1]          # cur != nxt: the next draw has to read nxt
        iteration += 1
    draw(st, iteration)
    assert words(st) == [0x89ABCDEF, 0x01234567, 44, 44]
    for head in heads:
        st = _ops.new_rng_state(seed, dev, 2 ** 32 - 1)
        draw(st, 2 ** 32 - 1)
        head(st)
        assert words(st)[2:] == [2 ** 32 - 1, 0]
        draw(st, 0)
        assert words(st)[2:] == [0, 0]
        # the numbers of the wrapped iteration too
        np.testing.assert_array_equal(C(_ops.rng_fill(st, 2, (257,))), ex.uniform(seed, 0, 2, np.arange(257)))


# ---- the numbers the sampling and compositing kernels draw themselves, at ragged shapes ------------------------------------------------
MKW = dict(num_layers=2, hidden_size=128, skip_connect_every=2, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
NOISE_STD = 0.2
THRESHOLDS = [1.0, 5.0]
# (n_rays, nc, nf): nc and nc + nf on the edges of the 64-sample compositing chunk, n_rays S never a whole network tile
RAGGED_SHAPES = ((1, 10, 1), (5, 63, 1), (5, 64, 1), (3, 65, 64), (67, 129, 64), (7, 100, 93))


@pytest.fixture(scope="module")
def small_nets(dev):
    """The smallest fused-trainable pair (2 x 128 with view directions) with their core, backward and input-gradient streams in fp32."""
    import nerf
    from nerf import _hip, _ops, synthetic as syn
    nets = []
    for seed in (31, 32):
        m = nerf.models.FlexibleNeRFModel(**MKW)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_gain=20.0, sigma_bias=0.0, **MKW).items()})
        m = m.to(dev)
        pk = m.packed(parts=_hip.PACK_CORE)
        assert pk.precision == _hip.PREC_F32
        _ops.ensure_backward_stream(m, pk, _hip.PREC_F32)
        _ops.ensure_input_grad_stream(m, pk)
        nets.append((m, pk))
    return nets


def ragged_rows(n, dev):
    """(n, 11) ray rows [origin, direction (not unit length), near 2, far 6, unit view direction] through the box the field lives in."""
    g = torch.Generator().manual_seed(1000 + n)
    ro = torch.cat(((torch.rand(n, 2, generator=g) - 0.5) * 0.6, torch.full((n, 1), -4.0)), -1)
    rd = torch.cat(((torch.rand(n, 2, generator=g) - 0.5) * 0.5, torch.ones(n, 1)), -1) * (0.9 + 0.2 * torch.rand(n, 1, generator=g))
    vd = torch.nn.functional.normalize(rd, dim=-1)
    return torch.cat((ro, rd, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), vd), -1).to(dev)


def read_draws(state, n, nc, nf):
    """The four draws of `state`'s current iteration as the tensors a caller injects (dn_rng_fill)."""
    from nerf import _ops
    return dict(t_rand=_ops.rng_fill(state, 0, (n, nc)), noise_c=_ops.rng_fill(state, 1, (n, nc), normal=True),
                u=_ops.rng_fill(state, 2, (n, nf)), noise_f=_ops.rng_fill(state, 3, (n, nc + nf), normal=True))


def upstream(n, dev):
    """((g_rgb, g_depth, g_acc) coarse, the same fine): random upstream gradients of the six maps."""
    g = torch.Generator().manual_seed(2000 + n)
    return tuple(tuple(torch.randn(shape, generator=g).to(dev) for shape in ((n, 3), (n,), (n,))) for _ in range(2))


def run_iteration(small_nets, rows, nc, nf, draws, rng_state, perturb):
    """One training forward and both backwards: dict of numpy arrays - the seven maps of dn_render_rays_train and of
    dn_render_rays_train_geom, z_samples, dW / db of both networks from dn_render_rays_backward and from dn_render_rays_backward_geom,
    d_rays."""
    from nerf import _hip, _ops
    (mc, pc), (mf, pf) = small_nets
    dev = rows.device
    n = rows.shape[0]
    g_c, g_f = upstream(n, dev)
    shapes = [[tuple(x.weight.shape) for x in m.linear_modules()] for m in (mc, mf)]
    out = {}
    maps, saved = _ops.render_rays_train(pc, pf, rows, nc, nf, False, NOISE_STD, True, THRESHOLDS, draws, prec=_hip.PREC_F32,
                                         rng_state=rng_state, perturb=perturb)
    assert len(maps) == 7 and all(m is not None for m in maps)
    for k, m in enumerate(maps):
        out[f"map{k}"] = C(m)
    views = [_ops.zeroed_grad_views(s, dev) for s in shapes]
    keep = _ops.render_rays_backward(pc, pf, saved, g_c, g_f, views[0], views[1], nets=3)
    for tag, view in zip("cf", views):
        for k, (dw, db) in enumerate(view):
            out[f"dW_{tag}{k}"], out[f"db_{tag}{k}"] = C(dw), C(db)
    maps, saved = _ops.render_rays_train_geom(pc, pf, rows, nc, nf, False, NOISE_STD, True, THRESHOLDS, draws, prec=_hip.PREC_F32,
                                              rng_state=rng_state, perturb=perturb)
    for k, m in enumerate(maps):
        out[f"geom_map{k}"] = C(m)
    out["z_samples"] = C(saved["z_samples"])
    views = [_ops.zeroed_grad_views(s, dev) for s in shapes]
    d_rays, keep_geom = _ops.render_rays_backward_geom(pc, pf, saved, g_c, g_f, views[0], views[1])
    out["d_rays"] = C(d_rays)
    for tag, view in zip("cf", views):
        for k, (dw, db) in enumerate(view):
            out[f"geom_dW_{tag}{k}"], out[f"geom_db_{tag}{k}"] = C(dw), C(db)
    torch.cuda.synchronize()
    del keep, keep_geom
    return out


def assert_same_iteration(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=f"{name} {what}")
    for k in range(7):
        np.testing.assert_array_equal(a[f"geom_map{k}"], a[f"map{k}"], err_msg=f"geom map {k} {what}")
    assert all(np.isfinite(v).all() for name, v in a.items() if name.startswith(("dW", "db", "d_rays", "z_samples")))
    # the inputs have teeth: both networks receive a gradient
    assert max(float(np.abs(a[k]).max()) for k in a if k.startswith("dW_c")) > 0.0, what
    assert max(float(np.abs(a[k]).max()) for k in a if k.startswith("dW_f")) > 0.0, what


@pytest.fixture
def deterministic_weight_gradients():
    from nerf import _ops
    _ops.set_deterministic_weight_gradients(True)
    try:
        yield
    finally:
        _ops.set_deterministic_weight_gradients(True)      # (the default)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nc,nf", RAGGED_SHAPES)
def test_in_kernel_draws_equal_rng_fill_at_ragged_shapes(dev, small_nets, deterministic_weight_gradients, n, nc, nf):
    """dn_render_rays_train(_geom) drawing its own jitter, coarse noise, u and fine noise (rng_state, perturb) against the same call
    with the four draws read back by dn_rng_fill and injected (no rng_state): the seven maps, z_samples, every dW / db of both networks
    (the compositing backward regenerates the noise) and d_rays (the coarse-depth backward regenerates the jitter) bit for bit."""
    from nerf import _ops
    rows = ragged_rows(n, dev)
    seed, iteration = 77 + n, 2 ** 32 - 3 + (nc % 3)
    st = _ops.new_rng_state(seed, dev, iteration)
    drawn = run_iteration(small_nets, rows, nc, nf, None, st, True)
    assert words(st) == words(_ops.new_rng_state(seed, dev, iteration))          # a render reads the state, no more
    injected = run_iteration(small_nets, rows, nc, nf, read_draws(_ops.new_rng_state(seed, dev, iteration), n, nc, nf), None, True)
    assert_same_iteration(drawn, injected, f"n={n} nc={nc} nf={nf}")


@pytest.mark.gpu
def test_partial_injection_and_unperturbed_draws(dev, small_nets, deterministic_weight_gradients):
    """(5, 65, 64).  An injected jitter beside an rng_state: every other draw falls back to the state on its own - equal to the fully
    injected call.  perturb=False with an rng_state: jitter and u stay deterministic, the two noises are still drawn - equal to the
    call with only the two noises injected.  And each of the four draws moves the result: a shifted copy changes the fine colour."""
    from nerf import _ops
    n, nc, nf = 5, 65, 64
    rows = ragged_rows(n, dev)
    seed, iteration = 5, 9
    st = _ops.new_rng_state(seed, dev, iteration)
    draws = read_draws(_ops.new_rng_state(seed, dev, iteration), n, nc, nf)
    full = run_iteration(small_nets, rows, nc, nf, draws, None, True)
    partial = run_iteration(small_nets, rows, nc, nf, dict(t_rand=draws["t_rand"]), st, True)
    assert_same_iteration(partial, full, "jitter injected, the rest drawn")
    plain = run_iteration(small_nets, rows, nc, nf, None, st, False)
    noises = run_iteration(small_nets, rows, nc, nf, dict(t_rand=None, noise_c=draws["noise_c"], u=None, noise_f=draws["noise_f"]), None, False)
    assert_same_iteration(plain, noises, "perturb=False")
    assert not np.array_equal(plain["map3"], full["map3"]) and not np.array_equal(plain["z_samples"], full["z_samples"])
    for name in ("t_rand", "noise_c", "u", "noise_f"):
        moved = dict(draws)
        moved[name] = torch.roll(draws[name].reshape(-1), 1).reshape(draws[name].shape)
        other = run_iteration(small_nets, rows, nc, nf, moved, None, True)
        assert not np.array_equal(other["map3"], full["map3"]) or not np.array_equal(other["dW_f0"], full["dW_f0"]), name
