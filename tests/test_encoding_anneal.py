"""nerf.EncodingAnneal - the coarse-to-fine positional encoding of BARF (eq. 14) on the fused steps - and the three entry points of
include/dexnerf_hip_anneal.h.

Yardsticks.  The amplitude table: the float64 formula written here, at 1e-6 absolute (one fp32 rounding of a value in [0, 1] is at most
6e-8; the fp64 cosine's own error is below 1e-15), the clamped ends and the raw-input columns exactly.  Everything else BIT FOR BIT
(torch.equal): an amplitude on the encoding is a column scale of the weights that multiply it, so a network with the schedule attached
is compared with a CLONE WHOSE WEIGHTS WERE PRE-MULTIPLIED IN TORCH (one fp32 multiply per element on the device table) running the
same kernels with nothing attached - forward in every precision, the camera half of the joint step, the weight gradients (equal on the
hidden columns, equal to G_eff * a on the band columns), replayed against eager steps, a run against its resumption.

Scene: tests/test_render_loss.py's (3 views of 24 x 24, 16 + 16 samples) at 64 - 256 rays.  Networks: D8 / W256 / skip 4 / L_xyz = 10 and
D6 / W128 / skip_connect_every = 2 / L_xyz = 6 (two wide layers; the run-time-shape kernels) - the shipped 4 x 128 net has no wide layer."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import REPO
from test_render_loss import TRAIN_H, TRAIN_POSES, TRAIN_W, scene  # noqa: F401  (the module-scoped scene fixture)

ANNEAL = ("dn_encoding_anneal_amplitudes", "dn_encoding_anneal_scale_weights", "dn_encoding_anneal_scale_grads",
          "dn_encoding_anneal_scale_weights_pair", "dn_encoding_anneal_scale_grads_pair")
NETS = {
    "d8w256": dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
    "d6w128": dict(num_layers=6, hidden_size=128, skip_connect_every=2, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True),
}
RAYS = {"d8w256": 256, "d6w128": 200}      # (200: no multiple of 64 or of the tile)
SHAPES = sorted(NETS)


def formula(it, start, end, num_bands):
    """BARF eq. 14 in float64: the amplitudes of the bands of one encoding."""
    if end > start:
        p = min(max((it - start) / (end - start), 0.0), 1.0)
    else:
        p = 1.0 if it >= start else 0.0
    return [(1.0 - math.cos(math.pi * min(max(p * num_bands - k, 0.0), 1.0))) / 2.0 for k in range(num_bands)]


def clamped(it, start, end, num_bands):
    """Per band: 0.0 / 1.0 where the schedule's clamp decides the value, None inside the cosine."""
    p = min(max((it - start) / (end - start), 0.0), 1.0) if end > start else (1.0 if it >= start else 0.0)
    return [0.0 if p * num_bands - k <= 0.0 else (1.0 if p * num_bands - k >= 1.0 else None) for k in range(num_bands)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_anneal_header_declares_exactly_its_table_and_the_older_headers_stay():
    from nerf import _hip
    names = lambda name: set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", open(os.path.join(REPO, "include", name)).read()))  # noqa: E731
    assert names("dexnerf_hip_anneal.h") == set(_hip.ANNEAL_EXPORTS) == set(ANNEAL)
    v2, ext = names("dexnerf_hip.h"), names("dexnerf_hip_ext.h")
    assert len(v2) == 76 and v2 == set(_hip.EXPORTS) and len(ext) == 3 and ext == set(_hip.EXT_EXPORTS)
    assert not (v2 | ext) & set(ANNEAL)
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "dexnerf_hip_anneal.h" in entry       # build() checks the new header's symbols too


@pytest.mark.parametrize("shape", SHAPES)
def test_masked_encoding_is_a_column_scale_of_the_weights_in_float64(shape):
    """The identity the feature rests on, on the nn.Linear composition: net(a * enc) == net_scaled(enc), and the weight gradients of
    the two differ by the column scale."""
    import nerf
    from nerf.anneal import EncodingAnneal
    torch.manual_seed(3)
    kw = NETS[shape]
    net = nerf.models.FlexibleNeRFModel(**kw).double()
    l_xyz, l_dir = kw["num_encoding_fn_xyz"], kw["num_encoding_fn_dir"]
    a_xyz = torch.tensor([1.0] * 3 + [a for a in formula(37, 0, 100, l_xyz) for _ in range(6)], dtype=torch.float64)
    a_dir = torch.tensor([1.0] * 3 + [a for a in formula(37, 0, 100, l_dir) for _ in range(6)], dtype=torch.float64)
    assert any(0.0 < a < 1.0 for a in a_xyz.tolist()) and 0.0 in a_xyz.tolist() and 1.0 in a_xyz.tolist()[3:]
    scaled = nerf.models.FlexibleNeRFModel(**kw).double()
    scaled.load_state_dict(net.state_dict())
    affected = EncodingAnneal.affected(net)
    assert affected == [0] + [1 + i for i in net.skip_layers] + [kw["num_layers"]] and len(net.skip_layers) == (1 if shape == "d8w256" else 2)
    col = {}
    for i in affected:
        w = scaled.linear_modules()[i].weight
        a = a_dir if i == kw["num_layers"] else a_xyz
        col[i] = torch.cat((torch.ones(w.shape[1] - a.numel(), dtype=torch.float64), a))
        with torch.no_grad():
            w.mul_(col[i])
    x = torch.randn(50, net.dim_xyz + net.dim_dir, dtype=torch.float64)
    g = torch.randn(50, 4, dtype=torch.float64)
    out_masked = net._forward_modules(x * torch.cat((a_xyz, a_dir)))
    out_scaled = scaled._forward_modules(x)
    assert float((out_masked - out_scaled).detach().abs().max()) <= 1e-12 * float(out_scaled.detach().abs().max())
    (out_masked * g).sum().backward()
    (out_scaled * g).sum().backward()
    for i, (m, s) in enumerate(zip(net.linear_modules(), scaled.linear_modules())):
        want = s.weight.grad * col[i] if i in col else s.weight.grad
        assert float((m.weight.grad - want).abs().max()) <= 1e-12 * float(want.abs().max()), i
        assert float((m.bias.grad - s.bias.grad).abs().max()) <= 1e-12 * float(s.bias.grad.abs().max()), i


def test_entry_points_judge_their_arguments_before_gpu_work():
    from nerf import _hip
    if not _hip.available():
        pytest.skip("libdexnerf_hip.so is not built")
    lib = _hip.lib()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in ANNEAL) and lib.dn_abi_version() == 2
    fake = ctypes.c_void_p(1024)
    defaults = dict(rng=None, it=0, start=0.0, end=10.0, lx=10, ld=4, ad=1, amp=fake, st=None)
    amp = lambda **kw: lib.dn_encoding_anneal_amplitudes(*{**defaults, **kw}.values())  # noqa: E731
    for kw in (dict(amp=None), dict(lx=0), dict(lx=33), dict(ld=-1), dict(ld=33), dict(start=-1.0), dict(start=11.0), dict(end=float("inf")),
               dict(start=float("nan")), dict(it=-1)):
        assert amp(**kw) == -1000, kw
        assert b"dn_encoding_anneal_amplitudes" in lib.dn_last_error(), kw
    desc = _hip.MlpDesc(8, 256, 4, 10, 4, 1, 1, 1, 1, 1)
    ptrs = (ctypes.c_void_p * 12)(*[1024] * 12)
    holes = (ctypes.c_void_p * 12)(*[1024 if i != 5 else 0 for i in range(12)])      # layers_xyz[4], the wide layer
    by = ctypes.byref
    assert lib.dn_encoding_anneal_scale_weights(by(desc), None, fake, ptrs, None) == -1000
    assert lib.dn_encoding_anneal_scale_weights(by(desc), ptrs, None, ptrs, None) == -1000
    assert lib.dn_encoding_anneal_scale_weights(by(desc), ptrs, fake, ptrs, None) == -1000 and b"itself" in lib.dn_last_error()
    assert lib.dn_encoding_anneal_scale_weights(by(desc), ptrs, fake, holes, None) == -1000 and b"NULL" in lib.dn_last_error()
    assert lib.dn_encoding_anneal_scale_grads(by(desc), None, ptrs, None) == -1000
    assert lib.dn_encoding_anneal_scale_grads(by(desc), fake, None, None) == -1000
    assert lib.dn_encoding_anneal_scale_grads(by(desc), fake, holes, None) == -1000
    bad = _hip.MlpDesc(8, 192, 4, 10, 4, 1, 1, 1, 1, 1)
    assert lib.dn_encoding_anneal_scale_weights(by(bad), ptrs, fake, holes, None) != 0
    assert lib.dn_encoding_anneal_scale_grads(by(bad), fake, ptrs, None) != 0
    # the pair forms: one table for both networks
    l6 = _hip.MlpDesc(8, 256, 4, 6, 4, 1, 1, 1, 1, 1)
    assert lib.dn_encoding_anneal_scale_weights_pair(by(desc), ptrs, holes, by(l6), ptrs, holes, fake, None) == -1000 and b"agree" in lib.dn_last_error()
    assert lib.dn_encoding_anneal_scale_grads_pair(by(desc), ptrs, by(l6), ptrs, fake, None) == -1000 and b"agree" in lib.dn_last_error()
    assert lib.dn_encoding_anneal_scale_weights_pair(by(desc), ptrs, holes, by(desc), ptrs, ptrs, fake, None) == -1000
    assert lib.dn_encoding_anneal_scale_weights_pair(by(desc), ptrs, None, by(desc), ptrs, holes, fake, None) == -1000
    assert lib.dn_encoding_anneal_scale_grads_pair(by(desc), ptrs, by(desc), holes, fake, None) == -1000
    assert lib.dn_encoding_anneal_scale_grads_pair(by(desc), ptrs, by(bad), ptrs, fake, None) != 0


def test_schedule_and_driver_flags_are_checked_on_the_host():
    import nerf
    import train_dexnerf
    for start, end in ((-1, 5), (6, 5), (0, float("inf"))):
        with pytest.raises(ValueError, match="EncodingAnneal"):
            nerf.EncodingAnneal(start, end)
    a, b = nerf.models.FlexibleNeRFModel(**NETS["d8w256"]), nerf.models.FlexibleNeRFModel(**NETS["d6w128"])
    with pytest.raises(ValueError, match="agree on L_xyz"):
        nerf.EncodingAnneal(0, 10).attach(a, b)
    assert a._encoding_anneal is None and b._encoding_anneal is None and len(a.param_key()) == len(a.linear_modules()) + 1
    state = nerf.EncodingAnneal(5, 50, anneal_dir=False).state_dict(iteration=17)
    assert state == dict(start=5.0, end=50.0, anneal_dir=False, iteration=17)
    again = nerf.EncodingAnneal.from_state_dict(state)
    assert (again.start, again.end, again.anneal_dir, again.iteration) == (5.0, 50.0, False, 17)
    args = train_dexnerf.parse_args(["--anneal-encoding", "100", "2000", "--anneal-xyz-only", "--refine-poses"])
    assert args.anneal_encoding == [100, 2000] and args.anneal_xyz_only
    assert train_dexnerf.parse_args([]).anneal_encoding is None
    for argv in (["--anneal-encoding", "10", "5"], ["--anneal-encoding", "-1", "5"], ["--anneal-xyz-only"],
                 ["--anneal-encoding", "0", "5", "--autograd-step"]):
        with pytest.raises(SystemExit):
            train_dexnerf.parse_args(argv)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_modes():
    import nerf
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def table(dev, it, start, end, l_xyz, l_dir, anneal_dir=True, rng_state=None):
    from nerf import _hip
    amp = torch.full((l_xyz + l_dir,), -7.0, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().dn_encoding_anneal_amplitudes(_hip.ptr(rng_state), int(it), float(start), float(end), l_xyz, l_dir, int(anneal_dir),
                                                        _hip.ptr(amp), _hip.stream()), "dn_encoding_anneal_amplitudes")
    return amp


def check_table(amp, it, start, end, l_xyz, l_dir, anneal_dir=True, what=""):
    """The device table against the float64 formula: 1e-6 absolute, the clamped ends exact (+0.0 with its sign, 1.0)."""
    got = amp.cpu()
    want = formula(it, start, end, l_xyz) + (formula(it, start, end, l_dir) if anneal_dir else [1.0] * l_dir)
    ends = clamped(it, start, end, l_xyz) + (clamped(it, start, end, l_dir) if anneal_dir else [1.0] * l_dir)
    err = max(abs(float(g) - w) for g, w in zip(got, want))
    print(f"amplitude table {what} it={it} [{start}, {end}] L={l_xyz}+{l_dir} dir={anneal_dir}: max |err| {err:.2e}")
    assert err <= 1e-6
    for g, e in zip(got, ends):
        if e is not None:
            assert float(g) == e and not bool(torch.signbit(g)), (float(g), e)


@pytest.mark.gpu
@pytest.mark.parametrize("anneal_dir", [True, False])
@pytest.mark.parametrize("l_xyz", [10, 6])
def test_amplitude_table_against_the_float64_formula(dev, l_xyz, anneal_dir):
    from nerf import _ops
    start, end = 100, 1100
    for it in (50, 233, 617, 987, 1100, 5000):      # before the start, three interior points, the end, past it
        amp = table(dev, it, start, end, l_xyz, 4, anneal_dir)
        check_table(amp, it, start, end, l_xyz, 4, anneal_dir)
        # an RNG record whose `nxt` word is `it` (and whose `cur` is not): the same bits
        state = _ops.new_rng_state(9, dev, it)
        state[2] = 7
        assert torch.equal(table(dev, 0, start, end, l_xyz, 4, anneal_dir, rng_state=state), amp), it
    inner = table(dev, 617, start, end, l_xyz, 4, anneal_dir)[:l_xyz]
    assert bool(((inner > 0) & (inner < 1)).any())
    # end == start: a step at start
    check_table(table(dev, 99, 100, 100, l_xyz, 4, anneal_dir), 99, 100, 100, l_xyz, 4, anneal_dir, "step")
    check_table(table(dev, 100, 100, 100, l_xyz, 4, anneal_dir), 100, 100, 100, l_xyz, 4, anneal_dir, "step")


def make_pair(shape, dev, init=5, sigma_bias=None):
    """A coarse and a fine network at torch's default init; sigma_bias: fc_alpha's bias set to it (see the p = 0 test)."""
    import nerf
    torch.manual_seed(init)
    nets = [nerf.models.FlexibleNeRFModel(**NETS[shape]).to(dev) for _ in range(2)]
    if sigma_bias is not None:
        with torch.no_grad():
            for net in nets:
                net.fc_alpha.bias.fill_(sigma_bias)
    return nets


def column_scales(model, amp):
    """{index in linear_modules(): full-width column scale} formed by torch from the device table: hidden and raw-input columns 1."""
    l_xyz = model.num_encoding_fn_xyz
    out = {}
    for i in [0] + [1 + s for s in model.skip_layers] + [model.num_layers]:
        bands = amp[l_xyz:] if i == model.num_layers else amp[:l_xyz]
        width = model.linear_modules()[i].weight.shape[1]
        out[i] = torch.cat((torch.ones(width - 6 * bands.numel(), dtype=torch.float32, device=amp.device), bands.repeat_interleave(6)))
    return out


def premultiplied(nets, amp, dev):
    """Clones of `nets` with nothing attached whose weights carry the column scale, multiplied in torch (fp32, on the device)."""
    import nerf
    out = []
    for net in nets:
        clone = nerf.models.FlexibleNeRFModel(**{k: getattr(net, k) for k in NETS["d8w256"]}).to(dev)
        clone.load_state_dict(net.state_dict())
        with torch.no_grad():
            for i, col in column_scales(net, amp).items():
                w = clone.linear_modules()[i].weight
                w.copy_(w * col)
        out.append(clone)
    return out


def encoders(shape):
    import nerf
    return nerf.get_embedding_function(NETS[shape]["num_encoding_fn_xyz"]), nerf.get_embedding_function(4)


def some_rays(scene, dev, n):
    import nerf
    from nerf import synthetic as syn
    kmat = torch.from_numpy(syn.intrinsic(TRAIN_H, TRAIN_W)).to(dev)
    pose = torch.from_numpy(syn.scene_pose(TRAIN_POSES[1])).to(dev)
    ro, rd = nerf.get_ray_bundle(TRAIN_H, TRAIN_W, float(kmat[0, 0]), pose, kmat)
    pick = torch.arange(n, device=dev) * 5 % (TRAIN_H * TRAIN_W)
    return float(kmat[0, 0]), ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous()


def renders(scene, dev, shape, nets, n=100):
    """run_network, a coarse + fine run_one_iter_of_nerf and render_dex_depth under no_grad on the same rays and draws."""
    import nerf
    ex, ed = encoders(shape)
    focal, ro, rd = some_rays(scene, dev, n)
    pts = ro[:, None, :] + rd[:, None, :] * torch.linspace(2.0, 6.0, 13, device=dev)[None, :, None]
    rows = torch.cat((ro, rd, torch.zeros(n, 2, device=dev), torch.nn.functional.normalize(rd, dim=-1)), dim=-1)
    with torch.no_grad():
        out = [nerf.run_network(nets[1], pts, rows, 4096, ex, ed)]
        torch.manual_seed(77)
        out += [t for t in nerf.run_one_iter_of_nerf(TRAIN_H, TRAIN_W, focal, nets[0], nets[1], ro, rd, scene.cfg, mode="train",
                                                     encode_position_fn=ex, encode_direction_fn=ed)[:6]]
        torch.manual_seed(77)
        out += [t for t in nerf.render_dex_depth(TRAIN_H, TRAIN_W, focal, nets[0], nets[1], ro, rd, scene.cfg, mode="train",
                                                 encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=[5.0, 20.0])]
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_scaled_copies_equal_torch_products(dev, shape):
    import nerf
    nets = make_pair(shape, dev)
    anneal = nerf.EncodingAnneal(0, 100).attach(*nets)
    anneal.set_iteration(37)
    check_table(anneal.amplitudes(), 37, 0, 100, NETS[shape]["num_encoding_fn_xyz"], 4, what="attached")
    for net in nets:
        weights = [m.weight for m in net.linear_modules()]
        got = anneal.scaled_weights(net, weights)
        cols = column_scales(net, anneal.amplitudes())
        assert sorted(cols) == anneal.affected(net)
        for i, (g, w) in enumerate(zip(got, weights)):
            if i in cols:
                assert g.data_ptr() != w.data_ptr() and torch.equal(g, w.detach() * cols[i]) and not torch.equal(g, w.detach()), i
            else:
                assert g.data_ptr() == w.data_ptr(), i
        assert net.pack_weights(scaled=False)[0] is net.layer1.weight
    # both networks in one launch: the same copies, and the same gradient scale
    singles = [[t.clone() for t in anneal.scaled_weights(net, [m.weight for m in net.linear_modules()])] for net in nets]
    for net in nets:
        for buf in anneal._copies[id(net)].values():
            buf.fill_(float("nan"))
    assert all(same(a, b) for a, b in zip(anneal.scaled_weights_pair(*nets), singles))
    gen = torch.Generator(device=dev).manual_seed(4)
    views = [[(torch.randn(m.weight.shape, generator=gen, device=dev), None) for m in net.linear_modules()] for net in nets]
    one_by_one = [[(w.clone(), None) for w, _ in v] for v in views]
    for net, v in zip(nets, one_by_one):
        anneal.scale_grads(net, v)
    anneal.scale_grads_pair(nets[0], views[0], nets[1], views[1])
    for v, w in zip(views, one_by_one):
        assert same([g for g, _ in v], [g for g, _ in w])
    gen = torch.Generator(device=dev).manual_seed(4)      # the same draws again: every element against raw * a in torch
    for net, v in zip(nets, views):
        cols = column_scales(net, anneal.amplitudes())
        for i, m in enumerate(net.linear_modules()):
            raw = torch.randn(m.weight.shape, generator=gen, device=dev)
            assert torch.equal(v[i][0], raw * cols[i] if i in cols else raw), i


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16-policy"])
@pytest.mark.parametrize("shape", SHAPES)
def test_no_grad_renders_equal_the_premultiplied_clone_bit_for_bit(dev, scene, shape, mode):
    """... also after an optimizer step: the copies are scaled from the weights of the moment of the pack, not from older ones."""
    import nerf
    nerf.set_precision("fp32" if mode == "fp32" else "bf16")
    nerf.set_render_policy("fp16" if mode == "fp16-policy" else "bf16")
    nets = make_pair(shape, dev)
    anneal = nerf.EncodingAnneal(0, 100).attach(*nets)
    anneal.set_iteration(37)
    plain = renders(scene, dev, shape, premultiplied(nets, torch.ones_like(anneal.amplitudes()), dev))
    got = renders(scene, dev, shape, nets)
    assert same(got, renders(scene, dev, shape, premultiplied(nets, anneal.amplitudes(), dev)))
    assert not torch.equal(got[0], plain[0]) and not torch.equal(got[4], plain[4])       # the schedule is in the render
    # the stale-copy case: an optimizer step, then the same comparison against a clone of the UPDATED weights
    opt = torch.optim.SGD([p for net in nets for p in net.parameters()], lr=0.05)
    gen = torch.Generator(device=dev).manual_seed(1)
    for net in nets:
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen, device=dev)
    opt.step()
    after = renders(scene, dev, shape, nets)
    assert same(after, renders(scene, dev, shape, premultiplied(nets, anneal.amplitudes(), dev))) and not torch.equal(after[0], got[0])
    # another iteration of the schedule reaches the next render, and detach() ends it
    anneal.set_iteration(80)
    assert same(renders(scene, dev, shape, nets), renders(scene, dev, shape, premultiplied(nets, anneal.amplitudes(), dev)))
    anneal.detach()
    assert same(renders(scene, dev, shape, nets), renders(scene, dev, shape, premultiplied(nets, torch.ones(14 if shape == "d8w256" else 10, device=dev), dev)))


def train_step(scene, dev, shape, nets, seed=31, **kw):
    import nerf
    from nerf import parallel
    ex, ed = encoders(shape)
    bucket = parallel.FlatGradBucket(nets)
    step = nerf.FusedTrainStep(nets[0], nets[1], scene.sel, scene.cfg, bucket, ex, ed, RAYS[shape], seed=seed, draw_view="rays", **kw)
    return step, bucket


def weight_grads(nets):
    return [[(m.weight.grad.clone(), m.bias.grad.clone()) for m in net.linear_modules()] for net in nets]


def table_at(dev, shape, it, start, end):
    return table(dev, it, start, end, NETS[shape]["num_encoding_fn_xyz"], 4)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradients_are_the_clones_times_the_column_scale(dev, scene, shape, precision):
    import nerf
    nerf.set_precision(precision)
    nets = make_pair(shape, dev)
    amp = table_at(dev, shape, 37, 0, 100)
    clones = premultiplied(nets, amp, dev)
    step, _ = train_step(scene, dev, shape, nets, first_iteration=37, encoding_anneal=nerf.EncodingAnneal(0, 100))
    ref, _ = train_step(scene, dev, shape, clones, first_iteration=37)
    loss, loss_ref = step.forward_backward().clone(), ref.forward_backward().clone()
    assert torch.equal(step.anneal.amplitudes(), amp) and step.rng_state.tolist()[2:] == [37, 38]
    assert torch.equal(loss, loss_ref) and bool(torch.isfinite(loss).all())
    for net, got, want in zip(nets, weight_grads(nets), weight_grads(clones)):
        cols = column_scales(net, amp)
        for i, ((gw, gb), (ww, wb)) in enumerate(zip(got, want)):
            assert torch.equal(gb, wb) and float(ww.abs().max()) > 0, i
            if i not in cols:
                assert torch.equal(gw, ww), i
                continue
            band = cols[i].numel() - 6 * (4 if i == net.num_layers else net.num_encoding_fn_xyz)
            assert torch.equal(gw[:, :band], ww[:, :band]), i                          # hidden columns and the raw x, y, z
            assert torch.equal(gw[:, band:], ww[:, band:] * cols[i][band:]), i         # G_eff * a
            assert not torch.equal(gw[:, band:], ww[:, band:]), i


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_data_parallel_halves_scale_each_network_before_its_exchange(dev, scene, shape):
    """The halves a data-parallel step runs around the fine network's all-reduce (forward_and_fine_backward, coarse_backward): when the
    first returns - the point where the fine segment is handed to the collective - the fine gradients already carry the column scale
    and the coarse ones are untouched; the second does the same for the coarse network.  Against the halves on the clones."""
    import nerf
    nets = make_pair(shape, dev)
    amp = table_at(dev, shape, 37, 0, 100)
    clones = premultiplied(nets, amp, dev)
    step, bucket = train_step(scene, dev, shape, nets, first_iteration=37, encoding_anneal=nerf.EncodingAnneal(0, 100))
    ref, ref_bucket = train_step(scene, dev, shape, clones, first_iteration=37)

    def scaled(net, grads):
        cols = column_scales(net, amp)
        return [(gw * cols[i] if i in cols else gw, gb) for i, (gw, gb) in enumerate(grads)]

    def equal(a, b):
        return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    for s, b in ((step, bucket), (ref, ref_bucket)):
        b.zero()
        s.forward_and_fine_backward(_zero=False)
    got, want = weight_grads(nets), weight_grads(clones)
    assert equal(got[1], scaled(nets[1], want[1])) and not equal(got[1], want[1]) and float(want[1][0][0].abs().max()) > 0
    assert all(float(gw.abs().max()) == 0 and float(gb.abs().max()) == 0 for gw, gb in got[0])
    step.coarse_backward(); ref.coarse_backward()
    got, want = weight_grads(nets), weight_grads(clones)
    assert equal(got[1], scaled(nets[1], want[1])) and equal(got[0], scaled(nets[0], want[0])) and not equal(got[0], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_at_p_zero_the_frequency_columns_get_no_gradient_and_do_not_move(dev, scene, shape):
    """fc_alpha's bias at 0.3: with every band off a freshly initialised network sees x, y, z alone, and the D6 / W128 fine network of
    this seed then has sigma < 0 at every sample of the scene - no gradient at all, and nothing for the test to see."""
    import nerf
    nets = make_pair(shape, dev, sigma_bias=0.3)
    amp = table_at(dev, shape, 3, 50, 100)
    assert bool((amp == 0).all())
    clones = premultiplied(nets, amp, dev)
    step, bucket = train_step(scene, dev, shape, nets, first_iteration=3, encoding_anneal=nerf.EncodingAnneal(50, 100))
    ref, _ = train_step(scene, dev, shape, clones, first_iteration=3)
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    before = [[m.weight.detach().clone() for m in net.linear_modules()] for net in nets]
    assert torch.equal(step.forward_backward(), ref.forward_backward())
    grads = weight_grads(nets)
    opt.step()
    torch.cuda.synchronize()
    for net, g_net, w0 in zip(nets, grads, before):
        for i in nerf.EncodingAnneal.affected(net):
            band = 6 * (4 if i == net.num_layers else net.num_encoding_fn_xyz)
            g = g_net[i][0][:, -band:]
            assert bool((g == 0).all()) and not bool(torch.signbit(g).any()), i
            w = net.linear_modules()[i].weight.detach()
            assert torch.equal(w[:, -band:], w0[i][:, -band:]) and not torch.equal(w[:, :-band], w0[i][:, :-band]), i
            assert float(g_net[i][0][:, :-band].abs().max()) > 0, i


@pytest.mark.gpu
@pytest.mark.parametrize("first", [8, 20])
@pytest.mark.parametrize("shape", SHAPES)
def test_past_the_end_a_step_leaves_the_bits_of_a_step_with_nothing_attached(dev, scene, shape, first):
    import nerf
    runs = []
    for anneal in (nerf.EncodingAnneal(0, 8), None):
        nets = make_pair(shape, dev)
        step, bucket = train_step(scene, dev, shape, nets, first_iteration=first, encoding_anneal=anneal)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        loss = step.forward_backward().clone()
        grads = bucket.flat.clone()
        opt.step()
        runs.append((loss, grads, bucket.flat_params.clone()))
    assert same(runs[0], runs[1]) and float(runs[0][1].abs().max()) > 0


def params_of(nets):
    return [p.detach().clone() for net in nets for p in net.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_replayed_training_steps_follow_the_schedule_like_eager_ones(dev, scene, shape, precision):
    """start = 0, end = 8, six steps: a host amplitude baked into the capture would freeze the table at the captured iteration."""
    import nerf
    nerf.set_precision(precision)
    runs = []
    for use_graphs in (True, False):
        nets = make_pair(shape, dev)
        step, bucket = train_step(scene, dev, shape, nets, encoding_anneal=nerf.EncodingAnneal(0, 8))
        graphed = nerf.GraphedTrainStep(step, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3, use_graphs=use_graphs)
        tables = []
        for it in range(6):
            graphed.step()
            torch.cuda.synchronize()
            check_table(step.anneal.amplitudes(), it, 0, 8, NETS[shape]["num_encoding_fn_xyz"], 4, what=f"graphs={use_graphs}")
            tables.append(step.anneal.amplitudes().clone())
        assert graphed.fallback_reason is None and (graphed.graphs is not None) == use_graphs, graphed.fallback_reason
        assert not torch.equal(tables[3], tables[5])
        runs.append((params_of(nets), tables, step.loss3.clone()))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert all(bool(torch.isfinite(p).all()) for p in runs[0][0])


def make_joint(scene, dev, shape, nets, seed=21, **kw):
    import nerf
    from nerf import parallel, synthetic as syn
    ex, ed = encoders(shape)
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in TRAIN_POSES]).to(dev)
    k = torch.from_numpy(syn.intrinsic(TRAIN_H, TRAIN_W)).to(dev)
    bucket = parallel.FlatGradBucket(list(nets))
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    step = nerf.FusedJointStep(nets[0], nets[1], scene.cfg, TRAIN_H, TRAIN_W, k, e0, scene.images, ex, ed, RAYS[shape], bucket, opt, 1e-3,
                               seed=seed, fixed_views=(0,), **kw)
    return step, bucket, opt


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_replayed_joint_steps_follow_the_schedule_like_eager_ones(dev, scene, shape):
    import nerf
    runs = []
    for use_graphs in (True, False):
        nets = make_pair(shape, dev)
        step, _, _ = make_joint(scene, dev, shape, nets, encoding_anneal=nerf.EncodingAnneal(0, 8), eager_iterations=1, use_graphs=use_graphs)
        for it in range(4):
            step.step()
            torch.cuda.synchronize()
            check_table(step.anneal.amplitudes(), it, 0, 8, NETS[shape]["num_encoding_fn_xyz"], 4, what=f"joint graphs={use_graphs}")
        assert step.fallback_reason is None and (step.graph is not None) == use_graphs, step.fallback_reason
        runs.append((params_of(nets), step.xi.clone(), step.loss3.clone()))
    assert same(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert float(runs[0][1][1:].abs().max()) > 0 and bool(torch.isfinite(runs[0][2]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16-s16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_camera_half_of_the_joint_step_equals_the_premultiplied_clones(dev, scene, shape, precision):
    import nerf
    nerf.set_precision(precision)
    nets = make_pair(shape, dev)
    amp = table_at(dev, shape, 37, 0, 100)
    clones = premultiplied(nets, amp, dev)
    got, _, _ = make_joint(scene, dev, shape, nets, first_iteration=37, encoding_anneal=nerf.EncodingAnneal(0, 100), use_graphs=False)
    ref, _, _ = make_joint(scene, dev, shape, clones, first_iteration=37, use_graphs=False)
    plain, _, _ = make_joint(scene, dev, shape, make_pair(shape, dev), first_iteration=37, use_graphs=False)
    for step in (got, ref, plain):
        step.step()
    torch.cuda.synchronize()
    assert torch.equal(got.anneal.amplitudes(), amp)
    d_rays, d_rays_ref = got._keep[6], ref._keep[6]
    assert torch.equal(got.loss3, ref.loss3) and torch.equal(got.last_grad, ref.last_grad) and torch.equal(d_rays, d_rays_ref)
    assert float(got.last_grad[1:].abs().max()) > 0 and bool(torch.isfinite(d_rays).all()) and torch.equal(got.xi, ref.xi)
    assert not torch.equal(got.last_grad, plain.last_grad)


def run_graphed(scene, dev, shape, n, first_iteration=0, anneal=None, restore=None):
    import nerf
    from nerf import models
    nets = make_pair(shape, dev)
    step, bucket = train_step(scene, dev, shape, nets, first_iteration=first_iteration, encoding_anneal=anneal)
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    if restore is not None:
        for dst, src in zip((bucket.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_state), restore):
            dst.copy_(src)
        models.mark_parameters_updated()
    graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1)
    for _ in range(n):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.fallback_reason is None, graphed.fallback_reason
    return step, (bucket.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_state.clone())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_a_run_resumes_mid_schedule_from_its_state(dev, scene, shape):
    import nerf
    whole, end_whole = run_graphed(scene, dev, shape, 6, anneal=nerf.EncodingAnneal(0, 8, anneal_dir=False))
    first, mid = run_graphed(scene, dev, shape, 3, anneal=nerf.EncodingAnneal(0, 8, anneal_dir=False))
    state = first.anneal.state_dict(iteration=3)
    assert state == dict(start=0.0, end=8.0, anneal_dir=False, iteration=3)
    resumed = nerf.EncodingAnneal.from_state_dict(state)
    second, end_second = run_graphed(scene, dev, shape, 3, first_iteration=state["iteration"], anneal=resumed, restore=mid)
    assert same(end_whole, end_second) and torch.equal(whole.loss3, second.loss3)
    assert torch.equal(whole.anneal.amplitudes(), second.anneal.amplitudes())
    check_table(second.anneal.amplitudes(), 5, 0, 8, NETS[shape]["num_encoding_fn_xyz"], 4, anneal_dir=False, what="resumed")


@pytest.mark.gpu
def test_autograd_route_refuses_an_annealed_model_and_frozen_weights_still_differentiate_inputs(dev, scene):
    import nerf
    shape = "d6w128"
    ex, ed = encoders(shape)
    nets = make_pair(shape, dev)
    anneal = nerf.EncodingAnneal(0, 100).attach(*nets)
    anneal.set_iteration(37)
    focal, ro, rd = some_rays(scene, dev, 64)
    pts = (ro[:, None, :] + rd[:, None, :] * torch.linspace(2.0, 6.0, 9, device=dev)[None, :, None]).contiguous()
    rows = torch.cat((ro, rd, torch.zeros(64, 2, device=dev), torch.nn.functional.normalize(rd, dim=-1)), dim=-1)
    with pytest.raises(RuntimeError, match=r"EncodingAnneal attached cannot be trained through autograd.*FusedTrainStep\(encoding_anneal"):
        nerf.run_network(nets[1], pts, rows, 4096, ex, ed)
    with pytest.raises(RuntimeError, match="FusedJointStep"):
        nerf.run_one_iter_of_nerf(TRAIN_H, TRAIN_W, focal, nets[0], nets[1], ro, rd, scene.cfg, mode="train", encode_position_fn=ex,
                                  encode_direction_fn=ed)
    with pytest.raises(RuntimeError, match="FusedTrainStep"):
        nerf.run_network(nets[1], pts.clone().requires_grad_(True), rows, 4096, ex, ed)
    # frozen weights: the input gradient goes through the packs - equal to the pre-multiplied clone's, bit for bit
    clones = premultiplied(nets, anneal.amplitudes(), dev)
    grads = []
    for pair in (nets, clones):
        for p in pair[1].parameters():
            p.requires_grad_(False)
        x = pts.clone().requires_grad_(True)
        out = nerf.run_network(pair[1], x, rows, 4096, ex, ed)
        out.backward(torch.ones_like(out))
        grads.append((out.detach(), x.grad.clone()))
    assert same(grads[0], grads[1]) and float(grads[0][1].abs().max()) > 0


CLI = ["--size", "24", "--views", "3", "--num-random-rays", "200", "--layers", "6", "--width", "128", "--xyz-freqs", "6", "--num-coarse", "16",
       "--num-fine", "16", "--precision", "fp32", "--validate-every", "0", "--seed", "11", "--quiet"]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--refine-poses", "--pose-noise", "0.02", "0.04"]], ids=["train", "joint"])
def test_driver_stores_the_schedule_and_resumes_it(dev, tmp_path, flags):
    import eval_nerf
    import train_dexnerf
    mid, end = os.path.join(str(tmp_path), "mid.ckpt"), os.path.join(str(tmp_path), "end.ckpt")
    schedule = ["--anneal-encoding", "2", "12", "--anneal-xyz-only"]
    whole = train_dexnerf.main(CLI + flags + schedule + ["--iters", "8", "--save", end])
    train_dexnerf.main(CLI + flags + schedule + ["--iters", "4", "--save", mid])
    ck = torch.load(mid, map_location="cpu")
    assert ck["encoding_anneal"] == dict(start=2.0, end=12.0, anneal_dir=False, iteration=4)
    resumed = train_dexnerf.main(CLI + flags + ["--iters", "8", "--load-checkpoint", mid])        # the schedule comes from the checkpoint
    want = formula(8, 2, 12, 6) + [1.0] * 4
    assert max(abs(a - b) for a, b in zip(resumed["encoding_amplitudes"], want)) <= 1e-6
    assert resumed["encoding_amplitudes"] == whole["encoding_amplitudes"] and 0.0 < resumed["encoding_amplitudes"][3] < 1.0
    print("final loss: whole", float(whole["final_loss"]).hex(), "resumed", float(resumed["final_loss"]).hex())
    assert resumed["final_loss"] == whole["final_loss"] and resumed["val_psnr"] == whole["val_psnr"]
    assert torch.load(end, map_location="cpu")["encoding_anneal"]["iteration"] == 8
    # eval_nerf renders the mid-schedule checkpoint at its stored amplitudes: other pixels than the same weights without the entry
    render = ["--size", "24", "--views", "2", "--num-coarse", "16", "--num-fine", "16", "--precision", "fp32", "--quiet"]
    at_schedule = eval_nerf.main(["--checkpoint", mid] + render)["frames"]
    del ck["encoding_anneal"]
    bare = os.path.join(str(tmp_path), "bare.ckpt")
    torch.save(ck, bare)
    full_bands = eval_nerf.main(["--checkpoint", bare] + render)["frames"]
    assert all(bool(torch.isfinite(a[0]).all()) for a in at_schedule) and not torch.equal(at_schedule[0][0], full_bands[0][0])
