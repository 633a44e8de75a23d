"""The render driver's network launches claim their tiles from a device counter (mlp_fused48_kernel.h "claimed tiles": a workgroup's
first tile is blockIdx.x, every later one comes from an atomic add on a word of the render's status block) instead of striding by the
grid size.  Which workgroup computes a tile must not show in any output bit.

dn_render_rays is the entry point that hands out counters, so the launches under test are its coarse and its fine launch (D8/W256
synthetic nets, rays + depths input, 64 + 128 samples: two rays per 384-point tile of the fine launch); their raw outputs and depths
are read back from the render workspace and compared, bit for bit, with the same launch without a counter (dn_run_network on the same
depths: the fixed stride) and with the run-time-shape kernel (DEXNERF_G48_RUNTIME_SHAPE=1).  Fine-launch tile counts, C = compute
units: 5 (most workgroups claim nothing that exists and leave after one tile), exactly C, C + 1, 3C + 5 with a half-full last tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
TILE = 384            # points per workgroup tile
NC, NF = 64, 128
QUEUE = 2             # claimed ids a workgroup holds beyond the tile it runs
WORD_COARSE, WORD_FINE = 16, 32   # status-block words of the two counters (api.cpp kStatusTilesCoarse / kStatusTilesFine)
THRES = [float(m) for m in range(5, 105, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()  # must load: no fallback
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    import nerf
    from nerf import synthetic as syn
    out = []
    for seed, bias in ((42, -150.0), (43, -20.0)):
        m = nerf.models.FlexibleNeRFModel(**KW)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **KW).items()})
        out.append(m.to(dev))
    return out


def units(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def fine_tiles(dev):
    c = units(dev)
    return {"under_full_grid": 5, "exactly_c": c, "c_plus_one": c + 1, "three_c_plus_five_half_full": 3 * c + 5}


def rays_of(dev, case):
    """Ray count whose fine launch (192 samples) has the case's tile count; the last case ends in a half-full tile."""
    t = fine_tiles(dev)[case]
    per_tile = TILE // (NC + NF)
    return t * per_tile - (1 if case == "three_c_plus_five_half_full" else 0)


def make_rays(dev, n):
    g = torch.Generator(device="cpu").manual_seed(4000 + n)
    rd = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(n, 3, generator=g), dim=-1) * 1.3
    ro = torch.tensor([0.0, 0.0, 4.0]) + 0.05 * torch.randn(n, 3, generator=g)
    return torch.cat([ro, rd, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), torch.nn.functional.normalize(rd, dim=-1)], -1).to(dev).contiguous()


def workspace_views(n):
    """(z_c, rf_c, z_f, rf_f, status words) of the latest dn_render_rays call on this stream, copied out of its workspace (api.cpp
    carve: z_c | rf_c | w_c | z_f | rf_f | 256-byte status block, each region padded to 256 bytes)."""
    from nerf import _ops
    ws = _ops._latest_render_workspace()
    off = 0

    def take(floats):
        nonlocal off
        t = ws[off: off + floats * 4].view(torch.float32).clone()
        off += (floats * 4 + 255) // 256 * 256
        return t
    z_c = take(n * NC).reshape(n, NC)
    rf_c = take(n * NC * 4).reshape(n, NC, 4)
    take(n * NC)
    z_f = take(n * (NC + NF)).reshape(n, NC + NF)
    rf_f = take(n * (NC + NF) * 4).reshape(n, NC + NF, 4)
    assert off + 256 == ws.numel()
    status = ws[off: off + 256].view(torch.int32).clone()
    return z_c, rf_c, z_f, rf_f, status


def check_counter(dev, name, word, n_points):
    n_tiles = (n_points + TILE - 1) // TILE
    grid = min(n_tiles, units(dev))
    value = grid + int(word)      # the next id the counter would hand out: ids start at the grid size, the word at zero
    print(f"{name}: {n_tiles} tiles on {grid} workgroups, counter at {value}")
    # every tile past the first of each workgroup was claimed exactly once (ids are handed out in order: reaching n_tiles means none
    # was skipped, and an atomic add hands none out twice); a workgroup gives up at most its queue of ids past the end
    assert n_tiles <= value <= n_tiles + grid * QUEUE, (name, n_tiles, grid, value)


def run_network(monkeypatch, pk, rays, z, **env):
    from nerf import _ops
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with torch.no_grad():
            return _ops.run_network_rays(pk, rays, z)
    finally:
        for k in env:
            monkeypatch.delenv(k)


CASES = ["under_full_grid", "exactly_c", "c_plus_one", "three_c_plus_five_half_full"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prec16", ["bf16", "fp16"])
def test_claimed_launches_equal_the_fixed_stride_and_the_runtime_shape_kernel(dev, nets, monkeypatch, prec16, case):
    import nerf
    from nerf import _ops
    n = rays_of(dev, case)
    n_tiles = fine_tiles(dev)[case]
    assert (n * (NC + NF) + TILE - 1) // TILE == n_tiles
    if case == "three_c_plus_five_half_full":
        assert (n * (NC + NF)) % TILE == TILE // 2
    nerf.set_precision(prec16)
    try:
        pc, pf = nets[0].packed(), nets[1].packed()
        rays = make_rays(dev, n)
        with torch.no_grad():
            maps = [m.clone() for m in _ops.render_rays(pc, pf, rays, NC, NF, False, 0.0, False, THRES)]
        z_c, rf_c, z_f, rf_f, status = workspace_views(n)
        assert torch.isfinite(rf_c).all() and torch.isfinite(rf_f).all() and float(rf_f.abs().max()) > 0.0
        assert int(status[0]) == 0 and int(status[1]) == 0   # what the fp16 guard sums: the counters are elsewhere
        check_counter(dev, f"{prec16} {case} coarse", status[WORD_COARSE], n * NC)
        check_counter(dev, f"{prec16} {case} fine", status[WORD_FINE], n * (NC + NF))
        for label, pk, z, got in (("coarse", pc, z_c, rf_c), ("fine", pf, z_f, rf_f)):
            stride = run_network(monkeypatch, pk, rays, z)                                    # same instance, no counter
            rt = run_network(monkeypatch, pk, rays, z, DEXNERF_G48_RUNTIME_SHAPE="1")
            for ref_name, ref in (("fixed stride", stride), ("run-time shape", rt)):
                differ = int((got != ref).any(-1).sum())
                print(f"{prec16} {case} {label}: {differ} of {got.shape[0] * got.shape[1]} points differ from the {ref_name} launch")
                assert torch.equal(got, ref), (prec16, case, label, ref_name, differ)
        # a second call: the driver zeroes the counters again, the bits are the same
        with torch.no_grad():
            again = _ops.render_rays(pc, pf, rays, NC, NF, False, 0.0, False, THRES)
        _, rf_c2, _, rf_f2, status2 = workspace_views(n)
        assert torch.equal(rf_c2, rf_c) and torch.equal(rf_f2, rf_f)
        for a, b in zip(maps, again):
            assert torch.equal(a, b)
        assert int(status2[WORD_COARSE]) == int(status[WORD_COARSE]) and int(status2[WORD_FINE]) == int(status[WORD_FINE])
        check_counter(dev, f"{prec16} {case} fine, second call", status2[WORD_FINE], n * (NC + NF))
    finally:
        nerf.set_precision("fp32")


@pytest.mark.parametrize("prec16", ["bf16", "fp16"])
def test_render_rays_equals_the_stage_composition_and_the_guard_does_not_see_the_counters(dev, nets, monkeypatch, prec16):
    """dn_render_rays (16 x 16 rays, 64 + 128 samples, 20 Dex thresholds) against the same render composed stage by stage with both
    network launches on the run-time-shape kernel: every map equal; status words 0 and 1 stay zero."""
    import nerf
    from nerf import _ops
    nerf.set_precision(prec16)
    try:
        pc, pf = nets[0].packed(), nets[1].packed()
        n = 16 * 16
        rays = make_rays(dev, n)
        with torch.no_grad():
            got = _ops.render_rays(pc, pf, rays, NC, NF, False, 0.0, False, THRES)
            words = _ops.render_status_words().tolist()
            count = _ops.render_nonfinite_count()
            status = workspace_views(n)[4]
            monkeypatch.setenv("DEXNERF_G48_RUNTIME_SHAPE", "1")
            try:
                z_c = _ops.coarse_depths(rays, NC, False, None)
                rf_c = _ops.run_network_rays(pc, rays, z_c)
                rgb_c, _, acc_c, w_c, depth_c, _ = _ops.volume_render_fwd(rf_c, z_c, rays[:, 3:6], None, 0.0, False, [])
                z_f = _ops.fine_depths(z_c, w_c, NF, None)
                rf_f = _ops.run_network_rays(pf, rays, z_f)
                rgb_f, _, acc_f, _, depth_f, dex = _ops.volume_render_fwd(rf_f, z_f, rays[:, 3:6], None, 0.0, False, THRES)
            finally:
                monkeypatch.delenv("DEXNERF_G48_RUNTIME_SHAPE")
        assert words == [0, 0] and count == 0
        assert int(status[WORD_COARSE]) > 0 and int(status[WORD_FINE]) > 0   # the launches did claim
        want = (rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, dex)
        names = ("rgb_coarse", "depth_coarse", "acc_coarse", "rgb_fine", "depth_fine", "acc_fine", "dex")
        assert float(rf_f.abs().max()) > 0.0
        for name, a, b in zip(names, got, want):
            assert a.shape == b.shape and torch.isfinite(a).all(), name
            print(f"{prec16} {name}: {int((a != b).sum())} of {a.numel()} values differ")
            assert torch.equal(a, b), name
    finally:
        nerf.set_precision("fp32")
