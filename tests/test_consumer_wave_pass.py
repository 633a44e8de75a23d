"""The fixed-shape W = 256 render instances of the 48-point forward kernel compile their persistent tile loop once per wave role
(mlp_fused48_kernel.h tile_loop: waves 0-3 fetch the weight stream, waves 4-7 only consume it) and a wave picks its copy once, behind
the prologue.  The two copies must stay one pass: the same barriers per period, the same ring positions, the same counted waits.

Reference: the run-time-shape 48-point kernel (DEXNERF_G48_RUNTIME_SHAPE=1, read per call) - one compiler-scheduled loop for every
wave, the same pieces, products and accumulation order.  Outputs must be EQUAL, for the instance that encodes tile t + 1 inside tile t's
view-direction stage (rays + depths, the default) and for the plain one (DEXNERF_G48_NO_OVERLAP=1), in bf16 and fp16, at the sizes where
a split can go wrong: a ragged single tile, exactly one tile, one workgroup wrapping the ring into a second tile, several tiles per
workgroup with a ragged last one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
TILE = 384   # points per workgroup tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()  # must load: no fallback
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    import nerf
    from nerf import synthetic as syn
    m = nerf.models.FlexibleNeRFModel(**KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(15, sigma_gain=5.0, sigma_bias=0.0, **KW).items()})
    return m.to(dev)


def case_shapes(dev):
    """(rays, samples) per case; C = compute units = the most workgroups a launch gets (one per tile up to one per unit)."""
    c = torch.cuda.get_device_properties(dev).multi_processor_count
    return {
        "ragged_single_tile": (37, 53),                                   # partial tile, partial wave, partial point group
        "exactly_one_tile": (6, 64),                                      # prologue straight into the last tile
        "one_workgroup_wraps": ((c + 1) * (TILE // 64), 64),              # C + 1 tiles: workgroup 0 runs two, the ring wraps once
        "several_tiles_per_workgroup": ((3 * c + 5) * (TILE // 192) - 1, 192),   # 3C + 5 tiles, the last one half full
    }


def case_inputs(dev, name):
    n_rays, s = case_shapes(dev)[name]
    gen = torch.Generator(device="cpu").manual_seed(1000 + n_rays + s)
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).to(dev)
    rays = torch.cat([torch.randn(n_rays, 3, generator=gen).to(dev), vd * 1.5, torch.zeros(n_rays, 2, device=dev), vd], -1).contiguous()
    z = torch.sort(torch.rand(n_rays, s, generator=gen) * 4 + 2, -1)[0].to(dev).contiguous()
    return rays, z


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


CASES = ["ragged_single_tile", "exactly_one_tile", "one_workgroup_wraps", "several_tiles_per_workgroup"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prec16", ["bf16", "fp16"])
def test_role_split_instances_equal_the_runtime_shape_kernel(dev, net, monkeypatch, prec16, case):
    import nerf
    n_rays, s = case_shapes(dev)[case]
    if case == "one_workgroup_wraps":
        assert (n_rays * s) // TILE == torch.cuda.get_device_properties(dev).multi_processor_count + 1 and (n_rays * s) % TILE == 0
    if case == "several_tiles_per_workgroup":
        assert (n_rays * s) % TILE == TILE // 2
    nerf.set_precision(prec16)
    try:
        pk = net.packed()
        rays, z = case_inputs(dev, case)
        ref = run_network(monkeypatch, pk, rays, z, DEXNERF_G48_RUNTIME_SHAPE="1")
        assert ref.shape == (n_rays, s, 4) and torch.isfinite(ref).all()
        in_stage = run_network(monkeypatch, pk, rays, z)                                  # next tile's encoding inside the stage
        plain = run_network(monkeypatch, pk, rays, z, DEXNERF_G48_NO_OVERLAP="1")       # every tile encoded at its top
        for label, out in (("in-stage encoding", in_stage), ("plain", plain)):
            differ = int((out != ref).any(-1).sum())
            print(f"{prec16} {case} {label}: {differ} of {n_rays * s} points differ from the run-time-shape kernel")
            assert torch.equal(out, ref), (prec16, case, label, differ)
    finally:
        nerf.set_precision("fp32")


@pytest.mark.parametrize("prec16", ["bf16", "fp16"])
def test_two_calls_give_the_same_bits(dev, net, monkeypatch, prec16):
    """A race between the two roles around a barrier (a slot recycled before the other role has left it) shows as a run-to-run
    difference: several tiles per workgroup, both instances, twice each."""
    import nerf
    nerf.set_precision(prec16)
    try:
        pk = net.packed()
        rays, z = case_inputs(dev, "several_tiles_per_workgroup")
        for env in ({}, {"DEXNERF_G48_NO_OVERLAP": "1"}):
            a = run_network(monkeypatch, pk, rays, z, **env)
            b = run_network(monkeypatch, pk, rays, z, **env)
            assert torch.isfinite(a).all() and torch.equal(a, b), (prec16, env)
    finally:
        nerf.set_precision("fp32")


def test_render_rays_equals_the_stage_composition_through_the_runtime_shape_kernel(dev, monkeypatch):
    """dn_render_rays end to end (16 x 16 rays, 64 + 128 samples, bf16) against the same render composed stage by stage with both
    network launches on the run-time-shape kernel: every map equal."""
    import nerf
    from nerf import _ops, synthetic as syn
    thres = [float(m) for m in range(5, 105, 5)]
    nerf.set_precision("bf16")
    try:
        nets = []
        for seed, bias in ((42, -150.0), (43, -20.0)):
            m = nerf.models.FlexibleNeRFModel(**KW)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **KW).items()})
            nets.append(m.to(dev))
        pc, pf = nets[0].packed(), nets[1].packed()
        n, nc, nf = 16 * 16, 64, 128
        g = torch.Generator(device="cpu").manual_seed(77)
        rd = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(n, 3, generator=g), dim=-1) * 1.3
        ro = torch.tensor([0.0, 0.0, 4.0]) + 0.05 * torch.randn(n, 3, generator=g)
        rays = torch.cat([ro, rd, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), torch.nn.functional.normalize(rd, dim=-1)], -1).to(dev).contiguous()
        with torch.no_grad():
            got = _ops.render_rays(pc, pf, rays, nc, nf, False, 0.0, False, thres)
            monkeypatch.setenv("DEXNERF_G48_RUNTIME_SHAPE", "1")
            try:
                z_c = _ops.coarse_depths(rays, nc, False, None)
                rf_c = _ops.run_network_rays(pc, rays, z_c)
                rgb_c, _, acc_c, w_c, depth_c, _ = _ops.volume_render_fwd(rf_c, z_c, rays[:, 3:6], None, 0.0, False, [])
                z_f = _ops.fine_depths(z_c, w_c, nf, None)
                rf_f = _ops.run_network_rays(pf, rays, z_f)
                rgb_f, _, acc_f, _, depth_f, dex = _ops.volume_render_fwd(rf_f, z_f, rays[:, 3:6], None, 0.0, False, thres)
            finally:
                monkeypatch.delenv("DEXNERF_G48_RUNTIME_SHAPE")
        want = (rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, dex)
        names = ("rgb_coarse", "depth_coarse", "acc_coarse", "rgb_fine", "depth_fine", "acc_fine", "dex")
        assert float(rf_f.abs().max()) > 0.0   # the maps carry network outputs
        for name, a, b in zip(names, got, want):
            assert a.shape == b.shape and torch.isfinite(a).all(), name
            print(f"{name}: {int((a != b).sum())} of {a.numel()} values differ")
            assert torch.equal(a, b), name
    finally:
        nerf.set_precision("fp32")
