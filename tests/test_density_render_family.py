"""What the three density renders share (dn_render_rays_depth, dn_render_rays_depth_quantiles, dn_render_rays_normals): one set of
refusals under each entry point's own name, one workspace layout, one coarse pass.  A fourth density-only render inherits these.

Seeded 4 x 128 networks (L_xyz = 10), 37 rays, 16 + 16 samples, fp32.  Bit comparisons only: the three renders run the same launches on
the same inputs up to their last pass."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
N, NC, NF, K, Q = 37, 16, 16, 3, 2
ENTRIES = ("dn_render_rays_depth", "dn_render_rays_depth_quantiles", "dn_render_rays_normals")
SENTINEL = -7.25
SIZES = [(n, nc, nf) for n in (0, 1, 5, 4097) for nc, nf in ((16, 0), (16, 16), (64, 128))]


def rand(seed, *shape, normal=False):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) if normal else torch.rand(*shape, generator=g)).cuda()


@pytest.fixture(scope="module")
def family():
    """Packs, streams, rays and draws of the one case, built once."""
    import nerf
    from nerf import _hip, synthetic as syn
    assert torch.cuda.is_available()
    _hip.lib()
    nerf.set_precision("fp32")
    dev = torch.device("cuda:0")
    models = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**NET)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **NET).items()})
        models.append(m.to(dev))
    with torch.no_grad():
        packs = [m.packed_density(True, True, precision=_hip.PREC_F32) for m in models]
        streams = models[1].packed_density_grad(True, True, precision=_hip.PREC_F32)
    rd = rand(1, N, 3, normal=True)
    rays = torch.cat([rand(2, N, 3) - 0.5, rd, torch.full((N, 1), 2.0, device=dev), torch.full((N, 1), 6.0, device=dev)], dim=1).contiguous()
    draws = dict(t_rand=rand(3, N, NC), noise_c=rand(4, N, NC, normal=True), u=rand(5, N, NF), noise_f=rand(6, N, NC + NF, normal=True))
    thres = torch.tensor([0.5, 2.0, 8.0], dtype=torch.float32, device=dev)
    quantiles = torch.tensor([0.25, 0.5], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    return dict(dev=dev, packs=packs, streams=streams, rays=rays, draws=draws, thres=thres, quantiles=quantiles)


def raw_call(lib, f, entry, out, ws, desc_c=None, nc=NC, ws_offset=0, stride=8, k=K, packed_f="own"):
    """The C call of `entry` on the fixture's case - valid as it stands - with one argument replaced."""
    from nerf import _hip
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    pc, pf = f["packs"]
    nets = [ctypes.byref(pc.desc if desc_c is None else desc_c), p(pc.buffer), ctypes.byref(pf.desc), p(pf.buffer) if packed_f == "own" else packed_f]
    chunk = [_hip.PREC_F32, p(f["rays"]), stride, N, nc, NF, 0, 0.0, p(f["thres"]), k, None, None, None, None]
    wsp = ctypes.c_void_p(ws.data_ptr() + ws_offset)
    if entry == "dn_render_rays_normals":
        return lib.dn_render_rays_normals(*nets, p(f["streams"].buffer_bwd), p(f["streams"].buffer_ig), *chunk, p(out["depth_c"]), p(out["acc_c"]),
                                          p(out["depth_f"]), p(out["acc_f"]), p(out["dex"]), p(out["normal"]), p(out["dex_normal"]), wsp,
                                          ws.numel() - 256, None)
    maps = [p(out[name]) for name in ("depth_c", "acc_c", "depth_f", "acc_f", "dex")]
    if entry == "dn_render_rays_depth":
        return lib.dn_render_rays_depth(*nets, *chunk, *maps, wsp, None)
    return lib.dn_render_rays_depth_quantiles(*nets, *chunk, *maps, p(f["quantiles"]), Q, 0, p(out["qdepth"]), wsp, None)


def test_shared_refusals_name_the_entry_point_and_leave_the_outputs_alone(family):
    from nerf import _hip, _ops
    lib, dev = _hip.lib(), family["dev"]
    need = _ops.render_normals_workspace_bytes(*family["packs"], N, NC, NF)
    assert need >= lib.dn_render_depth_workspace_bytes(N, NC, NF) > 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    shapes = dict(depth_c=(N,), acc_c=(N,), depth_f=(N,), acc_f=(N,), dex=(K, N), qdepth=(Q, N), normal=(N, 3), dex_normal=(K, N, 3))
    out = {name: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev) for name, shape in shapes.items()}
    with_dirs = _hip.MlpDesc.from_buffer_copy(bytes(family["packs"][0].desc))
    with_dirs.use_viewdirs = 1
    refusals = {"a descriptor with use_viewdirs = 1": dict(desc_c=with_dirs), "num_fine > 0 with num_coarse = 9": dict(nc=9),
                "a workspace pointer offset by 16 bytes": dict(ws_offset=16), "ray_stride = 7": dict(stride=7),
                "a negative threshold count": dict(k=-1), "a fine pass without a fine pack": dict(packed_f=None)}
    for what, kw in refusals.items():
        texts = set()
        for entry in ENTRIES:
            assert raw_call(lib, family, entry, out, ws, **kw) != 0, (what, entry)
            err = lib.dn_last_error().decode()
            assert err.startswith(entry + ": "), (what, entry, err)
            texts.add(err[len(entry):])
        assert len(texts) == 1, (what, texts)
    torch.cuda.synchronize()
    for name, t in out.items():
        assert bool((t == SENTINEL).all()), name
    assert int(ws.sum()) == 0   # nor was the workspace (its status block among it) written


def layout_bytes(n, nc, nf, weights):
    """The render workspaces restated: regions rounded up to 256 bytes each, the status block the last 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    regions = [4 * n * nc, 16 * n * nc] + ([4 * n * nc] if weights else [])           # z_c, rf_c, the coarse weights
    regions += [4 * n * (nc + nf), 16 * n * (nc + nf)] if nf else []                     # z_f, rf_f
    return sum(up(b) for b in regions) + 256


@pytest.mark.parametrize("n,nc,nf", SIZES)
def test_workspace_sizes_equal_the_restated_layout(n, nc, nf):
    from nerf import _hip
    lib = _hip.lib()
    assert lib.dn_render_depth_workspace_bytes(n, nc, nf) == layout_bytes(n, nc, nf, weights=False)
    assert lib.dn_render_workspace_bytes(n, nc, nf) == layout_bytes(n, nc, nf, weights=True)


def test_the_three_renders_share_their_coarse_pass_bit_for_bit(family):
    from nerf import _ops
    same = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
    args = (*family["packs"], family["rays"], NC, NF, False, 0.25, family["thres"], family["draws"])
    depth = _ops.render_rays_depth(*args)
    quant = _ops.render_rays_depth(*args, quantiles=family["quantiles"])
    normals = _ops.render_rays_normals(*family["packs"], family["streams"], *args[2:])
    torch.cuda.synchronize()
    assert len(depth) == 5 and len(quant) == 6 and len(normals) == 7
    for i, name in enumerate(("depth_c", "acc_c")):
        assert same(depth[i], quant[i]) and same(depth[i], normals[i]), name
        assert bool(torch.isfinite(depth[i]).all()) and float(depth[i].abs().max()) > 0.0, name
    for i, name in ((2, "depth_f"), (3, "acc_f"), (4, "dex")):      # the quantile pass is the depth pass with a readout beside it
        assert same(depth[i], quant[i]), name
    # (the normals render's last pass runs the training-forward kernel: its depth / acc / dex are not compared bit for bit)
    assert normals[2].shape == (N,) and normals[4].shape == (K, N) and quant[5].shape == (Q, N)
