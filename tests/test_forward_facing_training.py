"""Forward-facing training on the fused kernels: networks with a 6-frequency xyz encoding (L_xyz = 6: the reference's fern / llff
configs, the shipped fern-lowres checkpoint, FlexibleNeRFModel()'s default) and NDC rays (dataset.no_ndc: False).

Every GPU test proves that the fused route ran: while the fused call runs, the nn.Linear composition (FlexibleNeRFModel._forward_modules)
and the torch-encoding fallback (_train._modules_on_points) raise."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import rel_err


def C(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def no_fallback(monkeypatch):
    """The fused route or an error: the two compositions a training call could fall back to raise while the block runs."""
    import nerf
    from nerf import _train

    def boom(*a, **k):
        raise AssertionError("the training call left the fused kernels")
    with monkeypatch.context() as mp:
        mp.setattr(nerf.models.FlexibleNeRFModel, "_forward_modules", boom)
        mp.setattr(_train, "_modules_on_points", boom)
        yield


def torch_encoding(x, num_fns, log_sampling):
    """positional_encoding (reference nerf/nerf_helpers.py:115-159) as plain torch ops."""
    if log_sampling:
        freqs = 2.0 ** torch.linspace(0.0, num_fns - 1, num_fns, dtype=x.dtype, device=x.device)
    else:
        freqs = torch.linspace(2.0 ** 0.0, 2.0 ** (num_fns - 1), num_fns, dtype=x.dtype, device=x.device)
    out = [x]
    for f in freqs:
        out += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(out, -1)


def g48_pe_col(kind, g, u, L):
    """csrc/mlp_geo48.h g48_pe_col: encoding column of slot u of lane group g in the 48-point geometry, -1 for padding."""
    slots = 16 if kind == 1 else 8
    comp = (u + g) % 3
    rank = sum(1 for gg in range(g + 1) for uu in range(u if gg == g else slots) if (uu + gg) % 3 == comp)
    if rank == 0:
        return comp
    f, is_cos = (rank - 1) // 2, (rank - 1) % 2
    return 3 + 6 * f + 3 * is_cos + comp if f < L else -1


def pe_slot_col(L, h, u):
    """csrc/mlp_layout.h pe_slot_col: the 32-point geometry's slot -> encoding column, -1 for padding."""
    nf = L // 2
    if u < 6 * nf:
        return 3 + 6 * ((nf if h else 0) + u // 6) + (u % 6)
    v = u - 6 * nf
    if h == 0:
        return v if v < 2 else -1
    return 2 if v == 0 else -1


def mlp_desc(l_xyz, depth=4, width=128):
    from nerf import _hip
    return _hip.MlpDesc(num_layers=depth, hidden_size=width, skip_connect_every=4, num_encoding_fn_xyz=l_xyz, num_encoding_fn_dir=4,
                        include_input_xyz=1, include_input_dir=1, use_viewdirs=1, log_sampling_xyz=1, log_sampling_dir=1)


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_xyz", [6, 10])
def test_the_64_wide_xyz_panel_holds_every_encoding_column_once(l_xyz):
    """Both geometries' slot maps put each of the 3 + 6 L columns in exactly one slot of the 64-slot panel; every other slot is padding
    (the weight-gradient epilogues drop it, the forward stores zeros there)."""
    for cols in ([g48_pe_col(1, g, u, l_xyz) for g in range(4) for u in range(16)],
                 [pe_slot_col(l_xyz, h, u) for h in range(2) for u in range(32)]):
        live = [c for c in cols if c >= 0]
        assert sorted(live) == list(range(3 + 6 * l_xyz))
        assert len(cols) - len(live) == 64 - (3 + 6 * l_xyz)


def test_training_sizes_cover_l_xyz_6_and_refuse_others(hiplib):
    """dn_mlp_train_sizes sizes the saved tensors of an L_xyz = 6 net in all three training precisions (the panel is the same
    64-wide one as L_xyz = 10's, so are the sizes); L_xyz = 8 stays refused with DN_E_UNSUPPORTED and a message naming {6, 10}."""
    from nerf import _hip, _train
    import nerf
    assert _train.TRAIN_L_XYZ == (6, 10)
    assert _train.train_fused_ok(nerf.models.FlexibleNeRFModel())      # the reference's default net: 4 x 128, L_xyz = 6
    for depth, width in ((4, 128), (8, 256)):
        for prec in (_hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_BF16_S8):
            got = {}
            for l_xyz in (6, 10):
                a, m, g = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
                d = mlp_desc(l_xyz, depth, width)
                assert hiplib.dn_mlp_train_sizes(ctypes.byref(d), prec, 5000, ctypes.byref(a), ctypes.byref(m), ctypes.byref(g)) == 0, \
                    hiplib.dn_last_error()
                assert a.value > 0 and m.value > 0 and g.value > 0
                got[l_xyz] = (a.value, m.value, g.value)
            assert got[6] == got[10]
        assert hiplib.dn_mlp_backward_packed_bytes(ctypes.byref(mlp_desc(6, depth, width)), _hip.PREC_BF16_S8) > 0
    a, m, g = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    for prec in (_hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_BF16_S8):
        assert hiplib.dn_mlp_train_sizes(ctypes.byref(mlp_desc(8)), prec, 5000, ctypes.byref(a), ctypes.byref(m), ctypes.byref(g)) == -1001
        err = hiplib.dn_last_error()
        assert b"6" in err and b"10" in err
    assert hiplib.dn_mlp_backward_packed_bytes(ctypes.byref(mlp_desc(8)), _hip.PREC_BF16_S8) == 0


def test_ndc_draw_argument_validation_needs_no_gpu(hiplib):
    null = None
    assert hiplib.dn_select_rays_draw_ndc(4, 4, null, null, 0, 0.0, 1.0, null, 4, null, 0, null, null, null, 50.0, 1.0, null) == -1000
    assert b"dn_select_rays_draw_ndc" in hiplib.dn_last_error()
    cams = ctypes.c_void_p(16)   # (never dereferenced: the focal check comes first)
    assert hiplib.dn_select_rays_draw_ndc(4, 4, cams, cams, 1, 0.0, 1.0, cams, 4, null, 0, cams, null, null, 0.0, 1.0, null) == -1000
    assert b"focal" in hiplib.dn_last_error()


def test_fused_step_needs_a_focal_length_for_ndc():
    """FusedTrainStep.applicable accepts NDC rays only with the capture's focal length, and the constructor refuses NDC without one."""
    import nerf
    cfg = nerf.CfgNode(dict(dataset=dict(near=0.0, far=1.0, no_ndc=False),
                            nerf=dict(use_viewdirs=True, train=dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=True,
                                                                     radiance_field_noise_std=1.0, white_background=False))))
    nets = [nerf.models.FlexibleNeRFModel(num_encoding_fn_xyz=6, use_viewdirs=True) for _ in range(2)]
    ex, ed = nerf.get_embedding_function(6), nerf.get_embedding_function(4)
    assert not nerf.FusedTrainStep.applicable(nets[0], nets[1], cfg, ex, ed, 1024)
    assert nerf.FusedTrainStep.applicable(nets[0], nets[1], cfg, ex, ed, 1024, ndc_focal=400.0)
    with pytest.raises(ValueError, match="focal"):
        nerf.FusedTrainStep(nets[0], nets[1], None, cfg, None, ex, ed, 1024)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _bf16_renders():
    import nerf
    nerf.set_render_policy("bf16")
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def cosine(a, b):
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


@pytest.mark.gpu
@pytest.mark.parametrize("log_sampling", [True, False])
@pytest.mark.parametrize("depth,width,viewdirs,skip", [(4, 128, True, 4), (8, 256, True, 4), (5, 128, False, 2)])
def test_fused_training_l_xyz_6_shapes(dev, depth, width, viewdirs, skip, log_sampling, monkeypatch):
    """Parameter gradients of run_network on L_xyz = 6 nets through the fused training kernels in the three training precisions,
    against autograd over the nn.Linear composition on the torch encoding: fp32 to cosine > 0.99999 / 1e-3, bf16-s16 to cosine
    > 0.95, bf16-s8 (the 48-point geometry) to cosine > 0.99 against the bf16-s16 gradients."""
    import nerf
    from nerf import _train
    torch.manual_seed(13)
    kw = dict(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=viewdirs)
    base = nerf.models.FlexibleNeRFModel(**kw).to(dev)
    assert _train.train_fused_ok(base)
    n, s = 23, 47
    pts = torch.randn(n, s, 3, device=dev)
    vd = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1)
    rays = torch.cat([torch.zeros(n, 8, device=dev), vd], -1)
    g_up = torch.randn(n, s, 4, device=dev)
    emb = torch_encoding(pts.reshape(-1, 3), 6, log_sampling)
    if viewdirs:
        emb = torch.cat([emb, torch_encoding(vd[:, None, :].expand(n, s, 3).reshape(-1, 3), 4, log_sampling)], -1)
    (base._forward_modules(emb).reshape(n, s, 4) * g_up).sum().backward()
    ref = {k: C(p.grad).astype(np.float64).reshape(-1) for k, p in base.named_parameters()}
    ex = nerf.get_embedding_function(6, True, log_sampling)
    ed = nerf.get_embedding_function(4, True, log_sampling) if viewdirs else None
    got = {}
    for prec in ("fp32", "bf16-s16", "bf16-s8"):
        nerf.set_precision(prec)
        m = nerf.models.FlexibleNeRFModel(**kw).to(dev)
        m.load_state_dict(base.state_dict())
        with no_fallback(monkeypatch):
            out = nerf.run_network(m, pts, rays, 4096, ex, ed)
            (out * g_up).sum().backward()
        got[prec] = {k: C(p.grad).astype(np.float64).reshape(-1) for k, p in m.named_parameters()}
    nerf.set_precision("fp32")
    for k in ref:
        assert cosine(got["fp32"][k], ref[k]) > 0.99999, ("fp32", k)
        assert rel_err(got["fp32"][k], ref[k]) < 1e-3, ("fp32", k)
        assert cosine(got["bf16-s16"][k], ref[k]) > 0.95, ("bf16-s16", k)
        assert cosine(got["bf16-s8"][k], got["bf16-s16"][k]) > 0.99, ("bf16-s8", k)


@pytest.mark.gpu
def test_s8_xyz_panel_of_an_l_xyz_6_net_is_padded_with_zero_bytes(dev, monkeypatch):
    """The 8-bit saved xyz unit of an L_xyz = 6 net (48-point geometry, ragged point count: a partial 384-point tile): its 39 live
    columns are the e4m3 rounding of the HIP encoding, and every byte of a slot g48_pe_col maps to no column is an exact zero (a
    non-finite byte there would meet a zero weight in the 64-deep contraction of the weight gradient: NaN x 0 = NaN)."""
    import nerf
    from nerf import _hip, _ops
    nerf.set_precision("bf16-s16")
    torch.manual_seed(4)
    m = nerf.models.FlexibleNeRFModel(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                                      use_viewdirs=True).to(dev)
    pk = m.packed()
    _ops.pack_backward(pk, [x.weight for x in m.linear_modules()], _hip.PREC_BF16_S8)
    assert _ops.s8_supported(pk)
    n_rays, s = 29, 41
    n = n_rays * s                       # 1189 points: 3 whole 384-point tiles + 37 points
    pts = (torch.rand(n, 3, device=dev) * 2 - 1) * 3.0
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
    with no_fallback(monkeypatch):
        out8, act8, _ = _ops.run_network_train(pk, pts, vd, s, prec=_hip.PREC_BF16_S8)
    assert bool(torch.isfinite(out8).all())
    xyz = _ops.mlp_unpack(pk, 0, act8, n, 0, m.dim_xyz, 1, torch.full((n, m.dim_xyz), float("nan"), device=dev), prec=_hip.PREC_BF16_S8)
    enc = _ops.positional_encoding(pts, 6, True, True)
    assert xyz.shape == enc.shape == (n, 39) and bool(torch.isfinite(xyz).all())
    want = enc.to(torch.bfloat16).to(torch.float8_e4m3fn).float()
    # (the kernel's hardware sine and the encoding kernel's differ in the last bits: a value next to an e4m3 rounding boundary may
    #  round to the neighbour - one e4m3 step at most)
    exact = (xyz == want).double().mean().item()
    assert exact > 0.99, exact
    assert bool(((xyz - want).abs() <= 0.125 * want.abs() + 2.0 ** -9).all())
    # raw bytes: units of 1 KiB, record T = G / 2 holds per slot the units of groups 2T and 2T + 1 side by side (mlp_geo48.h)
    units_per_group = 1 + 1 + 2 + 3 * 2 + 2 + 1     # xyz, dir, layer1, 3 trunk stages, fc_feat, layers_dir.0 (W = 128)
    raw = act8.view(torch.uint8).reshape(-1)
    groups = (n + 15) // 16
    g_idx = torch.arange(groups, device=dev)
    base_unit = ((g_idx // 2) * units_per_group) * 2 + (g_idx % 2)                  # slot 0: the xyz panel
    unit = raw[(base_unit[:, None] * 1024 + torch.arange(1024, device=dev)[None, :]).reshape(-1)].reshape(groups, 64, 16)
    pad = torch.tensor([[g48_pe_col(1, lane // 16, b, 6) < 0 for b in range(16)] for lane in range(64)], device=dev)
    lane = torch.arange(64, device=dev)
    j = (lane % 16) ^ (((lane // 16) % 2) * 8)                                       # stored rows of odd lane groups are swizzled
    valid = (g_idx[:, None] * 16 + j[None, :]) < n                                   # (groups, 64)
    mask = valid[:, :, None] & pad[None, :, :]
    assert int(pad.sum()) == 64 * 16 - 39 * 16
    assert int(mask.sum()) > 0 and int(unit[mask].max()) == 0
    assert int(unit[valid[:, :, None] & ~pad[None, :, :]].ne(0).sum()) > 0


def forward_facing_selector(h, w, f, dev, n_views=2, images=None):
    """Cameras of a forward-facing capture (looking down -z from z = 4, the layout of test_training_from_an_llff_capture) in the
    kernels' convention: E = inv([R diag(1, -1, -1) | t])."""
    import nerf
    k = torch.tensor([[f, 0.0, w * 0.5], [0.0, f, h * 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32)
    extr = []
    for v in range(n_views):
        c2w = np.eye(4)
        c2w[:3, :3] = np.diag([1.0, -1.0, -1.0])
        c2w[:3, 3] = [0.3 * v - 0.2, 0.1 * v, 4.0]
        extr.append(torch.from_numpy(np.linalg.inv(c2w).astype(np.float32)).to(dev))
    if images is None:
        images = torch.rand(n_views, h, w, 3, device=dev)
    return nerf.MultiViewRaySelector(h, w, extr, [k] * n_views, 0.0, 1.0, images=images, device=dev), extr, k


@pytest.mark.gpu
def test_ndc_draw_equals_a_plain_draw_followed_by_ndc_rays(dev):
    """dn_select_rays_draw_ndc on an RNG state = dn_select_rays_draw on the same state followed by dn_ndc_rays on columns 0:6 (near
    plane 1): rows bit for bit, the view directions (those of the unwarped rays), near / far, the target pixels and the drawn pixels
    identical, and the iteration counter advanced exactly as the plain draw advances it."""
    from nerf import _ops
    h, w, f = 36, 52, 47.5
    sel, _, _ = forward_facing_selector(h, w, f, dev, n_views=3)
    for it, view in ((0, sel.view), (4, None)):
        st_a, st_b = _ops.new_rng_state(31, dev, it), _ops.new_rng_state(31, dev, it)
        rays, target, pix = _ops.select_rays_draw(h, w, sel.cams, view, 0.0, 1.0, st_a, 700, sel.images, want_pixels=True)
        rays_n, target_n, pix_n = _ops.select_rays_draw(h, w, sel.cams, view, 0.0, 1.0, st_b, 700, sel.images, want_pixels=True, ndc_focal=f)
        ro, rd = _ops.ndc_rays(h, w, f, 1.0, rays[:, :3].contiguous(), rays[:, 3:6].contiguous())
        assert torch.equal(rays_n[:, :3], ro) and torch.equal(rays_n[:, 3:6], rd)
        assert torch.equal(rays_n[:, 6:], rays[:, 6:]) and torch.equal(target_n, target) and torch.equal(pix_n, pix)
        assert torch.equal(st_a, st_b) and st_b.tolist()[2] == it
        assert not torch.equal(rays_n[:, :6], rays[:, :6]) and bool(torch.isfinite(rays_n).all())


def make_ff_cfg(chunksize=4096, nc=64, nf=64, perturb=True, noise_std=0.5):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=False, num_coarse=nc, num_fine=nf, perturb=perturb, radiance_field_noise_std=noise_std,
                white_background=False)
    return nerf.CfgNode(dict(dataset=dict(near=0.0, far=1.0, no_ndc=False), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


FERN_KW = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True)


@pytest.mark.gpu
def test_one_ndc_training_step_of_the_fern_nets_against_the_cpu_oracle_fp32(dev, monkeypatch):
    """One training iteration of the 4 x 128, L_xyz = 6 nets on NDC rays (run_one_iter_of_nerf with no_ndc: False, near 0 / far 1,
    perturbed sampling + density noise, the draws injected) in the fp32 mode against autograd through the CPU oracle (oracle.ndc_rays +
    predict_and_render): loss 1e-4, every gradient 1e-3, the parameters after one Adam step 1e-4 (by the fraction of
    elements, as test_train_step_matches_reference: Adam's first step is ~lr sign(g) wherever |g| is at the 1e-8 level)."""
    import nerf
    from nerf import synthetic as syn
    from oracle import nerf_oracle as oc
    nerf.set_precision("fp32")
    sd_c, sd_f = syn.synth_state_dict(51, sigma_bias=-1.0, **FERN_KW), syn.synth_state_dict(52, sigma_bias=-1.0, **FERN_KW)
    nets = []
    for sd in (sd_c, sd_f):
        mdl = nerf.models.FlexibleNeRFModel(**FERN_KW)
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        nets.append(mdl.to(dev))
    mc, mf = nets
    h, w, f, n, nc, nf = 60, 80, 70.0, 128, 64, 64
    _, extr, kmat = forward_facing_selector(h, w, f, dev, n_views=1)
    ro, rd = nerf.get_ray_bundle(h, w, f, extr[0], kmat.to(dev))
    pick = torch.from_numpy(syn.select_rays(h, w, n, seed=3)).to(dev)
    ro, rd = ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous()
    gen = torch.Generator().manual_seed(17)
    draws = dict(t_rand=torch.rand(n, nc, generator=gen), noise_c=torch.randn(n, nc, generator=gen),
                 u=torch.rand(n, nf, generator=gen), noise_f=torch.randn(n, nc + nf, generator=gen))
    target = torch.rand(n, 3, generator=gen)
    q_rand, q_randn = [draws["t_rand"].to(dev), draws["u"].to(dev)], [draws["noise_c"].to(dev), draws["noise_f"].to(dev)]
    params = list(mc.parameters()) + list(mf.parameters())
    lr = 5e-3
    opt = torch.optim.Adam(params, lr=lr)
    ex, ed = nerf.get_embedding_function(6), nerf.get_embedding_function(4)
    with no_fallback(monkeypatch):
        monkeypatch.setattr(torch, "rand", lambda *a, **k: q_rand.pop(0))
        monkeypatch.setattr(torch, "randn", lambda *a, **k: q_randn.pop(0))
        out = nerf.run_one_iter_of_nerf(h, w, f, mc, mf, ro, rd, make_ff_cfg(nc=nc, nf=nf), mode="train", encode_position_fn=ex,
                                        encode_direction_fn=ed, m_thres_cand=None)
        monkeypatch.undo()
        tgt = target.to(dev)
        loss = nerf.img2mse(out[0], tgt) + nerf.img2mse(out[3], tgt)
        loss.backward()
    assert not q_rand and not q_randn
    # the oracle: NDC rows (view directions of the unwarped rays) through predict_and_render, autograd on the CPU
    ro_c, rd_c = ro.cpu(), rd.cpu()
    ro_n, rd_n = oc.ndc_rays(h, w, f, 1.0, ro_c, rd_c)
    rays_o = torch.cat([ro_n, rd_n, torch.zeros(n, 1), torch.ones(n, 1), rd_c / rd_c.norm(p=2, dim=-1, keepdim=True)], -1)
    tsd_c, tsd_f = oc.to_torch_sd(sd_c, requires_grad=True), oc.to_torch_sd(sd_f, requires_grad=True)
    mcfg = oc.ModelCfg(**FERN_KW)
    cfg_o = oc.RenderCfg(num_coarse=nc, num_fine=nf, near=0.0, far=1.0, perturb=True, noise_std=0.5, chunksize=4096, m_thres=())
    ref = oc.predict_and_render(rays_o, tsd_c, tsd_f, mcfg, mcfg, cfg_o, draws=draws)
    mse = torch.nn.functional.mse_loss
    loss_ref = mse(ref[0], target) + mse(ref[3], target)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    for model, tsd in ((mc, tsd_c), (mf, tsd_f)):
        for k, p in model.named_parameters():
            assert rel_err(C(p.grad), tsd[k].grad.numpy()) < 1e-3, k
    opt.step()
    ref_opt = torch.optim.Adam(list(tsd_c.values()) + list(tsd_f.values()), lr=lr)
    ref_opt.step()
    n_close = n_all = 0
    for model, tsd in ((mc, tsd_c), (mf, tsd_f)):
        for k, p in model.named_parameters():
            r = tsd[k].detach().numpy()
            close = np.abs(C(p) - r) <= 1e-4 * max(np.abs(r).max(), 1e-30)
            n_close += int(close.sum())
            n_all += close.size
            assert close.mean() > 0.85, (k, close.mean())
            assert np.abs(C(p) - r).max() < 2.5 * lr, k
    assert n_close / n_all > 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16-s8"])
def test_fused_ndc_train_step_equals_the_autograd_path_on_the_same_draws(dev, precision, monkeypatch):
    """nerf.FusedTrainStep on NDC rays (no_ndc: False, the focal length given) with the fern nets (4 x 128, L_xyz = 6) against
    predict_and_render_radiance under autograd fed the same NDC rows (the draw kernel's, checked against dn_ndc_rays) and the same
    in-kernel draws: the six maps bit for bit, the loss to 1e-5, the gradients to 1e-4 (fp32) / 2e-3 (bf16-s8); then the same step
    captured and replayed by GraphedTrainStep."""
    import nerf
    from nerf import _ops, parallel, synthetic as syn
    h, w, f, n = 40, 52, 45.0, 512
    cfg = make_ff_cfg()
    ex, ed = nerf.get_embedding_function(6), nerf.get_embedding_function(4)
    nerf.set_precision(precision)

    def models():
        out = []
        for seed in (61, 62):
            mdl = nerf.models.FlexibleNeRFModel(**FERN_KW)
            mdl.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **FERN_KW).items()})
            out.append(mdl.to(dev))
        return out
    sel, _, _ = forward_facing_selector(h, w, f, dev)
    sel.view.fill_(1)
    mc, mf = models()
    bucket = parallel.FlatGradBucket([mc, mf])
    step = nerf.FusedTrainStep(mc, mf, sel, cfg, bucket, ex, ed, n, seed=91, first_iteration=5, ndc_focal=f)
    peek = _ops.new_rng_state(91, dev, 5)
    rays_ref, target_ref = _ops.select_rays_draw(h, w, sel.cams, sel.view, 0.0, 1.0, peek, n, sel.images, ndc_focal=f)
    draws = [_ops.rng_fill(peek, 0, (n, 64)), _ops.rng_fill(peek, 1, (n, 64), normal=True), _ops.rng_fill(peek, 2, (n, 64)),
             _ops.rng_fill(peek, 3, (n, 128), normal=True)]
    with no_fallback(monkeypatch):
        loss3 = step.forward_backward()
        torch.cuda.synchronize()
    assert step.rng_state.tolist()[2:] == [5, 6]
    grads_fused = [p.grad.detach().clone() for p in bucket.params]
    maps_fused = step._keep[2]
    assert torch.equal(step._keep[3], rays_ref)
    mc2, mf2 = models()
    q_rand, q_randn = [draws[0], draws[2]], [draws[1], draws[3]]
    monkeypatch.setattr(torch, "rand", lambda *a, **k: q_rand.pop(0))
    monkeypatch.setattr(torch, "randn", lambda *a, **k: q_randn.pop(0))
    out = nerf.predict_and_render_radiance(rays_ref, mc2, mf2, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=None)
    monkeypatch.undo()
    assert not q_rand and not q_randn
    for a, b in zip(maps_fused[:6], out[:6]):
        assert torch.equal(a, b.detach())
    mse_c, mse_f = nerf.img2mse(out[0], target_ref), nerf.img2mse(out[3], target_ref)
    (mse_c + mse_f).backward()
    got = loss3.tolist()
    assert abs(got[0] - (mse_c + mse_f).item()) < 1e-5 * abs((mse_c + mse_f).item())
    tol = 1e-4 if precision == "fp32" else 2e-3
    for g, p in zip(grads_fused, list(mc2.parameters()) + list(mf2.parameters())):
        assert rel_err(C(g), C(p.grad)) < tol, (tuple(g.shape), rel_err(C(g), C(p.grad)))
    # graph capture and replay of the NDC iteration (FlatAdam; eager steps first, then one captured + replayed one)
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1)
    with no_fallback(monkeypatch):
        for _ in range(3):
            graphed.step()
        torch.cuda.synchronize()
    assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
    assert step.rng_state.tolist()[3] == 9 and bool(torch.isfinite(step.loss3).all())
    it = step.rng_state.tolist()[3]
    peek = _ops.new_rng_state(91, dev, it)
    rays_next, _ = _ops.select_rays_draw(h, w, sel.cams, sel.view, 0.0, 1.0, peek, n, sel.images, ndc_focal=f)
    graphed.step()                                    # a replay draws exactly what the eager draw of that iteration would
    torch.cuda.synchronize()
    assert torch.equal(step._keep[3], rays_next)


@pytest.mark.gpu
def test_llff_training_with_six_xyz_frequencies_takes_the_fused_ndc_step(dev, tmp_path, monkeypatch):
    """train_dexnerf.py --llff --xyz-freqs 6 on a small forward-facing capture of the built-in teacher scene: the iteration is
    nerf.FusedTrainStep on NDC rows (dn_select_rays_draw_ndc) and the student learns (+6 dB)."""
    import nerf
    import train_dexnerf
    from PIL import Image
    from nerf import synthetic as syn
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "images"))
    h = w = 48
    f = 60.0
    teacher = []
    for seed, bias in ((42, -150.0), (43, -20.0)):
        mdl = nerf.models.FlexibleNeRFModel(**FERN_KW)
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **FERN_KW).items()})
        teacher.append(mdl.to(dev))
    mode = dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(6), nerf.get_embedding_function(4)
    rows = []
    k = 0
    for y in (-0.5, 0.0, 0.5):
        for x in (-0.6, -0.2, 0.2, 0.6):
            c2w = np.eye(4, dtype=np.float32)
            c2w[:3, 3] = [x, y, 4.0]
            ro, rd = nerf.get_ray_bundle(h, w, f, torch.from_numpy(c2w).to(dev))
            with torch.no_grad():
                out = nerf.run_one_iter_of_nerf(h, w, f, teacher[0], teacher[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                encode_direction_fn=ed)
            img = (C(out[3]).clip(0, 1) * 255 + 0.5).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "images", f"{k:02d}.png"))
            block = np.stack([-c2w[:3, 1], c2w[:3, 0], c2w[:3, 2], c2w[:3, 3], np.array([h, w, f], dtype=np.float32)], axis=1)
            rows.append(np.concatenate([block.reshape(-1), [2.0, 6.0]]))
            k += 1
    np.save(os.path.join(root, "poses_bounds.npy"), np.stack(rows).astype(np.float64))
    built = []
    orig_init = nerf.FusedTrainStep.__init__

    def spy(self, *a, **kw):
        built.append(kw.get("ndc_focal"))
        orig_init(self, *a, **kw)
    monkeypatch.setattr(nerf.FusedTrainStep, "__init__", spy)
    try:
        with no_fallback(monkeypatch):
            res = train_dexnerf.main(["--llff", root, "--llff-factor", "1", "--llffhold", "6", "--iters", "300", "--num-random-rays", "512",
                                      "--layers", "4", "--width", "128", "--num-fine", "64", "--validate-every", "0", "--quiet",
                                      "--precision", "bf16", "--xyz-freqs", "6"])
    finally:
        nerf.set_precision("fp32")
    assert built == [f]
    first, last = res["history"][0], res["history"][-1]
    assert np.isfinite(last[1]) and last[2] - first[2] > 6.0, (first, last)
    assert res["val_psnr"] > 12.0
