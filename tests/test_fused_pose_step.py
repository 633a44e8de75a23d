"""The pose-refinement iteration as library launches only: camera records from twists on the device (dn_pose_records and its
backward), the render with its ray gradient (dn_render_rays_train_geom / dn_render_rays_backward_geom), the _ops wrappers and
nerf.FusedPoseStep (eager and replayed as one HIP graph).

Yardsticks: a float64 restatement of the records in this file (nerf.se3_exp, torch.inverse, autograd) at 1e-6 - the kernels compute in
fp64 and round once to fp32 (2^-24), the figure test_pose_refinement uses for extrinsic(); the stage-by-stage autograd route of
predict_and_render_radiance on the same draws at 1e-5 - the same kernels on the same bits, only the order in which the contributions
are added differs, the figure of test_batched_pose_gradient_equals_the_one_camera_chain_per_view; dn_render_rays_train /
dn_render_rays_backward_ws bit for bit.  Tolerances in the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES, D4
from test_camera_gradients import NDC_F, NDC_H, NDC_W
from test_input_gradients import make_cfg, make_models, no_fallback
from test_mixed_view_batches import POSES, V, ndc_cameras

NEW_SYMBOLS = ("dn_pose_records", "dn_pose_records_backward", "dn_render_rays_train_geom", "dn_render_backward_geom_workspace_bytes",
               "dn_render_rays_backward_geom")
GEOM_N = (1, 64, 65, 257)
# (perturb, noise_std, white_background, lindisp)
GEOM_CASES = {"a": (False, 0.0, False, False), "b": (True, 0.2, True, False), "c": (True, 0.0, False, True)}


def C(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


def d4_desc():
    from nerf import _hip
    return _hip.MlpDesc(**{k: int(v) for k, v in dict(D4, include_input_xyz=1, include_input_dir=1, log_sampling_xyz=1, log_sampling_dir=1).items()})


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_resolvable(hiplib):
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(raw, name), name
        assert getattr(hiplib, name).argtypes is not None, name
    assert hiplib.dn_abi_version() == 2 and "#define DN_ABI_VERSION 2" in header


def test_pose_entry_points_validate_before_gpu_work(hiplib):
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def rec(xi=fake, e0=fake, k=fake, per_view=0, focal=0.0, nv=3, cams=fake, extr=None):
        return hiplib.dn_pose_records(xi, e0, k, per_view, focal, nv, cams, extr, None)
    for kw in (dict(xi=None), dict(e0=None), dict(k=None), dict(cams=None), dict(nv=-1), dict(xi=odd), dict(cams=odd), dict(extr=odd),
               dict(focal=-1.0), dict(focal=float("nan")), dict(focal=float("inf")), dict(nv=0, cams=None)):
        assert rec(**kw) == -1000, kw
        assert b"dn_pose_records" in hiplib.dn_last_error(), kw
    assert rec(nv=0) == 0

    def bwd(g=fake, xi=fake, e0=fake, nv=3, out=fake, keep=None):
        return hiplib.dn_pose_records_backward(g, xi, e0, nv, out, keep, None)
    for kw in (dict(g=None), dict(xi=None), dict(e0=None), dict(out=None), dict(nv=-2), dict(g=odd), dict(out=odd), dict(keep=odd),
               dict(nv=0, out=None)):
        assert bwd(**kw) == -1000, kw
        assert b"dn_pose_records_backward" in hiplib.dn_last_error(), kw
    assert bwd(nv=0) == 0 and bwd(nv=0, keep=fake) == 0


def test_geom_render_entry_points_validate_before_gpu_work(hiplib):
    from nerf import _hip
    desc = d4_desc()
    d = ctypes.byref(desc)
    fake, odd = ctypes.c_void_p(1024), ctypes.c_void_p(1024 + 64)
    big = 1 << 40

    def fwd(dc=d, pc=fake, df=d, pf=fake, prec=0, rays=fake, stride=11, n=4, nc=64, nf=64, ws=fake, act_c=fake, masks_c=fake, act_f=fake,
            masks_f=fake, zs=fake):
        return hiplib.dn_render_rays_train_geom(dc, pc, df, pf, prec, rays, stride, n, nc, nf, 0, 0.0, 0, None, 0, None, None, None, None,
                                                fake, fake, fake, fake, fake, fake, None, ws, act_c, masks_c, act_f, masks_f, None, 0, zs, None)
    for kw in (dict(dc=None), dict(pc=None), dict(rays=None), dict(ws=None), dict(act_c=None), dict(masks_c=None), dict(df=None), dict(pf=None),
               dict(act_f=None), dict(masks_f=None), dict(ws=odd), dict(n=-1), dict(n=0, rays=None), dict(n=0, ws=odd)):
        assert fwd(**kw) == -1000, kw
        assert b"dn_render_rays_train" in hiplib.dn_last_error(), kw
    assert fwd(n=0) == 0 and fwd(n=0, zs=None) == 0

    def bwd(dc=d, bc=fake, ic=fake, df=d, bf=fake, igf=fake, prec=0, rays=fake, stride=11, n=4, nc=64, nf=64, zs=fake, ws=fake, masks_c=fake,
            grads_c=fake, masks_f=fake, grads_f=fake, dw_c=None, db_c=None, dw_f=None, db_f=None, act_c=None, act_f=None, wg=None, wg_bytes=0,
            gws=fake, gws_bytes=big, d_rays=fake):
        return hiplib.dn_render_rays_backward_geom(dc, bc, ic, df, bf, igf, prec, rays, stride, n, nc, nf, 0, 0, 0.0, 0, None, None, None, zs,
                                                   fake, None, None, fake, None, None, ws, act_c, masks_c, grads_c, act_f, masks_f, grads_f,
                                                   dw_c, db_c, dw_f, db_f, None, wg, wg_bytes, gws, gws_bytes, d_rays, None)
    arr = (ctypes.c_void_p * 16)()
    need = hiplib.dn_render_backward_geom_workspace_bytes(d, d, 4, 11, 64, 64)
    for kw in (dict(dc=None), dict(bc=None), dict(ic=None), dict(rays=None), dict(ws=None), dict(masks_c=None), dict(grads_c=None),
               dict(d_rays=None), dict(gws=None), dict(df=None), dict(bf=None), dict(igf=None), dict(masks_f=None), dict(grads_f=None),
               dict(zs=None), dict(ws=odd), dict(gws=odd), dict(n=-1), dict(nc=0), dict(nf=-1), dict(stride=7), dict(wg_bytes=64),
               dict(dw_c=arr), dict(dw_c=arr, db_c=arr), dict(dw_c=arr, db_c=arr, dw_f=arr, db_f=arr), dict(gws_bytes=need - 1),
               dict(prec=7), dict(n=0, d_rays=None), dict(n=0, gws=odd)):
        assert bwd(**kw) == -1000, kw
        assert b"dn_render_rays_backward_geom" in hiplib.dn_last_error(), kw
    assert bwd(gws_bytes=need - 1) == -1000 and b"geom_workspace" in hiplib.dn_last_error()
    assert bwd(n=0) == 0 and bwd(n=0, nf=0, df=None, bf=None, igf=None, zs=None) == 0
    for prec in (_hip.PREC_BF16_S8, _hip.PREC_F16):
        assert bwd(prec=prec) == -1001 and bwd(prec=prec, n=0) == -1001
        assert b"dn_render_rays_backward_geom" in hiplib.dn_last_error()


def test_geom_workspace_query(hiplib):
    d = ctypes.byref(d4_desc())
    q = hiplib.dn_render_backward_geom_workspace_bytes
    assert q(None, d, 4, 11, 64, 64) == 0 and q(d, None, 4, 11, 64, 64) == 0 and q(d, d, -1, 11, 64, 64) == 0
    assert q(d, d, 4, 7, 64, 64) == 0 and q(d, d, 4, 11, 0, 64) == 0 and q(d, d, 4, 11, 64, -1) == 0
    ns = (0, 1, 64, 65, 257, 2048, 4096)
    for nf, df in ((64, d), (0, None)):
        sizes = [q(d, df, n, 11, 64, nf) for n in ns]
        assert sizes == sorted(sizes) and sizes[1] > 0 and sizes[-1] > sizes[1] and all(s % 256 == 0 for s in sizes), sizes
        assert sizes == [q(d, df, n, 11, 64, nf) for n in ns]
    assert q(d, d, 257, 11, 64, 64) > q(d, None, 257, 11, 64, 0)


def test_fused_pose_step_refuses_host_tensors_and_mismatched_views():
    import nerf
    from nerf import synthetic as syn
    h, w = 8, 10
    e = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES])
    k = torch.from_numpy(syn.intrinsic(h, w))
    images = torch.zeros(V, h, w, 3)

    def make(e=e, k=k, images=images):
        return nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        make()
    with pytest.raises(ValueError, match="intrinsics"):
        make(k=torch.stack([k, k]))
    with pytest.raises(ValueError, match="images"):
        make(images=images[:2])
    with pytest.raises(ValueError, match="images"):
        make(images=images[0])
    with pytest.raises(ValueError, match=r"\(V,4,4\)"):
        make(e=e[:, :3])


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
    nerf.set_render_policy("bf16")
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


@pytest.fixture(scope="module")
def lego(dev):
    """(coarse, fine) lego-shaped 4 x 128 networks, parameters frozen, and the two encoders."""
    import nerf
    mkw, wfn, _ = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    return mc, mf, nerf.get_embedding_function(10), nerf.get_embedding_function(4)


def pose_inputs():
    """xi (5,6) with |omega| in {0, 1e-8, 1e-4, 0.3, 3.0} and non-zero translations, e0 (5,4,4), k (5,3,3), g_cams (5,16), all fp32."""
    from nerf import synthetic as syn
    gen = torch.Generator().manual_seed(11)
    axes = torch.nn.functional.normalize(torch.randn(5, 3, generator=gen, dtype=torch.float64), dim=1)
    omega = axes * torch.tensor([0.0, 1e-8, 1e-4, 0.3, 3.0], dtype=torch.float64)[:, None]
    trans = torch.randn(5, 3, generator=gen, dtype=torch.float64) * 0.4 + 0.1
    xi = torch.cat([omega, trans], dim=1).float()
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in (3, 9, 14, 5, 20)]).float()
    k = torch.stack([torch.from_numpy(syn.intrinsic(40, 52)).clone() for _ in range(5)])
    for v in range(5):
        k[v, 0, 0] += 0.5 * v
        k[v, 0, 2] += 0.25 * v
        k[v, 1, 2] -= 0.125 * v
    g_cams = torch.randn(5, 16, generator=gen)
    return xi, e0, k, g_cams


def records64(xi, e0):
    """float64 restatement: (cams[:, :12] (V,12), extrinsics (V,4,4)) of E = se3_exp(xi) @ e0, differentiable in xi."""
    import nerf
    recs, es = [], []
    for v in range(xi.shape[0]):
        e = nerf.se3_exp(xi[v]) @ e0[v]
        rinv = torch.inverse(e[:3, :3])
        recs.append(torch.cat([rinv.reshape(-1), torch.inverse(e)[:3, 3]]))
        es.append(e)
    return torch.stack(recs), torch.stack(es)


@pytest.mark.gpu
def test_pose_records_and_their_backward_against_float64(dev):
    from nerf import _ops
    xi, e0, k, g_cams = pose_inputs()
    norms = xi[:, :3].double().norm(dim=1).tolist()
    assert norms[0] == 0.0 and all(abs(a - b) <= 1e-6 * b for a, b in zip(norms[1:], (1e-8, 1e-4, 0.3, 3.0))) and bool((xi[:, 3:] != 0).all())
    g_cams[2] = 0.0
    g_cams[2, 12:] = torch.tensor([0.3, -0.2, 0.1, 0.7])       # slots 12:16 are ignored: this row still counts as zero
    xi_d, e0_d, k_d, g_d = xi.to(dev), e0.to(dev), k.to(dev), g_cams.to(dev)
    cams, extr = _ops.pose_records(xi_d, e0_d, k_d, ndc_focal=NDC_F, want_extrinsics=True)
    g_xi = _ops.pose_records_backward(g_d, xi_d, e0_d)
    xi64 = xi.double().requires_grad_(True)
    want, want_e = records64(xi64, e0.double())
    (want * g_cams[:, :12].double()).sum().backward()
    errs = dict(rinv=rel_err(C(cams[:, :9]), want[:, :9].detach().numpy()), origin=rel_err(C(cams[:, 9:12]), want[:, 9:12].detach().numpy()),
                extrinsics=rel_err(C(extr), want_e.detach().numpy()), g_xi=rel_err(C(g_xi), xi64.grad.numpy()))
    per_view = [rel_err(C(g_xi[v]), xi64.grad[v].numpy()) for v in (0, 1, 3, 4)]
    print("pose records vs float64:", {n: f"{e:.2e}" for n, e in errs.items()}, "g_xi per view", [f"{e:.2e}" for e in per_view])
    assert bool(torch.isfinite(cams).all()) and bool(torch.isfinite(g_xi).all())
    assert all(e <= 1e-6 for e in errs.values()), errs
    assert all(e <= 1e-6 for e in per_view), per_view
    assert torch.equal(cams[:, 12:].cpu(), torch.stack([k[:, 0, 0], k[:, 0, 2], k[:, 1, 2], torch.full((5,), NDC_F)], dim=1))
    assert torch.equal(extr[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(5, 4))
    assert bool((g_xi[2] == 0).all()) and float(g_xi[[0, 1, 3, 4]].abs().amin(dim=1).max()) > 0
    # two calls: the same bits; the second output of the backward: the same values; buffers given by the caller are the ones written
    cams2, extr2 = _ops.pose_records(xi_d, e0_d, k_d, ndc_focal=NDC_F, want_extrinsics=True)
    keep = torch.full((5, 6), float("nan"), device=dev)
    g_xi2 = _ops.pose_records_backward(g_d, xi_d, e0_d, keep=keep)
    assert torch.equal(cams, cams2) and torch.equal(extr, extr2) and torch.equal(g_xi, g_xi2) and torch.equal(g_xi, keep)
    # one shared (3,3) intrinsic = the same matrix per view; no NDC focal: slot 15 is 0
    shared = _ops.pose_records(xi_d, e0_d, k_d[1].contiguous())
    per_view_k = _ops.pose_records(xi_d, e0_d, k_d[1][None].expand(5, 3, 3).contiguous())
    assert shared.shape == (5, 16) and torch.equal(shared, per_view_k) and torch.equal(shared[:, :12], cams[:, :12])
    assert bool((shared[:, 15] == 0).all()) and torch.equal(shared[:, 12:15].cpu(), torch.stack([k[1, 0, 0], k[1, 0, 2], k[1, 1, 2]]).expand(5, 3))


def geom_rows(n, dev, seed=0):
    """n ray rows (n,11) of the synthetic scene (pose 9, 400 x 400, near 2 / far 6): the centre pixel, then pixels drawn from a seeded
    host generator."""
    import nerf
    from nerf import synthetic as syn
    pix = torch.randint(0, 400 * 400, (n,), generator=torch.Generator().manual_seed(100 + seed + n))
    pix[0] = 200 * 400 + 200          # the image centre first: a lone ray should look at the object
    pix = pix.to(dev)
    rows, _ = nerf.select_camera_rays(400, 400, torch.from_numpy(syn.scene_pose(9)).to(dev), torch.from_numpy(syn.intrinsic(400, 400)).to(dev),
                                      2.0, 6.0, pix)
    return rows


def fused_packs(lego):
    """The two packed networks as FusedPoseStep uses them: core stream, backward stream, input-gradient stream."""
    from nerf import _hip, _ops
    mc, mf, ex, ed = lego
    packs = []
    for m in (mc, mf):
        pk = m.packed(ex.log_sampling, ed.log_sampling, parts=_hip.PACK_CORE)
        _ops.ensure_backward_stream(m, pk, pk.precision)
        _ops.ensure_input_grad_stream(m, pk)
        packs.append(pk)
    return packs


def geom_forward(lego, rows, case, nf, state):
    from nerf import _ops
    perturb, std, white, lindisp = GEOM_CASES[case]
    pc, pf = fused_packs(lego)
    if nf == 0:
        pf = None
    maps, saved = _ops.render_rays_train_geom(pc, pf, rows, 64, nf, lindisp, std, white, [], None, prec=pc.precision, rng_state=state,
                                              perturb=perturb)
    return pc, pf, maps, saved


def draw_queues(state, n, nf, case):
    """The in-kernel draws of the iteration as the tensors torch.rand / torch.randn hand the stage-by-stage route, in its call order."""
    from nerf import _ops
    perturb, std, _, _ = GEOM_CASES[case]
    q_rand, q_randn = [], []
    if perturb:
        q_rand.append(_ops.rng_fill(state, 0, (n, 64)))
        if nf:
            q_rand.append(_ops.rng_fill(state, 2, (n, nf)))
    if std > 0.0:
        q_randn.append(_ops.rng_fill(state, 1, (n, 64), normal=True))
        if nf:
            q_randn.append(_ops.rng_fill(state, 3, (n, 64 + nf), normal=True))
    return q_rand, q_randn


def workspace_regions(ws, n, nc, nf):
    """The saved tensors of dn_render_rays_train's workspace (csrc/api.cpp carve): z_c, rf_c, w_c, z_f, rf_f as flat fp32 views."""
    out, off = [], 0
    for count in (n * nc, n * nc * 4, n * nc) + ((n * (nc + nf), n * (nc + nf) * 4) if nf else ()):
        out.append(ws[off:off + 4 * count].view(torch.float32))
        off += (4 * count + 255) // 256 * 256
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GEOM_CASES))
def test_train_geom_forward_equals_the_training_forward_and_returns_the_resamples(dev, lego, case):
    from nerf import _ops
    n, nc, nf = 257, 64, 64
    perturb, std, white, lindisp = GEOM_CASES[case]
    rows = geom_rows(n, dev)
    state = _ops.new_rng_state(5, dev, 3)
    pc, pf, maps, saved = geom_forward(lego, rows, case, nf, state)
    maps0, saved0 = _ops.render_rays_train(pc, pf, rows, nc, nf, lindisp, std, white, [], None, prec=pc.precision, rng_state=state, perturb=perturb)
    for a, b in zip(maps[:6], maps0[:6]):
        assert torch.equal(a, b)
    regions, regions0 = workspace_regions(saved["ws"], n, nc, nf), workspace_regions(saved0["ws"], n, nc, nf)
    assert len(regions) == 5 and all(torch.equal(a, b) for a, b in zip(regions, regions0))
    z_c, w_c, z_f = regions[0].view(n, nc), regions[2].view(n, nc), regions[3].view(n, nc + nf)
    u = _ops.rng_fill(state, 2, (n, nf)) if perturb else None
    z_fine, z_samples = _ops.fine_depths(z_c, w_c, nf, u, want_samples=True)
    assert torch.equal(z_fine, z_f) and torch.equal(saved["z_samples"], z_samples) and saved["z_samples"].shape == (n, nf)


def stagewise_reference(lego, rows, cfg, queues, g_c, g_f, monkeypatch):
    """predict_and_render_radiance with rows that require grad (the stage-by-stage autograd route, no fallback), on the given draws and
    upstream gradients: (maps, rows.grad)."""
    import nerf
    mc, mf, ex, ed = lego
    q_rand, q_randn = queues
    ref = rows.clone().requires_grad_(True)
    with no_fallback(monkeypatch), monkeypatch.context() as mp:
        mp.setattr(torch, "rand", lambda *a, **k: q_rand.pop(0))
        mp.setattr(torch, "randn", lambda *a, **k: q_randn.pop(0))
        out = nerf.predict_and_render_radiance(ref, mc, mf if g_f is not None else None, cfg, mode="train", encode_position_fn=ex,
                                               encode_direction_fn=ed)
    assert not q_rand and not q_randn
    if g_f is None:
        out[0].backward(g_c)
    else:
        torch.autograd.backward([out[0], out[3]], [g_c, g_f])
    return out, ref.grad


def check_d_rays(d_rays, want, what):
    groups = {"origin 0:3": slice(0, 3), "direction 3:6": slice(3, 6), "near/far 6:8": slice(6, 8), "viewdir 8:11": slice(8, 11)}
    errs = {name: rel_err(C(d_rays[:, sl]), C(want[:, sl])) for name, sl in groups.items()}
    print(f"d_rays vs the stage-by-stage route, {what}:", {k: f"{e:.2e}" for k, e in errs.items()},
          "max|want| per group", [f"{float(want[:, sl].abs().max()):.2e}" for sl in groups.values()])
    if want.shape[0] > 1:    # (a lone ray may see nothing under a white background: its gradient is 0 on both routes)
        assert all(float(want[:, sl].abs().max()) > 0 for sl in groups.values())
    assert all(e <= 1e-5 for e in errs.values()), (what, errs)


def run_d_rays_case(dev, lego, monkeypatch, n, nf, case):
    from nerf import _ops
    perturb, std, white, lindisp = GEOM_CASES[case]
    rows = geom_rows(n, dev)
    state = _ops.new_rng_state(9, dev, 2)
    pc, pf, maps, saved = geom_forward(lego, rows, case, nf, state)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(n)).to(dev)
    _, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target)
    d_rays, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, None, None))
    again, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, None, None))
    assert d_rays.shape == rows.shape and torch.equal(d_rays, again) and bool(torch.isfinite(d_rays).all())
    cfg = make_cfg(dict(num_coarse=64, num_fine=nf, near=2.0, far=6.0, perturb=perturb, noise_std=std, white_background=white, lindisp=lindisp))
    out, want = stagewise_reference(lego, rows, cfg, draw_queues(state, n, nf, case), g_c, g_f, monkeypatch)
    for a, b in zip(maps[:6], out[:6]):
        assert (a is None and b is None) or torch.equal(a, b.detach())
    check_d_rays(d_rays, want, f"n={n} nf={nf} case {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GEOM_CASES))
@pytest.mark.parametrize("n", GEOM_N)
def test_ray_gradient_equals_the_stage_by_stage_autograd_route(dev, lego, monkeypatch, n, case):
    """64 + 64 samples: the coarse pass is one 64-sample compositing chunk, the fine pass two (the geometry backward's carry across
    chunks); N spans the wave and the 256-thread workgroup edges."""
    run_d_rays_case(dev, lego, monkeypatch, n, 64, case)


@pytest.mark.gpu
def test_ray_gradient_of_a_coarse_only_render(dev, lego, monkeypatch):
    run_d_rays_case(dev, lego, monkeypatch, 65, 0, "b")


@pytest.mark.gpu
def test_ray_gradient_in_bf16_with_16_bit_saves(dev, lego, monkeypatch):
    import nerf
    nerf.set_precision("bf16-s16")
    run_d_rays_case(dev, lego, monkeypatch, 257, 64, "b")


@pytest.mark.gpu
def test_weight_gradients_pass_through_the_geometry_backward(dev, lego):
    """With h_dW / h_db given: the weight gradients of dn_render_rays_backward_ws (nets = 3, deterministic scratch) on the same saved
    forward, bit for bit, and the d_rays of the frozen call, bit for bit."""
    from nerf import _ops
    mc, mf = lego[0], lego[1]
    n = 257
    rows = geom_rows(n, dev)
    state = _ops.new_rng_state(9, dev, 2)
    pc, pf, maps, saved = geom_forward(lego, rows, "b", 64, state)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(n)).to(dev)
    _, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target)
    frozen, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, None, None))
    shapes_c = [tuple(m.weight.shape) for m in mc.linear_modules()]
    shapes_f = [tuple(m.weight.shape) for m in mf.linear_modules()]
    views_c, views_f = _ops.zeroed_grad_views(shapes_c, dev), _ops.zeroed_grad_views(shapes_f, dev)
    d_rays, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, None, None), views_c, views_f)
    want_c, want_f = _ops.zeroed_grad_views(shapes_c, dev), _ops.zeroed_grad_views(shapes_f, dev)
    _ops.render_rays_backward(pc, pf, saved, (g_c, None, None), (g_f, None, None), want_c, want_f, nets=3)
    assert torch.equal(d_rays, frozen)
    for got, want in ((views_c, want_c), (views_f, want_f)):
        for (gw, gb), (ww, wb) in zip(got, want):
            assert float(ww.abs().max()) > 0 and torch.equal(gw, ww) and torch.equal(gb, wb)


# ---- the step -------------------------------------------------------------------------------------------------------------------------
STEP_CFG = dict(num_coarse=64, num_fine=64, perturb=True, noise_std=0.2, white_background=True)
XI_START = ((0.01, -0.02, 0.015, 0.03, -0.01, 0.02), (-0.02, 0.01, 0.005, -0.01, 0.02, 0.015), (0.005, 0.015, -0.01, 0.02, 0.01, -0.03))


def world_problem(dev):
    from nerf import synthetic as syn
    h, w = 40, 52
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES]).to(dev)
    k = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
    images = torch.rand(V, h, w, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    return h, w, e0, k, images, make_cfg(dict(STEP_CFG, near=2.0, far=6.0)), None


def ndc_problem(dev):
    e0, k = ndc_cameras()
    images = torch.rand(V, NDC_H, NDC_W, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    return NDC_H, NDC_W, e0.to(dev), k.to(dev), images, make_cfg(dict(STEP_CFG, near=0.0, far=1.0)), NDC_F


def make_step(lego, problem, num_rays, seed, **kw):
    import nerf
    mc, mf, ex, ed = lego
    h, w, e0, k, images, cfg, focal = problem
    return nerf.FusedPoseStep(mc, mf, cfg, h, w, k, e0, images, ex, ed, num_rays=num_rays, lr=1e-3, seed=seed, ndc_focal=focal, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,num_rays", [("world", 96), ("world", 2), ("ndc", 96)])
def test_one_step_is_the_chain_of_its_pieces(dev, lego, monkeypatch, scene, num_rays):
    """One eager step from a non-zero xi against the chain built from the pieces pinned above and in the existing suites, on the step's
    own drawn pairs: records, rows and targets (bit for bit), the stage-by-stage render under autograd, dn_camera_grad_views,
    dn_pose_records_backward; then torch.optim.Adam on that gradient; the RNG counter advances by one.  num_rays = 2 over three views:
    at least one view has no ray - zero gradient, xi unchanged."""
    import nerf
    from nerf import _ops
    problem = world_problem(dev) if scene == "world" else ndc_problem(dev)
    h, w, e0, k, images, cfg, focal = problem
    step = make_step(lego, problem, num_rays, seed=21, first_iteration=4, use_graphs=False)
    assert step.xi.shape == (V, 6) and step.xi.dtype == torch.float32 and step.xi.is_cuda and float(step.xi.abs().max()) == 0
    step.xi.copy_(torch.tensor(XI_START))
    xi0 = step.xi.clone()
    peek = _ops.new_rng_state(21, dev, 4)
    loss3 = step.step()
    assert loss3 is step.loss3 and step.rng_state.tolist()[2:] == [4, 5] and step.graph is None
    views, pix, rows, target = step.latest_draw()
    n = num_rays
    assert views.dtype == torch.int32 and pix.dtype == torch.int64 and rows.shape == (n, 11) and target.shape == (n, 3)
    assert (views.long() * (h * w) + pix).unique().numel() == n
    cams = _ops.pose_records(xi0, e0, k, focal)
    rows2, target2 = _ops.select_rays_views(h, w, cams, views, cfg.dataset.near, cfg.dataset.far, pix, images, ndc_focal=focal, ndc_near=1.0)
    assert torch.equal(rows2, rows) and torch.equal(target2, target)
    mc, mf, ex, ed = lego
    q_rand = [_ops.rng_fill(peek, 0, (n, 64)), _ops.rng_fill(peek, 2, (n, 64))]
    q_randn = [_ops.rng_fill(peek, 1, (n, 64), normal=True), _ops.rng_fill(peek, 3, (n, 128), normal=True)]
    ref = rows.clone().requires_grad_(True)
    with no_fallback(monkeypatch), monkeypatch.context() as mp:
        mp.setattr(torch, "rand", lambda *a, **kw: q_rand.pop(0))
        mp.setattr(torch, "randn", lambda *a, **kw: q_randn.pop(0))
        out = nerf.predict_and_render_radiance(ref, mc, mf, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
    assert not q_rand and not q_randn
    mse_c, mse_f = nerf.img2mse(out[0], target), nerf.img2mse(out[3], target)
    (mse_c + mse_f).backward()
    g = ref.grad
    g_cams = _ops.camera_grad_views(h, w, cams, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal or 0.0, 1.0)
    want = _ops.pose_records_backward(g_cams, xi0, e0)
    err = rel_err(C(step.last_grad), C(want))
    got = loss3.tolist()
    losses = [(mse_c + mse_f).item(), mse_c.item(), mse_f.item()]
    print(f"{scene} {n} rays: last_grad vs the chain {err:.2e}; loss3 {got} vs {losses}; rays per view {torch.bincount(views, minlength=V).tolist()}")
    assert float(want.abs().max()) > 0 and err <= 1e-5, err
    assert all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(got, losses)), (got, losses)
    param = xi0.clone().requires_grad_(True)
    param.grad = step.last_grad.clone()
    torch.optim.Adam([param], lr=1e-3).step()
    assert rel_err(C(step.xi), C(param)) <= 1e-6
    empty = torch.bincount(views, minlength=V) == 0
    if n < V:
        assert bool(empty.any())
    assert bool((step.last_grad[empty] == 0).all()) and torch.equal(step.xi[empty], xi0[empty])
    assert bool((step.xi[~empty] != xi0[~empty]).any(dim=1).all())
    est = step.extrinsics()
    want_e = torch.stack([nerf.se3_exp(step.xi[v].double().cpu()) @ e0[v].double().cpu() for v in range(V)])
    assert est.shape == (V, 4, 4) and est.is_cuda and rel_err(C(est), want_e.numpy()) <= 1e-6


@pytest.mark.gpu
def test_replayed_steps_equal_eager_steps_and_leave_the_networks_alone(dev, lego):
    from nerf import _ops
    mc, mf = lego[0], lego[1]
    problem = world_problem(dev)
    h, w, e0, k, images, cfg, _ = problem
    params = list(mc.parameters()) + list(mf.parameters())
    before = [p.detach().clone() for p in params]
    flags = [i % 2 == 0 for i in range(len(params))]
    for p, flag in zip(params, flags):
        p.requires_grad_(flag)
    import nerf
    with pytest.raises(ValueError, match="fused training kernels"):      # no network / no Embedder: the documented error, not an AttributeError
        nerf.FusedPoseStep(None, None, cfg, h, w, k, e0, images, None, None, num_rays=4, lr=1e-3)
    with pytest.raises(ValueError, match="fused training kernels"):
        nerf.FusedPoseStep(mc, mf, cfg, h, w, k, e0, images, lambda x: x, lambda x: x, num_rays=4, lr=1e-3)
    try:
        eager = make_step(lego, problem, 96, seed=8, use_graphs=False)
        graphed = make_step(lego, problem, 96, seed=8, eager_iterations=1)
        other = make_step(lego, problem, 96, seed=9, use_graphs=False)
        for it in range(4):
            eager.step(); graphed.step(); other.step()
            assert (graphed.graph is not None) == (it >= 1)
        torch.cuda.synchronize()
        assert graphed.graph is not None and graphed.fallback_reason is None, graphed.fallback_reason
        assert eager.graph is None and eager.fallback_reason is None
        assert torch.equal(eager.xi, graphed.xi) and torch.equal(eager.last_grad, graphed.last_grad) and torch.equal(eager.loss3, graphed.loss3)
        assert bool(torch.isfinite(eager.xi).all()) and bool((eager.xi.abs().amax(dim=1) > 0).all()) and not torch.equal(eager.xi, other.xi)
        assert eager.rng_state.tolist()[2:] == [3, 4] and graphed.rng_state.tolist()[2:] == [3, 4]
        # a replayed step draws exactly what an eager draw of that iteration would
        peek = _ops.new_rng_state(8, dev, 4)
        cams = _ops.pose_records(graphed.xi.clone(), e0, k)
        rows_next, target_next = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, peek, 96, images)
        graphed.step()
        torch.cuda.synchronize()
        rows = graphed.latest_draw()[2]
        assert torch.equal(rows, rows_next) and torch.equal(graphed.latest_draw()[3], target_next)
        # a step inside the caller's own capture raises nothing
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            eager.step()
        assert [p.requires_grad for p in params] == flags and all(p.grad is None for p in params)
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    finally:
        for p in params:
            p.requires_grad_(False)
