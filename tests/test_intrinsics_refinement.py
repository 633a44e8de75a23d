"""Camera intrinsics refined with the poses on the fused device step: dn_camera_records and its backward (records with slots 12:15 from
phi, the pose mask, the shared gradient summed in view order), the _ops wrappers, nerf.FusedPoseStep(refine_intrinsics=, fixed_views=,
refine_pose=) eager and replayed, and nerf.MultiPoseRefiner as the host-side parity reference.

The parameterisation (one definition; csrc/pose.hip's header comment): fx = fx0 exp(s a), cx = cx0 + s fx0 b, cy = cy0 + s fx0 c.

Yardsticks: a float64 restatement in this file (nerf.se3_exp, torch.inverse, the three formulas, autograd) at 1e-6 - the kernels compute
in fp64 and round once, the gate of test_pose_records_and_their_backward_against_float64; dn_pose_records / dn_pose_records_backward bit
for bit at phi = 0; the stage-by-stage chain at 1e-5 (test_one_step_is_the_chain_of_its_pieces' gate: the same kernels, only the order of
the last additions differs); against MultiPoseRefiner, the xi discrepancy of the same two objects in the same run (see the last test).
Tolerances in the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from test_camera_gradients import NDC_F
from test_fused_pose_step import STEP_CFG, XI_START, C, _restore_modes, dev, hiplib, lego, make_step, ndc_problem, pose_inputs, records64, world_problem  # noqa: F401
from test_input_gradients import make_cfg, no_fallback
from test_mixed_view_batches import POSES, V

NEW_SYMBOLS = ("dn_camera_records", "dn_camera_records_scratch_bytes", "dn_camera_records_backward")
MODES = ("shared", "per_view")
PHI_START = {"shared": (0.02, -0.01, 0.015), "per_view": ((0.02, -0.01, 0.015), (-0.03, 0.02, -0.005), (0.01, 0.025, -0.02))}


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_resolvable(hiplib):
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(raw, name), name
        assert getattr(hiplib, name).argtypes is not None, name
    assert len(_hip.EXPORTS) == len(set(_hip.EXPORTS)) == 76
    assert hiplib.dn_abi_version() == 2 and "#define DN_ABI_VERSION 2" in header


def test_camera_entry_points_validate_before_gpu_work(hiplib):
    """Fake pointers: every call below must be judged before any GPU work (none of the accepted ones launches: n_views == 0 without a
    shared g_phi)."""
    fake, odd, odd8 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(260)
    bad_scales = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))

    def rec(xi=fake, phi=fake, pv=0, s=1.0, e0=fake, k=fake, kpv=0, focal=0.0, nv=3, cams=fake, extr=None):
        return hiplib.dn_camera_records(xi, phi, pv, s, e0, k, kpv, focal, nv, cams, extr, None)
    cases = [dict(xi=None), dict(e0=None), dict(k=None), dict(cams=None), dict(nv=-1), dict(xi=odd), dict(phi=odd), dict(e0=odd), dict(k=odd),
             dict(cams=odd), dict(extr=odd), dict(focal=-1.0), dict(focal=float("nan")), dict(focal=float("inf")), dict(nv=0, cams=None),
             dict(nv=0, s=0.0), dict(phi=None, s=-2.0)] + [dict(s=s) for s in bad_scales]
    for kw in cases:
        assert rec(**kw) == -1000, kw
        assert b"dn_camera_records:" in hiplib.dn_last_error(), kw
    assert rec(nv=0) == 0 and rec(nv=0, phi=None, pv=1, kpv=1, extr=fake) == 0

    q = hiplib.dn_camera_records_scratch_bytes
    sizes = [q(n) for n in (0, 1, 5, 64, 65, 1000)]
    assert q(-1) == 0 and sizes[0] == 0 and sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)
    assert all(s >= 24 * n for s, n in zip(sizes, (0, 1, 5, 64, 65, 1000)))
    need = q(3)

    def bwd(g=fake, xi=fake, phi=fake, pv=0, s=1.0, e0=fake, k=fake, kpv=0, mask=None, nv=3, out=fake, keep=None, gphi=fake, gkeep=None,
            scratch=fake, nbytes=need):
        return hiplib.dn_camera_records_backward(g, xi, phi, pv, s, e0, k, kpv, mask, nv, out, keep, gphi, gkeep, scratch, nbytes, None)
    cases = [dict(g=None), dict(xi=None), dict(e0=None), dict(k=None), dict(out=None), dict(nv=-2), dict(g=odd), dict(xi=odd), dict(phi=odd),
             dict(e0=odd), dict(k=odd), dict(mask=odd), dict(out=odd), dict(keep=odd), dict(gphi=odd), dict(gkeep=odd),
             dict(gphi=None, gkeep=fake), dict(nv=0, out=None), dict(nv=0, s=0.0), dict(pv=1, gphi=None, s=-1.0),
             dict(nbytes=need - 1), dict(nbytes=0), dict(scratch=None), dict(scratch=odd8), dict(mask=fake, nbytes=need - 1)]
    cases += [dict(s=s) for s in bad_scales]
    for kw in cases:
        assert bwd(**kw) == -1000, kw
        assert b"dn_camera_records_backward" in hiplib.dn_last_error(), kw
    assert bwd(nbytes=need - 1) == -1000 and b"scratch" in hiplib.dn_last_error()
    assert bwd(nv=0, gphi=None) == 0 and bwd(nv=0, pv=1, keep=fake, gkeep=fake, scratch=None, nbytes=0) == 0
    assert bwd(nv=0, phi=None, gphi=None, mask=fake, scratch=None, nbytes=0) == 0


def test_refiners_refuse_bad_refinement_settings():
    import nerf
    from nerf import synthetic as syn
    h, w = 8, 10
    e = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES])
    k = torch.from_numpy(syn.intrinsic(h, w))
    images = torch.zeros(V, h, w, 3)

    def fused(**kw):
        return nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3, **kw)

    def host(**kw):
        return nerf.MultiPoseRefiner(None, None, None, h, w, k, e, None, None, num_rays=4, lr=1e-3, **kw)
    bad = [dict(refine_intrinsics="both"), dict(refine_intrinsics=True), dict(fixed_views=(V,)), dict(fixed_views=(0, -1)),
           dict(refine_intrinsics="shared", intrinsics_scale=0.0), dict(refine_intrinsics="per_view", intrinsics_scale=-1.0),
           dict(intrinsics_scale=float("nan")), dict(intrinsics_scale=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError, match="FusedPoseStep"):
            fused(**kw)
        with pytest.raises(ValueError, match="MultiPoseRefiner"):
            host(**kw)
    with pytest.raises(ValueError, match="FusedPoseStep.*nothing to refine"):
        fused(refine_pose=False)
    with pytest.raises(ValueError, match="FusedPoseStep"):
        fused(refine_pose=False, fixed_views=(1,))
    # good settings get as far as the device check
    for kw in (dict(refine_intrinsics="shared", intrinsics_scale=0.25, fixed_views=(0, 2)), dict(refine_intrinsics="per_view")):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            fused(**kw)
        with pytest.raises(RuntimeError, match="ROCm device only"):
            host(**kw)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fused(refine_intrinsics="shared", refine_pose=False)


def test_refined_intrinsics_is_the_parameterisation():
    """The host form MultiPoseRefiner differentiates: the three formulas, every other entry as given, (V,3,3) when K0 or phi is per view."""
    from nerf.pose import refined_intrinsics
    k0 = torch.tensor([[50.0, 0.3, 26.0], [0.1, 48.0, 20.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    phi = torch.tensor([0.1, 0.01, -0.02], dtype=torch.float64, requires_grad=True)
    s = 0.25
    got = refined_intrinsics(k0, phi, s)
    want = k0.clone()
    want[0, 0], want[0, 2], want[1, 2] = 50.0 * np.exp(s * 0.1), 26.0 + s * 50.0 * 0.01, 20.0 - s * 50.0 * 0.02
    assert got.shape == (3, 3) and torch.allclose(got.detach(), want, rtol=1e-15, atol=0)
    (got[0, 0] * 2.0 + got[0, 2] * 3.0 + got[1, 2] * 5.0).backward()
    assert torch.allclose(phi.grad, torch.tensor([2.0 * s * float(want[0, 0]), 3.0 * s * 50.0, 5.0 * s * 50.0], dtype=torch.float64), rtol=1e-14)
    assert torch.equal(refined_intrinsics(k0, torch.zeros(3, dtype=torch.float64), s), k0)
    per_view = refined_intrinsics(k0, torch.stack([phi.detach(), torch.zeros(3, dtype=torch.float64)]), s)
    assert per_view.shape == (2, 3, 3) and torch.equal(per_view[0], got.detach()) and torch.equal(per_view[1], k0)
    stacked = refined_intrinsics(torch.stack([k0, 2.0 * k0]), phi.detach(), s)
    assert stacked.shape == (2, 3, 3) and torch.equal(stacked[0], got.detach()) and float(stacked[1, 0, 0]) == 2.0 * float(got.detach()[0, 0])


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------------------------
def camera_inputs(n_views, mode, seed=0):
    """pose_inputs() repeated to n_views (V = 1: its |omega| = 0.3 view) with phi in [-0.1, 0.1] ((3,) | (V,3)) and a random g_cams."""
    xi, e0, k, _ = pose_inputs()
    idx = torch.tensor([3]) if n_views == 1 else torch.arange(n_views) % 5
    gen = torch.Generator().manual_seed(40 + seed + n_views)
    xi = xi[idx] + (torch.arange(n_views) // 5)[:, None] * 1e-3          # the repeats differ a little
    phi = (torch.rand((3,) if mode == "shared" else (n_views, 3), generator=gen) * 2.0 - 1.0) * 0.1
    return xi.contiguous(), phi, e0[idx].contiguous(), k[idx].contiguous(), torch.randn(n_views, 16, generator=gen)


def intrinsics64(phi, k, s):
    """(V,3) [fx, cx, cy] in float64 of phi (3,) | (V,3) float64 and k (V,3,3): the three formulas."""
    k = k.double()
    fx0 = k[:, 0, 0]
    a, b, c = (phi[..., i].expand(k.shape[0]) for i in range(3))
    return torch.stack([fx0 * torch.exp(s * a), k[:, 0, 2] + s * fx0 * b, k[:, 1, 2] + s * fx0 * c], dim=1)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", (1.0, 0.25))
@pytest.mark.parametrize("n_views", (1, 5, 65))
@pytest.mark.parametrize("mode", MODES)
def test_camera_records_and_their_backward_against_float64(dev, mode, n_views, scale):
    from nerf import _ops
    xi, phi, e0, k, g_cams = camera_inputs(n_views, mode)
    assert 0.05 < float(phi.abs().max()) <= 0.1
    d = [t.to(dev) for t in (xi, phi, e0, k, g_cams)]
    cams, extr = _ops.camera_records(d[0], d[1], d[2], d[3], scale, ndc_focal=NDC_F, want_extrinsics=True)
    g_xi, g_phi = _ops.camera_records_backward(d[4], d[0], d[1], d[2], d[3], scale)
    xi64 = xi.double().requires_grad_(True)
    # one leaf per view, so that a shared phi's per-view contributions are at hand
    phi_views = (phi.double().expand(n_views, 3) if mode == "shared" else phi.double()).clone().requires_grad_(True)
    want12, want_e = records64(xi64, e0.double())
    want_k = intrinsics64(phi_views, k, scale)
    ((want12 * g_cams[:, :12].double()).sum() + (want_k * g_cams[:, 12:15].double()).sum()).backward()
    contributions = phi_views.grad
    want_phi = contributions.sum(dim=0) if mode == "shared" else contributions
    errs = dict(rinv=rel_err(C(cams[:, :9]), want12[:, :9].detach().numpy()), origin=rel_err(C(cams[:, 9:12]), want12[:, 9:12].detach().numpy()),
                intrinsics=rel_err(C(cams[:, 12:15]), want_k.detach().numpy()), extrinsics=rel_err(C(extr), want_e.detach().numpy()),
                g_xi=rel_err(C(g_xi), xi64.grad.numpy()),
                # (shared: relative to the largest per-view contribution, not to the possibly cancelled sum)
                g_phi=float((g_phi.cpu().double() - want_phi).abs().max() / contributions.abs().max()))
    print(f"camera records vs float64, {mode} V={n_views} s={scale}:", {n: f"{e:.2e}" for n, e in errs.items()})
    assert g_phi.shape == ((3,) if mode == "shared" else (n_views, 3)) and g_xi.shape == (n_views, 6)
    assert bool(torch.isfinite(cams).all()) and bool(torch.isfinite(g_xi).all()) and bool(torch.isfinite(g_phi).all())
    assert float(want_phi.abs().min()) > 0 and bool((cams[:, 12] > 0).all())
    assert all(e <= 1e-6 for e in errs.values()), errs
    assert bool((cams[:, 15] == NDC_F).all()) and torch.equal(extr[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(n_views, 4))
    # one shared (3,3) K0 = the same matrix per view
    one = _ops.camera_records(d[0], d[1], d[2], d[3][0].contiguous(), scale)
    same = _ops.camera_records(d[0], d[1], d[2], d[3][0][None].expand(n_views, 3, 3).contiguous(), scale)
    assert torch.equal(one, same) and bool((one[:, 15] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_zero_phi_gives_the_bits_of_the_pose_records(dev, mode):
    from nerf import _ops
    xi, _, e0, k, g_cams = (t.to(dev) for t in camera_inputs(5, mode))
    want_c, want_e = _ops.pose_records(xi, e0, k, ndc_focal=NDC_F, want_extrinsics=True)
    want_g = _ops.pose_records_backward(g_cams, xi, e0)
    zeros = torch.zeros((3,) if mode == "shared" else (5, 3), device=dev)
    for phi in (zeros, None):
        for scale in (1.0, 0.25):
            cams, extr = _ops.camera_records(xi, phi, e0, k, scale, ndc_focal=NDC_F, want_extrinsics=True)
            g_xi, g_phi = _ops.camera_records_backward(g_cams, xi, phi, e0, k, scale, shared=mode == "shared")
            assert torch.equal(cams, want_c) and torch.equal(extr, want_e) and torch.equal(g_xi, want_g)
            assert g_phi.shape == zeros.shape and float(g_phi.abs().min()) > 0
        only, none = _ops.camera_records_backward(g_cams, xi, phi, e0, k, want_phi=False)
        assert none is None and torch.equal(only, want_g)
    shared_k = k[1].contiguous()
    assert torch.equal(_ops.camera_records(xi, zeros, e0, shared_k), _ops.pose_records(xi, e0, shared_k))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_masked_views_get_exact_zeros_and_keep_their_intrinsics_gradient(dev, mode):
    from nerf import _ops
    xi, phi, e0, k, g_cams = (t.to(dev) for t in camera_inputs(5, mode))
    free_xi, free_phi = _ops.camera_records_backward(g_cams, xi, phi, e0, k, 0.25)
    mask = torch.tensor([1, 0, 1, 0, 7], dtype=torch.int32, device=dev)
    g_xi, g_phi = _ops.camera_records_backward(g_cams, xi, phi, e0, k, 0.25, pose_mask=mask)
    held = mask == 0
    assert bool((g_xi[held] == 0).all()) and not bool(torch.signbit(g_xi[held]).any())
    assert torch.equal(g_xi[~held], free_xi[~held]) and float(free_xi[held].abs().min()) > 0
    assert torch.equal(g_phi, free_phi) and float(g_phi.abs().min()) > 0
    all_held, phi_only = _ops.camera_records_backward(g_cams, xi, phi, e0, k, 0.25, pose_mask=torch.zeros(5, dtype=torch.int32, device=dev))
    assert bool((all_held == 0).all()) and torch.equal(phi_only, free_phi)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_calls_give_the_same_bits_and_write_the_buffers_given(dev, mode):
    from nerf import _ops
    n_views = 65
    xi, phi, e0, k, g_cams = (t.to(dev) for t in camera_inputs(n_views, mode))
    cams, extr = _ops.camera_records(xi, phi, e0, k, want_extrinsics=True)
    cams_buf, extr_buf = torch.full((n_views, 16), float("nan"), device=dev), torch.full((n_views, 4, 4), float("nan"), device=dev)
    out = _ops.camera_records(xi, phi, e0, k, cams=cams_buf, extrinsics=extr_buf)
    assert out[0] is cams_buf and out[1] is extr_buf and torch.equal(cams_buf, cams) and torch.equal(extr_buf, extr)
    g_xi, g_phi = _ops.camera_records_backward(g_cams, xi, phi, e0, k)
    bufs = [torch.full(shape, float("nan"), device=dev) for shape in ((n_views, 6), (n_views, 6), tuple(g_phi.shape), tuple(g_phi.shape))]
    got = _ops.camera_records_backward(g_cams, xi, phi, e0, k, out=bufs[0], keep=bufs[1], out_phi=bufs[2], keep_phi=bufs[3])
    assert got[0] is bufs[0] and got[1] is bufs[2]
    assert torch.equal(bufs[0], g_xi) and torch.equal(bufs[1], g_xi) and torch.equal(bufs[2], g_phi) and torch.equal(bufs[3], g_phi)
    if mode == "shared":        # no views: the three zeros
        empty = torch.zeros(0, 6, device=dev)
        g0 = _ops.camera_records_backward(torch.zeros(0, 16, device=dev), empty, phi, torch.zeros(0, 4, 4, device=dev), k[0].contiguous(),
                                          out_phi=torch.full((3,), float("nan"), device=dev))[1]
        assert torch.equal(g0.cpu(), torch.zeros(3))


# ---- GPU: the step ----------------------------------------------------------------------------------------------------------------------
def start(step, mode):
    step.xi.copy_(torch.tensor(XI_START))
    if mode is not None:
        step.phi.copy_(torch.tensor(PHI_START[mode]))
    return step.xi.clone(), None if mode is None else step.phi.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,num_rays", [("world", 96), ("world", 2), ("ndc", 96)])
@pytest.mark.parametrize("mode", MODES)
def test_one_step_is_the_chain_of_its_pieces(dev, lego, monkeypatch, mode, scene, num_rays):
    """test_fused_pose_step's test of this name with the intrinsics refined, from a non-zero xi AND a non-zero phi: camera_records,
    rows and targets bit for bit, the stage-by-stage render under autograd, dn_camera_grad_views, dn_camera_records_backward; then
    torch.optim.Adam on the concatenated [xi | phi].  2 rays over three views, per view: a view without a ray keeps its xi and phi."""
    import nerf
    from nerf import _ops
    problem = world_problem(dev) if scene == "world" else ndc_problem(dev)
    h, w, e0, k, images, cfg, focal = problem
    scale = 0.5
    step = make_step(lego, problem, num_rays, seed=21, first_iteration=4, use_graphs=False, refine_intrinsics=mode, intrinsics_scale=scale)
    shape = (3,) if mode == "shared" else (V, 3)
    assert step.xi.shape == (V, 6) and step.phi.shape == shape and step.phi.dtype == torch.float32 and step.phi.is_cuda
    assert float(step.phi.abs().max()) == 0 and float(step.xi.abs().max()) == 0
    assert step.phi.data_ptr() == step.xi.data_ptr() + 4 * 6 * V and step._flat.shape[1] % 4 == 0       # one flat Adam buffer
    xi0, phi0 = start(step, mode)
    peek = _ops.new_rng_state(21, dev, 4)
    loss3 = step.step()
    assert loss3 is step.loss3 and step.rng_state.tolist()[2:] == [4, 5] and step.graph is None
    views, pix, rows, target = step.latest_draw()
    n = num_rays
    assert rows.shape == (n, 11) and target.shape == (n, 3) and (views.long() * (h * w) + pix).unique().numel() == n
    cams = _ops.camera_records(xi0, phi0, e0, k, scale, focal)
    rows2, target2 = _ops.select_rays_views(h, w, cams, views, cfg.dataset.near, cfg.dataset.far, pix, images, ndc_focal=focal, ndc_near=1.0)
    assert torch.equal(rows2, rows) and torch.equal(target2, target)
    assert not torch.equal(cams[:, 12:15], _ops.pose_records(xi0, e0, k, focal)[:, 12:15])
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
    want, want_phi = _ops.camera_records_backward(g_cams, xi0, phi0, e0, k, scale)
    err, err_phi = rel_err(C(step.last_grad), C(want)), rel_err(C(step.last_grad_phi), C(want_phi))
    got = loss3.tolist()
    losses = [(mse_c + mse_f).item(), mse_c.item(), mse_f.item()]
    print(f"{mode} {scene} {n} rays: last_grad vs the chain {err:.2e}, last_grad_phi {err_phi:.2e}; loss3 {got} vs {losses}; "
          f"rays per view {torch.bincount(views, minlength=V).tolist()}")
    assert step.last_grad_phi.shape == shape and float(want.abs().max()) > 0 and float(want_phi.abs().max()) > 0
    assert err <= 1e-5 and err_phi <= 1e-5, (err, err_phi)
    assert all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(got, losses)), (got, losses)
    param = torch.cat([xi0.reshape(-1), phi0.reshape(-1)]).requires_grad_(True)
    param.grad = torch.cat([step.last_grad.reshape(-1), step.last_grad_phi.reshape(-1)])
    torch.optim.Adam([param], lr=1e-3).step()
    assert rel_err(C(torch.cat([step.xi.reshape(-1), step.phi.reshape(-1)])), C(param)) <= 1e-6
    assert rel_err(C(step.phi).reshape(-1), C(param[6 * V:])) <= 1e-6 and not torch.equal(step.phi, phi0)
    empty = torch.bincount(views, minlength=V) == 0
    if n < V:
        assert bool(empty.any())
    assert bool((step.last_grad[empty] == 0).all()) and torch.equal(step.xi[empty], xi0[empty])
    assert bool((step.xi[~empty] != xi0[~empty]).any(dim=1).all())
    if mode == "per_view":
        assert bool((step.last_grad_phi[empty] == 0).all()) and torch.equal(step.phi[empty], phi0[empty])
        assert bool((step.phi[~empty] != phi0[~empty]).any(dim=1).all())
    est = step.intrinsics()
    k_views = k.double().cpu().expand(V, 3, 3)
    want_k = k_views.clone()
    fx_cx_cy = intrinsics64(step.phi.double().cpu(), k_views, scale)
    want_k[:, 0, 0], want_k[:, 0, 2], want_k[:, 1, 2] = fx_cx_cy[:, 0], fx_cx_cy[:, 1], fx_cx_cy[:, 2]
    if mode == "shared":
        want_k = want_k[0]
    assert est.shape == want_k.shape and est.is_cuda and est.dtype == torch.float32 and rel_err(C(est), want_k.numpy()) <= 1e-6
    untouched = torch.ones(3, 3, dtype=torch.bool)
    untouched[0, 0] = untouched[0, 2] = untouched[1, 2] = False
    assert torch.equal(est[..., untouched].cpu(), k.cpu().expand(est.shape)[..., untouched])


@pytest.mark.gpu
def test_fixed_views_and_a_fixed_pose_stay_bit_for_bit(dev, lego):
    problem = world_problem(dev)
    for kw in (dict(fixed_views=(1,)), dict(fixed_views=(0, 2), refine_intrinsics="per_view")):
        mode = kw.get("refine_intrinsics")
        step = make_step(lego, problem, 96, seed=5, use_graphs=False, **kw)
        xi0, phi0 = start(step, mode)
        for _ in range(4):
            step.step()
        fixed = torch.zeros(V, dtype=torch.bool)
        fixed[list(kw["fixed_views"])] = True
        assert (step.phi is None) == (mode is None) and (step.last_grad_phi is None) == (mode is None)
        assert torch.equal(step.xi[fixed], xi0[fixed]) and bool((step.last_grad[fixed] == 0).all())
        assert bool((step.xi[~fixed] != xi0[~fixed]).any(dim=1).all()) and bool(torch.isfinite(step.xi).all())
        if mode is not None:
            assert bool((step.phi != phi0).any(dim=1).all())
    step = make_step(lego, problem, 96, seed=5, use_graphs=False, refine_intrinsics="shared", refine_pose=False)
    xi0, phi0 = start(step, "shared")
    for _ in range(4):
        step.step()
    assert torch.equal(step.xi, xi0) and bool((step.last_grad == 0).all())
    assert bool((step.phi != phi0).all()) and bool(torch.isfinite(step.phi).all()) and float(step.last_grad_phi.abs().min()) > 0
    # what a fixed pose leaves of the intrinsics gradient is the free step's (the first step of both starts from the same state)
    free = make_step(lego, problem, 96, seed=5, use_graphs=False, refine_intrinsics="shared")
    held = make_step(lego, problem, 96, seed=5, use_graphs=False, refine_intrinsics="shared", refine_pose=False)
    for s in (free, held):
        start(s, "shared")
        s.step()
    assert torch.equal(free.last_grad_phi, held.last_grad_phi) and float(free.last_grad.abs().max()) > 0


@pytest.mark.gpu
def test_replayed_steps_equal_eager_steps_with_shared_intrinsics(dev, lego):
    mc, mf = lego[0], lego[1]
    problem = world_problem(dev)
    params = list(mc.parameters()) + list(mf.parameters())
    before = [p.detach().clone() for p in params]
    flags = [i % 2 == 0 for i in range(len(params))]
    for p, flag in zip(params, flags):
        p.requires_grad_(flag)
    try:
        eager = make_step(lego, problem, 96, seed=8, use_graphs=False, refine_intrinsics="shared")
        graphed = make_step(lego, problem, 96, seed=8, eager_iterations=1, refine_intrinsics="shared")
        for s in (eager, graphed):
            start(s, "shared")
        for it in range(4):
            eager.step(); graphed.step()
            assert (graphed.graph is not None) == (it >= 1)
        torch.cuda.synchronize()
        assert graphed.graph is not None and graphed.fallback_reason is None, graphed.fallback_reason
        assert eager.graph is None and eager.fallback_reason is None
        assert torch.equal(eager.xi, graphed.xi) and torch.equal(eager.phi, graphed.phi) and torch.equal(eager.loss3, graphed.loss3)
        assert torch.equal(eager.last_grad, graphed.last_grad) and torch.equal(eager.last_grad_phi, graphed.last_grad_phi)
        assert bool(torch.isfinite(eager.phi).all()) and float(eager.last_grad_phi.abs().min()) > 0
        assert not torch.equal(eager.phi, torch.tensor(PHI_START["shared"], device=dev))
        assert eager.rng_state.tolist()[2:] == [3, 4] and graphed.rng_state.tolist()[2:] == [3, 4]
        assert [p.requires_grad for p in params] == flags and all(p.grad is None for p in params)
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    finally:
        for p in params:
            p.requires_grad_(False)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused_step_against_the_host_reference(dev, lego, mode):
    """FusedPoseStep against MultiPoseRefiner (float64 phi and xi on the host, K built differentiably, select_camera_rays under autograd)
    on the fused step's own pairs, both rendering deterministically from the same non-zero xi and phi.  The yardstick for last_grad_phi is
    the last_grad (xi) discrepancy of the same two objects in the same run - fp32 records against float64 host inverses, parent-commit code
    on both sides: gate max(1e-5, 4 x that); the factor 4 for phi's chain, which multiplies by fx and, shared, sums V = 3 views.  A
    yardstick above 1e-3 is too loose to gate on and is reported (a warning with both figures) instead.

    Measured on an MI355X (profiles/intrinsics_refinement.md): shared - xi 2.126e-03, phi 2.102e-03; per_view - xi 8.222e-03, phi
    7.817e-03: the yardstick is above 1e-3 in both modes, so both report.  The two routes' rows differ in their last bits (the host
    inverts in fp32, the device in fp64 rounded once) and the 10-frequency encoding and the resampling turn that into the third digit
    of a 96-ray gradient; phi's discrepancy follows xi's, and on identical rows test_one_step_is_the_chain_of_its_pieces holds both
    gradients to 1e-5."""
    import nerf
    mc, mf, ex, ed = lego
    h, w, e0, k, images, _, _ = world_problem(dev)
    cfg = make_cfg(dict(STEP_CFG, perturb=False, noise_std=0.0, near=2.0, far=6.0))
    scale = 0.5
    fused = nerf.FusedPoseStep(mc, mf, cfg, h, w, k, e0, images, ex, ed, num_rays=96, lr=1e-3, seed=13, use_graphs=False,
                               refine_intrinsics=mode, intrinsics_scale=scale)
    host = nerf.MultiPoseRefiner(mc, mf, cfg, h, w, k, e0, ex, ed, num_rays=96, lr=1e-3, seed=13, refine_intrinsics=mode, intrinsics_scale=scale)
    start(fused, mode)
    with torch.no_grad():
        host.xi.copy_(torch.tensor(XI_START, dtype=torch.float64))
        host.phi.copy_(torch.tensor(PHI_START[mode], dtype=torch.float64))
    assert host.phi.dtype == torch.float64 and not host.phi.is_cuda and host.phi.shape == fused.phi.shape
    assert rel_err(C(fused.intrinsics()), C(host.intrinsics())) <= 1e-6 and host.intrinsics().is_cuda
    loss3 = fused.step()
    views, pix = fused.latest_draw()[:2]
    loss = host.step(images, pairs=(views, pix))
    d_xi = rel_err(C(fused.last_grad), host.last_grad.numpy())
    d_phi = rel_err(C(fused.last_grad_phi), host.last_grad_phi.numpy())
    gate = max(1e-5, 4.0 * d_xi)
    print(f"fused vs host, {mode}: last_grad (xi) discrepancy {d_xi:.3e}, last_grad_phi discrepancy {d_phi:.3e}, gate {gate:.3e}; "
          f"loss {float(loss3[0]):.6e} vs {float(loss):.6e}")
    assert host.last_grad_phi.shape == fused.last_grad_phi.shape and float(host.last_grad_phi.abs().max()) > 0
    assert bool(torch.isfinite(fused.last_grad_phi).all()) and bool(torch.isfinite(host.last_grad_phi).all())
    if d_xi > 1e-3:
        warnings.warn(f"FusedPoseStep against MultiPoseRefiner, {mode}: the xi yardstick itself is {d_xi:.3e} (> 1e-3): reported, not gated; phi {d_phi:.3e}")
    else:
        assert d_phi <= gate, (d_phi, gate)
