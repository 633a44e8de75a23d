"""Ray generation differentiated w.r.t. the camera: dn_camera_grad (the backward of dn_ray_bundle / dn_select_rays* w.r.t. the
16-float camera record) and dn_select_rays_indirect_ndc, _ops.camera_record / CameraRaysFn, and the routing of nerf.get_ray_bundle and
nerf.select_camera_rays - so that a pose, an intrinsic matrix, a focal length or an NDC focal length that requires grad receives
the gradient float64 autograd through the oracle gives it.  (se3_exp / PoseRefiner and the end-to-end chain: test_pose_refinement.py.)

Yardstick: float64 autograd of oracle.nerf_oracle.get_ray_bundle -> selection -> rd / |rd| -> ndc_rays (where it applies), on the
same fp32 values cast up, with random upstream gradients.  Gate 1e-5 in the project's norm, max|a - b| <= tol * max|b| per tensor
(conftest.rel_err): plain fp32 CPU autograd of the same chain is within 9e-7 of it on these inputs, and the kernel forms its
Jacobian and sums in fp64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

NEW_SYMBOLS = ("dn_camera_grad", "dn_camera_grad_scratch_bytes", "dn_select_rays_indirect_ndc")
GATE = 1e-5
SHAPES = ((7, 13), (45, 67))     # 91 rays: below a wave wide, a partial second wave; 3015 rays: several workgroups, the last partial
SELECT_N = (1, 64, 65, 257)
NDC_N = (1, 65, 257)
NDC_H, NDC_W, NDC_F, NDC_NEAR = 45, 67, 60.0, 1.0


def C(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def world_camera(h, w):
    """(E, K) fp32 host tensors: pose 9 of the synthetic scene, the Blender-style intrinsic."""
    from nerf import synthetic as syn
    return torch.from_numpy(syn.scene_pose(9)), torch.from_numpy(syn.intrinsic(h, w))


def c2w_camera(h, w):
    """(c2w, focal) fp32 host tensors of the same view in the 4-argument (camera-to-world, OpenGL axes) convention."""
    from nerf import synthetic as syn
    theta = np.linspace(-180.0, 180.0, 41)[:-1][9]
    return torch.from_numpy(syn.pose_spherical_c2w(float(theta), -30.0, 4.0)), torch.tensor(float(syn.intrinsic(h, w)[0, 0]))


def ndc_camera():
    """(E, K) of the first forward-facing camera of test_forward_facing_training.forward_facing_selector, rotated by 0.05 rad about y
    so that no entry of the camera record is a structural zero.  Every direction has rd_z near -1."""
    c2w = np.eye(4)
    c2w[:3, :3] = np.diag([1.0, -1.0, -1.0])
    c2w[:3, 3] = [-0.2, 0.0, 4.0]
    a = 0.05
    rot = np.array([[np.cos(a), 0.0, np.sin(a), 0.0], [0.0, 1.0, 0.0, 0.0], [-np.sin(a), 0.0, np.cos(a), 0.0], [0.0, 0.0, 0.0, 1.0]])
    e = torch.from_numpy(np.linalg.inv(rot @ c2w).astype(np.float32))
    k = torch.tensor([[NDC_F, 0.0, NDC_W * 0.5], [0.0, NDC_F, NDC_H * 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return e, k


def selection(n, total, seed=3):
    """n pixel indices: pixel 0, pixel H W - 1, one repeated pixel, a descending run, then random ones (n = 1: pixel 0 alone)."""
    gen = torch.Generator().manual_seed(seed)
    head = [0, total - 1, 100, 100] + list(range(2000, 1988, -1))
    rest = torch.randint(0, total, (max(n, 16),), generator=gen).tolist()
    return torch.tensor((head + rest)[:n], dtype=torch.int64)


def upstream(n, cols, seed):
    """Random fp32 upstream gradients (n, cols); row 5 (when there is one) all zeros."""
    g = torch.randn(n, cols, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    if n > 5:
        g[5] = 0.0
    return g


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
def oracle_rays64(h, w, e64, k64, pix=None, ndc=None):
    """(ro, rd, viewdir) (N,3) float64 through the oracle; ndc = (focal, near): ro / rd warped, the view direction that of the
    unwarped direction."""
    from oracle import nerf_oracle as oc
    ro, rd = oc.get_ray_bundle(h, w, e64, k64)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    if pix is not None:
        ro, rd = ro[pix], rd[pix]
    vd = rd / rd.norm(dim=-1, keepdim=True)
    if ndc is not None:
        ro, rd = oc.ndc_rays(h, w, ndc[0], ndc[1], ro, rd)
    return ro, rd, vd


def oracle_grads_5arg(h, w, e32, k32, pix, g_ro, g_rd, g_vd, ndc_focal=None):
    """(dE, dK[, d ndc_focal]) in float64."""
    e64, k64 = e32.double().requires_grad_(True), k32.double().requires_grad_(True)
    f64 = None if ndc_focal is None else torch.tensor(float(ndc_focal), dtype=torch.float64, requires_grad=True)
    ro, rd, vd = oracle_rays64(h, w, e64, k64, pix, None if f64 is None else (f64, NDC_NEAR))
    loss = (ro * g_ro.double()).sum() + (rd * g_rd.double()).sum()
    if g_vd is not None:
        loss = loss + (vd * g_vd.double()).sum()
    loss.backward()
    return (e64.grad, k64.grad) + (() if f64 is None else (f64.grad,))


def oracle_grads_4arg(h, w, c2w32, focal32, pix, g_ro, g_rd, g_vd):
    """(d c2w, d focal) in float64: the 4-argument convention is the 5-argument one with E = inv(c2w diag(1, -1, -1, 1)),
    K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]].  d c2w is that of the three rows the convention reads (the constant bottom
    row [0, 0, 0, 1] is an input of this composition only)."""
    c64, f64 = c2w32.double().requires_grad_(True), focal32.double().requires_grad_(True)
    e64 = torch.inverse(c64 @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64)))
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    k64 = torch.stack([torch.stack([f64, zero, one * (w * 0.5)]), torch.stack([zero, f64, one * (h * 0.5)]), torch.stack([zero, zero, one])])
    ro, rd, vd = oracle_rays64(h, w, e64, k64, pix)
    loss = (ro * g_ro.double()).sum() + (rd * g_rd.double()).sum()
    if g_vd is not None:
        loss = loss + (vd * g_vd.double()).sum()
    loss.backward()
    return c64.grad[:3], f64.grad


def check_grads(got, want, what):
    errs = [rel_err(C(a), b.numpy()) for a, b in zip(got, want)]
    print(f"{what}: " + ", ".join(f"{e:.2e}" for e in errs))
    for b in want:
        assert float(b.abs().max()) > 0, what
    assert max(errs) <= GATE, (what, errs)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_resolvable(hiplib):
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(raw, name), name
    assert hiplib.dn_abi_version() == 2 and "#define DN_ABI_VERSION 2" in header


def test_argument_validation_returns_before_gpu_work(hiplib):
    """DN_E_INVAL (-1000) with a message, before anything is launched or dereferenced (the device pointers are small integers).
    dn_camera_grad with zero rays still has 16 zeros to write, so its n = 0 case runs on the GPU (test below); the selection entry
    point returns 0 for zero rays like its siblings."""
    fake = ctypes.c_void_p(256)
    big = 1 << 20

    def grad(h=8, w=8, cam=fake, n=4, g_ro=fake, s_ro=3, g_rd=fake, s_rd=3, g_vd=None, s_vd=0, focal=0.0, near=1.0, scratch=fake,
             nbytes=big, g_cam=fake, pix=fake):
        return hiplib.dn_camera_grad(h, w, cam, pix, n, g_ro, s_ro, g_rd, s_rd, g_vd, s_vd, focal, near, scratch, nbytes, g_cam, None)
    need = hiplib.dn_camera_grad_scratch_bytes(4)
    for kw in (dict(cam=None), dict(g_cam=None), dict(g_ro=None, g_rd=None, g_vd=None), dict(s_ro=2), dict(s_rd=0), dict(g_vd=fake, s_vd=2),
               dict(scratch=None), dict(nbytes=need - 1), dict(nbytes=0), dict(h=1 << 16, w=1 << 15), dict(h=0), dict(w=-1), dict(n=-1),
               dict(focal=float("nan")), dict(focal=float("inf")), dict(focal=-1.0), dict(near=float("nan")), dict(pix=None, n=65),
               dict(n=0, cam=None), dict(n=0, g_ro=None, g_rd=None)):
        assert grad(**kw) == -1000, kw
        assert b"dn_camera_grad" in hiplib.dn_last_error(), kw
    assert grad(nbytes=need - 1) == -1000 and b"scratch" in hiplib.dn_last_error()
    assert grad(s_ro=2) == -1000 and b"stride" in hiplib.dn_last_error()

    def sel(h=8, w=8, cams=fake, view=fake, pix=fake, n=4, images=None, channels=0, rays=fake, target=None, focal=50.0, near=1.0):
        return hiplib.dn_select_rays_indirect_ndc(h, w, cams, view, 0.0, 1.0, pix, n, images, channels, rays, target, focal, near, None)
    for kw in (dict(cams=None), dict(view=None), dict(pix=None), dict(rays=None), dict(h=0), dict(n=-1), dict(target=fake),
               dict(target=fake, images=fake, channels=2), dict(focal=0.0), dict(focal=float("nan")), dict(near=float("inf"))):
        assert sel(**kw) == -1000, kw
        assert b"dn_select_rays_indirect_ndc" in hiplib.dn_last_error(), kw
    assert sel(n=0) == 0 and sel(n=0, cams=None) == 0


def test_scratch_size_is_a_function_of_n_alone(hiplib):
    sizes = [hiplib.dn_camera_grad_scratch_bytes(n) for n in (0, 1, 91, 256, 257, 3015, 4096, 160000, 640000, 1 << 40)]
    assert all(s > 0 and s % 128 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes == [hiplib.dn_camera_grad_scratch_bytes(n) for n in (0, 1, 91, 256, 257, 3015, 4096, 160000, 640000, 1 << 40)]
    assert sizes[-1] == sizes[-2] <= 64 * 1024          # the number of workgroups is capped: the second launch stays small


@pytest.mark.parametrize("h,w", SHAPES)
def test_host_ray_bundle_carries_the_gradient_to_pose_and_intrinsic(h, w):
    """Host tensors, 5-argument convention: dE, dK <= 1e-5 against the float64 oracle; values torch.equal to the no-grad call's."""
    import nerf
    e32, k32 = world_camera(h, w)
    g_ro, g_rd = upstream(h * w, 3, 11), upstream(h * w, 3, 12)
    e, k = e32.clone().requires_grad_(True), k32.clone().requires_grad_(True)
    ro, rd = nerf.get_ray_bundle(h, w, 1.0, e, k)
    ro0, rd0 = nerf.get_ray_bundle(h, w, 1.0, e32, k32)
    assert torch.equal(ro, ro0) and torch.equal(rd, rd0) and not ro0.requires_grad and not rd0.requires_grad
    ((ro.reshape(-1, 3) * g_ro).sum() + (rd.reshape(-1, 3) * g_rd).sum()).backward()
    assert e.grad is not None and k.grad is not None
    check_grads((e.grad, k.grad), oracle_grads_5arg(h, w, e32, k32, None, g_ro, g_rd, None), f"host bundle {h}x{w} (E, K)")
    with torch.no_grad():
        ro1, rd1 = nerf.get_ray_bundle(h, w, 1.0, e, k)
    assert ro1.grad_fn is None and rd1.grad_fn is None and torch.equal(rd1, rd0)


@pytest.mark.parametrize("h,w", SHAPES)
def test_host_ray_bundle_4_argument_convention(h, w):
    import nerf
    c32, f32 = c2w_camera(h, w)
    g_ro, g_rd = upstream(h * w, 3, 13), upstream(h * w, 3, 14)
    c, f = c32.clone().requires_grad_(True), f32.clone().requires_grad_(True)
    ro, rd = nerf.get_ray_bundle(h, w, f, c)
    ro0, rd0 = nerf.get_ray_bundle(h, w, float(f32), c32)
    assert torch.equal(ro, ro0) and torch.equal(rd, rd0)
    ((ro.reshape(-1, 3) * g_ro).sum() + (rd.reshape(-1, 3) * g_rd).sum()).backward()
    assert not c.grad[3].any()
    check_grads((c.grad[:3], f.grad), oracle_grads_4arg(h, w, c32, f32, None, g_ro, g_rd, None), f"host bundle {h}x{w} (c2w, focal)")


def test_camera_record_layout():
    """[rinv9, origin3, fx, cx, cy, ndc_focal]: the values get_ray_bundle / RaySelector hand the kernels."""
    from nerf import _ops
    import nerf
    h, w = 45, 67
    e32, k32 = world_camera(h, w)
    rec = _ops.camera_record(e32, k32, None, h, w, ndc_focal=torch.tensor(60.0))
    sel = nerf.RaySelector(h, w, e32, k32, 2.0, 6.0, device="cpu")
    assert rec.shape == (16,) and rec.dtype == torch.float32
    assert rec.tolist() == sel.rinv + sel.origin + [sel.fx, sel.cx, sel.cy, 60.0]
    c32, f32 = c2w_camera(h, w)
    rec4 = _ops.camera_record(c32, None, f32, h, w)
    flipped = c32[:3, :3].clone()
    flipped[:, 1:] = -flipped[:, 1:]
    assert rec4.tolist() == flipped.reshape(-1).tolist() + c32[:3, 3].tolist() + [float(f32), w * 0.5, h * 0.5, 0.0]


def test_select_camera_rays_is_device_only():
    import nerf
    e32, k32 = world_camera(45, 67)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.select_camera_rays(45, 67, e32, k32, 2.0, 6.0, selection(8, 45 * 67))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf import _hip
    _hip.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_device_ray_bundle_5_argument_gradient(dev, h, w):
    """get_ray_bundle on a device pose / intrinsic that require grad: values torch.equal to the no-grad call's, dE, dK <= 1e-5."""
    import nerf
    e32, k32 = world_camera(h, w)
    g_ro, g_rd = upstream(h * w, 3, 21), upstream(h * w, 3, 22)
    e, k = e32.to(dev).requires_grad_(True), k32.to(dev).requires_grad_(True)
    ro, rd = nerf.get_ray_bundle(h, w, 1.0, e, k)
    ro0, rd0 = nerf.get_ray_bundle(h, w, 1.0, e32.to(dev), k32.to(dev))
    assert ro.grad_fn is not None and rd.grad_fn is not None and ro0.grad_fn is None and rd0.grad_fn is None
    assert ro.shape == (h, w, 3) and torch.equal(ro, ro0) and torch.equal(rd, rd0)
    ((ro.reshape(-1, 3) * g_ro.to(dev)).sum() + (rd.reshape(-1, 3) * g_rd.to(dev)).sum()).backward()
    assert e.grad.is_cuda and k.grad.is_cuda
    check_grads((e.grad, k.grad), oracle_grads_5arg(h, w, e32, k32, None, g_ro, g_rd, None), f"device bundle {h}x{w} (E, K)")
    # only the directions used: the origin's gradient pointer is NULL
    e2 = e32.to(dev).requires_grad_(True)
    _, rd2 = nerf.get_ray_bundle(h, w, 1.0, e2, k32.to(dev))
    (rd2.reshape(-1, 3) * g_rd.to(dev)).sum().backward()
    want = oracle_grads_5arg(h, w, e32, k32, None, torch.zeros_like(g_ro), g_rd, None)
    check_grads((e2.grad,), want[:1], f"device bundle {h}x{w}, rd only (E)")


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_device_ray_bundle_4_argument_gradient(dev, h, w):
    import nerf
    c32, f32 = c2w_camera(h, w)
    g_ro, g_rd = upstream(h * w, 3, 23), upstream(h * w, 3, 24)
    c, f = c32.to(dev).requires_grad_(True), f32.to(dev).requires_grad_(True)
    ro, rd = nerf.get_ray_bundle(h, w, f, c)
    ro0, rd0 = nerf.get_ray_bundle(h, w, float(f32), c32.to(dev))
    assert rd.grad_fn is not None and torch.equal(ro, ro0) and torch.equal(rd, rd0)
    ((ro.reshape(-1, 3) * g_ro.to(dev)).sum() + (rd.reshape(-1, 3) * g_rd.to(dev)).sum()).backward()
    assert not c.grad[3].any()
    check_grads((c.grad[:3], f.grad), oracle_grads_4arg(h, w, c32, f32, None, g_ro, g_rd, None), f"device bundle {h}x{w} (c2w, focal)")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SELECT_N)
def test_select_camera_rays_rows_and_gradient(dev, n):
    """World-space rows of the 45 x 67 camera: rows and targets torch.equal to RaySelector.select's; dE, dK with upstream gradients on
    all 11 columns (near / far receive one and contribute nothing) <= 1e-5; the 4-argument convention's d c2w, d focal too."""
    import nerf
    h, w = SHAPES[1]
    e32, k32 = world_camera(h, w)
    pix = selection(n, h * w)
    image = torch.rand(h, w, 4, generator=torch.Generator().manual_seed(9)).to(dev)
    g = upstream(n, 11, 30 + n)
    e, k = e32.to(dev).requires_grad_(True), k32.to(dev).requires_grad_(True)
    rows, target = nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix.to(dev), image=image)
    rows0, target0 = nerf.RaySelector(h, w, e32.to(dev), k32.to(dev), 2.0, 6.0).select(pix.to(dev), image)
    assert rows.grad_fn is not None and not target.requires_grad
    assert torch.equal(rows, rows0) and torch.equal(target, target0)
    (rows * g.to(dev)).sum().backward()
    check_grads((e.grad, k.grad), oracle_grads_5arg(h, w, e32, k32, pix, g[:, 0:3], g[:, 3:6], g[:, 8:11]), f"rows N={n} (E, K)")
    c32, f32 = c2w_camera(h, w)
    c, f = c32.to(dev).requires_grad_(True), f32.to(dev).requires_grad_(True)
    rows4, none = nerf.select_camera_rays(h, w, c, None, 2.0, 6.0, pix.to(dev), focal_length=f)
    assert none is None and rows4.shape == (n, 11)
    (rows4 * g.to(dev)).sum().backward()
    assert not c.grad[3].any()
    check_grads((c.grad[:3], f.grad), oracle_grads_4arg(h, w, c32, f32, pix, g[:, 0:3], g[:, 3:6], g[:, 8:11]), f"rows N={n} (c2w, focal)")


@pytest.mark.gpu
@pytest.mark.parametrize("n", NDC_N)
def test_select_camera_rays_ndc_rows_and_gradient(dev, n):
    """NDC rows of the rotated forward-facing camera (f = 60, near plane 1): torch.equal to RaySelector.select followed by
    _ops.ndc_rays on columns 0:6, columns 6:11 untouched; dE, dK, d ndc_focal <= 1e-5."""
    import nerf
    from nerf import _ops
    h, w = NDC_H, NDC_W
    e32, k32 = ndc_camera()
    pix = selection(n, h * w)
    image = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    g = upstream(n, 11, 40 + n)
    e, k = e32.to(dev).requires_grad_(True), k32.to(dev).requires_grad_(True)
    focal = torch.tensor(NDC_F, device=dev, requires_grad=True)
    rows, target = nerf.select_camera_rays(h, w, e, k, 0.0, 1.0, pix.to(dev), image=image, ndc_focal=focal, ndc_near=NDC_NEAR)
    rows0, target0 = nerf.RaySelector(h, w, e32.to(dev), k32.to(dev), 0.0, 1.0).select(pix.to(dev), image)
    ro, rd = _ops.ndc_rays(h, w, NDC_F, NDC_NEAR, rows0[:, :3].contiguous(), rows0[:, 3:6].contiguous())
    assert torch.equal(rows[:, :3], ro) and torch.equal(rows[:, 3:6], rd) and torch.equal(rows[:, 6:], rows0[:, 6:])
    assert torch.equal(target, target0)
    assert float((rows0[:, 5].abs()).min()) > 0.5           # rd_z well away from 0
    (rows * g.to(dev)).sum().backward()
    want = oracle_grads_5arg(h, w, e32, k32, pix, g[:, 0:3], g[:, 3:6], g[:, 8:11], ndc_focal=NDC_F)
    check_grads((e.grad, k.grad, focal.grad), want, f"NDC rows N={n} (E, K, ndc_focal)")
    # without grad: the same rows from the same kernel, no graph
    rows1, _ = nerf.select_camera_rays(h, w, e32.to(dev), k32.to(dev), 0.0, 1.0, pix.to(dev), image=image, ndc_focal=NDC_F)
    assert rows1.grad_fn is None and torch.equal(rows1, rows)


@pytest.mark.gpu
def test_camera_grad_is_bit_reproducible_and_writes_zeros_for_no_rays(dev, hiplib):
    from nerf import _ops
    h, w = SHAPES[1]
    e32, k32 = ndc_camera()
    cam = _ops.camera_record(e32, k32, None, h, w).to(dev)
    for n, pix in ((h * w, None), (257, selection(257, h * w).to(dev))):
        g = upstream(n, 11, 50).to(dev)
        for focal in (0.0, NDC_F):
            a = _ops.camera_grad(h, w, cam, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, NDC_NEAR)
            b = _ops.camera_grad(h, w, cam, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, NDC_NEAR)
            assert torch.isfinite(a).all() and float(a.abs().max()) > 0 and torch.equal(a, b)
            assert (float(a[15]) != 0.0) == (focal > 0.0)
    g = torch.zeros(1, 11, device=dev)
    out = torch.full((16,), 7.0, device=dev)
    scratch = torch.empty(hiplib.dn_camera_grad_scratch_bytes(0) // 8, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = hiplib.dn_camera_grad(h, w, p(cam), None, 0, p(g), 11, p(g), 11, None, 0, 0.0, 1.0, p(scratch), scratch.numel() * 8, p(out),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and torch.equal(out, torch.zeros(16, device=dev))


@pytest.mark.gpu
def test_cameras_without_grad_take_todays_path(dev):
    """A camera that does not require grad, and a call under torch.no_grad(): no grad_fn, torch.equal values."""
    import nerf
    h, w = SHAPES[0]
    e32, k32 = world_camera(h, w)
    pix = selection(64, h * w).clamp(max=h * w - 1).to(dev)
    e, k = e32.to(dev).requires_grad_(True), k32.to(dev).requires_grad_(True)
    ro, rd = nerf.get_ray_bundle(h, w, 1.0, e, k)
    rows, _ = nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix)
    with torch.no_grad():
        ro1, rd1 = nerf.get_ray_bundle(h, w, 1.0, e, k)
        rows1, _ = nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix)
    ro2, rd2 = nerf.get_ray_bundle(h, w, 1.0, e.detach(), k.detach())
    rows2, _ = nerf.select_camera_rays(h, w, e.detach(), k.detach(), 2.0, 6.0, pix)
    for t in (ro1, rd1, rows1, ro2, rd2, rows2):
        assert t.grad_fn is None and not t.requires_grad
    assert torch.equal(ro1, ro) and torch.equal(rd1, rd) and torch.equal(ro2, ro) and torch.equal(rd2, rd)
    assert torch.equal(rows1, rows) and torch.equal(rows2, rows)
