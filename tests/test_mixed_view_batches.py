"""Mixed-camera ray batches: a view index per ray through the selection kernel (dn_select_rays_views), the in-kernel draw
(dn_select_rays_draw_views) and the camera gradient (dn_camera_grad_views), and what sits on them - _ops wrappers,
MultiViewRaySelector.select(view=(N,)), nerf.select_camera_rays(view_index=...), FusedTrainStep(draw_view="rays"), nerf.MultiPoseRefiner.

Yardsticks: the one-camera entry points on each view's subset (rows and targets bit for bit; per-view gradients to 1e-6: both are fp32
roundings of fp64 sums that differ only in order, one fp32 ulp = 1.2e-7 of the element at most), and float64 autograd of
oracle.nerf_oracle.get_ray_bundle per view at test_camera_gradients.GATE = 1e-5.  Tolerances in the project's norm,
max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES
from test_camera_gradients import GATE, NDC_F, NDC_H, NDC_NEAR, NDC_W, ndc_camera, oracle_grads_5arg, upstream
from test_input_gradients import POSE_XI, make_cfg, make_models, no_fallback

NEW_SYMBOLS = ("dn_select_rays_views", "dn_select_rays_draw_views", "dn_camera_grad_views_scratch_bytes", "dn_camera_grad_views")
SHAPES = ((7, 13), (45, 67))
SELECT_N = (1, 64, 65, 257)
POSES = (3, 9, 14)
V = 3


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
def world_cameras(h, w):
    """(E (3,4,4), K (3,3,3)) fp32 host tensors: poses 3, 9 and 14 of the synthetic scene; the intrinsics differ a little per view so
    that a row built with the wrong view's K is caught."""
    from nerf import synthetic as syn
    e = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES])
    k = torch.stack([torch.from_numpy(syn.intrinsic(h, w)).clone() for _ in POSES])
    for v in range(V):
        k[v, 0, 0] += 0.5 * v
        k[v, 0, 2] += 0.25 * v
        k[v, 1, 2] -= 0.125 * v
    return e, k


def ndc_cameras():
    """test_camera_gradients.ndc_camera and two small rotations of it (about x by 0.03 rad, about z by -0.04 rad): E (3,4,4), K (3,3)."""
    e0, k = ndc_camera()

    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        m = np.eye(4)
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return torch.from_numpy(m.astype(np.float32))
    return torch.stack([e0, e0 @ rot(0, 0.03), e0 @ rot(2, -0.04)]), k


def mixed_selection(n, total, seed=3, empty_view=None):
    """(view_index int32, pixel_index int64) of n rays: unsorted, interleaved views; pixel 5 under views 0 and 1, the last pixel twice
    under view 2 (n >= 4); then random pairs.  empty_view: that view gets no ray (its rays go to the next one)."""
    gen = torch.Generator().manual_seed(seed)
    views = [2, 0, 2, 1] + torch.randint(0, V, (n,), generator=gen).tolist()
    pixels = [total - 1, 5, total - 1, 5] + torch.randint(0, total, (n,), generator=gen).tolist()
    views, pixels = torch.tensor(views[:n], dtype=torch.int32), torch.tensor(pixels[:n], dtype=torch.int64)
    if empty_view is not None:
        views[views == empty_view] = (empty_view + 1) % V
    return views, pixels


def records(e, k, h, w, ndc_focal=None):
    from nerf import _ops
    return torch.stack([_ops.camera_record(e[v], k[v] if k.dim() == 3 else k, None, h, w, ndc_focal) for v in range(e.shape[0])])


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
    """DN_E_INVAL (-1000) with a message naming the entry point, before anything is launched or dereferenced (the device pointers
    are small integers)."""
    fake = ctypes.c_void_p(256)
    big = 1 << 24
    nan, inf = float("nan"), float("inf")

    def sel(h=8, w=8, cams=fake, nv=3, views=fake, pix=fake, n=4, images=None, channels=0, rays=fake, target=None, focal=0.0, near=1.0):
        return hiplib.dn_select_rays_views(h, w, cams, nv, views, 0.0, 1.0, pix, n, images, channels, rays, target, focal, near, None)
    for kw in (dict(cams=None), dict(views=None), dict(pix=None), dict(rays=None), dict(nv=0), dict(nv=-2), dict(h=0), dict(n=-1),
               dict(h=1 << 15, w=1 << 15, nv=2), dict(target=fake), dict(target=fake, images=fake, channels=2), dict(focal=-1.0),
               dict(focal=nan), dict(focal=inf), dict(near=nan)):
        assert sel(**kw) == -1000, kw
        assert b"dn_select_rays_views" in hiplib.dn_last_error(), kw
    assert sel(n=0) == 0

    def draw(h=8, w=8, cams=fake, nv=3, st=fake, n=4, images=None, channels=0, rays=fake, target=None, focal=0.0, near=1.0):
        return hiplib.dn_select_rays_draw_views(h, w, cams, nv, 0.0, 1.0, st, n, images, channels, rays, target, None, None, focal, near, None)
    for kw in (dict(cams=None), dict(st=None), dict(rays=None), dict(nv=0), dict(w=0), dict(n=0), dict(n=3 * 64 + 1),
               dict(h=1 << 15, w=1 << 15, nv=2), dict(target=fake), dict(focal=-60.0), dict(focal=nan), dict(near=inf)):
        assert draw(**kw) == -1000, kw
        assert b"dn_select_rays_draw_views" in hiplib.dn_last_error(), kw
    assert draw(n=3 * 64 + 1) == -1000 and b"without replacement" in hiplib.dn_last_error()
    assert draw(h=1 << 15, w=1 << 15, nv=2, n=1) == -1000 and b"too large" in hiplib.dn_last_error()

    def grad(h=8, w=8, cams=fake, nv=3, views=fake, pix=fake, n=4, g_ro=fake, s_ro=3, g_rd=fake, s_rd=3, g_vd=None, s_vd=0, focal=0.0,
             near=1.0, scratch=fake, nbytes=big, g_cams=fake):
        return hiplib.dn_camera_grad_views(h, w, cams, nv, views, pix, n, g_ro, s_ro, g_rd, s_rd, g_vd, s_vd, focal, near, scratch, nbytes,
                                           g_cams, None)
    need = hiplib.dn_camera_grad_views_scratch_bytes(4, 3)
    for kw in (dict(cams=None), dict(g_cams=None), dict(views=None), dict(pix=None), dict(nv=0), dict(nv=-1), dict(g_ro=None, g_rd=None),
               dict(s_ro=2), dict(s_rd=0), dict(g_vd=fake, s_vd=2), dict(scratch=None), dict(nbytes=need - 1), dict(nbytes=0),
               dict(scratch=ctypes.c_void_p(260)), dict(h=1 << 15, w=1 << 15, nv=2), dict(h=0), dict(n=-1), dict(focal=nan), dict(focal=inf),
               dict(focal=-1.0), dict(near=nan), dict(n=0, cams=None), dict(n=0, g_cams=None)):
        assert grad(**kw) == -1000, kw
        assert b"dn_camera_grad_views" in hiplib.dn_last_error(), kw
    assert grad(nbytes=need - 1) == -1000 and b"scratch" in hiplib.dn_last_error()
    assert grad(scratch=ctypes.c_void_p(260)) == -1000 and b"aligned" in hiplib.dn_last_error()
    assert grad(s_ro=2) == -1000 and b"stride" in hiplib.dn_last_error()


def test_scratch_size_is_a_function_of_n_and_views_alone(hiplib):
    ns, vs = (0, 1, 91, 256, 257, 3015, 4096, 160000, 1 << 40), (1, 2, 3, 20, 100)
    table = [[hiplib.dn_camera_grad_views_scratch_bytes(n, v) for v in vs] for n in ns]
    assert table == [[hiplib.dn_camera_grad_views_scratch_bytes(n, v) for v in vs] for n in ns]
    for row in table:
        assert row == sorted(row) and all(s >= 16 * 8 and s % 128 == 0 for s in row)      # monotone in V; >= one partial, also at n = 0
    for col in zip(*table):
        assert list(col) == sorted(col)                                                    # monotone in n
    assert table[-1] == table[-2]                                                          # the number of workgroups per view is capped
    assert [r[0] for r in table] == [hiplib.dn_camera_grad_scratch_bytes(n) for n in ns]   # one view: dn_camera_grad's


def test_fused_train_step_rejects_an_unknown_draw_view():
    import nerf
    with pytest.raises(ValueError, match="draw_view"):
        nerf.FusedTrainStep(None, None, None, None, None, None, None, 8, draw_view="nonsense")


def test_batched_entry_points_are_device_only():
    import nerf
    h, w = SHAPES[0]
    e, k = world_cameras(h, w)
    views, pix = mixed_selection(8, h * w)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix, view_index=views)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.MultiPoseRefiner(None, None, None, h, w, k[0], e, None, None, num_rays=4, lr=1e-3)


def test_mismatched_view_counts_raise():
    import nerf
    h, w = SHAPES[0]
    e, k = world_cameras(h, w)
    views, pix = mixed_selection(8, h * w)
    with pytest.raises(ValueError, match="intrinsics"):
        nerf.select_camera_rays(h, w, e, k[:2], 2.0, 6.0, pix, view_index=views)
    with pytest.raises(ValueError, match="images"):
        nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix, image=torch.zeros(2, h, w, 3), view_index=views)
    with pytest.raises(ValueError, match="images"):
        nerf.select_camera_rays(h, w, e, k[0], 2.0, 6.0, pix, image=torch.zeros(h, w, 3), view_index=views)
    with pytest.raises(ValueError, match=r"\(V,4,4\)"):
        nerf.select_camera_rays(h, w, e[0], k[0], 2.0, 6.0, pix, view_index=views)


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


def per_view_rows(fn, views, pix, n_cols=11):
    """fn(v, pixel subset) -> (rows, target) of the one-camera entry point, scattered back into batch order."""
    dev_ = pix.device
    rows = torch.full((pix.numel(), n_cols), float("nan"), device=dev_)
    target = torch.full((pix.numel(), 3), float("nan"), device=dev_)
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1)
        if idx.numel():
            r, t = fn(v, pix[idx].contiguous())
            rows[idx], target[idx] = r, t
    return rows, target


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("n", SELECT_N)
def test_selection_equals_the_one_camera_kernel_per_view(dev, h, w, n):
    """World-space rows and targets of an unsorted, interleaved batch (a pixel under two views, a pixel twice within a view):
    torch.equal to dn_select_rays_indirect on each view's subset; through MultiViewRaySelector.select(view=(N,)) as well."""
    import nerf
    from nerf import _ops
    e, k = world_cameras(h, w)
    cams = records(e, k, h, w).to(dev)
    images = torch.rand(V, h, w, 4, generator=torch.Generator().manual_seed(9)).to(dev)
    views, pix = [t.to(dev) for t in mixed_selection(n, h * w)]
    rows, target = _ops.select_rays_views(h, w, cams, views, 2.0, 6.0, pix, images)

    def one(v, sub):
        return _ops.select_rays_indirect(h, w, cams, torch.tensor(v, dtype=torch.int32, device=dev), 2.0, 6.0, sub, images)
    want_rows, want_target = per_view_rows(one, views, pix)
    assert torch.equal(rows, want_rows) and torch.equal(target, want_target)
    sel = nerf.MultiViewRaySelector(h, w, list(e), list(k), 2.0, 6.0, images=images, device=dev)
    rows2, target2 = sel.select(pix, view=views)
    assert torch.equal(rows2, rows) and torch.equal(target2, target)
    sel.view.fill_(1)                                            # a 0-dim view / None: today's call
    r1, _ = sel.select(pix)
    r1b, _ = sel.select(pix, view=torch.tensor(1, dtype=torch.int32, device=dev))
    assert torch.equal(r1, one(1, pix)[0]) and torch.equal(r1b, r1)
    none_rows, none_target = _ops.select_rays_views(h, w, cams, views, 2.0, 6.0, pix)
    assert none_target is None and torch.equal(none_rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SELECT_N)
def test_ndc_selection_equals_the_one_camera_ndc_kernel_per_view(dev, n):
    from nerf import _ops
    h, w = NDC_H, NDC_W
    e, k = ndc_cameras()
    cams = records(e, k, h, w).to(dev)
    images = torch.rand(V, h, w, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    views, pix = [t.to(dev) for t in mixed_selection(n, h * w, seed=4)]
    rows, target = _ops.select_rays_views(h, w, cams, views, 0.0, 1.0, pix, images, ndc_focal=NDC_F, ndc_near=NDC_NEAR)

    def one(v, sub):
        return _ops.select_rays_indirect_ndc(h, w, cams, torch.tensor(v, dtype=torch.int32, device=dev), 0.0, 1.0, sub, NDC_F, NDC_NEAR, images)
    want_rows, want_target = per_view_rows(one, views, pix)
    assert torch.equal(rows, want_rows) and torch.equal(target, want_target)
    world, _ = _ops.select_rays_views(h, w, cams, views, 0.0, 1.0, pix, images)
    assert not torch.equal(world[:, :6], rows[:, :6]) and torch.equal(world[:, 6:], rows[:, 6:])


def draw_cams(n_views, dev):
    cams = torch.zeros(n_views, 16, device=dev)
    cams[:, 0] = cams[:, 4] = cams[:, 8] = 1.0
    cams[:, 12], cams[:, 13], cams[:, 14] = 50.0, 3.0, 2.0
    cams[:, 9] = torch.arange(n_views, device=dev, dtype=torch.float32)          # the camera position tells the views apart
    return cams


@pytest.mark.gpu
def test_device_pair_draw_is_a_permutation_with_uniform_marginals(dev):
    """dn_select_rays_draw_views: the (view, pixel) pairs of an iteration are a keyed permutation of the V H W pixels of all views.  A
    full-length draw hits every pair once; the same (seed, iteration) gives the same draw, the next iteration another; the draw
    publishes nxt as cur and only the loss kernel advances nxt; with one view it is dn_select_rays_draw(view=0); rows and targets are
    dn_select_rays_views' on the drawn pairs; over 4,000 iterations of 256-ray draws at (5,20,15) no draw repeats a pair, the chi-square
    of the pair counts is within 5 sigma of its degrees of freedom and every view's share of the rays within 5 sigma of 1/5."""
    from nerf import _ops
    for (nv, h, w) in ((3, 4, 4), (3, 37, 29), (5, 20, 15)):
        cams = draw_cams(nv, dev)
        total = nv * h * w
        st = _ops.new_rng_state(11, dev)
        rays, _, pix, views = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, st, total, want_pixels=True)
        assert views.dtype == torch.int32 and pix.dtype == torch.int64
        assert int(views.min()) == 0 and int(views.max()) == nv - 1 and int(pix.min()) == 0 and int(pix.max()) == h * w - 1
        assert torch.equal(torch.sort(views.long() * (h * w) + pix)[0], torch.arange(total, device=dev))
        assert torch.equal(rays[:, 0], views.float())
        assert st.tolist()[2] == 0 and st.tolist()[3] == 0
        again = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, _ops.new_rng_state(11, dev), total, want_pixels=True)
        assert torch.equal(pix, again[2]) and torch.equal(views, again[3])
        other = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, _ops.new_rng_state(11, dev, first_iteration=1), total, want_pixels=True)
        assert not (torch.equal(pix, other[2]) and torch.equal(views, other[3]))
        st7 = _ops.new_rng_state(11, dev, first_iteration=7)
        st7[2] = 3                                                # cur is overwritten by the draw: nxt is what it reads
        _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, st7, 4)
        assert st7.tolist()[2:] == [7, 7]
    # one view: dn_select_rays_draw with view 0, bit for bit
    h, w, n = 37, 29, 300
    cams1, imgs1 = draw_cams(1, dev), torch.rand(1, h, w, 3, device=dev)
    a = _ops.select_rays_draw_views(h, w, cams1, 2.0, 6.0, _ops.new_rng_state(5, dev, 2), n, imgs1, want_pixels=True)
    b = _ops.select_rays_draw(h, w, cams1, torch.zeros((), dtype=torch.int32, device=dev), 2.0, 6.0, _ops.new_rng_state(5, dev, 2), n, imgs1,
                              want_pixels=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not bool(a[3].any())
    # marginals
    nv, h, w, n, iters = 5, 20, 15, 256, 4000
    total = nv * h * w
    cams, images = draw_cams(nv, dev), torch.rand(nv, h, w, 3, device=dev)
    counts = torch.zeros(total, dtype=torch.int64, device=dev)
    most = torch.zeros((), dtype=torch.int64, device=dev)
    st = _ops.new_rng_state(5, dev)
    dummy = torch.zeros(n, 3, device=dev)
    for it in range(iters):
        rays, target, pix, views = _ops.select_rays_draw_views(h, w, cams, 2.0, 6.0, st, n, images, want_pixels=True)
        if it < 3:
            ref_rays, ref_target = _ops.select_rays_views(h, w, cams, views, 2.0, 6.0, pix, images)
            assert torch.equal(rays, ref_rays) and torch.equal(target, ref_target)
        mine = torch.bincount(views.long() * (h * w) + pix, minlength=total)
        most = torch.maximum(most, mine.max())
        counts += mine
        _ops.mse2_loss(dummy, dummy, dummy, rng_state=st)          # what advances the iteration counter in a training loop
    assert st.tolist()[3] == iters and int(counts.sum()) == iters * n
    assert int(most) == 1                                          # no draw repeats a pair
    # sampling without replacement: variance of a pair's count = iters * p (1 - p), p = n / (V H W)
    p = n / total
    expect = iters * p
    chi2 = float(((counts.double() - expect) ** 2).sum() / (iters * p * (1 - p)))
    dof = total - 1
    print(f"pair draw: chi2 {chi2:.1f} for {dof} degrees of freedom (5 sigma: {5.0 * (2 * dof) ** 0.5:.1f})")
    assert abs(chi2 - dof) < 5.0 * (2 * dof) ** 0.5, (chi2, dof)
    # a view's rays per draw are hypergeometric (n out of V H W, H W of them in the view): variance n q (1 - q) (T - n) / (T - 1), q = 1/V
    q = 1.0 / nv
    sigma = (iters * n * q * (1 - q) * (total - n) / (total - 1)) ** 0.5 / (iters * n)
    share = counts.reshape(nv, h * w).sum(1).double() / (iters * n)
    print(f"pair draw: view shares {share.tolist()}, sigma {sigma:.2e}")
    assert float((share - q).abs().max()) < 5.0 * sigma, (share.tolist(), sigma)


def pull_back(cams_host, g_cams, e, k, h, w, ndc_focal=None):
    """(V,16) record gradients through the host record (camera_record) to dE (V,4,4), dK, d ndc_focal."""
    from nerf import _ops
    e_, k_ = e.clone().requires_grad_(True), k.clone().requires_grad_(True)
    f_ = None if ndc_focal is None else torch.tensor(float(ndc_focal), requires_grad=True)
    rec = torch.stack([_ops.camera_record(e_[v], k_[v] if k_.dim() == 3 else k_, None, h, w, f_) for v in range(e.shape[0])])
    assert torch.equal(rec.detach(), cams_host)
    (rec * g_cams).sum().backward()
    return (e_.grad, k_.grad) + (() if f_ is None else (f_.grad,))


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("n", SELECT_N)
@pytest.mark.parametrize("empty_view", [None, 1])
def test_camera_gradient_per_view_against_the_oracle_and_the_one_camera_kernel(dev, h, w, n, empty_view):
    """World-space rows, upstream gradients on all 11 columns: g_cams pulled through the host record to dE, dK per view against float64
    autograd of the oracle (1e-5); each g_cams[v] against dn_camera_grad on view v's subset (1e-6); a view without a ray: 16 exact zeros."""
    from nerf import _ops
    e, k = world_cameras(h, w)
    cams_host = records(e, k, h, w)
    cams = cams_host.to(dev)
    views, pix = mixed_selection(n, h * w, seed=6, empty_view=empty_view)
    g = upstream(n, 11, 60 + n)
    gd = g.to(dev)
    g_cams = _ops.camera_grad_views(h, w, cams, views.to(dev), pix.to(dev), n, gd[:, 0:3], gd[:, 3:6], gd[:, 8:11])
    assert g_cams.shape == (V, 16) and bool(torch.isfinite(g_cams).all())
    d_e, d_k = pull_back(cams_host, g_cams.cpu(), e, k, h, w)
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1)
        if idx.numel() == 0:
            assert v == empty_view or n < V + 1
            assert torch.equal(g_cams[v], torch.zeros(16, device=dev)), v
            continue
        sub = gd[idx.to(dev)].contiguous()
        one = _ops.camera_grad(h, w, cams[v].contiguous(), pix[idx].to(dev), idx.numel(), sub[:, 0:3], sub[:, 3:6], sub[:, 8:11])
        err = rel_err(C(g_cams[v]), C(one))
        want = oracle_grads_5arg(h, w, e[v], k[v], pix[idx], g[idx, 0:3], g[idx, 3:6], g[idx, 8:11])
        errs = [rel_err(d_e[v].numpy(), want[0].numpy()), rel_err(d_k[v].numpy(), want[1].numpy())]
        print(f"{h}x{w} N={n} view {v} ({idx.numel()} rays): vs dn_camera_grad {err:.2e}, vs oracle (E, K) {errs[0]:.2e}, {errs[1]:.2e}")
        assert err <= 1e-6, (v, err)
        if bool(g[idx].any()):
            assert max(errs) <= GATE, (v, errs)
    if empty_view is not None and n > 1:
        assert not bool((views == empty_view).any()) and not bool(g_cams[empty_view].any())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SELECT_N)
def test_ndc_camera_gradient_per_view_against_the_oracle_and_the_one_camera_kernel(dev, n):
    """NDC rows: dE, dK per view and the per-view shares of d ndc_focal (slot 15) against the oracle; g_cams[v] against dn_camera_grad."""
    from nerf import _ops
    h, w = NDC_H, NDC_W
    e, k = ndc_cameras()
    cams_host = records(e, k, h, w, NDC_F)
    cams = cams_host.to(dev)
    views, pix = mixed_selection(n, h * w, seed=7)
    g = upstream(n, 11, 70 + n)
    gd = g.to(dev)
    g_cams = _ops.camera_grad_views(h, w, cams, views.to(dev), pix.to(dev), n, gd[:, 0:3], gd[:, 3:6], gd[:, 8:11], NDC_F, NDC_NEAR)
    host = g_cams.cpu()
    d_e = pull_back(cams_host, host, e, k, h, w, NDC_F)[0]
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1)
        if idx.numel() == 0:
            assert torch.equal(host[v], torch.zeros(16))
            continue
        sub = gd[idx.to(dev)].contiguous()
        one = _ops.camera_grad(h, w, cams[v].contiguous(), pix[idx].to(dev), idx.numel(), sub[:, 0:3], sub[:, 3:6], sub[:, 8:11], NDC_F, NDC_NEAR)
        err = rel_err(C(g_cams[v]), C(one))
        want = oracle_grads_5arg(h, w, e[v], k, pix[idx], g[idx, 0:3], g[idx, 3:6], g[idx, 8:11], ndc_focal=NDC_F)
        # dK is shared by the views: view v's share is the pull-back of row v alone
        one_hot = torch.zeros_like(host)
        one_hot[v] = host[v]
        share = pull_back(cams_host, one_hot, e, k, h, w, NDC_F)
        errs = [rel_err(d_e[v].numpy(), want[0].numpy()), rel_err(share[1].numpy(), want[1].numpy()), rel_err(share[2].numpy(), want[2].numpy())]
        print(f"NDC N={n} view {v} ({idx.numel()} rays): vs dn_camera_grad {err:.2e}, vs oracle (E, K, ndc_focal) " + ", ".join(f"{x:.2e}" for x in errs))
        assert err <= 1e-6, (v, err)
        if bool(g[idx].any()):
            assert max(errs) <= GATE, (v, errs)


@pytest.mark.gpu
def test_camera_grad_views_is_bit_reproducible_and_writes_zeros_for_no_rays(dev, hiplib):
    from nerf import _ops
    h, w = SHAPES[1]
    e, k = ndc_cameras()
    cams = records(e, k, h, w).to(dev)
    n = 257
    views, pix = [t.to(dev) for t in mixed_selection(n, h * w, seed=8)]
    g = upstream(n, 11, 50).to(dev)
    for focal in (0.0, NDC_F):
        a = _ops.camera_grad_views(h, w, cams, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, NDC_NEAR)
        b = _ops.camera_grad_views(h, w, cams, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, NDC_NEAR)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)
        assert bool((a[:, 15] != 0).all()) == (focal > 0.0)
    out = torch.full((V, 16), 7.0, device=dev)
    scratch = torch.empty(hiplib.dn_camera_grad_views_scratch_bytes(0, V) // 8, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = hiplib.dn_camera_grad_views(h, w, p(cams), V, p(views), p(pix), 0, p(g), 11, p(g), 11, None, 0, 0.0, 1.0, p(scratch), scratch.numel() * 8,
                                     p(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and out.shape == (V, 16) and torch.equal(out, torch.zeros(V, 16, device=dev))
    none = _ops.camera_grad_views(h, w, cams, views[:0], pix[:0], 0, g[:0, 0:3], g[:0, 3:6], g[:0, 8:11])
    assert none.shape == (V, 16) and torch.equal(none, torch.zeros(V, 16, device=dev))


@pytest.mark.gpu
def test_select_camera_rays_with_a_view_index(dev):
    """nerf.select_camera_rays(view_index=...): rows and targets torch.equal to the one-camera call per view; dE (V,4,4) and dK (V,3,3)
    against the oracle per view; a shared (3,3) intrinsic receives the sum; no grad: the forward alone, equal rows."""
    import nerf
    h, w = SHAPES[1]
    n = 257
    e32, k32 = world_cameras(h, w)
    views, pix = mixed_selection(n, h * w, seed=12)
    images = torch.rand(V, h, w, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    g = upstream(n, 11, 80)
    e, k = e32.to(dev).requires_grad_(True), k32.to(dev).requires_grad_(True)
    rows, target = nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix.to(dev), image=images, view_index=views.to(dev))
    assert rows.grad_fn is not None and not target.requires_grad

    def one(v, sub):
        return nerf.select_camera_rays(h, w, e32[v].to(dev), k32[v].to(dev), 2.0, 6.0, sub, image=images[v])
    want_rows, want_target = per_view_rows(one, views.to(dev), pix.to(dev))
    assert torch.equal(rows, want_rows) and torch.equal(target, want_target)
    (rows * g.to(dev)).sum().backward()
    assert e.grad.shape == (V, 4, 4) and k.grad.shape == (V, 3, 3) and e.grad.is_cuda
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1)
        want = oracle_grads_5arg(h, w, e32[v], k32[v], pix[idx], g[idx, 0:3], g[idx, 3:6], g[idx, 8:11])
        errs = [rel_err(C(e.grad[v]), want[0].numpy()), rel_err(C(k.grad[v]), want[1].numpy())]
        assert max(errs) <= GATE, (v, errs)
    # a shared intrinsic: the sum over the views of what each view's K would get
    ks = k32[0].to(dev).requires_grad_(True)
    rows_s, _ = nerf.select_camera_rays(h, w, e32.to(dev), ks, 2.0, 6.0, pix.to(dev), view_index=views.to(dev))
    (rows_s * g.to(dev)).sum().backward()
    total = 0
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1)
        total = total + oracle_grads_5arg(h, w, e32[v], k32[0], pix[idx], g[idx, 0:3], g[idx, 3:6], g[idx, 8:11])[1]
    assert rel_err(C(ks.grad), total.numpy()) <= GATE
    with torch.no_grad():
        rows1, _ = nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix.to(dev), view_index=views.to(dev))
    rows2, _ = nerf.select_camera_rays(h, w, e.detach(), k.detach(), 2.0, 6.0, pix.to(dev), view_index=views.to(dev))
    assert rows1.grad_fn is None and rows2.grad_fn is None and torch.equal(rows1, rows) and torch.equal(rows2, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,luminance", [("fp32", False), ("bf16-s8", False), ("fp32", True)])
def test_fused_train_step_on_mixed_view_draws_equals_the_autograd_path(dev, precision, luminance, monkeypatch):
    """test_hip_parity.test_fused_train_step_equals_the_autograd_path_on_the_same_draws with three cameras and draw_view="rays": the draw
    holds more than one view; the six maps bit for bit; loss, MSEs and parameter gradients within that test's gates; the counter
    advances once per step; then three GraphedTrainStep steps replay without a fallback and keep changing the loss."""
    import nerf
    from nerf import _ops, parallel, synthetic as syn
    h, w, n = 40, 52, 512
    mkw = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    cfg = make_cfg(dict(num_coarse=64, num_fine=64, near=2.0, far=6.0, perturb=True, noise_std=0.2, white_background=True), chunksize=4096)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    poses = [torch.from_numpy(syn.scene_pose(k)) for k in POSES]
    kmat = torch.from_numpy(syn.intrinsic(h, w))
    images = torch.rand(V, h, w, 3, device=dev)
    nerf.set_precision(precision)
    try:
        def models():
            return make_models(mkw, syn.synth_state_dict(21, sigma_bias=-1.0, **mkw), syn.synth_state_dict(22, sigma_bias=-1.0, **mkw), dev)
        sel = nerf.MultiViewRaySelector(h, w, poses, [kmat] * V, 2.0, 6.0, images=images, device=dev)
        mc, mf = models()
        bucket = parallel.FlatGradBucket([mc, mf])
        step = nerf.FusedTrainStep(mc, mf, sel, cfg, bucket, ex, ed, n, seed=77, luminance=luminance, first_iteration=5, draw_view="rays")
        peek = _ops.new_rng_state(77, dev, 5)
        rays_ref, target_ref, pix, views = _ops.select_rays_draw_views(h, w, sel.cams, 2.0, 6.0, peek, n, images, want_pixels=True)
        assert views.unique().numel() > 1
        draws = [_ops.rng_fill(peek, 0, (n, 64)), _ops.rng_fill(peek, 1, (n, 64), normal=True), _ops.rng_fill(peek, 2, (n, 64)),
                 _ops.rng_fill(peek, 3, (n, 128), normal=True)]
        loss3 = step.forward_backward()
        assert step.rng_state.tolist()[2:] == [5, 6]
        assert torch.equal(step._keep[3], rays_ref) and torch.equal(step._keep[4], target_ref)
        grads_fused = [p.grad.detach().clone() for p in bucket.params]
        maps_fused = step._keep[2]
        mc2, mf2 = models()
        q_rand, q_randn = [draws[0], draws[2]], [draws[1], draws[3]]
        monkeypatch.setattr(torch, "rand", lambda *a, **k: q_rand.pop(0))
        monkeypatch.setattr(torch, "randn", lambda *a, **k: q_randn.pop(0))
        out = nerf.predict_and_render_radiance(rays_ref, mc2, mf2, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=None)
        monkeypatch.undo()
        assert not q_rand and not q_randn
        for a, b in zip(maps_fused[:6], out[:6]):
            assert torch.equal(a, b.detach())

        def head(t):
            return (0.299 * t[..., 0] + 0.587 * t[..., 1] + 0.114 * t[..., 2]) if luminance else t
        mse_c, mse_f = nerf.img2mse(head(out[0]), head(target_ref)), nerf.img2mse(head(out[3]), head(target_ref))
        (mse_c + mse_f).backward()
        got = loss3.tolist()
        assert abs(got[1] - mse_c.item()) < 1e-5 * abs(mse_c.item()) and abs(got[2] - mse_f.item()) < 1e-5 * abs(mse_f.item())
        assert abs(got[0] - (mse_c + mse_f).item()) < 1e-5 * abs((mse_c + mse_f).item())
        tol = 1e-4 if precision == "fp32" else 2e-3
        for g, p in zip(grads_fused, list(mc2.parameters()) + list(mf2.parameters())):
            assert rel_err(C(g), C(p.grad)) < tol, (tuple(g.shape), rel_err(C(g), C(p.grad)))
        step.forward_backward()
        assert step.rng_state.tolist()[2:] == [6, 7]
        # graph capture and replay of the mixed-view iteration
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1)
        losses = []
        for _ in range(3):
            graphed.step()
            losses.append(float(step.loss3[0]))
        torch.cuda.synchronize()
        assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
        assert step.rng_state.tolist()[3] == 10 and all(np.isfinite(losses)) and len(set(losses)) == 3, losses
        peek = _ops.new_rng_state(77, dev, 10)
        rays_next, _ = _ops.select_rays_draw_views(h, w, sel.cams, 2.0, 6.0, peek, n, sel.images)
        graphed.step()                                    # a replay draws exactly what the eager draw of that iteration would
        torch.cuda.synchronize()
        assert torch.equal(step._keep[3], rays_next)
    finally:
        nerf.set_precision("fp32")


# ---- refinement -----------------------------------------------------------------------------------------------------------------------
RH = RW = 400


@pytest.fixture(scope="module")
def lego(dev):
    """(coarse, fine) lego-shaped networks with frozen parameters, the encoders and the render options (as test_pose_refinement.lego)."""
    import nerf
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    return mc, mf, nerf.get_embedding_function(10), nerf.get_embedding_function(4), make_cfg(rkw), rkw


def refinement_problem():
    """Poses 3, 9, 14 at 400 x 400, one intrinsic, 192 fixed (view, pixel) pairs, a fixed random target per ray, a non-zero xi per view."""
    from nerf import synthetic as syn
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES])
    k = torch.from_numpy(syn.intrinsic(RH, RW))
    gen = torch.Generator().manual_seed(31)
    views = torch.randint(0, V, (192,), generator=gen).to(torch.int32)
    pix = torch.randint(0, RH * RW, (192,), generator=gen)
    target = torch.rand(192, 3, generator=gen)
    xi = torch.tensor([POSE_XI, [-x for x in POSE_XI], [0.5 * x for x in POSE_XI]], dtype=torch.float64)
    return e0, k, views, pix, target, xi


@pytest.mark.gpu
def test_batched_pose_gradient_equals_the_one_camera_chain_per_view(dev, lego, monkeypatch):
    """xi (V,6) -> E_v = se3_exp(xi_v) @ E0_v -> select_camera_rays(view_index) -> predict_and_render_radiance -> sum-form coarse + fine
    squared error -> dL/dxi (V,6): row v equals dL/dxi_v of the one-camera chain on camera v's rays to 1e-5 (the rows are bit-identical, so
    only the order of the camera gradient's sums differs)."""
    import nerf
    mc, mf, ex, ed, cfg, rkw = lego
    e0, k, views, pix, target, xi0 = refinement_problem()
    views_d, pix_d, tgt = views.to(dev), pix.to(dev), target.to(dev)

    def loss_of(rows, t):
        out = nerf.predict_and_render_radiance(rows, mc, mf, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
        return ((out[0] - t) ** 2).sum() + ((out[3] - t) ** 2).sum()
    xi = xi0.clone().requires_grad_(True)
    with no_fallback(monkeypatch):
        e_all = torch.stack([nerf.se3_exp(xi[v]) @ e0[v].double() for v in range(V)])
        rows, _ = nerf.select_camera_rays(RH, RW, e_all, k, rkw["near"], rkw["far"], pix_d, view_index=views_d)
        assert rows.grad_fn is not None
        loss_of(rows, tgt).backward()
    batched = xi.grad.clone()
    assert batched.shape == (V, 6)
    for v in range(V):
        idx = torch.nonzero(views == v).reshape(-1).to(dev)
        xv = xi0[v].clone().requires_grad_(True)
        rows_v, _ = nerf.select_camera_rays(RH, RW, nerf.se3_exp(xv) @ e0[v].double(), k, rkw["near"], rkw["far"], pix_d[idx].contiguous())
        assert torch.equal(rows_v, rows.detach()[idx])
        loss_of(rows_v, tgt[idx]).backward()
        err = rel_err(batched[v].numpy(), xv.grad.numpy())
        print(f"dL/dxi view {v} ({idx.numel()} rays): batched vs one-camera chain {err:.2e}; {xv.grad.tolist()}")
        assert float(xv.grad.abs().max()) > 0 and err <= 1e-5, (v, err)


def _multi_refiner(dev, lego, seed, num_rays=192):
    import nerf
    mc, mf, ex, ed, cfg, _ = lego
    e0, k = refinement_problem()[:2]
    return nerf.MultiPoseRefiner(mc, mf, cfg, RH, RW, k.to(dev), e0.to(dev), ex, ed, num_rays=num_rays, lr=1e-3, seed=seed)


@pytest.mark.gpu
def test_multi_pose_refiner_is_reproducible_and_leaves_the_networks_alone(dev, lego):
    """Two refiners with one seed end three steps with bit-identical xi (V,6); another seed draws other pairs; the pairs are distinct;
    extrinsics() is (V,4,4) and follows xi; the networks' requires_grad flags (here: mixed) and .grad are untouched."""
    import nerf
    mc, mf = lego[0], lego[1]
    e0 = refinement_problem()[0]
    params = list(mc.parameters()) + list(mf.parameters())
    flags = [i % 2 == 0 for i in range(len(params))]
    for p, flag in zip(params, flags):
        p.requires_grad_(flag)
    try:
        images = torch.rand(V, RH, RW, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        a, b = _multi_refiner(dev, lego, seed=4), _multi_refiner(dev, lego, seed=4)
        for _ in range(3):
            la, lb = a.step(images), b.step(images)
            assert la.dim() == 0 and not la.requires_grad and torch.equal(la, lb)
        assert a.xi.shape == (V, 6) and a.xi.dtype == torch.float64 and not a.xi.is_cuda
        assert torch.equal(a.xi.detach(), b.xi.detach()) and bool((a.xi.detach().abs().amax(dim=1) > 0).all())
        assert a.last_grad.shape == (V, 6)
        assert [p.requires_grad for p in params] == flags and all(p.grad is None for p in params)
        est = a.extrinsics()
        assert est.shape == (V, 4, 4) and est.is_cuda and not est.requires_grad
        want = torch.stack([nerf.se3_exp(a.xi.detach()[v]) @ e0[v].double() for v in range(V)])
        assert rel_err(est.cpu().numpy(), want.numpy()) <= 1e-6
        va, pa = _multi_refiner(dev, lego, seed=4).draw_pairs()
        vc, pc = _multi_refiner(dev, lego, seed=5).draw_pairs()
        assert va.dtype == torch.int32 and pa.dtype == torch.int64 and va.numel() == 192
        assert (va.long() * (RH * RW) + pa).unique().numel() == 192 and va.unique().numel() > 1
        assert not (torch.equal(va, vc) and torch.equal(pa, pc))
        sel = nerf.MultiViewRaySelector(RH, RW, list(e0), [refinement_problem()[1]] * V, 2.0, 6.0, device=dev)
        vs, ps = sel.random_pairs(100, generator=torch.Generator(device=dev).manual_seed(1))
        assert vs.dtype == torch.int32 and ps.dtype == torch.int64 and (vs.long() * (RH * RW) + ps).unique().numel() == 100
        assert int(vs.min()) >= 0 and int(vs.max()) < V and int(ps.min()) >= 0 and int(ps.max()) < RH * RW
    finally:
        for p in params:
            p.requires_grad_(False)
