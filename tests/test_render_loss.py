"""The general loss head dn_render_loss - weighted colour terms plus a masked depth term, value and upstream gradients in one launch -
and its consumers: _ops.render_loss, nerf.render_loss under autograd, nerf.FusedTrainStep / GraphedTrainStep and nerf.FusedPoseStep
with depth_images / loss_weights / depth_weights.

Yardsticks: a float64 torch restatement of the head written here (loss6[0:5] and every gradient tensor at 1e-5 max|ref| - the project's
gate for fp32 gradient kernels against float64: each element is a handful of fp32 roundings, each sum at most 12288 terms added in a
lane-strided tree; the valid-ray count exactly; invalid-ray gradients exactly +0); dn_mse2_loss bit for bit where the head restates it;
the chain of the pinned pieces bit for bit for the fused steps; the stage-by-stage autograd route at test_fused_pose_step's 1e-5.
Tolerances in the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from test_fused_pose_step import XI_START, make_step, world_problem
from test_input_gradients import make_cfg, make_models, no_fallback
from test_mixed_view_batches import V

INF = float("inf")
LO, HI = 0.5, 5.0        # both exact in fp32


def C(t):
    return t.detach().cpu().numpy()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_loss_head_and_the_abi_is_still_2():
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    assert "dn_render_loss" in declared and "dn_mse2_loss" in declared
    assert "#define DN_ABI_VERSION 2" in header


def test_binding_resolves_the_symbol_and_the_entry_point_validates_before_gpu_work():
    from nerf import _hip
    if not _hip.available():
        pytest.skip("libdexnerf_hip.so is not built")
    lib = _hip.lib()
    assert "dn_render_loss" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "dn_render_loss")
    assert lib.dn_render_loss.argtypes is not None and len(lib.dn_render_loss.argtypes) == 25 and lib.dn_abi_version() == 2
    fake = ctypes.c_void_p(1024)

    def call(rgb_c=fake, target=fake, depth_c=fake, depth_src=None, pix=None, views=None, view=None, hw=35, n=4, w=(1.0, 1.0, 0.0, 0.0),
             lo=0.0, hi=INF, loss6=fake):
        return lib.dn_render_loss(rgb_c, fake, target, depth_c, fake, depth_src, pix, views, view, hw, n, 0, *w, lo, hi, loss6, fake, fake, fake,
                                  fake, None, None)
    for kw in (dict(rgb_c=None), dict(target=None), dict(loss6=None), dict(n=0), dict(n=-3), dict(w=(float("nan"), 1.0, 0.0, 0.0)),
               dict(w=(1.0, 1.0, INF, 0.0)), dict(depth_src=fake, depth_c=None), dict(depth_src=fake, lo=float("nan")),
               dict(depth_src=fake, hi=float("nan")), dict(depth_src=fake, pix=fake, hw=0), dict(pix=fake), dict(views=fake), dict(view=fake),
               dict(depth_src=fake, views=fake), dict(depth_src=fake, view=fake), dict(depth_src=fake, n=(1 << 24) + 1)):
        assert call(**kw) == -1000, kw
        assert b"dn_render_loss" in lib.dn_last_error(), kw


def test_fused_steps_refuse_loss_head_settings_they_cannot_honour():
    import nerf
    from nerf import synthetic as syn
    h = w = 8
    cfg = make_cfg(dict(num_coarse=16, num_fine=16, near=2.0, far=6.0))
    depth = torch.ones(V, h, w)
    sel = types.SimpleNamespace(cams=torch.zeros(V, 16), height=h, width=w)

    def train(**kw):
        return nerf.FusedTrainStep(None, None, sel, cfg, None, None, None, 16, **kw)
    with pytest.raises(ValueError, match="draw_view"):
        train(depth_images=depth, depth_weights=(0.1, 0.1), draw_view=True)
    for weights in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="loss_weights"):
            train(loss_weights=weights)
    with pytest.raises(ValueError, match="need depth_images"):
        train(depth_weights=(0.1, 0.1))
    with pytest.raises(ValueError, match="depth_weights"):
        train(depth_images=depth, depth_weights=(0.1, -0.1))
    with pytest.raises(ValueError, match=r"\(V,H,W\)"):
        train(depth_images=depth[0], depth_weights=(0.1, 0.1))
    with pytest.raises(ValueError, match="depth_images of shape"):
        train(depth_images=depth[:, :4], depth_weights=(0.1, 0.1), draw_view="rays")
    with pytest.raises(ValueError, match="pairs"):
        train(depth_images=depth, depth_weights=(0.1,))
    ndc = make_cfg(dict(num_coarse=16, num_fine=16, near=0.0, far=1.0))
    ndc.dataset.no_ndc = False
    with pytest.raises(ValueError, match="NDC"):
        nerf.FusedTrainStep(None, None, sel, ndc, None, None, None, 16, ndc_focal=20.0, depth_images=depth, depth_weights=(0.1, 0.1), draw_view="rays")

    e = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in (3, 9, 14)])
    k = torch.from_numpy(syn.intrinsic(h, w))
    images = torch.zeros(V, h, w, 3)

    def pose(**kw):
        return nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3, **kw)
    with pytest.raises(ValueError, match="need depth_images"):
        pose(depth_weights=(0.0, 0.1))
    with pytest.raises(ValueError, match="every loss weight is zero"):
        pose(loss_weights=(0.0, 0.0))
    with pytest.raises(ValueError, match="NDC"):
        pose(depth_images=depth, depth_weights=(0.0, 0.1), ndc_focal=20.0)
    with pytest.raises(ValueError, match="depth_images of shape"):
        pose(depth_images=depth[:2], depth_weights=(0.0, 0.1))
    with pytest.raises(ValueError, match="loss_weights"):
        pose(loss_weights=(-1.0, 1.0))
    with pytest.raises(RuntimeError, match="ROCm device only"):      # a fine-only loss is a valid setting: the next check is the device one
        pose(loss_weights=(0.0, 1.0))


def test_trainer_refuses_a_depth_weight_on_llff_captures(capsys):
    import train_dexnerf
    with pytest.raises(SystemExit):
        train_dexnerf.main(["--llff", "/nonexistent", "--depth-weight", "0.1"])
    assert "depth" in capsys.readouterr().err


# ---- GPU: the head alone --------------------------------------------------------------------------------------------------------------
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
    nerf.set_render_policy("bf16")          # (as test_fused_pose_step, whose shapes and autograd route the pose tests here reuse)
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def head_inputs(n, mask, seed=0):
    """Host fp32 tensors of a head call: maps, targets, and target depths with the mask case worked in - 'all' valid, 'none', 'last'
    (exactly one valid ray, at the last index), 'junk' (about a third invalid: NaN, 0 = the exclusive lower bound, and values past HI)."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    rgb_c, rgb_f, target = (torch.rand(n, 3, generator=gen) for _ in range(3))
    depth_c, depth_f = (2.0 + 2.0 * torch.rand(n, generator=gen) for _ in range(2))
    d = 1.0 + 3.5 * torch.rand(n, generator=gen)            # inside (LO, HI)
    if mask == "none":
        d = torch.where(torch.arange(n) % 2 == 0, torch.full((n,), float("nan")), torch.zeros(n))
    elif mask == "last":
        d[:-1] = torch.tensor([float("nan"), 0.0, HI, 7.0, LO, -1.0, INF])[torch.arange(n - 1) % 7]
    elif mask == "junk":
        bad = torch.rand(n, generator=gen) < 0.35
        junk = torch.tensor([float("nan"), 0.0, HI + 0.25])[torch.arange(n) % 3]
        d = torch.where(bad, junk, d)
    else:
        assert mask == "all"
    return rgb_c, rgb_f, target, depth_c, depth_f, d


def head64(rgb_c, rgb_f, target, depth_c, depth_f, d, weights, depth_weights, lo, hi, luminance):
    """float64 restatement of the head, differentiable in the maps: (loss, [loss, mse_c, mse_f, D_c, D_f, M], valid mask)."""
    def col(t):
        return 0.299 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2] if luminance else t
    zero = torch.zeros((), dtype=torch.float64, device=rgb_c.device)
    mse_c = ((col(rgb_c) - col(target)) ** 2).mean()
    mse_f = ((col(rgb_f) - col(target)) ** 2).mean() if rgb_f is not None else zero
    loss = weights[0] * mse_c + weights[1] * mse_f
    d_c = d_f = zero
    m = 0
    valid = None
    if d is not None:
        valid = (d > lo) & (d < hi)
        m = int(valid.sum())
        safe = torch.where(valid, d, torch.zeros_like(d))

        def term(depth):
            return (torch.where(valid, depth - safe, torch.zeros_like(d)) ** 2).sum() / max(m, 1)
        d_c = term(depth_c)
        d_f = term(depth_f) if depth_f is not None else zero
        loss = loss + depth_weights[0] * d_c + depth_weights[1] * d_f
    return loss, torch.stack([loss, mse_c, mse_f, d_c, d_f, torch.tensor(float(m), dtype=torch.float64, device=rgb_c.device)]), valid


def check_head(dev, n, mask, luminance=False, weights=(0.7, 1.3), depth_weights=(0.1, 0.25), fine=True, what=""):
    from nerf import _ops
    host = head_inputs(n, mask)
    rgb_c, rgb_f, target, depth_c, depth_f, d = (t.to(dev) for t in host)
    if not fine:
        rgb_f = depth_f = None
    got = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, d, weights=weights, depth_weights=depth_weights, depth_range=(LO, HI),
                           luminance=luminance)
    again = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, d, weights=weights, depth_weights=depth_weights, depth_range=(LO, HI),
                             luminance=luminance)
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)                     # two calls: the same bits
    leaves = [None if t is None else t.double().requires_grad_(True) for t in (rgb_c, rgb_f, depth_c, depth_f)]
    loss, ref6, valid = head64(leaves[0], leaves[1], target.double(), leaves[2], leaves[3], d.double(), weights, depth_weights, LO, HI, luminance)
    loss.backward()
    loss6, grads = got[0], got[1:]
    m = int(valid.sum())
    assert {"all": m == n, "none": m == 0, "last": m == 1 and bool(valid[-1]), "junk": 0 < m < n}[mask]
    assert float(loss6[5]) == float(m)                                           # exact
    assert bool(torch.isfinite(loss6).all()) and all(g is None or bool(torch.isfinite(g).all()) for g in grads)
    errs = {"loss6": rel_err(C(loss6[:5]), C(ref6[:5]))}
    for name, g, leaf in zip(("g_rgb_c", "g_rgb_f", "g_depth_c", "g_depth_f"), grads, leaves):
        assert (g is None) == (leaf is None), name
        if g is not None:
            want = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            errs[name] = rel_err(C(g), C(want))
    print(f"head n={n} mask={mask} lum={luminance} {what}: M={m} loss6 {[f'{v:.6g}' for v in loss6.tolist()]} errors",
          {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs
    for g, weight in zip(grads[2:], depth_weights):
        if g is not None:
            assert bool((g[~valid] == 0).all()) and not bool(torch.signbit(g[~valid]).any())      # exactly +0 on invalid rays
            assert m == 0 or weight == 0.0 or float(g[valid].abs().max()) > 0
    if m == 0:
        assert float(loss6[3]) == 0.0 and float(loss6[4]) == 0.0
    return got, (rgb_c, rgb_f, target, depth_c, depth_f, d), valid


HEAD_CASES = [(1, "all"), (1, "none"), (63, "none"), (63, "junk"), (64, "last"), (64, "all"), (65, "junk"), (65, "last"), (1023, "all"),
              (1023, "junk"), (1025, "last"), (1025, "none"), (1025, "junk"), (4096, "junk"), (4096, "all"), (4096, "last")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,mask", HEAD_CASES)
def test_head_against_float64(dev, n, mask):
    check_head(dev, n, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("n,mask", [(65, "junk"), (1025, "last"), (4096, "all")])
def test_head_luminance_form_against_float64(dev, n, mask):
    check_head(dev, n, mask, luminance=True)


@pytest.mark.gpu
def test_head_coarse_only_and_zero_depth_weights(dev):
    check_head(dev, 257, "junk", fine=False, what="coarse only")
    check_head(dev, 257, "junk", depth_weights=(0.0, 0.0), what="zero depth weights")      # D_c, D_f and M are still reported
    check_head(dev, 257, "junk", weights=(0.0, 1.0), depth_weights=(0.0, 0.1), what="fine only")


@pytest.mark.gpu
@pytest.mark.parametrize("n,mask", [(65, "junk"), (1025, "none"), (1025, "last"), (4096, "junk")])
def test_values_in_invalid_slots_change_no_output(dev, n, mask):
    """NaN, 0 and out-of-range values in the invalid slots - of the target depth and of the rendered depths - are replaced by other
    invalid values: every output keeps its bits."""
    from nerf import _ops
    got, (rgb_c, rgb_f, target, depth_c, depth_f, d), valid = check_head(dev, n, mask)
    other = torch.tensor([-2.0, INF, HI, LO, 1e30, -INF, 0.0], device=dev)[torch.arange(n, device=dev) % 7]
    d2 = torch.where(valid, d, other)
    assert bool(torch.isnan(d[~valid]).any()) and bool((d[~valid] == 0).any()) and not torch.equal(d2[~valid], d[~valid])
    depth_c2 = torch.where(valid, depth_c, torch.full_like(depth_c, float("nan")))
    depth_f2 = torch.where(valid, depth_f, torch.full_like(depth_f, INF))
    kw = dict(weights=(0.7, 1.3), depth_weights=(0.1, 0.25), depth_range=(LO, HI))
    for dc, df, dd in ((depth_c, depth_f, d2), (depth_c2, depth_f2, d), (depth_c2, depth_f2, d2)):
        for a, b in zip(got, _ops.render_loss(rgb_c, rgb_f, target, dc, df, dd, **kw)):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1025])
def test_gathered_depth_targets_equal_direct_ones_bit_for_bit(dev, n):
    """depth_src (V, H W) gathered inside the kernel at (view, pixel_index) against the same values gathered by torch and handed over
    as an (N) array: a view per ray, one view as a device scalar, and neither (view 0).  V = 3, H W = 35 (as (3,5,7) maps)."""
    from nerf import _ops
    n_views, hw = 3, 35
    gen = torch.Generator().manual_seed(n)
    maps = 1.0 + 3.5 * torch.rand(n_views, 5, 7, generator=gen)
    maps.view(-1)[::4] = torch.tensor([float("nan"), 0.0, 6.0])[torch.arange(len(maps.view(-1)[::4])) % 3]
    maps = maps.to(dev)
    pix = torch.randint(0, hw, (n,), generator=gen).to(dev)
    views = torch.randint(0, n_views, (n,), generator=gen).to(torch.int32).to(dev)
    pix[-1], views[-1] = hw - 1, n_views - 1                                                     # the last element of the maps is reachable
    one = torch.tensor(2, dtype=torch.int32, device=dev)
    rgb_c, rgb_f, target, depth_c, depth_f, _ = (t.to(dev) for t in head_inputs(n, "all", seed=1))
    kw = dict(weights=(0.7, 1.3), depth_weights=(0.1, 0.25), depth_range=(LO, HI))
    flat = maps.reshape(n_views, hw)
    for what, extra, direct in (("view per ray", dict(view_index=views), flat[views.long(), pix]), ("view scalar", dict(view=one), flat[2, pix]),
                                ("view 0", dict(), flat[0, pix])):
        want = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, direct.contiguous(), **kw)
        got = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, maps, pixel_index=pix, **extra, **kw)
        m = float(want[0][5])
        assert 0 < m < n, (what, m)
        for a, b in zip(got, want):
            assert torch.equal(a, b), what


@pytest.mark.gpu
@pytest.mark.parametrize("luminance", [False, True])
@pytest.mark.parametrize("n", [65, 4096])
def test_unit_weights_without_depth_equal_mse2_loss_bit_for_bit(dev, n, luminance):
    from nerf import _ops
    rgb_c, rgb_f, target, depth_c, depth_f, _ = (t.to(dev) for t in head_inputs(n, "all", seed=2))
    st_a, st_b = _ops.new_rng_state(3, dev, 7), _ops.new_rng_state(3, dev, 7)
    loss3, g_c, g_f = _ops.mse2_loss(rgb_c, rgb_f, target, luminance, st_a)
    loss6, h_c, h_f, hd_c, hd_f = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, None, luminance=luminance, rng_state=st_b)
    assert torch.equal(loss6[:3], loss3) and torch.equal(h_c, g_c) and torch.equal(h_f, g_f) and hd_c is None and hd_f is None
    assert loss6[3:].tolist() == [0.0, 0.0, 0.0]
    assert st_a.tolist()[2:] == [7, 8] and st_b.tolist() == st_a.tolist()
    # coarse only
    loss3, g_c, _ = _ops.mse2_loss(rgb_c, None, target, luminance)
    loss6, h_c, h_f, _, _ = _ops.render_loss(rgb_c, None, target, luminance=luminance)
    assert torch.equal(loss6[:3], loss3) and torch.equal(h_c, g_c) and h_f is None


# ---- GPU: nerf.render_loss under autograd ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("luminance,scale", [(False, 1.0), (True, -2.5)])
def test_render_loss_under_autograd(dev, luminance, scale):
    """The gradients of the six maps (acc_* take none) against torch.autograd of the float64 restatement; grad_output scales them."""
    import nerf
    n = 257
    rgb_c, rgb_f, target, depth_c, depth_f, d = (t.to(dev) for t in head_inputs(n, "junk", seed=3))
    acc_c, acc_f = torch.rand(n, device=dev), torch.rand(n, device=dev)
    maps = [t.clone().requires_grad_(True) for t in (rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f)]
    kw = dict(weights=(0.7, 1.3), depth_weights=(0.1, 0.25), depth_range=(LO, HI), luminance=luminance)
    loss = nerf.render_loss(maps[0], maps[3], target, depth_c=maps[1], depth_f=maps[4], target_depth=d, **kw)
    assert loss.shape == () and loss.requires_grad and loss.terms.shape == (6,) and not loss.terms.requires_grad
    assert float(loss.detach()) == float(loss.terms[0])
    (loss + 0.0 * (maps[2].sum() + maps[5].sum())).backward(torch.tensor(scale, device=dev))
    ref = [t.double().requires_grad_(True) for t in (rgb_c, depth_c, rgb_f, depth_f)]
    want, ref6, valid = head64(ref[0], ref[2], target.double(), ref[1], ref[3], d.double(), kw["weights"], kw["depth_weights"], LO, HI, luminance)
    want.backward(torch.tensor(scale, dtype=torch.float64, device=dev))
    errs = {name: rel_err(C(maps[i].grad), C(r.grad)) for name, i, r in zip(("rgb_c", "depth_c", "rgb_f", "depth_f"), (0, 1, 3, 4), ref)}
    errs["terms"] = rel_err(C(loss.terms[:5]), C(ref6[:5]))
    print(f"render_loss autograd lum={luminance} grad_output={scale}:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs
    assert float(loss.terms[5]) == float(valid.sum()) and bool((maps[1].grad[~valid] == 0).all())
    assert float(maps[2].grad.abs().max()) == 0 and float(maps[5].grad.abs().max()) == 0
    # no depth target: the photometric loss; host tensors are refused
    plain = nerf.render_loss(rgb_c.clone().requires_grad_(True), None, target)
    assert plain.terms[3:].tolist() == [0.0, 0.0, 0.0] and float(plain.terms[2]) == 0.0
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.render_loss(rgb_c.cpu(), None, target.cpu())


# ---- GPU: FusedTrainStep --------------------------------------------------------------------------------------------------------------
TRAIN_KW = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
TRAIN_H = TRAIN_W = 24
TRAIN_RAYS = 256
TRAIN_POSES = (3, 9, 14)
TRAIN_RANGE = (0.0, 6.0)       # the synthetic scene's Dex validation mask


@pytest.fixture(scope="module")
def scene(dev):
    """V = 3 views of 24 x 24 of the synthetic teacher scene (a fixed random coarse + fine pair rendered at 16 + 16 samples): images,
    fine expected-depth maps, the selector - computed once, read only."""
    import nerf
    from nerf import synthetic as syn
    cfg = make_cfg(dict(num_coarse=16, num_fine=16, near=2.0, far=6.0, perturb=True, noise_std=0.0, white_background=False))
    still = make_cfg(dict(num_coarse=16, num_fine=16, near=2.0, far=6.0))          # the teacher is rendered without jitter
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    teacher = make_models(TRAIN_KW, syn.synth_state_dict(42, sigma_bias=-150.0, **TRAIN_KW), syn.synth_state_dict(43, sigma_bias=-20.0, **TRAIN_KW), dev)
    kmat = torch.from_numpy(syn.intrinsic(TRAIN_H, TRAIN_W))
    poses = [torch.from_numpy(syn.scene_pose(p)) for p in TRAIN_POSES]
    images, depths = [], []
    for pose in poses:
        ro, rd = nerf.get_ray_bundle(TRAIN_H, TRAIN_W, float(kmat[0, 0]), pose.to(dev), kmat.to(dev))
        with torch.no_grad():
            out = nerf.run_one_iter_of_nerf(TRAIN_H, TRAIN_W, float(kmat[0, 0]), teacher[0], teacher[1], ro, rd, still, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed)
        images.append(out[3].reshape(TRAIN_H, TRAIN_W, 3))
        depths.append(out[4].reshape(TRAIN_H, TRAIN_W))
    images, depths = torch.stack(images), torch.stack(depths).contiguous()
    inside = (depths > TRAIN_RANGE[0]) & (depths < TRAIN_RANGE[1])
    print(f"teacher scene: depth min {float(depths.min()):.3f} max {float(depths.max()):.3f}, {float(inside.float().mean()):.3f} of the pixels "
          f"inside {TRAIN_RANGE}")
    assert float(inside.float().mean()) > 0.05
    sel = nerf.MultiViewRaySelector(TRAIN_H, TRAIN_W, poses, [kmat] * len(poses), 2.0, 6.0, images=images, device=dev)
    return types.SimpleNamespace(cfg=cfg, ex=ex, ed=ed, sel=sel, images=images, depths=depths)


def train_step(scene, dev, seed=31, init=5, **kw):
    """A fresh student pair (torch's default init from `init`), its bucket and a FusedTrainStep on the scene."""
    import nerf
    from nerf import parallel
    torch.manual_seed(init)
    nets = [nerf.models.FlexibleNeRFModel(**TRAIN_KW).to(dev) for _ in range(2)]
    bucket = parallel.FlatGradBucket(nets)
    step = nerf.FusedTrainStep(nets[0], nets[1], scene.sel, scene.cfg, bucket, scene.ex, scene.ed, TRAIN_RAYS, seed=seed, **kw)
    return step, bucket, nets


def flat_params(nets):
    return torch.cat([p.detach().reshape(-1) for m in nets for p in m.parameters()])


DEPTH_KW = dict(depth_weights=(0.1, 0.1), depth_range=TRAIN_RANGE)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_route_is_untouched(dev, scene, precision, monkeypatch):
    """Without the new arguments the step never reaches the new head (it raises here), and three steps end in weights bit-identical to
    an instance given the defaults explicitly; a step through the new head with unit colour weights and a zero depth weight ends in
    the same bits too (x * 1.0f is exact, a zero depth weight hands the backward no depth gradient)."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    real = _ops.render_loss

    def boom(*a, **k):
        raise AssertionError("the default route reached dn_render_loss")
    results = []
    for kw, through_head in ((dict(), False), (dict(depth_images=None, loss_weights=(1, 1), depth_weights=(0, 0), depth_range=(0.0, INF)), False),
                             (dict(depth_images=scene.depths, depth_range=TRAIN_RANGE), True)):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", **kw)
        assert (step.head is not None) == through_head
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        with monkeypatch.context() as mp:
            if not through_head:
                mp.setattr(_ops, "render_loss", boom)
            for _ in range(3):
                step.forward_backward()
                opt.step()
        assert _ops.render_loss is real
        assert (step.loss6 is not None) == through_head and step.loss3.shape == (3,)
        results.append((flat_params(nets), step.loss3.clone()))
    for params, loss3 in results[1:]:
        assert torch.equal(params, results[0][0]) and torch.equal(loss3, results[0][1])
    assert bool(torch.isfinite(results[0][0]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("draw_view", ["rays", False])
def test_depth_supervised_step_is_the_chain_of_its_pieces(dev, scene, precision, draw_view):
    """One step with depth_images and lambda = 0.1 against dn_render_rays_train -> dn_render_loss (targets gathered by torch from the kept
    draw) -> dn_render_rays_backward with the depth gradients, on the step's own rows and draws: loss6 and the bucket bit for bit."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    step, bucket, nets = train_step(scene, dev, seed=31, first_iteration=2, draw_view=draw_view, depth_images=scene.depths, **DEPTH_KW)
    scene.sel.view.fill_(1)
    try:
        peek = _ops.new_rng_state(31, dev, 2)
        loss3 = step.forward_backward()
        assert step.rng_state.tolist()[2:] == [2, 3] and torch.equal(loss3, step.loss6[:3])
        views, pix, rows, target = step.latest_draw()
        if draw_view == "rays":
            assert views.dtype == torch.int32 and len(torch.unique(views)) == V
            d = scene.depths.reshape(V, -1)[views.long(), pix]
        else:
            assert views is None
            d = scene.depths.reshape(V, -1)[1, pix]
        assert pix.dtype == torch.int64 and rows.shape == (TRAIN_RAYS, 11)
        mc, mf = nets
        got = [(m.weight.grad.clone(), m.bias.grad.clone()) for net in nets for m in net.linear_modules()]
        pc, pf, prec = _ops.pack_train_pair(mc, mf, step.logs)
        maps, saved = _ops.render_rays_train(pc, pf, rows, 16, 16, False, 0.0, False, [], None, prec=prec, rng_state=peek, perturb=True)
        loss6, g_c, g_f, gd_c, gd_f = _ops.render_loss(maps[0], maps[3], target, maps[1], maps[4], d.contiguous(), depth_weights=(0.1, 0.1),
                                                       depth_range=TRAIN_RANGE)
        want_c = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mc.linear_modules()], dev)
        want_f = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mf.linear_modules()], dev)
        _ops.render_rays_backward(pc, pf, saved, (g_c, gd_c, None), (g_f, gd_f, None), want_c, want_f, nets=3)
        m_valid = float(loss6[5])
        print(f"train chain {precision} draw_view={draw_view}: loss6 {step.loss6.tolist()}")
        assert 0 < m_valid <= TRAIN_RAYS and float(loss6[3]) > 0 and float(loss6[4]) > 0 and float(gd_f.abs().max()) > 0
        assert torch.equal(step.loss6, loss6)
        for (gw, gb), (ww, wb) in zip(got, want_c + want_f):
            assert float(ww.abs().max()) > 0 and torch.equal(gw, ww) and torch.equal(gb, wb)
        # the depth term reaches the weights: the photometric backward on the same forward gives other gradients
        plain_c = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mc.linear_modules()], dev)
        plain_f = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mf.linear_modules()], dev)
        _ops.render_rays_backward(pc, pf, saved, (g_c, None, None), (g_f, None, None), plain_c, plain_f, nets=3)
        assert not torch.equal(plain_f[0][0], want_f[0][0])
    finally:
        scene.sel.view.fill_(0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_depth_supervised_steps_equal_eager_ones(dev, scene, precision):
    import nerf
    nerf.set_precision(precision)
    runs = []
    for use_graphs in (False, True):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", depth_images=scene.depths, **DEPTH_KW)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1, use_graphs=use_graphs)
        for _ in range(4):
            graphed.step()
        torch.cuda.synchronize()
        assert graphed.fallback_reason is None and (graphed.graphs is not None) == use_graphs, graphed.fallback_reason
        assert step.rng_state.tolist()[2:] == [3, 4]
        runs.append((flat_params(nets), step.loss6.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][1][5]) > 0


@pytest.mark.gpu
def test_data_parallel_halves_carry_the_depth_gradients(dev, scene):
    """forward_and_fine_backward() + coarse_backward() (the nets = 2 / nets = 1 halves of the data-parallel split) against the one-call
    step (nets = 3): the same kernels on the same saved tensors up to the weight-gradient launch, which forms both networks' gradients
    together or one at a time - at most another order of the fp32 partial sums, gated at 1e-4 as
    test_fused_train_step_equals_the_autograd_path_on_the_same_draws gates that reordering in fp32."""
    import nerf
    nerf.set_precision("fp32")
    grads = []
    for both in (True, False):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", depth_images=scene.depths, **DEPTH_KW)
        bucket.zero()
        step.forward_and_fine_backward(_zero=False, both=both)
        if not both:
            step.coarse_backward()
        grads.append([p.grad.clone() for p in bucket.params])
    for a, b in zip(*grads):
        assert float(a.abs().max()) > 0 and rel_err(C(b), C(a)) <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_depth_supervision_lowers_the_fine_depth_error(dev, scene, precision):
    """150 steps from one seed (the same student, the same draws): the final D_f (loss6[4], on the last step's batch) with lambda = 0.1
    is lower than with lambda = 0 - that run goes through the same head with zero depth weights so that it reports D_f.  Measured on an
    MI355X: 0.0268 against 3.83 (ratio 0.0070) in fp32, 0.0268 against 3.93 (0.0068) in bf16; only "lower" is gated."""
    import nerf
    nerf.set_precision(precision)
    final = {}
    for lam in (0.0, 0.1):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", depth_images=scene.depths, depth_weights=(lam, lam), depth_range=TRAIN_RANGE)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1)
        for _ in range(150):
            graphed.step()
        torch.cuda.synchronize()
        assert graphed.fallback_reason is None, graphed.fallback_reason
        final[lam] = step.loss6.tolist()
    print(f"{precision}: loss6 after 150 steps, lambda=0 {final[0.0]}, lambda=0.1 {final[0.1]}; D_f ratio {final[0.1][4] / final[0.0][4]:.4f}")
    assert all(np.isfinite(v).all() for v in final.values()) and final[0.0][5] == final[0.1][5] > 0
    assert final[0.1][4] < final[0.0][4]


@pytest.mark.gpu
def test_fused_train_step_value_errors_on_the_device(dev, scene):
    with pytest.raises(ValueError, match="draw_view"):
        train_step(scene, dev, draw_view=True, depth_images=scene.depths, **DEPTH_KW)
    with pytest.raises(ValueError, match="loss_weights"):
        train_step(scene, dev, draw_view="rays", loss_weights=(0.0, 1.0))
    with pytest.raises(ValueError, match="depth_images of shape"):
        train_step(scene, dev, draw_view="rays", depth_images=scene.depths[:2], **DEPTH_KW)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        train_step(scene, dev, draw_view="rays", depth_images=scene.depths.cpu(), **DEPTH_KW)


# ---- GPU: FusedPoseStep ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lego(dev):
    """(coarse, fine) lego-shaped 4 x 128 networks, parameters frozen, and the two encoders (test_fused_pose_step's)."""
    import nerf
    from golden_cases import CASES
    mkw, wfn, _ = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    return mc, mf, nerf.get_embedding_function(10), nerf.get_embedding_function(4)


def pose_depths(problem, dev):
    """(V,H,W) target depths for the pose problem: inside (2, 6) but for a fifth of the pixels (NaN, 0, 7)."""
    h, w = problem[0], problem[1]
    gen = torch.Generator().manual_seed(4)
    depth = 2.5 + 3.0 * torch.rand(V, h, w, generator=gen)
    junk = torch.tensor([float("nan"), 0.0, 7.0])[torch.arange(V * h * w) % 3].reshape(V, h, w)
    return torch.where(torch.rand(V, h, w, generator=gen) < 0.2, junk, depth).to(dev)


@pytest.mark.gpu
def test_fine_only_pose_step_equals_the_autograd_route_with_the_fine_term_alone(dev, lego, monkeypatch):
    """loss_weights = (0, 1): one eager step from a non-zero xi against the stage-by-stage autograd route (predict_and_render_radiance on
    the step's own rows and draws, the fine MSE alone) -> dn_camera_grad_views -> dn_pose_records_backward, at 1e-5."""
    import nerf
    from nerf import _ops
    problem = world_problem(dev)
    h, w, e0, k, images, cfg, focal = problem
    n = 96
    step = make_step(lego, problem, n, seed=21, first_iteration=4, use_graphs=False, loss_weights=(0.0, 1.0))
    step.xi.copy_(torch.tensor(XI_START))
    xi0 = step.xi.clone()
    peek = _ops.new_rng_state(21, dev, 4)
    loss3 = step.step()
    assert step.rng_state.tolist()[2:] == [4, 5] and torch.equal(loss3, step.loss6[:3])
    views, pix, rows, target = step.latest_draw()
    cams = _ops.pose_records(xi0, e0, k, focal)
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
    mse_f.backward()
    g = ref.grad
    g_cams = _ops.camera_grad_views(h, w, cams, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], 0.0, 1.0)
    want = _ops.pose_records_backward(g_cams, xi0, e0)
    err = rel_err(C(step.last_grad), C(want))
    got = step.loss6.tolist()
    print(f"fine-only pose step: last_grad vs the autograd route {err:.2e}; loss6 {got} vs mse_c {mse_c.item()} mse_f {mse_f.item()}")
    assert bool(torch.isfinite(step.last_grad).all()) and bool(torch.isfinite(step.xi).all()) and bool(torch.isfinite(step.loss6).all())
    assert float(want.abs().max()) > 0 and err <= 1e-5, err
    assert abs(got[0] - mse_f.item()) <= 1e-5 * mse_f.item() and abs(got[2] - mse_f.item()) <= 1e-5 * mse_f.item()
    assert abs(got[1] - mse_c.item()) <= 1e-5 * mse_c.item() and got[3:] == [0.0, 0.0, 0.0]
    assert bool((step.xi != xi0).any())


@pytest.mark.gpu
def test_depth_supervised_pose_step_is_the_chain_of_its_pieces(dev, lego):
    """depth_images with depth_weights = (0, 0.1): the xi gradient of one eager step against dn_pose_records -> dn_select_rays_views ->
    dn_render_rays_train_geom -> dn_render_loss (targets gathered by torch) -> dn_render_rays_backward_geom with the depth gradient ->
    dn_camera_grad_views -> dn_pose_records_backward on the step's own pairs and draws, bit for bit."""
    from nerf import _hip, _ops
    problem = world_problem(dev)
    h, w, e0, k, images, cfg, focal = problem
    depths = pose_depths(problem, dev)
    n = 96
    kw = dict(depth_images=depths, depth_weights=(0.0, 0.1), depth_range=(2.0, 6.0))
    step = make_step(lego, problem, n, seed=21, first_iteration=4, use_graphs=False, **kw)
    step.xi.copy_(torch.tensor(XI_START))
    xi0 = step.xi.clone()
    peek = _ops.new_rng_state(21, dev, 4)
    step.step()
    views, pix, rows, target = step.latest_draw()
    mc, mf, ex, ed = lego
    packs = []
    for m in (mc, mf):
        pk = m.packed(ex.log_sampling, ed.log_sampling, parts=_hip.PACK_CORE)
        _ops.ensure_backward_stream(m, pk, pk.precision)
        _ops.ensure_input_grad_stream(m, pk)
        packs.append(pk)
    pc, pf = packs
    cams = _ops.pose_records(xi0, e0, k, focal)
    rows2, target2 = _ops.select_rays_views(h, w, cams, views, 2.0, 6.0, pix, images)
    assert torch.equal(rows2, rows) and torch.equal(target2, target)
    maps, saved = _ops.render_rays_train_geom(pc, pf, rows2, 64, 64, False, 0.2, True, [], None, prec=pc.precision, rng_state=peek, perturb=True)
    d = depths.reshape(V, -1)[views.long(), pix].contiguous()
    loss6, g_c, g_f, gd_c, gd_f = _ops.render_loss(maps[0], maps[3], target2, maps[1], maps[4], d, depth_weights=(0.0, 0.1), depth_range=(2.0, 6.0))
    d_rays, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, gd_f, None))
    g_cams = _ops.camera_grad_views(h, w, cams, views, pix, n, d_rays[:, 0:3], d_rays[:, 3:6], d_rays[:, 8:11], 0.0, 1.0)
    want = _ops.pose_records_backward(g_cams, xi0, e0)
    plain, _ = _ops.render_rays_backward_geom(pc, pf, saved, (g_c, None, None), (g_f, None, None))
    print(f"depth pose step: loss6 {step.loss6.tolist()}")
    assert 0 < float(loss6[5]) < n and float(loss6[4]) > 0 and float(gd_f.abs().max()) > 0 and not torch.equal(plain, d_rays)
    assert torch.equal(step.loss6, loss6) and torch.equal(step.last_grad, want) and float(want.abs().max()) > 0
    assert bool(torch.isfinite(step.xi).all())


@pytest.mark.gpu
def test_replayed_pose_steps_with_the_new_head_equal_eager_ones(dev, lego):
    problem = world_problem(dev)
    kw = dict(depth_images=pose_depths(problem, dev), loss_weights=(0.0, 1.0), depth_weights=(0.0, 0.1), depth_range=(2.0, 6.0))
    eager = make_step(lego, problem, 96, seed=8, use_graphs=False, **kw)
    graphed = make_step(lego, problem, 96, seed=8, eager_iterations=1, **kw)
    for it in range(4):
        eager.step(); graphed.step()
        assert (graphed.graph is not None) == (it >= 1)
    torch.cuda.synchronize()
    assert graphed.fallback_reason is None and eager.graph is None, graphed.fallback_reason
    assert torch.equal(eager.xi, graphed.xi) and torch.equal(eager.last_grad, graphed.last_grad) and torch.equal(eager.loss6, graphed.loss6)
    assert bool(torch.isfinite(eager.xi).all()) and bool((eager.xi.abs().amax(dim=1) > 0).all()) and float(eager.loss6[5]) > 0
    assert eager.rng_state.tolist()[2:] == [3, 4] and graphed.rng_state.tolist()[2:] == [3, 4]
