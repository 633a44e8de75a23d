"""Per-view exposure on the fused device steps: dn_render_loss_exposure (include/dexnerf_hip_exposure.h), nerf.render_loss(exposure=),
nerf.apply_exposure, refine_exposure= on nerf.FusedPoseStep / nerf.FusedJointStep and the drivers' flags.

Yardsticks.  The kernel: a float64 torch restatement written here (tests/test_render_loss.py's head64 on the corrected colours),
differentiated by autograd, at that file's gate - 1e-5 of each tensor's largest magnitude - for loss6, both colour gradients and g_eps;
the depth half, the all-zero rows and everything a step with eps == 0 computes BIT FOR BIT against dn_render_loss / the steps without the
refinement (bits compared as integers: signed zeros count).  The steps: replayed against eager, a run against its repetition and its
resumption, bit for bit.  Recovery: known per-view gains and offsets on the frozen networks' own renders, see the test's docstring.

Shapes: N in {1, 64, 1025, 2500} rays (one ray, one wave, one past the head's 1024-thread stride, a ragged multi-stride tail), V in
{1, 5, 65} views (64 rays of 65 views: views without a ray), P in {1, 6}; the steps on test_joint_pose_training's 3 views of 24 x 20
pixels, 200 rays, lego 4 x 128 networks."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import REPO
from test_input_gradients import make_cfg
from test_joint_pose_training import H, N_RAYS, RENDER, V, W, cameras, encoders, make_joint, make_nets, params_of, problem, run_steps, same
from test_render_loss import HI, LO, head64

EXPOSURE = ("dn_render_loss_exposure",)
SCALE = 0.75          # exact in fp32
MODES = {1: "gain", 6: "affine"}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(bits(a), bits(b)))


def positive_zero(t):
    return bool((bits(t) == 0).all())


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_exposure_header_declares_exactly_its_table_and_the_library_exports_it():
    from nerf import _hip
    names = lambda name: set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", open(os.path.join(REPO, "include", name)).read()))  # noqa: E731
    assert names("dexnerf_hip_exposure.h") == set(_hip.EXPOSURE_EXPORTS) == set(EXPOSURE)
    older = names("dexnerf_hip.h") | names("dexnerf_hip_ext.h") | names("dexnerf_hip_anneal.h")
    assert not older & set(EXPOSURE) and older == set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS)
    assert "dexnerf_hip_exposure.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()      # build() checks the new header's symbols too
    assert os.path.exists(_hip.LIB_PATH), "libdexnerf_hip.so is not built"
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in EXPOSURE) and _hip.lib().dn_abi_version() == 2


def test_entry_point_judges_its_arguments_before_gpu_work():
    from nerf import _hip
    lib = _hip.lib()
    fake = ctypes.c_void_p(1024)
    defaults = dict(rgb_c=fake, rgb_f=fake, target=fake, depth_c=None, depth_f=None, depth_src=None, pix=None, views=fake, view=None, hw=0, n=8,
                    lum=0, w_c=1.0, w_f=1.0, wd_c=0.0, wd_f=0.0, lo=0.0, hi=1.0, eps=fake, p=6, n_views=3, scale=1.0, mask=None, loss6=fake,
                    g_c=fake, g_f=fake, gd_c=None, gd_f=None, g_eps=fake, rng=None, stream=None)
    call = lambda **kw: lib.dn_render_loss_exposure(*{**defaults, **kw}.values())  # noqa: E731
    for kw in (dict(eps=None), dict(p=0), dict(p=3), dict(p=7), dict(n_views=0), dict(n_views=65536), dict(scale=0.0), dict(scale=-1.0),
               dict(scale=float("inf")), dict(scale=float("nan")), dict(n=0), dict(rgb_c=None), dict(target=None), dict(loss6=None),
               dict(w_c=float("nan")), dict(depth_src=fake), dict(pix=fake), dict(depth_src=fake, depth_c=fake, lo=float("nan")),
               dict(depth_src=fake, depth_c=fake, pix=fake, hw=0)):
        assert call(**kw) == -1000, kw
        assert b"dn_render_loss_exposure" in lib.dn_last_error()


def test_steps_and_loss_refuse_bad_exposure_settings_before_any_device_call(monkeypatch):
    import nerf
    from golden_cases import CASES
    from nerf import _hip

    def no_device(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_hip, "lib", no_device)
    e, k = cameras()
    images = torch.zeros(V, H, W, 3)
    cfg = make_cfg(RENDER)
    ex, ed = encoders()
    good = nerf.models.FlexibleNeRFModel(**dict(CASES["render_lego_val"][0]))

    def pose(**kw):
        return nerf.FusedPoseStep(good, good, cfg, H, W, k, e, images, ex, ed, N_RAYS, 1e-3, **kw)

    def joint(**kw):
        return nerf.FusedJointStep(good, good, cfg, H, W, k, e, images, ex, ed, N_RAYS, None, None, 1e-3, **kw)
    for make in (pose, joint):
        for bad in ("all", "offset", 6, True):
            with pytest.raises(ValueError, match="refine_exposure"):
                make(refine_exposure=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan"), "big"):
            with pytest.raises(ValueError, match="exposure_scale"):
                make(refine_exposure="gain", exposure_scale=bad)
        for bad in ((V,), (0, -1)):
            with pytest.raises(ValueError, match="exposure_fixed_views"):
                make(refine_exposure="affine", exposure_fixed_views=bad)
        with pytest.raises(ValueError, match="exposure_fixed_views"):
            make(exposure_fixed_views=(0,))                                  # rows held, but no rows
    with pytest.raises(ValueError, match="nothing to refine"):               # the pose step's own words stay
        pose(refine_pose=False)
    rgb = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="view_index"):
        nerf.render_loss(rgb, rgb, rgb, exposure=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="exposure"):
        nerf.render_loss(rgb, rgb, rgb, exposure=torch.zeros(2, 3), view_index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="exposure"):
        nerf.render_loss(rgb, rgb, rgb, exposure=torch.zeros(2, 6), view_index=torch.zeros(4, dtype=torch.int32), exposure_mode="gain")
    with pytest.raises(ValueError, match="exposure_scale"):
        nerf.render_loss(rgb, rgb, rgb, exposure=torch.zeros(2, 6), view_index=torch.zeros(4, dtype=torch.int32), exposure_scale=0.0)
    with pytest.raises(ValueError, match="without exposure"):
        nerf.render_loss(rgb, rgb, rgb, view_index=torch.zeros(4, dtype=torch.int32))


def test_driver_flags_need_refine_poses():
    import train_dexnerf
    args = train_dexnerf.parse_args(["--refine-poses", "--refine-exposure", "affine", "--exposure-scale", "0.5", "--fix-exposure-views", "0", "2"])
    assert args.refine_exposure == "affine" and args.exposure_scale == 0.5 and args.fix_exposure_views == [0, 2]
    plain = train_dexnerf.parse_args(["--refine-poses", "--refine-exposure", "gain"])
    assert plain.refine_exposure == "gain" and plain.exposure_scale == 1.0 and plain.fix_exposure_views == [0]
    off = train_dexnerf.parse_args(["--refine-poses"])
    assert off.refine_exposure is None and off.fix_exposure_views is None
    none = train_dexnerf.parse_args([])
    assert none.refine_exposure is None and none.exposure_scale is None and none.fix_exposure_views is None
    for bad in (["--refine-exposure", "gain"], ["--exposure-scale", "0.5"], ["--fix-exposure-views", "1"],
                ["--refine-poses", "--refine-exposure", "offset"], ["--refine-poses", "--exposure-scale", "0.5"],
                ["--refine-poses", "--refine-exposure", "gain", "--exposure-scale", "0"], ["--refine-poses", "--fix-exposure-views", "1"],
                ["--refine-poses", "--refine-exposure", "gain", "--fix-exposure-views", "-1"]):
        with pytest.raises(SystemExit):
            train_dexnerf.parse_args(bad)


def test_apply_exposure_matches_its_formula():
    import nerf
    gen = torch.Generator().manual_seed(4)
    rgb = torch.rand(7, 5, 3, generator=gen, dtype=torch.float64)
    row = torch.tensor([0.3, -0.2, 0.1, 0.05, -0.04, 0.02], dtype=torch.float64)
    got = nerf.apply_exposure(rgb, row, "affine", 0.5)
    for k in range(3):
        want = math.exp(0.5 * float(row[k])) * rgb[..., k] + 0.5 * float(row[3 + k])
        assert float((got[..., k] - want).abs().max()) <= 1e-15
    got = nerf.apply_exposure(rgb, [0.4], "gain", 2.0)
    assert float((got - math.exp(0.8) * rgb).abs().max()) <= 1e-15
    assert torch.equal(nerf.apply_exposure(rgb, torch.zeros(6), "affine", 3.0), rgb) and torch.equal(nerf.apply_exposure(rgb, [0.0], "gain"), rgb)
    leaf = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    nerf.apply_exposure(rgb, leaf, "affine", 0.5).sum().backward()
    assert float((leaf.grad[3:] - 0.5 * 35).abs().max()) <= 1e-12
    for bad in (dict(eps_row=row, mode="gain"), dict(eps_row=[0.1], mode="affine"), dict(eps_row=row, mode="offset")):
        with pytest.raises(ValueError):
            nerf.apply_exposure(rgb, scale=1.0, **bad)


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


HW = 37               # pixels per depth map of the gathered depth targets


def kernel_inputs(n, v, p, seed=0):
    """Host tensors of a head call: maps, targets, view / pixel indices, (V, HW) depth maps (about a fifth invalid), exposure rows with
    |s a| <= 0.5 and |s b| <= 0.2 - every third row exactly zero - and a mask that holds every fourth view."""
    gen = torch.Generator().manual_seed(7919 * seed + 131 * n + 7 * v + p)
    rgb_c, rgb_f, target = (torch.rand(n, 3, generator=gen) for _ in range(3))
    depth_c, depth_f = (2.0 + 2.0 * torch.rand(n, generator=gen) for _ in range(2))
    views = torch.randint(0, v, (n,), generator=gen, dtype=torch.int32)
    pix = torch.randint(0, HW, (n,), generator=gen, dtype=torch.int64)
    maps = 1.0 + 3.5 * torch.rand(v, HW, generator=gen)
    junk = torch.tensor([float("nan"), 0.0, HI + 0.25])[torch.arange(v * HW) % 3].view(v, HW)
    maps = torch.where(torch.rand(v, HW, generator=gen) < 0.2, junk, maps)
    eps = (2.0 * torch.rand(v, p, generator=gen) - 1.0) * (0.5 / SCALE)
    if p == 6:
        eps[:, 3:] *= 0.4
    eps[torch.arange(v) % 3 == 1] = 0.0
    mask = (torch.arange(v) % 4 != 3).to(torch.int32)
    return rgb_c, rgb_f, target, depth_c, depth_f, views, pix, maps, eps, mask


def corrected64(rgb, eps, views, p):
    """apply_exposure per ray in float64, differentiable in rgb and eps."""
    row = eps[views.long()]
    if p == 1:
        return torch.exp(SCALE * row[:, :1]) * rgb
    return torch.exp(SCALE * row[:, :3]) * rgb + SCALE * row[:, 3:]


def rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


WEIGHTS, DEPTH_WEIGHTS = (0.7, 1.3), (0.1, 0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [1, 5, 65])
@pytest.mark.parametrize("n", [1, 64, 1025, 2500])
def test_kernel_against_float64(dev, n, v):
    """Every P, both luminance modes, with and without the fine map at (n, v); the depth term on, its targets gathered.  The measured
    errors are printed (the largest over all shapes stands in DESIGN.md section 4.5)."""
    from nerf import _ops
    worst = {}
    for p in (1, 6):
        host = kernel_inputs(n, v, p)
        rgb_c, rgb_f, target, depth_c, depth_f, views, pix, maps, eps, mask = (t.to(dev) for t in host)
        present = torch.bincount(views.long().cpu(), minlength=v) > 0
        if n == 64 and v == 65:
            assert not bool(present.all())                                   # views without a ray
        for luminance in (False, True):
            for fine in (True, False):
                f = rgb_f if fine else None
                df = depth_f if fine else None
                kw = dict(weights=WEIGHTS, depth_weights=DEPTH_WEIGHTS, depth_range=(LO, HI), luminance=luminance)
                got = _ops.render_loss_exposure(rgb_c, f, target, eps, SCALE, views, None, mask, depth_c, df, maps, pix, **kw)
                again = _ops.render_loss_exposure(rgb_c, f, target, eps, SCALE, views, None, mask, depth_c, df, maps, pix, **kw)
                assert all(same_bits(a, b) for a, b in zip(got, again))                       # two runs: the same bits
                plain = _ops.render_loss(rgb_c, f, target, depth_c, df, maps, pix, views, None, **kw)
                loss6, g_c, g_f, gd_c, gd_f, g_eps = got
                assert same_bits(gd_c, plain[3]) and same_bits(gd_f, plain[4]) and same_bits(loss6[3:6], plain[0][3:6])   # the depth half
                leaves = [None if t is None else t.double().requires_grad_(True) for t in (rgb_c, f)]
                eps64 = eps.double().requires_grad_(True)
                d = maps.double()[views.long(), pix]
                loss, ref6, _ = head64(corrected64(leaves[0], eps64, views, p), None if f is None else corrected64(leaves[1], eps64, views, p),
                                       target.double(), depth_c.double(), None if df is None else df.double(), d, WEIGHTS, DEPTH_WEIGHTS, LO, HI,
                                       luminance)
                loss.backward()
                want_eps = eps64.grad * mask.double()[:, None]
                errs = dict(loss6=rel(loss6[:5], ref6[:5]), g_rgb_c=rel(g_c, leaves[0].grad), g_eps=rel(g_eps, want_eps))
                if f is not None:
                    errs["g_rgb_f"] = rel(g_f, leaves[1].grad)
                print(f"exposure head n={n} V={v} P={p} lum={luminance} fine={fine}: errors", {k: f"{e:.2e}" for k, e in errs.items()})
                for k, e in errs.items():
                    worst[k] = max(worst.get(k, 0.0), e)
                assert float(want_eps.abs().max()) > 0 or not bool((present & (mask.cpu() != 0)).any())
                assert all(e <= 1e-5 for e in errs.values()), errs
                quiet = (~present) | (mask.cpu() == 0)                                        # ray-less and masked views: exact +0
                assert positive_zero(g_eps.cpu()[quiet])
                assert (g_f is None) == (f is None)
    print(f"exposure head n={n} V={v}: worst", {k: f"{e:.2e}" for k, e in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", [(65, 1), (1025, 5), (2500, 65)])
def test_one_view_word_and_missing_outputs(dev, n, v):
    """view_index NULL: every ray is of view *view, and the other rows get +0; g_eps NULL: loss and colour gradients unchanged."""
    from nerf import _ops
    rgb_c, rgb_f, target, _, _, views, _, _, eps, _ = (t.to(dev) for t in kernel_inputs(n, v, 6, seed=3))
    one = v - 1
    eps[one] = torch.tensor([0.2, -0.3, 0.1, 0.05, -0.1, 0.02], device=dev)
    word = torch.tensor([one], dtype=torch.int32, device=dev)
    a = _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, SCALE, None, word)
    b = _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, SCALE, torch.full((n,), one, dtype=torch.int32, device=dev))
    assert all(same_bits(x, y) for x, y in zip(a, b))
    others = torch.arange(v) != one
    assert positive_zero(a[5].cpu()[others]) and float(a[5][one].abs().min()) > 0
    c = _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, SCALE, views, want_eps=False)
    d = _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, SCALE, views)
    assert c[5] is None and all(same_bits(x, y) for x, y in zip(c[:5], d[:5]))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 6])
@pytest.mark.parametrize("luminance", [False, True])
@pytest.mark.parametrize("n,v", [(1, 1), (64, 65), (1025, 5), (2500, 65)])
def test_all_zero_rows_give_the_plain_head_bit_for_bit(dev, n, v, p, luminance):
    """eps == 0 (both signs of zero): loss6, the colour and the depth gradients are dn_render_loss's bits - with -0.0 colours, zero
    targets, and the rng counter advanced alike."""
    from nerf import _ops
    rgb_c, rgb_f, target, depth_c, depth_f, views, pix, maps, eps, mask = (t.to(dev) for t in kernel_inputs(n, v, p, seed=5))
    rgb_c[::3] = -0.0
    rgb_f[1::4, 1] = -0.0
    target[::2] = 0.0
    target[1::5] = -0.0
    eps = torch.zeros_like(eps)
    eps[::2] = -0.0
    kw = dict(weights=WEIGHTS, depth_weights=DEPTH_WEIGHTS, depth_range=(LO, HI), luminance=luminance)
    rng_a, rng_b = _ops.new_rng_state(11, dev, 4), _ops.new_rng_state(11, dev, 4)
    got = _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, SCALE, views, None, None, depth_c, depth_f, maps, pix, rng_state=rng_a, **kw)
    want = _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, maps, pix, views, None, rng_state=rng_b, **kw)
    assert all(same_bits(a, b) for a, b in zip(got[:5], want)) and torch.equal(rng_a, rng_b) and int(rng_a[3]) == 5
    assert bool(torch.signbit(got[1]).any()) or luminance                    # (the signed zeros reached the outputs)
    coarse = _ops.render_loss_exposure(rgb_c, None, target, eps, SCALE, views, **kw)
    assert all(same_bits(a, b) for a, b in zip(coarse[:5], _ops.render_loss(rgb_c, None, target, **kw)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gain", "affine"])
def test_render_loss_with_exposure_under_autograd(dev, mode):
    import nerf
    from nerf import _ops
    p = nerf.loss.EXPOSURE_MODES[mode]
    n, v = 300, 5
    rgb_c, rgb_f, target, depth_c, depth_f, views, pix, maps, eps, _ = (t.to(dev) for t in kernel_inputs(n, v, p, seed=9))
    d = maps[views.long(), pix]
    leaves = [t.clone().requires_grad_(True) for t in (rgb_c, rgb_f, depth_c, depth_f, eps)]
    kw = dict(weights=WEIGHTS, depth_weights=DEPTH_WEIGHTS, depth_range=(LO, HI))
    loss = nerf.render_loss(leaves[0], leaves[1], target, leaves[2], leaves[3], d, exposure=leaves[4], view_index=views, exposure_mode=mode,
                            exposure_scale=SCALE, **kw)
    (-2.5 * loss).backward()
    ref = [t.double().requires_grad_(True) for t in (rgb_c, rgb_f, depth_c, depth_f, eps)]
    loss64, ref6, _ = head64(corrected64(ref[0], ref[4], views, p), corrected64(ref[1], ref[4], views, p), target.double(), ref[2], ref[3],
                             d.double(), WEIGHTS, DEPTH_WEIGHTS, LO, HI, False)
    (-2.5 * loss64).backward()
    errs = {"loss": rel(loss.detach().reshape(1), loss64.detach().reshape(1)), "terms": rel(loss.terms[:5], ref6[:5].detach())}
    for name, a, b in zip(("rgb_c", "rgb_f", "depth_c", "depth_f", "exposure"), leaves, ref):
        errs[name] = rel(a.grad, b.grad)
    print("render_loss(exposure=) under autograd", mode, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs
    plain = nerf.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, d, **kw)               # exposure=None: today's function
    assert plain.grad_fn is None and torch.equal(plain.terms, _ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, d, **kw)[0])


# ---- the steps --------------------------------------------------------------------------------------------------------------------------
STEP_PRECISIONS = ("fp32", "bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", STEP_PRECISIONS)
def test_zero_pose_lr_equals_the_step_without_the_refinement_bit_for_bit(dev, precision):
    """lr_pose = 0 holds [xi | phi | eps] at zero: the new head then runs its plain branch on every ray, and the joint step trains the
    networks as without the refinement.  Six steps: 3 eager, the capture, 2 replays."""
    import nerf
    nerf.set_precision(precision)
    runs = []
    for kw in (dict(refine_exposure="affine"), dict()):
        nets = make_nets(dev)
        step, _, _ = make_joint(dev, nets, seed=13, lr_pose=0.0, eager_iterations=3, **kw)
        trace = []
        for _ in range(6):
            trace.append(step.step().clone())
        torch.cuda.synchronize()
        assert isinstance(step.graph, torch.cuda.CUDAGraph) and step.fallback_reason is None, step.fallback_reason
        runs.append((params_of(nets), trace, step.xi.clone(), step))
    (params_a, trace_a, xi_a, with_eps), (params_b, trace_b, xi_b, without) = runs
    assert same(params_a, params_b) and all(same_bits(a, b) for a, b in zip(trace_a, trace_b)) and same_bits(xi_a, xi_b)
    assert positive_zero(with_eps.eps) and tuple(with_eps.eps.shape) == (V, 6) and float(with_eps.last_grad_eps.abs().max()) > 0
    assert without.eps is None and without.exposure() is None and without.last_grad_eps is None
    assert with_eps._flat.shape[1] == (6 * V + 6 * V + 3) // 4 * 4 and without._flat.shape[1] == (6 * V + 3) // 4 * 4


@pytest.mark.gpu
@pytest.mark.parametrize("precision", STEP_PRECISIONS)
@pytest.mark.parametrize("mode", ["gain", "affine"])
def test_replayed_steps_equal_eager_ones_and_fixed_rows_stay(dev, precision, mode):
    import nerf
    nerf.set_precision(precision)
    p = nerf.loss.EXPOSURE_MODES[mode]
    held = torch.linspace(-0.2, 0.3, p)
    out = []
    for graphs in (True, False, True):
        nets = make_nets(dev)
        step, _, _ = make_joint(dev, nets, seed=17, lr_pose=2e-3, use_graphs=graphs, eager_iterations=3, refine_exposure=mode,
                                exposure_scale=SCALE, exposure_fixed_views=(1,), fixed_views=(0,))
        step.eps[1] = held.to(dev)
        for _ in range(6):
            step.step()
            assert positive_zero(step.last_grad_eps[1]) and float(step.last_grad_eps[0].abs().min()) > 0
        torch.cuda.synchronize()
        assert (step.graph is not None) == graphs and step.fallback_reason is None, step.fallback_reason
        assert same_bits(step.eps[1], held.to(dev))                           # the held row: untouched
        assert float(step.eps[0].abs().min()) > 0 and float(step.eps[2].abs().min()) > 0
        assert same_bits(step.exposure(), step.eps) and step.exposure().data_ptr() != step.eps.data_ptr()
        out.append((step._flat[0].clone(), params_of(nets)))
    (flat_g, params_g), (flat_e, params_e), (flat_r, params_r) = out
    assert same_bits(flat_g, flat_e) and same(params_g, params_e)             # replayed == eager
    assert same_bits(flat_g, flat_r) and same(params_g, params_r)             # a run is a function of its seed


@pytest.mark.gpu
@pytest.mark.parametrize("precision", STEP_PRECISIONS)
def test_a_run_with_exposure_resumes_from_its_state(dev, precision):
    import nerf
    nerf.set_precision(precision)
    kw = dict(refine_exposure="affine", exposure_scale=SCALE, exposure_fixed_views=(0,))
    whole, params_w, draws_w, _ = run_steps(dev, 5, 6, **kw)
    first, _, draws_1, snapshot = run_steps(dev, 5, 3, **kw)
    state = snapshot[4]
    assert state["refine_exposure"] == "affine" and state["exposure_scale"] == SCALE
    second, params_2, draws_2, _ = run_steps(dev, 5, 3, first_iteration=3, restore=snapshot, **kw)
    assert same(draws_1 + draws_2, draws_w) and same(params_2, params_w)
    assert same_bits(second._flat[0], whole._flat[0]) and same_bits(second.eps, whole.eps) and float(whole.eps[1:].abs().min()) > 0
    plain, _, _, snapshot_plain = run_steps(dev, 5, 1)
    assert "refine_exposure" not in snapshot_plain[4] and "exposure_scale" not in snapshot_plain[4]
    plain.load_state_dict(snapshot_plain[4])                                  # a state without the keys: no exposure rows
    for step, bad in ((plain, state), (whole, snapshot_plain[4]), (whole, dict(state, exposure_scale=1.0)), (whole, dict(state, refine_exposure="gain"))):
        with pytest.raises(ValueError, match="load_state_dict"):
            step.load_state_dict(bad)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_drivers_train_store_resume_and_apply_the_rows(dev, tmp_path):
    import eval_nerf
    import nerf
    import train_dexnerf
    from test_joint_pose_training import CLI
    path = os.path.join(str(tmp_path), "exposure.ckpt")
    flags = ["--refine-poses", "--fix-views", "0", "1", "2", "--refine-exposure", "affine", "--exposure-scale", "0.5"]
    res = train_dexnerf.main(CLI + flags + ["--iters", "12", "--save", path])
    rows = torch.tensor(res["exposure"])
    assert res["hip_graphs"] == 1 and bool((res["xi"] == 0).all())           # every pose held: networks and exposure alone
    assert tuple(rows.shape) == (3, 6) and bool((rows[0] == 0).all()) and float(rows[1:].abs().min()) > 0
    ck = torch.load(path, map_location="cpu")
    assert torch.equal(ck["refined_exposure"], rows) and ck["refined_exposure_mode"] == "affine" and ck["refined_exposure_scale"] == 0.5
    state = ck[train_dexnerf.JOINT_KEY]
    assert state["refine_exposure"] == "affine" and torch.equal(state["params"][18:36].view(3, 6), rows)
    again = train_dexnerf.main(CLI + flags + ["--iters", "12", "--load-checkpoint", path])      # no iteration left: the saved rows
    assert again["exposure"] == res["exposure"]
    render = ["--checkpoint", path, "--size", "24", "--num-coarse", "16", "--num-fine", "24", "--precision", "fp32", "--quiet", "--use-refined-poses"]
    plain = eval_nerf.main(render)["frames"]
    shown = eval_nerf.main(render + ["--apply-exposure"])["frames"]
    assert torch.equal(plain[0][0], shown[0][0])                             # view 0: the identity row
    for v in (1, 2):
        assert torch.equal(shown[v][0], nerf.apply_exposure(plain[v][0], rows[v], "affine", 0.5)) and not torch.equal(shown[v][0], plain[v][0])
    with pytest.raises(SystemExit):
        eval_nerf.main(render[:-1] + ["--apply-exposure"])                   # needs --use-refined-poses
    without = os.path.join(str(tmp_path), "poses.ckpt")
    train_dexnerf.main(CLI + ["--refine-poses", "--iters", "4", "--save", without])
    assert "refined_exposure" not in torch.load(without, map_location="cpu")
    with pytest.raises(SystemExit):
        eval_nerf.main(["--checkpoint", without] + render[2:] + ["--apply-exposure"])


# ---- recovery ---------------------------------------------------------------------------------------------------------------------------
GAINS = ((1.2, 0.85, 1.1), (0.8, 1.15, 0.9), (1.1, 1.2, 0.8))               # per view and channel: of the order of +-20 %
OFFSETS = ((0.05, -0.04, 0.03), (-0.05, 0.03, 0.04), (0.04, 0.05, -0.05))   # +-0.05
RECOVERY_STEPS, RECOVERY_LR = 600, 0.01
# Measured on an MI355X after 600 steps at lr 0.01, seed 3: max |exp(s a) - gain| 1.216e-04, max |s b - offset| 1.132e-04, the fine mse
# 3.28e-02 -> 4.6e-10 (seeds 4 / 5: 0.69e-04 / 1.64e-04 and 0.68e-04 / 1.54e-04; after 300 steps the errors were still 9.7e-03 / 9.1e-03,
# after 1000 they sit at fp32's floor, 2e-05).  The gate: three times the measured error - 270 times below half the perturbation.
RECOVERY_GATE = dict(gain=3 * 1.216e-04, offset=3 * 1.132e-04)


@pytest.mark.gpu
def test_exposure_is_recovered_on_frozen_networks(dev):
    """Targets: the frozen lego networks' own fine renders at the true cameras (no jitter, no density noise), each view multiplied and
    offset per channel by GAINS / OFFSETS.  FusedPoseStep(refine_pose=False, refine_exposure="affine", loss_weights=(0, 1)) from
    eps = 0 for RECOVERY_STEPS steps of RECOVERY_LR on 200 rays: the optimum exp(s a) = GAINS, s b = OFFSETS is exact (zero fine mse).
    Had eps stayed at zero the errors would be the perturbations themselves (0.2, 0.05); half of them is the condition, the gate is
    three times the error measured on an MI355X (see RECOVERY_GATE)."""
    import nerf
    nerf.set_precision("fp32")
    nets = make_nets(dev)
    for m in nets:
        for q in m.parameters():
            q.requires_grad_(False)
    e0, k, _, _ = problem(dev)
    render = dict(RENDER, perturb=False, noise_std=0.0)
    options = make_cfg(render)
    ex, ed = encoders()
    gains, offsets = torch.tensor(GAINS, device=dev), torch.tensor(OFFSETS, device=dev)
    images = []
    with torch.no_grad():
        for view in range(V):
            ro, rd = nerf.get_ray_bundle(H, W, float(k[0, 0]), e0[view], k)
            out = nerf.run_one_iter_of_nerf(H, W, float(k[0, 0]), nets[0], nets[1], ro, rd, options, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed)
            images.append(out[3].reshape(H, W, 3) * gains[view] + offsets[view])
    images = torch.stack(images)
    spread = [float(images[view].reshape(-1, 3).std(0).min()) for view in range(V)]
    step = nerf.FusedPoseStep(nets[0], nets[1], options, H, W, k, e0, images, ex, ed, N_RAYS, RECOVERY_LR, seed=3, refine_pose=False,
                              refine_exposure="affine", exposure_scale=1.0, loss_weights=(0.0, 1.0))
    first = float(step.step()[2])
    for _ in range(RECOVERY_STEPS - 1):
        step.step()
    last = float(step.loss3[2])
    assert step.fallback_reason is None and step.graph is not None, step.fallback_reason
    eps = step.exposure()
    err_gain = float((torch.exp(eps[:, :3]) - gains).abs().max())
    err_offset = float((eps[:, 3:] - offsets).abs().max())
    print(f"exposure recovery: {RECOVERY_STEPS} steps, lr {RECOVERY_LR}: fine mse {first:.3e} -> {last:.3e}; max |exp(s a) - gain| "
          f"{err_gain:.3e}, max |s b - offset| {err_offset:.3e}; colour spread per view {spread}")
    assert positive_zero(step.xi) and float(step.last_grad.abs().max()) == 0.0             # the poses: held
    assert last < first
    assert RECOVERY_GATE["gain"] <= 0.1 and RECOVERY_GATE["offset"] <= 0.025             # never looser than half the perturbation
    assert err_gain <= RECOVERY_GATE["gain"] and err_offset <= RECOVERY_GATE["offset"], (err_gain, err_offset)
