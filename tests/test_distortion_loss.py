"""The distortion regulariser: dn_distortion_loss (the loss of mip-NeRF 360 on compositing's weights and depths, value and gradients by
prefix sums), its route through the render backward (dn_render_rays_backward_reg) and its consumers - _ops.distortion_loss,
nerf.distortion_loss under autograd, nerf.FusedTrainStep / GraphedTrainStep with distortion_weights, train_dexnerf.py --distortion-weight.

Yardsticks: a float64 torch restatement written here in the PAIRWISE O(S^2) form with gradients from torch autograd (independent of the
kernel's prefix form) at 1e-5 max|ref| per tensor - the project's gate for fp32 gradient kernels against float64; the kernel sums in
fp64 and rounds each output once, so the measured error sits at fp32 rounding (profiles/distortion_loss.md).  The chain of the pinned
pieces, bit for bit, for the fused step.  Tolerances in the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from test_input_gradients import make_cfg
from test_render_loss import TRAIN_RAYS, _restore_modes, dev, flat_params, scene, train_step  # noqa: F401  (_restore_modes, dev, scene: fixtures)

INF = float("inf")
NAN = float("nan")
TOL = 1e-5
EXT = ("dn_distortion_loss", "dn_render_reg_workspace_bytes", "dn_render_rays_backward_reg")


def C(t):
    return t.detach().cpu().numpy()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_extension_header_declares_exactly_the_extension_table_and_the_v2_table_stays():
    from nerf import _hip
    ext = open(os.path.join(REPO, "include", "dexnerf_hip_ext.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", ext)) == set(_hip.EXT_EXPORTS) == set(EXT)
    assert '#include "dexnerf_hip.h"' in ext and "DN_ABI_VERSION" not in ext.replace("DN_ABI_VERSION stay", "")
    v2 = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", v2))
    assert len(declared) == 76 and declared == set(_hip.EXPORTS) and not declared & set(EXT)
    assert "#define DN_ABI_VERSION 2" in v2


def hiplib():
    from nerf import _hip
    if not _hip.available():
        pytest.skip("libdexnerf_hip.so is not built")
    return _hip.lib()


def test_binding_resolves_the_extension_symbols():
    from nerf import _hip
    lib = hiplib()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in _hip.EXT_EXPORTS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
    assert lib.dn_abi_version() == 2 and len(_hip.EXPORTS) == 76
    assert len(lib.dn_distortion_loss.argtypes) == 13
    assert len(lib.dn_render_rays_backward_reg.argtypes) == len(lib.dn_render_rays_backward_ws.argtypes) + 5
    assert lib.dn_render_reg_workspace_bytes.restype is ctypes.c_size_t


def test_distortion_loss_validates_before_gpu_work():
    lib = hiplib()
    fake = ctypes.c_void_p(1024)

    def call(weights=fake, z=fake, near_far=fake, stride=2, n=4, s=16, scale=1.0, g_w=fake, g_z=None, ray_loss=fake, mean=fake):
        return lib.dn_distortion_loss(weights, z, near_far, stride, n, s, scale, g_w, g_z, 0, ray_loss, mean, None)
    for kw in (dict(weights=None), dict(z=None), dict(near_far=None), dict(g_w=None), dict(ray_loss=None), dict(mean=None), dict(n=-1),
               dict(s=0), dict(s=-5), dict(s=1025), dict(stride=1), dict(stride=0), dict(scale=NAN), dict(scale=INF), dict(scale=-INF)):
        assert call(**kw) == -1000, kw
        assert b"dn_distortion_loss" in lib.dn_last_error(), kw
    # an empty batch returns before any check of its pointers, as elsewhere
    assert call(n=0, weights=None, z=None, near_far=None, g_w=None, ray_loss=None, mean=None) == 0


def test_render_backward_reg_validates_before_gpu_work():
    from nerf import _hip
    lib = hiplib()
    fake = ctypes.c_void_p(1024)
    desc = _hip.MlpDesc()
    arrays = [(ctypes.c_void_p * 4)() for _ in range(4)]
    need = lib.dn_render_reg_workspace_bytes(8, 16, 16)
    assert need >= 8 * 32 * 4 * 2 + 8 * 8 and need % 256 == 0
    for bad in ((-1, 16, 16), (8, 0, 16), (8, 16, -1)):
        assert lib.dn_render_reg_workspace_bytes(*bad) == 0

    def call(rays=fake, ws=fake, n=8, nc=16, nf=16, nets=3, w=(0.01, 0.01), reg_ws=fake, reg_bytes=need, reg2=fake, stride=11):
        return lib.dn_render_rays_backward_reg(ctypes.byref(desc), fake, ctypes.byref(desc), fake, 0, rays, stride, n, nc, nf, 0.0, 0, None, None,
                                               fake, None, None, fake, None, None, ws, fake, fake, fake, fake, fake, fake, *arrays, nets, None,
                                               None, 0, w[0], w[1], reg_ws, reg_bytes, reg2, None)
    for kw in (dict(rays=None), dict(ws=None), dict(n=-1), dict(nets=4), dict(ws=ctypes.c_void_p(1028)), dict(w=(-0.01, 0.0)), dict(w=(0.0, -1.0)),
               dict(w=(NAN, 0.0)), dict(w=(0.0, INF)), dict(reg_ws=None), dict(reg2=None), dict(reg_ws=ctypes.c_void_p(1028)),
               dict(reg_bytes=need - 1), dict(reg_bytes=0), dict(nc=600, nf=600, reg_bytes=1 << 30), dict(nc=1025, nf=0, w=(0.01, 0.0), reg_bytes=1 << 30),
               dict(stride=7), dict(nc=0)):
        assert call(**kw) == -1000, kw
        assert b"dn_render_rays_backward_reg" in lib.dn_last_error(), kw
    assert call(n=0, rays=None, ws=None, reg_ws=None, reg2=None) == 0


def test_steps_and_trainer_refuse_distortion_settings_they_cannot_honour(capsys):
    import nerf
    import train_dexnerf
    from nerf import synthetic as syn
    h = w = 8
    cfg = make_cfg(dict(num_coarse=16, num_fine=16, near=2.0, far=6.0))
    sel = types.SimpleNamespace(cams=torch.zeros(3, 16), height=h, width=w)
    for bad in ((-0.1, 0.0), (0.0, NAN), (INF, 0.0), (0.1,), (0.1, 0.1, 0.1), 0.1):
        with pytest.raises(ValueError, match="distortion_weights"):
            nerf.FusedTrainStep(None, None, sel, cfg, None, None, None, 16, distortion_weights=bad)
    e = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in (3, 9, 14)])
    k = torch.from_numpy(syn.intrinsic(h, w))
    images = torch.zeros(3, h, w, 3)
    with pytest.raises(ValueError, match="geometry route takes no distortion regulariser"):
        nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3, distortion_weights=(0.0, 0.01))
    with pytest.raises(ValueError, match="geometry route takes no distortion regulariser"):
        nerf.FusedJointStep(None, None, None, h, w, k, e, images, None, None, 4, None, None, 1e-3, distortion_weights=(0.01, 0.0))
    with pytest.raises(ValueError, match="distortion_weights"):
        nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3, distortion_weights=(0.0, -1.0))
    with pytest.raises(RuntimeError, match="ROCm device only"):     # zero weights are the default: the next check is the device one
        nerf.FusedPoseStep(None, None, None, h, w, k, e, images, None, None, num_rays=4, lr=1e-3, distortion_weights=(0.0, 0.0))
    for argv, word in ((["--distortion-weight", "-0.1"], "finite"), (["--distortion-weight", "nan"], "finite"),
                       (["--distortion-weight-coarse", "inf"], "finite"), (["--distortion-weight", "0.01", "--refine-poses"], "geometry route"),
                       (["--distortion-weight-coarse", "0.01", "--autograd-step"], "fused step")):
        with pytest.raises(SystemExit):
            train_dexnerf.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    args = train_dexnerf.parse_args(["--distortion-weight", "0.01"])
    assert (args.distortion_weight_coarse, args.distortion_weight) == (0.0, 0.01)


# ---- GPU: the kernel alone ------------------------------------------------------------------------------------------------------------
def pairwise64(weights, z, near_far, scale):
    """The float64 restatement, pairwise: (L_ray (N), mean, scale dL/dw, scale dL/dz, tied (N) bool).  `tied`: rows where two interval
    midpoints coincide - |m_i - m_j| is not differentiable in the depths there (torch's abs takes 0, the kernel the subgradient of
    the sorted order), so the depth gradient of such a row is not compared."""
    w = weights.detach().double().cpu().requires_grad_(True)
    zz = z.detach().double().cpu().requires_grad_(True)
    nf = near_far.detach().double().cpu()
    live = nf[:, 1] > nf[:, 0]
    k = torch.where(live, 1.0 / (nf[:, 1] - nf[:, 0]), torch.zeros_like(nf[:, 0]))[:, None]
    m = torch.cat([0.5 * (zz[:, :-1] + zz[:, 1:]), zz[:, -1:]], dim=1) * k
    delta = torch.cat([zz[:, 1:] - zz[:, :-1], torch.zeros_like(zz[:, -1:])], dim=1) * k
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(dim=(1, 2))
    ray = torch.where(live, pair + (w * w * delta).sum(dim=1) / 3.0, torch.zeros_like(pair))
    g_w, g_z = torch.autograd.grad(scale * ray.sum(), (w, zz))
    md = m.detach()
    tied = (md[:, 1:] == md[:, :-1]).any(dim=1) if md.shape[1] > 1 else torch.zeros(md.shape[0], dtype=torch.bool)
    return ray.detach(), ray.detach().mean(), g_w, g_z, tied & live


def make_case(n, s, dev, seed, real_weights):
    """Weights (from dn_volume_render on random rows, or random with exact zeros), sorted depths with equal neighbours worked in (rows
    0 mod 3: none; 1 mod 3: one equal pair inside the ray - still differentiable; 2 mod 3: three equal depths and an equal last pair -
    not), near / far per ray with far - near != 1."""
    from nerf import _ops
    g = torch.Generator().manual_seed(seed)
    near = 2.0 + 0.25 * torch.randint(0, 4, (n,), generator=g).float()
    far = near + 2.5 + 0.5 * torch.randint(0, 4, (n,), generator=g).float()
    z = near[:, None] + (far - near)[:, None] * torch.sort(torch.rand(n, s, generator=g), dim=1).values
    for r in range(n):
        if r % 3 == 1 and s >= 4:
            i = 1 + (7 * r) % (s - 3)
            z[r, i + 1] = z[r, i]
        if r % 3 == 2 and s >= 3:
            i = (5 * r) % (s - 2)
            z[r, i + 1] = z[r, i]; z[r, i + 2] = z[r, i]
            z[r, s - 1] = z[r, s - 2]
    z = z.to(dev).contiguous()
    if real_weights:
        rf = torch.randn(n, s, 4, generator=g)
        rf[..., 3] = rf[..., 3] * 3.0 + 0.5
        rd = torch.randn(n, 3, generator=g)
        weights = _ops.volume_render_fwd(rf.to(dev), z, rd.to(dev), None, 0.0, False, [])[3]
    else:
        weights = torch.rand(n, s, generator=g) * (torch.rand(n, s, generator=g) > 0.3).float()
        weights.view(-1)[::5] = 0.0
        weights = weights.to(dev)
    return weights.contiguous(), z, torch.stack([near, far], dim=1).to(dev).contiguous()


SHAPES = [(1, 1), (3, 2), (5, 63), (4, 64), (5, 65), (3, 192), (2, 1024), (1025, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("real_weights", [True, False], ids=["rendered", "random"])
@pytest.mark.parametrize("n,s", SHAPES)
def test_kernel_against_pairwise_float64(dev, n, s, real_weights):
    from nerf import _ops
    weights, z, near_far = make_case(n, s, dev, 100 * s + n, real_weights)
    scale = 0.37
    mean, ray_loss, g_w, g_z = _ops.distortion_loss(weights, z, near_far, scale=scale, want_z=True)
    ray64, mean64, g_w64, g_z64, tied = pairwise64(weights, z, near_far, scale)
    smooth = ~tied
    errs = dict(mean=rel_err(C(mean)[0], mean64.numpy()), ray=rel_err(C(ray_loss), ray64.numpy()), g_w=rel_err(C(g_w), g_w64.numpy()),
                g_z=rel_err(C(g_z)[smooth.numpy()], g_z64[smooth].numpy()) if bool(smooth.any()) else 0.0)
    print(f"distortion ({n},{s}) {'rendered' if real_weights else 'random'} weights: rel err " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f"; {int(tied.sum())} tied rows, mean L {float(mean64):.5f}")
    assert ray_loss.dtype == torch.float64 and g_w.shape == g_z.shape == (n, s) and mean.shape == (1,)
    if s == 1:      # a single sample has no spread and no interval: exact zeros
        assert not bool(mean.any()) and not bool(ray_loss.any()) and not bool(g_w.any()) and not bool(g_z.any())
    else:
        assert float(mean64) > 0 and float(g_z64.abs().max()) > 0
    if n >= 3 and s >= 4:
        assert bool(tied.any()) and bool(smooth.any())
    assert all(v <= TOL for v in errs.values()), errs
    # the tied rows: the subgradient stays finite (and is the sorted order's: checked in test_tied_depths_take_the_sorted_order below)
    assert bool(torch.isfinite(g_z).all())
    # two runs: the same bits, and nothing depends on what the outputs held before
    again = _ops.distortion_loss(weights, z, near_far, scale=scale, want_z=True)
    for a, b in zip((mean, ray_loss, g_w, g_z), again):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_tied_depths_take_the_sorted_order(dev):
    """Three equal depths: moving the later of the tied samples up by an ulp-sized step makes the row differentiable without changing
    the order, and the kernel's depth gradient on the tied row is the limit of those - checked against float64 on the nudged row."""
    from nerf import _ops
    z = torch.tensor([[2.5, 3.0, 3.0, 3.0, 4.0, 5.5]], device=dev)
    nudged = torch.tensor([[2.5, 3.0, 3.0 + 2e-6, 3.0 + 4e-6, 4.0, 5.5]], device=dev)
    weights = torch.tensor([[0.1, 0.3, 0.2, 0.15, 0.05, 0.1]], device=dev)
    near_far = torch.tensor([[2.0, 6.0]], device=dev)
    got = _ops.distortion_loss(weights, z, near_far, scale=1.0, want_z=True)
    _, _, g_w64, g_z64, tied = pairwise64(weights, nudged, near_far, 1.0)
    assert not bool(tied.any()) and bool(pairwise64(weights, z, near_far, 1.0)[4].all())
    assert rel_err(C(got[3]), g_z64.numpy()) <= TOL and rel_err(C(got[2]), g_w64.numpy()) <= 1e-5 + 4e-6


@pytest.mark.gpu
@pytest.mark.parametrize("s,at", [(2, 0), (65, 63), (65, 64), (192, 100), (192, 191)])
def test_one_sample_ray_is_w_squared_delta_over_three(dev, s, at):
    from nerf import _ops
    z = (2.0 + 4.0 * torch.sort(torch.rand(1, s, generator=torch.Generator().manual_seed(s))).values).to(dev)
    weights = torch.zeros(1, s, device=dev)
    weights[0, at] = 0.8125
    near_far = torch.tensor([[1.5, 6.5]], device=dev)
    mean, ray_loss, g_w, g_z = _ops.distortion_loss(weights, z, near_far, want_z=True)
    zd = z.double().cpu()[0]
    delta = float(zd[at + 1] - zd[at]) / 5.0 if at + 1 < s else 0.0      # the last sample's interval is degenerate
    want = 0.8125 ** 2 * delta / 3.0
    assert abs(float(ray_loss[0]) - want) <= 1e-12 * max(want, 1e-30) + 1e-300
    assert abs(float(mean[0]) - want) <= 2.0 ** -23 * want
    if at + 1 < s:
        assert float(mean[0]) > 0


@pytest.mark.gpu
def test_rays_without_a_span_give_zeros_and_accumulate_mode_adds(dev):
    from nerf import _ops
    n, s = 9, 70
    weights, z, near_far = make_case(n, s, dev, 7, False)
    dead = [1, 4, 6]
    near_far[1, 1] = near_far[1, 0]          # far == near
    near_far[4, 1] = near_far[4, 0] - 1.0    # far < near
    near_far[6, 1] = NAN
    mean, ray_loss, g_w, g_z = _ops.distortion_loss(weights, z, near_far, scale=2.0, want_z=True)
    for r in dead:
        assert float(ray_loss[r]) == 0.0 and not bool(g_w[r].any()) and not bool(g_z[r].any())
    nf64 = near_far.clone()
    nf64[6, 1] = nf64[6, 0]
    ray64, mean64, g_w64, g_z64, tied = pairwise64(weights, z, nf64, 2.0)
    assert rel_err(C(mean)[0], mean64.numpy()) <= TOL and rel_err(C(g_w), g_w64.numpy()) <= TOL and float(mean64) > 0
    # the ray rows form: near / far read from columns 6:8 of packed rows - the same bits
    rows = torch.zeros(n, 11, device=dev)
    rows[:, 6:8] = near_far
    by_rows = _ops.distortion_loss(weights, z, rays=rows, scale=2.0, want_z=True)
    for a, b in zip((mean, ray_loss, g_w, g_z), by_rows):
        assert torch.equal(a, b)
    # accumulate mode: added to what is there (one fp32 addition per element), dead rays untouched
    before = torch.randn(n, s, device=dev)
    total = before.clone()
    out = _ops.distortion_loss(weights, z, near_far, scale=2.0, g_z=total)
    assert out[3] is total and torch.equal(total, before + g_z) and torch.equal(out[2], g_w)
    for r in dead:
        assert torch.equal(total[r], before[r])
    # without want_z no depth gradient is formed
    assert _ops.distortion_loss(weights, z, near_far, scale=2.0)[3] is None
    with pytest.raises(ValueError, match="one of them"):
        _ops.distortion_loss(weights, z)
    # an empty batch
    empty = _ops.distortion_loss(weights[:0], z[:0], near_far[:0], want_z=True)
    assert empty[0].tolist() == [0.0] and empty[2].shape == (0, s)


@pytest.mark.gpu
@pytest.mark.parametrize("grad_output", [1.0, -2.5])
def test_distortion_loss_under_autograd(dev, grad_output):
    import nerf
    n, s = 6, 40
    weights, z, _ = make_case(n, s, dev, 11, True)
    # (rows 2 and 5 hold tied depths: compared in the weights only, below)
    lead_w = weights.reshape(2, 3, s).clone().requires_grad_(True)
    lead_z = z.reshape(2, 3, s).clone().requires_grad_(True)
    loss = nerf.distortion_loss(lead_w, lead_z, 2.0, 6.0)
    assert loss.shape == () and loss.requires_grad
    (loss * grad_output).backward()
    near_far = torch.tensor([[2.0, 6.0]], device=dev).expand(n, 2)
    ray64, mean64, g_w64, g_z64, tied = pairwise64(weights, z, near_far, grad_output / n)
    smooth = (~tied).numpy()
    assert rel_err(float(loss.detach()), float(mean64)) <= TOL
    assert rel_err(C(lead_w.grad).reshape(n, s), g_w64.numpy()) <= TOL
    assert smooth.any() and rel_err(C(lead_z.grad).reshape(n, s)[smooth], g_z64.numpy()[smooth]) <= TOL
    # weights alone: no depth gradient is formed; per-ray near / far tensors
    w_only = weights.clone().requires_grad_(True)
    nerf.distortion_loss(w_only, z, near_far[:, 0].contiguous(), near_far[:, 1].contiguous()).backward()
    assert rel_err(C(w_only.grad) * grad_output, g_w64.numpy()) <= TOL
    # behind volume_render_radiance_field's weights on the eager route: the gradient reaches the radiance field
    rf = torch.randn(n, s, 4, device=dev).requires_grad_(True)
    out = nerf.volume_render_radiance_field(rf, z, torch.randn(n, 3, device=dev))
    nerf.distortion_loss(out[3], z, 2.0, 6.0).backward()
    assert rf.grad is not None and float(rf.grad[..., 3].abs().max()) > 0 and not bool(rf.grad[..., :3].any())
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.distortion_loss(weights.cpu(), z.cpu(), 2.0, 6.0)


# ---- GPU: the fused step --------------------------------------------------------------------------------------------------------------
REG = (0.0625, 0.125)         # both exact in fp32, as is their quotient by the 256 rays of the step


def workspace_views(saved):
    """(z_c, rf_c, w_c, z_f, rf_f) of a training workspace - dn_render_train_workspace_bytes' layout: 256-byte aligned fp32 blocks."""
    n, nc, nf = saved["n"], saved["nc"], saved["nf"]
    words = saved["ws"].view(torch.float32)
    out, off = [], 0
    for count, shape in ((n * nc, (n, nc)), (n * nc * 4, (n, nc, 4)), (n * nc, (n, nc)), (n * (nc + nf), (n, nc + nf)), (n * (nc + nf) * 4, (n, nc + nf, 4))):
        out.append(words[off:off + count].reshape(shape))
        off += (count * 4 + 255) // 256 * 64
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_route_never_reaches_the_new_entry_point(dev, scene, precision, monkeypatch):
    """Default arguments, and (0, 0) given explicitly: the step calls dn_render_rays_backward_ws as ever (the new entry point raises
    here), exposes no reg2, and three steps end in the same weights, bit for bit."""
    import nerf
    from nerf import _hip
    nerf.set_precision(precision)
    lib = _hip.lib()
    real = lib.dn_render_rays_backward_reg

    def boom(*a, **k):
        raise AssertionError("the default route reached dn_render_rays_backward_reg")
    results = []
    for kw in (dict(), dict(distortion_weights=(0.0, 0.0)), dict(distortion_weights=(0, 0))):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", **kw)
        assert step.reg2 is None and step.distortion_weights == (0.0, 0.0)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        with monkeypatch.context() as mp:
            mp.setattr(lib, "dn_render_rays_backward_reg", boom)
            for _ in range(3):
                step.forward_backward()
                opt.step()
        assert lib.dn_render_rays_backward_reg is real
        assert step.loss6 is None and step.loss3.shape == (3,)
        results.append((flat_params(nets), step.loss3.clone()))
    for params, loss3 in results[1:]:
        assert torch.equal(params, results[0][0]) and torch.equal(loss3, results[0][1])
    assert bool(torch.isfinite(results[0][0]).all())
    # and a step with the term does reach it
    step, bucket, nets = train_step(scene, dev, draw_view="rays", distortion_weights=REG)
    with monkeypatch.context() as mp:
        mp.setattr(lib, "dn_render_rays_backward_reg", boom)
        with pytest.raises(AssertionError, match="reached dn_render_rays_backward_reg"):
            step.forward_backward()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_regularised_step_is_the_chain_of_its_pieces(dev, scene, precision):
    """One step with distortion_weights = REG against dn_render_rays_train -> dn_mse2_loss -> per network: dn_volume_render for the
    weights -> dn_distortion_loss -> dn_volume_render_backward(g_weights) -> dn_mlp_backward_data -> dn_mlp_weight_grad_all, on the
    step's own rows and draws: reg2 and every weight gradient bit for bit.  The step runs as its two halves (nets = 2, then nets = 1:
    one weight-gradient launch per network, as in the chain); the one-call form sums both networks' partials in one launch and is
    compared with the halves in test_replayed_halved_and_reseeded_steps."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    step, bucket, nets = train_step(scene, dev, seed=31, first_iteration=2, draw_view="rays", distortion_weights=REG)
    peek = _ops.new_rng_state(31, dev, 2)
    bucket.zero()
    step.forward_and_fine_backward(_zero=False)
    step.coarse_backward()
    assert step.rng_state.tolist()[2:] == [2, 3] and step.loss6 is None
    _, _, rows, target = step.latest_draw()
    assert rows.shape == (TRAIN_RAYS, 11)
    mc, mf = nets
    got = [(m.weight.grad.clone(), m.bias.grad.clone()) for net in nets for m in net.linear_modules()]
    pc, pf, prec = _ops.pack_train_pair(mc, mf, step.logs)
    maps, saved = _ops.render_rays_train(pc, pf, rows, 16, 16, False, 0.0, False, [], None, prec=prec, rng_state=peek, perturb=True)
    loss3, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target)
    assert torch.equal(loss3, step.loss3)
    z_c, rf_c, w_c, z_f, rf_f = workspace_views(saved)
    rd = rows[:, 3:6]
    want, plain, reg2 = [], [], []
    for packed, model, z, rf, kept, g_rgb, act, masks, weight in ((pc, mc, z_c, rf_c, w_c, g_c, saved["act_c"], saved["masks_c"], REG[0]),
                                                                    (pf, mf, z_f, rf_f, None, g_f, saved["act_f"], saved["masks_f"], REG[1])):
        n_points = z.numel()
        weights = _ops.volume_render_fwd(rf, z, rd, None, 0.0, False, [])[3]
        if kept is not None:
            assert torch.equal(weights, kept)          # the coarse weights the forward left in the workspace are these
        mean, _, g_w, _ = _ops.distortion_loss(weights, z, rays=rows, scale=weight / TRAIN_RAYS)
        reg2.append(mean)
        for sink, upstream in ((want, g_w), (plain, None)):
            g_rf = _ops.volume_render_bwd(rf, z, rd, None, 0.0, False, g_rgb, None, None, None, upstream)
            grads = _ops.mlp_backward_data(packed, g_rf, masks, n_points, prec=prec)
            views = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in model.linear_modules()], dev)
            _ops.mlp_weight_grad_all_into(packed, act, grads, n_points, views, prec=prec)
            sink.extend(views)
    reg2 = torch.cat(reg2)
    print(f"regularised chain {precision}: loss3 {step.loss3.tolist()} reg2 {step.reg2.tolist()}")
    assert torch.equal(step.reg2, reg2) and float(reg2.min()) > 0
    for (gw, gb), (ww, wb) in zip(got, want):
        assert float(ww.abs().max()) > 0 and torch.equal(gw, ww) and torch.equal(gb, wb)
    # the term reaches the weights of both networks: the photometric backward on the same forward gives other gradients
    n_c = len(list(mc.linear_modules()))
    assert not torch.equal(plain[0][0], want[0][0]) and not torch.equal(plain[n_c][0], want[n_c][0])
    # the new entry point with both weights 0 is the old one, bit for bit, and writes no reg2 word
    outs = []
    for reg in (None, ((0.0, 0.0), torch.full((2,), -7.0, device=dev))):
        v_c = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mc.linear_modules()], dev)
        v_f = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mf.linear_modules()], dev)
        _ops.render_rays_backward(pc, pf, saved, (g_c, None, None), (g_f, None, None), v_c, v_f, nets=3, reg=reg)
        outs.append(v_c + v_f)
        if reg is not None:
            assert reg[1].tolist() == [-7.0, -7.0]
    for (aw, ab), (bw, bb) in zip(*outs):
        assert torch.equal(aw, bw) and torch.equal(ab, bb)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replayed_halved_and_reseeded_steps(dev, scene, precision):
    """Four optimizer steps: replayed graphs equal eager launches and a second eager run of the same seed, bit for bit in the weights
    and in reg2; another seed gives another run.  The two data-parallel halves against the one-call step: reg2 bit for bit, the
    gradients at the 1e-4 at which test_render_loss gates the other order of the weight-gradient partial sums (fp32)."""
    import nerf
    nerf.set_precision(precision)
    runs = []
    for use_graphs, seed in ((False, 31), (True, 31), (False, 31), (False, 32)):
        step, bucket, nets = train_step(scene, dev, seed=seed, draw_view="rays", distortion_weights=REG)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1, use_graphs=use_graphs)
        for _ in range(4):
            graphed.step()
        torch.cuda.synchronize()
        assert graphed.fallback_reason is None and (graphed.graphs is not None) == use_graphs, graphed.fallback_reason
        assert step.rng_state.tolist()[2:] == [3, 4]
        runs.append((flat_params(nets), step.reg2.clone(), step.loss3.clone()))
    for other in runs[1:3]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[3][0]) and not torch.equal(runs[0][1], runs[3][1])
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][1].min()) > 0
    if precision != "fp32":
        return
    halves = []
    for both in (True, False):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", distortion_weights=REG)
        bucket.zero()
        step.forward_and_fine_backward(_zero=False, both=both)
        if not both:
            assert float(step.reg2[1]) > 0 and float(step.reg2[0]) == 0.0      # each half writes its own word
            step.coarse_backward()
        halves.append(([p.grad.clone() for p in bucket.params], step.reg2.clone()))
    assert torch.equal(halves[0][1], halves[1][1]) and float(halves[0][1].min()) > 0
    for a, b in zip(halves[0][0], halves[1][0]):
        assert float(a.abs().max()) > 0 and rel_err(C(b), C(a)) <= 1e-4


EFFECT_STEPS = 300
EFFECT_WEIGHTS = (0.0, 0.01)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_term_lowers_the_fine_distortion(dev, scene, precision):
    """300 steps from one seed with distortion_weights = (0, 0.01) - the weight mip-NeRF 360 publishes for this term - and without the
    term (the same student, the same draws); then every pixel of view 1, without jitter: the fine network's mean L_ray must be strictly
    lower with the term, and its mse finite.  Only "lower" is gated.  Measured on an MI355X: 0.0282 against 0.3204 (ratio 0.088) in
    fp32, 0.0279 against 0.3366 (0.083) in bf16; fine mse 5.7e-3 against 2.0e-4 and 1.1e-3 against 2.0e-4.  On this 3-view scene the
    term buys its low distortion by moving density onto the last sample (profiles/distortion_loss.md has the sweep of weights)."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    pix = torch.arange(scene.sel.height * scene.sel.width, device=dev)
    rows, target = scene.sel.select(pix, view=torch.ones(pix.numel(), dtype=torch.int32, device=dev))
    final = {}
    for weights in ((0.0, 0.0), EFFECT_WEIGHTS):
        step, bucket, nets = train_step(scene, dev, draw_view="rays", distortion_weights=weights)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1)
        for _ in range(EFFECT_STEPS):
            graphed.step()
        torch.cuda.synchronize()
        assert graphed.fallback_reason is None, graphed.fallback_reason
        pc, pf, prec = _ops.pack_train_pair(nets[0], nets[1], step.logs)
        maps, saved = _ops.render_rays_train(pc, pf, rows, 16, 16, False, 0.0, False, [], None, prec=prec, rng_state=None, perturb=False)
        z_c, rf_c, w_c, z_f, rf_f = workspace_views(saved)
        w_f = _ops.volume_render_fwd(rf_f, z_f, rows[:, 3:6], None, 0.0, False, [])[3]
        dist = float(_ops.distortion_loss(w_f, z_f, rays=rows)[0])
        mse = float(((maps[3] - target) ** 2).mean())
        final[weights] = (dist, mse, float(maps[5].mean()))
    (d0, m0, a0), (d1, m1, a1) = final[(0.0, 0.0)], final[EFFECT_WEIGHTS]
    print(f"{precision}: after {EFFECT_STEPS} steps, fine mean distortion / mse / acc on view 1 without the term {d0:.6f} / {m0:.6f} / {a0:.4f}, "
          f"with {EFFECT_WEIGHTS} {d1:.6f} / {m1:.6f} / {a1:.4f}; distortion ratio {d1 / d0:.4f}")
    assert np.isfinite([d0, m0, d1, m1]).all()
    assert d1 < d0
