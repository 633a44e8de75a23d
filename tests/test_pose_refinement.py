"""Pose refinement on the library's kernels: nerf.se3_exp, the end-to-end chain xi -> E = se3_exp(xi) @ E0 -> select_camera_rays ->
predict_and_render_radiance -> loss -> dL/dxi against float64 autograd through the oracle, and nerf.PoseRefiner.

Tolerances use the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from golden_cases import CASES
from test_input_gradients import POSE_XI, make_cfg, make_models, no_fallback

H = W = 400


# ---- se3_exp (CPU) --------------------------------------------------------------------------------------------------------------------
def twist64(xi):
    wx, wy, wz, tx, ty, tz = [float(v) for v in xi]
    return torch.tensor([[0.0, -wz, wy, tx], [wz, 0.0, -wx, ty], [-wy, wx, 0.0, tz], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)


@pytest.mark.parametrize("xi", [POSE_XI, (0.7, -1.1, 0.4, 2.0, -3.0, 0.5), (0.0, 0.0, 0.0, 1.0, 2.0, 3.0), (1e-9, 0.0, 0.0, 0.0, 0.0, 0.0)])
def test_se3_exp_is_the_matrix_exponential_of_the_twist(xi):
    import nerf
    got = nerf.se3_exp(torch.tensor(xi, dtype=torch.float64))
    want = torch.linalg.matrix_exp(twist64(xi))
    assert rel_err(got.numpy(), want.numpy()) <= 1e-12
    rot = got[:3, :3]
    assert float((rot @ rot.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12
    assert float((got[3] - torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).abs().max()) <= 1e-15


def test_se3_exp_at_zero_is_the_identity_with_a_finite_gradient():
    import nerf
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    m = nerf.se3_exp(xi)
    assert torch.equal(m.detach(), torch.eye(4, dtype=torch.float64))
    coeff = torch.arange(1.0, 17.0, dtype=torch.float64).reshape(4, 4)
    (m * coeff).sum().backward()
    assert torch.isfinite(xi.grad).all()
    # d exp(xi) / d xi at 0 is the twist's generator: d/d omega_x = e_21 - e_12, ..., d/d t_x = e_03, ...
    want = torch.tensor([coeff[2, 1] - coeff[1, 2], coeff[0, 2] - coeff[2, 0], coeff[1, 0] - coeff[0, 1], coeff[0, 3], coeff[1, 3], coeff[2, 3]])
    assert rel_err(xi.grad.numpy(), want.numpy()) <= 1e-12
    x32 = torch.zeros(6, dtype=torch.float32, requires_grad=True)
    nerf.se3_exp(x32).sum().backward()
    assert torch.isfinite(x32.grad).all()


def test_pose_refiner_is_device_only():
    import nerf
    from nerf import synthetic as syn
    e0, k = torch.from_numpy(syn.scene_pose(9)), torch.from_numpy(syn.intrinsic(8, 8))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        nerf.PoseRefiner(None, None, None, 8, 8, k, e0, None, None, num_rays=4, lr=1e-3)


# ---- the end-to-end chain -------------------------------------------------------------------------------------------------------------
def camera_pose_problem():
    """Pose 9 of the synthetic scene at 400 x 400, the 256 pixels of the fixed selection seed 77 (none chosen or dropped by its
    behaviour), a fixed random target: (E0, K) fp32, pixel indices (row-major int64), target (256,3) float64."""
    from nerf import synthetic as syn
    e0, k = torch.from_numpy(syn.scene_pose(9)), torch.from_numpy(syn.intrinsic(H, W))
    sel = torch.from_numpy(syn.select_rays(H, W, 256, seed=77)).to(torch.int64)
    target = torch.rand(256, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return e0, k, sel, target


def oracle_camera_pose_gradient(dtype):
    """dL/dxi through the oracle: E = exp(twist(xi)) E0 in float64, then - in `dtype` - get_ray_bundle, the selection, run_one_iter
    (lego weights, 64 + 64 samples, perturb off, noise 0) and the coarse + fine MSE."""
    from oracle import nerf_oracle as oc
    e0, k, sel, target = camera_pose_problem()
    mkw, wfn, rkw = CASES["render_lego_val"]
    sd_c, sd_f = wfn()
    tsd_c = {n: torch.from_numpy(v).to(dtype) for n, v in sd_c.items()}
    tsd_f = {n: torch.from_numpy(v).to(dtype) for n, v in sd_f.items()}
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    zero = torch.zeros((), dtype=torch.float64)
    twist = torch.stack([torch.stack([zero, -xi[2], xi[1], xi[3]]), torch.stack([xi[2], zero, -xi[0], xi[4]]),
                         torch.stack([-xi[1], xi[0], zero, xi[5]]), torch.stack([zero, zero, zero, zero])])
    e_mat = torch.linalg.matrix_exp(twist) @ e0.double()
    ro, rd = oc.get_ray_bundle(H, W, e_mat.to(dtype), k.to(dtype))
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    cfg_o = oc.RenderCfg(chunksize=4096, m_thres=(), num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"], near=rkw["near"], far=rkw["far"],
                         white_background=rkw["white_background"])
    mcfg = oc.ModelCfg(**mkw)
    out = oc.run_one_iter(ro, rd, tsd_c, tsd_f, mcfg, mcfg, cfg_o)
    mse = torch.nn.functional.mse_loss
    loss = mse(out[0], target.to(dtype)) + mse(out[3], target.to(dtype))
    loss.backward()
    return xi.grad.numpy().copy()


CAMERA_POSE_FLOOR = 3.17e-2   # oracle_camera_pose_floor()[0] as measured on the build machine's CPU; the gate below is pinned to it.  (70 x the
# floor of test_input_gradients' ray-space pose test: here the fp32 run also forms E's two inverses and the bundle in fp32, which moves more
# inverse-CDF resamples across a bin edge than rounding the rays does - with the bundle formed in float64 and only the rays rounded, the same
# measurement gives 1.7e-3.)


def oracle_camera_pose_floor():
    """The oracle's own fp32-vs-float64 difference of dL/dxi on this chain (max-norm, relative).  How CAMERA_POSE_FLOOR was measured;
    the test does not re-measure it, so a numerically worse oracle run cannot widen the gate."""
    g64 = oracle_camera_pose_gradient(torch.float64)
    return rel_err(oracle_camera_pose_gradient(torch.float32), g64), g64


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
    """(coarse, fine) lego-shaped networks with frozen parameters, the encoders and the render options."""
    import nerf
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    return mc, mf, nerf.get_embedding_function(10), nerf.get_embedding_function(4), make_cfg(rkw), rkw


@pytest.fixture(scope="module")
def library_pose_gradient(dev, lego):
    """dL/dxi of the chain on the library, computed once (the tests below leave it unchanged)."""
    import nerf
    mc, mf, ex, ed, cfg, rkw = lego
    e0, k, sel, target = camera_pose_problem()
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    e_mat = nerf.se3_exp(xi) @ e0.double()
    rows, _ = nerf.select_camera_rays(H, W, e_mat, k, rkw["near"], rkw["far"], sel.to(dev))
    assert rows.grad_fn is not None
    out = nerf.predict_and_render_radiance(rows, mc, mf, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
    tgt = target.float().to(dev)
    (nerf.img2mse(out[0], tgt) + nerf.img2mse(out[3], tgt)).backward()
    return xi.grad.clone()


@pytest.mark.gpu
def test_camera_pose_gradient_end_to_end_against_the_float64_oracle(dev, lego, monkeypatch):
    """xi -> E = se3_exp(xi) @ E0 -> select_camera_rays -> predict_and_render_radiance -> coarse + fine MSE, fp32 mode, under
    no_fallback: dL/dxi against float64 autograd of the whole chain through the oracle.  The gate follows
    test_input_gradients.test_pose_gradient_end_to_end_against_the_float64_oracle: max(1e-3, 4 x floor), floor = the oracle's own
    fp32-vs-float64 difference on this chain, measured once on the CPU (oracle_camera_pose_floor) and recorded as CAMERA_POSE_FLOOR.
    Measured on an MI355X: the library is 1.71e-3 from the float64 oracle, against a gate of 1.27e-1 - the recipe's gate is loose here
    because the oracle's own fp32 run is (3.17e-2), so this test guards the routing of the chain (no fallback, every stage carries the
    gradient, the right sign and scale); the accuracy of the camera gradient itself is held to 1e-5 in test_camera_gradients.py, and that of
    the ray gradient behind it in test_ray_gradients.py / test_input_gradients.py."""
    import nerf
    mc, mf, ex, ed, cfg, rkw = lego
    e0, k, sel, target = camera_pose_problem()
    g64 = oracle_camera_pose_gradient(torch.float64)
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    with no_fallback(monkeypatch):
        rows, _ = nerf.select_camera_rays(H, W, nerf.se3_exp(xi) @ e0.double(), k, rkw["near"], rkw["far"], sel.to(dev))
        out = nerf.predict_and_render_radiance(rows, mc, mf, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
        tgt = target.float().to(dev)
        (nerf.img2mse(out[0], tgt) + nerf.img2mse(out[3], tgt)).backward()
    err = rel_err(xi.grad.numpy(), g64)
    gate = max(1e-3, 4.0 * CAMERA_POSE_FLOOR)
    print(f"camera pose gradient: oracle fp32-vs-float64 floor {CAMERA_POSE_FLOOR:.3e}, gate {gate:.3e}, library vs float64 oracle {err:.3e}, "
          f"dL/dxi {g64}")
    assert err <= gate, (err, gate, CAMERA_POSE_FLOOR)


def _refiner(dev, lego, seed, num_rays=256):
    import nerf
    mc, mf, ex, ed, cfg, _ = lego
    e0, k, _, _ = camera_pose_problem()
    return nerf.PoseRefiner(mc, mf, cfg, H, W, k.to(dev), e0.to(dev), ex, ed, num_rays=num_rays, lr=1e-3, seed=seed)


@pytest.mark.gpu
def test_pose_refiner_first_step_gradient_is_the_end_to_end_gradient(dev, lego, library_pose_gradient):
    """Started at POSE_XI and given the same pixels (the target pixels scattered into an image), the first step's xi.grad is the
    gradient of the chain above, bit for bit; the step moves xi and extrinsic() follows it."""
    import nerf
    e0, _, sel, target = camera_pose_problem()
    image = torch.zeros(H * W, 3, device=dev)
    image[sel.to(dev)] = target.float().to(dev)
    ref = _refiner(dev, lego, seed=0)
    with torch.no_grad():
        ref.xi.copy_(torch.tensor(POSE_XI, dtype=torch.float64))
    loss = ref.step(image.reshape(H, W, 3), pixel_index=sel.to(dev))
    assert loss.dim() == 0 and not loss.requires_grad and float(loss) > 0
    assert torch.equal(ref.last_grad, library_pose_gradient)
    assert not torch.equal(ref.xi.detach(), torch.tensor(POSE_XI, dtype=torch.float64))
    est = ref.extrinsic()
    assert est.is_cuda and not est.requires_grad
    want = nerf.se3_exp(ref.xi.detach()) @ e0.double()
    assert rel_err(est.cpu().numpy(), want.numpy()) <= 1e-6


@pytest.mark.gpu
def test_pose_refiner_is_reproducible_and_leaves_the_networks_alone(dev, lego):
    """Two refiners with the same seed end three steps with bit-identical xi; another seed draws other pixels; the networks'
    requires_grad flags are what they were (here: mixed) and no parameter has a .grad."""
    mc, mf = lego[0], lego[1]
    params = list(mc.parameters()) + list(mf.parameters())
    flags = [i % 2 == 0 for i in range(len(params))]
    for p, flag in zip(params, flags):
        p.requires_grad_(flag)
    try:
        image = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        a, b = _refiner(dev, lego, seed=4, num_rays=192), _refiner(dev, lego, seed=4, num_rays=192)
        for _ in range(3):
            la, lb = a.step(image), b.step(image)
            assert torch.equal(la, lb)
        assert torch.equal(a.xi.detach(), b.xi.detach()) and float(a.xi.detach().abs().max()) > 0
        assert [p.requires_grad for p in params] == flags and all(p.grad is None for p in params)
        c = _refiner(dev, lego, seed=5, num_rays=192)
        pa, pc = _refiner(dev, lego, seed=4, num_rays=192).draw_pixels(), c.draw_pixels()
        assert pa.numel() == 192 and pa.unique().numel() == 192 and not torch.equal(pa, pc)
    finally:
        for p in params:
            p.requires_grad_(False)
