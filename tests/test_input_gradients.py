"""Input gradients of the fused network: dL/d(points), dL/d(view directions), dL/d(ray rows), dL/d(depths) from
dn_mlp_backward_input (csrc/mlp_input_grad.hip), the autograd function on top of it (_train.FusedNetInputFn) and the routing of
run_network / predict_and_render_radiance / run_one_iter_of_nerf for inputs that require grad (pose / ray optimisation).

Tolerances use the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES

NEW_SYMBOLS = ("dn_mlp_input_grad_packed_bytes", "dn_mlp_pack_input_grad", "dn_mlp_backward_input_workspace_bytes",
               "dn_mlp_backward_input")


def C(t):
    return t.detach().cpu().numpy()


def mlp_desc(l_xyz=10, depth=4, width=128, viewdirs=1, skip=4):
    from nerf import _hip
    return _hip.MlpDesc(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=l_xyz, num_encoding_fn_dir=4,
                        include_input_xyz=1, include_input_dir=1, use_viewdirs=viewdirs, log_sampling_xyz=1, log_sampling_dir=1)


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_resolvable(hiplib):
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(raw, name), name
    assert hiplib.dn_abi_version() == 2      # additive: the ABI version stays


def test_argument_validation_returns_before_gpu_work(hiplib):
    """NULL descriptor -> DN_E_INVAL; fp16 and the 8-bit-saved layout -> DN_E_UNSUPPORTED with a message; a width outside the kernels ->
    DN_E_UNSUPPORTED.  No pointer is dereferenced (the device pointers here are small integers)."""
    from nerf import _hip
    fake = ctypes.c_void_p(256)
    d = mlp_desc()

    def call(desc, prec, packed=fake, grads=fake):
        return hiplib.dn_mlp_backward_input(desc, prec, packed, grads, fake, fake, None, 0, None, 4, 8, fake, fake, None, None, fake, 1 << 20, None)
    assert call(None, _hip.PREC_F32) == -1000
    assert b"NULL descriptor" in hiplib.dn_last_error()
    for prec in (_hip.PREC_F16, _hip.PREC_BF16_S8):
        assert call(ctypes.byref(d), prec) == -1001
        assert b"16-bit saved tensors" in hiplib.dn_last_error()
        assert hiplib.dn_mlp_input_grad_packed_bytes(ctypes.byref(d), prec) == 0
        assert hiplib.dn_mlp_pack_input_grad(ctypes.byref(d), prec, None, fake, None) == -1001
    wide = mlp_desc(width=192)
    assert call(ctypes.byref(wide), _hip.PREC_F32) == -1001
    assert hiplib.dn_mlp_input_grad_packed_bytes(ctypes.byref(wide), _hip.PREC_F32) == 0
    assert call(ctypes.byref(mlp_desc(l_xyz=8)), _hip.PREC_BF16) == -1001
    # supported descriptor, bad pointers / sizes: still before any launch
    assert call(ctypes.byref(d), _hip.PREC_F32, packed=None) == -1000
    assert hiplib.dn_mlp_backward_input(ctypes.byref(d), _hip.PREC_F32, fake, fake, None, None, fake, 8, fake, 4, 8, None, None, fake, fake,
                                        fake, 1 << 20, None) == -1000          # ray rows of a view-direction net need 11 columns
    assert b"ray_stride" in hiplib.dn_last_error()
    assert hiplib.dn_mlp_backward_input(ctypes.byref(d), _hip.PREC_F32, fake, fake, fake, fake, None, 0, None, 4, 8, fake, fake, None, None,
                                        fake, 16, None) == -1000               # workspace too small
    assert b"workspace" in hiplib.dn_last_error()


def test_input_grad_stream_size(hiplib):
    """The stream is whole 1 KiB pieces: two 32-row tiles x W / kpp pieces per xyz stage (layer1 + the wide trunk layers) and one tile x
    W / 2 / kpp pieces for layers_dir.0; a net without view directions holds exactly the xyz stages."""
    from nerf import _hip
    for prec, kpp in ((_hip.PREC_F32, 8), (_hip.PREC_BF16, 16)):
        for depth, width, skip, n_x in ((4, 128, 4, 1), (8, 256, 4, 2), (9, 128, 2, 4)):
            kh = width // kpp
            with_dirs = hiplib.dn_mlp_input_grad_packed_bytes(ctypes.byref(mlp_desc(10, depth, width, 1, skip)), prec)
            without = hiplib.dn_mlp_input_grad_packed_bytes(ctypes.byref(mlp_desc(10, depth, width, 0, skip)), prec)
            assert with_dirs % 1024 == 0 and without % 1024 == 0
            assert without == n_x * 2 * kh * 1024
            assert with_dirs - without == (kh // 2) * 1024
    d = mlp_desc()
    assert hiplib.dn_mlp_backward_input_workspace_bytes(ctypes.byref(d), 1000, 1) >= 2 * 12000
    assert hiplib.dn_mlp_backward_input_workspace_bytes(ctypes.byref(mlp_desc(viewdirs=0)), 1000, 0) == 0


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
def _restore_modes():
    import nerf
    nerf.set_render_policy("bf16")
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


@contextlib.contextmanager
def no_fallback(monkeypatch):
    """The fused route or an error: the nn.Linear composition and the torch-encoding fallback raise while the block runs."""
    import nerf
    from nerf import _train

    def boom(*a, **k):
        raise AssertionError("the call left the fused kernels")
    with monkeypatch.context() as mp:
        mp.setattr(nerf.models.FlexibleNeRFModel, "_forward_modules", boom)
        mp.setattr(_train, "_modules_on_points", boom)
        yield


def torch_encoding(x, num_fns, log_sampling):
    """positional_encoding (reference nerf/nerf_helpers.py:115-159) as plain torch ops."""
    out = [x]
    for f in freqs32(num_fns, log_sampling).to(x.dtype):
        out += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(out, -1)


def cosine(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def make_models(mkw, sd_c, sd_f, dev):
    import nerf
    out = []
    for sd in (sd_c, sd_f):
        m = nerf.models.FlexibleNeRFModel(**mkw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        out.append(m.to(dev))
    return out


def make_cfg(rkw, chunksize=4096):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=rkw.get("lindisp", False), num_coarse=rkw["num_coarse"],
                num_fine=rkw["num_fine"], perturb=rkw.get("perturb", False),
                radiance_field_noise_std=rkw.get("noise_std", 0.0), white_background=rkw.get("white_background", False))
    return nerf.CfgNode(dict(dataset=dict(near=rkw["near"], far=rkw["far"], no_ndc=True),
                             nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def freqs32(num_fns, log_sampling):
    """The encoding's frequencies as fp32 numbers (reference nerf/nerf_helpers.py:132-141)."""
    if log_sampling:
        return 2.0 ** torch.linspace(0.0, num_fns - 1, num_fns, dtype=torch.float32)
    return torch.linspace(2.0 ** 0.0, 2.0 ** (num_fns - 1), num_fns, dtype=torch.float32)


def encoding_vjp64(x32, g_enc, num_fns, log_sampling):
    """dx_d = g[d] + sum_k f_k (cos(f_k x_d) g[3 + 6k + d] - sin(f_k x_d) g[6 + 6k + d]) in float64.  The argument f_k x_d is the
    fp32 product, as the forward forms it (for the reference's power-of-two frequencies the product is exact anyway; for linearly
    spaced ones the encoding that was differentiated is the one of the rounded argument)."""
    x32 = x32.detach().cpu().float()
    g = g_enc.double().cpu()
    dx = g[:, :3].clone()
    for k, f in enumerate(freqs32(num_fns, log_sampling)):
        arg = (x32 * f).double()
        dx += float(f) * (torch.cos(arg) * g[:, 3 + 6 * k:6 + 6 * k] - torch.sin(arg) * g[:, 6 + 6 * k:9 + 6 * k])
    return dx


STAGE_CASES = {
    # name: (model kwargs | golden case, log sampling, rays, samples)
    "lego_4x128_L10": ("render_lego_val", True, 37, 24),
    "d8w256_skip4": ("render_d8w256_val", True, 21, 32),
    "4x128_L6": (dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True), True, 23, 47),
    "linear_sampling": (dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True), False, 16, 33),
    "no_viewdirs": (dict(num_layers=5, hidden_size=128, skip_connect_every=2, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=False), True, 19, 40),
    "ragged_8x19": ("render_lego_val", True, 8, 19),
    # four xyz stages: the fp32 transposed stream is 272 KiB, over the kernel's LDS budget, so its A operand is read through L2
    # (in the 16-bit mode it is 136 KiB and sits in LDS); 9 x 29 = 261 points = a second workgroup with one ragged tile
    "d8w256_skip2_stream_over_lds": (dict(num_layers=8, hidden_size=256, skip_connect_every=2, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True), True, 9, 29),
}


def stage_model(spec, dev):
    import nerf
    if isinstance(spec, str):
        return make_models(CASES[spec][0], *CASES[spec][1](), dev)[0]
    torch.manual_seed(11)
    return nerf.models.FlexibleNeRFModel(**spec).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16-s16"])
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_input_grad_kernel_against_float64_from_the_unpacked_records(dev, case, precision):
    """Stage test.  The gradient records of a backward-data launch are unpacked (dn_mlp_unpack) and d_pts / d_viewdirs / d_rays / d_z
    formed in float64 from those rows and the parameters - the fp32 parameters in the fp32 mode, their bf16 roundings in the 16-bit
    mode (the records are already rounded): the kernel sees identical inputs, only summation order and sin / cos differ.  Both
    forms of the entry point (points + view directions; ray rows + depths) must agree to 1e-4, the project's stage rule."""
    import nerf
    from nerf import _hip, _ops, _train
    spec, log_sampling, n_rays, s = STAGE_CASES[case]
    nerf.set_precision(precision)
    m = stage_model(spec, dev)
    pk = m.packed(log_sampling, log_sampling)
    assert pk.precision == (_hip.PREC_F32 if precision == "fp32" else _hip.PREC_BF16)
    _ops.pack_backward(pk, [x.weight for x in m.linear_modules()], pk.precision)
    stream_bytes = _ops.ensure_input_grad_stream(m, pk).numel()
    if case == "d8w256_skip2_stream_over_lds":      # (kIgLdsBudget of csrc/mlp_input_grad.hip is 160 KiB)
        assert (stream_bytes > 160 * 1024) == (precision == "fp32"), stream_bytes
    torch.manual_seed(5)
    n = n_rays * s
    ro = torch.randn(n_rays, 3, device=dev) * 0.7
    rd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1) * (0.5 + torch.rand(n_rays, 1, device=dev))
    vd = torch.nn.functional.normalize(rd, dim=-1)
    near, far = torch.full((n_rays, 1), 0.5, device=dev), torch.full((n_rays, 1), 3.0, device=dev)
    rays = torch.cat([ro, rd, near, far] + ([vd] if m.use_viewdirs else []), -1).contiguous()
    z = (0.5 + 2.5 * torch.rand(n_rays, s, device=dev)).sort(-1).values.contiguous()
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3).contiguous()      # mul then add, as the kernels form it
    out, act, masks = _ops.run_network_train(pk, None, None, None, rays=rays, z_vals=z, prec=pk.precision)
    grads = _ops.mlp_backward_data(pk, torch.randn(n, 4, device=dev), masks, n, prec=pk.precision)
    d_rays, d_z = _ops.mlp_backward_input(pk, grads, n_rays, s, rays=rays, z_vals=z)
    d_pts, d_vd = _ops.mlp_backward_input(pk, grads, n_rays, s, pts=pts, viewdirs=vd if m.use_viewdirs else None)
    torch.cuda.synchronize()

    # ---- the same in float64 ----
    _, gslots, kh = _train._slots(m, pk.precision)
    w, dx_dim = m.hidden_size, m.dim_xyz
    lowp = (lambda t: t.to(torch.bfloat16).float()) if precision == "bf16-s16" else (lambda t: t)

    def rows(slot, width):
        return _ops.mlp_unpack(pk, 1, grads, n, slot, width, 0, torch.empty((n, width), dtype=torch.float32, device=dev)).double().cpu()

    def w64(t):
        return lowp(t.detach()).double().cpu()
    g_enc = rows(gslots["layer1"], w) @ w64(m.layer1.weight)
    for i in m.skip_layers:
        g_enc += rows(gslots["trunk0"] + i * kh, w) @ w64(m.layers_xyz[i].weight)[:, w:w + dx_dim]
    assert g_enc.shape == (n, dx_dim)
    ref_pts = encoding_vjp64(pts, g_enc, m.num_encoding_fn_xyz, log_sampling)
    ref_vd = None
    if m.use_viewdirs:
        g_dir = rows(gslots["dirout"], w // 2) @ w64(m.layers_dir[0].weight)[:, w:w + m.dim_dir]
        per_point = encoding_vjp64(vd[:, None, :].expand(n_rays, s, 3).reshape(-1, 3), g_dir, m.num_encoding_fn_dir, log_sampling)
        ref_vd = per_point.reshape(n_rays, s, 3).sum(1)
    p3 = ref_pts.reshape(n_rays, s, 3)
    z64, rd64 = z.double().cpu(), rd.double().cpu()
    ref_rays = torch.zeros(n_rays, rays.shape[1], dtype=torch.float64)
    ref_rays[:, :3] = p3.sum(1)
    ref_rays[:, 3:6] = (p3 * z64[:, :, None]).sum(1)
    if m.use_viewdirs:
        ref_rays[:, 8:11] = ref_vd
    ref_z = (p3 * rd64[:, None, :]).sum(-1)

    errs = {"d_pts": rel_err(C(d_pts), ref_pts.numpy()), "d_z": rel_err(C(d_z), ref_z.numpy()),
            "d_ro": rel_err(C(d_rays[:, :3]), ref_rays[:, :3].numpy()), "d_rd": rel_err(C(d_rays[:, 3:6]), ref_rays[:, 3:6].numpy())}
    if m.use_viewdirs:
        errs["d_viewdirs"] = rel_err(C(d_vd), ref_vd.numpy())
        errs["d_rays_viewdir"] = rel_err(C(d_rays[:, 8:11]), ref_vd.numpy())
    else:
        assert d_vd is None
    print(f"input-grad stage {case} {precision}: {errs}")
    assert float(ref_pts.abs().max()) > 0
    assert bool((d_rays[:, 6:8] == 0).all())
    for k, e in errs.items():
        assert e <= 1e-4, (case, precision, k, e)


def _f64_model(m):
    import copy
    ref = copy.deepcopy(m).cpu().double()
    ref.zero_grad(set_to_none=True)
    return ref


def _f64_reference(m, pts32, vd32, log_sampling=True):
    """net(pts, vd) on the CPU in float64 through the nn.Linear composition; returns the model, the leaves and the output."""
    ref = _f64_model(m)
    pts = pts32.detach().cpu().double().requires_grad_(True)
    vd = vd32.detach().cpu().double().requires_grad_(True)
    n, s = pts.shape[0], pts.shape[1]
    emb = torch_encoding(pts.reshape(-1, 3), m.num_encoding_fn_xyz, log_sampling)
    emb = torch.cat([emb, torch_encoding(vd[:, None, :].expand(n, s, 3).reshape(-1, 3), m.num_encoding_fn_dir, log_sampling)], -1)
    out = ref._forward_modules(emb).reshape(n, s, 4)
    return ref, pts, vd, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["render_lego_val", "render_d8w256_val"])
def test_autograd_through_the_fused_route_against_float64(golden, dev, name, monkeypatch):
    """Autograd test, fp32 mode: run_network with points and view directions that require grad, and run_network_fused_rays with ray
    rows and depths that require grad, against the float64 nn.Linear composition on the CPU: input gradients and parameter
    gradients to 1e-3, the project's gradient tolerance (the fp32 composition itself sits at 2e-7 .. 8e-7 against float64 on these
    points); the near / far columns of d_rays exactly 0."""
    import nerf
    from nerf import _train
    g = golden(name)
    mkw, wfn, _ = CASES[name]
    m = make_models(mkw, *wfn(), dev)[0]
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    n, s = 12, 21
    torch.manual_seed(3)
    g_up = torch.randn(n, s, 4, device=dev)
    # ---- points + view directions ----
    pts = torch.from_numpy(np.ascontiguousarray(g["pts_coarse"][:n, :s])).to(dev).clone().requires_grad_(True)
    vd = torch.nn.functional.normalize(torch.from_numpy(np.ascontiguousarray(g["rd"][:n])).to(dev), dim=-1).clone().requires_grad_(True)
    rays = torch.cat([torch.zeros(n, 8, device=dev), vd], -1)
    with no_fallback(monkeypatch):
        out = nerf.run_network(m, pts, rays, 4096, ex, ed)
        (out * g_up).sum().backward()
    ref, pts64, vd64, out64 = _f64_reference(m, pts, vd)
    (out64 * g_up.double().cpu()).sum().backward()
    errs = {"out": rel_err(C(out), out64.detach().numpy()), "d_pts": rel_err(C(pts.grad), pts64.grad.numpy()),
            "d_viewdirs": rel_err(C(vd.grad), vd64.grad.numpy())}
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        errs[k] = rel_err(C(p.grad), q.grad.numpy())
    print(f"autograd (points form) {name}: {errs}")
    for k, e in errs.items():
        assert e <= 1e-3, (name, k, e)
    # ---- ray rows + depths ----
    m.zero_grad(set_to_none=True)
    ro = torch.from_numpy(np.ascontiguousarray(g["ro"][:n])).to(dev)
    rd = torch.from_numpy(np.ascontiguousarray(g["rd"][:n])).to(dev)
    rows = torch.cat([ro, rd, torch.full((n, 1), 2.0, device=dev), torch.full((n, 1), 6.0, device=dev), vd.detach()], -1).clone().requires_grad_(True)
    z = (2.0 + 4.0 * torch.rand(n, s, device=dev)).sort(-1).values.clone().requires_grad_(True)
    with no_fallback(monkeypatch):
        out = _train.run_network_fused_rays(m, rows, z)
        (out * g_up).sum().backward()
    rows64 = rows.detach().cpu().double().requires_grad_(True)
    z64 = z.detach().cpu().double().requires_grad_(True)
    p64 = rows64[:, None, :3] + rows64[:, None, 3:6] * z64[:, :, None]
    with torch.no_grad():    # the kernel's points are the fp32 mul-then-add: the same VALUES here, the derivative in float64
        p32 = (rows[:, None, :3] + rows[:, None, 3:6] * z[:, :, None]).detach().cpu().double()
        shift = p32 - p64
    ref = _f64_model(m)
    emb = torch.cat([torch_encoding((p64 + shift).reshape(-1, 3), 10, True),
                     torch_encoding(rows64[:, None, 8:11].expand(n, s, 3).reshape(-1, 3), 4, True)], -1)
    out64 = ref._forward_modules(emb).reshape(n, s, 4)
    (out64 * g_up.double().cpu()).sum().backward()
    assert bool((rows.grad[:, 6:8] == 0).all())
    errs = {"out": rel_err(C(out), out64.detach().numpy()), "d_z": rel_err(C(z.grad), z64.grad.numpy())}
    for k, sl in (("d_ro", slice(0, 3)), ("d_rd", slice(3, 6)), ("d_viewdir", slice(8, 11))):
        errs[k] = rel_err(C(rows.grad[:, sl]), rows64.grad[:, sl].numpy())
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        errs[k] = rel_err(C(p.grad), q.grad.numpy())
    print(f"autograd (rays form) {name}: {errs}")
    for k, e in errs.items():
        assert e <= 1e-3, (name, k, e)


def _scene_rays(n, dev, seed=77, pose=9, h=400, w=400):
    import nerf
    from nerf import synthetic as syn
    e_mat, k_mat = torch.from_numpy(syn.scene_pose(pose)), torch.from_numpy(syn.intrinsic(h, w))
    ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), e_mat.to(dev), k_mat.to(dev))
    sel = torch.from_numpy(syn.select_rays(h, w, n, seed=seed)).to(dev)
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def _pack_rows(ro, rd, near=2.0, far=6.0):
    vd = rd / rd.norm(p=2, dim=-1, keepdim=True)
    return torch.cat([ro, rd, torch.full_like(rd[:, :1], near), torch.full_like(rd[:, :1], far), vd], -1)


def _good(t):
    return t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


@contextlib.contextmanager
def no_modules_on_points(monkeypatch):
    from nerf import _train

    def boom(*a, **k):
        raise AssertionError("a call whose inputs require grad left the fused kernels")
    with monkeypatch.context() as mp:
        mp.setattr(_train, "_modules_on_points", boom)
        yield


def _three_calls(mc, mf, dev, n=48):
    """run_network, predict_and_render_radiance and run_one_iter_of_nerf with inputs that require grad; returns their input gradients."""
    import nerf
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    cfg = make_cfg(CASES["render_lego_val"][2], 32)      # chunks of 32 rays: get_minibatches keeps working
    ro, rd = _scene_rays(n, dev)
    got = {}
    rows = _pack_rows(ro, rd)
    pts = (ro[:, None, :] + rd[:, None, :] * torch.linspace(2.0, 6.0, 16, device=dev)[None, :, None]).clone().requires_grad_(True)
    nerf.run_network(mc, pts, rows, 4096, ex, ed).square().sum().backward()
    got["run_network d_pts"] = pts.grad
    batch = rows.clone().requires_grad_(True)
    out = nerf.predict_and_render_radiance(batch, mc, mf, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
    (out[0].square().sum() + out[3].square().sum()).backward()
    got["predict_and_render_radiance d_rays"] = batch.grad
    ro_l, rd_l = ro.clone().requires_grad_(True), rd.clone().requires_grad_(True)
    out = nerf.run_one_iter_of_nerf(400, 400, 1.0, mc, mf, ro_l, rd_l, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
    assert out[0].shape == (n, 3) and out[3].shape == (n, 3)
    (out[0].square().sum() + out[3].square().sum()).backward()
    got["run_one_iter_of_nerf d_ro"], got["run_one_iter_of_nerf d_rd"] = ro_l.grad, rd_l.grad
    return got


@pytest.mark.gpu
def test_inputs_that_require_grad_stay_on_the_fused_kernels(dev, monkeypatch):
    """Route test.  With _train._modules_on_points raising, run_network, predict_and_render_radiance and run_one_iter_of_nerf with
    rays that require grad succeed in 'fp32', 'bf16-s16' and the default 'bf16' and return finite, non-zero input gradients; with
    every parameter frozen (pose refinement) no weight-gradient launch happens; in 'fp16' the nn.Linear route is still the one taken."""
    import nerf
    from nerf import _ops, _train
    mkw, wfn, _ = CASES["render_lego_val"]
    for prec in ("fp32", "bf16-s16", "bf16"):
        nerf.set_precision(prec)
        mc, mf = make_models(mkw, *wfn(), dev)
        with no_modules_on_points(monkeypatch):
            got = _three_calls(mc, mf, dev)
        for k, t in got.items():
            assert _good(t), (prec, k)
        assert all(p.grad is not None for p in mc.parameters()) and all(p.grad is not None for p in mf.parameters())
    # frozen weights: the backward must not form weight gradients at all
    nerf.set_precision("fp32")
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)

    def no_wgrad(*a, **k):
        raise AssertionError("a weight-gradient launch with every parameter frozen")
    with no_modules_on_points(monkeypatch), monkeypatch.context() as mp:
        for name in ("mlp_weight_grad_all", "mlp_weight_grad_all_into", "mlp_weight_grad", "render_rays_backward"):
            mp.setattr(_ops, name, no_wgrad)
        got = _three_calls(mc, mf, dev)
    for k, t in got.items():
        assert _good(t), ("frozen", k)
    assert all(p.grad is None for p in mc.parameters())
    # fp16 is a render-only precision: inputs that require grad keep the differentiable torch composition
    nerf.set_precision("fp16")
    calls = []
    real = _train._modules_on_points
    with monkeypatch.context() as mp:
        mp.setattr(_train, "_modules_on_points", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        ro, rd = _scene_rays(8, dev)
        batch = _pack_rows(ro, rd).clone().requires_grad_(True)
        z = torch.linspace(2.0, 6.0, 16, device=dev).expand(8, 16).contiguous()
        _train.run_network_fused_rays(mc, batch, z).square().sum().backward()
    assert calls and _good(batch.grad)


@pytest.mark.gpu
def test_default_bf16_parameter_step_is_undisturbed_by_an_input_gradient_call(dev, monkeypatch):
    """Default-mode isolation: a parameter-only training step in 'bf16' (8-bit saves, 48-point kernels) gives bit-identical parameter
    gradients before and after an input-gradient call on the same models (which runs 16-bit saves on the 32-point kernels)."""
    import nerf
    nerf.set_precision("bf16")
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    cfg = make_cfg(rkw)
    ro, rd = _scene_rays(64, dev)
    target = torch.rand(64, 3, device=dev)

    def step():
        for m in (mc, mf):
            m.zero_grad(set_to_none=True)
        out = nerf.run_one_iter_of_nerf(400, 400, 1.0, mc, mf, ro, rd, cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
        (nerf.img2mse(out[0], target) + nerf.img2mse(out[3], target)).backward()
        return [p.grad.clone() for m in (mc, mf) for p in m.parameters()]
    before = step()
    for m in (mc, mf):
        m.zero_grad(set_to_none=True)
    with no_modules_on_points(monkeypatch):
        got = _three_calls(mc, mf, dev)
    assert all(_good(t) for t in got.values())
    after = step()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16-s16"])
def test_input_gradients_are_bit_reproducible(dev, precision, monkeypatch):
    """Determinism: two backward passes on the same inputs give bit-identical d_rays, d_z and d_pts (plain stores, fixed order)."""
    import nerf
    from nerf import _train
    nerf.set_precision(precision)
    mkw, wfn, _ = CASES["render_d8w256_val"]
    m = make_models(mkw, *wfn(), dev)[0]
    ro, rd = _scene_rays(50, dev)
    torch.manual_seed(9)
    z0 = (2.0 + 4.0 * torch.rand(50, 37, device=dev)).sort(-1).values
    g_up = torch.randn(50, 37, 4, device=dev)
    runs = []
    for _ in range(2):
        rows = _pack_rows(ro, rd).clone().requires_grad_(True)
        z = z0.clone().requires_grad_(True)
        pts = (ro[:, None, :] + rd[:, None, :] * z0[:, :, None]).clone().requires_grad_(True)
        with no_modules_on_points(monkeypatch):
            (_train.run_network_fused_rays(m, rows, z) * g_up).sum().backward()
            (_train.run_network_fused(m, pts, rows[:, -3:].detach(), 37) * g_up.reshape(-1, 4)).sum().backward()
        runs.append((rows.grad.clone(), z.grad.clone(), pts.grad.clone()))
    for a, b in zip(*runs):
        assert _good(a) and torch.equal(a, b)


def _pose_rays64(xi, ro64, rd64):
    """World-space rays under the rigid update exp(xi): ro' = R ro + t, rd' = R rd, R = exp([omega]x), xi = (omega, t)."""
    wx, wy, wz = xi[0], xi[1], xi[2]
    zero = torch.zeros((), dtype=xi.dtype)
    skew = torch.stack([torch.stack([zero, -wz, wy]), torch.stack([wz, zero, -wx]), torch.stack([-wy, wx, zero])])
    rot = torch.linalg.matrix_exp(skew)
    return ro64 @ rot.T + xi[3:], rd64 @ rot.T


POSE_XI = (0.01, -0.02, 0.015, 0.03, -0.01, 0.02)


def _oracle_pose_gradient(dtype, ro64, rd64, target64):
    from oracle import nerf_oracle as oc
    mkw, wfn, rkw = CASES["render_lego_val"]
    sd_c, sd_f = wfn()
    tsd_c = {k: torch.from_numpy(v).to(dtype) for k, v in sd_c.items()}
    tsd_f = {k: torch.from_numpy(v).to(dtype) for k, v in sd_f.items()}
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    ro, rd = _pose_rays64(xi, ro64, rd64)
    cfg_o = oc.RenderCfg(chunksize=4096, m_thres=(), num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"], near=rkw["near"], far=rkw["far"],
                         white_background=rkw["white_background"])
    mcfg = oc.ModelCfg(**mkw)
    out = oc.run_one_iter(ro.to(dtype), rd.to(dtype), tsd_c, tsd_f, mcfg, mcfg, cfg_o)
    mse = torch.nn.functional.mse_loss
    loss = mse(out[0], target64.to(dtype)) + mse(out[3], target64.to(dtype))
    loss.backward()
    return xi.grad.numpy().copy(), loss.item()


def pose_problem():
    """256 rays of the synthetic scene (pose 9, 400 x 400, the fixed selection seed 77 - no ray was chosen or dropped by its
    behaviour) as float64 CPU tensors, and a fixed random target."""
    from nerf import synthetic as syn
    from oracle import nerf_oracle as oc
    h = w = 400
    e_mat, k_mat = torch.from_numpy(syn.scene_pose(9)), torch.from_numpy(syn.intrinsic(h, w))
    ro, rd = oc.get_ray_bundle(h, w, e_mat, k_mat)
    sel = torch.from_numpy(syn.select_rays(h, w, 256, seed=77))
    target = torch.rand(256, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return ro.reshape(-1, 3)[sel].double(), rd.reshape(-1, 3)[sel].double(), target


POSE_FLOOR = 4.6e-4      # oracle_pose_floor()[0] as measured on the build machine's CPU; the gate below is pinned to it


def oracle_pose_floor():
    """The oracle's own fp32-vs-float64 difference of dL/dxi (max-norm, relative) - the floor resampling flips put under the test.
    How POSE_FLOOR was measured; the test itself does not re-measure it, so a numerically worse oracle run cannot widen the gate."""
    ro64, rd64, target = pose_problem()
    g64, _ = _oracle_pose_gradient(torch.float64, ro64, rd64, target)
    g32, _ = _oracle_pose_gradient(torch.float32, ro64, rd64, target)
    return rel_err(g32, g64), g64


@pytest.mark.gpu
def test_pose_gradient_end_to_end_against_the_float64_oracle(dev, monkeypatch):
    """dL/dxi of coarse + fine MSE through run_one_iter_of_nerf (lego weights, 64 + 64 samples, perturb off, noise 0, fp32 mode),
    xi = a small rotation + translation applied to 256 world-space rays, against float64 autograd through the CPU oracle (plain
    torch, the same detach of the resamples).  An inverse-CDF resample that lands on the other side of a bin edge in fp32 than in
    float64 moves a fine depth by a bin: the floor is the oracle's own fp32-vs-float64 difference of dL/dxi on the same rays,
    measured once on the build machine's CPU (oracle_pose_floor: 4.6e-4, recorded as POSE_FLOOR), and the gate is the constant
    max(1e-3, 4 x POSE_FLOOR) = 1.84e-3 - four times because the library's fp32 path re-associates once more than the oracle's.
    All 256 rays of the fixed selection are used; none was picked by its behaviour."""
    import nerf
    floor = POSE_FLOOR
    ro64, rd64, target = pose_problem()
    g64, _ = _oracle_pose_gradient(torch.float64, ro64, rd64, target)
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    ro, rd = _pose_rays64(xi, ro64, rd64)
    with no_fallback(monkeypatch):
        out = nerf.run_one_iter_of_nerf(400, 400, 1.0, mc, mf, ro.float().to(dev), rd.float().to(dev), make_cfg(rkw), mode="train",
                                        encode_position_fn=ex, encode_direction_fn=ed)
        tgt = target.float().to(dev)
        (nerf.img2mse(out[0], tgt) + nerf.img2mse(out[3], tgt)).backward()
    err = rel_err(xi.grad.numpy(), g64)
    gate = max(1e-3, 4.0 * floor)
    print(f"pose gradient: oracle fp32-vs-float64 floor {floor:.3e}, gate {gate:.3e}, library vs float64 oracle {err:.3e}, dL/dxi {g64}")
    assert err <= gate, (err, gate, floor)


@pytest.mark.gpu
def test_16bit_input_gradient_quality_beside_the_parameter_gradient(dev, monkeypatch):
    """16-bit quality, recorded and lightly gated: the cosine of d_pts in 'bf16-s16' against the fp32-mode d_pts, beside the cosine of
    layer1.weight.grad of the same step (the gradient quality the project already trains on), over five seeds.  Gate: the mean
    input-gradient cosine is not below the mean parameter cosine minus three seed-to-seed standard deviations (of the difference of
    the two cosines: the quantity being bounded)."""
    import nerf
    mkw, wfn, _ = CASES["render_lego_val"]
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    cos_in, cos_par = [], []
    for seed in range(5):
        ro, rd = _scene_rays(128, dev, seed=100 + seed)
        rows = _pack_rows(ro, rd)
        torch.manual_seed(seed)
        z = (2.0 + 4.0 * torch.rand(128, 64, device=dev)).sort(-1).values
        g_up = torch.randn(128, 64, 4, device=dev)
        got = {}
        for prec in ("fp32", "bf16-s16"):
            nerf.set_precision(prec)
            m = make_models(mkw, *wfn(), dev)[0]
            pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).clone().requires_grad_(True)
            with no_modules_on_points(monkeypatch):
                (nerf.run_network(m, pts, rows, 1 << 20, ex, ed) * g_up).sum().backward()
            got[prec] = (C(pts.grad), C(m.layer1.weight.grad))
        cos_in.append(cosine(got["bf16-s16"][0], got["fp32"][0]))
        cos_par.append(cosine(got["bf16-s16"][1], got["fp32"][1]))
    cos_in, cos_par = np.array(cos_in), np.array(cos_par)
    sd = float(np.std(cos_par - cos_in, ddof=1))
    print(f"16-bit quality: cos(d_pts) {cos_in.tolist()} mean {cos_in.mean():.6f}; cos(layer1.weight.grad) {cos_par.tolist()} "
          f"mean {cos_par.mean():.6f}; seed-to-seed sd of the difference {sd:.2e}")
    assert cos_in.mean() >= cos_par.mean() - 3.0 * sd, (cos_in.tolist(), cos_par.tolist(), sd)
