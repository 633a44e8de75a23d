"""The surface-normal render (include/dexnerf_hip_normals.h): dn_composite_normals, dn_render_rays_normals and their Python surface -
_ops.composite_normals / density_gradient / render_rays_normals, FlexibleNeRFModel.packed_density_grad, nerf.density_gradient,
nerf.render_dex_normals, eval_nerf.py --normals.

Yardsticks.  The compositing kernel: a float64 restatement written here on identical inputs (sigma and the threshold compare restated
in fp32, so the crossing indices are exact) at 1e-5 - the gate of the project's other fp32-vs-float64 small kernels - with depth / acc /
dex BIT FOR BIT dn_composite_density's.  The gradient stage: float64 autograd through encoding + trunk + fc_alpha built from the model's
own state dict, 1e-4 on sigma (the stage rule) and 1e-3 on the gradient (the gradient tolerance).  The driver: bit for bit the
composition of its stages, in fp32 and bf16.  The image-level render: bit for bit independent of chunking and of the workspace split.
Norms: conftest.rel_err (max|a - b| / max|b| per tensor)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES, D4, D8
from test_input_gradients import STAGE_CASES, _f64_model, stage_model, torch_encoding

NORMALS = ("dn_composite_normals", "dn_render_normals_workspace_bytes", "dn_render_rays_normals")
INVAL, UNSUPPORTED = -1000, -1001


def C(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(bits(a), bits(b)))


def full_desc(width, l_xyz, depth, skip=4, viewdirs=1):
    from nerf import _hip
    return _hip.MlpDesc(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=l_xyz, num_encoding_fn_dir=4,
                        include_input_xyz=1, include_input_dir=1, use_viewdirs=viewdirs, log_sampling_xyz=1, log_sampling_dir=1)


def density_desc(width=128, l_xyz=10, depth=4, skip=4):
    from nerf import _hip
    d = _hip.MlpDesc()
    assert _hip.lib().dn_mlp_density_desc(ctypes.byref(full_desc(width, l_xyz, depth, skip)), ctypes.byref(d)) == 0
    assert d.use_viewdirs == 0
    return d


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_normals_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    names = lambda name: set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", open(os.path.join(REPO, "include", name)).read()))  # noqa: E731
    assert names("dexnerf_hip_normals.h") == set(_hip.NORMALS_EXPORTS) == set(NORMALS)
    older = set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS)
    assert not older & set(NORMALS)
    assert "dexnerf_hip_normals.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()      # build() checks the new header's symbols too
    assert "composite_normals.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in NORMALS) and hiplib.dn_abi_version() == 2


def test_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    from nerf import _hip
    fake = ctypes.c_void_p(4096)
    dd = density_desc()
    need = hiplib.dn_render_normals_workspace_bytes(ctypes.byref(dd), ctypes.byref(dd), _hip.PREC_F32, 8, 16, 24)
    assert need > 0
    defaults = dict(desc_c=ctypes.byref(dd), packed_c=fake, desc_f=ctypes.byref(dd), packed_f=fake, bwd=fake, ig=fake, prec=_hip.PREC_F32,
                    rays=fake, stride=8, n=8, nc=16, nf=24, lindisp=0, std=0.0, thres=fake, k=3, t_rand=None, noise_c=None, u=None,
                    noise_f=None, depth_c=fake, acc_c=fake, depth=fake, acc=fake, dex=fake, normal=fake, dex_normal=fake, ws=fake,
                    ws_bytes=need, stream=None)
    call = lambda **kw: hiplib.dn_render_rays_normals(*{**defaults, **kw}.values())  # noqa: E731
    with_dirs = full_desc(128, 10, 4)
    for kw in (dict(desc_c=None), dict(packed_c=None), dict(bwd=None), dict(ig=None), dict(rays=None), dict(ws=None), dict(n=-1),
               dict(desc_f=None), dict(packed_f=None),                           # a fine pass without its network
               dict(ws=ctypes.c_void_p(4096 + 16)),                               # misaligned workspace
               dict(ws_bytes=need - 1),                                           # workspace too small
               dict(desc_f=ctypes.byref(with_dirs)), dict(desc_c=ctypes.byref(with_dirs)),   # a full descriptor where a density one is required
               dict(nc=9), dict(nc=513), dict(nc=512, nf=1537), dict(nc=0), dict(nf=-1), dict(stride=7),
               dict(k=-1), dict(thres=None), dict(dex=None, dex_normal=None)):    # thresholds without either Dex output
        assert call(**kw) == INVAL, kw
        assert b"dn_render_rays_normals" in hiplib.dn_last_error(), kw
    for prec in (_hip.PREC_F16, _hip.PREC_BF16_S8):
        assert call(prec=prec) == UNSUPPORTED
        assert b"16-bit saved tensors" in hiplib.dn_last_error()
        assert hiplib.dn_render_normals_workspace_bytes(ctypes.byref(dd), ctypes.byref(dd), prec, 8, 16, 24) == 0
    assert call(desc_f=ctypes.byref(density_desc(l_xyz=8))) == UNSUPPORTED          # outside the training kernels
    # the size query: bad sizes and what the render refuses give 0
    q = hiplib.dn_render_normals_workspace_bytes
    assert q(None, None, _hip.PREC_F32, 8, 16, 0) == 0 and q(ctypes.byref(dd), None, _hip.PREC_F32, 8, 16, 24) == 0
    assert q(ctypes.byref(dd), ctypes.byref(dd), _hip.PREC_F32, -1, 16, 24) == 0 and q(ctypes.byref(dd), None, _hip.PREC_F32, 8, 0, 0) == 0
    assert q(ctypes.byref(dd), ctypes.byref(with_dirs), _hip.PREC_F32, 8, 16, 24) == 0
    assert q(ctypes.byref(dd), None, _hip.PREC_BF16, 8, 16, 0) > 0                  # coarse only: no fine descriptor needed
    assert q(ctypes.byref(dd), ctypes.byref(dd), _hip.PREC_F32, 16, 16, 24) > need  # grows with the rays
    # n_rays == 0 is a valid no-op once the arguments are in order
    assert call(n=0) == 0

    comp = dict(rf=fake, z=fake, rd=fake, rd_stride=3, noise=None, std=0.0, g=fake, thres=fake, k=2, n=4, s=8, depth=fake, acc=fake, dex=fake,
                normal=fake, dex_normal=fake, stream=None)
    ccall = lambda **kw: hiplib.dn_composite_normals(*{**comp, **kw}.values())  # noqa: E731
    for kw in (dict(rf=None), dict(z=None), dict(rd=None), dict(g=None), dict(s=0), dict(n=-1), dict(rd_stride=2), dict(k=-1), dict(thres=None),
               dict(dex=None, dex_normal=None), dict(rf=ctypes.c_void_p(4096 + 4))):
        assert ccall(**kw) == INVAL, kw
        assert b"dn_composite_normals" in hiplib.dn_last_error(), kw
    assert ccall(n=0) == 0


COVERED = [(w, l, d, s) for w in (128, 256) for l in (6, 10) for d, s in ((8, 4), (4, 4))]   # noqa: E741


@pytest.mark.parametrize("width,l_xyz,depth,skip", COVERED)
def test_training_sizes_of_the_density_descriptors_are_non_zero(hiplib, width, l_xyz, depth, skip):
    """The density sub-network of every shape fused_ok() covers is a network the training forward, the backward-data chain and the
    input gradient accept as it is - no shape takes a fallback through the full network."""
    from nerf import _hip
    dd = density_desc(width, l_xyz, depth, skip)
    for prec in (_hip.PREC_F32, _hip.PREC_BF16):
        a, m, g = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert hiplib.dn_mlp_train_sizes(ctypes.byref(dd), prec, 1000, ctypes.byref(a), ctypes.byref(m), ctypes.byref(g)) == 0
        assert a.value > 0 and m.value > 0 and g.value > 0
        assert hiplib.dn_mlp_backward_packed_bytes(ctypes.byref(dd), prec) > 0
        assert hiplib.dn_mlp_input_grad_packed_bytes(ctypes.byref(dd), prec) > 0
        need = hiplib.dn_render_normals_workspace_bytes(ctypes.byref(dd), ctypes.byref(dd), prec, 100, 16, 24)
        assert need > a.value + g.value                 # 4000 points: it holds the last pass's saved tensors and gradient records


def test_python_surface_refuses_grad_and_fp16_before_any_device_call(monkeypatch):
    import nerf
    from nerf import _hip, _ops
    from test_input_gradients import make_cfg

    def no_device(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_hip, "lib", no_device)
    monkeypatch.setattr(_ops, "lib", no_device)
    m = nerf.models.FlexibleNeRFModel(**D4)
    ex = nerf.get_embedding_function(10)
    cfg = make_cfg(dict(num_coarse=16, num_fine=24, near=2.0, far=6.0))
    ro, rd = torch.zeros(2, 3, 3), torch.ones(2, 3, 3)
    pts = torch.zeros(5, 3)

    def render(ro=ro, rd=rd):
        return nerf.render_dex_normals(2, 3, 1.0, m, m, ro, rd, cfg, mode="validation", encode_position_fn=ex, m_thres_cand=[5.0])
    try:
        nerf.set_precision("fp32")
        with pytest.raises(RuntimeError, match="no-grad"):
            render()                                                             # parameters require grad, autograd enabled
        with pytest.raises(RuntimeError, match="no-grad"):
            nerf.density_gradient(m, pts, ex)
        for p in m.parameters():
            p.requires_grad_(False)
        with pytest.raises(RuntimeError, match="no-grad"):
            render(rd=rd.clone().requires_grad_(True))                           # rays that require grad
        with pytest.raises(RuntimeError, match="no-grad"):
            nerf.density_gradient(m, pts.clone().requires_grad_(True), ex)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="ROCm device"):
                render()                                                         # host tensors: refused, never computed on the CPU
            nerf.set_precision("fp16")
            with pytest.raises(RuntimeError, match="fp16"):
                render()
            with pytest.raises(RuntimeError, match="fp16"):
                nerf.density_gradient(m, pts, ex)
    finally:
        nerf.set_precision("fp32")


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
def _fp32_on_exit():
    import nerf
    yield
    nerf.set_precision("fp32")


def unit_normals64(g):
    """-g / |g| in float64 from fp32 components; 0 where |g| is 0 or not finite."""
    g = np.asarray(g, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
        ok = np.isfinite(length) & (length > 0)
        n = np.where(ok[..., None], -g / np.where(ok, length, 1.0)[..., None], 0.0)
    return n.astype(np.float32).astype(np.float64)      # each component rounded to fp32 once


def composite_normals64(rf, z, rd, g, noise, noise_std, thres):
    """volume_render_radiance_field's weights (reference nerf/volume_rendering_utils.py:33-47) in float64 from the fp32 sigma - the noise
    product, the sum and the relu restated in fp32 - and the normals composited with them; the first crossings from the fp32 compare."""
    raw = np.asarray(rf, np.float32)[..., 3]
    if noise_std > 0.0:
        raw = raw + np.asarray(noise, np.float32) * np.float32(noise_std)
    sigma = np.maximum(raw, np.float32(0.0))
    assert sigma.dtype == np.float32
    z64, rd64 = np.asarray(z, np.float64), np.asarray(rd, np.float64)
    dists = np.concatenate([z64[:, 1:] - z64[:, :-1], np.full((z64.shape[0], 1), 1e10)], -1) * np.linalg.norm(rd64, axis=-1, keepdims=True)
    alpha = 1.0 - np.exp(-sigma.astype(np.float64) * dists)
    trans = np.cumprod(np.concatenate([np.ones((z64.shape[0], 1)), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * trans
    n = unit_normals64(g)
    normal = (w[..., None] * n).sum(1)
    m = np.asarray(thres, np.float32)
    over = sigma[None, :, :] > m[:, None, None]                       # (K, N, S), fp32 compare
    crossed = over.any(-1)
    first = np.where(crossed, over.argmax(-1), -1)
    rays = np.arange(z64.shape[0])[None, :]
    dex_normal = np.where(crossed[..., None], n[rays, np.maximum(first, 0)], 0.0)
    return normal, dex_normal, first, w.sum(1)


COMPOSITE_CASES = [(1, 1, 0), (5, 19, 3), (67, 64, 1), (3, 65, 65), (2, 200, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("noise_std", [0.0, 1.5])
@pytest.mark.parametrize("n,s,k", COMPOSITE_CASES)
def test_composite_normals_against_float64_and_composite_density(dev, n, s, k, noise_std):
    """dn_composite_normals on random rows, sorted depths and random gradients: normal and dex_normal against the float64 restatement at
    1e-5; depth / acc / dex the bits of dn_composite_density.  Shapes: one ray of one sample, a ragged workgroup, the 64-sample chunk
    edge from both sides (64, 65, 200), the 64-threshold group edge from both sides (64, 65).  Planted: a zero gradient row, rows with an
    inf and a NaN component (all three -> the zero normal), a ray whose sigma never crosses; then constant gradients: every valid Dex
    normal is one vector, the expected normal that vector times acc.  No output may hold a NaN.
    Measured on an MI355X (rel_err, printed by the test): normal 3.7e-8 .. 1.3e-7 over the ten cases (0 for the one-sample ray), dex_normal 0
    in every case, acc 3e-10 .. 1.2e-7, the constant-gradient normal against unit * acc 0 .. 1.9e-7."""
    from nerf import _ops
    gen = torch.Generator().manual_seed(1000 * n + 10 * s + k)
    rf = (torch.randn(n, s, 4, generator=gen) * 15.0).to(dev)
    z = (2.0 + 4.0 * torch.rand(n, s, generator=gen)).sort(-1).values.to(dev)
    rd = (torch.randn(n, 3, generator=gen) * 0.8).to(dev)
    g = (torch.randn(n, s, 3, generator=gen) * torch.exp(3.0 * torch.randn(n, s, 1, generator=gen))).to(dev)
    noise = torch.randn(n, s, generator=gen).to(dev) if noise_std > 0 else None
    rf[0, 0, 3] = rf[0, 0, 3].abs() + 10.0                            # the first ray's first sample is opaque, noise or not: a non-zero normal
    flat = g.view(-1, 3)
    if n * s >= 4:
        flat[1] = 0.0
        flat[2, 1] = float("inf")
        flat[3, 0] = float("nan")
    if n >= 2:
        rf[n - 1, :, 3] = -1.0e6                                       # never crosses, noise or not
    thres = [float(m) for m in np.linspace(0.25, 40.0, k)] if k else []
    depth, acc, dex, normal, dex_normal = _ops.composite_normals(rf, z, rd, g, noise, noise_std, thres)
    depth0, acc0, dex0 = _ops.composite_density(rf, z, rd, noise, noise_std, thres)
    only_normals = _ops.composite_normals(rf, z, rd, g, noise, noise_std, thres, want_dex=False)
    torch.cuda.synchronize()
    assert same_bits(depth, depth0) and same_bits(acc, acc0) and same_bits(dex, dex0)
    assert only_normals[2] is None and same_bits(only_normals[4], dex_normal) and same_bits(only_normals[3], normal)
    for t in (depth, acc, dex, normal, dex_normal):
        assert t is None or torch.isfinite(t).all()
    ref_normal, ref_dex_normal, first, acc64 = composite_normals64(C(rf), C(z), C(rd), C(g), None if noise is None else C(noise), noise_std, thres)
    errs = {"normal": rel_err(C(normal), ref_normal), "acc": rel_err(C(acc), acc64)}
    assert normal.shape == (n, 3) and float(np.abs(ref_normal).max()) > 0
    if k:
        assert dex_normal.shape == (k, n, 3)
        errs["dex_normal"] = rel_err(C(dex_normal), ref_dex_normal)
        # the Dex depth is the depth of the very sample the normal was taken at; no crossing: z[0] and the exact zero vector
        zc = C(z)
        assert np.array_equal(C(dex), zc[np.arange(n)[None, :], np.maximum(first, 0)])
        assert np.array_equal(C(dex_normal)[first < 0], np.zeros(((first < 0).sum(), 3), np.float32))
        if n >= 2:
            assert (first[:, n - 1] < 0).all()
        assert (first >= 0).any() or s == 1
    else:
        assert dex is None and dex_normal is None
    print(f"composite_normals N={n} S={s} K={k} noise={noise_std}: {errs}")
    for name, e in errs.items():
        assert e <= 1e-5, (name, e)

    # constant gradients
    const = torch.tensor([0.3, -2.0, 1.5], device=dev)
    gc = const.expand(n, s, 3).contiguous()
    _, acc_c, _, normal_c, dex_normal_c = _ops.composite_normals(rf, z, rd, gc, noise, noise_std, thres)
    unit = torch.from_numpy(unit_normals64(C(const)).astype(np.float32)).to(dev)
    assert same_bits(acc_c, acc)
    e_const = rel_err(C(normal_c), C(acc_c)[:, None].astype(np.float64) * C(unit)[None, :].astype(np.float64))
    print(f"  constant gradient: normal vs unit * acc {e_const:.3e}")
    assert e_const <= 1e-5
    if k:
        valid = torch.from_numpy(first >= 0).to(dev)
        assert torch.equal(bits(dex_normal_c[valid]), bits(unit.expand_as(dex_normal_c)[valid]))
        assert not dex_normal_c[~valid].any()


def sigma_and_gradient64(m, pts32):
    """Encoding + trunk + fc_alpha (fc_out's row 3 without view directions) in float64 on the CPU, differentiated by autograd."""
    ref = _f64_model(m)
    pts = pts32.detach().cpu().double().reshape(-1, 3).requires_grad_(True)
    xyz = torch_encoding(pts, m.num_encoding_fn_xyz, True)
    h = ref.layer1(xyz)
    for i, layer in enumerate(ref.layers_xyz):
        if i in ref.skip_layers:
            h = torch.cat((h, xyz), dim=-1)
        h = torch.relu(layer(h))
    sigma = ref.fc_alpha(h)[:, 0] if m.use_viewdirs else ref.fc_out(h)[:, 3]
    grad, = torch.autograd.grad(sigma.sum(), pts)
    return sigma.detach().numpy(), grad.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["lego_4x128_L10", "d8w256_skip4", "4x128_L6"])
def test_density_gradient_against_float64_autograd(dev, case):
    """nerf.density_gradient in fp32 mode on tests/test_input_gradients.py's networks at its shapes (37 x 24, 21 x 32, 23 x 47 points):
    sigma to 1e-4, the gradient to 1e-3; two chunkings give the same bits, and the ray form of _ops.density_gradient the bits of the
    points form.  Measured on an MI355X (printed by the test; sigma, gradient): 4.9e-7, 2.6e-7 (lego 4x128 / L10); 1.5e-6, 5.9e-7 (D8/W256);
    4.4e-7, 4.8e-7 (4x128 / L6)."""
    import nerf
    from nerf import _ops
    spec, log_sampling, n_rays, s = STAGE_CASES[case]
    assert log_sampling
    nerf.set_precision("fp32")
    m = stage_model(spec, dev).requires_grad_(False)
    ex = nerf.get_embedding_function(m.num_encoding_fn_xyz)
    torch.manual_seed(5)
    ro = torch.randn(n_rays, 3, device=dev) * 0.7
    rd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1) * (0.5 + torch.rand(n_rays, 1, device=dev))
    z = (0.5 + 2.5 * torch.rand(n_rays, s, device=dev)).sort(-1).values.contiguous()
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).contiguous()      # mul then add, as the kernels form it
    sigma, grad = nerf.density_gradient(m, pts, ex)
    sigma_b, grad_b = nerf.density_gradient(m, pts, ex, chunksize=100)
    rays = torch.cat([ro, rd, torch.full((n_rays, 1), 0.5, device=dev), torch.full((n_rays, 1), 3.0, device=dev)], -1).contiguous()
    sigma_r, grad_r = _ops.density_gradient(m.packed_density(), m.packed_density_grad(), rays=rays, z=z)
    torch.cuda.synchronize()
    assert sigma.shape == (n_rays * s,) and grad.shape == (n_rays * s, 3)
    assert same_bits(sigma, sigma_b) and same_bits(grad, grad_b)
    assert same_bits(sigma_r.reshape(-1), sigma) and same_bits(grad_r.reshape(-1, 3), grad)
    ref_sigma, ref_grad = sigma_and_gradient64(m, pts)
    e_sigma, e_grad = rel_err(C(sigma), ref_sigma), rel_err(C(grad), ref_grad)
    print(f"density_gradient {case}: sigma {e_sigma:.3e}, gradient {e_grad:.3e} (max |grad| {np.abs(ref_grad).max():.3e})")
    assert np.abs(ref_grad).max() > 0
    assert e_sigma <= 1e-4 and e_grad <= 1e-3


FIRST_RAY = {"render_lego_val": 46, "render_d8w256_val": 0}   # the lego fixture's first 46 rays miss the model: start where they hit


def golden_ro_rd(golden, name, n, dev):
    g = golden(name)
    rows = slice(FIRST_RAY[name], FIRST_RAY[name] + n)
    return (torch.from_numpy(np.ascontiguousarray(g["ro"][rows])).to(dev), torch.from_numpy(np.ascontiguousarray(g["rd"][rows])).to(dev))


def golden_rays(golden, name, n, dev):
    from nerf import _ops
    return _ops.pack_ray_rows(*golden_ro_rd(golden, name, n, dev), None, 2.0, 6.0)


def nets_of(name, dev):
    from test_input_gradients import make_models
    mkw, wfn, _ = CASES[name]
    return [m.requires_grad_(False) for m in make_models(mkw, *wfn(), dev)]


DRIVER_CASES = {
    # name: (golden case, rays, num_coarse, num_fine, thresholds)
    "4x128_16+24": ("render_lego_val", 37, 16, 24, (5.0, 15.0, 45.0)),
    "d8w256_12+20": ("render_d8w256_val", 9, 12, 20, (10.0, 50.0)),
    "coarse_only": ("render_lego_val", 5, 16, 0, (5.0, 15.0, 45.0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(DRIVER_CASES))
def test_driver_is_the_composition_of_its_stages_bit_for_bit(golden, dev, case, precision):
    """coarse_depths -> density forward -> density_resample -> density_gradient on (rays, z_fine) -> composite_normals, by hand, against
    dn_render_rays_normals: every output bit for bit, in both precisions (the bf16 path has no numeric gate of its own: it shares every
    kernel with the fp32 mode, and this test and the split test hold it)."""
    import nerf
    from nerf import _hip, _ops
    name, n, nc, nf, thres = DRIVER_CASES[case]
    nerf.set_precision(precision)
    prec = _hip.PREC_F32 if precision == "fp32" else _hip.PREC_BF16
    mc, mf = nets_of(name, dev)
    rays = golden_rays(golden, name, n, dev)
    rd = rays[:, 3:6]
    pc, pf = mc.packed_density(precision=prec), mf.packed_density(precision=prec)
    last, last_pack = (mf, pf) if nf else (mc, pc)
    streams = last.packed_density_grad(precision=prec)
    assert pc.precision == prec and streams.precision == prec
    th = torch.tensor(thres, dtype=torch.float32, device=dev)
    with torch.no_grad():
        z = _ops.coarse_depths(rays, nc, False, None)
        depth_c = acc_c = None
        if nf:
            rf_c = _ops.run_network_rays(pc, rays, z)
            depth_c, acc_c, z = _ops.density_resample(rf_c, z, rd, nf)
        sigma, g_pts = _ops.density_gradient(last_pack, streams, rays=rays, z=z)
        rf = torch.zeros(n, nc + nf, 4, device=dev)
        rf[..., 3] = sigma
        by_hand = (depth_c, acc_c) + _ops.composite_normals(rf, z, rd, g_pts, None, 0.0, th)
        driver = _ops.render_rays_normals(pc, pf if nf else None, streams, rays, nc, nf, False, 0.0, th)
    torch.cuda.synchronize()
    names = ("depth_c", "acc_c", "depth", "acc", "dex", "normal", "dex_normal")
    for label, a, b in zip(names, driver, by_hand):
        assert same_bits(a, b), (case, precision, label)
    normal, dex_normal = driver[5], driver[6]
    assert torch.isfinite(normal).all() and torch.isfinite(dex_normal).all()
    assert bool((normal.norm(dim=-1) <= driver[3] * (1 + 1e-5) + 1e-6).all())       # |sum w n| <= sum w = acc
    crossed = int((dex_normal.abs().sum(-1) > 0).sum())
    print(f"driver {case} {precision}: {crossed} of {dex_normal.shape[0] * n} (threshold, ray) pairs cross; max |normal| {float(normal.norm(dim=-1).max()):.3f}")
    assert float(normal.abs().max()) > 0


@pytest.mark.gpu
def test_normal_render_is_hipgraph_capturable(golden, dev):
    """dn_render_rays_normals reads nothing back on the host: a captured chunk replays to the eager outputs bit for bit."""
    from nerf import _hip, _ops
    mc, mf = nets_of("render_lego_val", dev)
    rays = golden_rays(golden, "render_lego_val", 21, dev)
    pc, pf = mc.packed_density(precision=_hip.PREC_F32), mf.packed_density(precision=_hip.PREC_F32)
    streams = mf.packed_density_grad(precision=_hip.PREC_F32)
    thres = torch.tensor([5.0, 15.0], device=dev)
    eager = _ops.render_rays_normals(pc, pf, streams, rays, 16, 24, False, 0.0, thres)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = _ops.render_rays_normals(pc, pf, streams, rays, 16, 24, False, 0.0, thres)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert same_bits(a, b)
    assert float(captured[5].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_render_dex_normals_does_not_depend_on_the_split(golden, dev, precision):
    """A 6 x 5 image of the 4 x 128 networks, 16 + 24 samples: chunksize 7, chunksize 30 and a max_workspace_bytes that forces a split
    of the one chunk give the same bits, and so do two calls; validation mode is image-shaped, train mode flat."""
    import nerf
    from nerf import _ops
    from test_input_gradients import make_cfg
    nerf.set_precision(precision)
    mc, mf = nets_of("render_lego_val", dev)
    ro, rd = (t.reshape(6, 5, 3) for t in golden_ro_rd(golden, "render_lego_val", 30, dev))
    ex = nerf.get_embedding_function(10)
    rkw = dict(num_coarse=16, num_fine=24, near=2.0, far=6.0)
    thres = [5.0, 15.0]

    def render(chunksize, mode="validation", **kw):
        with torch.no_grad():
            return nerf.render_dex_normals(6, 5, 1.0, mc, mf, ro, rd, make_cfg(rkw, chunksize), mode=mode, encode_position_fn=ex,
                                           m_thres_cand=thres, **kw)
    whole = render(30)
    need = _ops.render_normals_workspace_bytes(mc.packed_density(), mf.packed_density(), 30, 16, 24)
    one_ray = _ops.render_normals_workspace_bytes(mc.packed_density(), mf.packed_density(), 1, 16, 24)
    assert one_ray < need // 3
    others = {"chunksize 7": render(7), "workspace split": render(30, max_workspace_bytes=need // 3), "again": render(30)}
    flat = render(30, mode="train")
    torch.cuda.synchronize()
    assert isinstance(whole, nerf.DexNormals) and whole._fields == ("depth", "acc", "normal", "dex_depth", "dex_normal")
    assert whole.depth.shape == (6, 5) and whole.acc.shape == (6, 5) and whole.normal.shape == (6, 5, 3)
    assert len(whole.dex_depth) == 2 and len(whole.dex_normal) == 2
    assert whole.dex_depth[0].shape == (6, 5) and whole.dex_normal[1].shape == (6, 5, 3)
    assert flat.depth.shape == (30,) and flat.normal.shape == (30, 3) and flat.dex_normal[0].shape == (30, 3)

    def maps(out):
        return [out.depth, out.acc, out.normal] + list(out.dex_depth) + list(out.dex_normal)
    for label, out in others.items():
        for a, b in zip(maps(out), maps(whole)):
            assert same_bits(a, b), (precision, label)
    for a, b in zip(maps(flat), maps(whole)):
        assert same_bits(a, b.reshape(a.shape))
    assert float(whole.normal.abs().max()) > 0 and float(whole.dex_normal[0].abs().max()) > 0
    with pytest.raises(RuntimeError, match="max_workspace_bytes"):
        render(30, max_workspace_bytes=one_ray - 1)
    # the depth of the fine pass is render_dex_depth's up to the last bits (its sigma comes from the training-forward kernel)
    if precision == "fp32":
        with torch.no_grad():
            ref = nerf.render_dex_depth(6, 5, 1.0, mc, mf, ro, rd, make_cfg(rkw, 30), mode="validation", encode_position_fn=ex,
                                        m_thres_cand=thres)
        assert rel_err(C(whole.depth), C(ref[2])) <= 1e-5 and rel_err(C(whole.acc), C(ref[3])) <= 1e-5


@pytest.mark.gpu
def test_eval_driver_normals(dev, tmp_path):
    """eval_nerf.py --normals --m-thres 15 on a synthetic checkpoint at size 6: normal_<view>.npy / .png and one pair per threshold; the
    .npy files hold nerf.render_dex_normals' maps; --precision fp16 is refused."""
    import eval_nerf
    import nerf
    from nerf import synthetic as syn
    sd_c, sd_f = syn.synth_state_dict(7, **D4), syn.synth_state_dict(8, **D4)
    ck = tmp_path / "synthetic.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "6", "--views", "1", "--num-coarse", "16", "--num-fine", "24", "--normals", "--m-thres", "15",
              "--quiet"]
    with pytest.raises(SystemExit):
        eval_nerf.main(common + ["--precision", "fp16"])
    with pytest.raises(SystemExit):
        eval_nerf.main(common + ["--precision", "fp32", "--depth-only"])
    out = tmp_path / "out"
    res = eval_nerf.main(common + ["--precision", "fp32", "--savedir", str(out)])
    stems = ["normal_0000"] + [f"dex_normal_0000_m{m}" for m in (5, 10, 15)]
    assert sorted(p.name for p in out.iterdir()) == sorted([s + ".npy" for s in stems] + [s + ".png" for s in stems])
    # the API on the same view
    nerf.set_precision("fp32")
    coarse = eval_nerf.model_from_state_dict({k: torch.from_numpy(v) for k, v in sd_c.items()}, dev)
    fine = eval_nerf.model_from_state_dict({k: torch.from_numpy(v) for k, v in sd_f.items()}, dev)
    mode = dict(chunksize=36, lindisp=False, num_coarse=16, num_fine=24, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    pose = torch.from_numpy(syn.scene_pose(0, n_views=1)).to(dev)
    k_mat = torch.from_numpy(syn.intrinsic(6, 6)).to(dev)
    with torch.no_grad():
        ro, rd = nerf.get_ray_bundle(6, 6, float(k_mat[0, 0]), pose, k_mat)
        api = nerf.render_dex_normals(6, 6, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                      encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=[5.0, 10.0, 15.0])
    assert np.array_equal(np.load(out / "normal_0000.npy"), C(api.normal)) and api.normal.shape == (6, 6, 3)
    for m, n_map in zip((5, 10, 15), api.dex_normal):
        assert np.array_equal(np.load(out / f"dex_normal_0000_m{m}.npy"), C(n_map))
    assert same_bits(res["frames"][0][2].normal, api.normal)
    from PIL import Image
    png = np.asarray(Image.open(out / "dex_normal_0000_m15.png"))
    assert png.shape == (6, 6, 3)
    none = C(api.dex_normal[2]).any(-1) == 0
    assert (png[none] == 0).all() and (png[~none].any(-1)).all()                  # black exactly where there is no normal
