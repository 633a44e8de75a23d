"""The complete ray gradient: compositing backward w.r.t. depths and directions (dn_volume_render_backward_geom), backward of the
coarse depths (dn_coarse_depths_backward) and of the coarse + fine merge (dn_fine_depths_backward), their autograd functions and the
routing of volume_render_radiance_field / predict_and_render_radiance / run_one_iter_of_nerf - so that d ray_batch equals the
reference's autograd in all 11 columns, for world-space and for NDC rays.

Tolerances use the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES
from test_input_gradients import POSE_XI, _pose_rays64, make_cfg, make_models, no_fallback, pose_problem

NEW_SYMBOLS = ("dn_volume_render_backward_geom", "dn_coarse_depths_backward", "dn_fine_depths_backward")
UPSTREAMS = ("rgb", "depth", "acc", "disp", "weights")


def C(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- the yardstick: the closed form of the issue in float64 -------------------------------------------------------------------------
def closed_form64(rf, z, rd, noise, noise_std, white, ups):
    """g_z (N,S), g_rd (N,3) in float64 from the kernel's quantities: dalpha_i = s_i T_i - R_i / o_i, ddist_i = dalpha_i sigma_i
    exp(-sigma_i dist_i), g_z_i = gD w_i + |rd| (ddist_{i-1} - ddist_i) (no -ddist term for the last sample), g_rd = (sum ddist_i
    dz_i) rd / |rd|.  `ups`: dict of the upstream gradients present (rgb (N,3), depth, acc, disp (N), weights (N,S))."""
    rf, z, rd = rf.double(), z.double(), rd.double()
    n, s = z.shape
    nrm = rd.norm(dim=-1, keepdim=True)
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e10, dtype=torch.float64)], -1)
    dist = dz * nrm
    raw = rf[..., 3] + (noise.double() * noise_std if noise_std > 0.0 else 0.0)
    sigma = torch.relu(raw)
    e = torch.exp(-sigma * dist)
    alpha = 1.0 - e
    o = 1.0 - alpha + 1e-10
    trans = torch.cat([torch.ones(n, 1, dtype=torch.float64), torch.cumprod(o, -1)[:, :-1]], -1)
    w = alpha * trans
    c = torch.sigmoid(rf[..., :3])
    zero1, zero3 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64)
    g_c = ups["rgb"].double() if "rgb" in ups else zero3
    g_d = ups["depth"].double() if "depth" in ups else zero1
    g_a = ups["acc"].double() if "acc" in ups else zero1
    if white:
        g_a = g_a - g_c.sum(-1)
    if "disp" in ups:
        depth, acc = (w * z).sum(-1), w.sum(-1)
        q = depth / acc
        g_q = torch.where(q > 1e-10, -ups["disp"].double() / (q * q), zero1)
        g_d = g_d + g_q / acc
        g_a = g_a - g_q * depth / (acc * acc)
    s_i = (g_c[:, None, :] * c).sum(-1) + g_d[:, None] * z + g_a[:, None]
    if "weights" in ups:
        s_i = s_i + ups["weights"].double()
    sw = s_i * w
    r_i = sw.flip(-1).cumsum(-1).flip(-1) - sw      # sum over k > i
    dalpha = s_i * trans - r_i / o
    ddist = torch.where(raw > 0, dalpha * sigma * e, torch.zeros_like(dalpha))
    prev = torch.cat([torch.zeros(n, 1, dtype=torch.float64), ddist[:, :-1]], -1)
    own = ddist.clone()
    own[:, -1] = 0.0
    g_z = g_d[:, None] * w + nrm * (prev - own)
    g_rd = (ddist * dz).sum(-1, keepdim=True) * rd / nrm
    return g_z, g_rd


def oracle_grads64(rf, z, rd, noise, noise_std, white, ups):
    """(g_rf, g_z, g_rd): float64 autograd of oracle.volume_render on the same (fp32) inputs."""
    from oracle import nerf_oracle as oc
    rf64, z64, rd64 = (t.detach().cpu().double().requires_grad_(True) for t in (rf, z, rd))
    nz = None if noise is None else noise.detach().cpu().double()
    out = oc.volume_render(rf64, z64, rd64, nz, noise_std, white, ())
    loss = sum((out[k] * ups[k].detach().cpu().double()).sum() for k in ups)
    loss.backward()
    return rf64.grad, z64.grad, rd64.grad


def render_inputs(n, s, seed, dead_ray=None, tie_ray=1):
    """rf (n,s,4), z (n,s) ascending in [2,6] (ray `tie_ray`: two equal consecutive depths), ray rows (n,11), noise (n,s), upstream
    gradients; dead_ray: that ray's raw sigma is so negative that sigma + noise <= 0 everywhere."""
    gen = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float32)
    rf = randn(n, s, 4)
    rf[..., 3] = rf[..., 3] * 2.0 + 0.5
    if dead_ray is not None:
        rf[dead_ray, :, 3] = -5.0 - rf[dead_ray, :, 3].abs()
    z = (2.0 + 4.0 * torch.rand(n, s, generator=gen)).sort(-1).values
    if s >= 2:
        z[tie_ray, s // 2] = z[tie_ray, s // 2 - 1]
    rows = randn(n, 11)
    rows[:, 3:6] = torch.nn.functional.normalize(randn(n, 3), dim=-1) * (0.5 + torch.rand(n, 1, generator=gen))
    noise = randn(n, s)
    ups = dict(rgb=randn(n, 3), depth=randn(n), acc=randn(n), disp=randn(n), weights=randn(n, s))
    return rf, z, rows, noise, ups


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_resolvable(hiplib):
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(raw, name), name
    assert hiplib.dn_abi_version() == 2      # additive: the ABI version stays


def test_argument_validation_returns_before_gpu_work(hiplib):
    """NULL rf / z / rd, more than 1024 samples, a misaligned rf -> DN_E_INVAL with a message; zero rays -> 0.  No pointer is
    dereferenced and nothing is launched (the device pointers here are small integers)."""
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def geom(rf=fake, z=fake, rd=fake, n=4, s=8, g_rf=fake, g_z=fake, g_rd=fake):
        return hiplib.dn_volume_render_backward_geom(rf, z, rd, 3, None, 0.0, 0, n, s, fake, None, None, None, None, g_rf, g_z, g_rd, None)
    for kw in (dict(rf=None), dict(z=None), dict(rd=None), dict(g_rf=None, g_z=None, g_rd=None)):
        assert geom(**kw) == -1000, kw
        assert b"dn_volume_render_backward_geom: bad arguments" in hiplib.dn_last_error()
    assert geom(s=1025) == -1000
    assert b"1024 samples" in hiplib.dn_last_error()
    assert geom(rf=odd) == -1000
    assert b"16-byte aligned" in hiplib.dn_last_error()
    assert geom(g_rf=odd) == -1000
    assert b"16-byte aligned" in hiplib.dn_last_error()
    assert geom(n=0) == 0 and geom(n=0, rf=None) == 0

    def coarse(rays=fake, stride=11, n=4, nc=8, g_z=fake, out=fake):
        return hiplib.dn_coarse_depths_backward(rays, stride, n, nc, 0, None, g_z, out, None)
    for kw in (dict(rays=None), dict(g_z=None), dict(out=None), dict(stride=6), dict(nc=0)):
        assert coarse(**kw) == -1000, kw
        assert b"dn_coarse_depths_backward" in hiplib.dn_last_error()
    assert coarse(n=0) == 0

    def fine(zc=fake, zs=fake, g=fake, n=4, nc=8, nf=8, out=fake):
        return hiplib.dn_fine_depths_backward(zc, zs, g, n, nc, nf, out, None)
    for kw in (dict(zc=None), dict(zs=None), dict(g=None), dict(out=None), dict(nc=0), dict(nc=513), dict(nf=0), dict(nc=512, nf=1537)):
        assert fine(**kw) == -1000, kw
        assert b"dn_fine_depths_backward" in hiplib.dn_last_error()
    assert fine(n=0) == 0


@pytest.mark.parametrize("white,noise_std", [(True, 0.0), (False, 0.2)])
def test_closed_form_equals_float64_autograd_of_the_oracle(white, noise_std):
    """Guards the yardstick: the closed form the kernel implements, as this file's float64 helper, against float64 autograd of
    oracle.volume_render (N = 5, S = 65, every upstream gradient live) to 1e-12."""
    rf, z, rows, noise, ups = render_inputs(5, 65, seed=1)
    rd = rows[:, 3:6]
    _, g_z, g_rd = oracle_grads64(rf, z, rd, noise, noise_std, white, ups)
    c_z, c_rd = closed_form64(rf, z, rd, noise, noise_std, white, ups)
    assert float(g_z.abs().max()) > 0 and float(g_rd.abs().max()) > 0
    assert rel_err(c_z.numpy(), g_z.numpy()) <= 1e-12
    assert rel_err(c_rd.numpy(), g_rd.numpy()) <= 1e-12


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
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
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def _geom_case(dev, rf, z, rows, noise, noise_std, white, ups, stride, what):
    """One launch of the geometry kernel against the float64 oracle and against the plain kernel's g_rf."""
    from nerf import _ops
    rows_d = rows.to(dev)
    rd_d = rows_d[:, 3:6] if stride == 11 else rows_d[:, 3:6].contiguous()
    assert rd_d.stride(0) == stride
    nz = noise.to(dev) if noise_std > 0.0 else None
    g = {k: v.to(dev) for k, v in ups.items()}
    args = (rf.to(dev), z.to(dev), rd_d, nz, noise_std, white, g.get("rgb"), g.get("depth"), g.get("acc"), g.get("disp"), g.get("weights"))
    g_rf, g_z, g_rd = _ops.volume_render_bwd_geom(*args)
    plain = _ops.volume_render_bwd(*args)
    assert torch.equal(g_rf, plain), (what, "g_rf differs from dn_volume_render_backward's")
    only_z = _ops.volume_render_bwd_geom(*args, want_rf=False, want_rd=False)
    assert only_z[0] is None and only_z[2] is None and torch.equal(only_z[1], g_z), what
    ref_rf, ref_z, ref_rd = oracle_grads64(rf, z, rows[:, 3:6], noise if noise_std > 0.0 else None, noise_std, white, ups)
    e_rf, e_z, e_rd = rel_err(C(g_rf), ref_rf.numpy()), rel_err(C(g_z), ref_z.numpy()), rel_err(C(g_rd), ref_rd.numpy())
    assert e_rf <= 1e-4 and e_z <= 1e-4 and e_rd <= 1e-4, (what, e_rf, e_z, e_rd)
    return e_rf, e_z, e_rd


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 2, 64, 65, 192, 300, 520, 1024])
def test_geometry_kernel_against_float64_autograd_of_the_oracle(dev, s):
    """dn_volume_render_backward_geom, N = 5 (the last workgroup is not full), S on both sides of every chunk boundary, in every
    MAXC instance and at the maximum (1024: 16 full chunks), rd_stride 3 and 11, white background on / off, injected noise (std 0.2)
    and none, each upstream gradient alone and all five together; one ray holds two equal consecutive depths.  A second data set
    has one ray with every sigma <= 0 (no g_disp there: disp is NaN in the reference too).  g_rf, g_z, g_rd <= 1e-4 against float64
    autograd of oracle.volume_render on the same fp32 inputs; g_rf bit-equal to dn_volume_render_backward's."""
    rf, z, rows, noise, ups = render_inputs(5, s, seed=10 + s)
    worst = [0.0, 0.0, 0.0]
    for stride in (3, 11):
        for white in (False, True):
            for noise_std in (0.0, 0.2):
                for pick in UPSTREAMS + ("all",):
                    chosen = dict(ups) if pick == "all" else {pick: ups[pick]}
                    e = _geom_case(dev, rf, z, rows, noise, noise_std, white, chosen, stride, (s, stride, white, noise_std, pick))
                    worst = [max(a, b) for a, b in zip(worst, e)]
    rf, z, rows, noise, ups = render_inputs(5, s, seed=50 + s, dead_ray=2)
    del ups["disp"]
    for stride in (3, 11):
        for white in (False, True):
            for noise_std in (0.0, 0.2):
                e = _geom_case(dev, rf, z, rows, noise, noise_std, white, ups, stride, (s, stride, white, noise_std, "dead ray"))
                worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"geometry kernel S={s}: worst g_rf {worst[0]:.2e}, g_z {worst[1]:.2e}, g_rd {worst[2]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("nc", [2, 64, 128])
def test_coarse_depths_backward_against_float64_autograd_of_the_oracle(dev, nc, lindisp):
    """dn_coarse_depths_backward, N = 5, with and without the stratified jitter, ray rows of 8 and 11 columns: <= 1e-4."""
    from nerf import _ops
    from oracle import nerf_oracle as oc
    gen = torch.Generator().manual_seed(nc + int(lindisp))
    n = 5
    for jitter in (False, True):
        for cols in (8, 11):
            rows = torch.randn(n, cols, generator=gen)
            rows[:, 6] = 0.3 + 1.7 * torch.rand(n, generator=gen)
            rows[:, 7] = 4.0 + 2.0 * torch.rand(n, generator=gen)
            t_rand = torch.rand(n, nc, generator=gen) if jitter else None
            g_z = torch.randn(n, nc, generator=gen)
            near = rows[:, 6:7].double().requires_grad_(True)
            far = rows[:, 7:8].double().requires_grad_(True)
            z64 = oc.coarse_depths(near, far, nc, lindisp, None if t_rand is None else t_rand.double())
            (z64 * g_z.double()).sum().backward()
            ref = torch.cat([near.grad, far.grad], -1)
            got = _ops.coarse_depths_bwd(rows.to(dev), nc, lindisp, None if t_rand is None else t_rand.to(dev), g_z.to(dev))
            # the forward the backward belongs to is the library's own
            z_lib = _ops.coarse_depths(rows.to(dev), nc, lindisp, None if t_rand is None else t_rand.to(dev))
            assert rel_err(C(z_lib), z64.detach().numpy()) <= 1e-6
            err = rel_err(C(got), ref.numpy())
            print(f"coarse depths backward nc={nc} lindisp={lindisp} jitter={jitter} cols={cols}: {err:.2e}")
            assert float(ref.abs().max()) > 0 and err <= 1e-4, (nc, lindisp, jitter, cols, err)


@pytest.mark.gpu
@pytest.mark.parametrize("nc,nf", [(5, 3), (64, 64), (64, 128)])
def test_fine_depths_backward_is_the_gather_of_a_stable_sort(dev, nc, nf):
    """dn_fine_depths_backward: exact equality with the gather torch.sort(cat(z_coarse, z_samples), stable=True) defines.  Ray 0:
    both halves ascending; ray 1: a sample equal to a coarse depth (the coarse entry comes first); ray 2: a descending z_coarse; ray
    3: unsorted samples; ray 4: ties inside z_coarse and unsorted samples.  z_fine[p(j)] == z_coarse[j] bitwise; the sums agree bit
    for bit."""
    from nerf import _ops
    gen = torch.Generator().manual_seed(nc * 1000 + nf)
    n = 5
    zc = (2.0 + 4.0 * torch.rand(n, nc, generator=gen)).sort(-1).values
    zs = 2.0 + 4.0 * torch.rand(n, nf, generator=gen)
    zs[:3] = zs[:3].sort(-1).values
    zs[1, nf // 2] = zc[1, nc // 2]
    zs[1] = zs[1].sort(-1).values
    zc[2] = zc[2].flip(-1)
    zc[4, 2] = zc[4, 1]
    zs[4, 0] = zc[4, 1]
    g_fine = torch.randn(n, nc + nf, generator=gen)
    vals, idx = torch.sort(torch.cat([zc, zs], -1), dim=-1, stable=True)
    slot = torch.argsort(idx, dim=-1)[:, :nc]            # p(j): where element j of the concatenation went
    assert torch.equal(vals.gather(-1, slot), zc)
    ref = g_fine.gather(-1, slot)
    got = _ops.fine_depths_bwd(zc.to(dev), zs.to(dev), g_fine.to(dev))
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(got.sum(), ref.to(dev).sum())
    if nc >= 10:      # the forward's own merge puts the coarse depths where the backward reads their gradient
        ordered = torch.tensor([0, 1, 3, 4])
        w = torch.rand(n, nc, generator=gen)
        z_fine, z_samp = _ops.fine_depths(zc.to(dev), w.to(dev), nf, None, want_samples=True)
        probe = torch.arange(nc + nf, dtype=torch.float32, device=dev).expand(n, nc + nf).contiguous()
        where = _ops.fine_depths_bwd(zc.to(dev), z_samp, probe).long()
        assert torch.equal(z_fine.gather(-1, where).cpu()[ordered], zc[ordered])
        assert torch.equal(z_fine.gather(-1, where).cpu()[2], zc[2])


@pytest.mark.gpu
def test_volume_render_radiance_field_autograd_in_depths_and_directions(dev, monkeypatch):
    """volume_render_radiance_field: z and rd requiring grad with a detached rf; all three requiring grad (rd a strided view of ray
    rows: its gradient comes back through the slice); and with neither z nor rd requiring grad the geometry entry is not called and
    rf.grad is bit-identical to dn_volume_render_backward's."""
    import nerf
    from nerf import _ops
    rf, z, rows, noise, ups = render_inputs(5, 65, seed=3)
    up = {k: v.to(dev) for k, v in ups.items()}

    def loss_of(out):
        return ((out[0] * up["rgb"]).sum() + (out[1] * up["disp"]).sum() + (out[2] * up["acc"]).sum() + (out[3] * up["weights"]).sum()
                + (out[4] * up["depth"]).sum())
    ref_rf, ref_z, ref_rd = oracle_grads64(rf, z, rows[:, 3:6], None, 0.0, True, ups)
    # z, rd with a detached rf
    z_l = z.to(dev).requires_grad_(True)
    rd_l = rows[:, 3:6].to(dev).contiguous().requires_grad_(True)
    loss_of(nerf.volume_render_radiance_field(rf.to(dev), z_l, rd_l, white_background=True, m_thres_cand=[5.0, 10.0])).backward()
    assert rel_err(C(z_l.grad), ref_z.numpy()) <= 1e-4 and rel_err(C(rd_l.grad), ref_rd.numpy()) <= 1e-4
    # all three, rd a column slice of rows that require grad
    rf_l = rf.to(dev).requires_grad_(True)
    z_l = z.to(dev).requires_grad_(True)
    rows_l = rows.to(dev).requires_grad_(True)
    loss_of(nerf.volume_render_radiance_field(rf_l, z_l, rows_l[:, 3:6], white_background=True)).backward()
    assert rel_err(C(z_l.grad), ref_z.numpy()) <= 1e-4 and rel_err(C(rows_l.grad[:, 3:6]), ref_rd.numpy()) <= 1e-4
    assert rel_err(C(rf_l.grad), ref_rf.numpy()) <= 1e-4
    assert bool((rows_l.grad[:, :3] == 0).all()) and bool((rows_l.grad[:, 6:] == 0).all())
    plain = _ops.volume_render_bwd(rf.to(dev), z.to(dev), rows.to(dev)[:, 3:6], None, 0.0, True, up["rgb"], up["depth"], up["acc"],
                                   up["disp"], up["weights"])
    assert torch.equal(rf_l.grad, plain)
    # rf alone: the geometry entry must not run
    def boom(*a, **k):
        raise AssertionError("the geometry backward ran although neither z nor rd requires grad")
    with monkeypatch.context() as mp:
        mp.setattr(_ops, "volume_render_bwd_geom", boom)
        rf_l = rf.to(dev).requires_grad_(True)
        loss_of(nerf.volume_render_radiance_field(rf_l, z.to(dev), rows.to(dev)[:, 3:6], white_background=True)).backward()
    assert torch.equal(rf_l.grad, plain)


# ---- the contract: d ray_batch in all 11 columns ------------------------------------------------------------------------------------
BLOCKS = {"ro": slice(0, 3), "rd": slice(3, 6), "near_far": slice(6, 8), "viewdir": slice(8, 11)}
H = W = 400


def _focal():
    from nerf import synthetic as syn
    return float(syn.intrinsic(H, W)[0, 0])


def _rows_of(kind, ro64, rd64, focal=None):
    """The packed ray rows [ro, rd, near, far, viewdir] in float64: world space (near 2, far 6), or warped to NDC by oracle.ndc_rays
    (near 0, far 1; the view direction stays that of the unwarped ray, as run_one_iter_of_nerf packs it)."""
    from oracle import nerf_oracle as oc
    vd = rd64 / rd64.norm(dim=-1, keepdim=True)
    if kind == "world":
        ro, rd, near, far = ro64, rd64, 2.0, 6.0
    else:
        ro, rd = oc.ndc_rays(H, W, _focal() if focal is None else focal, 1.0, ro64, rd64)
        near, far = 0.0, 1.0
    return torch.cat([ro, rd, torch.full_like(vd[:, :1], near), torch.full_like(vd[:, :1], far), vd], -1)


def _loss(out, target):
    """Both MSEs plus small multiples of the means of depth_c, depth_f and acc_f: every upstream path of the compositing is live."""
    mse = torch.nn.functional.mse_loss
    return mse(out[0], target) + mse(out[3], target) + 0.05 * out[1].mean() + 0.05 * out[4].mean() + 0.05 * out[5].mean()


def _oracle_render(rows, dtype):
    from oracle import nerf_oracle as oc
    mkw, wfn, rkw = CASES["render_lego_val"]
    sd_c, sd_f = wfn()
    tsd_c = {k: torch.from_numpy(v).to(dtype) for k, v in sd_c.items()}
    tsd_f = {k: torch.from_numpy(v).to(dtype) for k, v in sd_f.items()}
    cfg_o = oc.RenderCfg(chunksize=4096, m_thres=(), num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"], near=rkw["near"], far=rkw["far"],
                         white_background=rkw["white_background"])
    mcfg = oc.ModelCfg(**mkw)
    return oc.predict_and_render(rows, tsd_c, tsd_f, mcfg, mcfg, cfg_o)


def _oracle_row_gradient(kind, dtype):
    """d loss / d ray rows (256, 11) through oracle.predict_and_render in `dtype`; the rows are the fp32 roundings in both."""
    ro64, rd64, target = pose_problem()
    rows = _rows_of(kind, ro64, rd64).float().to(dtype).requires_grad_(True)
    _loss(_oracle_render(rows, dtype), target.to(dtype)).backward()
    return rows.grad.double().numpy()


# the oracle's own fp32-vs-float64 difference per column block (oracle_row_floors(), measured on the build machine's CPU); the gates
# below are pinned to these constants
ROW_FLOORS = {
    "world": {"ro": 5.7e-4, "rd": 3.4e-4, "near_far": 6.6e-5, "viewdir": 1.6e-5},
    "ndc": {"ro": 2.4e-5, "rd": 2.7e-5, "near_far": 3.9e-5, "viewdir": 2.4e-5},
}


def oracle_row_floors():
    """How ROW_FLOORS was measured; the tests do not re-measure it, so a numerically worse oracle run cannot widen a gate."""
    out = {}
    for kind in ("world", "ndc"):
        g64, g32 = _oracle_row_gradient(kind, torch.float64), _oracle_row_gradient(kind, torch.float32)
        out[kind] = {k: rel_err(g32[:, sl], g64[:, sl]) for k, sl in BLOCKS.items()}
    return out


@pytest.fixture(scope="module")
def row_refs():
    return {kind: _oracle_row_gradient(kind, torch.float64) for kind in ("world", "ndc")}


def _library_row_gradient(kind, dev, monkeypatch):
    import nerf
    ro64, rd64, target = pose_problem()
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    rows = _rows_of(kind, ro64, rd64).float().to(dev).requires_grad_(True)
    with no_fallback(monkeypatch):
        out = nerf.predict_and_render_radiance(rows, mc, mf, make_cfg(rkw), mode="train", encode_position_fn=ex, encode_direction_fn=ed)
        _loss(out, target.float().to(dev)).backward()
    return rows.grad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["world", "ndc"])
def test_ray_batch_gradient_equals_the_oracles_in_all_11_columns(dev, row_refs, kind, monkeypatch):
    """The contract.  d ray_batch of predict_and_render_radiance (fp32 mode, lego weights, 64 + 64 samples, perturb off, noise 0,
    frozen weights, all 256 rays of pose_problem()) against float64 autograd of oracle.predict_and_render, per column block (ro, rd,
    near / far, view direction), for world-space rows and for rows warped to NDC.  Gate per block: max(1e-3, 4 x floor), floor = the
    oracle's own fp32-vs-float64 difference on the same rows (ROW_FLOORS, measured once on the CPU by oracle_row_floors()).
    Before this feature near / far were exactly 0 and rd lacked its term through |rd|."""
    got = C(_library_row_gradient(kind, dev, monkeypatch))
    ref = row_refs[kind]
    assert got.shape == ref.shape == (256, 11)
    errs = {k: rel_err(got[:, sl], ref[:, sl]) for k, sl in BLOCKS.items()}
    gates = {k: max(1e-3, 4.0 * ROW_FLOORS[kind][k]) for k in BLOCKS}
    print(f"d ray_batch ({kind}): errors {errs}, gates {gates}, block maxima { {k: float(np.abs(ref[:, sl]).max()) for k, sl in BLOCKS.items()} }")
    for k in BLOCKS:
        assert float(np.abs(ref[:, BLOCKS[k]]).max()) > 0, k
        assert errs[k] <= gates[k], (kind, k, errs[k], gates[k])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["world", "ndc"])
def test_ray_batch_gradient_is_bit_reproducible(dev, kind, monkeypatch):
    a = _library_row_gradient(kind, dev, monkeypatch)
    b = _library_row_gradient(kind, dev, monkeypatch)
    assert bool(torch.isfinite(a).all()) and float(a[:, 6:8].abs().max()) > 0
    assert torch.equal(a, b)


# ---- NDC pose and focal gradient end to end -----------------------------------------------------------------------------------------
def _oracle_ndc_pose_focal_gradient(dtype):
    ro64, rd64, target = pose_problem()
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    focal = torch.tensor(_focal(), dtype=torch.float64, requires_grad=True)
    ro, rd = _pose_rays64(xi, ro64, rd64)
    rows = _rows_of("ndc", ro.to(dtype), rd.to(dtype), focal=focal.to(dtype))
    _loss(_oracle_render(rows, dtype), target.to(dtype)).backward()
    return xi.grad.numpy().copy(), focal.grad.numpy().copy().reshape(1)


# oracle_ndc_pose_floors() as measured on the build machine's CPU: (dL/dxi, dL/dfocal)
NDC_POSE_FLOORS = (7.1e-4, 5.9e-4)


def oracle_ndc_pose_floors():
    """The oracle's own fp32-vs-float64 difference of dL/dxi and dL/dfocal; how NDC_POSE_FLOORS was measured."""
    g64, g32 = _oracle_ndc_pose_focal_gradient(torch.float64), _oracle_ndc_pose_focal_gradient(torch.float32)
    return tuple(rel_err(a, b) for a, b in zip(g32, g64))


@pytest.mark.gpu
def test_ndc_pose_and_focal_gradient_end_to_end_against_the_float64_oracle(dev, monkeypatch):
    """dL/dxi (the rigid update of test_input_gradients._pose_rays64) and dL/dfocal through run_one_iter_of_nerf with
    dataset.no_ndc False - the NDC warp and the view-direction normalisation under torch autograd, everything behind them on the HIP
    kernels - against float64 autograd through the CPU oracle.  The warped directions change length with the pose and with the
    focal length: the terms this gradient lacked.  Gate: max(1e-3, 4 x floor), floors recorded in NDC_POSE_FLOORS."""
    import nerf
    ro64, rd64, target = pose_problem()
    ref_xi, ref_f = _oracle_ndc_pose_focal_gradient(torch.float64)
    mkw, wfn, rkw = CASES["render_lego_val"]
    mc, mf = make_models(mkw, *wfn(), dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    cfg = make_cfg(dict(rkw, near=0.0, far=1.0))
    cfg.dataset.no_ndc = False
    xi = torch.tensor(POSE_XI, dtype=torch.float64, requires_grad=True)
    focal = torch.tensor(_focal(), dtype=torch.float64, device=dev, requires_grad=True)
    ro, rd = _pose_rays64(xi, ro64, rd64)
    with no_fallback(monkeypatch):
        out = nerf.run_one_iter_of_nerf(H, W, focal, mc, mf, ro.float().to(dev), rd.float().to(dev), cfg, mode="train",
                                        encode_position_fn=ex, encode_direction_fn=ed)
        _loss(out, target.float().to(dev)).backward()
    e_xi, e_f = rel_err(xi.grad.numpy(), ref_xi), rel_err(C(focal.grad).reshape(1), ref_f)
    gates = [max(1e-3, 4.0 * f) for f in NDC_POSE_FLOORS]
    print(f"NDC pose / focal gradient: dL/dxi {ref_xi} err {e_xi:.3e} (gate {gates[0]:.3e}); dL/dfocal {ref_f} err {e_f:.3e} (gate {gates[1]:.3e})")
    assert float(np.abs(ref_f).max()) > 0
    assert e_xi <= gates[0] and e_f <= gates[1], (e_xi, e_f, gates)
