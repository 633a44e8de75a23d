"""The depth-only render path (nerf.render_dex_depth -> dn_render_rays_depth): the density sub-network pack, the fixed-shape
no-view-direction instances of the 48-point kernel, the sigma-only compositing / resampling kernels and the Python surface.

Tolerances are the project's (tests/test_hip_parity.py): index work and everything that is the same
arithmetic on the same inputs is compared bit for bit; fp32 against the reference-recorded goldens at `max|a-b| <= 1e-4 max|b|`
and 0.995 Dex agreement; the 16-bit modes against the floors of test_headline_kernel_16bit_against_reference_golden."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from golden_cases import CASES, D4, D8, M_THRES, d8_weights, lego_weights

TOL = 1e-4                      # test_hip_parity.TOL
DEX_AGREE_FP32 = 0.995          # test_render_goldens_end_to_end
FLOORS_16 = {"bf16": (36.5, 0.975), "fp16": (53.0, 0.996)}   # (depth_floor dB, dex_floor) of the 16-bit headline test
SHAPES = {"lego": (D4, lego_weights), "d8w256": (D8, d8_weights)}


def full_desc(_hip, kw):
    return _hip.MlpDesc(kw["num_layers"], kw["hidden_size"], kw["skip_connect_every"], kw["num_encoding_fn_xyz"],
                        kw["num_encoding_fn_dir"], 1, 1, int(kw["use_viewdirs"]), 1, 1)


def density_desc(_hip, kw):
    out = _hip.MlpDesc()
    assert _hip.lib().dn_mlp_density_desc(ctypes.byref(full_desc(_hip, kw)), ctypes.byref(out)) == 0
    return out


# ---- CPU tests --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("dn_mlp_density_desc", "dn_mlp_density_packed_bytes", "dn_mlp_pack_density", "dn_composite_density",
               "dn_density_resample", "dn_render_depth_workspace_bytes", "dn_render_rays_depth")


def test_new_entry_points_are_declared_exported_and_resolvable():
    import re
    from nerf import _hip
    header = open(os.path.join(REPO, "include", "dexnerf_hip.h")).read()
    declared = set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", header))
    lib = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert lib.dn_abi_version() == 2 and "#define DN_ABI_VERSION 2" in header


def test_density_descriptor_and_packed_size():
    from nerf import _hip
    lib = _hip.lib()
    for kw in (D4, D8, dict(D8, num_layers=6, hidden_size=128, skip_connect_every=3)):
        full, dens = full_desc(_hip, kw), density_desc(_hip, kw)
        assert dens.use_viewdirs == 0
        for f in ("num_layers", "hidden_size", "skip_connect_every", "num_encoding_fn_xyz", "log_sampling_xyz"):
            assert getattr(dens, f) == getattr(full, f)
        again = _hip.MlpDesc()   # a descriptor without view directions passes through
        assert lib.dn_mlp_density_desc(ctypes.byref(dens), ctypes.byref(again)) == 0 and bytes(again) == bytes(dens)
        for prec in (_hip.PREC_F32, _hip.PREC_BF16, _hip.PREC_F16):
            n = lib.dn_mlp_density_packed_bytes(ctypes.byref(full), prec)
            assert n > 0 and n == lib.dn_mlp_packed_bytes(ctypes.byref(dens), prec)
    assert lib.dn_mlp_density_desc(None, ctypes.byref(_hip.MlpDesc())) == -1000
    # both fixed shapes carry the complete fp16 range tracker (the condition of the guarded fp16 render policy)
    assert lib.dn_fp16_range_guard(ctypes.byref(density_desc(_hip, D8))) == 1
    assert lib.dn_fp16_range_guard(ctypes.byref(density_desc(_hip, D4))) == 1


def test_render_rays_depth_validates_its_arguments_without_a_gpu():
    from nerf import _hip
    lib = _hip.lib()
    fake = ctypes.c_void_p(256 * 4096)   # never dereferenced: every case below is refused before any GPU work
    dens, full = density_desc(_hip, D8), full_desc(_hip, D8)

    def call(dc=dens, df=dens, nf=128, k=0, th=None, dex=None, pc=fake, n=16):
        return lib.dn_render_rays_depth(None if dc is None else ctypes.byref(dc), pc, None if df is None else ctypes.byref(df),
                                        fake if df is not None else None, _hip.PREC_BF16, fake, 8, n, 64, nf, 0, 0.0, th, k, None,
                                        None, None, None, fake, fake, fake, fake, dex, fake, None)
    assert call(dc=None) == -1000                                   # NULL descriptor
    assert b"bad arguments" in lib.dn_last_error()
    assert call(df=None) == -1000                                   # fine pass without a fine net
    assert call(k=-1) == -1000                                      # K < 0
    assert call(k=3, th=None, dex=fake) == -1000                    # thresholds missing
    assert call(dc=full) == -1000 and call(df=full) == -1000        # a density descriptor that still has use_viewdirs = 1
    assert b"use_viewdirs" in lib.dn_last_error()
    w64 = density_desc(_hip, dict(D8, hidden_size=64))
    assert call(dc=w64) == -1001                                    # unsupported width
    assert lib.dn_render_depth_workspace_bytes(-1, 64, 64) == 0
    n, nc, nf = 100, 64, 128
    need = 4 * n * (nc + 4 * nc + (nc + nf) + 4 * (nc + nf)) + 256
    assert need <= lib.dn_render_depth_workspace_bytes(n, nc, nf) < lib.dn_render_workspace_bytes(n, nc, nf)   # no weights buffer


@pytest.mark.parametrize("shape", list(SHAPES))
def test_density_subnetwork_algebra_in_float64(shape):
    """Host restatement: trunk + a 4-row head (rows 0-2 zero, row 3 = fc_alpha) gives the sigma of the full network."""
    from oracle import nerf_oracle as oc
    kw, wfn = SHAPES[shape]
    rng = np.random.default_rng(3)
    for sd in wfn():
        sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}
        mc = oc.ModelCfg(**kw)
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(257, mc.dim_xyz + mc.dim_dir)))
        ref = oc.flexible_mlp(sd, x, mc)[:, 3]
        width = kw["hidden_size"]
        sub = {k: v for k, v in sd.items() if k.startswith(("layer1.", "layers_xyz."))}
        sub["fc_out.weight"] = torch.cat([torch.zeros(3, width, dtype=torch.float64), sd["fc_alpha.weight"]], 0)
        sub["fc_out.bias"] = torch.cat([torch.zeros(3, dtype=torch.float64), sd["fc_alpha.bias"]], 0)
        out = oc.flexible_mlp(sub, x[:, : mc.dim_xyz], oc.ModelCfg(**dict(kw, use_viewdirs=False)))
        assert torch.equal(out[:, :3], torch.zeros_like(out[:, :3]))
        assert float((out[:, 3] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ---- GPU tests --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _named_precision_and_fp32_on_exit():
    """As in test_hip_parity: a test that names 'bf16' renders in bf16 unless it sets the policy itself; fp32 on exit."""
    import nerf
    from nerf import train_utils
    nerf.set_render_policy("bf16")
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")
    train_utils._FP16_RENDER_DISABLED[0] = False


def G(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(t):
    return t.detach().cpu().numpy()


_MODELS = {}


def models_of(name, dev):
    """(coarse, fine) FlexibleNeRFModels of a golden case, built once per weight set."""
    import nerf
    mkw, wfn, _ = CASES[name]
    key = (wfn.__name__, str(dev))
    if key not in _MODELS:
        out = []
        for sd in wfn():
            m = nerf.models.FlexibleNeRFModel(**mkw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            out.append(m.to(dev))
        _MODELS[key] = out
    return _MODELS[key]


def make_cfg(rkw, chunksize=4096, no_ndc=True, **over):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=rkw.get("lindisp", False), num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"],
                perturb=rkw.get("perturb", False), radiance_field_noise_std=rkw.get("noise_std", 0.0),
                white_background=rkw.get("white_background", False))
    mode.update(over)
    return nerf.CfgNode(dict(dataset=dict(near=rkw["near"], far=rkw["far"], no_ndc=no_ndc),
                             nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def dex_agreement(dex, dex_ref):
    dex, dex_ref = np.asarray(dex, np.float64), np.asarray(dex_ref, np.float64)
    return float((np.abs(dex - dex_ref) <= TOL * np.abs(dex_ref).max()).mean())


def psnr_db(a, b, peak):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float(10.0 * np.log10(peak * peak / max(mse, 1e-14)))


def embedders():
    import nerf
    return nerf.get_embedding_function(10), nerf.get_embedding_function(4)


def depth_render(name, g, dev, mode="validation", thres=M_THRES, cfg=None, rays=None):
    import nerf
    mc, mf = models_of(name, dev)
    ex, ed = embedders()
    ro, rd = (G(g["ro"], dev)[None], G(g["rd"], dev)[None]) if rays is None else rays
    with torch.no_grad():
        return nerf.render_dex_depth(1, ro.shape[-2], 1.0, mc, mf, ro, rd, cfg or make_cfg(CASES[name][2]), mode=mode,
                                     encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=None if thres is None else list(thres))


def full_render(name, g, dev, mode="validation", thres=M_THRES, cfg=None, rays=None):
    import nerf
    mc, mf = models_of(name, dev)
    ex, ed = embedders()
    ro, rd = (G(g["ro"], dev)[None], G(g["rd"], dev)[None]) if rays is None else rays
    with torch.no_grad():
        return nerf.run_one_iter_of_nerf(1, ro.shape[-2], 1.0, mc, mf, ro, rd, cfg or make_cfg(CASES[name][2]), mode=mode,
                                         encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=None if thres is None else list(thres))


def sigma_pair(name, g, dev):
    """(full pack's raw field, density pack's raw field) of the fine net on the golden fine points, current precision."""
    from nerf import _ops
    mf = models_of(name, dev)[1]
    pts = G(g["pts_fine"], dev)
    rd = torch.from_numpy(g["rd"])
    vd = (rd / rd.norm(p=2, dim=-1).unsqueeze(-1)).to(dev)
    s = pts.shape[1]
    with torch.no_grad():
        full = _ops.run_network_pts(mf.packed(), pts.reshape(-1, 3), vd, s)
        dens = _ops.run_network_pts(mf.packed_density(), pts.reshape(-1, 3), None, s)
    return full.reshape(-1, s, 4), dens.reshape(-1, s, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["render_lego_val", "render_d8w256_val"])
def test_density_pack_gives_the_full_networks_sigma(golden, dev, name, precision):
    import nerf
    from nerf import _ops
    g = golden(name)
    nerf.set_precision(precision)
    full, dens = sigma_pair(name, g, dev)
    assert torch.equal(dens[..., :3], torch.zeros_like(dens[..., :3]))       # rows 0-2 and biases 0-2 are +0
    assert not torch.signbit(dens[..., :3]).any()
    bit_equal = torch.equal(full[..., 3], dens[..., 3])
    print(f"{name} {precision}: density sigma bit-equal to the full pack's: {bit_equal}; "
          f"max |diff| {float((full[..., 3] - dens[..., 3]).abs().max()):.3e}")
    if precision == "fp32":
        assert rel_err(C(dens[..., 3]), g["rf_fine"][..., 3]) < TOL
    elif name == "render_d8w256_val":
        # the 16-bit gate of the headline test, stage-wise: Dex readout on this sigma against the readout on the golden sigma
        z, rdv = G(g["z_fine"], dev), G(g["rd"], dev)
        with torch.no_grad():
            dex16 = _ops.volume_render_fwd(dens, z, rdv, None, 0.0, False, list(M_THRES), want_weights=False)[5]
        frac = dex_agreement(C(dex16), g["vf_dex"])
        print(f"  fixed-depth Dex agreement {frac:.4f}")
        assert frac > FLOORS_16[precision][1]
    assert torch.isfinite(dens).all()


RESAMPLE_CASES = [(64, 64, False), (64, 128, False), (37, 22, False), (64, 64, True), (64, 128, True), (37, 22, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("nc,nf,drawn", RESAMPLE_CASES)
def test_density_resample_is_bit_identical_to_composite_plus_fine_depths(golden, dev, nc, nf, drawn):
    """97 rays (not a multiple of the four rays of a workgroup) of the golden coarse field."""
    from nerf import _ops
    g = golden("render_d8w256_val")
    n = 97
    rf = G(g["rf_coarse"][:n, :nc], dev)
    rd = G(g["rd"][:n], dev)
    gen = torch.Generator().manual_seed(nc * 1000 + nf)
    if drawn:   # perturbed coarse depths (t_rand) and resampling draws (u)
        rays = torch.cat([G(g["ro"][:n], dev), rd, torch.full((n, 1), 2.0, device=dev), torch.full((n, 1), 6.0, device=dev)], -1)
        z = _ops.coarse_depths(rays, nc, False, torch.rand(n, nc, generator=gen).to(dev))
        u = torch.rand(n, nf, generator=gen).to(dev)
    else:
        z, u = G(g["z_coarse"][:n, :nc], dev), None
    with torch.no_grad():
        _, _, acc_ref, w_ref, depth_ref, _ = _ops.volume_render_fwd(rf, z, rd, None, 0.0, False, [])
        z_ref = _ops.fine_depths(z, w_ref, nf, u)
        depth, acc, z_fine = _ops.density_resample(rf, z, rd, nf, u=u)
    assert torch.equal(z_fine, z_ref)
    assert torch.equal(depth, depth_ref) and torch.equal(acc, acc_ref)
    if (nc, nf, drawn) == (64, 128, False):   # the golden's own configuration: wherever the existing pair reproduces it, so does this
        rows = (C(z_ref) == g["z_fine"][:n]).all(-1)
        print(f"rows on which the existing pair reproduces the golden z_fine: {rows.mean():.3f}")
        np.testing.assert_array_equal(C(z_fine)[rows], g["z_fine"][:n][rows])


@pytest.fixture(scope="module")
def composite_inputs(golden, dev):
    """Golden fine field of the D8 / W256 case (192 rays x 192 samples) with two edge rays planted, and its noise draws."""
    g = golden("render_d8w256_val")
    rf = g["rf_fine"].copy()
    rf[0, :, 3] = -1.0          # all sigma <= 0: every Dex row reads z[:, 0]
    rf[1, 0, 3] = 1.0e6         # sigma > every threshold at sample 0
    noise = torch.randn(rf.shape[:2], generator=torch.Generator().manual_seed(11))
    return G(rf, dev), G(g["z_fine"], dev), G(g["rd"], dev), noise.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [59, 64, 192])
@pytest.mark.parametrize("k", [0, 1, 20, 64])
def test_composite_density_is_bit_identical_to_volume_render(composite_inputs, dev, s, k):
    from nerf import _ops
    rf, z, rd, noise = composite_inputs
    rf, z, noise = rf[:, :s].contiguous(), z[:, :s].contiguous(), noise[:, :s].contiguous()
    thres = [5.0 * (i + 1) for i in range(k)]
    for nz, std in ((None, 0.0), (noise, 0.3)):
        with torch.no_grad():
            _, _, acc_ref, _, depth_ref, dex_ref = _ops.volume_render_fwd(rf, z, rd, nz, std, False, thres, want_weights=False)
            depth, acc, dex = _ops.composite_density(rf, z, rd, nz, std, thres)
        assert torch.equal(depth, depth_ref) and torch.equal(acc, acc_ref)
        if k == 0:
            assert dex is None
        else:
            assert torch.equal(dex, dex_ref)
            if std == 0.0:
                assert torch.equal(dex[:, 0], z[0, :1].expand(k)) and torch.equal(dex[:, 1], z[1, :1].expand(k))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [59, 192])
def test_composite_density_takes_a_hundred_thresholds(composite_inputs, dev, s):
    """m_thres: 500 gives K = 100 (thresholds 5 .. 500): each row is the row a K <= 64 call of the existing kernel gives."""
    from nerf import _ops
    rf, z, rd, noise = composite_inputs
    rf, z, noise = rf[:, :s].contiguous(), z[:, :s].contiguous(), noise[:, :s].contiguous()
    thres = [float(m) for m in range(5, 505, 5)]
    assert len(thres) == 100
    for nz, std in ((None, 0.0), (noise, 0.3)):
        with torch.no_grad():
            ref = torch.cat([_ops.volume_render_fwd(rf, z, rd, nz, std, False, part, want_weights=False)[5]
                             for part in (thres[:64], thres[64:])], 0)
            depth, acc, dex = _ops.composite_density(rf, z, rd, nz, std, thres)
        assert dex.shape == (100, rf.shape[0]) and torch.equal(dex, ref)
        if std == 0.0:
            sig_max = torch.relu(rf[..., 3]).max(-1)[0]
            never = sig_max[None, :] <= torch.tensor(thres, device=dev)[:, None]      # no sigma exceeds the threshold
            assert bool(never.any()) and torch.equal(dex[never], z[:, 0][None, :].expand(100, -1)[never])


FP32_CASES = ["render_lego_val", "render_lego_val_64_128", "render_d8w256_val", "render_d8w256_lindisp"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FP32_CASES)
def test_render_dex_depth_fp32_against_goldens_and_the_full_render(golden, dev, name):
    from nerf import _ops
    g = golden(name)
    n = len(g["ro"])
    out = depth_render(name, g, dev)
    assert len(out) == 4 + len(M_THRES) and all(o.shape == (1, n) for o in out)
    for label, o in zip(("depth_coarse", "acc_coarse", "depth_fine", "acc_fine"), out[:4]):
        err = rel_err(C(o).reshape(-1), g["out_" + label])
        print(f"{name}: {label} rel err {err:.2e}")
        assert err < TOL, label
    dex = np.stack([C(o).reshape(-1) for o in out[4:]])
    frac = dex_agreement(dex, g["out_dex_fine"])
    print(f"{name}: Dex agreement with the golden {frac:.4f}")
    assert frac > DEX_AGREE_FP32
    # against the library's own full fp32 render of the same rays
    full = full_render(name, g, dev)
    full_maps = [full[1], full[2], full[4], full[5]] + list(full[6:])
    sig_full, sig_dens = sigma_pair(name, g, dev)
    if torch.equal(sig_full[..., 3], sig_dens[..., 3]):
        for a, b in zip(out, full_maps):
            assert torch.equal(a, b)
        return
    # sigma differs in the last bits: the 1e-4 rule on the rays whose fine depths agree, at most 1 % of the rays left out
    mc = models_of(name, dev)[0]
    rkw = CASES[name][2]
    rays = _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), G(g["rd"], dev), rkw["near"], rkw["far"])
    with torch.no_grad():
        z = _ops.coarse_depths(rays, rkw["num_coarse"], rkw.get("lindisp", False))
        w_full = _ops.volume_render_fwd(_ops.run_network_rays(mc.packed(), rays, z), z, rays[:, 3:6], None, 0.0, False, [])[3]
        z_full = _ops.fine_depths(z, w_full, rkw["num_fine"])
        z_dens = _ops.density_resample(_ops.run_network_rays(mc.packed_density(), rays[:, :8].contiguous(), z), z, rays[:, 3:6],
                                       rkw["num_fine"])[2]
    same = C((z_full == z_dens).all(-1))
    print(f"{name}: rays whose fine depths differ between the two renders: {1.0 - same.mean():.4f}")
    assert 1.0 - same.mean() <= 0.01
    for a, b in zip(out[:4], full_maps[:4]):
        assert rel_err(C(a).reshape(-1)[same], C(b).reshape(-1)[same]) < TOL
    assert dex_agreement(dex[:, same], np.stack([C(o).reshape(-1) for o in full_maps[4:]])[:, same]) > DEX_AGREE_FP32


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_render_dex_depth_16bit_against_the_golden(golden, dev, precision):
    import nerf
    name = "render_d8w256_val"
    g = golden(name)
    depth_floor, dex_floor = FLOORS_16[precision]
    nerf.set_precision(precision)
    out = depth_render(name, g, dev)
    depth_psnr = psnr_db(C(out[2]).reshape(-1), g["out_depth_fine"], peak=4.0)
    frac = dex_agreement(np.stack([C(o).reshape(-1) for o in out[4:]]), g["out_dex_fine"])
    print(f"{precision} depth-only D8/W256 64+128 vs golden: depth {depth_psnr:.1f} dB, Dex agreement {frac:.4f}")
    assert depth_psnr > depth_floor and frac > dex_floor


@pytest.mark.gpu
def test_bf16_mode_renders_depth_in_guarded_fp16_by_default(golden, dev):
    """Under 'bf16' with the default policy the depth render runs the fp16 instances (equal to the 'fp16' mode bit for bit, unlike
    pure bf16); weights that push a hidden activation past 65504 trip status word 1: one warning, the bf16 render instead."""
    import nerf
    from nerf import _hip, _ops, train_utils
    name = "render_d8w256_val"
    g = golden(name)
    lib = _hip.lib()
    for kw in (D8, D4):
        assert lib.dn_fp16_range_guard(ctypes.byref(density_desc(_hip, kw))) == 1
    mc, mf = models_of(name, dev)
    assert _ops.fp16_range_guard(mc, density=True) and _ops.fp16_range_guard(mf, density=True)
    nerf.set_precision("fp16")
    ref16 = depth_render(name, g, dev)
    nerf.set_precision("bf16")
    nerf.set_render_policy("bf16")
    pure = depth_render(name, g, dev)
    nerf.set_render_policy("fp16")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pol = depth_render(name, g, dev)
    assert all(torch.equal(a, b) for a, b in zip(pol, ref16))
    assert not torch.equal(pol[2], pure[2])
    saved = mf.layers_xyz[2].weight.detach().clone()
    try:
        with torch.no_grad():
            mf.layers_xyz[2].weight.mul_(3.0e4)   # the existing overflow fixture's scale: outputs ~1e5, beyond fp16, nothing for bf16
        nerf.models.mark_parameters_updated()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            guarded = depth_render(name, g, dev)
            again = depth_render(name, g, dev)
        assert sum("fp16 render produced non-finite" in str(w.message) for w in caught) == 1
        assert train_utils._FP16_RENDER_DISABLED[0]
        nerf.set_render_policy("bf16")
        pure_big = depth_render(name, g, dev)
        for a, b, c in zip(guarded, pure_big, again):
            assert torch.equal(a, b) and torch.equal(c, b)
        assert bool(torch.isfinite(guarded[2]).all())
    finally:
        with torch.no_grad():
            mf.layers_xyz[2].weight.copy_(saved)
        nerf.models.mark_parameters_updated()
        train_utils._FP16_RENDER_DISABLED[0] = False


def _routing_outputs(path):
    """Density packs of both fixed shapes, both 16-bit precisions, both input forms, one point .. more tiles than workgroups:
    the raw fields, saved to `path` (run in the parent and, with DEXNERF_G48_RUNTIME_SHAPE=1, in a fresh child)."""
    import nerf
    from nerf import _ops, synthetic as syn
    dev = torch.device("cuda:0")
    out = {}
    gen = torch.Generator().manual_seed(9)
    for prec in ("bf16", "fp16"):
        nerf.set_precision(prec)
        for (depth, width) in ((8, 256), (4, 128)):
            kw = dict(num_layers=depth, hidden_size=width, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4,
                      use_viewdirs=True)
            m = nerf.models.FlexibleNeRFModel(**kw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(7 + depth, sigma_gain=5.0, sigma_bias=0.0, **kw).items()})
            pk = m.to(dev).packed_density()
            for n_rays, s in ((1, 1), (1, 385), (77, 5), (1100, 100)):   # 1100 x 100 = 287 tiles of 384 points > 256 workgroups
                pts = torch.randn(n_rays, s, 3, generator=gen).to(dev)
                rays = torch.cat([torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen), torch.zeros(n_rays, 2)], -1).to(dev)
                z = torch.sort(torch.rand(n_rays, s, generator=gen) * 4 + 2, -1)[0].to(dev).contiguous()
                with torch.no_grad():
                    out[f"{prec}_{width}_{n_rays}_{s}_pts"] = C(_ops.run_network_pts(pk, pts.reshape(-1, 3), None, s))
                    out[f"{prec}_{width}_{n_rays}_{s}_rays"] = C(_ops.run_network_rays(pk, rays, z))
    nerf.set_precision("fp32")
    np.savez(path, **out)


@pytest.mark.gpu
def test_fixed_density_instances_equal_the_runtime_shape_kernel_bit_for_bit(dev, tmp_path):
    fixed_path, runtime_path = str(tmp_path / "fixed.npz"), str(tmp_path / "runtime.npz")
    _routing_outputs(fixed_path)
    env = dict(os.environ, DEXNERF_G48_RUNTIME_SHAPE="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(REPO, 'tests')!r}); import test_depth_render as t; t._routing_outputs({runtime_path!r})"
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
    fixed, runtime = np.load(fixed_path), np.load(runtime_path)
    assert sorted(fixed.files) == sorted(runtime.files) and len(fixed.files) == 32
    for key in fixed.files:
        assert np.isfinite(fixed[key]).all() and np.array_equal(fixed[key], runtime[key]), key
        assert not fixed[key][..., :3].any(), key


@pytest.mark.gpu
def test_packed_density_follows_parameter_updates(dev):
    import nerf
    from nerf import _ops, synthetic as syn
    m = nerf.models.FlexibleNeRFModel(**D4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(5, **D4).items()})
    m = m.to(dev)
    pts = torch.randn(300, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(300, 3, generator=torch.Generator().manual_seed(2)), dim=-1).to(dev)

    def sigma():
        with torch.no_grad():
            return _ops.run_network_pts(m.packed_density(), pts, None, 1)[:, 3].clone()
    s0 = sigma()
    pk = m.packed_density()
    assert pk is m.packed_density() and pk is not m.packed() and pk.desc.use_viewdirs == 0   # its own cache, nothing re-packed
    with torch.no_grad():
        full0 = _ops.run_network_pts(m.packed(), pts, vd, 1)
    assert rel_err(C(s0), C(full0[:, 3])) < TOL
    with torch.no_grad():
        m.fc_alpha.bias.add_(1.0)                  # an ordinary in-place update: the tensor version changes
    s1 = sigma()
    assert float((s1 - (s0 + 1.0)).abs().max()) < 1e-4 * float(s0.abs().max() + 1.0)
    m.fc_alpha.bias.data.add_(1.0)                 # behind PyTorch's back (no version bump): what a graph replay does
    nerf.models.mark_parameters_updated()
    s2 = sigma()
    assert float((s2 - (s0 + 2.0)).abs().max()) < 1e-4 * float(s0.abs().max() + 2.0)
    opt = torch.optim.SGD(m.parameters(), lr=1.0)  # any optimizer step
    m.fc_alpha.bias.grad = torch.ones_like(m.fc_alpha.bias)
    opt.step()
    s3 = sigma()
    assert float((s3 - (s0 + 1.0)).abs().max()) < 1e-4 * float(s0.abs().max() + 1.0)


@pytest.mark.gpu
def test_render_dex_depth_consumes_the_generator_like_a_full_render(golden, dev):
    name = "render_lego_val"
    g = golden(name)
    cfg = make_cfg(CASES[name][2], chunksize=100, perturb=True, radiance_field_noise_std=0.1)   # 256 rays: three chunks
    rays = (G(g["ro"], dev), G(g["rd"], dev))
    torch.manual_seed(5)
    full = full_render(name, g, dev, mode="train", cfg=cfg, rays=rays)
    state_full = torch.cuda.get_rng_state(dev)
    torch.manual_seed(5)
    out = depth_render(name, g, dev, mode="train", cfg=cfg, rays=rays)
    state_depth = torch.cuda.get_rng_state(dev)
    assert torch.equal(state_full, state_depth)
    assert all(o.shape == (256,) for o in out)
    assert rel_err(C(out[0]), C(full[1])) < TOL and rel_err(C(out[1]), C(full[2])) < TOL   # the same draws reached the same places


@pytest.mark.gpu
def test_render_dex_depth_coarse_only_ndc_and_many_thresholds(golden, dev):
    """num_fine == 0 returns Nones and the coarse Dex list; NDC rays follow run_one_iter_of_nerf; K = 100 thresholds render."""
    name = "render_lego_val"
    g = golden(name)
    rkw = dict(CASES[name][2], num_fine=0)
    out = depth_render(name, g, dev, cfg=make_cfg(rkw))
    full = full_render(name, g, dev, cfg=make_cfg(rkw))
    assert out[2] is None and out[3] is None and len(out) == 4 + len(M_THRES)
    assert rel_err(C(out[0]), C(full[1])) < TOL and rel_err(C(out[1]), C(full[2])) < TOL
    assert dex_agreement(np.stack([C(o).reshape(-1) for o in out[4:]]), np.stack([C(o).reshape(-1) for o in full[6:]])) > DEX_AGREE_FP32
    # forward-facing rays in NDC (near plane 1): directions with z < 0
    gen = torch.Generator().manual_seed(4)
    ro = torch.cat([torch.rand(1, 90, 2, generator=gen) - 0.5, torch.zeros(1, 90, 1)], -1).to(dev)
    rd = torch.cat([0.4 * (torch.rand(1, 90, 2, generator=gen) - 0.5), -torch.ones(1, 90, 1)], -1).to(dev)
    ndc = dict(CASES[name][2], near=0.0, far=1.0)
    out = depth_render(name, g, dev, cfg=make_cfg(ndc, no_ndc=False), rays=(ro, rd))
    full = full_render(name, g, dev, cfg=make_cfg(ndc, no_ndc=False), rays=(ro, rd))
    for a, b in zip(out[:4], (full[1], full[2], full[4], full[5])):
        assert a.shape == (1, 90) and rel_err(C(a), C(b)) < TOL
    many = [float(m) for m in range(5, 505, 5)]
    out100 = depth_render(name, g, dev, thres=many)
    out20 = depth_render(name, g, dev)
    assert len(out100) == 104
    for k in range(20):
        assert torch.equal(out100[4 + k], out20[4 + k])


@pytest.mark.gpu
def test_render_dex_depth_refuses_what_it_does_not_cover(golden, dev):
    import nerf
    name = "render_lego_val"
    g = golden(name)
    mc, mf = models_of(name, dev)
    ex, ed = embedders()
    cfg = make_cfg(CASES[name][2])
    ro, rd = G(g["ro"], dev)[None], G(g["rd"], dev)[None]

    def call(mc=mc, mf=mf, ro=ro, rd=rd):
        return nerf.render_dex_depth(1, ro.shape[1], 1.0, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                     encode_direction_fn=ed, m_thres_cand=list(M_THRES))
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            call(ro=ro.cpu(), rd=rd.cpu())                      # host tensors
        small = nerf.models.FlexibleNeRFModel(**dict(D4, hidden_size=64)).to(dev)
        assert not small.fused_ok()
        with pytest.raises(RuntimeError):
            call(mc=small, mf=small)                            # outside fused_ok(): no fallback
    with pytest.raises(RuntimeError, match="no-grad"):
        call()                                                  # autograd enabled, parameters require grad
    with torch.no_grad():
        assert len(call()) == 4 + len(M_THRES)


@pytest.mark.gpu
def test_eval_driver_depth_only(dev, tmp_path):
    """eval_nerf.py --depth-only: requires --m-thres, writes the depth / Dex maps, no RGB PNG; the maps are the full eval's."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "2", "--num-fine", "64", "--precision", "fp32", "--quiet"]
    with pytest.raises(SystemExit):
        eval_nerf.main(common + ["--depth-only"])
    out = tmp_path / "out"
    res = eval_nerf.main(common + ["--depth-only", "--m-thres", "20", "--savedir", str(out)])
    full = eval_nerf.main(common + ["--m-thres", "20"])
    names = sorted(p.name for p in out.iterdir())
    assert names == ["depth_0000.png", "depth_0001.png", "dex_0000.npz", "dex_0001.npz"]
    maps = np.load(out / "dex_0001.npz")
    assert maps["dex"].shape == (4, 24, 24) and list(maps["m_thres"]) == [5.0, 10.0, 15.0, 20.0]
    for (rgb, depth, dex), (_, depth_full) in zip(res["frames"], full["frames"]):
        assert rgb is None and depth.shape == (24, 24) and len(dex) == 4
        assert rel_err(C(depth), C(depth_full)) < TOL


@pytest.mark.gpu
def test_depth_render_is_hipgraph_capturable(golden, dev):
    """dn_render_rays_depth neither allocates nor synchronises: a captured chunk replays to the eager outputs bit for bit."""
    from nerf import _ops
    name = "render_lego_val"
    g = golden(name)
    mc, mf = models_of(name, dev)
    rays = _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), None, 2.0, 6.0)
    pc, pf = mc.packed_density(), mf.packed_density()
    thres = torch.tensor([5.0, 10.0], device=dev)
    eager = _ops.render_rays_depth(pc, pf, rays, 64, 64, False, 0.0, thres)   # also warms up (the per-stream workspace record)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _ops.render_rays_depth(pc, pf, rays, 64, 64, False, 0.0, thres)      # workspace for this stream
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = _ops.render_rays_depth(pc, pf, rays, 64, 64, False, 0.0, thres)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
