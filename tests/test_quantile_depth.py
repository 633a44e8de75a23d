"""Opacity-quantile (median) depth maps (include/dexnerf_hip_quantile.h): dn_composite_density_quantiles, dn_render_rays_depth_quantiles,
nerf.render_dex_depth(quantiles=...), the driver flags.

The definition is restated below in float64 numpy (`quantile_restatement`): C = cumsum of the fp32 weights in float64, the crossing
index i(q) = the first s with C_s >= q (or -1), sample mode z_i, linear mode z_i + (z_{i+1} - z_i) (q - C_{i-1}) / w_i, z_{S-1} for the last
sample and for rays that never cross.  Gates:
  * sample mode is INDEX work: equal to the restatement on the kernel's own fp32 weights for every (ray, q) whose restated
    min_s |C_s - q| >= 1e-9 (the kernel's fp64 scan adds in another order, about 1e-16); at most 1 % of the pairs may be left out;
  * linear mode against the restatement on the same pairs at 1e-5 max|z|, the project's gate for a kernel against float64 (the
    margin keeps w_i >= 1e-9 at the crossing, so the quotient is conditioned);
  * depth / acc / dex are dn_composite_density's bits;
  * the fp32 render against the restatement on the golden field at 1e-4 max|z| (the fp32-mode gate), on rays with |acc - q| >= 1e-3,
    at most 2 % of the rays left out.
Planted rays have closed forms and need no oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import CASES, D8, M_THRES, lego_weights

QUANTILE = ("dn_composite_density_quantiles", "dn_render_rays_depth_quantiles")
INVAL = -1000
MARGIN = 1e-9
Q3 = (0.1, 0.5, 0.9)


def quantile_restatement(w, z, q, interp):
    """float64 restatement of the definition.  w, z: (N,S); q: (Q,) -> (idx (Q,N) int, depth (Q,N) float64, margin (Q,N))."""
    w64, z64 = np.asarray(w, np.float64), np.asarray(z, np.float64)
    q64 = np.asarray(q, np.float32).astype(np.float64)          # the kernel compares against (double) of the fp32 quantile
    n, s = w64.shape
    c = np.cumsum(w64, axis=-1)
    hit = c[None] >= q64[:, None, None]                          # (Q,N,S)
    idx = np.where(hit.any(-1), hit.argmax(-1), -1)
    i = np.where(idx < 0, s - 1, idx)
    rows = np.arange(n)[None, :]
    zi = z64[rows, i]
    depth = zi.copy()
    if interp:
        inner = (idx >= 0) & (idx < s - 1)
        zn = z64[rows, np.minimum(i + 1, s - 1)]
        cprev = np.where(i > 0, c[rows, np.maximum(i - 1, 0)], 0.0)
        wi = w64[rows, i]
        lin = zi + (zn - zi) * (q64[:, None] - cprev) / np.where(inner, wi, 1.0)
        depth = np.where(inner, lin, zi)
    margin = np.abs(c[None] - q64[:, None, None]).min(-1)
    return idx, depth, margin


def weights_float64(rf, z, rd):
    """The compositing weights of a raw field in float64 (no noise): relu, dists (last 1e10) * |rd|, alpha, exclusive cumprod."""
    sigma = np.maximum(np.asarray(rf, np.float64)[..., 3], 0.0)
    z64 = np.asarray(z, np.float64)
    dists = np.concatenate([z64[:, 1:] - z64[:, :-1], np.full((len(z64), 1), 1e10)], -1) * np.linalg.norm(np.asarray(rd, np.float64), axis=-1)[:, None]
    alpha = 1.0 - np.exp(-sigma * dists)
    trans = np.cumprod(1.0 - alpha + 1e-10, axis=-1)
    trans = np.concatenate([np.ones((len(z64), 1)), trans[:, :-1]], -1)
    return alpha * trans


def q_spread(n):
    return [0.5] if n == 1 else [float(x) for x in np.linspace(0.01, 0.999, n)]


def full_desc(_hip, kw, viewdirs=1):
    return _hip.MlpDesc(kw["num_layers"], kw["hidden_size"], kw["skip_connect_every"], kw["num_encoding_fn_xyz"],
                        kw["num_encoding_fn_dir"], 1, 1, viewdirs, 1, 1)


def density_desc(_hip, kw):
    out = _hip.MlpDesc()
    assert _hip.lib().dn_mlp_density_desc(ctypes.byref(full_desc(_hip, kw)), ctypes.byref(out)) == 0
    return out


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_quantile_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    names = lambda name: set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", open(os.path.join(REPO, "include", name)).read()))  # noqa: E731
    assert names("dexnerf_hip_quantile.h") == set(_hip.QUANTILE_EXPORTS) == set(QUANTILE)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS))
    assert not older & set(QUANTILE)
    assert "dexnerf_hip_quantile.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()     # build() checks the new header's symbols too
    assert "composite_quantile.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in QUANTILE) and hiplib.dn_abi_version() == 2
    assert "#define DN_MAX_QUANTILES 64" in open(os.path.join(REPO, "include", "dexnerf_hip_quantile.h")).read() and _hip.MAX_QUANTILES == 64


def test_quantile_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    from nerf import _hip
    fake = ctypes.c_void_p(256 * 4096)
    dd, with_dirs = density_desc(_hip, D8), full_desc(_hip, D8)
    defaults = dict(desc_c=ctypes.byref(dd), packed_c=fake, desc_f=ctypes.byref(dd), packed_f=fake, prec=_hip.PREC_F32, rays=fake, stride=8, n=8,
                    nc=16, nf=24, lindisp=0, std=0.0, thres=fake, k=3, t_rand=None, noise_c=None, u=None, noise_f=None, depth_c=fake,
                    acc_c=fake, depth_f=fake, acc_f=fake, dex=fake, quant=fake, nq=3, interp=0, qdepth=fake, ws=fake, stream=None)
    call = lambda **kw: hiplib.dn_render_rays_depth_quantiles(*{**defaults, **kw}.values())  # noqa: E731
    for kw in (dict(qdepth=None), dict(quant=None),                               # quantiles without their input / output
               dict(nq=65), dict(nq=-1), dict(interp=2), dict(interp=-1),
               # dn_render_rays_depth's own refusals
               dict(desc_c=None), dict(packed_c=None), dict(rays=None), dict(ws=None), dict(n=-1), dict(desc_f=None), dict(packed_f=None),
               dict(ws=ctypes.c_void_p(256 * 4096 + 16)), dict(desc_f=ctypes.byref(with_dirs)), dict(desc_c=ctypes.byref(with_dirs)),
               dict(nc=9), dict(nc=513), dict(nc=512, nf=1537), dict(nc=0), dict(nf=-1), dict(stride=7), dict(k=-1), dict(thres=None),
               dict(dex=None)):
        assert call(**kw) == INVAL, kw
        assert b"dn_render_rays_depth_quantiles" in hiplib.dn_last_error(), kw
    w64 = density_desc(_hip, dict(D8, hidden_size=64))
    assert call(desc_c=ctypes.byref(w64)) == -1001                                 # unsupported width, as in dn_render_rays_depth
    assert call(n=0) == 0 and call(n=0, nq=64) == 0 and call(n=0, nq=0, quant=None, qdepth=None) == 0   # valid no-ops
    assert call(n=0, interp=1, k=0, thres=None, dex=None) == 0

    comp = dict(rf=fake, z=fake, rd=fake, rd_stride=3, noise=None, std=0.0, thres=fake, k=2, quant=fake, nq=3, interp=1, n=4, s=8, depth=fake,
                acc=fake, dex=fake, qdepth=fake, stream=None)
    ccall = lambda **kw: hiplib.dn_composite_density_quantiles(*{**comp, **kw}.values())  # noqa: E731
    for kw in (dict(qdepth=None), dict(quant=None), dict(nq=65), dict(nq=-1), dict(interp=2),
               dict(rf=None), dict(z=None), dict(rd=None), dict(s=0), dict(n=-1), dict(rd_stride=2), dict(k=-1), dict(thres=None), dict(dex=None),
               dict(rf=ctypes.c_void_p(256 * 4096 + 4))):
        assert ccall(**kw) == INVAL, kw
        assert b"dn_composite_density_quantiles" in hiplib.dn_last_error(), kw
    assert ccall(n=0) == 0


@pytest.mark.parametrize("name", ["render_d8w256_val", "render_lego_val"])
def test_definition_on_the_goldens_own_weights(golden, name):
    """The restated definition on the reference-recorded fine weights: the nerfstudio statement (searchsorted of the cumulative
    weights, clamped), monotone in q, the linear mode inside the crossing interval."""
    g = golden(name)
    w, z = g["vf_weights"], g["z_fine"]
    n, s = w.shape
    q = q_spread(64)
    idx, sample, _ = quantile_restatement(w, z, q, False)
    _, linear, _ = quantile_restatement(w, z, q, True)
    c = np.cumsum(w.astype(np.float64), -1)
    q64 = np.asarray(q, np.float32).astype(np.float64)
    for k in range(len(q)):
        ss = np.array([np.searchsorted(c[r], q64[k], side="left") for r in range(n)])
        np.testing.assert_array_equal(np.minimum(ss, s - 1), np.where(idx[k] < 0, s - 1, idx[k]))
        np.testing.assert_array_equal(ss == s, idx[k] < 0)
    i = np.where(idx < 0, s - 1, idx)
    assert (np.diff(i, axis=0) >= 0).all() and (np.diff(sample, axis=0) >= 0).all() and (np.diff(linear, axis=0) >= 0).all()
    rows = np.arange(n)[None, :]
    lo, hi = z.astype(np.float64)[rows, i], z.astype(np.float64)[rows, np.minimum(i + 1, s - 1)]
    assert (linear >= lo).all() and (linear <= hi).all()
    np.testing.assert_array_equal(sample, lo)
    crossed = (idx >= 0).mean(-1)
    assert 0.0 < crossed.min() and crossed.max() < 1.0             # both branches populated at every q


@pytest.mark.parametrize("bad", [[0.0], [1.0], [float("nan")], [float("inf")], [-0.1], [0.5, 1.5], [0.5] * 65, [0.99999999]])
def test_quantiles_are_validated_on_the_host(bad):
    """0, 1, NaN, out-of-range and 65 values raise ValueError before anything touches a device (0.99999999 is 1 in fp32)."""
    import eval_nerf
    import nerf
    import train_dexnerf
    from nerf import _ops
    with pytest.raises(ValueError):
        _ops.check_quantiles(bad)
    with pytest.raises(ValueError):   # host tensors, no models: the quantiles are judged first
        nerf.render_dex_depth(1, 4, 1.0, None, None, torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), None, quantiles=bad)
    text = ",".join(repr(float(q)) for q in bad)
    with pytest.raises(SystemExit):
        eval_nerf.main(["--checkpoint", "none.ckpt", "--depth-only", "--depth-quantiles", text])
    with pytest.raises(SystemExit):
        train_dexnerf.parse_args(["--val-quantiles", text])


def test_quantile_flags_parse_and_default_to_off():
    import eval_nerf
    import train_dexnerf
    from nerf import _ops
    assert train_dexnerf.parse_args([]).val_quantiles == []
    assert train_dexnerf.parse_args(["--val-quantiles", "0.1,0.5,0.9"]).val_quantiles == _ops.check_quantiles(Q3)
    assert _ops.check_quantiles([0.5, 0.25]) == [0.5, 0.25] and len(_ops.check_quantiles([0.5] * 64)) == 64
    for argv in (["--depth-only"], ["--depth-quantiles", "0.5"], ["--depth-only", "--m-thres", "20", "--quantile-interp"]):
        with pytest.raises(SystemExit):   # --depth-only needs thresholds or quantiles; the quantile flags belong to --depth-only
            eval_nerf.main(["--checkpoint", "none.ckpt"] + argv)


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
    from nerf import train_utils
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")
    train_utils._FP16_RENDER_DISABLED[0] = False


def G(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def composite_inputs(golden, dev):
    """tests/test_depth_render.py's recipe: the golden fine field of the D8 / W256 case (192 rays x 192 samples) with two edge rays
    planted, and its noise draws."""
    g = golden("render_d8w256_val")
    rf = g["rf_fine"].copy()
    rf[0, :, 3] = -1.0
    rf[1, 0, 3] = 1.0e6
    noise = torch.randn(rf.shape[:2], generator=torch.Generator().manual_seed(11))
    return G(rf, dev), G(g["z_fine"], dev), G(g["rd"], dev), noise.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("s", [1, 59, 64, 65, 192])
def test_quantile_kernel_against_the_restatement_and_composite_density(composite_inputs, dev, s, noisy):
    from nerf import _ops
    rf, z, rd, noise = composite_inputs
    rf, z, noise = rf[:, :s].contiguous(), z[:, :s].contiguous(), noise[:, :s].contiguous()
    nz, std = (noise, 0.3) if noisy else (None, 0.0)
    with torch.no_grad():
        w = C(_ops.volume_render_fwd(rf, z, rd, nz, std, False, [], want_weights=True)[3])   # the existing kernel's fp32 weights
    zc = C(z)
    z_max = float(np.abs(zc).max())
    worst = 0.0
    for nq in (1, 3, 64):
        q = q_spread(nq)
        ref = {interp: quantile_restatement(w, zc, q, interp) for interp in (False, True)}
        idx, _, margin = ref[False]
        keep = margin >= MARGIN
        print(f"S={s} noise={noisy} Q={nq}: pairs left out {(~keep).mean():.4f}, smallest margin {margin.min():.2e}, "
              f"rays crossing {(idx >= 0).mean(-1).min():.2f}..{(idx >= 0).mean(-1).max():.2f}, deepest crossing {idx.max()}")
        assert (~keep).mean() <= 0.01
        if s == 192 and nq == 64:   # both branches and all three chunks are populated
            assert (idx >= 0).any() and (idx < 0).any() and idx.max() >= 128 and ((idx >= 64) & (idx < 128)).any() and ((idx >= 0) & (idx < 64)).any()
        for k in (0, 20, 100):
            thres = [5.0 * (i + 1) for i in range(k)]
            with torch.no_grad():
                depth0, acc0, dex0 = _ops.composite_density(rf, z, rd, nz, std, thres)
            for interp in (False, True):
                with torch.no_grad():
                    depth, acc, dex, qd = _ops.composite_density_quantiles(rf, z, rd, nz, std, thres, q, interp=interp)
                assert torch.equal(depth, depth0) and torch.equal(acc, acc0)
                assert (dex is None and dex0 is None) if k == 0 else torch.equal(dex, dex0)
                assert qd.shape == (nq, rf.shape[0])
                got, want = C(qd), ref[interp][1]
                if not interp:
                    assert np.array_equal(got[keep], want.astype(np.float32)[keep])      # index work: exact
                else:
                    err = float(np.abs(got.astype(np.float64) - want)[keep].max()) / z_max
                    worst = max(worst, err)
                    assert err <= 1e-5, (nq, k, err)
    print(f"S={s} noise={noisy}: linear mode against the float64 restatement, worst max|diff| / max|z| = {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("s,n", [(65, 37), (192, 5)])
def test_planted_rays_have_closed_forms(dev, s, n):
    """Ray 0: raw sigma -1 everywhere -> z[S-1] in both modes.  Ray r >= 1: -1 everywhere but 1e6 at j -> w_j = 1 exactly, so i = j for
    every q: sample mode z_j, linear mode fp32(z_j + (z_{j+1} - z_j) q), z_{S-1} at the last sample.  j covers the first sample, the
    chunk edge 63 | 64 and the last sample; 37 rays leave the last workgroup partial."""
    from nerf import _ops
    gen = torch.Generator().manual_seed(s)
    plants = [None] + [(0, 63, 64, s - 1)[(r - 1) % 4] for r in range(1, n)]
    z = torch.linspace(2.0, 6.0, s)[None, :] + 0.01 * torch.rand(n, s, generator=gen)       # increasing: steps of >= 0.011
    rd = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1) * (0.5 + torch.rand(n, 1, generator=gen))
    rf = torch.randn(n, s, 4, generator=gen)
    rf[..., 3] = -1.0
    for r, j in enumerate(plants):
        if j is not None:
            rf[r, j, 3] = 1.0e6
    q = _ops.check_quantiles([0.01, 0.3, 0.5, 0.999])
    z64 = z.double().numpy()
    with torch.no_grad():
        depth0, acc0, dex0 = _ops.composite_density(rf.to(dev), z.to(dev), rd.to(dev), None, 0.0, [5.0, 50.0])
        for interp in (False, True):
            depth, acc, dex, qd = _ops.composite_density_quantiles(rf.to(dev), z.to(dev), rd.to(dev), None, 0.0, [5.0, 50.0], q, interp=interp)
            assert torch.equal(depth, depth0) and torch.equal(acc, acc0) and torch.equal(dex, dex0)
            qd = C(qd)
            for r, j in enumerate(plants):
                for k, qk in enumerate(q):
                    if j is None or j == s - 1 or not interp:
                        want = z[r, s - 1 if j is None else j].numpy()
                    else:
                        want = np.float32(z64[r, j] + (z64[r, j + 1] - z64[r, j]) * qk)
                    assert qd[k, r] == want, (interp, r, j, qk, qd[k, r], want)
    assert float(acc0[0]) == 0.0 and torch.equal(acc0[1:], torch.ones_like(acc0[1:]))


_MODELS = {}


def models_of(name, dev):
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


def depth_render(name, g, dev, cfg=None, rays=None, thres=M_THRES, mode="validation", **kw):
    import nerf
    mc, mf = models_of(name, dev)
    ex = nerf.get_embedding_function(10)
    ro, rd = (G(g["ro"], dev)[None], G(g["rd"], dev)[None]) if rays is None else rays
    with torch.no_grad():
        return nerf.render_dex_depth(1, ro.shape[-2], 1.0, mc, mf, ro, rd, cfg or make_cfg(CASES[name][2]), mode=mode,
                                     encode_position_fn=ex, m_thres_cand=None if thres is None else list(thres), **kw)


def monotone(maps):
    return all(bool((b >= a).all()) for a, b in zip(maps[:-1], maps[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["render_d8w256_val", "render_lego_val"])
def test_render_dex_depth_with_quantiles_fp32(golden, dev, name):
    g = golden(name)
    n, k = len(g["ro"]), len(M_THRES)
    plain = depth_render(name, g, dev)
    out = depth_render(name, g, dev, quantiles=Q3)
    lin = depth_render(name, g, dev, quantiles=Q3, quantile_interp=True)
    assert len(plain) == 4 + k and len(out) == len(lin) == 4 + k + 3 and all(o.shape == (1, n) for o in out)
    for a, b, c in zip(plain, out, lin):                             # the first 4 + K maps are the call's without quantiles
        assert torch.equal(a, b) and torch.equal(a, c)
    assert monotone(out[4 + k:]) and monotone(lin[4 + k:])
    several = depth_render(name, g, dev, cfg=make_cfg(CASES[name][2], chunksize=50), quantiles=Q3, quantile_interp=True)
    for a, b in zip(lin, several):                                   # independent of the chunking
        assert torch.equal(a, b)
    # linear mode against the float64 restatement on the golden field
    z = g["z_fine"]
    w = weights_float64(g["rf_fine"], z, g["rd"])
    _, want, _ = quantile_restatement(w, z, Q3, True)
    acc = w.sum(-1)
    keep = (np.abs(acc[None, :] - np.asarray(Q3)[:, None]) >= 1e-3).all(0)
    got = np.stack([C(m).reshape(-1) for m in lin[4 + k:]]).astype(np.float64)
    err = float(np.abs(got - want)[:, keep].max()) / float(np.abs(z).max())
    print(f"{name}: rays left out {int((~keep).sum())} of {n}; linear quantile depth against the float64 restatement on the golden "
          f"field: max|diff| / max|z| = {err:.3e}")
    assert (~keep).mean() <= 0.02 and err <= 1e-4


@pytest.mark.gpu
def test_quantiles_leave_the_draws_and_the_generator_alone(golden, dev):
    """Perturbed depths and density noise over three chunks: the maps before the quantile maps and the generator's final state are
    those of the call without quantiles."""
    name = "render_lego_val"
    g = golden(name)
    cfg = make_cfg(CASES[name][2], chunksize=100, perturb=True, radiance_field_noise_std=0.1)
    rays = (G(g["ro"], dev), G(g["rd"], dev))
    torch.manual_seed(5)
    plain = depth_render(name, g, dev, mode="train", cfg=cfg, rays=rays)
    state_plain = torch.cuda.get_rng_state(dev)
    torch.manual_seed(5)
    out = depth_render(name, g, dev, mode="train", cfg=cfg, rays=rays, quantiles=Q3)
    state_q = torch.cuda.get_rng_state(dev)
    assert torch.equal(state_plain, state_q)
    assert len(out) == len(plain) + 3 and all(torch.equal(a, b) for a, b in zip(plain, out))
    assert monotone(out[len(plain):])


@pytest.mark.gpu
def test_quantiles_in_bf16_mode_on_the_guarded_fp16_path(golden, dev):
    import nerf
    name = "render_d8w256_val"
    g = golden(name)
    nerf.set_precision("bf16")
    nerf.set_render_policy("fp16")
    for interp in (False, True):
        out = depth_render(name, g, dev, quantiles=Q3, quantile_interp=interp)
        qmaps = out[4 + len(M_THRES):]
        assert len(qmaps) == 3 and all(bool(torch.isfinite(m).all()) for m in qmaps) and monotone(qmaps)
        rkw = CASES[name][2]
        assert all(float(m.min()) >= rkw["near"] and float(m.max()) <= rkw["far"] for m in qmaps)   # inside the ray's sample range


@pytest.mark.gpu
def test_quantiles_coarse_only_and_ndc(golden, dev):
    name = "render_lego_val"
    g = golden(name)
    rkw = dict(CASES[name][2], num_fine=0)
    out = depth_render(name, g, dev, cfg=make_cfg(rkw), quantiles=Q3)
    plain = depth_render(name, g, dev, cfg=make_cfg(rkw))
    assert out[2] is None and out[3] is None and len(out) == 4 + len(M_THRES) + 3
    assert all(torch.equal(a, b) for a, b in zip(plain, out) if a is not None) and monotone(out[-3:])
    only_q = depth_render(name, g, dev, cfg=make_cfg(rkw), thres=None, quantiles=Q3)          # no Dex thresholds at all
    assert len(only_q) == 7 and all(torch.equal(a, b) for a, b in zip(only_q[4:], out[-3:]))
    gen = torch.Generator().manual_seed(4)
    ro = torch.cat([torch.rand(1, 90, 2, generator=gen) - 0.5, torch.zeros(1, 90, 1)], -1).to(dev)
    rd = torch.cat([0.4 * (torch.rand(1, 90, 2, generator=gen) - 0.5), -torch.ones(1, 90, 1)], -1).to(dev)
    ndc = dict(CASES[name][2], near=0.0, far=1.0)
    out = depth_render(name, g, dev, cfg=make_cfg(ndc, no_ndc=False), rays=(ro, rd), quantiles=Q3, quantile_interp=True)
    assert len(out) == 4 + len(M_THRES) + 3 and all(m.shape == (1, 90) for m in out[-3:]) and monotone(out[-3:])
    assert all(float(m.min()) >= 0.0 and float(m.max()) <= 1.0 for m in out[-3:])


@pytest.mark.gpu
def test_quantile_depth_render_is_hipgraph_capturable(golden, dev):
    """dn_render_rays_depth_quantiles neither allocates nor synchronises: a captured chunk replays to the eager outputs bit for bit."""
    from nerf import _ops
    name = "render_lego_val"
    g = golden(name)
    mc, mf = models_of(name, dev)
    rays = _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), None, 2.0, 6.0)
    pc, pf = mc.packed_density(), mf.packed_density()
    thres = torch.tensor([5.0, 10.0], device=dev)
    quant = torch.tensor(_ops.check_quantiles(Q3), device=dev)
    run = lambda: _ops.render_rays_depth(pc, pf, rays, 64, 64, False, 0.0, thres, quantiles=quant, interp=True)  # noqa: E731
    eager = run()
    assert len(eager) == 6 and eager[5].shape == (3, rays.shape[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                # workspace for this stream
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_eval_driver_depth_quantiles(dev, tmp_path):
    """eval_nerf.py --depth-only --depth-quantiles: runs without --m-thres and writes quantiles / qdepth into dex_<view>.npz."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "1", "--num-fine", "64", "--precision", "fp32", "--quiet", "--depth-only"]
    out = tmp_path / "out"
    eval_nerf.main(common + ["--depth-quantiles", "0.5", "--savedir", str(out)])
    maps = np.load(out / "dex_0000.npz")
    assert sorted(maps.files) == ["depth", "qdepth", "quantiles"] and maps["qdepth"].shape == (1, 24, 24) and list(maps["quantiles"]) == [0.5]
    both = tmp_path / "both"
    res = eval_nerf.main(common + ["--m-thres", "10", "--depth-quantiles", "0.1,0.9", "--quantile-interp", "--savedir", str(both)])
    maps2 = np.load(both / "dex_0000.npz")
    assert maps2["dex"].shape == (2, 24, 24) and maps2["qdepth"].shape == (2, 24, 24) and (maps2["qdepth"][1] >= maps2["qdepth"][0]).all()
    assert np.isfinite(maps["qdepth"]).all() and np.isfinite(maps2["qdepth"]).all()
    assert len(res["frames"][0]) == 4 and len(res["frames"][0][3]) == 2


@pytest.mark.gpu
def test_train_driver_val_quantiles(dev, capsys):
    """train_dexnerf.py --val-quantiles: the validation log and the result name the best quantile beside the best threshold; off by
    default: neither key nor text."""
    import nerf
    import train_dexnerf
    common = ["--iters", "12", "--size", "16", "--views", "3", "--num-random-rays", "128", "--layers", "4", "--width", "128", "--num-fine", "64",
              "--validate-every", "6", "--precision", "bf16", "--m-thres", "20"]
    try:
        plain = train_dexnerf.main(common)
        log_plain = capsys.readouterr().out
        res = train_dexnerf.main(common + ["--val-quantiles", "0.1,0.5,0.9"])
        log = capsys.readouterr().out
    finally:
        nerf.set_precision("fp32")
    assert "quantile" not in log_plain and "quantile_best" not in plain
    val_lines = [ln for ln in log.splitlines() if ln.startswith("[val]")]
    assert len(val_lines) == 2 and all("Dex best m=" in ln and "; quantile best q=" in ln for ln in val_lines)
    assert res["quantile_best"] in [float(np.float32(q)) for q in Q3] and np.isfinite(res["quantile_abs_err_mm"])
    assert res["dex_best_threshold"] == plain["dex_best_threshold"] and res["dex_abs_err_mm"] == plain["dex_abs_err_mm"]   # training untouched
