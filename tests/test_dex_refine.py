"""Sub-sample Dex depths (include/dexnerf_hip_refine.h): dn_composite_density_brackets, dn_dex_bisect, dn_dex_refine_finish,
dn_render_rays_depth_refined, nerf.render_dex_depth(refine_steps=...), the driver flags.

The header's definitions are restated below in numpy (`brackets_restatement`, `bisect_restatement`, `finish_restatement`): fp32 where
the header says fp32, float64 rounded once where it says so.  The three kernels are INDEX and SELECTION work plus one rounding each, so
they are compared bit for bit; the driver is compared bit for bit against a chain of the older entry points and the new standalone
ones.  The accuracy gate needs a truth: the first crossing among 513 dense evaluations of the CPU oracle inside each initial bracket,
interpolated; the GPU result may be worse than the same algorithm on the oracle network by the project's fp32-mode gate, 1e-4.
Planted records have closed forms and need no oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import CASES, D8, M_THRES, lego_weights

REFINE = ("dn_composite_density_brackets", "dn_dex_bisect", "dn_dex_refine_finish", "dn_render_depth_refined_workspace_bytes",
          "dn_render_rays_depth_refined")
INVAL = -1000
T3 = (5.0, 20.0, 60.0)
F32 = np.float32


# ---- the header's definitions in numpy ----------------------------------------------------------------------------------------------
def brackets_restatement(s, z, m):
    """s, z (N,S) fp32; m (K,) -> idx (N,K) int (-1: none), br (N,K,4) fp32, z_mid (N,K) fp32."""
    s, z, m = np.asarray(s, F32), np.asarray(z, F32), np.asarray(m, F32)
    n = len(s)
    with np.errstate(invalid="ignore"):
        hit = s[:, None, :] > m[None, :, None]                          # NaN never crosses, +inf does
    idx = np.where(hit.any(-1), hit.argmax(-1), -1)
    rows = np.arange(n)[:, None]
    hi, lo = np.maximum(idx, 0), np.maximum(idx - 1, 0)
    br = np.stack([z[rows, lo], z[rows, hi], s[rows, lo], s[rows, hi]], -1)
    none = idx < 0
    br[none, 2], br[none, 3] = F32(np.inf), F32(-np.inf)               # (z_0, z_0, +inf, -inf)
    return idx, br, midpoint(br)


def midpoint(br):
    with np.errstate(invalid="ignore"):
        return (br[..., 0] + F32(0.5) * (br[..., 1] - br[..., 0])).astype(F32)


def bisect_restatement(br, s_mid, m):
    """One step on br (N,K,4) with the densities s_mid (N,K) at the midpoints -> (br', z_mid')."""
    br = br.copy()
    zm = midpoint(br)
    live = br[..., 0] != br[..., 1]
    with np.errstate(invalid="ignore"):
        up = live & (s_mid > np.asarray(m, F32)[None, :])
    down = live & ~up                                                   # NaN included
    br[up, 1], br[up, 3] = zm[up], s_mid[up]
    br[down, 0], br[down, 2] = zm[down], s_mid[down]
    return br, midpoint(br)


def finish_restatement(br, m):
    """(refined (K,N) fp32, width (K,N) fp32) of br (N,K,4)."""
    b = br.astype(np.float64)
    m64 = np.asarray(m, F32).astype(np.float64)[None, :]
    lo, hi, s_lo, s_hi = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    none = br[..., 3] == F32(-np.inf)
    flat = br[..., 0] == br[..., 1]
    finite = np.isfinite(s_lo) & np.isfinite(s_hi)
    with np.errstate(all="ignore"):
        t = np.where(finite, (m64 - s_lo) / (s_hi - s_lo), 0.5)
        refined = np.where(none | flat, lo, lo + (hi - lo) * t).astype(F32)   # rounded once
        width = np.where(none, F32(-1.0), np.where(flat, F32(0.0), br[..., 1] - br[..., 0])).astype(F32)
    return refined.T.copy(), width.T.copy()


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


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


def make_cfg(rkw, chunksize=4096, **over):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=rkw.get("lindisp", False), num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"],
                perturb=rkw.get("perturb", False), radiance_field_noise_std=rkw.get("noise_std", 0.0),
                white_background=rkw.get("white_background", False))
    mode.update(over)
    return nerf.CfgNode(dict(dataset=dict(near=rkw["near"], far=rkw["far"], no_ndc=True),
                             nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_refine_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_refine.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.REFINE_EXPORTS) == set(REFINE)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS) | set(_hip.OCCUPANCY_EXPORTS) | set(_hip.CULL_EXPORTS))
    assert not older & set(REFINE)
    assert hiplib.dn_abi_version() == 2 and len(_hip.EXPORTS) == 76
    assert "dexnerf_hip_refine.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()       # build() checks the new header's symbols too
    assert "dex_refine.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in REFINE)
    assert "#define DN_MAX_REFINE_STEPS 24" in text and _hip.MAX_REFINE_STEPS == 24
    assert "need not be the first crossing" in text                       # the header says what the refinement does not promise


def test_refine_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    from nerf import _hip
    fake = ctypes.c_void_p(256 * 4096)
    odd = ctypes.c_void_p(256 * 4096 + 4)
    dd, with_dirs = density_desc(_hip, D8), full_desc(_hip, D8)
    defaults = dict(desc_c=ctypes.byref(dd), packed_c=fake, desc_f=ctypes.byref(dd), packed_f=fake, prec=_hip.PREC_F32, rays=fake, stride=8, n=8,
                    nc=16, nf=24, lindisp=0, std=0.0, thres=fake, k=3, t_rand=None, noise_c=None, u=None, noise_f=None, depth_c=fake,
                    acc_c=fake, depth_f=fake, acc_f=fake, dex=fake, steps=4, refined=fake, width=fake, ws=fake, stream=None)
    call = lambda **kw: hiplib.dn_render_rays_depth_refined(*{**defaults, **kw}.values())  # noqa: E731
    for kw in (dict(k=0), dict(k=0, thres=None, dex=None), dict(steps=-1), dict(steps=25), dict(std=0.1), dict(std=-0.1), dict(std=float("nan")),
               dict(refined=None), dict(n=2 ** 31, k=2),
               # dn_render_rays_depth's own refusals
               dict(desc_c=None), dict(packed_c=None), dict(rays=None), dict(ws=None), dict(n=-1), dict(desc_f=None), dict(packed_f=None),
               dict(ws=ctypes.c_void_p(256 * 4096 + 16)), dict(desc_f=ctypes.byref(with_dirs)), dict(desc_c=ctypes.byref(with_dirs)),
               dict(nc=9), dict(nc=513), dict(nc=512, nf=1537), dict(nc=0), dict(nf=-1), dict(stride=7), dict(k=-1), dict(thres=None),
               dict(dex=None)):
        assert call(**kw) == INVAL, kw
        assert b"dn_render_rays_depth_refined" in hiplib.dn_last_error(), kw
    w64 = density_desc(_hip, dict(D8, hidden_size=64))
    assert call(desc_c=ctypes.byref(w64)) == -1001                                 # unsupported width, as in dn_render_rays_depth
    assert call(n=0) == 0 and call(n=0, steps=0, width=None) == 0 and call(n=0, steps=24) == 0   # valid no-ops

    comp = dict(rf=fake, z=fake, rd=fake, rd_stride=3, thres=fake, k=2, n=4, s=8, depth=fake, acc=fake, dex=fake, br=fake, z_mid=fake, stream=None)
    ccall = lambda **kw: hiplib.dn_composite_density_brackets(*{**comp, **kw}.values())  # noqa: E731
    for kw in (dict(rf=None), dict(z=None), dict(rd=None), dict(br=None), dict(z_mid=None), dict(s=0), dict(n=-1), dict(rd_stride=2), dict(k=0),
               dict(k=-1), dict(thres=None), dict(rf=odd), dict(br=odd)):
        assert ccall(**kw) == INVAL, kw
        assert b"dn_composite_density_brackets" in hiplib.dn_last_error(), kw
    assert ccall(n=0) == 0

    step = dict(br=fake, rf_mid=fake, thres=fake, k=2, n=4, z_mid=fake, stream=None)
    scall = lambda **kw: hiplib.dn_dex_bisect(*{**step, **kw}.values())  # noqa: E731
    for kw in (dict(br=None), dict(rf_mid=None), dict(z_mid=None), dict(thres=None), dict(k=0), dict(k=-1), dict(n=-1), dict(br=odd),
               dict(rf_mid=odd), dict(n=2 ** 31, k=2)):
        assert scall(**kw) == INVAL, kw
        assert b"dn_dex_bisect" in hiplib.dn_last_error(), kw
    assert scall(n=0) == 0

    fin = dict(br=fake, thres=fake, k=2, n=4, refined=fake, width=fake, stream=None)
    fcall = lambda **kw: hiplib.dn_dex_refine_finish(*{**fin, **kw}.values())  # noqa: E731
    for kw in (dict(br=None), dict(refined=None), dict(thres=None), dict(k=0), dict(k=-1), dict(n=-1), dict(br=odd), dict(n=2 ** 31, k=2)):
        assert fcall(**kw) == INVAL, kw
        assert b"dn_dex_refine_finish" in hiplib.dn_last_error(), kw
    assert fcall(n=0) == 0 and fcall(n=0, width=None) == 0

    size = hiplib.dn_render_depth_refined_workspace_bytes
    plain = hiplib.dn_render_depth_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for n, nc, nf, k in ((8, 16, 24, 3), (100, 64, 0, 1), (0, 64, 128, 5), (4096, 64, 128, 65)):
        assert size(n, nc, nf, k) == plain(n, nc, nf) + up(16 * n * k) + up(4 * n * k) + up(16 * n * k)
    assert size(-1, 16, 24, 3) == 0 and size(8, 0, 24, 3) == 0 and size(8, 16, -1, 3) == 0 and size(8, 16, 24, 0) == 0
    assert size(2 ** 31, 16, 24, 2) == 0


@pytest.mark.parametrize("name", ["render_d8w256_val", "render_lego_val"])
def test_restatement_on_the_goldens_own_field(golden, name):
    """The restated definition on the reference-recorded fine field: its Dex depth is the recorded one bit for bit for all 20
    thresholds, and every restated linear refinement lies in its bracket."""
    g = golden(name)
    s, z = g["rf_fine"][..., 3], g["z_fine"]
    idx, br, z_mid = brackets_restatement(s, z, M_THRES)
    rows = np.arange(len(z))[:, None]
    assert same_bits(z[rows, np.maximum(idx, 0)].T.copy(), g["vf_dex"])
    refined, width = finish_restatement(br, M_THRES)
    assert (refined >= br[..., 0].T).all() and (refined <= br[..., 1].T).all()
    assert ((z_mid >= br[..., 0]) & (z_mid <= br[..., 1])).all()
    np.testing.assert_array_equal(width == -1.0, (idx < 0).T)
    proper = ((idx >= 1) & (br[..., 1] > br[..., 0])).mean(0)
    zero_width = ((idx >= 1) & (br[..., 1] == br[..., 0])).sum()
    print(f"{name}: proper brackets per threshold {proper.min():.3f} .. {proper.max():.3f}; zero-width proper brackets {zero_width}; "
          f"rays crossing at the first sample {(idx == 0).any(1).sum()}")
    if name == "render_lego_val":
        t3 = [M_THRES.index(m) for m in T3]
        assert proper.min() >= 0.25 and zero_width == 0 and proper[t3].min() >= 0.25


BAD_CALLS = [dict(refine_steps=-1), dict(refine_steps=25), dict(refine_steps=2.0), dict(refine_steps="3"), dict(refine_steps=True),
             dict(refine_steps=2, m_thres_cand=None), dict(refine_steps=2, m_thres_cand=[]), dict(refine_steps=2, m_thres_cand=[5.0, -1.0]),
             dict(refine_steps=2, m_thres_cand=[float("nan")]), dict(refine_steps=2, m_thres_cand=[float("inf")]),
             dict(refine_steps=2, quantiles=[0.5]), dict(refine_steps=2, occupancy="any grid"), dict(refine_steps=2, noise=0.2),
             dict(refine_width=True)]


@pytest.mark.parametrize("bad", BAD_CALLS, ids=[",".join(f"{k}={v!r}" for k, v in b.items()) for b in BAD_CALLS])
def test_refinement_is_validated_on_the_host(bad):
    """Every refusal is a ValueError before anything touches a device: host tensors, no models."""
    import nerf
    kw = dict(dict(m_thres_cand=[5.0, 20.0]), **bad)
    cfg = make_cfg(dict(CASES["render_lego_val"][2], noise_std=kw.pop("noise", 0.0)))
    with pytest.raises(ValueError):
        nerf.render_dex_depth(1, 4, 1.0, None, None, torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), cfg, **kw)


def test_refinement_helpers_and_flags():
    import eval_nerf
    from nerf import _ops
    assert [_ops.check_refine_steps(r) for r in (0, 1, 24)] == [0, 1, 24]
    assert _ops.check_refine_thresholds([0.0, 5, 60.5]) == [0.0, 5.0, 60.5]
    for bad in (-1, 25, 1.5, None, False):
        with pytest.raises(ValueError):
            _ops.check_refine_steps(bad)
    base = ["--checkpoint", "none.ckpt"]
    for argv in (["--dex-refine", "4"],                                                  # belongs to --depth-only with --m-thres
                 ["--depth-only", "--dex-refine", "4"],
                 ["--depth-only", "--depth-quantiles", "0.5", "--dex-refine", "4"],
                 ["--m-thres", "20", "--dex-refine", "4"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine-width"],               # the refinement is off by default
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "25"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "-1"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "2.5"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "4", "--depth-quantiles", "0.5"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "4", "--occupancy", "32"]):
        with pytest.raises(SystemExit):
            eval_nerf.main(base + argv)
    for argv in (["--depth-only", "--m-thres", "20"], ["--depth-only", "--m-thres", "20", "--dex-refine", "0"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine", "24", "--dex-refine-width"]):
        with pytest.raises(FileNotFoundError):   # every flag has been judged: the next thing is the checkpoint, which is not there
            eval_nerf.main(base + argv)


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


def thresholds(k):
    return (1.0 + 0.25 * np.arange(k)).astype(F32)


def planted_rays(s, k):
    """Seven rays of s samples for thresholds(k): below every threshold but where planted.  Rows 0-4 cross at index 0, 1, 63, 64 and
    s-1 (clipped to the ray) with a value the lower half of the thresholds cross; row 5 never crosses; row 6 ramps, so the thresholds
    cross at different samples.  On top: s == m exactly ahead of a crossing, NaN just before a crossing, a -inf sample, +inf crossings
    (what the upper thresholds, those of the second group among them, cross), two equal consecutive depths at a crossing."""
    gen = np.random.default_rng(100 * s + k)
    m = thresholds(k)
    n = 7
    z = (np.linspace(2.0, 6.0, s)[None, :] + 0.01 * gen.random((n, s))).astype(F32)
    sig = (-2.0 + 2.5 * gen.random((n, s))).astype(F32)                  # in [-2, 0.5): below m_0 = 1
    mid = F32(m[k // 2] + F32(0.125))
    plants = [0, 1, 63, 64, s - 1]
    for r, j in enumerate(plants):
        j = min(j, s - 1)
        sig[r, j] = mid
        if j >= 2:
            sig[r, j - 2] = m[0]                                         # s == m exactly: not a crossing
        if j >= 1 and r % 2 == 0:
            sig[r, j - 1] = np.nan                                       # NaN never crosses; it becomes s_lo
        if j >= 1 and r == 3:
            z[r, j] = z[r, j - 1]                                        # a zero-width proper bracket
    if s >= 3:
        sig[1, s - 1] = np.inf                                           # what the upper thresholds of row 1 cross
        sig[2, min(65, s - 1)] = np.inf
        sig[5, s // 2] = -np.inf
        sig[6] = (np.linspace(0.0, float(m[-1]) + 1.0, s)).astype(F32)   # a ramp: every threshold crosses somewhere else
        sig[6, s // 3] = np.nan
    rd = gen.standard_normal((n, 3)).astype(F32)
    rf = gen.standard_normal((n, s, 4)).astype(F32)
    rf[..., 3] = sig
    return rf, z, rd, m


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 64, 65])
@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 130])
def test_bracket_kernel_against_the_restatement_and_composite_density(dev, s, k):
    from nerf import _ops
    rf, z, rd, m = planted_rays(s, k)
    idx, br_want, mid_want = brackets_restatement(rf[..., 3], z, m)
    if s == 130 and k == 65:                                              # every planted case is there
        assert {0, 1, 63, 64, s - 1, -1} <= set(idx.reshape(-1).tolist())
        assert np.isnan(br_want[..., 2]).any() and np.isposinf(br_want[..., 3]).any() and (idx[:, 64] >= 0).any()
        assert ((idx >= 1) & (br_want[..., 0] == br_want[..., 1])).any()
    thres = G(m, dev)
    with torch.no_grad():
        depth0, acc0, dex0 = _ops.composite_density(G(rf, dev), G(z, dev), G(rd, dev), None, 0.0, thres)
        depth, acc, dex, br, z_mid = _ops.composite_density_brackets(G(rf, dev), G(z, dev), G(rd, dev), thres)
    assert same_bits(depth, depth0) and same_bits(acc, acc0) and same_bits(dex, dex0)
    assert br.shape == (7, k, 4) and z_mid.shape == (7, k)
    assert same_bits(br, br_want), (C(br), br_want)
    assert same_bits(z_mid, mid_want)
    rows = np.arange(7)[:, None]
    assert same_bits(dex, z[rows, np.maximum(idx, 0)].T.copy())           # the bracket's index is the Dex depth's


def planted_records(n, k, seed):
    """Records (n,k,4) of every kind, their thresholds and three rounds of midpoint densities."""
    gen = np.random.default_rng(seed)
    m = thresholds(k)
    lo = (2.0 + 3.0 * gen.random((n, k))).astype(F32)
    hi = (lo + F32(0.001) + F32(0.06) * gen.random((n, k)).astype(F32)).astype(F32)
    s_lo = (m[None, :] - 3.0 * gen.random((n, k))).astype(F32)
    s_hi = (m[None, :] + 0.01 + 30.0 * gen.random((n, k))).astype(F32)
    br = np.stack([lo, hi, s_lo, s_hi], -1).astype(F32)
    kind = gen.integers(0, 8, (n, k))
    kind.reshape(-1)[:8] = np.arange(8)[: n * k]                          # every kind at least once where there is room
    first, none, adjacent, nan_lo, inf_hi = kind == 0, kind == 1, kind == 2, kind == 3, kind == 4
    br[first, 1], br[first, 2] = br[first, 0], br[first, 3]               # (z_0, z_0, s_0, s_0)
    br[none, 1], br[none, 2], br[none, 3] = br[none, 0], F32(np.inf), F32(-np.inf)
    br[adjacent, 1] = np.nextafter(br[adjacent, 0], F32(np.inf))          # a bracket of two adjacent floats
    br[nan_lo, 2] = np.nan
    br[inf_hi, 3] = np.inf
    mids = []
    for _ in range(3):
        sm = (m[None, :] + 8.0 * (gen.random((n, k)) - 0.5)).astype(F32)
        pick = gen.integers(0, 6, (n, k))
        sm[pick == 0] = np.nan
        sm[pick == 1] = np.broadcast_to(m[None, :], (n, k))[pick == 1]    # s == m exactly: not a crossing
        sm[pick == 2] = np.inf
        mids.append(sm)
    return br, m, mids


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1, 1), (67, 1), (1, 65), (67, 65)])
def test_bisect_kernel_on_planted_records(dev, n, k):
    from nerf import _ops
    br0, m, mids = planted_records(n, k, 7 * n + k)
    thres = G(m, dev)
    br = G(br0, dev)
    want = br0
    for sm in mids:
        rf_mid = np.random.default_rng(1).standard_normal((n, k, 4)).astype(F32)
        rf_mid[..., 3] = sm
        before = want
        want, mid_want = bisect_restatement(want, sm, m)
        with torch.no_grad():
            z_mid = _ops.dex_bisect(br, G(rf_mid, dev), thres)
        assert same_bits(br, want) and same_bits(z_mid, mid_want)
        flat = before[..., 0] == before[..., 1]
        assert same_bits(want[flat], before[flat])                        # both degenerate kinds stay untouched
        changed = (bits(want) != bits(before)).any(-1)
        assert not changed[flat].any() and (n * k < 8 or changed.any())
    if n * k >= 8:
        assert (br0[..., 3] == -np.inf).any() and (np.nextafter(br0[..., 0], F32(np.inf)) == br0[..., 1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1, 1), (67, 3), (5, 65)])
def test_finish_kernel_against_the_float64_restatement(dev, n, k):
    from nerf import _ops
    br, m, _ = planted_records(n, k, 11 * n + k)
    br[0, 0] = (2.0, 3.0, 0.0, 4.0)                                       # closed forms, threshold m_0 = 1
    thres = G(m, dev)
    with torch.no_grad():
        refined, width = _ops.dex_refine_finish(G(br, dev), thres)
        only, nothing = _ops.dex_refine_finish(G(br, dev), thres, want_width=False)
    want_r, want_w = finish_restatement(br, m)
    assert refined.shape == (k, n) and same_bits(refined, want_r) and same_bits(width, want_w)
    assert nothing is None and same_bits(only, refined)                   # width = NULL
    assert float(refined[0, 0]) == 2.25 and float(width[0, 0]) == 1.0
    closed = np.array([[[2.0, 3.0, -1.0, np.inf]], [[2.0, 3.0, np.nan, 4.0]], [[2.5, 2.5, 7.0, 7.0]], [[2.5, 2.5, np.inf, -np.inf]],
                       [[2.0, 4.0, 1.0, 2.0]], [[2.0, 4.0, -1.0, 3.0]]], F32)    # (6 rays, 1 threshold)
    with torch.no_grad():
        r, w = _ops.dex_refine_finish(G(closed, dev), G(thresholds(1), dev))
    assert C(r)[0].tolist() == [2.5, 2.5, 2.5, 2.5, 2.0, 3.0]              # a non-finite end: the midpoint; s_lo == m: z_lo
    assert C(w)[0].tolist() == [1.0, 1.0, 0.0, -1.0, 2.0, 2.0]


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


def depth_render(name, g, dev, cfg=None, thres=T3, **kw):
    import nerf
    mc, mf = models_of(name, dev)
    ex = nerf.get_embedding_function(10)
    with torch.no_grad():
        return nerf.render_dex_depth(1, len(g["ro"]), 1.0, mc, mf, G(g["ro"], dev)[None], G(g["rd"], dev)[None], cfg or make_cfg(CASES[name][2]),
                                     mode="validation", encode_position_fn=ex, m_thres_cand=list(thres), **kw)


def ray_rows(name, g, dev):
    from nerf import _ops
    rkw = CASES[name][2]
    return _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), None, rkw["near"], rkw["far"])


def chain(packs, rays, nc, nf, thres, steps):
    """The refined render from the older entry points and the three standalone new ones."""
    from nerf import _ops
    pc, pf = packs
    rd = rays[:, 3:6]
    with torch.no_grad():
        z = _ops.coarse_depths(rays, nc, False)
        rf = _ops.run_network_rays(pc, rays, z)
        depth_c = acc_c = None
        last = pc
        if nf > 0:
            depth_c, acc_c, z = _ops.density_resample(rf, z, rd, nf)
            rf = _ops.run_network_rays(pf, rays, z)
            last = pf
        depth, acc, dex, br, z_mid = _ops.composite_density_brackets(rf, z, rd, thres)
        br0 = br.clone()
        for _ in range(steps):
            z_mid = _ops.dex_bisect(br, _ops.run_network_rays(last, rays, z_mid), thres)
        refined, width = _ops.dex_refine_finish(br, thres)
    maps = (depth_c, acc_c, depth, acc) if nf > 0 else (depth, acc, None, None)
    return dict(maps=maps + (dex, refined, width), br=br, br0=br0, z=z, rf=rf)


@pytest.fixture(scope="module")
def lego_chain(golden, dev):
    """The fp32 chain on the lego rays, 64+64, thresholds (5, 20, 60), without a step: depths, field and initial records - shared
    and left unchanged."""
    from nerf import _hip
    name = "render_lego_val"
    mc, mf = models_of(name, dev)
    packs = (mc.packed_density(precision=_hip.PREC_F32), mf.packed_density(precision=_hip.PREC_F32))
    rays = ray_rows(name, golden(name), dev)
    return packs, rays, chain(packs, rays, 64, 64, G(np.asarray(T3, F32), dev), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,thres", [("render_lego_val", T3), ("render_d8w256_val", (5.0,))])
def test_refined_driver_equals_the_chain_bit_for_bit(golden, dev, name, thres, precision):
    from nerf import _hip, _ops
    g = golden(name)
    rkw = CASES[name][2]
    nc, nf = rkw["num_coarse"], rkw["num_fine"]
    prec = dict(fp32=_hip.PREC_F32, bf16=_hip.PREC_BF16)[precision]
    packs = tuple(m.packed_density(precision=prec) for m in models_of(name, dev))
    rays = ray_rows(name, g, dev)
    n, k = rays.shape[0], len(thres)
    th = G(np.asarray(thres, F32), dev)
    cases = [(nf, r) for r in (0, 1, 5)] + ([(0, 5)] if (name, precision) == ("render_lego_val", "fp32") else [])
    for fine, steps in cases:
        want = chain(packs, rays, nc, fine, th, steps)
        with torch.no_grad():
            got = _ops.render_rays_depth(*packs, rays, nc, fine, False, 0.0, th, refine_steps=steps, want_width=True)
            off = _ops.render_refined_records_offset(n, nc, fine)
            br = _ops._latest_render_workspace()[off:off + 16 * n * k].clone().view(torch.float32).reshape(n, k, 4)
            plain = _ops.render_rays_depth(*packs, rays, nc, fine, False, 0.0, th)
            short = _ops.render_rays_depth(*packs, rays, nc, fine, False, 0.0, th, refine_steps=steps)
        assert len(got) == 7 and len(plain) == 5 and len(short) == 6 and same_bits(short[5], got[5])
        for label, a, b in zip(("depth_c", "acc_c", "depth_f", "acc_f", "dex", "refined", "width"), got, want["maps"]):
            assert (a is None and b is None) or same_bits(a, b), (name, precision, fine, steps, label)
        for a, b in zip(plain, got):                                      # the maps ahead of the refined ones are the plain render's
            assert (a is None and b is None) or same_bits(a, b)
        assert same_bits(br, want["br"])
        hit = C(got[6]) >= 0
        print(f"{name} {precision} {nc}+{fine} R={steps}: rays with a crossing {hit.mean(1).round(3).tolist()}, widest last bracket "
              f"{float(got[6].max()):.3e}")
        assert hit.any() and (C(got[6]) > 0).any()


@pytest.mark.gpu
def test_render_dex_depth_refined_follows_the_render_policy_and_none_is_the_plain_render(golden, dev):
    import warnings

    import nerf
    name = "render_d8w256_val"
    g = golden(name)
    k = len(T3)
    plain = depth_render(name, g, dev)
    same = depth_render(name, g, dev, refine_steps=None)
    out = depth_render(name, g, dev, refine_steps=3)
    wide = depth_render(name, g, dev, refine_steps=3, refine_width=True)
    assert len(plain) == len(same) == 4 + k and len(out) == 4 + 2 * k and len(wide) == 4 + 3 * k
    assert all(o.shape == (1, len(g["ro"])) for o in wide)
    assert all(same_bits(a, b) for a, b in zip(plain, same)) and all(same_bits(a, b) for a, b in zip(plain, out))
    assert all(same_bits(a, b) for a, b in zip(out, wide))
    # under 'bf16' the default policy renders in guarded fp16: the bits of the same call with the precision forced to fp16
    nerf.set_precision("fp16")
    ref16 = depth_render(name, g, dev, refine_steps=3, refine_width=True)
    nerf.set_precision("bf16")
    nerf.set_render_policy("bf16")
    pure = depth_render(name, g, dev, refine_steps=3, refine_width=True)
    nerf.set_render_policy(None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pol = depth_render(name, g, dev, refine_steps=3, refine_width=True)
    assert all(same_bits(a, b) for a, b in zip(pol, ref16))
    assert not all(same_bits(a, b) for a, b in zip(pol[4 + k:4 + 2 * k], pure[4 + k:4 + 2 * k]))


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 5, 8])
def test_refined_depths_stay_in_their_brackets_and_the_widths_halve(golden, dev, lego_chain, steps):
    from nerf import _ops
    packs, rays, ch = lego_chain
    name = "render_lego_val"
    th = G(np.asarray(T3, F32), dev)
    with torch.no_grad():
        out = _ops.render_rays_depth(*packs, rays, 64, 64, False, 0.0, th, refine_steps=steps, want_width=True)
    refined, width = C(out[5]), C(out[6])
    br0 = C(ch["br0"])
    idx, br_want, _ = brackets_restatement(C(ch["rf"])[..., 3], C(ch["z"]), T3)
    assert same_bits(br0, br_want)                                       # the chain's initial records are the restatement's
    lo, hi = br0[..., 0].T, br0[..., 1].T
    w0 = hi - lo
    proper = (idx.T >= 1) & (w0 > 0)
    assert proper.mean() >= 0.25
    assert (refined[proper] >= lo[proper]).all() and (refined[proper] <= hi[proper]).all()
    bound = w0.astype(np.float64) * 2.0 ** -steps + steps * np.spacing(hi).astype(np.float64)
    assert (width[proper] <= bound[proper]).all(), float((width - bound)[proper].max())
    assert (width[proper] > 0).all()
    np.testing.assert_array_equal(width == -1.0, idx.T < 0)              # -1 exactly where the plain Dex depth had no crossing
    np.testing.assert_array_equal(width == 0.0, (idx.T == 0) | ((idx.T >= 1) & (w0 == 0)))
    assert same_bits(refined[idx.T < 0], C(out[4])[idx.T < 0])            # no crossing: the Dex fallback z_0
    print(f"R={steps}: {int(proper.sum())} proper brackets, widest initial {w0[proper].max():.3e}, widest last {width[proper].max():.3e}")
    if steps == 5:                                                        # the maps do not depend on the chunking
        g = golden(name)
        one = depth_render(name, g, dev, refine_steps=steps, refine_width=True)
        several = depth_render(name, g, dev, cfg=make_cfg(CASES[name][2], chunksize=50), refine_steps=steps, refine_width=True)
        assert all(same_bits(a, b) for a, b in zip(one, several))
        assert same_bits(one[4 + 3][0], out[5][0]) and same_bits(one[4 + 6][0], out[6][0])


def oracle_sigma(sd, mc, ro, rd, z):
    """Raw density of the CPU oracle at ro + rd z, fp32: z (P, J) for P rays -> (P, J)."""
    from oracle import nerf_oracle as oc
    ro, rd, z = torch.from_numpy(ro), torch.from_numpy(rd), torch.from_numpy(np.ascontiguousarray(z, F32))
    pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
    with torch.no_grad():
        return oc.run_network(sd, pts, rd, mc)[..., 3].numpy()


@pytest.mark.gpu
def test_refined_depth_accuracy_against_dense_oracle_truth(golden, dev):
    """fp32, render_lego_val, thresholds (5, 20, 60), 8 steps.  Measured on an MI355X: 87 rays cross, 261 proper brackets, 1 left out
    (it crosses more than once); |z - truth| median / p99 / max: sample depth 7.8e-4 / 2.7e-2 / 4.1e-2, refined on the GPU 8.9e-8 /
    1.1e-6 / 1.9e-6, refined on the oracle 9.0e-8 / 1.1e-6 / 1.9e-6; worst excess of the GPU over the oracle 2.4e-7 (gate 1e-4)."""
    from nerf import _hip, _ops
    from oracle import nerf_oracle as oc
    name = "render_lego_val"
    g = golden(name)
    steps, dense = 8, 513
    m = np.asarray(T3, F32)
    s, z = g["rf_fine"][..., 3], g["z_fine"]
    idx, br_want, mid_want = brackets_restatement(s, z, m)
    th = G(m, dev)
    mf = models_of(name, dev)[1]
    pf = mf.packed_density(precision=_hip.PREC_F32)
    rays = ray_rows(name, g, dev)
    with torch.no_grad():
        _, _, _, br, z_mid = _ops.composite_density_brackets(G(g["rf_fine"], dev), G(z, dev), G(g["rd"], dev), th)
        assert same_bits(br, br_want) and same_bits(z_mid, mid_want)      # the initial brackets are the restatement's bit for bit
        for _ in range(steps):
            z_mid = _ops.dex_bisect(br, _ops.run_network_rays(pf, rays, z_mid), th)
        z_gpu = C(_ops.dex_refine_finish(br, th)[0]).T                    # (N,K)
    # the same algorithm on the oracle network
    mkw = CASES[name][0]
    mc = oc.ModelCfg(**mkw)
    sd = oc.to_torch_sd(lego_weights()[1])
    bo, mo = br_want, mid_want
    for _ in range(steps):
        bo, mo = bisect_restatement(bo, oracle_sigma(sd, mc, g["ro"], g["rd"], mo), m)
    z_oracle = finish_restatement(bo, m)[0].T
    # truth: the first crossing among 513 dense oracle evaluations inside each initial bracket, interpolated
    pairs = np.argwhere((idx >= 1) & (br_want[..., 1] > br_want[..., 0]))
    r, k = pairs[:, 0], pairs[:, 1]
    lo, hi = br_want[r, k, 0].astype(np.float64), br_want[r, k, 1].astype(np.float64)
    zd = (lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, dense)[None, :]).astype(F32)
    sdense = oracle_sigma(sd, mc, g["ro"][r], g["rd"][r], zd).astype(np.float64)
    above = sdense > m[k].astype(np.float64)[:, None]
    changes = (above[:, 1:] != above[:, :-1]).sum(-1)
    j = above.argmax(-1)
    usable = above.any(-1) & (changes <= 1)
    jm = np.maximum(j - 1, 0)
    rows = np.arange(len(pairs))
    s0, s1 = sdense[rows, jm], sdense[rows, j]
    z0, z1 = zd[rows, jm].astype(np.float64), zd[rows, j].astype(np.float64)
    with np.errstate(all="ignore"):
        z_true = np.where(j == 0, z0, z0 + (z1 - z0) * (m[k].astype(np.float64) - s0) / (s1 - s0))
    err_gpu = np.abs(z_gpu[r, k].astype(np.float64) - z_true)[usable]
    err_oracle = np.abs(z_oracle[r, k].astype(np.float64) - z_true)[usable]
    err_sample = np.abs(hi - z_true)[usable]
    print(f"{name}: {len(set(r.tolist()))} rays cross, {len(pairs)} proper (ray, threshold) brackets, {int((~usable).sum())} left out "
          f"({int((changes > 1).sum())} cross more than once); |z - truth| median / p99 / max: sample depth {np.median(err_sample):.2e} / "
          f"{np.quantile(err_sample, 0.99):.2e} / {err_sample.max():.2e}, refined on the GPU {np.median(err_gpu):.2e} / "
          f"{np.quantile(err_gpu, 0.99):.2e} / {err_gpu.max():.2e}, refined on the oracle {np.median(err_oracle):.2e} / "
          f"{np.quantile(err_oracle, 0.99):.2e} / {err_oracle.max():.2e}; worst excess over the oracle {(err_gpu - err_oracle).max():.2e}")
    assert len(pairs) >= 0.25 * idx.size and (~usable).mean() <= 0.02
    assert (err_gpu <= err_oracle + 1e-4).all()
    assert np.median(err_gpu) < 0.1 * np.median(err_sample)


@pytest.mark.gpu
def test_refined_depth_render_is_hipgraph_capturable(golden, dev, lego_chain):
    """dn_render_rays_depth_refined neither allocates nor reads back: a captured chunk replays to the eager outputs bit for bit."""
    from nerf import _ops
    packs, rays, _ = lego_chain
    thres = G(np.asarray(T3, F32), dev)
    run = lambda: _ops.render_rays_depth(*packs, rays, 64, 64, False, 0.0, thres, refine_steps=4, want_width=True)  # noqa: E731
    eager = run()
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
    assert all(same_bits(a, b) for a, b in zip(eager, captured))


@pytest.mark.gpu
def test_eval_driver_dex_refine(dev, tmp_path):
    """eval_nerf.py --depth-only --m-thres --dex-refine R [--dex-refine-width]: dex_refined / dex_width beside dex in dex_<view>.npz."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "1", "--num-fine", "64", "--precision", "fp32", "--quiet", "--depth-only",
              "--m-thres", "10"]
    out = tmp_path / "out"
    res = eval_nerf.main(common + ["--dex-refine", "4", "--dex-refine-width", "--savedir", str(out)])
    maps = np.load(out / "dex_0000.npz")
    assert sorted(maps.files) == ["depth", "dex", "dex_refine_steps", "dex_refined", "dex_width", "m_thres"]
    assert maps["dex"].shape == maps["dex_refined"].shape == maps["dex_width"].shape == (2, 24, 24) and int(maps["dex_refine_steps"]) == 4
    hit = maps["dex_width"] > 0
    assert hit.any() and (maps["dex_refined"][hit] <= maps["dex"][hit]).all() and np.isfinite(maps["dex_refined"]).all()
    assert np.array_equal(maps["dex_refined"][~hit], maps["dex"][~hit])       # first-sample crossings and misses keep the Dex depth
    assert len(res["frames"][0]) == 5
    plain = tmp_path / "plain"
    eval_nerf.main(common + ["--savedir", str(plain)])
    assert sorted(np.load(plain / "dex_0000.npz").files) == ["depth", "dex", "m_thres"]
    assert np.array_equal(np.load(plain / "dex_0000.npz")["dex"], maps["dex"])
