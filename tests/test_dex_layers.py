"""Dex depth layers (include/dexnerf_hip_layers.h): dn_composite_density_layers, dn_dex_layers_finish, dn_render_rays_depth_layers,
nerf.render_dex_layers, nerf.dex_thickness, the driver flags.

The header's definitions are restated below in numpy (`layers_restatement`, `finish_restatement`; the bisection step is the refine
header's and is restated as there): fp32 where the header says fp32, float64 rounded once where it says so.  The kernels are INDEX and
SELECTION work plus one rounding each, so they are compared bit for bit; the driver is compared bit for bit against a chain of the
older entry points and the new standalone ones.  The accuracy gate needs a truth: the one state change among 513 dense evaluations of
the CPU oracle inside each event's sample bracket, interpolated."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import CASES, D8, M_THRES, lego_weights

LAYERS = ("dn_composite_density_layers", "dn_dex_layers_finish", "dn_render_depth_layers_workspace_bytes", "dn_render_rays_depth_layers")
INVAL = -1000
T3 = (5.0, 20.0, 60.0)
F32 = np.float32
INF = F32(np.inf)


# ---- the header's definitions in numpy ----------------------------------------------------------------------------------------------
def layers_restatement(s, z, m, n_layers):
    """s, z (N,S) fp32; m (K,) -> count (K,N) int32, br (N,K,2L,4) fp32, z_mid (N,K*2L) fp32, idx (N,K,2L) int (-1: no such event)."""
    s, z, m = np.asarray(s, F32), np.asarray(z, F32), np.asarray(m, F32)
    n, k, e2 = len(s), len(m), 2 * n_layers
    with np.errstate(invalid="ignore"):
        above = s[:, None, :] > m[None, :, None]                         # NaN is not above, +inf is
    prev = np.concatenate([np.zeros_like(above[..., :1]), above[..., :-1]], -1)   # above_{-1} = false
    event = above != prev
    count = event.sum(-1).astype(np.int32).T.copy()
    br = np.empty((n, k, e2, 4), F32)
    br[..., 0] = br[..., 1] = z[:, 0][:, None, None]                   # "none": (z_0, z_0, +inf, -inf)
    br[..., 2], br[..., 3] = INF, -INF
    idx = np.full((n, k, e2), -1)
    for r in range(n):
        for t in range(k):
            for e, j in enumerate(np.flatnonzero(event[r, t])[:e2]):
                idx[r, t, e] = j
                b = max(j - 1, 0)
                lo, hi = (j, b) if e % 2 else (b, j)                     # the hi end is the sample above m: an exit's is the one before
                br[r, t, e] = (z[r, lo], z[r, hi], s[r, lo], s[r, hi])
    return count, br, midpoint(br).reshape(n, k * e2), idx


def midpoint(br):
    with np.errstate(invalid="ignore"):
        return (br[..., 0] + F32(0.5) * (br[..., 1] - br[..., 0])).astype(F32)


def bisect_restatement(br, s_mid, m_rec):
    """One step of the refine header on records br (..., 4) with the densities s_mid (...) at their midpoints and the threshold of
    every record m_rec (...) -> (br', z_mid')."""
    br = br.copy()
    zm = midpoint(br)
    live = br[..., 0] != br[..., 1]
    with np.errstate(invalid="ignore"):
        up = live & (s_mid > m_rec)
    down = live & ~up                                                   # NaN included
    br[up, 1], br[up, 3] = zm[up], s_mid[up]
    br[down, 0], br[down, 2] = zm[down], s_mid[down]
    return br, midpoint(br)


def finish_restatement(br, m, interp):
    """(events (K,2L,N) fp32, width (K,2L,N) fp32) of br (N,K,2L,4)."""
    b = br.astype(np.float64)
    m64 = np.asarray(m, F32).astype(np.float64)[None, :, None]
    lo, hi, s_lo, s_hi = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    none = br[..., 3] == -INF
    flat = br[..., 0] == br[..., 1]
    odd = (np.arange(br.shape[2]) % 2 == 1)[None, None, :]
    with np.errstate(all="ignore"):
        gap = np.abs(br[..., 1] - br[..., 0]).astype(F32)
        if interp:
            finite = np.isfinite(s_lo) & np.isfinite(s_hi)
            t = np.where(finite, (m64 - s_lo) / (s_hi - s_lo), 0.5)
            depth = np.where(flat, lo, lo + (hi - lo) * t).astype(F32)  # rounded once
            width = np.where(flat, F32(0.0), gap)
        else:
            depth = np.where(odd, br[..., 0], br[..., 1])               # the sample at which the state changes
            width = gap
    depth = np.where(none, INF, depth).astype(F32)
    width = np.where(none, F32(-1.0), width).astype(F32)
    return depth.transpose(1, 2, 0).copy(), width.transpose(1, 2, 0).copy()


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def same_ints(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)


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
def test_layers_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_layers.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.LAYERS_EXPORTS) == set(LAYERS)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS) | set(_hip.OCCUPANCY_EXPORTS) | set(_hip.CULL_EXPORTS)
             | set(_hip.REFINE_EXPORTS) | set(_hip.SPAN_EXPORTS))
    assert not older & set(LAYERS)
    assert hiplib.dn_abi_version() == 2 and len(_hip.EXPORTS) == 76 and len(_hip.REFINE_EXPORTS) == 5
    assert "dexnerf_hip_layers.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()       # build() checks the new header's symbols too
    assert "composite_layers.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in LAYERS)
    assert "#define DN_MAX_LAYERS 8" in text and _hip.MAX_LAYERS == 8
    assert "#define DN_MAX_LAYER_RECORDS 2048" in text and _hip.MAX_LAYER_RECORDS == 2048


def test_layers_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    from nerf import _hip
    fake = ctypes.c_void_p(256 * 4096)
    odd = ctypes.c_void_p(256 * 4096 + 4)
    dd, with_dirs = density_desc(_hip, D8), full_desc(_hip, D8)
    defaults = dict(desc_c=ctypes.byref(dd), packed_c=fake, desc_f=ctypes.byref(dd), packed_f=fake, prec=_hip.PREC_F32, rays=fake, stride=8, n=8,
                    nc=16, nf=24, lindisp=0, std=0.0, thres=fake, k=3, t_rand=None, noise_c=None, u=None, noise_f=None, depth_c=fake,
                    acc_c=fake, depth_f=fake, acc_f=fake, dex=fake, layers=2, steps=4, events=fake, count=fake, width=fake, ws=fake, stream=None)
    call = lambda **kw: hiplib.dn_render_rays_depth_layers(*{**defaults, **kw}.values())  # noqa: E731
    for kw in (dict(k=0), dict(k=0, thres=None, dex=None), dict(layers=0), dict(layers=9), dict(layers=-1), dict(k=129, layers=8),
               dict(k=1025, layers=1), dict(n=2 ** 27, k=1, layers=8), dict(n=2 ** 31, k=1, layers=1), dict(steps=-2), dict(steps=25),
               dict(std=0.1), dict(std=-0.1), dict(std=float("nan")), dict(events=None), dict(count=None),
               # dn_render_rays_depth's own refusals
               dict(desc_c=None), dict(packed_c=None), dict(rays=None), dict(ws=None), dict(n=-1), dict(desc_f=None), dict(packed_f=None),
               dict(ws=ctypes.c_void_p(256 * 4096 + 16)), dict(desc_f=ctypes.byref(with_dirs)), dict(desc_c=ctypes.byref(with_dirs)),
               dict(nc=9), dict(nc=513), dict(nc=512, nf=1537), dict(nc=0), dict(nf=-1), dict(stride=7), dict(k=-1), dict(thres=None),
               dict(dex=None)):
        assert call(**kw) == INVAL, kw
        assert b"dn_render_rays_depth_layers" in hiplib.dn_last_error(), kw
    w64 = density_desc(_hip, dict(D8, hidden_size=64))
    assert call(desc_c=ctypes.byref(w64)) == -1001                                 # unsupported width, as in dn_render_rays_depth
    assert call(n=0) == 0 and call(n=0, steps=-1, width=None) == 0 and call(n=0, steps=24, layers=8) == 0   # valid no-ops

    comp = dict(rf=fake, z=fake, rd=fake, rd_stride=3, thres=fake, k=2, layers=2, n=4, s=8, depth=fake, acc=fake, dex=fake, br=fake, z_mid=fake,
                count=fake, stream=None)
    ccall = lambda **kw: hiplib.dn_composite_density_layers(*{**comp, **kw}.values())  # noqa: E731
    for kw in (dict(rf=None), dict(z=None), dict(rd=None), dict(br=None), dict(z_mid=None), dict(count=None), dict(s=0), dict(n=-1),
               dict(rd_stride=2), dict(k=0), dict(k=-1), dict(thres=None), dict(rf=odd), dict(br=odd), dict(layers=0), dict(layers=9),
               dict(k=129, layers=8), dict(n=2 ** 27, k=1, layers=8)):
        assert ccall(**kw) == INVAL, kw
        assert b"dn_composite_density_layers" in hiplib.dn_last_error(), kw
    assert ccall(n=0) == 0

    fin = dict(br=fake, thres=fake, k=2, layers=2, interp=1, n=4, events=fake, width=fake, stream=None)
    fcall = lambda **kw: hiplib.dn_dex_layers_finish(*{**fin, **kw}.values())  # noqa: E731
    for kw in (dict(br=None), dict(events=None), dict(thres=None), dict(k=0), dict(k=-1), dict(n=-1), dict(br=odd), dict(layers=0), dict(layers=9),
               dict(interp=2), dict(interp=-1), dict(k=129, layers=8), dict(n=2 ** 27, k=1, layers=8)):
        assert fcall(**kw) == INVAL, kw
        assert b"dn_dex_layers_finish" in hiplib.dn_last_error(), kw
    assert fcall(n=0) == 0 and fcall(n=0, width=None, interp=0) == 0

    size = hiplib.dn_render_depth_layers_workspace_bytes
    plain = hiplib.dn_render_depth_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for n, nc, nf, k, layers in ((8, 16, 24, 3, 2), (100, 64, 0, 1, 1), (0, 64, 128, 5, 8), (4096, 64, 128, 65, 8)):
        ke = k * 2 * layers
        assert size(n, nc, nf, k, layers) == plain(n, nc, nf) + up(16 * n * ke) + up(4 * n * ke) + up(16 * n * ke) + up(4 * ke)
    assert size(-1, 16, 24, 3, 2) == 0 and size(8, 0, 24, 3, 2) == 0 and size(8, 16, -1, 3, 2) == 0 and size(8, 16, 24, 0, 2) == 0
    assert size(8, 16, 24, 3, 0) == 0 and size(8, 16, 24, 3, 9) == 0 and size(8, 16, 24, 129, 8) == 0 and size(2 ** 27, 16, 24, 1, 8) == 0


BAD_CALLS = [dict(layers=0), dict(layers=9), dict(layers=2.0), dict(layers="2"), dict(layers=True), dict(layers=None),
             dict(m_thres_cand=None), dict(m_thres_cand=[]), dict(m_thres_cand=[5.0, -1.0]), dict(m_thres_cand=[float("nan")]),
             dict(m_thres_cand=[float("inf")]), dict(m_thres_cand=[1.0] * 129, layers=8), dict(noise=0.2), dict(noise=0.2, refine_steps=2),
             dict(refine_steps=-1), dict(refine_steps=25), dict(refine_steps=1.5), dict(refine_steps=True),
             dict(refine_steps=2, occupancy="any grid"), dict(ray_span_pad=1.0)]


@pytest.mark.parametrize("bad", BAD_CALLS, ids=[",".join(f"{k}={str(v)[:24]}" for k, v in b.items()) for b in BAD_CALLS])
def test_layers_are_validated_on_the_host(bad):
    """Every refusal is a ValueError before anything touches a device: host tensors, no models."""
    import nerf
    kw = dict(dict(m_thres_cand=[5.0, 20.0], layers=2), **bad)
    cfg = make_cfg(dict(CASES["render_lego_val"][2], noise_std=kw.pop("noise", 0.0)))
    with pytest.raises(ValueError):
        nerf.render_dex_layers(1, 4, 1.0, None, None, torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), cfg, **kw)


def test_layer_helpers_and_flags():
    import eval_nerf
    from nerf import _ops
    assert [_ops.check_layers(n) for n in (1, 2, 8)] == [1, 2, 8]
    for bad in (0, 9, 1.5, None, False):
        with pytest.raises(ValueError):
            _ops.check_layers(bad)
    base = ["--checkpoint", "none.ckpt"]
    for argv in (["--dex-layers", "2"],                                                  # belongs to --depth-only with --m-thres
                 ["--depth-only", "--dex-layers", "2"],
                 ["--m-thres", "20", "--dex-layers", "2"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "0"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "9"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "2.5"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "2", "--depth-quantiles", "0.5"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "2", "--dex-refine", "4", "--occupancy", "32"],
                 ["--depth-only", "--m-thres", "20", "--dex-refine-width"]):              # still belongs to a refinement or to the layers
        with pytest.raises(SystemExit):
            eval_nerf.main(base + argv)
    for argv in (["--depth-only", "--m-thres", "20", "--dex-layers", "1"], ["--depth-only", "--m-thres", "20", "--dex-layers", "8", "--dex-refine", "0"],
                 ["--depth-only", "--m-thres", "20", "--dex-layers", "2", "--dex-refine-width"]):
        with pytest.raises(FileNotFoundError):   # every flag has been judged: the next thing is the checkpoint, which is not there
            eval_nerf.main(base + argv)


@pytest.mark.parametrize("name", ["render_d8w256_val", "render_lego_val"])
def test_restatement_on_the_goldens_own_field(golden, name):
    """The restated definition on the reference-recorded fine field, all 20 thresholds, two layers: event 0 of the sample mode is the
    recorded Dex depth bit for bit where the ray has an event, count is 0 exactly where no sample is above, the event depths do not
    decrease along a ray in either mode, every interpolated depth lies between its record's ends - and the inputs do have second
    layers, open ends and entries at the first sample."""
    g = golden(name)
    s, z = g["rf_fine"][..., 3], g["z_fine"]
    count, br, z_mid, idx = layers_restatement(s, z, M_THRES, 2)
    sample, w_sample = finish_restatement(br, M_THRES, False)
    interp, w_interp = finish_restatement(br, M_THRES, True)
    hit = count > 0
    assert same_bits(sample[:, 0][hit], g["vf_dex"][hit])
    with np.errstate(invalid="ignore"):
        any_above = (s[:, None, :] > np.asarray(M_THRES, F32)[None, :, None]).any(-1).T
    np.testing.assert_array_equal(count == 0, ~any_above)
    for ev in (sample, interp):
        assert (ev[:, 1:] >= ev[:, :-1]).all()                           # (+inf, "no such event", closes every row)
        np.testing.assert_array_equal(np.isinf(ev), (np.arange(4)[None, :, None] >= count[:, None, :]))
    lo, hi = np.minimum(br[..., 0], br[..., 1]).transpose(1, 2, 0), np.maximum(br[..., 0], br[..., 1]).transpose(1, 2, 0)
    stored = np.isfinite(interp)
    assert (interp[stored] >= lo[stored]).all() and (interp[stored] <= hi[stored]).all()
    mid = z_mid.reshape(len(z), len(M_THRES), 4).transpose(1, 2, 0)
    assert ((mid >= lo) & (mid <= hi)).all()
    np.testing.assert_array_equal(w_sample == -1.0, ~stored)
    np.testing.assert_array_equal(w_interp == -1.0, ~stored)
    exits = br[:, :, 1::2][idx[:, :, 1::2] >= 0]
    assert (exits[:, 0] >= exits[:, 1]).all() and (exits[:, 2] <= exits[:, 3]).all()     # an exit's lo end is the deeper, not-above one
    second = (count >= 4).sum(1)
    open_end = (count % 2 == 1).sum(1)
    at_zero = (idx[:, :, 0] == 0).sum(0)
    print(f"{name}: rays with an event {hit.sum(1).tolist()}, with a second layer {second.tolist()}, open at the end {open_end.tolist()}, "
          f"entering at sample 0 {at_zero.tolist()}, most events on a ray {int(count.max())}")
    if name == "render_lego_val":
        t3 = [M_THRES.index(m) for m in T3]
        assert second[t3].min() >= 30 and ((count[t3] >= 2) == hit[t3]).all()            # every ray that hits has an exit
    else:
        assert open_end[0] >= 5 and at_zero[0] >= 5


def test_dex_thickness_on_a_hand_made_result():
    import nerf
    nan = float("nan")
    events = torch.tensor([[[2.0, 2.5, 3.0, float("inf")], [2.25, 2.5, 4.0, 4.0], [3.0, 3.5, float("inf"), float("inf")],
                            [2.0, 2.0, 5.0, 5.5]]]).permute(0, 2, 1).contiguous()         # (K=1, 2L=4, N=4)
    count = torch.tensor([[1, 3, 0, 7]], dtype=torch.int32)
    events[0, :, 2] = float("inf")
    events[0, 1:, 0] = float("inf")
    res = nerf.DexLayers(None, None, None, events, count, None)
    first, second = nerf.dex_thickness(res), nerf.dex_thickness(res, layer=1)
    assert first.shape == second.shape == (1, 4)
    np.testing.assert_array_equal(first.numpy(), np.array([[nan, 0.25, nan, 0.0]], F32))   # an open layer and a miss have no thickness
    np.testing.assert_array_equal(second.numpy(), np.array([[nan, nan, nan, 0.5]], F32))
    shaped = nerf.DexLayers(None, None, None, events.reshape(1, 4, 2, 2), count.reshape(1, 2, 2), None)
    assert nerf.dex_thickness(shaped).shape == (1, 2, 2)
    for bad in (2, -1, 1.0, True):
        with pytest.raises(ValueError):
            nerf.dex_thickness(res, layer=bad)


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


N_PLANTED = 11   # nine planted rows and two random ones: three workgroups, the last one ragged (11 is no multiple of 4)


def planted_rays(s, k):
    """Eleven rays of s samples for thresholds(k).  `low` values lie below every threshold, `high` ones above every threshold, so the
    planted events are those of every threshold unless said otherwise.  Rows: 0 nothing above; 1 everything above (an entry at 0, an
    open end); 2 alternating every sample (count = s); 3, 4, 5 two samples above from sample 63, 64, 65 on (an event at the first, the
    second and the last-but-one lane of a chunk edge); 6 NaN, +inf and -inf next to crossings; 7 two equal depths at an entry and at an
    exit; 8 densities equal to the middle threshold (above for the thresholds below it only); 9, 10 random around the thresholds."""
    gen = np.random.default_rng(1000 * s + k)
    m = thresholds(k)
    n = N_PLANTED
    z = (np.linspace(2.0, 6.0, s)[None, :] + 0.01 * gen.random((n, s))).astype(F32)
    low = lambda *shape: (-2.0 + 2.5 * gen.random(shape)).astype(F32)    # noqa: E731  in [-2, 0.5): below m_0 = 1
    top = float(m[-1])
    high = lambda *shape: (top + 0.5 + 3.0 * gen.random(shape)).astype(F32)   # noqa: E731
    sig = low(n, s)
    sig[1] = high(s)
    sig[2, 0::2] = high(len(sig[2, 0::2]))

    def put(row, j, value):
        if 0 <= j < s:
            sig[row, j] = value
    for row, p in ((3, 63), (4, 64), (5, 65)):
        put(row, p, high(1)[0])
        put(row, p + 1, high(1)[0])
    a = s // 3
    for off, value in enumerate((np.nan, np.inf, -np.inf, high(1)[0], np.nan, low(1)[0], np.inf, np.inf, np.nan)):
        put(6, a + off, value)
    c = s // 2
    put(7, c, high(1)[0])
    put(7, c + 1, high(1)[0])
    if c >= 1:
        z[7, c] = z[7, c - 1]                                            # a zero-width entry bracket
    if c + 2 < s:
        z[7, c + 2] = z[7, c + 1]                                        # a zero-width exit bracket
    for off in range(3):
        put(8, s // 4 + off, m[k // 2])                                  # s == m exactly: not above
    put(8, s // 4 + 4, high(1)[0])                                       # (one low sample between: a layer of its own)
    sig[9:] = (-1.0 + (top + 3.0) * gen.random((n - 9, s))).astype(F32)
    rd = gen.standard_normal((n, 3)).astype(F32)
    rf = gen.standard_normal((n, s, 4)).astype(F32)
    rf[..., 3] = sig
    return rf, z, rd, m


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", [1, 2, 8])
@pytest.mark.parametrize("k", [1, 3, 65])
@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 130])
def test_layers_kernel_against_the_restatement_and_composite_density(dev, s, k, n_layers):
    from nerf import _ops
    rf, z, rd, m = planted_rays(s, k)
    count_want, br_want, mid_want, idx = layers_restatement(rf[..., 3], z, m, n_layers)
    assert (count_want[:, 0] == 0).all() and (count_want[:, 1] == 1).all() and (idx[1, :, 0] == 0).all()
    assert (count_want[:, 2] == s).all()                                   # alternating: every sample is an event
    if s == 130:                                                           # every planted case is there
        assert (idx[3, :, 0] == 63).all() and (idx[4, :, 0] == 64).all() and (idx[5, :, :2] == (65, 67)).all()
        assert (count_want[:, 2] > 2 * n_layers).all()
        assert np.isnan(br_want[6, ..., 2]).any() and np.isposinf(br_want[6, ..., 3]).any() and np.isneginf(br_want[6, :, 1, 2]).all()
        assert (br_want[7, :, 0, 0] == br_want[7, :, 0, 1]).all() and (idx[7, :, 0] >= 1).all()
        assert n_layers == 1 or (br_want[7, :, 1, 0] == br_want[7, :, 1, 1]).all()
        assert k == 1 or (count_want[: k // 2, 8] > count_want[k // 2, 8]).all()          # s == m: above for the lower thresholds alone
    thres = G(m, dev)
    with torch.no_grad():
        depth0, acc0, dex0 = _ops.composite_density(G(rf, dev), G(z, dev), G(rd, dev), None, 0.0, thres)
        depth, acc, dex, br, z_mid, count = _ops.composite_density_layers(G(rf, dev), G(z, dev), G(rd, dev), thres, n_layers)
    assert same_bits(depth, depth0) and same_bits(acc, acc0) and same_bits(dex, dex0)
    assert br.shape == (N_PLANTED, k, 2 * n_layers, 4) and z_mid.shape == (N_PLANTED, k * 2 * n_layers) and count.shape == (k, N_PLANTED)
    assert same_ints(count, count_want), (C(count), count_want)
    assert same_bits(br, br_want), (C(br), br_want)
    assert same_bits(z_mid, mid_want)
    hit = count_want > 0
    assert same_bits(C(dex)[hit], br_want[:, :, 0, 1].T[hit])               # event 0's hi end is the Dex depth


def planted_records(n, k, n_layers, seed):
    """Records (n,k,2L,4) of every kind and their thresholds: exits with the deeper end first."""
    gen = np.random.default_rng(seed)
    m = thresholds(k)
    shape = (n, k, 2 * n_layers)
    m3 = np.broadcast_to(m[None, :, None], shape)
    near = (2.0 + 3.0 * gen.random(shape)).astype(F32)
    far = (near + F32(0.001) + F32(0.06) * gen.random(shape).astype(F32)).astype(F32)
    odd = np.broadcast_to((np.arange(2 * n_layers) % 2 == 1)[None, None, :], shape)
    lo, hi = np.where(odd, far, near), np.where(odd, near, far)
    s_lo = (m3 - 3.0 * gen.random(shape)).astype(F32)
    s_hi = (m3 + 0.01 + 30.0 * gen.random(shape)).astype(F32)
    br = np.stack([lo, hi, s_lo, s_hi], -1).astype(F32)
    kind = gen.integers(0, 8, shape)
    kind.reshape(-1)[:8] = np.arange(8)[: kind.size]                     # every kind at least once where there is room
    first, none, adjacent, nan_lo, inf_hi, at_m = (kind == i for i in range(6))
    br[first, 1], br[first, 2] = br[first, 0], br[first, 3]               # (z_0, z_0, s_0, s_0)
    br[none, 1], br[none, 2], br[none, 3] = br[none, 0], INF, -INF
    br[adjacent, 1] = np.nextafter(br[adjacent, 0], np.where(odd, -INF, INF)[adjacent])   # a bracket of two adjacent floats
    br[nan_lo, 2] = np.nan
    br[inf_hi, 3] = np.inf
    br[at_m, 2] = m3[at_m]                                                # s_lo == m: t = 0
    return br, m


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,n_layers", [(1, 1, 1), (67, 3, 2), (5, 65, 8)])
def test_finish_kernel_against_the_float64_restatement(dev, n, k, n_layers):
    from nerf import _ops
    br, m = planted_records(n, k, n_layers, 11 * n + k)
    br[0, 0, 0] = (2.0, 3.0, 0.0, 4.0)                                    # closed forms, threshold m_0 = 1
    br[0, 0, 1] = (4.0, 3.0, -1.0, 3.0)
    thres = G(m, dev)
    for interp in (False, True):
        with torch.no_grad():
            events, width = _ops.dex_layers_finish(G(br, dev), thres, interp)
            only, nothing = _ops.dex_layers_finish(G(br, dev), thres, interp, want_width=False)
        want_e, want_w = finish_restatement(br, m, interp)
        assert events.shape == (k, 2 * n_layers, n) and same_bits(events, want_e) and same_bits(width, want_w)
        assert nothing is None and same_bits(only, events)                # width = NULL
        assert C(events)[0, :2, 0].tolist() == ([2.25, 3.5] if interp else [3.0, 4.0]) and C(width)[0, :2, 0].tolist() == [1.0, 1.0]
        if n * k * n_layers >= 4:
            none = br[..., 3] == -INF
            assert none.any() and (br[..., 0] == br[..., 1])[~none].any()
            assert np.isposinf(C(events).transpose(2, 0, 1)[none]).all() and (C(width).transpose(2, 0, 1)[none] == -1.0).all()
    closed = np.array([[[[2.0, 3.0, -1.0, np.inf], [3.0, 2.0, np.nan, 4.0], [2.5, 2.5, 7.0, 7.0], [2.5, 2.5, np.inf, -np.inf]]],
                       [[[2.0, 4.0, 1.0, 2.0], [4.0, 2.0, -1.0, 3.0], [2.0, 2.0, np.inf, -np.inf], [2.0, 2.0, np.inf, -np.inf]]]], F32)   # (2,1,4,4)
    with torch.no_grad():
        e1, w1 = _ops.dex_layers_finish(G(closed, dev), G(thresholds(1), dev), True)
        e0, w0 = _ops.dex_layers_finish(G(closed, dev), G(thresholds(1), dev), False)
    inf = float("inf")
    assert C(e1)[0].T.tolist() == [[2.5, 2.5, 2.5, inf], [2.0, 3.0, inf, inf]]     # a non-finite end: the midpoint; s_lo == m: z_lo
    assert C(w1)[0].T.tolist() == [[1.0, 1.0, 0.0, -1.0], [2.0, 2.0, -1.0, -1.0]]
    assert C(e0)[0].T.tolist() == [[3.0, 3.0, 2.5, inf], [4.0, 4.0, inf, inf]]     # an entry's hi end, an exit's lo end
    assert C(w0)[0].T.tolist() == [[1.0, 1.0, 0.0, -1.0], [2.0, 2.0, -1.0, -1.0]]


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


def ray_rows(name, g, dev):
    from nerf import _ops
    rkw = CASES[name][2]
    return _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), None, rkw["near"], rkw["far"])


def layers_render(name, g, dev, cfg=None, thres=T3, **kw):
    import nerf
    mc, mf = models_of(name, dev)
    with torch.no_grad():
        return nerf.render_dex_layers(1, len(g["ro"]), 1.0, mc, mf, G(g["ro"], dev)[None], G(g["rd"], dev)[None], cfg or make_cfg(CASES[name][2]),
                                      mode="validation", encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(thres), **kw)


def chain(packs, rays, nc, nf, thres, n_layers, steps):
    """The layers render from the older entry points and the two standalone new ones; steps None: sample mode."""
    from nerf import _ops
    pc, pf = packs
    rd = rays[:, 3:6]
    with torch.no_grad():
        z = _ops.coarse_depths(rays, nc, False)
        rf = _ops.run_network_rays(pc, rays, z)
        depth_c, acc_c, z = _ops.density_resample(rf, z, rd, nf)
        rf = _ops.run_network_rays(pf, rays, z)
        depth, acc, dex, br, z_mid, count = _ops.composite_density_layers(rf, z, rd, thres, n_layers)
        br0 = br.clone()
        n, k = br.shape[0], br.shape[1]
        records, repeated = br.view(n, k * 2 * n_layers, 4), thres.repeat_interleave(2 * n_layers)
        for _ in range(steps or 0):
            z_mid = _ops.dex_bisect(records, _ops.run_network_rays(pf, rays, z_mid), repeated)
        events, width = _ops.dex_layers_finish(br, thres, steps is not None)
    return dict(maps=(depth_c, acc_c, depth, acc, dex, events, count, width), br=br, br0=br0, z=z, rf=rf)


@pytest.fixture(scope="module")
def lego_chain(golden, dev):
    """The fp32 chain on the lego rays, 64+64, thresholds (5, 20, 60), two layers, sample mode: depths, field and sample records -
    shared and left unchanged."""
    from nerf import _hip
    name = "render_lego_val"
    mc, mf = models_of(name, dev)
    packs = (mc.packed_density(precision=_hip.PREC_F32), mf.packed_density(precision=_hip.PREC_F32))
    rays = ray_rows(name, golden(name), dev)
    return packs, rays, chain(packs, rays, 64, 64, G(np.asarray(T3, F32), dev), 2, None)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_layers_driver_equals_the_chain_bit_for_bit(golden, dev, precision):
    from nerf import _hip, _ops
    name = "render_lego_val"
    prec = dict(fp32=_hip.PREC_F32, bf16=_hip.PREC_BF16)[precision]
    packs = tuple(m.packed_density(precision=prec) for m in models_of(name, dev))
    rays = ray_rows(name, golden(name), dev)
    th = G(np.asarray(T3, F32), dev)
    labels = ("depth_c", "acc_c", "depth_f", "acc_f", "dex", "events", "count", "width")
    for steps in (None, 0, 3):
        want = chain(packs, rays, 64, 64, th, 2, steps)
        with torch.no_grad():
            got = _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, th, 2, refine_steps=steps, want_width=True)
            short = _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, th, 2, refine_steps=steps)
            plain = _ops.render_rays_depth(*packs, rays, 64, 64, False, 0.0, th)
        assert len(got) == 8 and short[7] is None and same_bits(short[5], got[5]) and same_ints(short[6], got[6])
        for label, a, b in zip(labels, got, want["maps"]):
            assert same_ints(a, b) if label == "count" else same_bits(a, b), (precision, steps, label)
        for a, b in zip(plain, got):                                      # the maps ahead of the events are the plain render's
            assert same_bits(a, b)
        count = C(got[6])
        print(f"{precision} R={steps}: rays with an event {(count > 0).sum(1).tolist()}, with a second layer {(count >= 4).sum(1).tolist()}, "
              f"widest bracket {float(got[7].max()):.3e}")
        assert (count >= 4).any() and (C(got[7]) > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_event_zero_is_the_refined_dex_depth_and_the_maps_are_the_depth_renders(golden, dev, precision):
    import nerf
    from nerf import _hip, _ops
    name = "render_lego_val"
    g = golden(name)
    prec = dict(fp32=_hip.PREC_F32, bf16=_hip.PREC_BF16)[precision]
    packs = tuple(m.packed_density(precision=prec) for m in models_of(name, dev))
    rays = ray_rows(name, g, dev)
    th = G(np.asarray(T3, F32), dev)
    with torch.no_grad():
        got = _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, th, 2, refine_steps=3)
        sample = _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, th, 2)
        refined = _ops.render_rays_depth(*packs, rays, 64, 64, False, 0.0, th, refine_steps=3)
    hit = C(got[6]) > 0
    assert hit.any() and (~hit).any()
    assert same_bits(C(got[5])[:, 0][hit], C(refined[5])[hit])
    assert same_bits(C(sample[5])[:, 0][hit], C(refined[4])[hit])          # sample mode: the Dex depth
    assert np.isposinf(C(got[5])[:, 0][~hit]).all()
    # the public function: depth / acc / dex are render_dex_depth's maps
    nerf.set_precision(precision)
    mc, mf = models_of(name, dev)
    with torch.no_grad():
        maps = nerf.render_dex_depth(1, len(g["ro"]), 1.0, mc, mf, G(g["ro"], dev)[None], G(g["rd"], dev)[None], make_cfg(CASES[name][2]),
                                     mode="validation", encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(T3), refine_steps=3)
    res = layers_render(name, g, dev, layers=2, refine_steps=3, want_width=True)
    n = len(g["ro"])
    assert res.depth.shape == res.acc.shape == (1, n) and res.dex.shape == res.count.shape == (3, 1, n)
    assert res.events.shape == res.width.shape == (3, 4, 1, n) and res.count.dtype == torch.int32
    assert same_bits(res.depth, maps[2]) and same_bits(res.acc, maps[3])
    for t in range(3):
        assert same_bits(res.dex[t], maps[4 + t])
        hit_t = C(res.count[t]) > 0
        assert same_bits(C(res.events[t, 0])[hit_t], C(maps[7 + t])[hit_t])
    assert layers_render(name, g, dev, layers=2).width is None
    several = layers_render(name, g, dev, cfg=make_cfg(CASES[name][2], chunksize=50), layers=2, refine_steps=3, want_width=True)
    for a, b in zip(res, several):                                        # the maps do not depend on the chunking
        assert same_ints(a, b) if a.dtype == torch.int32 else same_bits(a, b)


@pytest.mark.gpu
def test_render_dex_layers_follows_the_render_policy(golden, dev):
    import warnings

    import nerf
    name = "render_d8w256_val"
    g = golden(name)
    kw = dict(layers=2, refine_steps=3, want_width=True)
    nerf.set_precision("fp16")
    ref16 = layers_render(name, g, dev, **kw)
    nerf.set_precision("bf16")
    nerf.set_render_policy("bf16")
    pure = layers_render(name, g, dev, **kw)
    nerf.set_render_policy(None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pol = layers_render(name, g, dev, **kw)
    for a, b in zip(pol, ref16):                                          # the default policy: guarded fp16
        assert same_ints(a, b) if a.dtype == torch.int32 else same_bits(a, b)
    assert not same_bits(pol.events, pure.events)
    stored = np.arange(4)[None, :, None, None] < np.minimum(C(pol.count), 4)[:, None]
    assert stored.any() and np.isfinite(C(pol.events)[stored]).all() and np.isposinf(C(pol.events)[~stored]).all()
    # train mode: flat maps
    mc, mf = models_of(name, dev)
    with torch.no_grad():
        flat = nerf.render_dex_layers(1, len(g["ro"]), 1.0, mc, mf, G(g["ro"], dev), G(g["rd"], dev), make_cfg(CASES[name][2]), mode="train",
                                      encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(T3), **kw)
    n = len(g["ro"])
    assert flat.depth.shape == (n,) and flat.dex.shape == flat.count.shape == (3, n) and flat.events.shape == flat.width.shape == (3, 4, n)
    assert same_bits(flat.events, pol.events.reshape(3, 4, n)) and same_ints(flat.count, pol.count.reshape(3, n))


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 5])
def test_events_stay_in_their_sample_brackets_and_the_widths_halve(dev, lego_chain, steps):
    """The bound on a width after R steps: the midpoint lo + 0.5f (hi - lo) is off the true one by at most half an ulp of the depth (the
    difference and the halving are exact for ends this close, the sum rounds once), so a half is at most w / 2 + ulp / 2 wide, and
    after R steps the excess over w_0 2^-R is ulp (1 - 2^-R) < 1 ulp of the depth."""
    from nerf import _ops
    packs, rays, ch = lego_chain
    th = G(np.asarray(T3, F32), dev)
    with torch.no_grad():
        out = _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, th, 2, refine_steps=steps, want_width=True)
    events, count, width = C(out[5]), C(out[6]), C(out[7])
    br0 = C(ch["br0"])
    count_want, br_want, _, idx = layers_restatement(C(ch["rf"])[..., 3], C(ch["z"]), T3, 2)
    assert same_bits(br0, br_want) and same_ints(count, count_want)       # the chain's sample records are the restatement's
    lo = np.minimum(br0[..., 0], br0[..., 1]).transpose(1, 2, 0)
    hi = np.maximum(br0[..., 0], br0[..., 1]).transpose(1, 2, 0)
    w0 = hi - lo
    at = idx.transpose(1, 2, 0)
    proper = (at >= 1) & (w0 > 0)
    assert proper[:, 1].mean() >= 0.25 and proper[:, 2].sum() >= 30 and proper[:, 3].sum() >= 30
    assert (events[proper] >= lo[proper]).all() and (events[proper] <= hi[proper]).all()
    bound = w0.astype(np.float64) * 2.0 ** -steps + np.spacing(hi).astype(np.float64)
    assert (width[proper] <= bound[proper]).all(), float((width - bound)[proper].max())
    assert (width[proper] > 0).all()
    np.testing.assert_array_equal(width == -1.0, at < 0)
    np.testing.assert_array_equal(width == 0.0, (at == 0) | ((at >= 1) & (w0 == 0)))
    assert (events[:, 1:] >= events[:, :-1]).all()
    print(f"R={steps}: {int(proper.sum())} proper brackets, widest sample bracket {w0[proper].max():.3e}, widest last {width[proper].max():.3e}")


def oracle_sigma(sd, mc, ro, rd, z):
    """Raw density of the CPU oracle at ro + rd z, fp32: z (P, J) for P rays -> (P, J)."""
    from oracle import nerf_oracle as oc
    ro, rd, z = torch.from_numpy(ro), torch.from_numpy(rd), torch.from_numpy(np.ascontiguousarray(z, F32))
    pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
    with torch.no_grad():
        return oc.run_network(sd, pts, rd, mc)[..., 3].numpy()


@pytest.mark.gpu
def test_event_accuracy_against_dense_oracle_truth(golden, dev):
    """fp32, render_lego_val, thresholds (5, 20, 60), two layers, 8 steps, 513 dense oracle evaluations from the lo end to the hi end
    of every event's sample bracket; a bracket whose dense evaluation does not change state exactly once is left out.  Measured on an
    MI355X: 722 proper brackets (261 / 261 / 100 / 100 per event), 30 left out (0.042); |z - truth| median / p99: entries sample 1.0e-3 /
    5.8e-2, GPU 9.7e-8 / 1.9e-6, oracle 1.0e-7 / 1.9e-6; exits sample 1.7e-2 / 6.2e-2, GPU 1.9e-7 / 2.3e-5, oracle 1.9e-7 / 2.3e-5; worst
    excess of the GPU over the oracle 2.4e-7 (gate 1e-4)."""
    from nerf import _hip, _ops
    from oracle import nerf_oracle as oc
    name = "render_lego_val"
    g = golden(name)
    steps, dense, n_layers = 8, 513, 2
    m = np.asarray(T3, F32)
    s, z = g["rf_fine"][..., 3], g["z_fine"]
    n, k, e2 = len(z), len(m), 2 * n_layers
    count_want, br_want, mid_want, idx = layers_restatement(s, z, m, n_layers)
    m_rec = np.broadcast_to(m[None, :, None], (n, k, e2))
    th = G(m, dev)
    pf = models_of(name, dev)[1].packed_density(precision=_hip.PREC_F32)
    rays = ray_rows(name, g, dev)
    with torch.no_grad():
        _, _, _, br, z_mid, count = _ops.composite_density_layers(G(g["rf_fine"], dev), G(z, dev), G(g["rd"], dev), th, n_layers)
        assert same_bits(br, br_want) and same_bits(z_mid, mid_want) and same_ints(count, count_want)
        z_sample = C(_ops.dex_layers_finish(br, th, False)[0]).transpose(2, 0, 1)            # (N,K,2L)
        records, repeated = br.view(n, k * e2, 4), th.repeat_interleave(e2)
        for _ in range(steps):
            z_mid = _ops.dex_bisect(records, _ops.run_network_rays(pf, rays, z_mid), repeated)
        z_gpu = C(_ops.dex_layers_finish(br, th, True)[0]).transpose(2, 0, 1)
    # the same algorithm on the oracle network
    mc = oc.ModelCfg(**CASES[name][0])
    sd = oc.to_torch_sd(lego_weights()[1])
    bo, mo = br_want, mid_want.reshape(n, k, e2)
    for _ in range(steps):
        bo, mo = bisect_restatement(bo, oracle_sigma(sd, mc, g["ro"], g["rd"], mo.reshape(n, k * e2)).reshape(n, k, e2), m_rec)
    z_oracle = finish_restatement(bo, m, True)[0].transpose(2, 0, 1)
    # truth: the one state change among 513 dense oracle evaluations from the lo end (not above) to the hi end (above), interpolated
    triples = np.argwhere((idx >= 1) & (br_want[..., 0] != br_want[..., 1]))
    r, t, e = triples[:, 0], triples[:, 1], triples[:, 2]
    lo, hi = br_want[r, t, e, 0].astype(np.float64), br_want[r, t, e, 1].astype(np.float64)
    zd = (lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, dense)[None, :]).astype(F32)
    sdense = oracle_sigma(sd, mc, g["ro"][r], g["rd"][r], zd).astype(np.float64)
    mt = m[t].astype(np.float64)
    above = sdense > mt[:, None]
    change = above[:, 1:] != above[:, :-1]
    kept = change.sum(-1) == 1
    j = 1 + change.argmax(-1)                                             # the dense point after the (first) change
    rows = np.arange(len(triples))
    s0, s1 = sdense[rows, j - 1], sdense[rows, j]
    z0, z1 = zd[rows, j - 1].astype(np.float64), zd[rows, j].astype(np.float64)
    with np.errstate(all="ignore"):
        z_true = z0 + (z1 - z0) * (mt - s0) / (s1 - s0)
    err = {label: np.abs(v[r, t, e].astype(np.float64) - z_true) for label, v in (("sample", z_sample), ("gpu", z_gpu), ("oracle", z_oracle))}
    left_out = float((~kept).mean())
    print(f"{name}: {len(triples)} proper event brackets over the four events ({[int((e == i).sum()) for i in range(e2)]}), {int((~kept).sum())} "
          f"left out (share {left_out:.3f}); worst excess of the GPU over the oracle {(err['gpu'] - err['oracle'])[kept].max():.2e}")
    for parity, label in ((0, "entries"), (1, "exits")):
        sel = kept & (e % 2 == parity)
        print(f"  {label} ({int(sel.sum())}): |z - truth| median / p99: " + ", ".join(
            f"{what} {np.median(err[what][sel]):.2e} / {np.quantile(err[what][sel], 0.99):.2e}" for what in ("sample", "gpu", "oracle")))
    assert len(triples) >= 600 and left_out <= 0.06
    assert (err["gpu"][kept] <= err["oracle"][kept] + 1e-4).all()
    exits = kept & (e % 2 == 1)
    assert exits.sum() >= 100 and np.median(err["gpu"][exits]) < np.median(err["sample"][exits])


_VIEW = {}


def view_24(dev):
    """The rays of a 24 x 24 synthetic camera -> (ro, rd) (24,24,3) on the device, and the lego networks."""
    import nerf
    from nerf import synthetic as syn
    if "v" not in _VIEW:
        e_mat = torch.from_numpy(syn.scene_pose(3)).to(dev)
        k_mat = torch.from_numpy(syn.intrinsic(24, 24)).to(dev)
        _VIEW["v"] = nerf.get_ray_bundle(24, 24, float(k_mat[0, 0]), e_mat, k_mat)
    return _VIEW["v"]


@pytest.mark.gpu
def test_a_full_occupancy_grid_and_a_ray_span_grid(dev):
    """occupancy= with every cell set (sample mode) returns the bits of the render without a grid; ray_span= equals calling the span
    kernel by hand and then rendering the chunk."""
    import nerf
    from nerf import _hip, _ops
    name = "render_lego_val"
    mc, mf = models_of(name, dev)
    ro, rd = view_24(dev)
    cfg = make_cfg(CASES[name][2])
    ex = nerf.get_embedding_function(10)

    def render(**kw):
        with torch.no_grad():
            return nerf.render_dex_layers(24, 24, 1.0, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex, m_thres_cand=list(T3),
                                          layers=2, want_width=True, **kw)
    want = render()
    assert want.events.shape == (3, 4, 24, 24) and want.count.shape == (3, 24, 24) and (C(want.count) >= 2).any()
    print(f"24 x 24 view: pixels with an event {(C(want.count) > 0).sum((1, 2)).tolist()}, with a second layer {(C(want.count) >= 4).sum((1, 2)).tolist()}")
    full = nerf.OccupancyGrid.from_mask(torch.ones(3, 5, 4, dtype=torch.bool, device=dev), (-12.0, -12.0, -12.0, 12.0, 12.0, 12.0))
    got = render(occupancy=full)
    for label, a, b in zip(want._fields, got, want):
        assert same_ints(a, b) if a.dtype == torch.int32 else same_bits(a, b), label
    with pytest.raises(ValueError):
        render(occupancy=full, refine_steps=2)
    # ray_span=: the rows tightened by hand, then the chunk entry point
    mask = np.zeros((8, 7, 6), bool)
    mask[2:6, 1:6, 1:5] = True
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0))
    spanned = render(ray_span=grid, ray_span_pad=0.5, refine_steps=2)
    rows = _ops.pack_ray_rows(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), None, 2.0, 6.0)
    before = rows.clone()
    _, visits = grid.ray_spans(rows, pad_cells=0.5, apply=True)
    assert (C(visits) > 0).any() and not same_bits(rows, before)           # the tightening did tighten
    packs = tuple(m.packed_density(precision=_hip.PREC_F32) for m in (mc, mf))
    with torch.no_grad():
        maps = _ops.render_rays_depth_layers(*packs, rows, 64, 64, False, 0.0, G(np.asarray(T3, F32), dev), 2, refine_steps=2, want_width=True)
    assert same_bits(spanned.depth.reshape(-1), maps[2]) and same_bits(spanned.acc.reshape(-1), maps[3])
    assert same_bits(spanned.dex.reshape(3, -1), maps[4]) and same_bits(spanned.events.reshape(3, 4, -1), maps[5])
    assert same_ints(spanned.count.reshape(3, -1), maps[6]) and same_bits(spanned.width.reshape(3, 4, -1), maps[7])
    assert not same_bits(spanned.events, render(refine_steps=2).events)


@pytest.mark.gpu
def test_layers_render_is_hipgraph_capturable(dev, lego_chain):
    """dn_render_rays_depth_layers neither allocates nor reads back: a captured chunk replays to the eager outputs bit for bit."""
    from nerf import _ops
    packs, rays, _ = lego_chain
    thres = G(np.asarray(T3, F32), dev)
    run = lambda: _ops.render_rays_depth_layers(*packs, rays, 64, 64, False, 0.0, thres, 2, refine_steps=4, want_width=True)  # noqa: E731
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
    for a, b in zip(eager, captured):
        assert same_ints(a, b) if a.dtype == torch.int32 else same_bits(a, b)
    assert (C(eager[6]) >= 4).any()


@pytest.mark.gpu
def test_eval_driver_dex_layers(dev, tmp_path):
    """eval_nerf.py --depth-only --m-thres --dex-layers L [--dex-refine R] [--dex-refine-width]: dex_events / dex_event_count
    (/ dex_event_width) beside dex in dex_<view>.npz."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "1", "--num-fine", "64", "--precision", "fp32", "--quiet", "--depth-only",
              "--m-thres", "10"]
    out = tmp_path / "out"
    eval_nerf.main(common + ["--dex-layers", "2", "--dex-refine", "4", "--savedir", str(out)])
    maps = np.load(out / "dex_0000.npz")
    assert sorted(maps.files) == ["depth", "dex", "dex_event_count", "dex_events", "dex_refine_steps", "dex_refined", "m_thres"]
    k = maps["dex"].shape[0]
    assert maps["dex_events"].shape == (k, 4, 24, 24) and maps["dex_event_count"].shape == (k, 24, 24)
    assert maps["dex_event_count"].dtype == np.int32
    hit = maps["dex_event_count"] > 0
    assert hit.any() and np.array_equal(maps["dex_events"][:, 0][hit], maps["dex_refined"][hit])
    assert np.isposinf(maps["dex_events"][:, 0][~hit]).all()
    wide = tmp_path / "wide"
    eval_nerf.main(common + ["--dex-layers", "1", "--dex-refine-width", "--savedir", str(wide)])
    sample = np.load(wide / "dex_0000.npz")
    assert sorted(sample.files) == ["depth", "dex", "dex_event_count", "dex_event_width", "dex_events", "m_thres"]
    assert sample["dex_events"].shape == sample["dex_event_width"].shape == (k, 2, 24, 24)
    assert np.array_equal(sample["dex_events"][:, 0][hit], maps["dex"][hit]) and np.array_equal(sample["dex_event_count"], maps["dex_event_count"])
    plain = tmp_path / "plain"
    eval_nerf.main(common + ["--savedir", str(plain)])
    assert sorted(np.load(plain / "dex_0000.npz").files) == ["depth", "dex", "m_thres"]
    assert np.array_equal(np.load(plain / "dex_0000.npz")["dex"], maps["dex"])
