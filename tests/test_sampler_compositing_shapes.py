"""The inverse-CDF sampler (dn_sample_pdf, dn_fine_depths) and the forward compositing (dn_volume_render) at every width at which
their code takes another path: the four length-dependent paths of aten_order_sum, the carry of the fp64 cdf scan between 64-wide
chunks, the merge path's register rows and its fall-back to the bitonic sort, the 64-sample chunks of the compositing scan and the
Dex readout's found mask / chunk maximum / "lane k tracks threshold k".

Yardsticks: oracle/exact_sampler.py (numpy, bit for bit; guarded here against oracle.nerf_oracle.sample_pdf on torch CPU) and
oracle.nerf_oracle.volume_render in float64.  Sampler results and Dex depths are compared with assert_array_equal; the compositing
outputs with the project's norm, max|a - b| <= tol * max|b| per tensor (conftest.rel_err)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_ray_gradients import C, render_inputs

F = np.float32
N_SAMPLER = 9    # three workgroups of four waves: the last one has one live wave and three clamped ones
N_COMPOSITE = 5

# n_bins of dn_sample_pdf; L = n_bins - 1 is the width of the weights row
WIDTHS = (9,      # L 8: the minimum - one vector, no group, no tail
          10,     # L 9: tail of 1
          16,     # L 15: tail of 7
          33,     # L 32: exactly one group of four vectors
          41,     # L 40: one group plus one left-over vector
          64,     # L 63: just under one scan chunk
          65,     # L 64: one scan chunk exactly
          66,     # L 65: two scan chunks - the first carry
          129,    # L 128: two full scan chunks, no tail
          257,    # L 256: four full scan chunks
          512)    # L 511: the maximum - 15 groups, 3 vectors, tail 7, 8 scan chunks
NFS = (1, 63, 64, 65, 200)

# (nc, nf) of dn_fine_depths
FINE_SHAPES = ((10, 1),        # the minimum
               (64, 128),      # the baseline
               (65, 64),       # the merge path's second coarse register row
               (256, 512),     # the merge path's upper limit
               (257, 64),      # one past the coarse limit: ordered inputs take the bitonic sort
               (64, 513),      # one past the fine limit
               (100, 93),      # 193 depths padded to 256
               (128, 256),
               (512, 1536))    # the maximum: sort_len 2048
U_MODES = ("deterministic", "ascending", "unordered")


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- inputs and references, built once per shape and read-only ----------------------------------------------------------------------
def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def planted_u(cdf, nf, seed):
    """u (rows, nf) in [0, 1) with, per row, u == 0, u == 1, u bitwise equal to an interior cdf entry of that row (the
    side="right" case: the entry itself counts) and the float just below it - in columns 0..3, or, when nf < 4, one of the four in
    column 0, a different one from row to row."""
    rng = np.random.default_rng(seed)
    n, b = cdf.shape
    u = rng.random((n, nf), dtype=F)
    for r in range(n):
        edge = cdf[r, 1 + (7 * r) % (b - 2)]      # interior: entries 1 .. b - 2
        plants = (F(0.0), F(1.0), edge, np.nextafter(edge, F(0.0)))
        if nf >= 4:
            u[r, :4] = plants
        else:
            u[r, 0] = plants[r % 4]
    return u


@functools.lru_cache(maxsize=None)
def sampler_case(n_bins, nf):
    """bins (9, n_bins) ascending in [2, 6], weights (9, n_bins - 1) in [0, 1), an injected u, and sample_pdf_exact's results for
    u = None (`det`) and for that u (`inj`).  Row 0: all-zero weights; rows 1-3: a delta pdf in the first, a middle and the last
    bin; row 4: weights <= 1e-6; row 5: two equal consecutive bin edges; rows 6-8: plain."""
    from oracle import exact_sampler as ex
    rng = np.random.default_rng(n_bins)
    width = n_bins - 1
    bins = np.sort(2.0 + 4.0 * rng.random((N_SAMPLER, n_bins), dtype=F), -1)
    bins[5, n_bins // 2] = bins[5, n_bins // 2 - 1]
    w = rng.random((N_SAMPLER, width), dtype=F)
    w[0] = 0.0
    for row, at in ((1, 0), (2, width // 2), (3, width - 1)):
        w[row] = 0.0
        w[row, at] = 1.0
    w[4] *= F(1e-6)
    assert bins.dtype == F and w.dtype == F and float(w[4].max()) <= 1e-6
    det = ex.sample_pdf_exact(bins, w, nf)
    u = planted_u(det["cdf"], nf, seed=1000 * n_bins + nf)
    inj = ex.sample_pdf_exact(bins, w, nf, u)
    return _frozen(bins=bins, w=w, u=u, det=_frozen(**det), inj=_frozen(**inj))


@functools.lru_cache(maxsize=None)
def fine_case(nc, nf):
    """z_coarse (9, nc) ascending in [2, 6], weights (9, nc), per u mode the u (None: deterministic) and the reference: samples =
    sample_pdf_exact on bins = 0.5f * (z[i+1] + z[i]) formed in fp32 and weights[:, 1:-1], z_fine = sort(cat(z_coarse, samples)).
    Row 0: all-zero weights; row 1: a delta weight; row 5: two equal consecutive coarse depths.  The ascending u is the sorted
    unordered one, which holds planted_u's 0, 1 and cdf entries."""
    from oracle import exact_sampler as ex
    rng = np.random.default_rng(10000 * nc + nf)
    z = np.sort(2.0 + 4.0 * rng.random((N_SAMPLER, nc), dtype=F), -1)
    z[5, nc // 2] = z[5, nc // 2 - 1]
    w = rng.random((N_SAMPLER, nc), dtype=F)
    w[0] = 0.0
    w[1] = 0.0
    w[1, nc // 2] = 1.0
    bins = F(0.5) * (z[:, 1:] + z[:, :-1])
    assert bins.dtype == F
    inner = np.ascontiguousarray(w[:, 1:-1])
    cdf = ex.sample_pdf_exact(bins, inner, nf)["cdf"]
    unordered = planted_u(cdf, nf, seed=77 * nc + nf)
    us = dict(deterministic=None, ascending=np.sort(unordered, -1), unordered=unordered)
    ref = {}
    for mode, u in us.items():
        res = ex.sample_pdf_exact(bins, inner, nf, u)
        ref[mode] = _frozen(cdf=res["cdf"], inds=res["inds"], samples=res["samples"],
                            z_fine=np.sort(np.concatenate([z, res["samples"]], -1), -1))
    if nf >= 4:   # u = 1 (the last bin edge) in front of an interior cdf entry: the samples really are out of order
        assert all((np.diff(ref["unordered"]["samples"][r]) < 0).any() for r in range(N_SAMPLER))
    return _frozen(z=z, w=w, bins=bins, inner=inner, us=_frozen(**{k: v for k, v in us.items() if v is not None}), ref=ref)


# ---- CPU: the yardstick -------------------------------------------------------------------------------------------------------------
def _assert_exact_equals_torch(bins, w, nf, u, exact, what):
    from oracle import nerf_oracle as oc
    tu = None if u is None else torch.tensor(u)
    samples, aux = oc.sample_pdf(torch.tensor(bins), torch.tensor(w), nf, det=True, u=tu, return_aux=True)
    np.testing.assert_array_equal(exact["cdf"], aux["cdf"].numpy(), err_msg=f"cdf {what}")
    np.testing.assert_array_equal(exact["inds"], aux["inds"].numpy(), err_msg=f"inds {what}")
    np.testing.assert_array_equal(exact["samples"], samples.numpy(), err_msg=f"samples {what}")


@pytest.mark.parametrize("n_bins", WIDTHS)
def test_exact_sampler_equals_torch_cpu_at_every_sampler_width(n_bins):
    """sample_pdf_exact == oracle.nerf_oracle.sample_pdf (torch CPU sum / cumsum / searchsorted(right=True)) bitwise in cdf,
    indices and samples, on the planted rows and the planted u of the GPU test below."""
    for nf in NFS:
        case = sampler_case(n_bins, nf)
        _assert_exact_equals_torch(case["bins"], case["w"], nf, None, case["det"], (n_bins, nf, "deterministic"))
        _assert_exact_equals_torch(case["bins"], case["w"], nf, case["u"], case["inj"], (n_bins, nf, "injected"))


@pytest.mark.parametrize("nc,nf", FINE_SHAPES)
def test_exact_sampler_equals_torch_cpu_at_every_fine_depths_shape(nc, nf):
    case = fine_case(nc, nf)
    for mode in U_MODES:
        _assert_exact_equals_torch(case["bins"], case["inner"], nf, case["us"].get(mode), case["ref"][mode], (nc, nf, mode))


@pytest.mark.parametrize("nf", [1, 2, 7, 64, 65, 128, 130, 513])
def test_linspace_f32_equals_torch_linspace(nf):
    from oracle import exact_sampler as ex
    np.testing.assert_array_equal(ex.linspace_f32(0.0, 1.0, nf), torch.linspace(0.0, 1.0, steps=nf, dtype=torch.float32).numpy())


def test_more_than_64_dex_thresholds_are_refused_before_gpu_work(hiplib):
    """n_thres = 65 -> DN_E_INVAL with the "at most 64 Dex thresholds" message; nothing is dereferenced or launched (the device
    pointers are small integers)."""
    from nerf import _hip
    fake = ctypes.c_void_p(256)
    rc = hiplib.dn_volume_render(fake, fake, fake, 3, None, 0.0, 0, _hip.host_floats([1.0] * 65), 65, 4, 8, fake, fake, fake, fake, fake,
                                 fake, None)
    assert rc == -1000
    assert b"at most 64 Dex thresholds" in hiplib.dn_last_error()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


def G(a, dev):
    return torch.tensor(a, device=dev)     # (a copy: the cached arrays are read-only)


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", WIDTHS)
def test_sample_pdf_bit_equal_to_the_exact_sampler(dev, n_bins):
    """dn_sample_pdf, 9 rays, nf in {1, 63, 64, 65, 200}, u = None (the kernel's own linspace) and the injected u: indices and
    samples bit-equal to sample_pdf_exact."""
    from nerf import _ops
    for nf in NFS:
        case = sampler_case(n_bins, nf)
        bins, w = G(case["bins"], dev), G(case["w"], dev)
        for u, ref, mode in ((None, case["det"], "deterministic"), (G(case["u"], dev), case["inj"], "injected")):
            samples, inds = _ops.sample_pdf(bins, w, nf, u, want_inds=True)
            np.testing.assert_array_equal(C(inds), ref["inds"], err_msg=f"inds n_bins={n_bins} nf={nf} u {mode}")
            np.testing.assert_array_equal(C(samples), ref["samples"], err_msg=f"samples n_bins={n_bins} nf={nf} u {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("nc,nf", FINE_SHAPES)
def test_fine_depths_bit_equal_to_the_sorted_concatenation(dev, nc, nf):
    """dn_fine_depths, 9 rays, with a deterministic, an injected ascending and an injected unordered u (the bitonic sort: the only
    way into it at the shapes inside the merge limits): the samples bit-equal to sample_pdf_exact's, the merged depths bit-equal to
    np.sort(concatenate(z_coarse, samples))."""
    from nerf import _ops
    case = fine_case(nc, nf)
    z, w = G(case["z"], dev), G(case["w"], dev)
    for mode in U_MODES:
        u = case["us"].get(mode)
        z_fine, zs = _ops.fine_depths(z, w, nf, None if u is None else G(u, dev), want_samples=True)
        np.testing.assert_array_equal(C(zs), case["ref"][mode]["samples"], err_msg=f"samples nc={nc} nf={nf} u {mode}")
        np.testing.assert_array_equal(C(z_fine), case["ref"][mode]["z_fine"], err_msg=f"z_fine nc={nc} nf={nf} u {mode}")


FWD_OUTPUTS = ("rgb", "disp", "acc", "weights", "depth")


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 128, 129, 384, 1000])
def test_volume_render_forward_against_the_float64_oracle(dev, s):
    """dn_volume_render, 5 rays (ray 2 dead: every sigma <= 0, disp NaN in the reference too; ray 1: two equal consecutive depths),
    white background on / off, injected noise (std 0.2) and none, rd contiguous and as the stride-11 view of the ray rows: rgb, disp,
    acc, weights, depth <= 1e-5 against oracle.volume_render in float64 on the same fp32 inputs; want_weights=False leaves the other
    outputs bit-equal."""
    from nerf import _ops
    from oracle import nerf_oracle as oc
    rf, z, rows, noise, _ = render_inputs(N_COMPOSITE, s, seed=200 + s, dead_ray=2)
    rf_d, z_d, rows_d, noise_d = rf.to(dev), z.to(dev), rows.to(dev), noise.to(dev)
    worst = dict.fromkeys(FWD_OUTPUTS, 0.0)
    for white in (False, True):
        for noise_std in (0.0, 0.2):
            ref = oc.volume_render(rf.double(), z.double(), rows[:, 3:6].double(), noise.double() if noise_std > 0.0 else None, noise_std,
                                   white, ())
            assert bool(torch.isnan(ref["disp"][2]))
            for stride in (3, 11):
                rd_d = rows_d[:, 3:6] if stride == 11 else rows_d[:, 3:6].contiguous()
                assert rd_d.stride(0) == stride
                nz = noise_d if noise_std > 0.0 else None
                out = dict(zip(FWD_OUTPUTS, _ops.volume_render_fwd(rf_d, z_d, rd_d, nz, noise_std, white, ())))
                lean = dict(zip(FWD_OUTPUTS, _ops.volume_render_fwd(rf_d, z_d, rd_d, nz, noise_std, white, (), want_weights=False)))
                assert lean["weights"] is None
                for name in FWD_OUTPUTS:
                    err = rel_err(C(out[name]), ref[name].numpy())
                    worst[name] = max(worst[name], err)
                    assert err <= 1e-5, (s, white, noise_std, stride, name, err)
                    if name != "weights":
                        np.testing.assert_array_equal(C(lean[name]), C(out[name]), err_msg=f"{name} without weights, S={s}")
    print(f"volume render forward S={s}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- the Dex depth -------------------------------------------------------------------------------------------------------------------
def threshold_lists(k):
    """K thresholds in (0, 30], the largest exactly 30: ascending, descending, with duplicates (each value twice, still K entries),
    with one negative."""
    base = np.linspace(0.5, 30.0, k).astype(F) if k > 1 else np.array([30.0], F)
    negative = base.copy()
    negative[k // 2] = F(-1.0)
    return dict(ascending=base, descending=base[::-1].copy(), duplicates=base[(np.arange(k) // 2) * 2].copy(), negative=negative)


DEX_RAYS = 2 * N_COMPOSITE
LOW, HIGH = F(-10.0), F(45.0)     # raw sigma: 0 after the relu / above every threshold, with or without noise (|noise * 0.2| < 5)


def dex_inputs(s):
    """10 rays (two launches of 5) of raw sigma against thresholds in (0, 30]:
    0 crossing at sample 0; 1 crossing only at sample S-1; 2, 3, 4 first crossing at sample 63, 64, 65 (the last sample where S is
    shorter), high from there on; 5 sigma == 30 (the largest threshold) bitwise at its only non-zero sample S//2, where the noise is
    zeroed: no crossing of that threshold, the comparison is strict; 6 no crossing at all; 7 a slow ramp raw_i = c i up to 30.2: the
    thresholds are first crossed in different chunks, the largest one in the last; 8 a spike in chunk 0, nothing behind it; 9 a
    spike in chunk 0, nothing, then high again over the last 20 samples: later chunks must not overwrite the first crossing."""
    rf, z, rows, noise, _ = render_inputs(DEX_RAYS, s, seed=300 + s)
    raw = np.full((DEX_RAYS, s), LOW, F)
    raw[0, 0] = HIGH
    raw[1, s - 1] = HIGH
    for ray, first in ((2, 63), (3, 64), (4, 65)):
        raw[ray, min(first, s - 1):] = HIGH
    raw[5, s // 2] = F(30.0)
    noise[5, s // 2] = 0.0
    raw[7] = (F(30.2) / F(s - 1)) * np.arange(s, dtype=F)
    raw[8, 3:40] = HIGH
    raw[9, 3:40] = HIGH
    raw[9, s - 20:] = HIGH
    rf[..., 3] = torch.from_numpy(raw)
    return rf, z, rows, noise


def dex_reference(raw, noise, noise_std, z, thresholds):
    """(K, N): z[first i with sigma_i > m], z[0] if there is none; sigma = max(raw + noise * std, 0) in fp32, rounded as the kernel
    rounds it (the library is built with -ffp-contract=off)."""
    sigma = np.maximum(raw + noise * F(noise_std), F(0.0)) if noise_std > 0.0 else np.maximum(raw, F(0.0))
    assert sigma.dtype == F
    over = sigma[None, :, :] > thresholds[:, None, None]
    first = np.where(over.any(-1), over.argmax(-1), 0)
    return np.take_along_axis(np.broadcast_to(z, over.shape), first[..., None], -1)[..., 0], first


@pytest.mark.gpu
@pytest.mark.parametrize("s", [63, 64, 65, 129, 384])
def test_dex_depth_is_exact_at_chunk_edges_and_for_any_threshold_list(dev, s):
    """dn_volume_render's Dex readout, K in {1, 20, 64}, ascending / descending / duplicate / one-negative threshold lists, with
    and without noise, on the planted rays of dex_inputs: bit-equal to z[first i with sigma_i > m] for every ray and threshold."""
    from nerf import _ops
    rf, z, rows, noise = dex_inputs(s)
    raw_np, noise_np, z_np = rf[..., 3].numpy().copy(), noise.numpy(), z.numpy()
    rf_d, z_d, rd_d, noise_d = rf.to(dev), z.to(dev), rows.to(dev)[:, 3:6], noise.to(dev)
    for k in (1, 20, 64):
        for name, th in threshold_lists(k).items():
            for noise_std in (0.0, 0.2):
                ref, first = dex_reference(raw_np, noise_np, noise_std, z_np, th)
                if name == "ascending":      # the plants hold, with the noise too
                    assert (first[:, 0] == 0).all() and (first[:, 1] == s - 1).all() and (first[:, 6] == 0).all()
                    assert [int(first[0, r]) for r in (2, 3, 4)] == [min(p, s - 1) for p in (63, 64, 65)]
                    assert first[-1, 5] == 0 and (first[:-1, 5] == s // 2).all()
                    assert (first[:, 8] == 3).all() and (first[:, 9] == 3).all()
                    if k > 1 and s > 64 and noise_std == 0.0:
                        assert first[0, 7] < 64 and first[-1, 7] // 64 == (s - 1) // 64
                for lo in range(0, DEX_RAYS, N_COMPOSITE):
                    sl = slice(lo, lo + N_COMPOSITE)
                    dex = _ops.volume_render_fwd(rf_d[sl], z_d[sl], rd_d[sl], noise_d[sl] if noise_std > 0.0 else None, noise_std, False,
                                                 [float(m) for m in th])[5]
                    np.testing.assert_array_equal(C(dex), ref[:, sl], err_msg=f"Dex depth S={s} K={k} {name} noise {noise_std} rays {lo}+")
