"""A ray's near / far tightened to the occupied span of the occupancy grid (include/dexnerf_hip_span.h, nerf.OccupancyGrid.ray_spans,
ray_span= on nerf.render_dex_depth, nerf.render_dex_normals and nerf.run_one_iter_of_nerf).

The kernel is pinned bit for bit to a numpy restatement of the header's text (restate_spans).  The restatement itself is pinned, without
a GPU, to a float64 geometric truth (the cells of the midpoints of the segments between sorted boundary crossings) and to the
classification rule of the culled renders (every sample that rule keeps lies inside the span).  The renders are pinned bit for bit to
the chunk entry points of nerf._ops on rows whose columns 6 and 7 the restatement wrote.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from golden_cases import CASES, D4, lego_weights

SPAN = ("dn_occupancy_ray_spans",)
INVAL = -1000
NC, NF = 37, 22                      # the smallest coarse / fine counts tests/test_depth_render.py uses (RESAMPLE_CASES)
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
ODD_BOX = (-1.25, -0.5, 0.125, 1.0, 1.75, 2.5)
M_THRES = (5.0, 20.0, 60.0)
F = np.float32


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def grid_scale(bounds, cells):
    b = np.asarray(bounds, F)
    return np.array([F(cells[a] / (float(b[a + 3]) - float(b[a]))) for a in range(3)], F)


def restate_spans(rays, bounds, cells, mask, pad_cells):
    """The header's definition, all rays at once -> (span (N,2) fp32, visits (N) int32, whether a walk was still going after
    cx + cy + cz + 1 rounds (N) bool).  Every product and sum is one fp32 numpy operation: two roundings, as without FMA."""
    rays = np.asarray(rays, F)
    mask = np.asarray(mask, bool)
    n = rays.shape[0]
    cells_i = np.asarray(cells, np.int64)
    b0, s, c = np.asarray(bounds, F)[:3], grid_scale(bounds, cells), np.asarray(cells, F)
    near, far = rays[:, 6].copy(), rays[:, 7].copy()
    with np.errstate(all="ignore"):
        miss = ~np.isfinite(rays[:, :8]).all(axis=1)
        o = (rays[:, 0:3] - b0) * s
        d = rays[:, 3:6] * s
        assert o.dtype == F and d.dtype == F
        zero = d == 0
        miss |= (zero & ~((o >= 0) & (o < c))).any(axis=1)
        inv = F(1.0) / np.where(zero, F(1.0), d)                      # (an axis with d == 0 never reads its inv)
        t_in, t_out = near.copy(), far.copy()
        for a in range(3):
            ta, tb = (F(0) - o[:, a]) * inv[:, a], (c[a] - o[:, a]) * inv[:, a]
            fwd = ta <= tb
            lo_a, hi_a = np.where(fwd, ta, tb), np.where(fwd, tb, ta)
            t_in = np.where(~zero[:, a] & (lo_a > t_in), lo_a, t_in)
            t_out = np.where(~zero[:, a] & (hi_a < t_out), hi_a, t_out)
        miss |= ~(t_in < t_out)
        p = o + d * t_in[:, None]
        fl = np.floor(p)
        fl = np.where(F(0) > fl, F(0), fl)                            # max(floorf(p), 0)
        fl = np.where((c - F(1)) < fl, c - F(1), fl)                  # min(.., c - 1)
        i = np.clip(np.nan_to_num(fl, nan=0.0).astype(np.int64), 0, cells_i - 1)
        pos = (d > 0).astype(np.int64)
        step = np.where(d > 0, 1, np.where(d < 0, -1, 0)).astype(np.int64)
        tn = np.where(zero, F(np.inf), ((i + pos).astype(F) - o) * inv).astype(F)
        t_cur = t_in.copy()
        active = ~miss
        count = np.zeros(n, np.int32)
        lo, hi = np.zeros(n, F), np.zeros(n, F)
        for _ in range(int(cells_i.sum()) + 1):
            if not active.any():
                break
            use1 = tn[:, 1] < tn[:, 0]
            t01 = np.where(use1, tn[:, 1], tn[:, 0])
            use2 = tn[:, 2] < t01
            tn_a = np.where(use2, tn[:, 2], t01)
            axis = np.where(use2, 2, np.where(use1, 1, 0))
            t_exit = np.where(t_out < tn_a, t_out, tn_a)
            bit = active & mask[i[:, 0], i[:, 1], i[:, 2]]
            lo = np.where(bit & (count == 0), t_cur, lo)
            hi = np.where(bit, t_exit, hi)
            count += bit
            rows = np.nonzero(active & (tn_a < t_out))[0]
            ax = axis[rows]
            moved = i[rows, ax] + step[rows, ax]
            left = (moved < 0) | (moved >= cells_i[ax])
            rows, ax, moved = rows[~left], ax[~left], moved[~left]
            i[rows, ax] = moved
            t_cur[rows] = tn_a[rows]
            tn[rows, ax] = ((moved + pos[rows, ax]).astype(F) - o[rows, ax]) * inv[rows, ax]
            active = np.zeros(n, bool)
            active[rows] = True
        ad = np.abs(d)
        dmax = np.where(ad[:, 1] > ad[:, 0], ad[:, 1], ad[:, 0])
        dmax = np.where(ad[:, 2] > dmax, ad[:, 2], dmax)
        pad = F(pad_cells) / dmax
        s0, s1 = lo - pad, hi + pad
        s0 = np.where(s0 > near, s0, near)
        s1 = np.where(s1 < far, s1, far)
        assert s0.dtype == F and s1.dtype == F
    hit = count > 0
    span = np.stack([np.where(hit, s0.view(np.uint32), near.view(np.uint32)), np.where(hit, s1.view(np.uint32), far.view(np.uint32))], axis=1)
    return np.ascontiguousarray(span).view(F), count, active


def apply_spans(rays, span, visits):
    """The rows `apply` leaves: columns 6 and 7 of the hit rows replaced, every other bit kept."""
    out = np.array(rays, F, copy=True)
    hit = visits > 0
    out[hit, 6:8] = span[hit]
    return out


def truth_spans(rays, bounds, cells, mask):
    """float64 geometry in the same cell coordinates -> (hit (N) bool, visits (N), lo (N), hi (N)): the ray's [near, far] clipped to
    the box, cut at every cell boundary it crosses, and the cell of each piece's midpoint looked up."""
    rays = np.asarray(rays, F).astype(np.float64)
    b0, s = np.asarray(bounds, F)[:3].astype(np.float64), grid_scale(bounds, cells).astype(np.float64)
    n = rays.shape[0]
    hit, visits, lo, hi = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n), np.zeros(n)
    for r in range(n):
        o, d = (rays[r, 0:3] - b0) * s, rays[r, 3:6] * s
        t0, t1 = rays[r, 6], rays[r, 7]
        inside = True
        cuts = []
        for a in range(3):
            if d[a] == 0.0:
                inside = inside and 0.0 <= o[a] < cells[a]
                continue
            t = (np.arange(cells[a] + 1) - o[a]) / d[a]
            t0, t1 = max(t0, min(t[0], t[-1])), min(t1, max(t[0], t[-1]))
            cuts.append(t)
        if not (inside and t0 < t1):
            continue
        cuts = np.concatenate(cuts) if cuts else np.zeros(0)
        ts = np.concatenate([[t0], np.sort(cuts[(cuts > t0) & (cuts < t1)]), [t1]])
        for a_t, b_t in zip(ts[:-1], ts[1:]):
            if not b_t > a_t:
                continue
            cell = np.clip(np.floor(o + d * (0.5 * (a_t + b_t))).astype(np.int64), 0, np.asarray(cells) - 1)
            if mask[cell[0], cell[1], cell[2]]:
                if not hit[r]:
                    lo[r] = a_t
                hit[r], hi[r] = True, b_t
                visits[r] += 1
    return hit, visits, lo, hi


def restate_kept(rays, z, bounds, cells, mask):
    """The classification rule of the culled renders (include/dexnerf_hip_occupancy.h, restated here): x = ro + rd * z in fp32, multiply
    then add; t = (x - b0) * s; kept iff 0 <= t < cells on every axis and the bit of cell (int)t is set -> (N,S) bool."""
    rays, z = np.asarray(rays, F), np.asarray(z, F)
    b0, s = np.asarray(bounds, F)[:3], grid_scale(bounds, cells)
    with np.errstate(invalid="ignore", over="ignore"):
        x = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
        t = (x - b0) * s
        assert t.dtype == F
        inside = ((t >= F(0)) & (t < np.asarray(cells, F))).all(axis=-1)
        idx = np.where(inside[..., None], t, F(0)).astype(np.int64)
    return inside & np.asarray(mask, bool)[idx[..., 0], idx[..., 1], idx[..., 2]]


def random_mask(cells, seed, share=0.3):
    return np.random.default_rng(seed).random(cells) < share


def random_rays(n, bounds, seed, stride=8):
    """Rows with origins inside (every second ray) and outside the box, aimed at a point of the box stretched a little past it (so some
    rays miss), directions of length 0.5 .. 2 with both signs, every tenth ray with one exactly zero direction component."""
    rng = np.random.default_rng(seed)
    b = np.asarray(bounds, np.float64)
    centre, half = 0.5 * (b[:3] + b[3:]), 0.5 * (b[3:] - b[:3])
    rows = rng.normal(0.0, 1.0, (n, stride)).astype(F)
    inside = np.arange(n) % 2 == 0
    origin = np.where(inside[:, None], centre + half * rng.uniform(-1, 1, (n, 3)),
                      centre + half * rng.uniform(1.2, 3.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)))
    target = centre + half * rng.uniform(-1.3, 1.3, (n, 3))
    direction = target - origin
    length = np.linalg.norm(direction, axis=1, keepdims=True)
    direction = direction / length * rng.uniform(0.5, 2.0, (n, 1))
    tenth = np.arange(n) % 10 == 9
    direction[tenth, rng.integers(0, 3, tenth.sum())] = 0.0
    near = rng.uniform(0.0, 0.5, n)
    rows[:, 0:3], rows[:, 3:6] = origin, direction
    rows[:, 6], rows[:, 7] = near, near + rng.uniform(1.0, 4.0, n) * np.linalg.norm(2 * half)
    return rows


CPU_GRIDS = [((5, 7, 9), BOX, 1), ((16, 16, 16), ODD_BOX, 2), ((40, 33, 17), BOX, 3)]


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_span_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_span.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.SPAN_EXPORTS) == set(SPAN)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS) | set(_hip.OCCUPANCY_EXPORTS) | set(_hip.CULL_EXPORTS) | set(_hip.REFINE_EXPORTS))
    assert not older & set(SPAN) and len(_hip.EXPORTS) == 76
    assert "dexnerf_hip_span.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()           # build() checks the new header's symbols too
    assert "occupancy_span.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in SPAN) and hiplib.dn_abi_version() == 2


def test_span_entry_point_judges_its_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    fake, odd = ctypes.c_void_p(256 * 4096), ctypes.c_void_p(256 * 4096 + 2)
    nan, inf = float("nan"), float("inf")
    call = dict(rays=fake, stride=8, n=37, bits=fake, cx=5, cy=4, cz=3, x0=-1.0, y0=-1.0, z0=-1.0, x1=1.0, y1=1.0, z1=1.0, sx=2.5, sy=2.0,
                sz=1.5, pad=1.0, apply=0, span=fake, visits=fake, stream=None)
    cells = (dict(cx=0), dict(cy=-1), dict(cz=0), dict(cx=(1 << 24) + 1), dict(cx=1 << 12, cy=1 << 12, cz=1 << 12), dict(cx=1 << 20, cy=1 << 20, cz=1))
    bounds = (dict(x0=nan), dict(y1=inf), dict(z0=-inf), dict(x0=1.0), dict(y0=2.0), dict(z1=-1.0), dict(sx=0.0), dict(sy=-1.0), dict(sz=nan),
              dict(sx=inf))
    pads = (dict(pad=nan), dict(pad=inf), dict(pad=-inf), dict(pad=-0.5))
    for kw in cells + bounds + pads + (dict(rays=None), dict(bits=None), dict(rays=odd), dict(bits=odd), dict(span=odd), dict(visits=odd),
                                       dict(stride=7), dict(stride=0), dict(stride=-8), dict(n=-1), dict(n=-(1 << 40)), dict(span=None),
                                       dict(span=None, visits=None), dict(n=0, pad=nan), dict(n=0, span=None)):
        assert hiplib.dn_occupancy_ray_spans(*{**call, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_ray_spans" in hiplib.dn_last_error(), kw
    # no rays: 0 after the checks, whatever the outputs - nothing is launched
    for kw in (dict(n=0), dict(n=0, visits=None), dict(n=0, apply=1, span=None, visits=None), dict(n=0, pad=0.0)):
        assert hiplib.dn_occupancy_ray_spans(*{**call, **kw}.values()) == 0, kw


def small_model(dev=None, which=1):
    import nerf
    m = nerf.models.FlexibleNeRFModel(**D4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lego_weights()[which].items()})
    return m if dev is None else m.to(dev)


def make_cfg(nc=NC, nf=NF, chunksize=4096, **over):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    mode.update(over)
    return nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def test_the_python_layer_refuses_before_any_launch():
    import nerf
    from nerf import _ops
    m = small_model()
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    grid = nerf.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool), BOX)
    ro, rd = torch.zeros(5, 3), torch.ones(5, 3)
    meta = dict(ro=torch.zeros(5, 3, device="meta"), rd=torch.ones(5, 3, device="meta"))

    def depth(ro=ro, rd=rd, **kw):
        return nerf.render_dex_depth(1, 5, 1.0, m, m, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, m_thres_cand=[5.0], **kw)

    def normals(ro=ro, rd=rd, **kw):
        return nerf.render_dex_normals(1, 5, 1.0, m, m, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, m_thres_cand=[5.0], **kw)

    def colour(ro=ro, rd=rd, **kw):
        return nerf.run_one_iter_of_nerf(1, 5, 1.0, m, m, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, encode_direction_fn=ed,
                                         m_thres_cand=[5.0], **kw)
    for render in (depth, normals, colour):
        with torch.no_grad():
            for pad in (float("nan"), float("inf"), -1.0, -1e-9, 1e39, "wide"):
                with pytest.raises(ValueError, match="ray_span_pad"):
                    render(ray_span=grid, ray_span_pad=pad)
            with pytest.raises(ValueError, match="give ray_span="):                                # a pad without a grid
                render(ray_span_pad=1.0)
            with pytest.raises(ValueError, match="occupancy grid lives on"):                       # a grid on another device than the rays
                render(ray_span=grid, **meta)
            with pytest.raises(RuntimeError, match="ROCm device"):                                 # host tensors: no fallback
                render(ray_span=grid)
        with pytest.raises(RuntimeError, match="near/far gradient"):                               # parameters require grad, autograd enabled
            render(ray_span=grid)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="near/far gradient"):
                with torch.enable_grad():
                    render(ray_span=grid, ro=ro.clone().requires_grad_(True))
    rows = torch.zeros(5, 8)
    for pad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="pad"):
            grid.ray_spans(rows, pad_cells=pad)
    for bad in (torch.zeros(5, 7), torch.zeros(5, 8, dtype=torch.float64), torch.zeros(8), None):
        with pytest.raises(ValueError, match="rays are fp32 rows"):
            grid.ray_spans(bad)
    with pytest.raises(RuntimeError, match="ROCm device"):
        grid.ray_spans(rows)
    with pytest.raises(ValueError, match="occupancy grid lives on"):
        _ops.occupancy_ray_spans(torch.zeros(5, 8, device="meta"), grid)


def test_ray_span_flags_are_judged_before_the_checkpoint_is_read():
    import eval_nerf
    base = ["--checkpoint", "none.ckpt"]
    for argv in (base + ["--ray-span", "0"], base + ["--ray-span", "8,8"], base + ["--ray-span", "a"], base + ["--ray-span", "2048"],
                 base + ["--ray-span-pad", "1"], base + ["--depth-only", "--ray-span-pad", "0.5"],
                 base + ["--ray-span", "32", "--ray-span-pad", "-1"], base + ["--ray-span", "32", "--ray-span-pad", "nan"],
                 base + ["--ray-span", "32", "--ray-span-pad", "inf"], base + ["--ray-span", "32", "--occupancy-dilate", "9"],
                 base + ["--ray-span", "32", "--occupancy-level", "nan"],
                 base + ["--ray-span", "32", "--occupancy-bounds", "0", "0", "0", "1", "0", "1"],
                 base + ["--depth-only", "--occupancy-dilate", "2"], base + ["--depth-only", "--occupancy-level", "1"]):
        with pytest.raises(SystemExit):
            eval_nerf.main(argv)
    for mode in ([], ["--depth-only", "--m-thres", "20"], ["--normals", "--m-thres", "20"]):       # complete flags reach the checkpoint
        with pytest.raises(FileNotFoundError):
            eval_nerf.main(base + mode + ["--ray-span", "32,16,8", "--ray-span-pad", "0.5", "--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1",
                                          "--occupancy-level", "0.5", "--occupancy-dilate", "2", "--precision", "fp32"])


def test_the_restatement_on_hand_checked_cases():
    """The yardstick, pinned without a GPU: a 4 x 1 x 1 grid over [0,4] x [0,1] x [0,1] with cells 1 and 2 set."""
    bounds, cells = (0, 0, 0, 4, 1, 1), (4, 1, 1)
    mask = np.array([False, True, True, False]).reshape(4, 1, 1)
    rays = np.array([[-1, 0.5, 0.5, 1, 0, 0, 0, 9],          # along +x from outside: enters cell 1 at t = 2, leaves cell 2 at t = 4
                     [5, 0.5, 0.5, -2, 0, 0, 0, 9],          # along -x at twice the speed: t = 1 .. 2
                     [-1, 0.5, 0.5, 1, 0, 0, 2.5, 3.5],      # near and far inside the set cells
                     [-1, 1.5, 0.5, 1, 0, 0, 0, 9],          # a zero component outside its slab
                     [-1, 0.5, 0.5, 1, 0, 0, 0, 1.5],        # ends in cell 0: in the box, no set cell
                     [-1, 0.5, 0.5, 1, 0, 0, 4, 3],          # near >= far
                     [1.5, 0.5, 0.5, 0, 0, 0, 1, 2],         # no direction at all, inside a set cell
                     [np.nan, 0.5, 0.5, 1, 0, 0, 0, 9]], F)
    span, visits, over = restate_spans(rays, bounds, cells, mask, 0.0)
    assert visits.tolist() == [2, 2, 2, 0, 0, 0, 1, 0] and not over.any()
    assert span[:3].tolist() == [[2, 4], [1, 2], [2.5, 3.5]]
    assert span[3:6].tolist() == [[0, 9], [0, 1.5], [4, 3]] and span[6].tolist() == [1, 2]
    padded, _, _ = restate_spans(rays, bounds, cells, mask, 1.0)
    assert padded[:3].tolist() == [[1, 5], [0.5, 2.5], [2.5, 3.5]]                                  # one cell of travel; clipped to near / far
    assert np.array_equal(apply_spans(rays, padded, visits)[:, :6].view(np.uint32), rays[:, :6].view(np.uint32))
    hit, n, lo, hi = truth_spans(rays[:7], bounds, cells, mask)
    assert hit.tolist() == [True, True, True, False, False, False, True] and n.tolist() == [2, 2, 2, 0, 0, 0, 1]


@pytest.mark.parametrize("cells,bounds,seed", CPU_GRIDS)
def test_the_restatement_against_float64_geometry(cells, bounds, seed):
    mask = random_mask(cells, seed)
    rays = random_rays(400, bounds, 100 + seed)
    span, visits, over = restate_spans(rays, bounds, cells, mask, 0.0)
    assert not over.any()                                                                          # the walk stays inside its bound
    hit, n, lo, hi = truth_spans(rays, bounds, cells, mask)
    assert np.array_equal(visits > 0, hit) and 0.2 * len(rays) < hit.sum() < len(rays)
    same = hit & (visits == n)
    assert (hit & ~same).sum() <= 0.02 * hit.sum()
    travel = np.abs(rays[:, 3:6].astype(np.float64) * grid_scale(bounds, cells)).max(axis=1)
    err = np.maximum(np.abs(span[:, 0] - lo), np.abs(span[:, 1] - hi)) * travel
    assert err[same].max() <= 1e-4, err[same].max()
    miss = ~hit
    assert np.array_equal(span[miss].view(np.uint32), rays[miss, 6:8].view(np.uint32))


@pytest.mark.parametrize("cells,bounds,seed", CPU_GRIDS)
def test_every_sample_the_classification_keeps_lies_inside_the_span(cells, bounds, seed):
    mask = random_mask(cells, seed)
    rays = random_rays(400, bounds, 100 + seed)
    z = (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * np.linspace(0.0, 1.0, 2048, dtype=F)[None, :]).astype(F)
    keep = restate_kept(rays, z, bounds, cells, mask)
    assert keep.any(axis=1).sum() > 0.2 * len(rays)
    for pad in (0.0, 1.0):
        span, visits, _ = restate_spans(rays, bounds, cells, mask, pad)
        outside = keep & ((z < span[:, 0:1]) | (z > span[:, 1:2]))
        assert not outside.any(), (pad, int(outside.sum()))
        assert not (keep.any(axis=1) & (visits == 0)).any()


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
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def G(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def anchor_of(bounds):
    """A point of the box off every cell boundary of the grids used here: the hand-made rays go through it."""
    b = np.asarray(bounds, np.float64)
    return 0.5 * (b[:3] + b[3:]) + 0.13 * 0.5 * (b[3:] - b[:3])


def kernel_rays(bounds, seed, stride):
    """257 rows: the hand-made cases first, random ones after them."""
    rows = random_rays(257, bounds, seed, stride)
    b = np.asarray(bounds, np.float64)
    centre, half = 0.5 * (b[:3] + b[3:]), 0.5 * (b[3:] - b[:3])
    far_out, anchor = centre - 3.0 * half, anchor_of(bounds)
    aim = tuple((anchor - far_out) / 3.0)                                       # from far_out through the anchor at t = 3
    special = [
        (anchor, (1.0, 0.0, 0.0), 0.0, 9.0),                                      # zero components, inside their slabs
        (centre + np.array([0.0, 1.5, 0.0]) * half, (1.0, 0.0, 0.0), 0.0, 9.0),   # a zero component outside its slab
        (far_out, (-1.0, -1.0, -1.0), 0.0, 9.0),                                  # points away: misses the box
        (centre + 2.0 * half, (-1.0, -0.7, -0.4), 0.0, 20.0),                     # negative components, from outside
        (far_out, aim, 2.5, 3.4),                                                 # near and far fall inside the box (it spans t = 2 .. 4)
        (far_out, aim, 3.0, 3.0),                                                 # near == far
        (far_out, aim, 4.0, 2.0),                                                 # near > far
        (anchor, (0.0, 0.0, 0.0), 1.0, 2.0),                                      # no direction at all
        (centre - 0.9 * half, tuple(0.01 * half), 0.0, 500.0),                    # a long slow walk inside the box
        (2.0 * anchor - far_out, tuple(-np.asarray(aim)), 0.0, 9.0),              # the same line backwards: all components negative
    ]
    for r, (o, d, near, far) in enumerate(special):
        rows[r, 0:3], rows[r, 3:6], rows[r, 6], rows[r, 7] = o, d, near, far
    r = len(special)
    rows[r, 1] = np.nan
    rows[r + 1, 7] = np.inf
    rows[r + 2, 6] = np.nan
    rows[r + 3, 4] = -np.inf
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [8, 11])
@pytest.mark.parametrize("case", ["tenth", "one cell"])
def test_kernel_is_the_restatement_bit_for_bit(dev, case, stride):
    import nerf
    cells, bounds = ((5, 7, 9), BOX) if case == "tenth" else ((40, 33, 17), ODD_BOX)
    if case == "tenth":
        mask = random_mask(cells, 7, share=0.1)
    else:
        mask = np.zeros(cells, bool)
        at = np.floor((anchor_of(bounds) - np.asarray(bounds[:3])) * grid_scale(bounds, cells)).astype(int)
        mask[at[0], at[1], at[2]] = True                                     # the one cell the hand-made rays go through
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), bounds)
    rows = kernel_rays(bounds, 31 + stride, stride)
    seen = set()
    for pad in (0.0, 1.0):
        span, visits, over = restate_spans(rows, bounds, cells, mask, pad)
        assert not over.any()
        seen.add((int((visits > 0).sum()), int((visits == 0).sum())))
        assert (visits > 0).sum() >= (10 if case == "tenth" else 3) and (visits == 0).sum() >= 10
        dev_rows = G(rows, dev)
        got_span, got_visits = grid.ray_spans(dev_rows, pad_cells=pad)
        assert got_visits.dtype == torch.int32 and np.array_equal(C(got_visits), visits)
        assert same_bits(C(got_span), span)
        assert same_bits(C(dev_rows), rows)                                   # without apply: the rows keep every bit
        got_span, got_visits = grid.ray_spans(dev_rows, pad_cells=pad, apply=True)
        assert np.array_equal(C(got_visits), visits) and same_bits(C(got_span), span)
        want = apply_spans(rows, span, visits)
        assert same_bits(C(dev_rows), want)
        assert same_bits(want[:, :6], rows[:, :6]) and same_bits(want[:, 8:], rows[:, 8:]) and same_bits(want[visits == 0], rows[visits == 0])
        assert not same_bits(want, rows)                                      # and the tightening did tighten
    assert len(seen) == 1                                                     # the pad moves ends, not hits


def all_set_grid(dev, cells=(6, 5, 4)):
    import nerf
    return nerf.OccupancyGrid.from_mask(torch.ones(cells, dtype=torch.bool, device=dev), (-19.0, -19.5, -20.0, 19.0, 19.5, 20.0))


@pytest.mark.gpu
def test_an_all_set_grid_and_an_empty_grid_leave_the_rows_alone(dev):
    import nerf
    rows = random_rays(300, BOX, 5, 9)
    rows[:, 6] = np.random.default_rng(1).uniform(0.0, 1.0, 300).astype(F)
    rows[:, 7] = rows[:, 6] + F(2.0)                                          # |ro| < 4.5 per axis, |rd| <= 2, t <= 3: inside +-19
    full = all_set_grid(dev)
    empty = nerf.OccupancyGrid.from_mask(torch.zeros(6, 5, 4, dtype=torch.bool, device=dev), BOX)
    for pad in (0.0, 1.0):
        dev_rows = G(rows, dev)
        span, visits = full.ray_spans(dev_rows, pad_cells=pad, apply=True)
        assert (C(visits) > 0).all() and same_bits(C(dev_rows), rows) and same_bits(C(span), rows[:, 6:8])
        span, visits = empty.ray_spans(dev_rows, pad_cells=pad, apply=True)
        assert (C(visits) == 0).all() and same_bits(C(dev_rows), rows) and same_bits(C(span), rows[:, 6:8])
    span, visits = full.ray_spans(torch.zeros(0, 8, device=dev), apply=True)   # no rays: no launch
    assert span.shape == (0, 2) and visits.shape == (0,)


_CACHE = {}


def lego_models(dev):
    import nerf
    if "m" not in _CACHE:
        out = []
        for sd in lego_weights():
            m = nerf.models.FlexibleNeRFModel(**D4)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            out.append(m.to(dev))
        _CACHE["m"] = out
    return _CACHE["m"]


def rays_37(dev):
    """37 rays of a synthetic camera looking at the box -> (ro, rd) on the device"""
    import nerf
    from nerf import synthetic as syn
    if "r" not in _CACHE:
        h = w = 40
        e_mat = torch.from_numpy(syn.scene_pose(3)).to(dev)
        k_mat = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
        ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), e_mat, k_mat)
        sel = torch.from_numpy(syn.select_rays(h, w, 37, seed=5)).to(dev)
        _CACHE["r"] = (ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous())
    return _CACHE["r"]


def dex_depth(models, ro, rd, nc=NC, nf=NF, thres=M_THRES, **kw):
    import nerf
    with torch.no_grad():
        return nerf.render_dex_depth(1, ro.shape[0], 1.0, models[0], models[1] if nf else None, ro, rd, make_cfg(nc, nf), mode="train",
                                     encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(thres), **kw)


def assert_same_maps(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert same_bits(C(a), C(b)), i


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_an_all_set_grid_renders_the_bits_of_the_render_without_it(dev, precision):
    import nerf
    nerf.set_precision(precision)
    models = lego_models(dev)
    ro, rd = rays_37(dev)
    want = dex_depth(models, ro, rd)
    got = dex_depth(models, ro, rd, ray_span=all_set_grid(dev))
    assert len(want) == 4 + len(M_THRES)
    assert_same_maps(got, want)


def flat_maps(maps):
    """A chunk entry point's maps -> the flat list the image-level renders return: (K,N) blocks become K maps."""
    out = []
    for m in maps:
        if m is not None and m.dim() >= 2 and m.shape[0] != maps[0].shape[0]:
            out += [m[k] for k in range(m.shape[0])]
        else:
            out.append(m)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sub-box", "networks"])
def test_the_renders_are_the_chunk_entry_points_on_restated_rows(dev, kind):
    import nerf
    from nerf import _hip, _ops
    models = lego_models(dev)
    ro, rd = rays_37(dev)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    if kind == "sub-box":
        mask = np.zeros((8, 7, 6), bool)
        mask[2:6, 1:5, 2:5] = True
        grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    else:
        with torch.no_grad():
            grid = nerf.OccupancyGrid.from_networks(models, ex, BOX, 16, level=0.0, dilate=1)
        mask = C(grid.to_mask())
    pad = 1.0 if kind == "sub-box" else 0.25
    th = torch.tensor(M_THRES, dtype=torch.float32, device=dev)

    def restated(rows):
        host = C(rows)
        span, visits, over = restate_spans(host, grid.bounds, grid.cells, mask, pad)
        assert not over.any() and 0 < (visits > 0).sum() and not same_bits(apply_spans(host, span, visits), host)
        return G(apply_spans(host, span, visits), dev)
    rows = restated(_ops.pack_ray_rows(ro, rd, None, 2.0, 6.0))
    packs = [m.packed_density(True, True, precision=_hip.PREC_F32) for m in models]
    kw = dict(ray_span=grid, ray_span_pad=pad)
    with torch.no_grad():
        want = flat_maps(_ops.render_rays_depth(*packs, rows, NC, NF, False, 0.0, th, {}))
        assert_same_maps(dex_depth(models, ro, rd, **kw), want)
        want = flat_maps(_ops.render_rays_depth(*packs, rows, NC, NF, False, 0.0, th, {}, refine_steps=2))
        assert_same_maps(dex_depth(models, ro, rd, refine_steps=2, **kw), want)
        q = torch.tensor([0.5], dtype=torch.float32, device=dev)
        want = flat_maps(_ops.render_rays_depth(*packs, rows, NC, NF, False, 0.0, th, {}, quantiles=q))
        assert_same_maps(dex_depth(models, ro, rd, quantiles=[0.5], **kw), want)
        maps, stats = _ops.render_rays_depth_culled(*packs, rows, NC, NF, False, 0.0, th, grid, {})
        assert_same_maps(dex_depth(models, ro, rd, occupancy=grid, **kw), flat_maps(maps))
        # the colour render: rows with the view directions
        rows11 = restated(_ops.pack_ray_rows(ro, rd, rd, 2.0, 6.0))
        full = [m.packed(True, True, precision=_hip.PREC_F32) for m in models]
        want = flat_maps(_ops.render_rays(*full, rows11, NC, NF, False, 0.0, False, list(M_THRES), {}))
        got = nerf.run_one_iter_of_nerf(1, 37, 1.0, models[0], models[1], ro, rd, make_cfg(), mode="train", encode_position_fn=ex,
                                        encode_direction_fn=ed, m_thres_cand=list(M_THRES), **kw)
        assert_same_maps(got, want)
        # the normal render
        streams = models[1].packed_density_grad(True, True, precision=_hip.PREC_F32)
        _, _, depth, acc, dex, normal, dex_normal = _ops.render_rays_normals(*packs, streams, rows, NC, NF, False, 0.0, th, {})
        got = nerf.render_dex_normals(1, 37, 1.0, models[0], models[1], ro, rd, make_cfg(), mode="train", encode_position_fn=ex,
                                      m_thres_cand=list(M_THRES), **kw)
        assert_same_maps([got.depth, got.acc, got.normal, *got.dex_depth, *got.dex_normal],
                         [depth, acc, normal] + [dex[k] for k in range(3)] + [dex_normal[k] for k in range(3)])


def first_crossing_truth(models, rays, th):
    """The truth of scripts/dex_refine_measure.py's accuracy mode for its 64+0 render: the first brackets of the fp32 64+64 render of
    the untightened rays - the crossing the fine pass saw - and, inside each, the first crossing among 2049 dense evaluations of the CPU
    oracle.  Brackets whose dense samples cross more than once are left out, and so are those whose dense samples never cross (the
    oracle disagrees with the kernel about the bracket's last sample: no truth) -> ({(ray, k): z_true}, brackets, those crossing more
    than once)."""
    from nerf import _hip, _ops
    from oracle import nerf_oracle as oc
    sd_f, mc = oc.to_torch_sd(lego_weights()[1]), oc.ModelCfg(**D4)
    pc, pf = (mm.packed_density(True, True, precision=_hip.PREC_F32) for mm in models)
    m = np.asarray(M_THRES, F)
    with torch.no_grad():
        z = _ops.coarse_depths(rays, 64, False)
        z = _ops.density_resample(_ops.run_network_rays(pc, rays, z), z, rays[:, 3:6], 64)[2]
        br = _ops.composite_density_brackets(_ops.run_network_rays(pf, rays, z), z, rays[:, 3:6], th)[3]
    br0, host = C(br), C(rays)
    pairs = np.argwhere((br0[..., 3] != -np.inf) & (br0[..., 1] > br0[..., 0]))
    r, k = pairs[:, 0], pairs[:, 1]
    lo, hi = br0[r, k, 0].astype(np.float64), br0[r, k, 1].astype(np.float64)
    zd = (lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, 2049)[None, :]).astype(F)
    ro, rd = torch.from_numpy(host[r, 0:3].copy()), torch.from_numpy(host[r, 3:6].copy())
    with torch.no_grad():
        s = oc.run_network(sd_f, ro[:, None, :] + rd[:, None, :] * torch.from_numpy(zd)[..., None], rd, mc)[..., 3].numpy().astype(np.float64)
    above = s > m[k].astype(np.float64)[:, None]
    multi = (above[:, 1:] != above[:, :-1]).sum(-1) > 1
    j = above.argmax(-1)
    jm = np.maximum(j - 1, 0)
    i = np.arange(len(pairs))
    z0, z1, s0, s1 = zd[i, jm].astype(np.float64), zd[i, j].astype(np.float64), s[i, jm], s[i, j]
    with np.errstate(all="ignore"):
        z_true = np.where(j == 0, z0, z0 + (z1 - z0) * (m[k] - s0) / (s1 - s0))
    usable = above.any(-1) & ~multi
    return {(int(a), int(b)): zt for (a, b), zt, ok in zip(pairs, z_true, usable) if ok}, len(pairs), int(multi.sum())


def dex_errors(models, rows, th, truth):
    """|Dex depth - truth| of the 64+0 render of `rows` - the fine network on the 64 uniform depths, as in that script - over the
    brackets with a truth that cross in this render too."""
    from nerf import _hip, _ops
    pf = models[1].packed_density(True, True, precision=_hip.PREC_F32)
    with torch.no_grad():
        z = _ops.coarse_depths(rows, 64, False)
        _, _, dex, br, _ = _ops.composite_density_brackets(_ops.run_network_rays(pf, rows, z), z, rows[:, 3:6], th)
    br0, dex = C(br), C(dex).T
    return np.array([abs(float(dex[r, k]) - zt) for (r, k), zt in truth.items() if br0[r, k, 3] != -np.inf])


@pytest.mark.gpu
def test_tightened_rays_give_a_dex_depth_no_worse_than_untightened_ones(dev):
    """The lego golden rays, fp32, 64+0 samples, thresholds 5 / 20 / 60, a 32^3 grid of both lego networks, level 0, dilate 1, pad 1:
    profiles/ray_span.md has the medians, their ratio and the mean span fraction measured on an MI355X."""
    import nerf
    from nerf import _ops
    models = lego_models(dev)
    name = "render_lego_val"
    g, rkw = load_golden(name), CASES[name][2]
    rays = _ops.pack_ray_rows(G(g["ro"], dev), G(g["rd"], dev), None, rkw["near"], rkw["far"])
    with torch.no_grad():
        grid = nerf.OccupancyGrid.from_networks(models, nerf.get_embedding_function(10), BOX, 32, level=0.0, dilate=1)
    th = torch.tensor(M_THRES, dtype=torch.float32, device=dev)
    truth, n_brackets, n_multi = first_crossing_truth(models, rays, th)
    tight_rays = rays.clone()
    span, visits = grid.ray_spans(tight_rays, apply=True)
    hit = C(visits) > 0
    fraction = float(((C(span)[:, 1] - C(span)[:, 0]) / (rkw["far"] - rkw["near"]))[hit].mean())
    plain, tight = dex_errors(models, rays, th, truth), dex_errors(models, tight_rays, th, truth)
    print(f"ray span accuracy: {int(hit.sum())} of {len(hit)} rays hit, mean span fraction {fraction:.4f}; {len(truth)} of {n_brackets} "
          f"brackets with a truth, {n_multi} crossing more than once; untightened median {np.median(plain):.6f} over {len(plain)}, "
          f"tightened median {np.median(tight):.6f} over {len(tight)}; ratio {np.median(tight) / np.median(plain):.4f}")
    assert hit.any() and n_multi <= 0.05 * n_brackets
    assert len(plain) > 0.5 * len(truth) and len(tight) > 0.5 * len(truth)      # the medians speak for most of the truth
    assert np.median(tight) <= np.median(plain)


@pytest.mark.gpu
def test_eval_driver_with_a_ray_span_grid(dev, tmp_path, capsys):
    """eval_nerf.py --ray-span: the default bounds hold every sample, so a grid set everywhere (level below every density) tightens
    nothing and renders the plain maps bit for bit; a real grid reports its hit share and span fraction per view; with --occupancy of
    the same cells one grid serves both."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "2", "--num-fine", "64", "--precision", "fp32", "--depth-only", "--m-thres", "20"]
    plain = eval_nerf.main(common + ["--quiet"])
    res = eval_nerf.main(common + ["--ray-span", "12,10,8", "--occupancy-level=-1e30", "--occupancy-dilate", "0"])
    assert res["ray_span"].cells == (12, 10, 8) and res["ray_span"].occupied_fraction() == 1.0
    assert [row["hit_share"] for row in res["ray_spans"]] == [1.0, 1.0]
    assert all(row["mean_span_fraction"] == pytest.approx(1.0, abs=1e-6) for row in res["ray_spans"])
    for (_, depth, dex), (_, depth_plain, dex_plain) in zip(res["frames"], plain["frames"]):
        assert_same_maps([depth] + list(dex), [depth_plain] + list(dex_plain))
    text = capsys.readouterr().out
    assert "ray-span grid 12x10x8" in text and "ray span view 1: 100.00 % of the rays hit a set cell" in text
    res = eval_nerf.main(common + ["--quiet", "--ray-span", "16", "--ray-span-pad", "0.5", "--occupancy", "16"])
    assert res["ray_span"] is res["occupancy"] and 0 < sum(res["cull"]["kept"]) < sum(res["cull"]["total"])
    assert all(0.0 < row["hit_share"] <= 1.0 and 0.0 < row["mean_span_fraction"] < 1.0 for row in res["ray_spans"])
    for extra in (["--normals"], []):                                         # the normal render and the colour render take the flag too
        mode = [a for a in common if a != "--depth-only"] + extra
        res = eval_nerf.main(mode + ["--quiet", "--ray-span", "16"])
        assert len(res["ray_spans"]) == 2 and len(res["frames"]) == 2
