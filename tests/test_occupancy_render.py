"""Occupancy-grid culling of the depth-only Dex render (include/dexnerf_hip_occupancy.h, nerf.OccupancyGrid,
nerf.render_dex_depth(occupancy=...)).

The kernels are pinned bit for bit to a numpy restatement of the header's text: the bit grid (corners hot iff non-finite or > level,
Chebyshev dilation, OR-accumulation), the classification of a ray sample (x = ro + rd*z in fp32, t = (x - b0)*s, the cell's bit), the
slots (ranks in ascending sample order), the emitted points and the gathered sigma column.  The culled render is pinned bit for bit to
an oracle composed of entry points the library had before (dn_coarse_depths, the numpy classification, run_network_pts on the kept
points, the fill value, dn_density_resample, dn_composite_density / its quantile variant).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import D4, D8, d8_weights, lego_weights

OCC = ("dn_occupancy_words", "dn_occupancy_build", "dn_occupancy_compact_workspace_bytes", "dn_occupancy_compact_count",
       "dn_occupancy_compact_emit", "dn_occupancy_gather")
INVAL = -1000
FILL = np.float32(-3.4028234663852886e+38)
NETS = {"lego": (D4, lego_weights), "d8w256": (D8, d8_weights)}
NC, NF = 37, 22                      # the smallest coarse / fine counts tests/test_depth_render.py uses (RESAMPLE_CASES)
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
M_THRES = (5.0, 20.0, 60.0)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def restate_build(f, level, dilate):
    """bool (cx,cy,cz) from the vertex field (cx+1,cy+1,cz+1) fp32"""
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        hot = ~np.isfinite(f) | (f > np.float32(level))
    cx, cy, cz = (n - 1 for n in f.shape)
    raw = np.zeros((cx, cy, cz), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                raw |= hot[di:di + cx, dj:dj + cy, dk:dk + cz]
    out = np.zeros_like(raw)
    d = dilate
    for i in range(cx):
        for j in range(cy):
            for k in range(cz):
                out[i, j, k] = raw[max(i - d, 0):i + d + 1, max(j - d, 0):j + d + 1, max(k - d, 0):k + d + 1].any()
    return out


def pack_bits(mask):
    """uint32 words: cell c = (i*cy + j)*cz + k is bit c & 31 of word c >> 5"""
    flat = np.asarray(mask, bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, np.uint32)
    for c in np.nonzero(flat)[0]:
        words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return words


def grid_scale(bounds, cells):
    b = np.asarray(bounds, np.float32)
    return np.array([np.float32(cells[a] / (float(b[a + 3]) - float(b[a]))) for a in range(3)], np.float32)


def restate_classify(rays, z, bounds, cells, mask):
    """-> (keep (N,S) bool, x (N,S,3) fp32, slot (N,S) int32)"""
    rays, z = np.asarray(rays, np.float32), np.asarray(z, np.float32)
    b0, s = np.asarray(bounds, np.float32)[:3], grid_scale(bounds, cells)
    with np.errstate(invalid="ignore", over="ignore"):
        x = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]      # fp32: multiply, then add
        t = (x - b0) * s
        assert x.dtype == np.float32 and t.dtype == np.float32
        inside = ((t >= np.float32(0)) & (t < np.asarray(cells, np.float32))).all(axis=-1)
        idx = np.where(inside[..., None], t, np.float32(0)).astype(np.int64)
    keep = inside & np.asarray(mask, bool)[idx[..., 0], idx[..., 1], idx[..., 2]]
    slot = np.where(keep, np.cumsum(keep.reshape(-1)).reshape(keep.shape) - 1, -1).astype(np.int32)
    return keep, x, slot


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_occupancy_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_occupancy.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.OCCUPANCY_EXPORTS) == set(OCC)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS))
    assert not older & set(OCC) and len(_hip.EXPORTS) == 76
    assert "dexnerf_hip_occupancy.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()      # build() checks the new header's symbols too
    assert "occupancy.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in OCC) and hiplib.dn_abi_version() == 2
    for name, value in (("DN_OCC_MAX_AXIS_CELLS", _hip.OCC_MAX_AXIS_CELLS), ("DN_OCC_MAX_CELLS", _hip.OCC_MAX_CELLS),
                        ("DN_OCC_MAX_DILATE", _hip.OCC_MAX_DILATE), ("DN_OCC_MAX_SAMPLES", _hip.OCC_MAX_SAMPLES),
                        ("DN_OCC_MAX_SAMPLES_PER_RAY", _hip.OCC_MAX_SAMPLES_PER_RAY)):
        assert f"#define {name} {value}\n" in text
    assert "#define DN_OCC_FILL (-3.402823466e+38f)\n" in text and np.float32(_hip.OCC_FILL) == FILL == -np.finfo(np.float32).max
    assert hiplib.dn_occupancy_words(5, 4, 3) == 2 and hiplib.dn_occupancy_words(1, 1, 1) == 1 and hiplib.dn_occupancy_words(1024, 1024, 1024) == 1 << 25


def test_occupancy_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    fake, odd = ctypes.c_void_p(256 * 4096), ctypes.c_void_p(256 * 4096 + 2)
    cells = (dict(cx=0), dict(cy=-1), dict(cz=0), dict(cx=(1 << 24) + 1), dict(cx=1 << 12, cy=1 << 12, cz=1 << 12), dict(cx=1 << 20, cy=1 << 20, cz=1))
    build = dict(field=fake, stride=1, cx=5, cy=4, cz=3, level=0.5, dilate=1, acc=0, scratch=fake, bits=fake, stream=None)
    for kw in cells + (dict(field=None), dict(bits=None), dict(stride=0), dict(stride=-4), dict(dilate=-1), dict(dilate=9), dict(scratch=None),
                       dict(bits=odd), dict(scratch=odd)):
        assert hiplib.dn_occupancy_build(*{**build, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_build" in hiplib.dn_last_error(), kw
    for kw in cells:
        g = {**build, **kw}
        assert hiplib.dn_occupancy_words(g["cx"], g["cy"], g["cz"]) == 0, kw
    sizes = (dict(n=0), dict(n=-5), dict(s=0), dict(s=2049), dict(s=-1), dict(n=1 << 30, s=2), dict(n=(1 << 30) + 1, s=1))
    count = dict(rays=fake, stride=8, z=fake, n=37, s=59, bits=fake, cx=5, cy=4, cz=3, x0=-1.0, y0=-1.0, z0=-1.0, x1=1.0, y1=1.0, z1=1.0,
                 sx=2.5, sy=2.0, sz=1.5, ws=fake, slot=fake, record=fake, stream=None)
    nan, inf = float("nan"), float("inf")
    bounds = (dict(x0=nan), dict(y1=inf), dict(z0=-inf), dict(x0=1.0), dict(y0=2.0), dict(z1=-1.0), dict(sx=0.0), dict(sy=-1.0), dict(sz=nan),
              dict(sx=inf))
    common = (dict(rays=None), dict(z=None), dict(stride=0), dict(stride=-8), dict(stride=7)) + sizes
    for kw in common + cells + bounds + (dict(bits=None), dict(ws=None), dict(slot=None), dict(record=None), dict(ws=ctypes.c_void_p(256 * 4096 + 16)),
                                         dict(record=odd), dict(slot=odd)):
        assert hiplib.dn_occupancy_compact_count(*{**count, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_compact_count" in hiplib.dn_last_error(), kw
    emit = dict(rays=fake, stride=8, z=fake, n=37, s=59, slot=fake, cap=10, pts=fake, stream=None)
    for kw in common + (dict(slot=None), dict(cap=-1), dict(pts=None)):
        assert hiplib.dn_occupancy_compact_emit(*{**emit, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_compact_emit" in hiplib.dn_last_error(), kw
    assert hiplib.dn_occupancy_compact_emit(*{**emit, "cap": 0, "pts": None}.values()) == 0       # a capacity of 0 launches nothing
    for kw in sizes:
        g = {**count, **kw}
        assert hiplib.dn_occupancy_compact_workspace_bytes(g["n"], g["s"]) == 0, kw
    nbytes = hiplib.dn_occupancy_compact_workspace_bytes(37, 59)
    assert nbytes >= 8 and nbytes % 256 == 0 and hiplib.dn_occupancy_compact_workspace_bytes(1 << 19, 2048) > 0
    gather = dict(slot=fake, out=fake, rows=5, n=10, rf=fake, ws=fake, record=fake, stream=None)
    for kw in (dict(slot=None), dict(rf=None), dict(out=None), dict(rows=-1), dict(rows=11), dict(n=0), dict(n=(1 << 30) + 1), dict(ws=None),
               dict(record=None), dict(ws=ctypes.c_void_p(256 * 4096 + 16)), dict(record=odd)):
        assert hiplib.dn_occupancy_gather(*{**gather, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_gather" in hiplib.dn_last_error(), kw


def random_mask(cells, seed, share=0.3):
    return np.random.default_rng(seed).random(cells) < share


def test_occupancy_grid_host_side():
    import nerf
    mask = random_mask((33, 2, 7), 1)
    grid = nerf.OccupancyGrid.from_mask(torch.from_numpy(mask), BOX)
    assert grid.cells == (33, 2, 7) and grid.bits.dtype == torch.int32 and grid.bits.numel() == (33 * 2 * 7 + 31) // 32
    assert np.array_equal(grid.bits.numpy().view(np.uint32), pack_bits(mask))                      # the bits, pinned
    assert np.array_equal(grid.to_mask().numpy(), mask) and grid.occupied_fraction() == pytest.approx(mask.mean())
    assert grid.bounds == tuple(float(np.float32(b)) for b in BOX)
    assert np.array_equal(np.asarray(grid.scale, np.float32), grid_scale(BOX, grid.cells))         # float64 quotient, rounded to fp32 once
    odd_box = (0.1, -0.3, 1e-3, 0.7, 0.9, 3.3)
    assert np.array_equal(np.asarray(nerf.OccupancyGrid.from_mask(torch.from_numpy(mask), odd_box).scale, np.float32), grid_scale(odd_box, grid.cells))
    again = nerf.OccupancyGrid.from_state_dict(grid.state_dict())
    assert again.cells == grid.cells and again.bounds == grid.bounds and torch.equal(again.bits, grid.bits)
    one = nerf.OccupancyGrid.from_mask(torch.ones(1, 1, 1, dtype=torch.bool), BOX)
    assert one.bits.tolist() == [1] and one.occupied_fraction() == 1.0
    ok = torch.from_numpy(mask)
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, 1, float("nan")), (0, 0, 0, float("inf"), 1, 1), (1, 0, 0, 0, 1, 1),
                (0, 0, 0, 1e39, 1, 1)):
        with pytest.raises(ValueError):
            nerf.OccupancyGrid.from_mask(ok, bad)
    for bad in (torch.zeros(3, 3, 3), torch.zeros(3, 3, dtype=torch.bool), torch.zeros(0, 3, 3, dtype=torch.bool), mask):
        with pytest.raises(ValueError):
            nerf.OccupancyGrid.from_mask(bad, BOX)
    with pytest.raises(ValueError):
        nerf.OccupancyGrid(torch.zeros(3, dtype=torch.int32), BOX, (5, 4, 3))                      # 60 cells are two words
    with pytest.raises(ValueError):
        nerf.OccupancyGrid(torch.zeros(2, dtype=torch.int64), BOX, (5, 4, 3))
    m = small_model()
    ex = nerf.get_embedding_function(10)
    with torch.no_grad():
        for kw in (dict(cells=0), dict(cells=(4, 4)), dict(cells=(1 << 24) + 1), dict(cells=2048), dict(bounds=(0, 0, 0, 1, 1, 0)), dict(level=float("nan")),
                   dict(level=1e39), dict(dilate=-1), dict(dilate=9)):
            with pytest.raises(ValueError):
                nerf.OccupancyGrid.from_networks(**{**dict(models=[m], encode_position_fn=ex, bounds=BOX, cells=4), **kw})
        with pytest.raises(ValueError):
            nerf.OccupancyGrid.from_networks([None], ex, BOX, 4)
        with pytest.raises(RuntimeError, match="ROCm device"):
            nerf.OccupancyGrid.from_networks([m], ex, BOX, 4)                                      # host parameters: refused, never computed on the CPU
    with pytest.raises(RuntimeError, match="no-grad"):
        nerf.OccupancyGrid.from_networks([m], ex, BOX, 4)


def small_model(dev=None):
    import nerf
    m = nerf.models.FlexibleNeRFModel(**D4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lego_weights()[1].items()})
    return m if dev is None else m.to(dev)


def make_cfg(nc=NC, nf=NF, chunksize=4096, **over):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    mode.update(over)
    return nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def test_render_dex_depth_refuses_a_grid_before_any_launch():
    import nerf
    m = small_model()
    ex = nerf.get_embedding_function(10)
    grid = nerf.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool), BOX)
    ro, rd = torch.zeros(5, 3), torch.ones(5, 3)

    def render(ro=ro, rd=rd, **kw):
        return nerf.render_dex_depth(1, 5, 1.0, m, m, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, m_thres_cand=[5.0], **kw)
    try:
        with torch.no_grad():
            nerf.set_precision("fp16")
            with pytest.raises(RuntimeError, match="fp16"):
                render(occupancy=grid)
            nerf.set_precision("fp32")
            with pytest.raises(ValueError, match="occupancy grid lives on"):                       # a grid on another device than the rays
                render(ro=torch.zeros(5, 3, device="meta"), rd=torch.ones(5, 3, device="meta"), occupancy=grid)
            with pytest.raises(ValueError, match="cull_stats"):
                render(cull_stats=True)
            with pytest.raises(RuntimeError, match="ROCm device"):                                 # host tensors: no fallback
                render(occupancy=grid)
        with pytest.raises(RuntimeError, match="no-grad"):                                         # parameters require grad, autograd enabled
            render(occupancy=grid)
    finally:
        nerf.set_precision("fp32")


def test_occupancy_flags_are_judged_before_the_checkpoint_is_read():
    import eval_nerf
    base = ["--checkpoint", "none.ckpt", "--depth-only", "--m-thres", "20"]
    for argv in (["--checkpoint", "none.ckpt", "--occupancy", "64"],                                # needs --depth-only
                 base + ["--occupancy", "64", "--precision", "fp16"], base + ["--occupancy", "0"], base + ["--occupancy", "8,8"],
                 base + ["--occupancy", "a"], base + ["--occupancy", "2048"], base + ["--occupancy", "64", "--occupancy-dilate", "9"],
                 base + ["--occupancy", "64", "--occupancy-level", "nan"], base + ["--occupancy", "64", "--occupancy-bounds", "0", "0", "0", "1", "0", "1"],
                 base + ["--occupancy", "64", "--occupancy-bounds", "0", "0", "0", "1", "1"], base + ["--occupancy-check"],
                 base + ["--occupancy-dilate", "2"], base + ["--occupancy-level", "1"], base + ["--occupancy-bounds", "0", "0", "0", "1", "1", "1"],
                 ["--checkpoint", "none.ckpt", "--depth-only", "--depth-quantiles", "0.5", "--occupancy", "64", "--occupancy-check"]):
        with pytest.raises(SystemExit):
            eval_nerf.main(argv)
    with pytest.raises(FileNotFoundError):                                                         # a complete set of flags reaches the checkpoint
        eval_nerf.main(base + ["--occupancy", "32,16,8", "--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1", "--occupancy-level", "0.5",
                               "--occupancy-dilate", "2", "--occupancy-check", "--precision", "fp32"])


def test_the_restatement_on_hand_checked_cases():
    """The yardstick, pinned without a GPU."""
    f = np.full((3, 3, 3), -1.0, np.float32)
    f[2, 2, 2] = 1.0
    raw = restate_build(f, 0.0, 0)
    assert raw.sum() == 1 and raw[1, 1, 1]
    assert restate_build(f, 1.0, 0).sum() == 0                                                     # equal to the level: not above it
    assert restate_build(f, 0.0, 1).all()
    f[0, 0, 0] = np.nan
    assert restate_build(f, 5.0, 0)[0, 0, 0] and restate_build(f, 5.0, 0).sum() == 1               # non-finite counts as occupied
    assert pack_bits(np.ones((33, 1, 1), bool)).tolist() == [0xFFFFFFFF, 1]
    rays = np.array([[0, 0, 0, 1, 0, 0, 0, 9]], np.float32)
    z = np.array([[-0.5, 0.0, 0.5, 1.0, 1.5, 2.0, np.nan]], np.float32)
    mask = np.array([True, False]).reshape(2, 1, 1)
    keep, x, slot = restate_classify(rays, z, (0, -1, -1, 2, 1, 1), (2, 1, 1), mask)
    assert keep.tolist() == [[False, True, True, False, False, False, False]] and slot.tolist() == [[-1, 0, 1, -1, -1, -1, -1]]


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


def bits_of(t):
    return C(t).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def build_field(cells, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 1.0, tuple(c + 1 for c in cells)).astype(np.float32)
    f[rng.random(f.shape) < 0.6] = -2.0                                     # sparse: dilation has something to do
    flat = f.reshape(-1)
    flat[rng.integers(0, flat.size, 3)] = 0.25                              # values equal to the level
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [(5, 4, 3), (33, 2, 7), (1, 1, 1)])
def test_build_is_the_restatement(dev, cells):
    from nerf import _ops
    level = 0.25
    f = build_field(cells, sum(cells))
    planted = f.copy()
    planted.reshape(-1)[[0, planted.size // 2, planted.size - 1]] = (np.nan, np.inf, -np.inf)
    other = build_field(cells, 99)
    for field in (f, planted):
        assert (field == np.float32(level)).any() or field.size < 30
        for dilate in (0, 1, 2):
            want = restate_build(field, level, dilate)
            bits = _ops.occupancy_build(G(field, dev), cells, level, dilate)
            assert np.array_equal(bits_of(bits), pack_bits(want)), (cells, dilate)
            # accumulate: the second field OR-ed into the first one's bits; without it the bits are replaced
            both = _ops.occupancy_build(G(other, dev), cells, level, dilate, bits=bits.clone(), accumulate=True)
            assert np.array_equal(bits_of(both), pack_bits(want | restate_build(other, level, dilate))), (cells, dilate)
            replaced = _ops.occupancy_build(G(other, dev), cells, level, dilate, bits=bits.clone(), accumulate=False)
            assert np.array_equal(bits_of(replaced), pack_bits(restate_build(other, level, dilate))), (cells, dilate)
    # a strided field is read in place: column 3 of (P,4) rows
    rows = np.zeros((f.size, 4), np.float32)
    rows[:, 3] = f.reshape(-1)
    view = G(rows, dev)[:, 3].unflatten(0, f.shape)
    assert view.stride(2) == 4 and np.array_equal(bits_of(_ops.occupancy_build(view, cells, level, 1)), pack_bits(restate_build(f, level, 1)))


class NpGrid:
    """What the compaction wrappers read of a grid: device bits, cells, fp32 bounds, scales."""

    def __init__(self, mask, bounds, dev):
        self.mask, self.cells = np.asarray(mask, bool), tuple(mask.shape)
        self.bounds = tuple(float(np.float32(b)) for b in bounds)
        self.scale = tuple(float(s) for s in grid_scale(bounds, self.cells))
        self.bits = G(pack_bits(mask).view(np.int32), dev)


def sample_set(p, seed):
    """p samples as (rays (N,8), z (N,S)) with S the largest of 1, 3, 7 that divides p; points in and around the unit box"""
    rng = np.random.default_rng(seed)
    s = next(q for q in (7, 3, 1) if p % q == 0)
    n = p // s
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-0.2, 0.4, (n, 3))
    rays[:, 3:6] = rng.uniform(-0.5, 0.9, (n, 3))
    z = rng.uniform(0.0, 1.2, (n, s)).astype(np.float32)
    return rays, z


def check_compaction(dev, rays, z, grid, capacity=None):
    from nerf import _ops
    keep, x, slot = restate_classify(rays, z, grid.bounds, grid.cells, grid.mask)
    n_kept = int(keep.sum())
    r, zz = G(rays, dev), G(z, dev)
    got_slot, record, ws = _ops.occupancy_compact_count(r, zz, grid)
    assert C(record).tolist() == [n_kept, z.size, 0, 0]
    assert np.array_equal(C(got_slot), slot)
    cap = n_kept if capacity is None else capacity
    pts = torch.full((max(n_kept, 1) + 2, 3), 7.0, dtype=torch.float32, device=dev)
    _ops.occupancy_compact_emit(r, zz, got_slot, cap, pts)
    pts = C(pts)
    assert same_bits(pts[:min(cap, n_kept)], x[keep][:min(cap, n_kept)]) and (pts[min(cap, n_kept):] == 7.0).all()      # rows past the capacity untouched
    # gather: the network's rows stand in as a ramp with planted non-finite values
    out = np.random.default_rng(3).normal(size=(max(n_kept, 1), 4)).astype(np.float32)
    out[::97, 3] = np.nan
    out[5::131, 3] = np.inf
    out = out[:n_kept]
    rf = torch.full(z.shape + (4,), 3.0, dtype=torch.float32, device=dev)
    _ops.occupancy_gather(got_slot, G(out, dev) if n_kept else None, rf, ws, record)
    rf = C(rf)
    want = np.full(z.shape, FILL, np.float32)
    want[keep] = out[:, 3]
    assert same_bits(rf[..., 3], want) and (rf[..., :3] == 3.0).all()
    assert C(record).tolist() == [n_kept, z.size, int((~np.isfinite(out[:, 3])).sum()), 0]
    rf2 = torch.full(z.shape + (4,), 3.0, dtype=torch.float32, device=dev)
    _ops.occupancy_gather(got_slot, G(out, dev) if n_kept else None, rf2)                         # without the count: the same column
    assert same_bits(C(rf2)[..., 3], want)
    return n_kept


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 63, 64, 65, 1023, 1024, 1025, 1024 * 1024 + 3])
def test_compaction_and_gather_are_the_restatement(dev, p):
    rays, z = sample_set(p, p)
    cells = (5, 4, 3)
    box = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    flat = restate_classify(rays, z, box, cells, np.ones(cells, bool))[0].reshape(-1)
    masks = {"none": np.zeros(cells, bool), "all": np.ones(cells, bool), "random": random_mask(cells, 5, 0.4)}
    kept = {name: check_compaction(dev, rays, z, NpGrid(mask, box, dev)) for name, mask in masks.items()}
    assert kept["none"] == 0 and kept["all"] == int(flat.sum()) and (p < 63 or 0 < kept["random"] < kept["all"] < p)
    # only the first / only the last sample kept: that sample moved into a cell of its own
    for which in (0, p - 1):
        r2, z2 = rays.copy(), z.copy().reshape(-1)
        z2[:] = 5.0                                                         # every point leaves the box ...
        z2[which] = 0.0                                                     # ... but this one, which sits at its origin
        r2[:, 0:3] = (0.5, 0.5, 0.5)
        r2[:, 3:6] = (1.0, 1.0, 1.0)
        assert check_compaction(dev, r2, z2.reshape(z.shape), NpGrid(np.ones(cells, bool), box, dev)) == 1
    if p == 1025:                                                           # a capacity below n_kept
        assert kept["all"] > 10
        check_compaction(dev, rays, z, NpGrid(masks["all"], box, dev), capacity=10)
        check_compaction(dev, rays, z, NpGrid(masks["all"], box, dev), capacity=0)


@pytest.mark.gpu
def test_faces_outside_and_nan_depths(dev):
    """Points exactly on both faces of the box, outside it, and with a non-finite depth, against the restatement - and by hand."""
    box = (-1.0, 0.0, 0.5, 1.0, 2.0, 1.0)
    cells = (4, 3, 2)
    rays = np.zeros((6, 8), np.float32)
    rays[:, 0:3] = (0.0, 1.0, 0.75)
    rays[:, 3:6] = np.eye(3, dtype=np.float32).repeat(2, axis=0) * np.array([1, -1] * 3, np.float32)[:, None]
    z = np.tile(np.array([0.0, 0.25, 1.0, 1.5, np.nan, np.inf, -0.25, 0.999999], np.float32), (6, 1))
    grid = NpGrid(np.ones(cells, bool), box, dev)
    check_compaction(dev, rays, z, grid)
    keep = restate_classify(rays, z, grid.bounds, grid.cells, grid.mask)[0]
    # +x from the centre: x = 1 is the far face (t = cells: out), x = -1 the near face (t = 0: in); NaN and inf depths are culled
    assert keep[0].tolist() == [True, True, False, False, False, False, True, True]
    assert keep[1].tolist() == [True, True, True, False, False, False, True, True]
    assert keep[4].tolist() == [True, False, False, False, False, False, True, False]              # z axis: the box is 0.5 .. 1.0
    assert keep[5].tolist() == [True, True, False, False, False, False, False, False]


_MODELS = {}


def models_of(name, dev):
    import nerf
    if name not in _MODELS:
        kw, wfn = NETS[name]
        out = []
        for sd in wfn():
            m = nerf.models.FlexibleNeRFModel(**kw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            out.append(m.to(dev))
        _MODELS[name] = out
    return _MODELS[name]


_RAYS = {}


def rays_37(dev):
    """37 rays of a synthetic camera looking at the box -> (ro, rd) on the device"""
    import nerf
    from nerf import synthetic as syn
    if "r" not in _RAYS:
        h = w = 40
        e_mat = torch.from_numpy(syn.scene_pose(3)).to(dev)
        k_mat = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
        ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), e_mat, k_mat)
        sel = torch.from_numpy(syn.select_rays(h, w, 37, seed=5)).to(dev)
        _RAYS["r"] = (ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous())
    return _RAYS["r"]


def oracle_pass(pack, rays, z, mask, bounds):
    """sigma column of one culled pass from the numpy classification and run_network_pts on the kept points -> (rf, n_kept)"""
    from nerf import _ops
    keep, x, _ = restate_classify(C(rays), C(z), bounds, mask.shape, mask)
    sigma = np.full(keep.shape, FILL, np.float32)
    if keep.any():
        sigma[keep] = C(_ops.run_network_pts(pack, G(x[keep], rays.device), None, 1))[:, 3]
    rf = torch.zeros(keep.shape + (4,), dtype=torch.float32, device=rays.device)
    rf[..., 3] = G(sigma, rays.device)
    return rf, int(keep.sum())


def oracle_render(models, ro, rd, nc, nf, mask, bounds, thres, std=0.0, perturb=False, quantiles=None, interp=False, chunksize=4096):
    """The culled render composed of entry points the library had before -> (flat maps like render_dex_depth's in train mode, kept
    counts per chunk and pass).  Draws come from train_utils._draws in the render's order."""
    from nerf import _ops, train_utils
    fine = nf > 0
    prec = _ops._precision
    packs = [m.packed_density(True, True, precision=prec) for m in models[:2 if fine else 1]]
    rays_all = _ops.pack_ray_rows(ro, rd, None, 2.0, 6.0)
    th = torch.tensor(list(thres), dtype=torch.float32, device=ro.device)
    chunks, kept = [], []
    for r0 in range(0, rays_all.shape[0], chunksize):
        rays = rays_all[r0:r0 + chunksize]
        d = train_utils._draws(rays.shape[0], nc, nf, fine, perturb, std, ro.device)
        z = _ops.coarse_depths(rays, nc, False, d.get("t_rand"))
        rf, k_c = oracle_pass(packs[0], rays, z, mask, bounds)
        k_f = 0
        if fine:
            depth_c, acc_c, z = _ops.density_resample(rf, z, rays[:, 3:6], nf, d.get("noise_c"), std, d.get("u"))
            rf, k_f = oracle_pass(packs[1], rays, z, mask, bounds)
        noise = d.get("noise_f") if fine else d.get("noise_c")
        if quantiles is None:
            depth, acc, dex = _ops.composite_density(rf, z, rays[:, 3:6], noise, std, th)
            q = []
        else:
            depth, acc, dex, qd = _ops.composite_density_quantiles(rf, z, rays[:, 3:6], noise, std, th, quantiles, interp)
            q = list(qd)
        chunks.append(([depth_c, acc_c, depth, acc] if fine else [depth, acc, None, None]) + list(dex) + q + [z[:, 0]])
        kept.append((k_c, k_f))
    maps = [torch.cat(col) if col[0] is not None else None for col in zip(*chunks)]
    return maps[:-1], kept, maps[-1]


def culled_render(models, ro, rd, nc, nf, grid, thres, std=0.0, perturb=False, chunksize=4096, **kw):
    import nerf
    with torch.no_grad():
        return nerf.render_dex_depth(1, ro.shape[0], 1.0, models[0], models[1] if nf else None, ro, rd,
                                     make_cfg(nc, nf, chunksize, radiance_field_noise_std=std, perturb=perturb), mode="train",
                                     encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(thres), occupancy=grid, **kw)


def assert_same_maps(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert same_bits(C(a), C(b)), i


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [NF, 0])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_culled_render_is_the_oracle_bit_for_bit(dev, name, precision, nf):
    import nerf
    nerf.set_precision(precision)
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    want, kept, _ = oracle_render(models, ro, rd, NC, nf, mask, BOX, M_THRES)
    *got, stats = culled_render(models, ro, rd, NC, nf, grid, M_THRES, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == kept[0] and stats["total"] == (37 * NC, 37 * (NC + nf) if nf else 0) and stats["nonfinite"] == 0
    assert 0 < kept[0][0] < 37 * NC and (nf == 0 or 0 < kept[0][1] < 37 * (NC + nf))             # the grid culls some and keeps some
    assert len(culled_render(models, ro, rd, NC, nf, grid, M_THRES)) == len(got)                   # without cull_stats: the maps alone


@pytest.mark.gpu
def test_an_empty_grid_launches_no_network(dev, monkeypatch):
    import nerf
    from nerf import _ops
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    mask = np.zeros((4, 4, 4), bool)
    want, kept, z0 = oracle_render(models, ro, rd, NC, NF, mask, BOX, M_THRES)

    def no_launch(*a, **k):
        raise AssertionError("the network ran although no sample was kept")
    monkeypatch.setattr(_ops, "run_network_pts", no_launch)
    *got, stats = culled_render(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == (0, 0) and kept == [(0, 0)]
    for m in got[:4]:
        assert not C(m).any()                                               # depth = 0, acc = 0 in both passes
    for m in got[4:]:
        assert same_bits(C(m), C(z0))                                       # no crossing: the Dex depth falls back to z[0]


@pytest.mark.gpu
def test_chunks_that_keep_nothing_and_chunks_that_keep_some(dev):
    import nerf
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    ro = ro.clone()
    ro[:16, 0] += 100.0                                                     # the first chunk of 16 rays never meets the box
    mask = random_mask((8, 7, 6), 11)
    want, kept, _ = oracle_render(models, ro, rd, NC, NF, mask, BOX, M_THRES, chunksize=16)
    assert len(kept) == 3 and kept[0] == (0, 0) and kept[1][0] > 0 and kept[1][1] > 0
    *got, stats = culled_render(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, chunksize=16, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == tuple(sum(k[p] for k in kept) for p in range(2))


@pytest.mark.gpu
def test_perturb_and_noise_leave_the_generator_where_the_full_render_does(dev):
    import nerf
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    torch.manual_seed(7)
    want, _, _ = oracle_render(models, ro, rd, NC, NF, mask, BOX, M_THRES, std=1.0, perturb=True)
    torch.manual_seed(7)
    got = culled_render(models, ro, rd, NC, NF, grid, M_THRES, std=1.0, perturb=True)
    state = torch.cuda.get_rng_state(dev)
    assert_same_maps(got, want)
    torch.manual_seed(7)
    with torch.no_grad():
        nerf.render_dex_depth(1, 37, 1.0, models[0], models[1], ro, rd, make_cfg(NC, NF, radiance_field_noise_std=1.0, perturb=True), mode="train",
                              encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(M_THRES))
    assert torch.equal(state, torch.cuda.get_rng_state(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [False, True])
def test_three_quantiles(dev, interp):
    import nerf
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    qs = [0.1, 0.5, 0.9]
    want, _, _ = oracle_render(models, ro, rd, NC, NF, mask, BOX, M_THRES, quantiles=qs, interp=interp)
    got = culled_render(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, quantiles=qs, quantile_interp=interp)
    assert len(got) == 4 + len(M_THRES) + 3
    assert_same_maps(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_from_networks_is_the_build_on_density_grids_field(dev, precision):
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    models = models_of("lego", dev)
    ex = nerf.get_embedding_function(10)
    cells, level = (9, 8, 7), 1.0
    with torch.no_grad():
        grid = nerf.OccupancyGrid.from_networks(models, ex, BOX, cells, level=level, dilate=1, max_points=301)
        want = np.zeros(cells, bool)
        singles = []
        for m in models:
            field = nerf.density_grid(m, ex, BOX, tuple(c + 1 for c in cells))[0]
            singles.append(restate_build(C(field), level, 1))
            assert np.array_equal(bits_of(_ops.occupancy_build(field, cells, level, 1)), pack_bits(singles[-1]))
            want |= singles[-1]
    assert np.array_equal(bits_of(grid.bits), pack_bits(want)) and np.array_equal(C(grid.to_mask()), want)
    assert grid.bits.device == dev and 0 < want.mean() == pytest.approx(grid.occupied_fraction())
    assert not np.array_equal(singles[0], singles[1])                       # the OR has something to do


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NETS))
def test_a_full_grid_renders_what_the_full_render_does(dev, name):
    """All cells set and bounds that enclose every sample: the culled render differs from render_dex_depth without a grid only in how
    the network kernel gets its points - explicit points against rays + depths.  Measured on the parent commit on this test's points
    (37 rays, 37 / 59 / 64 samples, both networks of both shapes, fp32 and bf16): the largest |sigma| difference between
    run_network_rays and run_network_pts is 0 - the first assertion here repeats that measurement - so every map must be bit-equal."""
    import nerf
    from nerf import _ops
    nerf.set_precision("fp32")
    nerf.set_render_policy("bf16")                                         # (the configured precision: no fp16 instance under 'fp32' either way)
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    rays = _ops.pack_ray_rows(ro, rd, None, 2.0, 6.0)
    z = _ops.coarse_depths(rays, NC + NF, False)
    with torch.no_grad():
        for m in models:
            pack = m.packed_density(True, True, precision=_ops._precision)
            pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
            assert same_bits(C(_ops.run_network_rays(pack, rays, z))[..., 3].reshape(-1), C(_ops.run_network_pts(pack, pts, None, 1))[:, 3])
    wide = (-12.0, -12.0, -12.0, 12.0, 12.0, 12.0)
    grid = nerf.OccupancyGrid.from_mask(torch.ones(3, 5, 4, dtype=torch.bool, device=dev), wide)
    for nf in (NF, 0):
        *got, stats = culled_render(models, ro, rd, NC, nf, grid, M_THRES, cull_stats=True)
        assert stats["kept"] == stats["total"]                              # the box encloses every sample
        with torch.no_grad():
            full = nerf.render_dex_depth(1, 37, 1.0, models[0], models[1] if nf else None, ro, rd, make_cfg(NC, nf), mode="train",
                                         encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(M_THRES))
        assert_same_maps(got, full)


@pytest.mark.gpu
def test_eval_driver_with_an_occupancy_grid(dev, tmp_path, capsys):
    """eval_nerf.py --depth-only --occupancy: the default bounds hold every sample, so a grid set everywhere (level below every density)
    renders the plain depth-only maps bit for bit; --occupancy-check reports it per threshold."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "2", "--num-fine", "64", "--precision", "fp32", "--depth-only", "--m-thres", "20"]
    plain = eval_nerf.main(common + ["--quiet"])
    res = eval_nerf.main(common + ["--occupancy", "12,10,8", "--occupancy-level=-1e30", "--occupancy-dilate", "0", "--occupancy-check"])
    assert res["occupancy"].cells == (12, 10, 8) and res["occupancy"].occupied_fraction() == 1.0
    assert res["cull"]["kept"] == res["cull"]["total"] == [2 * 24 * 24 * 64, 2 * 24 * 24 * 128] and res["cull"]["nonfinite"] == 0
    assert res["occupancy_check"]["equal"] == [1.0] * 4 and res["occupancy_check"]["max_diff"] == [0.0] * 4
    for (_, depth, dex), (_, depth_plain, dex_plain) in zip(res["frames"], plain["frames"]):
        assert_same_maps([depth] + list(dex), [depth_plain] + list(dex_plain))
    text = capsys.readouterr().out
    assert "occupancy grid 12x10x8" in text and "occupancy check m_thres  20: 100.000 % of the pixels equal" in text
    # a real grid of the two networks culls something and still reports
    res = eval_nerf.main(common + ["--quiet", "--occupancy", "16", "--occupancy-level", "5", "--occupancy-check"])
    assert 0 < sum(res["cull"]["kept"]) < sum(res["cull"]["total"]) and len(res["occupancy_check"]["equal"]) == 4
