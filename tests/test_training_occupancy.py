"""Training on ray spans of an occupancy grid kept live on the device (include/dexnerf_hip_live.h, nerf.LiveOccupancyGrid,
nerf.FusedTrainStep(ray_span=...), train_dexnerf.py --train-occupancy, eval_nerf.py --ray-span checkpoint).

The two kernels are pinned bit for bit to a numpy restatement of the header's text (restate_points, restate_update), whose points come
from oracle.exact_rng and whose rules are pinned without a GPU on hand-made cases.  The fused step is pinned to a twin without a grid
(all-set and all-clear grids change nothing) and to OccupancyGrid.ray_spans of the twin's rows; a replayed loop to an eager one.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import D4, lego_weights
from oracle.exact_rng import rng_words
from test_input_gradients import make_cfg
from test_render_loss import _restore_modes, dev, flat_params, scene  # noqa: F401  (_restore_modes, dev, scene: fixtures)

LIVE = ("dn_occupancy_cell_points", "dn_occupancy_ema_workspace_bytes", "dn_occupancy_ema_update")
INVAL = -1000
F = np.float32
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
ODD_BOX = (-1.25, -0.5, 0.125, 1.0, 1.75, 2.5)
WIDE_BOX = (-19.0, -19.5, -20.0, 19.0, 19.5, 20.0)       # encloses [near, far] of every ray of the training scene (|ro| < 5, far 6)
KERNEL_CELLS = [(3, 3, 3), (7, 5, 2), (6, 5, 4), (8, 8, 8)]
RNG_STREAM_CELL = 6
STEP_RAYS, STEP_NC, STEP_NF = 64, 10, 8      # 10 coarse samples: the fewest dn_fine_depths takes (10 <= num_coarse)


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def cell_sizes(bounds, cells):
    b = np.asarray(bounds, F)
    return np.array([F((float(b[a + 3]) - float(b[a])) / cells[a]) for a in range(3)], F)


def restate_points(bounds, cells, seed, iteration, c0=0, n=None):
    """The header's cell points: x_a = b0_a + ((float)i_a + u_a) * h_a, every operation one fp32 numpy operation."""
    total = cells[0] * cells[1] * cells[2]
    n = total - c0 if n is None else n
    c = np.arange(c0, c0 + n, dtype=np.int64)
    idx = np.stack(np.unravel_index(c, cells), axis=1)
    w = rng_words(seed, iteration, RNG_STREAM_CELL, c.astype(np.uint64))
    b0, h = np.asarray(bounds, F)[:3], cell_sizes(bounds, cells)
    out = np.empty((n, 3), F)
    for a in range(3):
        u = (np.asarray(w[a]) >> np.uint64(8)).astype(F) * F(1.0 / 16777216.0)
        t = idx[:, a].astype(F) + u
        t = t * h[a]
        out[:, a] = b0[a] + t
        assert t.dtype == F
    return out


def pack_mask(mask):
    flat = np.asarray(mask, bool).reshape(-1)
    packed = np.zeros(4 * ((flat.size + 31) // 32), np.uint8)
    by = np.packbits(flat, bitorder="little")
    packed[:by.size] = by
    return packed.view("<u4").astype(np.uint32)


def unpack_bits(words, cells):
    n = cells[0] * cells[1] * cells[2]
    return np.unpackbits(np.asarray(words).view(np.uint32).astype("<u4").view(np.uint8), bitorder="little")[:n].astype(bool).reshape(cells)


def all_set_words(cells):
    return pack_mask(np.ones(cells, bool))


def dilate_mask(raw, d):
    """The OR over the Chebyshev neighbourhood d, clipped to the grid (include/dexnerf_hip_occupancy.h "Build")."""
    out = np.zeros_like(raw)
    cx, cy, cz = raw.shape
    for di in range(-d, d + 1):
        for dj in range(-d, d + 1):
            for dk in range(-d, d + 1):
                if abs(di) >= cx or abs(dj) >= cy or abs(dk) >= cz:      # the shifted grid does not meet the grid
                    continue
                src = raw[max(di, 0):cx + min(di, 0), max(dj, 0):cy + min(dj, 0), max(dk, 0):cz + min(dk, 0)]
                out[max(-di, 0):cx + min(-di, 0), max(-dj, 0):cy + min(-dj, 0), max(-dk, 0):cz + min(-dk, 0)] |= src
    return out


def restate_update(columns, ema, cells, decay, level, write_bits, dilate, words):
    """The header's update -> (ema', words'): words untouched without write_bits."""
    a = np.asarray(columns[0], F)
    with np.errstate(all="ignore"):
        hot = ~np.isfinite(a)
        s = a
        if len(columns) == 2:
            b = np.asarray(columns[1], F)
            hot = hot | ~np.isfinite(b)
            s = np.where(b > a, b, a)
        d = np.asarray(ema, F) * F(decay)
        e = np.where(hot, d, np.where(s > d, s, d))
        assert d.dtype == F and e.dtype == F
        raw = hot | (e > F(level))
    if not write_bits:
        return e, np.array(words, np.uint32, copy=True)
    return e, pack_mask(dilate_mask(raw.reshape(cells), dilate))


def record(seed, updates_done):
    """The grid's rng record after `updates_done` refreshes, as int32 words."""
    if updates_done == 0:
        words = [seed & 0xFFFFFFFF, seed >> 32, 0, 0]
    else:
        words = [seed & 0xFFFFFFFF, seed >> 32, updates_done - 1, updates_done]
    return np.array(words, np.uint32).view(np.int32).tolist()


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_live_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_live.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.LIVE_EXPORTS) == set(LIVE)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS) | set(_hip.OCCUPANCY_EXPORTS) | set(_hip.CULL_EXPORTS) | set(_hip.REFINE_EXPORTS)
             | set(_hip.SPAN_EXPORTS) | set(_hip.LAYERS_EXPORTS))
    assert not older & set(LIVE) and len(_hip.EXPORTS) == 76
    assert "dexnerf_hip_live.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()           # build() checks the new header's symbols too
    assert "occupancy_live.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    assert "kRngStreamCell = 6" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "dn_rng.h")).read() and _hip.RNG_STREAM_CELL == RNG_STREAM_CELL
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in LIVE) and hiplib.dn_abi_version() == 2


def test_live_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    fake, other, odd = ctypes.c_void_p(256 * 4096), ctypes.c_void_p(512 * 4096), ctypes.c_void_p(256 * 4096 + 2)
    nan, inf = float("nan"), float("inf")
    past = (dict(cx=0), dict(cy=-1), dict(cx=(1 << 24) + 1), dict(cx=1 << 12, cy=1 << 12, cz=1 << 12))
    call = dict(a=fake, sa=4, b=fake, sb=1, cx=7, cy=5, cz=2, decay=0.95, level=0.01, write=1, dilate=1, ema=fake, bits=fake, scratch=other,
                rng=fake, stream=None)
    for kw in past + (dict(decay=0.0), dict(decay=1.5), dict(decay=-0.5), dict(decay=nan), dict(decay=inf), dict(level=-0.5), dict(level=nan),
                      dict(level=inf), dict(dilate=9), dict(dilate=-1), dict(a=None), dict(a=None, b=None), dict(sa=0), dict(sb=-4),
                      dict(ema=None), dict(rng=None), dict(bits=None), dict(scratch=None), dict(scratch=fake), dict(a=odd), dict(b=odd),
                      dict(ema=odd), dict(bits=odd), dict(scratch=odd), dict(rng=odd)):
        assert hiplib.dn_occupancy_ema_update(*{**call, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_ema_update" in hiplib.dn_last_error(), kw
    call = dict(cx=7, cy=5, cz=2, x0=-1.0, y0=-1.0, z0=-1.0, hx=0.25, hy=0.5, hz=1.0, c0=0, n=70, rng=fake, pts=fake, stream=None)
    for kw in past + (dict(x0=nan), dict(y0=inf), dict(hx=0.0), dict(hy=-1.0), dict(hz=nan), dict(hx=inf), dict(c0=-1), dict(n=0), dict(n=71),
                      dict(c0=70, n=1), dict(c0=64, n=7), dict(c0=1 << 40), dict(n=-(1 << 40)), dict(rng=None), dict(pts=None), dict(rng=odd),
                      dict(pts=odd)):
        assert hiplib.dn_occupancy_cell_points(*{**call, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_cell_points" in hiplib.dn_last_error(), kw
    assert hiplib.dn_occupancy_ema_workspace_bytes(7, 5, 2, 1) == 4 * 3 == 4 * hiplib.dn_occupancy_words(7, 5, 2)
    assert hiplib.dn_occupancy_ema_workspace_bytes(128, 128, 128, 0) == 4 * (128 ** 3 // 32)
    for bad in ((0, 5, 2, 1), (7, 5, 2, 9), (7, 5, 2, -1), ((1 << 24) + 1, 1, 1, 0), (1 << 12, 1 << 12, 1 << 12, 1)):
        assert hiplib.dn_occupancy_ema_workspace_bytes(*bad) == 0, bad


def small_model(which=1):
    import nerf
    m = nerf.models.FlexibleNeRFModel(**D4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lego_weights()[which].items()})
    return m


def test_the_python_layer_refuses_before_any_launch(hiplib):
    import nerf
    ex = nerf.get_embedding_function(10)
    for kw in (dict(decay=0.0), dict(decay=1.5), dict(decay=float("nan")), dict(level=-1.0), dict(level=float("nan")), dict(level=float("inf")),
               dict(level=1e39), dict(dilate=9), dict(dilate=-1), dict(warmup_updates=-1), dict(cells=0), dict(cells=(1 << 24) + 1),
               dict(cells=(1 << 12, 1 << 12, 1 << 12)), dict(bounds=(0, 0, 0, 1, 0, 1)), dict(bounds=(0, 0, 0, 1, 1, float("nan")))):
        args = dict(bounds=BOX, cells=4, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match="LiveOccupancyGrid"):
            nerf.LiveOccupancyGrid(**args)
    live = nerf.LiveOccupancyGrid(BOX, (7, 5, 2), "cpu")
    assert live.grid is live.grid and live.grid.bits is live.bits and live.occupied_fraction() == 1.0
    assert np.array_equal(live.bits.numpy().view(np.uint32), all_set_words((7, 5, 2))) and float(live.ema.abs().max()) == 0.0
    m = small_model()
    with pytest.raises(RuntimeError, match="ROCm device"):                                         # host tensors: no fallback
        live.update([m, m], ex)
    with pytest.raises(ValueError, match="one or two"):
        live.update([], ex)
    with pytest.raises(ValueError, match="one or two"):
        live.update([m, m, m], ex)
    with pytest.raises(ValueError, match="max_points"):
        live.update(m, ex, max_points=0)
    nerf.set_precision("fp16")
    try:
        with pytest.raises(RuntimeError, match="fp16"):
            live.update(m, ex)
    finally:
        nerf.set_precision("fp32")
    assert live.updates_done == 0 and live.rng_state.tolist() == record(0, 0)


def test_the_fused_step_refuses_before_any_launch(hiplib):
    """The refusals of FusedTrainStep(ray_span=...) come ahead of everything that needs a device: host networks suffice."""
    import nerf
    from nerf import parallel
    nets = [small_model(0), small_model(1)]
    bucket = parallel.FlatGradBucket(nets)
    cfg = make_cfg(dict(num_coarse=STEP_NC, num_fine=STEP_NF, near=2.0, far=6.0))
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    live = nerf.LiveOccupancyGrid(BOX, 4, "cpu")

    def step(**kw):
        return nerf.FusedTrainStep(nets[0], nets[1], None, cfg, bucket, ex, ed, STEP_RAYS, **kw)
    with pytest.raises(ValueError, match="occupancy_update_every"):
        step(ray_span=live, occupancy_update_every=0)
    for pad in (float("nan"), float("inf"), -1.0, "wide"):
        with pytest.raises(ValueError, match="ray_span_pad"):
            step(ray_span=live.grid, ray_span_pad=pad)
    with pytest.raises(ValueError, match="occupancy grid lives on"):                               # a grid on another device than the networks
        step(ray_span=nerf.OccupancyGrid(torch.zeros(2, dtype=torch.int32, device="meta"), BOX, 4))
    with pytest.raises(ValueError, match="OccupancyGrid"):
        step(ray_span=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="encoding anneal"):
        step(ray_span=live, encoding_anneal=nerf.EncodingAnneal(0, 10))


def test_training_occupancy_flags_are_judged_before_the_dataset_is_read():
    import train_dexnerf
    ok = ["--train-occupancy", "8", "--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1"]
    for argv in (["--occupancy-level", "0.5"], ["--occupancy-decay", "0.9"], ["--occupancy-every", "4"], ["--occupancy-warmup", "2"],
                 ["--ray-span-pad", "1"], ["--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1"], ["--train-occupancy", "8"],
                 ["--train-occupancy", "0"] + ok[2:], ["--train-occupancy", "2048"] + ok[2:],
                 ["--train-occupancy", "8", "--occupancy-bounds", "0", "0", "0", "1", "0", "1"], ok + ["--occupancy-level", "-1"],
                 ok + ["--occupancy-level", "nan"], ok + ["--occupancy-decay", "0"], ok + ["--occupancy-decay", "1.5"],
                 ok + ["--occupancy-every", "0"], ok + ["--occupancy-warmup", "-1"], ok + ["--ray-span-pad", "-1"],
                 ok + ["--ray-span-pad", "nan"], ok + ["--autograd-step"], ok + ["--refine-poses"], ok + ["--anneal-encoding", "0", "10"]):
        with pytest.raises(SystemExit):
            train_dexnerf.parse_args(argv)
    args = train_dexnerf.parse_args(ok)
    assert (args.occupancy_level, args.occupancy_decay, args.occupancy_every, args.occupancy_warmup, args.ray_span_pad) == (0.01, 0.95, 16, 4, 1.0)
    args = train_dexnerf.parse_args(ok + ["--occupancy-level", "0.5", "--occupancy-decay", "1", "--occupancy-every", "2", "--occupancy-warmup", "0",
                                          "--ray-span-pad", "0"])
    assert (args.occupancy_level, args.occupancy_decay, args.occupancy_every, args.occupancy_warmup, args.ray_span_pad) == (0.5, 1.0, 2, 0, 0.0)
    import eval_nerf
    base = ["--checkpoint", "none.ckpt", "--depth-only", "--m-thres", "20"]
    for argv in (base + ["--ray-span", "checkpoint", "--occupancy-level", "1"], base + ["--ray-span", "checkpoint", "--occupancy-dilate", "2"],
                 base + ["--ray-span", "checkpoint", "--ray-span-pad", "-1"], base + ["--ray-span", "check"]):
        with pytest.raises(SystemExit):
            eval_nerf.main(argv)
    with pytest.raises(FileNotFoundError):                                                         # complete flags reach the checkpoint
        eval_nerf.main(base + ["--ray-span", "checkpoint", "--ray-span-pad", "0.5"])


def test_the_restatement_on_hand_checked_cases():
    """The yardstick, pinned without a GPU, on a 4 x 1 x 1 grid."""
    cells = (4, 1, 1)
    keep = np.array([0xDEADBEEF], np.uint32)
    # a hot cell does not enter ema, and is set whatever the level
    ema, words = restate_update([np.array([np.inf, np.nan, 2.0, -3.0], F)], np.array([1.0, 0.5, 0.25, 0.0], F), cells, 0.5, 100.0, True, 0, keep)
    assert ema.tolist() == [0.5, 0.25, 2.0, 0.0] and unpack_bits(words, cells).reshape(-1).tolist() == [True, True, False, False]
    # decay = 1 is a running maximum; the second column enters through max
    ema = np.zeros(4, F)
    for col, other in (([1.0, -1.0, 0.0, 3.0], [0.0, 0.0, 0.0, 0.0]), ([0.5, 2.0, -5.0, 1.0], [0.25, 0.0, 7.0, 0.0]), ([-1.0] * 4, [-2.0] * 4)):
        ema, words = restate_update([np.array(col, F), np.array(other, F)], ema, cells, 1.0, 0.0, True, 0, keep)
    assert ema.tolist() == [1.0, 2.0, 7.0, 3.0]
    # e' > level is strict
    ema, words = restate_update([np.array([0.5, 0.50000006, 0.49999997, 0.0], F)], np.zeros(4, F), cells, 0.95, 0.5, True, 0, keep)
    assert unpack_bits(words, cells).reshape(-1).tolist() == [False, True, False, False] and int(words[0]) < 16      # tail bits are 0
    # the decay is applied before the maximum, in fp32
    ema, _ = restate_update([np.array([0.0, 1.0, 0.0, 0.0], F)], np.array([3.0, 3.0, 0.1, 0.0], F), cells, 0.95, 0.5, True, 0, keep)
    assert ema.tolist() == [float(F(3.0) * F(0.95)), float(F(3.0) * F(0.95)), float(F(0.1) * F(0.95)), 0.0]
    # with write_bits = 0 the bits are untouched, ema is not
    ema, words = restate_update([np.array([9.0, 9.0, 9.0, 9.0], F)], np.zeros(4, F), cells, 0.95, 0.5, False, 1, keep)
    assert words.tolist() == keep.tolist() and ema.tolist() == [9.0] * 4
    # the dilation is the Chebyshev neighbourhood, clipped to the grid
    raw = np.zeros((5, 4, 3), bool)
    raw[0, 0, 0] = raw[4, 2, 1] = True
    out = dilate_mask(raw, 1)
    assert out.sum() == 8 + 2 * 3 * 3 and out[:2, :2, :2].all() and out[3:, 1:, :].all() and np.array_equal(dilate_mask(raw, 0), raw)
    # the points: inside their cells (up to the upper face's rounding), one word per axis, another iteration draws others
    for cells, bounds in (((7, 5, 2), ODD_BOX), ((3, 3, 3), BOX)):
        pts = restate_points(bounds, cells, 11, 0)
        idx = np.stack(np.unravel_index(np.arange(pts.shape[0]), cells), axis=1)
        t = (pts.astype(np.float64) - np.asarray(bounds[:3])) / cell_sizes(bounds, cells).astype(np.float64) - idx
        assert t.min() > -1e-5 and t.max() < 1 + 1e-5 and t.std() > 0.2
        assert not np.array_equal(pts, restate_points(bounds, cells, 11, 1)) and not np.array_equal(pts, restate_points(bounds, cells, 12, 0))
        assert np.array_equal(restate_points(bounds, cells, 11, 0, 5, 9), pts[5:14])
    w = rng_words(11, 0, RNG_STREAM_CELL, np.array([3], np.uint64))
    assert float(restate_points(BOX, (3, 3, 3), 11, 0)[3, 0]) == float(F(-1.5) + (F(0.0) + F(int(w[0][0]) >> 8) * F(2.0 ** -24)) * F(1.0))


def test_state_dict_round_trips_on_the_host():
    import nerf
    live = nerf.LiveOccupancyGrid(ODD_BOX, (7, 5, 2), "cpu", level=0.5, decay=0.9, dilate=2, warmup_updates=3, seed=(5 << 32) + 9)
    live.ema.copy_(torch.arange(70, dtype=torch.float32))
    live.bits.copy_(torch.tensor([-5, 77, 3], dtype=torch.int32))
    live.rng_state.copy_(torch.tensor([9, 5, 6, 7], dtype=torch.int32))
    live.updates_done = 7
    state = live.state_dict()
    assert set(state) == {"ema", "bits", "bounds", "cells", "level", "decay", "dilate", "warmup_updates", "seed", "rng_state", "updates_done"}
    import io
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    back = nerf.LiveOccupancyGrid.from_state_dict(torch.load(buf))
    assert torch.equal(back.ema, live.ema) and torch.equal(back.bits, live.bits) and torch.equal(back.rng_state, live.rng_state)
    assert (back.bounds, back.cells, back.level, back.decay, back.dilate, back.warmup_updates, back.seed, back.updates_done) == \
        (live.bounds, live.cells, live.level, live.decay, live.dilate, live.warmup_updates, live.seed, 7)
    assert back.level == float(F(0.5)) and back.decay == float(F(0.9)) and back.sizes == live.sizes
    live.ema[0] = -1.0                                                                             # independent tensors
    assert float(back.ema[0]) == 0.0
    with pytest.raises(ValueError, match="do not fit"):
        nerf.LiveOccupancyGrid.from_state_dict({**state, "ema": torch.zeros(69)})


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def G(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def densities(n, seed, junk):
    """Raw densities, about one in twenty above the level 0.5, with exact ties and, with `junk`, +inf / -inf / NaN in a few cells."""
    rng = np.random.default_rng(seed)
    s = rng.normal(-1.2, 1.0, n).astype(F)
    s[rng.integers(0, n, max(n // 9, 1))] = F(0.5)
    if junk:
        s[rng.integers(0, n, 2)] = np.inf
        s[rng.integers(0, n, 1)] = np.nan
        s[rng.integers(0, n, 1)] = -np.inf
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["one column", "two columns", "rows of four", "rows of four, two", "no dilation"])
@pytest.mark.parametrize("cells", KERNEL_CELLS, ids=lambda c: "x".join(map(str, c)))
def test_kernels_are_the_restatement_bit_for_bit(dev, cells, variant):
    """Three consecutive refreshes through nerf._ops on made-up densities: pts, ema, bits and the rng record after each; the first one is
    a warm-up (write_bits = 0) on all-set bits.  The points also in slabs of 50 cells, the second refresh on."""
    from nerf import _ops
    bounds, seed = (ODD_BOX if cells[0] != cells[1] else BOX), (3 << 32) + 17
    b, c, _ = _ops.check_occupancy_grid(bounds, cells)
    sizes = _ops.occupancy_cell_sizes(b, c)
    assert same_bits(np.array(sizes, F), cell_sizes(bounds, cells))
    n = cells[0] * cells[1] * cells[2]
    two = "two" in variant
    strided = "rows of four" in variant
    dilate = 0 if variant == "no dilation" else 1
    decay, level = 0.95, 0.5
    rng_state = _ops.new_rng_state(seed, dev)
    ema = torch.zeros(n, dtype=torch.float32, device=dev)
    bits = G(all_set_words(cells).view(np.int32), dev)
    assert _ops.occupancy_ema_workspace_words(cells, dilate) == bits.numel()
    scratch = torch.zeros(bits.numel(), dtype=torch.int32, device=dev) if dilate else None
    want_ema, want_words = np.zeros(n, F), all_set_words(cells)
    seen = set()
    for k in range(3):
        if k == 0:
            pts = _ops.occupancy_cell_points(b, c, sizes, 0, n, rng_state)
        else:
            pts = torch.cat([_ops.occupancy_cell_points(b, c, sizes, c0, min(50, n - c0), rng_state) for c0 in range(0, n, 50)])
        assert same_bits(C(pts), restate_points(bounds, cells, seed, k))
        assert rng_state.tolist() == record(seed, k + 1)[:2] + [k, k]                              # cur follows nxt; nxt waits for the update
        host = [densities(n, 10 * k + q, junk=k > 0) for q in range(2 if two else 1)]
        if strided:
            rows = [torch.full((n, 4), float("nan"), device=dev) for _ in host]
            for r, h in zip(rows, host):
                r[:, 3] = G(h, dev)
            columns = [r[:, 3] for r in rows]
        else:
            columns = [G(h, dev) for h in host]
        _ops.occupancy_ema_update(columns, c, decay, level, k > 0, dilate, ema, bits, scratch, rng_state)
        want_ema, want_words = restate_update(host, want_ema, cells, decay, level, k > 0, dilate, want_words)
        assert same_bits(C(ema), want_ema)
        assert np.array_equal(C(bits).view(np.uint32), want_words)
        assert rng_state.tolist() == record(seed, k + 1)
        seen.add(want_words.tobytes())
    assert len(seen) == 3                                                                          # the bits moved with every refresh
    assert 0 < unpack_bits(want_words, cells).sum() < n


@pytest.mark.gpu
def test_the_build_gives_the_bits_it_gave_and_the_update_dilates_like_it(dev):
    """dn_occupancy_build after the dilation moved into a shared function: its bits against the numpy dilation of the corner rule, and
    the update's bits for the same raw cells."""
    from nerf import _ops
    cells = (7, 5, 2)
    rng = np.random.default_rng(3)
    field = rng.normal(-1.0, 1.0, tuple(c + 1 for c in cells)).astype(F)
    hot = field > F(0.0)
    raw = np.zeros(cells, bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                raw |= hot[di:di + cells[0], dj:dj + cells[1], dk:dk + cells[2]]
    assert 0 < raw.sum() < raw.size
    for d in (0, 1, 3):
        bits = _ops.occupancy_build(G(field, dev), cells, 0.0, d)
        assert np.array_equal(C(bits).view(np.uint32), pack_mask(dilate_mask(raw, d)))
        n = raw.size
        ema = torch.zeros(n, dtype=torch.float32, device=dev)
        live_bits = torch.zeros_like(bits)
        scratch = torch.zeros_like(bits)
        _ops.occupancy_ema_update([G(raw.reshape(-1).astype(F), dev)], cells, 1.0, 0.5, True, d, ema, live_bits, scratch, _ops.new_rng_state(0, dev))
        assert torch.equal(live_bits, bits)


_CACHE = {}


def lego_models(dev):
    if "m" not in _CACHE:
        _CACHE["m"] = [small_model(w).to(dev) for w in (0, 1)]
    return _CACHE["m"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_live_grid_update_on_the_lego_networks(dev, precision):
    """LiveOccupancyGrid.update on the lego 4x128 weights: ema and bits are the restatement fed with _ops.run_network_pts - the entry
    point update() runs - on the restated points; a grid refreshed in slabs of 50 cells holds the same bits."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    models = lego_models(dev)
    ex = nerf.get_embedding_function(10)
    cells, seed, level = (6, 5, 4), 5, 0.5
    live = nerf.LiveOccupancyGrid(BOX, cells, dev, level=level, decay=0.9, dilate=1, warmup_updates=1, seed=seed)
    slabbed = nerf.LiveOccupancyGrid(BOX, cells, dev, level=level, decay=0.9, dilate=1, warmup_updates=1, seed=seed)
    bits_tensor = live.grid.bits
    want_ema, want_words = np.zeros(120, F), all_set_words(cells)
    with torch.no_grad():
        packs = [m.packed_density(True, True, precision=_ops._precision) for m in models]
    for k in range(3):
        live.update(models, ex)
        slabbed.update(models, ex, max_points=50)
        pts = G(restate_points(BOX, cells, seed, k), dev)
        with torch.no_grad():
            host = [C(_ops.run_network_pts(p, pts, None, 1)[:, 3]) for p in packs]
        want_ema, want_words = restate_update(host, want_ema, cells, live.decay, live.level, k >= 1, 1, want_words)
        assert same_bits(C(live.ema), want_ema) and np.array_equal(C(live.bits).view(np.uint32), want_words)
        assert live.rng_state.tolist() == record(seed, k + 1) and live.updates_done == k + 1
        assert torch.equal(slabbed.ema, live.ema) and torch.equal(slabbed.bits, live.bits) and torch.equal(slabbed.rng_state, live.rng_state)
    assert live.grid.bits is bits_tensor and live.grid.bits.data_ptr() == bits_tensor.data_ptr()   # written in place, never replaced
    fraction = live.occupied_fraction()
    print(f"lego {precision}: ema max {float(live.ema.max()):.3f}, {100 * fraction:.1f} % of {cells} set at level {level}")
    assert float(live.ema.max()) > level and 0.0 < fraction
    one = nerf.LiveOccupancyGrid(BOX, cells, dev, level=level, decay=0.9, dilate=1, warmup_updates=0, seed=seed)     # one network, no warm-up
    one.update(models[1], ex)
    pts = G(restate_points(BOX, cells, seed, 0), dev)
    with torch.no_grad():
        host = [C(_ops.run_network_pts(packs[1], pts, None, 1)[:, 3])]
    e, w = restate_update(host, np.zeros(120, F), cells, one.decay, one.level, True, 1, all_set_words(cells))
    assert same_bits(C(one.ema), e) and np.array_equal(C(one.bits).view(np.uint32), w)


def small_step(scene, dev, seed=31, init=5, **kw):
    """A fresh 4x128 student pair (torch's default init from `init`), its bucket and a FusedTrainStep on the scene: 64 rays, 10 + 8
    samples - the fewest coarse samples the sampler takes -, every ray's view drawn with its pixel."""
    import nerf
    from nerf import parallel
    torch.manual_seed(init)
    nets = [nerf.models.FlexibleNeRFModel(**D4).to(dev) for _ in range(2)]
    bucket = parallel.FlatGradBucket(nets)
    cfg = make_cfg(dict(num_coarse=STEP_NC, num_fine=STEP_NF, near=2.0, far=6.0, perturb=True, noise_std=0.0, white_background=False))
    step = nerf.FusedTrainStep(nets[0], nets[1], scene.sel, cfg, bucket, scene.ex, scene.ed, STEP_RAYS, seed=seed, draw_view="rays", **kw)
    return step, bucket, nets


def run_steps(step, bucket, n, use_graphs=False, opt=None):
    import nerf
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True) if opt is None else opt
    graphed = nerf.GraphedTrainStep(step, opt, eager_iterations=1, use_graphs=use_graphs)
    for _ in range(n):
        graphed.step()
    torch.cuda.synchronize()
    return graphed, opt


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_set_and_empty_grids_leave_training_alone(dev, scene, precision):
    """A grid set everywhere whose box encloses every ray's [near, far] segment clips nothing, and in an all-clear grid every ray is a
    miss: by the span's definition both leave the rows' bits alone, so three steps end in the twin's loss, parameters and rows."""
    import nerf
    nerf.set_precision(precision)
    twin, bucket, nets = small_step(scene, dev)
    run_steps(twin, bucket, 3)
    want = (twin.loss3.clone(), flat_params(nets).clone(), twin.latest_draw()[2].clone())
    assert want[2].shape == (STEP_RAYS, 11) and bool(torch.isfinite(want[1]).all())
    cells = (6, 5, 4)
    full = nerf.OccupancyGrid.from_mask(torch.ones(cells, dtype=torch.bool, device=dev), WIDE_BOX)
    empty = nerf.OccupancyGrid.from_mask(torch.zeros(cells, dtype=torch.bool, device=dev), BOX)
    for grid in (full, empty):
        for pad in (0.0, 1.0):
            step, bucket, nets = small_step(scene, dev, ray_span=grid, ray_span_pad=pad)
            run_steps(step, bucket, 3)
            assert torch.equal(step.loss3, want[0]) and torch.equal(flat_params(nets), want[1])
            assert same_bits(C(step.latest_draw()[2]), C(want[2]))
    # a box that does not enclose the rays: columns 6 / 7 differ and nothing else in the rows does
    tight = nerf.OccupancyGrid.from_mask(torch.ones(cells, dtype=torch.bool, device=dev), BOX)
    step, bucket, nets = small_step(scene, dev, ray_span=tight, ray_span_pad=0.0)
    run_steps(step, bucket, 1)
    twin, bucket, nets = small_step(scene, dev)
    run_steps(twin, bucket, 1)
    rows, plain = C(step.latest_draw()[2]), C(twin.latest_draw()[2])
    assert same_bits(rows[:, :6], plain[:, :6]) and same_bits(rows[:, 8:], plain[:, 8:]) and not same_bits(rows[:, 6:8], plain[:, 6:8])
    assert (rows[:, 6] >= plain[:, 6]).all() and (rows[:, 7] <= plain[:, 7]).all() and not torch.equal(step.loss3, twin.loss3)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_step_tightens_with_the_span_kernels_bits(dev, scene, precision):
    """A half-set grid: columns 6 / 7 of the step's rows are grid.ray_spans of the twin's untightened rows, and the loss is that of the
    chunk entry points run on those rows with the iteration's draws."""
    import nerf
    from nerf import _ops
    nerf.set_precision(precision)
    mask = np.random.default_rng(4).random((8, 7, 6)) < 0.5
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    pad = 0.5
    step, bucket, nets = small_step(scene, dev, ray_span=grid, ray_span_pad=pad)
    twin, bucket_t, nets_t = small_step(scene, dev)
    for s, b in ((step, bucket), (twin, bucket_t)):
        b.zero()
        s.forward_and_fine_backward(_zero=False, both=True)
    rows, plain = step.latest_draw()[2], twin.latest_draw()[2]
    span, visits = grid.ray_spans(plain, pad_cells=pad)
    hit = C(visits) > 0
    assert 0 < hit.sum() and not same_bits(C(span)[hit], C(plain)[hit, 6:8])
    want = C(plain).copy()
    want[hit, 6:8] = C(span)[hit]
    assert same_bits(C(rows), want) and torch.equal(step.latest_draw()[3], twin.latest_draw()[3])
    peek = _ops.new_rng_state(31, dev, 0)
    pc, pf, prec = _ops.pack_train_pair(nets[0], nets[1], step.logs)
    maps, saved = _ops.render_rays_train(pc, pf, G(want, dev), STEP_NC, STEP_NF, False, 0.0, False, [], None, prec=prec, rng_state=peek, perturb=True)
    loss3, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], step.latest_draw()[3])
    assert torch.equal(loss3, step.loss3) and not torch.equal(step.loss3, twin.loss3)


def live_run(scene, dev, n, use_graphs, live=None, first_iteration=0, resume=None):
    import nerf
    if live is None:
        live = nerf.LiveOccupancyGrid(BOX, (8, 8, 8), dev, level=0.08, decay=0.9, dilate=0, warmup_updates=1, seed=77)
    step, bucket, nets = small_step(scene, dev, ray_span=live, ray_span_pad=1.0, occupancy_update_every=2, first_iteration=first_iteration)
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    if resume is not None:
        for net, sd in zip(nets, resume["nets"]):
            net.load_state_dict(sd)
        nerf.models.mark_parameters_updated()
        opt.load_state_dict(resume["opt"])
    graphed, opt = run_steps(step, bucket, n, use_graphs=use_graphs, opt=opt)
    assert graphed.fallback_reason is None and (graphed.graphs is not None) == use_graphs, graphed.fallback_reason
    return live, nets, opt, step


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replayed_is_eager_and_a_resumed_grid_goes_on(dev, scene, precision):
    """8 steps with a live 8^3 grid refreshed before iterations 0, 2, 4, 6 (one warm-up refresh): the capture happens at iteration 1, so
    three refreshes fall between replays of the one graph, which reads the bits they wrote in place.  Replayed and eager loops end in
    the same parameters, ema, bits and rng record; so does a loop resumed from the state after step 4."""
    import copy

    import nerf
    nerf.set_precision(precision)
    eager = live_run(scene, dev, 8, False)
    replayed = live_run(scene, dev, 8, True)
    for a, b in ((eager, replayed),):
        assert torch.equal(flat_params(a[1]), flat_params(b[1])) and torch.equal(a[3].loss3, b[3].loss3)
        assert torch.equal(a[0].ema, b[0].ema) and torch.equal(a[0].bits, b[0].bits) and torch.equal(a[0].rng_state, b[0].rng_state)
    live = eager[0]
    assert live.updates_done == 4 and live.rng_state.tolist() == record(77, 4) and eager[3].rng_state.tolist()[2:] == [7, 8]
    fraction = live.occupied_fraction()
    print(f"{precision}: after 8 steps ema max {float(live.ema.max()):.4f}, {100 * fraction:.1f} % of 8^3 set")
    assert float(live.ema.max()) > 0.0 and bool(torch.isfinite(flat_params(eager[1])).all())
    plain, bucket, nets = small_step(scene, dev)
    run_steps(plain, bucket, 8)
    if 0.0 < fraction < 1.0:                                                                       # the grid did steer the training
        assert not torch.equal(flat_params(nets), flat_params(eager[1]))
    half = live_run(scene, dev, 4, False)
    state = copy.deepcopy(dict(grid=half[0].state_dict(), nets=[m.state_dict() for m in half[1]], opt=half[2].state_dict()))
    assert state["grid"]["updates_done"] == 2
    resumed = live_run(scene, dev, 4, True, live=nerf.LiveOccupancyGrid.from_state_dict(state["grid"], dev), first_iteration=4, resume=state)
    assert torch.equal(resumed[0].ema, live.ema) and torch.equal(resumed[0].bits, live.bits) and torch.equal(resumed[0].rng_state, live.rng_state)
    assert torch.equal(flat_params(resumed[1]), flat_params(eager[1]))


@pytest.mark.gpu
def test_training_driver_keeps_stores_and_resumes_the_grid(dev, tmp_path):
    """train_dexnerf.py --train-occupancy 8 on the synthetic scene: the checkpoint carries the grid, --load-checkpoint goes on with it,
    and eval_nerf.py --depth-only --ray-span checkpoint renders from it."""
    import eval_nerf
    import nerf
    import train_dexnerf
    ck_a, ck_b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    base = ["--size", "16", "--views", "3", "--num-random-rays", "64", "--layers", "4", "--width", "128", "--num-coarse", "16", "--num-fine", "16",
            "--validate-every", "0", "--quiet", "--precision", "bf16", "--train-occupancy", "8", "--occupancy-bounds", "-4", "-4", "-4", "4", "4", "4",
            "--occupancy-every", "2", "--occupancy-warmup", "1", "--occupancy-level", "0"]
    try:
        first = train_dexnerf.main(base + ["--iters", "6", "--save", ck_a])
        ck = torch.load(ck_a, map_location="cpu")
        grid = ck["train_occupancy"]
        assert grid["updates_done"] == 3 and tuple(grid["cells"]) == (8, 8, 8) and grid["rng_state"].tolist()[2:] == [2, 3]
        assert torch.equal(grid["ema"], first["train_occupancy"].ema.cpu()) and float(grid["ema"].max()) > 0.0
        second = train_dexnerf.main(base + ["--iters", "10", "--load-checkpoint", ck_a, "--save", ck_b])
        grid_b = torch.load(ck_b, map_location="cpu")["train_occupancy"]
        assert grid_b["updates_done"] == 5 and grid_b["rng_state"].tolist()[2:] == [4, 5] and (grid_b["level"], grid_b["warmup_updates"]) == (0.0, 1)
        assert np.isfinite(second["final_loss"]) and second["occupied_fraction"] == second["train_occupancy"].occupied_fraction()
        res = eval_nerf.main(["--checkpoint", ck_b, "--size", "16", "--views", "2", "--num-fine", "16", "--num-coarse", "16", "--precision", "bf16",
                              "--depth-only", "--m-thres", "20", "--ray-span", "checkpoint", "--quiet"])
        assert res["ray_span"].cells == (8, 8, 8) and torch.equal(res["ray_span"].bits.cpu(), grid_b["bits"])
        assert len(res["ray_spans"]) == 2 and len(res["frames"]) == 2
        plain = torch.load(ck_b, map_location="cpu")
        del plain["train_occupancy"]
        torch.save(plain, ck_a)
        with pytest.raises(SystemExit):                                                            # a checkpoint without a grid
            eval_nerf.main(["--checkpoint", ck_a, "--size", "16", "--views", "1", "--depth-only", "--m-thres", "20", "--ray-span", "checkpoint",
                            "--quiet"])
    finally:
        nerf.set_precision("fp32")
