"""Occupancy-grid culling of the full colour render and of the normal render (include/dexnerf_hip_cull.h,
nerf.run_one_iter_of_nerf(occupancy=...), nerf.render_dex_normals(occupancy=...)).

The two kernels are pinned bit for bit to a numpy restatement of the header's text: the emitted points are dn_occupancy_compact_emit's,
the emitted directions are columns 8..10 of the ray rows, the gathered rows are copies of bits with the fills where no row is named.
The culled renders are pinned bit for bit to oracles composed of entry points the library had before (dn_coarse_depths, the numpy
classification of tests/test_occupancy_render.py, run_network_pts / density_gradient on the kept points, the fills, dn_volume_render
/ dn_composite_normals, dn_fine_depths / dn_density_resample).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import D4, lego_weights
from test_occupancy_render import (BOX, FILL, INVAL, M_THRES, NC, NETS, NF, OCC, C, G, NpGrid, _fp32_on_exit, assert_same_maps, dev,  # noqa: F401
                                   hiplib, make_cfg, models_of, random_mask, rays_37, restate_classify, same_bits, sample_set, small_model)

CULL = ("dn_occupancy_compact_emit_dirs", "dn_occupancy_gather_rows")
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 1024 * 1024 + 3]     # the edges of the 1024-element scan block


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def restate_gather_rows(slot, src, n_rows, width, fills, dst):
    """-> (dst after the gather as uint32 (P, dst columns), the number of copied values that are not finite)"""
    slot = np.asarray(slot).reshape(-1)
    out = np.ascontiguousarray(dst, np.float32).view(np.uint32).reshape(slot.size, -1).copy()
    out[:, :width] = np.asarray(fills, np.float32).view(np.uint32)[:width]
    named = (slot >= 0) & (slot < n_rows)
    bad = 0
    if named.any():
        rows = np.ascontiguousarray(src, np.float32).view(np.uint32).reshape(len(src), -1)[slot[named], :width]
        out[named, :width] = rows
        bad = int(((rows & 0x7F800000) == 0x7F800000).sum())
    return out, bad


def test_the_gather_restatement_on_a_hand_checked_case():
    """The yardstick, pinned without a GPU."""
    src = np.array([[1, 2, 3], [np.nan, -0.0, np.inf]], np.float32)
    dst = np.full((4, 3), 9.0, np.float32)
    out, bad = restate_gather_rows([1, -1, 0, 2], src, 2, 2, (-0.0, 5.0), dst)
    nan, nzero = src.view(np.uint32)[1, 0], np.float32(-0.0).view(np.uint32)
    want = np.array([[nan, nzero], [nzero, np.float32(5).view(np.uint32)], src.view(np.uint32)[0, :2], [nzero, np.float32(5).view(np.uint32)]])
    assert np.array_equal(out[:, :2], want) and (out[:, 2].view(np.float32) == 9.0).all() and bad == 1     # the inf sits in column 2: not copied
    assert restate_gather_rows([0, 1], src, 1, 3, (0, 0, 0), dst[:2])[1] == 0                               # row 1 is past n_rows: a fill
    from nerf import _hip
    for width in range(1, _hip.CULL_MAX_WIDTH + 1):                                                         # every width the header allows
        out, bad = restate_gather_rows([-1, 5], np.zeros((1, 4), np.float32), 1, width, (1, 2, 3, 4), np.full((2, 4), 9.0, np.float32))
        assert out.view(np.float32).tolist() == [[1.0, 2.0, 3.0, 4.0][:width] + [9.0] * (4 - width)] * 2 and bad == 0


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_cull_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_cull.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.CULL_EXPORTS) == set(CULL)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS) | set(_hip.MESH_EXPORTS) | set(_hip.OCCUPANCY_EXPORTS))
    assert not older & set(CULL) and len(_hip.EXPORTS) == 76 and tuple(_hip.OCCUPANCY_EXPORTS) == OCC
    assert "dexnerf_hip_cull.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()             # build() checks the new header's symbols too
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in CULL + OCC) and hiplib.dn_abi_version() == 2
    assert f"#define DN_CULL_MAX_WIDTH {_hip.CULL_MAX_WIDTH}\n" in text and _hip.CULL_MAX_WIDTH == 4


def test_cull_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    fake, odd = ctypes.c_void_p(256 * 4096), ctypes.c_void_p(256 * 4096 + 2)
    other = ctypes.c_void_p(512 * 4096)
    sizes = (dict(n=0), dict(n=-5), dict(s=0), dict(s=2049), dict(s=-1), dict(n=1 << 30, s=2), dict(n=(1 << 30) + 1, s=1))
    emit = dict(rays=fake, stride=11, z=fake, n=37, s=59, slot=fake, cap=10, pts=fake, dirs=other, stream=None)
    for kw in sizes + (dict(rays=None), dict(z=None), dict(stride=0), dict(stride=-11), dict(stride=8), dict(stride=10), dict(slot=None),
                       dict(cap=-1), dict(pts=None), dict(dirs=None), dict(rays=odd), dict(z=odd), dict(slot=odd), dict(pts=odd), dict(dirs=odd),
                       dict(dirs=fake)):
        assert hiplib.dn_occupancy_compact_emit_dirs(*{**emit, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_compact_emit_dirs" in hiplib.dn_last_error(), kw
    assert hiplib.dn_occupancy_compact_emit_dirs(*{**emit, "cap": 0, "pts": None, "dirs": None}.values()) == 0      # a capacity of 0 launches nothing
    rows = dict(slot=fake, src=fake, ss=4, rows=5, n=10, width=4, f0=0.0, f1=0.0, f2=0.0, f3=float(FILL), dst=other, ds=4, ws=fake, record=fake,
                stream=None)
    for kw in (dict(slot=None), dict(dst=None), dict(src=None), dict(slot=odd), dict(dst=odd), dict(src=odd), dict(width=0), dict(width=5),
               dict(width=-1), dict(ss=3), dict(ds=3), dict(ss=0), dict(ds=-4), dict(width=2, ss=1), dict(width=3, ds=2), dict(rows=-1), dict(rows=11),
               dict(n=0), dict(n=-3), dict(n=(1 << 30) + 1), dict(ws=None), dict(record=None), dict(ws=ctypes.c_void_p(256 * 4096 + 16)),
               dict(record=odd)):
        assert hiplib.dn_occupancy_gather_rows(*{**rows, **kw}.values()) == INVAL, kw
        assert b"dn_occupancy_gather_rows" in hiplib.dn_last_error(), kw


def _host_setup():
    import nerf
    m = small_model()
    grid = nerf.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool), BOX)
    return m, nerf.get_embedding_function(10), nerf.get_embedding_function(4), grid, torch.zeros(5, 3), torch.ones(5, 3)


def _refusals(render, grid):
    """The table of refusals of a culled render, in the order of render_dex_depth(occupancy=...)'s, on host tensors."""
    import nerf
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
        with pytest.raises(RuntimeError, match="no-grad"):                                         # frozen parameters, rays that require grad
            render(model=small_model().requires_grad_(False), rd=torch.ones(5, 3, requires_grad=True), occupancy=grid)
    finally:
        nerf.set_precision("fp32")


def test_run_one_iter_of_nerf_refuses_a_grid_before_any_launch():
    import nerf
    m, ex, ed, grid, ro, rd = _host_setup()

    def render(ro=ro, rd=rd, model=m, ex=ex, ed=ed, **kw):
        return nerf.run_one_iter_of_nerf(1, 5, 1.0, model, model, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, encode_direction_fn=ed,
                                         m_thres_cand=[5.0], **kw)
    _refusals(render, grid)
    with torch.no_grad():
        for kw in (dict(model=torch.nn.Linear(3, 4)), dict(ex=lambda x: x), dict(ed=None), dict(ex=nerf.get_embedding_function(6))):
            with pytest.raises(RuntimeError, match="fused HIP kernels cover"):                     # networks / embedders the kernels do not cover
                render(occupancy=grid, **kw)


def test_render_dex_normals_refuses_a_grid_before_any_launch():
    import nerf
    m, ex, ed, grid, ro, rd = _host_setup()

    def render(ro=ro, rd=rd, model=m, ex=ex, **kw):
        return nerf.render_dex_normals(1, 5, 1.0, model, model, ro, rd, make_cfg(), mode="train", encode_position_fn=ex, m_thres_cand=[5.0], **kw)
    _refusals(render, grid)


def test_colour_and_normal_occupancy_flags_are_judged_before_the_checkpoint_is_read():
    import eval_nerf
    ck = ["--checkpoint", "none.ckpt"]
    occ = ["--occupancy", "16"]
    for argv in (ck + ["--occupancy-colour"],                                                       # needs --occupancy
                 ck + occ,                                                                          # --occupancy alone stays an error
                 ck + occ + ["--occupancy-colour", "--depth-only", "--m-thres", "20"], ck + occ + ["--occupancy-colour", "--normals"],
                 ck + occ + ["--normals", "--occupancy-check"], ck + occ + ["--normals", "--occupancy-check", "--m-thres", "20"],
                 ck + occ + ["--occupancy-colour", "--precision", "fp16"], ck + occ + ["--normals", "--precision", "fp16"],
                 ck + ["--occupancy", "0", "--occupancy-colour"], ck + ["--occupancy", "8,8", "--normals"],
                 ck + occ + ["--occupancy-colour", "--occupancy-dilate", "9"], ck + ["--normals", "--occupancy-check"],
                 ck + ["--normals", "--occupancy-level", "1"]):
        with pytest.raises(SystemExit):
            eval_nerf.main(argv)
    for argv in (ck + ["--occupancy", "32,16,8", "--occupancy-colour", "--occupancy-check", "--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1",
                       "--occupancy-level", "0.5", "--occupancy-dilate", "2", "--precision", "fp32", "--m-thres", "20"],
                 ck + occ + ["--occupancy-colour", "--occupancy-check"],                            # without thresholds: the rgb difference alone
                 ck + occ + ["--normals", "--m-thres", "20", "--precision", "bf16"]):
        with pytest.raises(FileNotFoundError):                                                     # a complete set of flags reaches the checkpoint
            eval_nerf.main(argv)


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------------------------
def widen(rays8, stride, seed):
    """(N,8) ray rows -> (N,stride) with random columns past the seventh (8..10: the view directions)"""
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(rays8.shape[0], stride)).astype(np.float32)
    rows[:, :8] = rays8
    rows[0, 8:11] = (np.nan, -0.0, np.inf)                                  # copied bit for bit, whatever the bits
    return rows


def check_emit_dirs(dev, rays, z, grid, capacity=None):
    from nerf import _ops
    keep, x, slot = restate_classify(rays, z, grid.bounds, grid.cells, grid.mask)
    n_kept = int(keep.sum())
    r, zz = G(rays, dev), G(z, dev)
    got_slot, record, _ = _ops.occupancy_compact_count(r, zz, grid)
    assert np.array_equal(C(got_slot), slot) and C(record).tolist()[0] == n_kept
    cap = n_kept if capacity is None else capacity
    room = max(n_kept, 1) + 2
    pts, dirs = (torch.full((room, 3), 7.0, dtype=torch.float32, device=dev) for _ in range(2))
    _ops.occupancy_compact_emit_dirs(r, zz, got_slot, cap, pts, dirs)
    plain = torch.full((room, 3), 7.0, dtype=torch.float32, device=dev)
    _ops.occupancy_compact_emit(r, zz, got_slot, cap, plain)
    assert same_bits(C(pts), C(plain))                                      # dn_occupancy_compact_emit's bits, untouched rows included
    pts, dirs, n = C(pts), C(dirs), min(cap, n_kept)
    want_dirs = np.broadcast_to(rays[:, None, 8:11], keep.shape + (3,))[keep]
    assert same_bits(pts[:n], x[keep][:n]) and same_bits(dirs[:n], np.ascontiguousarray(want_dirs[:n]))
    assert (pts[n:] == 7.0).all() and (dirs[n:] == 7.0).all()               # rows past the capacity keep the planted value
    return n_kept


@pytest.mark.gpu
@pytest.mark.parametrize("p", SIZES)
def test_emit_dirs_is_the_restatement(dev, p):
    rays8, z = sample_set(p, p)
    cells, box = (5, 4, 3), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    masks = {"none": np.zeros(cells, bool), "all": np.ones(cells, bool), "random": random_mask(cells, 5, 0.4)}
    for stride in (11, 13):
        rays = widen(rays8, stride, p + stride)
        kept = {name: check_emit_dirs(dev, rays, z, NpGrid(mask, box, dev)) for name, mask in masks.items()}
        assert kept["none"] == 0 and (p < 63 or 0 < kept["random"] < kept["all"] < p)
        if p == 1025:                                                       # a capacity below n_kept, and none
            assert kept["all"] > 10
            check_emit_dirs(dev, rays, z, NpGrid(masks["all"], box, dev), capacity=10)
            check_emit_dirs(dev, rays, z, NpGrid(masks["all"], box, dev), capacity=0)


def slots_of(p, seed, share=0.4):
    keep = np.random.default_rng(seed).random(p) < share
    if p > 2:
        keep[[0, p - 1]] = (True, False)
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32), int(keep.sum())


def source_rows(n, columns, seed):
    """n rows of `columns` floats with planted non-finite values, NaN payloads and negative zeros"""
    src = np.random.default_rng(seed).normal(size=(max(n, 1), columns)).astype(np.float32)
    flat = src.reshape(-1)
    flat[::97] = np.nan
    flat[5::131] = np.inf
    flat[7::173] = -np.inf
    flat[11::59] = -0.0
    flat.view(np.uint32)[13::211] = 0x7FC12345                             # a NaN with a payload
    return src[:n]


def run_gather_rows(dev, slot, src, n_rows, width, fills, dst_np, count=True, src_view=None, dst_view=None):
    """-> (dst after the call as uint32 (P, columns), the record after the call | None).  src_view / dst_view: what to hand the wrapper
    of the device copies of src / dst_np (a column view); the whole dst buffer comes back."""
    from nerf import _hip, _ops
    p = slot.size
    s_dev = G(slot, dev)
    src_dev = G(src, dev) if n_rows else None
    dst_dev = G(dst_np, dev)
    ws = record = None
    if count:
        ws = torch.empty(int(_hip.lib().dn_occupancy_compact_workspace_bytes(p, 1)), dtype=torch.uint8, device=dev)
        record = G(np.array([71, 72, 73, 74], np.int32), dev)
    _ops.occupancy_gather_rows(s_dev, None if src_dev is None else (src_view(src_dev) if src_view else src_dev)[:n_rows],
                               dst_view(dst_dev) if dst_view else dst_dev, width, fills, ws, record)
    return C(dst_dev).view(np.uint32).reshape(p, -1), None if record is None else C(record).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("p", SIZES)
def test_gather_rows_is_the_restatement(dev, p):
    from nerf import _ops
    slot, n_kept = slots_of(p, p)
    fills = (-0.0, float(FILL), 1.5, 0.0)
    for width in (1, 2, 3, 4):
        # dense rows on both sides (width 4: the 16-byte path), with the count
        src = source_rows(n_kept, width, p + width)
        dst = np.full((p, width), 3.0, np.float32)
        want, bad = restate_gather_rows(slot, src, n_kept, width, fills, dst)
        got, record = run_gather_rows(dev, slot, src, n_kept, width, fills[:width], dst)
        assert np.array_equal(got, want) and record == [71, 72, bad, 74], width
        assert p < 1023 or bad > 0
        assert np.array_equal(run_gather_rows(dev, slot, src, n_kept, width, fills[:width], dst, count=False)[0], want), width
        # fewer rows than kept samples: the slots at or past n_rows get the fills and are not counted
        half = n_kept // 2
        want, bad = restate_gather_rows(slot, src, half, width, fills, dst)
        got, record = run_gather_rows(dev, slot, src, half, width, fills[:width], dst)
        assert np.array_equal(got, want) and record == [71, 72, bad, 74], width
        # n_rows = 0 with a NULL source: the fills everywhere, nothing counted
        want, _ = restate_gather_rows(slot, src, 0, width, fills, dst)
        got, record = run_gather_rows(dev, slot, src, 0, width, fills[:width], dst)
        assert np.array_equal(got, want) and record == [71, 72, 0, 74] and (got[:, :width] == np.asarray(fills, np.float32).view(np.uint32)[:width]).all()
    # width 4 off the 16-byte path (source stride 6, destination stride 5) against the 16-byte path: not a bit changes
    src6, dst5 = source_rows(n_kept, 6, p), np.full((p, 5), 3.0, np.float32)
    want, bad = restate_gather_rows(slot, src6, n_kept, 4, fills, dst5)
    got, record = run_gather_rows(dev, slot, src6, n_kept, 4, fills, dst5)
    assert np.array_equal(got, want) and record[2] == bad
    vec, vec_record = run_gather_rows(dev, slot, np.ascontiguousarray(src6[:, :4]), n_kept, 4, fills, np.full((p, 4), 3.0, np.float32))
    assert np.array_equal(vec, got[:, :4]) and vec_record == record and (got[:, 4].view(np.float32) == 3.0).all()
    # destination stride 5 with width 3: the other columns keep the planted value
    src3 = source_rows(n_kept, 3, p + 9)
    want, bad = restate_gather_rows(slot, src3, n_kept, 3, (0.0, 0.0, 0.0), dst5)
    got, record = run_gather_rows(dev, slot, src3, n_kept, 3, (0.0, 0.0, 0.0), dst5)
    assert np.array_equal(got, want) and record[2] == bad and (got[:, 3:].view(np.float32) == 3.0).all()
    # width 1 on a column view (source stride 4, destination stride 4): dn_occupancy_gather bit for bit, record included
    net = source_rows(n_kept, 4, p + 17)
    rf = np.full((p, 4), 3.0, np.float32)
    got, record = run_gather_rows(dev, slot, net, n_kept, 1, (float(FILL),), rf, src_view=lambda t: t[:, 3:], dst_view=lambda t: t[:, 3:])
    want, bad = restate_gather_rows(slot, net[:, 3:], n_kept, 1, (FILL,), rf[:, 3:])
    assert np.array_equal(got[:, 3:], want) and (got[:, :3].view(np.float32) == 3.0).all() and record == [71, 72, bad, 74]
    old, old_record = G(rf, dev), G(np.array([71, 72, 73, 74], np.int32), dev)
    ws = torch.empty(int(_ops.lib().dn_occupancy_compact_workspace_bytes(p, 1)), dtype=torch.uint8, device=dev)
    _ops.occupancy_gather(G(slot, dev), G(net, dev) if n_kept else None, old, ws, old_record)
    assert np.array_equal(C(old).view(np.uint32), got) and C(old_record).tolist() == record


# ---- GPU: the culled colour render ------------------------------------------------------------------------------------------------------
def embedders():
    import nerf
    return nerf.get_embedding_function(10), nerf.get_embedding_function(4)


def colour_cfg(nc, nf, chunksize=4096, use_viewdirs=True, **over):
    cfg = make_cfg(nc, nf, chunksize, **over)
    cfg.nerf.use_viewdirs = use_viewdirs
    return cfg


def oracle_colour_pass(pack, rays, z, mask, bounds):
    """All four columns of one culled pass from the numpy classification and run_network_pts on the kept points, each with its ray's
    direction row -> (rf, n_kept)"""
    from nerf import _ops
    rows = C(rays)
    keep, x, _ = restate_classify(rows, C(z), bounds, mask.shape, mask)
    rf = np.zeros(keep.shape + (4,), np.float32)
    rf[..., 3] = FILL
    if keep.any():
        dirs = None
        if rows.shape[1] >= 11:
            dirs = G(np.ascontiguousarray(np.broadcast_to(rows[:, None, 8:11], keep.shape + (3,))[keep]), rays.device)
        rf[keep] = C(_ops.run_network_pts(pack, G(x[keep], rays.device), dirs, 1))
    return G(rf, rays.device), int(keep.sum())


def oracle_colour(models, ro, rd, nc, nf, mask, bounds, thres, std=0.0, perturb=False, white=False, chunksize=4096, viewdirs=True):
    """The culled colour render composed of entry points the library had before -> (flat maps like run_one_iter_of_nerf's in train mode,
    kept counts per chunk and pass, z[:, 0] of the last pass).  Draws come from train_utils._draws in the render's order."""
    from nerf import _ops, train_utils
    fine = nf > 0
    packs = [m.packed(True, True, precision=_ops._precision) for m in models[:2 if fine else 1]]
    rays_all = _ops.pack_ray_rows(ro, rd, rd if viewdirs else None, 2.0, 6.0)
    thres = list(thres)
    chunks, kept = [], []
    for r0 in range(0, rays_all.shape[0], chunksize):
        rays = rays_all[r0:r0 + chunksize]
        d = train_utils._draws(rays.shape[0], nc, nf, fine, perturb, std, ro.device)
        z = _ops.coarse_depths(rays, nc, False, d.get("t_rand"))
        rf, k_c = oracle_colour_pass(packs[0], rays, z, mask, bounds)
        rgb_c, _, acc_c, weights, depth_c, dex = _ops.volume_render_fwd(rf, z, rays[:, 3:6], d.get("noise_c"), std, white, [] if fine else thres, fine)
        rgb_f = depth_f = acc_f = None
        k_f = 0
        if fine:
            z = _ops.fine_depths(z, weights, nf, d.get("u"))
            rf, k_f = oracle_colour_pass(packs[1], rays, z, mask, bounds)
            rgb_f, _, acc_f, _, depth_f, dex = _ops.volume_render_fwd(rf, z, rays[:, 3:6], d.get("noise_f"), std, white, thres, False)
        chunks.append([rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f] + list(dex) + [z[:, 0]])
        kept.append((k_c, k_f))
    maps = [torch.cat(col) if col[0] is not None else None for col in zip(*chunks)]
    return maps[:-1], kept, maps[-1]


def culled_colour(models, ro, rd, nc, nf, grid, thres, std=0.0, perturb=False, white=False, chunksize=4096, viewdirs=True, **kw):
    import nerf
    ex, ed = embedders()
    with torch.no_grad():
        return nerf.run_one_iter_of_nerf(1, ro.shape[0], 1.0, models[0], models[1] if nf else None, ro, rd,
                                         colour_cfg(nc, nf, chunksize, viewdirs, radiance_field_noise_std=std, perturb=perturb, white_background=white),
                                         mode="train", encode_position_fn=ex, encode_direction_fn=ed if viewdirs else None,
                                         m_thres_cand=list(thres), occupancy=grid, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("nf", [NF, 0])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_culled_colour_render_is_the_oracle_bit_for_bit(dev, name, precision, nf, white):
    import nerf
    nerf.set_precision(precision)
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    want, kept, _ = oracle_colour(models, ro, rd, NC, nf, mask, BOX, M_THRES, white=white)
    *got, stats = culled_colour(models, ro, rd, NC, nf, grid, M_THRES, white=white, cull_stats=True)
    assert len(got) == 6 + len(M_THRES)
    assert_same_maps(got, want)
    assert stats["kept"] == kept[0] and stats["total"] == (37 * NC, 37 * (NC + nf) if nf else 0) and stats["nonfinite"] == 0
    assert 0 < kept[0][0] < 37 * NC and (nf == 0 or 0 < kept[0][1] < 37 * (NC + nf))             # the grid culls some and keeps some
    assert len(culled_colour(models, ro, rd, NC, nf, grid, M_THRES, white=white)) == len(got)      # without cull_stats: the maps alone


@pytest.mark.gpu
@pytest.mark.parametrize("white", [False, True])
def test_an_empty_grid_launches_no_colour_network(dev, monkeypatch, white):
    import nerf
    from nerf import _ops
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    mask = np.zeros((4, 4, 4), bool)
    want, kept, z0 = oracle_colour(models, ro, rd, NC, NF, mask, BOX, M_THRES, white=white)

    def no_launch(*a, **k):
        raise AssertionError("the network ran although no sample was kept")
    monkeypatch.setattr(_ops, "run_network_pts", no_launch)
    *got, stats = culled_colour(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, white=white, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == (0, 0) and kept == [(0, 0)]
    for rgb in (got[0], got[3]):
        assert (C(rgb) == (1.0 if white else 0.0)).all()
    for m in (got[1], got[2], got[4], got[5]):
        assert not C(m).any()                                               # depth = 0, acc = 0 in both passes
    for m in got[6:]:
        assert same_bits(C(m), C(z0))                                       # no crossing: the Dex depth falls back to z[0]


@pytest.mark.gpu
def test_colour_chunks_that_keep_nothing_and_chunks_that_keep_some(dev):
    import nerf
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    ro = ro.clone()
    ro[:16, 0] += 100.0                                                     # the first chunk of 16 rays never meets the box
    mask = random_mask((8, 7, 6), 11)
    want, kept, _ = oracle_colour(models, ro, rd, NC, NF, mask, BOX, M_THRES, chunksize=16)
    assert len(kept) == 3 and kept[0] == (0, 0) and kept[1][0] > 0 and kept[1][1] > 0
    *got, stats = culled_colour(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, chunksize=16, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == tuple(sum(k[p] for k in kept) for p in range(2))


@pytest.mark.gpu
def test_colour_perturb_and_noise_leave_the_generator_where_the_plain_render_does(dev):
    import nerf
    models = models_of("lego", dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    grid = nerf.OccupancyGrid.from_mask(G(mask, dev), BOX)
    torch.manual_seed(7)
    want, _, _ = oracle_colour(models, ro, rd, NC, NF, mask, BOX, M_THRES, std=1.0, perturb=True)
    torch.manual_seed(7)
    got = culled_colour(models, ro, rd, NC, NF, grid, M_THRES, std=1.0, perturb=True)
    state = torch.cuda.get_rng_state(dev)
    assert_same_maps(got, want)
    torch.manual_seed(7)
    culled_colour(models, ro, rd, NC, NF, None, M_THRES, std=1.0, perturb=True)                     # the plain run_one_iter_of_nerf
    assert torch.equal(state, torch.cuda.get_rng_state(dev))


@pytest.mark.gpu
def test_a_network_without_view_directions(dev):
    """8-column ray rows: the plain emit, no direction rows."""
    import nerf
    from nerf import synthetic as syn
    kw = dict(D4, use_viewdirs=False)
    models = []
    for seed in (31, 32):
        m = nerf.models.FlexibleNeRFModel(**kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, **kw).items()})
        models.append(m.to(dev))
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    want, kept, _ = oracle_colour(models, ro, rd, NC, NF, mask, BOX, M_THRES, viewdirs=False)
    *got, stats = culled_colour(models, ro, rd, NC, NF, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, viewdirs=False, cull_stats=True)
    assert_same_maps(got, want)
    assert stats["kept"] == kept[0] and 0 < kept[0][0] < 37 * NC and 0 < kept[0][1] < 37 * (NC + NF)


WIDE = (-12.0, -12.0, -12.0, 12.0, 12.0, 12.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NETS))
def test_a_full_grid_renders_the_plain_colour_render(dev, name):
    """All cells set and bounds that enclose every sample: the culled render differs from the plain run_one_iter_of_nerf only in how the
    network kernel gets its inputs - explicit points with a direction row each against ray rows + depths.  Measured on the parent
    commit on this test's points (37 rays, 37 + 22 samples, both networks of both shapes, fp32 and bf16): the largest difference
    between run_network_rays and run_network_pts over all four columns is 0 (profiles/occupancy_colour_render.md) - the first assertion
    here repeats that measurement - so every map must be bit-equal."""
    import nerf
    from nerf import _ops
    nerf.set_render_policy("bf16")                                         # (the configured precision: no fp16 instance either way)
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    ex, ed = embedders()
    rays = _ops.pack_ray_rows(ro, rd, rd, 2.0, 6.0)
    z = _ops.coarse_depths(rays, NC + NF, False)
    for precision in ("fp32", "bf16"):
        nerf.set_precision(precision)
        with torch.no_grad():
            for m in models:
                pack = m.packed(True, True, precision=_ops._precision)
                pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
                dirs = rays[:, None, 8:11].expand(-1, z.shape[1], -1).reshape(-1, 3)
                assert same_bits(C(_ops.run_network_rays(pack, rays, z)).reshape(-1, 4), C(_ops.run_network_pts(pack, pts, dirs, 1)))
        grid = nerf.OccupancyGrid.from_mask(torch.ones(3, 5, 4, dtype=torch.bool, device=dev), WIDE)
        for nf in (NF, 0):
            *got, stats = culled_colour(models, ro, rd, NC, nf, grid, M_THRES, cull_stats=True)
            assert stats["kept"] == stats["total"]                          # the box encloses every sample
            assert_same_maps(got, culled_colour(models, ro, rd, NC, nf, None, M_THRES))


# ---- GPU: the culled normal render ------------------------------------------------------------------------------------------------------
def oracle_normals(models, ro, rd, nc, nf, mask, bounds, thres):
    """The culled normal render composed of entry points the library had before -> (depth, acc, normal, dex..., dex normals..., kept)"""
    from nerf import _ops
    from test_occupancy_render import oracle_pass
    fine = nf > 0
    prec = _ops._precision
    packs = [m.packed_density(True, True, precision=prec) for m in models[:2 if fine else 1]]
    streams = models[1 if fine else 0].packed_density_grad(True, True, precision=prec)
    rays = _ops.pack_ray_rows(ro, rd, None, 2.0, 6.0)
    th = torch.tensor(list(thres), dtype=torch.float32, device=ro.device)
    z = _ops.coarse_depths(rays, nc, False, None)
    k_c = 0
    if fine:
        rf, k_c = oracle_pass(packs[0], rays, z, mask, bounds)
        _, _, z = _ops.density_resample(rf, z, rays[:, 3:6], nf, None, 0.0, None)
    keep, x, _ = restate_classify(C(rays), C(z), bounds, mask.shape, mask)
    rf = np.zeros(keep.shape + (4,), np.float32)
    rf[..., 3] = FILL
    g = np.zeros(keep.shape + (3,), np.float32)
    if keep.any():
        sigma, grad = _ops.density_gradient(packs[-1], streams, pts=G(x[keep], ro.device))
        rf[keep, 3], g[keep] = C(sigma), C(grad)
    depth, acc, dex, normal, dex_normal = _ops.composite_normals(G(rf, ro.device), z, rays[:, 3:6], G(g, ro.device), None, 0.0, th)
    return [depth, acc, normal] + list(dex) + list(dex_normal), ((k_c, int(keep.sum())) if fine else (int(keep.sum()), 0))


def normals_render(models, ro, rd, nc, nf, grid, thres, **kw):
    import nerf
    with torch.no_grad():
        return nerf.render_dex_normals(1, ro.shape[0], 1.0, models[0], models[1] if nf else None, ro, rd, make_cfg(nc, nf), mode="train",
                                       encode_position_fn=nerf.get_embedding_function(10), m_thres_cand=list(thres), occupancy=grid, **kw)


def normal_maps(out):
    return [out.depth, out.acc, out.normal] + list(out.dex_depth) + list(out.dex_normal)


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [NF, 0])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_culled_normal_render_is_the_oracle_bit_for_bit(dev, name, precision, nf):
    import nerf
    nerf.set_precision(precision)
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    mask = random_mask((8, 7, 6), 11)
    want, kept = oracle_normals(models, ro, rd, NC, nf, mask, BOX, M_THRES)
    out, stats = normals_render(models, ro, rd, NC, nf, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, cull_stats=True)
    assert_same_maps(normal_maps(out), want)
    assert stats["kept"] == kept and stats["nonfinite"] == 0 and 0 < sum(kept) < sum(stats["total"])
    assert C(out.normal).any() and not C(out.normal)[C(out.acc) == 0].any()                        # some normals; none where nothing was hit
    alone = normals_render(models, ro, rd, NC, nf, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES)
    assert_same_maps(normal_maps(alone), want)                                                     # without cull_stats: the DexNormals alone
    slabs = normals_render(models, ro, rd, NC, nf, nerf.OccupancyGrid.from_mask(G(mask, dev), BOX), M_THRES, max_workspace_bytes=1 << 20)
    assert_same_maps(normal_maps(slabs), want)                                                     # the kept points in slabs: the same maps


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NETS))
def test_a_full_grid_renders_the_plain_normal_render(dev, name):
    """All cells set and bounds that enclose every sample, against render_dex_normals without a grid.  Measured on the parent commit on
    this test's points (37 rays, 37 + 22 samples, the last pass's network of both shapes, fp32 and bf16): the largest difference between
    density_gradient(rays=, z=) and density_gradient(pts=) is 0 in sigma and in the gradient (profiles/occupancy_colour_render.md) - the
    first assertion here repeats that measurement - so every map must be bit-equal."""
    import nerf
    from nerf import _ops
    models = models_of(name, dev)
    ro, rd = rays_37(dev)
    rays = _ops.pack_ray_rows(ro, rd, None, 2.0, 6.0)
    z = _ops.coarse_depths(rays, NC + NF, False)
    grid = nerf.OccupancyGrid.from_mask(torch.ones(3, 5, 4, dtype=torch.bool, device=dev), WIDE)
    for precision in ("fp32", "bf16"):
        nerf.set_precision(precision)
        with torch.no_grad():
            m = models[1]
            pack, streams = m.packed_density(True, True, precision=_ops._precision), m.packed_density_grad(True, True, precision=_ops._precision)
            pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
            s_r, g_r = _ops.density_gradient(pack, streams, rays=rays, z=z)
            s_r, g_r = C(s_r).reshape(-1), C(g_r).reshape(-1, 3)
            s_p, g_p = _ops.density_gradient(pack, streams, pts=pts)
            assert same_bits(s_r, C(s_p)) and same_bits(g_r, C(g_p))
        for nf in (NF, 0):
            out, stats = normals_render(models, ro, rd, NC, nf, grid, M_THRES, cull_stats=True)
            assert stats["kept"] == stats["total"]
            assert_same_maps(normal_maps(out), normal_maps(normals_render(models, ro, rd, NC, nf, None, M_THRES)))


# ---- GPU: the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eval_driver_culls_the_colour_and_the_normal_render(dev, tmp_path, capsys):
    """eval_nerf.py --occupancy ... --occupancy-colour: the default bounds hold every sample, so a grid set everywhere (level below every
    density) renders the plain frames bit for bit and --occupancy-check reports it; a real grid culls something; --normals --occupancy
    runs and culls something."""
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    common = ["--checkpoint", str(ck), "--size", "24", "--views", "2", "--num-fine", "64", "--precision", "fp32", "--m-thres", "20"]
    plain = eval_nerf.main(common + ["--quiet"])
    res = eval_nerf.main(common + ["--occupancy", "12,10,8", "--occupancy-level=-1e30", "--occupancy-dilate", "0", "--occupancy-colour", "--occupancy-check"])
    assert res["occupancy"].cells == (12, 10, 8) and res["occupancy"].occupied_fraction() == 1.0
    assert res["cull"]["kept"] == res["cull"]["total"] == [2 * 24 * 24 * 64, 2 * 24 * 24 * 128] and res["cull"]["nonfinite"] == 0
    assert res["occupancy_check"]["equal"] == [1.0] * 4 and res["occupancy_check"]["max_diff"] == [0.0] * 4
    assert res["occupancy_check"]["max_rgb_diff"] == 0.0
    for (rgb, depth), (rgb_plain, depth_plain) in zip(res["frames"], plain["frames"]):
        assert_same_maps([rgb, depth], [rgb_plain, depth_plain])
    text = capsys.readouterr().out
    assert "occupancy grid 12x10x8" in text and "occupancy check m_thres  20: 100.000 % of the pixels equal" in text
    assert "occupancy check rgb: max |rgb difference| 0.000e+00" in text
    # a real grid of the two networks culls something and still reports
    res = eval_nerf.main(common + ["--quiet", "--occupancy", "16", "--occupancy-level", "5", "--occupancy-colour", "--occupancy-check"])
    assert 0 < sum(res["cull"]["kept"]) < sum(res["cull"]["total"]) and len(res["occupancy_check"]["equal"]) == 4
    assert res["occupancy_check"]["max_rgb_diff"] >= 0.0
    res = eval_nerf.main(common + ["--quiet", "--normals", "--occupancy", "16"])
    assert 0 < sum(res["cull"]["kept"]) < sum(res["cull"]["total"]) and len(res["frames"]) == 2
    assert res["frames"][0][2].normal.shape == (24, 24, 3)
