"""The Dex threshold surface as a triangle mesh (include/dexnerf_hip_mesh.h): dn_isosurface_workspace_bytes / _count / _emit,
_ops.isosurface, nerf.density_grid, nerf.extract_dex_mesh, nerf.save_ply, eval_nerf.py --mesh.

`restate` below is a float64 numpy restatement of the header's definition: inside = finite and f > level in fp32, the six Kuhn
tetrahedra per cell, vertices on the owned edges numbered by (owner, slot) and placed at a + (b - a) * t in float64 rounded once,
triangles by the header's rule in (cell, tetrahedron, triangle) order.  Its orientation is found GEOMETRICALLY (on the unit cube, the
vertices at the edge midpoints: the triangle's normal against the direction from the inside corners to the outside ones), not
taken from the kernel's table.  The definition fixes arithmetic and order, so every comparison of the kernels with the restatement
is exact: indices equal, coordinates bit for bit.  The restatement itself is pinned on analytic fields without a GPU: closed and
consistently oriented (every directed edge once, its reverse once), Euler characteristic, and a signed volume inside a bound
derived from the geometry (every point of the mesh lies in a tetrahedron the true surface crosses, so within the tetrahedron's
diameter h * sqrt(3) of the true surface)."""
import collections
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import REPO
from golden_cases import D4, lego_weights

MESH = ("dn_isosurface_workspace_bytes", "dn_isosurface_count", "dn_isosurface_emit")
INVAL = -1000
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def offset_of(code):
    return (code >> 2) & 1, (code >> 1) & 1, code & 1


def tet_codes(p):
    """corner codes 4dx + 2dy + dz of tetrahedron p: c0 = 0, c1 = c0 + e_p1, c2 = c1 + e_p2, c3 = (1,1,1)"""
    c1 = 4 >> PERMS[p][0]
    return (0, c1, c1 | (4 >> PERMS[p][1]), 7)


def _tet_case(p, m):
    """The triangles of tetrahedron p with inside bits m: a list of 3 edges each, an edge = (owner corner code, slot)."""
    codes = tet_codes(p)
    ins = [c for c in range(4) if (m >> c) & 1]
    outs = [c for c in range(4) if not (m >> c) & 1]
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in outs]]
    elif len(ins) == 3:
        tris = [[(a, outs[0]) for a in ins]]
    elif len(ins) == 2:
        (a, b), (o, q) = ins, outs
        quad = [(a, o), (a, q), (b, q), (b, o)]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    else:
        return []
    corner = [np.array(offset_of(c), np.float64) for c in codes]
    toward = np.mean([corner[c] for c in outs], axis=0) - np.mean([corner[c] for c in ins], axis=0)
    out = []
    for tri in tris:
        pos = [(corner[a] + corner[b]) / 2 for a, b in tri]
        dot = float(np.dot(np.cross(pos[1] - pos[0], pos[2] - pos[0]), toward))
        assert abs(dot) > 1e-9
        if dot < 0:
            tri = [tri[0], tri[2], tri[1]]
        out.append([(codes[min(a, b)], codes[max(a, b)] - codes[min(a, b)] - 1) for a, b in tri])
    return out


TET_CASES = [[_tet_case(p, m) for m in range(16)] for p in range(6)]


def restate(f, xs, ys, zs, level):
    """-> (vertices (V,3) float32, triangles (T,3) int64, n_nonfinite)"""
    f = np.asarray(f, np.float32)
    nx, ny, nz = f.shape
    level = np.float32(level)
    fin = np.isfinite(f)
    with np.errstate(invalid="ignore"):
        ins = fin & (f > level)
    has = np.zeros((nx, ny, nz, 7), bool)
    for s in range(7):
        dx, dy, dz = offset_of(s + 1)
        a = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        b = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        has[a + (s,)] = fin[a] & fin[b] & (ins[a] != ins[b])
    vid = (np.cumsum(has.reshape(-1), dtype=np.int64) - 1).reshape(has.shape)
    oi, oj, ok, slot = np.nonzero(has)                      # C order: ascending by (owner linear index, slot)
    far = np.array([offset_of(c) for c in range(8)])[slot + 1]
    fa = f[oi, oj, ok].astype(np.float64)
    fb = f[oi + far[:, 0], oj + far[:, 1], ok + far[:, 2]].astype(np.float64)
    t = (np.float64(level) - fa) / (fb - fa)
    cols = []
    for axis, (c, o) in enumerate(((xs, oi), (ys, oj), (zs, ok))):
        c64 = np.asarray(c, np.float32).astype(np.float64)
        a, b = c64[o], c64[o + far[:, axis]]
        cols.append(a + (b - a) * t)
    vertices = np.stack(cols, -1).astype(np.float32) if len(t) else np.zeros((0, 3), np.float32)

    ci, cj, ck = (g.reshape(-1) for g in np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"))
    corner = [offset_of(c) for c in range(8)]
    cin = [ins[ci + d[0], cj + d[1], ck + d[2]] for d in corner]
    cfin = [fin[ci + d[0], cj + d[1], ck + d[2]] for d in corner]
    keys, rows = [], []
    for p in range(6):
        codes = tet_codes(p)
        allfin = cfin[codes[0]] & cfin[codes[1]] & cfin[codes[2]] & cfin[codes[3]]
        m = sum(cin[codes[n]].astype(np.int64) << n for n in range(4)) * allfin
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if not sel.size:
                continue
            for tnum, tri in enumerate(TET_CASES[p][case]):
                idx = []
                for code, s in tri:
                    d = corner[code]
                    assert has[ci[sel] + d[0], cj[sel] + d[1], ck[sel] + d[2], s].all()
                    idx.append(vid[ci[sel] + d[0], cj[sel] + d[1], ck[sel] + d[2], s])
                keys.append(np.stack([sel, np.full_like(sel, p), np.full_like(sel, tnum)], -1))
                rows.append(np.stack(idx, -1))
    if not rows:
        return vertices, np.zeros((0, 3), np.int64), int((~fin).sum())
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return vertices, rows[order], int((~fin).sum())


# ---- mesh properties, as integer work ---------------------------------------------------------------------------------------------------
def directed_edges(tri):
    tri = np.asarray(tri, np.int64)
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])


def open_edges(tri, n_vertices):
    """The directed edges whose reverse is missing (an empty array: the surface is closed and consistently oriented); asserts that
    no directed edge occurs twice."""
    e = directed_edges(tri)
    key, rev = e[:, 0] * n_vertices + e[:, 1], e[:, 1] * n_vertices + e[:, 0]
    assert len(np.unique(key)) == len(key), "a directed edge occurs twice"
    return e[~np.isin(key, rev)]


def euler_characteristic(tri):
    e = directed_edges(tri)
    assert len(e) % 2 == 0
    return len(np.unique(tri)) - len(e) // 2 + len(tri)


def signed_volume(v, tri):
    p = np.asarray(v, np.float64)[np.asarray(tri, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def axes(n, lo=-1.0, hi=1.0):
    a = np.linspace(lo, hi, n).astype(np.float32)
    return a, a.copy(), a.copy()


def on_grid(fn, xs, ys, zs):
    x, y, z = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64), zs.astype(np.float64), indexing="ij")
    return fn(x, y, z).astype(np.float32)


def sphere(r):
    return lambda x, y, z: r - np.sqrt(x * x + y * y + z * z)


def torus(big, small):
    return lambda x, y, z: small - np.sqrt((np.sqrt(x * x + y * y) - big) ** 2 + z * z)


def noise_field(shape, seed):
    """random magnitudes of both signs with an outside border: every surface closes inside the grid"""
    f = np.random.default_rng(seed).normal(size=shape).astype(np.float32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


@pytest.fixture(scope="module")
def hiplib():
    from nerf import _hip
    if not _hip.available():
        import __graft_entry__ as ge
        ge.build()
    return _hip.lib()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_mesh_header_declares_exactly_its_table_and_the_library_exports_it(hiplib):
    from nerf import _hip
    text = open(os.path.join(REPO, "include", "dexnerf_hip_mesh.h")).read()
    assert set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", text)) == set(_hip.MESH_EXPORTS) == set(MESH)
    older = (set(_hip.EXPORTS) | set(_hip.EXT_EXPORTS) | set(_hip.ANNEAL_EXPORTS) | set(_hip.EXPOSURE_EXPORTS) | set(_hip.NORMALS_EXPORTS)
             | set(_hip.QUANTILE_EXPORTS))
    assert not older & set(MESH)
    assert "dexnerf_hip_mesh.h" in open(os.path.join(REPO, "__graft_entry__.py")).read()      # build() checks the new header's symbols too
    assert "isosurface.hip" in open(os.path.join(REPO, "dex-nerf_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert all(hasattr(raw, name) for name in MESH) and hiplib.dn_abi_version() == 2
    assert f"#define DN_ISO_SCAN_BLOCK {_hip.ISO_SCAN_BLOCK}\n" in text and f"#define DN_ISO_MAX_GRID_VERTICES {_hip.ISO_MAX_GRID_VERTICES}\n" in text
    assert _hip.ISO_MAX_GRID_VERTICES >= 512 ** 3 and hiplib.dn_isosurface_workspace_bytes(512, 512, 512) > 0      # the maximum admits 512^3


def test_mesh_entry_points_judge_their_arguments_before_gpu_work(hiplib):
    """Every refusal comes back before a launch: the device pointers here are small integers nothing may dereference."""
    fake = ctypes.c_void_p(256 * 4096)
    count = dict(field=fake, stride=1, xs=fake, ys=fake, zs=fake, nx=4, ny=5, nz=6, level=0.5, ws=fake, counts=fake, stream=None)
    emit = dict(field=fake, stride=4, xs=fake, ys=fake, zs=fake, nx=4, ny=5, nz=6, level=0.5, ws=fake, max_v=10, max_t=10, v=fake, t=fake,
                stream=None)
    grids = (dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-3),
             dict(nx=2, ny=2, nz=(1 << 26) + 1), dict(nx=1 << 16, ny=1 << 16, nz=2), dict(nx=1 << 20, ny=1 << 20, nz=1 << 20),   # past the maximum
             dict(nx=600, ny=600, nz=600))                                                                                    # 12 * cells >= 2^31
    common = (dict(field=None), dict(xs=None), dict(ys=None), dict(zs=None), dict(ws=None), dict(stride=0), dict(stride=-4),
              dict(ws=ctypes.c_void_p(256 * 4096 + 16))) + grids
    for kw in common + (dict(counts=None), dict(counts=ctypes.c_void_p(256 * 4096 + 2))):
        assert hiplib.dn_isosurface_count(*{**count, **kw}.values()) == INVAL, kw
        assert b"dn_isosurface_count" in hiplib.dn_last_error(), kw
    for kw in common + (dict(max_v=-1), dict(max_t=-1), dict(v=None), dict(t=None)):
        assert hiplib.dn_isosurface_emit(*{**emit, **kw}.values()) == INVAL, kw
        assert b"dn_isosurface_emit" in hiplib.dn_last_error(), kw
    for kw in grids:
        g = {**count, **kw}
        assert hiplib.dn_isosurface_workspace_bytes(g["nx"], g["ny"], g["nz"]) == 0, kw
    # the workspace holds the class words and the two prefixes of every grid vertex
    assert hiplib.dn_isosurface_workspace_bytes(4, 5, 6) >= 120 * 10 and hiplib.dn_isosurface_workspace_bytes(4, 5, 6) % 256 == 0
    assert hiplib.dn_isosurface_workspace_bytes(2, 2, 1 << 26) > 0


FIELDS = {
    "sphere": lambda: (on_grid(sphere(0.7), *axes(17)),) + axes(17),
    "torus": lambda: (on_grid(torus(0.6, 0.25), *axes(17)),) + axes(17),
    "noise": lambda: (noise_field((9, 8, 11), 3),) + (np.arange(9, dtype=np.float32), np.arange(8, dtype=np.float32) * 0.5,
                                                       np.cumsum(np.random.default_rng(4).uniform(0.2, 2.0, 11)).astype(np.float32)),
}


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_the_restatement_on_analytic_fields(name):
    """The yardstick, pinned without a GPU.  Volume bound: every point of the mesh lies in a tetrahedron that the true surface
    crosses, whose diameter is h * sqrt(3) - so the mesh lies in the shell of that half-width around the true surface, and its volume
    between the volumes of the surfaces offset by it (sphere: radius r -+ d; torus: tube radius r -+ d, which needs r + d < R)."""
    f, xs, ys, zs = FIELDS[name]()
    v, t, bad = restate(f, xs, ys, zs, 0.0)
    assert bad == 0 and len(v) and len(t) and t.min() == 0 and t.max() == len(v) - 1 and len(np.unique(t)) == len(v)
    assert len(open_edges(t, len(v))) == 0
    vol = signed_volume(v, t)
    assert vol > 0
    d = (2.0 / 16) * np.sqrt(3.0)
    if name == "sphere":
        assert euler_characteristic(t) == 2
        assert 4 / 3 * np.pi * (0.7 - d) ** 3 <= vol <= 4 / 3 * np.pi * (0.7 + d) ** 3
    if name == "torus":
        assert euler_characteristic(t) == 0
        assert 0.25 + d < 0.6 and 2 * np.pi ** 2 * 0.6 * (0.25 - d) ** 2 <= vol <= 2 * np.pi ** 2 * 0.6 * (0.25 + d) ** 2


def test_the_restatement_handles_nonfinite_samples_and_empty_surfaces():
    f, xs, ys, zs = FIELDS["noise"]()
    f[3, 3, 3], f[4, 4, 5], f[5, 2, 7] = np.nan, np.inf, -np.inf
    v, t, bad = restate(f, xs, ys, zs, 0.0)
    assert bad == 3 and np.isfinite(v).all() and len(open_edges(t, len(v))) > 0        # the holes around the three samples
    clean = restate(np.where(np.isfinite(f), f, -1.0), xs, ys, zs, 0.0)
    assert len(t) < len(clean[1])
    for level in (1e9, -1e9):
        v, t, _ = restate(f, xs, ys, zs, level)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def small_model(dev=None, **over):
    import nerf
    sd = lego_weights()[1]
    m = nerf.models.FlexibleNeRFModel(**{**D4, **over})
    if not over:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m if dev is None else m.to(dev)


def test_python_guards_raise_before_any_launch():
    import nerf
    from nerf import _ops
    ex = nerf.get_embedding_function(10)
    xs = torch.linspace(0, 1, 4)
    f = torch.zeros(4, 4, 4)
    for bad in (torch.tensor([0.0, 0.5, 0.5, 1.0]), torch.tensor([0.0, 2.0, 1.0, 3.0]), torch.tensor([0.0, 1.0, float("nan"), 3.0]),
                torch.tensor([0.0]), torch.linspace(0, 1, 4, dtype=torch.float64)):
        for where in range(3):
            coords = [xs, xs, xs]
            coords[where] = bad
            with pytest.raises(ValueError):
                _ops.isosurface(f if bad.numel() == 4 else torch.zeros([c.numel() for c in coords]), *coords, 0.0)
    for level in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="level"):
            _ops.isosurface(f, xs, xs, xs, level)
    with pytest.raises(ValueError):
        _ops.isosurface(torch.zeros(4, 4, 5), xs, xs, xs, 0.0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        _ops.isosurface(f, xs, xs, xs, 0.0)                                       # host tensors: refused, never computed on the CPU
    m = small_model()
    box = (-1, -1, -1, 1, 1, 1)
    try:
        nerf.set_precision("fp32")
        with pytest.raises(RuntimeError, match="no-grad"):
            nerf.density_grid(m, ex, box, 4)                                      # parameters require grad, autograd enabled
        with pytest.raises(RuntimeError, match="no-grad"):
            nerf.extract_dex_mesh(m, ex, box, 4, 1.0)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="ROCm device"):
                nerf.density_grid(m, ex, box, 4)
            with pytest.raises(RuntimeError, match="ROCm device"):
                nerf.extract_dex_mesh(m, ex, box, 4, 1.0)
            with pytest.raises(ValueError):
                nerf.extract_dex_mesh(m, ex, box, 4, float("nan"))
            nerf.set_precision("fp16")
            with pytest.raises(RuntimeError, match="fp16"):
                nerf.density_grid(m, ex, box, 4)
            with pytest.raises(RuntimeError, match="fp16"):
                nerf.extract_dex_mesh(m, ex, box, 4, 1.0)
    finally:
        nerf.set_precision("fp32")


def read_ply(path):
    """-> (property names, vertex rows (V, n) float32, faces (T,3) int32), parsing the header"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    n_f = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    props = [ln.split()[-1] for ln in lines if ln.startswith("property float")]
    assert "property list uchar int vertex_indices" in lines
    assert len(body) == n_v * 4 * len(props) + n_f * 13
    rows = np.frombuffer(body, "<f4", n_v * len(props)).reshape(n_v, len(props))
    faces = np.zeros((n_f, 3), np.int32)
    for i in range(n_f):
        n, a, b, c = struct.unpack_from("<Biii", body, n_v * 4 * len(props) + 13 * i)
        assert n == 3
        faces[i] = (a, b, c)
    return props, rows, faces


def test_save_ply_round_trip(tmp_path):
    import nerf
    f, xs, ys, zs = FIELDS["sphere"]()
    v, t, _ = restate(f, xs, ys, zs, 0.0)
    normals = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    nerf.save_ply(tmp_path / "a.ply", nerf.DexMesh(torch.from_numpy(v), torch.from_numpy(t.astype(np.int32)), torch.from_numpy(normals), 0))
    props, rows, faces = read_ply(tmp_path / "a.ply")
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(rows[:, :3], v) and np.array_equal(rows[:, 3:], normals) and np.array_equal(faces, t)
    nerf.save_ply(tmp_path / "b.ply", nerf.DexMesh(v, t, None, 0))
    props, rows, faces = read_ply(tmp_path / "b.ply")
    assert props == ["x", "y", "z"] and np.array_equal(rows, v) and np.array_equal(faces, t)
    nerf.save_ply(tmp_path / "c.ply", nerf.DexMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, 0))     # an empty surface
    assert read_ply(tmp_path / "c.ply")[1].shape == (0, 3)


def test_mesh_flags_are_judged_before_the_checkpoint_is_read():
    import eval_nerf
    box = ["--mesh-bounds=-1,-1,-1,1,1,1"]
    for argv in (["--mesh", "a.ply", "--mesh-thres", "5"], ["--mesh", "a.ply"] + box,                       # bounds / threshold missing
                 ["--mesh", "a.ply", "--mesh-thres", "5", "--precision", "fp16"] + box,
                 ["--mesh", "a.ply", "--mesh-thres", "5", "--mesh-resolution", "1"] + box,
                 ["--mesh", "a.ply", "--mesh-thres", "5", "--mesh-resolution", "8,8"] + box,
                 ["--mesh", "a.ply", "--mesh-thres", "nan"] + box, ["--mesh", "a.ply", "--mesh-thres", "5", "--mesh-bounds=0,0,0,1,0,1"],
                 ["--mesh", "a.ply", "--mesh-thres", "5", "--normals"] + box, ["--mesh-thres", "5"], box):
        with pytest.raises(SystemExit):
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
    yield
    nerf.set_precision("fp32")


def G(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(t):
    return t.detach().cpu().numpy()


def extract(f, xs, ys, zs, level, dev):
    from nerf import _ops
    v, t, bad = _ops.isosurface(G(f, dev), G(xs, dev), G(ys, dev), G(zs, dev), level)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    return C(v), C(t), bad


def same_mesh(got, want):
    (v, t, bad), (rv, rt, rbad) = got, want
    assert v.shape == rv.shape and t.shape == rt.shape and bad == rbad
    assert np.array_equal(t, rt)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))          # bit for bit
    return True


def coords(n, seed):
    return np.cumsum(np.random.default_rng(seed).uniform(0.25, 1.75, n)).astype(np.float32)


@pytest.mark.gpu
def test_one_cell_all_256_patterns(dev):
    """Every tetrahedron case and the winding table: the 256 inside / outside patterns of one cell, random magnitudes."""
    rng = np.random.default_rng(0)
    xs, ys, zs = coords(2, 1), coords(2, 2), coords(2, 3)
    for pattern in range(256):
        sign = np.array([1.0 if (pattern >> c) & 1 else -1.0 for c in range(8)]).reshape(2, 2, 2)
        f = (sign * rng.uniform(0.1, 3.0, (2, 2, 2))).astype(np.float32) + np.float32(0.5)
        assert same_mesh(extract(f, xs, ys, zs, 0.5, dev), restate(f, xs, ys, zs, 0.5)), pattern


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 4, 3), (3, 3, 2), (3, 3, 3), (3, 3, 64), (3, 3, 65), (3, 3, 66), (3, 3, 129)])
def test_order_and_wave_edges(dev, shape):
    """(5,4,3) catches any mix-up of axes or order; nz around 64 and 128 puts the wave's 64-sample edge at, before and after the column end."""
    f = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32)
    xs, ys, zs = coords(shape[0], 1), coords(shape[1], 2), coords(shape[2], 3)
    want = restate(f, xs, ys, zs, 0.1)
    assert len(want[1]) > 0
    assert same_mesh(extract(f, xs, ys, zs, 0.1, dev), want)


@pytest.mark.gpu
def test_every_scan_level_on_a_random_field(dev):
    """The scan has three levels of ISO_SCAN_BLOCK elements per workgroup, the top one a single workgroup by construction: this grid
    has 1025 workgroups at level 0 and 2 at level 1, and its last workgroups are ragged."""
    from nerf import _hip
    block = _hip.ISO_SCAN_BLOCK
    nz = block * block // 4 + 77
    assert -(-(4 * nz) // block) > block                      # more level-0 totals than one level-1 workgroup scans
    f = np.random.default_rng(7).normal(size=(2, 2, nz)).astype(np.float32)
    xs, ys, zs = coords(2, 1), coords(2, 2), coords(nz, 3)
    assert same_mesh(extract(f, xs, ys, zs, 0.0, dev), restate(f, xs, ys, zs, 0.0))


@pytest.mark.gpu
def test_planted_vertices_at_160_cubed(dev):
    """Isolated inside vertices (+1 in a field of -1, level 0) at interior positions of odd coordinates - at least two grid steps apart
    - on 160^3 (4000 workgroups at scan level 0, 4 at level 1): each yields the 14 edges and 24 tetrahedra of the Kuhn triangulation
    at an interior vertex, every vertex at an edge midpoint.  Closed forms; no oracle at this size."""
    from nerf import _ops
    n, count = 160, 1500
    lattice = np.random.default_rng(11).permutation(79 ** 3)[:count]
    pos = np.stack([lattice // (79 * 79), (lattice // 79) % 79, lattice % 79], -1) * 2 + 1            # odd coordinates in 1 .. 157
    pos = np.concatenate([pos, [[1, 1, 1], [157, 157, 157], [1, 157, 63], [157, 1, 65]]])                 # the extreme interior positions
    pos = np.unique(pos, axis=0)
    count = len(pos)
    f = torch.full((n, n, n), -1.0, device=dev)
    f[tuple(G(pos, dev).T)] = 1.0
    axis = torch.arange(n, dtype=torch.float32, device=dev)
    v, t, bad = _ops.isosurface(f, axis, axis, axis, 0.0)
    torch.cuda.synchronize()
    v, t = C(v).astype(np.float64), C(t).astype(np.int64)
    assert bad == 0 and v.shape == (14 * count, 3) and t.shape == (24 * count, 3)
    # the expected vertices in (owner, slot) order: the planted vertex owns 7 edges, 7 neighbours own one edge each toward it
    offs = np.array([offset_of(c) for c in range(1, 8)])
    owner = np.concatenate([np.repeat(pos, 7, 0), (pos[:, None, :] - offs[None]).reshape(-1, 3)])
    slot = np.concatenate([np.tile(np.arange(7), count), np.tile(np.arange(7), count)])
    mid = owner + offs[slot] / 2.0
    order = np.lexsort((slot, (owner[:, 0] * n + owner[:, 1]) * n + owner[:, 2]))
    assert np.array_equal(v, mid[order])
    # connectivity: every triangle stays with one planted vertex, 24 each; closed, oriented outward (the inside is the planted vertex)
    gid = np.full((n, n, n), -1, np.int64)
    gid[tuple(pos.T)] = np.arange(count)
    cand = v[:, None, :] - np.concatenate([offs, -offs])[None] / 2.0          # the planted end of the vertex's edge is one of these
    whole = (cand == np.rint(cand)).all(-1)
    ci = np.where(whole[..., None], cand, 0).astype(np.int64)
    near = np.where(whole, gid[ci[..., 0], ci[..., 1], ci[..., 2]], -1)
    group = near.max(-1)
    assert (group >= 0).all() and ((near >= 0).sum(-1) == 1).all()
    tg = group[t]
    assert (tg[:, 0] == tg[:, 1]).all() and (tg[:, 0] == tg[:, 2]).all() and (np.bincount(tg[:, 0], minlength=count) == 24).all()
    assert len(open_edges(t, len(v))) == 0 and euler_characteristic(t) == 2 * count
    p = v[t]
    outward = np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(1) - pos[tg[:, 0]])
    assert (outward > 0).all()


@pytest.mark.gpu
def test_nonfinite_samples(dev):
    f, xs, ys, zs = FIELDS["noise"]()
    f[3, 3, 3], f[4, 4, 5], f[5, 2, 7], f[0, 0, 0], f[8, 7, 10] = np.nan, np.inf, -np.inf, np.nan, np.inf
    got = extract(f, xs, ys, zs, 0.0, dev)
    assert same_mesh(got, restate(f, xs, ys, zs, 0.0)) and got[2] == 5 and np.isfinite(got[0]).all()


@pytest.mark.gpu
def test_empty_surfaces(dev):
    f, xs, ys, zs = FIELDS["noise"]()
    for level in (float(f.max()) + 1.0, float(f.min()) - 1.0, float(f.max())):        # (f > max is false everywhere: strict)
        v, t, bad = extract(f, xs, ys, zs, level, dev)
        assert v.shape == (0, 3) and t.shape == (0, 3) and bad == 0


@pytest.mark.gpu
def test_capacities_bound_the_writes(dev):
    from nerf import _ops
    f, xs, ys, zs = FIELDS["noise"]()
    full_v, full_t, _ = extract(f, xs, ys, zs, 0.0, dev)
    counted = _ops.isosurface_count(G(f, dev), G(xs, dev), G(ys, dev), G(zs, dev), 0.0)
    assert counted.totals() == (len(full_v), len(full_t), 0) and int(counted.counts[3]) == 0
    for cap_v, cap_t in ((len(full_v) // 2, len(full_t) // 3), (1, 1), (0, 5), (7, 0), (len(full_v), len(full_t))):
        v = torch.full((len(full_v) + 8, 3), -7.0, device=dev)
        t = torch.full((len(full_t) + 8, 3), -7, dtype=torch.int32, device=dev)
        _ops.isosurface_emit(counted, cap_v, cap_t, v, t)
        torch.cuda.synchronize()
        v, t = C(v), C(t)
        assert np.array_equal(v[:cap_v].view(np.uint32), full_v[:cap_v].view(np.uint32)) and (v[cap_v:] == -7.0).all()
        assert np.array_equal(t[:cap_t], full_t[:cap_t]) and (t[cap_t:] == -7).all()
        assert counted.totals() == (len(full_v), len(full_t), 0)                 # the record carries the true totals


@pytest.mark.gpu
def test_strided_field_is_read_in_place(dev):
    from nerf import _ops
    f, xs, ys, zs = FIELDS["noise"]()
    rows = torch.full((f.size, 4), float("nan"), device=dev)
    rows[:, 3] = G(f, dev).reshape(-1)
    view = rows[:, 3].view(f.shape)
    counted = _ops.isosurface_count(view, G(xs, dev), G(ys, dev), G(zs, dev), 0.0)
    assert counted.stride == 4 and counted.field.data_ptr() == rows.data_ptr() + 12
    v, t, bad = _ops.isosurface(view, G(xs, dev), G(ys, dev), G(zs, dev), 0.0)
    assert same_mesh((C(v), C(t), bad), extract(f, xs, ys, zs, 0.0, dev))


@pytest.mark.gpu
def test_analytic_sphere_on_a_nonuniform_grid(dev):
    """Closedness, orientation and the Euler characteristic asserted on the kernel's output directly, and every geometric face normal
    against the direction of decreasing field (radially outward) at the face centroid."""
    def axis(seed):
        a = np.cumsum(np.random.default_rng(seed).uniform(0.6, 1.4, 24))
        return ((a - a[0]) / (a[-1] - a[0]) * 2.0 - 1.0).astype(np.float32)
    xs, ys, zs = axis(1), axis(2), axis(3)
    v, t, bad = extract(on_grid(sphere(0.7), xs, ys, zs), xs, ys, zs, 0.0, dev)
    assert bad == 0 and len(open_edges(t, len(v))) == 0 and euler_characteristic(t) == 2 and signed_volume(v, t) > 0
    p = v.astype(np.float64)[t]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", normal, p.mean(1)) > 0).all()


LEGO_BOX, LEGO_RES = (-1.2, -1.2, -1.2, 1.2, 1.2, 1.2), (24, 23, 25)


@pytest.fixture(scope="module")
def lego(dev):
    """The committed 4x128 fine network, its 24x23x25 density grid in fp32 and the median of that field as the threshold."""
    import nerf
    m = small_model(dev)
    ex = nerf.get_embedding_function(10)
    nerf.set_precision("fp32")
    with torch.no_grad():
        field, xs, ys, zs = nerf.density_grid(m, ex, LEGO_BOX, LEGO_RES)
    torch.cuda.synchronize()
    level = float(np.median(C(field)))
    return collections.namedtuple("Lego", "model ex field xs ys zs level")(m, ex, field, xs, ys, zs, level)


@pytest.mark.gpu
def test_density_grid_is_the_density_pack_on_the_grid_points(dev, lego):
    import nerf
    from nerf import _ops
    assert lego.field.shape == LEGO_RES and lego.field.dtype == torch.float32 and lego.field.is_contiguous()
    for c, lo, hi, n in zip((lego.xs, lego.ys, lego.zs), LEGO_BOX[:3], LEGO_BOX[3:], LEGO_RES):
        assert np.array_equal(C(c), np.linspace(lo, hi, n).astype(np.float32))
    pts = torch.stack(torch.meshgrid(lego.xs, lego.ys, lego.zs, indexing="ij"), -1).reshape(-1, 3).contiguous()
    with torch.no_grad():
        want = _ops.run_network_pts(lego.model.packed_density(True, True, precision=_ops._precision), pts, None, 1)[:, 3]
        slabs = nerf.density_grid(lego.model, lego.ex, LEGO_BOX, LEGO_RES, max_points=1000)[0]
    torch.cuda.synchronize()
    assert np.array_equal(C(lego.field).reshape(-1).view(np.uint32), C(want).view(np.uint32))
    assert np.array_equal(C(slabs).view(np.uint32), C(lego.field).view(np.uint32))           # one slab against fourteen
    assert np.isfinite(C(lego.field)).all() and C(lego.field).min() < lego.level < C(lego.field).max()


@pytest.mark.gpu
def test_extract_dex_mesh_end_to_end_fp32(dev, lego):
    import nerf
    with torch.no_grad():
        mesh = nerf.extract_dex_mesh(lego.model, lego.ex, LEGO_BOX, LEGO_RES, lego.level)
        again = nerf.extract_dex_mesh(lego.model, lego.ex, LEGO_BOX, LEGO_RES, lego.level, max_points=777, normals=False)
        sigma, g = nerf.density_gradient(lego.model, mesh.vertices, lego.ex)
    torch.cuda.synchronize()
    want = restate(C(lego.field), C(lego.xs), C(lego.ys), C(lego.zs), lego.level)
    assert len(want[0]) > 100 and same_mesh((C(mesh.vertices), C(mesh.triangles), mesh.n_nonfinite), want)
    assert same_mesh((C(again.vertices), C(again.triangles), again.n_nonfinite), want) and again.normals is None
    g = C(g).astype(np.float64)
    length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    ok = np.isfinite(length) & (length > 0)
    normals = np.where(ok[:, None], -g / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)
    assert mesh.normals.shape == mesh.vertices.shape and mesh.normals.dtype == torch.float32
    assert np.array_equal(C(mesh.normals), normals)
    assert ok.all() and np.allclose(np.linalg.norm(normals.astype(np.float64), axis=-1), 1.0, atol=1e-6)


@pytest.mark.gpu
def test_extract_dex_mesh_bf16_is_closed_away_from_the_boundary(dev, lego):
    """No accuracy figure is gated in bf16 (profiles/dex_mesh.md has them): the mesh is closed away from the grid boundary - a surface
    that leaves the box ends on its faces, where every open edge has both ends - and its normals are finite."""
    import nerf
    nerf.set_precision("bf16")
    with torch.no_grad():
        mesh = nerf.extract_dex_mesh(lego.model, lego.ex, LEGO_BOX, LEGO_RES, lego.level)
    torch.cuda.synchronize()
    v, t = C(mesh.vertices), C(mesh.triangles)
    assert len(v) > 100 and len(t) > 100 and mesh.n_nonfinite == 0
    e = open_edges(t, len(v))
    lo, hi = np.array(LEGO_BOX[:3], np.float32), np.array(LEGO_BOX[3:], np.float32)
    on_face = ((v == lo) | (v == hi)).any(-1)
    assert on_face[e].all()
    assert np.isfinite(C(mesh.normals)).all() and np.isfinite(v).all()


@pytest.mark.gpu
def test_eval_driver_mesh(dev, tmp_path, lego):
    import eval_nerf
    sd_c, sd_f = lego_weights()
    ck = tmp_path / "lego.ckpt"
    torch.save({"model_coarse_state_dict": {k: torch.from_numpy(v) for k, v in sd_c.items()},
                "model_fine_state_dict": {k: torch.from_numpy(v) for k, v in sd_f.items()}}, ck)
    out = tmp_path / "meshes" / "lego.ply"
    res = eval_nerf.main(["--checkpoint", str(ck), "--precision", "fp32", "--quiet", "--mesh", str(out),
                          "--mesh-bounds=" + ",".join(str(b) for b in LEGO_BOX), "--mesh-resolution", ",".join(str(r) for r in LEGO_RES), "--mesh-thres",
                          repr(lego.level)])
    props, rows, faces = read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert len(rows) == res["n_vertices"] == res["mesh"].vertices.shape[0] and len(faces) == res["n_triangles"] == res["mesh"].triangles.shape[0]
    want = restate(C(lego.field), C(lego.xs), C(lego.ys), C(lego.zs), np.float32(lego.level))
    assert np.array_equal(rows[:, :3], want[0]) and np.array_equal(faces, want[1])
