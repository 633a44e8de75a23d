"""Developer timing probe: the Dex threshold surface as a mesh (nerf.extract_dex_mesh) in its parts - the field pass
(nerf.density_grid: the density pack through dn_run_network in slabs), the extraction's two calls (dn_isosurface_count: classify and
the scans; dn_isosurface_emit: vertices and triangles into preallocated outputs; the C calls alone, and the count through the
binding) and the vertex normals - at 128^3 and 256^3 for D8/W256 and the as-shipped 4 x 128 nets under nerf.set_precision('bf16').  HIP events, `--warmup` untimed runs, the median of
`--iters`, one process.  The threshold is a quantile of the field itself (0.5: half the grid inside, a very large surface; 0.99: a
sparse one), so the surface is non-empty whatever the synthetic weights do.

Yardsticks, written beside the times: for the extraction the copy rate of the device (6.29 TB/s) applied to the bytes each call must
move - count: 4 B read + 2 B written per sample (classify), 2 B read (block totals), 2 B read + 8 B written (prefixes) = 18 B per
sample; emit: 2 B per sample read by each of its two launches, plus 12 B per vertex and per triangle written - and for the field pass
the depth-only render's density kernels at the same point count (profiles/depth_render_time.md: 25.2 ms per 40.96 M points D8/W256,
2.354 ms per 24.88 M points 4 x 128, bf16).  A last block gives the bf16 field against the fp32 field on the same grid.

    python scripts/dex_mesh_time.py [--out profiles/dex_mesh.json] [--md profiles/dex_mesh.md]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
import nerf  # noqa: E402
import bench  # noqa: E402
from nerf import _hip, _ops  # noqa: E402

D4 = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
NETS = [("D8/W256", None, 25.2 / 40.96e6), ("4x128", D4, 2.354 / 24.8832e6)]     # ms per point of the density kernels, bf16
COPY_BYTES_PER_MS = 6.29e12 / 1e3
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, accuracy = [], []
    for net, kw, ms_per_point in NETS:
        models, _, _, _, ex, _ = bench.build_scene(dev, 0, h=8, w=8, nc=64, nf=64, model_kw=kw)
        model = models[1]
        for n in (128, 256):
            nerf.set_precision("bf16")
            with torch.no_grad():
                field, xs, ys, zs = nerf.density_grid(model, ex, BOX, n)
                field_ms = timed(lambda: nerf.density_grid(model, ex, BOX, n), args.warmup, args.iters)
            points = n ** 3
            for q in (0.5, 0.99):
                level = float(torch.quantile(field.reshape(-1)[:: max(1, points // (1 << 22))].float(), q))
                counted = _ops.isosurface_count(field, xs, ys, zs, level)
                n_v, n_t, n_bad = counted.totals()
                vertices = torch.empty((max(n_v, 1), 3), dtype=torch.float32, device=dev)
                triangles = torch.empty((max(n_t, 1), 3), dtype=torch.int32, device=dev)
                # the two C calls alone, on the workspace and outputs allocated above ...
                lib, grid = _hip.lib(), counted._grid_args()
                count_ms = timed(lambda: _hip.check(lib.dn_isosurface_count(*grid, _hip.ptr(counted.counts), _hip.stream())), args.warmup, args.iters)
                emit_ms = timed(lambda: _hip.check(lib.dn_isosurface_emit(*grid, n_v, n_t, _hip.ptr(vertices), _hip.ptr(triangles), _hip.stream())),
                                args.warmup, args.iters)
                # ... and the binding's count with its host-side rule (three device-to-host copies of the coordinates) and its allocations
                count_binding_ms = timed(lambda: _ops.isosurface_count(field, xs, ys, zs, level), args.warmup, args.iters)
                with torch.no_grad():
                    whole_ms = timed(lambda: nerf.extract_dex_mesh(model, ex, BOX, n, level), 1, 3)
                count_floor = 18.0 * points / COPY_BYTES_PER_MS
                emit_floor = (4.0 * points + 12.0 * (n_v + n_t)) / COPY_BYTES_PER_MS
                row = dict(probe="dex_mesh_time", net=net, grid=f"{n}^3", points=points, precision="bf16", level_quantile=q, level=level,
                           vertices=n_v, triangles=n_t, nonfinite=n_bad, field_ms=field_ms, field_yardstick_ms=ms_per_point * points,
                           field_over_yardstick=field_ms / (ms_per_point * points), count_ms=count_ms, count_binding_ms=count_binding_ms,
                           count_copy_floor_ms=count_floor,
                           count_fraction_of_copy_rate=count_floor / count_ms, emit_ms=emit_ms, emit_copy_floor_ms=emit_floor,
                           emit_fraction_of_copy_rate=emit_floor / emit_ms, extraction_over_field=(count_ms + emit_ms) / field_ms,
                           whole_with_normals_ms=whole_ms)
                rows.append(row)
                print(json.dumps(row), flush=True)
            if n == 128:      # the bf16 field against the fp32 field on the same grid
                nerf.set_precision("fp32")
                with torch.no_grad():
                    ref = nerf.density_grid(model, ex, BOX, n)[0]
                level = float(torch.quantile(ref.reshape(-1).float()[:: 2], 0.5))
                a = _ops.isosurface_count(field, xs, ys, zs, level).totals()
                b = _ops.isosurface_count(ref, xs, ys, zs, level).totals()
                acc = dict(probe="dex_mesh_bf16_field", net=net, grid=f"{n}^3", level=level,
                           max_abs_err_over_max_abs=float((field - ref).abs().max() / ref.abs().max()),
                           inside_flips=float(((field > level) != (ref > level)).float().mean()),
                           vertices_bf16=a[0], vertices_fp32=b[0], triangles_bf16=a[1], triangles_fp32=b[1])
                accuracy.append(acc)
                print(json.dumps(acc), flush=True)
    nerf.set_precision("fp32")
    lines = ["| net | grid | level quantile | vertices | triangles | field ms | field / density-kernel yardstick | count ms | count: fraction of copy "
             "rate | count through the binding ms | emit ms | emit: fraction of copy rate | (count + emit) / field | extract_dex_mesh with normals ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['net']} | {r['grid']} | {r['level_quantile']} | {r['vertices']:,} | {r['triangles']:,} | {r['field_ms']:.3f} | "
                     f"{r['field_over_yardstick']:.2f} | {r['count_ms']:.3f} | {r['count_fraction_of_copy_rate']:.3f} | {r['count_binding_ms']:.3f} | "
                     f"{r['emit_ms']:.3f} | "
                     f"{r['emit_fraction_of_copy_rate']:.3f} | {r['extraction_over_field']:.3f} | {r['whole_with_normals_ms']:.2f} |")
    lines += ["", "| net | grid | level | max abs err / max abs (bf16 vs fp32 field) | inside flips | vertices bf16 / fp32 | triangles bf16 / fp32 |",
              "|---|---|---|---|---|---|---|"]
    for r in accuracy:
        lines.append(f"| {r['net']} | {r['grid']} | {r['level']:.4g} | {r['max_abs_err_over_max_abs']:.3e} | {r['inside_flips']:.3e} | "
                     f"{r['vertices_bf16']:,} / {r['vertices_fp32']:,} | {r['triangles_bf16']:,} / {r['triangles_fp32']:,} |")
    print("\n" + "\n".join(lines))
    for path, text in ((args.out, json.dumps(dict(device=torch.cuda.get_device_name(0), rows=rows, bf16_field=accuracy), indent=1)),
                       (args.md, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)


if __name__ == "__main__":
    main()
