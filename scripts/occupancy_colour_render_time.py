"""Developer timing probe: the occupancy-culled full colour render (nerf.run_one_iter_of_nerf(occupancy=...)) and the culled normal
render (nerf.render_dex_normals(occupancy=...)) beside the same renders without a grid - the code paths of the parent commit, which
this feature leaves untouched - by the method of scripts/occupancy_render_time.py, whose shapes, thresholds, clock and frustum box
this probe imports:
  * 400 x 400, 64 + 128 samples, D8/W256/skip 4 (the bench step), and
  * 270 x 480, 64 + 64 samples, the as-shipped 4 x 128 nets,
whole image in one chunk, K = 20 Dex thresholds, nerf.set_precision('bf16') with the render policy 'bf16' for both legs.  A host clock
around renders that end in a device synchronise, `--warmup` untimed renders, the median of `--iters`; the legs alternate a / b / a / b
in one process.

Per shape and render: the real grid of both networks, the kept fraction per pass, the culled render's time, the largest difference
from the render without a grid; then the sweep over random 32^3 masks with its least-squares line and break-even kept fraction.

    python scripts/occupancy_colour_render_time.py [--out profiles/occupancy_colour_render.md] [--only-shape 0|1] [--only colour|normals]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from occupancy_render_time import SHAPES, THRES, frustum_box, timed  # noqa: E402  (it puts the repository on sys.path)
import nerf  # noqa: E402
import bench  # noqa: E402


def colour_render(scene, h, w):
    models, cfg, ro, rd, ex, ed = scene

    def render(grid=None, **more):
        with torch.no_grad():
            return nerf.run_one_iter_of_nerf(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                             encode_direction_fn=ed, m_thres_cand=THRES, occupancy=grid, **more)

    def compare(culled, full):
        share = [float((a == b).float().mean()) for a, b in zip(culled[6:], full[6:])]
        return (f"largest |rgb| difference {float((culled[3] - full[3]).abs().max()):.3e}, expected depth differs by at most "
                f"{float((culled[4] - full[4]).abs().max()):.5f}, Dex depth equal in {100 * min(share):.3f} % (worst threshold) to "
                f"{100 * max(share):.3f} % (best) of the pixels")
    return render, compare


def normal_render(scene, h, w):
    models, cfg, ro, rd, ex, ed = scene

    def render(grid=None, **more):
        with torch.no_grad():
            return nerf.render_dex_normals(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                           m_thres_cand=THRES, occupancy=grid, **more)

    def compare(culled, full):
        share = [float((a == b).float().mean()) for a, b in zip(culled.dex_depth, full.dex_depth)]
        return (f"largest |normal| difference {float((culled.normal - full.normal).abs().max()):.3e}, expected depth differs by at most "
                f"{float((culled.depth - full.depth).abs().max()):.5f}, Dex depth equal in {100 * min(share):.3f} % (worst threshold) to "
                f"{100 * max(share):.3f} % (best) of the pixels")
    return render, compare


RENDERS = {"colour": ("Full colour render (`nerf.run_one_iter_of_nerf`)", colour_render),
           "normals": ("Normal render (`nerf.render_dex_normals`)", normal_render)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "occupancy_colour_render.md"))
    ap.add_argument("--only-shape", type=int, default=-1)
    ap.add_argument("--only", default="", choices=["", "colour", "normals"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    nerf.set_precision("bf16")
    nerf.set_render_policy("bf16")
    lines = ["# Occupancy-culled colour and normal renders against the renders without a grid (MI355X)", "",
             f"`scripts/occupancy_colour_render_time.py`, the method of `profiles/occupancy_render.md`: host clock around renders that end in a "
             f"device synchronise, {args.warmup} warm-up renders, the median of {args.iters}, whole image in one chunk, K = 20 Dex thresholds, "
             "`nerf.set_precision('bf16')`, render policy `bf16` for both legs (the culled renders run in bf16).  `no grid` is the same call "
             "without `occupancy`: the parent commit's code path, which this feature does not touch; it and the culled render were run "
             f"alternately (a / b) in one process on one device ({torch.cuda.get_device_name(0)}).  The box-to-box spread of such timings is "
             "about 7 % (README): a ratio inside it is no difference.", "",
             "The networks are the benchmark's synthetic ones (seeded random weights with a density bias): the kept fractions and the "
             "differences from the render without a grid below are those of that field, not of a table-top scene - a random field has "
             "structure below the cell size.  The lines through the sweeps and the break-even fractions are properties of the renders and "
             "carry over to a trained scene; its kept fraction is what `eval_nerf.py --occupancy CELLS --occupancy-colour --occupancy-check` "
             "prints.", ""]
    for si, (net, h, w, nc, nf, kw) in enumerate(SHAPES):
        if args.only_shape >= 0 and si != args.only_shape:
            continue
        scene = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=nf, model_kw=kw)
        models, _, ro, rd, ex, _ = scene
        box = frustum_box(ro, rd)
        with torch.no_grad():
            grid = nerf.OccupancyGrid.from_networks(models, ex, box, args.cells, level=args.level, dilate=args.dilate)
        for which, (title, make) in RENDERS.items():
            if args.only and which != args.only:
                continue
            render, compare = make(scene, h, w)
            full_ms, culled_ms = [], []
            for _ in range(2):
                full_ms.append(timed(render, args.warmup, args.iters))
                culled_ms.append(timed(lambda: render(grid), args.warmup, args.iters))
            culled_out = render(grid, cull_stats=True)
            stats = culled_out[-1]
            culled_maps = culled_out[0] if which == "normals" else culled_out[:-1]
            check = compare(culled_maps, render())
            del culled_out, culled_maps
            total = sum(stats["total"])
            sweep = []
            rng = np.random.default_rng(0)
            for f in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0):
                g = nerf.OccupancyGrid.from_mask(torch.from_numpy(rng.random((32, 32, 32)) < f).to(dev), box)
                ms = timed(lambda: render(g), args.warmup, args.iters)
                sweep.append((f, sum(render(g, cull_stats=True)[-1]["kept"]) / total, ms))
            slope, intercept = np.polyfit([s[1] for s in sweep], [s[2] for s in sweep], 1)
            parent, culled = statistics.median(full_ms), statistics.median(culled_ms)
            kept_all = sum(stats["kept"]) / total
            breakeven = (parent - intercept) / slope
            ratio = culled / parent
            verdict = "no difference (inside the 7 % box-to-box spread)" if abs(ratio - 1.0) <= 0.07 else ("faster" if ratio < 1.0 else "slower")
            lines += [f"## {title}: {net}, {h}x{w}, {nc}+{nf} samples", "",
                      f"Grid: {args.cells}^3 cells over the camera's frustum box, level {args.level:g}, dilate {args.dilate}, both networks OR-ed: "
                      f"{100 * grid.occupied_fraction():.2f} % of the cells set.", "",
                      "| leg | ms per image (a / b) | median |", "|---|---|---|",
                      f"| no grid (parent path), bf16 | {full_ms[0]:.3f} / {full_ms[1]:.3f} | {parent:.3f} |",
                      f"| culled, bf16 | {culled_ms[0]:.3f} / {culled_ms[1]:.3f} | {culled:.3f} |", "",
                      f"Kept samples: coarse {stats['kept'][0]} of {stats['total'][0]} ({100 * stats['kept'][0] / stats['total'][0]:.2f} %), fine "
                      f"{stats['kept'][1]} of {stats['total'][1]} ({100 * stats['kept'][1] / max(stats['total'][1], 1):.2f} %), all "
                      f"{100 * kept_all:.2f} %; non-finite values among the gathered ones: {stats['nonfinite']}.", "",
                      f"**Culled / no grid = {ratio:.3f}** at a kept fraction of {kept_all:.3f}: {verdict}.", "",
                      f"Against the render without a grid (bf16 both): {check}.", "",
                      "Sweep over random 32^3 masks:", "", "| cells set | kept fraction of all samples | culled ms |", "|---|---|---|"]
            lines += [f"| {f:.2f} | {k:.4f} | {ms:.3f} |" for f, k, ms in sweep]
            lines += ["", f"Least-squares line: ms = {intercept:.3f} + {slope:.3f} x kept fraction.  **Break-even kept fraction: {breakeven:.3f}** "
                          f"(where the line meets the {parent:.3f} ms of the render without a grid); the fixed cost of culling is the intercept, "
                          f"{intercept:.3f} ms.", ""]
            print(f"{which} {net}: no grid {parent:.3f} ms, culled {culled:.3f} ms, kept {kept_all:.4f}, break-even {breakeven:.3f}", flush=True)
            with open(args.out + ".part", "w") as fh:        # what is measured so far, should a later leg run out of time
                fh.write("\n".join(lines))
    lines += ["## Rays mode against explicit-points mode of the network kernels", "",
              "The culled renders hand the networks explicit points (the colour render: with one view direction row per point) where the "
              "renders without a grid hand them ray rows and depths.  Measured on the points of `tests/test_occupancy_colour_render.py` (37 rays, "
              "37 + 22 samples, coarse and fine network of the 4x128 and the D8/W256 shape, fp32 and bf16) with entry points this feature "
              "does not touch, so on the parent commit's code: the largest difference between `run_network_rays` and `run_network_pts` over "
              "all four columns is 0, and the largest difference between `density_gradient(rays=, z=)` and `density_gradient(pts=)` is 0 in "
              "sigma and in the gradient.  A grid with every cell set therefore renders the bits of the render without a grid - colour, "
              "depth, accumulation, Dex depths, normals - and the tests assert that, repeating both measurements first.", ""]
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if os.path.exists(args.out + ".part"):
        os.remove(args.out + ".part")


if __name__ == "__main__":
    main()
