#!/usr/bin/env python3
"""Build-owned counterpart of the reference's eval_nerf.py (:116-206): load a checkpoint (the reference's dict format:
model_coarse_state_dict / model_fine_state_dict, optional height / width / focal_length), render a sweep of spherical
poses in validation mode, optionally save RGB / disparity-style depth PNGs, and print the average time per image.
`--depth-only --m-thres M` renders the depth and Dex depth maps alone (nerf.render_dex_depth): no colour is evaluated, no RGB PNG
is written, and the maps go to dex_<view>.npz beside depth_<view>.png.  `--depth-quantiles 0.1,0.5,0.9 [--quantile-interp]` adds the
opacity-quantile depth maps (0.5: the median depth) to the same render and the same file (quantiles / qdepth), with or without --m-thres.
`--depth-only --m-thres M --dex-refine R [--dex-refine-width]` adds the refined Dex depth maps (nerf.render_dex_depth(refine_steps=R): the first
crossing bracketed between two samples, halved R times on the density network, interpolated) as dex_refined / dex_width in the same file.
`--depth-only --m-thres M --dex-layers L [--dex-refine R] [--dex-refine-width]` adds the depth layers (nerf.render_dex_layers: every entry
into and exit from the region above the threshold, the first L layers stored) as dex_events / dex_event_count (/ dex_event_width).
`--depth-only --occupancy N[,N,N] [--occupancy-bounds x0 y0 z0 x1 y1 z1] [--occupancy-level L] [--occupancy-dilate D]` builds an
occupancy grid of the two networks (nerf.OccupancyGrid.from_networks) and renders with the networks evaluated only on the samples in
set cells; `--occupancy-check` renders every view both ways and reports, per threshold, the share of equal Dex depths.
`--occupancy N[,N,N] --occupancy-colour` culls the full colour render the same way (nerf.run_one_iter_of_nerf(occupancy=...)), and
`--normals --occupancy N[,N,N]` the normal render (nerf.render_dex_normals(occupancy=...)); with `--occupancy-colour`, `--occupancy-check`
also reports the largest |rgb| difference.
`--ray-span N[,N,N] [--ray-span-pad P]` (with `--depth-only`, `--normals` or the colour render) tightens every ray's near / far to the
occupied span of such a grid before the render (ray_span= of the three renders): the same number of samples, spent where the grid has set
cells.  It shares --occupancy-bounds / --occupancy-level / --occupancy-dilate, which are legal with --ray-span alone; when --occupancy names
the same cells one grid serves both.  Per view it prints the share of rays that hit a set cell and the mean of (t_hi - t_lo) / (far - near)
over them.
`--normals` renders density-gradient surface normals (nerf.render_dex_normals) instead: normal_<view>.npy holds the expected normal
(H,W,3) (not renormalised: its length is a confidence), normal_<view>.png shows (n/|n| + 1)/2, black where n = 0; with `--m-thres M` the
same pair per threshold, dex_normal_<view>_m<threshold>.npy / .png - the normal at the sample the Dex depth reports.
`--mesh OUT.ply --mesh-bounds=x0,y0,z0,x1,y1,z1 --mesh-resolution N[,N,N] --mesh-thres T` renders nothing: it extracts the Dex threshold
surface {sigma > T} of the fine network (the coarse one without a fine network) as a triangle mesh with vertex normals
(nerf.extract_dex_mesh) and writes it as a binary PLY.

    python dex-nerf_amd/eval_nerf.py --checkpoint ckpt.ckpt --size 400 --views 8 --precision fp16 --savedir out/

The network shape (layers / width) is read off the checkpoint tensors, so the reference's shipped 4x128
`pretrained/*/checkpoint*.ckpt` files and checkpoints written by train_dexnerf.py both load unchanged.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import nerf  # noqa: E402
from nerf import _ops, synthetic as syn  # noqa: E402


def model_from_state_dict(sd, dev):
    """FlexibleNeRFModel whose constructor arguments are inferred from the tensor shapes (reference key names)."""
    width = sd["layer1.weight"].shape[0]
    dim_xyz = sd["layer1.weight"].shape[1]
    n_trunk = len([k for k in sd if k.startswith("layers_xyz.") and k.endswith(".weight")])
    wide = [i for i in range(n_trunk) if sd[f"layers_xyz.{i}.weight"].shape[1] != width]
    use_viewdirs = "fc_rgb.weight" in sd
    dim_dir = sd["layers_dir.0.weight"].shape[1] - width if use_viewdirs else 0
    skip = wide[0] if wide else n_trunk + 1  # a skip that never fires reproduces a skip-free checkpoint
    m = nerf.models.FlexibleNeRFModel(num_layers=n_trunk + 1, hidden_size=width, skip_connect_every=max(skip, 1),
                                      num_encoding_fn_xyz=(dim_xyz - 3) // 6, num_encoding_fn_dir=max((dim_dir - 3) // 6, 0),
                                      use_viewdirs=use_viewdirs)
    m.load_state_dict(sd)
    return m.to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--size", type=int, default=0, help="image size (default: checkpoint's height, else 100)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--num-coarse", type=int, default=64)
    ap.add_argument("--num-fine", type=int, default=128)
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--far", type=float, default=6.0)
    ap.add_argument("--white-background", action="store_true")
    ap.add_argument("--m-thres", type=int, default=0, help="> 0: also produce the Dex depth maps for thresholds 5..m")
    ap.add_argument("--depth-only", action="store_true",
                    help="render depth / Dex depth maps only (nerf.render_dex_depth: density sub-networks, no colour); needs --m-thres > 0 or "
                         "--depth-quantiles")
    ap.add_argument("--depth-quantiles", default="", metavar="Q,Q,...",
                    help="--depth-only: also the opacity-quantile depth maps - the depth at which the ray's accumulated opacity reaches q "
                         "(0.5: the median depth), e.g. 0.1,0.5,0.9; at most 64 values strictly inside (0, 1); saved as quantiles / qdepth")
    ap.add_argument("--quantile-interp", action="store_true",
                    help="--depth-quantiles: the piecewise-linear CDF inversion instead of the depth of the crossing sample")
    ap.add_argument("--dex-refine", type=int, default=None, metavar="R",
                    help="--depth-only --m-thres: also the refined Dex depth maps - the first crossing bracketed between two samples, halved "
                         "R times (0..24) on the density network and interpolated (nerf.render_dex_depth(refine_steps=R)); saved as "
                         "dex_refined beside dex; not with --depth-quantiles or --occupancy")
    ap.add_argument("--dex-refine-width", action="store_true",
                    help="--dex-refine: also the width of the last bracket per pixel (-1: no crossing, 0: crossing at the first sample); "
                         "saved as dex_width")
    ap.add_argument("--dex-layers", type=int, default=None, metavar="L",
                    help="--depth-only --m-thres: also the depth layers - every entry into and exit from the region above the threshold "
                         "along each ray, the first L layers (1..8) stored (nerf.render_dex_layers, one more depth-only render per view); "
                         "saved as dex_events (K,2L,H,W; +inf: no such event) and dex_event_count (K,H,W) beside dex; with --dex-refine R "
                         "the events are refined like dex_refined, with --dex-refine-width dex_event_width is saved too; not with "
                         "--depth-quantiles")
    ap.add_argument("--normals", action="store_true",
                    help="render surface normals only (nerf.render_dex_normals: the density gradient at the samples, composited like the "
                         "depth; with --m-thres also the normal at every Dex depth); not with --precision fp16")
    ap.add_argument("--mesh", default="", metavar="OUT.ply",
                    help="extract the Dex threshold surface of the fine network (the coarse one without a fine network) as a triangle mesh "
                         "with vertex normals (nerf.extract_dex_mesh) and write it as a binary PLY instead of rendering; needs "
                         "--mesh-bounds and --mesh-thres; not with --precision fp16")
    ap.add_argument("--mesh-bounds", default="", metavar="x0,y0,z0,x1,y1,z1", help="--mesh: the box the grid spans, in the network's input space (write --mesh-bounds=-1,... when it starts with a minus)")
    ap.add_argument("--mesh-resolution", default="128", metavar="N[,N,N]", help="--mesh: grid points per axis (one number, or nx,ny,nz)")
    ap.add_argument("--mesh-thres", type=float, default=None, metavar="T", help="--mesh: the Dex threshold m_thres on the raw density")
    ap.add_argument("--occupancy", default="", metavar="N[,N,N]",
                    help="--depth-only: cull the ray samples against an occupancy grid of this many cells per axis (nerf.OccupancyGrid."
                         "from_networks on the coarse and the fine network) - the density networks run only where a cell is set; not with "
                         "--precision fp16")
    ap.add_argument("--occupancy-bounds", type=float, nargs=6, default=None, metavar=("x0", "y0", "z0", "x1", "y1", "z1"),
                    help="--occupancy: the grid's box in the network's input space (default: the box around every rendered camera's corner "
                         "rays between near and far)")
    ap.add_argument("--occupancy-level", type=float, default=0.0, metavar="L",
                    help="--occupancy: a cell is set when the raw density at one of its corners exceeds L (default 0: what a ReLU passes)")
    ap.add_argument("--occupancy-dilate", type=int, default=1, metavar="D", help="--occupancy: also set the cells within D cells of a set one (0..8)")
    ap.add_argument("--occupancy-colour", action="store_true",
                    help="--occupancy without --depth-only: cull the full colour render (nerf.run_one_iter_of_nerf(occupancy=...)) - both "
                         "networks, colour heads included, run only where a cell is set; not with --depth-only or --normals")
    ap.add_argument("--occupancy-check", action="store_true",
                    help="--occupancy: render every view with and without the grid (both in the configured precision) and print, per "
                         "threshold, the share of pixels with equal Dex depth and the largest depth difference - how to find the cells and "
                         "the dilation a scene needs")
    ap.add_argument("--ray-span", default="", metavar="N[,N,N] | checkpoint",
                    help="tighten every ray's near / far to the occupied span of an occupancy grid of this many cells per axis before the "
                         "render (ray_span= of render_dex_depth, render_dex_normals and run_one_iter_of_nerf); shares --occupancy-bounds / "
                         "-level / -dilate, and the grid itself when --occupancy names the same cells.  `checkpoint`: the grid stored in the "
                         "checkpoint by train_dexnerf.py --train-occupancy instead of one built here")
    ap.add_argument("--ray-span-pad", type=float, default=None, metavar="P",
                    help="--ray-span: widen each span by P cells of travel at both ends (default 1)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--savedir", default="")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--use-refined-poses", action="store_true",
                    help="a checkpoint of train_dexnerf.py --refine-poses: render its training views at the refined cameras it carries "
                         "(refined_extrinsics / refined_intrinsics) instead of the spherical sweep; --size must be the training size")
    ap.add_argument("--apply-exposure", action="store_true",
                    help="--use-refined-poses on a checkpoint of train_dexnerf.py --refine-exposure: show every training view in its own "
                         "stored exposure (nerf.apply_exposure); the default render is at the canonical exposure, the identity")
    args = ap.parse_args(argv)

    try:
        quantiles = _ops.check_quantiles([float(q) for q in args.depth_quantiles.split(",") if q.strip()], "--depth-quantiles")
    except ValueError as e:
        ap.error(str(e))
    if (quantiles or args.quantile_interp) and not args.depth_only:
        ap.error("--depth-quantiles / --quantile-interp belong to --depth-only")
    if args.quantile_interp and not quantiles:
        ap.error("--quantile-interp needs --depth-quantiles")
    if args.depth_only and args.m_thres <= 0 and not quantiles:
        ap.error("--depth-only renders the Dex / quantile depth maps: give --m-thres > 0 or --depth-quantiles")
    if args.dex_refine is not None:
        try:
            _ops.check_refine_steps(args.dex_refine, "--dex-refine")
        except ValueError as e:
            ap.error(str(e))
        if not args.depth_only or args.m_thres <= 0:
            ap.error("--dex-refine refines the Dex depth maps of --depth-only: it needs --depth-only and --m-thres > 0")
        if quantiles or args.occupancy:
            ap.error("--dex-refine is not supported together with --depth-quantiles or --occupancy")
    elif args.dex_refine_width and args.dex_layers is None:
        ap.error("--dex-refine-width belongs to --dex-refine")
    if args.dex_layers is not None:
        try:
            _ops.check_layers(args.dex_layers, "--dex-layers")
        except ValueError as e:
            ap.error(str(e))
        if not args.depth_only or args.m_thres <= 0:
            ap.error("--dex-layers reads the layers of the Dex thresholds of --depth-only: it needs --depth-only and --m-thres > 0")
        if quantiles:
            ap.error("--dex-layers is not supported together with --depth-quantiles")
    if args.normals and args.precision == "fp16":
        ap.error("--normals differentiates the density network on the training kernels, which exist for fp32 and bf16: not with --precision fp16")
    if args.normals and (args.depth_only or args.apply_exposure):
        ap.error("--normals is a render of its own: not with --depth-only or --apply-exposure")
    if args.apply_exposure and (not args.use_refined_poses or args.depth_only):
        ap.error("--apply-exposure corrects the colours of training views: it needs --use-refined-poses and no --depth-only")
    mesh_bounds = mesh_res = None
    if args.mesh:
        if args.precision == "fp16":
            ap.error("--mesh samples the density on the kernels of the density gradient, which exist for fp32 and bf16: not with --precision fp16")
        if args.depth_only or args.normals or args.apply_exposure or args.use_refined_poses:
            ap.error("--mesh is an extraction of its own: not with --depth-only, --normals, --use-refined-poses or --apply-exposure")
        try:
            mesh_bounds = [float(v) for v in args.mesh_bounds.split(",") if v.strip()]
            mesh_res = [int(v) for v in args.mesh_resolution.split(",") if v.strip()]
        except ValueError as e:
            ap.error(f"--mesh-bounds / --mesh-resolution: {e}")
        if len(mesh_bounds) != 6 or len(mesh_res) not in (1, 3) or min(mesh_res) < 2:
            ap.error("--mesh needs --mesh-bounds x0,y0,z0,x1,y1,z1 and --mesh-resolution N or nx,ny,nz with at least 2 points per axis")
        if not all(np.isfinite(mesh_bounds)) or any(mesh_bounds[a + 3] <= mesh_bounds[a] for a in range(3)):
            ap.error("--mesh-bounds: x1 > x0, y1 > y0, z1 > z0, all finite")
        if args.mesh_thres is None or not np.isfinite(np.float32(args.mesh_thres)):
            ap.error("--mesh needs a finite --mesh-thres")
        mesh_res = mesh_res * 3 if len(mesh_res) == 1 else mesh_res
    elif args.mesh_bounds or args.mesh_thres is not None:
        ap.error("--mesh-bounds / --mesh-thres belong to --mesh")
    def grid_cells(flag, text):
        try:
            cells = [int(v) for v in text.split(",") if v.strip()]
        except ValueError as e:
            ap.error(f"{flag}: {e}")
        if len(cells) not in (1, 3):
            ap.error(f"{flag} takes N or cx,cy,cz")
        cells = cells * 3 if len(cells) == 1 else cells
        try:
            _ops.check_occupancy_grid(args.occupancy_bounds or (0, 0, 0, 1, 1, 1), cells, flag)
        except ValueError as e:
            ap.error(str(e))
        if not np.isfinite(np.float32(args.occupancy_level)):
            ap.error("--occupancy-level must be finite")
        if not 0 <= args.occupancy_dilate <= 8:
            ap.error("--occupancy-dilate must be 0..8")
        return cells
    occ_cells = span_cells = None
    if args.ray_span:
        if args.mesh:
            ap.error("--ray-span tightens the rays of a render: not with --mesh")
        if args.ray_span == "checkpoint":      # the grid train_dexnerf.py --train-occupancy kept beside the networks and stored with them
            if args.occupancy_bounds is not None or args.occupancy_level != 0.0 or args.occupancy_dilate != 1:
                ap.error("--ray-span checkpoint uses the stored grid as it is: --occupancy-bounds / -level / -dilate belong to a grid built here")
            span_cells = "checkpoint"
        else:
            span_cells = grid_cells("--ray-span", args.ray_span)
        try:
            _ops.check_ray_span_pad(1.0 if args.ray_span_pad is None else args.ray_span_pad, "--ray-span-pad")
        except ValueError as e:
            ap.error(str(e))
    elif args.ray_span_pad is not None:
        ap.error("--ray-span-pad belongs to --ray-span")
    if args.occupancy:
        if not (args.depth_only or args.occupancy_colour or args.normals):
            ap.error("--occupancy culls the depth-only render: it needs --depth-only (or --occupancy-colour for the colour render, "
                     "--normals for the normal render)")
        if args.occupancy_colour and (args.depth_only or args.normals):
            ap.error("--occupancy-colour culls the full colour render: not with --depth-only or --normals")
        if args.occupancy_check and args.normals:
            ap.error("--occupancy-check compares depth-only or colour renders: not with --normals")
        if args.precision == "fp16":
            ap.error("--occupancy evaluates explicit points, which run in fp32 or bf16: not with --precision fp16")
        occ_cells = grid_cells("--occupancy", args.occupancy)
        if args.occupancy_check and args.m_thres <= 0 and not args.occupancy_colour:
            ap.error("--occupancy-check compares Dex depths: it needs --m-thres > 0")
    elif args.occupancy_check or args.occupancy_colour:
        ap.error("--occupancy-check / --occupancy-colour belong to --occupancy")
    elif not span_cells and (args.occupancy_bounds is not None or args.occupancy_level != 0.0 or args.occupancy_dilate != 1):
        ap.error("--occupancy-bounds / --occupancy-level / --occupancy-dilate belong to --occupancy or --ray-span")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    nerf.set_precision(args.precision)
    ck = torch.load(args.checkpoint, map_location="cpu")
    coarse = model_from_state_dict(ck["model_coarse_state_dict"], dev)
    fine = model_from_state_dict(ck["model_fine_state_dict"], dev) if ck.get("model_fine_state_dict") else None
    if ck.get("encoding_anneal") is not None:      # a checkpoint from inside a coarse-to-fine schedule: rendered at its stored amplitudes
        anneal = nerf.EncodingAnneal.from_state_dict(ck["encoding_anneal"]).attach(coarse, fine)
        if not args.quiet:
            print(f"encoding anneal {anneal.start:g}..{anneal.end:g} at iteration {anneal.iteration}: amplitudes "
                  f"{[round(a, 4) for a in anneal.amplitudes().tolist()]}", flush=True)
    size = args.size or int(ck.get("height", 100))
    mode = dict(chunksize=size * size, lindisp=False, num_coarse=args.num_coarse, num_fine=args.num_fine if fine else 0,
                perturb=False, radiance_field_noise_std=0.0, white_background=args.white_background)
    cfg = nerf.CfgNode(dict(dataset=dict(near=args.near, far=args.far, no_ndc=True),
                            nerf=dict(use_viewdirs=coarse.use_viewdirs, train=dict(mode), validation=dict(mode))))
    ex = nerf.get_embedding_function(coarse.num_encoding_fn_xyz, True, True)
    ed = nerf.get_embedding_function(coarse.num_encoding_fn_dir, True, True) if coarse.use_viewdirs else None
    if args.mesh:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            mesh = nerf.extract_dex_mesh(fine if fine is not None else coarse, ex, mesh_bounds, mesh_res, args.mesh_thres)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        if os.path.dirname(args.mesh):
            os.makedirs(os.path.dirname(args.mesh), exist_ok=True)
        nerf.save_ply(args.mesh, mesh)
        if not args.quiet:
            print(f"mesh: {mesh.vertices.shape[0]} vertices, {mesh.triangles.shape[0]} triangles at m_thres {args.mesh_thres:g} on a "
                  f"{mesh_res[0]}x{mesh_res[1]}x{mesh_res[2]} grid ({mesh.n_nonfinite} non-finite samples) in {seconds:.3f} s -> {args.mesh}",
                  flush=True)
        return dict(mesh=mesh, seconds=seconds, n_vertices=int(mesh.vertices.shape[0]), n_triangles=int(mesh.triangles.shape[0]))
    thres = np.arange(5, args.m_thres + 5, 5) if args.m_thres > 0 else None
    k_mat = torch.from_numpy(syn.intrinsic(size, size)).to(dev)
    if "focal_length" in ck:
        k_mat[0, 0] = k_mat[1, 1] = float(ck["focal_length"])
    if args.savedir:
        os.makedirs(args.savedir, exist_ok=True)
    times, frames = [], []
    if args.use_refined_poses:
        if "refined_extrinsics" not in ck:
            ap.error("--use-refined-poses: the checkpoint carries no refined cameras (train_dexnerf.py --refine-poses writes them)")
        refined_e = torch.as_tensor(ck["refined_extrinsics"], dtype=torch.float32, device=dev)
        refined_k = torch.as_tensor(ck["refined_intrinsics"], dtype=torch.float32, device=dev)
        cameras = [(refined_e[v], refined_k[v] if refined_k.dim() == 3 else refined_k) for v in range(refined_e.shape[0])]
        if args.apply_exposure and "refined_exposure" not in ck:
            ap.error("--apply-exposure: the checkpoint carries no exposure rows (train_dexnerf.py --refine-exposure writes them)")
    else:
        cameras = [(torch.from_numpy(syn.scene_pose(i, n_views=args.views)).to(dev), k_mat) for i in range(args.views)]
    grid, cull, check, rgb_diff = None, dict(kept=[0, 0], total=[0, 0], nonfinite=0), [], []

    def tally(stats):
        for p in range(2):
            cull["kept"][p] += stats["kept"][p]
            cull["total"][p] += stats["total"][p]
        cull["nonfinite"] += stats["nonfinite"]
    def build_grid(cells, what):
        bounds = args.occupancy_bounds
        if bounds is None:      # the box around the corner rays of every camera between near and far: it holds every sample
            corners = []
            for pose, k_cam in cameras:
                ro, rd = nerf.get_ray_bundle(size, size, float(k_cam[0, 0]), pose, k_cam)
                ro, rd = ro[[0, 0, -1, -1], [0, -1, 0, -1]].double(), rd[[0, 0, -1, -1], [0, -1, 0, -1]].double()
                corners += [ro + rd * args.near, ro + rd * args.far]
            pts = torch.cat(corners).cpu().numpy()
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            pad = 1e-3 * np.maximum(hi - lo, 1e-6)
            bounds = list(lo - pad) + list(hi + pad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            grid = nerf.OccupancyGrid.from_networks([coarse, fine], ex, bounds, cells, level=args.occupancy_level,
                                                    dilate=args.occupancy_dilate)
        torch.cuda.synchronize()
        if not args.quiet:
            print(f"{what} grid {cells[0]}x{cells[1]}x{cells[2]} over {[round(float(b), 4) for b in grid.bounds]}: "
                  f"{100 * grid.occupied_fraction():.2f} % of the cells set (level {args.occupancy_level:g}, dilate {args.occupancy_dilate}) "
                  f"in {time.perf_counter() - t0:.3f} s", flush=True)
        return grid
    span_grid, span_rows = None, []
    span_kw = {}
    if occ_cells:
        grid = build_grid(occ_cells, "occupancy and ray-span" if span_cells == occ_cells else "occupancy")
        if args.occupancy_check and args.precision == "bf16":
            nerf.set_render_policy("bf16")      # the culled render runs in bf16: compare it with a bf16 full render, not the guarded fp16 one
    if span_cells:
        if span_cells == "checkpoint":
            if ck.get("train_occupancy") is None:
                ap.error("--ray-span checkpoint: the checkpoint carries no occupancy grid (train_dexnerf.py --train-occupancy writes one)")
            span_grid = nerf.LiveOccupancyGrid.from_state_dict(ck["train_occupancy"], dev).grid
            if not args.quiet:
                print(f"ray-span grid {'x'.join(str(c) for c in span_grid.cells)} over {[round(float(b), 4) for b in span_grid.bounds]} from the "
                      f"checkpoint: {100 * span_grid.occupied_fraction():.2f} % of the cells set", flush=True)
        else:
            span_grid = grid if span_cells == occ_cells else build_grid(span_cells, "ray-span")
        span_kw = dict(ray_span=span_grid, ray_span_pad=args.ray_span_pad)

    def report_spans(view, ro, rd):
        """(outside the timed render) the share of rays that hit a set cell and the mean span fraction over them"""
        rows = _ops.pack_ray_rows(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), None, args.near, args.far)
        span, visits = span_grid.ray_spans(rows, pad_cells=1.0 if args.ray_span_pad is None else args.ray_span_pad)
        hit = visits > 0
        share = float(hit.float().mean())
        fraction = float(((span[:, 1] - span[:, 0]) / (args.far - args.near))[hit].mean()) if bool(hit.any()) else float("nan")
        span_rows.append(dict(view=view, hit_share=share, mean_span_fraction=fraction))
        if not args.quiet:
            print(f"ray span view {view}: {100 * share:.2f} % of the rays hit a set cell, mean span {100 * fraction:.2f} % of [near, far]", flush=True)
    for i, (pose, k_mat) in enumerate(cameras):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.normals:
            with torch.no_grad():
                ro, rd = nerf.get_ray_bundle(size, size, float(k_mat[0, 0]), pose, k_mat)
                out = nerf.render_dex_normals(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                              encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres, occupancy=grid,
                                              cull_stats=grid is not None, **span_kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            if span_grid is not None:
                report_spans(i, ro, rd)
            if grid is not None:
                out, stats = out
                tally(stats)
            frames.append((None, out.depth, out))
            if args.savedir:   # every normal map as float32, and as a PNG of the unit normal (black: no normal)
                from PIL import Image

                def save(stem, n):
                    n = n.cpu().numpy()
                    np.save(os.path.join(args.savedir, stem + ".npy"), n)
                    length = np.linalg.norm(n, axis=-1, keepdims=True)
                    unit = np.where(length > 0, (n / np.maximum(length, 1e-30) + 1.0) / 2.0, 0.0)
                    Image.fromarray((255 * unit).astype(np.uint8)).save(os.path.join(args.savedir, stem + ".png"))
                save(f"normal_{i:04d}", out.normal)
                for m, n in zip(thres if thres is not None else [], out.dex_normal):
                    save(f"dex_normal_{i:04d}_m{int(m)}", n)
            continue
        if args.depth_only:
            with torch.no_grad():
                ro, rd = nerf.get_ray_bundle(size, size, float(k_mat[0, 0]), pose, k_mat)
                out = nerf.render_dex_depth(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres,
                                            quantiles=quantiles or None, quantile_interp=args.quantile_interp, occupancy=grid,
                                            cull_stats=grid is not None, refine_steps=args.dex_refine,
                                            refine_width=args.dex_refine_width and args.dex_refine is not None, **span_kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            if span_grid is not None:
                report_spans(i, ro, rd)
            if grid is not None:
                *out, stats = out
                tally(stats)
                if args.occupancy_check and thres is not None:
                    with torch.no_grad():
                        full = nerf.render_dex_depth(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                                     encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres)
                    check.append([(float((a == b).float().mean()), float((a - b).abs().max())) for a, b in zip(out[4:4 + len(thres)], full[4:])])
            depth = out[2] if fine is not None else out[0]
            n_dex = 0 if thres is None else len(thres)
            dex_maps, q_maps = out[4:4 + n_dex], out[4 + n_dex:]
            refined_maps = width_maps = ()
            if args.dex_refine is not None:   # (never with quantiles: the maps behind the Dex maps are the refined ones, then the widths)
                refined_maps, width_maps, q_maps = out[4 + n_dex:4 + 2 * n_dex], out[4 + 2 * n_dex:], ()
            dex_layers = None
            if args.dex_layers is not None:   # (a render of its own, after the clock has stopped: the time per image is the depth render's)
                with torch.no_grad():
                    dex_layers = nerf.render_dex_layers(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                                        encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres,
                                                        layers=args.dex_layers, refine_steps=args.dex_refine,
                                                        want_width=args.dex_refine_width, occupancy=grid, **span_kw)
            frames.append((None, depth, dex_maps) + ((q_maps,) if quantiles else ()) + ((refined_maps, width_maps) if refined_maps else ())
                          + ((dex_layers,) if dex_layers is not None else ()))
            if args.savedir:   # the expected depth as a PNG, every map (depth + one Dex depth per threshold) as float32
                from PIL import Image
                d = depth.cpu().numpy()
                d = (255 * (d - d.min()) / max(d.max() - d.min(), 1e-8)).astype(np.uint8)
                Image.fromarray(d).save(os.path.join(args.savedir, f"depth_{i:04d}.png"))
                arrays = dict(depth=depth.cpu().numpy())
                if n_dex:
                    arrays.update(m_thres=np.asarray(thres, np.float32), dex=torch.stack(list(dex_maps)).cpu().numpy())
                if quantiles:
                    arrays.update(quantiles=np.asarray(quantiles, np.float32), qdepth=torch.stack(list(q_maps)).cpu().numpy())
                if refined_maps:
                    arrays.update(dex_refine_steps=np.int32(args.dex_refine), dex_refined=torch.stack(list(refined_maps)).cpu().numpy())
                if width_maps:
                    arrays.update(dex_width=torch.stack(list(width_maps)).cpu().numpy())
                if dex_layers is not None:
                    arrays.update(dex_events=dex_layers.events.cpu().numpy(), dex_event_count=dex_layers.count.cpu().numpy())
                    if dex_layers.width is not None:
                        arrays.update(dex_event_width=dex_layers.width.cpu().numpy())
                np.savez(os.path.join(args.savedir, f"dex_{i:04d}.npz"), **arrays)
            continue
        with torch.no_grad():
            ro, rd = nerf.get_ray_bundle(size, size, float(k_mat[0, 0]), pose, k_mat)
            out = nerf.run_one_iter_of_nerf(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres, occupancy=grid,
                                            cull_stats=grid is not None, **span_kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if span_grid is not None:
            report_spans(i, ro, rd)
        if grid is not None:
            *out, stats = out
            tally(stats)
            if args.occupancy_check:
                with torch.no_grad():
                    full = nerf.run_one_iter_of_nerf(size, size, float(k_mat[0, 0]), coarse, fine, ro, rd, cfg, mode="validation",
                                                     encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres)
                slot = 3 if fine is not None else 0
                rgb_diff.append(float((out[slot] - full[slot]).abs().max()))
                check.append([(float((a == b).float().mean()), float((a - b).abs().max())) for a, b in zip(out[6:], full[6:])])
        rgb = out[3] if fine is not None else out[0]
        if args.apply_exposure:      # training view i as its camera saw it
            rgb = nerf.apply_exposure(rgb, torch.as_tensor(ck["refined_exposure"])[i], ck["refined_exposure_mode"],
                                      float(ck["refined_exposure_scale"]))
        depth = out[4] if fine is not None else out[1]
        frames.append((rgb, depth))
        if args.savedir:
            from PIL import Image
            img = (rgb.clamp(0, 1) * 255).byte().cpu().numpy()
            Image.fromarray(img).save(os.path.join(args.savedir, f"{i:04d}.png"))
            d = depth.cpu().numpy()
            d = (255 * (d - d.min()) / max(d.max() - d.min(), 1e-8)).astype(np.uint8)
            Image.fromarray(d).save(os.path.join(args.savedir, f"depth_{i:04d}.png"))
    avg = float(np.mean(times[1:])) if len(times) > 1 else float(times[0])
    if not args.quiet:
        print(f"Avg time per image: {avg:.4f} s ({size}x{size}, {size * size / avg:.0f} rays/s, {args.precision})", flush=True)
    result = dict(avg_seconds=avg, frames=frames, times=times)
    if span_grid is not None:
        result.update(ray_span=span_grid, ray_spans=span_rows)
    if grid is not None:
        result.update(occupancy=grid, cull=cull)
        if not args.quiet:
            shares = [f"{100 * k / max(t, 1):.2f} % of {t}" for k, t in zip(cull["kept"], cull["total"])]
            print(f"occupancy: kept {shares[0]} coarse samples, {shares[1]} fine samples; {cull['nonfinite']} non-finite sigma", flush=True)
        if rgb_diff:
            result.update(occupancy_check=dict(max_rgb_diff=max(rgb_diff)))
            if not args.quiet:
                print(f"occupancy check rgb: max |rgb difference| {max(rgb_diff):.3e}", flush=True)
        if check and thres is not None:
            # per threshold over all views: the share of pixels with equal Dex depth, the largest depth difference
            equal = np.mean([[e for e, _ in view] for view in check], axis=0)
            worst = np.max([[d for _, d in view] for view in check], axis=0)
            result.setdefault("occupancy_check", {}).update(m_thres=[float(m) for m in thres], equal=equal.tolist(), max_diff=worst.tolist())
            if not args.quiet:
                for m, e, d in zip(thres, equal, worst):
                    print(f"occupancy check m_thres {int(m):3d}: {100 * e:.3f} % of the pixels equal, max |depth difference| {d:.5f}", flush=True)
    return result


if __name__ == "__main__":
    main()
