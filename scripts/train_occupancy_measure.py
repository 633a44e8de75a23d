"""Developer probe for training on the ray spans of a live occupancy grid (nerf.LiveOccupancyGrid, FusedTrainStep(ray_span=...)).
Recorded, not gated.

    python scripts/train_occupancy_measure.py --probe step --shape shipped|d8w256 --grid none|static|live [--tree PATH --label NAME]
    python scripts/train_occupancy_measure.py --probe refresh
    python scripts/train_occupancy_measure.py --probe quality [--iters N --seeds 0 1 2 --level L --grid-only]

    step      the fused training step replayed as one HIP graph (the set-up of scripts/distortion_time.py: draw_view="rays", bf16, 20
              views of 400 x 400): without a grid, with a fixed 64^3 grid (the one added launch) and with a live 64^3 grid refreshed
              every 16 steps (the refresh amortised into the step).  --tree PATH imports the package of another built checkout (the
              parent commit) instead of this one; it knows no ray_span, so --grid none there.
    refresh   LiveOccupancyGrid.update of both networks at 32^3 / 64^3 / 128^3, 4x128 and D8/W256, bf16: HIP events, the median of 20.
    quality   train_dexnerf.py on the synthetic scene with and without --train-occupancy, the same seeds, in three segments resumed
              from their checkpoints: held-out PSNR, the Dex depth error of the driver's sweep, the grid's occupied fraction and the
              mean span of the held-out view's rays at each segment's end.

One JSON line per measurement; profiles/train_occupancy.md holds the recorded tables."""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else REPO
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))

import torch  # noqa: E402

SHAPES = {
    "shipped": dict(net=dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True),
                    num_coarse=64, num_fine=64, rays=1024, what="4x128 L_xyz=6, 64+64 samples, 1024 rays"),
    "d8w256": dict(net=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
                   num_coarse=64, num_fine=128, rays=4096, what="D8/W256 L_xyz=10, 64+128 samples, 4096 rays"),
}
H = W = 400
VIEWS = 20
BOX = (-2.5, -2.5, -2.5, 2.5, 2.5, 2.5)
WARMUP, BLOCKS, BLOCK = 32, 5, 160          # (multiples of 16: every block holds the same number of refreshes)


def block_ms(fn):
    """Milliseconds per call of fn(): [median, min, max] over BLOCKS blocks of BLOCK calls between two HIP events, after the warm-ups."""
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BLOCK):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / BLOCK)
    return [statistics.median(ms), min(ms), max(ms)]


def models_of(net, dev):
    import nerf
    from nerf import synthetic as syn
    models = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**net)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **net).items()})
        models.append(m.to(dev))
    return models


def probe_step(args):
    import nerf
    from nerf import parallel, synthetic as syn
    dev = torch.device("cuda:0")
    shape = SHAPES[args.shape]
    net, n = shape["net"], shape["rays"]
    nerf.set_precision("bf16")
    models = models_of(net, dev)
    mode = dict(chunksize=4096, lindisp=False, num_coarse=shape["num_coarse"], num_fine=shape["num_fine"], perturb=True,
                radiance_field_noise_std=0.2, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    kmat = torch.from_numpy(syn.intrinsic(H, W))
    poses = [torch.from_numpy(syn.scene_pose(v, n_views=VIEWS)) for v in range(VIEWS)]
    gen = torch.Generator().manual_seed(1)
    sel = nerf.MultiViewRaySelector(H, W, poses, [kmat] * VIEWS, 2.0, 6.0, images=torch.rand(VIEWS, H, W, 3, generator=gen).to(dev), device=dev)
    ex = nerf.get_embedding_function(net["num_encoding_fn_xyz"])
    kw, grid = {}, None
    if args.grid == "static":
        with torch.no_grad():
            grid = nerf.OccupancyGrid.from_networks(models, ex, BOX, 64, level=0.0, dilate=1)
        kw = dict(ray_span=grid)
    elif args.grid == "live":
        grid = nerf.LiveOccupancyGrid(BOX, 64, dev, level=0.0, warmup_updates=1)
        kw = dict(ray_span=grid, occupancy_update_every=16)
    bucket = parallel.FlatGradBucket(models)
    step = nerf.FusedTrainStep(models[0], models[1], sel, cfg, bucket, ex, nerf.get_embedding_function(4), n, seed=7, draw_view="rays", **kw)
    graphed = nerf.GraphedTrainStep(step, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
    for _ in range(5):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
    ms = block_ms(graphed.step)
    assert bool(torch.isfinite(step.loss3).all())
    return [dict(probe="step", shape=args.shape, what=shape["what"], grid=args.grid, build=args.label, step_ms=ms, loss3=step.loss3.tolist(),
                 occupied=None if grid is None else grid.occupied_fraction())]


def probe_refresh(args):
    import nerf
    dev = torch.device("cuda:0")
    nerf.set_precision("bf16")
    rows = []
    for name in ("shipped", "d8w256"):
        net = SHAPES[name]["net"]
        models = models_of(net, dev)
        ex = nerf.get_embedding_function(net["num_encoding_fn_xyz"])
        for cells in (32, 64, 128):
            live = nerf.LiveOccupancyGrid(BOX, cells, dev, level=0.0, warmup_updates=0)
            for _ in range(5):
                live.update(models, ex)
            ms = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                live.update(models, ex)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rows.append(dict(probe="refresh", net=name, cells=cells, update_ms=[statistics.median(ms), min(ms), max(ms)],
                             per_step_at_16=statistics.median(ms) / 16, occupied=live.occupied_fraction()))
    return rows


def probe_quality(args):
    import nerf
    import train_dexnerf
    from nerf import _ops, synthetic as syn
    dev = torch.device("cuda:0")
    size, views = 64, 8
    base = ["--size", str(size), "--views", str(views), "--num-random-rays", "1024", "--layers", "4", "--width", "128", "--num-coarse", "32",
            "--num-fine", "32", "--validate-every", "0", "--quiet", "--precision", "bf16"]
    occ = ["--train-occupancy", "32", "--occupancy-bounds"] + [str(v) for v in BOX] + ["--occupancy-level", str(args.level)]
    kmat = torch.from_numpy(syn.intrinsic(size, size)).to(dev)
    ro, rd = nerf.get_ray_bundle(size, size, float(kmat[0, 0]), torch.from_numpy(syn.scene_pose(0, n_views=views)).to(dev), kmat)
    rows_plain = _ops.pack_ray_rows(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), None, 2.0, 6.0)
    marks = [args.iters // 4, args.iters // 2, args.iters]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for seed in args.seeds:
            for grid in ((True,) if args.grid_only else (False, True)):
                ck = os.path.join(tmp, f"s{seed}_{int(grid)}.ckpt")
                for k, iters in enumerate(marks):
                    argv = base + ["--seed", str(seed), "--iters", str(iters), "--save", ck] + (occ if grid else [])
                    res = train_dexnerf.main(argv + (["--load-checkpoint", ck] if k else []))
                    row = dict(probe="quality", seed=seed, grid=grid, level=args.level if grid else None, iters=iters, val_psnr=res["val_psnr"], dex_abs_err_mm=res.get("dex_abs_err_mm"),
                               dex_best_threshold=res.get("dex_best_threshold"), train_psnr=res["final_psnr"])
                    if grid:
                        live = res["train_occupancy"]
                        span, visits = live.grid.ray_spans(rows_plain.clone())
                        hit = visits > 0
                        row.update(occupied=res["occupied_fraction"], hit_share=float(hit.float().mean()),
                                   mean_span_fraction=float(((span[:, 1] - span[:, 0]) / 4.0)[hit].mean()) if bool(hit.any()) else None)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=("step", "refresh", "quality"), required=True)
    ap.add_argument("--tree", default="")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="d8w256")
    ap.add_argument("--grid", choices=("none", "static", "live"), default="none")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--level", type=float, default=0.01, help="quality: --occupancy-level of the runs with a grid")
    ap.add_argument("--grid-only", action="store_true", help="quality: skip the runs without a grid (measured before)")
    args = ap.parse_args()
    for row in dict(step=probe_step, refresh=probe_refresh, quality=probe_quality)[args.probe](args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
