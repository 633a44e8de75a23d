"""Developer probe for the general loss head (dn_render_loss: weighted colour terms + a masked depth term).  Recorded, not gated.

    python scripts/depth_supervision_time.py --all [--parent-tree PATH] --out profiles/depth_supervision

runs every probe below as a process of its own under its own `timeout -k 10` (a probe that fails ends the run; what was collected up
to there is still written), collects their JSON lines into <out>.json and writes the tables of <out>.md.  One probe by hand:
--probe NAME.

    step      the fused training step replayed as one HIP graph, draw_view="rays", bf16: --shape shipped (4 x 128 nets, L_xyz = 6,
              64 + 64 samples, 1024 rays) | d8w256 (D8/W256, L_xyz = 10, 64 + 128 samples, 4096 rays); --head default (dn_mse2_loss)
              | depth (dn_render_loss, depth maps of all views on the device, lambda = 0.1).  --tree PATH imports the package of
              another checkout (built there) instead of this one: --parent-tree hands --all the parent commit's, and the three
              variants of a shape are then run in turn, REPEATS times over, so that drift of the shared host shows as spread
    train     train_dexnerf.py on the synthetic scene, few views (--views 5), 1,000 iterations, --mix-views, --depth-weight LAMBDA:
              the held-out view's PSNR, expected-depth error and best-threshold Dex error
    refine    scripts/pose_step_time.py's refinement run (--weights lego | synthetic) with FusedPoseStep's loss_weights (1, 1) or
              (0, 1), optionally a depth term on depth maps rendered from the frozen nets

Step times: HIP events around BLOCK replays, 5 untimed warm-up replays, the median of 5 blocks (min - max), milliseconds per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(argv):
    """The checkout whose package this process imports (--tree PATH, default: this one) - decided before the first import."""
    return os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else REPO


TREE = _tree(sys.argv)
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

import torch  # noqa: E402

SHAPES = {
    "shipped": dict(net=dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True),
                    num_coarse=64, num_fine=64, rays=1024, what="4x128 L_xyz=6, 64+64 samples, 1024 rays"),
    "d8w256": dict(net=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
                   num_coarse=64, num_fine=128, rays=4096, what="D8/W256 L_xyz=10, 64+128 samples, 4096 rays"),
}
H = W = 400
VIEWS = 20
WARMUP, BLOCKS, BLOCK = 5, 5, 200
REPEATS = 3
LAMBDAS = (0.0, 0.01, 0.1)
SEEDS = (42, 43, 44)
TRAIN_ARGS = ["--iters", "1000", "--views", "5", "--mix-views", "--validate-every", "0", "--quiet"]


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


def probe_step(args):
    import nerf
    from nerf import parallel, synthetic as syn
    dev = torch.device("cuda:0")
    shape = SHAPES[args.shape]
    net, n = shape["net"], shape["rays"]
    nerf.set_precision("bf16")
    models = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**net)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **net).items()})
        models.append(m.to(dev))
    mode = dict(chunksize=4096, lindisp=False, num_coarse=shape["num_coarse"], num_fine=shape["num_fine"], perturb=True,
                radiance_field_noise_std=0.2, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    kmat = torch.from_numpy(syn.intrinsic(H, W))
    poses = [torch.from_numpy(syn.scene_pose(v, n_views=VIEWS)) for v in range(VIEWS)]
    gen = torch.Generator().manual_seed(1)
    sel = nerf.MultiViewRaySelector(H, W, poses, [kmat] * VIEWS, 2.0, 6.0, images=torch.rand(VIEWS, H, W, 3, generator=gen).to(dev), device=dev)
    head = {}
    if args.head == "depth":
        head = dict(depth_images=(2.0 + 4.5 * torch.rand(VIEWS, H, W, generator=gen)).to(dev), depth_weights=(0.1, 0.1), depth_range=(0.0, 6.0))
    bucket = parallel.FlatGradBucket(models)
    freqs = net["num_encoding_fn_xyz"]
    step = nerf.FusedTrainStep(models[0], models[1], sel, cfg, bucket, nerf.get_embedding_function(freqs), nerf.get_embedding_function(4), n, seed=7,
                               draw_view="rays", **head)
    graphed = nerf.GraphedTrainStep(step, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
    for _ in range(5):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
    ms = block_ms(graphed.step)
    assert bool(torch.isfinite(step.loss3).all())
    return [dict(probe="step", shape=args.shape, what=shape["what"], head=args.head, build=args.label, step_ms=ms,
                 loss=getattr(step, "loss6", None).tolist() if getattr(step, "loss6", None) is not None else step.loss3.tolist())]


def probe_train(args):
    import train_dexnerf
    argv = TRAIN_ARGS + ["--seed", str(args.seed)] + (["--depth-weight", str(args.depth_weight)] if args.depth_weight > 0 else [])
    res = train_dexnerf.main(argv)
    keep = ("final_loss", "val_psnr", "dex_best_threshold", "dex_abs_err_mm", "expected_depth_abs_err_mm", "steady_ms_per_iter", "hip_graphs",
            "s8_saturated_max")
    return [dict(probe="train", seed=args.seed, depth_weight=args.depth_weight, argv=argv, **{k: res.get(k) for k in keep})]


def probe_refine(args):
    """pose_step_time.py's refinement set-up (images of the frozen nets at the true poses, start poses off by its OFFSET twist), with
    the loss head's weights; depth maps for the depth term: the fine expected depth of the same renders."""
    import nerf
    import pose_step_time as pst
    from nerf import synthetic as syn
    dev, (mc, mf), cfg, k, e_true, ex, ed = pst.setup(3, "fp32", weights=args.weights)
    focal = float(syn.intrinsic(pst.H, pst.W)[0, 0])
    images, depths = [], []
    with torch.no_grad():
        for v in range(3):
            ro, rd = nerf.get_ray_bundle(pst.H, pst.W, focal, e_true[v], k)
            out = nerf.run_one_iter_of_nerf(pst.H, pst.W, focal, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex, encode_direction_fn=ed)
            images.append(out[3].reshape(pst.H, pst.W, 3))
            depths.append(out[4].reshape(pst.H, pst.W))
    images, depths = torch.stack(images), torch.stack(depths)
    offset = nerf.se3_exp(torch.tensor(pst.OFFSET, dtype=torch.float64)).to(dev, torch.float32)
    e_start = torch.stack([offset @ e_true[v] for v in range(3)])
    head = dict(loss_weights=tuple(args.loss_weights))
    if args.depth_weight > 0:
        head.update(depth_images=depths, depth_weights=(0.0, args.depth_weight), depth_range=(0.0, 6.0))
    step = nerf.FusedPoseStep(mc, mf, cfg, pst.H, pst.W, k, e_start, images, ex, ed, num_rays=pst.RAYS, lr=args.lr, seed=5, **head)
    trace = []
    for it in range(args.steps + 1):
        if it % 50 == 0:
            rot, trans = pst.pose_errors(step.extrinsics(), e_true)
            terms = step.loss6 if step.loss6 is not None else step.loss3
            trace.append(dict(step=it, terms=None if terms is None else terms.tolist(), rot_err_deg=rot, trans_err=trans))
        if it < args.steps:
            step.step()
    return [dict(probe="refine", weights=args.weights, loss_weights=list(args.loss_weights), depth_weight=args.depth_weight, rays=pst.RAYS, lr=args.lr,
                 steps=args.steps, hip_graph=step.graph is not None, fallback_reason=step.fallback_reason, trace=trace)]


PROBES = dict(step=probe_step, train=probe_train, refine=probe_refine)


def jobs_of(args):
    jobs = []
    for _ in range(REPEATS):
        for shape in SHAPES:
            if args.parent_tree:
                jobs.append((["--probe", "step", "--shape", shape, "--head", "default", "--label", "parent commit", "--tree", args.parent_tree], 180))
            jobs.append((["--probe", "step", "--shape", shape, "--head", "default", "--label", "this build"], 180))
            jobs.append((["--probe", "step", "--shape", shape, "--head", "depth", "--label", "this build"], 180))
    for seed in SEEDS:
        for lam in LAMBDAS:
            jobs.append((["--probe", "train", "--seed", str(seed), "--depth-weight", str(lam)], 240))
    for weights in ("lego", "synthetic"):
        for extra in (["--loss-weights", "1", "1"], ["--loss-weights", "0", "1"], ["--loss-weights", "0", "1", "--depth-weight", "0.1"]):
            jobs.append((["--probe", "refine", "--weights", weights, "--steps", str(args.steps)] + extra, 240))
    return jobs


def run_all(args):
    """Every probe as a child process under its own `timeout -k 10`; the first failure ends the run, after what there is was written."""
    me = os.path.abspath(__file__)
    rows, failed = [], None
    for extra, limit in jobs_of(args):
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me] + extra, capture_output=True, text=True)
        sys.stdout.write("".join(line + "\n" for line in done.stdout.splitlines() if line.startswith("{")))
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            failed = f"probe {extra} ended with status {done.returncode}: stopping"
            break
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"
    with open(args.out + ".json", "w") as fh:
        json.dump(dict(device=device, warmup=WARMUP, blocks=BLOCKS, block=BLOCK, repeats=REPEATS, rows=rows), fh, indent=1)
    with open(args.out + ".md", "w") as fh:
        fh.write(markdown(rows, device))
    if failed:
        raise SystemExit(failed)


def markdown(rows, device):
    by = lambda name: [r for r in rows if r["probe"] == name]   # noqa: E731
    out = ["# The loss head with a depth term: step time, depth error, fine-only refinement (scripts/depth_supervision_time.py)", "",
           f"{device}.  Recorded, not gated.  `python scripts/depth_supervision_time.py --all --parent-tree <a built checkout of the parent commit> "
           "--out profiles/depth_supervision`: every probe is a process of its own under its own `timeout -k 10`.  The raw rows are in "
           "`depth_supervision.json`.", "",
           "## (a) The replayed training step", "",
           f"`FusedTrainStep(draw_view=\"rays\")` + `FlatAdam` as one HIP graph, bf16, {VIEWS} views of {H} x {W} on the device.  HIP events "
           f"around {BLOCK} replays, {WARMUP} untimed warm-ups, {BLOCKS} blocks per process: ms per step, median (min - max) of the blocks.  The "
           f"variants of a shape run one after the other, {REPEATS} times over (one row per process, in run order), so the spread between rows of "
           "one variant is the run-to-run noise a difference between variants has to exceed.  The depth head replaces one one-workgroup "
           "launch (`dn_mse2_loss`) by another (`dn_render_loss`), asks the draw for its (view, pixel) pairs and hands the compositing "
           "backward two more (N) gradients.", ""]
    for shape, spec in SHAPES.items():
        mine = [r for r in by("step") if r["shape"] == shape]
        if not mine:
            continue
        out += [f"### {spec['what']}", "", "| build | loss head | ms per step, one row per process | median of the rows |", "|---|---|---|---|"]
        variants = []
        for r in mine:
            if (r["build"], r["head"]) not in variants:
                variants.append((r["build"], r["head"]))
        for build, head in variants:
            runs = [r["step_ms"] for r in mine if (r["build"], r["head"]) == (build, head)]
            shown = "; ".join(f"{m[0]:.4f} ({m[1]:.4f} - {m[2]:.4f})" for m in runs)
            name = "`dn_mse2_loss` (default arguments)" if head == "default" else "`dn_render_loss`, depth term, lambda = 0.1"
            out.append(f"| {build} | {name} | {shown} | {statistics.median(m[0] for m in runs):.4f} |")
        out.append("")
    train = by("train")
    if train:
        out += ["## (b) Depth error on the held-out view: `train_dexnerf.py " + " ".join(TRAIN_ARGS) + " --seed S [--depth-weight LAMBDA]`", "",
                "The synthetic teacher scene, 5 training views of 100 x 100, D8/W256 students, 2048 rays, bf16; the same seed gives the same "
                "student and the same draws for every lambda.  Errors in millimetres over the Dex validation mask (0 < gt < 6 m) of the "
                "held-out view: the fine pass's expected depth (what the depth term supervises) and the best-threshold Dex depth.", "",
                "| lambda | seed | held-out PSNR dB | expected-depth abs err mm | Dex abs err mm (best m) | steady ms / iteration |", "|---|---|---|---|---|---|"]
        for r in train:
            out.append(f"| {r['depth_weight']} | {r['seed']} | {r['val_psnr']:.2f} | {r['expected_depth_abs_err_mm']:.1f} | {r['dex_abs_err_mm']:.1f} "
                       f"({r['dex_best_threshold']}) | {r['steady_ms_per_iter']:.3f} |")
        for lam in sorted({r["depth_weight"] for r in train}):
            mine = [r for r in train if r["depth_weight"] == lam]
            mean = lambda key: statistics.mean(r[key] for r in mine)   # noqa: E731
            out.append(f"| {lam} | mean of {len(mine)} | {mean('val_psnr'):.2f} | {mean('expected_depth_abs_err_mm'):.1f} | {mean('dex_abs_err_mm'):.1f} | "
                       f"{mean('steady_ms_per_iter'):.3f} |")
        out.append("")
    for r in by("refine"):
        head = f"loss_weights = {tuple(r['loss_weights'])}" + (f", depth_weights = (0, {r['depth_weight']})" if r["depth_weight"] > 0 else "")
        out += [f"## (c) Refinement run, {r['weights']} nets, {head}", "",
                f"The set-up of `profiles/pose_step_time.md` (3 views, fp32, {r['rays']} rays per step, lr {r['lr']}, {r['steps']} steps, start poses "
                "off by the same twist, no jitter / noise); depth maps for the depth term: the fine expected depth of the frozen nets at the true "
                f"poses.  Replayed as a HIP graph: {r['hip_graph']} (fallback: {r['fallback_reason']}).", "",
                "| step | loss | mse_coarse | mse_fine | D_fine | rotation error (deg) | translation error |", "|---|---|---|---|---|---|---|"]
        for t in r["trace"]:
            terms = t["terms"]
            if terms is None:
                shown = "- | - | - | -"
            else:
                shown = " | ".join(f"{x:.3e}" for x in terms[:3]) + " | " + (f"{terms[4]:.3e}" if len(terms) > 3 else "-")
            out.append(f"| {t['step']} | {shown} | {t['rot_err_deg']:.4f} | {t['trans_err']:.5f} |")
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=sorted(PROBES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--tree", default="", help="step: import the package of this checkout (built there) instead of this script's")
    ap.add_argument("--parent-tree", default="", help="--all: a built checkout of the parent commit for the step probe")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="shipped")
    ap.add_argument("--head", choices=("default", "depth"), default="depth")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--depth-weight", type=float, default=0.0)
    ap.add_argument("--loss-weights", type=float, nargs=2, default=(1.0, 1.0))
    ap.add_argument("--weights", choices=("synthetic", "lego"), default="synthetic")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_supervision"))
    args = ap.parse_args()
    if args.all:
        return run_all(args)
    assert args.probe, "--probe NAME or --all"
    for row in PROBES[args.probe](args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
