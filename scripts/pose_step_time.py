"""Developer timing probe for the pose-refinement iteration: nerf.PoseRefiner.step (one camera) / nerf.MultiPoseRefiner.step (V cameras)
- float64 xi on the host, the render stage by stage under autograd, the camera gradient read back - against nerf.FusedPoseStep.step,
eager and replayed as one HIP graph.  Recorded, not gated.

    python scripts/pose_step_time.py --all --out profiles/pose_step_time

runs every probe below as a process of its own under its own `timeout -k 10` (a probe that fails ends the run), collects their JSON
lines into <out>.json and writes the tables of <out>.md.  One probe by hand: --probe NAME.

    step      one refinement step: --route refiner | fused-eager | fused-graph, --views 1 | 20, --precision fp32 | bf16; lego-shaped
              4 x 128 nets, 64 + 64 samples, 2048 rays, 400 x 400 images, frozen weights
    refine    a refinement run of FusedPoseStep (--weights lego | synthetic): images rendered from the frozen nets at known poses, start
              poses offset by a known twist, pose error and losses every 50 steps, and the losses of one step at the true poses

Step times: wall-clock between two device synchronisations around ONE step (the refiners' steps contain host work and a synchronising
read-back, so device events would time an idle GPU), 5 untimed warm-ups, the median of 30 (min - max)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
H = W = 400
RAYS = 2048
WARMUP, ITERS = 5, 30
OFFSET = (0.02, -0.015, 0.01, 0.04, -0.03, 0.02)    # refine: the twist the start poses are off by


def wall_ms(fn):
    """[median, min, max] wall-clock milliseconds of fn() between two device synchronisations, after the warm-ups."""
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(ms), min(ms), max(ms)]


def state_dicts(weights):
    """"synthetic": random 4 x 128 nets (nerf.synthetic); "lego": the trained lego-shaped pair of tests/golden/lego_weights.npz."""
    from nerf import synthetic as syn
    if weights == "lego":
        import numpy as np
        w = dict(np.load(os.path.join(REPO, "tests", "golden", "lego_weights.npz")))
        return [{k[3:]: v for k, v in w.items() if k.startswith(prefix)} for prefix in ("wc_", "wf_")]
    return [syn.synth_state_dict(seed, sigma_bias=-1.0, **NET) for seed in (21, 22)]


def render_cfg(perturb=False, noise_std=0.0):
    import nerf
    mode = dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=perturb, radiance_field_noise_std=noise_std,
                white_background=False)
    return nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def setup(n_views, precision, perturb=False, noise_std=0.0, weights="synthetic"):
    import nerf
    from nerf import synthetic as syn
    dev = torch.device("cuda:0")
    nerf.set_precision(precision)
    models = []
    for sd in state_dicts(weights):
        m = nerf.models.FlexibleNeRFModel(**NET)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.to(dev)
        for p in m.parameters():
            p.requires_grad_(False)
        models.append(m)
    cfg = render_cfg(perturb, noise_std)
    k = torch.from_numpy(syn.intrinsic(H, W)).to(dev)
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(v, n_views=max(n_views, 2))) for v in range(n_views)]).to(dev)
    return dev, models, cfg, k, e0, nerf.get_embedding_function(10), nerf.get_embedding_function(4)


def probe_step(args):
    import nerf
    dev, (mc, mf), cfg, k, e0, ex, ed = setup(args.views, args.precision)
    images = torch.rand(args.views, H, W, 3, device=dev)
    row = dict(probe="step", route=args.route, views=args.views, precision=args.precision, rays=RAYS, image=f"{H}x{W}",
               nets="4x128 L_xyz=10, 64+64 samples, frozen")
    if args.route == "refiner":
        if args.views == 1:
            ref = nerf.PoseRefiner(mc, mf, cfg, H, W, k, e0[0], ex, ed, num_rays=RAYS, lr=1e-3, seed=3)
            row["what"] = "PoseRefiner.step"
            row["step_ms"] = wall_ms(lambda: ref.step(images[0]))
        else:
            ref = nerf.MultiPoseRefiner(mc, mf, cfg, H, W, k, e0, ex, ed, num_rays=RAYS, lr=1e-3, seed=3)
            row["what"] = "MultiPoseRefiner.step"
            row["step_ms"] = wall_ms(lambda: ref.step(images))
        return [row]
    graph = args.route == "fused-graph"
    step = nerf.FusedPoseStep(mc, mf, cfg, H, W, k, e0, images, ex, ed, num_rays=RAYS, lr=1e-3, seed=3, use_graphs=graph, eager_iterations=3)
    for _ in range(5):
        step.step()
    torch.cuda.synchronize()
    assert (step.graph is not None) == graph and step.fallback_reason is None, step.fallback_reason
    row["what"] = "FusedPoseStep.step, " + ("one replayed HIP graph" if graph else "eager")
    row["step_ms"] = wall_ms(step.step)
    return [row]


def pose_errors(est, true):
    """(largest rotation angle in degrees, largest translation distance) between the estimated and the true world->camera extrinsics."""
    rel = est.double() @ torch.inverse(true.double())
    cos = ((rel[:, 0, 0] + rel[:, 1, 1] + rel[:, 2, 2] - 1.0) * 0.5).clamp(-1.0, 1.0)
    return float(torch.rad2deg(torch.acos(cos)).max()), float(rel[:, :3, 3].norm(dim=1).max())


def probe_refine(args):
    """Images of the frozen nets at the true poses (no jitter, no noise), start poses = exp(twist(OFFSET)) @ true; the refinement runs
    with the same settings."""
    import nerf
    from nerf import synthetic as syn
    dev, (mc, mf), cfg, k, e_true, ex, ed = setup(args.views, args.precision, weights=args.weights)
    focal = float(syn.intrinsic(H, W)[0, 0])
    images = []
    with torch.no_grad():
        for v in range(args.views):
            ro, rd = nerf.get_ray_bundle(H, W, focal, e_true[v], k)
            out = nerf.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex, encode_direction_fn=ed)
            images.append(out[3].reshape(H, W, 3))
    images = torch.stack(images)
    offset = nerf.se3_exp(torch.tensor(OFFSET, dtype=torch.float64)).to(dev, torch.float32)
    e_start = torch.stack([offset @ e_true[v] for v in range(args.views)])
    # (no jitter in the step either: against frozen nets it only adds noise to the loss, and at the true poses the fine render is then
    # the image itself - mse_fine there checks the set-up, mse_coarse is the constant gap between the two networks)
    at_truth = nerf.FusedPoseStep(mc, mf, cfg, H, W, k, e_true, images, ex, ed, num_rays=RAYS, lr=0.0, seed=5, use_graphs=False)
    loss_at_truth = at_truth.step().tolist()
    step = nerf.FusedPoseStep(mc, mf, cfg, H, W, k, e_start, images, ex, ed, num_rays=RAYS, lr=args.lr, seed=5)
    trace = []
    for it in range(args.steps + 1):
        if it % 50 == 0:
            rot, trans = pose_errors(step.extrinsics(), e_true)
            loss3 = None if step.loss3 is None else step.loss3.tolist()
            trace.append(dict(step=it, loss3=loss3, rot_err_deg=rot, trans_err=trans))
        if it < args.steps:
            step.step()
    return [dict(probe="refine", weights=args.weights, loss_at_true_poses=loss_at_truth, views=args.views, precision=args.precision, rays=RAYS, lr=args.lr, steps=args.steps, offset_twist=list(OFFSET),
                 hip_graph=step.graph is not None, fallback_reason=step.fallback_reason, trace=trace)]


PROBES = dict(step=probe_step, refine=probe_refine)


def run_all(args):
    """Every probe as a child process under its own `timeout -k 10`; the first failure ends the run."""
    me = os.path.abspath(__file__)
    jobs = []
    for precision in ("fp32", "bf16"):
        for views in (1, 20):
            for route in ("refiner", "fused-eager", "fused-graph"):
                jobs.append((["--probe", "step", "--route", route, "--views", str(views), "--precision", precision], 120))
    for weights in ("lego", "synthetic"):
        jobs.append((["--probe", "refine", "--views", "3", "--precision", "fp32", "--steps", str(args.steps), "--weights", weights], 240))
    rows = []
    for extra, limit in jobs:
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me] + extra, capture_output=True, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"probe {extra} ended with status {done.returncode}: stopping")
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    device = torch.cuda.get_device_name(0)
    with open(args.out + ".json", "w") as fh:
        json.dump(dict(device=device, warmup=WARMUP, iters=ITERS, rows=rows), fh, indent=1)
    with open(args.out + ".md", "w") as fh:
        fh.write(markdown(rows, device))


def markdown(rows, device):
    ms = lambda t: f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})"   # noqa: E731
    steps = [r for r in rows if r["probe"] == "step"]
    out = ["# The pose-refinement step: host route against the fused step (scripts/pose_step_time.py)", "",
           f"{device}.  Recorded, not gated.  `python scripts/pose_step_time.py --all --out profiles/pose_step_time`: every probe is a process of "
           f"its own under its own `timeout -k 10`.  Wall-clock milliseconds of ONE step between two device synchronisations, {WARMUP} untimed "
           f"warm-ups, then {ITERS} timed steps: median (min - max).  Lego-shaped 4 x 128 nets (L_xyz = 10), 64 + 64 samples, {RAYS} rays, "
           f"{H} x {W} images, frozen weights, no jitter / noise.  `PoseRefiner` / `MultiPoseRefiner` are unchanged code (the parent commit's), "
           "measured in the same run; `profiles/camera_grad_time.md` recorded 2.645 ms for `PoseRefiner.step` in an earlier session.  The raw "
           "rows are in `pose_step_time.json`.", "",
           "| precision | views | host route | ms | `FusedPoseStep` eager ms | `FusedPoseStep` replayed ms | host / replayed |", "|---|---|---|---|---|---|---|"]
    for precision in ("fp32", "bf16"):
        for views in (1, 20):
            mine = {r["route"]: r for r in steps if r["precision"] == precision and r["views"] == views}
            if len(mine) == 3:
                ref, eager, graph = mine["refiner"], mine["fused-eager"], mine["fused-graph"]
                out.append(f"| {precision} | {views} | `{ref['what']}` | {ms(ref['step_ms'])} | {ms(eager['step_ms'])} | {ms(graph['step_ms'])} | "
                           f"{ref['step_ms'][0] / graph['step_ms'][0]:.1f} |")
    for r in rows:
        if r["probe"] != "refine":
            continue
        out += ["", f"## A refinement run, {r['weights']} nets: {r['views']} views, {r['precision']}, {r['rays']} rays per step, lr {r['lr']}, {r['steps']} steps", "",
                "Images rendered from the frozen nets at the true poses (validation settings); start poses = exp(twist) @ true with twist "
                f"(omega, t) = {tuple(r['offset_twist'])}; the step renders with the same settings (no jitter, no noise).  Errors: the largest "
                "over the views of the rotation angle and of the translation distance of E_est E_true^-1.  [loss, mse_coarse, mse_fine] of one "
                "step AT the true poses: " + ", ".join(f"{x:.3e}" for x in r["loss_at_true_poses"]) + " (mse_coarse there is the gap between "
                "the coarse render and the fine image, a constant the refinement cannot remove).  Replayed as a HIP graph: "
                f"{r['hip_graph']} (fallback: {r['fallback_reason']}).", "",
                "| step | loss | mse_coarse | mse_fine | rotation error (deg) | translation error |", "|---|---|---|---|---|---|"]
        for t in r["trace"]:
            loss = "- | - | -" if t["loss3"] is None else " | ".join(f"{x:.3e}" for x in t["loss3"])
            out.append(f"| {t['step']} | {loss} | {t['rot_err_deg']:.4f} | {t['trans_err']:.5f} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=sorted(PROBES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--route", choices=("refiner", "fused-eager", "fused-graph"), default="fused-graph")
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--steps", type=int, default=300, help="refine: the number of steps")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weights", choices=("synthetic", "lego"), default="synthetic", help="refine: random nets or the trained lego-shaped pair")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_step_time"))
    args = ap.parse_args()
    if args.all:
        return run_all(args)
    assert args.probe, "--probe NAME or --all"
    for row in PROBES[args.probe](args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
