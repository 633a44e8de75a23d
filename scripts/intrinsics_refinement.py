"""Developer probe for intrinsics refinement on the fused pose step (nerf.FusedPoseStep(refine_intrinsics=...)): the replayed step time
beside the parent commit's, and one recovery run.  Recorded, not gated.  A sibling of scripts/pose_step_time.py, whose set-up it uses.

    git archive HEAD~1 dex-nerf_amd include | tar -x -C <dir> && make -C <dir>/dex-nerf_amd/csrc        # the parent commit, built
    python scripts/intrinsics_refinement.py --all --parent-tree <dir> --out profiles/intrinsics_refinement

runs every probe below as a process of its own under its own `timeout -k 10` (a probe that fails ends the run), collects their JSON
lines into <out>.json and writes <out>.md.  `--parity-log FILE`: the printed output of tests/test_intrinsics_refinement.py -s, whose
"fused vs host" lines are copied into the report.  One probe by hand: --probe NAME.

    step      the replayed step of pose_step_time.py's 20-view configuration (2048 rays, lego-shaped 4 x 128 nets, 64 + 64 samples,
              400 x 400 images, frozen weights): --mode off | shared | per_view, or --mode parent with --parent-tree: the same probe with
              the parent commit's package and library imported in place of this tree's (that process never imports this tree's nerf)
    recover   poses at the truth and held there or refined along, the trained lego-shaped pair, images rendered from the frozen nets
              with the true K, loss_weights=(0, 1); the step starts from a K0 whose focal length is 3 % high and whose principal point is
              4 px off in x and y, refine_intrinsics="shared": the intrinsics error every 50 steps

Step times as in pose_step_time.py: wall-clock between two device synchronisations around ONE step, 5 untimed warm-ups, median of 30
(min - max); every --mode is measured --repeats times, alternating, each in a fresh process."""
import argparse
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("parent", "off", "shared", "per_view")
FOCAL_FACTOR, SHIFT_PX = 1.03, 4.0


def import_tree(tree):
    """Put `tree`'s package (this repository's, or the parent commit's checkout) and this directory's pose_step_time on the path."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pose_step_time as pst       # (inserts this repository's paths ...)
    for p in (tree, os.path.join(tree, "dex-nerf_amd")):
        sys.path.insert(0, p)          # ... which the tree's own shadow
    return pst


def probe_step(args):
    tree = args.parent_tree if args.mode == "parent" else REPO
    assert tree, "--mode parent needs --parent-tree"
    pst = import_tree(tree)
    import torch
    import nerf
    assert os.path.abspath(nerf.__file__).startswith(os.path.abspath(tree) + os.sep), nerf.__file__
    from nerf import _hip
    dev, (mc, mf), cfg, k, e0, ex, ed = pst.setup(args.views, args.precision)
    images = torch.rand(args.views, pst.H, pst.W, 3, device=dev)
    kw = {} if args.mode in ("parent", "off") else dict(refine_intrinsics=args.mode)
    step = nerf.FusedPoseStep(mc, mf, cfg, pst.H, pst.W, k, e0, images, ex, ed, num_rays=pst.RAYS, lr=1e-3, seed=3, eager_iterations=3, **kw)
    for _ in range(5):
        step.step()
    torch.cuda.synchronize()
    assert step.graph is not None and step.fallback_reason is None, step.fallback_reason
    return [dict(probe="step", mode=args.mode, views=args.views, precision=args.precision, rays=pst.RAYS, library=os.path.relpath(_hip.LIB_PATH, tree),
                 step_ms=pst.wall_ms(step.step))]


def probe_recover(args):
    pst = import_tree(REPO)
    import torch
    import nerf
    from nerf import synthetic as syn
    h, w = pst.H, pst.W
    dev, (mc, mf), cfg, k_true, e_true, ex, ed = pst.setup(args.views, args.precision, weights="lego")
    focal = float(syn.intrinsic(h, w)[0, 0])
    images = []
    with torch.no_grad():
        for v in range(args.views):
            ro, rd = nerf.get_ray_bundle(h, w, focal, e_true[v], k_true)
            out = nerf.run_one_iter_of_nerf(h, w, focal, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex, encode_direction_fn=ed)
            images.append(out[3].reshape(h, w, 3))
    images = torch.stack(images)
    k0 = k_true.clone()
    k0[0, 0] *= FOCAL_FACTOR
    k0[0, 2] += SHIFT_PX
    k0[1, 2] += SHIFT_PX
    rows = []
    for refine_pose in (False, True):
        step = nerf.FusedPoseStep(mc, mf, cfg, h, w, k0, e_true, images, ex, ed, num_rays=pst.RAYS, lr=args.lr, seed=5, loss_weights=(0.0, 1.0),
                                  refine_intrinsics="shared", intrinsics_scale=args.scale, refine_pose=refine_pose)
        trace = []
        for it in range(args.steps + 1):
            if it % 50 == 0:
                est = step.intrinsics().double().cpu()
                rot, trans = pst.pose_errors(step.extrinsics(), e_true)
                trace.append(dict(step=it, loss3=None if step.loss3 is None else step.loss3.tolist(), phi=step.phi.tolist(),
                                  fx_err_percent=100.0 * (float(est[0, 0]) / float(k_true[0, 0]) - 1.0),
                                  cx_err_px=float(est[0, 2]) - float(k_true[0, 2]), cy_err_px=float(est[1, 2]) - float(k_true[1, 2]),
                                  rot_err_deg=rot, trans_err=trans))
            if it < args.steps:
                step.step()
        rows.append(dict(probe="recover", refine_pose=refine_pose, views=args.views, precision=args.precision, rays=pst.RAYS, lr=args.lr,
                         intrinsics_scale=args.scale, steps=args.steps, fx_true=float(k_true[0, 0]), hip_graph=step.graph is not None,
                         fallback_reason=step.fallback_reason, trace=trace))
    return rows


PROBES = dict(step=probe_step, recover=probe_recover)


def run_all(args):
    """Every probe as a child process under its own `timeout -k 10`; the first failure ends the run."""
    import torch
    me = os.path.abspath(__file__)
    modes = [m for m in MODES if m != "parent" or args.parent_tree]
    jobs = []
    for _ in range(args.repeats):
        for mode in modes:
            extra = ["--probe", "step", "--mode", mode, "--views", "20", "--precision", "fp32"]
            jobs.append((extra + (["--parent-tree", args.parent_tree] if mode == "parent" else []), 120))
    jobs.append((["--probe", "recover", "--views", "3", "--precision", "fp32", "--steps", str(args.steps), "--lr", str(args.lr),
                  "--scale", str(args.scale)], 420))
    rows = []
    for extra, limit in jobs:
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me] + extra, capture_output=True, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"probe {extra} ended with status {done.returncode}: stopping")
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    parity = []
    if args.parity_log and os.path.exists(args.parity_log):
        parity = [m.group(0).strip() for m in (re.search(r"fused vs host, \w+: .*", line) for line in open(args.parity_log)) if m]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    device = torch.cuda.get_device_name(0)
    with open(args.out + ".json", "w") as fh:
        json.dump(dict(device=device, rows=rows, parity=parity), fh, indent=1)
    with open(args.out + ".md", "w") as fh:
        fh.write(markdown(rows, device, parity))


def markdown(rows, device, parity):
    ms = lambda t: f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})"   # noqa: E731
    names = dict(parent="the parent commit's `FusedPoseStep` (its package and library)", off="`refine_intrinsics=None`",
                 shared='`refine_intrinsics="shared"`', per_view='`refine_intrinsics="per_view"`')
    n_rep = max([sum(1 for r in rows if r["probe"] == "step" and r["mode"] == m) for m in MODES] + [1])
    out = ["# Intrinsics refinement on the fused pose step (scripts/intrinsics_refinement.py)", "",
           f"{device}.  Recorded, not gated.", "", "## The replayed step", "",
           "The 20-view fp32 configuration of `pose_step_time.md`: 2048 rays, lego-shaped 4 x 128 nets (L_xyz = 10), 64 + 64 samples, 400 x 400 "
           "images, frozen weights, one replayed HIP graph.  Wall-clock milliseconds of ONE step between two device synchronisations, 5 untimed "
           "warm-ups, then 30 timed steps: median (min - max).  Every row is a process of its own; the rows of one repeat ran one after the "
           "other in the same run on the same machine, the parent's with the parent commit's package and library imported.  With "
           "`refine_intrinsics` set, `dn_camera_records` / `dn_camera_records_backward` stand in the places of `dn_pose_records` / "
           "`dn_pose_records_backward`, one launch each, so the launch count per step is the same in all four rows (a shared phi's gradient is "
           "summed inside the backward's launch, by one workgroup).", "",
           "| step | " + " | ".join(f"repeat {i + 1} ms" for i in range(n_rep)) + " |"]
    out.append("|---" * (out[-1].count("|") - 1) + "|")
    for mode in MODES:
        mine = [r for r in rows if r["probe"] == "step" and r["mode"] == mode]
        if mine:
            out.append(f"| {names[mode]} | " + " | ".join(ms(r["step_ms"]) for r in mine) + " |")
    for r in rows:
        if r["probe"] != "recover":
            continue
        what = "poses refined along, from the truth" if r["refine_pose"] else "poses held at the truth (`refine_pose=False`)"
        out += ["", f"## A recovery run, {what}", "",
                f"The trained lego-shaped pair, {r['views']} views, {r['precision']}, {r['rays']} rays per step, lr {r['lr']}, intrinsics_scale "
                f"{r['intrinsics_scale']}, {r['steps']} steps, `loss_weights=(0, 1)`, `refine_intrinsics=\"shared\"`.  Images rendered from the "
                f"frozen nets at the true poses with the true K (fx = {r['fx_true']:.3f}); the step is given a K0 with the focal length "
                f"{100 * (FOCAL_FACTOR - 1):.0f} % high and the principal point {SHIFT_PX:g} px off in x and in y, and renders with the same "
                f"settings (no jitter, no noise).  Errors of `intrinsics()` against the true K.  Replayed as a HIP graph: {r['hip_graph']} "
                f"(fallback: {r['fallback_reason']}).  Nothing was tuned for this run.", "",
                "| step | loss | mse_coarse | mse_fine | fx error (%) | cx error (px) | cy error (px) | rotation error (deg) | translation error |",
                "|---|---|---|---|---|---|---|---|---|"]
        for t in r["trace"]:
            loss = "- | - | -" if t["loss3"] is None else " | ".join(f"{x:.3e}" for x in t["loss3"])
            out.append(f"| {t['step']} | {loss} | {t['fx_err_percent']:+.4f} | {t['cx_err_px']:+.4f} | {t['cy_err_px']:+.4f} | "
                       f"{t['rot_err_deg']:.4f} | {t['trans_err']:.5f} |")
    if parity:
        out += ["", "## The fused step against the host reference", "",
                "`test_fused_step_against_the_host_reference` (tests/test_intrinsics_refinement.py): `FusedPoseStep` against `MultiPoseRefiner` "
                "on the same pairs; the gate for `last_grad_phi` is max(1e-5, 4 x the `last_grad` discrepancy of the same run), and a yardstick "
                "above 1e-3 is reported instead of gated on.  The two routes' rows differ in their last bits (4e-8: the host inverts in fp32, "
                "the device in fp64 rounded once); the fused launches alone, run on both sets of rows, reproduce the discrepancies below, "
                "nearly all of it in one or two of the 96 rays (the median ray's gradient is bit-identical).  On identical rows "
                "`test_one_step_is_the_chain_of_its_pieces` holds both gradients to 1e-5.", "", "```"]
        out += parity + ["```"]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=sorted(PROBES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--mode", choices=MODES, default="shared")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--parity-log", default=None)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--steps", type=int, default=500, help="recover: the number of steps")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--scale", type=float, default=1.0, help="recover: intrinsics_scale")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "intrinsics_refinement"))
    args = ap.parse_args()
    if args.all:
        return run_all(args)
    assert args.probe, "--probe NAME or --all"
    for row in PROBES[args.probe](args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
