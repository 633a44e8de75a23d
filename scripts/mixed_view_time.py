"""Developer timing probe for mixed-camera ray batches (a view index per ray).  Recorded, not gated.

    python scripts/mixed_view_time.py --all [--parent-lib PATH] --out profiles/mixed_view_time

runs every probe below as a process of its own under its own time limit (a probe that fails ends the run), collects their JSON
lines into <out>.json and writes the tables of <out>.md.  One probe by hand: --probe NAME.

    draw      dn_select_rays_draw_views against dn_select_rays_draw: 400 x 400 images, V = 20, 4096 rays, through ctypes alone, so
              that `--lib PATH` can point at another build of the library (--parent-lib: the parent commit's, which has only the latter)
    camgrad   dn_camera_grad_views at N = 4096, V in {1, 20, 100} against dn_camera_grad at N = 4096
    step      the fused training step of the 4 x 128 nets (L_xyz = 6, 64 + 64 samples, bf16) at 1024 rays, replayed as one HIP graph,
              with --draw-view view (one view per iteration) or rays (a view per ray); 20 views of 400 x 400
    train     train_dexnerf.py on the synthetic scene with its defaults and 2,000 iterations, with or without --mix-views: the
              held-out view's PSNR at every --validate-every and at the end

Kernel and step times: HIP events around one call, 5 untimed warm-ups, the median of 30."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True)
H = W = 400
WARMUP, ITERS = 5, 30


def event_ms(fn):
    """[median, min, max] milliseconds of fn() between two HIP events, after the warm-ups."""
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [statistics.median(ms), min(ms), max(ms)]


def scene_cams(n_views, dev):
    from nerf import _ops, synthetic as syn
    k = torch.from_numpy(syn.intrinsic(H, W))
    return torch.stack([_ops.camera_record(torch.from_numpy(syn.scene_pose(v, n_views=n_views)), k, None, H, W) for v in range(n_views)]).to(dev)


def probe_draw(args):
    from nerf import _hip
    path = args.lib or _hip.LIB_PATH
    lib = ctypes.CDLL(path)
    dev = torch.device("cuda:0")
    n_views, n = 20, 4096
    cams = scene_cams(n_views, dev)
    images = torch.rand(n_views, H, W, 3, device=dev)
    state = torch.tensor([5, 0, 0, 0], dtype=torch.int32, device=dev)
    rays, target = torch.empty(n, 11, device=dev), torch.empty(n, 3, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    f32, i64, i32, dbl = ctypes.c_float, ctypes.c_int64, ctypes.c_int, ctypes.c_double

    def draw():   # the view drawn in the kernel too (view = NULL), as the fused step calls it
        rc = lib.dn_select_rays_draw(i32(H), i32(W), p(cams), None, i32(n_views), f32(2.0), f32(6.0), p(state), i64(n), p(images), i32(3), p(rays),
                                     p(target), None, stream())
        assert rc == 0
    row = dict(probe="draw", label=args.label, views=n_views, rays=n, image=f"{H}x{W}", select_rays_draw_ms=event_ms(draw))
    if hasattr(lib, "dn_select_rays_draw_views"):
        def draw_views():
            rc = lib.dn_select_rays_draw_views(i32(H), i32(W), p(cams), i32(n_views), f32(2.0), f32(6.0), p(state), i64(n), p(images), i32(3),
                                               p(rays), p(target), None, None, dbl(0.0), dbl(1.0), stream())
            assert rc == 0
        row["select_rays_draw_views_ms"] = event_ms(draw_views)
    return [row]


def probe_camgrad(args):
    from nerf import _ops
    dev = torch.device("cuda:0")
    n = 4096
    torch.manual_seed(0)
    g = torch.randn(n, 11, device=dev)
    pix = torch.randint(0, H * W, (n,), device=dev)
    cams = scene_cams(100, dev)
    one = event_ms(lambda: _ops.camera_grad(H, W, cams[0].contiguous(), pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11]))
    rows = [dict(probe="camgrad", what="dn_camera_grad", rays=n, views=1, ms=one)]
    for v in (1, 20, 100):
        views = torch.randint(0, v, (n,), device=dev).to(torch.int32)
        sub = cams[:v].contiguous()
        ms = event_ms(lambda: _ops.camera_grad_views(H, W, sub, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11]))
        rows.append(dict(probe="camgrad", what="dn_camera_grad_views", rays=n, views=v, ms=ms))
    return rows   # (the wrappers allocate the scratch and the result inside the timed call, on both sides)


def probe_step(args):
    import nerf
    from nerf import parallel, synthetic as syn
    dev = torch.device("cuda:0")
    n_views, n = 20, 1024
    nerf.set_precision("bf16")
    models = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**NET)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **NET).items()})
        models.append(m.to(dev))
    mode = dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=True, radiance_field_noise_std=0.2, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    kmat = torch.from_numpy(syn.intrinsic(H, W))
    poses = [torch.from_numpy(syn.scene_pose(v, n_views=n_views)) for v in range(n_views)]
    sel = nerf.MultiViewRaySelector(H, W, poses, [kmat] * n_views, 2.0, 6.0, images=torch.rand(n_views, H, W, 3, device=dev), device=dev)
    bucket = parallel.FlatGradBucket(models)
    step = nerf.FusedTrainStep(models[0], models[1], sel, cfg, bucket, nerf.get_embedding_function(6), nerf.get_embedding_function(4), n, seed=7,
                               draw_view="rays" if args.draw_view == "rays" else True)
    graphed = nerf.GraphedTrainStep(step, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
    for _ in range(5):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
    return [dict(probe="step", draw_view=args.draw_view, nets="4x128 L_xyz=6, 64+64 samples, bf16", rays=n, views=n_views, image=f"{H}x{W}",
                 hip_graph=True, step_ms=event_ms(graphed.step))]


def probe_train(args):
    """train_dexnerf.py as a child process (its own defaults, 2,000 iterations); the [val] lines and the closing [done] line are parsed."""
    argv = [sys.executable, os.path.join(REPO, "dex-nerf_amd", "train_dexnerf.py"), "--iters", "2000", "--seed", str(args.seed)]
    argv += ["--mix-views"] if args.mix_views else []
    out = subprocess.run(argv, check=True, capture_output=True, text=True, timeout=args.timeout - 20).stdout
    val = [(int(i), float(p)) for i, p in re.findall(r"\[val\]\s+iter\s+(\d+) held-out view psnr ([-0-9.]+) dB", out)]
    done = re.search(r"\[done\] (\d+) iters in ([0-9.]+) s = (\d+) rays/s; held-out psnr ([-0-9.]+) dB", out)
    train = [(int(i), float(p)) for i, p in re.findall(r"\[train\] iter\s+(\d+) loss [0-9.]+ psnr ([-0-9.]+) dB", out)]
    return [dict(probe="train", mix_views=bool(args.mix_views), seed=args.seed, iters=2000, val_psnr_at=val, val_psnr_end=float(done.group(4)),
                 seconds=float(done.group(2)), rays_per_s=int(done.group(3)), train_psnr_last=train[-1][1] if train else None)]


PROBES = dict(draw=probe_draw, camgrad=probe_camgrad, step=probe_step, train=probe_train)


def run_all(args):
    """Every probe as a child process under its own time limit; the first failure ends the run."""
    me = os.path.abspath(__file__)
    jobs = [(["--probe", "draw", "--label", "this build"], 120)]
    if args.parent_lib:
        jobs.append((["--probe", "draw", "--label", "parent commit", "--lib", args.parent_lib], 120))
    jobs += [(["--probe", "camgrad"], 120), (["--probe", "step", "--draw-view", "view"], 180), (["--probe", "step", "--draw-view", "rays"], 180),
             ]
    for seed in (42, 43, 44):     # (42: the script's default seed)
        jobs += [(["--probe", "train", "--seed", str(seed), "--timeout", "300"], 300),
                 (["--probe", "train", "--seed", str(seed), "--mix-views", "--timeout", "300"], 300)]
    rows = []
    for extra, limit in jobs:
        done = subprocess.run([sys.executable, me] + extra, capture_output=True, text=True, timeout=limit)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"probe {extra} ended with status {done.returncode}: stopping")
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, iters=ITERS, rows=rows), fh, indent=1)
    with open(args.out + ".md", "w") as fh:
        fh.write(markdown(rows, torch.cuda.get_device_name(0)))


def markdown(rows, device):
    by = lambda name: [r for r in rows if r["probe"] == name]   # noqa: E731
    ms = lambda t: "-" if t is None else f"{t[0]:.4f} ({t[1]:.4f} - {t[2]:.4f})"   # noqa: E731
    out = ["# Mixed-camera ray batches: timings and a training comparison (scripts/mixed_view_time.py)", "",
           f"{device}.  Recorded, not gated.  `python scripts/mixed_view_time.py --all --parent-lib <the parent commit's library> --out "
           "profiles/mixed_view_time`: every probe is a process of its own under its own time limit.  Kernel and step times are HIP events "
           f"around ONE call, {WARMUP} untimed warm-ups, then {ITERS} timed calls: median (min - max) in milliseconds.  A single call of "
           "these kernels is a few microseconds of work behind a launch, so the figures are launch-bound latencies and differences inside "
           "the min - max spread mean nothing.  The raw rows are in `mixed_view_time.json`.", "",
           "## The draw kernel: 4096 rays out of 20 views of 400 x 400", "",
           "| build | `dn_select_rays_draw` (one view per iteration) | `dn_select_rays_draw_views` (a view per ray) |", "|---|---|---|"]
    for r in by("draw"):
        out.append(f"| {r['label']} | {ms(r['select_rays_draw_ms'])} | {ms(r.get('select_rays_draw_views_ms'))} |")
    out += ["", "## The camera gradient: N = 4096 rays of 400 x 400 cameras", "",
            "Wrapper calls (`_ops.camera_grad*`: the scratch and the result are allocated inside the timed call on both sides; two launches each).",
            "", "| entry point | views | ms |", "|---|---|---|"]
    for r in by("camgrad"):
        out.append(f"| `{r['what']}` | {r['views']} | {ms(r['ms'])} |")
    out += ["", "## The fused training step: 4 x 128 nets (L_xyz = 6), 64 + 64 samples, bf16, 1024 rays, one replayed HIP graph", "",
            "20 views of 400 x 400 on the device; `draw_view=True` gathers the targets from one image per step, `\"rays\"` from all of them.", "",
            "| `draw_view` | step ms |", "|---|---|"]
    for r in by("step"):
        shown = '"rays"' if r["draw_view"] == "rays" else "True"
        out.append(f"| `{shown}` | {ms(r['step_ms'])} |")
    train = by("train")
    iters = [i for i, _ in train[0]["val_psnr_at"]] if train else []
    out += ["", "## `train_dexnerf.py`, synthetic scene, defaults, 2,000 iterations", "",
            "The held-out view's PSNR in dB at every `--validate-every` and at the end (the last validation and the end are the same "
            "weights), one row per run; `--seed` changes the student's initialisation and the draws, the scene is the same.", "",
            "| run | seed | " + " | ".join(f"iter {i}" for i in iters) + " | end | rays/s | seconds |", "|---|---|" + "---|" * len(iters) + "---|---|---|"]
    for r in train:
        out.append(f"| {'`--mix-views`' if r['mix_views'] else 'default (one view per iteration)'} | {r['seed']} | "
                   + " | ".join(f"{p:.2f}" for _, p in r["val_psnr_at"]) + f" | {r['val_psnr_end']:.2f} | {r['rays_per_s']} | {r['seconds']:.1f} |")
    for mixed in (False, True):
        mine = [r for r in train if r["mix_views"] == mixed]
        if mine:
            cols = [statistics.mean(r["val_psnr_at"][k][1] for r in mine) for k in range(len(iters))] + [statistics.mean(r["val_psnr_end"] for r in mine)]
            out.append(f"| mean, {'`--mix-views`' if mixed else 'default'} | {len(mine)} runs | " + " | ".join(f"{c:.2f}" for c in cols) + " | | |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=sorted(PROBES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--lib", default="", help="draw: the library build to load")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--parent-lib", default="", help="--all: a build of the parent commit's library for the draw probe")
    ap.add_argument("--draw-view", choices=("view", "rays"), default="rays")
    ap.add_argument("--mix-views", action="store_true")
    ap.add_argument("--seed", type=int, default=42, help="train: the training script's --seed")
    ap.add_argument("--timeout", type=int, default=420, help="train: the time limit of the child training process, plus 20 s")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_view_time"))
    args = ap.parse_args()
    if args.all:
        return run_all(args)
    assert args.probe, "--probe NAME or --all"
    for row in PROBES[args.probe](args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
