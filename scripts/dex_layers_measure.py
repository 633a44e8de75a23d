"""Developer probe of the Dex depth layers (nerf.render_dex_layers, include/dexnerf_hip_layers.h): what they cost, on the GPU.

    python scripts/dex_layers_measure.py time  [--out profiles/dex_layers_time.json]
    python scripts/dex_layers_measure.py plain [--tree PATH] [--label NAME] [--out FILE]    # the A/B leg: the older renders alone

time    median time per image, whole image in one chunk, at 400 x 400 D8/W256 64+128 and at 270 x 480 4x128 64+64, under
        nerf.set_precision('bf16') with the default render policy (guarded fp16), K in {1, 5} thresholds: the plain render_dex_depth, the
        refined one (R = 6), and render_dex_layers with L in {1, 2, 4} in sample mode and with R = 6.  HIP events, `--warmup` untimed
        renders, the median of `--iters`.  Beside each time with R = 6: the model 2 L x the refined render's added time.
plain   the plain and the refined (R = 6) render_dex_depth alone, from this tree or - `--tree` - from another checkout's dex-nerf_amd
        package with its own library (the parent commit's build): alternate the two in one GPU call to see whether the older paths
        moved."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D4 = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
SHAPES = [("D8/W256", 400, 400, 64, 128, None), ("4x128", 270, 480, 64, 64, D4)]
THRES = {1: [20.0], 5: [5.0, 10.0, 20.0, 40.0, 60.0]}
LAYERS = (1, 2, 4)
STEPS = 6


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


def render_fn(render, scene, h, w, thres, **kw):
    models, cfg, ro, rd, ex, ed = scene

    def run():
        with torch.no_grad():
            return render(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex, encode_direction_fn=ed,
                          m_thres_cand=thres, **kw)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "plain"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tree", default=REPO, help="plain: the checkout whose dex-nerf_amd package (and library) is measured")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(tree, "dex-nerf_amd"))
    import nerf
    assert os.path.abspath(nerf.__file__).startswith(tree), nerf.__file__
    import bench
    assert torch.cuda.is_available(), "this probe measures on a GPU"
    dev = torch.device("cuda:0")
    nerf.set_precision("bf16")
    rows = []
    for net, h, w, nc, nf, kw in SHAPES:
        scene = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=nf, model_kw=kw)
        for k, thres in THRES.items():
            t = lambda render, **more: timed(render_fn(render, scene, h, w, thres, **more), args.warmup, args.iters)   # noqa: E731
            row = dict(probe="dex_layers_" + args.mode, tree=args.label, net=net, image=f"{h}x{w}", samples=f"{nc}+{nf}", K=k,
                       plain_ms=t(nerf.render_dex_depth), refined_R6_ms=t(nerf.render_dex_depth, refine_steps=STEPS))
            if args.mode == "time":
                added = row["refined_R6_ms"] - row["plain_ms"]
                for n_layers in LAYERS:
                    row[f"L{n_layers}_sample_ms"] = t(nerf.render_dex_layers, layers=n_layers)
                    row[f"L{n_layers}_R6_ms"] = t(nerf.render_dex_layers, layers=n_layers, refine_steps=STEPS)
                    row[f"L{n_layers}_sample_added_ms"] = row[f"L{n_layers}_sample_ms"] - row["plain_ms"]
                    row[f"L{n_layers}_R6_added_ms"] = row[f"L{n_layers}_R6_ms"] - row["plain_ms"]
                    row[f"L{n_layers}_R6_model_ms"] = 2 * n_layers * added
            rows.append(row)
            print(json.dumps(row), flush=True)
    nerf.set_precision("fp32")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
