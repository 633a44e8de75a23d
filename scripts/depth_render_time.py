"""Developer timing probe: the depth-only render (nerf.render_dex_depth) beside the full no-grad render (nerf.run_one_iter_of_nerf)
with the same K = 20 Dex thresholds, whole image in one chunk, on
  * 400 x 400, 64 + 128 samples, D8/W256/skip 4 (the bench step), and
  * 270 x 480, 64 + 64 samples, the as-shipped 4 x 128 nets,
under nerf.set_precision('bf16') with the render policy 'bf16' and with the default policy (guarded fp16).  HIP events, `--warmup`
untimed renders, the median of `--iters`, both legs in one process (full render first).  The full-render leg uses nothing this path
added, so the script also runs on a tree without render_dex_depth and then records that leg alone (`--label` names the tree).
A third block times the density sub-network's forward launch alone (dn_run_network on the coarse + fine point counts of the shape)
on the fixed-shape instances and, with DEXNERF_G48_RUNTIME_SHAPE=1, on the run-time-shape kernel.

    python scripts/depth_render_time.py [--label NAME] [--out profiles/depth_render_time.json] [--only-shape 0|1] [--profile-leg depth|full]

`--profile-leg` renders a few images of one leg and exits: the form to run under `rocprofv3 --kernel-trace --stats`."""
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

D4 = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
# multiply-accumulates per point, from the layer shapes: full network | trunk + fc_alpha
MACS = {"D8/W256": (593408, 491264), "4x128": (83840, 57344)}
SHAPES = [("D8/W256", 400, 400, 64, 128, None), ("4x128", 270, 480, 64, 64, D4)]
THRES = [float(m) for m in range(5, 105, 5)]


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default="")
    ap.add_argument("--only-shape", type=int, default=-1)
    ap.add_argument("--profile-leg", default="", choices=["", "depth", "full"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    have_depth = hasattr(nerf, "render_dex_depth")
    rows = []
    nerf.set_precision("bf16")
    for si, (net, h, w, nc, nf, kw) in enumerate(SHAPES):
        if args.only_shape >= 0 and si != args.only_shape:
            continue
        models, cfg, ro, rd, ex, ed = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=nf, model_kw=kw)

        def full():
            with torch.no_grad():
                return nerf.run_one_iter_of_nerf(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                 encode_direction_fn=ed, m_thres_cand=THRES)

        def depth():
            with torch.no_grad():
                return nerf.render_dex_depth(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                             encode_direction_fn=ed, m_thres_cand=THRES)
        if args.profile_leg:
            nerf.set_render_policy(None)
            for _ in range(5):
                (depth if args.profile_leg == "depth" else full)()
            torch.cuda.synchronize()
            continue
        for policy in ("bf16", None):
            nerf.set_render_policy(policy)
            row = dict(probe="depth_render_time", tree=args.label, net=net, image=f"{h}x{w}", samples=f"{nc}+{nf}",
                       policy=policy or "default (guarded fp16)", full_ms=timed(full, args.warmup, args.iters))
            if have_depth:
                row["depth_ms"] = timed(depth, args.warmup, args.iters)
                row["ratio"] = row["depth_ms"] / row["full_ms"]
                row["mac_ratio"] = MACS[net][1] / MACS[net][0]
                a, b = full(), depth()
                row["depth_fine_equal_bits"] = bool(torch.equal(a[4], b[2]))   # faster and different is not faster
            rows.append(row)
            print(json.dumps(row), flush=True)
        nerf.set_render_policy(None)
        if have_depth:
            # the density sub-network's forward launches alone: fixed-shape instances against the run-time-shape kernel
            from nerf import _ops
            rays = _ops.pack_ray_rows(ro.reshape(-1, 3), rd.reshape(-1, 3), None, 2.0, 6.0)
            n = rays.shape[0]
            z_c = _ops.coarse_depths(rays, nc, False)
            z_f = torch.sort(2.0 + 4.0 * torch.rand(n, nc + nf, device=dev), -1)[0].contiguous()
            for prec in ("bf16", "fp16"):
                nerf.set_precision(prec)
                pc, pf = models[0].packed_density(), models[1].packed_density()

                def nets():
                    with torch.no_grad():
                        _ops.run_network_rays(pc, rays, z_c)
                        _ops.run_network_rays(pf, rays, z_f)
                fixed_ms = timed(nets, args.warmup, args.iters)
                os.environ["DEXNERF_G48_RUNTIME_SHAPE"] = "1"
                try:
                    runtime_ms = timed(nets, args.warmup, args.iters)
                finally:
                    del os.environ["DEXNERF_G48_RUNTIME_SHAPE"]
                row = dict(probe="density_net_instances", tree=args.label, net=net, points=n * (2 * nc + nf), precision=prec,
                           fixed_ms=fixed_ms, runtime_shape_ms=runtime_ms, ratio=fixed_ms / runtime_ms)
                rows.append(row)
                print(json.dumps(row), flush=True)
            nerf.set_precision("bf16")
    nerf.set_precision("fp32")
    if args.profile_leg:
        return
    print("\n| tree | net | image | samples | policy | full ms | depth-only ms | ratio | MAC ratio |\n|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["probe"] == "depth_render_time":
            d = f"{r['depth_ms']:.3f} | {r['ratio']:.3f} | {r['mac_ratio']:.3f}" if "depth_ms" in r else "- | - | -"
            print(f"| {r['tree']} | {r['net']} | {r['image']} | {r['samples']} | {r['policy']} | {r['full_ms']:.3f} | {d} |")
    print("\n| net | points | precision | fixed instances ms | run-time shape ms | ratio |\n|---|---|---|---|---|---|")
    for r in rows:
        if r["probe"] == "density_net_instances":
            print(f"| {r['net']} | {r['points']} | {r['precision']} | {r['fixed_ms']:.3f} | {r['runtime_shape_ms']:.3f} | {r['ratio']:.3f} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
