"""Developer probe of the surface-normal render (nerf.render_dex_normals), two parts:

  * time: render_dex_normals beside render_dex_depth (the render it extends; that code is older than the normal render) per image, on
    400 x 400, 64 + 128 samples, D8/W256/skip 4 (the bench scene) and 270 x 480, 64 + 64 samples, the as-shipped 4 x 128 nets, in fp32
    and bf16 (render policy 'bf16': both legs in bf16), K = 20 thresholds, whole image in one chunk, the default 2 GiB workspace cap.
    HIP events, `--warmup` untimed renders, the median of `--iters`, both legs in one process.
  * bf16 against fp32 (the bf16 path has no reference of its own): the mean cosine of the per-point density gradients and the median
    angle between the Dex normals of the two modes where both have one, on the test suite's 4 x 128 (lego) and D8/W256 networks and
    golden rays.

    python scripts/normal_render_time.py [--out profiles/normal_render.json] [--skip-time]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dex-nerf_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import nerf  # noqa: E402
import bench  # noqa: E402
from nerf import _hip, _ops  # noqa: E402

D4 = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
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


def time_rows(dev, warmup, iters):
    rows = []
    nerf.set_render_policy("bf16")
    for net, h, w, nc, nf, kw in SHAPES:
        models, cfg, ro, rd, ex, ed = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=nf, model_kw=kw)
        for m in models:
            m.requires_grad_(False)
        for precision in ("fp32", "bf16"):
            nerf.set_precision(precision)

            def depth():
                with torch.no_grad():
                    return nerf.render_dex_depth(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                 encode_direction_fn=ed, m_thres_cand=THRES)

            def normals():
                with torch.no_grad():
                    return nerf.render_dex_normals(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                   encode_direction_fn=ed, m_thres_cand=THRES)
            prec = _hip.PREC_F32 if precision == "fp32" else _hip.PREC_BF16
            packs = (models[0].packed_density(precision=prec), models[1].packed_density(precision=prec))
            one = _ops.render_normals_workspace_bytes(*packs, 1024, nc, nf) / (1024 * (nc + nf))
            row = dict(probe="normal_render_time", net=net, image=f"{h}x{w}", samples=f"{nc}+{nf}", precision=precision,
                       depth_ms=timed(depth, warmup, iters), normals_ms=timed(normals, warmup, iters), workspace_bytes_per_fine_point=one)
            row["ratio"] = row["normals_ms"] / row["depth_ms"]
            row["ns_per_fine_point"] = 1e6 * (row["normals_ms"] - row["depth_ms"]) / (h * w * (nc + nf))
            rows.append(row)
            print(json.dumps(row), flush=True)
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")
    return rows


def accuracy_rows(dev):
    from golden_cases import CASES
    from conftest import load_golden
    rows = []
    for name, n, nc, nf, thres in (("render_lego_val", 256, 64, 64, (5.0, 15.0, 45.0)), ("render_d8w256_val", 256, 64, 128, (10.0, 50.0))):
        mkw, wfn, _ = CASES[name]
        g = load_golden(name)
        models = []
        for sd in wfn():
            m = nerf.models.FlexibleNeRFModel(**mkw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            models.append(m.to(dev).requires_grad_(False))
        n = min(n, g["ro"].shape[0])
        rays = _ops.pack_ray_rows(torch.from_numpy(np.ascontiguousarray(g["ro"][:n])).to(dev),
                                  torch.from_numpy(np.ascontiguousarray(g["rd"][:n])).to(dev), None, 2.0, 6.0)
        th = torch.tensor(thres, device=dev)
        out = {}
        with torch.no_grad():
            # the fine depths of the fp32 mode for both, so that the gradients are compared at the same points
            pc32 = models[0].packed_density(precision=_hip.PREC_F32)
            z_c = _ops.coarse_depths(rays, nc, False, None)
            _, _, z_f = _ops.density_resample(_ops.run_network_rays(pc32, rays, z_c), z_c, rays[:, 3:6], nf)
            for label, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16)):
                pf = models[1].packed_density(precision=prec)
                streams = models[1].packed_density_grad(precision=prec)
                sigma, grad = _ops.density_gradient(pf, streams, rays=rays, z=z_f)
                rf = torch.zeros(n, nc + nf, 4, device=dev)
                rf[..., 3] = sigma
                out[label] = (grad.double(), _ops.composite_normals(rf, z_f, rays[:, 3:6], grad, None, 0.0, th)[4].double())
        (g32, n32), (g16, n16) = out["fp32"], out["bf16"]
        cos = torch.nn.functional.cosine_similarity(g32.reshape(-1, 3), g16.reshape(-1, 3), dim=-1)
        both = (n32.abs().sum(-1) > 0) & (n16.abs().sum(-1) > 0)
        angle = torch.rad2deg(torch.acos((n32[both] * n16[both]).sum(-1).clamp(-1.0, 1.0)))
        row = dict(probe="bf16_vs_fp32", net=name, rays=n, samples=nc + nf, mean_gradient_cosine=float(cos.mean()),
                   median_gradient_cosine=float(cos.median()), dex_normal_pairs=int(both.sum()),
                   median_dex_normal_angle_deg=float(angle.median()) if int(both.sum()) else None,
                   dex_crossing_agreement=float(((n32.abs().sum(-1) > 0) == (n16.abs().sum(-1) > 0)).double().mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-time", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = accuracy_rows(dev)
    if not args.skip_time:
        rows += time_rows(dev, args.warmup, args.iters)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
