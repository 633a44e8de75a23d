"""Developer timing probe of the density renders for profiles/density_render_refactor.md: one process, one tree, one JSON line.

  * nerf.render_dex_depth of the 400 x 400, 64 + 128, D8/W256 image (the shape of scripts/quantile_depth_time.py: bf16 mode, so the
    guarded fp16 render; K = 20 thresholds; the whole image in one chunk) without quantiles and with quantiles (0.1, 0.5, 0.9), and
    nerf.render_dex_normals of the same image - the three legs alternate inside each round, HIP events, median over `--rounds`;
  * the host enqueue time of one _ops.render_rays_depth call on a 4096-ray chunk (no synchronisation inside the timed loop), in the
    manner of scripts/host_overhead_probe.py: the Python on the per-chunk path.

    python scripts/density_render_time.py [--tree <a built checkout>] [--rounds 9]

--tree PATH imports the package (and bench.py's scene) of another checkout, built there.  Alternate the two trees process by process."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else REPO
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))
import bench  # noqa: E402
import nerf  # noqa: E402
from nerf import _ops, train_utils  # noqa: E402

THRES = [float(m) for m in range(5, 105, 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    assert os.path.abspath(nerf.__file__).startswith(TREE)
    dev = torch.device("cuda:0")
    nerf.set_precision("bf16")
    h = w = 400
    models, cfg, ro, rd, ex, ed = bench.build_scene(dev, 0, h=h, w=w, nc=64, nf=128)
    for m in models:
        m.requires_grad_(False)

    def depth(q=None):
        return lambda: nerf.render_dex_depth(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                             m_thres_cand=THRES, quantiles=q)
    legs = {"render_dex_depth_ms": depth(), "render_dex_depth_q3_ms": depth([0.1, 0.5, 0.9]),
            "render_dex_normals_ms": lambda: nerf.render_dex_normals(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation",
                                                                     encode_position_fn=ex, m_thres_cand=THRES)}
    ms = {name: [] for name in legs}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if r >= args.warmup:
                    ms[name].append(a.elapsed_time(b))
    row = dict(label=args.label, tree=TREE, **{name: statistics.median(v) for name, v in ms.items()})

    # host enqueue of the per-chunk wrapper: fp16 density packs (what the guarded render runs), 4096 rays, K = 20
    prec = _ops.render_precision()
    packs = (models[0].packed_density(True, True, precision=prec), models[1].packed_density(True, True, precision=prec))
    rays = _ops.pack_ray_rows(ro.reshape(-1, 3)[:4096].contiguous(), rd.reshape(-1, 3)[:4096].contiguous(), None, 2.0, 6.0)
    m_thres = train_utils._threshold_tensor(THRES, dev)

    def chunk():
        _ops.render_rays_depth(*packs, rays, 64, 128, False, 0.0, m_thres, None)
    for _ in range(20):
        chunk()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(40):
            chunk()
        per_call.append((time.perf_counter() - t0) / 40 * 1e6)
        torch.cuda.synchronize()
    row["render_rays_depth_host_enqueue_us"] = statistics.median(per_call)
    nerf.set_precision("fp32")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
