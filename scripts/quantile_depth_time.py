"""Developer timing probe of the opacity-quantile depth maps (profiles/quantile_depth.md).

  * nerf.render_dex_depth of the 400 x 400, 64 + 128, D8/W256 image (the bench scene), K = 20 Dex thresholds, whole image in one chunk:
    the call without quantiles (twice per round: its own run-to-run spread) and with Q = 3 and Q = 64 quantiles in both modes;
  * the compositing kernel alone, straight through the C ABI on preallocated buffers: dn_composite_density against
    dn_composite_density_quantiles on a 160,000 x 192 field.
One process, every leg warmed, the legs ALTERNATE inside each round, HIP events; median, minimum and maximum over `--rounds`.
Before timing, the maps every leg shares (depth, acc, Dex) are compared bit for bit with the call without quantiles.

    python scripts/quantile_depth_time.py [--rounds 15] [--out profiles/quantile_depth.json]"""
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
from nerf import _hip  # noqa: E402

THRES = [float(m) for m in range(5, 105, 5)]


def quantiles(n):
    return [0.1, 0.5, 0.9] if n == 3 else [0.01 + 0.989 * i / (n - 1) for i in range(n)]


def alternate(legs, warmup, rounds):
    """legs: name -> callable.  Every round runs every leg once, in order; returns name -> list of ms."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return ms


def summary(probe, ms, base):
    rows = []
    for name, v in ms.items():
        rows.append(dict(probe=probe, leg=name, median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                         vs_base=statistics.median(v) / statistics.median(ms[base])))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    nerf.set_precision("bf16")
    h = w = 400
    models, cfg, ro, rd, ex, ed = bench.build_scene(dev, 0, h=h, w=w, nc=64, nf=128)

    def render(q=None, interp=False):
        def fn():
            with torch.no_grad():
                return nerf.render_dex_depth(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                             m_thres_cand=THRES, quantiles=q, quantile_interp=interp)
        return fn
    legs = {"no quantiles (a)": render(), "Q=3 sample": render(quantiles(3)), "Q=3 linear": render(quantiles(3), True),
            "Q=64 sample": render(quantiles(64)), "Q=64 linear": render(quantiles(64), True), "no quantiles (b)": render()}
    base = legs["no quantiles (a)"]()
    for name, fn in legs.items():
        out = fn()
        assert all(torch.equal(a, b) for a, b in zip(base, out)), name       # faster and different is not faster
        qmaps = out[len(base):]
        assert all(bool((b >= a).all()) for a, b in zip(qmaps[:-1], qmaps[1:])), name
    rows = summary("render_dex_depth 400x400 64+128 D8/W256 bf16 mode (guarded fp16), K=20", alternate(legs, args.warmup, args.rounds),
                   "no quantiles (a)")

    # the kernel alone
    n, s = 160000, 192
    gen = torch.Generator(device=dev).manual_seed(3)
    rf = torch.randn(n, s, 4, device=dev, generator=gen)
    rf[..., 3] = 30.0 * rf[..., 3] - 40.0                                   # mostly empty space with a few dense samples per ray
    z = torch.sort(2.0 + 4.0 * torch.rand(n, s, device=dev, generator=gen), -1)[0].contiguous()
    rdir = torch.randn(n, 3, device=dev, generator=gen)
    th = torch.tensor(THRES, device=dev)
    depth, acc, dex = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(20, n, device=dev)
    lib, p, st = _hip.lib(), _hip.ptr, _hip.stream

    def plain():
        _hip.check(lib.dn_composite_density(p(rf), p(z), p(rdir), 3, None, 0.0, p(th), 20, n, s, p(depth), p(acc), p(dex), st()))
    klegs = {"dn_composite_density": plain}
    for nq in (3, 64):
        qt = torch.tensor(quantiles(nq), device=dev)
        qd = torch.empty(nq, n, device=dev)
        for interp in (0, 1):
            def fn(qt=qt, qd=qd, nq=nq, interp=interp):
                _hip.check(lib.dn_composite_density_quantiles(p(rf), p(z), p(rdir), 3, None, 0.0, p(th), 20, p(qt), nq, interp, n, s, p(depth),
                                                              p(acc), p(dex), p(qd), st()))
            klegs[f"quantiles Q={nq} {'linear' if interp else 'sample'}"] = fn
    klegs["dn_composite_density (b)"] = plain
    plain()
    ref = (depth.clone(), acc.clone(), dex.clone())
    for name, fn in klegs.items():
        fn()
        assert torch.equal(depth, ref[0]) and torch.equal(acc, ref[1]) and torch.equal(dex, ref[2]), name
    frac = float((acc >= 0.5).float().mean())
    print(json.dumps(dict(probe="kernel field", rays=n, samples=s, rays_with_acc_above_half=frac)), flush=True)
    rows += summary(f"compositing kernel alone, {n} x {s}, K=20", alternate(klegs, args.warmup, args.rounds), "dn_composite_density")
    nerf.set_precision("fp32")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
