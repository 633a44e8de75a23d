"""Developer probe of the ray span (nerf.OccupancyGrid.ray_spans, ray_span= on the renders, include/dexnerf_hip_span.h): what the kernel
costs and what the tightening buys, on the GPU.

    python scripts/ray_span_measure.py kernel   [--out profiles/ray_span_kernel.json]
    python scripts/ray_span_measure.py accuracy [--out profiles/ray_span_accuracy.json]

kernel    the time of dn_occupancy_ray_spans (apply, no other output: the renders' call) for the 160,000 rays of a 400 x 400 view of the
          lego networks' box, against grids of 32^3, 64^3 and 128^3 cells built from the two lego networks (level 0, dilate 1); beside
          it the share of rays hit, the mean number of set cells a hit ray walks through and the mean span fraction.  HIP events,
          `--warmup` untimed launches, the median of `--iters`.
accuracy  the lego golden rays (tests/golden/render_lego_val, 4x128, near 2, far 6), fp32, thresholds 5, 20, 60, a 32^3 grid of the two
          networks (level 0, dilate 1, pad 1): the Dex error of the nc+nf render with and without tightened rows, for a ladder of sample
          counts from 64+128 down.  The truth is scripts/dex_refine_measure.py's: the first crossing among 2049 dense evaluations of
          the CPU oracle inside each first bracket; brackets whose dense samples cross more than once, or never, are left out and
          counted.  Beside each row: the time of nerf.render_dex_depth for a 400 x 400 view at that sample count, with and without
          ray_span=.  The plain render's A/B against the parent commit's build is scripts/dex_refine_measure.py's `plain` mode."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
T3 = (5.0, 20.0, 60.0)
LADDER = ((64, 128), (64, 64), (48, 48), (32, 64), (32, 32), (24, 24), (16, 32), (16, 16))


def lego(nerf, dev):
    from golden_cases import D4, lego_weights
    models = []
    for sd in lego_weights():
        m = nerf.models.FlexibleNeRFModel(**D4)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        models.append(m.to(dev))
    return models


def view_rays(nerf, dev, size=400):
    from nerf import synthetic as syn
    e_mat = torch.from_numpy(syn.scene_pose(3)).to(dev)
    k_mat = torch.from_numpy(syn.intrinsic(size, size)).to(dev)
    return nerf.get_ray_bundle(size, size, float(k_mat[0, 0]), e_mat, k_mat)


def kernel_mode(args, nerf):
    from dex_refine_measure import timed
    from nerf import _ops
    dev = torch.device("cuda:0")
    models = lego(nerf, dev)
    ex = nerf.get_embedding_function(10)
    ro, rd = view_rays(nerf, dev)
    rows0 = _ops.pack_ray_rows(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), None, 2.0, 6.0)
    out = []
    for cells in (32, 64, 128):
        with torch.no_grad():
            grid = nerf.OccupancyGrid.from_networks(models, ex, BOX, cells, level=0.0, dilate=1)
        span, visits = grid.ray_spans(rows0)
        hit = visits > 0
        rows = rows0.clone()

        def launch():
            rows.copy_(rows0)      # (the timed pair: a 5 MB copy and the kernel; the copy alone is timed beside it)
            _ops.tighten_ray_rows(rows, grid, 1.0)
        both = timed(launch, args.warmup, args.iters)
        copy = timed(lambda: rows.copy_(rows0), args.warmup, args.iters)
        row = dict(probe="ray_span_kernel", rays=int(rows0.shape[0]), cells=cells, occupied=grid.occupied_fraction(), kernel_and_copy_ms=both,
                   copy_ms=copy, kernel_ms=both - copy, hit_share=float(hit.float().mean()), mean_visits=float(visits[hit].float().mean()),
                   mean_span_fraction=float(((span[:, 1] - span[:, 0]) / 4.0)[hit].mean()))
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def accuracy_mode(args, nerf):
    from conftest import load_golden
    from dex_refine_measure import stats, timed
    from golden_cases import CASES, D4, lego_weights
    from nerf import _hip, _ops
    from oracle import nerf_oracle as oc
    dev = torch.device("cuda:0")
    models = lego(nerf, dev)
    ex = nerf.get_embedding_function(10)
    g, rkw = load_golden("render_lego_val"), CASES["render_lego_val"][2]
    rays = _ops.pack_ray_rows(torch.from_numpy(g["ro"]).to(dev), torch.from_numpy(g["rd"]).to(dev), None, rkw["near"], rkw["far"])
    with torch.no_grad():
        grid = nerf.OccupancyGrid.from_networks(models, ex, BOX, 32, level=0.0, dilate=1)
    tight = rays.clone()
    span, visits = grid.ray_spans(tight, apply=True)
    hit = visits > 0
    fraction = float(((span[:, 1] - span[:, 0]) / (rkw["far"] - rkw["near"]))[hit].mean())
    sd_f, mc = oc.to_torch_sd(lego_weights()[1]), oc.ModelCfg(**D4)
    packs = [m.packed_density(True, True, precision=_hip.PREC_F32) for m in models]
    m = np.asarray(T3, np.float32)
    th = torch.from_numpy(m).to(dev)

    def errors(rows, nc, nf):
        with torch.no_grad():
            z = _ops.coarse_depths(rows, nc, False)
            rf = _ops.run_network_rays(packs[0], rows, z)
            z = _ops.density_resample(rf, z, rows[:, 3:6], nf)[2]
            rf = _ops.run_network_rays(packs[1], rows, z)
            _, _, dex, br, _ = _ops.composite_density_brackets(rf, z, rows[:, 3:6], th)
        br0, dex, host = br.cpu().numpy(), dex.cpu().numpy().T, rows.cpu().numpy()
        pairs = np.argwhere((br0[..., 3] != -np.inf) & (br0[..., 1] > br0[..., 0]))
        r, k = pairs[:, 0], pairs[:, 1]
        lo, hi = br0[r, k, 0].astype(np.float64), br0[r, k, 1].astype(np.float64)
        zd = (lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, 2049)[None, :]).astype(np.float32)
        ro, rd = torch.from_numpy(host[r, 0:3].copy()), torch.from_numpy(host[r, 3:6].copy())
        with torch.no_grad():
            s = oc.run_network(sd_f, ro[:, None, :] + rd[:, None, :] * torch.from_numpy(zd)[..., None], rd, mc)[..., 3].numpy().astype(np.float64)
        above = s > m[k].astype(np.float64)[:, None]
        multi = (above[:, 1:] != above[:, :-1]).sum(-1) > 1
        j = above.argmax(-1)
        jm = np.maximum(j - 1, 0)
        i = np.arange(len(pairs))
        z0, z1, s0, s1 = zd[i, jm].astype(np.float64), zd[i, j].astype(np.float64), s[i, jm], s[i, j]
        with np.errstate(all="ignore"):
            z_true = np.where(j == 0, z0, z0 + (z1 - z0) * (m[k] - s0) / (s1 - s0))
        usable = above.any(-1) & ~multi
        return dict(stats(np.abs(dex[r, k] - z_true)[usable]), brackets=int(len(pairs)), crossing_more_than_once=int(multi.sum()),
                    never_crossing=int((~above.any(-1)).sum()))

    # the render's time at each sample count: a 400 x 400 view, one chunk
    ro, rd = view_rays(nerf, dev)

    def render_ms(nc, nf, **kw):
        mode = dict(chunksize=400 * 400, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False, radiance_field_noise_std=0.0, white_background=False)
        cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))

        def run():
            with torch.no_grad():
                nerf.render_dex_depth(400, 400, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                      m_thres_cand=list(T3), **kw)
        return timed(run, args.warmup, args.iters)
    out = []
    for nc, nf in LADDER:
        row = dict(probe="ray_span_accuracy", precision="fp32", samples=f"{nc}+{nf}", rays=int(rays.shape[0]), rays_hit=int(hit.sum()),
                   mean_span_fraction=fraction, plain=errors(rays, nc, nf), tightened=errors(tight, nc, nf),
                   plain_ms=render_ms(nc, nf), tightened_ms=render_ms(nc, nf, ray_span=grid))
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "accuracy"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import nerf
    assert torch.cuda.is_available(), "this probe measures on a GPU"
    nerf.set_precision("fp32")
    rows = kernel_mode(args, nerf) if args.mode == "kernel" else accuracy_mode(args, nerf)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
