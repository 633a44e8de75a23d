"""Developer probe of the refined Dex depth (nerf.render_dex_depth(refine_steps=R), include/dexnerf_hip_refine.h): what it costs and
what it buys, on the GPU.

    python scripts/dex_refine_measure.py time     [--out profiles/dex_refine_time.json]
    python scripts/dex_refine_measure.py plain    [--tree PATH] [--label NAME]        # the A/B leg: the plain depth render alone
    python scripts/dex_refine_measure.py accuracy [--out profiles/dex_refine_accuracy.json]

time      median time per image of render_dex_depth, whole image in one chunk, at 400 x 400 D8/W256 64+128 and at 270 x 480 4x128 64+64,
          under nerf.set_precision('bf16') with the render policy 'bf16' and with the default policy (guarded fp16), K in {1, 5}
          thresholds, plain and R in {0, 2, 4, 6, 8}; then the fewer-samples render - the fine network on the 64 uniform depths, no fine
          pass (the fine model handed over as model_coarse, num_fine = 0) - with R in {6, 8}.  HIP events, `--warmup`
          untimed renders, the median of `--iters`.  Beside each refined time: the model R K / (nc + nf) of the last pass's network
          time (measured in the same process on the same rays) and what is left over per launch of the 2 R + 1 added ones.
plain     the plain render's times alone, from this tree or - `--tree` - from another checkout's dex-nerf_amd package with its own
          library (the parent commit's build): alternate the two in one GPU call to see whether the plain path moved.
accuracy  the lego golden rays (tests/golden/render_lego_val, 4x128, near 2, far 6), thresholds 5, 20, 60, in fp32 and bf16: the
          error of the sample depth, of the linear interpolation (R = 0) and of R = 1 .. 8 against the first crossing among 2049
          dense evaluations of the CPU oracle inside each initial bracket; brackets whose dense samples cross more than once are
          left out and counted.  Then the 64+0 render with R in {6, 8} against the truth of the 64+64 render's brackets, tail included."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D4 = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
SHAPES = [("D8/W256", 400, 400, 64, 128, None), ("4x128", 270, 480, 64, 64, D4)]
THRES = {1: [20.0], 5: [5.0, 10.0, 20.0, 40.0, 60.0]}
STEPS = (0, 2, 4, 6, 8)
T3 = (5.0, 20.0, 60.0)


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


def render_fn(nerf, scene, h, w, thres, **kw):
    models, cfg, ro, rd, ex, ed = scene

    def run():
        with torch.no_grad():
            return nerf.render_dex_depth(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                         encode_direction_fn=ed, m_thres_cand=thres, **kw)
    return run


def time_mode(args, nerf, bench, plain_only):
    dev = torch.device("cuda:0")
    rows = []
    nerf.set_precision("bf16")
    for net, h, w, nc, nf, kw in SHAPES:
        scene = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=nf, model_kw=kw)
        for policy in ("bf16", None):
            nerf.set_render_policy(policy)
            for k, thres in THRES.items():
                row = dict(probe="dex_refine_time", tree=args.label, net=net, image=f"{h}x{w}", samples=f"{nc}+{nf}",
                           policy=policy or "default (guarded fp16)", K=k, plain_ms=timed(render_fn(nerf, scene, h, w, thres), args.warmup, args.iters))
                if not plain_only:
                    from nerf import _ops
                    # the last pass's network launch alone, in the precision the render runs it in: the model's yardstick
                    models, _, ro, rd, _, _ = scene
                    rays = _ops.pack_ray_rows(ro.reshape(-1, 3), rd.reshape(-1, 3), None, 2.0, 6.0)
                    z = torch.sort(2.0 + 4.0 * torch.rand(rays.shape[0], nc + nf, device=dev), -1)[0].contiguous()
                    pf = models[1].packed_density(precision=_ops.render_precision())

                    def last_pass():
                        with torch.no_grad():
                            _ops.run_network_rays(pf, rays, z)
                    row["last_pass_net_ms"] = timed(last_pass, args.warmup, args.iters)
                    for r in STEPS:
                        ms = timed(render_fn(nerf, scene, h, w, thres, refine_steps=r), args.warmup, args.iters)
                        model = row["last_pass_net_ms"] * r * k / (nc + nf)
                        row[f"R{r}_ms"] = ms
                        row[f"R{r}_added_ms"] = ms - row["plain_ms"]
                        row[f"R{r}_model_ms"] = model
                        row[f"R{r}_left_per_launch_us"] = 1000.0 * (ms - row["plain_ms"] - model) / (2 * r + 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
        if not plain_only:
            # the fewer-samples render: 64 uniform samples, no fine pass, then R bisections
            # (the FINE network on the uniform depths: with num_fine = 0 the render's one network is `model_coarse`)
            models, cfg, ro, rd, ex, ed = scene
            coarse_cfg = bench.build_scene(dev, 0, h=h, w=w, nc=nc, nf=0, model_kw=kw)[1]
            few = ((models[1], None), coarse_cfg, ro, rd, ex, ed)
            for policy in ("bf16", None):
                nerf.set_render_policy(policy)
                for k, thres in THRES.items():
                    row = dict(probe="dex_refine_fewer_samples", tree=args.label, net=net, image=f"{h}x{w}", policy=policy or "default (guarded fp16)",
                               K=k, full_plain_ms=timed(render_fn(nerf, scene, h, w, thres), args.warmup, args.iters),
                               coarse_only_plain_ms=timed(render_fn(nerf, few, h, w, thres), args.warmup, args.iters))
                    for r in (6, 8):
                        row[f"coarse_only_R{r}_ms"] = timed(render_fn(nerf, few, h, w, thres, refine_steps=r), args.warmup, args.iters)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        nerf.set_render_policy(None)
    nerf.set_precision("fp32")
    return rows


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------
def stats(err):
    err = np.asarray(err, np.float64)
    return dict(n=int(err.size), median=float(np.median(err)), p90=float(np.quantile(err, 0.9)), p99=float(np.quantile(err, 0.99)),
                max=float(err.max()))


def accuracy_mode(args, nerf):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from conftest import load_golden
    from golden_cases import CASES, lego_weights
    from nerf import _hip, _ops
    from oracle import nerf_oracle as oc
    dev = torch.device("cuda:0")
    name = "render_lego_val"
    g = load_golden(name)
    mkw, _, rkw = CASES[name]
    models = []
    for sd in lego_weights():
        m = nerf.models.FlexibleNeRFModel(**mkw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        models.append(m.to(dev))
    sd_f = oc.to_torch_sd(lego_weights()[1])
    mc = oc.ModelCfg(**mkw)
    ro, rd = torch.from_numpy(g["ro"]), torch.from_numpy(g["rd"])
    rays = _ops.pack_ray_rows(ro.to(dev), rd.to(dev), None, rkw["near"], rkw["far"])
    m = np.asarray(T3, np.float32)
    th = torch.from_numpy(m).to(dev)
    nc, nf, dense = rkw["num_coarse"], rkw["num_fine"], 2049

    def oracle_sigma(rows, z):
        pts = ro[rows][:, None, :] + rd[rows][:, None, :] * torch.from_numpy(np.ascontiguousarray(z, np.float32))[..., None]
        with torch.no_grad():
            return oc.run_network(sd_f, pts, rd[rows], mc)[..., 3].numpy().astype(np.float64)

    def truth_of(br0):
        """(pairs (P,2), z_true (P,), usable (P,), crossing more than once (P,)) of the proper initial brackets br0 (N,K,4)."""
        pairs = np.argwhere((br0[..., 3] != -np.inf) & (br0[..., 1] > br0[..., 0]))
        r, k = pairs[:, 0], pairs[:, 1]
        lo, hi = br0[r, k, 0].astype(np.float64), br0[r, k, 1].astype(np.float64)
        zd = (lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, dense)[None, :]).astype(np.float32)
        s = oracle_sigma(r, zd)
        above = s > m[k].astype(np.float64)[:, None]
        multi = (above[:, 1:] != above[:, :-1]).sum(-1) > 1
        j = above.argmax(-1)
        jm = np.maximum(j - 1, 0)
        rows = np.arange(len(pairs))
        z0, z1, s0, s1 = zd[rows, jm].astype(np.float64), zd[rows, j].astype(np.float64), s[rows, jm], s[rows, j]
        with np.errstate(all="ignore"):
            z_true = np.where(j == 0, z0, z0 + (z1 - z0) * (m[k] - s0) / (s1 - s0))
        return pairs, z_true, above.any(-1) & ~multi, multi

    def chain(packs, fine, steps_list):
        """{R: refined (N,K)}, the initial records (N,K,4) and the Dex depths (N,K) of the chain with `fine` fine samples."""
        pc, pf = packs
        with torch.no_grad():
            z = _ops.coarse_depths(rays, nc, False)
            rf = _ops.run_network_rays(pc, rays, z)
            last = pc
            if fine:
                z = _ops.density_resample(rf, z, rays[:, 3:6], fine)[2]
                rf = _ops.run_network_rays(pf, rays, z)
                last = pf
            _, _, dex, br, z_mid = _ops.composite_density_brackets(rf, z, rays[:, 3:6], th)
            br0 = br.cpu().numpy().copy()
            out = {0: _ops.dex_refine_finish(br, th)[0].cpu().numpy().T}
            for r in range(1, max(steps_list) + 1):
                z_mid = _ops.dex_bisect(br, _ops.run_network_rays(last, rays, z_mid), th)
                if r in steps_list:
                    out[r] = _ops.dex_refine_finish(br, th)[0].cpu().numpy().T
        return out, br0, dex.cpu().numpy().T

    rows = []
    truth_fp32 = None
    for precision, code in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16)):
        packs = tuple(mm.packed_density(precision=code) for mm in models)
        refined, br0, dex = chain(packs, nf, tuple(range(1, 9)))
        pairs, z_true, usable, multi = truth_of(br0)
        if precision == "fp32":
            truth_fp32 = {(int(r), int(k)): zt for (r, k), zt, ok in zip(pairs, z_true, usable) if ok}
        r, k = pairs[usable, 0], pairs[usable, 1]
        zt = z_true[usable]
        row = dict(probe="dex_refine_accuracy", precision=precision, samples=f"{nc}+{nf}", rays_crossing=int(len(set(pairs[:, 0].tolist()))),
                   brackets=int(len(pairs)), crossing_more_than_once=int(multi.sum()), left_out=int((~usable).sum()),
                   sample_depth=stats(np.abs(dex[r, k] - zt)), linear=stats(np.abs(refined[0][r, k] - zt)))
        for s in range(1, 9):
            row[f"R{s}"] = stats(np.abs(refined[s][r, k] - zt))
        rows.append(row)
        print(json.dumps(row), flush=True)
        # the fewer-samples render against the truth of the fp32 64+64 brackets: the first crossing the fine pass saw
        # (the FINE network on the 64 uniform depths: the same field, fewer samples)
        few, br_few, dex_few = chain((packs[1], packs[1]), 0, (6, 8))
        hit = [(rr, kk) for (rr, kk) in truth_fp32 if br_few[rr, kk, 3] != -np.inf]
        rr, kk = np.array([p[0] for p in hit]), np.array([p[1] for p in hit])
        zt = np.array([truth_fp32[p] for p in hit])
        row = dict(probe="dex_refine_fewer_samples_accuracy", precision=precision, samples=f"{nc}+0", truth="fp32 64+64 brackets",
                   pairs_with_truth=len(truth_fp32), of_them_crossing_here=len(hit), sample_depth=stats(np.abs(dex_few[rr, kk] - zt)))
        for s in (0, 6, 8):
            err = np.abs(few[s][rr, kk] - zt)
            row["linear" if s == 0 else f"R{s}"] = dict(stats(err), share_above_1e2=float((err > 1e-2).mean()), share_above_1e3=float((err > 1e-3).mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "plain", "accuracy"])
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
    if args.mode == "accuracy":
        rows = accuracy_mode(args, nerf)
    else:
        rows = time_mode(args, nerf, bench, plain_only=args.mode == "plain")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
