"""Developer timing probe for the ray gradient (dn_volume_render_backward_geom, dn_coarse_depths_backward, dn_fine_depths_backward).

    python scripts/ray_grad_time.py --parent-lib <parent commit's libdexnerf_hip.so> --parent-pkg <parent commit's dex-nerf_amd/> \
        [--out profiles/ray_grad_time.json]      (the markdown table goes beside it)

A/B against the parent commit in the same session on the same box: every measurement runs in a fresh child process that loads one
library (DEXNERF_HIP_LIB) - parent, this build, parent, this build, parent - so the parent's run-to-run spread is measured by
repeating it.  Per shape (4096 rays x 64 and x 192 samples):
  * the plain compositing backward (dn_volume_render_backward; g_rgb, g_depth, g_acc, g_weights given) of both libraries;
  * the geometry instance of this build, with the byte ratio it is expected to cost when HBM-bound: 40 B/sample (rf 16, z 4,
    g_weights 4, g_rf 16) -> 44 B/sample (+ g_z 4) + 12 B/ray (g_rd);
  * dn_coarse_depths_backward (Nc = 64) and dn_fine_depths_backward (64 + 128);
and one frozen-weights forward + backward of predict_and_render_radiance (4 x 128 nets, 4096 rays, 64 + 128 samples, fp32) with rows
that require grad, through the parent's package and through this one.  HIP events around batches of back-to-back launches, untimed
warm-up, the median of the batches."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

NOTES = """Every figure is the median of 15 batches of 20 back-to-back launches between HIP events (the render: 10 batches of 2
steps), after untimed warm-up, in a fresh process per library; parent and this build alternate (parent, this, parent, this, parent) so
the parent's own run-to-run spread sits beside the difference.  The working sets (10 MB at 64 samples, 31 MB at 192) are re-read by
every launch of a batch and stay resident in the last-level cache: these are not HBM-cold times, and a launch of a few microseconds is
partly launch cost, so the geometry / plain ratio is expected near the byte ratio (44 S + 12) / 40 S, not on it.  The plain instances
of this build are instruction for instruction the parent's (same disassembly, same VGPR / SGPR counts); no geometry instance uses
scratch, the 8- and 16-chunk ones included (142 and 256 VGPRs)."""

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 4096
SHAPES = (64, 192)


def timed(fn, warmup=5, batches=15, per_batch=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_batch):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / per_batch)
    return statistics.median(us)


def worker_kernels(tag):
    """Raw ctypes on the library DEXNERF_HIP_LIB names (the parent's lacks the new symbols: no binding module is involved)."""
    import torch
    lib = ctypes.CDLL(os.environ["DEXNERF_HIP_LIB"])
    dev = torch.device("cuda:0")
    vp = ctypes.c_void_p

    def p(t):
        return vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    plain_args = [vp, vp, vp, ctypes.c_int, vp, ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_int] + [vp] * 5
    lib.dn_volume_render_backward.argtypes = plain_args + [vp, vp]
    has_new = hasattr(lib, "dn_volume_render_backward_geom")
    if has_new:
        lib.dn_volume_render_backward_geom.argtypes = plain_args + [vp, vp, vp, vp]
        lib.dn_coarse_depths_backward.argtypes = [vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        lib.dn_fine_depths_backward.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp]
    torch.manual_seed(0)
    n = N_RAYS
    for s in SHAPES:
        rf = torch.randn(n, s, 4, device=dev)
        z = (2.0 + 4.0 * torch.rand(n, s, device=dev)).sort(-1).values.contiguous()
        rd = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1).contiguous()
        g_rgb, g_depth, g_acc, g_w = torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev), torch.randn(n, s, device=dev)
        g_rf, g_z, g_rd = torch.empty_like(rf), torch.empty_like(z), torch.empty_like(rd)
        head = (p(rf), p(z), p(rd), 3, None, 0.0, 0, n, s, p(g_rgb), p(g_depth), p(g_acc), None, p(g_w))

        def plain():
            assert lib.dn_volume_render_backward(*head, p(g_rf), stream) == 0
        print(json.dumps(dict(probe="composite_bwd_plain", lib=tag, rays=n, samples=s, us=timed(plain))), flush=True)
        if has_new:
            def geom():
                assert lib.dn_volume_render_backward_geom(*head, p(g_rf), p(g_z), p(g_rd), stream) == 0
            print(json.dumps(dict(probe="composite_bwd_geom", lib=tag, rays=n, samples=s, us=timed(geom), bytes_plain=40 * s,
                                  bytes_geom=44 * s + 12)), flush=True)
    if has_new:
        nc, nf = 64, 128
        rows = torch.randn(n, 11, device=dev)
        rows[:, 6], rows[:, 7] = 2.0, 6.0
        t_rand, g_zc = torch.rand(n, nc, device=dev), torch.randn(n, nc, device=dev)
        out2 = torch.empty(n, 2, device=dev)
        for jitter in (False, True):
            def coarse():
                assert lib.dn_coarse_depths_backward(p(rows), 11, n, nc, 0, p(t_rand) if jitter else None, p(g_zc), p(out2), stream) == 0
            print(json.dumps(dict(probe="coarse_depths_bwd", lib=tag, rays=n, num_coarse=nc, jitter=jitter, us=timed(coarse))), flush=True)
        zc = (2.0 + 4.0 * torch.rand(n, nc, device=dev)).sort(-1).values.contiguous()
        zs = 2.0 + 4.0 * torch.rand(n, nf, device=dev)
        g_zf, g_out = torch.randn(n, nc + nf, device=dev), torch.empty(n, nc, device=dev)
        for ordered in (True, False):
            zs_in = zs.sort(-1).values.contiguous() if ordered else zs

            def fine():
                assert lib.dn_fine_depths_backward(p(zc), p(zs_in), p(g_zf), n, nc, nf, p(g_out), stream) == 0
            print(json.dumps(dict(probe="fine_depths_bwd", lib=tag, rays=n, num_coarse=nc, num_fine=nf, samples_ascending=ordered,
                                  us=timed(fine))), flush=True)


def worker_render(tag, pkg):
    sys.path.insert(0, os.path.dirname(os.path.abspath(pkg)))
    sys.path.insert(0, os.path.abspath(pkg))
    import torch
    import nerf
    from nerf import synthetic as syn
    dev = torch.device("cuda:0")
    nerf.set_precision("fp32")
    kw = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    models = []
    for seed, bias in ((42, -20.0), (43, -5.0)):
        m = nerf.models.FlexibleNeRFModel(**kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **kw).items()})
        for q in m.parameters():
            q.requires_grad_(False)
        models.append(m.to(dev))
    mode = dict(chunksize=N_RAYS, lindisp=False, num_coarse=64, num_fine=128, perturb=False, radiance_field_noise_std=0.0,
                white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(10, True, True), nerf.get_embedding_function(4, True, True)
    torch.manual_seed(0)
    ro = torch.randn(N_RAYS, 3, device=dev) * 0.3
    rd = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, device=dev), dim=-1)
    rows0 = torch.cat([ro, rd, torch.full((N_RAYS, 1), 2.0, device=dev), torch.full((N_RAYS, 1), 6.0, device=dev), rd], -1)
    target = torch.rand(N_RAYS, 3, device=dev)

    def step():
        rows = rows0.clone().requires_grad_(True)
        out = nerf.predict_and_render_radiance(rows, models[0], models[1], cfg, mode="train", encode_position_fn=ex, encode_direction_fn=ed)
        (nerf.img2mse(out[0], target) + nerf.img2mse(out[3], target) + 0.05 * out[4].mean()).backward()
        return rows.grad
    us = timed(step, warmup=3, batches=10, per_batch=2)
    g = step()
    print(json.dumps(dict(probe="predict_and_render_radiance_fwd_bwd", lib=tag, rays=N_RAYS, samples="64+128", precision="fp32", weights="frozen",
                          us=us, near_far_gradient_nonzero=bool((g[:, 6:8] != 0).any()))), flush=True)


def child(mode, tag, lib, pkg):
    env = dict(os.environ, DEXNERF_HIP_LIB=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--tag", tag, "--pkg", pkg], env=env, check=True,
                         capture_output=True, text=True, timeout=300).stdout
    rows = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-pkg", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", default="", help="a JSON this script wrote: rebuild the tables from its recorded rows, measure nothing")
    ap.add_argument("--worker", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--pkg", default=os.path.join(REPO, "dex-nerf_amd"))
    args = ap.parse_args()
    if args.worker == "kernels":
        return worker_kernels(args.tag)
    if args.worker == "render":
        return worker_render(args.tag, args.pkg)
    if args.rows:
        recorded = json.load(open(args.rows))
        return report(recorded["rows"], recorded["device"], args.out)
    assert args.parent_lib and args.parent_pkg, "the A/B needs the parent commit's library and package"
    this_lib = os.path.join(REPO, "dex-nerf_amd", "lib", "libdexnerf_hip.so")
    this_pkg = os.path.join(REPO, "dex-nerf_amd")
    rows = []
    for tag, lib in (("parent#1", args.parent_lib), ("this#1", this_lib), ("parent#2", args.parent_lib), ("this#2", this_lib),
                     ("parent#3", args.parent_lib)):
        rows += child("kernels", tag, lib, this_pkg)
    for tag, lib, pkg in (("parent#1", args.parent_lib, args.parent_pkg), ("this#1", this_lib, this_pkg),
                          ("parent#2", args.parent_lib, args.parent_pkg), ("this#2", this_lib, this_pkg)):
        rows += child("render", tag, lib, pkg)
    import torch
    report(rows, torch.cuda.get_device_name(0), args.out)


def report(rows, device, out):
    def pick(probe, **kw):
        return [r for r in rows if r["probe"] == probe and all(r.get(k) == v for k, v in kw.items())]
    # the condition on the plain instance: not slower than the parent's slowest run by more than the parent's own run-to-run spread
    md = ["| rays x samples | plain, parent (3 runs) us | parent spread | plain, this build (2 runs) us | slower than the parent beyond its spread | "
          "geometry us | geometry / plain | byte ratio |", "|---|---|---|---|---|---|---|---|"]
    summary = []
    for s in SHAPES:
        par = [r["us"] for r in pick("composite_bwd_plain", samples=s) if r["lib"].startswith("parent")]
        new = [r["us"] for r in pick("composite_bwd_plain", samples=s) if r["lib"].startswith("this")]
        geo = [r["us"] for r in pick("composite_bwd_geom", samples=s)]
        spread = max(par) - min(par)
        slower = statistics.mean(new) > max(par) + spread
        ratio, byte_ratio = statistics.mean(geo) / statistics.mean(new), (44 * s + 12) / (40 * s)
        summary.append(dict(samples=s, parent_us=par, this_us=new, parent_spread_us=spread, plain_slower_than_parent_beyond_spread=slower, geom_us=geo,
                            geom_over_plain=ratio, byte_ratio=byte_ratio))
        md.append(f"| {N_RAYS} x {s} | {', '.join(f'{v:.2f}' for v in par)} | {spread:.2f} | {', '.join(f'{v:.2f}' for v in new)} | "
                  f"{'YES' if slower else 'no'} | {', '.join(f'{v:.2f}' for v in geo)} | {ratio:.2f} | {byte_ratio:.2f} |")
    md += ["", "| kernel | shape | us |", "|---|---|---|"]
    for r in pick("coarse_depths_bwd", lib="this#1"):
        md.append(f"| dn_coarse_depths_backward | {r['rays']} x {r['num_coarse']}, jitter {r['jitter']} | {r['us']:.1f} |")
    for r in pick("fine_depths_bwd", lib="this#1"):
        md.append(f"| dn_fine_depths_backward | {r['rays']} x ({r['num_coarse']} + {r['num_fine']}), samples ascending {r['samples_ascending']} | {r['us']:.1f} |")
    md += ["", "| predict_and_render_radiance fwd + bwd, rows require grad, frozen 4 x 128 nets, 4096 x (64 + 128), fp32 | us | near / far gradient |",
           "|---|---|---|"]
    for r in pick("predict_and_render_radiance_fwd_bwd"):
        md.append(f"| {r['lib']} | {r['us']:.0f} | {'non-zero' if r['near_far_gradient_nonzero'] else 'zero'} |")
    print("\n".join(md))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(dict(device=device, summary=summary, rows=rows), fh, indent=1)
        with open(os.path.splitext(out)[0] + ".md", "w") as fh:
            fh.write("# Ray gradient timing (scripts/ray_grad_time.py)\n\n" + f"Device: {device}.  " + NOTES + "\n\n" + "\n".join(md) + "\n")


if __name__ == "__main__":
    main()
