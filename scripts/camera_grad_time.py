"""Developer timing probe for the camera gradient: forward + backward of nerf.get_ray_bundle at 400 x 400 and of
nerf.select_camera_rays at 4096 rays with a pose and an intrinsic that require grad (the forward ray kernels + dn_camera_grad, the
record's two 3x3 / 4x4 inverses on the host, one 64-byte read-back), beside the same math written as a torch composition on the
device - what a user had to write before the library had a camera gradient (restated here, nothing imported from oracle/); and one
nerf.PoseRefiner.step at 2048 rays on the lego-shaped 4 x 128 networks.  Same process, same inputs, library route first.  Wall-clock
time between device synchronisations (the steps contain host work and one synchronising read-back), `--warmup` untimed iterations,
the median of `--iters`.  Recorded, not gated.  `--probe` picks one measurement, so that each runs as a process under its own timeout:

    for p in bundle rows refiner; do timeout -k 10 120 python scripts/camera_grad_time.py --probe $p || break; done

One JSON line per measurement, then a markdown table."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
import nerf  # noqa: E402
from nerf import synthetic as syn  # noqa: E402

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)


def timed(fn, warmup, iters):
    """Median wall-clock milliseconds of fn() between two device synchronisations.  Every step here contains host work (the record's
    two matrix inverses, the 64-byte read-back of the camera gradient, an optimizer step on the host), so device events would time
    an idle GPU: the wall clock is the quantity a refinement loop pays."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def torch_bundle(h, w, e, k):
    """get_ray_bundle (fork convention) as device torch ops: dir = [(i - cx) / fx, (j - cy) / fx, 1], rd = inv(E[:3,:3]) dir,
    ro = inv(E)[:3,3]."""
    jj, ii = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=e.device), torch.arange(w, dtype=torch.float32, device=e.device),
                            indexing="ij")
    d = torch.stack([(ii - k[0, 2]) / k[0, 0], (jj - k[1, 2]) / k[0, 0], torch.ones_like(ii)], -1)
    rd = (d[..., None, :] * torch.inverse(e[:3, :3])).sum(-1)
    return torch.inverse(e)[:3, -1].expand(rd.shape), rd


def torch_rows(h, w, e, k, near, far, pix):
    ro, rd = torch_bundle(h, w, e, k)
    ro, rd = ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix]
    ones = torch.ones_like(rd[:, :1])
    return torch.cat([ro, rd, near * ones, far * ones, rd / rd.norm(dim=-1, keepdim=True)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--probe", choices=("bundle", "rows", "refiner", "all"), default="all")
    args = ap.parse_args()
    assert args.warmup >= 3 and args.iters >= 10
    dev = torch.device("cuda:0")
    nerf.set_precision("fp32")
    h = w = 400
    e0, k0 = torch.from_numpy(syn.scene_pose(9)).to(dev), torch.from_numpy(syn.intrinsic(h, w)).to(dev)
    torch.manual_seed(0)
    g_ro, g_rd = torch.randn(h, w, 3, device=dev), torch.randn(h, w, 3, device=dev)
    pix = torch.randperm(h * w, device=dev)[:4096]
    g_rows = torch.randn(4096, 11, device=dev)
    rows = []

    def run(what, n_rays, lib_step, torch_step):
        lib_ms = timed(lib_step, args.warmup, args.iters)
        torch_ms = timed(torch_step, args.warmup, args.iters)
        ga, gb = lib_step(), torch_step()
        err = float((ga - gb).abs().max() / gb.abs().max())
        row = dict(probe="camera_grad_time", what=what, rays=n_rays, library_ms=lib_ms, torch_ms=torch_ms, ratio=torch_ms / lib_ms,
                   dE_library_vs_torch=err)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def bundle_step(fn):
        def step():
            e, k = e0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
            ro, rd = fn(e, k)
            ((ro * g_ro).sum() + (rd * g_rd).sum()).backward()
            return e.grad
        return step
    if args.probe in ("bundle", "all"):
        run("get_ray_bundle 400x400, forward + backward", h * w, bundle_step(lambda e, k: nerf.get_ray_bundle(h, w, 1.0, e, k)),
            bundle_step(lambda e, k: torch_bundle(h, w, e, k)))

    def rows_step(fn):
        def step():
            e, k = e0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
            (fn(e, k) * g_rows).sum().backward()
            return e.grad
        return step
    if args.probe in ("rows", "all"):
        run("select_camera_rays 4096 of 400x400, forward + backward", 4096,
            rows_step(lambda e, k: nerf.select_camera_rays(h, w, e, k, 2.0, 6.0, pix)[0]), rows_step(lambda e, k: torch_rows(h, w, e, k, 2.0, 6.0, pix)))

    if args.probe in ("refiner", "all"):
        models = []
        for seed in (43, 44):
            m = nerf.models.FlexibleNeRFModel(**NET)
            m.load_state_dict({n: torch.from_numpy(v) for n, v in syn.synth_state_dict(seed, sigma_bias=-20.0, **NET).items()})
            models.append(m.to(dev))
        mode = dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=False, radiance_field_noise_std=0.0, white_background=False)
        cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
        ref = nerf.PoseRefiner(models[0], models[1], cfg, h, w, k0, e0, nerf.get_embedding_function(10), nerf.get_embedding_function(4),
                               num_rays=2048, lr=1e-3, seed=0)
        image = torch.rand(h, w, 3, device=dev)
        step_ms = timed(lambda: ref.step(image), args.warmup, args.iters)
        row = dict(probe="pose_refiner_step", net="4x128 coarse + fine, 64 + 64 samples, fp32", rays=2048, step_ms=step_ms)
        rows.append(row)
        print(json.dumps(row), flush=True)

    print("\n| what | rays | library ms | torch composition ms | ratio | dE library vs torch |\n|---|---|---|---|---|---|")
    for r in rows:
        if r["probe"] == "camera_grad_time":
            print(f"| {r['what']} | {r['rays']} | {r['library_ms']:.3f} | {r['torch_ms']:.3f} | {r['ratio']:.1f} | {r['dE_library_vs_torch']:.1e} |")
    for r in rows:
        if r["probe"] == "pose_refiner_step":
            print(f"\n| PoseRefiner.step | rays | ms |\n|---|---|---|\n| {r['net']} | {r['rays']} | {r['step_ms']:.3f} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
