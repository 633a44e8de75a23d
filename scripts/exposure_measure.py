"""Developer measurements for the per-view exposure refinement (refine_exposure= on the fused steps): profiles/exposure_refinement.md.
Recorded, not gated.

    python scripts/exposure_measure.py --mode head --out profiles/x.json                      # this tree: both heads
    python scripts/exposure_measure.py --mode head --pkg <parent checkout>/dex-nerf_amd ...   # a built parent commit: dn_render_loss alone
    python scripts/exposure_measure.py --mode step [--pkg ...] --out ...
    python scripts/exposure_measure.py --mode recovery --out ...
    python scripts/exposure_measure.py --mode train --out ...

One process per package tree (two trees cannot share a process): parent and change are separate processes of one run.

--mode head: the loss head alone at 2048 and 4096 rays, V in {3, 20, 100} views, random maps, the depth term off: 50 calls captured into
one HIP graph, wall clock around 40 replays ending in a device synchronise, per call; 7 windows, median (min - max).  dn_render_loss (the
head the steps use without the refinement), dn_render_loss_exposure without g_eps (the head alone: one launch) and with it (the per-view
reduction as a second launch), "gain" and "affine" rows of |s a| <= 0.5.  --tail-lib: a library that exports the same entry point with
the reduction as a tail of the head's workgroup, timed the same way.

--mode step: FusedJointStep replayed as one HIP graph under 'bf16' on lego-shaped 4 x 128 nets, 64 + 64 samples, 2048 rays, 3 views of
400 x 400 (profiles/joint_training.md's probe): windows of 200 replayed steps, 20 untimed first, 7 windows; without the refinement, and
(this tree) with "gain" and "affine".  Launches: the device kernels, memsets and copies torch.profiler sees in one eager step.

--mode recovery: tests/test_exposure_refinement.py's recovery protocol over step counts, learning rates and seeds.

--mode train: 3 views of 24 x 20, targets = the lego networks' renders at the true poses (64 + 64 samples) with a per-view gain (1, 1.25,
0.8); the 4 x 128 networks start from the lego weights and train for 600 steps (200 rays, 16 + 24 samples, jitter, fp32, lr 5e-4) with
every pose held - without the refinement and with refine_exposure="gain", exposure_fixed_views=(0,).  Then, over all pixels of the three
views at validation settings: the fine PSNR against the UN-gained renders (the canonical exposure) and the mean |Dex depth - teacher's
Dex depth| at the density threshold 15."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dex-nerf_amd"),
                help="the built package tree to import")
ap.add_argument("--mode", required=True, choices=["head", "step", "recovery", "train"])
ap.add_argument("--tail-lib", default="")
ap.add_argument("--out", required=True)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch  # noqa: E402

import nerf  # noqa: E402
from nerf import _hip, _ops, parallel, synthetic as syn  # noqa: E402

dev = torch.device("cuda:0")
HAVE = hasattr(_ops, "render_loss_exposure")


def summary(w):
    return dict(windows=w, median=statistics.median(w), min=min(w), max=max(w))


def time_graph(fn, calls=50, replays=40, windows=7):
    """Microseconds per call of `fn` (library launches only), replayed from one HIP graph of `calls` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(calls)]
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(replays):
            g.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / (replays * calls))
    del keep
    return out


def mode_head():
    results = {}
    tail = None
    if args.tail_lib:
        tail = ctypes.CDLL(os.path.abspath(args.tail_lib))
        tail.dn_render_loss_exposure.argtypes = _hip.lib().dn_render_loss_exposure.argtypes
    for n in (2048, 4096):
        gen = torch.Generator().manual_seed(n)
        rgb_c, rgb_f, target = (torch.rand(n, 3, generator=gen).to(dev) for _ in range(3))
        results[f"render_loss n={n}"] = summary(time_graph(lambda: _ops.render_loss(rgb_c, rgb_f, target)))
        print(args.tag, f"render_loss n={n}", results[f"render_loss n={n}"]["median"], flush=True)
        if not HAVE:
            continue
        for v in (3, 20, 100):
            views = torch.randint(0, v, (n,), generator=gen, dtype=torch.int32).to(dev)
            for p in (1, 6):
                eps = ((2.0 * torch.rand(v, p, generator=gen) - 1.0) * 0.5).to(dev)
                g_eps = torch.empty(v, p, device=dev)
                probes = {"head alone": lambda: _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, 1.0, views, want_eps=False),
                          "head + second launch": lambda: _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, 1.0, views, g_eps=g_eps)}
                if tail is not None:
                    loss6, g_c, g_f = torch.empty(6, device=dev), torch.empty_like(rgb_c), torch.empty_like(rgb_f)
                    g_tail = torch.empty(v, p, device=dev)
                    pt = _hip.ptr

                    def tail_call():
                        rc = tail.dn_render_loss_exposure(pt(rgb_c), pt(rgb_f), pt(target), None, None, None, None, pt(views), None, 0, n, 0, 1.0, 1.0,
                                                          0.0, 0.0, 0.0, 1.0, pt(eps), p, v, 1.0, None, pt(loss6), pt(g_c), pt(g_f), None, None,
                                                          pt(g_tail), None, _hip.stream())
                        assert rc == 0, rc
                    probes["head with tail"] = tail_call
                for name, fn in probes.items():
                    key = f"{name} n={n} V={v} P={p}"
                    results[key] = summary(time_graph(fn))
                    print(args.tag, key, f"{results[key]['median']:.2f} us", flush=True)
                if tail is not None:      # the two forms agree (the orders of their sums differ: fp64 sums rounded once)
                    _ops.render_loss_exposure(rgb_c, rgb_f, target, eps, 1.0, views, g_eps=g_eps)
                    tail_call()
                    torch.cuda.synchronize()
                    results[f"tail vs second launch n={n} V={v} P={p}"] = float((g_tail - g_eps).abs().max() / g_eps.abs().max())
    return results


def launches(eager):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eager()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer.step")]
    return len(names), sorted(set(names))


def time_probe(step_fn, windows=7, per=200, warm=20):
    for _ in range(warm):
        step_fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(per):
            step_fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / per)
    return out


def mode_step():
    nerf.set_precision("bf16")
    size, v, rays = 400, 3, 2048
    images = torch.rand(v, size, size, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in (3, 9, 14)]).to(dev)
    kmat = torch.from_numpy(syn.intrinsic(size, size)).to(dev)
    mode = dict(chunksize=65536, lindisp=False, num_coarse=64, num_fine=64, perturb=True, radiance_field_noise_std=0.2, white_background=True)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    kw = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    variants = [None] + (["gain", "affine"] if HAVE else [])
    steps = {}
    for mode_name in variants:
        torch.manual_seed(5)
        nets = [nerf.models.FlexibleNeRFModel(**kw).to(dev) for _ in range(2)]
        bucket = parallel.FlatGradBucket(nets)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        extra = dict(refine_exposure=mode_name, exposure_fixed_views=(0,)) if mode_name else {}
        steps[mode_name] = nerf.FusedJointStep(nets[0], nets[1], cfg, size, size, kmat, e0, images, ex, ed, rays, bucket, opt, 1e-3, seed=1,
                                               fixed_views=(0,), **extra)
    for s in steps.values():
        for _ in range(20):
            s.step()
    torch.cuda.synchronize()
    windows = {m: [] for m in steps}
    for _ in range(7):                                   # the probes alternated window by window
        for m, s in steps.items():
            windows[m] += time_probe(s.step, windows=1, warm=0)
    results = {}
    for m, s in steps.items():
        assert s.graph is not None and s.fallback_reason is None, s.fallback_reason
        count, names = launches(s._enqueue)
        results[f"joint bf16 refine_exposure={m}"] = dict(summary(windows[m]), launches=count, kernels=names, loss=s.loss3.tolist())
        print(args.tag, f"joint bf16 refine_exposure={m}", f"{statistics.median(windows[m]):.4f} ms", count, flush=True)
    return results


def teacher_images(nets, e0, k, h, w, ex, ed, nc=64, nf=64, thres=None):
    mode = dict(chunksize=4096, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False, radiance_field_noise_std=0.0, white_background=True)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    rgb, dex = [], []
    for v in range(e0.shape[0]):
        ro, rd = nerf.get_ray_bundle(h, w, float(k[0, 0]), e0[v], k)
        with torch.no_grad():
            out = nerf.run_one_iter_of_nerf(h, w, float(k[0, 0]), nets[0], nets[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                            encode_direction_fn=ed, m_thres_cand=thres)
        rgb.append(out[3].reshape(h, w, 3).clone())
        if thres is not None:
            dex.append(out[6].reshape(h, w).clone())
    return torch.stack(rgb), (torch.stack(dex) if dex else None)


def mode_recovery():
    from test_exposure_refinement import GAINS, OFFSETS
    from test_input_gradients import make_cfg
    from test_joint_pose_training import H, N_RAYS, RENDER, V, W, cameras, encoders, make_nets
    nerf.set_precision("fp32")
    e0, k = (t.to(dev) for t in cameras())
    ex, ed = encoders()
    nets = make_nets(dev)
    for m in nets:
        for q in m.parameters():
            q.requires_grad_(False)
    options = make_cfg(dict(RENDER, perturb=False, noise_std=0.0))
    gains, offsets = torch.tensor(GAINS, device=dev), torch.tensor(OFFSETS, device=dev)
    images, _ = teacher_images(nets, e0, k, H, W, ex, ed, RENDER["num_coarse"], RENDER["num_fine"])
    images = images * gains[:, None, None, :] + offsets[:, None, None, :]
    results = []
    for lr in (0.01, 0.02, 0.005):
        for seed in (3, 4, 5):
            step = nerf.FusedPoseStep(nets[0], nets[1], options, H, W, k, e0, images, ex, ed, N_RAYS, lr, seed=seed, refine_pose=False,
                                      refine_exposure="affine", loss_weights=(0.0, 1.0))
            for it in range(3000):
                step.step()
                if it + 1 in (300, 600, 1000, 2000, 3000):
                    eps = step.exposure()
                    rec = dict(lr=lr, seed=seed, steps=it + 1, fine_mse=float(step.loss3[2]),
                               err_gain=float((torch.exp(eps[:, :3]) - gains).abs().max()), err_offset=float((eps[:, 3:] - offsets).abs().max()))
                    results.append(rec)
                    print(json.dumps(rec), flush=True)
    return results


def mode_train():
    from test_input_gradients import make_cfg
    from test_joint_pose_training import H, N_RAYS, RENDER, V, W, cameras, encoders, make_nets
    nerf.set_precision("fp32")
    e0, k = (t.to(dev) for t in cameras())
    ex, ed = encoders()
    thres = [15.0]
    canonical, dex_teacher = teacher_images(make_nets(dev), e0, k, H, W, ex, ed, thres=thres)
    view_gain = torch.tensor([1.0, 1.25, 0.8], device=dev)
    images = canonical * view_gain[:, None, None, None]
    train_cfg = make_cfg(dict(RENDER, noise_std=0.0))
    results = []
    for seed in range(3):
        for mode_name in (None, "gain"):
            nets = make_nets(dev)
            bucket = parallel.FlatGradBucket(nets)
            opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
            extra = dict(refine_exposure=mode_name, exposure_fixed_views=(0,)) if mode_name else {}
            step = nerf.FusedJointStep(nets[0], nets[1], train_cfg, H, W, k, e0, images, ex, ed, N_RAYS, bucket, opt, 1e-3, seed=seed,
                                       fixed_views=tuple(range(V)), **extra)
            for _ in range(600):
                step.step()
            torch.cuda.synchronize()
            assert step.fallback_reason is None, step.fallback_reason
            rgb, dex = teacher_images(nets, e0, k, H, W, ex, ed, thres=thres)
            both = torch.isfinite(dex) & torch.isfinite(dex_teacher)
            rec = dict(seed=seed, refine_exposure=mode_name, train_loss=step.loss3.tolist(),
                       psnr_canonical=float(nerf.mse2psnr(float(nerf.img2mse(rgb, canonical)))),
                       psnr_per_view=[float(nerf.mse2psnr(float(nerf.img2mse(rgb[v], canonical[v])))) for v in range(V)],
                       dex_mean_abs=float((dex - dex_teacher)[both].abs().mean()), dex_pixels=int(both.sum()),
                       gains=None if mode_name is None else torch.exp(step.exposure()[:, 0]).tolist())
            results.append(rec)
            print(json.dumps(rec), flush=True)
    return results


res = dict(head=mode_head, step=mode_step, recovery=mode_recovery, train=mode_train)[args.mode]()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
