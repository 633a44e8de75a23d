"""Developer measurements for the coarse-to-fine positional encoding (nerf.EncodingAnneal): profiles/encoding_anneal.md.  Recorded, not
gated.

    python scripts/encoding_anneal_measure.py --mode time --anneal 1 --out profiles/x.json            # this tree, with and without
    python scripts/encoding_anneal_measure.py --mode time --pkg <parent checkout>/dex-nerf_amd --out ...   # a built parent commit
    python scripts/encoding_anneal_measure.py --mode recovery --out ...

--mode time: every probe is an iteration replayed as one HIP graph under 'bf16', 64 + 64 samples, 3 views of 200 x 200 random pixels,
training settings (jitter, density noise 0.2), FlatAdam: FusedTrainStep(draw_view="rays") + GraphedTrainStep on 4 x 128 / 1024 rays and
D8 / W256 / 4096 rays, FusedJointStep on 4 x 128 / 2048 rays.  Wall clock around a window of 200 replayed steps that ends in a device
synchronise, divided by 200; 20 untimed steps first; 7 windows; median (min - max).  One process per package tree (two trees cannot
share a process), so parent and change are alternated process by process.  Launches: the calls of the anneal entry points in the
probe's first eager step (each makes one launch).  The schedule of a timed probe is (0, 1,000,000): every band but the first is off.

--mode recovery: the protocol of test_joint_training_recovers_perturbed_poses_and_beats_training_at_them (3 views of 24 x 20, 200 rays,
16 + 24 samples, fp32, lr 5e-4 / lr_pose 1e-3, fixed_views=(0,)) but from FRESHLY INITIALISED 4 x 128 networks, at that test's
perturbation and at five times it, 3 seeds, 2000 joint steps, without a schedule and with (0, 800) and (100, 1200); every 400 steps the
mean rotation error, the mean camera-centre distance and the fine MSE on a fixed ray set at the true poses."""
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
ap.add_argument("--mode", required=True, choices=["time", "recovery"])
ap.add_argument("--anneal", type=int, default=0)
ap.add_argument("--out", required=True)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch  # noqa: E402

import nerf  # noqa: E402
from nerf import parallel, synthetic as syn  # noqa: E402

dev = torch.device("cuda:0")
HAVE = hasattr(nerf, "EncodingAnneal")


def make_cfg(nc, nf, perturb=True, noise=0.2, white=True, chunk=65536):
    mode = dict(chunksize=chunk, lindisp=False, num_coarse=nc, num_fine=nf, perturb=perturb, radiance_field_noise_std=noise, white_background=white)
    return nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


def nets_of(kw, seed=5):
    torch.manual_seed(seed)
    return [nerf.models.FlexibleNeRFModel(**kw).to(dev) for _ in range(2)]


def count_anneal_launches(fn):
    from nerf import _hip
    if not HAVE:
        fn()
        return 0
    lib = _hip.lib()
    counts = [0]
    saved = {}
    for name in _hip.ANNEAL_EXPORTS:
        real = getattr(lib, name)
        saved[name] = real

        def wrapper(*a, _real=real):
            counts[0] += 1
            return _real(*a)
        setattr(lib, name, wrapper)
    try:
        fn()
    finally:
        for name, real in saved.items():
            setattr(lib, name, real)
    return counts[0]


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


def mode_time():
    nerf.set_precision("bf16")
    size, v = 200, 3
    images = torch.rand(v, size, size, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    poses = [torch.from_numpy(syn.scene_pose(p)) for p in (3, 9, 14)]
    kmat = torch.from_numpy(syn.intrinsic(size, size))
    cfg = make_cfg(64, 64)
    results = {}
    shapes = {"4x128_1024": (dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True), 1024),
              "d8w256_4096": (dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True), 4096)}
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    variants = [False] + ([True] if (HAVE and args.anneal) else [])
    for name, (kw, rays) in shapes.items():
        for with_anneal in variants:
            nets = nets_of(kw)
            bucket = parallel.FlatGradBucket(nets)
            sel = nerf.MultiViewRaySelector(size, size, poses, [kmat] * v, 2.0, 6.0, images=images, device=dev)
            extra = dict(encoding_anneal=nerf.EncodingAnneal(0, 1000000)) if with_anneal else {}
            fused = nerf.FusedTrainStep(nets[0], nets[1], sel, cfg, bucket, ex, ed, rays, seed=1, draw_view="rays", **extra)
            graphed = nerf.GraphedTrainStep(fused, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
            launches = count_anneal_launches(graphed.step)
            w = time_probe(graphed.step)
            assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
            results[f"{name}{'+anneal' if with_anneal else ''}"] = dict(windows_ms=w, median=statistics.median(w), min=min(w), max=max(w),
                                                                       anneal_launches=launches, loss=fused.loss3.tolist())
            print(args.tag, name, with_anneal, results[f"{name}{'+anneal' if with_anneal else ''}"], flush=True)
    kw = shapes["4x128_1024"][0]
    e0 = torch.stack(poses).to(dev)
    for with_anneal in variants:
        nets = nets_of(kw)
        bucket = parallel.FlatGradBucket(nets)
        opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
        extra = dict(encoding_anneal=nerf.EncodingAnneal(0, 1000000)) if with_anneal else {}
        joint = nerf.FusedJointStep(nets[0], nets[1], cfg, size, size, kmat.to(dev), e0, images, ex, ed, 2048, bucket, opt, 1e-3, seed=1,
                                    fixed_views=(0,), **extra)
        launches = count_anneal_launches(joint.step)
        w = time_probe(joint.step)
        assert joint.graph is not None and joint.fallback_reason is None, joint.fallback_reason
        key = f"joint_4x128_2048{'+anneal' if with_anneal else ''}"
        results[key] = dict(windows_ms=w, median=statistics.median(w), min=min(w), max=max(w), anneal_launches=launches, loss=joint.loss3.tolist())
        print(args.tag, key, results[key], flush=True)
    return results


def mode_recovery():
    """The protocol of test_joint_training_recovers_perturbed_poses_and_beats_training_at_them from FRESH networks."""
    import train_dexnerf
    from nerf import _ops
    from test_joint_pose_training import H, N_RAYS, RECOVERY, RECOVERY_ROT, RECOVERY_TRANS, V, W, cameras, encoders, make_nets
    nerf.set_precision("fp32")
    e_true, k = (t.to(dev) for t in cameras())
    ex, ed = encoders()
    teacher = make_nets(dev)
    render = make_cfg(64, 64, perturb=False, noise=0.0, white=True, chunk=4096)
    images = []
    for v in range(V):
        ro, rd = nerf.get_ray_bundle(H, W, float(k[0, 0]), e_true[v], k)
        with torch.no_grad():
            out = nerf.run_one_iter_of_nerf(H, W, float(k[0, 0]), teacher[0], teacher[1], ro, rd, render, mode="validation", encode_position_fn=ex,
                                            encode_direction_fn=ed)
        images.append(out[3].reshape(H, W, 3))
    images = torch.stack(images)
    flat = torch.randperm(V * H * W, generator=torch.Generator().manual_seed(123))[:600]
    views, pix = (flat // (H * W)).to(torch.int32).to(dev), (flat % (H * W)).to(dev)
    rows, target = _ops.select_rays_views(H, W, _ops.pose_records(torch.zeros(V, 6, device=dev), e_true.contiguous(), k), views, 2.0, 6.0, pix, images)
    quiet = make_cfg(16, 24, perturb=False, noise=0.0, white=True, chunk=4096)
    train_cfg = make_cfg(RECOVERY["num_coarse"], RECOVERY["num_fine"], perturb=True, noise=0.0, white=True, chunk=4096)
    mkw = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    total, every = 2000, 400
    results = []
    for scale in (1.0, 5.0):
        for seed in range(3):
            e_start = train_dexnerf.perturbed_poses(e_true, RECOVERY_ROT * scale, RECOVERY_TRANS * scale, 1000 + seed, keep=(0,))
            rot0, trans0 = train_dexnerf.pose_distance(e_start, e_true)
            for schedule in (None, (0, 800), (100, 1200)):
                nets = nets_of(mkw, seed=50 + seed)
                bucket = parallel.FlatGradBucket(nets)
                opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
                anneal = nerf.EncodingAnneal(*schedule) if schedule else None
                step = nerf.FusedJointStep(nets[0], nets[1], train_cfg, H, W, k, e_start, images, ex, ed, N_RAYS, bucket, opt, 1e-3, seed=seed,
                                           fixed_views=(0,), encoding_anneal=anneal)
                curve = []
                for it in range(total):
                    step.step()
                    if (it + 1) % every == 0:
                        torch.cuda.synchronize()
                        if anneal is not None:
                            anneal.set_iteration(it + 1)
                        with torch.no_grad():
                            out = nerf.predict_and_render_radiance(rows, nets[0], nets[1], quiet, mode="validation", encode_position_fn=ex,
                                                                   encode_direction_fn=ed)
                        rot, trans = train_dexnerf.pose_distance(step.extrinsics(), e_true)
                        curve.append(dict(step=it + 1, rot_deg=rot, centre=trans, fine_mse=float(nerf.img2mse(out[3], target))))
                assert step.fallback_reason is None, step.fallback_reason
                rec = dict(scale=scale, seed=seed, schedule=schedule, start=dict(rot_deg=rot0, centre=trans0), curve=curve)
                results.append(rec)
                print(json.dumps(rec), flush=True)
    return results


res = mode_time() if args.mode == "time" else mode_recovery()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
