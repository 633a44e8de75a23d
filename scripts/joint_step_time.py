"""Developer timing probe for the joint pose-and-network iteration (nerf.FusedJointStep) beside the steps it stands in for.  Recorded,
not gated.

    python scripts/joint_step_time.py --out profiles/joint_training

One process.  Every probe is a step replayed as one HIP graph: lego-shaped 4 x 128 nets (L_xyz = 10), 64 + 64 samples, 2048 rays, 3
views of 400 x 400 random pixels, training settings (jitter, density noise 0.2), FlatAdam on the networks.

    joint fp32 | joint bf16          FusedJointStep.step (bf16: 16-bit saved tensors), fixed_views=(0,)
    train bf16-s16                   FusedTrainStep(draw_view="rays") + GraphedTrainStep under 'bf16-s16': the network half alone
    pose fp32 | pose bf16            FusedPoseStep.step on frozen networks: the camera half alone
    train bf16                       the parameter-only step in the default 8-bit saved-tensor mode, which the joint step cannot use
    train fp32                       the parameter-only step in fp32

Times: wall clock around a window of WINDOW replayed steps that ends in a device synchronise, divided by WINDOW; 20 untimed steps per
probe first (3 eager, the capture, replays); REPEATS windows per probe, the probes ALTERNATED window by window (the machine is shared);
the median (min - max) over the windows.  Launches: the device kernels and memsets torch.profiler sees in ONE eager step of the same
object, taken straight after the probe's own 20 steps - the launches the captured graph holds."""
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

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
H = W = 400
V, RAYS = 3, 2048
WINDOW, REPEATS, WARMUP = 200, 7, 20
POSES = (3, 9, 14)


def build(kind, precision, dev):
    """(step callable, the object that holds .graph / .graphs, eager-step callable) of one probe."""
    import numpy as np

    import nerf
    from nerf import parallel, synthetic as syn
    nerf.set_precision(precision)
    w = dict(np.load(os.path.join(REPO, "tests", "golden", "lego_weights.npz")))
    nets = []
    for prefix in ("wc_", "wf_"):
        m = nerf.models.FlexibleNeRFModel(**NET)
        m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in w.items() if k.startswith(prefix)})
        nets.append(m.to(dev))
    mode = dict(chunksize=4096, lindisp=False, num_coarse=64, num_fine=64, perturb=True, radiance_field_noise_std=0.2, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    k = torch.from_numpy(syn.intrinsic(H, W)).to(dev)
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES]).to(dev)
    images = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    if kind == "pose":
        for m in nets:
            for p in m.parameters():
                p.requires_grad_(False)
        step = nerf.FusedPoseStep(nets[0], nets[1], cfg, H, W, k, e0, images, ex, ed, RAYS, 1e-3, seed=3, fixed_views=(0,))
        return step.step, step, lambda: step._enqueue()
    bucket = parallel.FlatGradBucket(nets)
    opt = nerf.FlatAdam(bucket, lr=5e-4, lr_decay_factor=0.1, lr_decay_steps=250000, zero_grads=True)
    if kind == "joint":
        step = nerf.FusedJointStep(nets[0], nets[1], cfg, H, W, k, e0, images, ex, ed, RAYS, bucket, opt, 1e-3, seed=3, fixed_views=(0,))
        return step.step, step, lambda: step._enqueue()
    sel = nerf.MultiViewRaySelector(H, W, list(e0), [k] * V, 2.0, 6.0, images=images, device=dev)
    fused = nerf.FusedTrainStep(nets[0], nets[1], sel, cfg, bucket, ex, ed, RAYS, seed=3, draw_view="rays")
    loop = nerf.GraphedTrainStep(fused, opt, eager_iterations=3)
    return loop.step, loop, loop._eager


def launches(eager):
    """Device kernels + memsets of one eager step, or None when the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            eager()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer.step")]
        return (len(names), sorted(set(names))) if names else None
    except Exception as exc:  # noqa: BLE001
        return None if not str(exc) else (None, [f"{type(exc).__name__}: {exc}"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing probe needs the GPU"
    dev = torch.device("cuda:0")
    import nerf
    probes = [("joint", "fp32"), ("joint", "bf16"), ("train", "bf16-s16"), ("pose", "fp32"), ("pose", "bf16"), ("train", "bf16"), ("train", "fp32")]
    built = {}
    for kind, precision in probes:
        step, holder, eager = build(kind, precision, dev)
        for _ in range(WARMUP):
            nerf.set_precision(precision)
            step()
        torch.cuda.synchronize()
        graphs = getattr(holder, "graphs", None) or ([holder.graph] if getattr(holder, "graph", None) is not None else [])
        assert len(graphs) == 1 and holder.fallback_reason is None, (kind, precision, holder.fallback_reason)
        # counted here, straight after the probe's own steps: a later optimizer step of ANOTHER probe makes a frozen pose step re-pack
        built[(kind, precision)] = (step, launches(eager))
    windows = {p: [] for p in probes}
    for _ in range(REPEATS):
        for p in probes:
            nerf.set_precision(p[1])
            step = built[p][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(WINDOW):
                step()
            torch.cuda.synchronize()
            windows[p].append((time.perf_counter() - t0) * 1e3 / WINDOW)
    rows = []
    for p in probes:
        nerf.set_precision(p[1])
        count = built[p][1]
        ms = windows[p]
        rows.append(dict(probe=f"{p[0]} {p[1]}", ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), windows=ms,
                         launches=None if count is None else count[0], kernels=None if count is None else count[1]))
        print(json.dumps({k: v for k, v in rows[-1].items() if k != "kernels"}), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), rays=RAYS, views=V, image=f"{H}x{W}", samples="64+64", nets="lego 4x128 L_xyz=10",
                  window=WINDOW, repeats=REPEATS, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".json", "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
