"""Developer probe for the distortion regulariser (dn_distortion_loss, FusedTrainStep(distortion_weights=...)).  Recorded, not gated.

    python scripts/distortion_time.py --probe kernel
    python scripts/distortion_time.py --probe step --shape shipped|d8w256 --weights WC WF [--tree PATH --label NAME]

    kernel    dn_distortion_loss at (N, S) = (4096, 192) and (1024, 128): g_weights only, g_weights + g_z stored, + g_z accumulated; and
              the weights-only dn_volume_render pass the fused step adds for the fine network (what a variant that recomputes the
              weights inside the distortion kernel could save at most).  HIP events around BLOCK calls, the median of BLOCKS blocks.
    step      the fused training step replayed as one HIP graph (the set-up of scripts/depth_supervision_time.py: draw_view="rays",
              bf16, 20 views of 400 x 400) without the term, with it on the fine network, on both.  --tree PATH imports the package of
              another built checkout (the parent commit) instead of this one; it knows no distortion_weights, so --weights 0 0 there.

One JSON line per measurement; profiles/distortion_loss.md holds the recorded tables."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else REPO
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))

import torch  # noqa: E402

SHAPES = {
    "shipped": dict(net=dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True),
                    num_coarse=64, num_fine=64, rays=1024, what="4x128 L_xyz=6, 64+64 samples, 1024 rays"),
    "d8w256": dict(net=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
                   num_coarse=64, num_fine=128, rays=4096, what="D8/W256 L_xyz=10, 64+128 samples, 4096 rays"),
}
H = W = 400
VIEWS = 20
WARMUP, BLOCKS, BLOCK = 5, 5, 200
KERNEL_SHAPES = ((4096, 192), (1024, 128))


def block_ms(fn):
    """Milliseconds per call of fn(): [median, min, max] over BLOCKS blocks of BLOCK calls between two HIP events, after the warm-ups."""
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BLOCK):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / BLOCK)
    return [statistics.median(ms), min(ms), max(ms)]


def graphed_ms(fn):
    """block_ms of one HIP graph holding 20 calls of fn(), per call: the launches without the host's share (ctypes, allocator)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            fn()
    return [t / 20 for t in block_ms(g.replay)]


def probe_kernel(args):
    from nerf import _ops
    dev = torch.device("cuda:0")
    rows = []
    for n, s in KERNEL_SHAPES:
        gen = torch.Generator().manual_seed(n + s)
        z = (2.0 + 4.0 * torch.sort(torch.rand(n, s, generator=gen), dim=1).values).to(dev)
        rf = torch.randn(n, s, 4, generator=gen).to(dev)
        rays = torch.zeros(n, 11)
        rays[:, 3:6] = torch.randn(n, 3, generator=gen)
        rays[:, 6], rays[:, 7] = 2.0, 6.0
        rays = rays.to(dev)
        rd = rays[:, 3:6]
        weights = _ops.volume_render_fwd(rf, z, rd, None, 0.0, False, [])[3]
        acc = torch.zeros(n, s, device=dev)
        cases = {
            "dn_distortion_loss, g_weights": (lambda: _ops.distortion_loss(weights, z, rays=rays, scale=0.01 / n), 12 * n * s),
            "dn_distortion_loss, g_weights + g_z stored": (lambda: _ops.distortion_loss(weights, z, rays=rays, scale=0.01 / n, want_z=True), 16 * n * s),
            "dn_distortion_loss, g_weights + g_z accumulated": (lambda: _ops.distortion_loss(weights, z, rays=rays, scale=0.01 / n, g_z=acc), 20 * n * s),
            "dn_volume_render, weights only (the fine network's extra pass)": (lambda: _ops.volume_render_fwd(rf, z, rd, None, 0.0, False, []), 24 * n * s),
        }
        for name, (fn, nbytes) in cases.items():
            ms = graphed_ms(fn)
            rows.append(dict(probe="kernel", n=n, s=s, what=name, ms_per_call=ms, bytes=nbytes, gb_per_s=nbytes / ms[0] / 1e6))
    return rows


def probe_step(args):
    import nerf
    from nerf import parallel, synthetic as syn
    dev = torch.device("cuda:0")
    shape = SHAPES[args.shape]
    net, n = shape["net"], shape["rays"]
    nerf.set_precision("bf16")
    models = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**net)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **net).items()})
        models.append(m.to(dev))
    mode = dict(chunksize=4096, lindisp=False, num_coarse=shape["num_coarse"], num_fine=shape["num_fine"], perturb=True,
                radiance_field_noise_std=0.2, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    kmat = torch.from_numpy(syn.intrinsic(H, W))
    poses = [torch.from_numpy(syn.scene_pose(v, n_views=VIEWS)) for v in range(VIEWS)]
    gen = torch.Generator().manual_seed(1)
    sel = nerf.MultiViewRaySelector(H, W, poses, [kmat] * VIEWS, 2.0, 6.0, images=torch.rand(VIEWS, H, W, 3, generator=gen).to(dev), device=dev)
    reg = dict(distortion_weights=tuple(args.weights)) if max(args.weights) > 0 or TREE == REPO else {}
    bucket = parallel.FlatGradBucket(models)
    step = nerf.FusedTrainStep(models[0], models[1], sel, cfg, bucket, nerf.get_embedding_function(net["num_encoding_fn_xyz"]),
                               nerf.get_embedding_function(4), n, seed=7, draw_view="rays", **reg)
    graphed = nerf.GraphedTrainStep(step, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
    for _ in range(5):
        graphed.step()
    torch.cuda.synchronize()
    assert graphed.graphs is not None and graphed.fallback_reason is None, graphed.fallback_reason
    ms = block_ms(graphed.step)
    assert bool(torch.isfinite(step.loss3).all())
    reg2 = getattr(step, "reg2", None)
    return [dict(probe="step", shape=args.shape, what=shape["what"], weights=list(args.weights), build=args.label, step_ms=ms,
                 loss3=step.loss3.tolist(), reg2=None if reg2 is None else reg2.tolist())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", choices=("kernel", "step"), required=True)
    ap.add_argument("--tree", default="")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="shipped")
    ap.add_argument("--weights", type=float, nargs=2, default=(0.0, 0.0), metavar=("WC", "WF"))
    args = ap.parse_args()
    for row in (probe_kernel if args.probe == "kernel" else probe_step)(args):
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
