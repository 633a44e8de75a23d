#!/usr/bin/env python3
"""Headline benchmark: rays/s of the nerf-pytorch / Dex-NeRF ray-marching hot path on MI355X.

Workload (BASELINE.json configs[1], SURVEY.md section 8d "C2"): a 400x400 synthetic Lego-style view,
64 coarse + 128 fine samples per ray, coarse and fine FlexibleNeRFModel D=8 / W=256 / skip 4 with view
directions, PE L=10/4, K=20 Dex thresholds, validation-mode render (deterministic resampling, no noise).
One "step" = one full image (160,000 rays) through run_one_iter_of_nerf -> predict_and_render_radiance on
this rank's GPU, inputs (ray bundle, packed weights) resident in HBM before the timed region.

    python bench.py --gpus N --steps K --warmup W            (N > 1: launched by torch.distributed.run)
    python bench.py --gpus N --steps K --warmup W --full     (+ every informational leg, a few minutes)
    python bench.py ... --dump-outputs DIR                   (+ the last timed step's maps as DIR/<name>.npy)

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step, dtype, config).
--full adds what takes runs of its own: the fine-net kernel's roofline (HIP events, PMC record, library-GEMM
yardstick), the CPU oracle baseline with PSNR / Dex agreement, the fp16-policy and exact-fp32 renders, the other
BASELINE configs, the training-iteration rates and, at N > 1, the data-parallel step and the sharded image.
Multi-GPU: rays/images are independent units -> each rank renders its own view of the scene (weak scaling,
no data-path collective); the barrier + max-over-ranks timing uses RCCL.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "dex-nerf_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H = W = 400
NC, NF = 64, 128
MODEL_KW = dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4,
                use_viewdirs=True)
FLOP_PER_POINT = 1186816           # unpadded dims, SURVEY.md section 8d
POINTS_PER_RAY = NC + (NC + NF)    # coarse net + fine net
M_THRES = [float(m) for m in range(5, 105, 5)]
PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3}   # dense MFMA peaks, MI355X_MICROARCH.md


def build_scene(dev, rank, h=H, w=W, nc=NC, nf=NF, model_kw=None, near=2.0, far=6.0):
    import nerf
    from nerf import synthetic as syn
    model_kw = MODEL_KW if model_kw is None else model_kw
    models = []
    for seed, bias in ((42, -150.0), (43, -20.0)):
        m = nerf.models.FlexibleNeRFModel(**model_kw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **model_kw).items()})
        models.append(m.to(dev))
    mode = dict(chunksize=h * w, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False,
                radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=near, far=far, no_ndc=True),
                            nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    k_mat = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
    e_mat = torch.from_numpy(syn.scene_pose(7 + rank)).to(dev)   # each rank: its own view of the scene
    ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), e_mat, k_mat)
    ex, ed = nerf.get_embedding_function(10, True, True), nerf.get_embedding_function(4, True, True)
    return models, cfg, ro, rd, ex, ed


def render(models, cfg, ro, rd, ex, ed):
    import nerf
    h, w = ro.shape[0], ro.shape[1]
    with torch.no_grad():
        return nerf.run_one_iter_of_nerf(h, w, 1.0, models[0], models[1], ro, rd, cfg, mode="validation",
                                         encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=M_THRES)


def render_dtype():
    """Arithmetic type of the no-grad render under the current precision + render policy (nerf.set_render_policy)."""
    from nerf import _hip, _ops
    return {_hip.PREC_F32: "fp32", _hip.PREC_BF16: "bf16", _hip.PREC_F16: "fp16"}[_ops.render_precision()]


def time_dominant_kernel(models, ro, rd, precision=None, reps=5, samples=NC + NF, flop_per_point=FLOP_PER_POINT, near=2.0, far=6.0):
    """HIP-event timing of the dominant kernel (fused PE+MLP on the fine network, all rays x all samples of the image) on the
    stream it is launched on (PyTorch's current stream), in the precision the no-grad render runs in."""
    from nerf import _ops
    dev = ro.device
    n = ro.shape[0] * ro.shape[1]
    rays = torch.cat([ro.reshape(-1, 3), rd.reshape(-1, 3), torch.full((n, 1), near, device=dev),
                      torch.full((n, 1), far, device=dev),
                      torch.nn.functional.normalize(rd.reshape(-1, 3), dim=-1)], -1).contiguous()
    z = torch.sort(torch.rand(n, samples, device=dev) * (far - near) + near, -1)[0].contiguous()
    packed = models[1].packed(precision=_ops.render_precision())
    _ops.run_network_rays(packed, rays, z)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _ops.run_network_rays(packed, rays, z)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    t = float(np.mean(times))
    flops = n * samples * flop_per_point
    return t, flops / t / 1e12


def other_config_render(dev, rank, tag, h, w, nc, nf, model_kw, flop_per_point, near, far, steps=3):
    """BASELINE configs[2] / configs[3] as single-GPU render workloads, with the fine-net launch's roofline (informational legs of
    the line: the headline stays configs[1])."""
    models, cfg, ro, rd, ex, ed = build_scene(dev, rank, h, w, nc, nf, model_kw, near, far)
    render(models, cfg, ro, rd, ex, ed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        render(models, cfg, ro, rd, ex, ed)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    kt, ktf = time_dominant_kernel(models, ro, rd, reps=3, samples=nc + nf, flop_per_point=flop_per_point, near=near, far=far)
    peak = PEAK_TFLOPS[render_dtype()]
    pts = nc + (nc + nf)
    return {"workload": tag, "value": h * w / dt, "unit": "rays/s", "ms_per_image": dt * 1e3, "dtype": render_dtype(),
            "kernel_ms": kt * 1e3, "tflops": ktf, "peak": peak, "frac": ktf / peak,
            "whole_path_tflops": h * w / dt * pts * flop_per_point / 1e12, "flop_per_ray": pts * flop_per_point}


def geometry48(precision):
    """True when the 16-bit fine-net launch runs the 48-points-per-wave kernel (the default; DEXNERF_BF16_GEOM=32 keeps the 32-point one)."""
    return precision in ("bf16", "fp16") and os.environ.get("DEXNERF_BF16_GEOM", "") != "32"


KERNEL_SOURCES = ("mlp_fused48.hip", "mlp_fused48_kernel.h", "mlp_stage48.h", "mlp_device.h", "mlp_geo48.h")


def kernel_source_sha16():
    """sha256 (first 16 hex digits) over the sources of the headline kernel as they are in this tree: a committed PMC record names the
    sources it was collected on (scripts/pmc_collect.py writes the same figure) and is refused when they have changed since."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(REPO, "dex-nerf_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def kernel_isa_sha16(precision):
    """sha256 (first 16 hex digits) of the instruction stream of the headline kernel instance in the library this process loads
    (scripts/codeobj.py: code objects out of the .so, llvm-objdump): the identity of the kernel BINARY.  None without the LLVM tools."""
    try:
        scripts = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts")
        if scripts not in sys.path:
            sys.path.insert(0, scripts)
        import codeobj
        lib = os.environ.get("DEXNERF_HIP_LIB") or codeobj.DEFAULT_LIB
        return codeobj.kernel_isa_sha16(headline_kernel_name(precision) + "(", lib)
    except Exception:  # noqa: BLE001 - informational: the source hash below still guards the record
        return None


def headline_kernel_name(precision):
    """Demangled name of the instance the fine-net launch of the headline configuration runs (what rocprofv3 reports)."""
    if geometry48(precision):
        # (rays + depths: the instance that encodes tile t + 1 inside tile t's view-direction stage, unless switched off)
        ovl = 0 if os.environ.get("DEXNERF_G48_NO_OVERLAP") else 2
        return f"mlp_forward48_kernel<256, {2 if precision == 'fp16' else 1}, 8, 16u, 1, 0, {ovl}, 0>"
    return "mlp_forward_kernel<256, 10, 4"


def pmc_record(precision):
    """The committed rocprofv3 --pmc passes on this exact launch (scripts/pmc_fine_net.sh -> profiles/r0N_pmc_fine_net_<type>.json:
    FETCH_SIZE and WRITE_SIZE collected in SEPARATE passes, FETCH_SIZE doubled per the gfx950 correction of
    MI355X_MICROARCH.md).  bench.py itself cannot run the profiler.  A record is used only if it names the kernel instance this run
    times AND was collected on this kernel binary (or, failing that check, these kernel sources); otherwise `traffic` is null and
    `traffic_record` says why."""
    want = headline_kernel_name(precision)
    for rnd in ("r04", "r03", "r02"):
        path = os.path.join(REPO, "profiles", f"{rnd}_pmc_fine_net_{precision}.json")
        if not os.path.exists(path):
            continue
        doc = json.load(open(path))
        kernel = doc.get("kernel", "")
        if want not in kernel.replace("dn::", ""):
            return {"record": f"profiles/{os.path.basename(path)} refused: it profiles `{kernel[:80]}`, this run times `{want}`"}
        # the record must belong to the kernel this run times: the same instruction stream (the record's isa_sha16 against the loaded
        # library's - survives comments and refactors, not a moved instruction), or, where either side lacks it, the same sources
        isa_here = kernel_isa_sha16(precision) if doc.get("isa_sha16") else None
        if isa_here is not None:
            if doc["isa_sha16"] != isa_here:
                return {"record": f"profiles/{os.path.basename(path)} refused: collected on kernel binary {doc['isa_sha16']}, this library holds {isa_here}"}
        elif doc.get("source_sha16") != kernel_source_sha16():
            return {"record": f"profiles/{os.path.basename(path)} refused: collected on kernel sources {doc.get('source_sha16')}, this tree has {kernel_source_sha16()}"}
        rec = dict(doc.get("derived", {}))
        rec["record"] = "profiles/" + os.path.basename(path)
        rec["record_tied_by"] = "isa_sha16" if isa_here is not None else "source_sha16"
        return rec
    return {"record": "no committed PMC record for this precision"}


def library_gemm_tflops(dev, precision):
    """Yardstick next to the datasheet peak: what the vendor GEMM library (torch a @ b) reaches on this box for a large
    square GEMM in the same input type (informational; ~15 ms)."""
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(precision, torch.float32)
    m = 8192
    a = torch.randn(m, m, device=dev, dtype=dt)
    b = torch.randn(m, m, device=dev, dtype=dt)
    for _ in range(3):
        a @ b
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(10):
        a @ b
    ev[1].record()
    torch.cuda.synchronize()
    return {"shape": f"{m}^3 {precision}", "tflops": 2.0 * m ** 3 * 10 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e12}


def train_rate(models, cfg, ro, rd, ex, ed, n_rays=4096, steps=8, dist=None, pose_id=7, nc=NC, nf=NF, luminance=False, h=H, w=W,
               near=2.0, far=6.0, what_tail="64+128 samples, perturb + noise 0.2, D8/W256 x2"):
    """Secondary metric (SURVEY.md section 8d ii): rays/s of a full training iteration (perturbed sampling, density
    noise, forward + backward + Adam) on n_rays random rays of this rank's view.  With `dist` (N > 1) it is the data-parallel
    step north_star names (reference loop: train_dexnerf_rgb.py:264-289): every rank its own rays, the gradients of both nets
    averaged over RCCL (one message per network, the fine one overlapped with the coarse backward - nerf/parallel.py), identical
    fused Adam on every rank; barrier + max-over-ranks timing like the headline."""
    import nerf
    from nerf import _hip, _ops, parallel
    dev = ro.device
    world = dist.get_world_size() if dist is not None else 1
    cfg.nerf.train.perturb = True
    cfg.nerf.train.radiance_field_noise_std = 0.2
    cfg.nerf.train.chunksize = n_rays
    if dist is not None:
        parallel.broadcast_parameters(models)
    bucket = parallel.FlatGradBucket(models)
    # Adam over the flat parameter buffer: one launch, clears the gradients in the same pass (nerf.FlatAdam; what train_dexnerf.py steps)
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    from nerf import synthetic as syn
    image = torch.rand(1, h, w, 3, device=dev)
    selector = nerf.MultiViewRaySelector(h, w, [torch.from_numpy(syn.scene_pose(pose_id))], [torch.from_numpy(syn.intrinsic(h, w))], near, far,
                                         images=image, device=dev)
    # the iteration the build's training driver runs (train_dexnerf.py): device-side pixel draw, the render with its draws made
    # in the kernels, loss head + upstream gradients in one launch, backward, exchange, fused Adam (nerf.FusedTrainStep)
    fused = nerf.FusedTrainStep(models[0], models[1], selector, cfg, bucket, ex, ed, n_rays, seed=1234 + pose_id, luminance=luminance)

    # ... replayed as HIP graphs: one graph at N = 1; at N > 1 three graphs around the exchange - draw .. fine backward | coarse
    # backward | Adam, each network's all-reduce launched eagerly in between (nerf.GraphedTrainStep)
    graphed = nerf.GraphedTrainStep(fused, opt, eager_iterations=3, use_graphs=os.environ.get("DEXNERF_BENCH_NO_GRAPH", "") != "1")
    step = graphed.step
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = (time.perf_counter() - t0) / steps
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    res = {"rays_per_s": world * n_rays / dt, "ms_per_step": dt * 1e3, "rays_per_step_per_gpu": n_rays, "n_gpus": world,
           "hip_graphs_per_step": len(graphed.graphs) if graphed.graphs else 0, "graph_fallback": graphed.fallback_reason,
           "what": "device pixel draw + ray rows + fwd + loss + bwd + Adam (nerf.FusedTrainStep + nerf.FlatAdam under nerf.GraphedTrainStep), " + what_tail}
    # roofline of the step: HBM-bound by construction (HISTORY.md section 4.6) - the saved activations and gradients are written
    # once by the forward / backward chains and read once by the weight-gradient kernel; MFMA rate beside it (3x forward FLOP)
    nbytes = 0
    for m, s in ((models[0], nc), (models[1], nc + nf)):
        a, mk, g = _ops.train_sizes(m.packed(train=True), n_rays * s, prec=_ops.train_precision(m.packed(train=True)))
        nbytes += 2 * (a + g) + 2 * mk + n_rays * s * (16 + 16 + 4) * 2   # + rf / g_rf / z through compositing
    flops = 3.0 * n_rays * (nc + nc + nf) * FLOP_PER_POINT
    res["roofline"] = {"bound": "hbm", "achieved": nbytes / dt / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": nbytes / dt / 8e12,
                       "bytes_per_step": nbytes, "mfma_tflops": flops / dt / 1e12,
                       "mfma_frac": flops / dt / 1e12 / PEAK_TFLOPS[nerf.get_precision().split("-")[0]],
                       "what": "algorithmic bytes per step per GPU = 2 x (saved activations + saved gradients) + 2 x ReLU masks "
                               "(dn_mlp_train_sizes, both nets) + the radiance-field tensors through compositing; whole step time"}
    if dist is not None:
        # the exchange alone: both segments, back to back, nothing to overlap with
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(3):
            dist.all_reduce(bucket.segment(1)); dist.all_reduce(bucket.segment(0))
        torch.cuda.synchronize()
        evs[0].record()
        for _ in range(10):
            dist.all_reduce(bucket.segment(1)); dist.all_reduce(bucket.segment(0))
        evs[1].record()
        torch.cuda.synchronize()
        res["allreduce_ms"] = evs[0].elapsed_time(evs[1]) / 10
        res["allreduce_bytes"] = int(bucket.flat.numel() * 4)
        res["rccl_ranks"] = world
        res["what"] += "; data-parallel: per-network RCCL all-reduce (ReduceOp.AVG; the fine one overlapped with the coarse backward's graph), every rank its own rays"
    return res


def sharded_render_rate(dev, rank, dist, steps=3):
    """ONE 800x800 image (BASELINE configs[3]: 64 + 192 samples, D8/W256) rendered by all ranks together - nerf.parallel.render_sharded:
    every rank renders its block of rows, one all_gather per output map hands every rank the whole image.  Strong scaling of a
    single image, next to the weak-scaling headline (one image per rank).  all_gather_ms: the same exchange alone."""
    import nerf
    from nerf import parallel
    h = w = 800
    models, cfg, ro, rd, ex, ed = build_scene(dev, 0, h, w, 64, 192)      # (every rank: the SAME view)
    world = dist.get_world_size()

    def block(ro_b, rd_b):
        cfg.nerf.validation.chunksize = ro_b.shape[0] * ro_b.shape[1]
        return tuple(render(models, cfg, ro_b, rd_b, ex, ed))

    def timed(fn):
        fn()
        torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize(); dist.barrier()
        t = torch.tensor([(time.perf_counter() - t0) / steps], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), out
    dt, out = timed(lambda: parallel.render_sharded(block, ro, rd))
    lo, hi = parallel.shard_bounds(h, rank, world)
    mine = block(ro[lo:hi], rd[lo:hi])
    dt_gather, _ = timed(lambda: parallel.render_sharded(lambda a, b: mine, ro, rd))
    assert all(o is None or o.shape[0] == h for o in out)
    return {"workload": "ONE 800x800 image, 64+192 samples, D8/W256, rows split over the ranks (parallel.render_sharded)",
            "render_sharded_ms": dt * 1e3, "all_gather_ms": dt_gather * 1e3, "rays_per_s": h * w / dt, "n_gpus": world,
            "gathered_bytes_per_rank": int(sum(o.numel() * o.element_size() for o in out if o is not None))}


def dex_agreement(out, ref, sel, dev):
    """Dex-NeRF fixed-sigma depth readout (reference nerf/volume_rendering_utils.py:51-58) of this render against the fp32 CPU
    oracle on the sampled rays: fraction of (threshold, ray) entries within 1e-4 of the depth range's maximum, and the worst
    miss in metres (the readout is a thresholded first crossing: one flipped sample moves it by a sample spacing or more)."""
    idx = torch.from_numpy(sel).to(dev)
    mine = np.stack([o.reshape(-1)[idx].cpu().numpy() for o in out[6:]]).astype(np.float64)
    theirs = np.stack([o.numpy() for o in ref[6:]]).astype(np.float64)
    miss = np.abs(mine - theirs)
    return {"agree_frac": float((miss <= 1e-4 * np.abs(theirs).max()).mean()), "worst_miss_m": float(miss.max()),
            "mean_miss_m": float(miss.mean()), "entries": int(miss.size)}


def train_psnr_vs_oracle(dev, iters=300, precision="bf16"):
    """SURVEY section 8(d) metric (b): training PSNR at a matched iteration count, this library's training iteration (nerf.FusedTrainStep +
    nerf.FlatAdam: device-side draws, fused loss head, one-launch Adam with the in-kernel schedule - what train_dexnerf.py runs) against the
    CPU oracle's (autograd through its restatement of the reference path, torch.optim.Adam, the reference's loop:
    train_dexnerf_rgb.py:229-289).  Same teacher images, same initial weights, same loss / optimizer / schedule; each side draws its
    own views, pixels and jitter, so the comparison is statistical: PSNR = mse2psnr(MSE_coarse + MSE_fine) of the training batch,
    averaged over the last 20 iterations before each mark.  4 x 128 nets (the fork's as-shipped architecture), 32 x 32 views,
    256 rays per step, 32 + 32 samples - sized so the oracle's side takes ~10 s of CPU."""
    import nerf
    from nerf import parallel, synthetic as syn
    from oracle import nerf_oracle as oc
    hh = ww = 32
    views, n, nc, nf = 6, 256, 32, 32
    kw = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    mode = dict(chunksize=hh * ww, lindisp=False, num_coarse=nc, num_fine=nf, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True),
                            nerf=dict(use_viewdirs=True, train=dict(mode, perturb=True), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(10), nerf.get_embedding_function(4)
    k_mat = torch.from_numpy(syn.intrinsic(hh, ww))
    poses = [torch.from_numpy(syn.scene_pose(i, n_views=views)) for i in range(views)]
    before = nerf.get_precision()
    nerf.set_precision("fp32")
    try:
        teacher = []
        for seed, bias in ((42, -150.0), (43, -20.0)):
            m = nerf.models.FlexibleNeRFModel(**kw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **kw).items()})
            teacher.append(m.to(dev))
        images = []
        for pose in poses:
            ro, rd = nerf.get_ray_bundle(hh, ww, float(k_mat[0, 0]), pose.to(dev), k_mat.to(dev))
            with torch.no_grad():
                out = nerf.run_one_iter_of_nerf(hh, ww, 1.0, teacher[0], teacher[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                encode_direction_fn=ed)
            images.append(out[3].reshape(hh, ww, 3))
        torch.manual_seed(1)
        init = [nerf.models.FlexibleNeRFModel(**kw).state_dict() for _ in range(2)]
        marks = [m for m in (100, 200, 300, 400) if m <= iters]
        lr0, factor, decay_steps = 5e-4, 0.1, 250000
        # ---- this library's iteration
        nerf.set_precision(precision)
        models = []
        for sd in init:
            m = nerf.models.FlexibleNeRFModel(**kw)
            m.load_state_dict(sd)
            models.append(m.to(dev))
        bucket = parallel.FlatGradBucket(models)
        opt = nerf.FlatAdam(bucket, lr=lr0, lr_decay_factor=factor, lr_decay_steps=decay_steps, zero_grads=True)
        selector = nerf.MultiViewRaySelector(hh, ww, poses, [k_mat] * views, 2.0, 6.0, images=torch.stack(images), device=dev)
        fused = nerf.FusedTrainStep(models[0], models[1], selector, cfg, bucket, ex, ed, n, seed=7, draw_view=True)
        step = nerf.GraphedTrainStep(fused, opt, eager_iterations=iters + 1)      # (eager: every iteration's loss is read back)
        losses = []
        for _ in range(iters):
            step.step()
            losses.append(fused.loss3[0:1].clone())
        mine = torch.cat(losses).cpu().numpy().astype(np.float64)
        # ---- the CPU oracle's iteration (reference loop)
        nerf.set_precision("fp32")
        mc = oc.ModelCfg(**kw)
        rcfg = oc.RenderCfg(num_coarse=nc, num_fine=nf, near=2.0, far=6.0, perturb=True, m_thres=())
        sds = [oc.to_torch_sd({k: v.numpy() for k, v in sd.items()}, requires_grad=True) for sd in init]
        o_opt = torch.optim.Adam([t for sd in sds for t in sd.values()], lr=lr0)
        gen = np.random.default_rng(0)
        imgs_cpu = [im.reshape(-1, 3).cpu() for im in images]
        bundles = [oc.get_ray_bundle(hh, ww, pose, k_mat) for pose in poses]
        theirs = []
        t0 = time.perf_counter()
        for it in range(iters):
            v = int(gen.integers(views))
            pix = gen.choice(hh * ww, n, replace=False)
            ro, rd = bundles[v]
            out = oc.run_one_iter(ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix], sds[0], sds[1], mc, mc, rcfg)
            loss = oc.nerf_loss(out, imgs_cpu[v][pix])
            o_opt.zero_grad(set_to_none=True)
            loss.backward()
            o_opt.step()
            for g in o_opt.param_groups:
                g["lr"] = lr0 * factor ** (it / decay_steps)
            theirs.append(float(loss.detach()))
        cpu_s = time.perf_counter() - t0
        theirs = np.asarray(theirs)

        def psnr_at(curve, m):
            return float(-10.0 * np.log10(max(curve[max(m - 20, 0): m].mean(), 1e-12)))
        rows = [{"iteration": m, "hip_psnr_db": psnr_at(mine, m), "oracle_psnr_db": psnr_at(theirs, m)} for m in marks]
        return {"marks": rows, "final_delta_db": rows[-1]["hip_psnr_db"] - rows[-1]["oracle_psnr_db"], "iterations": iters,
                "precision": precision, "oracle_cpu_s": cpu_s,
                "what": "training PSNR (mse2psnr of coarse + fine MSE, mean of the 20 batches before each mark) at matched iteration counts: "
                        "nerf.FusedTrainStep + nerf.FlatAdam on the device vs autograd through the CPU oracle with torch.optim.Adam; 4x128 nets, "
                        "6 views of 32x32, 256 rays/step, 32+32 samples, same initial weights, each side its own draws"}
    finally:
        nerf.set_precision(before)


def cpu_baseline(sample_rays=16384, return_aux=False):
    """The CPU oracle (a restatement of the reference's PyTorch path, pinned to goldens captured from the
    reference) timed on this box's host cores on a bounded sample of the same workload.
    return_aux (the stage-wise parity test): also the oracle's intermediates per ray - coarse / merged depths, both raw radiance
    fields, the coarse weights, the sampler's indices - and the packed ray rows (same arithmetic, same time)."""
    from nerf import synthetic as syn
    from oracle import nerf_oracle as oc
    # the GPU box gives one-GPU jobs a 16-CPU share: more threads than that only oversubscribes
    threads = max(1, min(len(os.sched_getaffinity(0)), os.cpu_count() or 1, 16))
    torch.set_num_threads(threads)
    sd_c = oc.to_torch_sd(syn.synth_state_dict(42, sigma_bias=-150.0, **MODEL_KW))
    sd_f = oc.to_torch_sd(syn.synth_state_dict(43, sigma_bias=-20.0, **MODEL_KW))
    ro, rd = oc.get_ray_bundle(H, W, syn.scene_pose(7), syn.intrinsic(H, W))
    sel = syn.select_rays(H, W, sample_rays, seed=0)
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    cfg = oc.RenderCfg(num_coarse=NC, num_fine=NF, near=2.0, far=6.0, chunksize=4096, m_thres=M_THRES)
    mc = oc.ModelCfg(**MODEL_KW)
    aux = None
    with torch.no_grad():
        oc.run_one_iter(ro[:512], rd[:512], sd_c, sd_f, mc, mc, cfg)  # warm-up
        t0 = time.perf_counter()
        if not return_aux:
            out = oc.run_one_iter(ro, rd, sd_c, sd_f, mc, mc, cfg)
        else:   # run_one_iter's own loop (ray chunking as train_utils.py:252-271), keeping the intermediates
            rays = oc.pack_rays(ro, rd, cfg)
            outs, auxs = [], []
            for i in range(0, rays.shape[0], cfg.chunksize):
                o, a = oc.predict_and_render(rays[i: i + cfg.chunksize], sd_c, sd_f, mc, mc, cfg, None, return_aux=True)
                outs.append(o)
                auxs.append(dict(z_coarse=a["z_coarse"], rf_coarse=a["rf_coarse"], w_coarse=a["vc"]["weights"], z_fine=a["z_fine"],
                                 rf_fine=a["rf_fine"], inds=a["sp"]["inds"], z_samples=a["z_samples"]))
            out = tuple(torch.cat(c, dim=0) for c in zip(*outs))
            aux = {k: torch.cat([a[k] for a in auxs], dim=0) for k in auxs[0]}
            aux["rays"] = rays
        dt = time.perf_counter() - t0
    cb = dict(value=sample_rays / dt, unit="rays/s", cores=threads, kind="port",
              sample=f"{sample_rays} rays of the same 400x400 view, 64+128 samples, D8/W256 fp32, "
                     f"torch {torch.__version__} CPU, {threads} threads, {dt:.1f} s")
    return (cb, sel, out, aux) if return_aux else (cb, sel, out)


OUTPUT_NAMES = ("rgb_coarse", "depth_coarse", "acc_coarse", "rgb_fine", "depth_fine", "acc_fine")


def dump_outputs(out, path):
    """What the timed render returned (run_one_iter_of_nerf, validation mode) as float32 .npy files under `path`: the six image maps
    by name and the K Dex depth maps stacked as dex_depth (K, H, W) - 400 x 400 x 30 floats, 19.2 MB."""
    os.makedirs(path, exist_ok=True)
    arrays = dict(zip(OUTPUT_NAMES, out[:6]))
    arrays["dex_depth"] = torch.stack(list(out[6:]))
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.detach().float().cpu().numpy())
    return sorted(arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--full", action="store_true", help="also every informational leg (roofline, CPU baseline, other precisions / "
                                                        "configs, training rates); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the maps of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle and the legs compared with it")
    ap.add_argument("--no-train", action="store_true", help="with --full: skip the training-iteration measurements")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world == 1 and "TORCHELASTIC_RUN_ID" not in os.environ:
        # started plainly (`python bench.py --gpus N`): launch the ranks ourselves - a CHILD torch.distributed.run (this process has
        # not touched the GPU and never will: no exec), one rank per GPU over RCCL; relay its one JSON line, exit with its code
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in proc.stdout.splitlines():
            if line.lstrip().startswith("{"):
                print(line, flush=True)
            else:
                print(line, file=sys.stderr, flush=True)
        raise SystemExit(proc.returncode)
    if os.environ.get("DEXNERF_DIST_BACKEND", "nccl") != "nccl":
        local_rank %= max(torch.cuda.device_count(), 1)      # rehearsal: ranks may share a GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ:   # under torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # "nccl" is RCCL on ROCm.  DEXNERF_DIST_BACKEND=gloo lets the N > 1 leg be rehearsed with several ranks on ONE GPU
        # (RCCL refuses two ranks on the same device); ranks then share cuda:0
        backend = os.environ.get("DEXNERF_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus} but the RCCL process group has {dist.get_world_size()} ranks")

    import nerf
    from nerf import _hip
    _hip.lib()  # fail loudly if the HIP extension is missing
    nerf.set_precision(args.precision)
    # The headline is timed in the CONFIG's arithmetic type (BASELINE configs[1]: bf16 - what rounds 1-2 reported): every kernel of the
    # render in bf16.  The library's own default under set_precision("bf16") - no-grad renders on the fp16 instance of the same MFMA
    # kernel, for the Dex depth readout - is the leg `default_policy_fp16_render` of the line.
    if args.precision == "bf16":
        nerf.set_render_policy("bf16")
    models, cfg, ro, rd, ex, ed = build_scene(dev, rank)
    def note(msg):
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)
    note(f"scene built: {H}x{W} rays, precision {args.precision}")
    for i in range(max(args.warmup, 0)):
        out = render(models, cfg, ro, rd, ex, ed)
        torch.cuda.synchronize()
        note(f"warmup {i} done")
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = render(models, cfg, ro, rd, ex, ed)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    rays_total = world * H * W * args.steps
    value = rays_total / elapsed

    note(f"timed region: {elapsed:.3f} s for {args.steps} steps")
    if args.dump_outputs and rank == 0:
        names = dump_outputs(out, args.dump_outputs)
        note(f"outputs of the last timed step: {', '.join(names)} -> {args.dump_outputs}")
    train_dp = None
    if world > 1 and args.full and not args.no_train:
        # the data-parallel training step (BASELINE configs 4 / 5 are training configs): collective inside, so every rank runs it
        train_dp = train_rate(models, cfg, ro, rd, ex, ed, dist=dist, pose_id=7 + rank)
        note(f"data-parallel training step: {train_dp['ms_per_step']:.2f} ms, all-reduce alone {train_dp['allreduce_ms']:.3f} ms")
        train_dp["render_sharded"] = sharded_render_rate(dev, rank, dist)
        note(f"one 800x800 image over {world} ranks: {train_dp['render_sharded']['render_sharded_ms']:.1f} ms, gather alone {train_dp['render_sharded']['all_gather_ms']:.2f} ms")
    result = None
    if rank == 0:
        rdt = render_dtype()   # 'bf16' runs its no-grad renders in fp16 under the default render policy (nerf.set_render_policy)
        result = {
            "metric": "rays/sec (64+128 samples) + PSNR vs ref, 400x400 scene", "value": value, "unit": "rays/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": rdt,
            "config_dtype": args.precision, "render_dtype": rdt, "library_default_render_dtype": "fp16" if args.precision == "bf16" else rdt,
            "data": "synthetic",
            "precision_policy": {"set_precision": args.precision, "render": rdt, "train": args.precision,
                                 "what": "the headline (value, roofline, PSNR, Dex agreement) is the config's type: nerf.set_precision('bf16') + "
                                         "nerf.set_render_policy('bf16'), every kernel of the render in bf16 (rounds 1-2 reported this; round 3's "
                                         "headline was the fp16 leg).  The library's DEFAULT under set_precision('bf16') renders no-grad images - and "
                                         "what the Dex depth sweep of train_dexnerf_rgb.py:391-408 reads - on the fp16 instance of the same MFMA "
                                         "kernel, guarded against fp16's range (falls back to bf16): leg `default_policy_fp16_render`"},
            "config": {"workload": "C2 render: 400x400 rays/step/GPU, 64 coarse + 128 fine samples, coarse+fine "
                                   "FlexibleNeRFModel D8/W256/skip4 + viewdirs, PE L=10/4, 20 Dex thresholds, "
                                   "validation mode (det. resampling, no noise)",
                       "rays_per_step_per_gpu": H * W, "sharding": f"{world} ranks x own view (no collective in the path)"},
        }
        if args.full:
            full_legs(args, result, dev, rank, world, value, train_dp, models, cfg, ro, rd, ex, ed, out, note)
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def full_legs(args, result, dev, rank, world, value, train_dp, models, cfg, ro, rd, ex, ed, out, note):
    """The informational legs of `--full`, added to `result` (rank 0): the headline kernel's roofline first, then the CPU baseline and
    the legs compared with it, the other BASELINE configs, the training rates and the library-GEMM yardstick."""
    import nerf
    rdt = result["render_dtype"]
    kt, ktf = time_dominant_kernel(models, ro, rd)
    note(f"dominant kernel ({rdt}) {kt * 1e3:.2f} ms = {ktf:.0f} TFLOP/s")
    peak = PEAK_TFLOPS[rdt]
    whole_tf = value / world * POINTS_PER_RAY * FLOP_PER_POINT / 1e12
    result["roofline"] = {"bound": "mfma", "achieved": ktf, "peak": peak, "unit": "TFLOP/s", "frac": ktf / peak,
                          "traffic": pmc_record(rdt).get("hbm_bytes_per_launch"),
                          "traffic_record": pmc_record(rdt).get("record"),
                          "algorithmic_bytes": H * W * (NC + NF) * 20 + H * W * 44,
                          "matrix_pipe_busy_frac_pmc": pmc_record(rdt).get("matrix_pipe_busy_frac"),
                          "kernel": headline_kernel_name(rdt) + " (fine net, 160000x192 points)",
                          "kernel_ms": kt * 1e3, "whole_path_tflops": whole_tf}
    if train_dp is not None:
        result["train_dp"] = train_dp
    if world > 1:
        args.no_cpu_baseline = True   # the CPU baseline is reported at N=1 only
    if not args.no_cpu_baseline:
        cb, sel, ref = cpu_baseline()
        result["cpu_baseline"] = cb
        rgb = out[3].reshape(-1, 3)[torch.from_numpy(sel).to(dev)].cpu().numpy()
        mse = float(np.mean((rgb - ref[3].numpy()) ** 2))
        result["psnr_vs_oracle_db"] = float(-10.0 * np.log10(max(mse, 1e-12)))
        result["dex_vs_oracle"] = dex_agreement(out, ref, sel, dev)
        result["gpu_over_cpu"] = value / world / cb["value"]
    if args.precision == "bf16" and not args.no_cpu_baseline:
        # the same render on the library's default policy: the fp16 instance of the kernel (range-guarded), round 3's headline
        nerf.set_render_policy(None)
        try:
            render(models, cfg, ro, rd, ex, ed)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                out16 = render(models, cfg, ro, rd, ex, ed)
            torch.cuda.synchronize()
            dt16 = (time.perf_counter() - t1) / 3
            kt16, ktf16 = time_dominant_kernel(models, ro, rd, reps=3)
            rgb16 = out16[3].reshape(-1, 3)[torch.from_numpy(sel).to(dev)].cpu().numpy()
            mse16 = float(np.mean((rgb16 - ref[3].numpy()) ** 2))
            result["default_policy_fp16_render"] = {"value": H * W / dt16, "unit": "rays/s", "dtype": render_dtype(), "kernel_ms": kt16 * 1e3,
                                                    "tflops": ktf16, "frac": ktf16 / PEAK_TFLOPS["fp16"],
                                                    "kernel": headline_kernel_name(render_dtype()),
                                                    "traffic": pmc_record(render_dtype()).get("hbm_bytes_per_launch"),
                                                    "traffic_record": pmc_record(render_dtype()).get("record"),
                                                    "psnr_vs_oracle_db": float(-10.0 * np.log10(max(mse16, 1e-12))),
                                                    "dex_vs_oracle": dex_agreement(out16, ref, sel, dev)}
        finally:
            nerf.set_render_policy("bf16")
    if args.precision == "bf16" and not args.no_cpu_baseline:
        # the same render in the exact-fp32 parity mode (north_star's 1e-4 tolerance holds in this mode only): 3 steps
        nerf.set_precision("fp32")
        try:
            render(models, cfg, ro, rd, ex, ed)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                out32 = render(models, cfg, ro, rd, ex, ed)
            torch.cuda.synchronize()
            dt32 = (time.perf_counter() - t1) / 3
            kt32, ktf32 = time_dominant_kernel(models, ro, rd, "fp32", reps=2)
            rgb32 = out32[3].reshape(-1, 3)[torch.from_numpy(sel).to(dev)].cpu().numpy().astype(np.float64)
            per_ray = np.abs(rgb32 - ref[3].numpy()).max(-1) / np.abs(ref[3].numpy()).max()
            # max over 16,384 rays sits on a handful of rays where an ulp in sigma moves a resampled depth: two fp32-level
            # evaluations of the reference itself differ by 6.0e-4 there (3 rays over 1e-4, p99.9 9.4e-6:
            # profiles/r02_fp32_noise_floor.md); the 1e-4 gate of the parity tests is on the golden rays
            result["fp32_mode"] = {"value": H * W / dt32, "unit": "rays/s", "kernel_ms": kt32 * 1e3, "tflops": ktf32,
                                   "peak": PEAK_TFLOPS["fp32"], "frac": ktf32 / PEAK_TFLOPS["fp32"],
                                   "rgb_fine_rel_err_vs_oracle": {"max": float(per_ray.max()), "p99_9": float(np.quantile(per_ray, 0.999)),
                                                                  "rays_over_1e-4": int((per_ray > 1e-4).sum()), "rays": int(per_ray.size)},
                                   "dex_vs_oracle": dex_agreement(out32, ref, sel, dev)}
        finally:
            nerf.set_precision(args.precision)
    if world == 1 and not args.no_cpu_baseline:
        # BASELINE configs[2] (Dex-NeRF transparent-object scene on the as-shipped 4 x 128 nets: 270x480 after the fork's half-res
        # rule, 64+64, near 0.3 / far 4 - config/messytable-obj-remote.yml) and configs[3] as a single-GPU render (800x800, 64+192,
        # D8/W256), 3 images each, with the fine-net launch's own roofline
        kw_shipped = dict(MODEL_KW, num_layers=4, hidden_size=128)
        result["c3_render"] = other_config_render(dev, rank, "C3 render: 270x480, 64+64 samples, 4x128 nets (as shipped), near 0.3 far 4",
                                                  270, 480, 64, 64, kw_shipped, 167680, 0.3, 4.0)
        result["c4_render"] = other_config_render(dev, rank, "C4 render: 800x800, 64+192 samples, D8/W256 nets",
                                                  800, 800, 64, 192, MODEL_KW, FLOP_PER_POINT, 2.0, 6.0)
        result["c3_render_128_192"] = other_config_render(dev, rank, "C3 render, the fork's second sampling (config/messytable-obj-edward.yml:136-138): "
                                                          "270x480, 128+192 samples, 4x128 nets, near 0.3 far 4", 270, 480, 128, 192, kw_shipped, 167680, 0.3, 4.0)
        note(f"C3 {result['c3_render']['value'] / 1e6:.2f} M rays/s ({result['c3_render']['frac']:.3f} of peak), "
             f"C3 128+192 {result['c3_render_128_192']['value'] / 1e6:.2f} M rays/s ({result['c3_render_128_192']['frac']:.3f}), "
             f"C4 {result['c4_render']['value'] / 1e6:.2f} M rays/s ({result['c4_render']['frac']:.3f})")
        # BASELINE configs[4] as configured: the IR scene's 128 + 256 samples in exact fp32 (train_dexnerf_ir.py; D8/W256 nets on the
        # MessyTable frame, 270x480) - one image; its training step (luminance loss head, train_nerf_ir.py:260-263) below
        nerf.set_precision("fp32")
        try:
            result["c5_render"] = other_config_render(dev, rank, "C5 render: 270x480, 128+256 samples, D8/W256 nets, exact fp32, near 0.3 far 4",
                                                      270, 480, 128, 256, MODEL_KW, FLOP_PER_POINT, 0.3, 4.0, steps=1)
            if not args.no_train:
                m5, cfg5, ro5, rd5, _, _ = build_scene(dev, rank, 270, 480, 128, 256, MODEL_KW, 0.3, 4.0)
                result["c5_train"] = train_rate(m5, cfg5, ro5, rd5, ex, ed, n_rays=1024, steps=4, nc=128, nf=256, luminance=True, h=270, w=480,
                                                near=0.3, far=4.0, what_tail="128+256 samples, perturb + noise 0.2, D8/W256 x2, exact fp32, "
                                                "IR loss head (MSE on the luminance of both passes: train_nerf_ir.py:260-263)")
        finally:
            nerf.set_precision(args.precision)
        note(f"C5 render {result['c5_render']['value'] / 1e6:.3f} M rays/s ({result['c5_render']['frac']:.3f} of the fp32 peak)")
    if not args.no_train and world == 1:
        result["train"] = train_rate(models, cfg, ro, rd, ex, ed)
    if not args.no_train and world == 1 and args.precision == "bf16":
        # the same iteration with the tensors saved for the backward at 16 bits on the 32-point training kernels (what 'bf16' meant up to
        # round 3; 'bf16' now saves at 8 bits on the 48-point kernels - same forward bits; HISTORY.md section 4.6)
        nerf.set_precision("bf16-s16")
        try:
            models16, cfg16, _, _, _, _ = build_scene(dev, rank)
            result["train_s16_mode"] = train_rate(models16, cfg16, ro, rd, ex, ed)
        finally:
            nerf.set_precision(args.precision)
        # the same iteration in the exact-fp32 parity mode (BASELINE config 5 trains in fp32): informational
        nerf.set_precision("fp32")
        try:
            models32, cfg32, _, _, _, _ = build_scene(dev, rank)
            result["train_fp32_mode"] = train_rate(models32, cfg32, ro, rd, ex, ed, steps=4)
        finally:
            nerf.set_precision(args.precision)
        # BASELINE config 3 as a shape: the as-shipped 4 x 128 nets, 1024 rays per step, 64+64 samples, whole iteration
        # replayed as one HIP graph by the build-owned driver (informational; a few seconds)
        try:
            sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
            import train_dexnerf
            for key, prec in (("train_as_shipped", "bf16"), ("train_as_shipped_s16_mode", "bf16-s16")):
                res = train_dexnerf.main(["--iters", "4000", "--size", "64", "--views", "8", "--num-random-rays", "1024", "--layers", "4",
                                          "--width", "128", "--num-fine", "64", "--validate-every", "0", "--quiet", "--precision", prec])
                result[key] = {"rays_per_s": res["rays_per_s"], "rays_per_step": 1024, "final_train_psnr_db": res["history"][-1][2],
                               "steady_ms_per_iter": res.get("steady_ms_per_iter"),
                               "steady_rays_per_s": 1024.0 / (res["steady_ms_per_iter"] * 1e-3) if res.get("steady_ms_per_iter") else None,
                               "hip_graphs_per_iter": res.get("hip_graphs"),
                               "what": f"train_dexnerf.py --precision {prec}, 4x128 nets, 64+64 samples, nerf.FusedTrainStep + nerf.FlatAdam "
                                       "replayed as one HIP graph; rays_per_s over all 4000 iterations incl. the eager ones and the capture, "
                                       "steady_*: from iteration 20 on"}
        except Exception as exc:  # noqa: BLE001
            result["train_as_shipped"] = {"error": f"{type(exc).__name__}: {exc}"}
        finally:
            nerf.set_precision(args.precision)
    if world == 1 and not args.no_cpu_baseline and not args.no_train:
        result["train_psnr_vs_oracle"] = train_psnr_vs_oracle(dev, precision=args.precision)
        note(f"training PSNR at the last mark: {result['train_psnr_vs_oracle']['marks'][-1]}")
    result["roofline"]["library_gemm"] = library_gemm_tflops(dev, rdt)


if __name__ == "__main__":
    main()
