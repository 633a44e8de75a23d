"""Developer timing probe: forward + backward of run_network_fused_rays with ray rows that require grad (pose / ray optimisation),
on the fused route (_train.FusedNetInputFn: dn_run_network_train, dn_mlp_backward_data, dn_mlp_backward_input, and the weight-gradient
launch when the weights are not frozen) and on the retained torch route (_train._modules_on_points: torch encodings + nn.Linear
autograd), same process, same inputs, fused route first.  HIP events, `--warmup` untimed iterations, the median of `--iters`.

    python scripts/input_grad_time.py [--out profiles/input_grad_time.json]

Shapes: 4096 rays x 192 samples on D8/W256 (fp32, bf16-s16), 1024 x 128 on the as-shipped 4 x 128 nets; weights frozen and unfrozen.
Also times dn_mlp_backward_input alone and reports its achieved bytes/s (kernel_bytes_per_point: gradient slots, depths, the per-point
results written and read back by the reduction, d_z) against the 6.29 TB/s copy rate.  One JSON line per measurement, then a markdown table."""
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
from nerf import _ops, _train, synthetic as syn  # noqa: E402

COPY_RATE = 6.29e12
NETS = {
    "D8/W256": dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
    "4x128": dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True),
}
SHAPES = [("D8/W256", 4096, 192, "fp32"), ("D8/W256", 4096, 192, "bf16-s16"), ("4x128", 1024, 128, "fp32"), ("4x128", 1024, 128, "bf16-s16")]


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


def kernel_bytes_per_point(model, prec):
    """HBM bytes per point of dn_mlp_backward_input in the rays form, both launches.  The ray row (44 B per ray, shared by its S
    samples and served from cache) and the transposed weight stream (once per workgroup) are left out: the figure is a lower bound
    of the traffic, so the bytes/s it gives is a lower bound too."""
    elem = 4 if prec == "fp32" else 2
    vd = 1 if model.use_viewdirs else 0
    grad_values = model.hidden_size * (1 + len(model.skip_layers)) + vd * model.hidden_size // 2   # layer1 + wide layers + layers_dir.0
    grad_read = grad_values * elem          # main launch: the gradient slots, once
    z_read_main = 4                         # main launch: the depth (the point is ro + rd z)
    per_point_write = 12 + 12 * vd          # main launch: d_pts + per-point d_viewdir into the workspace
    per_point_reread = per_point_write      # reduction: reads them back
    z_read_reduce = 4                       # reduction: the depth again (d_rd = sum z d_pts)
    d_z_write = 4                           # reduction: d_z
    return grad_read + z_read_main + per_point_write + per_point_reread + z_read_reduce + d_z_write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.warmup >= 3 and args.iters >= 10
    dev = torch.device("cuda:0")
    rows = []
    for net, n_rays, s, prec in SHAPES:
        nerf.set_precision(prec)
        kw = NETS[net]
        model = nerf.models.FlexibleNeRFModel(**kw)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(43, sigma_bias=-20.0, **kw).items()})
        model = model.to(dev)
        torch.manual_seed(0)
        ro = torch.randn(n_rays, 3, device=dev) * 0.3
        rd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
        rays0 = torch.cat([ro, rd, torch.full((n_rays, 1), 2.0, device=dev), torch.full((n_rays, 1), 6.0, device=dev), rd], -1)
        z = (2.0 + 4.0 * torch.rand(n_rays, s, device=dev)).sort(-1).values
        g_up = torch.randn(n_rays, s, 4, device=dev)
        for frozen in (True, False):
            for p in model.parameters():
                p.requires_grad_(not frozen)

            def step():
                model.zero_grad(set_to_none=True)
                rays = rays0.clone().requires_grad_(True)
                (_train.run_network_fused_rays(model, rays, z) * g_up).sum().backward()
                return rays.grad
            fused_ms = timed(step, args.warmup, args.iters)
            g_fused = step()
            keep = _train.train_fused_ok
            _train.train_fused_ok = lambda m: False       # the retained route: _modules_on_points, code unchanged
            try:
                torch_ms = timed(step, args.warmup, args.iters)
                g_torch = step()
            finally:
                _train.train_fused_ok = keep
            cos = float(torch.nn.functional.cosine_similarity(g_fused[:, :6].reshape(-1).double(), g_torch[:, :6].reshape(-1).double(), dim=0))
            row = dict(probe="input_grad_time", net=net, rays=n_rays, samples=s, precision=prec, weights="frozen" if frozen else "trained",
                       fused_ms=fused_ms, torch_ms=torch_ms, ratio=torch_ms / fused_ms, cos_d_rays_fused_vs_torch=cos)
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the kernel alone
        pk = _train._packed_core(model, True, True)
        _ops.ensure_backward_stream(model, pk, pk.precision)
        _ops.ensure_input_grad_stream(model, pk)
        n = n_rays * s
        out, act, masks = _ops.run_network_train(pk, None, None, None, rays=rays0, z_vals=z, prec=pk.precision)
        grads = _ops.mlp_backward_data(pk, g_up.reshape(-1, 4), masks, n, prec=pk.precision)
        k_ms = timed(lambda: _ops.mlp_backward_input(pk, grads, n_rays, s, rays=rays0, z_vals=z), args.warmup, args.iters)
        bpp = kernel_bytes_per_point(model, prec)
        row = dict(probe="input_grad_kernel", net=net, rays=n_rays, samples=s, precision=prec, kernel_ms=k_ms, bytes_per_point=bpp,
                   bytes_per_s=bpp * n / (k_ms * 1e-3), fraction_of_copy_rate=bpp * n / (k_ms * 1e-3) / COPY_RATE)
        rows.append(row)
        print(json.dumps(row), flush=True)
    nerf.set_precision("fp32")
    print("\n| net | rays x samples | precision | weights | fused ms | torch route ms | ratio |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if r["probe"] == "input_grad_time":
            print(f"| {r['net']} | {r['rays']} x {r['samples']} | {r['precision']} | {r['weights']} | {r['fused_ms']:.3f} | {r['torch_ms']:.3f} | {r['ratio']:.1f} |")
    print("\n| net | rays x samples | precision | dn_mlp_backward_input ms | B/point | TB/s | of 6.29 TB/s |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if r["probe"] == "input_grad_kernel":
            print(f"| {r['net']} | {r['rays']} x {r['samples']} | {r['precision']} | {r['kernel_ms']:.3f} | {r['bytes_per_point']} | "
                  f"{r['bytes_per_s'] / 1e12:.2f} | {100 * r['fraction_of_copy_rate']:.0f} % |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
