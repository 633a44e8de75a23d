"""Developer timing probe: the training iteration of the shipped fern shape (4 x 128 nets, L_xyz = 6, 64 + 64 samples, 4096 rays per step,
NDC rays, the default 'bf16' precision) through train_dexnerf.py --llff on a small forward-facing capture of a teacher scene.

    python scripts/fern_step_time.py fused        nerf.FusedTrainStep replayed as one HIP graph (GraphedTrainStep)
    python scripts/fern_step_time.py autograd     --autograd-step (torch composition + autograd over the fused network kernels)
    python scripts/fern_step_time.py aten         the route these nets took before the fused kernels covered L_xyz = 6: --autograd-step
                                                  with the training gate closed, i.e. nn.Linear autograd on library GEMMs + torch encodings

Each mode runs the driver `--repeats` times (120 iterations, the last 100 timed: steady_ms_per_iter) and prints one JSON line with
the median; run every mode as its own process under its own time limit."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
import nerf  # noqa: E402
import train_dexnerf  # noqa: E402
from nerf import synthetic as syn  # noqa: E402

FERN = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4, use_viewdirs=True)


def write_capture(root, dev, h=120, w=160, f=150.0):
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    teacher = []
    for seed, bias in ((42, -150.0), (43, -20.0)):
        m = nerf.models.FlexibleNeRFModel(**FERN)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=bias, **FERN).items()})
        teacher.append(m.to(dev))
    mode = dict(chunksize=65536, lindisp=False, num_coarse=64, num_fine=64, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(6), nerf.get_embedding_function(4)
    rows = []
    k = 0
    for y in (-0.4, 0.0, 0.4):
        for x in (-0.5, -0.15, 0.15, 0.5):
            c2w = np.eye(4, dtype=np.float32)
            c2w[:3, 3] = [x, y, 4.0]
            ro, rd = nerf.get_ray_bundle(h, w, f, torch.from_numpy(c2w).to(dev))
            with torch.no_grad():
                out = nerf.run_one_iter_of_nerf(h, w, f, teacher[0], teacher[1], ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                encode_direction_fn=ed)
            Image.fromarray((out[3].cpu().numpy().clip(0, 1) * 255 + 0.5).astype(np.uint8)).save(os.path.join(root, "images", f"{k:02d}.png"))
            block = np.stack([-c2w[:3, 1], c2w[:3, 0], c2w[:3, 2], c2w[:3, 3], np.array([h, w, f], dtype=np.float32)], axis=1)
            rows.append(np.concatenate([block.reshape(-1), [2.0, 6.0]]))
            k += 1
    np.save(os.path.join(root, "poses_bounds.npy"), np.stack(rows).astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["fused", "autograd", "aten"])
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    built = []
    orig_init = nerf.FusedTrainStep.__init__

    def spy(self, *a, **kw):
        built.append(True)
        orig_init(self, *a, **kw)
    nerf.FusedTrainStep.__init__ = spy
    if args.mode == "aten":
        from nerf import fused_step, train_utils
        train_utils.train_fused_ok = fused_step.train_fused_ok = lambda model: False
    runs = []
    with tempfile.TemporaryDirectory() as root:
        write_capture(root, dev)
        argv = ["--llff", root, "--llff-factor", "1", "--llffhold", "6", "--iters", str(args.iters), "--num-random-rays", str(args.rays),
                "--layers", "4", "--width", "128", "--num-coarse", "64", "--num-fine", "64", "--validate-every", "0", "--quiet",
                "--precision", "bf16", "--xyz-freqs", "6"] + ([] if args.mode == "fused" else ["--autograd-step"])
        for _ in range(args.repeats):
            res = train_dexnerf.main(argv)
            runs.append(res["steady_ms_per_iter"])
            psnr = (res["history"][0][2], res["history"][-1][2])
    med = statistics.median(runs)
    line = dict(probe="fern_step_time", mode=args.mode, fused_step=bool(built), rays_per_step=args.rays, samples="64+64", nets="4x128 L_xyz=6",
                ndc=True, precision="bf16", ms_per_iter_runs=runs, ms_per_iter_median=med, rays_per_s_median=args.rays / med * 1e3,
                train_psnr_first_last=psnr, device=torch.cuda.get_device_name(0))
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
