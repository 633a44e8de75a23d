#!/usr/bin/env python3
"""Build-owned training / evaluation driver (counterpart of the reference's train_dexnerf_rgb.py:178-457 and
eval_nerf.py:166-206) on the MI355X-native `nerf` package.

What it keeps from the reference loop: one random training view per iteration, `num_random_rays` random pixels,
loss = MSE(rgb_coarse) + MSE(rgb_fine) (or, with --ir, on the luminance of both: train_nerf_ir.py:260-263), PSNR = mse2psnr(loss), Adam with the per-iteration exponential LR
`lr0 * factor^(i / (lr_decay * 1000))`, validation renders with the Dex threshold sweep
(`m_thres_cand = arange(5, m_thres + 5, 5)`, best threshold by mean |depth error| on the (0, 1.25 m] mask-style
validity mask), and the checkpoint dict keys (iter, model_*_state_dict, optimizer_state_dict, loss, psnr).
What it adds: data-parallel training (one process per GPU under torch.distributed.run; one flat-bucket gradient
all-reduce per step) and a synthetic "teacher" scene, because no dataset ships with the reference: a fixed random
coarse/fine FlexibleNeRFModel pair is rendered from spherical poses and the student learns to reproduce it.

    python dex-nerf_amd/train_dexnerf.py --iters 2000 --size 100 --precision bf16
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 dex-nerf_amd/train_dexnerf.py ...
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import nerf  # noqa: E402
from nerf import parallel, synthetic as syn  # noqa: E402


def make_cfg(args):
    def mode(train):
        return dict(chunksize=args.chunksize, lindisp=False, num_coarse=args.num_coarse, num_fine=args.num_fine,
                    perturb=train, radiance_field_noise_std=args.noise_std if train else 0.0, white_background=False)
    return nerf.CfgNode(dict(dataset=dict(near=args.near, far=args.far, no_ndc=not getattr(args, "ndc", False)),
                             nerf=dict(use_viewdirs=True, train=mode(True), validation=mode(False))))


def build_models(kw, dev, state=None):
    out = []
    for i in range(2):
        m = nerf.models.FlexibleNeRFModel(**kw)
        if state is not None:
            m.load_state_dict({k: torch.from_numpy(v) for k, v in state[i].items()})
        out.append(m.to(dev))
    return out


def render_view(models, cfg, pose, k_mat, hw, ex, ed, thres, mode="validation"):
    h, w = hw
    ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), pose, k_mat)
    with torch.no_grad():
        return nerf.run_one_iter_of_nerf(h, w, float(k_mat[0, 0]), models[0], models[1], ro, rd, cfg, mode=mode,
                                         encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=thres)


def dex_sweep(outputs, depth_gt, thres, gt_hi=6.0):
    """Pick the Dex threshold with the smallest mean |depth error| (reference train_dexnerf_rgb.py:391-408): all
    candidates in one kernel + one copy (nerf.dex_error_sweep).  Ground mask 0 < gt < gt_hi (the reference: 1.25 m for
    its table-top scenes; the built-in synthetic scene spans (0, 6) m)."""
    best, errs = nerf.dex_error_sweep(depth_gt, list(outputs[6:]), gt_lo=0.0, gt_hi=gt_hi)
    best = int(np.argmin([e["depth_abs_err"] for e in errs])) if best is None else best
    return thres[best], errs[best]


def parse_quantiles(text):
    """'0.1,0.5,0.9' -> the opacity quantiles of --val-quantiles / eval_nerf.py --depth-quantiles, under the library's host-side rule
    (finite, strictly inside (0, 1), at most 64): ValueError otherwise."""
    from nerf import _ops
    return _ops.check_quantiles([float(q) for q in text.split(",") if q.strip()], "quantiles")


def quantile_sweep(models, cfg, pose, k_mat, hw, ex, depth_gt, quantiles, gt_hi=6.0):
    """--val-quantiles: one depth-only render of the view with the opacity-quantile depth maps (nerf.render_dex_depth), scored like
    the Dex thresholds (nerf.dex_error_sweep, the same mask and metric): (best quantile, its error record)."""
    h, w = hw
    ro, rd = nerf.get_ray_bundle(h, w, float(k_mat[0, 0]), pose, k_mat)
    with torch.no_grad():
        out = nerf.render_dex_depth(h, w, float(k_mat[0, 0]), models[0], models[1], ro, rd, cfg, mode="validation",
                                    encode_position_fn=ex, quantiles=quantiles)
    best, errs = nerf.dex_error_sweep(depth_gt, list(out[4:]), gt_lo=0.0, gt_hi=gt_hi)
    best = int(np.argmin([e["depth_abs_err"] for e in errs])) if best is None else best
    return quantiles[best], errs[best]


def synthetic_dataset(args, kw, cfg, ex, ed, thres, dev):
    """No dataset ships with the reference: a fixed random coarse/fine FlexibleNeRFModel pair ("teacher") is rendered from
    `views` + 1 spherical poses; the last pose is held out."""
    hw = (args.size, args.size)
    k_mat = torch.from_numpy(syn.intrinsic(*hw)).to(dev)
    poses = [torch.from_numpy(syn.scene_pose(i, n_views=args.views + 1)).to(dev) for i in range(args.views + 1)]
    teacher = build_models(kw, dev, (syn.synth_state_dict(42, sigma_bias=-150.0, **kw), syn.synth_state_dict(43, sigma_bias=-20.0, **kw)))
    images, depths = [], []
    for pose in poses:
        out = render_view(teacher, cfg, pose, k_mat, hw, ex, ed, thres)
        images.append(out[3].reshape(-1, 3))
        depths.append(out[4].reshape(hw))
    return dict(hw=hw, poses=poses, intrinsics=[k_mat] * len(poses), images=images, depths=depths,
                train=list(range(args.views)), val=args.views, mask_hi=6.0)


def messytable_dataset(args, dev):
    """A scene directory in the reference's MessyTable / Dex-NeRF layout (nerf/load_messytable.py; `half_res` = the
    fork's 270 x 480 training resolution with the principal point pinned to (240, 135))."""
    imgs, poses, _, hwf, i_split, intrinsics, depths = nerf.load_messytable_data(
        args.messytable, half_res=True, imgname=args.imgname, is_real_rgb=args.real_rgb)
    hw = (int(hwf[0]), int(hwf[1]))
    n = imgs.shape[0]
    val = int(i_split[1][0]) if len(i_split[1]) else int(i_split[0][-1])
    return dict(hw=hw, poses=[poses[i].to(dev) for i in range(n)], intrinsics=[intrinsics[i].to(dev) for i in range(n)],
                images=[imgs[i, ..., :3].reshape(-1, 3).to(dev) for i in range(n)], depths=[depths[i].to(dev) for i in range(n)],
                train=[int(i) for i in i_split[0]], val=val, mask_hi=1.25)


def llff_dataset(args, dev):
    """A forward-facing capture in the LLFF layout (nerf/llff.py; reference nerf/load_llff.py + the LLFF branch of
    train_nerf_rgb.py:70-95): camera-to-world poses in NeRF's (right, up, back) frame with a shared pinhole (f, W/2, H/2).
    The kernels take the fork's convention - a world-to-camera extrinsic in OpenCV axes plus a 3x3 K (nerf_helpers.py:67-112:
    dir = [(i-cx)/fx, (j-cy)/fx, 1], rd = inv(E[:3,:3]) dir, ro = inv(E)[:3,3]) - so E = inv([R diag(1,-1,-1) | t])."""
    images, poses, bds, _, i_test = nerf.load_llff_data(args.llff, factor=args.llff_factor)
    h, w, f = int(poses[0, 0, 4]), int(poses[0, 1, 4]), float(poses[0, 2, 4])
    k_mat = torch.tensor([[f, 0.0, w * 0.5], [0.0, f, h * 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    flip = np.diag([1.0, -1.0, -1.0])
    extr = []
    for c2w in poses[:, :3, :4].astype(np.float64):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = c2w[:, :3] @ flip, c2w[:, 3]
        extr.append(torch.from_numpy(np.linalg.inv(m).astype(np.float32)).to(dev))
    n = images.shape[0]
    hold = list(range(n))[::args.llffhold] if args.llffhold > 0 else [int(i_test)]
    train = [i for i in range(n) if i not in hold] or [int(i_test)]
    return dict(hw=(h, w), poses=extr, intrinsics=[k_mat] * n, images=[torch.from_numpy(images[i].reshape(-1, 3)).to(dev) for i in range(n)],
                depths=[None] * n, train=train, val=hold[0], mask_hi=None, focal=f,
                bounds=(float(bds.min()) * 0.9, float(bds.max()) * 1.0))


JOINT_KEY = "joint_step_state_dict"      # checkpoint key of nerf.FusedJointStep.state_dict() (--refine-poses)


def pose_distance(extrinsics, reference):
    """(mean rotation angle in degrees, mean distance of the camera centres) between two (V,4,4) sets of world->camera extrinsics."""
    a, b = extrinsics.detach().double().cpu(), reference.detach().double().cpu()
    rel = a[:, :3, :3] @ b[:, :3, :3].transpose(1, 2)
    cos = (rel.diagonal(dim1=1, dim2=2).sum(-1) - 1.0) * 0.5
    skew = torch.stack([rel[:, 2, 1] - rel[:, 1, 2], rel[:, 0, 2] - rel[:, 2, 0], rel[:, 1, 0] - rel[:, 0, 1]], dim=1)
    angle = torch.atan2(skew.norm(dim=1) * 0.5, cos)      # (well conditioned at 0, where acos is not)
    centre = lambda e: -(e[:, :3, :3].transpose(1, 2) @ e[:, :3, 3:]).squeeze(-1)  # noqa: E731
    return float(torch.rad2deg(angle).mean()), float((centre(a) - centre(b)).norm(dim=1).mean())


def perturbed_poses(extrinsics, rot, trans, seed, keep=()):
    """--pose-noise: E_v <- se3_exp(xi_v) E_v with seeded twists, |omega_v| = rot (radians), |t_v| = trans, directions uniform on the
    sphere; the views in `keep` (the gauge: --fix-views) stay as given.  (V,4,4) fp32 on the device of `extrinsics`."""
    gen = torch.Generator().manual_seed(int(seed))
    n = int(extrinsics.shape[0])
    unit = lambda: torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=1)  # noqa: E731
    xi = torch.cat([unit() * float(rot), unit() * float(trans)], dim=1)
    host = extrinsics.detach().double().cpu()
    out = [host[v] if v in keep else nerf.se3_exp(xi[v]) @ host[v] for v in range(n)]
    return torch.stack(out).to(extrinsics.device, torch.float32)


def joint_checkpoint_entries(joint, train_ids, extrinsics0):
    """What --refine-poses adds to the checkpoint dict: the step's state, and the cameras as plain host tensors for other tools (eval_nerf.py --use-refined-poses)."""
    entries = {JOINT_KEY: joint.state_dict(), "refined_views": [int(v) for v in train_ids],
               "refined_extrinsics": joint.extrinsics().cpu(), "refined_intrinsics": joint.intrinsics().cpu(),
               "joint_initial_extrinsics": extrinsics0.detach().cpu()}
    if joint.exposure_mode is not None:      # --refine-exposure: the rows (V,P) with what nerf.apply_exposure needs to read them
        entries.update(refined_exposure=joint.exposure().cpu(), refined_exposure_mode=joint.exposure_mode,
                       refined_exposure_scale=joint.exposure_scale)
    return entries


def restore_joint_state(ck, joint):
    """--load-checkpoint with --refine-poses: the step's state from the checkpoint dict.  False (and nothing is touched) for a
    checkpoint without the key - one written without --refine-poses, or by the reference."""
    state = ck.get(JOINT_KEY)
    if state is None:
        return False
    joint.load_state_dict(state)
    return True


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--size", type=int, default=100, help="image height = width of the synthetic views")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--num-random-rays", type=int, default=2048)
    ap.add_argument("--num-coarse", type=int, default=64)
    ap.add_argument("--num-fine", type=int, default=128)
    ap.add_argument("--chunksize", type=int, default=65536)
    ap.add_argument("--noise-std", type=float, default=0.2)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--lr-decay", type=int, default=250)
    ap.add_argument("--lr-decay-factor", type=float, default=0.1)
    ap.add_argument("--m-thres", type=int, default=100)
    ap.add_argument("--val-quantiles", default="", metavar="Q,Q,...",
                    help="at validation also render the opacity-quantile depth maps (one nerf.render_dex_depth with these quantiles, e.g. "
                         "0.1,0.5,0.9) and log the best quantile and its depth error beside the best Dex threshold; off by default")
    ap.add_argument("--ir", action="store_true", help="IR head of train_nerf_ir.py / train_dexnerf_ir.py: MSE on the luminance "
                                                      "0.299 r + 0.587 g + 0.114 b of prediction and target (:260-263)")
    ap.add_argument("--s8-grad-scale", type=float, default=None,
                    help="bf16: power of two the 8-bit saved layer gradients are scaled by; default 0 = chosen per launch from the "
                         "largest upstream gradient (nerf.set_s8_grad_scale)")
    ap.add_argument("--atomic-weight-gradients", action="store_true",
                    help="add the weight-gradient partials with fp32 atomics (no scratch buffer, a few percent faster on small nets) instead "
                         "of the fixed-order reduction: a run is then no longer reproducible bit for bit")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16-s8", "bf16-s16", "fp32"],
                    help="bf16 (= bf16-s8): bf16 kernels, the tensors saved for the backward at 8 bits; bf16-s16: at 16 bits (nerf.set_precision)")
    ap.add_argument("--validate-every", type=int, default=500)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--save", default="", help="checkpoint path (reference dict format)")
    ap.add_argument("--load-checkpoint", default="")
    ap.add_argument("--messytable", default="", help="train on a scene directory in the reference's MessyTable / Dex-NeRF "
                                                     "layout instead of the built-in synthetic scene")
    ap.add_argument("--llff", default="", help="train on a forward-facing capture in the LLFF layout (poses_bounds.npy + images[_N]/); "
                                               "rays are warped to NDC like the reference's LLFF configs unless --no-ndc")
    ap.add_argument("--llff-factor", type=int, default=8, help="image downsampling factor (images_<factor>/; the reference default)")
    ap.add_argument("--llffhold", type=int, default=8, help="every N-th view is held out (0: only the view nearest the average pose)")
    ap.add_argument("--no-ndc", action="store_true", help="LLFF: keep world-space rays with the capture's depth bounds")
    ap.add_argument("--imgname", default="0128_irL_kuafu_half.png")
    ap.add_argument("--real-rgb", action="store_true")
    ap.add_argument("--near", type=float, default=None, help="default 2 (synthetic scene) / 0.3 (MessyTable)")
    ap.add_argument("--far", type=float, default=None, help="default 6 (synthetic scene) / 4 (MessyTable)")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--xyz-freqs", type=int, default=10, choices=[6, 10],
                    help="frequencies of the xyz encoding (num_encoding_fn_xyz): 10 as in the reference's blender / MessyTable configs, 6 as "
                         "in its fern / llff configs and the shipped fern-lowres checkpoint")
    ap.add_argument("--linear-freqs", action="store_true",
                    help="linearly spaced encoding frequencies for both encodings (log_sampling_xyz / _dir: False, as in llff.yml)")
    ap.add_argument("--autograd-step", action="store_true",
                    help="run the iteration as torch ops + autograd over the fused kernels (torch.randperm / rand / randn draws, mse_loss, "
                         "loss.backward()) instead of nerf.FusedTrainStep")
    ap.add_argument("--torch-adam", action="store_true",
                    help="step torch.optim.Adam (fused, multi-tensor) instead of the flat one-launch Adam of this build (nerf.FlatAdam)")
    ap.add_argument("--no-hip-graph", action="store_true",
                    help="launch every kernel of an iteration from Python instead of replaying one captured HIP graph "
                         "(single-GPU runs capture by default: the as-shipped 4x128 nets at 1024 rays are launch-bound)")
    ap.add_argument("--mix-views", action="store_true",
                    help="draw every ray's training view together with its pixel (a batch across all training images, upstream NeRF's "
                         "default; nerf.FusedTrainStep(draw_view=\"rays\")) instead of one view per iteration")
    ap.add_argument("--depth-weight", type=float, default=0.0,
                    help="weight of the depth term of the loss, coarse and fine alike: the mean squared error of the expected depth against "
                         "the dataset's depth maps over the pixels inside --depth-range (nerf.FusedTrainStep(depth_images=...)); needs a "
                         "dataset with depths (the synthetic scene, --messytable) and implies --mix-views")
    ap.add_argument("--depth-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="pixels whose depth lies strictly inside (LO, HI) are supervised; default: the Dex validation mask, 0 to the "
                         "dataset's mask_hi")
    ap.add_argument("--distortion-weight", type=float, default=0.0, metavar="W",
                    help="weight of the distortion regulariser (mip-NeRF 360) on the fine network's sample weights: it penalises density "
                         "spread out or split into clusters along a ray - floaters, which move the Dex depth "
                         "(nerf.FusedTrainStep(distortion_weights=...))")
    ap.add_argument("--distortion-weight-coarse", type=float, default=None, metavar="WC",
                    help="the regulariser's weight on the coarse network (default 0)")
    ap.add_argument("--refine-poses", action="store_true",
                    help="train the cameras of the training views together with the networks (nerf.FusedJointStep: twists on the given "
                         "poses under their own Adam, in the same replayed step); implies --mix-views.  Training views are then rendered at "
                         "their refined cameras; held-out views keep their given poses")
    ap.add_argument("--pose-lr", type=float, default=None, help="--refine-poses: learning rate of the twists (and intrinsics); default 1e-3")
    ap.add_argument("--pose-lr-decay", type=float, nargs=2, default=None, metavar=("FACTOR", "STEPS"),
                    help="--refine-poses: the pose learning rate is multiplied by FACTOR ** (iteration / STEPS)")
    ap.add_argument("--refine-intrinsics", default=None, choices=["shared", "per_view"],
                    help="--refine-poses: refine fx, cx, cy as well, one set for all training views or one per view")
    ap.add_argument("--intrinsics-scale", type=float, default=None,
                    help="--refine-intrinsics: size of an intrinsics step relative to a twist step (default 1)")
    ap.add_argument("--fix-views", type=int, nargs="+", default=None, metavar="I",
                    help="--refine-poses: training views (positions in the training set) whose poses stay as given; default 0 - with "
                         "every view free the scene can drift by a rigid motion, one fixed camera pins it")
    ap.add_argument("--refine-exposure", default=None, choices=["gain", "affine"],
                    help="--refine-poses: refine a photometric row per training view as well - one gain, or a gain and an offset per "
                         "channel - so that a view's exposure / white balance is not explained by the networks; with every view in "
                         "--fix-views (or --pose-lr 0) the run trains the networks and the exposure alone")
    ap.add_argument("--exposure-scale", type=float, default=None,
                    help="--refine-exposure: size of an exposure step relative to a twist step (default 1)")
    ap.add_argument("--fix-exposure-views", type=int, nargs="+", default=None, metavar="I",
                    help="--refine-exposure: training views (positions in the training set) whose rows stay at the identity; default 0 - a "
                         "common gain of all views is absorbed by the networks, one fixed view pins it")
    ap.add_argument("--anneal-encoding", type=int, nargs=2, default=None, metavar=("START", "END"),
                    help="coarse-to-fine positional encoding (BARF): the bands of the encodings are switched on one after the other "
                         "between iterations START and END (nerf.EncodingAnneal on the fused steps; with and without --refine-poses). The "
                         "checkpoint stores the schedule; --load-checkpoint resumes it")
    ap.add_argument("--anneal-xyz-only", action="store_true", help="--anneal-encoding: leave the view-direction encoding un-annealed")
    ap.add_argument("--train-occupancy", type=int, default=None, metavar="CELLS",
                    help="keep an occupancy grid of CELLS^3 cells live beside the networks (nerf.LiveOccupancyGrid: a decayed running maximum "
                         "of their density at one jittered point per cell, refreshed on the device) and tighten every training ray's near / "
                         "far to its occupied span (nerf.FusedTrainStep(ray_span=...)).  The checkpoint stores the grid (train_occupancy); "
                         "--load-checkpoint resumes it and eval_nerf.py --ray-span checkpoint renders with it")
    ap.add_argument("--occupancy-bounds", type=float, nargs=6, default=None, metavar=("x0", "y0", "z0", "x1", "y1", "z1"),
                    help="--train-occupancy: the grid's box in the networks' input space (required; NDC space for NDC rays)")
    ap.add_argument("--occupancy-level", type=float, default=None, metavar="L",
                    help="--train-occupancy: a cell is set while the running density exceeds L (default 0.01; >= 0)")
    ap.add_argument("--occupancy-decay", type=float, default=None, metavar="D",
                    help="--train-occupancy: the running maximum is multiplied by D at every refresh (default 0.95; in (0, 1])")
    ap.add_argument("--occupancy-every", type=int, default=None, metavar="K", help="--train-occupancy: refresh before every K-th iteration (default 16)")
    ap.add_argument("--occupancy-warmup", type=int, default=None, metavar="U",
                    help="--train-occupancy: the first U refreshes only feed the running density; the grid stays all set (default 4)")
    ap.add_argument("--ray-span-pad", type=float, default=None, metavar="P",
                    help="--train-occupancy: widen each span by P cells of travel at both ends (default 1)")
    ap.add_argument("--pose-noise", type=float, nargs=2, default=None, metavar=("ROT", "TRANS"),
                    help="perturb the loaded training poses (all but --fix-views) by seeded twists of ROT radians and TRANS scene units "
                         "before training: for experiments and tests")
    return ap


def parse_args(argv=None):
    """The command line, checked: inconsistent combinations end in the parser's error (SystemExit 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    try:      # "" (the default): no quantile render at validation
        args.val_quantiles = parse_quantiles(args.val_quantiles)
    except ValueError as e:
        ap.error(f"--val-quantiles: {e}")
    if not args.refine_poses:
        for flag, value in (("--pose-lr", args.pose_lr), ("--pose-lr-decay", args.pose_lr_decay), ("--refine-intrinsics", args.refine_intrinsics),
                            ("--intrinsics-scale", args.intrinsics_scale), ("--fix-views", args.fix_views),
                            ("--refine-exposure", args.refine_exposure), ("--exposure-scale", args.exposure_scale),
                            ("--fix-exposure-views", args.fix_exposure_views)):
            if value is not None:
                ap.error(f"{flag} needs --refine-poses")
    else:
        if args.autograd_step:
            ap.error("--refine-poses runs on the fused step (nerf.FusedJointStep), not with --autograd-step")
        if args.pose_lr is not None and not args.pose_lr >= 0.0:
            ap.error("--pose-lr must be >= 0")
        if args.pose_lr_decay is not None and not (args.pose_lr_decay[0] > 0.0 and args.pose_lr_decay[1] > 0.0):
            ap.error("--pose-lr-decay FACTOR STEPS: both > 0")
        if args.intrinsics_scale is not None and (args.refine_intrinsics is None or not args.intrinsics_scale > 0.0):
            ap.error("--intrinsics-scale needs --refine-intrinsics and must be > 0")
        if args.fix_views is not None and min(args.fix_views) < 0:
            ap.error("--fix-views: positions in the training set, >= 0")
        if args.exposure_scale is not None and (args.refine_exposure is None or not 0.0 < args.exposure_scale < float("inf")):
            ap.error("--exposure-scale needs --refine-exposure and must be > 0")
        if args.fix_exposure_views is not None and (args.refine_exposure is None or min(args.fix_exposure_views) < 0):
            ap.error("--fix-exposure-views needs --refine-exposure: positions in the training set, >= 0")
        args.exposure_scale = 1.0 if args.exposure_scale is None else args.exposure_scale
        if args.refine_exposure is not None and args.fix_exposure_views is None:
            args.fix_exposure_views = [0]
        args.pose_lr = 1e-3 if args.pose_lr is None else args.pose_lr
        args.intrinsics_scale = 1.0 if args.intrinsics_scale is None else args.intrinsics_scale
        args.fix_views = [0] if args.fix_views is None else args.fix_views
        args.mix_views = True
    if args.anneal_encoding is not None:
        if args.autograd_step:
            ap.error("--anneal-encoding runs on the fused steps (nerf.FusedTrainStep / nerf.FusedJointStep), not with --autograd-step")
        if not 0 <= args.anneal_encoding[0] <= args.anneal_encoding[1]:
            ap.error("--anneal-encoding START END: iterations with 0 <= START <= END")
    elif args.anneal_xyz_only:
        ap.error("--anneal-xyz-only needs --anneal-encoding")
    if args.pose_noise is not None and not (args.pose_noise[0] >= 0.0 and args.pose_noise[1] >= 0.0):
        ap.error("--pose-noise ROT TRANS: both >= 0")
    args.distortion_weight_coarse = 0.0 if args.distortion_weight_coarse is None else args.distortion_weight_coarse
    for flag, value in (("--distortion-weight", args.distortion_weight), ("--distortion-weight-coarse", args.distortion_weight_coarse)):
        if not 0.0 <= value < float("inf"):
            ap.error(f"{flag} must be finite and >= 0")
    if max(args.distortion_weight, args.distortion_weight_coarse) > 0.0:
        if args.refine_poses:
            ap.error("--distortion-weight does not run with --refine-poses yet: the geometry route (nerf.FusedJointStep) takes no distortion regulariser")
        if args.autograd_step:
            ap.error("--distortion-weight runs on the fused step (nerf.FusedTrainStep), not with --autograd-step")
    occupancy_flags = (("--occupancy-bounds", args.occupancy_bounds), ("--occupancy-level", args.occupancy_level),
                       ("--occupancy-decay", args.occupancy_decay), ("--occupancy-every", args.occupancy_every),
                       ("--occupancy-warmup", args.occupancy_warmup), ("--ray-span-pad", args.ray_span_pad))
    if args.train_occupancy is None:
        for flag, value in occupancy_flags:
            if value is not None:
                ap.error(f"{flag} needs --train-occupancy")
    else:
        from nerf import _ops
        if args.autograd_step or args.refine_poses:
            ap.error("--train-occupancy runs on nerf.FusedTrainStep: not with --autograd-step, and not with --refine-poses (the rewrite "
                     "of near / far cuts their gradient and the cameras move)")
        if args.anneal_encoding is not None:
            ap.error("--train-occupancy reads the networks' density without the encoding anneal's amplitudes: not with --anneal-encoding")
        if args.occupancy_bounds is None:
            ap.error("--train-occupancy needs --occupancy-bounds x0 y0 z0 x1 y1 z1")
        args.occupancy_level = 0.01 if args.occupancy_level is None else args.occupancy_level
        args.occupancy_decay = 0.95 if args.occupancy_decay is None else args.occupancy_decay
        args.occupancy_every = 16 if args.occupancy_every is None else args.occupancy_every
        args.occupancy_warmup = 4 if args.occupancy_warmup is None else args.occupancy_warmup
        args.ray_span_pad = 1.0 if args.ray_span_pad is None else args.ray_span_pad
        try:
            _ops.check_occupancy_grid(args.occupancy_bounds, args.train_occupancy, "--train-occupancy")
            _ops.check_live_occupancy(args.occupancy_level, args.occupancy_decay, 1, "--train-occupancy")
            _ops.check_ray_span_pad(args.ray_span_pad, "--ray-span-pad")
        except ValueError as e:
            ap.error(str(e))
        if args.occupancy_every < 1:
            ap.error("--occupancy-every must be >= 1")
        if args.occupancy_warmup < 0:
            ap.error("--occupancy-warmup must be >= 0")
    if args.depth_weight < 0.0:
        ap.error("--depth-weight must be >= 0")
    if args.depth_weight > 0.0:
        if args.llff:
            ap.error("--depth-weight needs a dataset with depth maps; LLFF captures carry none (and an NDC depth is not metric)")
        if args.autograd_step:
            ap.error("--depth-weight runs on the fused step (nerf.FusedTrainStep), not with --autograd-step")
        args.mix_views = True
    return args


def main(argv=None):
    args = parse_args(argv)
    user_bounds = args.near is not None or args.far is not None
    args.ndc = bool(args.llff) and not args.no_ndc
    if args.ndc:
        args.near, args.far = 0.0, 1.0        # the NDC cube (the reference's LLFF configs)
    if args.near is None:
        args.near = 0.3 if args.messytable else 2.0
    if args.far is None:
        args.far = 4.0 if args.messytable else 6.0

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)   # (rehearsals: ranks may share a GPU)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # "nccl" is RCCL on ROCm; DEXNERF_DIST_BACKEND=gloo lets the data-parallel loop be rehearsed with several ranks on
        # one GPU (RCCL refuses two ranks on the same device)
        backend = os.environ.get("DEXNERF_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    np.random.seed(args.seed + rank)          # reference seeds np + torch from cfg.experiment.randomseed (:97-99)
    torch.manual_seed(args.seed + rank)
    nerf.set_precision(args.precision)
    if args.s8_grad_scale is not None:
        nerf.set_s8_grad_scale(args.s8_grad_scale)
    from nerf import _ops as _nerf_ops
    _nerf_ops.set_deterministic_weight_gradients(not args.atomic_weight_gradients)
    s8_warned, s8_saturated_max = False, 0.0

    kw = dict(num_layers=args.layers, hidden_size=args.width, skip_connect_every=4, num_encoding_fn_xyz=args.xyz_freqs,
              num_encoding_fn_dir=4, use_viewdirs=True)
    cfg = make_cfg(args)
    ex = nerf.get_embedding_function(args.xyz_freqs, True, not args.linear_freqs)
    ed = nerf.get_embedding_function(4, True, not args.linear_freqs)
    thres = np.arange(5, args.m_thres + 5, 5)
    if args.llff:
        data = llff_dataset(args, dev)
        if not args.ndc and not user_bounds:      # world-space rays: the capture's own depth bounds
            args.near, args.far = data["bounds"]
            cfg.dataset.near, cfg.dataset.far = data["bounds"]
    else:
        data = messytable_dataset(args, dev) if args.messytable else synthetic_dataset(args, kw, cfg, ex, ed, thres, dev)
    hw, poses, intrinsics, images, depths = data["hw"], data["poses"], data["intrinsics"], data["images"], data["depths"]
    held_out = data["val"]

    torch.manual_seed(args.seed)              # identical student init on every rank
    student = build_models(kw, dev)
    parallel.broadcast_parameters(student)
    torch.manual_seed(args.seed + 1000 + rank)
    bucket = parallel.FlatGradBucket(student)
    use_graph = not args.no_hip_graph         # (world > 1: graphs around the exchange, nerf.GraphedTrainStep; the autograd step only with one rank)
    # The whole iteration on this library's kernels (nerf.FusedTrainStep: pixel draw, jitter, resampling and density noise drawn
    # inside the kernels, loss head + upstream gradients in one launch, no autograd graph) wherever the fused training kernels
    # cover the configuration - NDC rays included (the draw kernel warps them); --autograd-step keeps the torch composition
    # (torch.randperm / rand / randn, autograd).
    ndc_focal = data["focal"] if args.ndc else None
    fused_ok = (not args.autograd_step
                and nerf.FusedTrainStep.applicable(student[0], student[1], cfg, ex, ed, args.num_random_rays, ndc_focal))
    flat_adam = fused_ok and not args.torch_adam
    lr_t = torch.tensor(args.lr, dtype=torch.float32, device=dev)   # (torch's Adam) a device scalar: the schedule is applied by fill_()
    if flat_adam:
        # Adam over ONE flat parameter buffer: one launch, the learning-rate schedule evaluated inside it, the gradients cleared
        # in the same pass (reference: torch.optim.Adam + zero_grad + the schedule, train_dexnerf_rgb.py:146-148, 280-289)
        opt = nerf.FlatAdam(bucket, lr=args.lr, lr_decay_factor=args.lr_decay_factor, lr_decay_steps=args.lr_decay * 1000, zero_grads=True)
    else:
        opt = torch.optim.Adam(bucket.params, lr=lr_t, fused=True, capturable=True)
    start = 0
    if args.load_checkpoint:
        ck = torch.load(args.load_checkpoint, map_location=dev)
        student[0].load_state_dict(ck["model_coarse_state_dict"])
        student[1].load_state_dict(ck["model_fine_state_dict"])
        nerf.models.mark_parameters_updated()
        opt.load_state_dict(ck["optimizer_state_dict"])
        if not flat_adam:
            for group in opt.param_groups:
                group["lr"] = lr_t
        start = ck["iter"]
    # the coarse-to-fine schedule of the encodings: the command line's, else the one a loaded checkpoint was saved inside.  It follows
    # the iteration counter of the fused step's RNG record (first_iteration=start), so resuming needs nothing else
    anneal = None
    if args.anneal_encoding is not None:
        anneal = nerf.EncodingAnneal(args.anneal_encoding[0], args.anneal_encoding[1], anneal_dir=not args.anneal_xyz_only)
    elif args.load_checkpoint and ck.get("encoding_anneal") is not None and not args.autograd_step:
        anneal = nerf.EncodingAnneal.from_state_dict(ck["encoding_anneal"])
    if anneal is not None and not fused_ok:
        raise SystemExit("--anneal-encoding: this configuration is outside the fused steps (see FusedTrainStep.applicable)")
    train_ids = data["train"][rank::world] or [data["train"][rank % len(data["train"])]]
    # All training cameras + images live on the device and the view is a device scalar: from pixel draws to packed ray rows
    # + target pixels is ONE kernel with no per-view host constant (reference: full-image bundle + coordinate grid + three
    # gathers + normalise + cat per step), so the whole iteration can be captured once and replayed for any view.
    selector = nerf.MultiViewRaySelector(hw[0], hw[1], [poses[v] for v in train_ids], [intrinsics[v] for v in train_ids],
                                         args.near, args.far,
                                         images=torch.stack([images[v].reshape(hw[0], hw[1], 3) for v in train_ids]), device=dev)
    loss_t = torch.zeros((), dtype=torch.float32, device=dev)
    fused = None
    # the occupancy grid that lives beside the networks: the command line's, or - resuming - the one the checkpoint stored, which goes
    # on with the same draws.  Every rank keeps its own copy, refreshed from bit-identical weights and the grid's own seed: no exchange
    live = None
    if args.train_occupancy is not None:
        if not fused_ok:
            raise SystemExit("--train-occupancy: this configuration is outside nerf.FusedTrainStep (see FusedTrainStep.applicable)")
        if args.load_checkpoint and ck.get("train_occupancy") is not None:
            live = nerf.LiveOccupancyGrid.from_state_dict(ck["train_occupancy"], dev)
        else:
            live = nerf.LiveOccupancyGrid(args.occupancy_bounds, args.train_occupancy, dev, level=args.occupancy_level,
                                          decay=args.occupancy_decay, warmup_updates=args.occupancy_warmup, seed=args.seed)
    head = {}
    if args.depth_weight > 0.0:
        if not fused_ok:
            raise SystemExit("--depth-weight: this configuration is outside nerf.FusedTrainStep (see FusedTrainStep.applicable)")
        head = dict(depth_images=torch.stack([depths[v].reshape(hw).to(torch.float32) for v in train_ids]),
                    depth_weights=(args.depth_weight, args.depth_weight),
                    depth_range=tuple(args.depth_range) if args.depth_range else (0.0, float(data["mask_hi"])))
    distortion = (args.distortion_weight_coarse, args.distortion_weight)
    if max(distortion) > 0.0 and not fused_ok:
        raise SystemExit("--distortion-weight: this configuration is outside nerf.FusedTrainStep (see FusedTrainStep.applicable)")
    joint = given_extrinsics = extrinsics0 = None
    if args.refine_poses or args.pose_noise is not None:
        given_extrinsics = torch.stack([poses[v].to(torch.float32) for v in train_ids])
        extrinsics0 = given_extrinsics
        if args.load_checkpoint and "joint_initial_extrinsics" in ck:       # the poses the saved twists are relative to
            extrinsics0 = torch.as_tensor(ck["joint_initial_extrinsics"], dtype=torch.float32, device=dev)
        elif args.pose_noise is not None:
            extrinsics0 = perturbed_poses(given_extrinsics, args.pose_noise[0], args.pose_noise[1], args.seed + 31337,
                                          keep=tuple(args.fix_views or ()) if args.refine_poses else ())
        if not args.refine_poses:       # training at the perturbed poses: the selector's records are rebuilt from them
            selector = nerf.MultiViewRaySelector(hw[0], hw[1], list(extrinsics0), [intrinsics[v] for v in train_ids], args.near, args.far,
                                                 images=selector.images, device=dev)
    if args.refine_poses:
        if world > 1:
            raise SystemExit("--refine-poses: one GPU only (nerf.FusedJointStep)")
        if not fused_ok:
            raise SystemExit("--refine-poses: this configuration is outside nerf.FusedJointStep (see FusedTrainStep.applicable); "
                             "nerf.MultiPoseRefiner + autograd covers those")
        if max(args.fix_views) >= len(train_ids):
            raise SystemExit(f"--fix-views {args.fix_views}: the training set has {len(train_ids)} views")
        if args.refine_exposure is not None and max(args.fix_exposure_views) >= len(train_ids):
            raise SystemExit(f"--fix-exposure-views {args.fix_exposure_views}: the training set has {len(train_ids)} views")
        joint = nerf.FusedJointStep(student[0], student[1], cfg, hw[0], hw[1], torch.stack([intrinsics[v] for v in train_ids]), extrinsics0,
                                    selector.images, ex, ed, args.num_random_rays, bucket, opt, args.pose_lr,
                                    pose_lr_decay=args.pose_lr_decay, luminance=args.ir, seed=args.seed, first_iteration=start,
                                    ndc_focal=ndc_focal, use_graphs=use_graph, eager_iterations=3, refine_intrinsics=args.refine_intrinsics,
                                    intrinsics_scale=args.intrinsics_scale, fixed_views=args.fix_views, encoding_anneal=anneal,
                                    refine_exposure=args.refine_exposure, exposure_scale=args.exposure_scale,
                                    exposure_fixed_views=tuple(args.fix_exposure_views or ()), **head)
        if args.load_checkpoint:
            restore_joint_state(ck, joint)
        fused_ok = False                # the joint step is the training iteration

    def camera_of(view):
        """(extrinsic, K) a view is rendered at: a training view under --refine-poses at its refined camera, any other as given."""
        if joint is not None and view in train_ids:
            k_now = joint.intrinsics()
            return joint.extrinsics()[train_ids.index(view)], (k_now[train_ids.index(view)] if k_now.dim() == 3 else k_now)
        return poses[view], intrinsics[view]

    def log_pose_distances(it):
        current = joint.extrinsics()
        rot0, trans0 = pose_distance(current, extrinsics0)
        text = f"[pose]  iter {it:6d} from the initial poses: {rot0:.4f} deg, {trans0:.5f}"
        if args.pose_noise is not None:
            rot1, trans1 = pose_distance(current, given_extrinsics)
            text += f"; from the unperturbed poses: {rot1:.4f} deg, {trans1:.5f}"
        if not args.quiet:
            print(text, flush=True)

    if fused_ok:
        fused = nerf.FusedTrainStep(student[0], student[1], selector, cfg, bucket, ex, ed, args.num_random_rays, seed=args.seed + 7919 * rank,
                                    luminance=args.ir, first_iteration=start, draw_view="rays" if args.mix_views else True,
                                    ndc_focal=ndc_focal, distortion_weights=distortion, encoding_anneal=anneal,
                                    **(dict(ray_span=live, ray_span_pad=args.ray_span_pad, occupancy_update_every=args.occupancy_every)
                                       if live is not None else {}), **head)
    graphed = nerf.GraphedTrainStep(fused, opt, eager_iterations=3, use_graphs=use_graph) if fused is not None else None
    use_graph = use_graph and world == 1      # (the autograd step's single graph below: one rank only)

    def iteration():
        """The torch composition (--autograd-step, configurations outside nerf.FusedTrainStep): select rays -> coarse +
        fine render -> loss -> backward -> (all-reduce) -> Adam; device-side state only."""
        if args.mix_views:
            view_index, pixel_index = selector.random_pairs(args.num_random_rays)
            rays, target = selector.select(pixel_index, view=view_index)
        else:
            rays, target = selector.select(selector.random_pixels(args.num_random_rays))
        if args.ndc:
            # run_one_iter_of_nerf's NDC branch (reference train_utils.py:240-262) on the selected rows: origins / directions
            # through dn_ndc_rays (near plane at 1), bounds 0 .. 1, view directions stay those of the unwarped rays
            ro, rd = nerf.ndc_rays(hw[0], hw[1], data["focal"], 1.0, rays[:, :3].contiguous(), rays[:, 3:6].contiguous())
            rays = torch.cat([ro, rd, rays[:, 6:]], dim=-1)
        chunks = [nerf.predict_and_render_radiance(batch, student[0], student[1], cfg, mode="train", encode_position_fn=ex,
                                                   encode_direction_fn=ed, m_thres_cand=thres)
                  for batch in nerf.get_minibatches(rays, chunksize=args.chunksize)]
        out = chunks[0] if len(chunks) == 1 else [torch.cat(c, dim=0) for c in zip(*chunks)]
        if args.ir:
            lum = lambda t: 0.299 * t[..., 0] + 0.587 * t[..., 1] + 0.114 * t[..., 2]  # noqa: E731
            loss = nerf.img2mse(lum(out[0]), lum(target)) + nerf.img2mse(lum(out[3]), lum(target))
        else:
            loss = nerf.img2mse(out[0][..., :3], target) + nerf.img2mse(out[3][..., :3], target)
        bucket.zero()
        loss.backward()
        bucket.all_reduce_mean()              # one flat all-reduce (RCCL over xGMI when world > 1)
        opt.step()
        loss_t.copy_(loss.detach())

    graph, graph_warned = None, False
    history = []
    t0 = time.perf_counter()
    t_steady = None
    loss_val = psnr = float("nan")
    for it in range(start, args.iters):
        if fused is None and joint is None:                                          # (the fused steps draw their views in the kernel)
            selector.view.fill_(int(np.random.randint(len(train_ids))))              # one random training view per iteration
        lr = args.lr * args.lr_decay_factor ** (it / (args.lr_decay * 1000))         # train_dexnerf_rgb.py:284-289
        if not flat_adam:
            lr_t.fill_(lr)
        if it == start + 20:                   # past the eager iterations and the capture: the steady part is timed from here
            torch.cuda.synchronize()
            t_steady = time.perf_counter()
        if joint is not None:
            joint.step()
            if joint.fallback_reason and not args.quiet and not graph_warned:
                graph_warned = True
                print(f"[train] HIP-graph capture unavailable ({joint.fallback_reason}); launching eagerly", flush=True)
        elif graphed is not None:
            graphed.step()
            if graphed.fallback_reason and rank == 0 and not args.quiet and not graph_warned:
                graph_warned = True
                print(f"[train] HIP-graph capture unavailable ({graphed.fallback_reason}); launching eagerly", flush=True)
        elif use_graph and graph is None and it >= start + 3:
            # three eager iterations have initialised every lazy state (optimizer moments, packed streams); capture the
            # fourth and replay it from here on.  Anything that cannot be captured falls back to eager launches.
            try:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    iteration()
                graph.replay()                         # a capture only records: this iteration's step runs here
                nerf.models.mark_parameters_updated()
            except Exception as exc:  # noqa: BLE001
                graph, use_graph = None, False
                torch.cuda.synchronize()
                if rank == 0 and not args.quiet:
                    print(f"[train] HIP-graph capture unavailable ({type(exc).__name__}: {exc}); launching eagerly", flush=True)
                iteration()
        elif graph is not None:
            graph.replay()
            nerf.models.mark_parameters_updated()   # the replayed optimizer step ran no Python hook
        else:
            iteration()
        if it % 100 == 0 or it == args.iters - 1:
            loss_val = (joint.loss3[0] if joint is not None else fused.loss3[0] if fused is not None else loss_t).item()
            psnr = nerf.mse2psnr(loss_val)
            history.append((it, loss_val, psnr))
            if rank == 0 and not args.quiet:
                reg = "" if fused is None or fused.reg2 is None else "distortion coarse {:.5f} fine {:.5f} ".format(*fused.reg2.tolist())
                print(f"[train] iter {it:6d} loss {loss_val:.5f} psnr {psnr:.2f} dB {reg}lr {lr:.2e} "
                      f"{(time.perf_counter() - t0):.1f} s", flush=True)
            s8 = nerf.s8_grad_stats() if args.precision in ("bf16", "bf16-s8") else None
            if s8 is not None:
                s8_saturated_max = max(s8_saturated_max, s8["saturated"])
                if s8["saturated"] > 1e-4 and rank == 0 and not s8_warned:
                    s8_warned = True
                    print(f"[train] WARNING: {s8['saturated']:.2e} of the 8-bit saved layer gradients are clipped at e5m2's largest value "
                          f"(scale {s8['scale']}): the loss is outside the range the fixed gradient scale covers (a sum-reduced or "
                          "scaled loss?) - pass --s8-grad-scale 0 (per-launch scale) or a smaller power of two", flush=True)
        if rank == 0 and args.validate_every and (it + 1) % args.validate_every == 0:
            if joint is not None:
                log_pose_distances(it + 1)
            if anneal is not None:
                anneal.set_iteration(it + 1)     # renders see the amplitudes of the steps taken (the next step forms its own table)
            out = render_view(student, cfg, *camera_of(held_out), hw, ex, ed, thres)
            vmse = nerf.img2mse(out[3].reshape(-1, 3), images[held_out]).item()
            if depths[held_out] is None:     # (LLFF captures carry no depth maps: no Dex threshold sweep)
                if not args.quiet:
                    print(f"[val]   iter {it + 1:6d} held-out view psnr {nerf.mse2psnr(vmse):.2f} dB", flush=True)
                continue
            m_best, err = dex_sweep(out, depths[held_out], thres, data["mask_hi"])
            q_log = ""
            val_quantiles = args.val_quantiles
            if val_quantiles:
                q_best, q_err = quantile_sweep(student, cfg, *camera_of(held_out), hw, ex, depths[held_out], val_quantiles, data["mask_hi"])
                q_log = f"; quantile best q={q_best:g} abs depth err {q_err['depth_abs_err']:.1f} mm"
            if not args.quiet:
                print(f"[val]   iter {it + 1:6d} held-out view psnr {nerf.mse2psnr(vmse):.2f} dB; Dex best m={m_best} "
                      f"abs depth err {err['depth_abs_err']:.1f} mm{q_log}", flush=True)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    result = dict(history=history, final_loss=loss_val, final_psnr=psnr, seconds=elapsed,
                  rays_per_s=world * args.num_random_rays * (args.iters - start) / max(elapsed, 1e-9))
    if t_steady is not None and args.iters - start > 20:
        result["steady_ms_per_iter"] = (t0 + elapsed - t_steady) * 1e3 / (args.iters - start - 20)
    if joint is not None:
        result["hip_graphs"] = int(joint.graph is not None)
        result["pose_from_initial"] = pose_distance(joint.extrinsics(), extrinsics0)      # (degrees, scene units), means over the views
        if args.pose_noise is not None:
            result["pose_from_unperturbed"] = pose_distance(joint.extrinsics(), given_extrinsics)
        result["xi"] = joint.xi.detach().cpu()
        if joint.exposure_mode is not None:      # the final rows, (V,P)
            result["exposure"] = joint.exposure().cpu().tolist()
    else:
        result["hip_graphs"] = len(graphed.graphs) if (graphed is not None and graphed.graphs) else int(graph is not None)   # graphs replayed per iteration
    if args.precision in ("bf16", "bf16-s8"):
        result["s8_saturated_max"] = s8_saturated_max
    if args.save and rank != 0 and os.environ.get("DEXNERF_SAVE_ALL_RANKS"):   # rehearsals: compare the replicas
        torch.save({"model_coarse_state_dict": student[0].state_dict(), "model_fine_state_dict": student[1].state_dict()}, args.save)
    if live is not None:
        result["train_occupancy"] = live
        result["occupied_fraction"] = live.occupied_fraction()
    if anneal is not None:
        anneal.set_iteration(args.iters)
        result["encoding_amplitudes"] = anneal.amplitudes().tolist()
    if rank == 0:
        out = render_view(student, cfg, *camera_of(held_out), hw, ex, ed, thres)
        result["val_psnr"] = nerf.mse2psnr(nerf.img2mse(out[3].reshape(-1, 3), images[held_out]).item())
        if depths[held_out] is not None:
            m_best, err = dex_sweep(out, depths[held_out], thres, data["mask_hi"])
            result["dex_best_threshold"], result["dex_abs_err_mm"] = int(m_best), err["depth_abs_err"]
            # the expected depth sum(w z) of the fine pass - what --depth-weight supervises - under the same mask and metric
            _, expected = nerf.dex_error_sweep(depths[held_out], [out[4]], gt_lo=0.0, gt_hi=data["mask_hi"])
            result["expected_depth_abs_err_mm"] = expected[0]["depth_abs_err"]
            if args.val_quantiles:
                q_best, q_err = quantile_sweep(student, cfg, *camera_of(held_out), hw, ex, depths[held_out], args.val_quantiles,
                                               data["mask_hi"])
                result["quantile_best"], result["quantile_abs_err_mm"] = float(q_best), q_err["depth_abs_err"]
        if args.save:
            opt_state = opt.state_dict()
            for group in opt_state["param_groups"]:   # the reference stores a Python float (train_dexnerf_rgb.py:443-456), not the
                group["lr"] = float(group["lr"])     # device scalar the captured graph reads the schedule from
            extra = joint_checkpoint_entries(joint, train_ids, extrinsics0) if joint is not None else {}
            if anneal is not None:
                extra["encoding_anneal"] = anneal.state_dict(iteration=args.iters)
            if live is not None:
                extra["train_occupancy"] = live.state_dict()
            torch.save({"iter": args.iters, "model_coarse_state_dict": student[0].state_dict(),
                        "model_fine_state_dict": student[1].state_dict(), "optimizer_state_dict": opt_state,
                        "loss": loss_val, "psnr": psnr, **extra}, args.save)
        if not args.quiet:
            print(f"[done] {args.iters - start} iters in {elapsed:.1f} s = {result['rays_per_s']:.0f} rays/s; "
                  f"held-out psnr {result['val_psnr']:.2f} dB", flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    # process-wide switches this run set go back to the library's defaults (main() is also called as a function: tests, bench.py)
    if args.s8_grad_scale is not None:
        nerf.set_s8_grad_scale(0.0)
    _nerf_ops.set_deterministic_weight_gradients(True)
    return result


if __name__ == "__main__":
    main()
