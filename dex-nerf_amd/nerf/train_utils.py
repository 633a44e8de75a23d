"""run_network / predict_and_render_radiance / run_one_iter_of_nerf with the reference's call surface
(reference nerf/train_utils.py:72-288), plus the Dex depth-error helpers (:9-70)."""
import collections
import os

import numpy as np
import torch

from . import _ops
from ._train import inputs_need_grad, needs_grad, render_rays_train, run_network_fused, run_network_fused_rays, train_fused_ok
from .models import FlexibleNeRFModel
from .nerf_helpers import Embedder, _require_device, get_minibatches, ndc_rays
from .nerf_helpers import sample_pdf_2 as sample_pdf  # noqa: F401  (reference train_utils.py:6 alias)
from .volume_rendering_utils import _thresholds, volume_render_radiance_field


# ---- Dex depth metrics (reference train_utils.py:9-70; validation-time logging, numpy/torch host code) ----
def _err_dict(row):
    n = row[4]
    return {"depth_abs_err": row[0] / n, "depth_err2": row[1] / n, "depth_err4": row[2] / n, "depth_err8": row[3] / n}


def compute_err_metric(depth_gt, depth_pred, mask):
    """Masked depth errors (reference :9-30): mean |err| in millimetres (inputs are metres) and the fraction
    of masked pixels whose error exceeds 2 / 4 / 8 mm.  `mask` is a boolean selector.  Device inputs are reduced by
    one HIP kernel and a single 40-byte copy; host inputs by the reference's torch composition."""
    if depth_gt.is_cuda:
        out = _ops.dex_error_sweep(depth_gt, depth_pred.reshape(1, -1), mask.to(depth_gt.device))
        return _err_dict(out[0].tolist())
    gt, pred = depth_gt[mask], depth_pred[mask]
    diff = torch.abs(gt - pred)
    count = diff.numel()
    return {"depth_abs_err": torch.mean(torch.abs(pred * 1000 - gt * 1000)).item(),
            "depth_err2": int((diff > 2e-3).sum()) / count,
            "depth_err4": int((diff > 4e-3).sum()) / count,
            "depth_err8": int((diff > 8e-3).sum()) / count}


def dex_error_sweep(depth_gt, depth_fine_dex, mask=None, gt_lo=0.0, gt_hi=1.25):
    """The reference's validation loop over the Dex threshold candidates (train_dexnerf_rgb.py:391-408) on the device:
    every candidate depth map against the ground truth in ONE kernel and ONE device->host copy (the reference moves
    each of the K maps to the CPU).  `mask=None` is the reference's ground mask (0 < gt < 1.25 m).
    Returns (best_index, [err dict per candidate]); best = the first candidate whose mean abs error undercuts the
    running minimum, starting from 1000 mm as the reference does (None if none does)."""
    maps = depth_fine_dex if torch.is_tensor(depth_fine_dex) else torch.stack([d.reshape(-1) for d in depth_fine_dex])
    rows = _ops.dex_error_sweep(depth_gt, maps, None if mask is None else mask.to(depth_gt.device), gt_lo, gt_hi).tolist()
    errs = [_err_dict(r) for r in rows]
    best, min_abs = None, 1000.0
    for i, e in enumerate(errs):
        if e["depth_abs_err"] < min_abs:
            best, min_abs = i, e["depth_abs_err"]
    return best, errs


def gen_error_colormap_depth():
    """Piecewise-constant blue->red colormap rows [lo, hi, r, g, b] (reference :31-48)."""
    cols = np.array(
        [[0, 0.00001, 0, 0, 0], [0.00001, 2000. / (2 ** 10), 49, 54, 149], [2000. / (2 ** 10), 2000. / (2 ** 9), 69, 117, 180],
         [2000. / (2 ** 9), 2000. / (2 ** 8), 116, 173, 209], [2000. / (2 ** 8), 2000. / (2 ** 7), 171, 217, 233],
         [2000. / (2 ** 7), 2000. / (2 ** 6), 224, 243, 248], [2000. / (2 ** 6), 2000. / (2 ** 5), 254, 224, 144],
         [2000. / (2 ** 5), 2000. / (2 ** 4), 253, 174, 97], [2000. / (2 ** 4), 2000. / (2 ** 3), 244, 109, 67],
         [2000. / (2 ** 3), 2000. / (2 ** 2), 215, 48, 39], [2000. / (2 ** 2), np.inf, 165, 0, 38]], dtype=np.float32)
    cols[:, 2:5] /= 255.
    return cols


def depth_error_img(D_est_tensor, D_gt_tensor, mask, abs_thres=1., dilate_radius=1):
    """Colour-coded |gt - est| / abs_thres image for logging: inputs (B, H, W), returns the first image
    (H, W, 3) as numpy with the colour legend painted in its top-left corner (reference :46-70).  Device inputs
    are coloured by a HIP kernel (one (H,W,3) copy back instead of three input copies)."""
    if D_gt_tensor.is_cuda:
        img = _ops.depth_error_image(D_est_tensor.detach()[0], D_gt_tensor.detach()[0], mask.detach()[0].to(D_gt_tensor.device),
                                     abs_thres)
        return img.cpu().numpy()
    gt = D_gt_tensor.detach().cpu().numpy()
    est = D_est_tensor.detach().cpu().numpy()
    valid = mask.detach().cpu().numpy().astype(bool)
    batch, height, width = gt.shape
    err = np.abs(gt - est)
    err[~valid] = 0
    err[valid] = err[valid] / abs_thres
    cols = gen_error_colormap_depth()
    img = np.zeros([batch, height, width, 3], dtype=np.float32)
    for row in cols:
        img[np.logical_and(err >= row[0], err < row[1])] = row[2:]
    img[~valid] = 0.
    for i, row in enumerate(cols):  # legend: 20-pixel-wide swatches along the top edge
        img[:, :10, i * 20:(i + 1) * 20, :] = row[2:]
    return img[0]


# ---- hot path ------------------------------------------------------------------------------------------
_FP16_RENDER_DISABLED = [False]   # set once an fp16 render overflowed (see _fp16_guard / _warn_fp16_range)
_STAGEWISE_TRAINING = [bool(int(os.environ.get("DEXNERF_STAGEWISE_TRAINING", "0")))]   # tests flip this to compare the two routes


def _fusable(network_fn, embed_fn, embeddirs_fn, density=False):
    """True when the fused HIP kernels cover this network with these embedders; density=True asks for the position embedder
    alone (render_dex_depth: the density sub-network reads no view direction)."""
    if not (isinstance(network_fn, FlexibleNeRFModel) and network_fn.fused_ok()):
        return False
    if not isinstance(embed_fn, Embedder):
        return False
    if embed_fn.num_encoding_functions != network_fn.num_encoding_fn_xyz or not embed_fn.include_input:
        return False
    if network_fn.use_viewdirs and not density:
        if not isinstance(embeddirs_fn, Embedder):
            return False
        if embeddirs_fn.num_encoding_functions != network_fn.num_encoding_fn_dir or not embeddirs_fn.include_input:
            return False
    return True


def run_network(network_fn, pts, ray_batch, chunksize, embed_fn, embeddirs_fn):
    """Embed points (+ per-ray view directions) and evaluate the network: (..., S, 3) -> (..., S, 4)
    (reference train_utils.py:72-89).  A FlexibleNeRFModel with this package's embedders runs as one fused
    HIP kernel (encoding never materialised); any other callable gets the generic composition:
    HIP encoding -> network_fn minibatches -> concat."""
    _require_device(pts, "run_network")
    if _fusable(network_fn, embed_fn, embeddirs_fn) and (train_fused_ok(network_fn) or not needs_grad(network_fn, pts)):  # noqa: E501
        s = pts.shape[-2] if pts.dim() >= 2 else 1
        viewdirs = ray_batch[..., -3:] if network_fn.use_viewdirs else None
        log_dir = embeddirs_fn.log_sampling if network_fn.use_viewdirs else True
        out = run_network_fused(network_fn, pts, viewdirs, s, embed_fn.log_sampling, log_dir)
        return out.reshape(list(pts.shape[:-1]) + [4])
    pts_flat = pts.reshape((-1, pts.shape[-1]))
    embedded = embed_fn(pts_flat)
    if embeddirs_fn is not None:
        viewdirs = ray_batch[..., None, -3:]
        input_dirs = viewdirs.expand(pts.shape).reshape((-1, 3))
        embedded = torch.cat((embedded, embeddirs_fn(input_dirs)), dim=-1)
    preds = [network_fn(batch) for batch in get_minibatches(embedded, chunksize=chunksize)]
    radiance_field = torch.cat(preds, dim=0)
    return radiance_field.reshape(list(pts.shape[:-1]) + [radiance_field.shape[-1]])


def _wants_grad(*models):
    if not torch.is_grad_enabled():
        return False
    return any(m is not None and isinstance(m, torch.nn.Module) and any(p.requires_grad for p in m.parameters())
               for m in models)


def _draws(n, nc, nf, fine, perturb, std, dev):
    """The random numbers of one chunk of n rays, drawn in the reference's order (train_utils.py:92-202): rand, randn, rand, randn
    -> t_rand (n, nc), noise_c (n, nc), u (n, nf), noise_f (n, nc + nf).  What the settings do not use is neither drawn nor
    present.  A parity rule: every fused render path takes its draws from here."""
    def rand(*shape):
        return torch.rand(shape, dtype=torch.float32, device=dev)

    def randn(*shape):
        return torch.randn(shape, dtype=torch.float32, device=dev)
    draws = {}
    if perturb:
        draws["t_rand"] = rand(n, nc)
    if std > 0.0:
        draws["noise_c"] = randn(n, nc)
    if fine and perturb:
        draws["u"] = rand(n, nf)
    if fine and std > 0.0:
        draws["noise_f"] = randn(n, nc + nf)
    return draws


def _fp16_guard(models, density=False):
    """(precision code a no-grad render of `models` runs in, guarded?).  In the bf16 modes such a render runs the fp16 instances of
    the kernels (_ops.set_render_policy), guarded against fp16's range by the status words the render leaves in its workspace.
    Guarded = the render precision differs from the configured one, the stream is not capturing (a capture cannot read the
    words back: no synchronisation inside it), no earlier fp16 render of this process overflowed, and every network's kernel
    instance (density=True: its density sub-network's) carries the range tracker.  Otherwise: the configured precision."""
    prec = _ops.render_precision()
    guarded = (prec != _ops._precision and not torch.cuda.is_current_stream_capturing() and not _FP16_RENDER_DISABLED[0]
               and all(_ops.fp16_range_guard(m, density=density) for m in models))
    return (prec if guarded else _ops._precision), guarded


def _warn_fp16_range():
    import warnings
    # stacklevel 4 = the caller of the public function: this <- _render_chunk / _render_chunks <- public function <- caller
    warnings.warn("nerf: an fp16 render produced non-finite raw radiance-field values (a hidden activation beyond fp16's "
                  "range, 65504); this render is repeated in bf16 and every later one in this process runs in bf16 "
                  "(nerf.set_render_policy)", RuntimeWarning, stacklevel=4)
    _FP16_RENDER_DISABLED[0] = True


def _join_chunks(chunks):
    """Per-chunk lists of maps -> one list, rows concatenated; a None column stays None.  A single chunk is returned as it is
    (the very same tensors: cat would copy every map)."""
    if len(chunks) == 1:
        return list(chunks[0])
    return [torch.cat(col, dim=0) if col[0] is not None else None for col in zip(*chunks)]


def _render_chunks(rays, chunksize, render_chunk):
    """The chunk loop of the image-level renders.  render_chunk(batch, status) -> maps renders one chunk: with a list as `status`
    under the guarded-fp16 policy (a guarded chunk appends a device copy of the status words the guard reads), with None in the
    configured precision.  The words of all chunks are summed and read back ONCE (one host synchronisation per image, not per
    chunk); if some chunk left fp16's range: one warning and the whole call again in the configured precision."""
    def run(status):
        return [render_chunk(batch, status) for batch in get_minibatches(rays, chunksize=chunksize)]
    status = []
    chunks = run(status)
    if status and int(torch.stack(status).sum().item()) > 0:
        _warn_fp16_range()
        chunks = run(None)   # (chunks that draw random numbers draw FRESH ones here, not those of the fp16 attempt)
    return _join_chunks(chunks)


def predict_and_render_radiance(ray_batch, model_coarse, model_fine, options, mode="train",
                                encode_position_fn=None, encode_direction_fn=None, m_thres_cand=None):
    """One ray chunk through coarse sampling -> coarse net -> composite -> inverse-CDF resampling -> fine
    net -> composite (reference train_utils.py:92-202).

    Returns (rgb_coarse, depth_coarse, acc_coarse, rgb_fine, depth_fine, acc_fine, *depth_fine_dex[K]).
    Supersets of the fork: m_thres_cand=None gives exactly six outputs (eval_nerf.py:175-187 unpacks six);
    num_fine == 0 / model_fine None returns None for the fine maps and the coarse Dex depths instead of the
    fork's NameError (:201).  RNG draw order matches the reference (rand, randn, rand, randn).
    A no-grad render under the guarded-fp16 policy checks this chunk itself (one host read); if it left fp16's range it is
    repeated in bf16 on the same draws.
    """
    return _render_chunk(ray_batch, model_coarse, model_fine, options, mode, encode_position_fn, encode_direction_fn, m_thres_cand)


def _render_chunk(ray_batch, model_coarse, model_fine, options, mode, encode_position_fn, encode_direction_fn, m_thres_cand,
                  status=None, fp16_ok=True):
    """predict_and_render_radiance.  status: a list - the image-level drivers' way to defer the fp16 guard: a guarded render
    appends a copy of its status words (the workspace may be reused by the next chunk) instead of reading them; fp16_ok=False:
    a no-grad render in the configured precision, unguarded."""
    _require_device(ray_batch, "predict_and_render_radiance")
    opt = getattr(options.nerf, mode)
    thres = _thresholds(m_thres_cand)
    n = ray_batch.shape[0]
    nc, nf = int(opt.num_coarse), int(opt.num_fine)
    fine = nf > 0 and model_fine is not None
    perturb = bool(opt.perturb)
    std = float(opt.radiance_field_noise_std)
    white = bool(opt.white_background)
    lindisp = bool(opt.lindisp)
    dev = ray_batch.device
    use_viewdirs = ray_batch.shape[-1] > 8

    def outputs(maps):
        dex = maps[6]
        return tuple(list(maps[:6]) + ([] if dex is None else [dex[k] for k in range(dex.shape[0])]))

    fused_models = (_fusable(model_coarse, encode_position_fn, encode_direction_fn)
                    and (not fine or _fusable(model_fine, encode_position_fn, encode_direction_fn))
                    and model_coarse.use_viewdirs == use_viewdirs)
    if fused_models and not _wants_grad(model_coarse, model_fine) and not inputs_need_grad(ray_batch):
        # whole chunk in one C-ABI call (dn_render_rays)
        draws = _draws(n, nc, nf, fine, perturb, std, dev)
        lx = encode_position_fn.log_sampling
        ld = encode_direction_fn.log_sampling if use_viewdirs else True
        models = [model_coarse] + ([model_fine] if fine else [])

        def render(prec):
            pc = model_coarse.packed(lx, ld, precision=prec)
            pf = model_fine.packed(lx, ld, precision=prec) if fine else None
            return _ops.render_rays(pc, pf, ray_batch, nc, nf if fine else 0, lindisp, std, white, thres, draws)
        prec, guarded = _fp16_guard(models) if fp16_ok else (_ops._precision, False)
        maps = render(prec)
        if guarded and status is not None:
            status.append(_ops.render_status_words())
        elif guarded and _ops.render_nonfinite_count() > 0:
            _warn_fp16_range()
            maps = render(_ops._precision)
        return outputs(maps)

    if (fused_models and train_fused_ok(model_coarse) and (not fine or train_fused_ok(model_fine))
            and not inputs_need_grad(ray_batch) and not _STAGEWISE_TRAINING[0]):
        # training: the whole chunk as one differentiable op - one C-ABI call forward (dn_render_rays_train), one backward
        # (dn_render_rays_backward)
        draws = _draws(n, nc, nf, fine, perturb, std, dev)
        logs = (encode_position_fn.log_sampling, encode_direction_fn.log_sampling if use_viewdirs else True)
        return outputs(render_rays_train(model_coarse, model_fine if fine else None, _ops.f32c(ray_batch),
                                         (nc, nf if fine else 0, lindisp, std, white), draws, thres, logs))

    # stage-by-stage composition (autograd through a network the fused training kernels do not cover, inputs that
    # require grad, or DEXNERF_STAGEWISE_TRAINING=1); the compositing stages draw their own noise, in the same order
    rays = _ops.f32c(ray_batch)
    ro, rd = rays[..., :3], rays[..., 3:6]
    # rows that require grad (pose / ray optimisation): the depths carry their gradient to near / far, through the merge and - in
    # volume_render_radiance_field - through dists and depth; rows without grad take none of that
    ray_grad = inputs_need_grad(ray_batch)
    t_rand = torch.rand((n, nc), dtype=torch.float32, device=dev) if perturb else None
    z_vals = _ops.CoarseDepthsFn.apply(rays, nc, lindisp, t_rand) if ray_grad else _ops.coarse_depths(rays, nc, lindisp, t_rand)

    def network(model, z):
        if fused_models and (train_fused_ok(model) or not needs_grad(model)):
            # ray rows + depths straight into the fused kernel (the points are formed there)
            lx = encode_position_fn.log_sampling
            ld = encode_direction_fn.log_sampling if use_viewdirs else True
            return run_network_fused_rays(model, rays, z, lx, ld)
        pts = ro[..., None, :] + rd[..., None, :] * z[..., :, None]
        return run_network(model, pts, rays, opt.chunksize, encode_position_fn, encode_direction_fn)

    rf = network(model_coarse, z_vals)
    coarse = volume_render_radiance_field(rf, z_vals, rd, radiance_field_noise_std=std, white_background=white,
                                          m_thres_cand=thres)
    rgb_c, acc_c, weights, depth_c = coarse[0], coarse[2], coarse[3], coarse[4]
    if not fine:
        return tuple([rgb_c, depth_c, acc_c, None, None, None] + list(coarse[5:]))
    u = torch.rand((n, nf), dtype=torch.float32, device=dev) if perturb else None
    z_fine = _ops.FineDepthsFn.apply(z_vals, weights.detach(), nf, u) if ray_grad else _ops.fine_depths(z_vals, weights.detach(), nf, u)
    rf = network(model_fine, z_fine)
    fine_out = volume_render_radiance_field(rf, z_fine, rd, radiance_field_noise_std=std, white_background=white,
                                            m_thres_cand=thres)
    return tuple([rgb_c, depth_c, acc_c, fine_out[0], fine_out[4], fine_out[2]] + list(fine_out[5:]))


def _to_image(maps, shapes):
    return tuple(m.reshape(shape) if m is not None else None for m, shape in zip(maps, shapes))


def _culled_precision(who):
    """Precision code of a culled render: the configured one; 'fp16' raises (explicit points carry no range status)."""
    if _ops._precision == _ops._hip.PREC_F16:
        raise RuntimeError(f"{who}(occupancy=...): the culled render evaluates explicit points, which carry no fp16 range status - it "
                           "runs in 'fp32' or bf16, not under nerf.set_precision('fp16')")
    return _ops._precision


def _check_ray_span(who, ray_span, ray_span_pad, models, ray_origins, ray_directions):
    """Every refusal of ray_span= / ray_span_pad= before any GPU work -> the pad as an fp32 value, or None without a grid
    (ray_span_pad=None stands for 1 cell)."""
    if ray_span is None:
        if ray_span_pad is not None:
            raise ValueError(f"{who}: ray_span_pad widens a ray's span: give ray_span=")
        return None
    pad = _ops.check_ray_span_pad(1.0 if ray_span_pad is None else ray_span_pad, f"{who}: ray_span_pad")
    ray_span.check_render(ray_directions.device, who)
    if _wants_grad(*models) or inputs_need_grad(ray_origins, ray_directions):
        raise RuntimeError(f"{who}(ray_span=...) is a no-grad render: the tightening replaces each ray's near and far by values read "
                           "from the grid, which would cut the near/far gradient of the rays; call it under torch.no_grad() (or with "
                           "parameters and rays that do not require grad); training with spans is not provided")
    return pad


class _CullTotals:
    """The sum of a culled render's per-chunk stats (_ops.render_rays_*_culled): the kept / total counts per pass on the host (the
    chain reads them anyway), the non-finite counts on the device - read once, by result(), and only when `wanted` (else it gives None)."""

    def __init__(self, wanted):
        self.wanted, self.kept, self.total, self.records = wanted, [0, 0], [0, 0], []

    def add(self, stats):
        for p in range(2):
            self.kept[p] += stats["kept"][p]
            self.total[p] += stats["total"][p]
        self.records.extend(stats["records"])

    def result(self):
        if not self.wanted:
            return None
        return dict(kept=tuple(self.kept), total=tuple(self.total), nonfinite=int(torch.stack(self.records)[:, 2].sum().item()))


def _refuse_culled_colour(model_coarse, model_fine, ray_origins, ray_directions, options, mode, encode_position_fn, encode_direction_fn,
                          occupancy):
    """Every refusal of run_one_iter_of_nerf(occupancy=...) before any GPU work, in render_dex_depth(occupancy=...)'s order -> (the
    precision code, whether a fine pass runs)."""
    who = "run_one_iter_of_nerf"
    prec = _culled_precision(who)
    occupancy.check_render(ray_directions.device, who)
    fine = int(getattr(options.nerf, mode).num_fine) > 0 and model_fine is not None
    models = [model_coarse] + ([model_fine] if fine else [])
    if _wants_grad(*models) or inputs_need_grad(ray_origins, ray_directions):
        raise RuntimeError(f"{who}(occupancy=...) is a no-grad render: call it under torch.no_grad() (or with parameters and rays that "
                           "do not require grad); culling in training is not provided")
    for m in models:
        if not _fusable(m, encode_position_fn, encode_direction_fn) or m.use_viewdirs != bool(options.nerf.use_viewdirs):
            raise RuntimeError(f"{who}(occupancy=...): needs FlexibleNeRFModel networks the fused HIP kernels cover (fused_ok()), this "
                               "package's embedders with the networks' encodings and nerf.use_viewdirs as the networks have it; there "
                               "is no fallback")
    for t in [ray_directions, ray_origins] + [m.layer1.weight for m in models]:
        _require_device(t, who)
    return prec, fine


def run_one_iter_of_nerf(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options,
                         mode="train", encode_position_fn=None, encode_direction_fn=None, m_thres_cand=None, occupancy=None,
                         cull_stats=False, ray_span=None, ray_span_pad=None):
    """Pack rays, chunk, render, concatenate (reference train_utils.py:205-288).

    Output order: rgb_coarse, depth_coarse, acc_coarse, rgb_fine, depth_fine, acc_fine, *dex_fine[K]; flat
    (N,3)/(N,) in train mode, reshaped to the image in validation mode (slots 1/4 are depth, not disparity).

    occupancy: an nerf.OccupancyGrid on the rays' device - a no-grad render whose chunks go through _ops.render_rays_culled: the
    samples of both passes are classified against the grid, the networks run only on the kept ones (explicit points, one view
    direction row per point), and a culled sample composites as empty space (rgb 0, sigma -FLT_MAX: weight exactly 0).  What
    render_dex_depth says of its grid holds here: the space the grid lives in, the level, the noise, the draws (made as without a
    grid), the precision - nerf.set_precision's, 'fp16' raises, the guarded-fp16 render policy does not apply -, two host reads per
    chunk, no HIP-graph capture.  No-grad only, device tensors only, networks the fused kernels cover only: anything else raises before
    any GPU work.  cull_stats=True (with a grid only) appends render_dex_depth's dict(kept=, total=, nonfinite=) to the return -
    nonfinite counts all four columns of the kept rows.  occupancy=None: the launches and the return are what they were.

    ray_span: an nerf.OccupancyGrid on the rays' device - a no-grad render whose ray rows are tightened once, right after they are
    packed (and after the NDC warp where there is one): render_dex_depth's ray_span=, with the same ray_span_pad, the same refusals
    and the same limits; it works with and without occupancy=.  ray_span=None: the launches and the return are what they were.
    """
    if occupancy is None and cull_stats:
        raise ValueError("run_one_iter_of_nerf: cull_stats reports on a culled render: give occupancy=")
    span_pad = _check_ray_span("run_one_iter_of_nerf", ray_span, ray_span_pad, [model_coarse, model_fine], ray_origins, ray_directions)
    culled = None
    if occupancy is not None:
        culled = _refuse_culled_colour(model_coarse, model_fine, ray_origins, ray_directions, options, mode, encode_position_fn,
                                       encode_direction_fn, occupancy)
    _require_device(ray_directions, "run_one_iter_of_nerf")
    thres = _thresholds(m_thres_cand)
    # device rays that need no gradient: the rows are packed by one kernel (dn_pack_ray_rows), op for op what follows
    one_launch = (ray_directions.is_cuda and ray_origins.is_cuda and ray_directions.dtype == torch.float32
                  and ray_origins.dtype == torch.float32 and not ray_directions.requires_grad and not ray_origins.requires_grad)
    viewdirs = None
    if options.nerf.use_viewdirs and not one_launch:
        viewdirs = ray_directions / ray_directions.norm(p=2, dim=-1).unsqueeze(-1)
        viewdirs = viewdirs.reshape((-1, 3))
    img_shape = ray_directions.shape
    if options.dataset.no_ndc is False:
        ro, rd = ndc_rays(height, width, focal_length, 1.0, ray_origins, ray_directions)
    else:
        ro, rd = ray_origins, ray_directions
    ro, rd = ro.reshape((-1, 3)), rd.reshape((-1, 3))
    if one_launch:
        rays = _ops.pack_ray_rows(ro, rd, ray_directions.reshape((-1, 3)) if options.nerf.use_viewdirs else None,
                                  options.dataset.near, options.dataset.far)
    else:
        near = options.dataset.near * torch.ones_like(rd[..., :1])
        far = options.dataset.far * torch.ones_like(rd[..., :1])
        parts = [ro, rd, near, far] + ([viewdirs] if viewdirs is not None else [])
        rays = torch.cat(parts, dim=-1).float()
    if ray_span is not None:
        rays = _ops.tighten_ray_rows(rays.contiguous(), ray_span, span_pad)

    def render_chunk(batch, status):
        return _render_chunk(batch, model_coarse, model_fine, options, mode, encode_position_fn, encode_direction_fn, thres,
                             status=status, fp16_ok=status is not None)
    stats = None
    if culled is None:
        images = _render_chunks(rays, getattr(options.nerf, mode).chunksize, render_chunk)
    else:
        images, stats = _render_chunks_culled(rays, model_coarse, model_fine, options, mode, encode_position_fn, encode_direction_fn, thres,
                                              occupancy, culled, cull_stats)
    tail = (stats,) if cull_stats else ()
    if mode != "validation":
        return tuple(images) + tail
    # rgb, depth, acc per pass (coarse-only: the reference returns the 3 maps + three Nones), then the Dex depths
    three = [img_shape, img_shape[:-1], img_shape[:-1]]
    return _to_image(images, three + (three if model_fine else [None, None, None]) + [img_shape[:-1]] * len(thres)) + tail


def _render_chunks_culled(rays, model_coarse, model_fine, options, mode, encode_position_fn, encode_direction_fn, thres, occupancy, culled,
                          cull_stats):
    """run_one_iter_of_nerf's chunk loop on _ops.render_rays_culled -> (the joined maps, the stats dict | None: _CullTotals): the draws
    of every chunk from _draws, as without a grid."""
    prec, fine = culled
    opt = getattr(options.nerf, mode)
    nc, nf = int(opt.num_coarse), int(opt.num_fine) if fine else 0
    std = float(opt.radiance_field_noise_std)
    lx = encode_position_fn.log_sampling
    ld = encode_direction_fn.log_sampling if model_coarse.use_viewdirs else True
    pc = model_coarse.packed(lx, ld, precision=prec)
    pf = model_fine.packed(lx, ld, precision=prec) if fine else None
    totals = _CullTotals(cull_stats)

    def render_chunk(batch):
        draws = _draws(batch.shape[0], nc, nf, fine, bool(opt.perturb), std, batch.device)
        maps, stats = _ops.render_rays_culled(pc, pf, batch, nc, nf, bool(opt.lindisp), std, bool(opt.white_background), thres, occupancy,
                                              draws, count_nonfinite=cull_stats)
        totals.add(stats)
        dex = maps[6]
        return list(maps[:6]) + ([] if dex is None else [dex[k] for k in range(dex.shape[0])])
    images = _join_chunks([render_chunk(batch) for batch in get_minibatches(rays, chunksize=opt.chunksize)])
    return images, totals.result()


_THRESHOLDS_ON_DEVICE = {}   # (thresholds, device) -> device tensor: one host-to-device copy per threshold set, none per render


def _threshold_tensor(thres, dev):
    if not len(thres):
        return None
    key = (tuple(float(m) for m in thres), str(dev))
    t = _THRESHOLDS_ON_DEVICE.get(key)
    if t is None:
        if len(_THRESHOLDS_ON_DEVICE) >= 64:
            _THRESHOLDS_ON_DEVICE.clear()
        t = _THRESHOLDS_ON_DEVICE[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
    return t


def _require_density_net(model, encode_position_fn, who):
    if not _fusable(model, encode_position_fn, None, density=True):
        raise RuntimeError(f"{who}: needs FlexibleNeRFModel networks the fused HIP kernels cover (fused_ok()) and this package's "
                           "position embedder with the network's encoding; there is no fallback")
    _require_device(model.layer1.weight, who)


_DensityRender = collections.namedtuple("_DensityRender", "rays img_shape dev nc nf fine models lindisp std perturb lx m_thres")


def _density_render_setup(who, instead, height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options, mode,
                          encode_position_fn, m_thres_cand, ray_span=None, span_pad=None):
    """What the density renders (render_dex_depth, render_dex_normals) settle before their chunk loops, every refusal before any GPU
    work: no autograd (`instead`: where the message sends the caller), device rays, density networks the fused kernels cover; then
    the NDC warp, the ray rows without view-direction columns (the density sub-network does not read them) - tightened to the occupied
    span of the grid `ray_span` where one is given (span_pad: _check_ray_span's) -, the mode's options and the thresholds on the
    device.  nf is 0 without a fine pass."""
    opt = getattr(options.nerf, mode)
    nc, nf = int(opt.num_coarse), int(opt.num_fine)
    fine = nf > 0 and bool(model_fine)
    models = [model_coarse] + ([model_fine] if fine else [])
    if _wants_grad(*models) or inputs_need_grad(ray_origins, ray_directions):
        raise RuntimeError(f"{who} is a no-grad render: call it under torch.no_grad() (or with parameters and rays that do "
                           f"not require grad); {instead}")
    _require_device(ray_directions, who)
    _require_device(ray_origins, who)
    for m in models:
        _require_density_net(m, encode_position_fn, who)
    dev = ray_directions.device
    if options.dataset.no_ndc is False:
        ro, rd = ndc_rays(height, width, focal_length, 1.0, ray_origins, ray_directions)
    else:
        ro, rd = ray_origins, ray_directions
    ro, rd = ro.reshape((-1, 3)).float(), rd.reshape((-1, 3)).float()
    rays = _ops.pack_ray_rows(ro.contiguous(), rd.contiguous(), None, options.dataset.near, options.dataset.far)
    if ray_span is not None:
        _ops.tighten_ray_rows(rays, ray_span, span_pad)
    return _DensityRender(rays, ray_directions.shape, dev, nc, nf if fine else 0, fine, models, bool(opt.lindisp),
                          float(opt.radiance_field_noise_std), bool(opt.perturb), encode_position_fn.log_sampling,
                          _threshold_tensor(_thresholds(m_thres_cand), dev))


def _density_packs(r, prec):
    """(coarse, fine | None) density packs of a _DensityRender's networks in precision `prec`."""
    return tuple(m.packed_density(r.lx, True, precision=prec) for m in r.models) + (() if r.fine else (None,))


def _render_dex_depth_culled(r, prec, occupancy, q_dev, interp, cull_stats, chunksize, mode):
    """render_dex_depth's chunk loop on _ops.render_rays_depth_culled: the draws of every chunk from _draws, as without a grid; the
    stats (_CullTotals) close the return when asked for."""
    packs = _density_packs(r, prec)
    totals = _CullTotals(cull_stats)

    def render_chunk(batch):
        draws = _draws(batch.shape[0], r.nc, r.nf, r.fine, r.perturb, r.std, r.dev)
        (depth_c, acc_c, depth_f, acc_f, dex, *qdepth), stats = _ops.render_rays_depth_culled(
            *packs, batch, r.nc, r.nf, r.lindisp, r.std, r.m_thres, occupancy, draws, quantiles=q_dev, interp=interp,
            count_nonfinite=cull_stats)
        totals.add(stats)
        maps = [depth_c, acc_c, depth_f, acc_f] + ([] if dex is None else [dex[k] for k in range(dex.shape[0])])
        return maps + ([qdepth[0][k] for k in range(qdepth[0].shape[0])] if qdepth else [])
    maps = _join_chunks([render_chunk(batch) for batch in get_minibatches(r.rays, chunksize=chunksize)])
    out = _to_image(maps, [r.img_shape[:-1]] * len(maps)) if mode == "validation" else tuple(maps)
    return out + ((totals.result(),) if cull_stats else ())


def render_dex_depth(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options,
                     mode="validation", encode_position_fn=None, encode_direction_fn=None, m_thres_cand=None, quantiles=None,
                     quantile_interp=False, occupancy=None, cull_stats=False, refine_steps=None, refine_width=False, ray_span=None,
                     ray_span_pad=None):
    """The depth half of run_one_iter_of_nerf and nothing else: expected depth, accumulation and the Dex first-crossing depths
    depend on sigma alone (reference nerf/volume_rendering_utils.py:33-58), so this render evaluates only the density
    sub-networks (trunk + fc_alpha: FlexibleNeRFModel.packed_density) and composites no colour (dn_render_rays_depth).

    Returns (depth_coarse, acc_coarse, depth_fine, acc_fine, *dex_fine[K]) - flat (N,) in train mode, image-shaped in validation
    mode; num_fine == 0 / model_fine None gives None for the fine maps and the coarse Dex depths.  Rays, chunking, NDC, lindisp,
    perturb / noise draws (rand, randn, rand, randn: the generator ends where a full render leaves it) follow
    run_one_iter_of_nerf; the number of thresholds is not limited.  No-grad only, device tensors only, networks the fused kernels
    cover only: anything else raises.  Follows nerf.set_render_policy like every no-grad render (guarded fp16 under 'bf16').

    quantiles: Q <= 64 fractions strictly inside (0, 1) (checked here, on the host, before anything else) - Q more maps follow the K
    Dex maps: the depth at which the ray's accumulated opacity first reaches q (0.5: the median depth; z(0.9) - z(0.1): a per-pixel
    depth confidence), from the same pass (dn_render_rays_depth_quantiles: the same launches).  quantile_interp=False gives the z of
    the crossing sample, the convention of the Dex depth; True the piecewise-linear CDF inversion the fine-depth sampler uses.  A ray
    whose accumulation stays below q reports its LAST sample's depth (it went through) - not z[0] like a Dex depth without a crossing.
    quantiles=None: the launches and the return are what they were.

    occupancy: an nerf.OccupancyGrid on the rays' device - each chunk then goes through _ops.render_rays_depth_culled: the samples of
    both passes are classified against the grid, the density networks run only on the kept ones, and a culled sample composites as
    empty space (sigma = -FLT_MAX).  The grid lives in the space of the sampled points (after the NDC warp where there is one).  With
    level 0 and no density noise a correctly classified culled sample contributes exactly nothing; a level above 0 changes the coarse
    weights and with them the fine samples; with noise the full render can revive a negative sigma and the culled one cannot.  The
    draws are made as without a grid, so the generator ends where the full render leaves it; quantiles are supported.  The culled
    render runs in nerf.set_precision's mode - 'fp32', or bf16 for 'bf16' and 'bf16-s16'; 'fp16' raises, as in density_grid - and does
    NOT follow the guarded-fp16 render policy: the network runs on explicit points, a launch that carries no range status (the
    guarded-fp16 policy on this path is a follow-up).  It reads the kept count back once per network pass - two host reads per chunk -
    and cannot be captured into a HIP graph.  cull_stats=True (with a grid only) appends one more value to the return: dict(kept=
    (coarse, fine), total=(coarse, fine), nonfinite=...) summed over the chunks - nonfinite: the non-finite raw sigma values the kept
    samples produced.  occupancy=None: the launches and the return are what they were.

    refine_steps: an int R in 0 .. 24 - K refined maps follow the K Dex maps (dn_render_rays_depth_refined): the Dex depth is z_i of
    the first sample whose density exceeds m, up to one sample interval late; the refined depth takes the bracket [z_{i-1}, z_i], halves
    it R times with one evaluation of the last pass's density network at the midpoint per step, and interpolates the last bracket
    linearly (R = 0: the interpolation of the sample bracket alone, no evaluation).  A ray whose first sample already crosses keeps z_0;
    a ray without a crossing keeps the Dex fallback z_0.  refine_width=True: K width maps follow the refined ones - the last bracket's
    width, 0 for a crossing at the first sample and -1 for rays without a crossing: the hit mask the Dex depth never had.  The
    refinement finds A crossing inside the first bracket: where the field crosses m three times between two samples that need not be
    the first one, and a crossing thinner than the sample spacing can be stepped over altogether, as by the Dex depth itself.  Judged
    here, on the host, before any GPU work (ValueError): steps that are not an int in 0 .. 24, no thresholds, a negative or non-finite
    threshold, a mode whose radiance_field_noise_std is not 0 (the brackets are those of the raw density), and quantiles= or occupancy=
    together with a refinement (both are follow-ups: a culled sample's -FLT_MAX is not a density to interpolate with).  Follows
    nerf.set_render_policy like the plain render: the midpoint evaluations report into the status words the guard reads.  No host read:
    a chunk can be captured into a HIP graph.  refine_steps=None: the launches and the return are what they were.

    ray_span: an nerf.OccupancyGrid on the rays' device (the same grid as occupancy=, or another) - the ray rows are tightened once,
    right after they are packed (and after the NDC warp where there is one: the grid lives in the space of the sampled points): one
    launch of dn_occupancy_ray_spans walks every ray through the grid and replaces its near and far by the depth range from the entry
    of the first set cell to the exit of the last one, widened by ray_span_pad cells of travel (None: 1) and clipped to the dataset's
    [near, far].  Everything downstream is what it was - the same number of samples, now spent where the grid has cells, so the Dex
    depth's one-sample-interval error shrinks with the span.  A ray that meets no set cell keeps its [near, far] and renders as
    before (a culled render skips its samples anyway).  No host read: it can be captured into a HIP graph, follows the render policy,
    and works with and without occupancy=, with refine_steps= and with quantiles=.  What the span does not promise: a ray that grazes
    a cell boundary within fp32 rounding can lose samples that occupancy='s classification would keep - the pad and the grid's
    `dilate` are the margins for that; the grid is a sampled approximation of the field; and the reference's 1e10 last interval is
    unchanged, so everything past the tightened far is treated as what the grid says it is: empty.  Refused before any GPU work: a
    grid on another device, a pad that is not finite or is below 0 (ValueError), ray_span_pad without ray_span (ValueError), and a
    call that wants gradients (RuntimeError: the tightening would cut the near/far gradient).  ray_span=None: the launches and the
    return are what they were."""
    span_pad = _check_ray_span("render_dex_depth", ray_span, ray_span_pad, [model_coarse, model_fine], ray_origins, ray_directions)
    if refine_steps is not None:
        _ops.check_refine_steps(refine_steps, "render_dex_depth: refine_steps")
        _ops.check_refine_thresholds(m_thres_cand, "render_dex_depth: refine_steps")
        if quantiles is not None or occupancy is not None:
            raise ValueError("render_dex_depth: refine_steps together with quantiles= or occupancy= is not supported")
        if float(getattr(options.nerf, mode).radiance_field_noise_std) != 0.0:
            raise ValueError("render_dex_depth: refine_steps brackets the raw density: the mode's radiance_field_noise_std must be 0")
    elif refine_width:
        raise ValueError("render_dex_depth: refine_width reports on a refinement: give refine_steps=")
    qs = None if quantiles is None else _ops.check_quantiles(quantiles, "render_dex_depth: quantiles")
    if occupancy is None and cull_stats:
        raise ValueError("render_dex_depth: cull_stats reports on a culled render: give occupancy=")
    if occupancy is not None:
        # every refusal of the culled path before any GPU work: the precision, the grid's device, then the setup's own
        prec = _culled_precision("render_dex_depth")
        occupancy.check_render(ray_directions.device, "render_dex_depth")
    r = _density_render_setup("render_dex_depth", "differentiable renders go through run_one_iter_of_nerf", height, width, focal_length,
                              model_coarse, model_fine, ray_origins, ray_directions, options, mode, encode_position_fn, m_thres_cand,
                              ray_span, span_pad)
    q_dev = _threshold_tensor(qs, r.dev) if qs else None   # (the same cache: one host-to-device copy per quantile set)
    if occupancy is not None:
        return _render_dex_depth_culled(r, prec, occupancy, q_dev, quantile_interp, cull_stats, getattr(options.nerf, mode).chunksize, mode)
    guard = _fp16_guard(r.models, density=True)
    # precision code -> the density packs: fetched once per pass over the chunks, not per chunk (a pass runs in one precision, and
    # the re-render after a trip in another - the configured one is never the guarded one - so it fetches its own)
    packs = {}

    def render_chunk(batch, status):
        prec, guarded = guard if status is not None else (_ops._precision, False)
        if prec not in packs:
            packs[prec] = _density_packs(r, prec)
        draws = _draws(batch.shape[0], r.nc, r.nf, r.fine, r.perturb, r.std, r.dev)
        depth_c, acc_c, depth_f, acc_f, dex, *more = _ops.render_rays_depth(*packs[prec], batch, r.nc, r.nf, r.lindisp, r.std, r.m_thres, draws,
                                                                            quantiles=q_dev, interp=quantile_interp, refine_steps=refine_steps,
                                                                            want_width=refine_width)
        maps = [depth_c, acc_c, depth_f, acc_f] + ([] if dex is None else [dex[k] for k in range(dex.shape[0])])
        for extra in more:   # qdepth (Q,N), or refined (K,N) and then width (K,N)
            maps += [extra[k] for k in range(extra.shape[0])]
        words = _ops.render_status_words()   # (copied for unguarded chunks too, as it always was: same launches on every path)
        if guarded:
            status.append(words)
        return maps
    maps = _render_chunks(r.rays, getattr(options.nerf, mode).chunksize, render_chunk)
    return _to_image(maps, [r.img_shape[:-1]] * len(maps)) if mode == "validation" else tuple(maps)


# ---- Dex depth layers ----------------------------------------------------------------------------------------------------------------
DexLayers = collections.namedtuple("DexLayers", "depth acc dex events count width")


def render_dex_layers(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options, mode="validation",
                      encode_position_fn=None, encode_direction_fn=None, m_thres_cand=None, layers=1, refine_steps=None, want_width=False,
                      ray_span=None, ray_span_pad=None, occupancy=None):
    """The depth-only render (render_dex_depth: density sub-networks, no colour) with EVERY entry into and exit from the region
    {sigma > m} along each ray, not the first entry alone (include/dexnerf_hip_layers.h): the back face and the wall thickness of a
    glass, the second wall of a hollow object, a floater in front of the surface as a thin first layer.

    Returns DexLayers(depth, acc, dex, events, count, width): depth, acc and dex (K, ...) are the last pass's maps - the fine pass's,
    or the coarse one's without a fine pass - with render_dex_depth's bits; events (K, 2L, ...) the depths of the first 2L events of
    every ray and threshold - events 0, 2, ... are entries, 1, 3, ... exits, +inf where the ray has no such event (a ray still inside
    the region at its last sample has an open last layer: an entry without an exit); count (K, ...) int32 the number of events of the
    ray, not capped at 2L; width (K, 2L, ...) with want_width=True, else None - the width of the bracket an event was read from, 0 for
    an entry at the first sample, -1 where there is no event.  The maps are image-shaped in validation mode and flat in train mode.

    refine_steps=None is the sample mode: an event's depth is that of the sample at which the state changes, as for the Dex depth -
    where count > 0, events[:, 0] carries dex's bits.  refine_steps=R, an int in 0 .. 24, is the interpolated mode: every event's
    bracket between two samples is halved R times on the last pass's density network (K*2L evaluations per ray and step) and
    interpolated linearly - events[:, 0] then carries the bits of render_dex_depth(refine_steps=R)'s refined maps where count > 0.  As
    there, a refined event is A crossing inside its sample bracket, and a layer thinner than the sample spacing can be stepped over.

    Judged here, on the host, before any GPU work (ValueError): layers that is not an int in 1 .. 8, no thresholds, a negative or
    non-finite threshold, more than 2048 records per ray (K * 2L), refine_steps that is not an int in 0 .. 24, a mode whose
    radiance_field_noise_std is not 0 (the events are those of the raw density).  Follows nerf.set_render_policy like render_dex_depth;
    no host read: a chunk can be captured into a HIP graph.  ray_span= / ray_span_pad=: render_dex_depth's.

    occupancy: an nerf.OccupancyGrid - sample mode only: each chunk goes through the culled depth chain
    (_ops.render_rays_depth_culled) with its last compositing launch replaced by the layers one; a culled sample's -FLT_MAX is "not
    above".  With refine_steps= it is refused, for render_dex_depth's reason: a culled sample's -FLT_MAX is not a density to
    interpolate with."""
    who = "render_dex_layers"
    span_pad = _check_ray_span(who, ray_span, ray_span_pad, [model_coarse, model_fine], ray_origins, ray_directions)
    _ops.check_layers(layers, f"{who}: layers")
    thres = _ops.check_refine_thresholds(m_thres_cand, who)
    if len(thres) * 2 * layers > _ops._hip.MAX_LAYER_RECORDS:
        raise ValueError(f"{who}: at most {_ops._hip.MAX_LAYER_RECORDS} records per ray (thresholds * 2 layers), got {len(thres)} * {2 * layers}")
    if refine_steps is not None:
        _ops.check_refine_steps(refine_steps, f"{who}: refine_steps")
        if occupancy is not None:
            raise ValueError(f"{who}: refine_steps together with occupancy= is not supported")
    if float(getattr(options.nerf, mode).radiance_field_noise_std) != 0.0:
        raise ValueError(f"{who}: the events are those of the raw density: the mode's radiance_field_noise_std must be 0")
    if occupancy is not None:
        culled_prec = _culled_precision(who)
        occupancy.check_render(ray_directions.device, who)
    r = _density_render_setup(who, "differentiable renders go through run_one_iter_of_nerf", height, width, focal_length, model_coarse,
                              model_fine, ray_origins, ray_directions, options, mode, encode_position_fn, m_thres_cand, ray_span, span_pad)
    chunksize = getattr(options.nerf, mode).chunksize
    last = slice(2, 4) if r.fine else slice(0, 2)

    def columns(maps):   # one chunk's (depth_c, acc_c, depth_f, acc_f, dex, events, count, width) -> rows to join: the ray axis first
        dex, events, count, wd = maps[4:]
        return list(maps[last]) + [dex.t(), events.permute(2, 0, 1), count.t()] + ([wd.permute(2, 0, 1)] if want_width else [])
    if occupancy is not None:
        packs = _density_packs(r, culled_prec)

        def render_culled(batch):
            draws = _draws(batch.shape[0], r.nc, r.nf, r.fine, r.perturb, r.std, r.dev)
            return columns(_ops.render_rays_depth_culled(*packs, batch, r.nc, r.nf, r.lindisp, r.std, r.m_thres, occupancy, draws, layers=layers,
                                                         want_width=want_width)[0])
        cols = _join_chunks([render_culled(batch) for batch in get_minibatches(r.rays, chunksize=chunksize)])
    else:
        guard = _fp16_guard(r.models, density=True)
        packs = {}   # precision code -> the density packs, as in render_dex_depth

        def render_chunk(batch, status):
            prec, guarded = guard if status is not None else (_ops._precision, False)
            if prec not in packs:
                packs[prec] = _density_packs(r, prec)
            draws = _draws(batch.shape[0], r.nc, r.nf, r.fine, r.perturb, r.std, r.dev)
            maps = _ops.render_rays_depth_layers(*packs[prec], batch, r.nc, r.nf, r.lindisp, r.std, r.m_thres, layers, refine_steps=refine_steps,
                                                 want_width=want_width, draws=draws)
            words = _ops.render_status_words()
            if guarded:
                status.append(words)
            return columns(maps)
        cols = _render_chunks(r.rays, chunksize, render_chunk)
    depth, acc, dex, events, count = cols[:5]
    shape = tuple(r.img_shape[:-1]) if mode == "validation" else (depth.shape[0],)
    k = dex.shape[1]
    return DexLayers(depth.reshape(shape), acc.reshape(shape), dex.t().reshape((k,) + shape),
                     events.permute(1, 2, 0).reshape((k, 2 * layers) + shape), count.t().reshape((k,) + shape),
                     cols[5].permute(1, 2, 0).reshape((k, 2 * layers) + shape) if want_width else None)


def dex_thickness(layers_result, layer=0):
    """exit - entry of layer `layer` of a DexLayers: (K, ...) like its dex maps; NaN where the ray has no such closed layer
    (count < 2 * layer + 2) - an open last layer among them.  Plain torch: a convenience, not a hot path."""
    events, count = layers_result.events, layers_result.count
    if isinstance(layer, bool) or not isinstance(layer, int) or not 0 <= layer < events.shape[1] // 2:
        raise ValueError(f"dex_thickness: layer must be an int in 0 .. {events.shape[1] // 2 - 1} (the layers stored), got {layer!r}")
    closed = count >= 2 * layer + 2
    return torch.where(closed, events[:, 2 * layer + 1] - events[:, 2 * layer], torch.full_like(events[:, 0], float("nan")))


# ---- density-gradient surface normals ------------------------------------------------------------------------------------------------
DexNormals =collections.namedtuple("DexNormals", "depth acc normal dex_depth dex_normal")


def _normals_precision(who):
    """Precision code of the differentiated density network: 'fp32' runs fp32, 'bf16' and 'bf16-s16' both run bf16 with 16-bit saved
    tensors; 'fp16' raises (there is no fp16 instance of the training kernels)."""
    if _ops._precision == _ops._hip.PREC_F16:
        raise RuntimeError(f"{who}: the density gradient runs on the training kernels, which exist for fp32 and bf16 - not under "
                           "nerf.set_precision('fp16')")
    return _ops._precision


def density_gradient(model, pts, encode_position_fn, chunksize=1 << 16):
    """The density field and its gradient at arbitrary points: (sigma (P,), grad (P,3)) for pts (..., 3) flattened to (P,3) - sigma the
    network's RAW density output (before noise and ReLU), grad = d sigma / d x in the network's input space (world space, or NDC space
    for forward-facing scenes; nothing converts it).  For surface extraction and planners; -grad / |grad| is the surface normal
    render_dex_normals composites.  No-grad only, device tensors only, `chunksize` points per launch chain; runs in nerf.set_precision's
    mode: 'fp32', or bf16 with 16-bit saved tensors ('bf16' and 'bf16-s16' alike); 'fp16' raises."""
    prec = _normals_precision("density_gradient")
    if _wants_grad(model) or inputs_need_grad(pts):
        raise RuntimeError("density_gradient is a no-grad evaluation: call it under torch.no_grad() (or with parameters and points that "
                           "do not require grad); gradients through the normals are second order and not provided")
    _require_device(pts, "density_gradient")
    _require_density_net(model, encode_position_fn, "density_gradient")
    lx = encode_position_fn.log_sampling
    pack = model.packed_density(lx, True, precision=prec)
    streams = model.packed_density_grad(lx, True, precision=prec)
    flat = pts.reshape(-1, 3).float()
    parts = [_ops.density_gradient(pack, streams, pts=batch) for batch in get_minibatches(flat, chunksize=int(chunksize))]
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p[0] for p in parts], dim=0), torch.cat([p[1] for p in parts], dim=0)


def _rays_within_workspace(packs, n, nc, nf, max_bytes):
    """The largest ray count <= n whose dn_render_normals_workspace_bytes stays at or below max_bytes."""
    need = _ops.render_normals_workspace_bytes(*packs, n, nc, nf)
    if need <= max_bytes:
        return n
    m = max(1, min(n, int(max_bytes // -(-need // n))))
    while m > 1 and _ops.render_normals_workspace_bytes(*packs, m, nc, nf) > max_bytes:
        m -= max(1, m // 64)
    if _ops.render_normals_workspace_bytes(*packs, m, nc, nf) > max_bytes:
        raise RuntimeError(f"render_dex_normals: max_workspace_bytes={max_bytes} does not hold one ray of {nc}+{nf} samples")
    return m


def render_dex_normals(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options,
                       mode="validation", encode_position_fn=None, encode_direction_fn=None, m_thres_cand=None,
                       max_workspace_bytes=2 ** 31, occupancy=None, cull_stats=False, ray_span=None, ray_span_pad=None):
    """render_dex_depth's last pass with surface normals: the density sub-network of the last pass (the fine one; the coarse one
    without a fine pass) is differentiated w.r.t. its input points, and n = -grad sigma_raw / |grad sigma_raw| is composited beside
    the depths (dn_render_rays_normals).

    Returns DexNormals(depth, acc, normal, dex_depth, dex_normal): depth / acc of the last pass; normal = sum_s w_s n_s with the
    compositing weights - NOT renormalised: its length is at most acc and works as a confidence; dex_depth / dex_normal: tuples of K
    maps, the Dex depth of threshold k and n at the same first-crossing sample, (0,0,0) where no sample crosses (the depth then
    falls back to z[0]; the zero vector is the only "no surface" marker).  Flat (N,) / (N,3) in train mode, image-shaped in
    validation mode (normals (H,W,3)).  Normals live in the network's input space: world space, or NDC space for forward-facing
    scenes (dataset.no_ndc False) - nothing converts them.

    Rays, chunking, NDC, lindisp and the perturb / noise draws (rand, randn, rand, randn per chunk) follow render_dex_depth.  The
    differentiated pass keeps its saved tensors: each chunk is split so that dn_render_normals_workspace_bytes stays at or below
    `max_workspace_bytes`; rays are independent, so the maps do not depend on the split.  No-grad only, device tensors only,
    networks the fused kernels cover only: anything else raises.  Precision follows nerf.set_precision: 'fp32' runs fp32, 'bf16' and
    'bf16-s16' both run bf16 with 16-bit saved tensors, 'fp16' raises - there is no fp16 instance of the training kernels, so the
    fp16 render policy (nerf.set_render_policy) and its range guard do not apply here.  The last pass's sigma comes from the
    training-forward kernel: depth may differ from render_dex_depth's in the last bits.

    occupancy: an nerf.OccupancyGrid on the rays' device - each chunk then goes through _ops.render_rays_normals_culled: the samples of
    both passes are classified against the grid, the coarse density network and the differentiated last pass (forward, backward-data
    chain, input gradient) run only on the kept ones; a culled sample composites as empty space with a zero gradient, the kernel's "no
    normal".  What render_dex_depth says of its grid holds here (space, level, noise, draws, two host reads per chunk, no HIP-graph
    capture); max_workspace_bytes then bounds the saved tensors of the kept points, which are differentiated in slabs (points are
    independent: the maps do not depend on the slabs), not the rays of a chunk.  cull_stats=True (with
    a grid only) returns (DexNormals, dict(kept=, total=, nonfinite=)).  occupancy=None: the launches and the return are what they
    were.

    ray_span: an nerf.OccupancyGrid on the rays' device - the ray rows are tightened to the occupied span of the grid once, before
    the chunk loop: render_dex_depth's ray_span=, with the same ray_span_pad, the same refusals and the same limits; it works with
    and without occupancy=.  ray_span=None: the launches and the return are what they were."""
    if occupancy is None and cull_stats:
        raise ValueError("render_dex_normals: cull_stats reports on a culled render: give occupancy=")
    span_pad = _check_ray_span("render_dex_normals", ray_span, ray_span_pad, [model_coarse, model_fine], ray_origins, ray_directions)
    prec = _normals_precision("render_dex_normals")
    if occupancy is not None:
        occupancy.check_render(ray_directions.device, "render_dex_normals")
    r = _density_render_setup("render_dex_normals", "gradients through the normals are second order and not provided", height, width,
                              focal_length, model_coarse, model_fine, ray_origins, ray_directions, options, mode, encode_position_fn,
                              m_thres_cand, ray_span, span_pad)
    nc, nf = r.nc, r.nf
    k = 0 if r.m_thres is None else int(r.m_thres.numel())
    packs = _density_packs(r, prec)
    streams = r.models[-1].packed_density_grad(r.lx, True, precision=prec)
    max_bytes = int(max_workspace_bytes)

    def render_chunk(batch):
        n = batch.shape[0]
        draws = _draws(n, nc, nf, r.fine, r.perturb, r.std, r.dev)
        step = _rays_within_workspace(packs, n, nc, nf, max_bytes)
        pieces = []
        for r0 in range(0, n, step):
            rows = slice(r0, min(r0 + step, n))
            _, _, depth, acc, dex, normal, dex_normal = _ops.render_rays_normals(
                *packs, streams, batch[rows], nc, nf, r.lindisp, r.std, r.m_thres, {name: d[rows] for name, d in draws.items()})
            pieces.append([depth, acc, normal] + [dex[i] for i in range(k)] + [dex_normal[i] for i in range(k)])
        return _join_chunks(pieces)
    totals = _CullTotals(cull_stats)
    max_points = max(1, max_bytes // _ops.density_gradient_bytes_per_point(packs[1] if r.fine else packs[0])) if occupancy is not None else None

    def render_chunk_culled(batch):
        draws = _draws(batch.shape[0], nc, nf, r.fine, r.perturb, r.std, r.dev)
        (_, _, depth, acc, dex, normal, dex_normal), stats = _ops.render_rays_normals_culled(
            *packs, streams, batch, nc, nf, r.lindisp, r.std, r.m_thres, occupancy, draws, count_nonfinite=cull_stats, max_points=max_points)
        totals.add(stats)
        return [depth, acc, normal] + [dex[i] for i in range(k)] + [dex_normal[i] for i in range(k)]
    one_chunk = render_chunk if occupancy is None else render_chunk_culled
    maps = _join_chunks([one_chunk(batch) for batch in get_minibatches(r.rays, chunksize=getattr(options.nerf, mode).chunksize)])
    if mode == "validation":
        flat, vec = r.img_shape[:-1], r.img_shape
        maps = _to_image(maps, [flat, flat, vec] + [flat] * k + [vec] * k)
    out = DexNormals(maps[0], maps[1], maps[2], tuple(maps[3:3 + k]), tuple(maps[3 + k:3 + 2 * k]))
    return (out, totals.result()) if cull_stats else out


# ---- the Dex threshold surface as a triangle mesh -------------------------------------------------------------------------------------
DexMesh = collections.namedtuple("DexMesh", "vertices triangles normals n_nonfinite")


def _grid_axes(bounds, resolution, who):
    """bounds (x0,y0,z0,x1,y1,z1) and resolution N | (nx,ny,nz) -> three host fp32 coordinate tensors (float64 linspace, rounded once),
    checked by the rule of the extraction (finite, strictly increasing, >= 2 per axis)."""
    b = [float(v) for v in bounds]
    res = [int(resolution)] * 3 if isinstance(resolution, (int, np.integer)) else [int(r) for r in resolution]
    if len(b) != 6 or len(res) != 3:
        raise ValueError(f"{who}: bounds are (x0, y0, z0, x1, y1, z1) and resolution is N or (nx, ny, nz)")
    if min(res) < 2 or not all(np.isfinite(b)):
        raise ValueError(f"{who}: needs finite bounds and at least 2 grid points per axis")
    axes = [torch.from_numpy(np.linspace(b[a], b[a + 3], res[a]).astype(np.float32)) for a in range(3)]
    _ops.check_isosurface_grid(*axes, 0.0, who)
    return axes


def _density_pack(model, encode_position_fn, who):
    """The guards of density_gradient, then the density pack in nerf.set_precision's mode."""
    prec = _normals_precision(who)
    if _wants_grad(model):
        raise RuntimeError(f"{who} is a no-grad evaluation: call it under torch.no_grad() (or with parameters that do not require grad)")
    _require_density_net(model, encode_position_fn, who)
    return model.packed_density(encode_position_fn.log_sampling, True, precision=prec)


def density_grid(model, encode_position_fn, bounds, resolution, max_points=1 << 24):
    """The network's RAW density (before noise and ReLU: what the Dex readout compares with m_thres) on a regular grid:
    (field (nx,ny,nz) fp32, xs (nx), ys (ny), zs (nz)) on the model's device, field[i,j,k] = sigma_raw(xs[i], ys[j], zs[k]).  bounds =
    (x0, y0, z0, x1, y1, z1), resolution = N or (nx, ny, nz); the coordinates are float64 linspaces rounded to fp32 once, end points
    included.  The density pack (FlexibleNeRFModel.packed_density) runs through dn_run_network on explicit points - every grid point
    fed to the network is bit-exactly (xs[i], ys[j], zs[k]) - in slabs of at most `max_points` points written into one dense field; points
    are independent, so the field does not depend on the slabs.  The grid lives in the network's input space: world space, or NDC
    space for forward-facing scenes; nothing converts it.  Runs in nerf.set_precision's mode, 'fp32' or bf16; 'fp16' raises, as in
    density_gradient.  No-grad only, device tensors only, networks the fused kernels cover only: anything else raises."""
    pack = _density_pack(model, encode_position_fn, "density_grid")
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("density_grid: max_points must be at least 1")
    dev = model.layer1.weight.device
    xs, ys, zs = (a.to(dev) for a in _grid_axes(bounds, resolution, "density_grid"))
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    total = nx * ny * nz
    field = torch.empty(total, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for p0 in range(0, total, max_points):
            idx = torch.arange(p0, min(p0 + max_points, total), dtype=torch.int64, device=dev)
            plane = torch.div(idx, nz, rounding_mode="floor")
            pts = torch.stack([xs[torch.div(plane, ny, rounding_mode="floor")], ys[plane % ny], zs[idx % nz]], dim=-1)
            field[p0:p0 + pts.shape[0]] = _ops.run_network_pts(pack, pts, None, 1)[:, 3]
    return field.view(nx, ny, nz), xs, ys, zs


def extract_dex_mesh(model, encode_position_fn, bounds, resolution, m_thres, normals=True, max_points=1 << 24):
    """The Dex surface as one object: the boundary of {x : sigma_raw(x) > m_thres} - the region whose samples the Dex depth readout
    calls "hit" - as an indexed, watertight, consistently oriented triangle mesh, DexMesh(vertices (V,3) fp32, triangles (T,3) int32,
    normals (V,3) fp32 | None, n_nonfinite).  density_grid samples the field, _ops.isosurface extracts it on the device (marching
    tetrahedra; the definition, the fixed vertex and triangle order and the orientation - geometric normals toward decreasing density
    - are those of include/dexnerf_hip_mesh.h).  normals=True adds the analytic vertex normals -g/|g| with g = d sigma_raw / d x at
    the vertices (_ops.density_gradient, in chunks), by composite_normals' conventions: |g| formed in fp64, the zero vector where |g| is
    zero or not finite.  n_nonfinite counts the grid samples that were not finite (they emit nothing).  The mesh lives in the network's
    input space: world space, or NDC space for forward-facing scenes; nothing converts it.  An empty surface is a valid result: (0,3)
    tensors.  Precision and guards as density_grid; other thresholds on the same field: call _ops.isosurface on density_grid's result."""
    level = float(m_thres)
    if not np.isfinite(np.float32(level)):
        raise ValueError(f"extract_dex_mesh: m_thres must be finite as fp32, got {m_thres!r}")
    pack = _density_pack(model, encode_position_fn, "extract_dex_mesh")
    field, xs, ys, zs = density_grid(model, encode_position_fn, bounds, resolution, max_points=max_points)
    vertices, triangles, n_bad = _ops.isosurface(field, xs, ys, zs, level)
    vertex_normals = None
    if normals:
        streams = model.packed_density_grad(encode_position_fn.log_sampling, True, precision=pack.precision)
        parts = [_ops.density_gradient(pack, streams, pts=batch)[1] for batch in get_minibatches(vertices, chunksize=1 << 16)]
        g = (torch.cat(parts, dim=0) if parts else vertices.new_zeros((0, 3))).double()
        length = torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
        ok = torch.isfinite(length) & (length > 0)
        vertex_normals = torch.where(ok[:, None], -g / torch.where(ok, length, torch.ones_like(length))[:, None], torch.zeros_like(g)).float()
    return DexMesh(vertices, triangles, vertex_normals, n_bad)


def save_ply(path, mesh):
    """Binary little-endian PLY of a DexMesh (or anything with .vertices (V,3), .triangles (T,3) and optional .normals (V,3); tensors
    or arrays): x y z [nx ny nz] as float32, faces as a uchar count and three int32 indices.  Host code, no dependency."""
    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = np.ascontiguousarray(host(mesh.vertices), dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(host(mesh.triangles), dtype="<i4").reshape(-1, 3)
    n = getattr(mesh, "normals", None)
    props = ["x", "y", "z"]
    if n is not None:
        n = np.ascontiguousarray(host(n), dtype="<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("save_ply: normals must match the vertices")
        v = np.concatenate([v, n], axis=1)
        props += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", "comment Dex threshold surface", f"element vertex {len(v)}"]
    header += [f"property float {p}" for p in props]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    faces = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"], faces["v"] = 3, t
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.astype("<f4").tobytes())
        fh.write(faces.tobytes())
