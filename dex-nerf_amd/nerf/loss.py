"""The loss head of the training loop under autograd: weighted mse(rgb_coarse) + mse(rgb_fine) plus a masked depth term, value and
gradients from ONE kernel launch (dn_render_loss).  FusedTrainStep / FusedPoseStep call the same head without an autograd graph.
distortion_loss: the distortion regulariser of compositing's weights (dn_distortion_loss) under autograd."""
import torch

from . import _hip, _ops
from .nerf_helpers import _require_device


def loss_head_settings(who, depth_images, loss_weights, depth_weights, depth_range, shape=None, ndc=False, colour_weights_positive=False):
    """The loss-head arguments of a fused step (FusedTrainStep / FusedPoseStep), validated.  None when they are all at their defaults:
    the step then keeps the reference's head, dn_mse2_loss.  `shape`: the (V,H,W) the depth maps must have.  Else a dict(depth_images (V,H,W) fp32 on the device | None, weights,
    depth_weights, depth_range) for _ops.render_loss.  Raises ValueError on settings the step cannot honour."""
    weights, d_weights = tuple(float(w) for w in loss_weights), tuple(float(w) for w in depth_weights)
    d_range = tuple(float(x) for x in depth_range)
    if len(weights) != 2 or len(d_weights) != 2 or len(d_range) != 2:
        raise ValueError(f"{who}: loss_weights, depth_weights and depth_range are pairs (coarse, fine) / (lo, hi)")
    if depth_images is None and weights == (1.0, 1.0) and d_weights == (0.0, 0.0):
        return None
    finite = all(w == w and abs(w) != float("inf") for w in weights + d_weights)
    if not finite or min(weights + d_weights) < 0.0:
        raise ValueError(f"{who}: loss_weights / depth_weights must be finite and >= 0 (got {weights}, {d_weights})")
    if colour_weights_positive and min(weights) <= 0.0:
        raise ValueError(f"{who}: both loss_weights must be > 0 on the training step (got {weights}): its default 8-bit mode scales the "
                         "saved gradients per launch from the largest upstream gradient")
    if weights == (0.0, 0.0) and d_weights == (0.0, 0.0):
        raise ValueError(f"{who}: every loss weight is zero")
    if max(d_weights) > 0.0:
        if depth_images is None:
            raise ValueError(f"{who}: depth_weights {d_weights} need depth_images")
        if ndc:
            raise ValueError(f"{who}: no depth term on NDC rows - an NDC depth is not metric (depth_weights {d_weights})")
    if d_range[0] != d_range[0] or d_range[1] != d_range[1]:
        raise ValueError(f"{who}: depth_range must not hold NaN")
    if depth_images is not None:
        if depth_images.dim() != 3:
            raise ValueError(f"{who}: depth_images is (V,H,W) (got {tuple(depth_images.shape)})")
        if shape is not None and tuple(depth_images.shape) != tuple(int(x) for x in shape):
            raise ValueError(f"{who}: depth_images of shape {tuple(depth_images.shape)} for {shape[0]} views of {shape[1]} x {shape[2]}")
        _require_device(depth_images, who)
        depth_images = _hip.f32c(depth_images.detach())
    return dict(depth_images=depth_images, weights=weights, depth_weights=d_weights, depth_range=d_range)


EXPOSURE_MODES = {None: 0, "gain": 1, "affine": 6}      # refine_exposure -> P, the floats of a view's exposure row


def exposure_settings(who, n_views, refine_exposure, exposure_scale, exposure_fixed_views):
    """The checked (mode, P, scale, mask as a list of V 0 / 1 - 0: the row is held) of a fused step's exposure refinement.  Raises
    ValueError; asks for no device."""
    if refine_exposure not in EXPOSURE_MODES:
        raise ValueError(f"{who}: refine_exposure is None, 'gain' or 'affine' (got {refine_exposure!r})")
    try:
        scale = float(exposure_scale)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: exposure_scale must be a positive finite number (got {exposure_scale!r})") from None
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"{who}: exposure_scale must be a positive finite number (got {exposure_scale!r})")
    fixed = [int(v) for v in exposure_fixed_views]
    if any(v < 0 or v >= n_views for v in fixed):
        raise ValueError(f"{who}: exposure_fixed_views {fixed} out of range for {n_views} views")
    if refine_exposure is None and fixed:
        raise ValueError(f"{who}: exposure_fixed_views {fixed} without refine_exposure")
    return refine_exposure, EXPOSURE_MODES[refine_exposure], scale, [0 if v in fixed else 1 for v in range(n_views)]


def apply_exposure(rgb, eps_row, mode, scale=1.0):
    """A render (..., 3) in one view's exposure: exp(s a) rgb for mode "gain" (eps_row = [a]), exp(s a_k) rgb_k + s b_k for "affine"
    (eps_row = [a_r, a_g, a_b, b_r, b_g, b_b]), s = scale - what the loss head of a step with refine_exposure compares with that view's
    pixels.  Plain torch on any device, differentiable; for showing or scoring a render, not a hot path."""
    if mode not in ("gain", "affine"):
        raise ValueError(f"apply_exposure: mode is 'gain' or 'affine' (got {mode!r})")
    row = torch.as_tensor(eps_row, dtype=rgb.dtype, device=rgb.device).reshape(-1)
    if row.numel() != EXPOSURE_MODES[mode]:
        raise ValueError(f"apply_exposure: a {mode!r} row holds {EXPOSURE_MODES[mode]} numbers (got {row.numel()})")
    if mode == "gain":
        return torch.exp(scale * row[0]) * rgb
    return torch.exp(scale * row[:3]) * rgb + scale * row[3:]


def fused_loss_head(head, maps, target, rng_state, luminance=False, pixel_index=None, view_index=None, view=None, exposure=None):
    """The loss head of a fused step on the maps of render_rays_train: dn_mse2_loss for head None (loss_head_settings), else
    dn_render_loss with the depth targets gathered from head["depth_images"] at (view_index | view, pixel_index).  Returns (loss3,
    loss6 | None, g_c, g_f): loss6 = [loss, mse_c, mse_f, D_c, D_f, valid rays], loss3 its first three words; g_c / g_f the upstream
    (g_rgb, g_depth, g_acc) of the coarse / fine maps - no depth gradient where its weight is 0 (the backward of a photometric step).
    `exposure` (a step that refines it): dict(eps (V,P), scale, mask (V) int32 | None, grad (V,P)) - dn_render_loss_exposure in the place
    of either head (head None: its weights are (1, 1), no depth term), the rows' gradient written into exposure["grad"]; loss6 always."""
    if exposure is not None:
        h = head or dict(depth_images=None, weights=(1.0, 1.0), depth_weights=(0.0, 0.0), depth_range=(0.0, float("inf")))
        gather = h["depth_images"] is not None
        loss6, g_c, g_f, gd_c, gd_f, _ = _ops.render_loss_exposure(
            maps[0], maps[3], target, exposure["eps"], exposure["scale"], view_index, view if view_index is None else None, exposure["mask"],
            maps[1] if gather else None, maps[4] if gather else None, h["depth_images"], pixel_index if gather else None, h["weights"],
            h["depth_weights"], h["depth_range"], luminance, rng_state, g_eps=exposure["grad"])
        w_c, w_f = h["depth_weights"]
        return loss6[:3], loss6, (g_c, gd_c if w_c != 0.0 else None, None), (g_f, gd_f if w_f != 0.0 else None, None)
    if head is None:
        loss3, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target, luminance, rng_state)
        return loss3, None, (g_c, None, None), (g_f, None, None)
    gather = head["depth_images"] is not None
    loss6, g_c, g_f, gd_c, gd_f = _ops.render_loss(
        maps[0], maps[3], target, maps[1], maps[4], head["depth_images"], pixel_index if gather else None, view_index if gather else None,
        view if (gather and view_index is None) else None, head["weights"], head["depth_weights"], head["depth_range"], luminance, rng_state)
    w_c, w_f = head["depth_weights"]
    return loss6[:3], loss6, (g_c, gd_c if w_c != 0.0 else None, None), (g_f, gd_f if w_f != 0.0 else None, None)


class RenderLossFn(torch.autograd.Function):
    """(rgb_c, rgb_f | None, depth_c | None, depth_f | None) -> (loss (), loss6 (6)).  The forward runs dn_render_loss and keeps the
    gradients it wrote; the backward multiplies them by grad_output."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, depth_c, depth_f, target, target_depth, weights, depth_weights, depth_range, luminance):
        loss6, *grads = _ops.render_loss(rgb_c.detach(), None if rgb_f is None else rgb_f.detach(), target,
                                         None if depth_c is None else depth_c.detach(), None if depth_f is None else depth_f.detach(),
                                         target_depth, weights=weights, depth_weights=depth_weights, depth_range=depth_range,
                                         luminance=luminance)
        ctx.present = [g is not None for g in grads]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(loss6)
        return loss6[0].clone(), loss6

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_terms):
        saved = iter(ctx.saved_tensors)
        out = []
        for present, needs in zip(ctx.present, ctx.needs_input_grad[:4]):
            g = next(saved) if present else None
            out.append(g * g_loss if (g is not None and needs) else None)
        return tuple(out) + (None,) * 6


class RenderLossExposureFn(torch.autograd.Function):
    """RenderLossFn with the exposure rows as a fifth differentiable input: (rgb_c, rgb_f | None, depth_c | None, depth_f | None,
    exposure (V,P)) -> (loss (), loss6 (6)).  The forward runs dn_render_loss_exposure and keeps the gradients it wrote."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, depth_c, depth_f, exposure, view_index, scale, target, target_depth, weights, depth_weights, depth_range,
                luminance):
        loss6, *grads = _ops.render_loss_exposure(rgb_c.detach(), None if rgb_f is None else rgb_f.detach(), target, exposure.detach(), scale,
                                                  view_index, None, None, None if depth_c is None else depth_c.detach(),
                                                  None if depth_f is None else depth_f.detach(), target_depth, None, weights, depth_weights,
                                                  depth_range, luminance, want_eps=ctx.needs_input_grad[4])
        ctx.present = [g is not None for g in grads]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(loss6)
        return loss6[0].clone(), loss6

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_terms):
        saved = iter(ctx.saved_tensors)
        out = []
        for present, needs in zip(ctx.present, ctx.needs_input_grad[:5]):
            g = next(saved) if present else None
            out.append(g * g_loss if (g is not None and needs) else None)
        return tuple(out) + (None,) * 8


def render_loss(rgb_c, rgb_f, target, depth_c=None, depth_f=None, target_depth=None, weights=(1.0, 1.0), depth_weights=(0.0, 0.0),
                depth_range=(0.0, float("inf")), luminance=False, exposure=None, view_index=None, exposure_mode=None, exposure_scale=1.0):
    """weights[0] mse(rgb_c, target) + weights[1] mse(rgb_f, target) + depth_weights[0] D(depth_c) + depth_weights[1] D(depth_f), with
    D(depth) the mean of (depth - target_depth)^2 over the rays whose target depth lies inside depth_range (exclusive; NaN: outside).
    `luminance`: the IR head (both colour sides through 0.299 r + 0.587 g + 0.114 b).  rgb_f / depth_f may be None (coarse only);
    target_depth None: no depth term.  Returns the scalar loss, differentiable in the four maps; its `.terms` is the device tensor
    [loss, mse_coarse, mse_fine, D_coarse, D_fine, number of valid rays].  Device tensors only.

    `exposure` (V,1) | (V,6) with `view_index` (N) int32: the colours of ray i enter the colour terms as apply_exposure(rgb[i],
    exposure[view_index[i]], mode, exposure_scale) (dn_render_loss_exposure; `exposure_mode` "gain" | "affine", None: by the row length);
    the loss is then differentiable in `exposure` as well.  None: the head above, untouched."""
    if exposure is not None:
        if view_index is None:
            raise ValueError("render_loss: exposure needs view_index (the view of every ray)")
        mode = exposure_mode if exposure_mode is not None else {1: "gain", 6: "affine"}.get(int(exposure.shape[-1]) if exposure.dim() == 2 else -1)
        if mode not in ("gain", "affine") or exposure.dim() != 2 or int(exposure.shape[1]) != EXPOSURE_MODES[mode]:
            raise ValueError(f"render_loss: exposure is (V,1) for exposure_mode 'gain', (V,6) for 'affine' (got {tuple(exposure.shape)}, "
                             f"{exposure_mode!r})")
        if not 0.0 < float(exposure_scale) < float("inf"):
            raise ValueError(f"render_loss: exposure_scale must be a positive finite number (got {exposure_scale!r})")
    elif view_index is not None or exposure_mode is not None:
        raise ValueError("render_loss: view_index / exposure_mode without exposure")
    for t in (rgb_c, rgb_f, target, depth_c, depth_f, target_depth, exposure, view_index):
        if t is not None:
            _require_device(t, "render_loss")
    if target_depth is None:
        depth_c = depth_f = None
    elif depth_c is None:
        raise ValueError("render_loss: target_depth needs depth_c")
    n = rgb_c.reshape(-1, 3).shape[0]
    flat = [rgb_c.reshape(n, 3), None if rgb_f is None else rgb_f.reshape(n, 3), None if depth_c is None else depth_c.reshape(n),
            None if depth_f is None else depth_f.reshape(n)]
    rest = (target.detach().reshape(n, -1)[:, :3], None if target_depth is None else target_depth.detach().reshape(n), tuple(weights),
            tuple(depth_weights), tuple(depth_range), bool(luminance))
    if exposure is None:
        loss, terms = RenderLossFn.apply(*flat, *rest)
    else:
        loss, terms = RenderLossExposureFn.apply(*flat, _hip.f32c(exposure), view_index.detach().reshape(n), float(exposure_scale), *rest)
    loss.terms = terms
    return loss


def distortion_weight_settings(who, distortion_weights):
    """(coarse, fine) weights of the distortion regulariser on a fused step, validated: finite and >= 0, else ValueError."""
    try:
        weights = tuple(float(w) for w in distortion_weights)
    except TypeError:
        raise ValueError(f"{who}: distortion_weights is a pair (coarse, fine) (got {distortion_weights!r})") from None
    if len(weights) != 2:
        raise ValueError(f"{who}: distortion_weights is a pair (coarse, fine) (got {distortion_weights!r})")
    if not all(w == w and abs(w) != float("inf") and w >= 0.0 for w in weights):
        raise ValueError(f"{who}: distortion_weights must be finite and >= 0 (got {weights})")
    return weights


class DistortionLossFn(torch.autograd.Function):
    """(weights (N,S), z (N,S)) -> mean over the rays of L_ray.  The forward runs dn_distortion_loss with scale = 1 / N and keeps the
    gradients it wrote; the backward multiplies them by grad_output."""

    @staticmethod
    def forward(ctx, weights, z, near_far):
        n = z.shape[0]
        mean, _, g_w, g_z = _ops.distortion_loss(weights.detach(), z.detach(), near_far, scale=1.0 / max(n, 1), want_z=ctx.needs_input_grad[1])
        ctx.save_for_backward(g_w, *([g_z] if g_z is not None else []))
        return mean[0].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        g_w, *g_z = ctx.saved_tensors
        return (g_w * g_loss if ctx.needs_input_grad[0] else None, g_z[0] * g_loss if (g_z and ctx.needs_input_grad[1]) else None, None)


def distortion_loss(weights, z_vals, near, far):
    """The distortion regulariser of mip-NeRF 360 on the weights (..., S) volume_render_radiance_field returns and their depths
    z_vals (..., S), S <= 1024: the mean over the rays of sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i, with compositing's
    interval midpoints m and lengths delta (the last, open interval has length 0) in units of far - near.  near / far: numbers or
    per-ray tensors (...); they get no gradient, and a ray without far > near contributes zero.  Differentiable in weights and z_vals
    (tied depths: the subgradient of their order).  Device tensors only."""
    _require_device(weights, "distortion_loss")
    _require_device(z_vals, "distortion_loss")
    s = z_vals.shape[-1]
    w2, z2 = weights.reshape(-1, s), z_vals.reshape(-1, s)
    n = z2.shape[0]
    cols = [torch.as_tensor(v, dtype=torch.float32, device=z2.device).detach().reshape(-1).expand(n) for v in (near, far)]
    return DistortionLossFn.apply(w2, z2, torch.stack(cols, dim=1).contiguous())
