"""Tensor-level wrappers over the C ABI (one function per entry point) + autograd glue.

Every function here requires ROCm device tensors and calls straight into libdexnerf_hip.so; there is
no alternative implementation behind them.
"""
import collections
import ctypes
import math
import types
from ctypes import c_void_p

import torch

from . import _hip
from ._hip import MlpDesc, check, f32c, host_floats, lib, ptr, stream

_precision = _hip.PREC_F32
_save8 = False   # bf16 training keeps its saved activations / gradients at 8 bits (the 'bf16' mode; 'bf16-s16' keeps 16)


def set_precision(name):
    """'fp32' (exact fp32 MFMA chains, the parity mode); 'bf16' (bf16 MFMA, fp32 accumulate; render + training - the TRAINING step
    stores what it saves for the backward at 8 bits where the 48-point training kernels cover the network (widths 128 / 256, depth <= 9
    with view directions): activations as e4m3, layer gradients as e5m2 x a power-of-two scale chosen per launch from the largest
    upstream gradient, weight gradients formed with the fp8 MFMA - half the saved-tensor traffic of 16-bit saves, same forward bits;
    'bf16-s8' is the older name of this mode); 'bf16-s16' (bf16 with 16-bit saved tensors on the 32-point training kernels: what
    'bf16' meant up to round 3, and what 'bf16' falls back to for networks the 48-point training kernels do not cover); 'fp16' (fp16
    MFMA at bf16's rate with a 10-bit mantissa: ~57 dB instead of ~42 dB against fp32; render only - training in this mode
    differentiates the nn.Linear composition).  Rendering is identical in the three bf16 modes."""
    global _precision, _save8
    name = str(name).lower().replace("_", "-")
    _save8 = name in ("bf16", "bf16-s8")
    _precision = {"fp32": _hip.PREC_F32, "f32": _hip.PREC_F32, "bf16": _hip.PREC_BF16, "fp16": _hip.PREC_F16,
                  "f16": _hip.PREC_F16, "bf16-s8": _hip.PREC_BF16, "bf16-s16": _hip.PREC_BF16}[name]


_render16 = [None]   # what no-grad renders run in the bf16 modes: None = the environment decides (default "fp16")


def set_render_policy(name):
    """What `predict_and_render_radiance` WITHOUT autograd (validation images, the Dex depth sweep, eval_nerf) runs while the
    precision is 'bf16' / 'bf16-s8': "fp16" (default) = the fp16 instance of the same kernel - same matrix rate and layouts, a
    10-bit mantissa: ~58 dB / 0.997 Dex-depth agreement against fp32 where bf16 gives ~42 dB / 0.976, because the Dex readout
    is an argmax over thresholded sigma - guarded against fp16's range (65504): a render whose raw radiance field holds a
    non-finite value is repeated in bf16, with one warning; "bf16" = renders in bf16 like the training kernels.  The
    environment variable DEXNERF_BF16_RENDER sets the default.  Training is never affected."""
    name = None if name is None else str(name).lower()
    if name not in (None, "fp16", "bf16"):
        raise ValueError("render policy: 'fp16', 'bf16' or None (environment default)")
    _render16[0] = name


def get_render_policy():
    import os
    name = _render16[0] or os.environ.get("DEXNERF_BF16_RENDER", "fp16").lower()
    return name if name in ("fp16", "bf16") else "fp16"


def render_precision():
    """Precision code of no-grad renders under the current precision + render policy."""
    if _precision == _hip.PREC_BF16 and get_render_policy() == "fp16":
        return _hip.PREC_F16
    return _precision


def fp16_range_guard(model, density=False):
    """True when an fp16 render of this FlexibleNeRFModel reports every hidden activation that leaves fp16's range
    (dn_fp16_range_guard: the kernel instances that carry the tracker) - the condition for the fp16 render policy.
    density=True: the same question for its density sub-network (render_dex_depth)."""
    desc = _desc(model.desc_kwargs())
    return bool(lib().dn_fp16_range_guard(ctypes.byref(_density_desc(desc) if density else desc)))


def get_precision():
    if _precision == _hip.PREC_BF16:
        return "bf16" if _save8 else "bf16-s16"
    return {_hip.PREC_F32: "fp32", _hip.PREC_F16: "fp16"}[_precision]


def train_precision(packed):
    """The precision code the TRAINING entry points get for this packed network: DN_PREC_BF16_S8 in the 'bf16-s8' mode where the
    48-point training kernels cover the network (other shapes train in plain bf16).  A forward records it with what it saves; the
    backward of those buffers uses the recorded code."""
    if _save8 and packed.precision == _hip.PREC_BF16 and s8_supported(packed):
        return _hip.PREC_BF16_S8
    return packed.precision


def set_s8_grad_scale(scale):
    """Power of two the saved layer gradients are multiplied by before they are rounded to e5m2, or 0 (the DEFAULT): every
    backward-data launch takes the power of two that puts ITS largest finite upstream gradient at 2^12 (one small maximum kernel per
    launch) - whatever the loss's reduction or scaling.  A fixed scale, e.g. 65536 = 2^16, saves that kernel: with 2^16, per-point
    gradients dL/d(pre-activation) between 2.3e-10 (e5m2's smallest subnormal / 2^16; smaller ones flush to zero) and 0.87
    (57344 / 2^16; larger ones saturate) are representable, 2 mantissa bits each - the range of a mean-reduced MSE loss over
    10^3 .. 10^5 rays from the first iteration to > 40 dB; s8_grad_stats tells whether a fixed scale fits."""
    check(lib().dn_set_s8_grad_scale(float(scale)), "dn_set_s8_grad_scale")


def adam_step(params, grads, exp_avg, exp_avg_sq, state, lr, lr_decay_per_step, betas, eps, zero_grads):
    """dn_adam_step on flat fp32 buffers (nerf.parallel.FlatAdam).  lr: float or device scalar."""
    lr_t = lr if torch.is_tensor(lr) else None
    check(lib().dn_adam_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), ptr(state), ptr(lr_t),
                             0.0 if lr_t is not None else float(lr), float(lr_decay_per_step), float(betas[0]), float(betas[1]),
                             float(eps), int(bool(zero_grads)), stream()), "dn_adam_step")


S8_RECORD_BYTES = 256     # kS8BlockBytes, csrc/mlp_geo48.h: the record behind the 8-bit saved gradients of a launch
_s8_records = []          # device views of the records of the latest backward launches (bounded; read by s8_grad_stats)


def _note_s8_record(grads, prec):
    if prec == _hip.PREC_BF16_S8 and grads is not None:
        _s8_records.append(grads[-S8_RECORD_BYTES:].view(torch.int32))   # (a view: keeps that buffer's storage until two later launches)
        del _s8_records[:-2]


def s8_grad_stats(grads=None):
    """What the 8-bit saved gradients of the latest training step lost to e5m2's range (include/dexnerf_hip.h, "8-bit saved
    tensors"): of the sampled non-zero gradient bytes (one 32-point record in sixteen, every layer), the fraction at e5m2's largest
    magnitude (saturated: clipped at 57344 / scale) and at its smallest (the edge of flushing to zero), plus the scale in use.
    grads = one saved-gradient buffer, or None = the buffers of the latest backward launches together.  Synchronises (a host
    read): call it at a logging interval, not every iteration.  None when no 8-bit backward has run."""
    recs = [grads[-S8_RECORD_BYTES:].view(torch.int32)] if grads is not None else list(_s8_records)
    if not recs:
        return None
    rows = torch.stack([r[:40] for r in recs]).cpu()
    # eight replicas of (saturated, floor, sampled) at words 8 + 4 r (csrc/mlp_geo48.h): a workgroup adds to one of them
    sat, floor, sampled = (int(rows[:, 8 + k:40:4].sum()) for k in (0, 1, 2))
    scales = sorted({float(v) for v in rows[:, 4].contiguous().view(torch.float32).tolist()})
    return {"saturated": sat / max(sampled, 1), "floor": floor / max(sampled, 1), "sampled": sampled, "scale": scales}


# ---- marshalling: each rule of the C ABI's calling convention once -----------------------------------------------------
def _desc(desc_kwargs):
    return MlpDesc(**{k: int(v) for k, v in desc_kwargs.items()})


def _density_desc(full):
    """Descriptor of the density sub-network (trunk + fc_alpha, no view directions) of the network `full` describes."""
    desc = MlpDesc()
    check(lib().dn_mlp_density_desc(ctypes.byref(full), ctypes.byref(desc)), "dn_mlp_density_desc")
    return desc


def _sized(nbytes, what):
    """A *_bytes answer of the library; 0 means the shape is outside the kernels: raise its error."""
    if nbytes == 0:
        check(-1001, what)
    return nbytes


def _ptr_array(tensors, sources=False):
    """(void* array of the tensors' device pointers, the tensors it points at).  sources=True: parameters a pack kernel reads -
    detached and made fp32-contiguous first (possibly copies): the caller keeps the returned list alive until that kernel has
    run on this stream.  Otherwise the pointers are those of the very tensors given (outputs: dense views)."""
    if sources:
        tensors = [f32c(t.detach()) for t in tensors]
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), tensors


def _view_ptrs(views):
    """The (dW pointers, db pointers) arrays of [(dW, db)] in linear_modules() order; (None, None) for None."""
    if views is None:
        return None, None
    return _ptr_array([w for w, _ in views])[0], _ptr_array([b for _, b in views])[0]


def _dir_rows(rd):
    """(pointer, row stride in floats, the tensor to keep until the launch) of ray directions: an fp32 (N,3)-like view whose last
    dim is contiguous goes as it is (a column slice of the ray rows: no copy), anything else as a contiguous fp32 copy."""
    if not (rd.dtype == torch.float32 and rd.dim() == 2 and rd.stride(1) == 1):
        rd = f32c(rd).reshape(-1, 3)
    assert rd.is_cuda
    return c_void_p(rd.data_ptr()), int(rd.stride(0)), rd


def _draw_tensors(draws):
    """(t_rand, noise_c, u, noise_f) of a ray chunk's `draws` dict as fp32-contiguous tensors, None where not drawn - the order
    of the render entry points' arguments."""
    given = draws or {}
    return [None if given.get(name) is None else f32c(given[name]) for name in ("t_rand", "noise_c", "u", "noise_f")]


def _empty(dev, *shape):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _net_args(packed_c, packed_f, fine, attr="buffer", key=None):
    """The four (descriptor, packed stream) arguments of a render entry point: coarse pair, fine pair (NULLs without a fine pass).
    The stream is the pack's `attr` (the inference stream by default), or its entry `key` when that is a dict (buffers_bwd[prec])."""
    def pair(packed):
        buf = getattr(packed, attr)
        return [ctypes.byref(packed.desc), ptr(buf if key is None else buf[key])]
    return pair(packed_c) + (pair(packed_f) if fine else [None, None])


_RenderCall = collections.namedtuple("_RenderCall", "rays n dev fine nf k draws net_args")


def _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws):
    """The prelude of the render wrappers: fp32-contiguous ray rows, their count and device, whether a fine pass runs and its sample
    count, the number of thresholds (a list, a device tensor or None), the four draw tensors in argument order (_draw_tensors) and
    the four network arguments on the inference streams (_net_args)."""
    rays = f32c(rays)
    fine = num_fine > 0 and packed_f is not None
    k = 0 if m_thres is None else (int(m_thres.numel()) if torch.is_tensor(m_thres) else len(m_thres))
    return _RenderCall(rays, rays.shape[0], rays.device, fine, num_fine if fine else 0, k, _draw_tensors(draws),
                       _net_args(packed_c, packed_f, fine))


def _pass_maps(dev, n, present=True, rgb=False):
    """The output buffers of one pass: (depth, acc), led by rgb (n,3) when asked; a None each for a pass that does not run."""
    shapes = ([(n, 3)] if rgb else []) + [(n,), (n,)]
    return tuple(_empty(dev, *shape) if present else None for shape in shapes)


_SigmaCall = collections.namedtuple("_SigmaCall", "n s dev head thres k keep")


def _sigma_call(rf, z, rd, noise, noise_std, m_thres=None):
    """What the sigma-compositing wrappers prepare: rf (N,S,4) and z (N,S) fp32-contiguous, the direction rows (_dir_rows), the noise
    tensor only when noise_std > 0, the thresholds - a list or a device tensor - as a device tensor (None for none).  head: the six
    leading arguments of their entry points (rf, z, rd, rd_stride, noise, noise_std); keep: the tensors behind its pointers."""
    rf, z = f32c(rf), f32c(z)
    n, s = z.shape
    dev = rf.device
    rd_ptr, rd_stride, rd = _dir_rows(rd)
    nz = None if (noise is None or noise_std <= 0.0) else f32c(noise)
    th = m_thres
    if th is not None and not torch.is_tensor(th):
        th = torch.tensor([float(m) for m in th], dtype=torch.float32, device=dev) if len(th) else None
    k = 0 if th is None else int(th.numel())
    return _SigmaCall(n, s, dev, [ptr(rf), ptr(z), rd_ptr, rd_stride, ptr(nz), float(noise_std)], th if k else None, k, (rf, z, rd, nz))


def _grads_buf(packed, n_points, prec, dev):
    return torch.empty(train_sizes(packed, n_points, prec=prec)[2], dtype=torch.uint8, device=dev)


def _ray_outputs(n, image, dev):
    """(rays (n,11), target (n,3) | None, fp32-contiguous image | None, its channel count) of the select_rays* wrappers."""
    rays = torch.empty((n, 11), dtype=torch.float32, device=dev)
    if image is None:
        return rays, None, None, 0
    img = f32c(image)
    return rays, torch.empty((n, 3), dtype=torch.float32, device=dev), img, img.shape[-1]


def zeroed_grad_views(shapes, dev):
    """[(dW, db)] for `shapes` = [(out, in)] in linear_modules() order, as views of ONE zero-filled fp32 buffer."""
    flat = torch.zeros(sum(o * i + o for o, i in shapes), dtype=torch.float32, device=dev)
    out, off = [], 0
    for o, i in shapes:
        out.append((flat[off:off + o * i].view(o, i), flat[off + o * i:off + o * i + o]))
        off += o * i + o
    return out


# ------------------------------------------------------------------------------------------------
def ray_bundle(height, width, rinv, origin, fx, cx, cy, device):
    ro = torch.empty((height, width, 3), dtype=torch.float32, device=device)
    rd = torch.empty_like(ro)
    check(lib().dn_ray_bundle(height, width, host_floats(rinv), host_floats(origin), float(fx), float(cx), float(cy),
                              ptr(ro), ptr(rd), stream()), "dn_ray_bundle")
    return ro, rd


def select_rays(height, width, rinv, origin, fx, cx, cy, near, far, pixel_index, image=None):
    """Packed ray rows (N,11) [ro, rd, near, far, viewdir] for the chosen pixels (+ their RGB from `image` (H,W,C))."""
    pix = pixel_index.contiguous()
    assert pix.dtype == torch.int64 and pix.is_cuda
    n = pix.numel()
    rays, target, img, channels = _ray_outputs(n, image, pix.device)
    check(lib().dn_select_rays(height, width, host_floats(rinv), host_floats(origin), float(fx), float(cx), float(cy), float(near),
                               float(far), ptr(pix), n, ptr(img), channels, ptr(rays), ptr(target), stream()), "dn_select_rays")
    return rays, target


def select_rays_indirect(height, width, cams, view, near, far, pixel_index, images=None):
    """select_rays with the camera record chosen by the device scalar `view` (int32) out of `cams` (V,16)."""
    pix = pixel_index.contiguous()
    assert pix.dtype == torch.int64 and view.dtype == torch.int32 and cams.dtype == torch.float32 and cams.is_contiguous()
    n = pix.numel()
    rays, target, img, channels = _ray_outputs(n, images, pix.device)
    check(lib().dn_select_rays_indirect(height, width, ptr(cams), ptr(view), float(near), float(far), ptr(pix), n, ptr(img), channels,
                                        ptr(rays), ptr(target), stream()), "dn_select_rays_indirect")
    return rays, target


def select_rays_indirect_ndc(height, width, cams, view, near, far, pixel_index, focal, ndc_near, images=None):
    """select_rays_indirect with origin / direction of every row warped to NDC (dn_select_rays_indirect_ndc)."""
    pix = pixel_index.contiguous()
    assert pix.dtype == torch.int64 and view.dtype == torch.int32 and cams.dtype == torch.float32 and cams.is_contiguous()
    n = pix.numel()
    rays, target, img, channels = _ray_outputs(n, images, pix.device)
    check(lib().dn_select_rays_indirect_ndc(height, width, ptr(cams), ptr(view), float(near), float(far), ptr(pix), n, ptr(img), channels,
                                            ptr(rays), ptr(target), float(focal), float(ndc_near), stream()), "dn_select_rays_indirect_ndc")
    return rays, target


# ---- camera -> rays, differentiable in the camera -----------------------------------------------------------------------
def camera_record(extrinsic, intrinsic, focal_length, height, width, ndc_focal=None):
    """The 16-float camera record [rinv9, origin3, fx, cx, cy, ndc_focal | 0] of the ray kernels as differentiable torch ops on
    the HOST: the two fp32 torch.inverse calls of get_ray_bundle (5-argument fork convention: world->camera `extrinsic`, 3x3
    `intrinsic`), or - `intrinsic=None`, the 4-argument convention - the camera-to-world rotation with its y / z columns negated,
    cx = W / 2, cy = H / 2, fx = focal_length.  `tensor.to("cpu")` is differentiable, so a gradient of the record reaches
    `extrinsic` / `intrinsic` / `focal_length` / `ndc_focal` on whatever device they live on."""
    host = extrinsic.to("cpu", torch.float32)
    if intrinsic is not None:
        k = intrinsic.to("cpu", torch.float32)
        rinv = torch.inverse(host[:3, :3])
        origin = torch.inverse(host)[:3, -1]
        intr = torch.stack([k[0, 0], k[0, 2], k[1, 2]])
    else:
        rinv = host[:3, :3] * torch.tensor([1.0, -1.0, -1.0])
        origin = host[:3, -1]
        fx = (focal_length.to("cpu", torch.float32).reshape(()) if torch.is_tensor(focal_length)
              else torch.tensor(float(focal_length), dtype=torch.float32))
        intr = torch.stack([fx, torch.tensor(width * 0.5), torch.tensor(height * 0.5)])
    if torch.is_tensor(ndc_focal):
        last = ndc_focal.to("cpu", torch.float32).reshape(1)
    else:
        last = torch.tensor([0.0 if ndc_focal is None else float(ndc_focal)])
    return torch.cat([rinv.reshape(-1), origin, intr, last])


def camera_grad_scratch_bytes(n):
    return int(lib().dn_camera_grad_scratch_bytes(int(n)))


def camera_grad(height, width, cam16, pixel_index, n, g_ro, g_rd, g_viewdir, ndc_focal=0.0, ndc_near=1.0):
    """dn_camera_grad: the (16,) device gradient of the camera record from upstream gradients of the rays' origins / directions /
    view directions - (N, >= 3) fp32 views whose last dim is contiguous (column slices of packed rows go as they are), None = absent."""
    assert cam16.is_cuda and cam16.dtype == torch.float32 and cam16.is_contiguous() and cam16.numel() == 16
    keep, args = [], []
    for g in (g_ro, g_rd, g_viewdir):
        if g is None:
            args += [None, 0]
        else:
            p, stride, t = _dir_rows(g)
            keep.append(t)
            args += [p, stride]
    pix = None
    if pixel_index is not None:
        pix = pixel_index.contiguous()
        assert pix.dtype == torch.int64 and pix.is_cuda and pix.numel() == n
    nbytes = camera_grad_scratch_bytes(n)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=cam16.device)
    g_cam = torch.empty(16, dtype=torch.float32, device=cam16.device)
    check(lib().dn_camera_grad(int(height), int(width), ptr(cam16), ptr(pix), int(n), *args, float(ndc_focal), float(ndc_near),
                               ptr(scratch), nbytes, ptr(g_cam), stream()), "dn_camera_grad")
    return g_cam


def _camera_rays_forward(values, cams, height, width, pixel_index, near, far, image, ndc_focal, ndc_near):
    """The existing forward op for a camera record: `values` = its 16 floats on the host (full-image bundle and world-space rows:
    dn_ray_bundle / dn_select_rays, as get_ray_bundle / RaySelector.select call them), `cams` = the record on the device (NDC rows)."""
    rinv, origin, (fx, cx, cy) = values[:9], values[9:12], values[12:15]
    if pixel_index is None:
        return ray_bundle(height, width, rinv, origin, fx, cx, cy, cams.device if cams is not None else None)
    if ndc_focal:
        view = torch.zeros((), dtype=torch.int32, device=cams.device)
        images = None if image is None else image[None]
        return select_rays_indirect_ndc(height, width, cams.reshape(1, 16), view, near, far, pixel_index, ndc_focal, ndc_near, images)
    return select_rays(height, width, rinv, origin, fx, cx, cy, near, far, pixel_index, image)


class CameraRaysFn(torch.autograd.Function):
    """Rays of one camera, differentiable w.r.t. its record (camera_record): the full-image bundle (pixel_index None -> ro, rd
    (H,W,3)) or the packed rows of chosen pixels (-> rows (N,11), target (N,3) | None; with `ndc_focal` origin / direction warped
    to NDC).  The forward is the existing forward op on the record's values - outputs bit-identical to get_ray_bundle /
    RaySelector.select / the NDC draw.  The backward is dn_camera_grad (fp64 Jacobian, fixed-order sums) into a (16,) device
    tensor, returned as the gradient of the HOST record: one 64-byte device-to-host read per backward, which synchronises - so it
    cannot run under stream capture, and raises there."""

    @staticmethod
    def forward(ctx, record, device, height, width, pixel_index, near, far, image, ndc_focal, ndc_near):
        rec = record.detach().to(torch.float32).contiguous()
        cams = rec.to(device)
        ctx.save_for_backward(cams, pixel_index if pixel_index is not None else torch.empty(0, dtype=torch.int64, device=device))
        ctx.cfg = (int(height), int(width), pixel_index is not None, float(ndc_focal or 0.0), float(ndc_near), record.dtype)
        out = _camera_rays_forward(rec.tolist(), cams, int(height), int(width), pixel_index, near, far, image, ndc_focal, ndc_near)
        if pixel_index is not None and out[1] is not None:
            ctx.mark_non_differentiable(out[1])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_a, g_b):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("CameraRaysFn.backward: the camera gradient is read back to the host (64 bytes), which cannot be "
                               "captured into a HIP graph; run the camera's backward outside the capture")
        cams, pix = ctx.saved_tensors
        height, width, selected, ndc_focal, ndc_near, dtype = ctx.cfg
        if selected:
            n = pix.numel()
            g = f32c(g_a) if g_a is not None else torch.zeros((n, 11), dtype=torch.float32, device=cams.device)
            g_cam = camera_grad(height, width, cams, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], ndc_focal, ndc_near)
        else:
            n = height * width
            if g_a is None and g_b is None:
                g_a = torch.zeros((n, 3), dtype=torch.float32, device=cams.device)
            g_ro = None if g_a is None else f32c(g_a).reshape(n, 3)
            g_rd = None if g_b is None else f32c(g_b).reshape(n, 3)
            g_cam = camera_grad(height, width, cams, None, n, g_ro, g_rd, None, 0.0, 1.0)
        return (g_cam.cpu().to(dtype),) + (None,) * 9


# ---- mixed-camera batches: a view index per ray --------------------------------------------------------------------------
def _view_index(view_index, n):
    views = view_index.contiguous()
    assert views.dtype == torch.int32 and views.is_cuda and views.dim() == 1 and views.numel() == n, "view_index: (N,) int32 on the device"
    return views


def select_rays_views(height, width, cams, view_index, near, far, pixel_index, images=None, ndc_focal=None, ndc_near=1.0):
    """select_rays_indirect with a view per ray (dn_select_rays_views): row i is pixel `pixel_index[i]` of camera `view_index[i]`
    ((N,) int32, device) out of `cams` (V,16), its target from `images` (V,H,W,C).  ndc_focal: NDC rows (select_rays_indirect_ndc's)."""
    pix = pixel_index.contiguous()
    assert pix.dtype == torch.int64 and cams.dtype == torch.float32 and cams.is_contiguous() and cams.dim() == 2
    n = pix.numel()
    views = _view_index(view_index, n)
    rays, target, img, channels = _ray_outputs(n, images, pix.device)
    check(lib().dn_select_rays_views(int(height), int(width), ptr(cams), int(cams.shape[0]), ptr(views), float(near), float(far), ptr(pix), n,
                                     ptr(img), channels, ptr(rays), ptr(target), float(ndc_focal or 0.0), float(ndc_near), stream()),
          "dn_select_rays_views")
    return rays, target


def select_rays_draw_views(height, width, cams, near, far, rng_state, n_rays, images=None, want_pixels=False, ndc_focal=None, ndc_near=1.0):
    """select_rays_draw with the view of every ray drawn too (dn_select_rays_draw_views): `n_rays` distinct (view, pixel) pairs out of
    the V H W pixels of all cameras in `cams`, from `rng_state`'s next iteration.  Returns (rows, target), with want_pixels also the
    drawn pixels (int64) and views (int32)."""
    assert cams.dtype == torch.float32 and cams.is_contiguous() and cams.dim() == 2 and rng_state.dtype == torch.int32
    dev = cams.device
    rays, target, img, channels = _ray_outputs(n_rays, images, dev)
    pix = torch.empty((n_rays,), dtype=torch.int64, device=dev) if want_pixels else None
    views = torch.empty((n_rays,), dtype=torch.int32, device=dev) if want_pixels else None
    check(lib().dn_select_rays_draw_views(int(height), int(width), ptr(cams), int(cams.shape[0]), float(near), float(far), ptr(rng_state),
                                          int(n_rays), ptr(img), channels, ptr(rays), ptr(target), ptr(pix), ptr(views),
                                          float(ndc_focal or 0.0), float(ndc_near), stream()), "dn_select_rays_draw_views")
    return (rays, target, pix, views) if want_pixels else (rays, target)


def camera_grad_views_scratch_bytes(n, n_views):
    return int(lib().dn_camera_grad_views_scratch_bytes(int(n), int(n_views)))


def camera_grad_views(height, width, cams, view_index, pixel_index, n, g_ro, g_rd, g_viewdir, ndc_focal=0.0, ndc_near=1.0):
    """dn_camera_grad_views: the (V,16) device gradient of the camera records `cams` from upstream gradients of a mixed batch's
    origins / directions / view directions (as camera_grad takes them); row v sums the rays with view_index == v."""
    assert cams.is_cuda and cams.dtype == torch.float32 and cams.is_contiguous() and cams.dim() == 2 and cams.shape[1] == 16
    pix = pixel_index.contiguous()
    assert pix.dtype == torch.int64 and pix.is_cuda and pix.numel() == n
    views = _view_index(view_index, n)
    if n == 0:   # empty tensors carry NULL data pointers, which the entry point refuses: one unread element each (V x 16 zeros are written)
        pix, views = pix.new_zeros(1), views.new_zeros(1)
        g_ro, g_rd, g_viewdir = torch.zeros((1, 3), dtype=torch.float32, device=cams.device), None, None
    keep, args = [], []
    for g in (g_ro, g_rd, g_viewdir):
        if g is None:
            args += [None, 0]
        else:
            p, stride, t = _dir_rows(g)
            keep.append(t)
            args += [p, stride]
    n_views = int(cams.shape[0])
    nbytes = camera_grad_views_scratch_bytes(n, n_views)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=cams.device)
    g_cams = torch.empty((n_views, 16), dtype=torch.float32, device=cams.device)
    check(lib().dn_camera_grad_views(int(height), int(width), ptr(cams), n_views, ptr(views), ptr(pix), int(n), *args, float(ndc_focal),
                                     float(ndc_near), ptr(scratch), nbytes, ptr(g_cams), stream()), "dn_camera_grad_views")
    return g_cams


class CameraRaysViewsFn(torch.autograd.Function):
    """CameraRaysFn for a mixed batch: `records` (V,16) on the host (camera_record per view, stacked), `view_index` / `pixel_index`
    (N) on the device -> rows (N,11), target (N,3) | None.  Forward dn_select_rays_views, backward dn_camera_grad_views into a (V,16)
    device tensor returned as the gradient of the host records: ONE device-to-host read per backward (V x 64 bytes), which
    synchronises - so it cannot run under stream capture, and raises there."""

    @staticmethod
    def forward(ctx, records, device, height, width, view_index, pixel_index, near, far, images, ndc_focal, ndc_near):
        cams = records.detach().to(torch.float32).contiguous().to(device)
        ctx.save_for_backward(cams, view_index, pixel_index)
        ctx.cfg = (int(height), int(width), float(ndc_focal or 0.0), float(ndc_near), records.dtype)
        out = select_rays_views(int(height), int(width), cams, view_index, near, far, pixel_index, images, ndc_focal, ndc_near)
        if out[1] is not None:
            ctx.mark_non_differentiable(out[1])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_a, g_b):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("CameraRaysViewsFn.backward: the camera gradient is read back to the host (64 bytes per view), which cannot be "
                               "captured into a HIP graph; run the camera's backward outside the capture")
        cams, views, pix = ctx.saved_tensors
        height, width, ndc_focal, ndc_near, dtype = ctx.cfg
        n = pix.numel()
        g = f32c(g_a) if g_a is not None else torch.zeros((n, 11), dtype=torch.float32, device=cams.device)
        g_cams = camera_grad_views(height, width, cams, views, pix, n, g[:, 0:3], g[:, 3:6], g[:, 8:11], ndc_focal, ndc_near)
        return (g_cams.cpu().to(dtype),) + (None,) * 10


def camera_needs_grad(*values):
    """True when grad is enabled and one of the camera quantities (tensors; floats and None are skipped) requires grad."""
    return torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in values)


def new_rng_state(seed, device, first_iteration=0):
    """Device record {seed_lo, seed_hi, cur, nxt} for the in-kernel draws of a training loop (csrc/dn_rng.h)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = [seed & 0xFFFFFFFF, seed >> 32, int(first_iteration) & 0xFFFFFFFF, int(first_iteration) & 0xFFFFFFFF]
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=device)


def rng_fill(rng_state, stream_id, shape, normal=False):
    """The numbers the kernels draw for the current iteration from `rng_state`, stream `stream_id` (dn_rng_fill)."""
    out = torch.empty(shape, dtype=torch.float32, device=rng_state.device)
    check(lib().dn_rng_fill(ptr(rng_state), int(stream_id), out.numel(), int(bool(normal)), ptr(out), stream()), "dn_rng_fill")
    return out


def pack_ray_rows(ro, rd, view_d, near, far):
    """(N,3) origins / directions -> the (N, 8 | 11) ray rows of run_one_iter_of_nerf in one launch (dn_pack_ray_rows);
    view_d = the directions the unit view vectors come from (None: rows without them)."""
    ro, rd = f32c(ro), f32c(rd)
    vd = None if view_d is None else f32c(view_d)
    n = ro.shape[0]
    rows = torch.empty((n, 8 if vd is None else 11), dtype=torch.float32, device=ro.device)
    check(lib().dn_pack_ray_rows(ptr(ro), ptr(rd), ptr(vd), float(near), float(far), n, ptr(rows), stream()), "dn_pack_ray_rows")
    return rows


def select_rays_draw(height, width, cams, view, near, far, rng_state, n_rays, images=None, want_pixels=False, ndc_focal=None, ndc_near=1.0):
    """select_rays_indirect with the pixels drawn on the device, without replacement, from `rng_state`'s next iteration.
    view=None: the training view is drawn in the kernel too (uniformly from the cameras in `cams`).
    ndc_focal: forward-facing rows (dn_select_rays_draw_ndc) - origin and direction warped to NDC as ndc_rays(height, width,
    ndc_focal, ndc_near, ...) warps them, the view direction that of the unwarped ray, near / far as given."""
    assert (view is None or view.dtype == torch.int32) and cams.dtype == torch.float32 and cams.is_contiguous() and rng_state.dtype == torch.int32
    dev = cams.device
    rays, target, img, channels = _ray_outputs(n_rays, images, dev)
    pix = torch.empty((n_rays,), dtype=torch.int64, device=dev) if want_pixels else None
    if ndc_focal is not None:
        check(lib().dn_select_rays_draw_ndc(height, width, ptr(cams), ptr(view), int(cams.shape[0]), float(near), float(far), ptr(rng_state), n_rays,
                                            ptr(img), channels, ptr(rays), ptr(target), ptr(pix), float(ndc_focal), float(ndc_near), stream()),
              "dn_select_rays_draw_ndc")
    else:
        check(lib().dn_select_rays_draw(height, width, ptr(cams), ptr(view), int(cams.shape[0]), float(near), float(far), ptr(rng_state), n_rays, ptr(img), channels,
                                        ptr(rays), ptr(target), ptr(pix), stream()), "dn_select_rays_draw")
    return (rays, target, pix) if want_pixels else (rays, target)


def _loss_head_args(name, n_out, rgb_c, rgb_f, target, depth_c=None, depth_f=None, depth_src=None, pixel_index=None, view_index=None, view=None,
                    views_gather_only=False):
    """What the loss heads share (`name`: the caller, for messages): the colour inputs as contiguous fp32, `out` (n_out) and the
    gradient buffers, the depth-target arguments (depth_c / depth_f / depth_src, pix, hw; all None / 0 without a depth target) and the
    view arguments (views (N) int32, else the `view` scalar, else None).  views_gather_only: the views only say where depth targets
    are gathered - there must be none beside direct targets, and they are dropped without gathered ones."""
    a = types.SimpleNamespace(rgb_c=f32c(rgb_c), rgb_f=None, target=f32c(target), g_f=None, depth_c=None, depth_f=None, depth_src=None,
                              gd_c=None, gd_f=None, pix=None, hw=0, views=None, view=None)
    a.n = n = a.rgb_c.shape[0]
    a.out = torch.empty(n_out, dtype=torch.float32, device=a.rgb_c.device)
    a.g_c = torch.empty_like(a.rgb_c)
    if rgb_f is not None:
        a.rgb_f = f32c(rgb_f)
        a.g_f = torch.empty_like(a.rgb_f)
    if depth_src is not None:
        if depth_c is None:
            raise ValueError(f"{name}: a depth target needs depth_c")
        a.depth_src, a.depth_c = f32c(depth_src), f32c(depth_c)
        assert a.depth_c.numel() == n and a.depth_src.is_cuda
        a.gd_c = torch.empty_like(a.depth_c)
        if depth_f is not None:
            a.depth_f = f32c(depth_f)
            assert a.depth_f.numel() == n
            a.gd_f = torch.empty_like(a.depth_f)
        if pixel_index is None:
            assert a.depth_src.numel() == n and not (views_gather_only and (view_index is not None or view is not None)), \
                f"{name}: direct depth targets are (N)"
        else:
            a.pix = pixel_index.contiguous()
            assert a.pix.dtype == torch.int64 and a.pix.is_cuda and a.pix.numel() == n and a.depth_src.dim() >= 2
            a.hw = a.depth_src[0].numel()     # (an empty stack of maps raises here)
    if views_gather_only and a.pix is None:
        return a
    if view_index is not None:
        a.views = _view_index(view_index, n)
    elif view is not None:
        assert view.dtype == torch.int32 and view.is_cuda and view.numel() == 1
        a.view = view
    return a


def mse2_loss(rgb_c, rgb_f, target, luminance=False, rng_state=None):
    """(loss3 = [loss, mse_coarse, mse_fine] on the device, g_rgb_coarse, g_rgb_fine): the loss head + its upstream gradients in
    one launch (dn_mse2_loss); advances `rng_state`'s iteration counter."""
    a = _loss_head_args("mse2_loss", 3, rgb_c, rgb_f, target)
    check(lib().dn_mse2_loss(ptr(a.rgb_c), ptr(a.rgb_f), ptr(a.target), a.n, int(bool(luminance)), ptr(a.out), ptr(a.g_c), ptr(a.g_f),
                             ptr(rng_state), stream()), "dn_mse2_loss")
    return a.out, a.g_c, a.g_f


def render_loss(rgb_c, rgb_f, target, depth_c=None, depth_f=None, depth_src=None, pixel_index=None, view_index=None, view=None,
                weights=(1.0, 1.0), depth_weights=(0.0, 0.0), depth_range=(0.0, float("inf")), luminance=False, rng_state=None):
    """(loss6 = [loss, mse_coarse, mse_fine, D_coarse, D_fine, M] on the device, g_rgb_coarse, g_rgb_fine, g_depth_coarse, g_depth_fine):
    the general loss head + its upstream gradients in one launch (dn_render_loss); advances `rng_state`'s iteration counter.
    depth_src: (N) target depths, or with pixel_index (N) int64 the (V, H W) / (V,H,W) depth maps they are gathered from - the view of
    ray i is view_index[i] ((N) int32), else `view` (device int32 scalar), else 0.  None: no depth term (both depth gradients None)."""
    a = _loss_head_args("render_loss", 6, rgb_c, rgb_f, target, depth_c, depth_f, depth_src, pixel_index, view_index, view, views_gather_only=True)
    check(lib().dn_render_loss(ptr(a.rgb_c), ptr(a.rgb_f), ptr(a.target), ptr(a.depth_c), ptr(a.depth_f), ptr(a.depth_src), ptr(a.pix),
                               ptr(a.views), ptr(a.view), a.hw, a.n, int(bool(luminance)), float(weights[0]), float(weights[1]),
                               float(depth_weights[0]), float(depth_weights[1]), float(depth_range[0]), float(depth_range[1]), ptr(a.out),
                               ptr(a.g_c), ptr(a.g_f), ptr(a.gd_c), ptr(a.gd_f), ptr(rng_state), stream()), "dn_render_loss")
    return a.out, a.g_c, a.g_f, a.gd_c, a.gd_f


def render_loss_exposure(rgb_c, rgb_f, target, eps, exposure_scale=1.0, view_index=None, view=None, view_mask=None, depth_c=None, depth_f=None,
                         depth_src=None, pixel_index=None, weights=(1.0, 1.0), depth_weights=(0.0, 0.0), depth_range=(0.0, float("inf")),
                         luminance=False, rng_state=None, g_eps=None, want_eps=True):
    """render_loss with the colours of every ray corrected by its view's exposure row (dn_render_loss_exposure): eps (V,1) "gain" |
    (V,6) "affine", the view of ray i view_index[i] ((N) int32), else `view` (device int32 scalar), else 0 - the view the depth targets
    are gathered at too.  view_mask (V) int32: rows whose gradient is formed (None: all).  Returns (loss6, g_rgb_coarse, g_rgb_fine,
    g_depth_coarse, g_depth_fine, g_eps (V,P)); g_eps is written into the tensor given, or allocated (want_eps=False: None, one launch
    less)."""
    assert eps.is_cuda and eps.dtype == torch.float32 and eps.is_contiguous() and eps.dim() == 2 and eps.shape[1] in (1, 6)
    n_views, p = int(eps.shape[0]), int(eps.shape[1])
    a = _loss_head_args("render_loss_exposure", 6, rgb_c, rgb_f, target, depth_c, depth_f, depth_src, pixel_index, view_index, view)
    if view_mask is not None:
        assert view_mask.dtype == torch.int32 and view_mask.is_cuda and view_mask.is_contiguous() and view_mask.numel() == n_views
    if g_eps is None and want_eps:
        g_eps = torch.empty((n_views, p), dtype=torch.float32, device=a.out.device)
    if g_eps is not None:
        assert g_eps.is_cuda and g_eps.dtype == torch.float32 and g_eps.is_contiguous() and tuple(g_eps.shape) == (n_views, p)
    check(lib().dn_render_loss_exposure(ptr(a.rgb_c), ptr(a.rgb_f), ptr(a.target), ptr(a.depth_c), ptr(a.depth_f), ptr(a.depth_src), ptr(a.pix),
                                        ptr(a.views), ptr(a.view), a.hw, a.n, int(bool(luminance)), float(weights[0]), float(weights[1]),
                                        float(depth_weights[0]), float(depth_weights[1]), float(depth_range[0]), float(depth_range[1]),
                                        ptr(eps), p, n_views, float(exposure_scale), ptr(view_mask), ptr(a.out), ptr(a.g_c), ptr(a.g_f),
                                        ptr(a.gd_c), ptr(a.gd_f), ptr(g_eps), ptr(rng_state), stream()), "dn_render_loss_exposure")
    return a.out, a.g_c, a.g_f, a.gd_c, a.gd_f, g_eps


def ndc_rays(height, width, focal, near, rays_o, rays_d):
    ro, rd = f32c(rays_o), f32c(rays_d)
    n = ro.numel() // 3
    ro_out, rd_out = torch.empty_like(ro), torch.empty_like(rd)
    check(lib().dn_ndc_rays(int(height), int(width), float(focal), float(near), ptr(ro), ptr(rd), n, ptr(ro_out), ptr(rd_out),
                            stream()), "dn_ndc_rays")
    return ro_out, rd_out


def dex_error_sweep(depth_gt, depth_pred, mask=None, gt_lo=0.0, gt_hi=1.25):
    """(K,5) float64 device tensor of [sum |err| mm, #>2mm, #>4mm, #>8mm, #masked] per candidate map."""
    gt = f32c(depth_gt).reshape(-1)
    pred = f32c(depth_pred).reshape(-1, gt.numel())
    k = pred.shape[0]
    m = None if mask is None else mask.reshape(-1).to(torch.uint8).contiguous()
    out = torch.empty((k, 5), dtype=torch.float64, device=gt.device)
    check(lib().dn_dex_error_sweep(ptr(gt), ptr(pred), k, gt.numel(), ptr(m), float(gt_lo), float(gt_hi), ptr(out), stream()),
          "dn_dex_error_sweep")
    return out


def depth_error_image(depth_est, depth_gt, mask, abs_thres=1.0):
    est, gt = f32c(depth_est), f32c(depth_gt)
    h, w = gt.shape[-2:]
    m = mask.to(torch.uint8).contiguous()
    out = torch.empty((h, w, 3), dtype=torch.float32, device=gt.device)
    check(lib().dn_depth_error_image(ptr(est), ptr(gt), ptr(m), h, w, float(abs_thres), ptr(out), stream()), "dn_depth_error_image")
    return out


def coarse_depths(rays, num_coarse, lindisp, t_rand=None):
    rays = f32c(rays)
    n = rays.shape[0]
    z = torch.empty((n, num_coarse), dtype=torch.float32, device=rays.device)
    tr = None if t_rand is None else f32c(t_rand)
    check(lib().dn_coarse_depths(ptr(rays), rays.shape[1], n, num_coarse, int(bool(lindisp)), ptr(tr), ptr(z),
                                 stream()), "dn_coarse_depths")
    return z


def coarse_depths_bwd(rays, num_coarse, lindisp, t_rand, g_z):
    """dn_coarse_depths_backward: (N,2) = [dL/dnear, dL/dfar] of the ray rows."""
    rays, g_z = f32c(rays), f32c(g_z)
    n = rays.shape[0]
    out = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
    tr = None if t_rand is None else f32c(t_rand)
    check(lib().dn_coarse_depths_backward(ptr(rays), rays.shape[1], n, num_coarse, int(bool(lindisp)), ptr(tr), ptr(g_z), ptr(out),
                                          stream()), "dn_coarse_depths_backward")
    return out


class CoarseDepthsFn(torch.autograd.Function):
    """coarse_depths, differentiable w.r.t. the near / far columns of the ray rows (pose / ray optimisation: the stage-by-stage route
    of predict_and_render_radiance takes it when the rows require grad).  The jitter draws carry no gradient."""

    @staticmethod
    def forward(ctx, rays, num_coarse, lindisp, t_rand):
        rows = f32c(rays)
        ctx.save_for_backward(rows, t_rand if t_rand is not None else torch.empty(0, device=rows.device))
        ctx.cfg = (int(num_coarse), bool(lindisp), t_rand is not None, rays.dtype)
        return coarse_depths(rows, num_coarse, lindisp, t_rand)

    @staticmethod
    def backward(ctx, g_z):
        rows, t_rand = ctx.saved_tensors
        nc, lindisp, jitter, dtype = ctx.cfg
        g_rows = torch.zeros_like(rows)
        g_rows[:, 6:8] = coarse_depths_bwd(rows, nc, lindisp, t_rand if jitter else None, g_z)
        return g_rows.to(dtype), None, None, None


def positional_encoding(x, num_fns, include_input=True, log_sampling=True):
    shape = x.shape
    dim = shape[-1]
    xf = f32c(x).reshape(-1, dim)
    width = dim * ((1 if include_input else 0) + 2 * num_fns)
    out = torch.empty((xf.shape[0], width), dtype=torch.float32, device=x.device)
    check(lib().dn_positional_encoding(ptr(xf), xf.shape[0], dim, num_fns, int(bool(include_input)),
                                       int(bool(log_sampling)), ptr(out), stream()), "dn_positional_encoding")
    return out.reshape(*shape[:-1], width)


# ------------------------------------------------------------------------------------------------
class _Packed:
    """What the packed forms of a network share: the descriptor the kernels get, the precision, the device buffer (sized by the
    library) and the marshalling of the parameters for a pack call.  The subclasses differ in `pack` and in
    `require_fresh_inference_stream`."""

    def __init__(self, desc, device, precision, packed_bytes, what):
        self.desc = desc
        self.precision = _precision if precision is None else precision
        self.buffer = torch.empty(_sized(packed_bytes(self.precision), what), dtype=torch.uint8, device=device)
        self.key = None          # parameter key the streams (PackedMLP: the core stream) were packed from

    def _sources(self, weights, biases):
        """(weight pointers, bias pointers) of device tensors in the reference parameter order."""
        wp, ws = _ptr_array(weights, sources=True)
        bp, bs = _ptr_array(biases, sources=True)
        self._keep = (ws, bs)  # keep sources alive until the pack kernels have run on this stream
        return wp, bp


class PackedMLP(_Packed):
    """MFMA fragment stream of one FlexibleNeRFModel, rebuilt when the parameters change."""

    def __init__(self, desc_kwargs, device, precision=None):
        desc = _desc(desc_kwargs)
        super().__init__(desc, device, precision, lambda prec: lib().dn_mlp_packed_bytes(ctypes.byref(desc), prec), "dn_mlp_packed_bytes")
        # self.key: the core stream (bias tiles + pieces: every kernel but one)
        self.key48 = None        # ... and the stream of the 48-point inference kernel: a training loop leaves it stale until a render
        self.buffers_bwd = {}    # transposed streams for the backward-data chain, per training precision code (the 8-bit-saved-tensor
        self.keys_bwd = {}       # mode runs the 48-point chain: another stream), packed on first training use
        self.buffer_ig = None    # transposed stream of the encoding blocks (dn_mlp_backward_input), packed on first use by a call
        self.key_ig = None       # whose points / rays require grad

    def pack(self, weights, biases, parts=_hip.PACK_ALL):
        """weights/biases: lists of device tensors in the reference parameter order; parts: _hip.PACK_CORE | _hip.PACK_G48."""
        wp, bp = self._sources(weights, biases)
        check(lib().dn_mlp_pack_parts(ctypes.byref(self.desc), self.precision, wp, bp, ptr(self.buffer), int(parts), stream()),
              "dn_mlp_pack_parts")

    def require_fresh_inference_stream(self, what):
        """The inference entry points may run the 48-point kernel, whose stream lives behind the core one in `buffer` and is
        left stale by the training entry points (FlexibleNeRFModel.packed(train=True)).  A caller that kept this object across
        optimizer steps instead of asking `model.packed()` again would render OLD weights without any error: refuse."""
        if self.key48 != self.key:
            raise RuntimeError(f"{what}: the packed network's 48-point inference stream is older than its core stream or the other "
                               "way round (it was last packed by a training entry point, which refreshes only the stream it reads) - "
                               "obtain the packed network with model.packed() (no train=True) before rendering")


class PackedDensityMLP(_Packed):
    """MFMA fragment streams of the DENSITY sub-network of a FlexibleNeRFModel (dn_mlp_pack_density): its trunk and fc_alpha as
    row 3 of a 4-row head - an ordinary packed no-view-direction network (`desc` is the density descriptor), so the inference
    entry points (run_network_pts / run_network_rays, render_rays_depth) take it like a PackedMLP.  One key: its two streams are
    always packed together."""

    def __init__(self, desc_kwargs, device, precision=None):
        full = self.full_desc = _desc(desc_kwargs)
        super().__init__(_density_desc(full), device, precision, lambda prec: lib().dn_mlp_density_packed_bytes(ctypes.byref(full), prec),
                         "dn_mlp_density_packed_bytes")
        self.grad_streams = None   # DensityGradStreams, created by FlexibleNeRFModel.packed_density_grad on first use

    def pack(self, weights, biases):
        """weights/biases: the FULL network's device tensors in the reference parameter order."""
        wp, bp = self._sources(weights, biases)
        check(lib().dn_mlp_pack_density(ctypes.byref(self.full_desc), self.precision, wp, bp, ptr(self.buffer), stream()),
              "dn_mlp_pack_density")

    def require_fresh_inference_stream(self, what):
        pass   # one key: the two streams are never packed apart


def pack_backward(packed, weights, prec=None):
    """(Re)build the transposed weight stream dn_mlp_backward_data uses under training precision code `prec`."""
    prec = train_precision(packed) if prec is None else prec
    buf = packed.buffers_bwd.get(prec)
    if buf is None:
        nbytes = _sized(lib().dn_mlp_backward_packed_bytes(ctypes.byref(packed.desc), prec), "dn_mlp_backward_packed_bytes")
        buf = packed.buffers_bwd[prec] = torch.empty(nbytes, dtype=torch.uint8, device=packed.buffer.device)
    wp, packed._keep_bwd = _ptr_array(weights, sources=True)
    check(lib().dn_mlp_pack_backward(ctypes.byref(packed.desc), prec, wp, ptr(buf), stream()), "dn_mlp_pack_backward")


def ensure_backward_stream(model, packed, prec=None):
    """The backward stream of `packed` for precision code `prec`, re-packed when the parameters changed (or under capture)."""
    prec = train_precision(packed) if prec is None else prec
    key = model.param_key()
    if packed.keys_bwd.get(prec) != key or torch.cuda.is_current_stream_capturing():
        pack_backward(packed, model.pack_weights(scaled=False), prec)
        packed.keys_bwd[prec] = key
    return packed.buffers_bwd[prec]


def ensure_input_grad_stream(model, packed):
    """The input-gradient stream of `packed` (dn_mlp_pack_input_grad), re-packed when the parameters changed (or under capture)."""
    key = model.param_key()
    if packed.key_ig != key or torch.cuda.is_current_stream_capturing():
        if packed.buffer_ig is None:
            nbytes = _sized(lib().dn_mlp_input_grad_packed_bytes(ctypes.byref(packed.desc), packed.precision),
                            "dn_mlp_input_grad_packed_bytes")
            packed.buffer_ig = torch.empty(nbytes, dtype=torch.uint8, device=packed.buffer.device)
        wp, packed._keep_ig = _ptr_array(model.pack_weights(), sources=True)
        check(lib().dn_mlp_pack_input_grad(ctypes.byref(packed.desc), packed.precision, wp, ptr(packed.buffer_ig), stream()),
              "dn_mlp_pack_input_grad")
        packed.key_ig = key
    return packed.buffer_ig


def mlp_backward_input(packed, grads, n_rays, samples_per_ray, pts=None, viewdirs=None, rays=None, z_vals=None):
    """dn_mlp_backward_input on the `grads` records of mlp_backward_data (precision = packed.precision: fp32, or bf16 with 16-bit
    saves).  Points form: (d_pts (P,3), d_viewdirs (N,3) | None); rays form: (d_rays (N,stride), d_z (N,S))."""
    ray_form = pts is None
    dev = grads.device
    n_pts = n_rays * samples_per_ray
    nbytes = int(lib().dn_mlp_backward_input_workspace_bytes(ctypes.byref(packed.desc), n_pts, int(ray_form)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    d_pts = d_vd = d_rays = d_z = None
    stride = 0
    if ray_form:
        rays, z_vals = f32c(rays), f32c(z_vals)
        stride = rays.shape[1]
        d_rays, d_z = torch.empty_like(rays), torch.empty_like(z_vals)
    else:
        pts = f32c(pts).reshape(-1, 3)
        d_pts = torch.empty_like(pts)
        if packed.desc.use_viewdirs:
            viewdirs = f32c(viewdirs).reshape(-1, 3)
            d_vd = torch.empty_like(viewdirs)
    check(lib().dn_mlp_backward_input(ctypes.byref(packed.desc), packed.precision, ptr(packed.buffer_ig), ptr(grads), ptr(pts), ptr(viewdirs),
                                      ptr(rays), stride, ptr(z_vals), n_rays, samples_per_ray, ptr(d_pts), ptr(d_vd), ptr(d_rays), ptr(d_z),
                                      ptr(ws), nbytes, stream()), "dn_mlp_backward_input")
    return (d_rays, d_z) if ray_form else (d_pts, d_vd)


def pack_train_pair(model_a, model_b, logs):
    """The streams a DN_PREC_BF16_S8 training step reads, for two networks of one architecture, in two launches (dn_mlp_pack_train_pair)
    - or, when that does not apply (different shapes, another precision, nothing stale), the per-network route.  Returns the two
    packed networks and the precision code."""
    pa, pb = model_a._packed_slot(*logs), model_b._packed_slot(*logs)
    prec = train_precision(pa)
    capturing = torch.cuda.is_current_stream_capturing()
    same = bytes(pa.desc) == bytes(pb.desc) and train_precision(pb) == prec == _hip.PREC_BF16_S8
    ka, kb = model_a.param_key(), model_b.param_key()
    stale = lambda pk, key: pk.key48 != key or pk.keys_bwd.get(prec) != key   # noqa: E731
    if same and (capturing or (stale(pa, ka) and stale(pb, kb))):
        for pk in (pa, pb):
            if pk.buffers_bwd.get(prec) is None:
                pk.buffers_bwd[prec] = torch.empty(lib().dn_mlp_backward_packed_bytes(ctypes.byref(pk.desc), prec), dtype=torch.uint8,
                                                   device=pk.buffer.device)
        arrays, keep = [], []
        anneal = model_a._encoding_anneal      # one schedule on both networks: their scaled copies in one launch
        paired = anneal.scaled_weights_pair(model_a, model_b) if (anneal is not None and anneal is model_b._encoding_anneal) else None
        for k, model in enumerate((model_a, model_b)):
            mods = model.linear_modules()
            wp, ws = _ptr_array(model.pack_weights() if paired is None else paired[k], sources=True)
            bp, bs = _ptr_array([m.bias for m in mods], sources=True)
            keep.append((ws, bs))
            arrays.append((wp, bp))
        check(lib().dn_mlp_pack_train_pair(ctypes.byref(pa.desc), arrays[0][0], arrays[0][1], ptr(pa.buffer), ptr(pa.buffers_bwd[prec]),
                                           arrays[1][0], arrays[1][1], ptr(pb.buffer), ptr(pb.buffers_bwd[prec]), stream()),
              "dn_mlp_pack_train_pair")
        pa._keep_pair = keep
        for pk, key in ((pa, ka), (pb, kb)):
            pk.key48 = key
            pk.keys_bwd[prec] = key
        return pa, pb, prec
    pa, pb = model_a.packed(*logs, train=True), model_b.packed(*logs, train=True)
    prec = train_precision(pa)
    if train_precision(pb) != prec:
        prec = pa.precision
    ensure_backward_stream(model_a, pa, prec)
    ensure_backward_stream(model_b, pb, prec)
    return pa, pb, prec


def s8_supported(packed):
    """True when the 8-bit-saved-tensor training kernels (48-point geometry) cover this network."""
    return lib().dn_mlp_backward_packed_bytes(ctypes.byref(packed.desc), _hip.PREC_BF16_S8) != 0


def train_sizes(packed, n_points, s8=False, prec=None):
    a, m, g = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    if prec is None:
        prec = _hip.PREC_BF16_S8 if s8 else packed.precision
    check(lib().dn_mlp_train_sizes(ctypes.byref(packed.desc), prec, n_points, ctypes.byref(a), ctypes.byref(m),
                                   ctypes.byref(g)), "dn_mlp_train_sizes")
    return a.value, m.value, g.value


def run_network_train(packed, pts, viewdirs, samples_per_ray, rays=None, z_vals=None, prec=None):
    """Training forward: raw radiance field + the opaque (act, masks) buffers the backward needs.  Either explicit
    points (+ per-ray view directions) or packed ray rows + depths (the points are formed in the kernel)."""
    if rays is not None:
        rays, z_vals = f32c(rays), f32c(z_vals)
        n_rays, samples_per_ray = z_vals.shape
        n_pts = n_rays * samples_per_ray
        dev = rays.device
    else:
        pts = f32c(pts).reshape(-1, 3)
        n_pts = pts.shape[0]
        assert n_pts % samples_per_ray == 0
        dev = pts.device
    prec = packed.precision if prec is None else prec
    a_bytes, m_bytes, _ = train_sizes(packed, n_pts, prec=prec)
    out = torch.empty((n_pts, 4), dtype=torch.float32, device=dev)
    act = torch.empty(a_bytes, dtype=torch.uint8, device=dev)
    masks = torch.empty(m_bytes, dtype=torch.uint8, device=dev)
    if rays is not None:
        check(lib().dn_run_network_train(ctypes.byref(packed.desc), prec, ptr(packed.buffer), None, None, ptr(rays),
                                         rays.shape[1], ptr(z_vals), n_pts // samples_per_ray, samples_per_ray, ptr(out),
                                         ptr(act), ptr(masks), stream()), "dn_run_network_train")
        return out, act, masks
    vd = None if viewdirs is None else f32c(viewdirs).reshape(-1, 3)
    check(lib().dn_run_network_train(ctypes.byref(packed.desc), prec, ptr(packed.buffer), ptr(pts), ptr(vd), None,
                                     0, None, n_pts // samples_per_ray, samples_per_ray, ptr(out), ptr(act), ptr(masks),
                                     stream()), "dn_run_network_train")
    return out, act, masks


def mlp_backward_data(packed, g_out, masks, n_points, prec=None):
    g_out = f32c(g_out).reshape(-1, 4)
    prec = packed.precision if prec is None else prec
    _, _, g_bytes = train_sizes(packed, n_points, prec=prec)
    grads = torch.empty(g_bytes, dtype=torch.uint8, device=g_out.device)
    check(lib().dn_mlp_backward_data(ctypes.byref(packed.desc), prec, ptr(packed.buffers_bwd[prec]), ptr(g_out),
                                     ptr(masks), n_points, ptr(grads), stream()), "dn_mlp_backward_data")
    _note_s8_record(grads, prec)
    return grads


def mlp_unpack(packed, which, native, n_points, slot, width, kind, out, col0=0, prec=None):
    """native pieces -> out[:, col0:col0+width_or_pe_dim] (plain fp32 rows).  prec = PREC_BF16_S8: the 8-bit units of the
    48-point training kernels (slot in units of 64 features per 16-point group; kind 3 = the custom output-gradient unit)."""
    check(lib().dn_mlp_unpack(ctypes.byref(packed.desc), packed.precision if prec is None else prec, which, ptr(native), n_points, slot, width, kind,
                              ptr(out), out.shape[1], col0, stream()), "dn_mlp_unpack")
    return out


def mlp_weight_grad(packed, act, grads, n_points, g_slot, n_out, x_slot, x_width, pe_kind, d_w, d_b):
    """bf16 buffers: d_w (n_out, >= x_width + pe_dim) += dY^T [X | PE], d_b += sum dY (both pre-zeroed fp32)."""
    check(lib().dn_mlp_weight_grad(ctypes.byref(packed.desc), packed.precision, ptr(act), ptr(grads), n_points, g_slot, n_out,
                                   x_slot, x_width, pe_kind, ptr(d_w), d_w.shape[1], ptr(d_b), stream()), "dn_mlp_weight_grad")


_DETERMINISTIC_WGRAD = [True]


def set_deterministic_weight_gradients(on):
    """True (default): the weight-gradient launches of the training paths reduce their workgroups' partials in a fixed order (a partial
    per workgroup in a scratch buffer + a second small launch: dn_*_ws) - a training run is then a pure function of its seed, bit for
    bit, like the reference on the CPU.  False: fp32 atomics straight into the gradients (no scratch; the sum's last bits change from
    launch to launch)."""
    _DETERMINISTIC_WGRAD[0] = bool(on)


def _wgrad_scratch(n_networks, *packs):
    """(tensor, bytes) of reduction scratch for a launch over `n_networks` networks of these architectures - ONE allocation of
    the largest need - or (None, 0).  A fresh stream-ordered allocation per call (the caching allocator hands the same block
    back every step; inside a graph capture it belongs to the graph's pool)."""
    if not _DETERMINISTIC_WGRAD[0]:
        return None, 0
    nbytes = max(int(lib().dn_mlp_weight_grad_scratch_bytes(ctypes.byref(pk.desc), int(n_networks))) for pk in packs)
    if nbytes <= 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=packs[0].buffer.device), nbytes


def mlp_weight_grad_all(packed, act, grads, n_points, shapes, s8=False, prec=None):
    """bf16 buffers: every layer's (dW, db) in one launch.  `shapes` = [(out, in)] in linear_modules() order; returns
    [(dW, db)] as views of ONE zero-filled fp32 buffer.  s8: the buffers are in the 8-bit unit layout (convert_saved_s8)."""
    out = zeroed_grad_views(shapes, act.device)
    wp, bp = _view_ptrs(out)
    if prec is None:
        prec = _hip.PREC_BF16_S8 if s8 else packed.precision
    scratch, nbytes = _wgrad_scratch(1, packed)
    check(lib().dn_mlp_weight_grad_all_ws(ctypes.byref(packed.desc), prec, ptr(act), ptr(grads), n_points, wp, bp, ptr(scratch), nbytes, stream()),
          "dn_mlp_weight_grad_all")
    return out


def mlp_weight_grad_all_into(packed, act, grads, n_points, views, prec=None):
    """The same launch accumulating into caller-owned (dW, db) tensors (dense fp32 with the nn.Linear shapes, e.g. the
    `.grad` views of a parallel.FlatGradBucket, already zeroed for this step)."""
    wp, bp = _view_ptrs(views)
    scratch, nbytes = _wgrad_scratch(1, packed)
    check(lib().dn_mlp_weight_grad_all_ws(ctypes.byref(packed.desc), packed.precision if prec is None else prec, ptr(act), ptr(grads),
                                          n_points, wp, bp, ptr(scratch), nbytes, stream()), "dn_mlp_weight_grad_all")


def run_network_pts(packed, pts, viewdirs, samples_per_ray):
    packed.require_fresh_inference_stream("run_network")
    pts = f32c(pts).reshape(-1, 3)
    n_pts = pts.shape[0]
    assert n_pts % samples_per_ray == 0
    out = torch.empty((n_pts, 4), dtype=torch.float32, device=pts.device)
    vd = None if viewdirs is None else f32c(viewdirs).reshape(-1, 3)
    check(lib().dn_run_network(ctypes.byref(packed.desc), packed.precision, ptr(packed.buffer), ptr(pts), ptr(vd), None, 0,
                               None, n_pts // samples_per_ray, samples_per_ray, ptr(out), stream()), "dn_run_network")
    return out


def run_network_rays(packed, rays, z_vals):
    packed.require_fresh_inference_stream("run_network")
    rays, z_vals = f32c(rays), f32c(z_vals)
    n, s = z_vals.shape
    out = torch.empty((n, s, 4), dtype=torch.float32, device=rays.device)
    check(lib().dn_run_network(ctypes.byref(packed.desc), packed.precision, ptr(packed.buffer), None, None, ptr(rays),
                               rays.shape[1], ptr(z_vals), n, s, ptr(out), stream()), "dn_run_network")
    return out


def mlp_forward_encoded(packed, x):
    x = f32c(x)
    shape = x.shape
    xf = x.reshape(-1, shape[-1])
    out = torch.empty((xf.shape[0], 4), dtype=torch.float32, device=x.device)
    check(lib().dn_mlp_forward_encoded(ctypes.byref(packed.desc), packed.precision, ptr(packed.buffer), ptr(xf),
                                       xf.shape[0], ptr(out), stream()), "dn_mlp_forward_encoded")
    return out.reshape(*shape[:-1], 4)


# ------------------------------------------------------------------------------------------------
def volume_render_fwd(rf, z, rd, noise, noise_std, white, m_thres, want_weights=True):
    rf, z = f32c(rf), f32c(z)
    n, s = z.shape
    dev = rf.device
    rd_ptr, rd_stride, rd = _dir_rows(rd)
    k = len(m_thres)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((n,), dtype=torch.float32, device=dev)
    acc = torch.empty_like(disp)
    depth = torch.empty_like(disp)
    weights = torch.empty((n, s), dtype=torch.float32, device=dev) if want_weights else None
    dex = torch.empty((k, n), dtype=torch.float32, device=dev) if k else None
    nz = None if (noise is None or noise_std <= 0.0) else f32c(noise)
    check(lib().dn_volume_render(ptr(rf), ptr(z), rd_ptr, rd_stride, ptr(nz), float(noise_std), int(bool(white)),
                                 host_floats(m_thres), k, n, s, ptr(rgb), ptr(disp), ptr(acc), ptr(weights), ptr(depth),
                                 ptr(dex), stream()), "dn_volume_render")
    return rgb, disp, acc, weights, depth, dex


def volume_render_bwd(rf, z, rd, noise, noise_std, white, g_rgb, g_depth, g_acc, g_disp, g_weights):
    rf, z = f32c(rf), f32c(z)
    n, s = z.shape
    rd_ptr, rd_stride, rd = _dir_rows(rd)
    g_rf = torch.empty((n, s, 4), dtype=torch.float32, device=rf.device)
    nz = None if (noise is None or noise_std <= 0.0) else f32c(noise)
    gs = [None if g is None else f32c(g) for g in (g_rgb, g_depth, g_acc, g_disp, g_weights)]
    check(lib().dn_volume_render_backward(ptr(rf), ptr(z), rd_ptr, rd_stride, ptr(nz), float(noise_std), int(bool(white)),
                                          n, s, ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(gs[4]), ptr(g_rf),
                                          stream()), "dn_volume_render_backward")
    return g_rf


def volume_render_bwd_geom(rf, z, rd, noise, noise_std, white, g_rgb, g_depth, g_acc, g_disp, g_weights, want_rf=True, want_z=True,
                           want_rd=True):
    """dn_volume_render_backward_geom: (g_rf (N,S,4), g_z (N,S), g_rd (N,3)), None for what is not wanted."""
    rf, z = f32c(rf), f32c(z)
    n, s = z.shape
    rd_ptr, rd_stride, rd = _dir_rows(rd)
    dev = rf.device
    g_rf = torch.empty((n, s, 4), dtype=torch.float32, device=dev) if want_rf else None
    g_z = torch.empty((n, s), dtype=torch.float32, device=dev) if want_z else None
    g_rd = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_rd else None
    nz = None if (noise is None or noise_std <= 0.0) else f32c(noise)
    gs = [None if g is None else f32c(g) for g in (g_rgb, g_depth, g_acc, g_disp, g_weights)]
    check(lib().dn_volume_render_backward_geom(ptr(rf), ptr(z), rd_ptr, rd_stride, ptr(nz), float(noise_std), int(bool(white)), n, s,
                                               ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(gs[4]), ptr(g_rf), ptr(g_z),
                                               ptr(g_rd), stream()), "dn_volume_render_backward_geom")
    return g_rf, g_z, g_rd


class VolumeRenderFn(torch.autograd.Function):
    """Differentiable w.r.t. the radiance field, the depths and the ray directions (dists = dz |rd|, depth = sum w z).  The
    geometry entry point runs only when z or rd ask for a gradient; otherwise the backward is dn_volume_render_backward as ever.
    The Dex depth maps are not differentiable, and the reference detaches z_samples (train_utils.py:170)."""

    @staticmethod
    def forward(ctx, rf, z, rd, noise, noise_std, white, m_thres):
        rgb, disp, acc, weights, depth, dex = volume_render_fwd(rf, z, rd, noise, noise_std, white, m_thres)
        ctx.set_materialize_grads(False)   # unused outputs arrive as None (the kernel takes NULL), not as zero-filled tensors
        ctx.save_for_backward(rf, z, rd, noise if noise is not None else torch.empty(0, device=rf.device))
        ctx.cfg = (float(noise_std), bool(white), noise is not None)
        outs = (rgb, disp, acc, weights, depth) + ((dex,) if dex is not None else ())
        if dex is not None:
            ctx.mark_non_differentiable(dex)
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_weights, g_depth, *_):
        rf, z, rd, noise = ctx.saved_tensors
        noise_std, white, has_noise = ctx.cfg

        def nz(g):
            return None if g is None else g.contiguous()
        need_rf, need_z, need_rd = ctx.needs_input_grad[:3]
        if need_z or need_rd:
            g_rf, g_z, g_rd = volume_render_bwd_geom(rf, z, rd, noise if has_noise else None, noise_std, white, nz(g_rgb), nz(g_depth),
                                                     nz(g_acc), nz(g_disp), nz(g_weights), need_rf, need_z, need_rd)
            if g_z is not None:
                g_z = g_z.to(z.dtype)
            if g_rd is not None:
                g_rd = g_rd.reshape(rd.shape).to(rd.dtype)
            return g_rf, g_z, g_rd, None, None, None, None
        g_rf = volume_render_bwd(rf, z, rd, noise if has_noise else None, noise_std, white, nz(g_rgb), nz(g_depth),
                                 nz(g_acc), nz(g_disp), nz(g_weights))
        return g_rf, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
def distortion_loss(weights, z, near_far=None, scale=1.0, want_z=False, rays=None, g_z=None):
    """dn_distortion_loss: the distortion regulariser of compositing's weights (N,S) and depths (N,S), S <= 1024.  The near / far of
    every ray come from near_far (N,2) or from columns 6:8 of packed ray rows (`rays`).  Returns (mean (1) - the unweighted mean of
    L_ray -, ray_loss (N) fp64, g_weights (N,S) = scale dL_ray/dw, g_z (N,S) = scale dL_ray/dz | None).  g_z given: the depth gradient
    is ADDED to it (and returned); else want_z decides whether it is formed."""
    if (near_far is None) == (rays is None):
        raise ValueError("distortion_loss: give near_far (N,2) or rays (N, >= 8), one of them")
    weights, z = f32c(weights), f32c(z)
    n, s = z.shape
    if tuple(weights.shape) != (n, s):
        raise ValueError(f"distortion_loss: weights {tuple(weights.shape)} for depths {tuple(z.shape)}")
    rows = f32c(near_far if rays is None else rays)
    if rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < (2 if rays is None else 8):
        raise ValueError(f"distortion_loss: near_far is (N,2), rays (N, >= 8) (got {tuple(rows.shape)} for {n} rays)")
    assert rows.is_cuda, "HIP entry points need contiguous device tensors"
    nf_ptr = None if n == 0 else ctypes.c_void_p(rows.data_ptr() + (0 if rays is None else 6 * 4))
    dev = z.device
    accumulate = g_z is not None
    if accumulate:
        assert g_z.dtype == torch.float32 and g_z.is_contiguous() and tuple(g_z.shape) == (n, s), "distortion_loss: g_z is (N,S) fp32, contiguous"
    elif want_z:
        g_z = torch.empty((n, s), dtype=torch.float32, device=dev)
    g_w = torch.empty((n, s), dtype=torch.float32, device=dev)
    ray_loss = torch.empty((n,), dtype=torch.float64, device=dev)
    mean = torch.zeros((1,), dtype=torch.float32, device=dev) if n == 0 else torch.empty((1,), dtype=torch.float32, device=dev)
    check(lib().dn_distortion_loss(ptr(weights), ptr(z), nf_ptr, rows.shape[1], n, s, float(scale), ptr(g_w), ptr(g_z), int(accumulate),
                                   ptr(ray_loss), ptr(mean), stream()), "dn_distortion_loss")
    return mean, ray_loss, g_w, g_z


# ------------------------------------------------------------------------------------------------
def sample_pdf(bins, weights, num_samples, u=None, want_inds=False):
    bins, weights = f32c(bins), f32c(weights)
    n, b = bins.shape
    assert weights.shape == (n, b - 1)
    samples = torch.empty((n, num_samples), dtype=torch.float32, device=bins.device)
    inds = torch.empty((n, num_samples), dtype=torch.int64, device=bins.device) if want_inds else None
    uu = None if u is None else f32c(u)
    check(lib().dn_sample_pdf(ptr(bins), ptr(weights), ptr(uu), n, b, num_samples, ptr(samples),
                              None if inds is None else c_void_p(inds.data_ptr()), stream()), "dn_sample_pdf")
    return (samples, inds) if want_inds else samples


def fine_depths(z_coarse, weights, num_fine, u=None, want_samples=False):
    z_coarse, weights = f32c(z_coarse), f32c(weights)
    n, nc = z_coarse.shape
    z_fine = torch.empty((n, nc + num_fine), dtype=torch.float32, device=z_coarse.device)
    zs = torch.empty((n, num_fine), dtype=torch.float32, device=z_coarse.device) if want_samples else None
    uu = None if u is None else f32c(u)
    check(lib().dn_fine_depths(ptr(z_coarse), ptr(weights), ptr(uu), n, nc, num_fine, ptr(z_fine), ptr(zs), stream()),
          "dn_fine_depths")
    return (z_fine, zs) if want_samples else z_fine


def fine_depths_bwd(z_coarse, z_samples, g_z_fine):
    """dn_fine_depths_backward: g_z_coarse (N,Nc), the gather of g_z_fine at the slots the coarse depths took in the merge."""
    z_coarse, z_samples, g_z_fine = f32c(z_coarse), f32c(z_samples), f32c(g_z_fine)
    n, nc = z_coarse.shape
    nf = z_samples.shape[1]
    assert g_z_fine.shape == (n, nc + nf)
    out = torch.empty((n, nc), dtype=torch.float32, device=z_coarse.device)
    check(lib().dn_fine_depths_backward(ptr(z_coarse), ptr(z_samples), ptr(g_z_fine), n, nc, nf, ptr(out), stream()),
          "dn_fine_depths_backward")
    return out


class FineDepthsFn(torch.autograd.Function):
    """fine_depths, differentiable w.r.t. the coarse depths through the merge; the resamples are detached, as in the reference
    (train_utils.py:170), so the weights and the draws get nothing.  Keeps z_samples for its backward."""

    @staticmethod
    def forward(ctx, z_coarse, weights, num_fine, u):
        z_fine, zs = fine_depths(z_coarse, weights, num_fine, u, want_samples=True)
        ctx.save_for_backward(z_coarse, zs)
        return z_fine

    @staticmethod
    def backward(ctx, g_z_fine):
        z_coarse, zs = ctx.saved_tensors
        return fine_depths_bwd(z_coarse, zs, g_z_fine).to(z_coarse.dtype), None, None, None


_render_ws = {}   # current stream -> (cached workspace buffer, the bytes the latest render call on that stream asked for)


def _stream_key():
    # (the current device's current stream: the one the kernels are enqueued on, _hip.stream())
    return torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream


def _render_workspace(dev, nbytes):
    """Workspace of a no-grad render call on the current stream: one cached buffer per stream, grown when needed, and the record
    of which bytes the LATEST call there used - its status block is their last 256 bytes (render_status_words)."""
    key = _stream_key()
    ws, _ = _render_ws.get(key, (None, 0))
    if ws is None or ws.device != dev or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _render_ws[key] = (ws, nbytes)
    return ws[:nbytes]


def _latest_render_workspace():
    if _stream_key() not in _render_ws:
        raise RuntimeError("render_status_words / render_nonfinite_count: no render_rays / render_rays_depth call on this stream yet")
    ws, nbytes = _render_ws[_stream_key()]
    return ws[:nbytes]


def render_rays(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, white, m_thres, draws=None):
    """dn_render_rays: the whole predict_and_render_radiance forward for one ray chunk (no autograd)."""
    packed_c.require_fresh_inference_stream("render_rays")
    if packed_f is not None:
        packed_f.require_fresh_inference_stream("render_rays")
    c = _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws)
    n, dev = c.n, c.dev
    ws = _render_workspace(dev, lib().dn_render_workspace_bytes(n, num_coarse, c.nf))
    maps = _pass_maps(dev, n, rgb=True) + _pass_maps(dev, n, c.fine, rgb=True) + (_empty(dev, c.k, n) if c.k else None,)
    check(lib().dn_render_rays(
        *c.net_args, packed_c.precision, ptr(c.rays), c.rays.shape[1], n, num_coarse, c.nf, int(bool(lindisp)), float(noise_std),
        int(bool(white)), host_floats(m_thres), c.k, *[ptr(d) for d in c.draws], *[ptr(m) for m in maps], ptr(ws), stream()),
        "dn_render_rays")
    return maps


def composite_density(rf, z, rd, noise, noise_std, m_thres):
    """dn_composite_density: (depth, acc, dex (K,N) or None) from the sigma column of rf (N,S,4); any number of thresholds."""
    c = _sigma_call(rf, z, rd, noise, noise_std, m_thres)
    depth, acc = _pass_maps(c.dev, c.n)
    dex = _empty(c.dev, c.k, c.n) if c.k else None
    check(lib().dn_composite_density(*c.head, ptr(c.thres), c.k, c.n, c.s, ptr(depth), ptr(acc), ptr(dex), stream()), "dn_composite_density")
    return depth, acc, dex


def check_quantiles(quantiles, who="quantiles"):
    """The host-side rule of the opacity quantiles (the C layer cannot read device memory): a list of at most 64 finite values
    strictly inside (0, 1) as fp32 - returned as Python floats of those fp32 values.  Raises ValueError before any GPU work."""
    qs = [float(q) for q in quantiles]
    if len(qs) > _hip.MAX_QUANTILES:
        raise ValueError(f"{who}: at most {_hip.MAX_QUANTILES} quantiles per call, got {len(qs)}")
    out = []
    for q in qs:
        q32 = ctypes.c_float(q).value if math.isfinite(q) else q
        if not (math.isfinite(q32) and 0.0 < q32 < 1.0):
            raise ValueError(f"{who}: every quantile must be finite and strictly inside (0, 1) as fp32, got {q!r}")
        out.append(q32)
    return out


def composite_density_quantiles(rf, z, rd, noise, noise_std, m_thres, quantiles, interp=False):
    """dn_composite_density_quantiles: composite_density's (depth, acc, dex (K,N) or None) and qdepth (Q,N) or None - the depth at
    which the accumulated opacity first reaches each quantile (interp: the piecewise-linear inversion instead of the sample's z)."""
    qs = check_quantiles(quantiles, "composite_density_quantiles")
    return composite_density_quantiles_on_device(rf, z, rd, noise, noise_std, m_thres,
                                                 torch.tensor(qs, dtype=torch.float32, device=rf.device) if qs else None, interp)


def composite_density_quantiles_on_device(rf, z, rd, noise, noise_std, m_thres, quantiles, interp=False):
    """composite_density_quantiles with the quantiles already judged (check_quantiles) and on the device - a float32 tensor, or None for
    none: no host read and no copy per call."""
    c = _sigma_call(rf, z, rd, noise, noise_std, m_thres)
    nq = 0 if quantiles is None else int(quantiles.numel())
    depth, acc = _pass_maps(c.dev, c.n)
    dex = _empty(c.dev, c.k, c.n) if c.k else None
    qdepth = _empty(c.dev, nq, c.n) if nq else None
    check(lib().dn_composite_density_quantiles(*c.head, ptr(c.thres), c.k, ptr(quantiles), nq, int(bool(interp)), c.n, c.s, ptr(depth),
                                               ptr(acc), ptr(dex), ptr(qdepth), stream()), "dn_composite_density_quantiles")
    return depth, acc, dex, qdepth


def density_resample(rf, z, rd, num_fine, noise=None, noise_std=0.0, u=None):
    """dn_density_resample: coarse sigma compositing fused with fine_depths -> (depth_c, acc_c, z_fine)."""
    c = _sigma_call(rf, z, rd, noise, noise_std)
    depth, acc = _pass_maps(c.dev, c.n)
    z_fine = _empty(c.dev, c.n, c.s + num_fine)
    uu = None if u is None else f32c(u)
    check(lib().dn_density_resample(*c.head, ptr(uu), c.n, c.s, num_fine, ptr(depth), ptr(acc), ptr(z_fine), stream()), "dn_density_resample")
    return depth, acc, z_fine


def check_refine_steps(steps, who="refine_steps"):
    """The host-side rule of the bisection count: an int (not a bool) in 0 .. 24.  Raises ValueError before any GPU work."""
    if isinstance(steps, bool) or not isinstance(steps, int) or not 0 <= steps <= _hip.MAX_REFINE_STEPS:
        raise ValueError(f"{who}: the number of bisection steps must be an int in 0 .. {_hip.MAX_REFINE_STEPS}, got {steps!r}")
    return steps


def check_refine_thresholds(m_thres, who="refine"):
    """The host-side rule of the thresholds a refinement brackets (the C layer cannot read device memory): at least one, each finite
    and >= 0 - for those relu(sigma) > m iff sigma > m, so the bracket is the Dex depth's.  Raises ValueError before any GPU work."""
    ms = [float(m) for m in (m_thres if m_thres is not None else [])]
    if not ms:
        raise ValueError(f"{who}: a refinement needs at least one Dex threshold")
    for m in ms:
        if not (math.isfinite(m) and m >= 0.0):
            raise ValueError(f"{who}: every refined threshold must be finite and >= 0, got {m!r}")
    return ms


def composite_density_brackets(rf, z, rd, m_thres):
    """dn_composite_density_brackets: composite_density's (depth, acc, dex (K,N)) without noise, then br (N,K,4) - the bracket record
    (z_lo, z_hi, s_lo, s_hi) of every first crossing - and z_mid (N,K), the first midpoints (include/dexnerf_hip_refine.h).  m_thres: a
    list or a device tensor of K >= 1 thresholds, each >= 0 (a list is checked here; a tensor is the caller's to validate)."""
    if not torch.is_tensor(m_thres):
        check_refine_thresholds(m_thres, "composite_density_brackets")
    c = _sigma_call(rf, z, rd, None, 0.0, m_thres)
    if not c.k:
        raise ValueError("composite_density_brackets: a refinement needs at least one Dex threshold")
    depth, acc = _pass_maps(c.dev, c.n)
    dex, br, z_mid = _empty(c.dev, c.k, c.n), _empty(c.dev, c.n, c.k, 4), _empty(c.dev, c.n, c.k)
    check(lib().dn_composite_density_brackets(*c.head[:4], ptr(c.thres), c.k, c.n, c.s, ptr(depth), ptr(acc), ptr(dex), ptr(br), ptr(z_mid),
                                              stream()), "dn_composite_density_brackets")
    return depth, acc, dex, br, z_mid


def dex_bisect(br, rf_mid, m_thres, z_mid=None):
    """dn_dex_bisect: one bisection step IN PLACE on the records br (N,K,4) with the density network's rows rf_mid (N,K,4) at the
    current midpoints; returns the next midpoints z_mid (N,K) (written into `z_mid` when given).  m_thres: a device tensor (K,)."""
    n, k = br.shape[0], br.shape[1]
    assert br.dtype == torch.float32 and br.is_contiguous() and br.shape == (n, k, 4) and m_thres.numel() == k
    rf_mid = f32c(rf_mid)
    assert rf_mid.numel() == n * k * 4
    z_mid = _empty(br.device, n, k) if z_mid is None else z_mid
    assert z_mid.dtype == torch.float32 and z_mid.is_contiguous() and z_mid.numel() == n * k
    check(lib().dn_dex_bisect(ptr(br), ptr(rf_mid), ptr(m_thres), k, n, ptr(z_mid), stream()), "dn_dex_bisect")
    return z_mid


def dex_refine_finish(br, m_thres, want_width=True):
    """dn_dex_refine_finish: (refined (K,N), width (K,N) | None) of the records br (N,K,4): the linear interpolation of the last
    bracket; width -1 marks rays without a crossing (refined = z[0], the Dex fallback), 0 a crossing at the first sample."""
    br = f32c(br)
    n, k = br.shape[0], br.shape[1]
    assert br.shape == (n, k, 4) and m_thres.numel() == k
    refined = _empty(br.device, k, n)
    width = _empty(br.device, k, n) if want_width else None
    check(lib().dn_dex_refine_finish(ptr(br), ptr(m_thres), k, n, ptr(refined), ptr(width), stream()), "dn_dex_refine_finish")
    return refined, width


def render_refined_records_offset(n, num_coarse, num_fine):
    """Byte offset of the bracket records br (N,K,4) in dn_render_rays_depth_refined's workspace (include/dexnerf_hip_refine.h)."""
    return lib().dn_render_depth_workspace_bytes(n, num_coarse, num_fine) - 256


def render_rays_depth(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, m_thres, draws=None, quantiles=None,
                      interp=False, refine_steps=None, want_width=False):
    """dn_render_rays_depth: the depth-only predict_and_render_radiance forward for one ray chunk (no autograd, no colour) on
    density packs (FlexibleNeRFModel.packed_density).  m_thres: a device tensor of K thresholds (any K) or None.
    quantiles: a device tensor of Q <= 64 opacity quantiles the caller has validated (check_quantiles) - the call then goes to
    dn_render_rays_depth_quantiles (same launches, the last pass composited by the quantile kernel) and returns qdepth (Q,N) as a
    sixth value; None: the call and the return are what they were.
    refine_steps: an int in 0 .. 24 - the call then goes to dn_render_rays_depth_refined (the last compositing launch writes the
    first-crossing brackets, then `refine_steps` bisections on the last pass's density network, then the finish) and returns
    refined (K,N) as a sixth value and, with want_width, width (K,N) as a seventh.  The thresholds must be >= 0 (the caller validates
    them: check_refine_thresholds), noise_std 0; not together with quantiles.  None: the call and the return are what they were."""
    if refine_steps is not None:
        check_refine_steps(refine_steps, "render_rays_depth: refine_steps")
        if quantiles is not None:
            raise ValueError("render_rays_depth: refine_steps together with quantiles is not supported")
        if float(noise_std) != 0.0:
            raise ValueError("render_rays_depth: refine_steps brackets the raw density: noise_std must be 0")
        if m_thres is None or not int(m_thres.numel()):
            raise ValueError("render_rays_depth: a refinement needs at least one Dex threshold")
    c = _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws)
    n, dev = c.n, c.dev
    if refine_steps is None:
        ws = _render_workspace(dev, lib().dn_render_depth_workspace_bytes(n, num_coarse, c.nf))
    else:
        ws = _render_workspace(dev, _sized(lib().dn_render_depth_refined_workspace_bytes(n, num_coarse, c.nf, c.k),
                                           "dn_render_depth_refined_workspace_bytes"))
    maps = _pass_maps(dev, n) + _pass_maps(dev, n, c.fine) + (_empty(dev, c.k, n) if c.k else None,)
    args = [*c.net_args, packed_c.precision, ptr(c.rays), c.rays.shape[1], n, num_coarse, c.nf, int(bool(lindisp)), float(noise_std),
            ptr(m_thres) if c.k else None, c.k, *[ptr(d) for d in c.draws], *[ptr(m) for m in maps]]
    if refine_steps is not None:
        refined = _empty(dev, c.k, n)
        width = _empty(dev, c.k, n) if want_width else None
        check(lib().dn_render_rays_depth_refined(*args, refine_steps, ptr(refined), ptr(width), ptr(ws), stream()),
              "dn_render_rays_depth_refined")
        return maps + ((refined, width) if want_width else (refined,))
    if quantiles is None:
        check(lib().dn_render_rays_depth(*args, ptr(ws), stream()), "dn_render_rays_depth")
        return maps
    nq = int(quantiles.numel())
    if not 1 <= nq <= _hip.MAX_QUANTILES or quantiles.dtype != torch.float32:
        raise ValueError(f"render_rays_depth: quantiles must be a float32 device tensor of 1 .. {_hip.MAX_QUANTILES} values")
    qdepth = _empty(dev, nq, n)
    check(lib().dn_render_rays_depth_quantiles(*args, ptr(quantiles), nq, int(bool(interp)), ptr(qdepth), ptr(ws), stream()),
          "dn_render_rays_depth_quantiles")
    return maps + (qdepth,)


# ---- Dex depth layers (include/dexnerf_hip_layers.h) --------------------------------------------------------------------------------
def check_layers(layers, who="layers"):
    """The host-side rule of the layer count: an int (not a bool) in 1 .. 8.  Raises ValueError before any GPU work."""
    if isinstance(layers, bool) or not isinstance(layers, int) or not 1 <= layers <= _hip.MAX_LAYERS:
        raise ValueError(f"{who}: the number of layers must be an int in 1 .. {_hip.MAX_LAYERS}, got {layers!r}")
    return layers


def _check_layer_records(who, n, k, layers):
    if k * 2 * layers > _hip.MAX_LAYER_RECORDS:
        raise ValueError(f"{who}: at most {_hip.MAX_LAYER_RECORDS} records per ray (thresholds * 2 layers), got {k} * {2 * layers}")
    if n * k * 2 * layers > 2 ** 31 - 1:
        raise ValueError(f"{who}: at most 2^31 - 1 records (rays * thresholds * 2 layers), got {n} * {k} * {2 * layers}")


def composite_density_layers(rf, z, rd, m_thres, layers):
    """dn_composite_density_layers: composite_density's (depth, acc, dex (K,N)) without noise, then br (N,K,2L,4) - the bracket records
    (z_lo, z_hi, s_lo, s_hi) of the first 2L entries into / exits from {sigma > m} -, z_mid (N,K*2L), their first midpoints, and
    count (K,N) int32, the number of events of every ray (include/dexnerf_hip_layers.h).  m_thres: a list or a device tensor of K >= 1
    thresholds, each >= 0 (a list is checked here; a tensor is the caller's to validate)."""
    check_layers(layers, "composite_density_layers")
    if not torch.is_tensor(m_thres):
        check_refine_thresholds(m_thres, "composite_density_layers")
    c = _sigma_call(rf, z, rd, None, 0.0, m_thres)
    if not c.k:
        raise ValueError("composite_density_layers: the layers need at least one Dex threshold")
    _check_layer_records("composite_density_layers", c.n, c.k, layers)
    depth, acc = _pass_maps(c.dev, c.n)
    dex, br, z_mid = _empty(c.dev, c.k, c.n), _empty(c.dev, c.n, c.k, 2 * layers, 4), _empty(c.dev, c.n, c.k * 2 * layers)
    count = torch.empty((c.k, c.n), dtype=torch.int32, device=c.dev)
    check(lib().dn_composite_density_layers(*c.head[:4], ptr(c.thres), c.k, layers, c.n, c.s, ptr(depth), ptr(acc), ptr(dex), ptr(br),
                                            ptr(z_mid), ptr(count), stream()), "dn_composite_density_layers")
    return depth, acc, dex, br, z_mid, count


def dex_layers_finish(br, m_thres, interp, want_width=True):
    """dn_dex_layers_finish: (events (K,2L,N), width (K,2L,N) | None) of the records br (N,K,2L,4).  interp False: the depth of the
    sample at which the state changes; True: the linear interpolation of the bracket.  A missing event: depth +inf, width -1."""
    br = f32c(br)
    n, k, e = br.shape[0], br.shape[1], br.shape[2]
    assert br.shape == (n, k, e, 4) and e % 2 == 0 and m_thres.numel() == k
    events = _empty(br.device, k, e, n)
    width = _empty(br.device, k, e, n) if want_width else None
    check(lib().dn_dex_layers_finish(ptr(br), ptr(m_thres), k, e // 2, int(bool(interp)), n, ptr(events), ptr(width), stream()),
          "dn_dex_layers_finish")
    return events, width


def render_rays_depth_layers(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, m_thres, layers, refine_steps=None,
                             want_width=False, draws=None):
    """dn_render_rays_depth_layers: render_rays_depth's five maps for one ray chunk on density packs, then events (K,2L,N), count (K,N)
    int32 and width (K,2L,N) | None - the depth layers of the last pass (include/dexnerf_hip_layers.h).  m_thres: a device tensor of
    K >= 1 thresholds, each >= 0 (the caller validates them: check_refine_thresholds).  refine_steps None: sample mode - no network
    launch beyond the render's; an int in 0 .. 24: interpolated mode after that many bisections on the last pass's density network.
    noise_std must be 0.  The workspace is render_rays_depth's cached one: render_status_words reads this call's status block."""
    check_layers(layers, "render_rays_depth_layers")
    if refine_steps is not None:
        check_refine_steps(refine_steps, "render_rays_depth_layers: refine_steps")
    if float(noise_std) != 0.0:
        raise ValueError("render_rays_depth_layers: the events are those of the raw density: noise_std must be 0")
    if m_thres is None or not int(m_thres.numel()):
        raise ValueError("render_rays_depth_layers: the layers need at least one Dex threshold")
    c = _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws)
    n, dev = c.n, c.dev
    _check_layer_records("render_rays_depth_layers", n, c.k, layers)
    ws = _render_workspace(dev, _sized(lib().dn_render_depth_layers_workspace_bytes(n, num_coarse, c.nf, c.k, layers),
                                       "dn_render_depth_layers_workspace_bytes"))
    maps = _pass_maps(dev, n) + _pass_maps(dev, n, c.fine) + (_empty(dev, c.k, n),)
    events = _empty(dev, c.k, 2 * layers, n)
    count = torch.empty((c.k, n), dtype=torch.int32, device=dev)
    width = _empty(dev, c.k, 2 * layers, n) if want_width else None
    check(lib().dn_render_rays_depth_layers(
        *c.net_args, packed_c.precision, ptr(c.rays), c.rays.shape[1], n, num_coarse, c.nf, int(bool(lindisp)), float(noise_std), ptr(m_thres),
        c.k, *[ptr(d) for d in c.draws], *[ptr(m) for m in maps], layers, -1 if refine_steps is None else refine_steps, ptr(events),
        ptr(count), ptr(width), ptr(ws), stream()), "dn_render_rays_depth_layers")
    return maps + (events, count, width)


# ---- density-gradient surface normals (include/dexnerf_hip_normals.h) ---------------------------------------------------------------
class DensityGradStreams:
    """The backward-data and input-gradient streams of the DENSITY sub-network a PackedDensityMLP holds (dn_mlp_pack_backward /
    dn_mlp_pack_input_grad on its density descriptor), packed from a no-view-direction network's weight list
    [layer1, trunk..., head (4,W)] (FlexibleNeRFModel.packed_density_grad builds the head).  fp32, or bf16 with 16-bit saves: the
    library refuses the sizes of anything else."""

    def __init__(self, packed_density):
        self.desc, self.precision = packed_density.desc, packed_density.precision
        dev = packed_density.buffer.device
        d, prec = ctypes.byref(self.desc), self.precision
        self.buffer_ig = torch.empty(_sized(lib().dn_mlp_input_grad_packed_bytes(d, prec), "dn_mlp_input_grad_packed_bytes"),
                                     dtype=torch.uint8, device=dev)
        self.buffer_bwd = torch.empty(_sized(lib().dn_mlp_backward_packed_bytes(d, prec), "dn_mlp_backward_packed_bytes"),
                                      dtype=torch.uint8, device=dev)
        self.key = None          # parameter key both streams were packed from

    def pack(self, weights_bwd, weights_ig):
        wb, keep_b = _ptr_array(weights_bwd, sources=True)
        wi, keep_i = _ptr_array(weights_ig, sources=True)
        self._keep = (keep_b, keep_i)   # until the pack kernels have run on this stream
        d = ctypes.byref(self.desc)
        check(lib().dn_mlp_pack_backward(d, self.precision, wb, ptr(self.buffer_bwd), stream()), "dn_mlp_pack_backward")
        check(lib().dn_mlp_pack_input_grad(d, self.precision, wi, ptr(self.buffer_ig), stream()), "dn_mlp_pack_input_grad")


def composite_normals(rf, z, rd, g_pts, noise, noise_std, m_thres, want_dex=True):
    """dn_composite_normals: (depth, acc, dex (K,N) | None, normal (N,3), dex_normal (K,N,3) | None) from the sigma column of rf (N,S,4)
    and the per-sample density gradients g_pts (N,S,3).  m_thres: a list of K thresholds or a device tensor of them (any K);
    want_dex=False leaves the Dex depths out (the Dex normals alone)."""
    c = _sigma_call(rf, z, rd, noise, noise_std, m_thres)
    g_pts = f32c(g_pts)
    n, dev, k = c.n, c.dev, c.k
    (depth, acc), normal = _pass_maps(dev, n), _empty(dev, n, 3)
    dex = _empty(dev, k, n) if (k and want_dex) else None
    dex_normal = _empty(dev, k, n, 3) if k else None
    check(lib().dn_composite_normals(*c.head, ptr(g_pts), ptr(c.thres), k, n, c.s, ptr(depth), ptr(acc), ptr(dex), ptr(normal),
                                     ptr(dex_normal), stream()), "dn_composite_normals")
    return depth, acc, dex, normal, dex_normal


def density_gradient(packed_density, streams, rays=None, pts=None, z=None):
    """(sigma_raw, d sigma_raw / d x) of the density sub-network at points given as `pts` (..., 3) -> ((...), (..., 3)) or as ray rows
    `rays` (N, >= 8) + depths `z` (N,S) -> ((N,S), (N,S,3)); x is the network's input space.  The training forward of the density
    pack, the seed g_out = (0,0,0,1), dn_mlp_backward_data on streams.buffer_bwd and dn_mlp_backward_input on streams.buffer_ig - in
    the ray form its per-point d_pts are read where it leaves them, the first region of its workspace.  Precision = the pack's
    (fp32, or bf16 with 16-bit saves)."""
    desc, prec = ctypes.byref(packed_density.desc), packed_density.precision
    if rays is not None:
        rays, z = f32c(rays), f32c(z)
        n, s = z.shape
        out, _, masks = run_network_train(packed_density, None, None, None, rays=rays, z_vals=z, prec=prec)
        shape = (n, s)
    else:
        shape = tuple(pts.shape[:-1])
        pts = f32c(pts).reshape(-1, 3)
        n, s = pts.shape[0], 1
        out, _, masks = run_network_train(packed_density, pts, None, 1, prec=prec)
    n_pts = n * s
    dev = out.device
    g_out = torch.zeros((n_pts, 4), dtype=torch.float32, device=dev)
    g_out[:, 3] = 1.0
    grads = _grads_buf(packed_density, n_pts, prec, dev)
    check(lib().dn_mlp_backward_data(desc, prec, ptr(streams.buffer_bwd), ptr(g_out), ptr(masks), n_pts, ptr(grads), stream()),
          "dn_mlp_backward_data")
    if rays is None:
        g_pts = torch.empty_like(pts)
        check(lib().dn_mlp_backward_input(desc, prec, ptr(streams.buffer_ig), ptr(grads), ptr(pts), None, None, 0, None, n, s, ptr(g_pts), None,
                                          None, None, None, 0, stream()), "dn_mlp_backward_input")
    else:
        nbytes = int(lib().dn_mlp_backward_input_workspace_bytes(desc, n_pts, 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d_rays, d_z = torch.empty_like(rays), torch.empty_like(z)
        check(lib().dn_mlp_backward_input(desc, prec, ptr(streams.buffer_ig), ptr(grads), None, None, ptr(rays), rays.shape[1], ptr(z), n, s, None,
                                          None, ptr(d_rays), ptr(d_z), ptr(ws), nbytes, stream()), "dn_mlp_backward_input")
        g_pts = ws[:n_pts * 12].view(torch.float32)
    return out[:, 3].reshape(shape), g_pts.reshape(shape + (3,))


def render_normals_workspace_bytes(packed_c, packed_f, n, num_coarse, num_fine):
    """dn_render_normals_workspace_bytes for these density packs (0: sizes / precision the normal render does not cover)."""
    fine = num_fine > 0 and packed_f is not None
    return int(lib().dn_render_normals_workspace_bytes(ctypes.byref(packed_c.desc), ctypes.byref(packed_f.desc) if fine else None,
                                                       packed_c.precision, n, num_coarse, num_fine if fine else 0))


def render_rays_normals(packed_c, packed_f, streams, rays, num_coarse, num_fine, lindisp, noise_std, m_thres, draws=None):
    """dn_render_rays_normals: the depth-only render of one ray chunk with its last pass differentiated, on density packs and the
    DensityGradStreams of the last pass's network (the fine one; the coarse one with num_fine == 0).  m_thres: a device tensor of K
    thresholds (any K) or None.  Returns (depth_c, acc_c, depth, acc, dex (K,N) | None, normal (N,3), dex_normal (K,N,3) | None);
    depth_c / acc_c are None without a fine pass."""
    c = _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws)
    n, dev, k = c.n, c.dev, c.k
    nbytes = _sized(render_normals_workspace_bytes(packed_c, packed_f, n, num_coarse, c.nf), "dn_render_normals_workspace_bytes")
    # (a stream-ordered allocation per call, not the cached render workspace: the saved tensors make it large, and its status
    # block is not where render_status_words looks)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    maps = _pass_maps(dev, n, c.fine) + _pass_maps(dev, n) + (_empty(dev, k, n) if k else None, _empty(dev, n, 3),
                                                              _empty(dev, k, n, 3) if k else None)
    check(lib().dn_render_rays_normals(
        *c.net_args, ptr(streams.buffer_bwd), ptr(streams.buffer_ig), packed_c.precision, ptr(c.rays), c.rays.shape[1], n, num_coarse, c.nf,
        int(bool(lindisp)), float(noise_std), ptr(m_thres) if k else None, k, *[ptr(d) for d in c.draws], *[ptr(m) for m in maps],
        ptr(ws), nbytes, stream()), "dn_render_rays_normals")
    return maps


def render_status_words(ws=None):
    """Device copy (no synchronisation) of the two status words of the last dn_render_rays / dn_render_rays_depth call on this
    stream - see render_nonfinite_count; the caller sums the copies of several chunks and reads them back once."""
    ws = _latest_render_workspace() if ws is None else ws
    return ws[ws.numel() - 256: ws.numel() - 248].view(torch.int32).clone()


def render_nonfinite_count(ws=None):
    """Status block of the last dn_render_rays / dn_render_rays_depth call on this stream (synchronises): non-finite raw
    radiance-field samples met by the compositing passes + waves of the fp16 network kernel that saw an activation leave fp16's range."""
    ws = _latest_render_workspace() if ws is None else ws
    words = ws[ws.numel() - 256: ws.numel() - 248].view(torch.int32).tolist()
    return int(words[0]) + int(words[1])


# ---- predict_and_render_radiance under autograd: one C call forward, one (or two halves) backward ----------------------
def render_rays_train(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, white, m_thres, draws=None, prec=None,
                      rng_state=None, perturb=False, geom=False):
    """dn_render_rays_train: the training forward of a whole ray chunk.  Returns (maps, saved): maps = (rgb_c, depth_c, acc_c,
    rgb_f, depth_f, acc_f, dex), saved = what dn_render_rays_backward needs (workspace, per-network act / masks, the draws).
    geom=True: dn_render_rays_train_geom - saved also holds the fine pass's resamples and what render_rays_backward_geom needs."""
    c = _render_call(packed_c, packed_f, rays, num_fine, m_thres, draws)
    rays, n, dev, fine, nf, k = c.rays, c.n, c.dev, c.fine, c.nf, c.k
    ws = torch.empty(max(lib().dn_render_train_workspace_bytes(n, num_coarse, nf), 1), dtype=torch.uint8, device=dev)
    prec = train_precision(packed_c) if prec is None else prec

    def bufs(packed, n_points):
        a, m, _ = train_sizes(packed, n_points, prec=prec)
        return torch.empty(a, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
    act_c, masks_c = bufs(packed_c, n * num_coarse)
    act_f, masks_f = bufs(packed_f, n * (num_coarse + nf)) if fine else (None, None)
    maps = _pass_maps(dev, n, rgb=True) + _pass_maps(dev, n, fine, rgb=True) + (_empty(dev, k, n) if k else None,)
    t_rand, noise_c, _, noise_f = c.draws
    args = [*c.net_args, prec, ptr(rays), rays.shape[1], n, num_coarse, nf, int(bool(lindisp)), float(noise_std), int(bool(white)),
            host_floats(m_thres), k, *[ptr(d) for d in c.draws], *[ptr(m) for m in maps], ptr(ws),
            ptr(act_c), ptr(masks_c), ptr(act_f), ptr(masks_f), ptr(rng_state), int(bool(perturb))]
    saved = dict(rays=rays, ws=ws, act_c=act_c, masks_c=masks_c, act_f=act_f, masks_f=masks_f, noise_c=noise_c,
                 noise_f=noise_f, n=n, nc=num_coarse, nf=nf, noise_std=float(noise_std), white=bool(white), prec=prec,
                 rng_state=rng_state)
    if geom:
        z_samples = _empty(dev, n, nf) if fine else None
        check(lib().dn_render_rays_train_geom(*args, ptr(z_samples), stream()), "dn_render_rays_train_geom")
        saved.update(t_rand=t_rand, z_samples=z_samples, lindisp=bool(lindisp), perturb=bool(perturb))
    else:
        check(lib().dn_render_rays_train(*args, stream()), "dn_render_rays_train")
    return maps, saved


def _backward_args(packed_c, packed_f, saved, g_c, g_f, views_c, views_f, nets, wgrad):
    """What both render backwards hand to the library for the networks in `nets`: (fine, grads_c, grads_f, the four (dW | db) pointer
    arrays, the six upstream gradients fp32-contiguous, the weight-gradient scratch and its size - (None, 0) without `wgrad`)."""
    dev = saved["rays"].device
    n, nc, nf, prec = saved["n"], saved["nc"], saved["nf"], saved["prec"]
    fine = nf > 0 and packed_f is not None
    use_c, use_f = bool(nets & 1), bool(fine and nets & 2)
    grads_c = _grads_buf(packed_c, n * nc, prec, dev) if use_c else None
    grads_f = _grads_buf(packed_f, n * (nc + nf), prec, dev) if use_f else None
    ptrs = _view_ptrs(views_c if use_c else None) + _view_ptrs(views_f if use_f else None)
    gs = [None if g is None else f32c(g) for g in tuple(g_c) + tuple(g_f)]
    scratch = _wgrad_scratch(2 if (fine and nets == 3) else 1, packed_c, *([packed_f] if fine else [])) if wgrad else (None, 0)
    return fine, grads_c, grads_f, ptrs, gs, scratch


def render_rays_backward(packed_c, packed_f, saved, g_c, g_f, views_c, views_f, nets=3, reg=None):
    """dn_render_rays_backward: composite backward -> backward-data chain -> weight gradients for the networks selected by
    `nets` (bit 0 coarse, bit 1 fine), ACCUMULATING into views_* = [(dW, db)] in linear_modules() order.
    g_c / g_f = (g_rgb, g_depth, g_acc) upstream gradients (None = zero).
    reg = ((weight_coarse, weight_fine), reg2): dn_render_rays_backward_reg in its place - the distortion regulariser of each network
    in `nets` with a non-zero weight, its gradient added ahead of the compositing backward and the mean L_ray written to reg2 (2) fp32
    ([coarse, fine]; a half writes its own word)."""
    n, nc, nf, prec = saved["n"], saved["nc"], saved["nf"], saved["prec"]
    fine, grads_c, grads_f, ptrs, gs, (scratch, scratch_bytes) = _backward_args(packed_c, packed_f, saved, g_c, g_f, views_c, views_f, nets, True)
    args = [*_net_args(packed_c, packed_f, fine, "buffers_bwd", prec), prec,
            ptr(saved["rays"]), saved["rays"].shape[1], n, nc, nf, saved["noise_std"], int(saved["white"]),
            ptr(saved["noise_c"]), ptr(saved["noise_f"]), *[ptr(g) for g in gs],
            ptr(saved["ws"]), ptr(saved["act_c"]), ptr(saved["masks_c"]), ptr(grads_c), ptr(saved["act_f"]), ptr(saved["masks_f"]),
            ptr(grads_f), *ptrs, int(nets), ptr(saved.get("rng_state")), ptr(scratch), scratch_bytes]
    reg_ws = None
    if reg is None:
        check(lib().dn_render_rays_backward_ws(*args, stream()), "dn_render_rays_backward")
    else:
        (w_c, w_f), reg2 = reg
        assert reg2.dtype == torch.float32 and reg2.is_contiguous() and reg2.numel() == 2, "render_rays_backward: reg2 is two fp32 words"
        nbytes = int(lib().dn_render_reg_workspace_bytes(n, nc, nf))
        reg_ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=saved["rays"].device)
        check(lib().dn_render_rays_backward_reg(*args, float(w_c), float(w_f), ptr(reg_ws), nbytes, ptr(reg2), stream()),
              "dn_render_rays_backward_reg")
    _note_s8_record(grads_c, prec); _note_s8_record(grads_f, prec)
    return grads_c, grads_f, scratch, reg_ws   # (kept alive by the caller until the stream has consumed them: PyTorch's caching allocator is stream-ordered)


# ---- the render with its ray gradient, and camera records from twists: the pieces of nerf.FusedPoseStep ----------------------------
def render_rays_train_geom(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, white, m_thres, draws=None, prec=None,
                           rng_state=None, perturb=False):
    """dn_render_rays_train_geom: render_rays_train that also keeps the fine pass's resamples (saved["z_samples"]) and the settings the
    geometry backward needs - what render_rays_backward_geom takes.  prec: PREC_F32, or PREC_BF16 with 16-bit saves (the default:
    the packed network's own precision, never the 8-bit-saved code)."""
    return render_rays_train(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, white, m_thres, draws,
                             packed_c.precision if prec is None else prec, rng_state, perturb, geom=True)


def render_rays_backward_geom(packed_c, packed_f, saved, g_c, g_f, views_c=None, views_f=None):
    """dn_render_rays_backward_geom on what render_rays_train_geom saved: returns (d_rays (N, stride), the buffers to keep alive until
    the stream has consumed them).  g_c / g_f = (g_rgb, g_depth, g_acc) upstream gradients (None = zero).  views_* = [(dW, db)] in
    linear_modules() order to ACCUMULATE the weight gradients into, as render_rays_backward does; None (both): frozen networks, no
    weight-gradient launch.  The packs need their backward and input-gradient streams (ensure_backward_stream /
    ensure_input_grad_stream)."""
    rays = saved["rays"]
    n, nc, nf, prec = saved["n"], saved["nc"], saved["nf"], saved["prec"]
    fine, grads_c, grads_f, ptrs, gs, (scratch, scratch_bytes) = _backward_args(packed_c, packed_f, saved, g_c, g_f, views_c, views_f, 3,
                                                                                  views_c is not None)
    desc_f = ctypes.byref(packed_f.desc) if fine else None
    nbytes = int(lib().dn_render_backward_geom_workspace_bytes(ctypes.byref(packed_c.desc), desc_f, n, rays.shape[1], nc, nf))
    geom_ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=rays.device)
    d_rays = torch.empty_like(rays)
    check(lib().dn_render_rays_backward_geom(
        ctypes.byref(packed_c.desc), ptr(packed_c.buffers_bwd[prec]), ptr(packed_c.buffer_ig),
        desc_f, ptr(packed_f.buffers_bwd[prec]) if fine else None, ptr(packed_f.buffer_ig) if fine else None, prec,
        ptr(rays), rays.shape[1], n, nc, nf, int(saved["lindisp"]), int(saved["perturb"]), saved["noise_std"], int(saved["white"]),
        ptr(saved["t_rand"]), ptr(saved["noise_c"]), ptr(saved["noise_f"]), ptr(saved["z_samples"]), *[ptr(g) for g in gs],
        ptr(saved["ws"]), ptr(saved["act_c"]), ptr(saved["masks_c"]), ptr(grads_c), ptr(saved["act_f"]), ptr(saved["masks_f"]), ptr(grads_f),
        *ptrs, ptr(saved.get("rng_state")), ptr(scratch), scratch_bytes, ptr(geom_ws), nbytes, ptr(d_rays), stream()),
        "dn_render_rays_backward_geom")
    return d_rays, (grads_c, grads_f, scratch, geom_ws, gs)


def _pose_inputs(xi, e0):
    assert xi.is_cuda and xi.dtype == torch.float32 and xi.is_contiguous() and xi.dim() == 2 and xi.shape[1] == 6, "xi: (V,6) fp32 on the device"
    n_views = int(xi.shape[0])
    assert e0.is_cuda and e0.dtype == torch.float32 and e0.is_contiguous() and e0.numel() == 16 * n_views, "e0: (V,4,4) fp32 on the device"
    return n_views


def pose_records(xi, e0, k, ndc_focal=None, cams=None, extrinsics=None, want_extrinsics=False):
    """dn_pose_records: the camera records (V,16) of E_v = se3_exp(xi[v]) @ e0[v] - xi (V,6) fp32 (omega, t), e0 (V,4,4) fp32
    world->camera, k (3,3) shared or (V,3,3), all on the device.  `cams` / `extrinsics`: buffers to write into (else allocated).
    Returns cams, or (cams, extrinsics (V,4,4)) with want_extrinsics / an extrinsics buffer."""
    n_views = _pose_inputs(xi, e0)
    assert k.is_cuda and k.dtype == torch.float32 and k.is_contiguous() and k.numel() in (9, 9 * n_views), "k: (3,3) or (V,3,3) fp32 on the device"
    if cams is None:
        cams = torch.empty((n_views, 16), dtype=torch.float32, device=xi.device)
    if extrinsics is None and want_extrinsics:
        extrinsics = torch.empty((n_views, 4, 4), dtype=torch.float32, device=xi.device)
    check(lib().dn_pose_records(ptr(xi), ptr(e0), ptr(k), int(k.dim() == 3), float(ndc_focal or 0.0), n_views, ptr(cams), ptr(extrinsics),
                                stream()), "dn_pose_records")
    return cams if extrinsics is None else (cams, extrinsics)


def pose_records_backward(g_cams, xi, e0, out=None, keep=None):
    """dn_pose_records_backward: g_xi (V,6) from g_cams (V,16) (camera_grad_views' output) at the given xi / e0.  `out`: the tensor to
    write (else allocated); `keep`: a second tensor that receives the same values."""
    n_views = _pose_inputs(xi, e0)
    assert g_cams.is_cuda and g_cams.dtype == torch.float32 and g_cams.is_contiguous() and g_cams.shape == (n_views, 16)
    if out is None:
        out = torch.empty((n_views, 6), dtype=torch.float32, device=xi.device)
    check(lib().dn_pose_records_backward(ptr(g_cams), ptr(xi), ptr(e0), n_views, ptr(out), ptr(keep), stream()), "dn_pose_records_backward")
    return out


def _intrinsics_inputs(phi, k, scale, n_views):
    """(phi_per_view, k_per_view) for phi None | (3,) shared | (V,3) per view and k (3,3) | (V,3,3), fp32 on the device."""
    assert k.is_cuda and k.dtype == torch.float32 and k.is_contiguous() and k.dim() in (2, 3) and k.numel() in (9, 9 * n_views), \
        "k: (3,3) or (V,3,3) fp32 on the device"
    assert float(scale) > 0.0, "intrinsics_scale: a positive number"
    if phi is None:
        return 0, int(k.dim() == 3)
    assert phi.is_cuda and phi.dtype == torch.float32 and phi.is_contiguous() and (phi.shape == (3,) or phi.shape == (n_views, 3)), \
        "phi: (3,) shared or (V,3) per view, fp32 on the device"
    return int(phi.dim() == 2), int(k.dim() == 3)


def camera_records(xi, phi, e0, k, intrinsics_scale=1.0, ndc_focal=None, cams=None, extrinsics=None, want_extrinsics=False):
    """dn_camera_records: pose_records with slots 12:15 from phi - fx = fx0 exp(s a), cx = cx0 + s fx0 b, cy = cy0 + s fx0 c, s =
    `intrinsics_scale`; phi (3,) shared by the views, (V,3) per view, or None (zeros: pose_records' bits)."""
    n_views = _pose_inputs(xi, e0)
    phi_per_view, k_per_view = _intrinsics_inputs(phi, k, intrinsics_scale, n_views)
    if cams is None:
        cams = torch.empty((n_views, 16), dtype=torch.float32, device=xi.device)
    if extrinsics is None and want_extrinsics:
        extrinsics = torch.empty((n_views, 4, 4), dtype=torch.float32, device=xi.device)
    check(lib().dn_camera_records(ptr(xi), ptr(phi), phi_per_view, float(intrinsics_scale), ptr(e0), ptr(k), k_per_view, float(ndc_focal or 0.0),
                                  n_views, ptr(cams), ptr(extrinsics), stream()), "dn_camera_records")
    return cams if extrinsics is None else (cams, extrinsics)


def camera_records_scratch_bytes(n_views):
    return int(lib().dn_camera_records_scratch_bytes(int(n_views)))


def camera_records_backward(g_cams, xi, phi, e0, k, intrinsics_scale=1.0, pose_mask=None, shared=None, out=None, keep=None, out_phi=None,
                            keep_phi=None, want_phi=True):
    """dn_camera_records_backward: (g_xi (V,6), g_phi (3,) | (V,3) | None) from g_cams (V,16) at the given xi / phi.  `pose_mask` (V)
    int32: views with 0 get exact zeros in g_xi.  phi None: `shared` says which gradient is wanted (True (3,), False (V,3)).  `out` /
    `out_phi`: the tensors to write (else allocated); `keep` / `keep_phi`: second tensors that receive the same values;
    want_phi=False: g_xi alone.  A shared g_phi is summed in view order over a scratch allocated here."""
    n_views = _pose_inputs(xi, e0)
    phi_per_view, k_per_view = _intrinsics_inputs(phi, k, intrinsics_scale, n_views)
    if phi is None:
        phi_per_view = int(shared is False)
    assert g_cams.is_cuda and g_cams.dtype == torch.float32 and g_cams.is_contiguous() and g_cams.shape == (n_views, 16)
    if pose_mask is not None:
        assert pose_mask.is_cuda and pose_mask.dtype == torch.int32 and pose_mask.is_contiguous() and pose_mask.shape == (n_views,), \
            "pose_mask: (V) int32 on the device"
    if out is None:
        out = torch.empty((n_views, 6), dtype=torch.float32, device=xi.device)
    scratch, nbytes = None, 0
    if want_phi:
        shape = (n_views, 3) if phi_per_view else (3,)
        if out_phi is None:
            out_phi = torch.empty(shape, dtype=torch.float32, device=xi.device)
        for t in (out_phi, keep_phi):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == shape), f"g_phi: {shape} fp32"
        if not phi_per_view:
            nbytes = camera_records_scratch_bytes(n_views)
            scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=xi.device)
    else:
        assert out_phi is None and keep_phi is None
    g_in, xi_in, e0_in, g_out = g_cams, xi, e0, out
    if n_views == 0:   # empty tensors carry NULL data pointers, which the entry point refuses: one unread element each
        g_in = xi_in = e0_in = g_out = torch.zeros(1, dtype=torch.float32, device=k.device)
        pose_mask = keep = None
    check(lib().dn_camera_records_backward(ptr(g_in), ptr(xi_in), ptr(phi), phi_per_view, float(intrinsics_scale), ptr(e0_in), ptr(k), k_per_view,
                                           ptr(pose_mask), n_views, ptr(g_out), ptr(keep), ptr(out_phi), ptr(keep_phi), ptr(scratch), nbytes,
                                           stream()), "dn_camera_records_backward")
    return out, out_phi


# ---- the Dex threshold surface as a triangle mesh (include/dexnerf_hip_mesh.h) ----------------------------------------------------------
def check_isosurface_grid(xs, ys, zs, level, who="isosurface"):
    """The host-side rule of the grid and the level (the C layer cannot read device memory, and takes the level by value): the level
    finite as fp32, every axis a 1-D fp32 tensor of >= 2 finite, strictly increasing coordinates.  Returns the level as the Python
    float of its fp32 value.  Raises ValueError before any GPU work."""
    level = float(level)
    l32 = ctypes.c_float(level).value if math.isfinite(level) else level
    if not math.isfinite(l32):
        raise ValueError(f"{who}: the level must be finite as fp32, got {level!r}")
    for name, c in (("xs", xs), ("ys", ys), ("zs", zs)):
        if not (torch.is_tensor(c) and c.dim() == 1 and c.dtype == torch.float32 and c.numel() >= 2):
            raise ValueError(f"{who}: {name} must be a 1-D fp32 tensor of at least 2 coordinates")
        h = c.detach().cpu()
        if not (bool(torch.isfinite(h).all()) and bool((h[1:] > h[:-1]).all())):
            raise ValueError(f"{who}: {name} must be finite and strictly increasing")
    return l32


class IsosurfaceCount:
    """What dn_isosurface_count leaves behind: the arguments, the workspace the scans filled and the device record `counts`
    (int32 x 4: n_vertices, n_triangles, n_nonfinite, 0) - isosurface_emit's input."""

    def __init__(self, field, stride, xs, ys, zs, level, workspace, counts):
        self.field, self.stride, self.xs, self.ys, self.zs, self.level = field, stride, xs, ys, zs, level
        self.workspace, self.counts = workspace, counts

    def totals(self):
        """(n_vertices, n_triangles, n_nonfinite) on the host: the one read a data-dependent output size needs."""
        return tuple(int(c) for c in self.counts[:3].tolist())

    def _grid_args(self):
        return (c_void_p(self.field.data_ptr()), self.stride, ptr(self.xs), ptr(self.ys), ptr(self.zs), self.xs.numel(), self.ys.numel(),
                self.zs.numel(), self.level, ptr(self.workspace))


def isosurface_count(field, xs, ys, zs, level):
    """dn_isosurface_count on field (nx,ny,nz) fp32 - dense, or a view whose strides are (ny*nz*s, nz*s, s) floats such as column 3 of
    the network's (P,4) rows (s = 4), which is read in place - over the grid xs (nx), ys (ny), zs (nz) -> IsosurfaceCount."""
    level = check_isosurface_grid(xs, ys, zs, level, "isosurface")
    if not (torch.is_tensor(field) and field.dim() == 3 and tuple(field.shape) == (xs.numel(), ys.numel(), zs.numel())):
        raise ValueError("isosurface: the field must be (nx, ny, nz) for the coordinate tensors xs (nx), ys (ny), zs (nz)")
    for t in (field, xs, ys, zs):
        if not t.is_cuda:
            raise RuntimeError("isosurface: the extraction runs on the ROCm device only (got a host tensor); move the inputs to 'cuda'")
    nx, ny, nz = field.shape
    s = field.stride(2)
    if not (field.dtype == torch.float32 and 1 <= s < 2 ** 31 and field.stride() == (ny * nz * s, nz * s, s)):
        field, s = f32c(field), 1
    xs, ys, zs = xs.contiguous(), ys.contiguous(), zs.contiguous()
    nbytes = int(lib().dn_isosurface_workspace_bytes(nx, ny, nz))
    if nbytes == 0:
        raise ValueError(f"isosurface: a {nx} x {ny} x {nz} grid is past the extraction's maximum ({_hip.ISO_MAX_GRID_VERTICES} grid "
                         "vertices, 12 * cells < 2^31)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=field.device)
    out = IsosurfaceCount(field, int(s), xs, ys, zs, level, ws, torch.empty(4, dtype=torch.int32, device=field.device))
    check(lib().dn_isosurface_count(*out._grid_args(), ptr(out.counts), stream()), "dn_isosurface_count")
    return out


def isosurface_emit(counted, max_vertices, max_triangles, vertices=None, triangles=None):
    """dn_isosurface_emit on an IsosurfaceCount: rows below the capacities are written into `vertices` (>= max_vertices, 3) fp32 and
    `triangles` (>= max_triangles, 3) int32 (allocated at the capacities when not given) -> (vertices, triangles)."""
    dev = counted.field.device
    max_vertices, max_triangles = int(max_vertices), int(max_triangles)
    if vertices is None:
        vertices = torch.empty((max(max_vertices, 0), 3), dtype=torch.float32, device=dev)
    if triangles is None:
        triangles = torch.empty((max(max_triangles, 0), 3), dtype=torch.int32, device=dev)
    assert vertices.dtype == torch.float32 and vertices.shape[0] >= max_vertices and vertices.shape[1:] == (3,)
    assert triangles.dtype == torch.int32 and triangles.shape[0] >= max_triangles and triangles.shape[1:] == (3,)
    check(lib().dn_isosurface_emit(*counted._grid_args(), max_vertices, max_triangles, ptr(vertices) if max_vertices > 0 else None,
                                   ptr(triangles) if max_triangles > 0 else None, stream()), "dn_isosurface_emit")
    return vertices, triangles


def isosurface(field, xs, ys, zs, level):
    """The surface {f > level} of a sampled field as an indexed triangle mesh (marching tetrahedra on the Kuhn triangulation of the
    grid; the definition, the vertex and triangle order and the orientation - normals toward decreasing f - are those of
    include/dexnerf_hip_mesh.h) -> (vertices (V,3) fp32, triangles (T,3) int32, n_nonfinite).  One host read between count and emit
    sizes the outputs; an empty surface gives (0,3) tensors."""
    counted = isosurface_count(field, xs, ys, zs, level)
    n_v, n_t, n_bad = counted.totals()
    vertices, triangles = isosurface_emit(counted, n_v, n_t)
    return vertices, triangles, n_bad


# ---- occupancy-grid culling of the depth-only render (include/dexnerf_hip_occupancy.h) ---------------------------------------------------
def check_occupancy_grid(bounds, cells, who="occupancy"):
    """The host-side rule of an occupancy grid: bounds (x0,y0,z0,x1,y1,z1) finite as fp32 with x1 > x0, y1 > y0, z1 > z0; cells N or
    (cx,cy,cz), each 1 .. 2^24, their product at most 2^30.  Returns (bounds as the Python floats of their fp32 values, (cx,cy,cz), the
    three scales cells / (b1 - b0): formed in float64 from the fp32 bounds and rounded to fp32 once, as the header asks).  Raises
    ValueError before any GPU work."""
    import numbers
    try:
        b = [float(v) for v in bounds]
        c = [int(cells)] * 3 if isinstance(cells, numbers.Integral) else [int(v) for v in cells]
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: bounds are six numbers and cells is N or (cx, cy, cz): {e}") from None
    if len(b) != 6 or len(c) != 3:
        raise ValueError(f"{who}: bounds are (x0, y0, z0, x1, y1, z1) and cells is N or (cx, cy, cz)")
    if not all(math.isfinite(v) for v in b):
        raise ValueError(f"{who}: the bounds must be finite, got {b}")
    b = [ctypes.c_float(v).value for v in b]
    if not all(math.isfinite(v) for v in b) or any(b[a + 3] <= b[a] for a in range(3)):
        raise ValueError(f"{who}: the bounds must be finite as fp32 with x1 > x0, y1 > y0, z1 > z0, got {b}")
    if min(c) < 1 or max(c) > _hip.OCC_MAX_AXIS_CELLS or c[0] * c[1] * c[2] > _hip.OCC_MAX_CELLS:
        raise ValueError(f"{who}: every axis needs 1 .. {_hip.OCC_MAX_AXIS_CELLS} cells and the grid at most {_hip.OCC_MAX_CELLS}, got {c}")
    scale = [ctypes.c_float(c[a] / (b[a + 3] - b[a])).value for a in range(3)]
    if not all(math.isfinite(s) and s > 0.0 for s in scale):
        raise ValueError(f"{who}: cells / (b1 - b0) must be finite and > 0 as fp32, got {scale}")
    return tuple(b), tuple(c), tuple(scale)


def occupancy_words(cells):
    return (int(cells[0]) * int(cells[1]) * int(cells[2]) + 31) // 32


def occupancy_build(field, cells, level, dilate=0, bits=None, accumulate=False):
    """dn_occupancy_build: the bit grid (int32 words, cell c = bit c & 31 of word c >> 5) of the cells (cx,cy,cz) from the vertex field
    (cx+1, cy+1, cz+1) fp32 - dense, or a strided view read in place like isosurface_count's.  A cell is set iff one of its corners is
    non-finite or > level, dilated by `dilate` cells (Chebyshev).  bits given and accumulate: OR-ed into it."""
    cells = tuple(int(c) for c in cells)
    level = float(level)
    l32 = ctypes.c_float(level).value if math.isfinite(level) else level
    if not math.isfinite(l32):
        raise ValueError(f"occupancy_build: the level must be finite as fp32, got {level!r}")
    dilate = int(dilate)
    if not 0 <= dilate <= _hip.OCC_MAX_DILATE:
        raise ValueError(f"occupancy_build: dilate must be 0 .. {_hip.OCC_MAX_DILATE}, got {dilate}")
    if not (torch.is_tensor(field) and field.dim() == 3 and tuple(field.shape) == tuple(c + 1 for c in cells)):
        raise ValueError("occupancy_build: the field must be (cx+1, cy+1, cz+1): the density at the cells' corners")
    if not field.is_cuda:
        raise RuntimeError("occupancy_build: runs on the ROCm device only (got a host tensor); move the field to 'cuda'")
    n_words = int(lib().dn_occupancy_words(*cells))
    if n_words == 0:
        raise ValueError(f"occupancy_build: cells {cells} are past the grid's maximum")
    ny, nz = field.shape[1:]
    s = field.stride(2)
    if not (field.dtype == torch.float32 and 1 <= s < 2 ** 31 and field.stride() == (ny * nz * s, nz * s, s)):
        field, s = f32c(field), 1
    dev = field.device
    if bits is None:
        if accumulate:
            raise ValueError("occupancy_build: accumulate needs the bits to accumulate into")
        bits = torch.empty(n_words, dtype=torch.int32, device=dev)
    assert bits.dtype == torch.int32 and bits.numel() == n_words and bits.device == dev
    scratch = torch.empty(n_words, dtype=torch.int32, device=dev) if dilate > 0 else None
    check(lib().dn_occupancy_build(c_void_p(field.data_ptr()), int(s), *cells, l32, dilate, int(bool(accumulate)), ptr(scratch), ptr(bits),
                                   stream()), "dn_occupancy_build")
    return bits


def occupancy_compact_count(rays, z, grid):
    """dn_occupancy_compact_count of the samples rays (N, >= 8) x z (N,S) against `grid` (bits, cells, bounds, scale: an
    nerf.OccupancyGrid) -> (slot (N,S) int32: the rank among the kept samples or -1, record int32 x 4 on the device: n_kept, N*S, 0, 0,
    the workspace - a counting occupancy_gather reuses it)."""
    rays, z = f32c(rays), f32c(z)
    n, s = z.shape
    nbytes = int(lib().dn_occupancy_compact_workspace_bytes(n, s))
    if nbytes == 0:
        raise ValueError(f"occupancy: {n} rays x {s} samples are outside the compaction (1 .. {_hip.OCC_MAX_SAMPLES_PER_RAY} samples per ray, "
                         f"at most {_hip.OCC_MAX_SAMPLES} in all)")
    dev = z.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    slot = torch.empty((n, s), dtype=torch.int32, device=dev)
    record = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib().dn_occupancy_compact_count(ptr(rays), rays.shape[1], ptr(z), n, s, ptr(grid.bits), *grid.cells, *grid.bounds, *grid.scale,
                                           ptr(ws), ptr(slot), ptr(record), stream()), "dn_occupancy_compact_count")
    return slot, record, ws


def occupancy_compact_emit_dirs(rays, z, slot, max_points, pts=None, dirs=None, want_dirs=True):
    """dn_occupancy_compact_emit_dirs: pts (max_points,3), row slot[p] = ro + rd * z of sample p, and, from the same launch, dirs
    (max_points,3): row slot[p] = columns 8..10 of sample p's ray row (rays (N, >= 11)); rows at or past max_points are not written.
    want_dirs=False: dn_occupancy_compact_emit - the points alone (rays (N, >= 8)), and None for the directions."""
    rays, z = f32c(rays), f32c(z)
    n, s = z.shape
    max_points = int(max_points)
    outs = [pts, dirs] if want_dirs else [pts]
    for i, t in enumerate(outs):
        if t is None:
            outs[i] = t = torch.empty((max(max_points, 0), 3), dtype=torch.float32, device=z.device)
        assert t.dtype == torch.float32 and t.shape[0] >= max_points and t.shape[1:] == (3,)
    name = "dn_occupancy_compact_emit_dirs" if want_dirs else "dn_occupancy_compact_emit"
    check(getattr(lib(), name)(ptr(rays), rays.shape[1], ptr(z), n, s, ptr(slot), max_points, *[ptr(t) if max_points > 0 else None for t in outs],
                               stream()), name)
    return outs[0], (outs[1] if want_dirs else None)


def occupancy_compact_emit(rays, z, slot, max_points, pts=None):
    """dn_occupancy_compact_emit: pts (max_points,3), row slot[p] = ro + rd * z of sample p; rows at or past max_points are not written."""
    return occupancy_compact_emit_dirs(rays, z, slot, max_points, pts, want_dirs=False)[0]


def occupancy_gather(slot, net_out, rf, ws=None, record=None):
    """dn_occupancy_gather: rf[p][3] = net_out[slot[p]][3], or the fill value (-FLT_MAX) for a culled sample; net_out (n_rows,4) or None
    (no sample kept).  ws and record (occupancy_compact_count's) given: word 2 of the record becomes the number of non-finite values."""
    n_rows = 0 if net_out is None else int(net_out.shape[0])
    assert rf.dtype == torch.float32 and rf.is_contiguous() and rf.shape[-1] == 4 and rf.numel() == 4 * slot.numel()
    check(lib().dn_occupancy_gather(ptr(slot), ptr(net_out) if n_rows else None, n_rows, slot.numel(), ptr(rf), ptr(ws), ptr(record), stream()),
          "dn_occupancy_gather")
    return rf


def occupancy_gather_rows(slot, src, dst, width, fills, ws=None, record=None):
    """dn_occupancy_gather_rows (include/dexnerf_hip_cull.h): dst[p][c] = src[slot[p]][c] for c < width where slot[p] names one of src's
    rows, else fills[c] - copies of bits.  src: (n_rows, >= width) fp32 with unit stride along a row (a column view like net_out[:, 3:]
    is read in place), or None (no sample kept).  dst: (..., >= width) fp32 of slot.numel() rows, likewise a view with unit stride along
    a row and one stride between rows; its other columns are not written.  fills: `width` numbers.  ws and record
    (occupancy_compact_count's) given: word 2 of the record becomes the number of non-finite copied values."""
    width = int(width)
    fills = [float(f) for f in fills]
    if not 1 <= width <= _hip.CULL_MAX_WIDTH or len(fills) != width:
        raise ValueError(f"occupancy_gather_rows: width must be 1 .. {_hip.CULL_MAX_WIDTH} with one fill per column, got {width} and {len(fills)} fills")
    n = slot.numel()
    rows = dst.view(n, dst.shape[-1])     # (a view or an error: never a copy the kernel would write into)
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.shape[1] >= width
    assert (rows.stride(1) == 1 or rows.shape[1] == 1) and (rows.stride(0) >= width or n == 1)
    n_rows = 0 if src is None else int(src.shape[0])
    src_stride = width
    if n_rows:
        assert src.dtype == torch.float32 and src.is_cuda and src.dim() == 2 and src.shape[1] >= width
        assert (src.stride(1) == 1 or src.shape[1] == 1) and (src.stride(0) >= width or n_rows == 1)
        src_stride = max(int(src.stride(0)), width)     # (the stride of a single row is never used)
    check(lib().dn_occupancy_gather_rows(ptr(slot), c_void_p(src.data_ptr()) if n_rows else None, src_stride, n_rows, n, width,
                                         *(fills + [0.0] * (_hip.CULL_MAX_WIDTH - width)), c_void_p(rows.data_ptr()), max(int(rows.stride(0)), width),
                                         ptr(ws), ptr(record), stream()), "dn_occupancy_gather_rows")
    return dst


# ---- a ray's near / far tightened to the occupied span of the grid (include/dexnerf_hip_span.h) -----------------------------------------
def check_ray_span_pad(pad_cells, who="ray_span_pad"):
    """The pad of a span in cells of travel: a number, finite as fp32 and >= 0 -> its fp32 value.  Raises ValueError before any GPU work."""
    try:
        pad = float(pad_cells)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the pad is a number of cells, got {pad_cells!r}") from None
    if not (math.isfinite(pad) and pad >= 0.0 and math.isfinite(ctypes.c_float(pad).value)):
        raise ValueError(f"{who}: the pad must be finite as fp32 and >= 0 cells, got {pad_cells!r}")
    return ctypes.c_float(pad).value


def occupancy_ray_spans(rays, grid, pad_cells=1.0, apply=False):
    """dn_occupancy_ray_spans of the ray rows (N, >= 8) fp32 against `grid` (bits, cells, bounds, scale: an nerf.OccupancyGrid) ->
    (span (N,2) fp32, visits (N) int32): the depth range in which the ray can meet a set cell, widened by pad_cells cells of travel and
    clipped to the row's [near, far], and the number of set cells the ray walks through; a ray that meets none keeps (near, far) and 0.
    apply=True also writes the span into columns 6 and 7 of the hit rays' rows, IN PLACE - so `rays` must then be a contiguous fp32
    device tensor (a copy would take the writes with it).  One launch, no host read."""
    pad = check_ray_span_pad(pad_cells, "occupancy_ray_spans: pad_cells")
    if not (torch.is_tensor(rays) and rays.dim() == 2 and rays.shape[1] >= 8 and rays.dtype == torch.float32):
        raise ValueError("occupancy_ray_spans: rays are fp32 rows (N, >= 8): origin, direction, near, far")
    if grid.bits.device != rays.device:
        raise ValueError(f"occupancy_ray_spans: the occupancy grid lives on {grid.bits.device} and the rays on {rays.device}; move it with grid.to(device)")
    if not rays.is_cuda:
        raise RuntimeError("occupancy_ray_spans: runs on the ROCm device only (got a host tensor); move the rays to 'cuda'")
    if apply and not rays.is_contiguous():
        raise ValueError("occupancy_ray_spans: apply=True writes the rows in place and needs contiguous rays")
    rays = rays.contiguous()
    n = rays.shape[0]
    span = torch.empty((n, 2), dtype=torch.float32, device=rays.device)
    visits = torch.empty(n, dtype=torch.int32, device=rays.device)
    if n:
        check(lib().dn_occupancy_ray_spans(ptr(rays), rays.shape[1], n, ptr(grid.bits), *grid.cells, *grid.bounds, *grid.scale, pad,
                                           int(bool(apply)), ptr(span), ptr(visits), stream()), "dn_occupancy_ray_spans")
    return span, visits


def tighten_ray_rows(rays, grid, pad):
    """The renders' use of dn_occupancy_ray_spans: columns 6 and 7 of the hit rows of `rays` (contiguous fp32 device rows the caller
    owns, a grid on their device, a pad from check_ray_span_pad) rewritten in place, no other output -> rays."""
    assert rays.dtype == torch.float32 and rays.is_contiguous() and rays.shape[1] >= 8 and grid.bits.device == rays.device
    if rays.shape[0]:
        check(lib().dn_occupancy_ray_spans(ptr(rays), rays.shape[1], rays.shape[0], ptr(grid.bits), *grid.cells, *grid.bounds, *grid.scale,
                                           pad, 1, None, None, stream()), "dn_occupancy_ray_spans")
    return rays


# ---- an occupancy grid refreshed while the networks train (include/dexnerf_hip_live.h) --------------------------------------------------
def check_live_occupancy(level, decay, dilate, who="LiveOccupancyGrid"):
    """The host-side rule of a live grid's settings: level finite as fp32 and >= 0, decay in (0, 1] as fp32, dilate 0 .. 8 ->
    (level, decay) as the Python floats of their fp32 values and dilate as an int.  Raises ValueError before any GPU work."""
    try:
        level, decay, dilate = float(level), float(decay), int(dilate)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: level and decay are numbers and dilate an integer, got {level!r}, {decay!r}, {dilate!r}") from None
    if not (math.isfinite(level) and level >= 0.0 and math.isfinite(ctypes.c_float(level).value)):
        raise ValueError(f"{who}: level must be finite as fp32 and >= 0, got {level!r}")
    d32 = ctypes.c_float(decay).value if math.isfinite(decay) else decay
    if not 0.0 < d32 <= 1.0:
        raise ValueError(f"{who}: decay must be in (0, 1] as fp32, got {decay!r}")
    if not 0 <= dilate <= _hip.OCC_MAX_DILATE:
        raise ValueError(f"{who}: dilate must be 0 .. {_hip.OCC_MAX_DILATE}, got {dilate}")
    return ctypes.c_float(level).value, d32, dilate


def occupancy_cell_sizes(bounds, cells):
    """h_a = (b1_a - b0_a) / cells_a of a checked grid: formed in float64 from the fp32 bounds and rounded to fp32 once."""
    h = tuple(ctypes.c_float((bounds[a + 3] - bounds[a]) / cells[a]).value for a in range(3))
    if not all(math.isfinite(v) and v > 0.0 for v in h):
        raise ValueError(f"occupancy: (b1 - b0) / cells must be finite and > 0 as fp32, got {h}")
    return h


def occupancy_cell_points(bounds, cells, sizes, c0, n, rng_state, pts=None):
    """dn_occupancy_cell_points: the jittered points of the cells c0 .. c0 + n - 1 -> pts (n,3) fp32, drawn from the grid's own record
    `rng_state` (int32 x 4 on the device); the call with c0 == 0 draws from the record's next iteration and makes it the current one."""
    if not (torch.is_tensor(rng_state) and rng_state.dtype == torch.int32 and rng_state.numel() == 4):
        raise ValueError("occupancy_cell_points: the rng record is an int32 tensor of 4 words")
    if not rng_state.is_cuda:
        raise RuntimeError("occupancy_cell_points: runs on the ROCm device only (got a host tensor); move the record to 'cuda'")
    c0, n = int(c0), int(n)
    if pts is None:
        pts = torch.empty((max(n, 0), 3), dtype=torch.float32, device=rng_state.device)
    assert pts.dtype == torch.float32 and pts.is_contiguous() and pts.shape == (n, 3) and pts.device == rng_state.device
    check(lib().dn_occupancy_cell_points(*cells, *bounds[:3], *sizes, c0, n, ptr(rng_state), ptr(pts), stream()), "dn_occupancy_cell_points")
    return pts


def occupancy_ema_workspace_words(cells, dilate):
    return int(lib().dn_occupancy_ema_workspace_bytes(*cells, int(dilate))) // 4


def occupancy_ema_update(columns, cells, decay, level, write_bits, dilate, ema, bits, scratch, rng_state):
    """dn_occupancy_ema_update: ema[c] = max(ema[c] * decay, the larger of the columns at c) - a cell with a non-finite value only
    decays and is set -, and with write_bits the grid's bits = dilate(non-finite || ema > level), in place.  columns: one or two 1-D
    fp32 device views of one value per cell, read in place at their stride (rows[:, 3] of dn_run_network's output)."""
    n = int(cells[0]) * int(cells[1]) * int(cells[2])
    if not 1 <= len(columns) <= 2:
        raise ValueError(f"occupancy_ema_update: one or two density columns, got {len(columns)}")
    args = []
    for t in columns:
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n):
            raise ValueError(f"occupancy_ema_update: a density column is a 1-D fp32 tensor of {n} values, one per cell")
        if not t.is_cuda:
            raise RuntimeError("occupancy_ema_update: runs on the ROCm device only (got a host tensor); move the densities to 'cuda'")
        stride = int(t.stride(0)) if n > 1 else 1
        if not 1 <= stride < 2 ** 31:
            raise ValueError(f"occupancy_ema_update: a density column needs a stride of 1 .. 2^31 - 1 floats, got {stride}")
        args += [c_void_p(t.data_ptr()), stride]
    if len(columns) == 1:
        args += [None, 0]
    dev = columns[0].device
    assert ema.dtype == torch.float32 and ema.is_contiguous() and ema.numel() == n and ema.device == dev
    assert bits.dtype == torch.int32 and bits.is_contiguous() and bits.numel() == occupancy_words(cells) and bits.device == dev
    assert scratch is None or (scratch.dtype == torch.int32 and scratch.numel() >= bits.numel() and scratch.device == dev)
    assert rng_state.dtype == torch.int32 and rng_state.numel() == 4 and rng_state.device == dev
    check(lib().dn_occupancy_ema_update(*args, *cells, decay, level, int(bool(write_bits)), int(dilate), ptr(ema), ptr(bits), ptr(scratch),
                                        ptr(rng_state), stream()), "dn_occupancy_ema_update")


# ---- the culled renders: depth, colour and normals over one pass ------------------------------------------------------------------------
class _CullStats:
    """What the passes of a culled driver report into: the kept and the total samples of pass 0 (coarse) and 1 (fine) - 0 for a pass
    that did not run - and the passes' device records in launch order."""

    def __init__(self):
        self.kept, self.total, self.records = [0, 0], [0, 0], []

    def add(self, index, n_kept, n_total, record):
        self.kept[index], self.total[index] = n_kept, n_total
        self.records.append(record)

    def result(self):
        return dict(kept=tuple(self.kept), total=tuple(self.total), records=self.records)


def _culled_call(who, packed_c, packed_f, rays, num_coarse, num_fine, lindisp, draws, colour=False):
    """The prelude of the culled drivers: the packs' inference streams fresh (refusals in `who`'s name), fp32-contiguous ray rows,
    whether a fine pass runs, the four draw tensors (_draw_tensors), the direction columns, the coarse depths, and whether a pass emits
    view directions - colour renders of networks that read them, which then need 11-column rays and both networks of one kind."""
    packed_c.require_fresh_inference_stream(who)
    rays = f32c(rays)
    fine = num_fine > 0 and packed_f is not None
    if fine:
        packed_f.require_fresh_inference_stream(who)
    dirs = colour and bool(packed_c.desc.use_viewdirs)
    if colour and (rays.shape[1] < (11 if dirs else 8) or (fine and bool(packed_f.desc.use_viewdirs) != dirs)):
        raise ValueError(f"{who}: networks with view directions need ray rows of 11 columns, and both networks the same kind")
    draws = _draw_tensors(draws)
    return rays, fine, draws, rays[:, 3:6], coarse_depths(rays, num_coarse, lindisp, draws[0]), dirs


def _network_rows(packed):
    """_culled_pass's `evaluate` of a network pass: its (n,4) rows at explicit points, one sample and one direction row per "ray"."""
    return lambda pts, dirs: run_network_pts(packed, pts, dirs, 1)


def _culled_pass(rays, z, grid, evaluate, stats, index, columns="sigma", dirs=False, count_nonfinite=False):
    """One network pass of a culled render, the only place where the sequence stands: dn_occupancy_compact_count, the host read of the
    kept count (it sizes the network launch), the emit (with a direction row per kept point when `dirs`), evaluate(pts, dirs | None) on
    the kept points - skipped when nothing is kept -, the gather with its fills.  Reports (kept, total, record) into `stats` as pass
    `index`.  columns:
      "sigma"       evaluate gives (n,4) rows; dn_occupancy_gather of their sigma, -FLT_MAX for a culled sample -> rf (N,S,4) whose sigma
                    column alone is written
      "rgb sigma"   evaluate gives (n,4) rows; dn_occupancy_gather_rows of all four, (+0, +0, +0, -FLT_MAX) for a culled sample -> rf
      "sigma grad"  evaluate gives (sigma (n,1), gradient (n,3)); dn_occupancy_gather_rows of sigma (width 1, -FLT_MAX) and of the
                    gradient (width 3, +0: dn_composite_normals' "no normal") -> (rf as for "sigma", g_pts (N,S,3))
    count_nonfinite: word 2 of the record becomes the number of non-finite gathered values - never of the gradient's."""
    slot, record, ws = occupancy_compact_count(rays, z, grid)
    n_kept = int(record[0].item())
    stats.add(index, n_kept, z.numel(), record)
    out = evaluate(*occupancy_compact_emit_dirs(rays, z, slot, n_kept, want_dirs=dirs)) if n_kept else None
    counted = (ws, record) if count_nonfinite else ()
    rf = torch.empty(tuple(z.shape) + (4,), dtype=torch.float32, device=z.device)
    if columns == "sigma":
        return occupancy_gather(slot, out, rf, *counted)
    if columns == "rgb sigma":
        return occupancy_gather_rows(slot, out, rf, 4, (0.0, 0.0, 0.0, _hip.OCC_FILL), *counted)
    sigma, g = out if n_kept else (None, None)
    g_pts = torch.empty(tuple(z.shape) + (3,), dtype=torch.float32, device=z.device)
    occupancy_gather_rows(slot, sigma, rf[..., 3:], 1, (_hip.OCC_FILL,), *counted)
    occupancy_gather_rows(slot, g, g_pts, 3, (0.0, 0.0, 0.0))
    return rf, g_pts


def render_rays_depth_culled(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, m_thres, occupancy, draws=None, quantiles=None,
                             interp=False, count_nonfinite=False, layers=None, want_width=False):
    """render_rays_depth with the network evaluated only on the samples whose occupancy cell is set, as a chain of entry points on the
    current stream: dn_coarse_depths, dn_occupancy_compact_count, a host read of the kept count, dn_occupancy_compact_emit,
    dn_run_network on the kept points (explicit points, one sample per "ray"; skipped when nothing is kept), dn_occupancy_gather
    (culled samples get -FLT_MAX: no opacity, no threshold crossing), dn_density_resample, the same compaction on the fine depths for
    the fine network, dn_composite_density or its quantile variant.  num_fine == 0 (or no fine pack) ends after a dn_composite_density
    of the coarse pass.

    Returns (render_rays_depth's maps, stats): stats = dict(kept=(coarse, fine), total=(coarse, fine), records=[the passes' device
    records]) - the fine entries 0 without a fine pass.  Two host reads per chunk (one per network pass: the kept count sizes the
    network launch) - the chain cannot be captured into a HIP graph.  The network runs in the packs' precision; an explicit-points
    launch carries no fp16 range status, so the guarded-fp16 render policy does not apply here.

    layers: an int L in 1 .. 8 - the last dn_composite_density becomes dn_composite_density_layers followed by dn_dex_layers_finish in
    sample mode, and the maps are followed by events (K,2L,N), count (K,N) int32 and width (K,2L,N) | None (want_width): a culled
    sample's -FLT_MAX is "not above".  Needs thresholds >= 0 (the caller validates them) and noise_std 0; not together with quantiles.
    None: the launches and the return are what they were."""
    if layers is not None:
        check_layers(layers, "render_rays_depth_culled: layers")
        if quantiles is not None:
            raise ValueError("render_rays_depth_culled: layers together with quantiles is not supported")
        if float(noise_std) != 0.0:
            raise ValueError("render_rays_depth_culled: the events are those of the raw density: noise_std must be 0")
        if m_thres is None or not int(m_thres.numel()):
            raise ValueError("render_rays_depth_culled: the layers need at least one Dex threshold")
    rays, fine, (_, noise_c, u, noise_f), rd, z, _ = _culled_call("render_rays_depth_culled", packed_c, packed_f, rays, num_coarse, num_fine,
                                                                   lindisp, draws)
    stats = _CullStats()
    rf = _culled_pass(rays, z, occupancy, _network_rows(packed_c), stats, 0, count_nonfinite=count_nonfinite)
    if fine:
        depth_c, acc_c, z = density_resample(rf, z, rd, num_fine, noise_c, noise_std, u)
        rf = _culled_pass(rays, z, occupancy, _network_rows(packed_f), stats, 1, count_nonfinite=count_nonfinite)
    noise = noise_f if fine else noise_c
    if layers is not None:
        depth, acc, dex, br, _, count = composite_density_layers(rf, z, rd, m_thres, layers)
        events, width = dex_layers_finish(br, m_thres, False, want_width)
        last = (depth, acc, dex, events, count, width)
    elif quantiles is None:
        last = composite_density(rf, z, rd, noise, noise_std, m_thres)
    else:
        if not 1 <= int(quantiles.numel()) <= _hip.MAX_QUANTILES or quantiles.dtype != torch.float32:
            raise ValueError(f"render_rays_depth_culled: quantiles must be a float32 device tensor of 1 .. {_hip.MAX_QUANTILES} values")
        last = composite_density_quantiles_on_device(rf, z, rd, noise, noise_std, m_thres, quantiles, interp)
    depth, acc, dex, *qdepth = last
    maps = ((depth_c, acc_c, depth, acc, dex) if fine else (depth, acc, None, None, dex)) + tuple(qdepth)
    return maps, stats.result()


def render_rays_culled(packed_c, packed_f, rays, num_coarse, num_fine, lindisp, noise_std, white, m_thres, occupancy, draws=None,
                       count_nonfinite=False):
    """render_rays with the networks evaluated only on the samples whose occupancy cell is set, as a chain of entry points on the
    current stream, per pass: dn_occupancy_compact_count, a host read of the kept count, dn_occupancy_compact_emit_dirs (the plain emit
    for a network without view directions), dn_run_network on the kept points - explicit points, one sample and one direction row per
    "ray"; skipped when nothing is kept -, dn_occupancy_gather_rows of its four columns (a culled sample gets rgb +0 and sigma -FLT_MAX:
    weight exactly 0, no threshold crossing), dn_volume_render.  dn_coarse_depths leads the coarse pass; with a fine pass the coarse one
    is composited with its weights and without thresholds, dn_fine_depths follows, then the same pass on the fine network.

    Full packs (FlexibleNeRFModel.packed).  m_thres: a list of thresholds.  Returns (render_rays' seven maps, stats): stats as
    render_rays_depth_culled's.  Two host reads per chunk; the chain cannot be captured into a HIP graph.  The network runs in the
    packs' precision; the guarded-fp16 render policy does not apply (an explicit-points launch carries no range status)."""
    rays, fine, (_, noise_c, u, noise_f), rd, z, dirs = _culled_call("render_rays_culled", packed_c, packed_f, rays, num_coarse, num_fine,
                                                                      lindisp, draws, colour=True)
    stats = _CullStats()
    thres = list(m_thres) if m_thres is not None else []
    rf = _culled_pass(rays, z, occupancy, _network_rows(packed_c), stats, 0, "rgb sigma", dirs, count_nonfinite)
    rgb_c, _, acc_c, weights, depth_c, dex = volume_render_fwd(rf, z, rd, noise_c, noise_std, white, [] if fine else thres, want_weights=fine)
    rgb_f = depth_f = acc_f = None
    if fine:
        z = fine_depths(z, weights, num_fine, u)
        rf = _culled_pass(rays, z, occupancy, _network_rows(packed_f), stats, 1, "rgb sigma", dirs, count_nonfinite)
        rgb_f, _, acc_f, _, depth_f, dex = volume_render_fwd(rf, z, rd, noise_f, noise_std, white, thres, want_weights=False)
    return (rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f, dex), stats.result()


def density_gradient_bytes_per_point(packed_density):
    """Device bytes density_gradient(pts=) holds per point: the saved tensors of the training forward, the gradient chain's buffers,
    the output rows, the seed, the points and their gradients."""
    n = 1 << 16
    return -(-sum(train_sizes(packed_density, n, prec=packed_density.precision)) // n) + 16 + 16 + 12 + 12


def _density_gradient_slabs(packed, streams, pts, max_points):
    """density_gradient on explicit points in slabs of at most max_points (None: one slab) -> (sigma (n,1), gradient (n,3)); points
    are independent, so the values do not depend on the slabs."""
    n = pts.shape[0]
    step = n if max_points is None else max(1, int(max_points))
    if n <= step:
        sigma, g = density_gradient(packed, streams, pts=pts)
        return sigma.unsqueeze(-1), g         # the .w column of the training forward's rows, read in place: row stride 4
    sigma, g = torch.empty((n, 1), dtype=torch.float32, device=pts.device), torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    for p0 in range(0, n, step):
        sigma[p0:p0 + step, 0], g[p0:p0 + step] = density_gradient(packed, streams, pts=pts[p0:p0 + step])
    return sigma, g


def render_rays_normals_culled(packed_c, packed_f, streams, rays, num_coarse, num_fine, lindisp, noise_std, m_thres, occupancy, draws=None,
                               count_nonfinite=False, max_points=None):
    """render_rays_normals with the networks evaluated only on the samples whose occupancy cell is set.  With a fine pass the coarse
    one is render_rays_depth_culled's (_culled_pass, dn_density_resample).  The last pass: count, host read, emit, density_gradient on
    the kept points (the training forward, the backward-data chain and the input gradient: the most expensive evaluation per sample
    the library has), dn_occupancy_gather_rows of its sigma (width 1, -FLT_MAX for a culled sample) and of its gradients (width 3, +0:
    a zero gradient is dn_composite_normals' "no normal"), dn_composite_normals.  max_points: the kept points are differentiated in
    slabs of at most that many (points are independent: the maps do not depend on the slabs).  Density packs and the
    DensityGradStreams of the last pass's network.  Returns (render_rays_normals' maps, stats as render_rays_depth_culled's); the count
    of non-finite values covers sigma, in both passes."""
    rays, fine, (_, noise_c, u, noise_f), rd, z, _ = _culled_call("render_rays_normals_culled", packed_c, packed_f, rays, num_coarse, num_fine,
                                                                   lindisp, draws)
    stats = _CullStats()
    depth_c = acc_c = None
    if fine:
        rf = _culled_pass(rays, z, occupancy, _network_rows(packed_c), stats, 0, count_nonfinite=count_nonfinite)
        depth_c, acc_c, z = density_resample(rf, z, rd, num_fine, noise_c, noise_std, u)
    last = packed_f if fine else packed_c
    rf, g_pts = _culled_pass(rays, z, occupancy, lambda pts, _: _density_gradient_slabs(last, streams, pts, max_points), stats,
                             1 if fine else 0, "sigma grad", count_nonfinite=count_nonfinite)
    depth, acc, dex, normal, dex_normal = composite_normals(rf, z, rd, g_pts, noise_f if fine else noise_c, noise_std, m_thres)
    return (depth_c, acc_c, depth, acc, dex, normal, dex_normal), stats.result()

