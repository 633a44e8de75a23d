"""Camera pose refinement against a trained NeRF (iNeRF-style): the chain pose -> rays -> render -> loss -> pose gradient on the
library's kernels (select_camera_rays forward / dn_camera_grad backward, predict_and_render_radiance with rows that require grad);
MultiPoseRefiner: all cameras of a capture together, on mixed-camera batches (dn_select_rays_views / dn_camera_grad_views);
FusedPoseStep: the same iteration as library launches only - twists, records, draw, render, loss, ray gradient, camera gradient,
twist gradient and Adam all on the device, replayed as one HIP graph; FusedJointStep: that iteration with the networks trained in
the same step - the packs inside the graph, the weight gradients from the same backward call, the networks' optimizer after it."""
import torch

from . import _hip, _ops
from .loss import distortion_weight_settings, exposure_settings, fused_loss_head, loss_head_settings
from .nerf_helpers import _require_device, img2mse, random_view_pixel_pairs, select_camera_rays
from .train_utils import predict_and_render_radiance


def se3_exp(xi):
    """The 4x4 rigid transform exp of the twist xi = (omega, t): torch.linalg.matrix_exp of [[omega]x, t; 0, 0].  Differentiable, and
    finite (value and gradient) at xi = 0."""
    zero = xi.new_zeros(())
    wx, wy, wz, tx, ty, tz = xi.unbind(-1)
    twist = torch.stack([torch.stack([zero, -wz, wy, tx]), torch.stack([wz, zero, -wx, ty]), torch.stack([-wy, wx, zero, tz]),
                         torch.stack([zero, zero, zero, zero])])
    return torch.linalg.matrix_exp(twist)


INTRINSICS_MODES = (None, "shared", "per_view")


def _refinement_settings(who, n_views, refine_intrinsics, intrinsics_scale, fixed_views, refine_pose=True, networks_train=False,
                         refine_exposure=None):
    """The checked (mode, scale, pose mask as a list of V 0 / 1) of FusedPoseStep / MultiPoseRefiner.  networks_train (FusedJointStep):
    the step has the networks to update, so holding every camera fixed is allowed; so it is with refine_exposure (the exposure rows are
    something refined)."""
    if refine_intrinsics not in INTRINSICS_MODES:
        raise ValueError(f"{who}: refine_intrinsics is None, 'shared' or 'per_view' (got {refine_intrinsics!r})")
    scale = float(intrinsics_scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"{who}: intrinsics_scale must be a positive finite number (got {intrinsics_scale!r})")
    fixed = [int(v) for v in fixed_views]
    if any(v < 0 or v >= n_views for v in fixed):
        raise ValueError(f"{who}: fixed_views {fixed} out of range for {n_views} views")
    if not refine_pose and refine_intrinsics is None and not networks_train and refine_exposure is None:
        raise ValueError(f"{who}: refine_pose=False with refine_intrinsics=None leaves nothing to refine")
    mask = [0 if (not refine_pose or v in fixed) else 1 for v in range(n_views)]
    return refine_intrinsics, scale, mask


def refined_intrinsics(k0, phi, scale):
    """K of the intrinsics parameterisation: fx = fx0 exp(s a), cx = cx0 + s fx0 b, cy = cy0 + s fx0 c with phi = (a, b, c) (3,) or
    (V,3) and k0 (3,3) or (V,3,3); every other entry as given.  Differentiable in phi; (V,3,3) when either is per view."""
    if phi.dim() == 2 and k0.dim() == 2:
        k0 = k0.expand(phi.shape[0], 3, 3)
    k0 = k0.to(phi.dtype)
    fx0 = k0[..., 0, 0]
    fx, cx, cy = fx0 * torch.exp(scale * phi[..., 0]), k0[..., 0, 2] + scale * fx0 * phi[..., 1], k0[..., 1, 2] + scale * fx0 * phi[..., 2]
    rows = [torch.stack([fx, k0[..., 0, 1], cx], -1), torch.stack([k0[..., 1, 0], k0[..., 1, 1], cy], -1), k0[..., 2, :].expand(fx.shape + (3,))]
    return torch.stack(rows, -2)


class PoseRefiner:
    """Refines one camera's world->camera extrinsic against an image, the networks frozen: E = se3_exp(xi) @ extrinsic0 with the
    6-vector xi (float64, on the host) under torch.optim.Adam.  Every `step` draws `num_rays` distinct pixels from the refiner's own
    seeded device generator.  `ndc_focal`: forward-facing scenes (rows warped to NDC).  All state lives in the object."""

    def __init__(self, model_coarse, model_fine, options, height, width, intrinsic, extrinsic0, encode_position_fn, encode_direction_fn,
                 num_rays, lr, seed=0, ndc_focal=None):
        _require_device(extrinsic0, "PoseRefiner")
        self.models = (model_coarse, model_fine)
        self.options = options
        self.height, self.width = int(height), int(width)
        self.device = extrinsic0.device
        self.intrinsic = intrinsic.detach().to("cpu", torch.float32)
        self.extrinsic0 = extrinsic0.detach().to("cpu", torch.float64)
        self.encoders = (encode_position_fn, encode_direction_fn)
        self.num_rays = min(int(num_rays), self.height * self.width)
        self.ndc_focal = ndc_focal
        self.xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
        self.optimizer = torch.optim.Adam([self.xi], lr=lr)
        self.last_grad = None   # dL/dxi of the latest step (Adam's step leaves xi.grad in place, zero_grad clears it)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))

    def draw_pixels(self):
        """`num_rays` distinct pixels (device int64, row-major) from the refiner's generator."""
        return torch.randperm(self.height * self.width, device=self.device, generator=self.generator)[:self.num_rays]

    def loss(self, image, pixel_index):
        """mse(rgb_coarse, target) + mse(rgb_fine, target) on the given pixels at the current xi (differentiable in xi)."""
        extrinsic = se3_exp(self.xi) @ self.extrinsic0
        near, far = float(self.options.dataset.near), float(self.options.dataset.far)
        rows, target = select_camera_rays(self.height, self.width, extrinsic, self.intrinsic, near, far, pixel_index, image=image,
                                          ndc_focal=self.ndc_focal)
        out = predict_and_render_radiance(rows, self.models[0], self.models[1], self.options, mode="train",
                                          encode_position_fn=self.encoders[0], encode_direction_fn=self.encoders[1])
        loss = img2mse(out[0], target[..., :3])
        if out[3] is not None:
            loss = loss + img2mse(out[3], target[..., :3])
        return loss

    def step(self, image, pixel_index=None):
        """One refinement step on `image` (H,W,C): draw the pixels (or take `pixel_index`), loss, backward, one Adam step on xi.
        The networks' parameters do not require grad while it runs (restored afterwards) and receive no gradient.  Returns the loss."""
        _require_device(image, "PoseRefiner.step")
        params = [p for m in self.models if m is not None for p in m.parameters()]
        flags = [p.requires_grad for p in params]
        for p in params:
            p.requires_grad_(False)
        try:
            pixels = self.draw_pixels() if pixel_index is None else pixel_index
            self.optimizer.zero_grad(set_to_none=True)
            loss = self.loss(image, pixels)
            loss.backward()
            self.last_grad = self.xi.grad.detach().clone()
            self.optimizer.step()
        finally:
            for p, flag in zip(params, flags):
                p.requires_grad_(flag)
        return loss.detach()

    def extrinsic(self):
        """The current estimate se3_exp(xi) @ extrinsic0, detached (fp32, on the refiner's device)."""
        with torch.no_grad():
            return (se3_exp(self.xi) @ self.extrinsic0).to(self.device, torch.float32)


class MultiPoseRefiner:
    """PoseRefiner for the V cameras of a capture refined together: E_v = se3_exp(xi[v]) @ extrinsics0[v], xi (V,6) float64 on the
    host under ONE torch.optim.Adam.  Every `step` draws `num_rays` distinct (view, pixel) pairs over all V H W pixels from the
    refiner's own seeded device generator, builds the mixed batch with one selection kernel (select_camera_rays with view_index) and
    reads all V camera gradients back at once.  `intrinsic`: (3,3) shared or (V,3,3).  All state lives in the object.

    `refine_intrinsics` "shared" | "per_view": phi (3,) | (V,3) float64 on the host under the same Adam, K = refined_intrinsics(intrinsic,
    phi, intrinsics_scale) handed to select_camera_rays (FusedPoseStep's parameterisation; its parity reference).  `fixed_views`: views
    whose xi gets a zero gradient."""

    def __init__(self, model_coarse, model_fine, options, height, width, intrinsic, extrinsics0, encode_position_fn, encode_direction_fn,
                 num_rays, lr, seed=0, ndc_focal=None, refine_intrinsics=None, intrinsics_scale=1.0, fixed_views=()):
        if extrinsics0.dim() != 3:
            raise ValueError("MultiPoseRefiner: extrinsics0 is (V,4,4)")
        self.mode, self.intrinsics_scale, mask = _refinement_settings("MultiPoseRefiner", int(extrinsics0.shape[0]), refine_intrinsics,
                                                                      intrinsics_scale, fixed_views)
        _require_device(extrinsics0, "MultiPoseRefiner")
        self.models = (model_coarse, model_fine)
        self.options = options
        self.height, self.width = int(height), int(width)
        self.device = extrinsics0.device
        self.n_views = int(extrinsics0.shape[0])
        self.intrinsic = intrinsic.detach().to("cpu", torch.float32)
        self.extrinsics0 = extrinsics0.detach().to("cpu", torch.float64)
        self.encoders = (encode_position_fn, encode_direction_fn)
        self.num_rays = min(int(num_rays), self.n_views * self.height * self.width)
        self.ndc_focal = ndc_focal
        self.xi = torch.zeros(self.n_views, 6, dtype=torch.float64, requires_grad=True)
        self.pose_mask = None if all(mask) else torch.tensor(mask, dtype=torch.float64)[:, None]
        self.phi = None
        if self.mode is not None:
            self.phi = torch.zeros((3,) if self.mode == "shared" else (self.n_views, 3), dtype=torch.float64, requires_grad=True)
        self.optimizer = torch.optim.Adam([self.xi] if self.phi is None else [self.xi, self.phi], lr=lr)
        self.last_grad = None   # dL/dxi (V,6) of the latest step
        self.last_grad_phi = None   # dL/dphi of the latest step
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))

    def draw_pairs(self):
        """(view_index int32, pixel_index int64): `num_rays` distinct (view, pixel) pairs from the refiner's generator."""
        return random_view_pixel_pairs(self.n_views, self.height * self.width, self.num_rays, self.device, self.generator)

    def _extrinsics(self):
        return torch.stack([se3_exp(self.xi[v]) @ self.extrinsics0[v] for v in range(self.n_views)])

    def _intrinsic(self):
        return self.intrinsic if self.phi is None else refined_intrinsics(self.intrinsic.double(), self.phi, self.intrinsics_scale)

    def loss(self, images, view_index, pixel_index):
        """mse(rgb_coarse, target) + mse(rgb_fine, target) on the given pairs at the current xi (differentiable in xi and phi)."""
        near, far = float(self.options.dataset.near), float(self.options.dataset.far)
        rows, target = select_camera_rays(self.height, self.width, self._extrinsics(), self._intrinsic(), near, far, pixel_index, image=images,
                                          ndc_focal=self.ndc_focal, view_index=view_index)
        out = predict_and_render_radiance(rows, self.models[0], self.models[1], self.options, mode="train",
                                          encode_position_fn=self.encoders[0], encode_direction_fn=self.encoders[1])
        loss = img2mse(out[0], target[..., :3])
        if out[3] is not None:
            loss = loss + img2mse(out[3], target[..., :3])
        return loss

    def step(self, images, pairs=None):
        """One refinement step on `images` (V,H,W,C): draw the pairs (or take `pairs` = (view_index, pixel_index)), loss, ONE backward,
        one Adam step on xi.  The networks' parameters do not require grad while it runs (restored afterwards) and receive no gradient.
        Returns the loss."""
        _require_device(images, "MultiPoseRefiner.step")
        params = [p for m in self.models if m is not None for p in m.parameters()]
        flags = [p.requires_grad for p in params]
        for p in params:
            p.requires_grad_(False)
        try:
            view_index, pixel_index = self.draw_pairs() if pairs is None else pairs
            self.optimizer.zero_grad(set_to_none=True)
            loss = self.loss(images, view_index, pixel_index)
            loss.backward()
            if self.pose_mask is not None:
                self.xi.grad.mul_(self.pose_mask)
            self.last_grad = self.xi.grad.detach().clone()
            if self.phi is not None:
                self.last_grad_phi = self.phi.grad.detach().clone()
            self.optimizer.step()
        finally:
            for p, flag in zip(params, flags):
                p.requires_grad_(flag)
        return loss.detach()

    def extrinsics(self):
        """The current estimates se3_exp(xi[v]) @ extrinsics0[v], (V,4,4), detached (fp32, on the refiner's device)."""
        with torch.no_grad():
            return self._extrinsics().to(self.device, torch.float32)

    def intrinsics(self):
        """The current K, (3,3) or (V,3,3) (per view when `intrinsic` or phi is), detached (fp32, on the refiner's device)."""
        with torch.no_grad():
            return self._intrinsic().to(self.device, torch.float32)


class FusedPoseStep:
    """The refinement iteration of MultiPoseRefiner with the networks frozen and nothing on the host: E_v = se3_exp(xi[v]) @
    extrinsics0[v] with xi (V,6) fp32 ON THE DEVICE under dn_adam_step.  One `step()` enqueues, on the current stream and without a
    host read,

        dn_pose_records              xi -> camera records (and the extrinsics)
        dn_select_rays_draw_views    `num_rays` distinct (view, pixel) pairs, their rows and targets (NDC rows with `ndc_focal`)
        dn_render_rays_train_geom    coarse + fine render on the cached packs; jitter, resampling u and density noise drawn in the kernels
        dn_mse2_loss                 loss3 = [loss, mse_coarse, mse_fine] and the upstream gradients
                                     (depth_images / loss_weights / depth_weights given: dn_render_loss in its place - weighted
                                     colour terms, e.g. loss_weights=(0, 1) for a fine-only refinement, plus a masked depth term
                                     on `depth_images` (V,H,W) gathered at the drawn pairs; loss6 = [loss, mse_coarse, mse_fine,
                                     D_coarse, D_fine, valid rays], loss3 its first three words)
        dn_render_rays_backward_geom the gradient of the rows, no weight gradients
        dn_camera_grad_views         -> the gradient of the records
        dn_pose_records_backward     -> the gradient of xi
        dn_adam_step                 constant `lr`, gradients cleared in the same pass

    Under nerf.set_precision('bf16' | 'bf16-s8' | 'bf16-s16') the step runs bf16 with 16-bit saved tensors (FusedNetInputFn's rule),
    under 'fp32' fp32.  The networks' parameters, their requires_grad flags and their .grad are never touched.  The first
    `eager_iterations` steps run eagerly and bring the packed streams up to date; the next one is captured into one HIP graph and
    replayed from then on (use_graphs=False: eager throughout).  If capture fails the loop goes on eagerly and `fallback_reason` says
    why.  Networks with view directions only (the selection kernels write 11-column rows), like FusedTrainStep.  `extrinsics0` (V,4,4) or (4,4), `intrinsic` (3,3) or (V,3,3), `images` (V,H,W,C), all on the device.

    loss3, xi, last_grad ((V,6): the gradient the latest step used) and rng_state are device tensors; PoseRefiner / MultiPoseRefiner
    (float64 xi on the host, explicit pixels) stay the parity reference.

    `refine_intrinsics` "shared" | "per_view": the intrinsics are refined with the poses - phi = (a, b, c) per refined camera (one for
    all views | (V,3)), fx = fx0 exp(s a), cx = cx0 + s fx0 b, cy = cy0 + s fx0 c with s = `intrinsics_scale` (the handle on phi's step
    relative to the twists': all of phi is dimensionless and of a rotation's size, so ONE dn_adam_step with one lr drives the flat
    buffer [xi (6V) | phi (3 | 3V) | pad to 4]).  dn_camera_records / dn_camera_records_backward then stand in the places of
    dn_pose_records / dn_pose_records_backward, one kernel launch each like the pair they replace: the step stays at the eight library
    calls above and its launch count does not grow in either mode (a shared phi's gradient is summed in view order inside the
    backward's one launch).  `fixed_views` (view indices) and `refine_pose=False` (every view) hold poses fixed:
    those views' twist gradients are exact zeros, which leaves their xi untouched bit for bit; either also puts the step on the new
    pair.  With all four at their defaults the step is the launches above.  phi (a device view into the flat buffer, None when the
    intrinsics are not refined), last_grad_phi, intrinsics().

    `refine_exposure` "gain" | "affine": a photometric row per view is refined with the cameras - eps[v] = [a] | [a_r, a_g, a_b, b_r,
    b_g, b_b], and a ray of view v meets its pixel as exp(s a_k) c_k (+ s b_k), s = `exposure_scale` (nerf.apply_exposure; the handle on
    the rows' step relative to the twists', as intrinsics_scale is for phi).  The flat buffer becomes [xi (6V) | phi | eps (P V) | pad to
    4] under the same ONE dn_adam_step; dn_render_loss_exposure stands in the head's place (the head and one workgroup per view that
    reduces the rows' gradient: one launch more) and a device-to-device copy of P V floats keeps last_grad_eps.
    `exposure_fixed_views` holds rows at their values (the kernel's mask: their gradients are exact zeros) - a common gain of all views
    is a gauge the networks absorb, (0,) pins it.  refine_pose=False with refine_exposure fits the appearance of (held-out) views on
    frozen networks.  eps (a device view into the flat buffer, None when the exposure is not refined), last_grad_eps, exposure().  With
    refine_exposure=None the step enqueues the launches above on the buffers above, nothing else.  Not covered: the 8-bit saved layout
    and the distortion term (the geometry route takes neither), several ranks; FusedTrainStep (fixed cameras) has no exposure rows."""

    _who = "FusedPoseStep"
    _networks_train = False       # FusedJointStep: the networks are parameters of the step too
    _other_route = "MultiPoseRefiner differentiates those"

    def __init__(self, model_coarse, model_fine, options, height, width, intrinsic, extrinsics0, images, encode_position_fn,
                 encode_direction_fn, num_rays, lr, seed=0, first_iteration=0, ndc_focal=None, use_graphs=True, eager_iterations=3,
                 depth_images=None, loss_weights=(1.0, 1.0), depth_weights=(0.0, 0.0), depth_range=(0.0, float("inf")),
                 refine_intrinsics=None, intrinsics_scale=1.0, fixed_views=(), refine_pose=True, distortion_weights=(0.0, 0.0),
                 refine_exposure=None, exposure_scale=1.0, exposure_fixed_views=()):
        who = self._who
        if max(distortion_weight_settings(who, distortion_weights)) > 0.0:
            raise ValueError(f"{who}: the geometry route takes no distortion regulariser yet (distortion_weights {tuple(distortion_weights)}): its "
                             "depth gradient is not added into the ray gradient - train with FusedTrainStep(distortion_weights=...)")
        if extrinsics0.dim() == 2:
            extrinsics0 = extrinsics0[None]
        if extrinsics0.dim() != 3 or tuple(extrinsics0.shape[1:]) != (4, 4):
            raise ValueError(f"{who}: extrinsics0 is (V,4,4) or (4,4)")
        self.n_views = int(extrinsics0.shape[0])
        if intrinsic.dim() == 3 and int(intrinsic.shape[0]) != self.n_views:
            raise ValueError(f"{who}: {self.n_views} extrinsics but {int(intrinsic.shape[0])} intrinsics")
        if images.dim() != 4 or int(images.shape[0]) != self.n_views:
            raise ValueError(f"{who}: {self.n_views} extrinsics but images of shape {tuple(images.shape)} (expected (V,H,W,C))")
        self.height, self.width = int(height), int(width)
        if tuple(images.shape[1:3]) != (self.height, self.width):
            raise ValueError(f"{who}: images of shape {tuple(images.shape)} for {self.height} x {self.width} cameras")
        self.exposure_mode, n_exp, self.exposure_scale, exposure_mask = exposure_settings(who, self.n_views, refine_exposure, exposure_scale,
                                                                                          exposure_fixed_views)
        self.mode, self.intrinsics_scale, mask = _refinement_settings(who, self.n_views, refine_intrinsics, intrinsics_scale,
                                                                      fixed_views, refine_pose, self._networks_train, self.exposure_mode)
        # None: the reference's head (dn_mse2_loss); else the settings of dn_render_loss (a zero colour weight is allowed here: fp32 or
        # 16-bit saves, no per-launch 8-bit gradient scale)
        self.head = loss_head_settings(who, depth_images, loss_weights, depth_weights, depth_range,
                                       shape=tuple(images.shape[:3]), ndc=ndc_focal is not None)
        if self._networks_train:      # a step that trains the networks refuses the ones it cannot train before it asks for a device
            self._check_networks(model_coarse, model_fine, encode_position_fn, encode_direction_fn)
        for t in (extrinsics0, intrinsic, images):
            _require_device(t, who)
        opt = options.nerf.train
        self.models = (model_coarse, model_fine)
        self.nc = int(opt.num_coarse)
        self.nf = int(opt.num_fine) if model_fine is not None else 0
        self.lindisp, self.perturb = bool(opt.lindisp), bool(opt.perturb)
        self.noise_std, self.white = float(opt.radiance_field_noise_std), bool(opt.white_background)
        self.near, self.far = float(options.dataset.near), float(options.dataset.far)
        if not self._networks_train:
            self._check_networks(model_coarse, model_fine, encode_position_fn, encode_direction_fn)
        self.luminance = False
        self.logs = (encode_position_fn.log_sampling, encode_direction_fn.log_sampling)
        dev = self.device = extrinsics0.device
        self.num_rays = min(int(num_rays), self.n_views * self.height * self.width)
        self.ndc_focal = None if ndc_focal is None else float(ndc_focal)
        self.lr = float(lr)
        self.e0 = extrinsics0.detach().to(torch.float32).contiguous()
        self.k = intrinsic.detach().to(torch.float32).contiguous()
        self.images = _hip.f32c(images.detach())
        n = 6 * self.n_views
        n_phi = {None: 0, "shared": 3, "per_view": 3 * self.n_views}[self.mode]
        n_eps = n_exp * self.n_views
        padded = (n + n_phi + n_eps + 3) // 4 * 4         # dn_adam_step works on multiples of four elements
        self._flat = torch.zeros(4, padded, dtype=torch.float32, device=dev)    # rows: xi, gradient, exp_avg, exp_avg_sq
        self.xi = self._flat[0, :n].view(self.n_views, 6)
        self._grad = self._flat[1, :n].view(self.n_views, 6)
        self.last_grad = torch.zeros(self.n_views, 6, dtype=torch.float32, device=dev)
        self.phi = self._grad_phi = self.last_grad_phi = None
        if self.mode is not None:
            shape = (3,) if self.mode == "shared" else (self.n_views, 3)
            self.phi = self._flat[0, n:n + n_phi].view(shape)
            self._grad_phi = self._flat[1, n:n + n_phi].view(shape)
            self.last_grad_phi = torch.zeros(shape, dtype=torch.float32, device=dev)
        # the exposure rows behind phi; _exposure: what fused_loss_head hands dn_render_loss_exposure (None: the heads as ever)
        self.eps = self.last_grad_eps = self._exposure = None
        if self.exposure_mode is not None:
            at = n + n_phi
            self.eps = self._flat[0, at:at + n_eps].view(self.n_views, n_exp)
            self.last_grad_eps = torch.zeros(self.n_views, n_exp, dtype=torch.float32, device=dev)
            self._exposure = dict(eps=self.eps, scale=self.exposure_scale, grad=self._flat[1, at:at + n_eps].view(self.n_views, n_exp),
                                  mask=None if all(exposure_mask) else torch.tensor(exposure_mask, dtype=torch.int32, device=dev))
        # dn_pose_records and its backward unless something of the new pair is asked for
        self.camera_pair = self.mode is not None or not all(mask)
        self.pose_mask = None if all(mask) else torch.tensor(mask, dtype=torch.int32, device=dev)
        # dn_adam_step's state record (parallel.FlatAdam): float [steps taken, ticket, last lr, -], then double [beta1^t, beta2^t, decay^t]
        self._adam_state = torch.zeros(12, dtype=torch.float32, device=dev)[:10]
        self._adam_state[4:10].view(torch.float64).fill_(1.0)
        self.rng_state = _ops.new_rng_state(seed, dev, first_iteration)
        self.cams = torch.zeros(self.n_views, 16, dtype=torch.float32, device=dev)
        self.loss3 = self.loss6 = None
        self.use_graphs, self.eager_left = bool(use_graphs), int(eager_iterations)
        self.graph = None
        self.fallback_reason = None
        self._keep = None
        self.anneal = None            # FusedJointStep(encoding_anneal=)

    def _check_networks(self, model_coarse, model_fine, encode_position_fn, encode_direction_fn):
        """Host-side: raises ValueError for networks outside the fused training kernels."""
        from ._train import train_fused_ok
        from .train_utils import _fusable
        nets = [m for m in (model_coarse, model_fine) if m is not None]
        if model_coarse is None or not all(_fusable(m, encode_position_fn, encode_direction_fn) and train_fused_ok(m) and m.use_viewdirs
                                           for m in nets):
            raise ValueError(f"{self._who}: a network outside the fused training kernels (W in {{128, 256}}, L_xyz in {{6, 10}}, view "
                             f"directions, precision fp32 / bf16); {self._other_route}")

    def _packs(self):
        """The packed networks (core stream) with their backward and input-gradient streams; brought up to date outside a capture
        only - the networks are frozen, a captured step reads the streams the eager steps left.  (A step that trains the networks
        packs every iteration, under capture too: the ensure_* calls and FlexibleNeRFModel._stale re-pack whenever the stream is
        capturing, so the graph holds the packs of the weights it runs on.)"""
        packs = []
        capturing = torch.cuda.is_current_stream_capturing() and not self._networks_train
        for m in self.models:
            if m is None:
                packs.append(None)
                continue
            if capturing:
                pk = m._packed_slot(*self.logs)
                if pk.buffers_bwd.get(pk.precision) is None or pk.buffer_ig is None:
                    raise RuntimeError("FusedPoseStep: a step was captured before an eager one had packed the networks")
            else:
                pk = m.packed(*self.logs, parts=_hip.PACK_CORE)
                _ops.ensure_backward_stream(m, pk, pk.precision)
                _ops.ensure_input_grad_stream(m, pk)
            packs.append(pk)
        return packs

    def _records(self, **kw):
        if self.camera_pair:
            return _ops.camera_records(self.xi, self.phi, self.e0, self.k, self.intrinsics_scale, self.ndc_focal, **kw)
        return _ops.pose_records(self.xi, self.e0, self.k, self.ndc_focal, **kw)

    def _clear_weight_gradients(self):
        """Before the backward: nothing to clear, the networks are frozen."""

    def _weight_gradient_views(self):
        """(views_c, views_f) the geometry backward accumulates the weight gradients into: none, the networks are frozen."""
        return None, None

    def _update(self):
        """The optimizer launches that end the iteration: Adam on [xi | phi] at a constant lr, the gradient cleared in the same pass."""
        _ops.adam_step(self._flat[0], self._flat[1], self._flat[2], self._flat[3], self._adam_state, self.lr, 1.0, (0.9, 0.999), 1e-8, True)

    def _enqueue(self):
        if self.anneal is not None:       # the table of this iteration (rng_state's counter, read on the device) before any pack
            self.anneal.advance(self.rng_state)
        pc, pf = self._packs()
        self._records(cams=self.cams)
        rays, target, pix, views = _ops.select_rays_draw_views(self.height, self.width, self.cams, self.near, self.far, self.rng_state,
                                                               self.num_rays, self.images, want_pixels=True, ndc_focal=self.ndc_focal,
                                                               ndc_near=1.0)
        maps, saved = _ops.render_rays_train_geom(pc, pf, rays, self.nc, self.nf, self.lindisp, self.noise_std, self.white, [], None,
                                                  prec=pc.precision, rng_state=self.rng_state, perturb=self.perturb)
        self.loss3, self.loss6, g_c, g_f = fused_loss_head(self.head, maps, target, self.rng_state, self.luminance, pix, views,
                                                           exposure=self._exposure)
        if self._exposure is not None:    # dn_adam_step clears the gradient row: the rows' gradient of this step, kept
            self.last_grad_eps.copy_(self._exposure["grad"])
        self._clear_weight_gradients()
        w_views = self._weight_gradient_views()
        d_rays, keep = _ops.render_rays_backward_geom(pc, pf, saved, g_c, g_f, *w_views)
        if self.anneal is not None:       # dL/dW = (dL/dW_eff) diag(a): the bucket holds this backward's contribution only
            self.anneal.scale_grads_pair(self.models[0], w_views[0], self.models[1], w_views[1])
        g_cams = _ops.camera_grad_views(self.height, self.width, self.cams, views, pix, self.num_rays, d_rays[:, 0:3], d_rays[:, 3:6],
                                        d_rays[:, 8:11], self.ndc_focal or 0.0, 1.0)
        if self.camera_pair:
            _ops.camera_records_backward(g_cams, self.xi, self.phi, self.e0, self.k, self.intrinsics_scale, self.pose_mask, out=self._grad,
                                         keep=self.last_grad, out_phi=self._grad_phi, keep_phi=self.last_grad_phi,
                                         want_phi=self.phi is not None)
        else:
            _ops.pose_records_backward(g_cams, self.xi, self.e0, out=self._grad, keep=self.last_grad)
        self._update()
        # alive until the next call (stream-ordered allocator; under capture they belong to the graph's pool)
        self._keep = (views, pix, rays, target, maps, saved, d_rays, g_cams, keep, g_c[0], g_f[0], g_c[1], g_f[1])

    def step(self):
        """One refinement iteration.  Returns loss3 (device, [loss, mse_coarse, mse_fine]); nothing is read back."""
        if torch.cuda.is_current_stream_capturing():      # inside the caller's own capture: the launches go into that graph
            self._enqueue()
            return self.loss3
        if self.graph is not None:
            self.graph.replay()
            return self.loss3
        if self.eager_left > 0 or not self.use_graphs:
            self.eager_left -= 1
            self._enqueue()
            return self.loss3
        try:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):    # a capture only records ...
                self._enqueue()
            self.graph = graph
        except Exception as exc:  # noqa: BLE001
            self.graph, self.use_graphs = None, False
            self.fallback_reason = f"{type(exc).__name__}: {exc}"
            torch.cuda.synchronize()
            self._enqueue()
            return self.loss3
        self.graph.replay()                                                     # ... this iteration's step runs here
        return self.loss3

    def latest_draw(self):
        """(view_index (N) int32, pixel_index (N) int64, rows (N,11), target (N,3)) of the latest step, device tensors kept alive until the
        next eager step (a replayed graph rewrites them in place) - for tests."""
        return self._keep[:4]

    def extrinsics(self):
        """The current estimates se3_exp(xi[v]) @ extrinsics0[v], (V,4,4) fp32 on the device (dn_pose_records at the current xi)."""
        return self._records(want_extrinsics=True)[1]

    def intrinsics(self):
        """The current K on the device (fp32): `intrinsic` with [0,0], [0,2], [1,2] replaced by the records' fx, cx, cy, every other entry
        as given; (3,3) when `intrinsic` is and the views share phi (or none is refined), else (V,3,3)."""
        cams = self._records()
        per_view = self.k.dim() == 3 or self.mode == "per_view"
        out = (self.k if self.k.dim() == 3 else self.k.expand(self.n_views, 3, 3)).clone()
        out[:, 0, 0], out[:, 0, 2], out[:, 1, 2] = cams[:, 12], cams[:, 13], cams[:, 14]
        return out if per_view else out[0]

    def exposure(self):
        """The current exposure rows, (V,P) fp32 on the device (a copy; row v with nerf.apply_exposure(rgb, row, refine_exposure,
        exposure_scale) shows a render as view v saw it); None when the exposure is not refined."""
        return None if self.eps is None else self.eps.detach().clone()


class FusedJointStep(FusedPoseStep):
    """The training iteration with the cameras as parameters beside the networks: FusedPoseStep's launches with the networks NOT
    frozen.  One `step()` enqueues, on the current stream and without a host read,

        dn_pose_records | dn_camera_records          [xi | phi] -> camera records (FusedPoseStep's choice rule: camera_pair)
        dn_select_rays_draw_views                    `num_rays` distinct (view, pixel) pairs, rows, targets (NDC rows with `ndc_focal`)
        the packs of BOTH networks, every iteration  core stream, backward stream, input-gradient stream (three launches per network;
                                                     a captured step holds them: it trains the weights it packs)
        dn_render_rays_train_geom                    coarse + fine render; draws made in the kernels
        dn_mse2_loss | dn_render_loss                FusedPoseStep's head (depth_images / loss_weights / depth_weights), `luminance`
        dn_render_rays_backward_geom                 with views_c / views_f: the ray gradient AND the weight gradients of both networks,
                                                     accumulated into the FlatGradBucket (one pair launch when the two networks share a
                                                     shape, one launch per network when they do not)
        dn_camera_grad_views, dn_pose_records_backward | dn_camera_records_backward    -> the gradient of [xi | phi]
        dn_adam_step on [xi | phi]                   `lr_pose`, times pose_lr_decay[0] ** (t / pose_lr_decay[1]) when given
        optimizer.step()                             the networks' own optimizer: nerf.FlatAdam on `bucket` (dn_adam_step) with its own
                                                     learning rate and schedule

    Both Adam steps come after both gradients: the two gradients are taken at the same iterate.  `bucket` (parallel.FlatGradBucket over
    the two networks) and `optimizer` as GraphedTrainStep takes them: with FlatAdam(zero_grads=True) every step ends with the bucket
    cleared, otherwise the step clears it (one memset) before the backward.  A parameter whose .grad is no longer the bucket's view
    raises.  Precision: 'fp32' runs fp32; 'bf16', 'bf16-s8' and 'bf16-s16' run bf16 with 16-bit saved tensors (FusedPoseStep's rule -
    the geometry entry points refuse the 8-bit saved layout).  Networks: the fused training kernels' set with view directions, a fine
    network required; coarse and fine need not share a shape.  One rank only.

    The first `eager_iterations` steps run eagerly (they create the pack buffers; the optimizers' moments exist from construction);
    the next one is captured into one HIP graph and replayed from then on; nerf.models.mark_parameters_updated() follows every step,
    so a later render packs the trained weights.  If capture fails the loop goes on eagerly and `fallback_reason` says why.

    `encoding_anneal` (nerf.EncodingAnneal): the coarse-to-fine schedule of the encoding's bands (BARF), attached to both networks -
    dn_encoding_anneal_amplitudes from rng_state's counter ahead of the packs, a dn_encoding_anneal_scale_weights per network ahead of its
    core and input-gradient packs, one dn_encoding_anneal_scale_grads_pair behind the backward; all inside the captured step.

    Gauge: with every view free the scene can drift by a rigid motion (and, with the intrinsics free, a scale) that the loss does not
    see.  The step does not remove it; `fixed_views=(0,)` pins it to the first camera.  refine_pose=False with refine_intrinsics=None
    is allowed here (the networks alone are trained, on the step's own mixed-view draws).

    `refine_exposure` / `exposure_scale` / `exposure_fixed_views`: FusedPoseStep's per-view exposure rows, trained with the cameras and
    the networks - [xi | phi | eps] under the one dn_adam_step at `lr_pose`, dn_render_loss_exposure in the head's place.  A view that is
    brighter than its neighbours is then explained by its row, not by view-dependent colour or haze in front of its camera.  Same limits:
    one rank, no 8-bit saved layout, no distortion term.

    state_dict() / load_state_dict(): [xi | phi | eps], the two Adam moments and dn_adam_step's state record (with refine_exposure its
    mode and scale too; a state without them is one without exposure rows, and a mismatch raises like refine_intrinsics'); with the
    networks', the optimizer's state and first_iteration = the number of steps taken, a fresh step continues the run."""

    _who = "FusedJointStep"
    _networks_train = True
    _other_route = "MultiPoseRefiner + autograd (loss.backward() through its loss, torch.optim over the networks) trains those"

    def __init__(self, model_coarse, model_fine, options, height, width, intrinsic, extrinsics0, images, encode_position_fn,
                 encode_direction_fn, num_rays, bucket, optimizer, lr_pose, pose_lr_decay=None, luminance=False, encoding_anneal=None, **kw):
        from .parallel import world_info
        if pose_lr_decay is not None:
            factor, steps = float(pose_lr_decay[0]), float(pose_lr_decay[1])
            if not (0.0 < factor < float("inf") and 0.0 < steps < float("inf")):
                raise ValueError(f"FusedJointStep: pose_lr_decay is (factor > 0, steps > 0) (got {pose_lr_decay!r})")
        if not float(lr_pose) >= 0.0:
            raise ValueError(f"FusedJointStep: lr_pose must be >= 0 (got {lr_pose!r})")
        if world_info()[1] > 1:
            raise ValueError("FusedJointStep: one rank only (multi-GPU joint training is not supported)")
        super().__init__(model_coarse, model_fine, options, height, width, intrinsic, extrinsics0, images, encode_position_fn,
                         encode_direction_fn, num_rays, lr_pose, **kw)
        if self.nf <= 0:
            raise ValueError("FusedJointStep: num_fine must be > 0 (the step trains a coarse and a fine network)")
        sinks = [getattr(m, "_grad_sink", None) for m in self.models]
        if any(s is None or s.bucket is not bucket for s in sinks):
            raise ValueError("FusedJointStep: `bucket` is the parallel.FlatGradBucket built over both networks")
        self.bucket, self.opt = bucket, optimizer
        self.luminance = bool(luminance)
        self.lr_decay_per_step = 1.0 if pose_lr_decay is None else factor ** (1.0 / steps)
        self.zero_in_step = not getattr(optimizer, "zero_grads", False)
        if not self.zero_in_step:
            bucket.flat.zero_()         # every step ends with the bucket cleared
        self.anneal = encoding_anneal
        if encoding_anneal is not None:
            encoding_anneal.attach(model_coarse, model_fine)

    def _check_networks(self, model_coarse, model_fine, encode_position_fn, encode_direction_fn):
        if model_fine is None:
            raise ValueError(f"FusedJointStep: a fine network is required; {self._other_route}")
        super()._check_networks(model_coarse, model_fine, encode_position_fn, encode_direction_fn)

    def _clear_weight_gradients(self):
        """The backward accumulates: one memset of the bucket, unless the optimizer leaves it cleared (FlatAdam(zero_grads=True))."""
        if self.zero_in_step:
            self.bucket.flat.zero_()

    def _weight_gradient_views(self):
        mc, mf = self.models
        views_c, views_f = mc._grad_sink.views(mc), mf._grad_sink.views(mf)
        if views_c is None or views_f is None:
            raise RuntimeError("FusedJointStep: a parameter's .grad is no longer the FlatGradBucket's view")
        return views_c, views_f

    def _update(self):
        _ops.adam_step(self._flat[0], self._flat[1], self._flat[2], self._flat[3], self._adam_state, self.lr, self.lr_decay_per_step,
                       (0.9, 0.999), 1e-8, True)
        self.opt.step()

    def step(self):
        """One training iteration.  Returns loss3 (device, [loss, mse_coarse, mse_fine]); nothing is read back."""
        from .models import mark_parameters_updated
        loss3 = super().step()
        mark_parameters_updated()      # a replayed optimizer step ran no Python hook
        return loss3

    def state_dict(self):
        """The camera half of the run: the flat buffer's rows [xi | phi | pad], exp_avg and exp_avg_sq, and dn_adam_step's state record
        (raw words: the step count and the running products), as independent tensors."""
        state = dict(params=self._flat[0].detach().clone(), exp_avg=self._flat[2].detach().clone(), exp_avg_sq=self._flat[3].detach().clone(),
                     adam_state=self._adam_state.detach().clone(), n_views=self.n_views, refine_intrinsics=self.mode)
        if self.exposure_mode is not None:      # (a state without the two keys: no exposure rows in the flat buffer)
            state.update(refine_exposure=self.exposure_mode, exposure_scale=self.exposure_scale)
        return state

    def load_state_dict(self, state):
        exposure = (state.get("refine_exposure"), float(state.get("exposure_scale", 1.0)) if state.get("refine_exposure") is not None else None)
        mine = (self.exposure_mode, self.exposure_scale if self.exposure_mode is not None else None)
        if int(state["n_views"]) != self.n_views or state["refine_intrinsics"] != self.mode or exposure != mine \
                or tuple(state["params"].shape) != tuple(self._flat[0].shape):
            raise ValueError(f"FusedJointStep.load_state_dict: a state of {state['n_views']} views, refine_intrinsics="
                             f"{state['refine_intrinsics']!r}, refine_exposure={exposure[0]!r} (scale {exposure[1]}) for a step of "
                             f"{self.n_views} views, refine_intrinsics={self.mode!r}, refine_exposure={mine[0]!r} (scale {mine[1]})")
        self._flat[0].copy_(state["params"])
        self._flat[1].zero_()
        self._flat[2].copy_(state["exp_avg"])
        self._flat[3].copy_(state["exp_avg_sq"])
        self._adam_state.copy_(state["adam_state"])
