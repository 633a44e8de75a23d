"""Camera pose refinement against a trained NeRF (iNeRF-style): the chain pose -> rays -> render -> loss -> pose gradient on the
library's kernels (select_camera_rays forward / dn_camera_grad backward, predict_and_render_radiance with rows that require grad);
MultiPoseRefiner: all cameras of a capture together, on mixed-camera batches (dn_select_rays_views / dn_camera_grad_views)."""
import torch

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
    reads all V camera gradients back at once.  `intrinsic`: (3,3) shared or (V,3,3).  All state lives in the object."""

    def __init__(self, model_coarse, model_fine, options, height, width, intrinsic, extrinsics0, encode_position_fn, encode_direction_fn,
                 num_rays, lr, seed=0, ndc_focal=None):
        _require_device(extrinsics0, "MultiPoseRefiner")
        if extrinsics0.dim() != 3:
            raise ValueError("MultiPoseRefiner: extrinsics0 is (V,4,4)")
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
        self.optimizer = torch.optim.Adam([self.xi], lr=lr)
        self.last_grad = None   # dL/dxi (V,6) of the latest step
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))

    def draw_pairs(self):
        """(view_index int32, pixel_index int64): `num_rays` distinct (view, pixel) pairs from the refiner's generator."""
        return random_view_pixel_pairs(self.n_views, self.height * self.width, self.num_rays, self.device, self.generator)

    def _extrinsics(self):
        return torch.stack([se3_exp(self.xi[v]) @ self.extrinsics0[v] for v in range(self.n_views)])

    def loss(self, images, view_index, pixel_index):
        """mse(rgb_coarse, target) + mse(rgb_fine, target) on the given pairs at the current xi (differentiable in xi)."""
        near, far = float(self.options.dataset.near), float(self.options.dataset.far)
        rows, target = select_camera_rays(self.height, self.width, self._extrinsics(), self.intrinsic, near, far, pixel_index, image=images,
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
            self.last_grad = self.xi.grad.detach().clone()
            self.optimizer.step()
        finally:
            for p, flag in zip(params, flags):
                p.requires_grad_(flag)
        return loss.detach()

    def extrinsics(self):
        """The current estimates se3_exp(xi[v]) @ extrinsics0[v], (V,4,4), detached (fp32, on the refiner's device)."""
        with torch.no_grad():
            return self._extrinsics().to(self.device, torch.float32)
