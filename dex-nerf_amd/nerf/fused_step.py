"""The training iteration of the Dex-NeRF loop (reference train_dexnerf_rgb.py:223-289: view and pixel draw -> ray rows -> coarse +
fine render -> mse + mse -> backward -> Adam) with nothing in it but this library's kernels - 16 launches on the as-shipped nets:

    dn_select_rays_draw      view + pixels drawn without replacement on the device, packed ray rows, target pixels   (1 kernel)
                             (draw_view="rays": dn_select_rays_draw_views - every ray's view drawn with its pixel, a batch
                             across all training images)
                             (forward-facing captures, no_ndc: False: dn_select_rays_draw_ndc - the rows warped to NDC in the
                             same kernel, near plane 1, as run_one_iter_of_nerf does)
    dn_mlp_pack_train_pair   both weight streams of both networks                                                     (2 kernels)
    dn_render_rays_train     coarse depths / net / composite, resampling, fine net / composite; the jitter, the resampling u and
                             the density noise drawn inside the kernels that consume them                             (6 kernels)
    dn_mse2_loss             loss, both MSEs and the two upstream gradients                                            (1 kernel)
                             (depth_images / loss_weights / depth_weights given: dn_render_loss in its place - weighted colour terms
                             plus a masked depth term whose targets it gathers from the depth maps at the drawn (view, pixel)
                             pairs, and the upstream gradients of the depth maps as well)
    dn_render_rays_backward  composite backward + backward-data chain per network, then ONE weight-gradient launch for the
                             layers of both (one rank; with several ranks the networks are done one at a time so that the
                             fine network's all-reduce overlaps the coarse half)                                       (5 kernels)
                             (distortion_weights given: dn_render_rays_backward_reg in its place - per network with a non-zero
                             weight the distortion regulariser of its sample weights, dn_distortion_loss, ahead of the compositing
                             backward, which takes its gradient as the upstream of every sample weight: 2 kernels, and for the
                             fine network one more compositing launch that forms the weights again)
    dn_adam_step             nerf.FlatAdam: step, learning-rate schedule and gradient clearing                         (1 kernel)

encoding_anneal (nerf.EncodingAnneal) given: three launches more on one rank in the default 'bf16' mode - dn_encoding_anneal_amplitudes
ahead of everything, dn_encoding_anneal_scale_weights_pair ahead of the pack, dn_encoding_anneal_scale_grads_pair behind the backward
(the per-network packs and the two halves of a data-parallel step: one dn_encoding_anneal_scale_weights / _scale_grads per network).

ray_span (an nerf.OccupancyGrid or an nerf.LiveOccupancyGrid) given: one launch more, dn_occupancy_ray_spans right after the draw - every
row's near / far tightened to its occupied span of the grid -, and with a live grid its refresh (LiveOccupancyGrid.update) before every
occupancy_update_every-th iteration, outside the replayed graph (refresh_occupancy(), called by GraphedTrainStep.step).

Per-view exposure rows (refine_exposure=, dn_render_loss_exposure) belong to the steps that own the cameras, nerf.FusedPoseStep /
nerf.FusedJointStep; this step trains on fixed cameras and has none.

The networks: W in {128, 256} with L_xyz in {6, 10} (the shipped fern / LLFF nets are 4 x 128, L_xyz = 6), view directions.
No autograd graph, no ATen elementwise / reduction / RNG launches (profiles/r03_as_shipped_kernel_summary.md).  The gradients land in
a parallel.FlatGradBucket (the `.grad` tensors of the parameters).  GraphedTrainStep replays the iteration as HIP graphs (three
around the exchange when world > 1).  The explicit-draw path (predict_and_render_radiance under autograd, draws as tensors) stays
what the parity tests drive."""
import torch

from . import _ops
from ._train import train_fused_ok
from .loss import distortion_weight_settings, fused_loss_head, loss_head_settings
from .occupancy import LiveOccupancyGrid, OccupancyGrid
from .train_utils import _fusable


class FusedTrainStep:
    def __init__(self, model_coarse, model_fine, selector, options, bucket, encode_position_fn, encode_direction_fn, num_rays, seed=0,
                 luminance=False, first_iteration=0, draw_view=False, ndc_focal=None, depth_images=None, loss_weights=(1.0, 1.0),
                 depth_weights=(0.0, 0.0), depth_range=(0.0, float("inf")), distortion_weights=(0.0, 0.0), encoding_anneal=None,
                 ray_span=None, ray_span_pad=1.0, occupancy_update_every=16):
        if not (isinstance(draw_view, bool) or draw_view == "rays"):
            raise ValueError(f"FusedTrainStep: draw_view must be False, True or \"rays\" (got {draw_view!r})")
        # the distortion regulariser of each network's sample weights (dn_render_rays_backward_reg); (0, 0): the backward as ever
        self.distortion_weights = distortion_weight_settings("FusedTrainStep", distortion_weights)
        opt = options.nerf.train
        self.ndc = getattr(options.dataset, "no_ndc", True) is False
        if depth_images is not None and draw_view is True:
            raise ValueError("FusedTrainStep: depth_images need the view of every ray (draw_view=False or \"rays\"); with "
                             "draw_view=True the view is drawn inside the selection kernel and not returned")
        shape = None if depth_images is None else (selector.cams.shape[0], selector.height, selector.width)
        # None: the reference's head (dn_mse2_loss); else the settings of dn_render_loss.  Both colour weights must be > 0 here: the
        # default 8-bit mode scales its saved gradients per launch from the largest upstream gradient
        self.head = loss_head_settings("FusedTrainStep", depth_images, loss_weights, depth_weights, depth_range, shape=shape, ndc=self.ndc,
                                       colour_weights_positive=True)
        if self.ndc and ndc_focal is None:
            raise ValueError("FusedTrainStep: NDC rays (dataset.no_ndc: False) need the capture's focal length (ndc_focal)")
        self.ndc_focal = float(ndc_focal) if self.ndc else None
        self.models = (model_coarse, model_fine)
        self.selector, self.bucket = selector, bucket
        self.num_rays = int(num_rays)
        self.nc, self.nf = int(opt.num_coarse), int(opt.num_fine)
        self.lindisp, self.perturb = bool(opt.lindisp), bool(opt.perturb)
        self.noise_std, self.white = float(opt.radiance_field_noise_std), bool(opt.white_background)
        self.luminance = bool(luminance)
        self.logs = (encode_position_fn.log_sampling, encode_direction_fn.log_sampling if model_coarse.use_viewdirs else True)
        if not self.applicable(model_coarse, model_fine, options, encode_position_fn, encode_direction_fn, num_rays, ndc_focal):
            raise ValueError("FusedTrainStep: configuration outside the fused training kernels (see FusedTrainStep.applicable)")
        dev = next(model_coarse.parameters()).device
        # ray_span: an nerf.OccupancyGrid, or an nerf.LiveOccupancyGrid that refresh_occupancy() keeps up to date - every drawn row's
        # near / far is tightened to its occupied span right after the draw (dn_occupancy_ray_spans: one launch, no host read).  The rows
        # are in the networks' input space there - NDC space with ndc_focal -, which is where a grid lives.  None: the launches as ever
        self.live = ray_span if isinstance(ray_span, LiveOccupancyGrid) else None
        self.span_grid = ray_span.grid if self.live is not None else ray_span
        self.span_pad = None
        self.update_every = int(occupancy_update_every)
        if ray_span is not None:
            if not isinstance(self.span_grid, OccupancyGrid):
                raise ValueError(f"FusedTrainStep: ray_span is an nerf.OccupancyGrid or an nerf.LiveOccupancyGrid, got {type(ray_span).__name__}")
            self.span_pad = _ops.check_ray_span_pad(ray_span_pad, "FusedTrainStep: ray_span_pad")
            if self.update_every < 1:
                raise ValueError(f"FusedTrainStep: occupancy_update_every must be >= 1, got {occupancy_update_every}")
            self.span_grid.check_render(dev, "FusedTrainStep")
            if self.live is not None and encoding_anneal is not None:
                raise ValueError("FusedTrainStep: a LiveOccupancyGrid reads the networks' density without the encoding anneal's band "
                                 "amplitudes; give one of the two")
        self.encode_position_fn = encode_position_fn
        self.iteration = int(first_iteration)      # host side: the iteration the next refresh_occupancy() stands before
        self.rng_state = _ops.new_rng_state(seed, dev, first_iteration)
        # [mean L_ray coarse, mean L_ray fine] of the latest step (a network with weight 0: 0); None without the regulariser.  Not part
        # of loss3 / loss6, which keep their meaning: the step minimises loss3[0] + w_c reg2[0] + w_f reg2[1]
        self.reg2 = torch.zeros(2, dtype=torch.float32, device=dev) if max(self.distortion_weights) > 0.0 else None
        self.loss3 = self.loss6 = None       # loss6 (general head only) = [loss, mse_c, mse_f, D_c, D_f, valid rays]; loss3 its first three
        # True: the iteration's training view is drawn in the kernel too (else: selector.view); "rays": the view of EVERY ray is drawn
        # with its pixel, a batch across all training images (dn_select_rays_draw_views)
        self.draw_view = draw_view
        self.zero_in_step = True     # False: the optimizer leaves the gradient bucket cleared (FlatAdam(zero_grads=True))
        # nerf.EncodingAnneal: the coarse-to-fine schedule of the encoding's bands, attached to both networks here.  Once per iteration,
        # before any pack, its table is formed on the device from rng_state's iteration counter (a replayed graph follows it); each
        # network's weight gradients get the bands' column scale right after the backward that forms them (before the exchange)
        self.anneal = encoding_anneal
        if encoding_anneal is not None:
            encoding_anneal.attach(model_coarse, model_fine)

    @staticmethod
    def applicable(model_coarse, model_fine, options, encode_position_fn, encode_direction_fn, num_rays, ndc_focal=None):
        """Both networks on the fused training kernels, a fine pass, one ray chunk; world-space rays, or NDC rays when the focal
        length of the capture is given."""
        opt = options.nerf.train
        return (model_fine is not None and int(opt.num_fine) > 0 and int(num_rays) <= int(opt.chunksize)
                and (getattr(options.dataset, "no_ndc", True) is not False or ndc_focal is not None)
                and _fusable(model_coarse, encode_position_fn, encode_direction_fn) and _fusable(model_fine, encode_position_fn, encode_direction_fn)
                and train_fused_ok(model_coarse) and train_fused_ok(model_fine) and model_coarse.use_viewdirs and model_fine.use_viewdirs)

    def forward_backward(self):
        """One iteration up to (and excluding) the end of the gradient exchange and the optimizer step.  Returns the device tensor
        [loss, mse_coarse, mse_fine]; the parameter gradients are in the bucket (world > 1: each network's all-reduce is started the
        moment its backward is enqueued - FlatGradBucket.segment_ready - and finished by bucket.all_reduce_mean())."""
        from .parallel import world_info
        mc, mf = self.models
        mc._grad_sink.forward_issued(); mf._grad_sink.forward_issued()
        if self.zero_in_step:
            self.bucket.zero()
        if world_info()[1] == 1:
            self.forward_and_fine_backward(_zero=False, both=True)    # one rank: nothing to overlap, one weight-gradient launch for both networks
            mf._grad_sink.backward_done(); mc._grad_sink.backward_done()
            return self.loss3
        self.forward_and_fine_backward(_zero=False)
        mf._grad_sink.backward_done()     # (world > 1: the fine network's all-reduce starts here, under the coarse half)
        self.coarse_backward()
        mc._grad_sink.backward_done()
        return self.loss3

    # The two halves a data-parallel loop replays as separate HIP graphs around the fine network's exchange (GraphedTrainStep): only
    # this library's launches and one memset - no bucket bookkeeping, no collective.
    def forward_and_fine_backward(self, _zero=True, both=False):
        """both=True: the coarse network's backward too, in the same call - dn_render_rays_backward then forms the weight gradients
        of both networks in ONE launch (dn_mlp_weight_grad_pair); coarse_backward() must not follow."""
        mc, mf = self.models
        sel = self.selector
        if self.anneal is not None:
            self.anneal.advance(self.rng_state)
        gather = self.head is not None and self.head["depth_images"] is not None
        # the draw: every ray's view with its pixel ("rays"), or pixels of one view - the selector's, or one drawn in the kernel;
        # the drawn (pixel, view) come back only when the depth targets are gathered at them
        by_ray = self.draw_view == "rays"
        draw = _ops.select_rays_draw_views if by_ray else _ops.select_rays_draw
        view = () if by_ray else (None if self.draw_view else sel.view,)
        rays, target, *drawn = draw(sel.height, sel.width, sel.cams, *view, sel.near, sel.far, self.rng_state, self.num_rays, sel.images,
                                    want_pixels=gather, ndc_focal=self.ndc_focal, ndc_near=1.0)
        pix, views = (drawn + [None, None])[:2]
        if self.span_grid is not None:
            _ops.tighten_ray_rows(rays, self.span_grid, self.span_pad)
        pc, pf, prec = _ops.pack_train_pair(mc, mf, self.logs)
        maps, saved = _ops.render_rays_train(pc, pf, rays, self.nc, self.nf, self.lindisp, self.noise_std, self.white, [], None, prec=prec,
                                             rng_state=self.rng_state, perturb=self.perturb)
        self.loss3, self.loss6, g_c, g_f = fused_loss_head(self.head, maps, target, self.rng_state, self.luminance, pix, views, sel.view)
        if _zero and self.zero_in_step:
            self.bucket.flat.zero_()
        views_c, views_f = mc._grad_sink.views(mc), mf._grad_sink.views(mf)
        if views_c is None or views_f is None:
            raise RuntimeError("FusedTrainStep: a parameter's .grad is no longer the FlatGradBucket's view")
        self._reg = None if self.reg2 is None else (self.distortion_weights, self.reg2)
        keep = [_ops.render_rays_backward(pc, pf, saved, g_c if both else (None, None, None), g_f, views_c, views_f, nets=3 if both else 2,
                                          reg=self._reg)]
        if self.anneal is not None and both:
            self.anneal.scale_grads_pair(mc, views_c, mf, views_f)
        elif self.anneal is not None:
            self.anneal.scale_grads(mf, views_f)
        self._half = (pc, pf, saved, g_c, views_c, views_f)
        self._keep = (keep, saved, maps, rays, target, g_c[0], g_f[0], pix, views, g_c[1], g_f[1])   # alive until the next call (stream-ordered allocator)

    def coarse_backward(self):
        pc, pf, saved, g_c, views_c, views_f = self._half
        self._keep[0].append(_ops.render_rays_backward(pc, pf, saved, g_c, (None, None, None), views_c, views_f, nets=1, reg=self._reg))
        if self.anneal is not None:
            self.anneal.scale_grads(self.models[0], views_c)

    def refresh_occupancy(self):
        """Call once before every iteration (GraphedTrainStep.step does): with a LiveOccupancyGrid, refreshes it from both networks'
        density before iteration i whenever i % occupancy_update_every == 0, i counted on the host from first_iteration.  Ordinary
        launches on the current stream, never part of a captured step: eager and replayed loops refresh at the same iterations."""
        if self.live is not None and self.iteration % self.update_every == 0:
            self.live.update(list(self.models), self.encode_position_fn)
        self.iteration += 1

    def latest_draw(self):
        """(view_index (N) int32 | None, pixel_index (N) int64 | None, rows, target) of the latest step - the pairs only with
        depth_images (the default head never asks the draw for them) - device tensors kept alive until the next eager step (a replayed
        graph rewrites them in place); for tests."""
        return self._keep[8], self._keep[7], self._keep[3], self._keep[4]


class GraphedTrainStep:
    """A FusedTrainStep + the gradient exchange + the optimizer step, replayed as HIP graphs (reference loop:
    train_dexnerf_rgb.py:229-289 - one optimizer step per drawn batch).

    world == 1: ONE graph (draw .. Adam).  world > 1: the collective stays outside the graphs -

        graph A  pixel draw, ray rows, coarse + fine render, loss head, fine network's backward
        all-reduce of the fine segment, asynchronous on torch.distributed's stream ..........  overlapped with
        graph B  coarse network's backward
        all-reduce of the coarse segment; both waited for on the compute stream
        graph C  optimizer step (fused Adam over the flat parameter list)

    RCCL averages inside the collective (ReduceOp.AVG); gloo (CPU tests, one-GPU rehearsals) sums and one division follows.
    The first `eager_iterations` calls run eagerly (they initialise the optimizer moments and the packed weight streams); the next
    one captures and replays.  If capture fails the loop goes on eagerly and `fallback_reason` says why."""

    def __init__(self, fused, optimizer, eager_iterations=3, use_graphs=True):
        self.fused, self.opt, self.bucket = fused, optimizer, fused.bucket
        if getattr(optimizer, "zero_grads", False):
            self.bucket.flat.zero_()
            fused.zero_in_step = False      # every step ends with the bucket cleared
        self.eager_left = int(eager_iterations)
        self.use_graphs = bool(use_graphs)
        self.graphs = None
        self.fallback_reason = None

    def _eager(self):
        self.fused.forward_backward()
        self.bucket.all_reduce_mean()
        self.opt.step()

    def _capture(self):
        from .parallel import world_info
        world = world_info()[1]
        torch.cuda.synchronize()
        # thread-local capture mode: with a process group alive, torch.distributed's watchdog thread queries events while this
        # thread captures - under the default (global) mode that is a capture error
        mode = dict(capture_error_mode="thread_local")
        if world == 1:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, **mode):
                self.fused.forward_and_fine_backward(both=True)
                self.opt.step()
            return [g]
        ga, gb, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga, **mode):
            self.fused.forward_and_fine_backward()
        with torch.cuda.graph(gb, pool=ga.pool(), **mode):     # (reads what graph A allocated: one memory pool, replayed in capture order)
            self.fused.coarse_backward()
        with torch.cuda.graph(gc, pool=ga.pool(), **mode):
            self.opt.step()
        return [ga, gb, gc]

    def _replay(self):
        import torch.distributed as dist
        from .models import mark_parameters_updated
        from .parallel import _avg_in_collective, world_info
        if len(self.graphs) == 1:
            self.graphs[0].replay()
        else:
            ga, gb, gc = self.graphs
            avg = _avg_in_collective()
            op = dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM
            # each network's segment through its own sink (the bucket's module order is the caller's choice)
            sinks = [m._grad_sink for m in self.fused.models]
            assert all(s.bucket is self.bucket for s in sinks), "GraphedTrainStep: both networks' gradients live in this step's bucket"
            ga.replay()
            w_fine = dist.all_reduce(self.bucket.segment(sinks[1].idx), op=op, async_op=True)
            gb.replay()
            w_coarse = dist.all_reduce(self.bucket.segment(sinks[0].idx), op=op, async_op=True)
            w_fine.wait(); w_coarse.wait()
            if not avg:
                self.bucket.flat.div_(world_info()[1])
            gc.replay()
        mark_parameters_updated()      # the replayed optimizer step ran no Python hook

    def step(self):
        """One training iteration.  The loss of the iteration is in self.fused.loss3 (device)."""
        self.fused.refresh_occupancy()      # outside every graph: where _eager and _replay both pass through
        if self.graphs is not None:
            return self._replay()
        if self.eager_left > 0 or not self.use_graphs:
            self.eager_left -= 1
            return self._eager()
        try:
            self.graphs = self._capture()          # a capture only records ...
        except Exception as exc:  # noqa: BLE001
            self.graphs, self.use_graphs = None, False
            self.fallback_reason = f"{type(exc).__name__}: {exc}"
            torch.cuda.synchronize()
            return self._eager()
        return self._replay()                      # ... this iteration's step runs here
