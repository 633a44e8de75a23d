"""Developer probe for the C driver layer refactor (one render-backward driver, one composite-backward launcher, one device-camera
ray-selection kernel): calls the touched entry points on seeded inputs and writes a sha256 per output tensor.  Recorded, not gated.

    python scripts/driver_refactor_bits.py --out profiles/driver_refactor_bits_change.json
    python scripts/driver_refactor_bits.py --tree <a built checkout of the parent commit> --out profiles/driver_refactor_bits_parent.json

--tree PATH imports the package of another checkout (built there) instead of this one.  The two files must be identical.

The smallest shapes that reach every branch: 12 x 12 images of 3 views; 37 and 300 rays (more than one 256-thread workgroup, not a
multiple of 64; a draw of one view's pixels is without replacement, so it takes 37 and 144); 16 + 16 samples and one coarse-only
render; two seeded 4 x 128 networks with view directions; world and NDC rows.  The calls: the seven dn_select_rays* entry points (the
five sources of (view, pixel)), dn_render_rays_train_geom, dn_render_rays_backward_ws with nets = 1, 2, 3 in fp32, bf16 with 16-bit
saves and the 8-bit-saved mode (absmax partials from the compositing backward, and DEXNERF_S8_ABSMAX_KERNEL=1),
dn_render_rays_backward_geom in fp32 / bf16 with and without weight-gradient views, dn_volume_render_backward(_geom) at 16 and 130
samples, dn_mse2_loss, dn_render_loss, dn_camera_grad, dn_camera_grad_views.

The one-body refactor of the loss heads and the forward compositing added loss_heads() and forward_compositing() (their docstrings
list the cases): dn_mse2_loss, dn_render_loss and dn_render_loss_exposure at 1, 65 and 1025 rays, and on 5 rays dn_volume_render,
dn_composite_density(_quantiles), dn_composite_normals, dn_density_resample, dn_volume_render_backward(_geom), a training render that
draws its density noise in the compositing kernel and a render with DEXNERF_FUSED_COMPOSITE=1.  Their thousands of small outputs are
folded into one digest per group of cases (fold_into).

The pass that gave the density renders one driver per layer added density_renders() (its docstring lists the cases;
--density-renders runs it alone): profiles/density_render_refactor_bits_{parent,change}.json.

The pass that collapsed the occupancy-culled path to one gather body, one emit body, one culled pass and one stats sum added
culled_renders() (its docstring lists the cases; --culled-renders runs it alone): profiles/cull_refactor_bits_{parent,change}.json."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(argv):
    """The checkout whose package this process imports (--tree PATH, default: this one) - decided before the first import."""
    return os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else REPO


TREE = _tree(sys.argv)
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))

NET = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
H = W = 12
V = 3
NDC_FOCAL = 14.0
OUT = {}
FOLD = []
TENSORS = [0]     # tensors hashed (the outputs a call does not produce, None, are not counted)


def record(name, *tensors):
    """sha256 of each tensor's bytes (None: "-") under name, name.1, ...; after fold_into(label) the bytes go, in call order, into the
    one digest kept under the label instead."""
    TENSORS[0] += sum(t is not None for t in tensors)
    if FOLD:
        for t in tensors:
            FOLD[-1][1].update(b"-" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
        OUT[FOLD[-1][0]] = FOLD[-1][1].hexdigest()
        return
    for k, t in enumerate(tensors):
        key = name if k == 0 else f"{name}.{k}"
        assert key not in OUT, key
        OUT[key] = "-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def fold_into(label):
    """From here on one sha256 under `label` over every tensor recorded (thousands of small outputs: one line per group of cases in the
    record); None: back to a hash per tensor."""
    assert label not in OUT, label
    FOLD[:] = [] if label is None else [(label, hashlib.sha256())]


def rand(seed, *shape, normal=False):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) if normal else torch.rand(*shape, generator=g)).cuda()


def views_of(model, dev):
    from nerf import _ops
    return _ops.zeroed_grad_views([tuple(m.weight.shape) for m in model.linear_modules()], dev)


def flat(views):
    return torch.cat([t.reshape(-1) for pair in views for t in pair])


def selection(dev, cams, cams_ndc, images):
    """Every dn_select_rays* entry point; returns the (world, NDC) rows, targets and pairs of the 37- and 300-ray batches."""
    from nerf import _ops
    batches = {}
    for n in (37, 300):
        g = torch.Generator().manual_seed(n)
        pix = torch.randint(0, H * W, (n,), generator=g).to(dev)
        views = torch.randint(0, V, (n,), generator=g).to(dev, torch.int32)
        view = torch.tensor(1, dtype=torch.int32, device=dev)
        c = cams[1].cpu().tolist()
        record(f"select_rays n={n}", *_ops.select_rays(H, W, c[:9], c[9:12], c[12], c[13], c[14], 2.0, 6.0, pix, images[1]))
        record(f"select_rays_indirect n={n}", *_ops.select_rays_indirect(H, W, cams, view, 2.0, 6.0, pix, images))
        record(f"select_rays_indirect_ndc n={n}", *_ops.select_rays_indirect_ndc(H, W, cams_ndc, view, 0.0, 1.0, pix, NDC_FOCAL, 1.0, images))
        world = _ops.select_rays_views(H, W, cams, views, 2.0, 6.0, pix, images)
        ndc = _ops.select_rays_views(H, W, cams_ndc, views, 0.0, 1.0, pix, images, ndc_focal=NDC_FOCAL, ndc_near=1.0)
        record(f"select_rays_views world n={n}", *world)
        record(f"select_rays_views ndc n={n}", *ndc)
        for focal in (None, NDC_FOCAL):
            state = _ops.new_rng_state(11, dev, 4)
            record(f"select_rays_draw_views focal={focal} n={n}",
                   *_ops.select_rays_draw_views(H, W, cams_ndc if focal else cams, 2.0, 6.0, state, n, images, want_pixels=True, ndc_focal=focal), state)
        batches[n] = dict(world=world, ndc=ndc, pix=pix, views=views)
    for n in (37, H * W):     # one view's pixels: without replacement
        for focal in (None, NDC_FOCAL):
            for view in (torch.tensor(2, dtype=torch.int32, device=dev), None):     # the given view / the view drawn in the kernel
                state = _ops.new_rng_state(12, dev, 7)
                record(f"select_rays_draw focal={focal} view={'given' if view is not None else 'drawn'} n={n}",
                       *_ops.select_rays_draw(H, W, cams_ndc if focal else cams, view, 2.0, 6.0, state, n, images, want_pixels=True, ndc_focal=focal), state)
    return batches


def models_on(dev, **over):
    import nerf
    from nerf import synthetic as syn
    net = dict(NET, **over)
    out = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**net)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **net).items()})
        out.append(m.to(dev))
    return out


def render(dev, batches):
    """The training forward with its geometry, the two backward drivers; per case (rows, num_fine, white background, lindisp)."""
    import nerf
    from nerf import _hip, _ops
    mc, mf = models_on(dev)
    cases = {"37 world 16+16": (batches[37]["world"], 16, False, False), "300 ndc 16+16": (batches[300]["ndc"], 16, True, False),
             "300 world 16+0": (batches[300]["world"], 0, False, True)}
    for label, ((rows, target), nf, white, lindisp) in cases.items():
        n = rows.shape[0]
        for mode in ("fp32", "bf16-s16"):
            nerf.set_precision(mode)
            packs = []
            for m in (mc, mf):
                pk = m.packed(True, True, parts=_hip.PACK_CORE)
                _ops.ensure_backward_stream(m, pk, pk.precision)
                _ops.ensure_input_grad_stream(m, pk)
                packs.append(pk)
            pc, pf = packs[0], (packs[1] if nf else None)
            state = _ops.new_rng_state(5, dev, 3)
            maps, saved = _ops.render_rays_train_geom(pc, pf, rows, 16, nf, lindisp, 0.2, white, [], None, prec=pc.precision, rng_state=state, perturb=True)
            what = f"{label} {mode}"
            record(f"train_geom {what}", *maps[:6], saved["z_samples"])
            _, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target)
            gd_c, gd_f = rand(n, n), (rand(n + 1, n) if nf else None)
            up_c, up_f = (g_c, gd_c, None), (g_f, gd_f, None)
            record(f"backward_geom frozen {what}", _ops.render_rays_backward_geom(pc, pf, saved, up_c, up_f)[0])
            views_c, views_f = views_of(mc, dev), views_of(mf, dev)
            record(f"backward_geom wgrad {what}", _ops.render_rays_backward_geom(pc, pf, saved, up_c, up_f, views_c, views_f)[0], flat(views_c), flat(views_f))
            for nets in (1, 2, 3):
                views_c, views_f = views_of(mc, dev), views_of(mf, dev)
                _ops.render_rays_backward(pc, pf, saved, up_c, up_f, views_c, views_f, nets=nets)
                record(f"backward_ws nets={nets} {what}", flat(views_c), flat(views_f))
        # the default 8-bit-saved mode, as FusedTrainStep drives it
        nerf.set_precision("bf16")
        pc, pf, prec = _ops.pack_train_pair(mc, mf, (True, True))
        assert prec == _hip.PREC_BF16_S8
        state = _ops.new_rng_state(5, dev, 3)
        maps, saved = _ops.render_rays_train(pc, pf if nf else None, rows, 16, nf, lindisp, 0.2, white, [], None, prec=prec, rng_state=state, perturb=True)
        record(f"train {label} bf16-s8", *maps[:6])
        _, g_c, g_f = _ops.mse2_loss(maps[0], maps[3], target)
        for absmax_kernel in (False, True):
            if absmax_kernel:
                os.environ["DEXNERF_S8_ABSMAX_KERNEL"] = "1"
            for nets in (1, 2, 3):
                views_c, views_f = views_of(mc, dev), views_of(mf, dev)
                _ops.render_rays_backward(pc, pf if nf else None, saved, (g_c, None, None), (g_f, None, None), views_c, views_f, nets=nets)
                record(f"backward_ws nets={nets} {label} bf16-s8 absmax_kernel={absmax_kernel}", flat(views_c), flat(views_f))
            os.environ.pop("DEXNERF_S8_ABSMAX_KERNEL", None)
    nerf.set_precision("fp32")


def compositing(dev, batches):
    from nerf import _ops
    for n in (37, 300):
        rows = batches[n]["world"][0]
        for s in (16, 130):     # one 64-sample chunk / three (the 4-chunk instance)
            rf = rand(s, n, s, 4, normal=True)
            z = torch.sort(2.0 + 4.0 * rand(s + 1, n, s), dim=1).values
            ups = [rand(s + 2, n, 3), rand(s + 3, n), rand(s + 4, n), rand(s + 5, n), rand(s + 6, n, s)]
            for noise_std, white in ((0.0, False), (0.3, True)):
                noise = rand(s + 7, n, s, normal=True) if noise_std else None
                what = f"n={n} s={s} noise={noise_std}"
                record(f"volume_render_backward {what}", _ops.volume_render_bwd(rf, z, rows[:, 3:6], noise, noise_std, white, *ups))
                record(f"volume_render_backward_geom {what}", *_ops.volume_render_bwd_geom(rf, z, rows[:, 3:6], noise, noise_std, white, *ups))
                record(f"volume_render_backward_geom rf only {what}",
                       _ops.volume_render_bwd_geom(rf, z, rows[:, 3:6], noise, noise_std, white, *ups, want_z=False, want_rd=False)[0])
                record(f"volume_render_backward_geom z, rd only {what}",
                       *_ops.volume_render_bwd_geom(rf, z, rows[:, 3:6], noise, noise_std, white, *ups[:3], None, None, want_rf=False)[1:])


def moved(dev, batches, cams, cams_ndc):
    """The loss heads and the camera gradient: code that only moved."""
    from nerf import _ops
    for n in (37, 300):
        b = batches[n]
        rgb_c, rgb_f, target = rand(n, n, 3), rand(n + 1, n, 3), b["world"][1]
        depth_c, depth_f, depth_maps = 2.0 + 4.0 * rand(n + 2, n), 2.0 + 4.0 * rand(n + 3, n), 1.0 + 6.0 * rand(n + 4, V, H, W)
        for luminance in (False, True):
            state = _ops.new_rng_state(3, dev, 9)
            record(f"mse2_loss n={n} luminance={luminance}", *_ops.mse2_loss(rgb_c, rgb_f, target, luminance, state), state)
            state = _ops.new_rng_state(3, dev, 9)
            record(f"render_loss n={n} luminance={luminance}",
                   *_ops.render_loss(rgb_c, rgb_f, target, depth_c, depth_f, depth_maps, b["pix"], b["views"], None, (0.7, 1.3), (0.1, 0.2), (2.0, 6.0),
                                     luminance, state), state)
        record(f"render_loss coarse only, no depth n={n}", *_ops.render_loss(rgb_c, None, target, weights=(0.5, 0.0)))
        g = rand(n + 5, n, 11, normal=True)
        for focal, records in ((0.0, cams), (NDC_FOCAL, cams_ndc)):
            record(f"camera_grad n={n} focal={focal}", _ops.camera_grad(H, W, records[1], b["pix"], n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, 1.0))
            record(f"camera_grad_views n={n} focal={focal}",
                   _ops.camera_grad_views(H, W, records, b["views"], b["pix"], n, g[:, 0:3], g[:, 3:6], g[:, 8:11], focal, 1.0))


def loss_heads(dev):
    """The three loss heads (one kernel template): one ray, not a multiple of 64, a second trip of the 1024-thread loop; luminance;
    with and without rgb_f; depth targets absent / direct / gathered by view_index / gathered by the `view` word, over a range that
    keeps every ray, some and none; exposure rows (P = 1, 6; 3 views) with an all-zero row, a view_index out of range, a masked view,
    g_eps wanted and not."""
    from nerf import _ops
    view = torch.tensor(2, dtype=torch.int32, device=dev)
    mask = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    for n in (1, 65, 1025):
        g = torch.Generator().manual_seed(n)
        pix = torch.randint(0, H * W, (n,), generator=g).to(dev)
        views = torch.randint(0, V, (n,), generator=g).to(dev, torch.int32)
        stray = views.clone()
        stray[-1] = 7      # no such view: the ray takes the uncorrected expressions (never used to gather depth targets)
        rgb_c, rgb_f, target = rand(n, n, 3), rand(n + 1, n, 3), rand(n + 5, n, 3)
        depth_c, depth_f, depth_maps = 2.0 + 4.0 * rand(n + 2, n), 2.0 + 4.0 * rand(n + 3, n), 1.0 + 6.0 * rand(n + 4, V, H, W)
        targets = {"none": {}, "direct": dict(depth_src=1.0 + 6.0 * rand(n + 9, n)),
                   "view_index": dict(depth_src=depth_maps, pixel_index=pix, view_index=views),
                   "view": dict(depth_src=depth_maps, pixel_index=pix, view=view)}
        for luminance in (False, True):
            fold_into(f"loss heads n={n} luminance={luminance}")
            for fine in (rgb_f, None):
                what = f"n={n} luminance={luminance} fine={fine is not None}"
                state = _ops.new_rng_state(3, dev, 9)
                record(f"heads mse2_loss {what}", *_ops.mse2_loss(rgb_c, fine, target, luminance, state), state)
                for tname, tkw in targets.items():
                    for rname, lohi in (("all", (0.0, float("inf"))), ("some", (2.0, 6.0)), ("none", (100.0, 200.0))):
                        if tname == "none" and rname != "all":
                            continue
                        state = _ops.new_rng_state(3, dev, 9)
                        dkw = dict(tkw, depth_c=depth_c, depth_f=depth_f if fine is not None else None) if tkw else {}
                        record(f"heads render_loss {what} target={tname} range={rname}",
                               *_ops.render_loss(rgb_c, fine, target, weights=(0.7, 1.3), depth_weights=(0.1, 0.2), depth_range=lohi,
                                                 luminance=luminance, rng_state=state, **dkw), state)
                        if rname == "some":
                            continue
                        for p in (1, 6):
                            eps = 0.3 * rand(n + 6 + p, V, p, normal=True)
                            eps[1] = 0.0
                            # (the depth targets of the exposure head are gathered at the exposure views: the stray view goes with
                            # direct targets or none)
                            vkw = dict(view=view) if tname == "view" else dict(view_index=views if tname == "view_index" else stray)
                            ekw = {k: v for k, v in dkw.items() if k not in ("view", "view_index")}
                            for want_eps in (True, False):
                                record(f"heads render_loss_exposure {what} target={tname} range={rname} P={p} g_eps={want_eps}",
                                       *_ops.render_loss_exposure(rgb_c, fine, target, eps, 0.5, view_mask=mask, weights=(0.7, 1.3),
                                                                  depth_weights=(0.1, 0.2), depth_range=lohi, luminance=luminance,
                                                                  want_eps=want_eps, **vkw, **ekw))


def forward_compositing(dev):
    """Every client of the forward compositing body on 5 rays (four per workgroup): one sample, a ragged chunk, exactly one chunk, one
    sample more, three chunks; noise from a tensor and drawn in the kernel (a training render); white background; the weights map
    wanted and not; thresholds from the host (0, 1, 64), on the device (0, 64, 65, 100), quantiles (1, 64; both modes), normals, the
    fused coarse pass + resampling, the compositing backward with and without g_disp / g_weights, and one render whose network
    launches composite their own rays."""
    import nerf
    from nerf import _hip, _ops
    n = 5
    rd = rand(70, n, 3, normal=True)
    thres = lambda k: [0.05 + 2.5 * i / max(k, 1) for i in range(k)]
    for s in (1, 63, 64, 65, 129):
        rf = rand(s, n, s, 4, normal=True)
        z = torch.sort(2.0 + 4.0 * rand(s + 1, n, s), dim=1).values
        g_pts = rand(s + 8, n, s, 3, normal=True)
        g_pts[0, 0] = 0.0     # a zero gradient: the zero normal
        fold_into(f"forward compositing, 5 rays, s={s}")
        for noise_std, white in ((0.0, False), (0.3, True)):
            noise = rand(s + 7, n, s, normal=True) if noise_std else None
            what = f"s={s} noise={noise_std}"
            for k in (0, 1, 64):
                for want_weights in (True, False):
                    record(f"volume_render {what} white={white} K={k} weights={want_weights}",
                           *_ops.volume_render_fwd(rf, z, rd, noise, noise_std, white, thres(k), want_weights))
            for k in (0, 64, 65, 100):
                record(f"composite_density {what} K={k}", *_ops.composite_density(rf, z, rd, noise, noise_std, thres(k)))
            for q in (1, 64):
                for interp in (False, True):
                    record(f"composite_density_quantiles {what} Q={q} interp={interp}",
                           *_ops.composite_density_quantiles(rf, z, rd, noise, noise_std, thres(3), [(i + 1.0) / (q + 1.0) for i in range(q)], interp))
            record(f"composite_normals {what}", *_ops.composite_normals(rf, z, rd, g_pts, noise, noise_std, thres(65)))
    for nc, nf in ((10, 1), (64, 65)):
        fold_into(f"density_resample, 5 rays, nc={nc} nf={nf}")
        rf = rand(nc, n, nc, 4, normal=True)
        z = torch.sort(2.0 + 4.0 * rand(nc + 1, n, nc), dim=1).values
        for noise_std in (0.0, 0.3):
            record(f"density_resample nc={nc} nf={nf} noise={noise_std}",
                   *_ops.density_resample(rf, z, rd, nf, rand(nc + 2, n, nc, normal=True) if noise_std else None, noise_std, rand(nc + 3, n, nf)))
    for s in (16, 64, 65, 130):
        fold_into(f"backward compositing, 5 rays, s={s}")
        rf = rand(s, n, s, 4, normal=True)
        z = torch.sort(2.0 + 4.0 * rand(s + 1, n, s), dim=1).values
        ups = [rand(s + 2, n, 3), rand(s + 3, n), rand(s + 4, n), rand(s + 5, n), rand(s + 6, n, s)]
        for noise_std, white in ((0.0, False), (0.3, True)):
            noise = rand(s + 7, n, s, normal=True) if noise_std else None
            for extras in (True, False):
                u = ups if extras else ups[:3] + [None, None]
                what = f"5 rays s={s} noise={noise_std} g_disp, g_weights={extras}"
                record(f"volume_render_backward {what}", _ops.volume_render_bwd(rf, z, rd, noise, noise_std, white, *u))
                record(f"volume_render_backward_geom {what}", *_ops.volume_render_bwd_geom(rf, z, rd, noise, noise_std, white, *u))
    fold_into(None)
    # the density noise drawn in the compositing kernel: a training render of 65 + 64 samples
    rows = torch.cat([rand(80, n, 3) - 0.5, rd, torch.full((n, 1), 2.0, device=dev), torch.full((n, 1), 6.0, device=dev),
                      torch.nn.functional.normalize(rd, dim=-1)], dim=1).contiguous()
    mc, mf = models_on(dev)
    nerf.set_precision("fp32")
    packs = []
    for m in (mc, mf):
        pk = m.packed(True, True, parts=_hip.PACK_CORE)
        _ops.ensure_backward_stream(m, pk, pk.precision)
        packs.append(pk)
    state = _ops.new_rng_state(5, dev, 3)
    maps, _ = _ops.render_rays_train(packs[0], packs[1], rows, 65, 64, False, 0.3, True, [], None, prec=packs[0].precision, rng_state=state, perturb=True)
    record("train 5 rays 65+64 noise drawn in the kernel", *maps[:6])
    # the network launches compositing their own rays (16-bit, whole rays per 384-point tile), and the same render without
    nerf.set_precision("bf16")
    try:
        pc, pf = mc.packed(precision=_hip.PREC_BF16), mf.packed(precision=_hip.PREC_BF16)
        for fused in (False, True):
            if fused:
                os.environ["DEXNERF_FUSED_COMPOSITE"] = "1"
            fold_into(f"render_rays 5 rays 64+128 bf16 fused={fused} (the two must agree)")
            try:
                record(f"render_rays 5 rays 64+128 bf16 fused={fused}", *_ops.render_rays(pc, pf, rows, 64, 128, False, 0.0, True, thres(3)))
            finally:
                os.environ.pop("DEXNERF_FUSED_COMPOSITE", None)
    finally:
        fold_into(None)
        nerf.set_precision("fp32")


def density_renders(dev):
    """The density renders and what stands beside them, for the pass that gave them one driver per layer.  Two seeded 4 x 128 networks
    (L_xyz = 10; full packs for render_rays, density packs for the rest).  5 and 37 rays (0 where the wrapper allows it: elsewhere the
    refusal's text is recorded), 16 + 16 samples and coarse-only; (K, noise_std, lindisp) in (0, 0, off), (1, 0.3, on), (65, 0.3, off)
    with given noise tensors (render_rays: K = 64, the host limit); fp32 and bf16, render_rays also in the fp16-guarded default;
    Q = 1 and 64 quantiles with interp 0 and 1; the status words after every render.  The standalone compositing calls at 130
    samples (a third chunk).  render_dex_depth (with and without quantiles) and render_dex_normals on a 6 x 7 image in validation
    mode with chunksize 16 (three chunks, a short last one), world and NDC.  The answers of seven *_workspace_bytes functions.
    One digest per group of cases (fold_into); the refusals are kept as text."""
    import nerf
    from nerf import _hip, _ops
    lib = _hip.lib()
    mc, mf = models_on(dev)
    thres = lambda k: [0.05 + 2.5 * i / max(k, 1) for i in range(k)]
    quants = lambda q: [(i + 1.0) / (q + 1.0) for i in range(q)]
    on_dev = lambda values: torch.tensor(values, dtype=torch.float32, device=dev) if values else None

    def refusal(name, fn):
        try:
            fn()
        except (RuntimeError, ValueError) as e:
            OUT[name] = f"refused: {e}"
        else:
            OUT[name] = "accepted"

    def rows_of(n):
        rd = rand(70 + n, n, 3, normal=True)
        return torch.cat([rand(80 + n, n, 3) - 0.5, rd, torch.full((n, 1), 2.0, device=dev), torch.full((n, 1), 6.0, device=dev),
                          torch.nn.functional.normalize(rd, dim=-1)], dim=1).contiguous()

    def draws_of(n, nf, std):
        d = dict(t_rand=rand(90, n, 16), u=rand(91, n, nf) if nf else None)
        if std:
            d.update(noise_c=rand(92, n, 16, normal=True), noise_f=rand(93, n, 16 + nf, normal=True) if nf else None)
        return d
    settings = ((0, 0.0, False), (1, 0.3, True), (65, 0.3, False))
    nerf.set_precision("bf16")
    guarded = _ops.render_precision()
    nerf.set_precision("fp32")
    for pname, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16), ("guarded", guarded)):
        full = (mc.packed(precision=prec), mf.packed(precision=prec))
        for n in (0, 5, 37):
            fold_into(f"render_rays {pname} n={n}")
            for nf in (16, 0):
                for k, std, lindisp in settings:
                    what = f"{pname} n={n} 16+{nf} K={k} noise={std} lindisp={lindisp}"
                    maps = _ops.render_rays(*full, rows_of(n), 16, nf, lindisp, std, k == 1, thres(min(k, 64)), draws_of(n, nf, std))
                    # (an empty call returns before the status block is zeroed: its words are not this call's)
                    record(f"render_rays {what}", *maps, _ops.render_status_words() if n else None)
        if pname == "guarded":
            continue
        dens = (mc.packed_density(True, True, precision=prec), mf.packed_density(True, True, precision=prec))
        streams = (mc.packed_density_grad(True, True, precision=prec), mf.packed_density_grad(True, True, precision=prec))
        for nf in (16, 0):
            refusal(f"render_rays_depth {pname} n=0 16+{nf}", lambda: _ops.render_rays_depth(*dens, rows_of(0), 16, nf, False, 0.0, None))
            refusal(f"render_rays_normals {pname} n=0 16+{nf}",
                    lambda: _ops.render_rays_normals(*dens, streams[1 if nf else 0], rows_of(0), 16, nf, False, 0.0, None))
        for n in (5, 37):
            fold_into(f"render_rays_depth (also with quantiles), render_rays_normals {pname} n={n}")
            for nf in (16, 0):
                for k, std, lindisp in settings:
                    what = f"{pname} n={n} 16+{nf} K={k} noise={std} lindisp={lindisp}"
                    args = (rows_of(n)[:, :8].contiguous(), 16, nf, lindisp, std, on_dev(thres(k)), draws_of(n, nf, std))
                    record(f"render_rays_depth {what}", *_ops.render_rays_depth(*dens, *args), _ops.render_status_words())
                    for q in (1, 64):
                        for interp in (False, True):
                            record(f"render_rays_depth {what} Q={q} interp={interp}",
                                   *_ops.render_rays_depth(*dens, *args, quantiles=on_dev(quants(q)), interp=interp), _ops.render_status_words())
                    record(f"render_rays_normals {what}", *_ops.render_rays_normals(*dens, streams[1 if nf else 0], *args))
    # the standalone compositing calls: a third 64-sample chunk
    s = 130
    for n in (0, 5, 37):
        rd = rand(100 + n, n, 3, normal=True)
        rf = rand(101, n, s, 4, normal=True)
        z = torch.sort(2.0 + 4.0 * rand(102, n, s), dim=1).values
        g_pts = rand(103, n, s, 3, normal=True)
        fold_into(f"standalone compositing n={n} s={s}")
        for k, std, _ in settings:
            noise = rand(104, n, s, normal=True) if std else None
            what = f"n={n} s={s} K={k} noise={std}"
            if n == 0:
                refusal(f"composite_density_quantiles {what}", lambda: _ops.composite_density_quantiles(rf, z, rd, noise, std, thres(k), quants(1)))
                refusal(f"composite_normals {what}", lambda: _ops.composite_normals(rf, z, rd, g_pts, noise, std, thres(k)))
            else:
                for q in (1, 64):
                    for interp in (False, True):
                        record(f"composite_density_quantiles {what} Q={q} interp={interp}",
                               *_ops.composite_density_quantiles(rf, z, rd, noise, std, thres(k), quants(q), interp))
                record(f"composite_normals {what}", *_ops.composite_normals(rf, z, rd, g_pts, noise, std, thres(k)))
                record(f"composite_normals no dex {what}", *_ops.composite_normals(rf, z, rd, g_pts, noise, std, on_dev(thres(k)), want_dex=False))
            record(f"composite_density {what}", *_ops.composite_density(rf, z, rd, noise, std, thres(k)))
            record(f"density_resample {what}", *_ops.density_resample(rf, z, rd, 65, noise, std, rand(105, n, 65)))
    # the image-level renders: 6 x 7, validation mode, three chunks of 16, 16, 10 rays
    from nerf import synthetic as syn
    h, w = 6, 7
    mode = dict(chunksize=16, lindisp=False, num_coarse=16, num_fine=16, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    ex = nerf.get_embedding_function(10, True, True)
    k_mat = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
    focal = float(k_mat[0, 0])
    ro, rd = nerf.get_ray_bundle(h, w, focal, torch.from_numpy(syn.scene_pose(3)).to(dev), k_mat)
    for space, dataset in (("world", dict(near=2.0, far=6.0, no_ndc=True)), ("ndc", dict(near=0.0, far=1.0, no_ndc=False))):
        for nf in (16, 0):
            cfg = nerf.CfgNode(dict(dataset=dataset, nerf=dict(use_viewdirs=True, train=dict(mode, num_fine=nf), validation=dict(mode, num_fine=nf))))
            for precision in ("fp32", "bf16"):
                nerf.set_precision(precision)
                what = f"{space} 16+{nf} {precision}"
                fold_into(f"render_dex_depth (also with quantiles), render_dex_normals 6 x 7 {what}")
                with torch.no_grad():
                    for qs in (None, (0.1, 0.5, 0.9)):
                        maps = nerf.render_dex_depth(h, w, focal, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex,
                                                     m_thres_cand=thres(2), quantiles=qs, quantile_interp=qs is not None)
                        record(f"render_dex_depth {what} quantiles={qs}", *maps, _ops.render_status_words())
                    out = nerf.render_dex_normals(h, w, focal, mc, mf, ro, rd, cfg, mode="validation", encode_position_fn=ex, m_thres_cand=thres(2))
                    record(f"render_dex_normals {what}", out.depth, out.acc, out.normal, *out.dex_depth, *out.dex_normal)
    nerf.set_precision("fp32")
    fold_into(None)
    # the workspace sizes
    full_desc, dens_desc = mc.packed(precision=_hip.PREC_F32).desc, mc.packed_density(True, True, precision=_hip.PREC_F32).desc
    sizes = []
    for n in (0, 1, 5, 4097):
        for nc, nf in ((16, 0), (16, 16), (64, 128)):
            d, f = ctypes.byref(dens_desc), ctypes.byref(full_desc)
            sizes.append([lib.dn_render_workspace_bytes(n, nc, nf), lib.dn_render_depth_workspace_bytes(n, nc, nf),
                          lib.dn_render_train_workspace_bytes(n, nc, nf), lib.dn_render_reg_workspace_bytes(n, nc, nf),
                          lib.dn_render_normals_workspace_bytes(d, d if nf else None, _hip.PREC_F32, n, nc, nf),
                          lib.dn_render_normals_workspace_bytes(d, d if nf else None, _hip.PREC_BF16, n, nc, nf),
                          lib.dn_render_backward_geom_workspace_bytes(f, f if nf else None, n, 11, nc, nf)])
    OUT["workspace bytes (render, depth, train, reg, normals fp32, normals bf16, backward_geom) over n x (nc, nf)"] = json.dumps(sizes)


def culled_renders(dev):
    """The occupancy-culled path, for the pass that gave it one gather body, one emit body, one culled pass and one stats sum.  A
    5 x 4 x 3 grid with no cell, every cell and a seeded 40 % of the cells set.  One digest per group of cases (fold_into); the kept /
    total counts are kept as text.

    The entry points, on p = 1, 63, 64, 65, 1023, 1024, 1025 and 1024 * 1024 + 3 samples in and around the unit box (7, 3 or 1 per ray,
    11-column rays): dn_occupancy_compact_count (slots and record); both emits at capacity 0, half the kept count and the kept count,
    into planted buffers; dn_occupancy_gather and dn_occupancy_gather_rows (widths 1 .. 4; dense rows - width 4: the 16-byte path - and
    column views: source stride 6, destination stride 5) with n_rows 0, half the kept count and the kept count, with and without the
    count, the sources carrying planted non-finite values; destination and record after every call.

    The drivers render_rays_depth_culled, render_rays_culled and render_rays_normals_culled on 37 and 300 rays, 16 + 16 samples and
    coarse-only, two seeded 4 x 128 networks, fp32 and bf16, (noise_std, lindisp) in (0, off), (0.3, on) with given draws,
    count_nonfinite off and on, three thresholds.  Depth: without quantiles and with three, interp off and on.  Colour: networks with
    view directions (11-column rays) and without (8-column rays).  Normals: one slab, and max_points = 50 - below the kept count
    wherever much is kept - so that the slab loop runs.  Maps, records and the kept / total counts of every call.

    The image-level renders with occupancy= and cull_stats=True (render_dex_depth - also with quantiles -, run_one_iter_of_nerf,
    render_dex_normals) on a 6 x 7 image in validation mode with chunksize 16 (three chunks), fp32 and bf16: the maps and the stats."""
    import nerf
    from nerf import _hip, _ops
    cells = (5, 4, 3)

    def grids(box):
        g = torch.Generator().manual_seed(5)
        draw = torch.rand(cells, generator=g)
        return {name: nerf.OccupancyGrid.from_mask((draw < share).to(dev), box) for name, share in (("none", 0.0), ("all", 2.0), ("random", 0.4))}

    def planted(seed, n, columns):
        """max(n, 1) rows of normal values with non-finite ones planted"""
        src = rand(seed, max(n, 1), columns, normal=True)
        flat = src.view(-1)
        flat[::97] = float("nan")
        flat[5::131] = float("inf")
        flat[7::173] = float("-inf")
        return src

    # ---- the entry points
    unit = grids((0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    fills = (-0.0, _hip.OCC_FILL, 1.5, 0.0)
    for p in (1, 63, 64, 65, 1023, 1024, 1025, 1024 * 1024 + 3):
        fold_into(f"culled entry points p={p}")
        s = next(q for q in (7, 3, 1) if p % q == 0)
        n = p // s
        rays = torch.cat([rand(p, n, 3) * 0.6 - 0.2, rand(p + 1, n, 3) * 1.4 - 0.5, rand(p + 2, n, 5)], dim=1).contiguous()
        z = (rand(p + 3, n, s) * 1.2).contiguous()
        counts = []
        for gname, grid in unit.items():
            slot, rec, ws = _ops.occupancy_compact_count(rays, z, grid)
            record(f"count p={p} {gname}", slot, rec)
            n_kept = int(rec[0].item())
            counts.append(n_kept)
            for cap in (0, n_kept // 2, n_kept):
                pts = torch.full((n_kept + 2, 3), 7.0, device=dev)
                record(f"emit p={p} {gname} cap={cap}", _ops.occupancy_compact_emit(rays, z, slot, cap, pts))
                pts, dirs = torch.full((n_kept + 2, 3), 7.0, device=dev), torch.full((n_kept + 2, 3), 9.0, device=dev)
                record(f"emit_dirs p={p} {gname} cap={cap}", *_ops.occupancy_compact_emit_dirs(rays, z, slot, cap, pts, dirs))
            net = planted(p + 4, n_kept, 4)
            sources = {width: (planted(p + 5 + width, n_kept, width), planted(p + 9 + width, n_kept, 6)) for width in (1, 2, 3, 4)}
            for n_rows in (0, n_kept // 2, n_kept):
                for count in (True, False):
                    what = f"p={p} {gname} n_rows={n_rows} count={count}"
                    rf, r2 = torch.full((n, s, 4), 3.0, device=dev), rec.clone()
                    _ops.occupancy_gather(slot, net[:n_rows] if n_rows else None, rf, *((ws, r2) if count else ()))
                    record(f"gather {what}", rf, r2)
                    for width in (1, 2, 3, 4):
                        dense, wide = sources[width]
                        for layout, src, dst in (("dense", dense, torch.full((p, width), 3.0, device=dev)),
                                                 ("views", wide[:, 2:2 + width], torch.full((p, 5), 3.0, device=dev))):
                            r2 = rec.clone()
                            _ops.occupancy_gather_rows(slot, src[:n_rows] if n_rows else None, dst if layout == "dense" else dst[:, 1:1 + width],
                                                       width, fills[:width], *((ws, r2) if count else ()))
                            record(f"gather_rows {what} width={width} {layout}", dst, r2)
        fold_into(None)
        OUT[f"culled entry points p={p}: kept (none, all, random)"] = json.dumps(counts)

    # ---- the drivers
    thres = [0.05, 0.9, 1.7]
    on_dev = lambda values: torch.tensor(values, dtype=torch.float32, device=dev)
    world = grids((-6.0, -6.0, -6.0, 6.0, 6.0, 6.0))
    with_dirs, without_dirs = models_on(dev), models_on(dev, use_viewdirs=False)

    def rows_of(n):
        rd = rand(70 + n, n, 3, normal=True)
        return torch.cat([rand(80 + n, n, 3) - 0.5, rd, torch.full((n, 1), 2.0, device=dev), torch.full((n, 1), 6.0, device=dev),
                          torch.nn.functional.normalize(rd, dim=-1)], dim=1).contiguous()

    def draws_of(n, nf, std):
        d = dict(t_rand=rand(90, n, 16), u=rand(91, n, nf) if nf else None)
        if std:
            d.update(noise_c=rand(92, n, 16, normal=True), noise_f=rand(93, n, 16 + nf, normal=True) if nf else None)
        return d
    for pname, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16)):
        full = {True: [m.packed(precision=prec) for m in with_dirs], False: [m.packed(precision=prec) for m in without_dirs]}
        dens = [m.packed_density(True, True, precision=prec) for m in with_dirs]
        streams = [m.packed_density_grad(True, True, precision=prec) for m in with_dirs]
        for n in (37, 300):
            fold_into(f"culled drivers {pname} n={n}")
            counts = {}
            for nf in (16, 0):
                for gname, grid in world.items():
                    for std, lindisp in ((0.0, False), (0.3, True)):
                        for count in (False, True):
                            what = f"{pname} n={n} 16+{nf} {gname} noise={std} lindisp={lindisp} count={count}"
                            rows, draws = rows_of(n), draws_of(n, nf, std)
                            rows8 = rows[:, :8].contiguous()

                            def keep(name, maps, stats):
                                record(name, *maps, *stats["records"])
                                counts[name] = [list(stats["kept"]), list(stats["total"])]
                            for qname, q, interp in (("none", None, False), ("3", on_dev([0.1, 0.5, 0.9]), False), ("3 interp", on_dev([0.1, 0.5, 0.9]), True)):
                                keep(f"depth {what} quantiles={qname}",
                                     *_ops.render_rays_depth_culled(*dens, rows8, 16, nf, lindisp, std, on_dev(thres), grid, draws, quantiles=q,
                                                                    interp=interp, count_nonfinite=count))
                            for dirs in (True, False):
                                keep(f"colour {what} viewdirs={dirs}",
                                     *_ops.render_rays_culled(*full[dirs], rows if dirs else rows8, 16, nf, lindisp, std, std > 0.0, thres, grid, draws,
                                                              count_nonfinite=count))
                            for max_points in (None, 50):
                                keep(f"normals {what} max_points={max_points}",
                                     *_ops.render_rays_normals_culled(*dens, streams[1 if nf else 0], rows8, 16, nf, lindisp, std, on_dev(thres), grid,
                                                                      draws, count_nonfinite=count, max_points=max_points))
            fold_into(None)
            OUT[f"culled drivers {pname} n={n}: (kept, total) per call"] = json.dumps(counts, sort_keys=True)

    # ---- the image-level renders: 6 x 7, validation mode, three chunks of 16, 16, 10 rays
    from nerf import synthetic as syn
    h, w = 6, 7
    mode = dict(chunksize=16, lindisp=False, num_coarse=16, num_fine=16, perturb=False, radiance_field_noise_std=0.0, white_background=False)
    cfg = nerf.CfgNode(dict(dataset=dict(near=2.0, far=6.0, no_ndc=True), nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))
    ex, ed = nerf.get_embedding_function(10, True, True), nerf.get_embedding_function(4, True, True)
    k_mat = torch.from_numpy(syn.intrinsic(h, w)).to(dev)
    focal = float(k_mat[0, 0])
    ro, rd = nerf.get_ray_bundle(h, w, focal, torch.from_numpy(syn.scene_pose(3)).to(dev), k_mat)
    mc, mf = with_dirs
    for precision in ("fp32", "bf16"):
        nerf.set_precision(precision)
        for gname, grid in world.items():
            what = f"6 x 7 {precision} {gname}"
            fold_into(f"culled image renders {what}")
            kw = dict(mode="validation", encode_position_fn=ex, m_thres_cand=thres, occupancy=grid, cull_stats=True)
            stats = []
            with torch.no_grad():
                for qs in (None, (0.1, 0.5, 0.9)):
                    *maps, st = nerf.render_dex_depth(h, w, focal, mc, mf, ro, rd, cfg, quantiles=qs, **kw)
                    record(f"render_dex_depth {what} quantiles={qs}", *maps)
                    stats.append(st)
                *maps, st = nerf.run_one_iter_of_nerf(h, w, focal, mc, mf, ro, rd, cfg, encode_direction_fn=ed, **kw)
                record(f"run_one_iter_of_nerf {what}", *maps)
                stats.append(st)
                out, st = nerf.render_dex_normals(h, w, focal, mc, mf, ro, rd, cfg, **kw)
                record(f"render_dex_normals {what}", out.depth, out.acc, out.normal, *out.dex_depth, *out.dex_normal)
                stats.append(st)
            fold_into(None)
            OUT[f"culled image renders {what}: stats (depth, depth with quantiles, colour, normals)"] = json.dumps(stats, sort_keys=True)
    nerf.set_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="import the package of this checkout (built there) instead of this script's")
    ap.add_argument("--out", required=True)
    ap.add_argument("--density-renders", action="store_true", help="the density_renders() group alone")
    ap.add_argument("--culled-renders", action="store_true", help="the culled_renders() group alone")
    args = ap.parse_args()
    from nerf import _ops, synthetic as syn
    dev = torch.device("cuda:0")
    if not (args.density_renders or args.culled_renders):
        e0 = torch.stack([torch.from_numpy(syn.scene_pose(v, n_views=8)) for v in range(V)]).to(dev)
        k = torch.from_numpy(syn.intrinsic(H, W)).to(dev)
        xi = torch.zeros(V, 6, device=dev)
        cams, cams_ndc = _ops.pose_records(xi, e0, k), _ops.pose_records(xi, e0, k, ndc_focal=NDC_FOCAL)
        images = rand(1, V, H, W, 3)
        batches = selection(dev, cams, cams_ndc, images)
        render(dev, batches)
        compositing(dev, batches)
        moved(dev, batches, cams, cams_ndc)
        loss_heads(dev)
        fold_into(None)
        forward_compositing(dev)
    if not args.culled_renders:
        density_renders(dev)
    if not args.density_renders:
        culled_renders(dev)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), sha256=OUT, tensors=TENSORS[0]), fh, indent=1, sort_keys=True)
    print(f"{TENSORS[0]} tensors hashed into {len(OUT)} entries -> {args.out}")


if __name__ == "__main__":
    main()
