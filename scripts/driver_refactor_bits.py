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
samples, dn_mse2_loss, dn_render_loss, dn_camera_grad, dn_camera_grad_views."""
import argparse
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


def record(name, *tensors):
    """sha256 of each tensor's bytes (None: "-") under name, name.1, ..."""
    for k, t in enumerate(tensors):
        key = name if k == 0 else f"{name}.{k}"
        assert key not in OUT, key
        OUT[key] = "-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


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


def models_on(dev):
    import nerf
    from nerf import synthetic as syn
    out = []
    for seed in (21, 22):
        m = nerf.models.FlexibleNeRFModel(**NET)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(seed, sigma_bias=-1.0, **NET).items()})
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="import the package of this checkout (built there) instead of this script's")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from nerf import _ops, synthetic as syn
    dev = torch.device("cuda:0")
    e0 = torch.stack([torch.from_numpy(syn.scene_pose(v, n_views=8)) for v in range(V)]).to(dev)
    k = torch.from_numpy(syn.intrinsic(H, W)).to(dev)
    xi = torch.zeros(V, 6, device=dev)
    cams, cams_ndc = _ops.pose_records(xi, e0, k), _ops.pose_records(xi, e0, k, ndc_focal=NDC_FOCAL)
    images = rand(1, V, H, W, 3)
    batches = selection(dev, cams, cams_ndc, images)
    render(dev, batches)
    compositing(dev, batches)
    moved(dev, batches, cams, cams_ndc)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), sha256=OUT), fh, indent=1, sort_keys=True)
    print(f"{len(OUT)} tensors hashed -> {args.out}")


if __name__ == "__main__":
    main()
