"""Developer probe for the network host layer refactor (one shape rule, table dispatch, one pack path): packs five seeded networks
through every pack entry point, runs every dispatch route of the network kernels, and writes a sha256 per output tensor.  Recorded,
not gated.

    python scripts/net_host_refactor_bits.py --out profiles/net_host_refactor_bits_change.json
    python scripts/net_host_refactor_bits.py --tree <a built checkout of the parent commit> --out profiles/net_host_refactor_bits_parent.json

--tree PATH imports the package of another checkout (built there) instead of this one.  The two files must be identical.

Every buffer a kernel writes into is zero-filled first, so padding cannot differ.  Inputs: 50 rays x 24 samples = 1,200 points - more than
three 384-point tiles with a ragged tail; 24 divides 384, so the self-compositing route applies; on 256 compute units the default
picks two point groups for the 8-bit training launches."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else REPO
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "dex-nerf_amd"))


def net(depth, width, skip, lxyz, viewdirs):
    return dict(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=lxyz, num_encoding_fn_dir=4, use_viewdirs=viewdirs)


NETS = {"4x128 L10": net(4, 128, 4, 10, True), "4x128 L6": net(4, 128, 4, 6, True), "D8W256": net(8, 256, 4, 10, True),
        "D3W128 no view": net(3, 128, 4, 10, False), "D6W256 skip3": net(6, 256, 3, 10, True)}
SWITCHES = {"none": {}, "geom32": {"DEXNERF_BF16_GEOM": "32"}, "runtime_shape": {"DEXNERF_G48_RUNTIME_SHAPE": "1"},
            "no_overlap": {"DEXNERF_G48_NO_OVERLAP": "1"}}
N_RAYS, S = 50, 24
OUT = {}


def record(name, *tensors):
    """OUT[name] = the sha256 of each tensor's bytes (None: "-"), in order; a callable is called first, and a refusal of the library is
    recorded with its text (some routes have no kernel, e.g. fp16 on the 32-point kernels of an L_xyz = 6 net)."""
    if len(tensors) == 1 and callable(tensors[0]):
        try:
            tensors = tensors[0]()
            tensors = tensors if isinstance(tensors, (tuple, list)) else (tensors,)
        except RuntimeError as e:
            OUT[name] = f"refused: {e}"
            return
    assert name not in OUT, name
    OUT[name] = ["-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for t in tensors]


class switched:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)


def models_of(kw, dev):
    import nerf
    out = []
    for seed in (31, 32):
        torch.manual_seed(seed)
        out.append(nerf.models.FlexibleNeRFModel(**kw).to(dev))
    return out


def zero_packed(cls, m, prec, *pack_args):
    """A packed network of m whose buffer was zero-filled before the pack."""
    pk = cls(m.desc_kwargs(), m.layer1.weight.device, prec)
    pk.buffer.zero_()
    mods = m.linear_modules()
    pk.pack([x.weight for x in mods], [x.bias for x in mods], *pack_args)
    return pk


def zero_backward_stream(m, pk, prec):
    from nerf import _ops
    nbytes = _ops.lib().dn_mlp_backward_packed_bytes(ctypes.byref(pk.desc), prec)
    pk.buffers_bwd[prec] = torch.zeros(nbytes, dtype=torch.uint8, device=pk.buffer.device)
    _ops.pack_backward(pk, [x.weight for x in m.linear_modules()], prec)
    return pk.buffers_bwd[prec]


def packs(name, ma, mb):
    """Every packed stream of the network: core + 48-point region in three precisions, density packs, backward streams 16-bit and
    8-bit, input-gradient streams, the four buffers of the pair call."""
    from nerf import _hip, _ops
    dev = ma.layer1.weight.device
    for pname, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16), ("fp16", _hip.PREC_F16)):
        record(f"pack {name} {pname}", zero_packed(_ops.PackedMLP, ma, prec).buffer)
        if ma.use_viewdirs:
            record(f"pack_density {name} {pname}", zero_packed(_ops.PackedDensityMLP, ma, prec).buffer)
    for pname, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16)):
        pk = _ops.PackedMLP(ma.desc_kwargs(), dev, prec)
        record(f"pack_backward {name} {pname}", zero_backward_stream(ma, pk, prec))
        nbytes = _ops.lib().dn_mlp_input_grad_packed_bytes(ctypes.byref(pk.desc), prec)
        pk.buffer_ig = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        record(f"pack_input_grad {name} {pname}", _ops.ensure_input_grad_stream(ma, pk))
    pa, pb = (_ops.PackedMLP(m.desc_kwargs(), dev, _hip.PREC_BF16) for m in (ma, mb))
    if not _ops.s8_supported(pa):
        return
    S8 = _hip.PREC_BF16_S8
    record(f"pack_backward {name} s8", zero_backward_stream(ma, pa, S8))
    arrays, keep = [], []
    for m, pk in ((ma, pa), (mb, pb)):
        pk.buffer.zero_()
        pk.buffers_bwd[S8] = torch.zeros(_ops.lib().dn_mlp_backward_packed_bytes(ctypes.byref(pk.desc), S8), dtype=torch.uint8, device=dev)
        mods = m.linear_modules()
        wp, ws = _ops._ptr_array([x.weight for x in mods], sources=True)
        bp, bs = _ops._ptr_array([x.bias for x in mods], sources=True)
        arrays += [wp, bp]
        keep.append((ws, bs))
    _ops.check(_ops.lib().dn_mlp_pack_train_pair(ctypes.byref(pa.desc), arrays[0], arrays[1], _ops.ptr(pa.buffer), _ops.ptr(pa.buffers_bwd[S8]),
                                                 arrays[2], arrays[3], _ops.ptr(pb.buffer), _ops.ptr(pb.buffers_bwd[S8]), _ops.stream()),
               "dn_mlp_pack_train_pair")
    torch.cuda.synchronize()
    record(f"pack_train_pair {name}", pa.buffer, pa.buffers_bwd[S8], pb.buffer, pb.buffers_bwd[S8])


def inputs(dev):
    g = torch.Generator().manual_seed(7)
    ro = torch.rand(N_RAYS, 3, generator=g) - 0.5
    rd = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=g), dim=-1) * (0.8 + 0.4 * torch.rand(N_RAYS, 1, generator=g))
    rows = torch.cat([ro, rd, torch.full((N_RAYS, 1), 2.0), torch.full((N_RAYS, 1), 6.0), torch.nn.functional.normalize(rd, dim=-1)], dim=1)
    z = torch.sort(2.0 + 4.0 * torch.rand(N_RAYS, S, generator=g), dim=1).values
    pts = (ro[:, None, :] + rd[:, None, :] * z[..., None]).reshape(-1, 3) * 0.25
    g_out = torch.randn(N_RAYS * S, 4, generator=g) * 1e-3
    return dict(rows=rows.to(dev), z=z.to(dev), pts=pts.to(dev), vd=rows[:, 8:11].contiguous().to(dev), g_out=g_out.to(dev))


def inference(name, m, x):
    """dn_run_network in the three input modes and three precisions under each switch, the density pair, dn_fp16_range_guard."""
    from nerf import _hip, _ops
    for sname, env in SWITCHES.items():
        with switched(env):
            OUT[f"fp16_range_guard {name} {sname}"] = int(_ops.fp16_range_guard(m))
            OUT[f"fp16_range_guard density {name} {sname}"] = int(_ops.fp16_range_guard(m, density=True)) if m.use_viewdirs else "-"
            for pname, prec in (("fp32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16), ("fp16", _hip.PREC_F16)):
                pk = zero_packed(_ops.PackedMLP, m, prec)
                what = f"{name} {pname} {sname}"
                record(f"run_network rays {what}", lambda: _ops.run_network_rays(pk, x["rows"], x["z"]))
                record(f"run_network pts {what}", lambda: _ops.run_network_pts(pk, x["pts"], x["vd"] if m.use_viewdirs else None, S))
                enc = [_ops.positional_encoding(x["pts"], m.num_encoding_fn_xyz)]
                if m.use_viewdirs:
                    enc.append(_ops.positional_encoding(x["vd"], 4).repeat_interleave(S, dim=0))
                record(f"forward_encoded {what}", lambda: _ops.mlp_forward_encoded(pk, torch.cat(enc, dim=1)))
                if m.use_viewdirs and sname in ("none", "runtime_shape"):   # (the only switch the density pair looks at)
                    record(f"run_network rays density {what}", lambda: _ops.run_network_rays(zero_packed(_ops.PackedDensityMLP, m, prec), x["rows"], x["z"]))


def renders(name, mc, mf, x):
    """dn_render_rays with and without in-kernel compositing, once on 25 samples (must not fuse); dn_render_rays_depth."""
    from nerf import _hip, _ops
    for pname, prec in (("bf16", _hip.PREC_BF16), ("fp16", _hip.PREC_F16)):   # (the precisions that have self-compositing instances)
        pc, pf = zero_packed(_ops.PackedMLP, mc, prec), zero_packed(_ops.PackedMLP, mf, prec)
        for fused, nc in (("0", 24), ("1", 24), ("1", 25)):
            with switched({"DEXNERF_FUSED_COMPOSITE": fused} if fused == "1" else {}):
                record(f"render_rays {name} {pname} fused={fused} {nc}+24", lambda: _ops.render_rays(pc, pf, x["rows"], nc, 24, False, 0.0, False, []))
        dc, df = zero_packed(_ops.PackedDensityMLP, mc, prec), zero_packed(_ops.PackedDensityMLP, mf, prec)
        record(f"render_rays_depth {name} {pname}", lambda: _ops.render_rays_depth(dc, df, x["rows"], 24, 24, False, 0.0, None))


def train_route(name, m, x, label, prec, rays=True):
    """dn_run_network_train + dn_mlp_backward_data (+ dn_mlp_backward_input in the 32-point modes) on zero-filled buffers."""
    from nerf import _hip, _ops
    lib, ptr, dev = _ops.lib(), _ops.ptr, x["rows"].device
    arith = _hip.PREC_BF16 if prec == _hip.PREC_BF16_S8 else prec
    pk = zero_packed(_ops.PackedMLP, m, arith)
    zero_backward_stream(m, pk, prec)
    n = N_RAYS * S
    a_bytes, m_bytes, g_bytes = _ops.train_sizes(pk, n, prec=prec)
    out = torch.zeros(n, 4, device=dev)
    act, masks, grads = (torch.zeros(b, dtype=torch.uint8, device=dev) for b in (a_bytes, m_bytes, g_bytes))
    vd = x["vd"] if m.use_viewdirs else None
    args = (None, None, ptr(x["rows"]), x["rows"].shape[1], ptr(x["z"])) if rays else (ptr(x["pts"]), ptr(vd), None, 0, None)
    _ops.check(lib.dn_run_network_train(ctypes.byref(pk.desc), prec, ptr(pk.buffer), *args, N_RAYS, S, ptr(out), ptr(act), ptr(masks), _ops.stream()),
               "dn_run_network_train")
    _ops.check(lib.dn_mlp_backward_data(ctypes.byref(pk.desc), prec, ptr(pk.buffers_bwd[prec]), ptr(x["g_out"]), ptr(masks), n, ptr(grads),
                                        _ops.stream()), "dn_mlp_backward_data")
    what = f"{name} {label} {'rays' if rays else 'pts'}"
    record(f"train {what}", out, act, masks, grads)
    if prec != _hip.PREC_BF16_S8:
        _ops.ensure_input_grad_stream(m, pk)
        if rays:
            record(f"backward_input {what}", lambda: _ops.mlp_backward_input(pk, grads, N_RAYS, S, rays=x["rows"], z_vals=x["z"]))
        else:
            record(f"backward_input {what}", lambda: _ops.mlp_backward_input(pk, grads, N_RAYS, S, pts=x["pts"], viewdirs=vd))


def training(name, m, x):
    from nerf import _hip, _ops

    def route(label, prec, rays):
        try:
            train_route(name, m, x, label, prec, rays)
        except RuntimeError as e:
            OUT[f"train {name} {label} {'rays' if rays else 'pts'}"] = f"refused: {e}"

    route("fp32", _hip.PREC_F32, True)
    route("fp32", _hip.PREC_F32, False)
    route("bf16-s16", _hip.PREC_BF16, True)
    if _ops.s8_supported(_ops.PackedMLP(m.desc_kwargs(), x["rows"].device, _hip.PREC_BF16)):
        for groups in ("", "2", "3"):
            with switched({"DEXNERF_G48_TRAIN_GROUPS": groups} if groups else {}):
                route(f"s8 groups={groups or 'auto'}", _hip.PREC_BF16_S8, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="import the package of this checkout (built there) instead of this script's")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import nerf
    nerf.set_precision("fp32")
    dev = torch.device("cuda:0")
    x = inputs(dev)
    for name, kw in NETS.items():
        ma, mb = models_of(kw, dev)
        packs(name, ma, mb)
        inference(name, ma, x)
        if ma.use_viewdirs:
            renders(name, ma, mb, x)
        training(name, ma, x)
        torch.cuda.synchronize()
        print(f"{name}: {len(OUT)} calls so far", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:     # one call per line
        fh.write('{"device": %s, "sha256": {\n' % json.dumps(torch.cuda.get_device_name(0)))
        fh.write(",\n".join(f"{json.dumps(k)}: {json.dumps(OUT[k])}" for k in sorted(OUT)) + "\n}}\n")
    print(f"{len(OUT)} calls, {sum(len(v) if isinstance(v, list) else 1 for v in OUT.values())} records -> {args.out}")


if __name__ == "__main__":
    main()
