"""The training kernels' saved records per point, and their weight gradients per element, in the three training precisions
(fp32, 'bf16-s16' = PREC_BF16, 'bf16' = PREC_BF16_S8: 48-point kernels, e4m3 / e5m2 saved tensors, fp8-MFMA weight gradients).

A. A point's records do not depend on the launch around it: one column of the MFMA B operand is one point and the K order is fixed by
   the kernel, so the output row, the saved activations and the saved gradients of the first n points of a launch over N points equal
   those of a launch over these n points alone, BIT FOR BIT - on both sides of the 16-point group, the 32-point record, the 48-point
   wave and the 256- / 384-point workgroup tiles.  No tolerance.
B. Every element of every weight and bias gradient against float64 GEMMs on the operands the weight-gradient kernel itself reads
   (unpacked with dn_mlp_unpack: exact bf16 / e4m3 / e5m2 values, the e5m2 ones divided by the recorded power-of-two scale): the
   products are exact in fp32, so kernel and reference differ in the fp32 summation alone, and the gate is the project's rule for
   that (1e-5, tests/test_hip_parity.py test_weight_grad_all_equals_per_layer_launches) applied per element against the sum of the
   magnitudes of the element's terms:  |got - ref| <= 1e-5 * S,  S_W = |dY|^T |X|,  S_b = sum_p |dY|;  where S = 0 the kernel's value
   is exactly 0.  A chain of at most a few dozen fp32 additions (MFMA blocks, the tiles of a workgroup, 20 - 40 workgroup partials) is
   about 3e-6 * S in the worst case.  Plain torch fp32 dY^T X on the same operands is printed beside every kernel figure.
   The fp8 kernel alone has a gate of its own, 6.4e-4 * S: twice what one of its MFMA instructions measures against float64 in a
   stand-alone probe, because that instruction does not add its products in fp32 (GATE_FP8 below).
   The gate can see one point: removing the last point from the float64 reference changes some element of every tensor by at least
   1e-3 * S (asserted), 100 x the gate.

Slots: nerf._train._slots for the 32-point layouts, training_slots.s8_slots for the s8-48 layout."""
import math

import pytest
import torch

from training_slots import s8_slots

# (depth, width, view directions, skip): the networks of the 8-bit tests - two fixed-shape instances (D8/W256, 4x128 as shipped) and
# two run-time-shape ones
NETS = [(8, 256, True, 4), (4, 128, True, 4), (5, 128, False, 2), (3, 256, True, 2)]
MODES = {"fp32": ("fp32", "PREC_F32"), "bf16-s16": ("bf16-s16", "PREC_BF16"), "bf16": ("bf16", "PREC_BF16_S8")}
GATE = 1e-5
# The fp8 kernel alone: v_mfma_f32_32x32x64_f8f6f4 does not add its 64 products in fp32.  It aligns them to the largest and cuts every
# other one off about 15 bits below that one's leading bit, towards zero (a product 2^-15 below the largest counts for nothing) -
# measured with ONE instruction against float64 by scripts/micro/fp8_mfma_accum_probe.hip (profiles/fp8_mfma_accumulation.md):
# 3.187e-4 * sum |a b| at the worst over 1024 instructions on operands with every finite e5m2 / e4m3 byte equally likely.  The fp8 gate
# is twice the probe's figure; the probe is the reference for it, not the kernel under test.  (The bf16 and fp32 kernels stay at 1e-5:
# they measure 1.5e-7 and 3.7e-7.)  It remains below what one missing point changes (LAST_POINT_FLOOR).
FP8_MFMA_PROBE_FIGURE = 3.187e-4
GATE_FP8 = 2 * FP8_MFMA_PROBE_FIGURE
LAST_POINT_FLOOR = 1e-3
assert GATE < GATE_FP8 < LAST_POINT_FLOOR


# ---- the reference and the gate (plain torch, any device) -----------------------------------------------------------------------
def float64_reference(dy, x):
    """(dW, db, S_W, S_b) of one layer in float64: dY^T X, sum_p dY and the sums of the magnitudes of their terms."""
    dy, x = dy.double(), x.double()
    return dy.t() @ x, dy.sum(0), dy.abs().t() @ x.abs(), dy.abs().sum(0)


def gate_figure(got, ref, s):
    """(max |got - ref| / S over the elements with S > 0, whether got is exactly 0 wherever S = 0)."""
    got = got.double()
    pos = s > 0
    figure = float(((got - ref).abs()[pos] / s[pos]).max()) if bool(pos.any()) else 0.0
    return figure, bool((got[~pos] == 0).all())


def last_point_share(dy, x):
    """What removing the last point changes in the float64 reference, as max |term| / S per tensor: (dW, db)."""
    dy, x = dy.double(), x.double()
    _, _, s_w, s_b = float64_reference(dy, x)
    t_w = dy[-1].abs()[:, None] * x[-1].abs()[None, :]
    t_b = dy[-1].abs()
    share = lambda t, s: float((t[s > 0] / s[s > 0]).max()) if bool((s > 0).any()) else 0.0   # noqa: E731
    return share(t_w, s_w), share(t_b, s_b)


def _record_measurement(key, values):
    """Measured figures behind a gate, appended to the suite's measurement record: the recorder of tests/test_hip_parity.py, so that
    the place and the format are said once."""
    from test_hip_parity import _record_measurement as record
    record(key, values)


# ---- CPU: the yardstick itself ---------------------------------------------------------------------------------------------------
def _synthetic_operands(n, n_out, k, fmt, gen):
    """ReLU-masked dY and X with exactly representable entries (bf16 x bf16, or e5m2 / 2^16 x e4m3), the last point and the first at
    the largest upstream magnitude."""
    dy = torch.randn(n, n_out, generator=gen) * 1e-4 * (torch.rand(n, n_out, generator=gen) < 0.5)
    x = torch.randn(n, k, generator=gen).clamp_min(0.0)
    top = dy.abs().max()
    for row in (0, n - 1):
        sign = torch.where(torch.randn(n_out, generator=gen) < 0, -1.0, 1.0)
        dy[row] = sign * top
    if fmt == "bf16":
        return dy.bfloat16().float(), x.bfloat16().float()
    return (dy * 65536.0).to(torch.float8_e5m2).float() / 65536.0, x.to(torch.float8_e4m3fn).float()


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_float64_reference_gate_and_last_point_condition_on_synthetic_operands(fmt):
    """The yardstick without a GPU, on synthetic operands of the layer shapes the kernels have (256x319, 128x283, 128x128, 64x155 and
    the 3- / 1-row heads) and the point counts of the GPU test:
      * plain fp32 dY^T X and sum dY pass the gate against the float64 reference with a wide margin (1.1e-7 * S at the worst measured;
        asserted at 1e-6, a tenth of the gate);
      * the last point weighs >= 1e-3 * S in some element of every tensor (3.6e-3 at the least, a bias gradient over 2077 points);
      * both gates notice what the cosine checks did not: the last 16-point group's gradient rows zeroed, a doubled db."""
    gen = torch.Generator().manual_seed(7)
    worst, floor = 0.0, 1.0
    for n_out, k in ((256, 319), (128, 283), (128, 128), (64, 155), (3, 128), (1, 256)):
        for n in (1, 31, 32, 33, 65, 777, 2077):
            dy, x = _synthetic_operands(n, n_out, k, fmt, gen)
            ref_w, ref_b, s_w, s_b = float64_reference(dy, x)
            fig_w, zero_w = gate_figure(dy.t() @ x, ref_w, s_w)
            fig_b, zero_b = gate_figure(dy.sum(0), ref_b, s_b)
            assert zero_w and zero_b and max(fig_w, fig_b) <= 1e-6, (n_out, k, n, fig_w, fig_b)
            worst = max(worst, fig_w, fig_b)
            share_w, share_b = last_point_share(dy, x)
            assert min(share_w, share_b) >= LAST_POINT_FLOOR, (n_out, k, n, share_w, share_b)
            floor = min(floor, share_w, share_b)
            # a kernel that dropped the ragged last 16-point group, or added db twice, gives these:
            cut = dy.clone()
            cut[(n - 1) // 16 * 16:] = 0
            assert gate_figure(cut.double().t() @ x.double(), ref_w, s_w)[0] > GATE_FP8 > GATE
            assert gate_figure(cut.double().sum(0), ref_b, s_b)[0] > GATE_FP8
            if float(ref_b.abs().max()) > 0:
                assert gate_figure(2 * ref_b, ref_b, s_b)[0] > GATE_FP8
    print(f"{fmt}: fp32 torch against float64 {worst:.3e} * S at the worst; the last point's share >= {floor:.3e}")


def test_gate_wants_an_exact_zero_where_no_term_exists():
    dy = torch.tensor([[1.0, 0.0], [2.0, 0.0]])
    x = torch.tensor([[1.0, 0.0, 3.0], [0.5, 0.0, 1.0]])
    ref_w, ref_b, s_w, s_b = float64_reference(dy, x)
    assert gate_figure(ref_w.float(), ref_w, s_w) == (0.0, True) and gate_figure(ref_b.float(), ref_b, s_b) == (0.0, True)
    off = ref_w.clone()
    off[1, 1] = 1e-30
    assert gate_figure(off, ref_w, s_w) == (0.0, False)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


def _restore_defaults():
    import nerf
    from nerf import _ops
    nerf.set_precision("fp32")
    nerf.set_s8_grad_scale(0.0)
    _ops.set_deterministic_weight_gradients(True)


def _network(net, mode, dev, seed=3):
    """(model, packed streams, precision code) of NETS entry `net` for training mode `mode`."""
    import nerf
    from nerf import _hip, _ops
    depth, width, viewdirs, skip = net
    nerf.set_precision(MODES[mode][0])
    prec = getattr(_hip, MODES[mode][1])
    torch.manual_seed(seed)
    m = nerf.models.FlexibleNeRFModel(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=10,
                                      num_encoding_fn_dir=4, use_viewdirs=viewdirs).to(dev)
    pk = m.packed()
    _ops.pack_backward(pk, [x.weight for x in m.linear_modules()], prec)
    if prec == _hip.PREC_BF16_S8:
        assert _ops.s8_supported(pk)
    return m, pk, prec


def _records(m, pk, prec, act, grads, n):
    """Every saved activation and every saved gradient of a launch over n points as plain (n, width) fp32 rows, by name, through
    dn_mlp_unpack.  'out' is the custom output-gradient unit in the order [d rgb (3) | d alpha] (or [d out (4)]): kind 3 in the
    8-bit layout; in the 32-point layouts one piece each for d rgb and d alpha, element e of lane half 0 = row e, which the hidden-vector
    unpacker (kind 0, one piece wide) puts in column e."""
    from nerf import _hip, _ops, _train
    dev = act.device
    d, w, view = m.num_layers, m.hidden_size, m.use_viewdirs

    def rows(which, buf, slot, width, kind=0, cols=None):
        out = torch.zeros((n, cols or width), dtype=torch.float32, device=dev)
        return _ops.mlp_unpack(pk, which, buf, n, slot, width, kind, out, prec=prec)

    if prec == _hip.PREC_BF16_S8:
        s, g, kh = s8_slots(d, w, view)
        wdir = max(w // 2, 64)              # (a W = 128 net's 64-wide layers_dir.0: one 64-feature unit)
        custom = rows(1, grads, g["out"], 8, 3, cols=8)
        g_out = custom[:, [0, 1, 2, 4]] if view else custom[:, :4]
    else:
        s, g, kh = _train._slots(m, prec)
        wdir = w // 2
        kpp = 16 if prec == _hip.PREC_BF16 else 8
        if view:
            g_out = torch.cat((rows(1, grads, g["out"], kpp)[:, :3], rows(1, grads, g["out"] + 1, kpp)[:, :1]), -1)
        else:
            g_out = rows(1, grads, g["out"], kpp)[:, :4]
    acts = {"xyz": rows(0, act, s["xyz"], m.dim_xyz, 1)}
    if view:
        acts["dir"] = rows(0, act, s["dir"], m.dim_dir, 2)
    acts["layer1"] = rows(0, act, s["layer1"], w)
    grds = {"layer1": rows(1, grads, g["layer1"], w)}
    for i in range(d - 1):
        acts[f"trunk{i}"] = rows(0, act, s["trunk0"] + i * kh, w)
        grds[f"trunk{i}"] = rows(1, grads, g["trunk0"] + i * kh, w)
    if view:
        acts["feat"] = rows(0, act, s["feat"], w)
        grds["feat"] = rows(1, grads, g["feat"], w)
        acts["dirout"] = rows(0, act, s["dirout"], wdir)[:, : w // 2]
        grds["dirout"] = rows(1, grads, g["dirout"], wdir)[:, : w // 2]
    grds["out"] = g_out.contiguous()
    return acts, grds


def _forward_backward(pk, prec, pts, vd, spr, g_out):
    from nerf import _ops
    n = pts.shape[0]
    out, act, masks = _ops.run_network_train(pk, pts, vd, spr, prec=prec)
    grads = _ops.mlp_backward_data(pk, g_out, masks, n, prec=prec)
    return out, act, grads


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- A ---------------------------------------------------------------------------------------------------------------------------
PREFIXES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 383, 384, 385, 769)
PREFIXES_19 = (19, 247, 266, 380, 399)          # whole rays of 19 samples
RECORD_CASES = [(mode, net, None) for mode in MODES for net in NETS] + \
               [("bf16", net, groups) for net in NETS[:2] for groups in ("2", "3")]     # the two fixed shapes' 256- and 384-point tiles


@pytest.mark.gpu
@pytest.mark.parametrize("mode,net,groups", RECORD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_a_points_records_do_not_depend_on_the_launch_around_it(dev, monkeypatch, mode, net, groups):
    """Forward + backward on N = 800 fixed points (one sample per ray: every prefix is a whole number of rays), then on each prefix of
    n points: the rows [0:n] of the raw output, of every saved activation (xyz panel, view-direction panel, layer1, each trunk layer,
    fc_feat, layers_dir.0) and of every saved gradient (incl. the custom output-gradient unit) are the long launch's rows, bit for
    bit.  The same with 19 samples per ray (the view direction of a point is its ray's).  8-bit mode: the fixed scale 2^16, so that the
    scale does not depend on the prefix; the two fixed shapes also with DEXNERF_G48_TRAIN_GROUPS forced to 2 and to 3 (256- and
    384-point workgroup tiles).  Rows >= n are padding and not compared."""
    import nerf
    try:
        m, pk, prec = _network(net, mode, dev)
        nerf.set_s8_grad_scale(65536.0)
        if groups is not None:
            monkeypatch.setenv("DEXNERF_G48_TRAIN_GROUPS", groups)
        gen = torch.Generator(device=dev).manual_seed(800)
        n_long = 800
        pts = torch.rand(n_long, 3, device=dev, generator=gen) * 2 - 1
        dirs = torch.nn.functional.normalize(torch.randn(n_long, 3, device=dev, generator=gen), dim=-1)
        g_out = torch.randn(n_long, 4, device=dev, generator=gen) * 1e-4

        def launch(n, spr):
            vd = dirs[: n // spr].contiguous() if m.use_viewdirs else None
            out, act, grads = _forward_backward(pk, prec, pts[:n].contiguous(), vd, spr, g_out[:n].contiguous())
            acts, grds = _records(m, pk, prec, act, grads, n)
            return {"out": out, "act": torch.cat(list(acts.values()), -1), "grads": torch.cat(list(grds.values()), -1)}, acts, grds

        for spr, n_whole, prefixes in ((1, n_long, PREFIXES), (19, 19 * 42, PREFIXES_19)):
            whole, acts, grds = launch(n_whole, spr)
            for name, t in list(acts.items()) + list(grds.items()) + [("out", whole["out"])]:
                assert not bool(torch.isnan(t).any()) and float(t.abs().max()) > 0, (name, spr)
            for n in prefixes:
                part, _, _ = launch(n, spr)
                for what in ("out", "act", "grads"):
                    a, b = part[what], whole[what][:n]
                    assert a.shape == b.shape and not bool(torch.isnan(a).any()) and float(a.abs().max()) > 0, (what, n, spr)
                    if not _same_bits(a, b):
                        bad = (a.view(torch.int32) != b.contiguous().view(torch.int32)).nonzero()
                        raise AssertionError(f"{what}: a launch over {n} points ({spr} per ray) differs from the first {n} of {n_whole} in "
                                             f"{bad.shape[0]} elements, the first at (point, column) {bad[0].tolist()}")
                    # (the comparison is of these points' rows: the long launch's rows one point further on are other bits)
                    assert not _same_bits(a, whole[what][1:n + 1]), (what, n, spr)
    finally:
        _restore_defaults()


@pytest.mark.gpu
def test_per_launch_scale_is_taken_from_the_largest_upstream_gradient_wherever_it_sits(dev):
    """Scale 0 = per launch: the recorded scale is 2^(12 - ceil(log2(max |g_out|))) (csrc/mlp_train48.hip) with the maximum at the
    first point and at the last point of a ragged launch (777 points: the last float4 row of the reduction kernel's last block)."""
    import nerf
    from nerf import _ops
    try:
        m, pk, prec = _network(NETS[1], "bf16", dev)
        nerf.set_s8_grad_scale(0.0)
        n_rays, spr = 37, 21
        n = n_rays * spr
        gen = torch.Generator(device=dev).manual_seed(777)
        pts = torch.rand(n, 3, device=dev, generator=gen) * 2 - 1
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev, generator=gen), dim=-1)
        base = torch.randn(n, 4, device=dev, generator=gen) * 1e-4
        _, _, masks = _ops.run_network_train(pk, pts, vd, spr, prec=prec)
        for (row, col), top in (((0, 2), 3.0e-3), ((n - 1, 1), -0.7)):
            g_out = base.clone()
            g_out[row, col] = top
            assert float(g_out.abs().max()) == abs(float(g_out[row, col]))
            grads = _ops.mlp_backward_data(pk, g_out, masks, n, prec=prec)
            want = 2.0 ** (12 - math.ceil(math.log2(abs(float(g_out[row, col])))))
            assert nerf.s8_grad_stats(grads)["scale"] == [want], (row, col, top, nerf.s8_grad_stats(grads), want)
    finally:
        _restore_defaults()


# ---- B ---------------------------------------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 31, 32, 33, 65, 777, 2077)   # 65: a tile pair lacks its second tile; 2077: workgroups stride, 29 points in the last tile


def _units(m, acts, grds):
    """(module, dY, X) of every (dW, db) unit as wg_add_network (csrc/mlp_wgrad.hip) lists them."""
    xyz = acts["xyz"]
    units = [(m.layer1, grds["layer1"], xyz)]
    prev = acts["layer1"]
    for i, layer in enumerate(m.layers_xyz):
        units.append((layer, grds[f"trunk{i}"], torch.cat((prev, xyz), -1) if i in m.skip_layers else prev))
        prev = acts[f"trunk{i}"]
    if m.use_viewdirs:
        units.append((m.layers_dir[0], grds["dirout"], torch.cat((acts["feat"], acts["dir"]), -1)))
        units.append((m.fc_alpha, grds["out"][:, 3:4], prev))
        units.append((m.fc_rgb, grds["out"][:, :3], acts["dirout"]))
        units.append((m.fc_feat, grds["feat"], prev))
    else:
        units.append((m.fc_out, grds["out"], prev))
    return units


def _gate_of(prec):
    from nerf import _hip
    return GATE_FP8 if prec == _hip.PREC_BF16_S8 else GATE


def _check_units(units, results, what, gate, want_last_point=True):
    """Gate every (dW, db) of `results` (module -> (dW, db)) against the float64 reference of its unit; returns the worst kernel figure,
    the worst figure of plain torch fp32 on the same operands and the smallest last-point share."""
    worst, worst_torch, floor = 0.0, 0.0, 1.0
    for mod, dy, x in units:
        d_w, d_b = results[mod]
        name = f"{what} {tuple(mod.weight.shape)}"
        assert d_w.shape == mod.weight.shape and d_b.shape == mod.bias.shape
        ref_w, ref_b, s_w, s_b = float64_reference(dy, x)
        assert float(s_w.max()) > 0 and float(s_b.max()) > 0, name
        if want_last_point:
            share_w, share_b = last_point_share(dy, x)
            assert min(share_w, share_b) >= LAST_POINT_FLOOR, (name, share_w, share_b)
            floor = min(floor, share_w, share_b)
        for tag, got, ref, s, plain in (("dW", d_w, ref_w, s_w, dy.t() @ x), ("db", d_b, ref_b, s_b, dy.sum(0))):
            assert bool(torch.isfinite(got).all()), (name, tag)
            figure, zeros = gate_figure(got, ref, s)
            figure_torch, _ = gate_figure(plain, ref, s)
            worst, worst_torch = max(worst, figure), max(worst_torch, figure_torch)
            if not (zeros and figure <= gate):
                err = (got.double() - ref).abs() / s.clamp_min(1e-300)
                at = int(torch.where(s > 0, err, torch.zeros_like(err)).argmax())
                raise AssertionError(f"{name} {tag}: |got - ref| = {figure:.3e} * S at the worst (gate {gate:.3e}; flat element {at}; plain "
                                     f"torch fp32 {figure_torch:.3e} * S), exact zeros where S = 0: {zeros}")
    return worst, worst_torch, floor


def _inputs(m, n, spr, dev, seed):
    """n points in n / spr rays; g_out ~ 1e-4 randn with the first and the last point at the batch's largest magnitude."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    pts = torch.rand(n, 3, device=dev, generator=gen) * 2 - 1
    vd = torch.nn.functional.normalize(torch.randn(n // spr, 3, device=dev, generator=gen), dim=-1) if m.use_viewdirs else None
    g_out = torch.randn(n, 4, device=dev, generator=gen) * 1e-4
    top = g_out.abs().max()
    for row in (0, n - 1):
        g_out[row] = torch.where(g_out[row] < 0, -top, top)
    return pts, vd, g_out


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("mode", list(MODES))
def test_weight_and_bias_gradients_every_element_against_float64_on_the_kernels_own_operands(dev, mode, net):
    """dn_mlp_weight_grad_all (deterministic two-phase reduction) in every precision, on every network and n in POINT_COUNTS; the
    8-bit mode once with the fixed scale 2^16 and once with the per-launch scale (the kernel divides by the scale the backward
    recorded; the unpacker does too, exactly: a power of two).  dY and X of every unit are what the kernel reads, unpacked; nothing is
    restated - the 32-point layouts' custom piece is unpacked like a hidden piece, and additionally asserted to be g_out (fp32) or
    g_out rounded to bf16.
    Launches (wg_launch_batch): fp32 weight_grad_batch_kernel_f32; bf16-s16 weight_grad_batch_kernel; 8-bit: 4x128 and 5x128 (every unit
    a small shape) weight_grad_batch_kernel_s8_small, two workgroups per CU; D8/W256 and 3x256 weight_grad_batch_kernel_s8.
    Gate: 1e-5 * S (fp32, bf16-s16); the fp8 kernel 6.374e-4 * S = twice what ONE of its MFMA instructions measures against float64
    (GATE_FP8 above: the instruction cuts products off about 15 bits below the largest of its 64).
    Measured on an MI355X, worst element of all tensors, n and scales, in units of S (kernel | plain torch fp32 on the same operands):
      fp32      D8/W256 3.2e-7 | 3.9e-7   4x128 2.6e-7 | 2.8e-7   5x128 2.9e-7 | 2.9e-7   3x256 3.7e-7 | 3.7e-7
      bf16-s16  D8/W256 1.5e-7 | 2.9e-7   4x128 1.0e-7 | 1.8e-7   5x128 9.2e-8 | 2.1e-7   3x256 1.1e-7 | 2.2e-7
      bf16      D8/W256 3.9e-4 | 5.9e-8   4x128 1.7e-4 | 3.3e-8   5x128 9.9e-5 | 3.0e-8   3x256 5.0e-4 | 4.6e-8
    (fp8: in a few per cent of the elements, spread over most rows and columns of every layer at every n - profiles/fp8_mfma_accumulation.md);
    the last point's share of some element of every tensor >= 2.4e-3 * S."""
    import nerf
    from nerf import _hip, _ops
    try:
        m, pk, prec = _network(net, mode, dev)
        mods = m.linear_modules()
        shapes = [tuple(x.weight.shape) for x in mods]
        worst, worst_torch, floor = 0.0, 0.0, 1.0
        for scale in ((65536.0, 0.0) if prec == _hip.PREC_BF16_S8 else (0.0,)):
            nerf.set_s8_grad_scale(scale)
            for n in POINT_COUNTS:
                spr = 31 if n == 2077 else (21 if n == 777 else 1)
                pts, vd, g_out = _inputs(m, n, spr, dev, seed=n)
                _, act, grads = _forward_backward(pk, prec, pts, vd, spr, g_out)
                results = dict(zip(mods, _ops.mlp_weight_grad_all(pk, act, grads, n, shapes, prec=prec)))
                acts, grds = _records(m, pk, prec, act, grads, n)
                if prec == _hip.PREC_F32:
                    assert torch.equal(grds["out"], g_out)
                elif prec == _hip.PREC_BF16:
                    assert torch.equal(grds["out"], g_out.bfloat16().float())
                w, wt, fl = _check_units(_units(m, acts, grds), results, f"{mode} {net} n={n} scale={scale}", _gate_of(prec))
                worst, worst_torch, floor = max(worst, w), max(worst_torch, wt), min(floor, fl)
        print(f"weight gradients {mode} {net}: {worst:.3e} * S at the worst (plain torch fp32 {worst_torch:.3e} * S); the last point's "
              f"share >= {floor:.3e}")
        _record_measurement(f"wgrad_float64_{mode}_{'x'.join(map(str, net))}", dict(kernel=worst, torch_fp32=worst_torch, last_point=floor))
    finally:
        _restore_defaults()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_weight_gradient_launch_forms_against_the_same_reference(dev, mode):
    """4x128, 777 points, one set of saved buffers, one float64 reference and gate: dn_mlp_weight_grad_all with the deterministic
    two-phase reduction and with fp32 atomics (set_deterministic_weight_gradients(False)), and in the 16-bit mode the per-layer
    dn_mlp_weight_grad launches.  Measured on an MI355X, in units of S: fp32 two-phase 1.5e-7, atomics 1.5e-7 (plain torch fp32
    3.1e-7); bf16-s16 7.7e-8, 7.7e-8, per-layer launches 1.3e-7 (1.2e-7); bf16 (weight_grad_batch_kernel_s8_small) 3.7e-5, 3.7e-5
    (2.5e-8)."""
    from nerf import _hip, _ops, _train
    try:
        net = NETS[1]
        m, pk, prec = _network(net, mode, dev)
        mods = m.linear_modules()
        shapes = [tuple(x.weight.shape) for x in mods]
        n, spr = 777, 21
        pts, vd, g_out = _inputs(m, n, spr, dev, seed=5)
        _, act, grads = _forward_backward(pk, prec, pts, vd, spr, g_out)
        acts, grds = _records(m, pk, prec, act, grads, n)
        units = _units(m, acts, grds)
        figures = {}
        for form, deterministic in (("two_phase", True), ("atomics", False)):
            _ops.set_deterministic_weight_gradients(deterministic)
            results = dict(zip(mods, _ops.mlp_weight_grad_all(pk, act, grads, n, shapes, prec=prec)))
            figures[form], figures["torch_fp32"], _ = _check_units(units, results, f"{mode} {form}", _gate_of(prec))
        if prec == _hip.PREC_BF16:
            slots, gslots, kh = _train._slots(m, prec)
            w = m.hidden_size
            per_layer = {}

            def one(mod, g_slot, n_out, x_slot, x_width, pe_kind):
                d_w, d_b = torch.zeros_like(mod.weight), torch.zeros_like(mod.bias)
                _ops.mlp_weight_grad(pk, act, grads, n, g_slot, n_out, x_slot, x_width, pe_kind, d_w, d_b)
                per_layer[mod] = (d_w, d_b)

            one(m.layer1, gslots["layer1"], w, 0, 0, 1)
            x_slot = slots["layer1"]
            for i, layer in enumerate(m.layers_xyz):
                one(layer, gslots["trunk0"] + i * kh, w, x_slot, w, 1 if i in m.skip_layers else 0)
                x_slot = slots["trunk0"] + i * kh
            one(m.fc_feat, gslots["feat"], w, x_slot, w, 0)
            one(m.fc_alpha, gslots["out"] + 1, 1, x_slot, w, 0)
            one(m.layers_dir[0], gslots["dirout"], w // 2, slots["feat"], w, 2)
            one(m.fc_rgb, gslots["out"], 3, slots["dirout"], w // 2, 0)
            figures["per_layer"], _, _ = _check_units(units, per_layer, f"{mode} per-layer launches", GATE)
        print(f"launch forms {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()) + " (* S)")
        _record_measurement(f"wgrad_launch_forms_{mode}", figures)
    finally:
        _restore_defaults()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_two_network_weight_gradient_launch_with_different_point_counts(dev, mode):
    """dn_mlp_weight_grad_pair_ws as the training step reaches it: dn_render_rays_backward on both networks of one architecture
    (4x128) runs the two backward-data chains and then ONE weight-gradient launch over the units of both (csrc/api.cpp).  One ray with
    65 coarse + 712 fine samples gives the batch 777 points for the fine network's units and 65 - an odd tile count - for the coarse
    one's.  Both networks' gradients against the float64 reference on the buffers that call left behind, same gate.  (The upstream
    gradient is the compositing backward's, so the last point carries no planted maximum: its share is not asserted here.)
    Measured on an MI355X, in units of S, coarse / fine (plain torch fp32): fp32 3.3e-7 / 2.6e-7 (4.4e-7 / 1.7e-6); bf16-s16 1.3e-7 /
    1.5e-7 (2.0e-7 / 2.3e-6); bf16 5.1e-5 / 3.1e-5 (6.3e-8 / 1.3e-7)."""
    import nerf
    from nerf import _hip, _ops
    try:
        nerf.set_precision(MODES[mode][0])
        depth, width, viewdirs, skip = NETS[1]
        nets = []
        for seed in (3, 4):
            torch.manual_seed(seed)
            nets.append(nerf.models.FlexibleNeRFModel(num_layers=depth, hidden_size=width, skip_connect_every=skip, num_encoding_fn_xyz=10,
                                                      num_encoding_fn_dir=4, use_viewdirs=viewdirs).to(dev))
            with torch.no_grad():
                nets[-1].fc_alpha.bias.fill_(1.0)      # density > 0 along the ray: every sample has a gradient
        mc, mf = nets
        pc, pf, prec = _ops.pack_train_pair(mc, mf, (True, True))
        assert prec == getattr(_hip, MODES[mode][1])
        nc, nf = 65, 712
        rd = torch.nn.functional.normalize(torch.tensor([[0.3, -0.5, 0.8]]), dim=-1)
        rows = torch.cat((torch.tensor([[0.1, -0.2, -0.9]]), rd, torch.tensor([[0.2, 1.8]]), rd), -1).to(dev)
        maps, saved = _ops.render_rays_train(pc, pf, rows, nc, nf, False, 0.0, False, [], None, prec=prec)
        views = [_ops.zeroed_grad_views([tuple(x.weight.shape) for x in net.linear_modules()], dev) for net in nets]
        g_c, g_f = torch.tensor([[0.7, -1.1, 0.4]], device=dev), torch.tensor([[-0.9, 0.6, 1.3]], device=dev)
        grads_c, grads_f, *keep = _ops.render_rays_backward(pc, pf, saved, (g_c, None, None), (g_f, None, None), views[0], views[1], nets=3)
        figures = {}
        for tag, net, pk, act, grads, n, view in (("coarse", mc, pc, saved["act_c"], grads_c, nc, views[0]),
                                                  ("fine", mf, pf, saved["act_f"], grads_f, nc + nf, views[1])):
            acts, grds = _records(net, pk, prec, act, grads, n)
            figures[tag], figures[tag + "_torch_fp32"], _ = _check_units(_units(net, acts, grds), dict(zip(net.linear_modules(), view)),
                                                                         f"{mode} pair launch, {tag} network ({n} points)", _gate_of(prec),
                                                                         want_last_point=False)
        print(f"two-network launch {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()) + " (* S)")
        _record_measurement(f"wgrad_pair_{mode}", figures)
    finally:
        _restore_defaults()
