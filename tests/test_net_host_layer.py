"""The host layer between the Python package and the network kernels (csrc/mlp_geo48.h, mlp_internal.h): instance selection of the
48-point forward family, checked without a GPU, and the merged single / pair pack launchers, checked on one."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import PKG


def test_g48_pick_reaches_every_instance_and_nothing_else():
    """csrc/g48_pick_check.cpp (make check): g48_pick over descriptors x precisions x inference / training x input modes x samples per
    ray x launch sizes x switches returns only rows of DN_FWD48_INSTANCES / DN_FWD48_DENSITY, and every one of the 22 + 4 rows at least
    once.  Host code only; fails (does not skip) without the compiler, which build() needs anyway."""
    run = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "check"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "26 rows, 0 unknown keys, 0 unreached rows" in run.stdout, run.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("depth,width,lxyz", [(4, 128, 6), (8, 256, 10)])
def test_pair_pack_equals_per_network_pack(depth, width, lxyz):
    """The streams a DN_PREC_BF16_S8 training step reads, packed per network (dn_mlp_pack_parts(ALL) + dn_mlp_pack_backward(BF16_S8))
    and by the pair call (dn_mlp_pack_parts(CORE) + dn_mlp_pack_train_pair): both buffers of both networks are equal, byte for
    byte, from zero-filled buffers.  The two routes share one launcher body per stream."""
    import nerf
    from nerf import _hip, _ops
    dev = torch.device("cuda:0")
    S8 = _hip.PREC_BF16_S8
    models, single, pair = [], [], []
    for seed in (1, 2):
        torch.manual_seed(seed)
        m = nerf.models.FlexibleNeRFModel(num_layers=depth, hidden_size=width, skip_connect_every=4, num_encoding_fn_xyz=lxyz,
                                          num_encoding_fn_dir=4, use_viewdirs=True).to(dev)
        models.append(m)
        weights, biases = [x.weight for x in m.linear_modules()], [x.bias for x in m.linear_modules()]
        for route, parts in ((single, _hip.PACK_ALL), (pair, _hip.PACK_CORE)):
            pk = _ops.PackedMLP(m.desc_kwargs(), dev, _hip.PREC_BF16)
            pk.buffer.zero_()
            pk.buffers_bwd[S8] = torch.zeros(_ops.lib().dn_mlp_backward_packed_bytes(ctypes.byref(pk.desc), S8), dtype=torch.uint8, device=dev)
            assert pk.buffers_bwd[S8].numel() > 0
            pk.pack(weights, biases, parts)
            route.append(pk)
        _ops.pack_backward(single[-1], weights, S8)
    arrays = []
    for m in models:
        arrays.append(_ops._ptr_array([x.weight for x in m.linear_modules()], sources=True))
        arrays.append(_ops._ptr_array([x.bias for x in m.linear_modules()], sources=True))
    pa, pb = pair
    _ops.check(_ops.lib().dn_mlp_pack_train_pair(ctypes.byref(pa.desc), arrays[0][0], arrays[1][0], _ops.ptr(pa.buffer), _ops.ptr(pa.buffers_bwd[S8]),
                                                 arrays[2][0], arrays[3][0], _ops.ptr(pb.buffer), _ops.ptr(pb.buffers_bwd[S8]), _ops.stream()),
               "dn_mlp_pack_train_pair")
    torch.cuda.synchronize()
    for one, two in zip(single, pair):
        assert one.buffer.any() and one.buffers_bwd[S8].any()
        assert torch.equal(one.buffer, two.buffer)
        assert torch.equal(one.buffers_bwd[S8], two.buffers_bwd[S8])
