"""The no-grad render drivers of nerf/train_utils.py (predict_and_render_radiance called directly, run_one_iter_of_nerf and
render_dex_depth over several chunks) under the guarded-fp16 render policy, and the per-stream status words of nerf/_ops.py.

All on the 192 rays of the reference-recorded golden `render_d8w256_val` (D8/W256, 64+128 samples: the smallest fixed-shape case
whose kernel instances carry the fp16 range tracker); chunksize 64 gives three chunks - a first, a middle and a last.  Everything
compared here is the same arithmetic on the same inputs, so every comparison is bit for bit."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from golden_cases import CASES, M_THRES

pytestmark = pytest.mark.gpu

NAME = "render_d8w256_val"
WARNING = "fp16 render produced non-finite"


@pytest.fixture(scope="module")
def scene(golden):
    """(coarse net, fine net, ro (1,192,3), rd (1,192,3), embedders, render settings) - built once for the module."""
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()   # must load: no fallback
    dev = torch.device("cuda:0")
    g = golden(NAME)
    mkw, wfn, rkw = CASES[NAME]
    models = []
    for sd in wfn():
        m = nerf.models.FlexibleNeRFModel(**mkw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        models.append(m.to(dev))
    ro = torch.from_numpy(np.ascontiguousarray(g["ro"])).to(dev)[None]
    rd = torch.from_numpy(np.ascontiguousarray(g["rd"])).to(dev)[None]
    return models[0], models[1], ro, rd, (nerf.get_embedding_function(10), nerf.get_embedding_function(4)), rkw


def make_cfg(rkw, chunksize, **over):
    import nerf
    mode = dict(chunksize=chunksize, lindisp=False, num_coarse=rkw["num_coarse"], num_fine=rkw["num_fine"], perturb=False,
                radiance_field_noise_std=0.0, white_background=False)
    mode.update(over)
    return nerf.CfgNode(dict(dataset=dict(near=rkw["near"], far=rkw["far"], no_ndc=True),
                             nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode))))


@contextlib.contextmanager
def bf16_mode(mf, overflow):
    """Precision 'bf16'; overflow: the existing overflow fixture on the fine net (weights stay inside fp16, the layer's outputs
    ~1e5 do not; nothing for bf16).  Weights, precision, render policy and the process-wide fp16 switch are restored on exit."""
    import nerf
    from nerf import train_utils
    saved = mf.layers_xyz[2].weight.detach().clone()
    try:
        nerf.set_precision("bf16")
        if overflow:
            with torch.no_grad():
                mf.layers_xyz[2].weight.mul_(3.0e4)
            nerf.models.mark_parameters_updated()
        yield
    finally:
        with torch.no_grad():
            mf.layers_xyz[2].weight.copy_(saved)
        nerf.models.mark_parameters_updated()
        nerf.set_precision("fp32")
        nerf.set_render_policy(None)
        train_utils._FP16_RENDER_DISABLED[0] = False


def assert_same_maps(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a, b)


def one_range_warning_at_this_file(caught):
    hits = [w for w in caught if WARNING in str(w.message)]
    assert len(hits) == 1
    assert hits[0].filename == __file__   # (stacklevel: the warning names the line that asked for the render)


def test_direct_chunk_render_repeats_in_bf16_on_the_same_draws(scene):
    """predict_and_render_radiance called directly checks its own chunk: one host read, one warning, and the bf16 repeat runs on
    the draws the fp16 attempt consumed - so it equals the policy-'bf16' render of the same seed bit for bit."""
    import nerf
    from nerf import _ops, train_utils
    mc, mf, ro, rd, (ex, ed), rkw = scene
    cfg = make_cfg(rkw, 4096, perturb=True, radiance_field_noise_std=1.0)
    rows = _ops.pack_ray_rows(ro[0], rd[0], rd[0], rkw["near"], rkw["far"])

    def render():
        torch.manual_seed(5)
        with torch.no_grad():
            return nerf.predict_and_render_radiance(rows, mc, mf, cfg, mode="validation", encode_position_fn=ex,
                                                    encode_direction_fn=ed, m_thres_cand=list(M_THRES))
    with bf16_mode(mf, overflow=True):
        nerf.set_render_policy("fp16")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            guarded = render()
        one_range_warning_at_this_file(caught)
        assert train_utils._FP16_RENDER_DISABLED[0]
        nerf.set_render_policy("bf16")
        assert_same_maps(guarded, render())
        assert len(guarded) == 6 + len(M_THRES) and bool(torch.isfinite(guarded[3]).all())


def image_render(scene, chunksize=64):
    import nerf
    mc, mf, ro, rd, (ex, ed), rkw = scene
    with torch.no_grad():
        return nerf.run_one_iter_of_nerf(1, ro.shape[1], 1.0, mc, mf, ro, rd, make_cfg(rkw, chunksize), mode="validation",
                                         encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=list(M_THRES))


def depth_render(scene, chunksize=64):
    import nerf
    mc, mf, ro, rd, (ex, ed), rkw = scene
    with torch.no_grad():
        return nerf.render_dex_depth(1, ro.shape[1], 1.0, mc, mf, ro, rd, make_cfg(rkw, chunksize), mode="validation",
                                     encode_position_fn=ex, encode_direction_fn=ed, m_thres_cand=list(M_THRES))


@pytest.mark.parametrize("render", [image_render, depth_render])
def test_three_chunks_one_read_one_warning_then_bf16(scene, render):
    """Overflow weights, three chunks: the status words of all chunks are read once - ONE warning - and the whole call is
    rendered again in bf16: equal to the policy-'bf16' render at the same chunk size."""
    import nerf
    from nerf import train_utils
    mf = scene[1]
    with bf16_mode(mf, overflow=True):
        nerf.set_render_policy("fp16")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            guarded = render(scene)
        one_range_warning_at_this_file(caught)
        assert train_utils._FP16_RENDER_DISABLED[0]
        nerf.set_render_policy("bf16")
        assert_same_maps(guarded, render(scene))
        assert guarded[-1].shape == (1, 192)


@pytest.mark.parametrize("render", [image_render, depth_render])
def test_three_chunks_healthy_weights_stay_in_fp16(scene, render):
    """Healthy weights: no warning, and the render under 'bf16' + policy 'fp16' is the 'fp16'-mode render at the same chunk size."""
    import nerf
    mf = scene[1]
    with bf16_mode(mf, overflow=False):
        nerf.set_render_policy("fp16")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            pol = render(scene)
        nerf.set_precision("fp16")
        assert_same_maps(pol, render(scene))


def test_status_words_belong_to_the_stream_that_rendered(scene):
    """render_status_words() / render_nonfinite_count() without an argument read the latest render of the CURRENT stream: a clean
    render on a side stream, then an overflowing one on the default stream - positive there, still zero on the side stream."""
    import nerf
    from nerf import _hip, _ops
    mc, mf, ro, rd, _, rkw = scene
    rows = _ops.pack_ray_rows(ro[0, :8], rd[0, :8], rd[0, :8], rkw["near"], rkw["far"])
    side = torch.cuda.Stream()

    def render():
        with torch.no_grad():
            _ops.render_rays(mc.packed(), mf.packed(), rows, rkw["num_coarse"], rkw["num_fine"], False, 0.0, False, list(M_THRES))
    with bf16_mode(mf, overflow=False):
        nerf.set_precision("fp16")
        assert mc.packed().precision == _hip.PREC_F16
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            render()
            assert _ops.render_nonfinite_count() == 0
        torch.cuda.synchronize()
        with torch.no_grad():
            mf.layers_xyz[2].weight.mul_(3.0e4)
        nerf.models.mark_parameters_updated()
        render()
        assert _ops.render_nonfinite_count() > 0
        assert int(_ops.render_status_words().sum()) > 0
        with torch.cuda.stream(side):
            assert _ops.render_nonfinite_count() == 0
            assert int(_ops.render_status_words().sum()) == 0
