"""nerf.FusedJointStep - the training iteration with the cameras as parameters beside the networks - and its driver flags
(train_dexnerf.py --refine-poses).

Yardsticks: the step is built from launches the existing suites pin one by one, so its halves are compared BIT FOR BIT (torch.equal)
with the steps that already make those launches: the camera half with nerf.FusedPoseStep (the network optimizer at lr = 0), the network
half with dn_render_rays_backward_ws (nets = 3) on the step's own saved tensors and with a FusedTrainStep(draw_view="rays") +
GraphedTrainStep loop on the step's own camera records (the pose learning rate at 0), a replayed run with an eager one, a run with
its repetition and with its resumption from state_dict(), a render between two replays with fresh models that load the parameters.
The one test with training in it states inequalities, no tolerance.

Shapes (ragged on purpose): 3 views of 24 x 20 pixels, 200 rays (no multiple of 256, of 64, or of the 4 rays per compositing
workgroup), 16 + 24 samples (3,200 and 8,000 points: a partial last tile in both passes), lego 4 x 128 / L10 networks; one case with a
coarse 4 x 128 and a fine D8 / W256 / skip 4 network at 64 rays and 10 + 8 samples (the per-network weight-gradient route; 10 coarse samples
are the fewest the library renders: dn_fine_depths needs num_coarse >= 10)."""
import os

import pytest
import torch

from golden_cases import CASES
from test_input_gradients import make_cfg
from test_mixed_view_batches import POSES, V

H, W, N_RAYS = 24, 20, 200
RENDER = dict(num_coarse=16, num_fine=24, near=2.0, far=6.0, perturb=True, noise_std=0.2, white_background=True)
RENDER_MIXED = dict(RENDER, num_coarse=10, num_fine=8)      # (num_coarse >= 10: dn_fine_depths)
XI_START = ((0.01, -0.02, 0.015, 0.03, -0.01, 0.02), (-0.02, 0.01, 0.005, -0.01, 0.02, 0.015), (0.005, 0.015, -0.01, 0.02, 0.01, -0.03))
PRECISIONS = ("fp32", "bf16-s16")


def cameras(h=H, w=W):
    """(E (V,4,4), K (3,3)) fp32 host tensors: the view set of test_mixed_view_batches (poses 3, 9, 14 of the synthetic scene)."""
    from nerf import synthetic as syn
    return torch.stack([torch.from_numpy(syn.scene_pose(p)) for p in POSES]), torch.from_numpy(syn.intrinsic(h, w))


def build_net(mkw, sd, dev):
    import nerf
    m = nerf.models.FlexibleNeRFModel(**mkw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev)


def make_nets(dev, shapes="lego"):
    """(coarse, fine): the lego 4 x 128 pair, or ("mixed") the lego coarse network with the D8 / W256 fine network."""
    mkw, wfn, _ = CASES["render_lego_val"]
    sd_c, sd_f = wfn()
    if shapes == "lego":
        return build_net(mkw, sd_c, dev), build_net(mkw, sd_f, dev)
    mkw8, wfn8, _ = CASES["render_d8w256_val"]
    return build_net(mkw, sd_c, dev), build_net(mkw8, wfn8()[1], dev)


def encoders():
    import nerf
    return nerf.get_embedding_function(10), nerf.get_embedding_function(4)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_joint_step_is_exported_and_refuses_what_it_cannot_train_before_any_device_call(monkeypatch):
    import nerf
    from nerf import _hip
    assert nerf.FusedJointStep is nerf.pose.FusedJointStep and issubclass(nerf.FusedJointStep, nerf.FusedPoseStep)

    def no_device(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_hip, "lib", no_device)
    e, k = cameras()
    images = torch.zeros(V, H, W, 3)
    cfg = make_cfg(RENDER)
    lego = dict(CASES["render_lego_val"][0])
    ex, ed = encoders()

    def make(mc, mf, ex=ex, ed=ed, e=e, k=k, images=images, **kw):
        return nerf.FusedJointStep(mc, mf, cfg, H, W, k, e, images, ex, ed, N_RAYS, None, None, 1e-3, **kw)
    good = nerf.models.FlexibleNeRFModel(**lego)
    refused = {"W = 192": (nerf.models.FlexibleNeRFModel(**dict(lego, hidden_size=192)), ex),
               "L_xyz = 8": (nerf.models.FlexibleNeRFModel(**dict(lego, num_encoding_fn_xyz=8)), nerf.get_embedding_function(8)),
               "no view directions": (nerf.models.FlexibleNeRFModel(**dict(lego, use_viewdirs=False)), ex)}
    for what, (bad, ex_bad) in refused.items():
        for pair in ((bad, good), (good, bad)):
            with pytest.raises(ValueError, match=r"MultiPoseRefiner \+ autograd") as info:
                make(*pair, ex=ex_bad)
            assert "FusedJointStep" in str(info.value) and "fused training kernels" in str(info.value), what
    with pytest.raises(ValueError, match=r"fine network is required.*MultiPoseRefiner \+ autograd"):
        make(good, None)
    with pytest.raises(ValueError, match="intrinsics"):
        make(good, good, k=torch.stack([k, k]))
    with pytest.raises(ValueError, match="images"):
        make(good, good, images=images[:2])
    for fixed in ((V,), (0, -1)):
        with pytest.raises(ValueError, match="fixed_views"):
            make(good, good, fixed_views=fixed)
    with pytest.raises(ValueError, match="refine_intrinsics"):
        make(good, good, refine_intrinsics="all")
    with pytest.raises(ValueError, match="pose_lr_decay"):
        make(good, good, pose_lr_decay=(0.0, 100))
    # FusedPoseStep keeps its own order of checks and its own words
    with pytest.raises(ValueError, match="nothing to refine"):
        nerf.FusedPoseStep(good, good, cfg, H, W, k, e, images, ex, ed, N_RAYS, 1e-3, refine_pose=False)


def test_driver_parser_accepts_the_new_flags_and_refuses_inconsistent_ones():
    import train_dexnerf
    args = train_dexnerf.parse_args(["--refine-poses", "--pose-lr", "2e-3", "--pose-lr-decay", "0.1", "5000", "--refine-intrinsics", "shared",
                                     "--intrinsics-scale", "0.5", "--fix-views", "0", "2", "--pose-noise", "0.02", "0.05", "--depth-weight", "0.1",
                                     "--ir"])
    assert args.refine_poses and args.mix_views and args.pose_lr == 2e-3 and args.pose_lr_decay == [0.1, 5000.0]
    assert args.refine_intrinsics == "shared" and args.intrinsics_scale == 0.5 and args.fix_views == [0, 2] and args.pose_noise == [0.02, 0.05]
    plain = train_dexnerf.parse_args(["--refine-poses"])
    assert plain.fix_views == [0] and plain.pose_lr == 1e-3 and plain.refine_intrinsics is None and plain.pose_noise is None and plain.mix_views
    off = train_dexnerf.parse_args([])
    assert not off.refine_poses and not off.mix_views and off.fix_views is None and off.pose_lr is None
    assert train_dexnerf.parse_args(["--pose-noise", "0.01", "0.0"]).pose_noise == [0.01, 0.0]      # training at perturbed poses: allowed
    for bad in (["--pose-lr", "1e-3"], ["--pose-lr-decay", "0.1", "100"], ["--refine-intrinsics", "shared"], ["--fix-views", "1"],
                ["--intrinsics-scale", "2.0"], ["--refine-poses", "--refine-intrinsics", "everything"], ["--refine-poses", "--pose-noise", "-0.1", "0.0"],
                ["--pose-noise", "0.1", "-1.0"], ["--refine-poses", "--autograd-step"], ["--refine-poses", "--intrinsics-scale", "2.0"],
                ["--refine-poses", "--pose-lr-decay", "0.0", "10"], ["--refine-poses", "--fix-views", "-1"]):
        with pytest.raises(SystemExit):
            train_dexnerf.parse_args(bad)


def test_checkpoint_without_the_joint_key_loads_unchanged():
    import train_dexnerf

    class Recorder:
        loaded = None

        def load_state_dict(self, state):
            self.loaded = state
    ck = {"iter": 7, "model_coarse_state_dict": {}, "model_fine_state_dict": {}, "optimizer_state_dict": {}, "loss": 0.5, "psnr": 3.0}
    before = dict(ck)
    rec = Recorder()
    assert train_dexnerf.restore_joint_state(ck, rec) is False and rec.loaded is None and ck == before
    state = {"params": torch.zeros(20)}
    assert train_dexnerf.restore_joint_state(dict(ck, **{train_dexnerf.JOINT_KEY: state}), rec) is True and rec.loaded is state
    assert train_dexnerf.JOINT_KEY not in ("iter", "model_coarse_state_dict", "model_fine_state_dict", "optimizer_state_dict", "loss", "psnr")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import nerf
    from nerf import _hip
    _hip.lib()
    nerf.set_precision("fp32")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_modes():
    import nerf
    nerf.set_render_policy("bf16")
    yield
    nerf.set_render_policy(None)
    nerf.set_precision("fp32")


def problem(dev, cfg=RENDER):
    e0, k = cameras()
    images = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    return e0.to(dev), k.to(dev), images, make_cfg(cfg)


def make_joint(dev, nets, seed, lr_net=5e-4, lr_pose=1e-3, zero_grads=True, num_rays=N_RAYS, cfg=RENDER, **kw):
    """A FusedJointStep on `nets` with its own bucket and nerf.FlatAdam; returns (step, bucket, optimizer)."""
    import nerf
    from nerf import parallel
    e0, k, images, options = problem(dev, cfg)
    ex, ed = encoders()
    bucket = parallel.FlatGradBucket(list(nets))
    opt = nerf.FlatAdam(bucket, lr=lr_net, zero_grads=zero_grads)
    step = nerf.FusedJointStep(nets[0], nets[1], options, H, W, k, e0, images, ex, ed, num_rays, bucket, opt, lr_pose, seed=seed, **kw)
    return step, bucket, opt


def params_of(nets):
    return [p.detach().clone() for m in nets for p in m.parameters()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [None, "shared"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_camera_half_equals_the_pose_step_bit_for_bit(dev, precision, mode):
    """The network optimizer at lr = 0 leaves every parameter's bits alone: the joint step then makes FusedPoseStep's launches on
    FusedPoseStep's inputs (the weight-gradient launches write elsewhere).  6 steps: 3 eager, 1 capture, 2 replays."""
    import nerf
    nerf.set_precision(precision)
    kw = dict(refine_intrinsics=mode, fixed_views=(0,))
    nets = make_nets(dev)
    start = params_of(nets)
    joint, _, _ = make_joint(dev, nets, seed=21, lr_net=0.0, **kw)
    frozen = make_nets(dev)
    for p in list(frozen[0].parameters()) + list(frozen[1].parameters()):
        p.requires_grad_(False)
    e0, k, images, options = problem(dev)
    ex, ed = encoders()
    pose = nerf.FusedPoseStep(frozen[0], frozen[1], options, H, W, k, e0, images, ex, ed, N_RAYS, 1e-3, seed=21, **kw)
    for step in (joint, pose):
        step.xi.copy_(torch.tensor(XI_START))
    for it in range(6):
        joint.step(); pose.step()
        torch.cuda.synchronize()
        for name in ("xi", "last_grad", "loss3") + (("phi", "last_grad_phi") if mode else ()):
            a, b = getattr(joint, name), getattr(pose, name)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (it, name, (a - b).abs().max().item())
    assert joint.graph is not None and pose.graph is not None and joint.fallback_reason is None, joint.fallback_reason
    assert float(joint.last_grad[1:].abs().min(dim=1).values.max()) > 0 and bool((joint.last_grad[0] == 0).all())
    assert torch.equal(joint.xi[0], torch.tensor(XI_START[0], device=dev)) and not torch.equal(joint.xi[1:], torch.tensor(XI_START[1:], device=dev))
    assert joint.phi is None if mode is None else float(joint.phi.abs().max()) > 0
    assert same(params_of(nets), start)
    assert torch.equal(joint.extrinsics(), pose.extrinsics()) and torch.equal(joint.intrinsics(), pose.intrinsics())


def reference_weight_gradients(step):
    """What dn_render_rays_backward_ws (nets = 3) accumulates from the saved tensors and upstream gradients of the step's latest
    iteration: [(dW, db)] per network in linear_modules() order."""
    from nerf import _ops
    keep = step._keep
    saved, g_c, g_f = keep[5], (keep[9], keep[11], None), (keep[10], keep[12], None)
    mc, mf = step.models
    pc, pf = mc._packed_slot(*step.logs), mf._packed_slot(*step.logs)
    want_c = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mc.linear_modules()], saved["rays"].device)
    want_f = _ops.zeroed_grad_views([tuple(m.weight.shape) for m in mf.linear_modules()], saved["rays"].device)
    _ops.render_rays_backward(pc, pf, saved, g_c, g_f, want_c, want_f, nets=3)
    return want_c, want_f


NETWORK_CASES = {"lego": ("lego", N_RAYS, RENDER), "mixed": ("mixed", 64, RENDER_MIXED)}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sorted(NETWORK_CASES))
def test_network_half_equals_the_training_step_bit_for_bit(dev, case, precision):
    """Cameras held (refine_pose=False, no intrinsics, lr_pose = 0).  (i) the .grad of every parameter after the third step of
    a run that clears the bucket in the step = the weight gradients of dn_render_rays_backward_ws (nets = 3) on that step's saved tensors; (ii) after 5 steps (3 eager, 1 capture, 1 replay)
    every parameter = that of a FusedTrainStep(draw_view="rays") + GraphedTrainStep loop with the same seed and optimizer settings on a
    selector that carries the joint step's own camera records."""
    import nerf
    from nerf import parallel
    nerf.set_precision(precision)
    shapes, n_rays, render = NETWORK_CASES[case]
    held = dict(refine_pose=False, refine_intrinsics=None, lr_pose=0.0, num_rays=n_rays, cfg=render)
    # (i) an optimizer that neither moves the parameters nor clears the gradients: the bucket holds the step's weight gradients
    nets = make_nets(dev, shapes)
    # - and so the step clears the bucket itself, one memset before every backward: three steps (1 eager, the capture, 1 replay), the
    # bucket must hold the THIRD step's gradients alone
    probe, _, _ = make_joint(dev, nets, seed=33, lr_net=0.0, zero_grads=False, eager_iterations=1, **held)
    for _ in range(3):
        probe.step()
    torch.cuda.synchronize()
    assert probe.graph is not None and probe.zero_in_step and probe.rng_state.tolist()[2:] == [2, 3]
    want_c, want_f = reference_weight_gradients(probe)
    for m, want in zip(nets, (want_c, want_f)):
        for lin, (dw, db) in zip(m.linear_modules(), want):
            assert float(dw.abs().max()) > 0 and torch.equal(lin.weight.grad, dw) and torch.equal(lin.bias.grad, db)
    assert bool((probe.last_grad == 0).all()) and bool((probe.xi == 0).all())
    # (ii)
    nets = make_nets(dev, shapes)
    joint, _, _ = make_joint(dev, nets, seed=33, **held)
    for _ in range(5):
        joint.step()
    torch.cuda.synchronize()
    assert joint.graph is not None and joint.fallback_reason is None, joint.fallback_reason
    e0, k, images, options = problem(dev, render)
    ex, ed = encoders()
    ref_nets = make_nets(dev, shapes)
    sel = nerf.MultiViewRaySelector(H, W, list(e0), [k] * V, 2.0, 6.0, images=images, device=dev)
    sel.cams = joint.cams.clone()
    bucket = parallel.FlatGradBucket(list(ref_nets))
    fused = nerf.FusedTrainStep(ref_nets[0], ref_nets[1], sel, options, bucket, ex, ed, n_rays, seed=33, draw_view="rays")
    loop = nerf.GraphedTrainStep(fused, nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True), eager_iterations=3)
    for _ in range(5):
        loop.step()
    torch.cuda.synchronize()
    assert loop.graphs is not None and loop.fallback_reason is None, loop.fallback_reason
    assert torch.equal(joint.loss3, fused.loss3) and torch.equal(joint.latest_draw()[2], fused.latest_draw()[2])
    got, want = params_of(nets), params_of(ref_nets)
    start = params_of(make_nets(dev, shapes))
    assert same(got, want), max((a - b).abs().max().item() for a, b in zip(got, want))
    assert all(not torch.equal(a, b) for a, b in zip(got, start))


REPLAY_KW = dict(refine_intrinsics="shared", fixed_views=(0,))


@pytest.fixture(scope="module", params=PRECISIONS)
def replay_runs(request, dev):
    """8 steps replayed (3 eager, 1 capture, 4 replays) and 8 steps eager from the same start: per step xi, phi, loss3 and every
    parameter; the networks and the step of the graphed run."""
    import nerf
    nerf.set_precision(request.param)
    try:
        runs = {}
        for graphs in (True, False):
            nets = make_nets(dev)
            step, _, _ = make_joint(dev, nets, seed=8, use_graphs=graphs, **REPLAY_KW)
            trace = []
            for _ in range(8):
                step.step()
                torch.cuda.synchronize()
                trace.append((step.xi.clone(), step.phi.clone(), step.loss3.clone(), params_of(nets)))
            runs[graphs] = (step, nets, trace)
    finally:
        nerf.set_precision("fp32")
    return request.param, runs


@pytest.mark.gpu
def test_replayed_steps_equal_eager_steps(replay_runs):
    _, runs = replay_runs
    (graphed, _, trace_g), (eager, _, trace_e) = runs[True], runs[False]
    assert graphed.fallback_reason is None and eager.fallback_reason is None, graphed.fallback_reason
    assert isinstance(graphed.graph, torch.cuda.CUDAGraph) and eager.graph is None
    for it, ((xi_g, phi_g, loss_g, p_g), (xi_e, phi_e, loss_e, p_e)) in enumerate(zip(trace_g, trace_e)):
        assert torch.equal(xi_g, xi_e) and torch.equal(phi_g, phi_e) and torch.equal(loss_g, loss_e) and same(p_g, p_e), it
    assert all(not torch.equal(a, b) for a, b in zip(trace_g[-1][3], trace_g[-2][3]))       # the replays keep training
    assert not torch.equal(trace_g[-1][0], trace_g[-2][0]) and bool(torch.isfinite(trace_g[-1][2]).all())
    assert graphed.rng_state.tolist()[2:] == [7, 8] and eager.rng_state.tolist()[2:] == [7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_render_between_replays_sees_the_weights_the_replay_trained(dev, precision):
    """The driver's pattern (--validate-every): render, replay, render again, on networks no other step touches in between.  The first
    render packs the streams it reads at the host's parameter key; a replay runs no Python hook, so only the
    mark_parameters_updated() that follows it in FusedJointStep.step makes the second render pack again.  The second render equals
    the render of fresh models that load the current parameters and differs from the first.  (Without that call the second render
    repeats the first one bit for bit - checked once by running this test with the call taken out.)"""
    import nerf
    from nerf import synthetic as syn
    nerf.set_precision(precision)
    nets = make_nets(dev)
    step, _, _ = make_joint(dev, nets, seed=8, **REPLAY_KW)
    for _ in range(5):                       # 3 eager, the capture, 1 replay
        step.step()
    torch.cuda.synchronize()
    assert isinstance(step.graph, torch.cuda.CUDAGraph) and step.fallback_reason is None, step.fallback_reason
    _, k = cameras()
    options = make_cfg(dict(RENDER, perturb=False, noise_std=0.0))
    ex, ed = encoders()
    ro, rd = nerf.get_ray_bundle(H, W, float(k[0, 0]), torch.from_numpy(syn.scene_pose(9)).to(dev), k.to(dev))

    def render(models):
        with torch.no_grad():
            out = nerf.run_one_iter_of_nerf(H, W, float(k[0, 0]), models[0], models[1], ro, rd, options, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed)
        return [t.clone() for t in out[:6]]
    first = render(nets)
    before = params_of(nets)
    step.step()                              # a replay, and nothing else, between the two renders
    second = render(nets)
    torch.cuda.synchronize()
    assert all(not torch.equal(a, b) for a, b in zip(params_of(nets), before))
    fresh = make_nets(dev)
    for m, trained in zip(fresh, nets):
        m.load_state_dict({name: t.detach().clone() for name, t in trained.state_dict().items()})
    want = render(fresh)
    for a, b, c in zip(second, want, first):
        assert torch.equal(a, b) and not torch.equal(a, c)


def run_steps(dev, seed, n, first_iteration=0, restore=None, **kw):
    """A fresh joint run of n steps; restore = (parameters, FlatAdam buffers, joint state) of an earlier run to continue."""
    from nerf import models
    nets = make_nets(dev)
    step, bucket, opt = make_joint(dev, nets, seed=seed, first_iteration=first_iteration, **REPLAY_KW, **kw)
    if restore is not None:
        flat_params, exp_avg, exp_avg_sq, step_state, joint_state = restore
        bucket.flat_params.copy_(flat_params); opt.exp_avg.copy_(exp_avg); opt.exp_avg_sq.copy_(exp_avg_sq); opt.step_state.copy_(step_state)
        models.mark_parameters_updated()
        step.load_state_dict(joint_state)
    draws = []
    for _ in range(n):
        step.step()
        torch.cuda.synchronize()
        draws.append(step.latest_draw()[1].clone())
    snapshot = (bucket.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_state.clone(), step.state_dict())
    return step, params_of(nets), draws, snapshot


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_run_is_a_function_of_its_seed_and_resumes_from_its_state(dev, precision):
    import nerf
    nerf.set_precision(precision)
    decay = dict(pose_lr_decay=(0.1, 20))
    a, params_a, draws_a, _ = run_steps(dev, 5, 10, **decay)
    b, params_b, draws_b, _ = run_steps(dev, 5, 10, **decay)
    assert same(params_a, params_b) and torch.equal(a.xi, b.xi) and torch.equal(a.phi, b.phi) and same(draws_a, draws_b)
    c, params_c, draws_c, _ = run_steps(dev, 6, 10, **decay)
    assert all(not torch.equal(x, y) for x, y in zip(draws_a, draws_c)) and not torch.equal(a.xi, c.xi) and not same(params_a, params_c)
    first, _, draws_1, snapshot = run_steps(dev, 5, 5, **decay)
    state = snapshot[4]
    assert set(state) >= {"params", "exp_avg", "exp_avg_sq", "adam_state"} and float(state["adam_state"][0]) == 5.0
    assert torch.equal(state["params"][:6 * V].view(V, 6), first.xi) and state["params"].data_ptr() != first.xi.data_ptr()
    second, params_2, draws_2, _ = run_steps(dev, 5, 5, first_iteration=5, restore=snapshot, **decay)
    assert same(draws_1 + draws_2, draws_a)
    assert torch.equal(second.xi, a.xi) and torch.equal(second.phi, a.phi) and same(params_2, params_a)
    assert torch.equal(second.state_dict()["adam_state"], a.state_dict()["adam_state"])
    # the decayed pose learning rate is what dn_adam_step reports it used: lr_pose * factor ** (t / steps) at t = 9
    assert abs(float(a.state_dict()["adam_state"][2]) - 1e-3 * 0.1 ** (9 / 20)) <= 1e-6 * 1e-3
    with pytest.raises(ValueError, match="load_state_dict"):
        make_joint(dev, make_nets(dev), seed=1, fixed_views=(0,))[0].load_state_dict(state)      # a state with phi into a step without


@pytest.mark.gpu
def test_default_bf16_parameter_step_is_undisturbed_by_joint_steps(dev):
    """The pattern of test_default_bf16_parameter_step_is_undisturbed_by_an_input_gradient_call: a parameter-only training step in
    'bf16' (8-bit saves, 48-point kernels) gives bit-identical parameter gradients before and after joint steps on the same models
    (which run 16-bit saves on the 32-point kernels and pack other streams).  Both optimizers of the joint steps at lr = 0."""
    import nerf
    from nerf import _hip, _ops
    nerf.set_precision("bf16")
    nets = make_nets(dev)
    start = params_of(nets)
    joint, bucket, _ = make_joint(dev, nets, seed=4, lr_net=0.0, lr_pose=1e-3, fixed_views=(0,))
    e0, k, images, options = problem(dev)
    ex, ed = encoders()
    sel = nerf.MultiViewRaySelector(H, W, list(e0), [k] * V, 2.0, 6.0, images=images, device=dev)

    def parameter_step():
        step = nerf.FusedTrainStep(nets[0], nets[1], sel, options, bucket, ex, ed, N_RAYS, seed=3, draw_view="rays")
        step.forward_backward()
        assert step._keep[1]["prec"] == _hip.PREC_BF16_S8
        grads = [p.grad.detach().clone() for p in bucket.params]
        bucket.zero()
        return grads
    before = parameter_step()
    for _ in range(5):
        joint.step()
    torch.cuda.synchronize()
    assert joint.graph is not None and joint._keep[5]["prec"] == _hip.PREC_BF16 and _ops.get_precision() == "bf16"
    assert float(joint.xi[1:].abs().max()) > 0 and same(params_of(nets), start)
    after = parameter_step()
    assert all(float(g.abs().max()) > 0 for g in before) and same(before, after)


# ---- what it is for -------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(num_coarse=16, num_fine=24, near=2.0, far=6.0, perturb=True, noise_std=0.0, white_background=True)
RECOVERY_ROT, RECOVERY_TRANS = 0.0269, 0.0539      # |omega|, |t| of the twist of the recovery runs in profiles/pose_step_time.md (its
FIXTURE_STEPS, RECOVERY_STEPS = 300, 400           # set-up is the one profiles/depth_supervision.md / intrinsics_refinement.md reuse)


@pytest.fixture(scope="module")
def trained_scene(dev):
    """The synthetic scene of this file's cameras: images = the lego networks rendered at the true poses (validation settings, 64 + 64
    samples); the 4 x 128 networks trained on them at the true poses for FIXTURE_STEPS iterations at the training settings of the
    test (16 + 24 samples, jitter) from the lego weights.  Returns what both runs of the test start from, and a fixed ray set of the
    training views at the true poses."""
    import nerf
    from nerf import _ops, models
    nerf.set_precision("fp32")
    e_true, k = (t.to(dev) for t in cameras())
    ex, ed = encoders()
    teacher = make_nets(dev)
    render = make_cfg(dict(num_coarse=64, num_fine=64, near=2.0, far=6.0, white_background=True))
    images = []
    for v in range(V):
        ro, rd = nerf.get_ray_bundle(H, W, float(k[0, 0]), e_true[v], k)
        with torch.no_grad():
            out = nerf.run_one_iter_of_nerf(H, W, float(k[0, 0]), teacher[0], teacher[1], ro, rd, render, mode="validation",
                                            encode_position_fn=ex, encode_direction_fn=ed)
        images.append(out[3].reshape(H, W, 3))
    images = torch.stack(images)
    flat = torch.randperm(V * H * W, generator=torch.Generator().manual_seed(123))[:600]
    views, pix = (flat // (H * W)).to(torch.int32).to(dev), (flat % (H * W)).to(dev)
    rows, target = _ops.select_rays_views(H, W, _ops.pose_records(torch.zeros(V, 6, device=dev), e_true.contiguous(), k), views, 2.0, 6.0, pix, images)
    nets = make_nets(dev)
    step, bucket, opt = recovery_step(dev, nets, e_true, k, images, seed=99, refine_pose=False, lr_pose=0.0)
    for _ in range(FIXTURE_STEPS):
        step.step()
    torch.cuda.synchronize()
    assert step.fallback_reason is None
    models.mark_parameters_updated()
    state = (bucket.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_state.clone())
    return dict(e_true=e_true, k=k, images=images, rows=rows, target=target, state=state)


def recovery_step(dev, nets, e_start, k, images, seed, lr_pose=1e-3, **kw):
    import nerf
    from nerf import parallel
    ex, ed = encoders()
    bucket = parallel.FlatGradBucket(list(nets))
    opt = nerf.FlatAdam(bucket, lr=5e-4, zero_grads=True)
    step = nerf.FusedJointStep(nets[0], nets[1], make_cfg(RECOVERY), H, W, k, e_start, images, ex, ed, N_RAYS, bucket, opt, lr_pose, seed=seed,
                               loss_weights=(1.0, 1.0), **kw)
    return step, bucket, opt


@pytest.mark.gpu
def test_joint_training_recovers_perturbed_poses_and_beats_training_at_them(dev, trained_scene):
    """From networks trained at the true poses, every view but view 0 is perturbed by a seeded twist of |omega| = 0.0269 rad, |t| =
    0.0539.  RECOVERY_STEPS iterations (a) of the joint step with fixed_views=(0,) and (b) of the networks alone at the perturbed
    poses (refine_pose=False - what the parent commit offers).  On each of 3 seeds (perturbation and draws), all views counted:
    (a) ends nearer the true poses than it started, in mean rotation and in mean translation, and (a) ends with a lower fine MSE than
    (b) on a fixed ray set of the training views at the TRUE poses.  Inequalities, no tolerance.  loss_weights = (1, 1): the coarse
    term did not keep these runs from converging.  fp32, 3 views of 24 x 20, 200 rays, 16 + 24 samples, lr 5e-4 / lr_pose 1e-3.

    Measured on an MI355X (profiles/joint_training.md), mean over the 3 views of [rotation deg, camera-centre distance], fine MSE:
        seed 0: start 1.0275 / 0.03593; (a) 0.4654 / 0.03274, MSE 1.037e-03; (b) MSE 2.150e-03
        seed 1: start 1.0275 / 0.03593; (a) 0.3777 / 0.01997, MSE 1.054e-03; (b) MSE 3.280e-03
        seed 2: start 1.0275 / 0.03593; (a) 0.3299 / 0.01783, MSE 9.668e-04; (b) MSE 7.441e-03
    (every checkpoint of an 800-step run, at 200, 400, 600 and 800 steps, met the three conditions on the three seeds)."""
    import nerf
    from nerf import models
    import train_dexnerf
    nerf.set_precision("fp32")
    s = trained_scene
    ex, ed = encoders()
    quiet = make_cfg(dict(RECOVERY, perturb=False))

    def fine_mse(nets):
        with torch.no_grad():
            out = nerf.predict_and_render_radiance(s["rows"], nets[0], nets[1], quiet, mode="validation", encode_position_fn=ex,
                                                   encode_direction_fn=ed)
        return float(nerf.img2mse(out[3], s["target"]))
    failures = []
    for seed in range(3):
        e_start = train_dexnerf.perturbed_poses(s["e_true"], RECOVERY_ROT, RECOVERY_TRANS, 1000 + seed, keep=(0,))
        rot0, trans0 = train_dexnerf.pose_distance(e_start, s["e_true"])
        assert torch.equal(e_start[0], s["e_true"][0]) and rot0 > 0.5 and trans0 > 0.02
        ends = {}
        for name, kw in (("a", dict(fixed_views=(0,))), ("b", dict(refine_pose=False))):
            nets = make_nets(dev)
            step, bucket, opt = recovery_step(dev, nets, e_start, s["k"], s["images"], seed=seed, **kw)
            for live, saved in zip((bucket.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_state), s["state"]):
                live.copy_(saved)
            models.mark_parameters_updated()
            for _ in range(RECOVERY_STEPS):
                step.step()
            torch.cuda.synchronize()
            assert step.graph is not None and step.fallback_reason is None, step.fallback_reason
            ends[name] = train_dexnerf.pose_distance(step.extrinsics(), s["e_true"]) + (fine_mse(nets),)
        print(f"seed {seed}: start {rot0:.4f} deg / {trans0:.5f}; (a) {ends['a'][0]:.4f} deg / {ends['a'][1]:.5f}, fine MSE {ends['a'][2]:.3e}; "
              f"(b) {ends['b'][0]:.4f} deg / {ends['b'][1]:.5f}, fine MSE {ends['b'][2]:.3e}")
        assert ends["b"][:2] == (rot0, trans0)          # (b) holds its cameras where they were put
        if not (ends["a"][0] < rot0 and ends["a"][1] < trans0 and ends["a"][2] < ends["b"][2]):
            failures.append((seed, rot0, trans0, ends))
    assert not failures, failures


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
CLI = ["--size", "24", "--views", "3", "--num-random-rays", "200", "--layers", "4", "--width", "128", "--num-coarse", "16", "--num-fine", "24",
       "--precision", "fp32", "--validate-every", "6", "--seed", "11", "--quiet"]


@pytest.mark.gpu
def test_driver_trains_saves_and_resumes_with_refined_poses(dev, tmp_path, capsys):
    import train_dexnerf
    path = os.path.join(str(tmp_path), "joint.ckpt")
    flags = ["--refine-poses", "--pose-noise", "0.02", "0.04", "--refine-intrinsics", "shared", "--pose-lr-decay", "0.1", "1000"]
    res = train_dexnerf.main(CLI[:-1] + flags + ["--iters", "12", "--save", path])
    printed = capsys.readouterr().out
    assert "[pose]  iter      6 from the initial poses" in printed and "from the unperturbed poses" in printed
    assert res["val_psnr"] == res["val_psnr"] and res["val_psnr"] > 0.0
    assert res["hip_graphs"] == 1 and res["final_loss"] == res["final_loss"] and float(res["xi"][1:].abs().max()) > 0 and bool((res["xi"][0] == 0).all())
    ck = torch.load(path, map_location="cpu")
    assert ck["iter"] == 12 and {"model_coarse_state_dict", "model_fine_state_dict", "optimizer_state_dict", "loss", "psnr"} <= set(ck)
    state = ck[train_dexnerf.JOINT_KEY]
    assert torch.equal(state["params"][:18].view(3, 6), res["xi"]) and float(state["adam_state"][0]) == 12.0
    assert tuple(ck["refined_extrinsics"].shape) == (3, 4, 4) and tuple(ck["refined_intrinsics"].shape) == (3, 3, 3) and ck["refined_views"] == [0, 1, 2]
    assert torch.equal(ck["refined_extrinsics"][0], ck["joint_initial_extrinsics"][0])
    assert not torch.equal(ck["refined_extrinsics"][1:], ck["joint_initial_extrinsics"][1:])
    rot, trans = res["pose_from_unperturbed"]
    # 12 Adam steps of at most lr = 1e-3 per component from twists of 0.02 rad: the mean over the views stays below 0.02 + 0.012 sqrt(3) rad
    assert 0.0 < rot < 57.3 * (0.02 + 0.012 * 3 ** 0.5) and 0.0 < trans < 0.5 and res["pose_from_initial"][0] > 0.0
    # resumed at iteration 12: no iteration left, the cameras are the saved ones; two more continue from them
    again = train_dexnerf.main(CLI + flags + ["--iters", "12", "--load-checkpoint", path])
    assert torch.equal(again["xi"], res["xi"]) and again["pose_from_unperturbed"] == res["pose_from_unperturbed"]
    more = train_dexnerf.main(CLI + flags + ["--iters", "14", "--load-checkpoint", path])
    assert not torch.equal(more["xi"][1:], res["xi"][1:]) and bool((more["xi"][0] == 0).all())
    # a checkpoint written without --refine-poses loads under it: the cameras start at the given poses
    # --torch-adam: torch.optim.Adam (fused, capturable) stepped inside the capture, the bucket cleared by the step's own memset
    torch_adam = train_dexnerf.main(CLI + flags + ["--iters", "12", "--torch-adam"])
    assert torch_adam["hip_graphs"] == 1 and torch_adam["final_loss"] == torch_adam["final_loss"] and torch_adam["val_psnr"] == torch_adam["val_psnr"]
    assert float(torch_adam["xi"][1:].abs().max()) > 0 and bool((torch_adam["xi"][0] == 0).all())
    # (printed, not compared: the optimizers agree to 2e-6 per step - test_flat_adam_against_torch_adam - but 12 steps of training
    # with density noise and resampling carry no bound on the loss that follows from that)
    print("final loss, FlatAdam", res["final_loss"], "torch.optim.Adam", torch_adam["final_loss"])
    # eval_nerf.py --use-refined-poses renders the training views at the cameras the checkpoint carries
    import eval_nerf
    render = ["--size", "24", "--num-coarse", "16", "--num-fine", "24", "--precision", "fp32", "--quiet"]
    frames = eval_nerf.main(["--checkpoint", path, "--use-refined-poses"] + render)["frames"]
    assert len(frames) == 3 and all(tuple(rgb.shape) == (24, 24, 3) and bool(torch.isfinite(rgb).all()) for rgb, _ in frames)
    plain = os.path.join(str(tmp_path), "plain.ckpt")
    at_given = train_dexnerf.main(CLI + ["--iters", "4", "--save", plain])
    with pytest.raises(SystemExit):
        eval_nerf.main(["--checkpoint", plain, "--use-refined-poses"] + render)
    # --pose-noise alone trains at the perturbed poses (the networks-only baseline of an experiment)
    at_noisy = train_dexnerf.main(CLI + ["--iters", "4", "--pose-noise", "0.02", "0.04"])
    assert at_noisy["final_loss"] == at_noisy["final_loss"] and at_noisy["final_loss"] != at_given["final_loss"] and "xi" not in at_noisy
    assert train_dexnerf.JOINT_KEY not in torch.load(plain, map_location="cpu")
    cont = train_dexnerf.main(CLI + ["--refine-poses", "--iters", "4", "--load-checkpoint", plain])
    assert bool((cont["xi"] == 0).all()) and max(cont["pose_from_initial"]) <= 1e-5


@pytest.mark.gpu
def test_driver_without_the_flag_trains_as_on_the_parent_commit(dev):
    """Without --refine-poses nothing about the driver changes: the final loss of one seeded run has the bits the parent commit's driver
    gave on the same command line (recorded on an MI355X: tests/golden/joint_training_driver_parent.json)."""
    import json

    import train_dexnerf
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "joint_training_driver_parent.json")) as f:
        parent = json.load(f)
    assert "--refine-poses" not in parent["argv"] and parent["argv"][:len(CLI)] == CLI
    res = train_dexnerf.main(list(parent["argv"]))
    print("final loss", float(res["final_loss"]).hex(), "parent", parent["final_loss_float_hex"])
    assert float(res["final_loss"]).hex() == parent["final_loss_float_hex"] and float(res["final_loss"]) == parent["final_loss"]
    assert "xi" not in res and "pose_from_initial" not in res and res["hip_graphs"] == 1
