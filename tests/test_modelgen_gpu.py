"""GPU tests of models generated from Python definitions (vihds.modelgen): the prpr_constant restatement against the
hand-written PrprConstant kernels and the reference fixtures, and a receiver model that is not built in against its own
definition in float64 (the yardstick of tests/test_decoder_dispatch_shapes.py)."""
import pytest
import torch

from fixture_util import Fixture, rel_err
from oracle import vihds_oracle as O
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_models as MM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXED = ["modeuler", "modeulerwhile", "euler", "midpoint", "rk4"]


def _key(cls, neural):
    modelgen.register_kernel(cls, neural)
    return cls.model_key


def _run(spec, th, cond, times, obs, weights):
    """forward + adjoint of one launch pair with random upstream gradients on the log-likelihood."""
    th = th.detach().clone().requires_grad_(True)
    w = None if weights is None else weights.detach().clone().requires_grad_(True)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, cond, times, obs, None, w)
    gen = torch.Generator(device=DEV).manual_seed(5)
    g = torch.randn(logp.shape, device=DEV, generator=gen)
    (logp * g).sum().backward()
    torch.cuda.synchronize()
    return traj.detach(), xpred.detach(), logp.detach(), th.grad, (None if w is None else w.grad)


def _random_weights(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return 0.3 * torch.randn(n, device=DEV, generator=gen)


@pytest.mark.parametrize("solver", FIXED + ["dopri5"])
@pytest.mark.parametrize("prec", ["constant", "neural_h0", "neural_h3"])
def test_generated_prpr_matches_the_handwritten_kernel(solver, prec):
    """Same kernel template (thread-per-trajectory, kernel_variant=1 for the built-in), different model body: trajectories,
    x_predict, log-likelihood, g_theta and g_weights agree to 1e-5 per species / parameter.  dopri5: one accepted grid
    (from the built-in's controller) handed to both."""
    neural = prec != "constant"
    fx = Fixture("prpr_constant_precisions_tiny_modeuler" if neural else "prpr_constant_tiny_modeuler")
    th, row_of = H.pack_theta(fx, DEV)
    cond, times, obs = fx.t("inputs", DEV), fx.t("times", DEV), fx.t("observations", DEV)
    hidden = 3 if prec == "neural_h3" else 0
    builtin = "prpr_constant_precisions" if neural else "prpr_constant"
    gen_key = _key(MM.PrprRestatedPrecisions if neural else MM.PrprRestated, neural)
    mk = lambda key, s, kv: ops.OdeProblemSpec(key, s, row_of, th.shape[0], C=cond.shape[1], kernel_variant=kv,  # noqa: E731
                                               n_hidden_prec=hidden)
    ref_spec = mk(builtin, solver, 1)
    gen_spec = mk(gen_key, solver, 0)
    weights = None
    if neural:
        n_w = hip.lib().vihds_model_n_weights(ref_spec.bind(fx.B, fx.S, times.shape[0]))
        assert n_w == hip.lib().vihds_model_n_weights(gen_spec.bind(fx.B, fx.S, times.shape[0])) > 0
        weights = _random_weights(n_w, 11)
    if solver == "dopri5":
        grid, index = ops.adaptive_grid(ref_spec, th, cond, times, None, weights)
        grid_g, _ = ops.adaptive_grid(gen_spec, th, cond, times, None, weights)  # (the generated model's controller runs)
        assert grid_g.shape[0] >= times.shape[0] and bool(torch.isfinite(grid_g).all())
        times = grid.to(DEV) if not grid.is_cuda else grid
        obs = torch.zeros((fx.B, 4, times.shape[0]), device=DEV)
    ref = _run(ref_spec, th, cond, times, obs, weights)
    got = _run(gen_spec, th, cond, times, obs, weights)
    assert rel_err(H.view_bsnt(got[0]), H.view_bsnt(ref[0])) < 1e-5
    assert rel_err(H.view_bsnt(got[1]), H.view_bsnt(ref[1])) < 1e-5
    assert rel_err(H.view_bs4(got[2]), H.view_bs4(ref[2]), dim=2) < 1e-5
    rows = sorted(set(row_of[s] for s in gen_spec.slots))
    assert rel_err(got[3][rows], ref[3][rows], dim=0) < 1e-5
    if neural:
        assert rel_err(got[4], ref[4]) < 1e-5


@pytest.mark.parametrize("name", ["prpr_constant_tiny_modeuler", "prpr_constant_precisions_tiny_modeuler"])
def test_generated_prpr_matches_the_reference_fixture(name):
    fx = Fixture(name)
    neural = "precisions" in name
    key = _key(MM.PrprRestatedPrecisions if neural else MM.PrprRestated, neural)
    th, row_of = H.pack_theta(fx, DEV)
    th.requires_grad_(True)
    spec = ops.OdeProblemSpec(key, fx.solver, row_of, th.shape[0], C=fx.z["inputs"].shape[1])
    wts = None
    if neural:
        prec_w, _, _ = fx.decoder_weights(DEV)
        wts = torch.cat([prec_w[k].reshape(-1) for k in ("prod_w", "prod_b", "degr_w", "degr_b")]).requires_grad_(True)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, fx.t("inputs", DEV), fx.t("times", DEV),
                                                  fx.t("observations", DEV), None, wts)
    assert rel_err(H.view_bs4(logp), fx.t("log_p_by_species"), dim=2) < 1e-4
    if neural:
        full = H.view_bsnt(traj)
        assert rel_err(full[:, :, :-4], fx.t("x_states")) < 1e-4
        assert rel_err(full[:, :, -4:], fx.t("precisions")) < 1e-4
    else:
        st = int(fx.z["sample_stride"])
        assert rel_err(H.view_bsnt(traj)[:, ::st], fx.t("x_states")) < 1e-4
    loss, log_w, _ = ops.iwae_loss(logp, fx.t("log_p", DEV), fx.t("log_q", DEV))
    assert rel_err(loss, fx.t("loss")) < 1e-4
    loss.backward()
    # (the reference's d loss / d theta also holds the log p - log q terms: added analytically, as test_hip_parity does)
    thc = fx.theta_dict(requires_grad=True)
    qm, qp = fx.q_params()
    pm, pp = fx.p_params()
    vals = [thc[n] for n in fx.names]
    lw_extra = O.chained_log_prob(fx.kinds, pm, pp, vals) - O.chained_log_prob(fx.kinds, qm, qp, vals)
    w = torch.softmax(log_w.detach().cpu(), dim=1) * (-1.0 / fx.B)
    (lw_extra * w).sum().backward()
    live = torch.tensor([k != O.CONSTANT for k in fx.kinds])
    extra = torch.stack([thc[n].grad if thc[n].grad is not None else torch.zeros(fx.B, fx.S) for n in fx.names])
    got = th.grad[: len(fx.names)].cpu() + extra
    assert rel_err(got[live], fx.t("theta_grad")[live], dim=0) < 5e-4
    if neural:
        ref = fx.decoder_weight_grads()
        keys = ("prec_production.weight", "prec_production.bias", "prec_degradation.weight", "prec_degradation.bias")
        gref = torch.cat([ref["ode_model.precisions." + k].reshape(-1) for k in keys])
        assert rel_err(wts.grad, gref) < 5e-4


def _lux_theta(B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    base = {"r": 1.0, "K": 2.0, "tlag": 2.0, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "dR": 0.5, "aYFP": 1.2,
            "aCFP": 0.9, "a530": 0.4, "a480": 0.3, "aR": 1.5, "e76": 0.05, "KGR": 2.0, "nR": 1.6, "KR6": 0.3, "KR12": 0.1,
            "init_x": 0.01, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1, "init_luxR": 0.2,
            "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0,
            "init_prec_x": 10.0, "init_prec_rfp": 10.0, "init_prec_yfp": 10.0, "init_prec_cfp": 10.0}
    return {k: (v * torch.exp(0.2 * torch.randn(B, S, generator=gen, dtype=torch.float64))) for k, v in base.items()}


def _lux_oracle(th, cond, times, obs, solver, prec_w, dtype):
    th = {k: v.to(dtype).detach().clone().requires_grad_(True) for k, v in th.items()}
    rhs, x0 = MM.LuxReceiver.torch_problem(th, cond.to(dtype))
    if prec_w is not None:
        pw = {k: v.to(dtype) for k, v in prec_w.items()}
        rhs = O._with_precisions(rhs, 7, pw)
        x0 = torch.cat([x0, torch.stack([th["init_prec_x"], th["init_prec_rfp"], th["init_prec_yfp"], th["init_prec_cfp"]],
                                        dim=2)], dim=2)
    sol = O.simulate(rhs, x0, times.to(dtype), solver)
    if prec_w is None:
        xs, prec = sol, O.expand_constant_precisions(th, times.shape[0])
    else:
        xs, prec = O.split_neural_precisions(sol)
    lpo = O.log_prob_observations(O.observe_default(xs), obs.to(dtype), prec)
    loss = -lpo.sum(dim=2).logsumexp(dim=1).mean()
    loss.backward()
    return loss.detach(), th


@pytest.mark.parametrize("solver", ["modeuler", "midpoint", "rk4"])
@pytest.mark.parametrize("neural", [False, True])
def test_generated_receiver_against_its_own_definition_in_float64(solver, neural):
    """A model that is not built in (LuxR-only receiver, parameter-exponent Hill term, two treatments, seven species) at
    B=36, S=200, T=86: loss and per-parameter gradients within max(floor, 8x the float32 oracle's own error)."""
    B, S, T = 36, 200, 86
    cls = MM.LuxReceiverPrecisions if neural else MM.LuxReceiver
    key = _key(cls, neural)
    th64 = _lux_theta(B, S, 3)
    gen = torch.Generator().manual_seed(4)
    cond = torch.log1p(2.0 * torch.rand(B, 2, generator=gen, dtype=torch.float64))
    times = torch.linspace(0.0, 17.0, T, dtype=torch.float64)
    prec_w = None
    if neural:
        nin = 8
        prec_w = {"prod_w": 0.3 * torch.randn(4, nin, generator=gen, dtype=torch.float64),
                  "prod_b": 0.3 * torch.randn(4, generator=gen, dtype=torch.float64),
                  "degr_w": 0.3 * torch.randn(4, nin, generator=gen, dtype=torch.float64),
                  "degr_b": 0.3 * torch.randn(4, generator=gen, dtype=torch.float64)}
    with torch.no_grad():
        th_obs = {k: v[:, :1].expand(B, 1) for k, v in th64.items()}
        rhs, x0 = MM.LuxReceiver.torch_problem(th_obs, cond)
        obs = O.observe_default(O.simulate(rhs, x0, times, "rk4"))[:, 0] * (1.0 + 0.05 * torch.randn(B, 4, T, generator=gen,
                                                                                                       dtype=torch.float64))
    loss64, g64 = _lux_oracle(th64, cond, times, obs, solver, prec_w, torch.float64)
    loss32, g32 = _lux_oracle({k: v.float() for k, v in th64.items()}, cond, times, obs, solver, prec_w, torch.float32)
    # the kernel
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([th64[n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=2)
    w = None
    if neural:
        w = torch.cat([prec_w[k].reshape(-1) for k in ("prod_w", "prod_b", "degr_w", "degr_b")]).float().to(DEV)
    _, _, logp = ops.OdeSolveObserve.apply(spec, th, cond.float().to(DEV), times.float().to(DEV), obs.float().to(DEV), None,
                                           w)
    loss = -H.view_bs4(logp).sum(dim=2).logsumexp(dim=1).mean()
    loss.backward()
    torch.cuda.synchronize()
    e32 = abs(loss32.double().item() - loss64.item()) / abs(loss64.item())
    e = abs(loss.double().item() - loss64.item()) / abs(loss64.item())
    print("%s neural=%s: loss rel err %.2e (fp32 oracle %.2e)" % (solver, neural, e, e32))
    assert e <= max(1e-6, 8 * e32)
    for n in slots:
        if n not in g64 or g64[n].grad is None:
            continue
        ref = g64[n].grad
        ge = rel_err(th.grad[row_of[n]].cpu(), ref)
        ge32 = rel_err(g32[n].grad, ref)
        assert ge <= max(1e-4, 8 * ge32), (n, ge, ge32)


def _build_named(fx, model_key, **over):
    """Config -> Parameters -> model -> Training from a fixture's recorded experiment, with `model:` naming model_key."""
    import json

    import numpy as np
    import e2e_util as E
    from vihds.config import Config
    from vihds.parameters import Parameters
    from vihds.training import Training
    from vihds.vae import build_model

    spec = json.loads(str(fx.z["spec_json"]))
    spec["model"] = model_key
    spec["params"]["solver"] = fx.solver
    spec["params"].update(over)
    args = E.make_args(fx.S, seed=fx.cfg["seed"], gpu=0)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    settings = Config(args=None, spec=spec)
    settings.device = torch.device(DEV)
    settings.seed = args.seed
    data = E._Pair(E._FakeDataset(fx), settings)
    parameters = Parameters(settings.params)
    model = build_model(args, settings, data, parameters)
    return args, settings, model, Training(args, settings, data, parameters, model)


def test_restated_dr_constant_trains_through_the_general_step(monkeypatch):
    """dr_constant v1 restated with vihds.modelgen, aR / aS conditioned on the device through condition_theta
    (condition_ones), selected by a spec through models.LOOKUP: one Training.step through the general path (ops.GeneralTail)
    on dr_constant_icml_tiny_modeuler's batch and the reference's random streams gives its -ELBO and the gradient of every
    encoder parameter."""
    import numpy as np
    import e2e_util as E
    import models
    from test_e2e_gpu import _ref_encoder_grads

    monkeypatch.setitem(models.LOOKUP, MM.DrRestated.model_key, MM.DrRestated)
    assert models.register(MM.DrRestated) is MM.DrRestated
    fx = Fixture("dr_constant_icml_tiny_modeuler")
    args, settings, model, training = _build_named(fx, MM.DrRestated.model_key, fused_step_tail=True)
    assert isinstance(model.decoder.ode_model, MM.DrRestated)
    model.train()
    batch = E.batch_from_fixture(fx, settings.device)
    np.random.seed(fx.cfg["seed"] + 1)
    torch.manual_seed(fx.cfg["seed"] + 1)
    rec = ops.LaunchRecorder()
    ops.TIMER = rec
    try:
        loss = training.step(batch, zero_grad=False)
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    assert training._gtail_ok is True, "the general step did not take the generated model"
    assert "step_tail" in rec.calls and "ode_bwd" in rec.calls, rec.calls
    assert hip.MODELS[MM.DrRestated.model_key] >= 1024
    assert rel_err(torch.tensor(float(loss)), fx.t("loss")) < 1e-4
    grads = {k: v.grad.detach() for k, v in model.named_parameters() if v.grad is not None}
    ref = _ref_encoder_grads(fx, model.encoder)
    assert ref
    for k, g in ref.items():
        assert rel_err(grads["encoder." + k].cpu(), g) < 1e-3, k


@pytest.mark.parametrize("cls,neural", [(MM.DrRestated, False), (MM.PrprRestatedPrecisions, True)])
def test_spec_naming_a_generated_model_runs_training_and_evaluation(cls, neural, tmp_path, monkeypatch):
    """End to end: a spec whose `model:` is a generated model (added to models.LOOKUP here).  Training steps replayed from
    the step's hipGraph (the reference's host streams staged into the replay) against hip_graph: false from the same seeds,
    through Training._run_batch: every loss equal (the tolerance of test_e2e_gpu's graph-replay test for the built-in
    models), both host generators left in the same state.  Then Training.run() for two epochs with graph capture, and
    Training.evaluate: finite ELBO, importance-weighted means and states."""
    import numpy as np
    import models
    from vihds.utils import TrainingLogData

    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    monkeypatch.chdir(tmp_path)
    fx = Fixture("prpr_constant_precisions_tiny_modeuler" if neural else "dr_constant_icml_tiny_modeuler")
    import e2e_util as E

    runs = {}
    for graph in (False, None):
        args, settings, model, training = _build_named(fx, cls.model_key, hip_graph=graph)
        assert training.use_graph == (graph is None)
        batch = E.batch_from_fixture(fx, settings.device)
        log = TrainingLogData()
        np.random.seed(21)
        torch.manual_seed(21)
        out = []
        orig_step = training.step

        def keeping(b, *a, **k):  # (the eager path hands the loss back through _run_batch's local only)
            training.last_elbo = orig_step(b, *a, **k)
            return training.last_elbo

        training.step = keeping
        for k in range(5):
            model.train()
            assert training._run_batch(0.0, batch, log, next_batch=batch if 2 <= k < 4 else None)
            out.append(float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo))
        runs[graph] = (out, np.random.rand(), float(torch.rand(1)))
    a, b = runs[False], runs[None]
    assert a[1] == b[1] and a[2] == b[2], "the host generators were consumed differently"
    for x, y in zip(a[0], b[0]):
        assert np.isfinite(x) and abs(x - y) <= 2e-5 * max(1.0, abs(x)), (a[0], b[0])
    # the whole loop
    args, settings, model, training = _build_named(fx, cls.model_key)
    assert training.use_graph
    args.epochs, args.test_epoch = 2, 2
    result = training.run()
    assert result is not None and np.isfinite(float(result.elbo)) and training._steps > 0
    model.eval()
    res = training.evaluate(training.train_data, fx.S)
    T = fx.z["times"].shape[0]
    assert res.iw_predict_mu.shape == (fx.B, 4, T) and res.iw_states.shape == (fx.B, len(cls.species), T)
    assert np.isfinite(res.iw_predict_mu).all() and np.isfinite(res.iw_states).all() and np.isfinite(float(res.elbo))
