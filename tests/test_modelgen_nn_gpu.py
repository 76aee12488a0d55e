"""GPU tests of generated models with networks (vihds.modelgen.Network): the kernels against the model's own float64
definition (torch_problem integrated with the oracle's step functions), bit-reproducible weight gradients, the network-free
twin, training through the general step (eager, hipGraph replay, Training.run, evaluate) and the host-driven adaptive solver.

Bounds: 1e-4 relative per species / signal for forward quantities, 5e-4 per parameter for g_theta; a
weight tensor max(5e-4, 8 x the error of the same definition run in float32 eager torch), the yardstick of
tests/test_decoder_dispatch_shapes.py."""
import numpy as np
import pytest
import torch

from fixture_util import rel_err
from oracle import vihds_oracle as O
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_hybrid_models as HM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, GTOL = 1e-4, 5e-4
PREC_MODES = {"constant": None, "neural_h0": 0, "neural_h20": 20}
PREC_INIT = ["init_prec_x", "init_prec_rfp", "init_prec_yfp", "init_prec_cfp"]


def _problem(B, S, T, seed, t_end=8.0):
    gen = torch.Generator().manual_seed(seed)
    base = {"r": 1.0, "K": 2.0, "tlag": 2.0, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP": 1.2, "aCFP": 0.9,
            "e76": 0.5, "init_x": 0.01, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
            "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0,
            "init_prec_x": 10.0, "init_prec_rfp": 10.0, "init_prec_yfp": 10.0, "init_prec_cfp": 10.0}
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    pb = {"th": {k: v * torch.exp(0.2 * rnd(B, S)) for k, v in base.items()},
          "cond": torch.log1p(2.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64)),
          "times": torch.linspace(0.0, t_end, T, dtype=torch.float64),
          "W": {name: tuple(0.6 * rnd(*shape) for shape in net.tensor_shapes())
                for name, net in HM.GrowthWithLatents.networks.items()},
          "g": rnd(B, S, 4), "B": B, "S": S, "T": T}
    pb["prec_w"] = {0: {"prod_w": 0.3 * rnd(4, 7), "prod_b": 0.3 * rnd(4), "degr_w": 0.3 * rnd(4, 7), "degr_b": 0.3 * rnd(4)},
                    20: {"hid_w": 0.3 * rnd(20, 7), "hid_b": 0.3 * rnd(20), "prod_w": 0.3 * rnd(4, 20), "prod_b": 0.3 * rnd(4),
                         "degr_w": 0.3 * rnd(4, 20), "degr_b": 0.3 * rnd(4)}}
    with torch.no_grad():
        th1 = {k: v[:, :1] for k, v in pb["th"].items()}
        rhs, x0 = HM.GrowthWithLatents.torch_problem(th1, pb["cond"], pb["W"])
        xp = O.observe_direct(O.simulate(rhs, x0, pb["times"], "rk4"))[:, 0]
        pb["obs"] = xp * (1.0 + 0.05 * rnd(B, 4, T))
    return pb


PREC_ORDER = ("hid_w", "hid_b", "prod_w", "prod_b", "degr_w", "degr_b")


def _definition(pb, solver, hidden, dtype, cls=HM.GrowthWithLatents, W=None, grid=None):
    """The model's own definition in `dtype` eager torch: forward quantities, g_theta and the weight gradients (buffer
    order) of sum(log-likelihood * g), or of sum(trajectory * g_traj) on an adaptive solver's accepted grid."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {k: leaf(v) for k, v in pb["th"].items()}
    W = pb["W"] if W is None else W
    Wl = {name: tuple(leaf(w) for w in ws) for name, ws in W.items()} if cls.networks else None
    rhs, x0 = cls.torch_problem(th, pb["cond"].to(dtype), Wl) if Wl else cls.torch_problem(th, pb["cond"].to(dtype))
    pw = None
    if hidden is not None:
        pw = {k: leaf(v) for k, v in pb["prec_w"][hidden].items()}
        rhs = O._with_precisions(rhs, 6, pw)
        x0 = torch.cat([x0, torch.stack([th[n] for n in PREC_INIT], dim=2)], dim=2)
    out = {}
    if grid is not None:
        sol = O.integrate_on_grid(grid[0], rhs, x0, grid[1].to(dtype)).permute(1, 2, 3, 0)
        out["traj"] = sol.detach()
        (sol * pb["g_traj"].to(dtype)).sum().backward()
    else:
        sol = O.simulate(rhs, x0, pb["times"].to(dtype), solver)
        xs, prec = (sol, O.expand_constant_precisions(th, pb["T"])) if hidden is None else O.split_neural_precisions(sol)
        xp = O.observe_direct(xs)
        lpo = O.log_prob_observations(xp, pb["obs"].to(dtype), prec)
        out.update(traj=sol.detach(), xpred=xp.detach(), logp=lpo.detach())
        (lpo * pb["g"].to(dtype)).sum().backward()
    out["g_theta"] = {k: v.grad for k, v in th.items() if v.grad is not None}
    gw = [w.grad for ws in (Wl or {}).values() for w in ws]
    if pw is not None:
        gw += [pw[k].grad for k in PREC_ORDER if k in pw]
    out["g_w"] = gw
    return out


def _flat_weights(pb, hidden, W=None):
    W = pb["W"] if W is None else W
    ts = [w for ws in W.values() for w in ws]
    if hidden is not None:
        ts += [pb["prec_w"][hidden][k] for k in PREC_ORDER if k in pb["prec_w"][hidden]]
    return torch.cat([t.reshape(-1) for t in ts]).float().to(DEV)


def _kernel(cls, pb, solver, hidden, W=None, with_weights=True, times=None, g_traj=None):
    neural = hidden is not None
    modelgen.register_kernel(cls, neural)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(cls.model_key, solver, row_of, th.shape[0], C=1, n_hidden_prec=hidden or 0)
    w = _flat_weights(pb, hidden, W).requires_grad_(True) if with_weights else None
    n_w = hip.lib().vihds_model_n_weights(spec.bind(pb["B"], pb["S"], pb["T"]))
    assert n_w == (0 if w is None else w.numel())
    times = pb["times"].float().to(DEV) if times is None else times
    obs = pb["obs"].float().to(DEV) if g_traj is None else torch.zeros((pb["B"], 4, times.shape[0]), device=DEV)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, pb["cond"].float().to(DEV), times, obs, None, w)
    if g_traj is None:
        (H.view_bs4(logp) * pb["g"].float().to(DEV)).sum().backward()
    else:
        (H.view_bsnt(traj) * g_traj.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots},
            "g_w": None if w is None else w.grad.cpu(), "spec": spec, "slots": slots}


def _compare(got, r64, r32, label, forward=("traj", "xpred", "logp")):
    """Prints every figure before it asserts."""
    lines, bad = [], []
    for k in forward:
        e = rel_err(got[k], r64[k], dim=2)
        lines.append("%s %s: %.2e (bound %.0e)" % (label, k, e, TOL))
        if not e < TOL:
            bad.append(lines[-1])
    for n in got["slots"]:
        if n not in r64["g_theta"]:
            continue
        e = rel_err(got["g_theta"][n], r64["g_theta"][n])
        lines.append("%s g_theta[%s]: %.2e (bound %.0e)" % (label, n, e, GTOL))
        if not e < GTOL:
            bad.append(lines[-1])
    o = 0
    for k, ref in enumerate(r64["g_w"]):
        g = got["g_w"][o:o + ref.numel()].view(ref.shape)
        o += ref.numel()
        scale = float(ref.abs().max())
        e, e32 = float((g.double() - ref).abs().max()) / scale, float((r32["g_w"][k].double() - ref).abs().max()) / scale
        bound = max(GTOL, 8.0 * e32)
        lines.append("%s weight tensor %d %s: %.2e (float32 eager %.2e, bound %.2e)" % (label, k, tuple(ref.shape), e, e32, bound))
        if not e <= bound:
            bad.append(lines[-1])
    assert o == (0 if got["g_w"] is None else got["g_w"].numel())
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("solver", ["modeuler", "euler", "midpoint", "rk4"])
@pytest.mark.parametrize("prec", list(PREC_MODES))
def test_hybrid_model_against_its_own_float64_definition(solver, prec):
    """GrowthWithLatents (5 -> 8 -> 4 ReLU latent network in NeuralStates' form, 3 -> 4 -> 1 tanh gate on the expression
    rate) at B=5, S=3, T=20: trajectory, x_predict, log-likelihood, g_theta and every weight gradient -- the eight network
    tensors and, with neural precisions (no hidden layer and 20 hidden units), the precision network's behind them."""
    hidden = PREC_MODES[prec]
    cls = HM.GrowthWithLatents if hidden is None else HM.GrowthWithLatentsPrecisions
    pb = _problem(5, 3, 20, 7)
    r64 = _definition(pb, solver, hidden, torch.float64)
    r32 = _definition(pb, solver, hidden, torch.float32)
    got = _kernel(cls, pb, solver, hidden)
    assert len(r64["g_w"]) == 8 + (0 if hidden is None else (6 if hidden else 4))
    assert all(float(g.abs().max()) > 0 for g in r64["g_w"])
    _compare(got, r64, r32, "%s/%s" % (solver, prec))


def test_hybrid_model_at_the_bench_shape():
    """B=36, S=200, T=86, rk4.  The float64 definition is integrated for ALL 7 200 trajectories (the weight gradient is a
    sum over all of them, so the full run is needed anyway: about a minute on the host); the forward quantities and g_theta
    are compared on every trajectory as well, not on a subset."""
    pb = _problem(36, 200, 86, 11, t_end=17.0)
    r64 = _definition(pb, "rk4", None, torch.float64)
    r32 = _definition(pb, "rk4", None, torch.float32)
    got = _kernel(HM.GrowthWithLatents, pb, "rk4", None)
    _compare(got, r64, r32, "bench shape rk4")


@pytest.mark.parametrize("prec", ["constant", "neural_h20"])
def test_weight_gradients_are_bit_reproducible(prec):
    """The adjoint run twice on the same inputs: torch.equal g_theta and weight gradients (Gram contraction and row sums in
    a fixed order, no atomics) -- with neural precisions the precision network's section too, whose bias sums a model with
    networks also takes from the dump."""
    hidden = PREC_MODES[prec]
    cls = HM.GrowthWithLatents if hidden is None else HM.GrowthWithLatentsPrecisions
    pb = _problem(36, 200, 30, 5)
    a = _kernel(cls, pb, "midpoint", hidden)
    b = _kernel(cls, pb, "midpoint", hidden)
    for n in a["slots"]:
        assert torch.equal(a["g_theta"][n], b["g_theta"][n]), n
    assert float(a["g_w"][:105].abs().max()) > 0
    assert torch.equal(a["g_w"], b["g_w"])
    assert a["g_w"].numel() == 105 + (0 if hidden is None else 20 * 7 + 20 + 2 * (4 * 20 + 4))


def test_zero_output_layers_give_the_network_free_model():
    """W2 = 0, b2 = 0 in both networks: every head is sigmoid(0), the trajectory that of GrowthWithoutNetworks."""
    pb = _problem(5, 3, 20, 7)
    Z = {name: (ws[0], ws[1], torch.zeros_like(ws[2]), torch.zeros_like(ws[3])) for name, ws in pb["W"].items()}
    for solver in ("modeuler", "rk4"):
        a = _kernel(HM.GrowthWithLatents, pb, solver, None, W=Z)
        b = _kernel(HM.GrowthWithoutNetworks, pb, solver, None, with_weights=False)
        for k in ("traj", "xpred", "logp"):
            e = rel_err(a[k], b[k], dim=2)
            print("%s %s: %.2e" % (solver, k, e))
            assert e < TOL


def test_dopri5_through_the_host_driven_controller():
    """The generated model's own step-size controller picks the accepted grid (forward only); the kernels then integrate on
    it with dopri5's tableau and run one adjoint (upstream gradient on the trajectory): compared with the float64 definition
    on the same accepted grid."""
    pb = _problem(5, 3, 12, 9)
    modelgen.register_kernel(HM.GrowthWithLatents, False)
    slots = hip.model_slots(HM.GrowthWithLatents.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV)
    spec = ops.OdeProblemSpec(HM.GrowthWithLatents.model_key, "dopri5", row_of, th.shape[0], C=1)
    grid, index = ops.adaptive_grid(spec, th, pb["cond"].float().to(DEV), pb["times"].float().to(DEV), None,
                                    _flat_weights(pb, None), rtol=1e-5, atol=1e-7)
    G = grid.shape[0]
    assert G >= pb["T"] and bool(torch.isfinite(grid).all()) and bool((grid[1:] > grid[:-1]).all())
    assert torch.equal(grid[index].cpu(), pb["times"].float())
    gen = torch.Generator().manual_seed(2)
    pb["g_traj"] = torch.randn(5, 3, 6, G, generator=gen, dtype=torch.float64)
    pb["T"] = G
    grid64 = grid.cpu().double()
    r64 = _definition(pb, "dopri5", None, torch.float64, grid=("dopri5", grid64))
    r32 = _definition(pb, "dopri5", None, torch.float32, grid=("dopri5", grid64))
    got = _kernel(HM.GrowthWithLatents, pb, "dopri5", None, times=grid, g_traj=pb["g_traj"])
    _compare(got, r64, r32, "dopri5", forward=("traj",))


def _hybrid_training(monkeypatch, cls, B=8, S=20, **over):
    import models
    from vihds import synthetic

    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    # the synthetic plate of a built-in workload whose spec defines every parameter the hybrid model reads (neural
    # precisions: the relay spec has the init_prec_* rows), observed through the hybrid model itself from other weights
    base = "relay_constant_precisions" if cls is HM.GrowthWithLatentsPrecisions else "dr_constant_icml"
    spec_fn, n_times = synthetic.WORKLOADS[base]
    monkeypatch.setitem(synthetic.WORKLOADS, "hybrid", (lambda solver: dict(spec_fn(solver), model=cls.model_key), n_times))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("hybrid",))
    return synthetic.build("hybrid", B, S, solver="midpoint", device=DEV, seed=3, **over)


@pytest.mark.parametrize("cls", [HM.GrowthWithLatents, HM.GrowthWithLatentsPrecisions])
def test_training_steps_eager_and_replayed_are_bit_identical(cls, monkeypatch, tmp_path):
    """A spec naming the hybrid model: 20 Training.steps eagerly and 20 from the hipGraph replay, from the same seeds --
    every loss and every parameter (network weights included) bit-identical, the general five-launch step taken, the
    network weights moved."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _hybrid_training(monkeypatch, cls, hip_graph=graph,
                                                                             n_hidden_decoder_precisions=0)
        assert training.use_graph == (graph is None)
        assert isinstance(model.decoder.ode_model, cls)
        w0 = [t.detach().clone() for t in model.decoder.ode_model.flat_weight_tensors()]
        batch = training.train_data
        log = TrainingLogData()
        np.random.seed(21)
        torch.manual_seed(21)
        losses = []
        orig_step = training.step

        def keeping(b, *a, _t=training, _o=orig_step, **k):
            _t.last_elbo = _o(b, *a, **k)
            return _t.last_elbo

        training.step = keeping
        for k in range(20):
            model.train()
            assert training._run_batch(0.0, batch, log, next_batch=batch)
            losses.append(float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo))
        torch.cuda.synchronize()
        assert training._gtail_ok is True, "the general step did not take the hybrid model"
        moved = [not torch.equal(a, b.detach()) for a, b in zip(w0, model.decoder.ode_model.flat_weight_tensors())]
        assert all(moved[:8]), moved
        runs[graph] = (losses, {k: v.detach().clone() for k, v in model.named_parameters()})
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert all(np.isfinite(x) for x in la)
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k


def test_training_lowers_the_loss_and_run_and_evaluate_complete(monkeypatch, tmp_path):
    """200 steps on the synthetic plate: the loss ends below the loss at step 0.  Then Training.run() (two epochs, graph
    capture) and Training.evaluate on a fresh model: finite Results arrays."""
    monkeypatch.chdir(tmp_path)
    cls = HM.GrowthWithLatents
    args, settings, data, parameters, model, training = _hybrid_training(monkeypatch, cls, hip_graph=False,
                                                                         learning_rate=0.002)
    batch = training.train_data
    model.train()
    losses = [float(training.step(batch)) for _ in range(200)]
    # (a -ELBO far below -|initial| is not a fit: it is the objective running away through log q of clipped samples, which
    # the spec's learning rate of 0.01 provokes on this plate after ~70 steps -- hence learning_rate below)
    print("loss at step 0 %.4f, after 200 steps %.4f (lowest %.4f, highest %.4f)" % (losses[0], losses[-1], min(losses), max(losses)))
    print("every 20th: " + " ".join("%.1f" % x for x in losses[::20]))
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert abs(losses[-1]) <= abs(losses[0]), "the objective ran away"
    args, settings, data, parameters, model, training = _hybrid_training(monkeypatch, cls)
    assert training.use_graph
    args.epochs, args.test_epoch = 2, 2
    result = training.run()
    assert result is not None and np.isfinite(float(result.elbo)) and training._steps > 0
    model.eval()
    res = training.evaluate(training.train_data, 20)
    assert res.iw_predict_mu.shape[:2] == (8, 4) and res.iw_states.shape[:2] == (8, 6)
    for name in ("iw_predict_mu", "iw_predict_std", "iw_states"):
        assert np.isfinite(getattr(res, name)).all(), name
    assert np.isfinite(float(res.elbo))


def test_summaries_list_the_network_tensors(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    args, settings, data, parameters, model, training = _hybrid_training(monkeypatch, HM.GrowthWithLatents, hip_graph=False)

    class Writer(object):
        def __init__(self):
            self.tags = []

        def add_scalar(self, tag, *a, **k):
            self.tags.append(tag)

        add_histogram = add_scalar

    w = Writer()
    model.decoder.ode_model.summaries(w, 0)
    for name in ("latent", "gate"):
        for layer in ("hidden", "out"):
            for kind in ("weights", "bias"):
                assert any("net_%s_%s_%s" % (name, layer, kind) in t for t in w.tags), (name, layer, kind, w.tags[:4])
