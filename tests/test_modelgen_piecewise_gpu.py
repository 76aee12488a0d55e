"""GPU tests of the piecewise operations of generated models (where, minimum, maximum, abs, sqrt, erf, erfc; fsel, fmin_nan,
fmax_nan, min_pass, max_pass, fsign, fsqrt of csrc/vihds_models.hpp): EveryPiecewiseOperation and PrprDosed against their own
definitions in float64 with every fixed-grid solver, PrprDosed through the host-driven adaptive controller, PlateReaderCensored
(a Tobit likelihood) through evaluation, one training step and the step's hipGraph replay, and the NaN rule.

Shapes: B=3, S=5 (one partly filled block) and B=3, S=100 (300 trajectories: a full block and a partial one); T=9.

Every comparison with float64 first asserts its precondition on the float64 run alone: the smallest margin |lhs - rhs| /
(|lhs| + |rhs| + 1) of every switch, at every point where the kernel evaluates it, is at least 1e-3 (modelgen_piecewise_models:
a float32 kernel and a float64 yardstick agree only where they take the same branches)."""
import numpy as np
import pytest
import torch

from fixture_util import rel_err
from oracle import vihds_oracle as O
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_noise_models as NM
import modelgen_piecewise_models as PM
from test_modelgen_noise_gpu import NOISE_BASE, _samples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4  # trajectory and x_predict per species / signal; log-likelihood per signal
_KEYS, _REFS = {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _definition(cls, pb, solver, dtype, grid=None):
    """The definition with torch ops in `dtype`, autograd for the gradient of sum(logp * G); in float64 the margins of its
    switches are recorded."""
    th = {n: v.to(dtype).detach().clone().requires_grad_(True) for n, v in pb["th"].items()}
    with PM.recording() as m:
        xs, xp, prec, logp = PM.forward(cls, th, pb["cond"].to(dtype), pb["times"].to(dtype), solver, pb["obs"].to(dtype), grid=grid)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    full = torch.cat([xs, prec], dim=2) if cls._precision_def is not None else xs
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: v.grad for n, v in th.items()}, "margins": m}


def _reference(cls, B, S, solver):
    k = (cls, B, S, solver)
    if k not in _REFS:
        pb = PM.problem(cls, B, S)
        _REFS[k] = (_definition(cls, pb, solver, torch.float64), _definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, th=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == PM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([(th or pb["th"])[n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=1)
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"]), None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _precondition(r64, label):
    m = r64["margins"]
    worst = min(m.by_label, key=m.by_label.get)
    print("%s: smallest switch margin %.2e (%s)" % (label, m.smallest, worst))
    assert m.smallest >= PM.MARGIN, "badly posed inputs: %s has margin %.2e" % (worst, m.smallest)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k


def _compare(got, r64, r32, label):
    """Prints every figure, then asserts: forward 1e-5 (log-likelihood 1e-4), the loss within max(1e-6, 8 x the float32 torch
    run's error), every theta row within max(1e-4, 8 x the float32 torch run's error)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        if not e <= bound:
            bad.append(lines[-1])

    check("traj", rel_err(got["traj"], r64["traj"], dim=2), TOL)
    check("xpred", rel_err(got["xpred"], r64["xpred"], dim=2), TOL)
    check("logp", rel_err(got["logp"], r64["logp"], dim=2), TOL_LOGP)
    scale = abs(float(r64["loss"]))
    check("loss", abs(float(got["loss"]) - float(r64["loss"])) / scale,
          max(1e-6, 8 * abs(float(r32["loss"]) - float(r64["loss"])) / scale))
    for n, g in r64["g_theta"].items():
        if g is None or float(g.abs().max()) == 0.0:
            assert float(got["g_theta"][n].abs().max()) == 0.0, n  # (a parameter the loss does not reach: tau, thr)
            continue
        check("g_theta[%s]" % n, rel_err(got["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g)))
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", PM.FIXED)
@pytest.mark.parametrize("cls", [PM.EveryPiecewiseOperation, PM.PrprDosed], ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, against
    torch_problem + O.simulate and the torch maps in float64."""
    B, S = shape
    r64, r32 = _reference(cls, B, S, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(r64, label)
    pb = PM.problem(cls, B, S)
    got = _kernel(cls, pb, solver)
    _compare(got, r64, r32, label)
    if cls is PM.EveryPiecewiseOperation:
        # `boost` is read inside one where branch: its row is non-zero on the trajectories that take the branch at some
        # stage, and exactly zero on those that never do (dosed after the end of the grid, or never dense enough)
        ref, g = r64["g_theta"]["boost"], got["g_theta"]["boost"]
        taken = ref != 0
        assert bool(taken.any()) and bool((~taken).any())
        assert bool((pb["th"]["tau"] > pb["times"][-1])[~taken].any())
        assert bool((g[taken] != 0).all()) and bool((g[~taken] == 0).all())
        # a switch time and a threshold get no gradient through the condition
        for n in ("tau", "thr"):
            assert float(got["g_theta"][n].abs().max()) == 0.0, n
        censored = pb["obs"][:, None, 1] >= pb["th"]["ceil"][:, :, None]
        assert bool(censored.any()) and bool((~censored).any())
    else:
        # the row dosed after the end keeps its production off: YFP decays only, and aYFP_PR gets no gradient there
        assert float(got["g_theta"]["aYFP_PR"][2].abs().max()) == 0.0 and float(got["g_theta"]["aYFP_PR"][:2].abs().min()) > 0.0


def test_dosed_model_through_the_host_driven_adaptive_controller():
    """PrprDosed with dopri5: ops.adaptive_grid runs the generated model's own controller, whose rhs sees the switch; the
    accepted grid is handed to the kernel and to the float64 definition, the margins are taken on that grid.  rtol 1e-3 /
    atol 1e-5: a controller that resolves the jump to 1e-7 ends with a step whose stages sit within 1e-7 of the switch
    time, where no float32 and float64 run can be asked to agree."""
    cls, (B, S) = PM.PrprDosed, SHAPES[0]
    base = PM.problem(cls, B, S)
    key = _key(cls)
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([base["th"][n] for n in slots]).float().to(DEV)
    spec = ops.OdeProblemSpec(key, "dopri5", row_of, th.shape[0], C=1)
    grid, index = ops.adaptive_grid(spec, th, base["cond"].float().to(DEV), base["times"].float().to(DEV), None, None,
                                    rtol=1e-3, atol=1e-5)
    n_grid = grid.shape[0]
    assert n_grid >= base["T"] and bool(torch.isfinite(grid).all()) and bool((grid[1:] > grid[:-1]).all())
    assert torch.equal(grid[index].cpu(), base["times"].float())
    grid64 = grid.cpu().double()
    gen = torch.Generator().manual_seed(2)
    pb = dict(base, times=grid64, T=n_grid)
    whole = (grid64.tolist(), list(range(n_grid)))
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in base["th"].items()}
        _, xp, _, _ = PM.forward(cls, th1, base["cond"], grid64, "dopri5", grid=whole)
        pb["obs"] = xp[:, 0] * (1.0 + 0.05 * torch.randn(B, 4, n_grid, generator=gen, dtype=torch.float64))
    r64 = _definition(cls, pb, "dopri5", torch.float64, grid=whole)
    r32 = _definition(cls, pb, "dopri5", torch.float32, grid=whole)
    label = "PrprDosed dopri5, %d grid points" % n_grid
    _precondition(r64, label)
    _compare(_kernel(cls, pb, "dopri5"), r64, r32, label)


def test_a_trajectory_that_goes_nan_stays_nan():
    """One trajectory's q makes sqrt(q + P) see a negative value: its Q (which takes maximum(root, 0.05): fmaxf would return
    0.05) and everything computed from it are NaN from the first step on; the other trajectories are bit-identical to the run
    without it."""
    cls, (B, S) = PM.EveryPiecewiseOperation, SHAPES[0]
    pb = PM.problem(cls, B, S)
    clean = _kernel(cls, pb, "rk4")
    th = {n: v.clone() for n, v in pb["th"].items()}
    th["q"][1, 2] = -5.0
    got = _kernel(cls, pb, "rk4", th=th)
    bad = torch.zeros(B, S, dtype=torch.bool)
    bad[1, 2] = True
    iq = cls.species.index("Q")
    assert bool(torch.isnan(got["traj"][1, 2, iq, 1:]).all()) and bool(torch.isnan(got["logp"][1, 2]).any())
    assert bool(torch.isnan(got["xpred"][1, 2, 3, 1:]).all())
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(got[k][~bad]).all()), k
        assert torch.equal(got[k][~bad], clean[k][~bad]), k
    for n in got["g_theta"]:
        assert torch.equal(got["g_theta"][n][~bad], clean["g_theta"][n][~bad]), n
    # the float64 definition says the same
    with torch.no_grad():
        xs, _, _, _ = PM.forward(cls, th, pb["cond"], pb["times"], "rk4", pb["obs"])
    assert torch.equal(torch.isnan(xs[:, :, iq, 1:]).all(-1), bad)


# ---- training: the censored plate reader through the plugin surface ----------------------------------------------------------
N_PLATE = 20
CEILING = 0.6  # what the saturated detector reports (the synthetic plate's signals are scaled to a maximum of 1)
CEIL_PRIOR = (float(np.log(0.54)), 0.01)  # the model's ceiling: every draw below CEILING and above the readings left alone
LEFT_ALONE = 0.45  # the fluorescence readings are rescaled so that 70 % lie below it; the others are replaced by CEILING
PASS_SEED = 12  # draws of the evaluation pass: of the seeds 1 .. 12, one whose float64 yardstick keeps every switch 1e-3 wide (9.6e-3)


def _censored_training(monkeypatch, B, S, solver="rk4", **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names PlateReaderCensored (registered through
    models.register, selected with `model:`); the largest 30 % of the fluorescence readings are replaced by CEILING."""
    import models
    from vihds import synthetic

    cls = PM.PlateReaderCensored
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        glob = spec["params"]["global"]
        glob.update({"gain_r": ln(0.3, 0.2), "bg_r": ln(-3.0, 0.2), "sat": ln(-0.5, 0.2), "auto": ln(-1.2, 0.2),
                     "leak": ln(-1.0, 0.2), "ceil": ln(*CEIL_PRIOR)})
        glob.update({n: ln(float(np.log(v)), 0.2) for n, v in NOISE_BASE.items()})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "reader_censored", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("reader_censored",))
    out = synthetic.build("reader_censored", B, S, solver=solver, device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.likelihood_kind == "custom" and ode.precision_kind == "custom"
    batch = out[5].train_data
    obs = batch.observations.clone()
    fl = obs[:, 1:]
    q70 = torch.quantile(fl.flatten(), 0.7)
    assert float(q70) > 0.0
    fl = fl * (LEFT_ALONE / q70)  # (the plate's fluorescence rescaled so that 30 % of its readings lie above LEFT_ALONE)
    at_ceiling = fl > LEFT_ALONE
    obs[:, 1:] = torch.where(at_ceiling, torch.full_like(fl, CEILING), fl)
    batch.observations.copy_(obs)  # (in place: the step's static copies are made from this tensor)
    # a known subset sits at the ceiling -- the 30 % largest readings -- and the rest well below every draw of the ceiling
    assert abs(float(at_ceiling.float().mean()) - 0.3) < 0.02 and bool((obs[:, 1:][at_ceiling] == CEILING).all())
    assert bool((obs[:, 1:][~at_ceiling] <= LEFT_ALONE).all())
    return out + (at_ceiling.cpu(),)


def _float64_censored(samples, batch, solver):
    """The decoder with the model's own map, noise and Tobit density, and the importance weights, in float64 from the samples
    of one pass; the margins of its switches."""
    cls = PM.PlateReaderCensored
    th, log_p, log_q = samples
    cond, times = batch.inputs.double().cpu(), batch.times.double().cpu()
    with PM.recording() as m:
        xs, xp, prec, logp = PM.forward(cls, th, cond, times, solver, batch.observations.double().cpu())
    return logp, logp.sum(2) + log_p - log_q, m


def test_evaluation_pass_of_the_censored_reader(monkeypatch, tmp_path):
    """Training.evaluate at B=3, S=5: the ELBO is within 1e-4 relative of the one formed in float64 from the pass's own
    samples with the model's definition; both likelihood branches are taken (the readings at the ceiling are above every
    sampled ceiling, the others below)."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training, at_ceiling = _censored_training(monkeypatch, B, S, hip_graph=False)
    cls = PM.PlateReaderCensored
    model.eval()
    seen = {}
    cost = training.cost

    def spy(batch, results, theta, q, p, **kw):
        seen.update(batch=batch, samples=_samples(cls, theta, q, p))
        return cost(batch, results, theta, q, p, **kw)

    monkeypatch.setattr(training, "cost", spy)
    np.random.seed(PASS_SEED)
    torch.manual_seed(PASS_SEED)
    res = training.evaluate(training.train_data, S)
    logp, log_w, m = _float64_censored(seen["samples"], seen["batch"], "rk4")
    worst = min(m.by_label, key=m.by_label.get)
    print("smallest switch margin %.2e (%s)" % (m.smallest, worst))
    assert m.smallest >= PM.MARGIN, "badly posed inputs: %s has margin %.2e" % (worst, m.smallest)
    ceil = seen["samples"][0]["ceil"]
    censored = seen["batch"].observations.double().cpu()[:, None, 1:] >= ceil[:, :, None, None]
    assert torch.equal(censored, at_ceiling[:, None].expand_as(censored))
    ref = float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    got = float(np.asarray(res.elbo))
    print("elbo %.6f, float64 %.6f" % (got, ref))
    assert bool(torch.isfinite(logp).all()) and abs(got - ref) <= 1e-4 * abs(ref)


def test_one_training_step_of_the_censored_reader(monkeypatch, tmp_path):
    """One Training.step through the general path: every encoder gradient is finite, the ceiling and the noise parameters
    move, and the data take both likelihood branches."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training, at_ceiling = _censored_training(monkeypatch, B, S, hip_graph=False)
    batch = training.train_data
    model.train()
    seen = {}
    tail = training._general_tail

    def spy(results, theta, q, p):
        seen["ceil"] = theta.ceil.detach().double().cpu()
        return tail(results, theta, q, p)

    monkeypatch.setattr(training, "_general_tail", spy)
    enc = model.encoder
    glob_names = [d.name for d in enc.glob]
    assert all(n in glob_names for n in NM.NOISE + ["ceil"])
    before = enc.global_free.detach().clone()
    np.random.seed(21)
    torch.manual_seed(21)
    loss = float(training.step(batch, zero_grad=False))
    torch.cuda.synchronize()
    assert training._gtail_ok is True, "the general step did not take the model"
    assert np.isfinite(loss)
    censored = batch.observations.double().cpu()[:, None, 1:] >= seen["ceil"][:, :, None, None]
    assert torch.equal(censored, at_ceiling[:, None].expand_as(censored)) and bool(censored.any()) and bool((~censored).any())
    grads = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert any(k.startswith("encoder.") for k in grads)
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
    after = enc.global_free.detach()
    for n in NM.NOISE + ["ceil"]:
        k = glob_names.index(n)
        assert not torch.equal(before[:, k], after[:, k]), n


def test_training_steps_eager_and_replayed_are_bit_identical(monkeypatch, tmp_path):
    """Five Training.steps eagerly and five from the step's hipGraph replay, from the same seeds: every loss and every
    parameter bit-identical."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training, _ = _censored_training(monkeypatch, 3, 5, hip_graph=graph)
        assert training.use_graph == (graph is None)
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
        for k in range(5):
            model.train()
            assert training._run_batch(0.0, batch, log, next_batch=batch)
            losses.append(float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo))
        torch.cuda.synchronize()
        assert training._gtail_ok is True, "the general step did not take the model"
        runs[graph] = (losses, {k: v.detach().clone() for k, v in model.named_parameters()})
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert all(np.isfinite(x) for x in la)
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
