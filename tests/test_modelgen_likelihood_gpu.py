"""GPU tests of a generated model's own observation log density (GeneratedOdeModel.log_likelihood, own_lik<> in the kernels):
the Gaussian written out against the kernels' own term on the same numbers, a Student-t (its own observe and precision) and a
contaminated Gaussian (constant precisions, two likelihood-only parameters) against their own definitions in float64, the
host-driven adaptive route, an evaluation pass and one training step.

Shapes (B, S): (3, 5) one partly filled wavefront; (5, 26) rows that straddle wavefronts; (3, 100) 300 trajectories, so that
a data row straddles two blocks of the LDS-staged forward; T=7 on a non-uniform grid.  (40, 1) at T=64 on a uniform grid: the
staged inputs would take (64 + 40 * 4 * 64) * 4 = 41 216 bytes, more than the launcher's 32 KB, so the forward that reads the
observations from global memory runs.

Observations: the float64 prediction of each data row's first sample with 5 % multiplicative noise; one time point per signal
and data row is then displaced by eight standard deviations (8 / sqrt(precision)) -- an outlier, where a heavy-tailed density
and the Gaussian differ by tens of nats."""
import numpy as np
import pytest
import torch

from fixture_util import rel_err
from oracle import vihds_oracle as O
from vihds import hip, ops

import hip_util as H
import modelgen_likelihood_models as LM
import modelgen_models as MM
import modelgen_noise_models as NM
from test_modelgen_noise_gpu import GTOL, NOISE_BASE, TOL, _key, _samples, _spread
from test_modelgen_observe_gpu import PRPR_BASE, READER_BASE, TIMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (5, 26), (3, 100)]
UNSTAGED = (40, 1, 64)  # (B, S, T) of the case whose staged inputs exceed 32 KB
CONTAMINATION_BASE = {"eps": -2.0, "kappa": 5.0}  # (sigmoid(-2) = 0.12 of the readings, five times the standard deviation)
_PROBLEMS, _REFS = {}, {}


def _times(T):
    if T == len(TIMES):
        return torch.tensor(TIMES, dtype=torch.float64)
    return 0.06 * torch.arange(T, dtype=torch.float64)  # (uniform: 0 .. 3.78, the span of TIMES)


def _base(cls):
    if issubclass(cls, NM.PlateReaderNoise):
        return dict({n: v for n, v in READER_BASE.items() if not n.startswith("prec_")}, **NOISE_BASE)
    base = {n: v for n, v in PRPR_BASE.items() if not n.startswith("init_prec_")}
    if cls is LM.PrprContaminated:
        base.update(CONTAMINATION_BASE)
    return base


def _slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else MM.PREC)


def _forward(cls, th, cond, times, solver):
    """-> species [B,S,N,T], x_predict [B,S,4,T], precisions [B,S,4,T] in the dtype of th."""
    rhs, x0 = cls.torch_problem(th, cond)
    xs = O.simulate(rhs, x0, times, solver)
    xp = cls.torch_observe(xs, th, cond) if cls._observe_def is not None else O.observe_default(xs)
    if cls._precision_def is not None:
        prec = cls.torch_precision(xs, th, cond)
    else:
        prec = torch.stack([th[n] for n in MM.PREC], dim=2)[:, :, :, None].expand_as(xp)
    return xs, xp, prec


def _problem(cls, B, S, T=len(TIMES)):
    """Inputs of one case (shared by the tests that use it; never modified)."""
    k = (cls, B, S, T)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    base = _base(cls)
    assert sorted(base) == sorted(_slot_names(cls))
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    N = len(cls.species)
    rows = N + (4 if cls._precision_def is not None else 0)
    pb = {"th": _spread(base, B, S, 6), "cond": torch.log1p(2.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64)),
          "times": _times(T), "B": B, "S": S, "T": T}
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in pb["th"].items()}
        xs, xp, prec = _forward(cls, th1, pb["cond"], pb["times"], "rk4")
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
        where = torch.randint(0, T, (B, 4, 1), generator=gen)
        obs.scatter_add_(2, where, 8.0 / prec[:, 0].gather(2, where).sqrt())
        pb["obs"] = obs
    pb["G"] = {"logp": rnd(B, S, 4), "xpred": rnd(B, S, 4, T), "traj": rnd(B, S, rows, T)}
    _PROBLEMS[k] = pb
    return pb


def _reference(cls, B, S, T, solver, upstream):
    """torch_problem integrated by the oracle's step functions, the observation map, the precisions, torch_log_likelihood,
    autograd -- in float64, once per case.  Also the Gaussian log-likelihood of the same inputs (what the kernels computed
    for such a class before the method existed)."""
    k = (cls, B, S, T, solver, upstream)
    if k not in _REFS:
        pb = _problem(cls, B, S, T)
        th = {n: v.detach().clone().requires_grad_(True) for n, v in pb["th"].items()}
        xs, xp, prec = _forward(cls, th, pb["cond"], pb["times"], solver)
        logp = cls.torch_log_likelihood(xp, pb["obs"], prec, th, pb["cond"]).sum(3)
        loss = (logp * pb["G"]["logp"]).sum()
        full = torch.cat([xs, prec], dim=2) if cls._precision_def is not None else xs
        if upstream:
            loss = loss + (xp * pb["G"]["xpred"]).sum() + (full * pb["G"]["traj"]).sum()
        loss.backward()
        _REFS[k] = {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(),
                    "gauss": O.log_prob_observations(xp, pb["obs"], prec).detach(),
                    "g_theta": {n: v.grad for n, v in th.items()}}
    return _REFS[k]


def _kernel(cls, B, S, T, solver, upstream, key_cls=None):
    """Forward and adjoint of `key_cls` (default cls) on the inputs of cls's case."""
    pb = _problem(cls, B, S, T)
    key = _key(key_cls or cls)
    slots = hip.model_slots(key)
    assert slots == _slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=1)
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"]), None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    if upstream:
        loss = loss + (H.view_bsnt(xpred) * f32(pb["G"]["xpred"])).sum() + (H.view_bsnt(traj) * f32(pb["G"]["traj"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _not_vacuous(cls, ref, only):
    """On the float64 reference alone: the model's log-likelihood is not the Gaussian's, every likelihood-only parameter has
    a gradient everywhere, nothing is infinite."""
    for j in range(4):
        d = float((ref["logp"][:, :, j] - ref["gauss"][:, :, j]).abs().max() / ref["gauss"][:, :, j].abs().max())
        assert d > 100 * TOL, (j, d)
    for n in only:
        assert float(ref["g_theta"][n].abs().min()) > 0.0, n
    for k in ("traj", "xpred", "logp", "gauss"):
        assert bool(torch.isfinite(ref[k]).all()), k
    for n, g in ref["g_theta"].items():
        assert g is not None and bool(torch.isfinite(g).all()), n


def _compare(got, ref, label):
    """Prints every figure, then asserts the bounds of DESIGN.md section 2."""
    lines, bad = [], []
    for k in ("traj", "xpred", "logp"):
        e = rel_err(got[k], ref[k], dim=2)
        lines.append("%s %s: %.2e (bound %.0e)" % (label, k, e, TOL))
        if not e <= TOL:
            bad.append(lines[-1])
    for n, g in ref["g_theta"].items():
        e = rel_err(got["g_theta"][n], g)
        lines.append("%s g_theta[%s]: %.2e (bound %.0e)" % (label, n, e, GTOL))
        if not e <= GTOL:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


CASES = [(B, S, len(TIMES), solver, upstream) for (B, S) in SHAPES for solver in ("rk4", "modeuler") for upstream in (False, True)]
CASES.append(UNSTAGED + ("rk4", True))
_ids = lambda c: "%dx%dxT%d-%s-%s" % (c[0], c[1], c[2], c[3], "upstream" if c[4] else "logp")  # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gaussian_written_out_against_the_kernels_own_term(case):
    """PrprGaussianThrough (the Gaussian as the model's log_likelihood) and plain PrprRestated on the same theta buffer,
    observations and upstream gradients: trajectory, x_predict, log-likelihood and every row of g_theta -- the prec_* rows,
    which the own branch fills from loglik_vjp's prb, included -- within 1e-5 (two float32 routes: the built-in branch folds
    log 2 pi - log prec once per trajectory, the own branch forms it per time point).

    At the unstaged shape (40, 1), T=64 the prec_* rows are held to float64 at 5e-4 on BOTH routes
    instead of to each other at 1e-5; every other figure keeps the 1e-5.  There that comparison is ill-conditioned by
    construction: with one sample per data row the outlier sits at exactly 8 / sqrt(prec) of that sample, so the Gaussian's
    prec_* gradient sum_t glp (0.5 / prec - 0.5 e^2) is 64 * 0.5 / prec - 0.5 * 64 / prec plus what the 5 % noise leaves: the
    65 terms cancel to about 0.6 % of their size, and two float32 routes that round the terms differently (a few 1e-7
    relative each: `0.5f / pr` against the time-loop reciprocal) differ by a few 1e-5 of the rest.  Measured on an MI355X:
    2.6e-5 between the routes on those rows, trajectory, x_predict and log-likelihood bit-identical; 1.1e-7 .. 3.5e-7 on all
    rows at the T=7 shapes."""
    B, S, T, solver, upstream = case
    cancelling = (B, S, T) == UNSTAGED
    ref = _kernel(LM.PrprGaussianThrough, B, S, T, solver, upstream, key_cls=MM.PrprRestated)
    got = _kernel(LM.PrprGaussianThrough, B, S, T, solver, upstream)
    rows = [n for n in _slot_names(MM.PrprRestated) if not (cancelling and n in MM.PREC)]
    stack = lambda d: torch.stack([d["g_theta"][n] for n in rows])  # noqa: E731
    figures = {"traj": rel_err(got["traj"], ref["traj"]), "xpred": rel_err(got["xpred"], ref["xpred"]),
               "logp": rel_err(got["logp"], ref["logp"], dim=2), "g_theta": rel_err(stack(got), stack(ref), dim=0)}
    print("%s: %s" % (_ids(case), "  ".join("%s %.2e" % kv for kv in figures.items())))
    for n in MM.PREC:  # (every prec_* row has a gradient to compare)
        assert float(ref["g_theta"][n].abs().max()) > 0.0, n
    if cancelling:
        f64 = _reference(LM.PrprGaussianThrough, B, S, T, solver, upstream)
        for n in MM.PREC:
            e_own, e_ref = rel_err(got["g_theta"][n], f64["g_theta"][n]), rel_err(ref["g_theta"][n], f64["g_theta"][n])
            print("%s g_theta[%s] against float64: own %.2e, built-in %.2e (bound %.0e)" % (_ids(case), n, e_own, e_ref, GTOL))
            assert e_own <= GTOL and e_ref <= GTOL, (n, e_own, e_ref)
    for name, e in figures.items():
        assert e < 1e-5, (name, e)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_student_t_against_its_own_definition_in_float64(case):
    """PlateReaderStudentT (its own observe, its own precision, a Student-t of 4 degrees of freedom): species, the stored
    precision rows, x_predict and the log-likelihood within 1e-4 per signal, every row of g_theta within 5e-4.  The noise
    parameters reach theta only through loglik_vjp's prb and precision_vjp; `upstream` adds gradients on x_predict and on
    all rows of the trajectory."""
    B, S, T, solver, upstream = case
    cls = LM.PlateReaderStudentT
    ref = _reference(cls, B, S, T, solver, upstream)
    _not_vacuous(cls, ref, NM.NOISE)
    _compare(_kernel(cls, B, S, T, solver, upstream), ref, _ids(case))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_contaminated_gaussian_against_its_own_definition_in_float64(case):
    """PrprContaminated (constant precisions, the default map, a two-component scale mixture): the same comparison; eps and
    kappa are read by log_likelihood only (loglik_vjp's pb ahead of prepare_vjp), the prec_* rows come from its prb."""
    B, S, T, solver, upstream = case
    cls = LM.PrprContaminated
    ref = _reference(cls, B, S, T, solver, upstream)
    _not_vacuous(cls, ref, LM.CONTAMINATION + MM.PREC)
    _compare(_kernel(cls, B, S, T, solver, upstream), ref, _ids(case))


# ---- the host paths -------------------------------------------------------------------------------------------------------
N_PLATE = 20


def _student_training(monkeypatch, B, S, solver="rk4", **over):
    """Config -> Parameters -> model -> Training on a synthetic plate of N_PLATE time points whose spec names
    PlateReaderStudentT and gives every parameter it reads a prior; the observations are simulated from the model itself."""
    import models
    from vihds import synthetic

    cls = LM.PlateReaderStudentT
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        glob = spec["params"]["global"]
        glob.update({"gain_r": ln(0.3, 0.2), "bg_r": ln(-3.0, 0.2), "sat": ln(-0.5, 0.2), "auto": ln(-1.2, 0.2),
                     "leak": ln(-1.0, 0.2)})
        glob.update({n: ln(float(np.log(v)), 0.2) for n, v in NOISE_BASE.items()})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "reader_student_t", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("reader_student_t",))
    out = synthetic.build("reader_student_t", B, S, solver=solver, device=DEV, seed=3, **over)
    assert isinstance(out[4].decoder.ode_model, cls) and out[4].decoder.ode_model.likelihood_kind == "custom"
    return out


def _float64_student(samples, batch, solver, grid=None):
    """The decoder with the model's own log density and the importance weights in float64 from the samples of one pass."""
    cls = LM.PlateReaderStudentT
    th, log_p, log_q = samples
    cond, times = batch.inputs.double().cpu(), batch.times.double().cpu()
    rhs, x0 = cls.torch_problem(th, cond)
    xs = O.simulate(rhs, x0, times, solver, **({"grid": grid} if grid is not None else {}))
    xp, prec = cls.torch_observe(xs, th, cond), cls.torch_precision(xs, th, cond)
    obs = batch.observations.double().cpu()
    logp = cls.torch_log_likelihood(xp, obs, prec, th, cond).sum(3)
    return logp, O.log_prob_observations(xp, obs, prec), logp.sum(2) + log_p - log_q


def test_host_driven_adaptive_route_takes_the_model_definition(monkeypatch, tmp_path):
    """dopri5 through OdeModel.solve: a registered model takes the host-driven controller, whose log-likelihood is formed by
    torch ops on the gathered rows -- with the model's own definition.  Against float64 on the accepted grid: 1e-4 per
    signal; and it is not the Gaussian's."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _student_training(monkeypatch, B, S, solver="dopri5", hip_graph=False)
    cls = LM.PlateReaderStudentT
    ode = model.decoder.ode_model
    model.eval()
    batch = training.train_data
    np.random.seed(5)
    torch.manual_seed(5)
    with torch.no_grad():
        results, theta, q, p = model(batch, S)
    torch.cuda.synchronize()
    grid = ode.last_adaptive_grid
    assert grid is not None, "the device-resident solver took a registered model"
    grid = grid.double().cpu()
    index = [int((grid - float(t)).abs().argmin()) for t in batch.times.cpu()]
    assert all(float(grid[i]) == float(t) for i, t in zip(index, batch.times.cpu()))
    logp, gauss, _ = _float64_student(_samples(cls, theta, q, p), batch, "dopri5", grid=(grid.tolist(), index))
    got = results.solution.log_p_by_species.detach().double().cpu()
    e = rel_err(got, logp, dim=2)
    print("dopri5, %d grid points: logp %.2e" % (grid.shape[0], e))
    for j in range(4):
        assert float((logp[:, :, j] - gauss[:, :, j]).abs().max() / gauss[:, :, j].abs().max()) > 100 * TOL, j
    assert bool(torch.isfinite(logp).all()) and e <= TOL


def test_evaluation_pass_of_a_model_with_its_own_likelihood(monkeypatch, tmp_path):
    """Training.evaluate on PlateReaderStudentT at B=3, S=5: the ELBO equals the one formed in float64 from the pass's own
    samples with the model's definition within 1e-4 relative, and is not the Gaussian model's."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _student_training(monkeypatch, B, S, hip_graph=False)
    cls = LM.PlateReaderStudentT
    model.eval()
    seen = {}
    cost = training.cost

    def spy(batch, results, theta, q, p, **kw):
        seen.update(batch=batch, samples=_samples(cls, theta, q, p))
        return cost(batch, results, theta, q, p, **kw)

    monkeypatch.setattr(training, "cost", spy)
    res = training.evaluate(training.train_data, S)
    logp, gauss, log_w = _float64_student(seen["samples"], seen["batch"], "rk4")
    ref = float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    other = float((torch.logsumexp(log_w - logp.sum(2) + gauss.sum(2), dim=1) - np.log(S)).mean())
    got = float(np.asarray(res.elbo))
    print("elbo %.6f, float64 %.6f (Gaussian on the same samples: %.6f)" % (got, ref, other))
    assert abs(other - ref) > 100 * TOL * abs(ref)
    assert abs(got - ref) <= TOL * abs(ref)


def test_one_training_step_through_the_general_path(monkeypatch, tmp_path):
    """One Training.step on PlateReaderStudentT through the general step (ops.GeneralTail, vihds_ode_bwd_elbo) with fixed
    draws: the loss equals the -ELBO formed in float64 from the step's own samples within 1e-4 relative.  The model has no
    parameter that only log_likelihood reads (its degrees of freedom are a number); its noise parameters reach the encoder
    only through the log density's adjoint (loglik_vjp's prb, then precision_vjp, then prepare_vjp): their columns move."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _student_training(monkeypatch, B, S, hip_graph=False)
    cls = LM.PlateReaderStudentT
    batch = training.train_data
    model.train()
    seen = {}
    tail = training._general_tail

    def spy(results, theta, q, p):  # (the step's own samples, copied before the tail's launches update anything)
        seen["samples"] = _samples(cls, theta, q, p)
        return tail(results, theta, q, p)

    monkeypatch.setattr(training, "_general_tail", spy)
    enc = model.encoder
    glob_names = [d.name for d in enc.glob]
    assert all(n in glob_names for n in NM.NOISE)
    before = enc.global_free.detach().clone()
    np.random.seed(21)
    torch.manual_seed(21)
    loss = float(training.step(batch))
    torch.cuda.synchronize()
    assert training._gtail_ok is True, "the general step did not take the model"
    logp, gauss, log_w = _float64_student(seen["samples"], batch, "rk4")
    ref = -float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    other = -float((torch.logsumexp(log_w - logp.sum(2) + gauss.sum(2), dim=1) - np.log(S)).mean())
    print("loss %.6f, float64 %.6f (Gaussian on the same samples: %.6f)" % (loss, ref, other))
    assert abs(other - ref) > 100 * TOL * abs(ref)
    assert abs(loss - ref) <= TOL * abs(ref)
    after = enc.global_free.detach()
    for n in NM.NOISE:
        k = glob_names.index(n)
        assert not torch.equal(before[:, k], after[:, k]), n


# ---- constant precisions through the host paths: the prpr_constant plate --------------------------------------------------
def _prpr_training(monkeypatch, cls, solver=None, **over):
    """Config -> Parameters -> model -> Training from the recorded prpr_constant experiment with `model:` naming cls (constant
    precisions: prec_x .. prec_cfp are global parameters of the spec), priors for the two contamination parameters, a data
    precision prior of e^3 (residuals of a few standard deviations, not hundreds) and initial states above zero."""
    import json

    import e2e_util as E
    import models
    from fixture_util import Fixture
    from vihds.config import Config
    from vihds.parameters import Parameters
    from vihds.training import Training
    from vihds.vae import build_model

    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    fx = Fixture("prpr_constant_tiny_modeuler")
    spec = json.loads(str(fx.z["spec_json"]))
    spec["model"] = cls.model_key
    spec["params"]["solver"] = solver or fx.solver
    spec["params"]["shared"]["data_prec"]["mu"] = 3.0
    spec["params"]["constant"].update({"init_rfp": 0.05, "init_yfp": 0.05, "init_cfp": 0.05})
    if cls is LM.PrprContaminated:
        spec["params"]["global"].update({"eps": {"distribution": "LogNormal", "mu": -1.0, "sigma": 0.2},
                                         "kappa": {"distribution": "LogNormal", "mu": float(np.log(5.0)), "sigma": 0.2}})
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
    training = Training(args, settings, data, parameters, model)
    batch = E.batch_from_fixture(fx, settings.device)
    batch.observations = batch.observations.clamp_min(0.02)  # (a log-scale density needs observations above zero)
    assert isinstance(model.decoder.ode_model, cls) and model.decoder.ode_model.likelihood_kind == "custom"
    return fx, settings, model, training, batch


def _float64_prpr(cls, theta, q, p, batch, solver, grid=None):
    """The decoder with the model's own log density in float64 from the samples of one pass -> logp [B,S,4], Gaussian logp,
    log importance weights."""
    th = {n: getattr(theta, n).detach().double().cpu() for n in _slot_names(cls)}
    cond, times = batch.inputs.double().cpu(), batch.times.double().cpu()
    rhs, x0 = cls.torch_problem(th, cond)
    xs = O.simulate(rhs, x0, times, solver, **({"grid": grid} if grid is not None else {}))
    xp = O.observe_default(xs)
    prec = torch.stack([th[n] for n in MM.PREC], dim=2)[:, :, :, None].expand_as(xp)
    obs = batch.observations.double().cpu()
    logp = cls.torch_log_likelihood(xp, obs, prec, th, cond).sum(3)
    ratio = p.log_prob(theta).detach().double().cpu() - q.log_prob(theta).detach().double().cpu()
    gauss = O.log_prob_observations(xp, obs, prec)
    return logp, gauss, logp.sum(2) + ratio, gauss.sum(2) + ratio


@pytest.mark.parametrize("cls", [LM.PrprContaminated, LM.PrprLogNormal], ids=lambda c: c.__name__)
def test_adaptive_route_with_constant_precisions_differentiates(cls, monkeypatch, tmp_path):
    """dopri5 through the decoder WITH a backward pass.  The host-driven route integrates on placeholder observations (zeros)
    and forms the log-likelihood with torch ops, so the adjoint kernel gets no log-likelihood gradient: it must skip
    loglik_vjp, not multiply it by zero -- PrprLogNormal's density is singular at an observation of zero (0 * inf).  Every
    encoder gradient is finite, the likelihood-only parameters' included; the log-likelihood (the constant-precision arm of
    the host formula) is within 1e-4 per signal of float64 on the accepted grid."""
    monkeypatch.chdir(tmp_path)
    fx, settings, model, training, batch = _prpr_training(monkeypatch, cls, solver="dopri5", hip_graph=False,
                                                          solver_rtol=1e-5, solver_atol=1e-7)
    ode = model.decoder.ode_model
    model.train()
    np.random.seed(5)
    torch.manual_seed(5)
    results, theta, q, p = model(batch, fx.S)
    got = results.solution.log_p_by_species
    got.sum().backward()
    torch.cuda.synchronize()
    grid = ode.last_adaptive_grid
    assert grid is not None, "the device-resident solver took a registered model"
    grid = grid.double().cpu()
    index = [int((grid - float(t)).abs().argmin()) for t in batch.times.cpu()]
    logp, gauss, _, _ = _float64_prpr(cls, theta, q, p, batch, "dopri5", grid=(grid.tolist(), index))
    e = rel_err(got.detach().double().cpu(), logp, dim=2)
    print("%s dopri5, %d grid points: logp %.2e" % (cls.__name__, grid.shape[0], e))
    assert bool(torch.isfinite(logp).all()) and e <= TOL
    for j in range(4):
        assert float((logp[:, :, j] - gauss[:, :, j]).abs().max() / gauss[:, :, j].abs().max()) > 100 * TOL, j
    grads = {k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    assert grads
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
    enc = model.encoder
    glob_names = [d.name for d in enc.glob]
    for n in (LM.CONTAMINATION if cls is LM.PrprContaminated else []) + MM.PREC:
        assert float(enc.global_free.grad[:, glob_names.index(n)].abs().max()) > 0.0, n


def test_training_step_moves_the_likelihood_only_parameters(monkeypatch, tmp_path):
    """One Training.step on PrprContaminated through the general step: eps and kappa are read by log_likelihood only, so their
    gradient reaches the encoder through loglik_vjp's pb and prepare_vjp alone (at the parent, where the method is ignored,
    their columns get the prior's and the entropy's gradient but none from the data: the loss there is the Gaussian's).  The
    loss equals the -ELBO formed in float64 from the step's own samples within 1e-4 relative, which the Gaussian's does not;
    both columns and the prec_* columns (loglik_vjp's prb) move."""
    monkeypatch.chdir(tmp_path)
    cls = LM.PrprContaminated
    fx, settings, model, training, batch = _prpr_training(monkeypatch, cls, hip_graph=False)
    model.train()
    seen = {}
    tail = training._general_tail

    def spy(results, theta, q, p):  # (the step's own samples, before the tail's launches update anything)
        seen["f64"] = _float64_prpr(cls, theta, q, p, batch, fx.solver)
        return tail(results, theta, q, p)

    monkeypatch.setattr(training, "_general_tail", spy)
    enc = model.encoder
    glob_names = [d.name for d in enc.glob]
    before = enc.global_free.detach().clone()
    np.random.seed(21)
    torch.manual_seed(21)
    loss = float(training.step(batch))
    torch.cuda.synchronize()
    assert training._gtail_ok is True, "the general step did not take the model"
    logp, gauss, log_w, log_w_gauss = seen["f64"]
    assert bool(torch.isfinite(logp).all())
    ref = -float((torch.logsumexp(log_w, dim=1) - np.log(fx.S)).mean())
    other = -float((torch.logsumexp(log_w_gauss, dim=1) - np.log(fx.S)).mean())
    print("loss %.6f, float64 %.6f (Gaussian on the same samples: %.6f)" % (loss, ref, other))
    assert abs(other - ref) > 100 * TOL * abs(ref)
    assert abs(loss - ref) <= TOL * abs(ref)
    after = enc.global_free.detach()
    for n in LM.CONTAMINATION + MM.PREC:
        k = glob_names.index(n)
        assert not torch.equal(before[:, k], after[:, k]), n
