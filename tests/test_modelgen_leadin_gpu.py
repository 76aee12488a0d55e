"""GPU tests of the start map and the lead-in phase of generated models (`start(self, y, p, c)`, `lead_in`, `lead_in_steps`:
M::start and ode_lead_in ahead of the time loop of ode_fwd_kernel; the recomputation of init, start and the lead-in's states,
ode_lead_in_vjp and M::start_vjp behind the time loop of ode_bwd_kernel, csrc/vihds_ode_kernels.hpp): every model of
tests/modelgen_leadin_models.py with the solvers it is tested with against the float64 definition
(modelgen_leadin_models.definition), through the C ABI; the definition with the hook or the phase removed far away; the rows of
a batch swapped; the C API's answer to an adaptive solver; one eager and one captured-and-replayed training step.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: blocks that span data rows, tail lanes that
write LDS columns of their own); T=9 on the projects' grids, and one case at T=2, the shortest grid, where the lead-in is most
of the work.  Bounds, those of `_compare` in tests/test_modelgen_substeps_gpu.py: trajectory and x_predict 1e-5 per species /
signal, log-likelihood 1e-4, the loss within max(1e-6, 8 x the float32 torch run's error), every theta row -- the parameter only
start reads included -- within max(1e-4, 8 x the float32 torch run of the same definition); for the stiff model the forward
bounds are max(., 8 x float32 run) too.  Preconditions, on the float64 run alone: everything finite; for beuler the last Newton
increment, lead-in steps included, at most 1e-9 of the state; the definition without the hook / without the phase more than
100 x 1e-5 away in the trajectory; the gradient of the start-only parameter not zero."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_jump_models as JM
import modelgen_leadin_models as LM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4
CASES = [(cls, solver) for cls in LM.MODELS for solver in LM.solvers_of(cls)]
SHORT = [0.0, 0.3]  # T = 2
_KEYS, _REFS = {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert (cls.model_key in hip.GENERATED_START) == (cls._start_def is not None)
        assert (cls.model_key in hip.GENERATED_LEAD_IN) == (cls.lead_in > 0)
    return _KEYS[cls]


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        _REFS[k] = (LM.definition(cls, pb, solver, torch.float64), LM.definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == LM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"] if pb["cond"].shape[1] else torch.zeros(pb["B"], 1, dtype=torch.float64)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"]), f32(pb["obs"]), None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _precondition(cls, pb, solver, r64, label):
    """On the float64 run alone (module docstring)."""
    if solver == "beuler":
        print("%s: last Newton increment of the float64 run, lead-in steps included, %.2e" % (label, r64["last_increment"]))
        assert r64["last_increment"] <= 1e-9, "badly posed inputs: Newton has not converged in the reference"
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    assert all(bool(torch.isfinite(g).all()) for g in r64["g_theta"].values())
    for what, has, kw in (("start", cls._start_def is not None, {"start": False}), ("lead_in", cls.lead_in > 0, {"lead": False})):
        if has:
            without = LM.definition(cls, pb, solver, torch.float64, **kw)["traj"]
            gap = rel_err(without, r64["traj"], dim=2) if bool(torch.isfinite(without).all()) else float("inf")
            print("%s: without %s the float64 trajectory differs by %.2e" % (label, what, gap))
            assert gap > 100 * TOL, what
    if cls in LM.START_ONLY:
        g = r64["g_theta"][LM.START_ONLY[cls]]
        print("%s: the float64 gradient of '%s', read by start alone, is up to %.2e" % (label, LM.START_ONLY[cls], float(g.abs().max())))
        assert float(g.abs().max()) > 0.0


def _compare(cls, got, r64, r32, label):
    """Prints every figure, then asserts (module docstring)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        if not e <= bound:
            bad.append(lines[-1])

    for name, tol in (("traj", TOL), ("xpred", TOL), ("logp", TOL_LOGP)):
        e32 = rel_err(r32[name], r64[name], dim=2)
        lines.append("%s %s: float32 torch run %.2e" % (label, name, e32))
        check(name, rel_err(got[name], r64[name], dim=2), max(tol, 8 * e32) if cls in LM.STIFF else tol)
    scale = abs(float(r64["loss"]))
    check("loss", abs(float(got["loss"]) - float(r64["loss"])) / scale,
          max(1e-6, 8 * abs(float(r32["loss"]) - float(r64["loss"])) / scale))
    for n, g in r64["g_theta"].items():
        if float(g.abs().max()) == 0.0:
            assert float(got["g_theta"][n].abs().max()) == 0.0, n
            continue
        check("g_theta[%s]" % n, rel_err(got["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g)))
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, after the
    preconditions on the float64 reference: a tree that does not trace start, or ignores lead_in, fails the case."""
    B, S = shape
    pb = LM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(cls, pb, solver, r64, label)
    _compare(cls, _kernel(cls, pb, solver), r64, r32, label)


@pytest.mark.parametrize("cls,solver", [(LM.PrprSteadyLead, "rk4"), (LM.PrprEverything, "modeuler"), (LM.FastBindingLead, "beuler")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_the_shortest_grid(cls, solver):
    """T = 2: the lead-in is most of the work, and the first and the last iteration of the time loops are adjacent."""
    pb = LM.problem(cls, 3, 5, times=SHORT)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s 3x5 T=2" % (cls.__name__, solver)
    _precondition(cls, pb, solver, r64, label)
    _compare(cls, _kernel(cls, pb, solver), r64, r32, label)


def test_swapping_the_rows_of_a_batch_swaps_their_results():
    """Three data rows with different treatments (one below, two above the induction threshold of start), forcings, theta and
    observations: with rows 0 and 2 of every input exchanged, every result of row 0 is bit for bit what row 2 gave, and the other
    way round; row 1 keeps its bits.  S = 100 puts two data rows into one block."""
    perm = [2, 1, 0]
    for cls in (LM.PrprSteadyLead, LM.PrprEverything):
        base = LM.problem(cls, *SHAPES[1])
        pb = dict(base, th={n: v[perm] for n, v in base["th"].items()}, cond=base["cond"][perm], obs=base["obs"][perm],
                  G={"logp": base["G"]["logp"][perm]})
        a, b = _kernel(cls, base, "rk4"), _kernel(cls, pb, "rk4")
        assert not torch.equal(a["traj"][0], a["traj"][2])
        for k in ("traj", "xpred", "logp"):
            assert torch.equal(b[k], a[k][perm]), (cls.__name__, k)
        for n in a["g_theta"]:
            assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), (cls.__name__, n)


def test_the_c_api_declines_an_adaptive_solver():
    """vihds_ode_fwd and vihds_ode_bwd with dopri5 on a model with a start map / a lead-in phase: VIHDS_E_UNSUPPORTED with a
    message, nothing queued; a valid launch that follows is fine."""
    B, S, T = 3, 5, 9
    L = hip.lib()
    times = torch.tensor(LM.TIMES, device=DEV)
    for cls, word in ((LM.PrprSteady, "start map"), (LM.PrprLeadOne, "lead-in phase"), (LM.PrprForcedLead, "lead-in phase")):
        key = _key(cls)
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        C = max(int(cls.n_conditions) + len(cls.forcings or ()) * T, 1)
        th = torch.full((len(slots), B, S), 0.5, device=DEV)
        N = L.vihds_model_n_states(hip.MODELS[key])
        prob = ops.OdeProblemSpec(key, "rk4", row_of, len(slots), C=C).bind(B, S, T)
        cond, obs = torch.ones((B, C), device=DEV), torch.zeros((B, 4, T), device=DEV)
        traj, xpred = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV)
        logp, g = torch.zeros((4, B, S), device=DEV), torch.zeros_like(th)

        def fwd():
            return L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                                   hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())

        prob.solver = hip.SOLVERS["dopri5"]
        rc = fwd()
        assert rc == hip.E_UNSUPPORTED and word in L.vihds_last_error().decode(), key
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and word in L.vihds_last_error().decode(), key
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
        with pytest.raises(NotImplementedError, match=word):
            ops.OdeProblemSpec(key, "dopri5", row_of, len(slots), C=C)
        prob.solver = hip.SOLVERS["rk4"]
        assert fwd() == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(traj).all()) and float(traj.abs().max()) > 0.0


# ---- training: PrprForcedLead through the plugin surface, on a plate whose items carry "forcings" ------------------------------
N_PLATE = 20


def _lead_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a small synthetic plate whose spec names PrprForcedLead and whose dataset
    hands out a "forcings" [1][T] entry per row (tests/test_modelgen_jump_gpu.py builds PrprDiluted's the same way)."""
    import models
    from vihds import synthetic

    cls = LM.PrprForcedLead
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    class LitPlate(synthetic.SyntheticPlateDataset):
        def __init__(self, *a, **k):
            super(LitPlate, self).__init__(*a, **k)
            self.forcings = JM.series_of(cls, len(self), self.times.double()).float()

        def __getitem__(self, idx):
            item = super(LitPlate, self).__getitem__(idx)
            item["forcings"] = self.forcings[idx]
            return item

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        spec["params"]["global"].update({"aYFP_PR": ln(0.0, 2.0), "aCFP_PR": ln(0.0, 2.0)})
        return spec

    monkeypatch.setattr(synthetic, "SyntheticPlateDataset", LitPlate)
    monkeypatch.setitem(synthetic.WORKLOADS, "prpr_forced_lead", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("prpr_forced_lead",))
    out = synthetic.build("prpr_forced_lead", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.has_lead_in and not ode.has_start
    assert tuple(out[5].train_data.forcings.shape) == (B, 1, N_PLATE)
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step on PrprForcedLead eagerly -- the loss finite, every parameter finite and the encoder's global
    parameters moved -- and the same step from its hipGraph replay: loss and every updated parameter equal bit for bit."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _lead_training(monkeypatch, 3, 5, hip_graph=graph)
        assert training.use_graph == (graph is None)
        batch = training.train_data
        free_before = model.encoder.global_free.detach().clone()
        log = TrainingLogData()
        np.random.seed(21)
        torch.manual_seed(21)
        orig_step = training.step

        def keeping(b, *a, _t=training, _o=orig_step, **k):
            _t.last_elbo = _o(b, *a, **k)
            return _t.last_elbo

        training.step = keeping
        model.train()
        assert training._run_batch(0.0, batch, log, next_batch=batch)
        loss = float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo)
        torch.cuda.synchronize()
        after = {k: v.detach().clone() for k, v in model.named_parameters()}
        runs[graph] = (loss, after)
        print("hip_graph=%s: loss %.6f" % (graph, loss))
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
        assert not torch.equal(free_before, model.encoder.global_free.detach())
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
