"""GPU tests of `substeps = m` for generated models (ode_substeps and ode_substeps_vjp in the time loops of ode_fwd_kernel and
ode_bwd_kernel, csrc/vihds_ode_kernels.hpp; the sub-step times of csrc/vihds_substeps.hpp): every model of
tests/modelgen_substep_models.py with every fixed-grid solver it takes against the float64 definition -- the m = 1 scheme on
the refined grid read at every m-th point (modelgen_substep_models.definition); beuler on the piecewise grid the implicit
tests had to leave; the stiff model's accuracy against a 400 times finer solution; a strongly non-uniform grid; rows swapped bit
for bit; the C API's answer to an adaptive solver; one eager and one captured-and-replayed training step.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: blocks that span data rows, and tail lanes in
the last block -- they shadow the last trajectory and write LDS columns of their own); T=9.  Bounds, those of `_compare` in
tests/test_modelgen_implicit_gpu.py: trajectory and x_predict 1e-5 per species / signal, log-likelihood 1e-4, the loss within
max(1e-6, 8 x the float32 torch run's error), every theta row within max(1e-4, 8 x the float32 torch run of the same
definition); for FastBindingSub4 the forward bounds are max(that, 8 x the float32 run's) too.  A beuler comparison first
asserts, on the float64 run alone, that the last Newton increment is at most 1e-9 of the state."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_substep_models as SM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4
RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # (tests/test_modelgen_forcing_gpu.py: steps 0.1 .. 1.0)
RAGGED_R = 0.25  # (tests/test_modelgen_implicit_gpu.py: growth rates of 0.25 exp(0.2 eps))
# test_beuler_on_the_piecewise_grid: the growth rates r = exp(0.2 eps) reach 1.77 among 300 draws and only 1.43 among 15, where
# Newton at m = 1 is merely slow (last increment 3e-4); scaled by 1.5 the small shape's largest rate is 2.15 and m = 1 leaves
# increments of order 1 as at the large shape (float64, CPU: 1.2 / 1.9 at m = 1, 1.5e-12 / 1.9e-12 at m = 4)
PIECEWISE_R = {(3, 5): 1.5, (3, 100): 1.0}
CASES = [(cls, solver) for cls in SM.MODELS for solver in SM.solvers_of(cls)]
_KEYS, _REFS, _FINE = {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert hip.GENERATED_SUBSTEPS[cls.model_key] == cls.substeps
    return _KEYS[cls]


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        _REFS[k] = (SM.definition(cls, pb, solver, torch.float64), SM.definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, cond=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == SM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"] if cond is None else cond
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"]), f32(pb["obs"]), None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _precondition(r64, label, solver):
    if solver == "beuler":
        print("%s: last Newton increment of the float64 run %.2e" % (label, r64["last_increment"]))
        assert r64["last_increment"] <= 1e-9, "badly posed inputs: Newton has not converged in the reference"
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k


def _compare(got, r64, r32, label, forward_by_float32=False):
    """Prints every figure, then asserts (module docstring)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        if not e <= bound:
            bad.append(lines[-1])

    for name, dim, tol in (("traj", 2, TOL), ("xpred", 2, TOL), ("logp", 2, TOL_LOGP)):
        e32 = rel_err(r32[name], r64[name], dim=dim)
        lines.append("%s %s: float32 torch run %.2e" % (label, name, e32))
        check(name, rel_err(got[name], r64[name], dim=dim), max(tol, 8 * e32) if forward_by_float32 else tol)
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
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood.  (The implicit
    models run on the grid of steps 0.1 .. 0.2 their m = 1 parents use, FastBindingSub4 and the others on the piecewise TIMES.)"""
    B, S = shape
    pb = SM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s m=%d %s %dx%d" % (cls.__name__, cls.substeps, solver, B, S)
    _precondition(r64, label, solver)
    if solver in ("euler", "beuler"):
        # a first-order scheme without the sub-steps is far outside the bound: the case fails where `substeps` is ignored
        coarse = SM.definition(cls, pb, solver, torch.float64, m=1)["traj"]
        gap = rel_err(coarse, r64["traj"], dim=2) if bool(torch.isfinite(coarse).all()) else float("inf")
        print("%s: the m = 1 scheme differs from the definition by %.2e" % (label, gap))
        assert gap > 100 * TOL
    _compare(_kernel(cls, pb, solver), r64, r32, label, forward_by_float32=cls is SM.FastBindingSub4)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls", [SM.PrprImplicitSub4, SM.DrImplicitSub4], ids=lambda c: c.__name__)
def test_beuler_on_the_piecewise_grid(cls, shape):
    """The grid the implicit tests had to leave (steps 0.3 .. 0.6, growth rates up to 1.8).  Preconditions on the float64
    reference: the last Newton increment is at most 1e-9 with m = 4, and above 1e-3 with m = 1 -- what the sub-steps buy."""
    B, S = shape
    pb = SM.problem(cls, B, S, times=SM.TIMES, r_scale=PIECEWISE_R[shape])
    r64, r32 = _reference(cls, pb, "beuler")
    label = "%s beuler piecewise grid %dx%d" % (cls.__name__, B, S)
    _precondition(r64, label, "beuler")
    one = SM.beuler_refined(cls, pb["th"], pb["cond"], pb["times"], 1)[2]
    print("%s: last Newton increment at m = 1 %.2e" % (label, one))
    assert one > 1e-3
    _compare(_kernel(cls, pb, "beuler"), r64, r32, label)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_accuracy_of_the_stiff_model(shape):
    """FastBindingSub4 against a float64 solution on a grid 400 times finer: per species the kernel's error is within twice the
    float64 scheme's own error at m = 4, and that error is below half the float64 scheme's at m = 1."""
    B, S = shape
    cls = SM.FastBindingSub4
    pb = SM.problem(cls, B, S)
    got = _kernel(cls, pb, "beuler")
    if shape not in _FINE:
        _FINE[shape] = IM.fast_refined(pb["th"], pb["times"])
    fine = _FINE[shape]
    four = _reference(cls, pb, "beuler")[0]["traj"]
    one = SM.beuler_refined(cls, pb["th"], pb["cond"], pb["times"], 1)[0]
    e1, e4 = float((one - fine).abs().max()), float((four - fine).abs().max())
    print("float64 scheme against the refined solution: %.3e at m = 1, %.3e at m = 4 (largest value %.2f)"
          % (e1, e4, float(fine.abs().max())))
    assert e4 < 0.5 * e1
    for j, name in enumerate(cls.species):
        own = float((four[:, :, j] - fine[:, :, j]).abs().max())
        e = float((got["traj"][:, :, j].double() - fine[:, :, j]).abs().max())
        print("%s: kernel against the refined solution %.3e, the float64 scheme's own error %.3e" % (name, e, own))
        assert e <= 2.0 * own, name


@pytest.mark.parametrize("cls,solver", [(SM.PrprForcedImplicitSub2, "beuler"), (SM.PrprForcedSub4, "rk4")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_non_uniform_grid(cls, solver):
    B, S = SHAPES[1]
    kw = {"r_scale": RAGGED_R} if cls.implicit else {}
    pb = SM.problem(cls, B, S, times=RAGGED, **kw)
    r64, r32 = _reference(cls, pb, solver)
    _precondition(r64, "ragged", solver)
    _compare(_kernel(cls, pb, solver), r64, r32, "%s %s ragged grid" % (cls.__name__, solver))


@pytest.mark.parametrize("cls,solver", [(SM.PrprForcedImplicitSub2, "beuler"), (SM.PrprForcedSub4, "rk4")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_swapping_two_rows_forcings_swaps_their_results(cls, solver):
    """Three data rows with the same theta and observations and different forcings: with the forcings of rows 0 and 2
    exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits.  S = 100
    leaves tail lanes in the last block and puts two data rows into one block: a shared LDS column would show here."""
    B, S = SHAPES[1]
    kw = {"r_scale": RAGGED_R} if cls.implicit else {}
    base = SM.problem(cls, B, S, times=RAGGED, **kw)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    pb = dict(base, th={n: same(v) for n, v in base["th"].items()}, obs=same(base["obs"]), G={"logp": same(base["G"]["logp"])})
    perm = [2, 1, 0]
    a = _kernel(cls, pb, solver, cond=FM.wide_cond(torch.zeros(B, 0), base["series"]))
    b = _kernel(cls, pb, solver, cond=FM.wide_cond(torch.zeros(B, 0), base["series"][perm]))
    assert not torch.equal(a["traj"][0], a["traj"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n


def test_the_c_api_declines_an_adaptive_solver():
    """vihds_ode_fwd and vihds_ode_bwd with dopri5 on a sub-stepped model: VIHDS_E_UNSUPPORTED with a message, nothing queued;
    so does the adaptive-grid entry point."""
    B, S, T = 3, 5, 9
    L = hip.lib()
    times = torch.tensor(SM.TIMES, device=DEV)
    for cls in (SM.PrprImplicitSub4, SM.PrprForcedSub2):
        key = _key(cls)
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        C = len(cls.forcings) * T
        th = torch.full((len(slots), B, S), 0.5, device=DEV)
        N = L.vihds_model_n_states(hip.MODELS[key])
        prob = ops.OdeProblemSpec(key, "rk4", row_of, len(slots), C=max(C, 1)).bind(B, S, T)
        prob.solver = hip.SOLVERS["dopri5"]
        cond, obs = torch.ones((B, max(C, 1)), device=DEV), torch.zeros((B, 4, T), device=DEV)
        traj, xpred = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV)
        logp, g = torch.zeros((4, B, S), device=DEV), torch.zeros_like(th)
        rc = L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "substeps > 1" in L.vihds_last_error().decode(), key
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "substeps > 1" in L.vihds_last_error().decode(), key
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
        with pytest.raises(NotImplementedError, match="substeps = %d" % cls.substeps):
            ops.OdeProblemSpec(key, "dopri5", row_of, len(slots), C=max(C, 1))


# ---- training: the plate reader at m = 3 through the plugin surface ------------------------------------------------------------
N_PLATE = 20


def _reader_training(monkeypatch, cls, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names `cls` (the priors of
    tests/test_modelgen_likelihood_gpu.py's plate)."""
    import models
    from vihds import synthetic
    from test_modelgen_noise_gpu import NOISE_BASE

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

    name = "reader_" + cls.__name__
    monkeypatch.setitem(synthetic.WORKLOADS, name, (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + (name,))
    out = synthetic.build(name, B, S, solver="rk4", device=DEV, seed=3, **over)
    assert isinstance(out[4].decoder.ode_model, cls)
    return out


def _one_step(monkeypatch, cls, graph):
    """One Training step; returns (loss, the parameters after it, the library calls that queued work)."""
    from test_step_routes import _recorded
    from vihds.utils import TrainingLogData

    args, settings, data, parameters, model, training = _reader_training(monkeypatch, cls, 3, 5, hip_graph=graph)
    assert training.use_graph == (graph is None)
    batch = training.train_data
    log = TrainingLogData()
    np.random.seed(21)
    torch.manual_seed(21)
    orig_step = training.step

    def keeping(b, *a, _t=training, _o=orig_step, **k):
        _t.last_elbo = _o(b, *a, **k)
        return _t.last_elbo

    training.step = keeping
    model.train()
    ok, calls = _recorded(lambda: training._run_batch(0.0, batch, log, next_batch=batch))
    assert ok
    loss = float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo)
    torch.cuda.synchronize()
    return loss, {k: v.detach().clone() for k, v in model.named_parameters()}, calls


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step on PlateReaderSub3 eagerly and the same step from its hipGraph replay: the loss finite, loss and
    every updated parameter equal on both routes; and the eager step queues the library calls the step of the m = 1 parent
    queues -- the sub-steps change what a launch computes, not which launches run."""
    monkeypatch.chdir(tmp_path)
    runs = {graph: _one_step(monkeypatch, SM.PlateReaderSub3, graph) for graph in (False, None)}
    for graph, (loss, after, _) in runs.items():
        print("hip_graph=%s: loss %.6f" % (graph, loss))
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
    (la, pa, calls), (lb, pb_, _) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
    parent_loss, _, parent_calls = _one_step(monkeypatch, SM.PARENT[SM.PlateReaderSub3], False)
    print("eager step queues %s" % calls)
    assert calls and calls == parent_calls
    assert parent_loss != la  # (three steps per interval are another scheme)
