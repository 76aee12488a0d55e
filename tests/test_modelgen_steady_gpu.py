"""GPU tests of pre-equilibration in generated models (`steady_species`, `steady_rate`: M::steady between start and the lead-in
ahead of the time loop of ode_fwd_kernel; the recomputation of init, start and steady, and M::steady_vjp between the lead-in's
adjoint and start_vjp behind the time loop of ode_bwd_kernel, csrc/vihds_ode_kernels.hpp and csrc/vihds_steady.hpp): every model
of tests/modelgen_steady_models.py with the solvers it is tested with against the float64 definition
(modelgen_steady_models.definition, whose x0 includes the solve), through the C ABI; the solved twin and its closed-form twin on
the same inputs; the exactly zero gradient of a slot that only feeds a guess; the forcings of two rows swapped; what the C API
declines; one eager and one captured-and-replayed training step.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: two blocks and a tail); T=9 on the project's
grid, and one ragged grid (RAGGED of tests/test_modelgen_implicit_gpu.py).  Bounds, those of `_compare` there: trajectory and
x_predict 1e-5 per species / signal, log-likelihood 1e-4, the loss within max(1e-6, 8 x the float32 torch run's error), every
theta row within max(1e-4, 8 x the float32 torch run of the same definition).  Preconditions, on the float64 run alone:
everything finite; the last increment of the solve at most 1e-9 of |y_E| in every row; for beuler the last Newton increment of
the steps at most 1e-9 of the state; the gradient of the parameter only steady_rate reads not zero."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_leadin_models as LM
import modelgen_steady_models as SS
from test_modelgen_implicit_gpu import RAGGED, _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
CASES = [(cls, solver) for cls in SS.MODELS for solver in SS.solvers_of(cls)]
_KEYS, _REFS = {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert hip.GENERATED_STEADY.get(cls.model_key, 0) == len(cls.steady_species or ())
    return _KEYS[cls]


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        define = LM.definition if cls is LM.PrprSteady else SS.definition
        _REFS[k] = (define(cls, pb, solver, torch.float64), define(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, cond=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == SS.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"] if cond is None else cond
    cond = cond if cond.shape[1] else torch.zeros(pb["B"], 1, dtype=torch.float64)
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
    inc, res, _ = SS.converged(cls, pb)
    print("%s: last increment of the float64 solve %.2e of |y_E|, |steady_rate| %.2e" % (label, inc, res))
    assert inc <= 1e-9, "badly posed inputs: the solve has not converged in the reference"
    if solver == "beuler":
        print("%s: last Newton increment of the float64 run %.2e" % (label, r64["last_increment"]))
        assert r64["last_increment"] <= 1e-9, "badly posed inputs: Newton has not converged in the reference"
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    assert all(bool(torch.isfinite(g).all()) for g in r64["g_theta"].values())
    if cls in SS.STEADY_ONLY:
        g = r64["g_theta"][SS.STEADY_ONLY[cls]]
        print("%s: the float64 gradient of '%s', read by steady_rate alone, is up to %.2e" % (label, SS.STEADY_ONLY[cls], float(g.abs().max())))
        assert float(g.abs().max()) > 0.0
    for n in SS.GUESS_ONLY.get(cls, ()):
        assert float(r64["g_theta"][n].abs().max()) == 0.0, n  # (_compare then asks the kernel for an exact 0 too)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, after the
    preconditions on the float64 reference: a tree that ignores steady_species fails the case."""
    B, S = shape
    pb = SS.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(cls, pb, solver, r64, label)
    _compare(_kernel(cls, pb, solver), r64, r32, label)


@pytest.mark.parametrize("cls,solver", [(SS.ToggleSteady, "rk4"), (SS.CascadeCombined, "midpoint"), (SS.BindingSteadyStiff, "beuler")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_ragged_grid(cls, solver):
    """Steps of 0.1 .. 1.0: nothing of the solve depends on the grid, what follows it does."""
    pb = SS.problem(cls, 3, 5, times=RAGGED)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s 3x5 ragged" % (cls.__name__, solver)
    _precondition(cls, pb, solver, r64, label)
    _compare(_kernel(cls, pb, solver), r64, r32, label)


@pytest.mark.parametrize("solver", SS.solvers_of(SS.PrprSteadySolved))
def test_the_solved_twin_and_the_closed_form_twin(solver):
    """PrprSteadySolved (the solve, the mu adjoint) and PrprSteady (the closed form in start, plain reverse mode) on the same
    inputs, 3 x 100: both are held to the float64 definition of PrprSteady, which has no solve in it; their direct difference
    is printed."""
    pb = SS.problem(SS.PrprSteadySolved, *SHAPES[1])
    inc, res, _ = SS.converged(SS.PrprSteadySolved, pb)
    print("PrprSteadySolved 3x100: last increment of the float64 solve %.2e of |y_E|, |steady_rate| %.2e" % (inc, res))
    assert inc <= 1e-9, "badly posed inputs: the solve has not converged in the reference"
    r64, r32 = _reference(LM.PrprSteady, pb, solver)
    solved, closed = _kernel(SS.PrprSteadySolved, pb, solver), _kernel(LM.PrprSteady, pb, solver)
    for k in ("traj", "xpred", "logp"):
        print("%s %s: solved against closed form, directly %.2e" % (solver, k, rel_err(solved[k], closed[k], dim=2)))
    for n in closed["g_theta"]:
        print("%s g_theta[%s]: solved against closed form, directly %.2e" % (solver, n, rel_err(solved["g_theta"][n], closed["g_theta"][n])))
    _compare(closed, r64, r32, "PrprSteady %s 3x100" % solver)
    _compare(solved, r64, r32, "PrprSteadySolved %s 3x100 (against PrprSteady's definition)" % solver)


def test_a_slot_that_only_feeds_a_guess_has_an_exactly_zero_gradient():
    """init_u and init_v of ToggleSteady, init_s of ChainEight: the gradient rows are exactly 0.0 -- nothing is differentiated
    through the iteration --, while the slots beside them have gradients."""
    for cls in (SS.ToggleSteady, SS.ChainEight):
        got = _kernel(cls, SS.problem(cls, *SHAPES[1]), "rk4")
        for n in SS.GUESS_ONLY[cls]:
            assert float(got["g_theta"][n].abs().max()) == 0.0, (cls.__name__, n)
        assert float(got["g_theta"]["init_x"].abs().min()) > 0.0 and float(got["g_theta"]["r"].abs().min()) > 0.0


def test_swapping_two_rows_forcings_swaps_their_results():
    """CascadeCombined, three data rows with the same theta, treatment and observations and different forcings (the light the
    solve reads at u_0, the dilution schedule): with the forcings of rows 0 and 2 exchanged, every result of row 0 is bit for
    bit what row 2 gave, and the other way round; row 1 keeps its bits.  S = 100 puts two data rows into one block."""
    cls, (B, S) = SS.CascadeCombined, SHAPES[1]
    base = SS.problem(cls, B, S)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    pb = dict(base, th={n: same(v) for n, v in base["th"].items()}, obs=same(base["obs"]), G={"logp": same(base["G"]["logp"])})
    perm = [2, 1, 0]
    a = _kernel(cls, pb, "rk4", cond=FM.wide_cond(same(base["treatments"]), base["series"]))
    b = _kernel(cls, pb, "rk4", cond=FM.wide_cond(same(base["treatments"]), base["series"][perm]))
    assert not torch.equal(a["traj"][0], a["traj"][2]) and not torch.equal(a["traj"][0, :, :, 0], a["traj"][2, :, :, 0])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n


def test_what_the_c_api_declines():
    """vihds_ode_fwd and vihds_ode_bwd with dopri5 on a model with steady species: VIHDS_E_UNSUPPORTED with a message that
    names the feature, nothing launched; the one-pass summaries are not available to it; a valid launch that follows is fine."""
    B, S, T = 3, 5, 9
    L = hip.lib()
    times = torch.tensor(SS.TIMES, device=DEV)
    for cls in (SS.ToggleSteady, SS.ChainEight):
        key = _key(cls)
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        C = max(int(cls.n_conditions), 1)
        th = torch.full((len(slots), B, S), 0.5, device=DEV)
        N = L.vihds_model_n_states(hip.MODELS[key])
        prob = ops.OdeProblemSpec(key, "rk4", row_of, len(slots), C=C).bind(B, S, T)
        assert L.vihds_ode_fwd_summaries_supported(ctypes.byref(prob)) == 0
        cond, obs = torch.ones((B, C), device=DEV), torch.zeros((B, 4, T), device=DEV)
        traj, xpred = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV)
        logp, g = torch.zeros((4, B, S), device=DEV), torch.zeros_like(th)

        def fwd():
            return L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                                   hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())

        prob.solver = hip.SOLVERS["dopri5"]
        rc = fwd()
        assert rc == hip.E_UNSUPPORTED and "steady species" in L.vihds_last_error().decode(), key
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "steady species" in L.vihds_last_error().decode(), key
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
        with pytest.raises(NotImplementedError, match="steady species"):
            ops.OdeProblemSpec(key, "dopri5", row_of, len(slots), C=C)
        prob.solver = hip.SOLVERS["rk4"]
        assert fwd() == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(traj).all()) and float(traj.abs().max()) > 0.0


# ---- training: ToggleSteady through the plugin surface with `solver: rk4` ------------------------------------------------------
N_PLATE = 20


def _toggle_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names ToggleSteady and the solver rk4; the
    priors are the draws of the numeric tests."""
    import models
    from vihds import synthetic

    cls = SS.ToggleSteady
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        draws = {n: v for n, v in SS.DRAWS[cls].items() if not n.startswith("prec_")}
        spec["params"]["constant"] = {n: v for n, v in spec["params"]["constant"].items() if n not in draws}
        spec["params"]["local"] = {n: v for n, v in spec["params"]["local"].items() if n not in draws}
        spec["params"]["global"].update({n: synthetic._ln(float(np.log(m)), sd) for n, (m, sd) in draws.items()})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "toggle_steady", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("toggle_steady",))
    out = synthetic.build("toggle_steady", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.n_steady_species == 2 and out[1].params.solver == "rk4"
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step on ToggleSteady eagerly -- the loss and every updated parameter finite, and `leak`, the rate constant
    only steady_rate reads, moves -- and the same step from its hipGraph replay: loss and every updated parameter equal bit
    for bit."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _toggle_training(monkeypatch, 3, 5, hip_graph=graph)
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
        kb = [d.name for d in model.encoder.glob].index("leak")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
