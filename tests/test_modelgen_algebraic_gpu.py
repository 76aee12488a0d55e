"""GPU tests of algebraic variables in generated models (csrc/vihds_algebraic.hpp; the solve inside the generated rhs / rhs_vjp
and observe / observe_vjp): every class of tests/modelgen_algebraic_models.py through ops.OdeSolveObserve, forward and adjoint,
against the definition in float64 (modelgen_algebraic_models.definition: the explicit scheme on the right-hand side that
solves the constraint by the defined Newton iteration, implicit-function gradient); BindingQss against the float64 definition
of its closed-form twin, which pins the mu adjoint to plain reverse mode; the reduction against the refined solution of the
stiff FastBinding it reduces; rows swapped bit for bit for the class with forcings, sub-steps and a jump; one eager and one
captured-and-replayed training step; what the C API declines.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: two blocks and a tail); T=9.  Bounds: those of
tests/test_modelgen_implicit_gpu.py (_compare, imported: trajectory and x_predict 1e-5 per species / signal, log-likelihood
1e-4, the loss and every theta row max(floor, 8 x the float32 torch run's error)).  Every comparison first asserts, on the
float64 run alone, that the last Newton increment is at most 1e-9 of |z|: the kernel differentiates the converged solution."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_algebraic_models as AM
import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
from test_modelgen_implicit_gpu import RAGGED, TOL, _compare, _precondition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
_KEYS, _REFS, _RUNS = {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        _REFS[k] = (AM.definition(cls, pb, solver, torch.float64), AM.definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, cond=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == AM.slot_names(cls)
    assert hip.GENERATED_ALGEBRAIC.get(key) == (len(cls.algebraic) or None) and key not in hip.GENERATED_IMPLICIT
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


def _run(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _RUNS:
        _RUNS[k] = _kernel(cls, pb, solver)
    return _RUNS[k]


CASES = [(cls, solver) for cls in AM.MODELS for solver in ("midpoint", "rk4")] + [(AM.BindingQss, "modeuler"), (AM.BindingQss, "euler")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood."""
    B, S = shape
    pb = AM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(r64, label)
    _compare(_run(cls, pb, solver), r64, r32, label)


def test_a_non_uniform_grid():
    cls, (B, S) = AM.Competing, SHAPES[1]
    pb = AM.problem(cls, B, S, times=RAGGED)
    r64, r32 = _reference(cls, pb, "rk4")
    _precondition(r64, "ragged")
    _compare(_run(cls, pb, "rk4"), r64, r32, "Competing rk4 ragged grid")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", ["midpoint", "rk4"])
def test_against_the_closed_form(solver, shape):
    """The BindingQss kernels (Newton, mu adjoint) and the BindingClosed kernels (one sqrt, plain reverse mode) on the same
    inputs, each held to the float64 definition of BindingClosed -- which has no algebraic variable in it -- by the rule of
    _compare; the direct difference between the two kernels is printed."""
    B, S = shape
    pb = AM.problem(AM.BindingQss, B, S)
    assert pb is AM.problem(AM.BindingClosed, B, S)
    r64, r32 = _reference(AM.BindingClosed, pb, solver)
    _precondition(_reference(AM.BindingQss, pb, solver)[0], "BindingQss %s %dx%d" % (solver, B, S))
    qss, closed = _run(AM.BindingQss, pb, solver), _run(AM.BindingClosed, pb, solver)
    for k in ("traj", "xpred", "logp"):
        print("%s: BindingQss kernel against BindingClosed kernel %.2e" % (k, rel_err(qss[k], closed[k], dim=2)))
    for n, g in closed["g_theta"].items():
        if float(g.abs().max()) > 0.0:
            print("g_theta[%s]: BindingQss kernel against BindingClosed kernel %.2e" % (n, rel_err(qss["g_theta"][n], g)))
    _compare(closed, r64, r32, "BindingClosed %s %dx%d against its definition" % (solver, B, S))
    _compare(qss, r64, r32, "BindingQss %s %dx%d against the closed form's definition" % (solver, B, S))


def test_the_reduction_does_what_it_is_for():
    """The draws at which the explicit FastBinding blows up (tests/test_modelgen_implicit_gpu.py shows that), 300 trajectories,
    rk4 on TIMES: the BindingQss kernel is finite everywhere, and for At, Bt and R its distance to the refined solution of the
    full stiff model (A + C, B + C, R of modelgen_implicit_models.fast_refined) is at most max(2 x the distance the float64
    definition itself has, the forward bound of _compare).  The size of the quasi-steady-state error is printed, not asserted."""
    cls, (B, S) = AM.BindingQss, SHAPES[1]
    pb = AM.problem(cls, B, S)
    got = _run(cls, pb, "rk4")
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(got[k]).all()), k
    assert all(bool(torch.isfinite(g).all()) for g in got["g_theta"].values())
    fine = IM.fast_refined(pb["th"], pb["times"])
    full = torch.stack([fine[:, :, 0] + fine[:, :, 2], fine[:, :, 1] + fine[:, :, 2], fine[:, :, 3]], dim=2)
    ref = _reference(cls, pb, "rk4")[0]["traj"]
    for j, name in enumerate(cls.species):
        own = float((ref[:, :, j] - full[:, :, j]).abs().max())
        e = float((got["traj"][:, :, j].double() - full[:, :, j]).abs().max())
        size = float(full[:, :, j].abs().max())
        print("%s: kernel against the refined stiff solution %.3e, the float64 definition's own distance %.3e (largest value %.2f)"
              % (name, e, own, size))
        assert e <= max(2.0 * own, TOL * size), name


def test_swapping_two_rows_forcings_swaps_their_results():
    """Three data rows with the same theta and observations and different forcings (the temperature the constraint reads, the
    dilution schedule): with the forcings of rows 0 and 2 exchanged, every result of row 0 is bit for bit what row 2 gave, and
    the other way round; row 1 keeps its bits."""
    cls, (B, S) = AM.BindingCombined, SHAPES[1]
    base = AM.problem(cls, B, S)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    pb = dict(base, th={n: same(v) for n, v in base["th"].items()}, obs=same(base["obs"]), G={"logp": same(base["G"]["logp"])})
    perm = [2, 1, 0]
    a = _kernel(cls, pb, "rk4", cond=FM.wide_cond(torch.zeros(B, 0), base["series"]))
    b = _kernel(cls, pb, "rk4", cond=FM.wide_cond(torch.zeros(B, 0), base["series"][perm]))
    assert not torch.equal(a["traj"][0], a["traj"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n


def test_what_the_c_api_declines():
    """A model with algebraic variables has a map of its own: the states summaries answer VIHDS_E_BADARG for its observe kind,
    the one-pass summaries are not available to it, and the device-resident adaptive solver declines a registered model."""
    cls = AM.BindingQss
    key = _key(cls)
    slots = hip.model_slots(key)
    B, S, T, N = 3, 5, 9, len(cls.species)
    spec = ops.OdeProblemSpec(key, "rk4", {n: i for i, n in enumerate(slots)}, len(slots), C=1)
    L = hip.lib()
    assert L.vihds_model_n_states(hip.MODELS[key]) == N
    assert L.vihds_ode_fwd_summaries_supported(ctypes.byref(spec.bind(B, S, T))) == 0
    kind = ops.OBSERVE_KINDS[cls.observe_kind]
    assert cls.observe_kind == "custom" and kind == 3
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    rows = (ctypes.c_int * 4)(0, 1, 2, 3)
    out = [z(B, 4, T), z(B, 4, T), z(B, N, T), z(B, 4, T)]
    rc = L.vihds_iw_summaries_states(B, S, T, N, N, kind, hip.ptr(z(B, S)), hip.ptr(z(B)), hip.ptr(z(T, N, B, S)),
                                     hip.ptr(z(4, B, S)), rows, hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(out[2]),
                                     hip.ptr(out[3]), hip.current_stream())
    assert rc == -1 and "VIHDS_OBS_CUSTOM" in L.vihds_last_error().decode()  # VIHDS_E_BADARG
    adaptive = ops.OdeProblemSpec(key, "dopri5", {n: i for i, n in enumerate(slots)}, len(slots), C=1)
    assert ops.adaptive_device_supported(adaptive, B, S, T, 256) is None
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in out)  # (nothing was launched)


# ---- training: Competing through the plugin surface with `solver: rk4` ---------------------------------------------------------
N_PLATE = 20


def _qss_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names Competing and the solver rk4; the priors
    are the draws of the numeric tests."""
    import models
    from vihds import synthetic

    cls = AM.Competing
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        spec["params"]["global"].update({n: synthetic._ln(float(np.log(m)), sd) for n, (m, sd) in AM.DRAWS[cls].items()
                                         if not n.startswith("prec_")})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "competing_qss", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("competing_qss",))
    out = synthetic.build("competing_qss", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and out[1].params.solver == "rk4"
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step through the general path eagerly -- the loss and every updated parameter finite, K1 moves -- and the
    same step from its hipGraph replay: loss and every updated parameter equal bit for bit."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _qss_training(monkeypatch, 3, 5, hip_graph=graph)
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
        kb = [d.name for d in model.encoder.glob].index("K1")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
