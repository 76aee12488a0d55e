"""GPU tests of the backward-Euler solver "beuler" for generated models with implicit = True (ode_step<M, VIHDS_SOLVER_BEULER>
and the implicit-function adjoint of ode_bwd_kernel, csrc/vihds_implicit.hpp): every model of tests/modelgen_implicit_models.py
against the scheme's definition in float64 (modelgen_implicit_models.definition: NEWTON iterations, autograd Jacobian, pivoted
solve, implicit-function adjoint); the stiff case no explicit scheme integrates; a strongly non-uniform grid and rows swapped
bit for bit for the forced model; the C API's answers; one eager and one captured-and-replayed training step.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: two blocks and a tail, blocks that span data
rows); T=9.  Bounds: trajectory and x_predict 1e-5 per species / signal, log-likelihood 1e-4, the loss and every theta row
max(floor, 8 x the float32 torch run's error) as tests/test_modelgen_forcing_gpu.py holds them; for FastBinding the forward
bounds are max(that, 8 x the float32 torch run's error) too -- the rounding of a linear solve scales with the conditioning of
I - h J, which is 4e2 in the median and 2e4 at worst at its inputs.  Every comparison first asserts, on the float64 run alone,
that the last Newton increment is at most 1e-9 of the state: the kernel differentiates the converged step."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_models as MM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4
RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # (tests/test_modelgen_forcing_gpu.py: steps 0.1 .. 1.0)
RAGGED_R = 0.25  # growth rates of 0.25 exp(0.2 eps): Newton from y_k converges on steps of up to 1.0 (asserted)
_KEYS, _REFS, _FINE = {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _reference(cls, pb):
    k = id(pb)
    if k not in _REFS:
        _REFS[k] = (IM.definition(cls, pb, torch.float64), IM.definition(cls, pb, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver="beuler", cond=None, th=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == IM.slot_names(cls) and key in hip.GENERATED_IMPLICIT
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([(th or pb["th"])[n] for n in slots]).float().to(DEV).requires_grad_(True)
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


def _precondition(r64, label):
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
@pytest.mark.parametrize("cls", IM.MODELS, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood."""
    B, S = shape
    pb = IM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb)
    label = "%s beuler %dx%d" % (cls.__name__, B, S)
    _precondition(r64, label)
    _compare(_kernel(cls, pb), r64, r32, label, forward_by_float32=cls is IM.FastBinding)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_stiff_case_explicit_schemes_cannot_do(shape):
    """FastBinding on TIMES.  Precondition on the float64 oracle: rk4 is non-finite in every row.  The kernel's beuler is finite
    everywhere and agrees, per species, with a float64 solution on a grid 400 times finer within twice the error the float64
    scheme itself has against that solution -- a first-order scheme's error is the reference's to state, not a constant."""
    B, S = shape
    cls = IM.FastBinding
    pb = IM.problem(cls, B, S)
    rhs, x0 = IM.torch_rhs(cls, pb["th"], pb["cond"], pb["times"])
    explicit = IM.rk4_38(rhs, x0, pb["times"])
    assert not bool(torch.isfinite(explicit).all(3).all(2).any()), "rk4 integrates some rows: the inputs are not stiff"
    got = _kernel(cls, pb)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(got[k]).all()), k
    assert all(bool(torch.isfinite(g).all()) for g in got["g_theta"].values())
    if shape not in _FINE:
        _FINE[shape] = IM.fast_refined(pb["th"], pb["times"])
    fine = _FINE[shape]
    ref = _reference(cls, pb)[0]["traj"]
    for j, name in enumerate(cls.species):
        own = float((ref[:, :, j] - fine[:, :, j]).abs().max())
        e = float((got["traj"][:, :, j].double() - fine[:, :, j]).abs().max())
        print("%s: kernel against the refined solution %.3e, the float64 scheme's own error %.3e (largest value %.2f)"
              % (name, e, own, float(fine[:, :, j].abs().max())))
        assert e <= 2.0 * own, name
    # the explicit schemes of the same library do blow up on these inputs
    assert not bool(torch.isfinite(_kernel(cls, pb, "rk4")["traj"]).all(3).all(2).any())


def test_a_non_uniform_grid():
    cls, (B, S) = IM.PrprForcedImplicit, SHAPES[1]
    pb = IM.problem(cls, B, S, times=RAGGED, r_scale=RAGGED_R)
    r64, r32 = _reference(cls, pb)
    _precondition(r64, "ragged")
    _compare(_kernel(cls, pb), r64, r32, "PrprForcedImplicit beuler ragged grid")


def test_swapping_two_rows_forcings_swaps_their_results():
    """Three data rows with the same theta and observations and different forcings: with the forcings of rows 0 and 2
    exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits."""
    cls, (B, S) = IM.PrprForcedImplicit, SHAPES[1]
    base = IM.problem(cls, B, S, times=RAGGED, r_scale=RAGGED_R)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    pb = dict(base, th={n: same(v) for n, v in base["th"].items()}, obs=same(base["obs"]), G={"logp": same(base["G"]["logp"])})
    perm = [2, 1, 0]
    a = _kernel(cls, pb, cond=FM.wide_cond(torch.zeros(B, 0), base["series"]))
    b = _kernel(cls, pb, cond=FM.wide_cond(torch.zeros(B, 0), base["series"][perm]))
    assert not torch.equal(a["traj"][0], a["traj"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n


def test_the_c_api_declines_a_model_without_a_jacobian():
    """Solver 9 on dr_constant and on a registered model without implicit = True: VIHDS_E_UNSUPPORTED with a message, forward
    and adjoint; the adaptive-grid entry point declines the implicit id for the implicit model."""
    B, S, T = 3, 5, 9
    L = hip.lib()
    times = torch.tensor(IM.TIMES, device=DEV)
    for key, C in (("dr_constant", 2), (_plain_key(), 0)):
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        th = torch.full((len(slots), B, S), 0.5, device=DEV)
        N = L.vihds_model_n_states(hip.MODELS[key])
        prob = ops.OdeProblemSpec(key, "rk4", row_of, len(slots), C=max(C, 1)).bind(B, S, T)
        prob.solver = hip.SOLVERS["beuler"]
        cond, obs = torch.zeros((B, max(C, 1)), device=DEV), torch.zeros((B, 4, T), device=DEV)
        traj, xpred = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV)
        logp, g = torch.zeros((4, B, S), device=DEV), torch.zeros_like(th)
        rc = L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "implicit = True" in L.vihds_last_error().decode(), key
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "implicit = True" in L.vihds_last_error().decode(), key
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
    cls = IM.FastBinding
    key = _key(cls)
    slots = hip.model_slots(key)
    spec = ops.OdeProblemSpec(key, "beuler", {n: i for i, n in enumerate(slots)}, len(slots), C=1)
    th = torch.full((len(slots), B, S), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match="needs an adaptive solver id"):
        ops.adaptive_grid(spec, th, torch.zeros((B, 1), device=DEV), times, None, None)


def _plain_key():
    modelgen.register_kernel(MM.PrprRestated, False)
    assert MM.PrprRestated.model_key not in hip.GENERATED_IMPLICIT
    return MM.PrprRestated.model_key


# ---- training: FastBinding through the plugin surface with `solver: beuler` ----------------------------------------------------
N_PLATE = 20


def _stiff_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names FastBinding and the solver beuler; the
    priors are the draws of the numeric tests (kon = 400 exp(eps), koff = 50 exp(eps)), so the samples are stiff."""
    import models
    from vihds import synthetic

    cls = IM.FastBinding
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        spec["params"]["global"].update({n: synthetic._ln(float(np.log(m)), sd) for n, (m, sd) in IM.FAST_DRAWS.items()
                                         if not n.startswith("prec_")})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "fast_binding", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("fast_binding",))
    out = synthetic.build("fast_binding", B, S, solver="beuler", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and out[1].params.solver == "beuler"
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step through the general path eagerly -- the loss and every updated parameter finite, kon moves -- and the
    same step from its hipGraph replay (an implicit solver is no adaptive one: the step is captured): loss and every updated
    parameter equal."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _stiff_training(monkeypatch, 3, 5, hip_graph=graph)
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
        kb = [d.name for d in model.encoder.glob].index("kon")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
