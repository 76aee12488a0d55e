"""GPU tests of the delayed reads of generated models (n_delays<>, the lookups of csrc/vihds_delay.hpp in the time loops of
ode_fwd_kernel and ode_bwd_kernel, the history adjoint in the adjoint's aux buffer): DelayedRepressor, TwoDelays and DelayedStart
against the float64 definition of tests/modelgen_delay_models.py with every fixed-grid solver; a delay above the whole span
against the frozen twin's kernels; rows swapped bit for bit and the adjoint run twice; the C API's answers; one training step
eagerly and from its hipGraph replay.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (two blocks and a tail, the blocks spanning data rows); T=9 on the
ragged grid of tests/test_modelgen_forcing_gpu.py (steps 0.1 .. 1.0) and one case with T=2.  Every comparison first asserts its
preconditions on the float64 inputs alone: (a) delays below the smallest step, between the smallest and the largest, above the
largest and above the whole span are all among the trajectories; (b) every s_lo, every unclamped s_hi and taue against each
step length are at least 1e-3 of the local step away from a kink of the tau gradient.  Bounds: those of
tests/test_modelgen_forcing_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_delay_models as DM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4  # trajectory and x_predict per species / signal; log-likelihood per signal
KINK = 1e-3
_KEYS, _REFS, _WORST = {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _definition(cls, pb, solver, dtype):
    """The definition with torch ops in `dtype`, autograd for the gradient of sum(logp * G) with respect to theta."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    xs, xp, logp = DM.forward(cls, th, pb["cond"].to(dtype), pb["times"].to(dtype), solver, pb["obs"].to(dtype))
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": xs.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: v.grad for n, v in th.items()}}


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        _REFS[k] = (_definition(cls, pb, solver, torch.float64), _definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, th=None, obs=None, G=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == DM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([(th or pb["th"])[n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"]
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"]), f32(pb["obs"] if obs is None else obs),
                                                  None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"] if G is None else G)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _precondition(cls, pb, r64, label):
    margin, classes = DM.kink_margins(cls, pb)
    print("%s: smallest kink margin %.2e of the local step, delay classes %s" % (label, margin, sorted(classes)))
    assert margin >= KINK, "badly posed inputs: %s has a kink margin of %.2e" % (label, margin)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    # the loss is bounded relative to its own size, with a floor of 1e-6 = 16 float32 roundings: a sum whose terms cancel loses
    # its condition number, so with terms good to about 4 roundings the inputs must keep that number below 4
    terms = r64["logp"] * pb["G"]["logp"]
    condition = float(terms.abs().sum() / terms.sum().abs())
    print("%s: condition number of the loss sum %.2f" % (label, condition))
    assert condition <= 4.0, "badly posed inputs: the loss of %s is a cancelling sum (%.1f)" % (label, condition)
    return classes


def _compare(got, r64, r32, label):
    """Prints every figure, then asserts: forward 1e-5 (log-likelihood 1e-4), the loss within max(1e-6, 8 x the float32 torch
    run's error), every theta row within max(1e-4, 8 x the float32 torch run's error)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        _WORST[name.split("[")[0]] = max(_WORST.get(name.split("[")[0], 0.0), e)
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
            assert float(got["g_theta"][n].abs().max()) == 0.0, n
            continue
        check("g_theta[%s]" % n, rel_err(got["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g)))
    print("\n".join(lines))
    print("largest so far: %s" % ", ".join("%s %.2e" % kv for kv in sorted(_WORST.items())))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", DM.FIXED)
@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, against the float64
    definition; the tau row is part of the comparison and is not zero in the reference."""
    B, S = shape
    pb = DM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    assert _precondition(cls, pb, r64, label) == {0, 1, 2, 3}
    assert float(r64["g_theta"]["tau"].abs().max()) > 0.0
    _compare(_kernel(cls, pb, solver), r64, r32, label)


@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
def test_two_time_points(solver):
    """T = 2: one interval, whose lookups are the constant history whatever the delay -- the tau row is exactly 0."""
    cls, (B, S) = DM.DelayedRepressor, SHAPES[1]
    pb = DM.problem(cls, B, S, times=[0.25, 0.75])
    r64, r32 = _reference(cls, pb, solver)
    _precondition(cls, pb, r64, "T=2 %s" % solver)
    got = _kernel(cls, pb, solver)
    g = r64["g_theta"]["tau"]
    assert (g is None or float(g.abs().max()) == 0.0) and float(got["g_theta"]["tau"].abs().max()) == 0.0
    _compare(got, r64, r32, "DelayedRepressor %s T=2" % solver)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", ["modeuler", "midpoint", "rk4"])
def test_a_delay_above_the_span_is_the_frozen_twin(solver, shape):
    """Every tau above t_end - t_0: the delay kernels agree with the kernels of the twin that reads the initial-state parameter,
    within the bounds of the float64 comparison, and the tau row is exactly 0."""
    B, S = shape
    span = DM.RAGGED[-1] - DM.RAGGED[0]
    pb = DM.problem(DM.DelayedRepressor, B, S, tau=1.25 * span)
    assert bool((pb["th"]["tau"] > span).all())
    r64, r32 = _reference(DM.DelayedRepressorFrozen, pb, solver)
    delayed, frozen = _kernel(DM.DelayedRepressor, pb, solver), _kernel(DM.DelayedRepressorFrozen, pb, solver)
    assert float(delayed["g_theta"]["tau"].abs().max()) == 0.0
    _compare(delayed, r64, r32, "tau above the span against the frozen twin's float64 definition, %s %dx%d" % (solver, B, S))
    assert rel_err(delayed["traj"], frozen["traj"], dim=2) <= TOL and rel_err(delayed["logp"], frozen["logp"], dim=2) <= TOL_LOGP
    for n, g in frozen["g_theta"].items():
        if n == "tau":
            continue
        e = rel_err(delayed["g_theta"][n], g)
        print("g_theta[%s]: delayed against frozen kernels %.2e" % (n, e))
        assert e <= max(1e-4, 8 * rel_err(r32["g_theta"][n], r64["g_theta"][n])), n


@pytest.mark.parametrize("cls", [DM.DelayedRepressor, DM.TwoDelays], ids=lambda c: c.__name__)
def test_swapping_two_rows_swaps_their_results_and_the_adjoint_repeats_its_bits(cls):
    """Data rows 0 and 2 exchanged (theta, treatments and forcings, observations, upstream gradient): every result of row 0 is
    bit for bit what row 2 gave and the other way round, row 1 keeps its bits; and the same launch twice gives the same g_theta
    bit for bit (every thread owns its column of the history adjoint: no atomics)."""
    B, S = SHAPES[1]
    pb = DM.problem(cls, B, S)
    perm = [2, 1, 0]
    swapped = dict(pb, th={n: v[perm] for n, v in pb["th"].items()}, cond=pb["cond"][perm], obs=pb["obs"][perm],
                   G={"logp": pb["G"]["logp"][perm]})
    a, again, b = _kernel(cls, pb, "rk4"), _kernel(cls, pb, "rk4"), _kernel(cls, swapped, "rk4")
    assert not torch.equal(a["traj"][0], a["traj"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n
        assert torch.equal(again["g_theta"][n], a["g_theta"][n]), n
    assert float(a["g_theta"]["tau"].abs().max()) > 0.0


def test_the_c_api_answers():
    """vihds_ode_bwd_aux_floats; VIHDS_E_BADARG without aux and without a trajectory buffer; VIHDS_E_UNSUPPORTED for the adaptive
    ids, the one-pass summaries and the device-resident solver; hip.GENERATED_DELAYS."""
    cls, (B, S) = DM.TwoDelays, SHAPES[0]
    pb = DM.problem(cls, B, S)
    key = _key(cls)
    assert hip.GENERATED_DELAYS[key] == 2 and hip.GENERATED_DELAYS[_key(DM.DelayedRepressor)] == 1
    assert _key(DM.DelayedRepressorFrozen) not in hip.GENERATED_DELAYS
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    T, C, N = pb["T"], pb["cond"].shape[1], len(cls.species)
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV)
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    cond, times, obs = f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"])
    traj, xpred, logp = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV), torch.zeros((4, B, S), device=DEV)
    L = hip.lib()
    spec = ops.OdeProblemSpec(key, "rk4", row_of, th.shape[0], C=C)
    prob = spec.bind(B, S, T)
    assert spec.n_delays == 2 and L.vihds_ode_bwd_aux_floats(ctypes.byref(prob)) == 2 * T * B * S
    frozen = ops.OdeProblemSpec(_key(DM.DelayedRepressorFrozen), "rk4", {n: i for i, n in enumerate(DM.slot_names(DM.DelayedRepressorFrozen))},
                                len(DM.slot_names(DM.DelayedRepressorFrozen)), C=0)
    assert frozen.n_delays == 0 and L.vihds_ode_bwd_aux_floats(ctypes.byref(frozen.bind(B, S, T))) == 0

    def fwd(p, traj_buf):
        rc = L.vihds_ode_fwd(ctypes.byref(p), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj_buf), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    assert fwd(prob, None) == -1 and "trajectory buffer" in L.vihds_last_error().decode()
    assert float(logp.abs().max()) == 0.0  # (nothing was launched)
    assert fwd(prob, traj) == 0
    g_theta, g_logp = torch.zeros_like(th), torch.ones((4, B, S), device=DEV)
    aux = torch.empty(2 * T * B * S, device=DEV)

    def bwd(aux_buf):
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None, hip.ptr(traj),
                             None, None, hip.ptr(g_logp), hip.ptr(g_theta), None, hip.ptr(aux_buf), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    assert bwd(None) == -1 and "history adjoint in aux" in L.vihds_last_error().decode()
    assert float(g_theta.abs().max()) == 0.0
    assert bwd(aux) == 0 and float(g_theta[row_of["tau"]].abs().max()) > 0.0
    # the adaptive ids: refused on the host before the library is asked ...
    for solver in hip.ADAPTIVE_SOLVERS:
        with pytest.raises(NotImplementedError, match="delayed reads"):
            ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=C)
    # ... and by the library: the launcher answers VIHDS_E_UNSUPPORTED for the ids themselves
    for solver in hip.ADAPTIVE_SOLVERS:
        p = spec.bind(B, S, T)
        p.solver = hip.SOLVERS[solver]
        assert fwd(p, traj) == hip.E_UNSUPPORTED, solver
    assert L.vihds_ode_fwd_summaries_supported(ctypes.byref(prob)) == 0
    p5 = spec.bind(B, S, T)
    p5.solver = hip.SOLVERS["dopri5"]
    assert L.vihds_ode_adaptive_tape_floats(ctypes.byref(p5), 256) <= 0  # (the device-resident solver: no registered model)
    p9 = spec.bind(B, S, T)
    p9.solver = hip.SOLVERS["beuler"]
    assert fwd(p9, traj) == hip.E_UNSUPPORTED


# ---- training: DelayedRepressor through the plugin surface ---------------------------------------------------------------------
N_PLATE = 20


def _delayed_training(monkeypatch, B, S, **over):
    import models
    from vihds import synthetic

    cls = DM.DelayedRepressor
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        spec["params"]["constant"]["init_x"] = 0.05
        spec["params"]["constant"]["init_r"] = 0.3
        spec["params"]["global"].update({n: synthetic._ln(float(np.log(DM.REPRESSOR_BASE[n])), 0.2)
                                         for n in ("cap", "beta", "gamma", "gain")})
        spec["params"]["global"]["tau"] = synthetic._ln(float(np.log(1.7)), 0.3)
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "delayed_repressor", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("delayed_repressor",))
    out = synthetic.build("delayed_repressor", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and out[1].params.solver == "rk4"
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step eagerly -- the loss and every updated parameter finite, the prior row behind tau moved -- and the same
    step captured and replayed: loss and every updated parameter equal bit for bit."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _delayed_training(monkeypatch, 3, 5, hip_graph=graph)
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
        assert training._gtail_ok is True, "the general step did not take the model"
        after = {k: v.detach().clone() for k, v in model.named_parameters()}
        runs[graph] = (loss, after)
        print("hip_graph=%s: loss %.6f" % (graph, loss))
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
        kb = [d.name for d in model.encoder.glob].index("tau")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
