"""GPU tests of the two-stage SDIRK that the solver "beuler" runs for a generated model with implicit_order = 2
(ode_step<M, VIHDS_SOLVER_BEULER> -> sdirk2_step and ode_step_vjp_sdirk2, csrc/vihds_implicit.hpp): every class of
tests/modelgen_sdirk_models.py -- the plain twins, a sub-stepped, a jump and a lead-in class -- against the scheme's definition
in float64 (modelgen_sdirk_models.definition: NEWTON iterations per stage, autograd Jacobian, pivoted solves, the written-out
adjoint); that the scheme is not backward Euler; a strongly non-uniform grid and rows swapped bit for bit for the forced class;
one eager and one captured-and-replayed training step of the stiff model.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: two blocks and a tail); T=9.  Bounds: the rule
of tests/test_modelgen_implicit_gpu.py's _compare, unchanged -- trajectory and x_predict 1e-5, log-likelihood 1e-4, the loss
max(1e-6, 8 x the float32 torch run's error), every theta row max(1e-4, 8 x the float32 torch run's); for the classes of the stiff
binding model the forward bounds are max(that, 8 x the float32 torch run's error) too.  Every comparison first asserts, on the
float64 run alone, that the last Newton increment of every stage is at most 1e-9 of the state: the kernel differentiates the
converged step.  Every class meets that on the grid of its order-1 twin (the stage matrix I - gamma h J is further from
singular than backward Euler's I - h J), so each is tested on its twin's grid and inputs."""
import numpy as np
import pytest
import torch

from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_sdirk_models as DM
from test_modelgen_implicit_gpu import N_PLATE, RAGGED, RAGGED_R, SHAPES, _compare, _precondition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_KEYS, _REFS, _FINE = {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _reference(cls, pb):
    k = (cls, id(pb))
    if k not in _REFS:
        _REFS[k] = (DM.definition(cls, pb, torch.float64), DM.definition(cls, pb, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, cond=None, order=2):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == DM.slot_names(cls) and key in hip.GENERATED_IMPLICIT and hip.GENERATED_IMPLICIT_ORDER[key] == order
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"] if cond is None else cond
    spec = ops.OdeProblemSpec(key, "beuler", row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"]), f32(pb["obs"]), None, None)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood."""
    B, S = shape
    pb = DM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb)
    label = "%s sdirk2 %dx%d" % (cls.__name__, B, S)
    _precondition(r64, label)
    _compare(_kernel(cls, pb), r64, r32, label, forward_by_float32=cls in DM.STIFF)


def test_the_scheme_is_not_backward_euler():
    """FastBinding on TIMES, 300 trajectories.  Against a float64 solution by the same scheme on a grid 64 times finer the kernel's
    error is, per species, within twice the error the float64 definition itself has; the kernel of the order-1 twin (backward
    Euler, same inputs, same solver name) is at least twice as far away as the order-2 kernel (the two float64 definitions
    differ 4.5 times)."""
    B, S = SHAPES[1]
    cls = DM.FastBindingSdirk
    pb = DM.problem(cls, B, S)
    got = _kernel(cls, pb)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(got[k]).all()), k
    assert all(bool(torch.isfinite(g).all()) for g in got["g_theta"].values())
    twin = _kernel(IM.FastBinding, pb, order=1)
    if (B, S) not in _FINE:
        _FINE[(B, S)] = DM.fast_sdirk2(pb["th"], pb["times"], refine=64, newton=3)
    fine = _FINE[(B, S)]
    ref = _reference(cls, pb)[0]["traj"]
    for j, name in enumerate(cls.species):
        own = float((ref[:, :, j] - fine[:, :, j]).abs().max())
        e = float((got["traj"][:, :, j].double() - fine[:, :, j]).abs().max())
        print("%s: kernel against the refined solution %.3e, the float64 scheme's own error %.3e (largest value %.2f)"
              % (name, e, own, float(fine[:, :, j].abs().max())))
        assert e <= 2.0 * own, name
    e2 = float((got["traj"].double() - fine).abs().max())
    e1 = float((twin["traj"].double() - fine).abs().max())
    print("largest error against the refined solution: order-2 kernel %.3e, order-1 kernel %.3e (%.1f times)" % (e2, e1, e1 / e2))
    assert e1 >= 2.0 * e2


def test_a_non_uniform_grid():
    cls, (B, S) = DM.PrprForcedSdirk, SHAPES[1]
    pb = DM.problem(cls, B, S, times=RAGGED, r_scale=RAGGED_R)
    r64, r32 = _reference(cls, pb)
    _precondition(r64, "ragged")
    _compare(_kernel(cls, pb), r64, r32, "PrprForcedSdirk sdirk2 ragged grid")


def test_swapping_two_rows_forcings_swaps_their_results():
    """Three data rows with the same theta and observations and different forcings: with the forcings of rows 0 and 2
    exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits."""
    cls, (B, S) = DM.PrprForcedSdirk, SHAPES[1]
    base = DM.problem(cls, B, S, times=RAGGED, r_scale=RAGGED_R)
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


# ---- training: the stiff model at order 2 through the plugin surface with `solver: beuler` -------------------------------------
def _stiff_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names FastBindingSdirk and the solver beuler (the
    pattern of tests/test_modelgen_implicit_gpu.py; the priors are the draws of the numeric tests, so the samples are stiff)."""
    import models
    from vihds import synthetic

    cls = DM.FastBindingSdirk
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        spec["params"]["global"].update({n: synthetic._ln(float(np.log(m)), sd) for n, (m, sd) in IM.FAST_DRAWS.items()
                                         if not n.startswith("prec_")})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "fast_binding_sdirk2", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("fast_binding_sdirk2",))
    out = synthetic.build("fast_binding_sdirk2", B, S, solver="beuler", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and out[1].params.solver == "beuler" and hip.GENERATED_IMPLICIT_ORDER[cls.model_key] == 2
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step through the general path eagerly -- the loss and every updated parameter finite, kon moves -- and the
    same step from its hipGraph replay: loss and every updated parameter equal."""
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
