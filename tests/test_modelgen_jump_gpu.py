"""GPU tests of the state jump of generated models (`jump(self, y, p, c)`: M::jump at the end of a time point's iteration of
ode_fwd_kernel, its recomputation and M::jump_vjp ahead of the hook adjoints in ode_bwd_kernel and its dump form,
csrc/vihds_ode_kernels.hpp): every model of tests/modelgen_jump_models.py with the solvers it is tested with against the float64
definition (modelgen_jump_models.definition), through the C ABI; the reference with and without the hook far apart; a schedule
belongs to its data row; an event at point 0 and one at the last point; the C API's answer to an adaptive solver; one eager and
one captured-and-replayed training step.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: blocks that span data rows, tail lanes in the
last block); T=9.  Bounds, those of `_compare` in tests/test_modelgen_substeps_gpu.py: trajectory and x_predict 1e-5 per species /
signal, log-likelihood 1e-4, the loss within max(1e-6, 8 x the float32 torch run's error), every theta row -- the parameters only
the jump reads included -- and every weight tensor within max(1e-4, 8 x the float32 torch run of the same definition).  A beuler
comparison first asserts, on the float64 run alone, that the last Newton increment is at most 1e-9 of the state; the
turbidostat's that every comparison of the float64 run is at least MARGIN = 1e-3 wide."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_jump_models as JM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4
CASES = [(cls, solver) for cls in JM.MODELS for solver in JM.solvers_of(cls)]
_KEYS, _REFS = {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert cls.model_key in hip.GENERATED_JUMP
    return _KEYS[cls]


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        _REFS[k] = (JM.definition(cls, pb, solver, torch.float64), JM.definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, cond=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == JM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    cond = pb["cond"] if cond is None else cond
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    w = None
    if pb["W"]:
        w = torch.cat([t.reshape(-1) for ws in pb["W"].values() for t in ws]).float().to(DEV).requires_grad_(True)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"]), f32(pb["obs"]), None, w)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}, "g_w": None if w is None else w.grad.cpu()}


def _precondition(r64, label, solver):
    if solver == "beuler":
        print("%s: last Newton increment of the float64 run %.2e" % (label, r64["last_increment"]))
        assert r64["last_increment"] <= 1e-9, "badly posed inputs: Newton has not converged in the reference"
    m = r64["margins"]
    if m.by_label:
        worst = min(m.by_label, key=m.by_label.get)
        print("%s: smallest switch margin %.2e (%s)" % (label, m.smallest, worst))
        assert m.smallest >= JM.MARGIN, "badly posed inputs: %s has margin %.2e" % (worst, m.smallest)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k


def _compare(got, r64, r32, label):
    """Prints every figure, then asserts (module docstring)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        if not e <= bound:
            bad.append(lines[-1])

    for name, tol in (("traj", TOL), ("xpred", TOL), ("logp", TOL_LOGP)):
        lines.append("%s %s: float32 torch run %.2e" % (label, name, rel_err(r32[name], r64[name], dim=2)))
        check(name, rel_err(got[name], r64[name], dim=2), tol)
    scale = abs(float(r64["loss"]))
    check("loss", abs(float(got["loss"]) - float(r64["loss"])) / scale,
          max(1e-6, 8 * abs(float(r32["loss"]) - float(r64["loss"])) / scale))
    for n, g in r64["g_theta"].items():
        if float(g.abs().max()) == 0.0:
            assert float(got["g_theta"][n].abs().max()) == 0.0, n
            continue
        check("g_theta[%s]" % n, rel_err(got["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g)))
    o = 0
    for k, ref in enumerate(r64["g_w"]):  # (the network's weight gradients, through the adjoint's dump)
        g = got["g_w"][o:o + ref.numel()].view(ref.shape)
        o += ref.numel()
        assert float(ref.abs().max()) > 0.0
        check("weight tensor %d %s" % (k, tuple(ref.shape)), rel_err(g, ref), max(1e-4, 8 * rel_err(r32["g_w"][k], ref)))
    assert o == (0 if got["g_w"] is None else got["g_w"].numel())
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood.  First, on the
    float64 reference alone: the jump matters -- with and without the hook the trajectories and the gradient of the parameter
    that only the jump reads differ by more than 100 x their tolerances, so a kernel that ignores the hook fails the case."""
    B, S = shape
    pb = JM.problem(cls, B, S)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(r64, label, solver)
    without = JM.definition(cls, pb, solver, torch.float64, jump=False)
    name = JM.JUMP_ONLY[cls]
    gap = rel_err(without["traj"], r64["traj"], dim=2) if bool(torch.isfinite(without["traj"]).all()) else float("inf")
    gap_g = rel_err(without["g_theta"][name], r64["g_theta"][name])
    print("%s: without the hook the float64 trajectory differs by %.2e, g_theta[%s] by %.2e" % (label, gap, name, gap_g))
    assert gap > 100 * TOL and gap_g > 100 * 1e-4
    assert float(r64["g_theta"][name].abs().max(dim=1).values.min()) > 0.0  # (every data row has a sample that reads it)
    _compare(_kernel(cls, pb, solver), r64, r32, label)


def test_the_turbidostat_triggers_in_some_samples_of_every_row():
    """On the float64 run alone: in every data row at least one sample is diluted and at least one never is, at both shapes
    (modelgen_jump_models.problem asserts the same when it keeps the samples); a sample that is never diluted gets no gradient
    for `dil`, and the kernel's is exactly zero there too."""
    cls = JM.PrprTurbidostat
    for B, S in SHAPES:
        pb = JM.problem(cls, B, S)
        r64 = _reference(cls, pb, "rk4")[0]
        trig = JM.triggered(cls, r64["traj"])
        print("%dx%d: samples diluted per data row %s of %d" % (B, S, trig.sum(1).tolist(), S))
        assert bool(trig.any(1).all()) and bool((~trig).any(1).all())
        got = _kernel(cls, pb, "rk4")
        assert float(r64["g_theta"]["dil"][~trig].abs().max()) == 0.0 and float(got["g_theta"]["dil"][~trig].abs().max()) == 0.0
        assert float(got["g_theta"]["dil"][trig].abs().min()) > 0.0


def _diluted_cond(pb, keep, dose):
    """The wide cond of PrprDiluted with the given keep / dose series [B,T] beside the problem's light."""
    series = torch.stack([pb["series"][:, 0], keep, dose], dim=1)
    return FM.wide_cond(torch.zeros(pb["B"], 0), series)


def test_swapping_two_rows_forcings_swaps_their_results():
    """Three data rows with the same theta and observations and different schedules: with the forcings of rows 0 and 2
    exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits.  S = 100
    puts two data rows into one block."""
    cls, (B, S) = JM.PrprDiluted, SHAPES[1]
    base = JM.problem(cls, B, S)
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


@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
def test_an_event_at_point_0_and_one_at_the_last_point(solver):
    """An event at point 0 changes y_1 and leaves the stored y_0 alone (the trajectory holds the left limits); an event at the
    last point alone changes nothing, bit for bit -- its jump is not evaluated."""
    cls, (B, S) = JM.PrprDiluted, SHAPES[0]
    pb = JM.problem(cls, B, S)
    T = pb["T"]
    ones, zeros = torch.ones(B, T, dtype=torch.float64), torch.zeros(B, T, dtype=torch.float64)
    none = _kernel(cls, pb, solver, cond=_diluted_cond(pb, ones, zeros))
    keep, dose = ones.clone(), zeros.clone()
    keep[:, 0], dose[:, 0] = 0.5, 0.4
    first = _kernel(cls, pb, solver, cond=_diluted_cond(pb, keep, dose))
    assert torch.equal(first["traj"][..., 0], none["traj"][..., 0]) and torch.equal(first["xpred"][..., 0], none["xpred"][..., 0])
    # what y_1 has to be: the float64 definition under the same schedule, which differs from the one without the event by more
    # than 100 x the tolerance in every species with a non-zero initial state, in every trajectory
    want = JM.definition(cls, dict(pb, cond=_diluted_cond(pb, keep, dose)), solver, torch.float64)["traj"]
    plain = JM.definition(cls, dict(pb, cond=_diluted_cond(pb, ones, zeros)), solver, torch.float64)["traj"]
    change = ((want[..., 1] - plain[..., 1]).abs() / plain[..., 1].abs().clamp_min(1e-30)).amin(dim=(0, 1))
    print("%s: an event at point 0 moves y_1 of the float64 definition by at least %s per species (relative)"
          % (solver, ["%.2e" % v for v in change.tolist()]))
    assert float(change[:4].min()) > 100 * TOL
    e = rel_err(first["traj"], want, dim=2)
    print("%s: the kernel against that definition %.2e (bound %.0e)" % (solver, e, TOL))
    assert e <= TOL and rel_err(none["traj"], plain, dim=2) <= TOL
    assert float(none["g_theta"]["bolus"].abs().max()) == 0.0 and float(first["g_theta"]["bolus"].abs().min()) > 0.0
    keep, dose = ones.clone(), zeros.clone()
    keep[:, T - 1], dose[:, T - 1] = 0.5, 0.4
    last = _kernel(cls, pb, solver, cond=_diluted_cond(pb, keep, dose))
    for k in ("traj", "xpred", "logp", "loss"):
        assert torch.equal(last[k], none[k]), k
    for n in none["g_theta"]:
        assert torch.equal(last["g_theta"][n], none["g_theta"][n]), n


def test_the_c_api_declines_an_adaptive_solver():
    """vihds_ode_fwd and vihds_ode_bwd with dopri5 on a model with a jump: VIHDS_E_UNSUPPORTED with a message, nothing queued; a
    valid launch that follows is fine."""
    B, S, T = 3, 5, 9
    L = hip.lib()
    times = torch.tensor(JM.TIMES, device=DEV)
    for cls in (JM.PrprTurbidostat, JM.PrprDiluted):
        key = _key(cls)
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        C = max(len(cls.forcings) * T, 1)
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
        assert rc == hip.E_UNSUPPORTED and "state jump" in L.vihds_last_error().decode(), key
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and "state jump" in L.vihds_last_error().decode(), key
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
        with pytest.raises(NotImplementedError, match="state jump"):
            ops.OdeProblemSpec(key, "dopri5", row_of, len(slots), C=C)
        prob.solver = hip.SOLVERS["rk4"]
        assert fwd() == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(traj).all()) and float(traj.abs().max()) > 0.0


# ---- training: PrprDiluted through the plugin surface, on a plate whose items carry "forcings" ---------------------------------
N_PLATE = 20


def _diluted_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a small synthetic plate whose spec names PrprDiluted and whose dataset hands
    out a "forcings" [3][T] entry per row: the light and the row's dilution-and-dose schedule."""
    import models
    from vihds import synthetic

    cls = JM.PrprDiluted
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    class DilutedPlate(synthetic.SyntheticPlateDataset):
        def __init__(self, *a, **k):
            super(DilutedPlate, self).__init__(*a, **k)
            self.forcings = JM.series_of(cls, len(self), self.times.double()).float()

        def __getitem__(self, idx):
            item = super(DilutedPlate, self).__getitem__(idx)
            item["forcings"] = self.forcings[idx]
            return item

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        spec["params"]["global"].update({"aYFP_PR": ln(0.0, 2.0), "aCFP_PR": ln(0.0, 2.0), "bolus": ln(-0.7, 0.2)})
        return spec

    monkeypatch.setattr(synthetic, "SyntheticPlateDataset", DilutedPlate)
    monkeypatch.setitem(synthetic.WORKLOADS, "prpr_diluted", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("prpr_diluted",))
    out = synthetic.build("prpr_diluted", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.has_jump
    assert tuple(out[5].train_data.forcings.shape) == (B, 3, N_PLATE)
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step on PrprDiluted eagerly -- the loss finite, `bolus` (read by the jump alone) moves -- and the same step
    from its hipGraph replay: loss and every updated parameter equal."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _diluted_training(monkeypatch, 3, 5, hip_graph=graph)
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
        kb = [d.name for d in model.encoder.glob].index("bolus")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
