"""GPU tests of the forcings of generated models (n_forcings<>, set_interval / set_point in the time loops of ode_fwd_kernel
and ode_bwd_kernel): PrprForced, PlateReaderForced and ForcedSwitch against their own definitions in float64 with every
fixed-grid solver; a strongly non-uniform grid; a grid long enough for the unstaged forward; rows swapped bit for bit; the
constant-treatment twin; evaluation, one training step and the step's hipGraph replay through Training; the C API's answers.

Shapes: B=3, S=5 (one partly filled block) and B=3, S=100 (300 trajectories: the blocks span data rows, which is where a wrong
row or stride for the samples shows); T=9.  Bounds: those of tests/test_modelgen_piecewise_gpu.py.  ForcedSwitch first asserts
the precondition on the float64 run alone: every switch at least modelgen_piecewise_models.MARGIN wide."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_forcing_models as FM
import modelgen_piecewise_models as PM

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


def _definition(cls, pb, solver, dtype):
    """The definition with torch ops in `dtype`, autograd for the gradient of sum(logp * G) with respect to theta and the
    network weights; in float64 the margins of its switches are recorded."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    W = {name: tuple(leaf(w) for w in ws) for name, ws in pb["W"].items()} or None
    with FM.recording() as m:
        xs, xp, prec, logp = FM.forward(cls, th, pb["cond"].to(dtype), pb["times"].to(dtype), solver, pb["obs"].to(dtype), W)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    full = torch.cat([xs, prec], dim=2) if cls._precision_def is not None else xs
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: v.grad for n, v in th.items()}, "g_w": [w.grad for ws in (W or {}).values() for w in ws],
            "margins": m}


def _reference(cls, B, S, solver, times=FM.TIMES):
    k = (cls, B, S, solver, tuple(times))
    if k not in _REFS:
        pb = FM.problem(cls, B, S, times)
        _REFS[k] = (_definition(cls, pb, solver, torch.float64), _definition(cls, pb, solver, torch.float32))
    return _REFS[k]


def _kernel(cls, pb, solver, cond=None, th=None):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == FM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([(th or pb["th"])[n] for n in slots]).float().to(DEV).requires_grad_(True)
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


def _precondition(r64, label):
    m = r64["margins"]
    if m.by_label:
        worst = min(m.by_label, key=m.by_label.get)
        print("%s: smallest switch margin %.2e (%s)" % (label, m.smallest, worst))
        assert m.smallest >= PM.MARGIN, "badly posed inputs: %s has margin %.2e" % (worst, m.smallest)
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k


def _compare(got, r64, r32, label):
    """Prints every figure, then asserts: forward 1e-5 (log-likelihood 1e-4), the loss within max(1e-6, 8 x the float32 torch
    run's error), every theta row and every weight tensor within max(1e-4, 8 x the float32 torch run's error)."""
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
@pytest.mark.parametrize("solver", FM.FIXED)
@pytest.mark.parametrize("cls", FM.MODELS, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, against
    torch_problem + O.simulate and the torch maps in float64."""
    B, S = shape
    r64, r32 = _reference(cls, B, S, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(r64, label)
    assert bool(r64["margins"].by_label) == (cls is FM.ForcedSwitch)
    pb = FM.problem(cls, B, S)
    assert not torch.equal(pb["series"][0], pb["series"][1]) and not torch.equal(pb["series"][1], pb["series"][2])
    _compare(_kernel(cls, pb, solver), r64, r32, label)


RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # steps 0.1 .. 1.0: a slope formed with the wrong interval's dt is far off


@pytest.mark.parametrize("solver", ["midpoint", "rk4"])
def test_a_non_uniform_grid(solver):
    cls, (B, S) = FM.PrprForced, SHAPES[1]
    r64, r32 = _reference(cls, B, S, solver, RAGGED)
    _precondition(r64, "ragged")
    _compare(_kernel(cls, FM.problem(cls, B, S, RAGGED), solver), r64, r32, "PrprForced %s ragged grid" % solver)


def test_a_grid_too_long_for_the_staged_forward():
    """launch_fwd_s stages times, observations and samples in LDS up to 32 KB: 4 T (1 + nb (4 + K)) bytes, with nb = 2 data
    rows per 64-thread block at B=3, S=100 and K=1: T = 745 is the first grid that takes the unstaged forward (744 * 11 * 4 =
    32 736 bytes still fit)."""
    cls, (B, S), T = FM.PrprForced, SHAPES[1], 745
    assert 4 * (T - 1) * (1 + 2 * 5) <= 32 * 1024 < 4 * T * (1 + 2 * 5)
    times = torch.linspace(0.0, 3.7, T, dtype=torch.float64).tolist()
    r64, r32 = _reference(cls, B, S, "midpoint", times)
    _precondition(r64, "long grid")
    _compare(_kernel(cls, FM.problem(cls, B, S, times), "midpoint"), r64, r32, "PrprForced midpoint T=%d" % T)


@pytest.mark.parametrize("cls", [FM.PrprForced, FM.ForcedSwitch], ids=lambda c: c.__name__)
def test_swapping_two_rows_forcings_swaps_their_results(cls):
    """Three data rows with the same theta, treatments and observations and different forcings: with the forcings of rows 0
    and 2 exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits."""
    B, S = SHAPES[1]
    base = FM.problem(cls, B, S)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    pb = dict(base, th={n: same(v) for n, v in base["th"].items()}, obs=same(base["obs"]),
              G={"logp": same(base["G"]["logp"])})
    perm = [2, 1, 0]
    series = base["series"]
    a = _kernel(cls, pb, "rk4", cond=FM.wide_cond(base["treatments"][:1].expand(B, -1), series))
    b = _kernel(cls, pb, "rk4", cond=FM.wide_cond(base["treatments"][:1].expand(B, -1), series[perm]))
    assert not torch.equal(a["traj"][0], a["traj"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n
    if a["g_w"] is not None:  # (a sum over all trajectories in a fixed order of blocks: the same terms in another order)
        assert rel_err(b["g_w"], a["g_w"]) <= 1e-5


@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
def test_a_constant_forcing_is_the_constant_treatment(solver):
    """The forcing gets no gradient and disturbs none: PrprForced with every sample equal to v against PrprTreated with the
    treatment log1p(v) -- the same trajectory and the same g_theta within the float32 bound of the float64 comparison."""
    B, S = SHAPES[1]
    pb = FM.problem(FM.PrprForced, B, S)
    v = torch.tensor([0.6, 1.0, 1.7], dtype=torch.float64)
    forced = _kernel(FM.PrprForced, pb, solver, cond=FM.wide_cond(torch.zeros(B, 0), v[:, None, None].expand(B, 1, pb["T"])))
    treated = _kernel(FM.PrprTreated, pb, solver, cond=torch.log1p(v)[:, None])
    ref = dict(pb, cond=torch.log1p(v)[:, None])
    r64, r32 = _definition(FM.PrprTreated, ref, solver, torch.float64), _definition(FM.PrprTreated, ref, solver, torch.float32)
    _compare(forced, r64, r32, "constant forcing against the twin's float64 definition, %s" % solver)
    for n, g in treated["g_theta"].items():
        e = rel_err(forced["g_theta"][n], g)
        print("g_theta[%s]: forcing against treatment %.2e" % (n, e))
        assert e <= max(1e-4, 8 * rel_err(r32["g_theta"][n], r64["g_theta"][n])), n
    assert rel_err(forced["traj"], treated["traj"], dim=2) <= TOL


def test_the_c_api_declines_what_the_host_refuses_first():
    """C too small: VIHDS_E_BADARG; an adaptive solver: VIHDS_E_UNSUPPORTED, from the forward entry point and from the
    host-driven controller's.  (GeneratedOdeModel.solve raises before either: tests/test_modelgen_forcing_host.py.)"""
    cls, (B, S) = FM.ForcedSwitch, SHAPES[0]
    pb = FM.problem(cls, B, S)
    key = _key(cls)
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    T, C = pb["T"], pb["cond"].shape[1]
    assert C == 1 + 2 * T
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV)
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    cond, times, obs = f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"])
    w = torch.cat([t.reshape(-1) for ws in pb["W"].values() for t in ws]).float().to(DEV)
    traj, xpred, logp = torch.empty((T, 4, B, S), device=DEV), torch.empty((T, 4, B, S), device=DEV), torch.empty((4, B, S), device=DEV)
    L = hip.lib()

    def fwd(solver, width):
        prob = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=width).bind(B, S, T)
        rc = L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), hip.ptr(w),
                             hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    assert fwd("rk4", C) == 0
    assert fwd("rk4", C - 1) == -1 and "C is too small" in L.vihds_last_error().decode()
    assert fwd("rk4", 1) == -1
    assert fwd("dopri5", C) == hip.E_UNSUPPORTED
    spec = ops.OdeProblemSpec(key, "dopri5", row_of, th.shape[0], C=C)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.adaptive_grid(spec, th, cond, times, None, w)


def _samples(cls, theta, q, p):
    """The samples of one pass (every slot the kernel reads) and their log-densities, copied to the host in float64."""
    return ({n: getattr(theta, n).detach().double().cpu() for n in FM.slot_names(cls)},
            p.log_prob(theta).detach().double().cpu(), q.log_prob(theta).detach().double().cpu())


# ---- training: ForcedSwitch through the plugin surface, on a plate whose items carry "forcings" --------------------------------
N_PLATE = 20


def _forced_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names ForcedSwitch and whose dataset hands out
    a "forcings" [2][T] entry per row: a square-wave light (levels 0.2 / 1.0, shifted from row to row) and a smooth
    temperature.  The plate's two treatments are more than the model's one: the samples sit behind both."""
    import models
    from vihds import synthetic

    cls = FM.ForcedSwitch
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    class ForcedPlate(synthetic.SyntheticPlateDataset):
        def __init__(self, *a, **k):
            super(ForcedPlate, self).__init__(*a, **k)
            n = len(self)
            self.forcings = torch.stack([FM.square_series(n, self.n_times), FM.smooth_series(n, self.times.double())], dim=1).float()

        def __getitem__(self, idx):
            item = super(ForcedPlate, self).__getitem__(idx)
            item["forcings"] = self.forcings[idx]
            return item

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        spec["params"]["global"]["boost"] = synthetic._ln(0.4, 0.2)
        return spec

    monkeypatch.setattr(synthetic, "SyntheticPlateDataset", ForcedPlate)
    monkeypatch.setitem(synthetic.WORKLOADS, "forced_switch", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("forced_switch",))
    out = synthetic.build("forced_switch", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.likelihood_kind == "custom" and ode.n_treatments == 2
    assert tuple(out[5].train_data.forcings.shape) == (B, 2, N_PLATE)
    return out


def test_evaluation_pass_with_forcings(monkeypatch, tmp_path):
    """Training.evaluate at B=3, S=5: the ELBO is within 1e-4 relative of the one formed in float64 from the pass's own
    samples, the network's weights and the batch's forcings with the model's definition."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _forced_training(monkeypatch, B, S, hip_graph=False)
    cls = FM.ForcedSwitch
    ode = model.decoder.ode_model
    model.eval()
    seen = {}
    cost = training.cost

    def spy(batch, results, theta, q, p, **kw):
        seen.update(batch=batch, samples=_samples(cls, theta, q, p))
        return cost(batch, results, theta, q, p, **kw)

    monkeypatch.setattr(training, "cost", spy)
    np.random.seed(12)
    torch.manual_seed(12)
    res = training.evaluate(training.train_data, S)
    batch = seen["batch"]
    th, log_p, log_q = seen["samples"]
    wide = ode.row_inputs(batch).double().cpu()
    assert wide.shape == (B, 2 + 2 * N_PLATE) and torch.equal(wide[:, 2:].float().reshape(B, 2, N_PLATE), batch.forcings.cpu())
    W = {name: tuple(w.detach().double().cpu() for w in ws) for name, ws in ode.network_weights().items()}
    with FM.recording() as m:
        xs, xp, prec, logp = FM.forward(cls, th, wide, batch.times.double().cpu(), "rk4", batch.observations.double().cpu(), W)
    print("smallest switch margin %.2e" % m.smallest)
    assert m.smallest >= PM.MARGIN
    log_w = logp.sum(2) + log_p - log_q
    ref = float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    got = float(np.asarray(res.elbo))
    print("elbo %.6f, float64 %.6f" % (got, ref))
    assert bool(torch.isfinite(logp).all()) and abs(got - ref) <= 1e-4 * abs(ref)


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step through the general path eagerly -- every gradient finite, `boost` (read in the branch the light
    selects) and the network's weights move -- and the same step from its hipGraph replay: loss and every updated parameter
    equal."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _forced_training(monkeypatch, 3, 5, hip_graph=graph)
        assert training.use_graph == (graph is None)
        batch = training.train_data
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
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
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
        moved = [k for k in after if not torch.equal(after[k], before[k])]
        assert any("nets.gate" in k for k in moved), moved
        glob_names = [d.name for d in model.encoder.glob]
        kb = glob_names.index("boost")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
