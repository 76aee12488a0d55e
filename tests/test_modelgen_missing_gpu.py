"""GPU tests of the missing observations of generated models (masked_obs<>, the mask words in the rows of cond, the selects at the
scoring points of ode_fwd_kernel and ode_bwd_kernel): the five classes of tests/modelgen_missing_models.py against their own
definitions in float64 with every fixed-grid solver; placeholders under the mask; a never-observed signal; a ragged tail against
the same class on the shorter grid; a fully observed mask against the unmasked twin; rows swapped bit for bit; a strongly
non-uniform grid and one long enough for the unstaged forward; evaluation, one training step and the step's hipGraph replay
through Training; the C API's answers.

Shapes: B=3, S=5 (one partly filled block) and B=3, S=100 (300 trajectories: the blocks span data rows, which is where a wrong
row or stride for the words shows); T=9.  Bounds: those of tests/test_modelgen_piecewise_gpu.py, as in the forcing tests.  The
precondition is asserted on the float64 run alone: everything finite, the loss not zero and no cancelling sum (sum |terms| at most
16 |sum|: the float32 torch run that scales the bounds loses the same digits), the gradient row of every parameter that the fully
observed problem scores not zero."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_missing_models as XM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4  # trajectory and x_predict per species / signal; log-likelihood per signal
RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # the forcing tests' grid: steps 0.1 .. 1.0
_REFS = {}


def _key(cls):
    modelgen.register_kernel(cls, cls in XM.NEURAL)
    return cls.model_key


def _reference(cls, B, S, solver, times=XM.TIMES, mask=XM.gaps_mask):
    k = (cls, B, S, solver, tuple(times), mask.__name__)
    if k not in _REFS:
        pb = XM.problem(cls, B, S, times, mask=mask)
        _REFS[k] = (XM.definition(cls, pb, solver, torch.float64), XM.definition(cls, pb, solver, torch.float32),
                    XM.definition(cls, pb, solver, torch.float64, observed=torch.ones_like(pb["observed"]), obs=pb["clean"]))
    return _REFS[k]


def _kernel(cls, pb, solver, obs=None, observed=None, cond=None, th=None, G=None, times=None):
    """Forward and adjoint through ops.OdeSolveObserve with the upstream gradient G on the log-likelihood.  observed: another
    mask than the problem's (None with cond given: the rows are taken as they are)."""
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == XM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([(th or pb["th"])[n] for n in slots]).float().to(DEV).requires_grad_(True)
    if cond is None:
        cond = pb["cond"] if observed is None else XM.cond_of(cls, pb["treatments"], pb["series"], observed)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    w = XM.flat_weights(pb)
    if w is not None:
        w = w.float().to(DEV).requires_grad_(True)
    obs = pb["obs"] if obs is None else obs
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(pb["times"] if times is None else times), f32(obs), None, w)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"] if G is None else G)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}, "g_w": None if w is None else w.grad.cpu()}


def _precondition(r64, full64, label):
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    assert float(r64["loss"]) != 0.0 and np.isfinite(float(r64["loss"]))
    assert r64["condition"] <= 16.0, "%s: the loss is a cancelling sum (%.1f)" % (label, r64["condition"])
    scored = [n for n, g in full64["g_theta"].items() if float(g.abs().max()) > 0.0]
    assert sorted(scored) == sorted(full64["g_theta"]), label  # (every slot of the five classes is read by some signal)
    for n in scored:
        g = r64["g_theta"][n]
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, "%s: %s" % (label, n)


def _compare(got, r64, r32, label, forward_only=False):
    """Prints every figure, then asserts: forward 1e-5 (log-likelihood 1e-4), the loss within max(1e-6, 8 x the float32 torch
    run's error), every theta row and every weight tensor within max(1e-4, 8 x the float32 torch run's error)."""
    lines, bad = [], []

    def check(name, e, bound):
        lines.append("%s %s: %.2e (bound %.2e)" % (label, name, e, bound))
        if not e <= bound:
            bad.append(lines[-1])

    check("traj", rel_err(got["traj"], r64["traj"], dim=2), TOL)
    check("xpred", rel_err(got["xpred"], r64["xpred"], dim=2), TOL)
    zero = r64["logp"] == 0.0  # (a never-observed signal: exactly 0 on both sides, and no scale for a relative error)
    assert torch.equal(got["logp"][zero], torch.zeros_like(got["logp"][zero]))
    check("logp", float(((got["logp"].double() - r64["logp"]).abs().amax(dim=(0, 1)) / r64["logp"].abs().amax(dim=(0, 1))).max()), TOL_LOGP)
    if not forward_only:
        scale = abs(float(r64["loss"]))
        check("loss", abs(float(got["loss"]) - float(r64["loss"])) / scale,
              max(1e-6, 8 * abs(float(r32["loss"]) - float(r64["loss"])) / scale))
        for n, g in r64["g_theta"].items():
            if g is None or float(g.abs().max()) == 0.0:
                assert float(got["g_theta"][n].abs().max()) == 0.0, n
                continue
            check("g_theta[%s]" % n, rel_err(got["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g)))
        o = 0
        for k, ref in enumerate(r64["g_w"]):  # (the precision network's weight gradients)
            g = got["g_w"][o:o + ref.numel()].view(ref.shape)
            o += ref.numel()
            assert float(ref.abs().max()) > 0.0
            check("weight tensor %d %s" % (k, tuple(ref.shape)), rel_err(g, ref), max(1e-4, 8 * rel_err(r32["g_w"][k], ref)))
        assert o == (0 if got["g_w"] is None else got["g_w"].numel())
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", XM.FIXED)
@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, NaN and 1e30 under
    the mask, against the class's own definition in float64."""
    B, S = shape
    r64, r32, full64 = _reference(cls, B, S, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(r64, full64, label)
    pb = XM.problem(cls, B, S)
    assert bool(torch.isnan(pb["obs"]).any()) and bool((pb["obs"] == 1e30).any())
    _compare(_kernel(cls, pb, solver), r64, r32, label)


@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_placeholders_under_the_mask_change_no_bit(cls):
    """NaN / 1e30, 1e30 everywhere and 0 everywhere under the mask: logp, g_theta and the weight gradients are the same bits.
    (The class under NeuralPrecisions at B=3, S=5: its bias gradients are added up with one atomic per wavefront, and a launch of
    one wavefront adds them in one order; the others at B=3, S=100.)"""
    B, S = SHAPES[0] if cls in XM.NEURAL else SHAPES[1]
    pb = XM.problem(cls, B, S)
    a = _kernel(cls, pb, "rk4")
    assert bool(torch.isfinite(a["logp"]).all()) and all(bool(torch.isfinite(g).all()) for g in a["g_theta"].values())
    assert (a["g_w"] is not None) == (cls in XM.NEURAL)
    for kinds in ((1e30, 1e30), (0.0, 0.0)):
        b = _kernel(cls, pb, "rk4", obs=XM.with_placeholders(pb["clean"], pb["observed"], kinds))
        assert torch.equal(b["logp"], a["logp"]), kinds
        for n in a["g_theta"]:
            assert torch.equal(b["g_theta"][n], a["g_theta"][n]), (kinds, n)
        if a["g_w"] is not None:
            assert bool(torch.isfinite(a["g_w"]).all()) and torch.equal(b["g_w"], a["g_w"]), kinds


@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_a_never_observed_signal(cls):
    """logp of the signal is exactly 0.0; with constant precisions the gradient of that signal's precision row is exactly 0."""
    B, S = SHAPES[1]
    pb = XM.problem(cls, B, S)
    got = _kernel(cls, pb, "midpoint")
    b, j = XM.EMPTY
    assert torch.equal(got["logp"][b, :, j], torch.zeros(S)) and bool((got["logp"][b, :, [0, 1, 3]] != 0.0).all())
    assert bool((got["logp"][0] != 0.0).all())
    if "prec_yfp" in got["g_theta"]:
        assert XM.PREC[j] == "prec_yfp"
        assert torch.equal(got["g_theta"]["prec_yfp"][b], torch.zeros(S)) and bool((got["g_theta"]["prec_yfp"][0] != 0.0).all())


@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_a_ragged_tail_is_the_shorter_grid(cls):
    """Every row loses its last three points: logp equals the same class run on the first six points bit for bit (the steps behind
    the last scored point change nothing before it), gradients agree within the theta bound."""
    B, S = SHAPES[1]
    pb = XM.problem(cls, B, S, mask=XM.tail_mask)
    T = pb["T"]
    long = _kernel(cls, pb, "rk4")
    short_pb = dict(pb, times=pb["times"][:T - 3], series=pb["series"][:, :, :T - 3], T=T - 3)
    ones = torch.ones(B, 4, T - 3, dtype=torch.bool)
    short = _kernel(cls, short_pb, "rk4", obs=pb["clean"][:, :, :T - 3], observed=ones)
    assert torch.equal(long["logp"], short["logp"])
    assert torch.equal(long["traj"][..., :T - 3], short["traj"]) and torch.equal(long["xpred"][..., :T - 3], short["xpred"])
    r64, r32, _ = _reference(cls, B, S, "rk4", mask=XM.tail_mask)
    for n, g in short["g_theta"].items():
        e = rel_err(long["g_theta"][n], g)
        print("g_theta[%s]: ragged tail against the short grid %.2e" % (n, e))
        assert e <= max(1e-4, 8 * rel_err(r32["g_theta"][n], r64["g_theta"][n])), n


@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_a_fully_observed_mask_is_the_unmasked_twin(cls, solver):
    """Within the forward bounds; bit equality is not required (the select can change how the accumulation is contracted)."""
    B, S = SHAPES[1]
    pb = XM.problem(cls, B, S)
    twin = XM.TWIN[cls]
    masked = _kernel(cls, pb, solver, obs=pb["clean"], observed=torch.ones_like(pb["observed"]))
    plain = _kernel(twin, pb, solver, obs=pb["clean"], cond=XM.cond_of(twin, pb["treatments"], pb["series"]))
    assert torch.equal(masked["traj"], plain["traj"]) and torch.equal(masked["xpred"], plain["xpred"])  # (the mask scores only)
    _compare(masked, plain, None, "%s %s fully observed against %s" % (cls.__name__, solver, twin.__name__), forward_only=True)


@pytest.mark.parametrize("cls", [XM.PrprMasked, XM.LightSub4Masked], ids=lambda c: c.__name__)
def test_swapping_two_rows_observations_and_masks_swaps_their_results(cls):
    """Three data rows with the same theta, treatments and forcings and different observations and masks: with rows 0 and 2
    exchanged, every result of row 0 is bit for bit what row 2 gave, and the other way round; row 1 keeps its bits.  (The class
    with process noise draws per trajectory index: its states stay with the row, so only what is scored moves -- compared on a
    batch whose draws are switched off by sigma = 0.)"""
    B, S = SHAPES[1]
    base = XM.problem(cls, B, S)
    same = lambda v: v[:1].expand_as(v).contiguous()  # noqa: E731
    th = {n: same(v) for n, v in base["th"].items()}
    if "sigma" in th and cls._diffusion_def is not None:
        th["sigma"] = torch.zeros_like(th["sigma"])
    G = same(base["G"]["logp"])
    tr, se = same(base["treatments"]), same(base["series"])
    perm = [2, 1, 0]
    a = _kernel(cls, base, "rk4", th=th, G=G, cond=XM.cond_of(cls, tr, se, base["observed"]))
    b = _kernel(cls, base, "rk4", th=th, G=G, cond=XM.cond_of(cls, tr, se, base["observed"][perm]), obs=base["obs"][perm])
    assert not torch.equal(a["logp"][0], a["logp"][2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(b[k], a[k][perm]), k
    for n in a["g_theta"]:
        if n == "sigma" and cls._diffusion_def is not None:
            continue  # (d loss / d sigma at sigma = 0 is the adjoint times the trajectory's own draws, which stay with the index)
        assert torch.equal(b["g_theta"][n], a["g_theta"][n][perm]), n


@pytest.mark.parametrize("solver", ["midpoint", "rk4"])
@pytest.mark.parametrize("cls", [XM.PrprMasked, XM.LightSub4Masked], ids=lambda c: c.__name__)
def test_a_non_uniform_grid(cls, solver):
    B, S = SHAPES[1]
    r64, r32, full64 = _reference(cls, B, S, solver, RAGGED)
    _precondition(r64, full64, "ragged grid")
    _compare(_kernel(cls, XM.problem(cls, B, S, RAGGED), solver), r64, r32, "%s %s ragged grid" % (cls.__name__, solver))


def _long_mask(B, T):
    """The gaps of gaps_mask stretched to a long grid: row 1 loses every third point of signal 1 and every fifth of signal 3,
    row 2 never observes signal 2, loses its last third and the first point of signal 0."""
    m = torch.ones(B, 4, T, dtype=torch.bool)
    m[1, 1, ::3] = False
    m[1, 3, 2::5] = False
    m[2, 2, :] = False
    m[2, :, T - T // 3:] = False
    m[2, 0, 0] = False
    return m


def test_a_grid_too_long_for_the_staged_forward():
    """launch_fwd_s stages times, observations and mask words in LDS up to 32 KB: 4 T (1 + nb (4 + K + 1)) bytes, with nb = 2
    data rows per 64-thread block at B=3, S=100 and K=0: T = 745 is the first grid that takes the unstaged forward (744 * 11 * 4
    = 32 736 bytes still fit)."""
    cls, (B, S), T = XM.PrprMasked, SHAPES[1], 745
    assert 4 * (T - 1) * (1 + 2 * 5) <= 32 * 1024 < 4 * T * (1 + 2 * 5)
    for n, stage in ((T - 1, "staged"), (T, "unstaged")):
        times = torch.linspace(0.0, 3.7, n, dtype=torch.float64).tolist()
        r64, r32, full64 = _reference(cls, B, S, "midpoint", times, _long_mask)
        _precondition(r64, full64, "long grid")
        _compare(_kernel(cls, XM.problem(cls, B, S, times, mask=_long_mask), "midpoint"), r64, r32,
                 "PrprMasked midpoint T=%d (%s)" % (n, stage))


def test_the_c_api_declines_what_the_host_refuses_first():
    """C too small: VIHDS_E_BADARG; an adaptive solver: VIHDS_E_UNSUPPORTED, from the forward entry point and from the
    host-driven controller's.  (GeneratedOdeModel.solve raises before either: tests/test_modelgen_missing_host.py.)"""
    for cls in (XM.PrprMasked, XM.LightSub4Masked):
        B, S = SHAPES[0]
        pb = XM.problem(cls, B, S)
        key = _key(cls)
        slots = hip.model_slots(key)
        row_of = {n: i for i, n in enumerate(slots)}
        T, C = pb["T"], pb["cond"].shape[1]
        assert C == (len(cls.forcings) + 1) * T + (2 if cls._diffusion_def is not None else 0)
        th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV)
        f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
        cond, times, obs = f32(pb["cond"]), f32(pb["times"]), f32(pb["clean"])
        N = len(cls.species)
        traj, xpred, logp = torch.empty((T, N, B, S), device=DEV), torch.empty((T, 4, B, S), device=DEV), torch.empty((4, B, S), device=DEV)
        L = hip.lib()

        def fwd(solver, width):
            # (the adaptive spec is declined by ops as well: build the fixed-grid one and change its solver id)
            prob = ops.OdeProblemSpec(key, "rk4", row_of, th.shape[0], C=width).bind(B, S, T)
            prob.solver = hip.SOLVERS[solver]
            rc = L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                                 hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
            torch.cuda.synchronize()
            return rc

        assert fwd("rk4", C) == 0
        assert fwd("rk4", C - 1) == -1 and "C is too small" in L.vihds_last_error().decode()
        assert fwd("rk4", C - T) == -1 and fwd("rk4", 1) == -1
        assert fwd("dopri5", C) == hip.E_UNSUPPORTED
        if cls.substeps == 1:  # (a class with sub-steps is declined for those first)
            assert "missing observations" in L.vihds_last_error().decode()
        with pytest.raises(NotImplementedError, match="missing observations" if cls.substeps == 1 else "adaptive solver 'dopri5'"):
            ops.OdeProblemSpec(key, "dopri5", row_of, th.shape[0], C=C)


# ---- training: ReaderStudentForcedMasked through the plugin surface, on a plate whose items carry "observed" ---------------------
N_PLATE = 20


def _plate_mask(n, T):
    """observed [n,4,T] of the synthetic plate: the three rows of gaps_mask's kind, repeated."""
    m = torch.ones(n, 4, T, dtype=torch.bool)
    for b in range(n):
        if b % 3 == 1:
            m[b, 1, 1::3] = False
            m[b, 3, ::4] = False
        if b % 3 == 2:
            m[b, 2, :] = False
            m[b, :, T - 3:] = False
            m[b, 0, 0] = False
    return m


def _masked_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate whose spec names ReaderStudentForcedMasked and whose dataset
    hands out "forcings" [1][T] and "observed" [4][T] per row, with NaN written under the mask and then filled as
    datasets.fill_unobserved fills it: what a dataset with missing entries stores."""
    import models
    from vihds import datasets, synthetic

    cls = XM.ReaderStudentForcedMasked
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    assert models.register(cls) is cls

    class MaskedPlate(synthetic.SyntheticPlateDataset):
        def __init__(self, *a, **k):
            super(MaskedPlate, self).__init__(*a, **k)
            n = len(self)
            self.forcings = XM.FM.smooth_series(n, self.times.double())[:, None, :].float()
            self.observed = _plate_mask(n, self.n_times).float()

        def __getitem__(self, idx):
            # (the plate's observations are simulated from the model after the dataset is built: the holes are cut here)
            item = super(MaskedPlate, self).__getitem__(idx)
            flags = self.observed.bool().numpy()
            holes = self.observations.clone().numpy()
            holes[~flags] = np.nan
            filled = torch.from_numpy(datasets.fill_unobserved(self.times.numpy(), holes, flags))
            item.update(observations=filled[idx], forcings=self.forcings[idx], observed=self.observed[idx])
            return item

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        glob = spec["params"]["global"]
        known = set(glob) | set(spec["params"]["local"]) | set(spec["params"]["constant"])
        glob.update({n: synthetic._ln(float(np.log(v)), 0.2) for n, v in XM.FM.READER_BASE.items() if n not in known})
        return spec

    monkeypatch.setattr(synthetic, "SyntheticPlateDataset", MaskedPlate)
    monkeypatch.setitem(synthetic.WORKLOADS, "masked_reader", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("masked_reader",))
    out = synthetic.build("masked_reader", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.likelihood_kind == "custom"
    assert tuple(out[5].train_data.observed.shape) == (B, 4, N_PLATE) and not bool(out[5].train_data.observed.bool().all())
    return out


def _samples(cls, theta, q, p):
    return ({n: getattr(theta, n).detach().double().cpu() for n in XM.slot_names(cls)},
            p.log_prob(theta).detach().double().cpu(), q.log_prob(theta).detach().double().cpu())


def test_evaluation_pass_with_a_mask(monkeypatch, tmp_path):
    """Training.evaluate at B=3, S=5: the ELBO is within 1e-4 relative of the one formed in float64 from the pass's own samples,
    the batch's forcings and its mask with the model's definition; what the encoder reads is finite."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _masked_training(monkeypatch, B, S, hip_graph=False)
    cls = XM.ReaderStudentForcedMasked
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
    assert bool(torch.isfinite(batch.observations).all()) and bool(torch.isfinite(training.train_data.observations).all())
    th, log_p, log_q = seen["samples"]
    wide = ode.row_inputs(batch).double().cpu()
    n_tr = ode.n_treatments
    assert wide.shape == (B, n_tr + 2 * N_PLATE)
    assert torch.equal(wide[:, n_tr + N_PLATE:], XM.words_of(batch.observed.bool().cpu()))
    observed = batch.observed.bool().cpu()
    # (the definition reads the model's n_conditions treatments in front of the samples)
    cond = torch.cat([wide[:, :int(cls.n_conditions)], wide[:, n_tr:]], dim=1)
    obs = XM.with_placeholders(batch.observations.double().cpu(), observed)  # (NaN / 1e30 under the mask: the fill is never scored)
    _, _, logp = XM.forward(cls, th, cond, batch.times.double().cpu(), "rk4", obs, observed)
    log_w = logp.sum(2) + log_p - log_q
    ref = float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    got = float(np.asarray(res.elbo))
    print("elbo %.6f, float64 %.6f" % (got, ref))
    assert bool(torch.isfinite(logp).all()) and abs(got - ref) <= 1e-4 * abs(ref)
    assert torch.equal(logp[2, :, 2], torch.zeros(S, dtype=torch.float64))


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step eagerly through the step that calls Training.cost (fused_step_tail off, so that the step's samples can be
    read) -- the loss within the loss bound of the float64 definition on those samples --, one through the default step -- every
    updated parameter finite --, and the default step from its hipGraph replay: loss and every updated parameter equal."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    cls = XM.ReaderStudentForcedMasked
    runs = {}
    for graph in ("through cost", False, None):
        over = dict(hip_graph=False, fused_step_tail=False) if graph == "through cost" else dict(hip_graph=graph)
        args, settings, data, parameters, model, training = _masked_training(monkeypatch, 3, 5, **over)
        assert training.use_graph == (graph is None)
        batch = training.train_data
        seen = {}
        if graph == "through cost":
            cost = training.cost

            def spy(b, results, theta, q, p, _cost=cost, **kw):
                seen.update(samples=_samples(cls, theta, q, p))
                return _cost(b, results, theta, q, p, **kw)

            monkeypatch.setattr(training, "cost", spy)
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
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
        assert bool(seen) == (graph == "through cost")
        if seen:
            ode = model.decoder.ode_model
            th, log_p, log_q = seen["samples"]
            S = log_p.shape[1]
            wide = ode.row_inputs(batch).double().cpu()
            cond = torch.cat([wide[:, :int(cls.n_conditions)], wide[:, ode.n_treatments:]], dim=1)
            observed = batch.observed.bool().cpu()
            obs = XM.with_placeholders(batch.observations.double().cpu(), observed)
            vals = {}
            for dtype in (torch.float64, torch.float32):
                t = {n: v.to(dtype) for n, v in th.items()}
                _, _, logp = XM.forward(cls, t, cond.to(dtype), batch.times.to(dtype).cpu(), "rk4", obs.to(dtype), observed)
                log_w = logp.double().sum(2) + log_p - log_q
                vals[dtype] = -float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
            ref, e32 = vals[torch.float64], abs(vals[torch.float32] - vals[torch.float64]) / abs(vals[torch.float64])
            e = abs(loss - ref) / abs(ref)
            print("eager step loss %.6f, float64 %.6f: %.2e (float32 torch %.2e)" % (loss, ref, e, e32))
            assert e <= max(1e-6, 8 * e32)
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
