"""GPU tests of the process noise of generated models (has_diffusion<>, noisy_step / noisy_step_vjp of csrc/vihds_sde.hpp in the
time loops of ode_fwd_kernel and ode_bwd_kernel and in the sub-step loops): the kernel's own draws, read back through Brownian8,
against the numpy restatement of tests/sde_ref.py; PrprLangevin, LightSub4 and DilutedHooked against the float64 definition of
tests/modelgen_sde_models.py, which is fed the draws read back from the kernels, with every fixed-grid solver; the first two rows
of a problem run on their own; the adjoint run twice; the statistics of OrnsteinUhlenbeck over 16 384 trajectories; the C API's
answers; one training step eagerly and from its hipGraph replay.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (two blocks and a tail, the blocks spanning data rows); T=9 on the
ragged grid of tests/test_modelgen_forcing_gpu.py (steps 0.1 .. 1.0) and one case with T=2.  Bounds: those of
tests/test_modelgen_delay_gpu.py.  Every comparison first asserts its preconditions on the float64 run alone."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_sde_models as SM
import sde_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
TOL, TOL_LOGP = 1e-5, 1e-4  # trajectory and x_predict per species / signal; log-likelihood per signal
TOL_U = 1e-4  # the kernel's normals against the numpy restatement, absolute (the bound of the theta stream's check)
KINK = 1e-3
_KEYS, _REFS, _DRAWS, _WORST = {}, {}, {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert cls.model_key in hip.GENERATED_DIFFUSION
    return _KEYS[cls]


def _launch(cls, solver, th, cond, times, obs, G=None):
    """ops.OdeSolveObserve on float32 copies; with G the adjoint of sum(logp * G) too."""
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == SM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([th[n] for n in slots]).float().to(DEV).requires_grad_(G is not None)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=cond.shape[1])
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(cond), f32(times), f32(obs), None, None)
    out = {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(), "logp": H.view_bs4(logp).detach().cpu()}
    if G is not None:
        loss = (H.view_bs4(logp) * f32(G)).sum()
        loss.backward()
        out.update(loss=loss.detach().cpu(), g_theta={n: th.grad[row_of[n]].cpu() for n in slots})
    torch.cuda.synchronize()
    return out


def _kernel_draws(B, S, n_steps, key):
    """xi [B,S,8,n_steps] as the kernels draw them: Brownian8 on a grid of n_steps unit steps, whose stored state at point
    c + 1 is exactly the draw of step c (rhs = 0, amplitude 1, sqrt(1) = 1, a jump to zero after every point)."""
    k = (B, S, n_steps, tuple(key))
    if k not in _DRAWS:
        th = {n: torch.ones(B, S) for n in SM.slot_names(SM.Brownian8)}
        cond = torch.tensor([float(key[0]), float(key[1])])[None, :].expand(B, 2)
        times = torch.arange(n_steps + 1, dtype=torch.float32)
        got = _launch(SM.Brownian8, "euler", th, cond, times, torch.zeros(B, 4, n_steps + 1))
        assert float(got["traj"][..., 0].abs().max()) == 0.0
        _DRAWS[k] = got["traj"][..., 1:].contiguous()
    return _DRAWS[k]


# ---- the draws ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_draws_against_the_numpy_restatement(shape):
    B, S = shape
    n = 8
    got = _kernel_draws(B, S, n, SM.KEY)
    want = torch.from_numpy(sde_ref.expected_draws(B, S, 8, n, SM.KEY))
    e = float((got - want).abs().max())
    print("draws %dx%d: largest difference %.2e (bound %.0e); mean %.3f, variance %.3f" % (B, S, e, TOL_U, float(got.mean()), float(got.var())))
    assert e <= TOL_U
    # every solver draws the same numbers (the step index and the key do not depend on the scheme; h = 1 for each of them)
    th = {n_: torch.ones(B, S) for n_ in SM.slot_names(SM.Brownian8)}
    cond = torch.tensor([float(SM.KEY[0]), float(SM.KEY[1])])[None, :].expand(B, 2)
    times, obs = torch.arange(n + 1, dtype=torch.float32), torch.zeros(B, 4, n + 1)
    for solver in ("modeuler", "modeulerwhile", "midpoint", "rk4"):
        assert torch.equal(_launch(SM.Brownian8, solver, th, cond, times, obs)["traj"][..., 1:], got), solver
    # another key gives other draws, the same key the same bits; per-row keys are per row
    other = (SM.KEY[0] + 1, SM.KEY[1])
    assert not torch.equal(_kernel_draws(B, S, n, other), got)
    assert float((_kernel_draws(B, S, n, other) - torch.from_numpy(sde_ref.expected_draws(B, S, 8, n, other))).abs().max()) <= TOL_U
    again = _launch(SM.Brownian8, "euler", th, cond, times, obs)["traj"][..., 1:]
    assert torch.equal(again, got)
    rows = torch.tensor([[float(SM.KEY[0]), float(SM.KEY[1])], [float(other[0]), float(other[1])], [0.0, 16777215.0]][:B])
    mixed = _launch(SM.Brownian8, "euler", th, rows, times, obs)["traj"][..., 1:]
    assert torch.equal(mixed[0], got[0]) and torch.equal(mixed[1], _kernel_draws(B, S, n, other)[1])
    assert float((mixed - torch.from_numpy(sde_ref.expected_draws(B, S, 8, n, rows.long().numpy()))).abs().max()) <= TOL_U


# ---- against the float64 definition -----------------------------------------------------------------------------------------------
def _definition(cls, pb, solver, dtype, xi):
    """The definition with torch ops in `dtype`, autograd for the gradient of sum(logp * G) with respect to theta."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    starts = []  # (the start state of every step, sub-steps included: where the amplitudes are evaluated)
    xs, xp, logp = SM.forward(cls, th, pb["cond"].to(dtype), pb["times"].to(dtype), solver, pb["obs"].to(dtype), xi.to(dtype), starts)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": xs.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "starts": starts,
            "g_theta": {n: v.grad for n, v in th.items()}}


def _reference(cls, pb, solver):
    """(float64 run, float32 run, the noise-free float64 run), all fed the draws read back from the kernels."""
    k = (cls, id(pb), solver)
    if k not in _REFS:
        xi = _kernel_draws(pb["B"], pb["S"], SM.n_steps(cls, pb["T"]), pb["key"])
        _REFS[k] = (_definition(cls, pb, solver, torch.float64, xi), _definition(cls, pb, solver, torch.float32, xi),
                    _definition(cls, pb, solver, torch.float64, torch.zeros_like(xi)))
    return _REFS[k]


def _precondition(cls, pb, r64, quiet, label):
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    margin = SM.kink_margin(cls, r64["starts"])
    moved = min(float((r64["traj"][:, :, j] - quiet["traj"][:, :, j]).abs().max()
                      / (quiet["traj"][:, :, j].max() - quiet["traj"][:, :, j].min())) for j in SM.noisy_species(cls))
    # the loss is bounded relative to its own size, with a floor of 1e-6 = 16 float32 roundings: a sum whose terms cancel loses
    # its condition number, so with terms good to about 4 roundings the inputs must keep that number below 4
    terms = r64["logp"] * pb["G"]["logp"]
    condition = float(terms.abs().sum() / terms.sum().abs())
    print("%s: kink margin %.2e, the noise moves a noisy species by at least %.1f %% of its range, condition number of the loss %.2f"
          % (label, margin, 100 * moved, condition))
    assert margin >= KINK, "badly posed inputs: %s has an argument of sqrt / maximum within %.2e of its kink" % (label, margin)
    assert moved >= 0.01, "badly posed inputs: a kernel that ignored the hook would pass %s" % label
    assert condition <= 4.0, "badly posed inputs: the loss of %s is a cancelling sum (%.1f)" % (label, condition)


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
@pytest.mark.parametrize("solver", SM.FIXED)
@pytest.mark.parametrize("cls", SM.PARITY, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, against the float64
    definition fed the kernels' own draws; the sigma row is part of the comparison and is not zero in the reference."""
    B, S = shape
    pb = SM.problem(cls, B, S)
    r64, r32, quiet = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(cls, pb, r64, quiet, label)
    assert float(r64["g_theta"]["sigma"].abs().max()) > 0.0
    _compare(_launch(cls, solver, pb["th"], pb["cond"], pb["times"], pb["obs"], pb["G"]["logp"]), r64, r32, label)


@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
def test_two_time_points(solver):
    """T = 2: one interval (four sub-steps of it for LightSub4)."""
    for cls in (SM.PrprLangevin, SM.LightSub4):
        B, S = SHAPES[1]
        pb = SM.problem(cls, B, S, times=[0.25, 0.75])
        r64, r32, quiet = _reference(cls, pb, solver)
        _precondition(cls, pb, r64, quiet, "%s %s T=2" % (cls.__name__, solver))
        assert float(r64["g_theta"]["sigma"].abs().max()) > 0.0
        _compare(_launch(cls, solver, pb["th"], pb["cond"], pb["times"], pb["obs"], pb["G"]["logp"]), r64, r32,
                 "%s %s T=2" % (cls.__name__, solver))


@pytest.mark.parametrize("cls", [SM.PrprLangevin, SM.LightSub4], ids=lambda c: c.__name__)
def test_the_first_two_rows_alone_and_the_adjoint_twice(cls):
    """The first two rows of the B = 3 problem run as a B = 2 problem with the same key give the same forward bits (the counter
    holds b * S + s, not the launch's size); and the same launch twice gives the same g_theta bit for bit (no atomics)."""
    B, S = SHAPES[1]
    pb = SM.problem(cls, B, S)
    a = _launch(cls, "rk4", pb["th"], pb["cond"], pb["times"], pb["obs"], pb["G"]["logp"])
    again = _launch(cls, "rk4", pb["th"], pb["cond"], pb["times"], pb["obs"], pb["G"]["logp"])
    two = _launch(cls, "rk4", {n: v[:2] for n, v in pb["th"].items()}, pb["cond"][:2], pb["times"], pb["obs"][:2], pb["G"]["logp"][:2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(two[k], a[k][:2]), k
        assert torch.equal(again[k], a[k]), k
    for n in a["g_theta"]:
        assert torch.equal(again["g_theta"][n], a["g_theta"][n]), n
        assert torch.equal(two["g_theta"][n], a["g_theta"][n][:2]), n
    assert float(a["g_theta"]["sigma"].abs().max()) > 0.0


# ---- statistics -----------------------------------------------------------------------------------------------------------------
def test_the_statistics_of_the_additive_noise_model():
    """OrnsteinUhlenbeck with euler at B=4, S=4096 (n = 16 384 trajectories), T=9 on the ragged grid, every trajectory with the
    same a, sigma and start: at the last point the sample mean and variance across trajectories lie within 5 standard errors of
    the exact recursion m' = (1 - a h) m, Var' = (1 - a h)^2 Var + sigma^2 h (standard error sqrt(Var / n) and sqrt(2 / n) Var);
    the correlations between two species, between two consecutive steps' increments and between neighbouring trajectories are
    below 5 / sqrt(n) in absolute value (SM.ou_statistics).  The key SM.STAT_KEY is fixed, so the outcome is deterministic;
    tests/test_modelgen_sde_host.py runs the same figures on the CPU with the draws of tests/sde_ref.py under that key."""
    cls, B, S = SM.OrnsteinUhlenbeck, SM.STAT_B, SM.STAT_S
    th = {k: torch.full((B, S), v) for k, v in dict(SM.BASES[cls], **SM.STAT_THETA).items()}
    cond = torch.tensor([float(SM.STAT_KEY[0]), float(SM.STAT_KEY[1])])[None, :].expand(B, 2)
    times = torch.tensor(SM.RAGGED)
    traj = _launch(cls, "euler", th, cond, times, torch.zeros(B, 4, len(SM.RAGGED)))["traj"].double().reshape(B * S, 4, -1)
    mean_se, var_se, corrs, bound = SM.ou_statistics(traj, times)
    for j in range(4):
        print("species %d: mean off by %.2f standard errors, variance by %.2f" % (j, mean_se[j], var_se[j]))
    for what, c in corrs.items():
        print("correlation between %s: %.4f (bound %.4f)" % (what, c, bound))
    assert all(abs(v) <= 5.0 for v in mean_se + var_se)
    for what, c in corrs.items():
        assert abs(c) <= bound, what


# ---- the C API ------------------------------------------------------------------------------------------------------------------
def test_the_c_api_answers():
    """An adaptive id: VIHDS_E_UNSUPPORTED; a C too small by the two key columns: VIHDS_E_BADARG with its message; neither queues
    anything.  hip.GENERATED_DIFFUSION."""
    cls, (B, S) = SM.PrprLangevin, SHAPES[0]  # (no sub-steps and no jump: the answers are those of the process noise)
    pb = SM.problem(cls, B, S)
    key = _key(cls)
    assert key in hip.GENERATED_DIFFUSION and _key(SM.Brownian8) in hip.GENERATED_DIFFUSION
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    T, C, N = pb["T"], pb["cond"].shape[1], len(cls.species)
    assert C == 2
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV)
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    cond, times, obs = f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"])
    traj, xpred, logp = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV), torch.zeros((4, B, S), device=DEV)
    L = hip.lib()

    def fwd(p):
        rc = L.vihds_ode_fwd(ctypes.byref(p), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    narrow = ops.OdeProblemSpec(key, "rk4", row_of, th.shape[0], C=C - 2).bind(B, S, T)
    assert fwd(narrow) == -1 and "two words of its key" in L.vihds_last_error().decode()
    assert float(logp.abs().max()) == 0.0 and float(traj.abs().max()) == 0.0  # (nothing was launched)
    spec = ops.OdeProblemSpec(key, "rk4", row_of, th.shape[0], C=C)
    for solver in hip.ADAPTIVE_SOLVERS:
        with pytest.raises(NotImplementedError, match="process noise"):
            ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=C)
        p = spec.bind(B, S, T)
        p.solver = hip.SOLVERS[solver]
        assert fwd(p) == hip.E_UNSUPPORTED and "process noise" in L.vihds_last_error().decode(), solver
    p9 = spec.bind(B, S, T)
    p9.solver = hip.SOLVERS["beuler"]
    assert fwd(p9) == hip.E_UNSUPPORTED
    assert float(logp.abs().max()) == 0.0 and float(traj.abs().max()) == 0.0
    assert L.vihds_ode_fwd_summaries_supported(ctypes.byref(spec.bind(B, S, T))) == 0
    assert fwd(spec.bind(B, S, T)) == 0 and float(traj.abs().max()) > 0.0


# ---- training: OrnsteinUhlenbeck through the plugin surface ---------------------------------------------------------------------------
N_PLATE = 20


def _noisy_training(monkeypatch, B, S, **over):
    import models
    from vihds import synthetic

    # (additive noise: the gradient is finite wherever the noise takes the state -- a square-root amplitude has an infinite
    # derivative at 0, where the noise of a culture that starts at OD 0.002 does take it, and such a step is skipped)
    cls = SM.OrnsteinUhlenbeck
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        spec["params"]["constant"]["init"] = 1.0
        spec["params"]["global"].update({"a": ln(float(np.log(0.8)), 0.2), "sigma": ln(float(np.log(0.5)), 0.2)})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "ornstein_uhlenbeck", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("ornstein_uhlenbeck",))
    out = synthetic.build("ornstein_uhlenbeck", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.has_diffusion
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step eagerly -- the loss and every updated parameter finite, the prior row behind sigma moved -- and the same
    step captured and replayed from the same key state: the same loss.  A second replay draws afresh: another loss, and the key
    state has advanced by two."""
    from vihds.utils import TrainingLogData

    monkeypatch.chdir(tmp_path)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters, model, training = _noisy_training(monkeypatch, 3, 5, hip_graph=graph)
        assert training.use_graph == (graph is None)
        ode = model.decoder.ode_model
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
        print("hip_graph=%s: loss %.6f, key state %s" % (graph, loss, ode.noise_state(DEV).tolist()))
        assert np.isfinite(loss) and all(bool(torch.isfinite(v).all()) for v in after.values())
        assert ode.noise_state(DEV).tolist() == [1.0, 0.0]  # (one step taken: a capture's warm-up is rolled back)
        kb = [d.name for d in model.encoder.glob].index("sigma")
        assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb])
        if graph is None:
            assert training.use_graph, "the capture fell back to eager launches"
            assert training._run_batch(0.0, batch, log, next_batch=batch)
            second = float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo)
            torch.cuda.synchronize()
            print("second replay: loss %.6f" % second)
            assert np.isfinite(second) and second != loss and ode.noise_state(DEV).tolist() == [2.0, 0.0]
    (la, pa), (lb, pb_) = runs[False], runs[None]
    assert la == lb, (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb_[k]), k
