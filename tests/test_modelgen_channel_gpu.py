"""GPU tests of the reaction-channel noise of generated models (noise_channels<M>: the channel paths of noisy_step /
noisy_step_vjp in csrc/vihds_sde.hpp, inside the time loops and the sub-step loops of ode_fwd_kernel and ode_bwd_kernel):
ExpressionCLE, HookedChannels and Channels8 against the float64 definition of tests/modelgen_channel_models.py, which is fed the
kernels' own draws read back through Brownian8, with every fixed-grid solver; DiagonalTwin against the `diffusion` class it
restates, bit for bit; the conservation of A + B by ConversionPair; the statistics of SharedChannel over 16 384 trajectories; two
time points, the first two rows alone and the adjoint twice; the C API's answer to an adaptive solver; one training step eagerly
and from its hipGraph replay.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (two blocks and a tail, the blocks spanning data rows); T=9 on the
ragged grid (steps 0.1 .. 1.0) and one case with T=2.  Bounds and helpers: those of tests/test_modelgen_sde_gpu.py (_compare,
_launch, _kernel_draws).  Every comparison first asserts its preconditions on the float64 run alone."""
import ctypes

import numpy as np
import pytest
import torch

from vihds import hip, ops

import modelgen_channel_models as CM
import modelgen_sde_models as SM
import test_modelgen_sde_gpu as SG

pytestmark = pytest.mark.gpu
DEV = SG.DEV
SHAPES = SG.SHAPES
KINK = SG.KINK
_REFS = {}


# ---- against the float64 definition -----------------------------------------------------------------------------------------------
def _definition(cls, pb, solver, dtype, xi):
    """The definition with torch ops in `dtype`, autograd for the gradient of sum(logp * G) with respect to theta."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    starts = []  # (the start state of every step, sub-steps included: where the amplitudes are evaluated)
    xs, xp, logp = CM.forward(cls, th, pb["cond"].to(dtype), pb["times"].to(dtype), solver, pb["obs"].to(dtype), xi.to(dtype), starts,
                              pb.get("observed"))
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": xs.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "starts": starts,
            "g_theta": {n: v.grad for n, v in th.items()}}


def _reference(cls, pb, solver):
    """(float64 run, float32 run, the noise-free float64 run), all fed the draws read back from the kernels."""
    k = (cls, id(pb), solver)
    if k not in _REFS:
        xi = SG._kernel_draws(pb["B"], pb["S"], CM.n_steps(cls, pb["T"]), pb["key"])
        _REFS[k] = (_definition(cls, pb, solver, torch.float64, xi), _definition(cls, pb, solver, torch.float32, xi),
                    _definition(cls, pb, solver, torch.float64, torch.zeros_like(xi)))
    return _REFS[k]


def _precondition(cls, pb, r64, quiet, label):
    for k in ("traj", "xpred", "logp"):
        assert bool(torch.isfinite(r64[k]).all()), k
    margin = CM.kink_margin(cls, r64["starts"])
    moved = min(float((r64["traj"][:, :, j] - quiet["traj"][:, :, j]).abs().max()
                      / (quiet["traj"][:, :, j].max() - quiet["traj"][:, :, j].min())) for j in CM.noisy_species(cls))
    terms = r64["logp"] * pb["G"]["logp"]
    condition = float(terms.abs().sum() / terms.sum().abs())
    print("%s: kink margin %.2e, the noise moves a noisy species by at least %.1f %% of its range, condition number of the loss %.2f"
          % (label, margin, 100 * moved, condition))
    assert margin >= KINK, "badly posed inputs: %s has an argument of sqrt / maximum / where within %.2e of its kink" % (label, margin)
    assert moved >= 0.01, "badly posed inputs: a kernel that ignored the hook would pass %s" % label
    assert condition <= 4.0, "badly posed inputs: the loss of %s is a cancelling sum (%.1f)" % (label, condition)
    for n in CM.NOISE_PARAMETERS[cls]:
        assert float(r64["g_theta"][n].abs().max()) > 0.0, "badly posed inputs: the gradient row of %s is zero" % n


def _run(cls, solver, pb, with_gradient=True):
    return SG._launch(cls, solver, pb["th"], pb["cond"], pb["times"], pb["obs"], pb["G"]["logp"] if with_gradient else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", CM.FIXED)
@pytest.mark.parametrize("cls", CM.PARITY, ids=lambda c: c.__name__)
def test_against_the_definition_in_float64(cls, solver, shape):
    """Forward and adjoint through ops.OdeSolveObserve with a random upstream gradient on the log-likelihood, against the float64
    definition fed the kernels' own draws (channels 0 .. 7 of Brownian8's read-back); the rows of the noise parameters are part of
    the comparison and are not zero in the reference."""
    B, S = shape
    pb = CM.problem(cls, B, S)
    r64, r32, quiet = _reference(cls, pb, solver)
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    _precondition(cls, pb, r64, quiet, label)
    SG._compare(_run(cls, solver, pb), r64, r32, label)


# ---- the diagonal twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", ["euler", "rk4"])
def test_the_diagonal_twin_repeats_the_diffusion_class(solver, shape):
    """DiagonalTwin (one channel per noisy species, the diagonal amplitudes) on PrprLangevin's problem: trajectory, x_predict and
    log-likelihood equal the `diffusion` class's bit for bit; its theta gradient is held to the bound of the comparison with the
    definition (the two adjoints order the sum into the shared parameter's row in their own way)."""
    B, S = shape
    twin, diag = CM.DiagonalTwin, CM.TWIN[CM.DiagonalTwin]
    pb = SM.problem(diag, B, S)
    a, b = _run(twin, solver, pb), _run(diag, solver, pb)
    for k in ("traj", "xpred", "logp"):
        differ = float((a[k] - b[k]).abs().max())
        print("DiagonalTwin %s %dx%d %s: largest difference from the diffusion class %.2e" % (solver, B, S, k, differ))
        assert torch.equal(a[k], b[k]), k
    r64, r32, quiet = _reference(twin, pb, solver)
    label = "DiagonalTwin %s %dx%d" % (solver, B, S)
    _precondition(twin, pb, r64, quiet, label)
    SG._compare(a, r64, r32, label)


# ---- conservation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_conversion_conserves_the_total(shape):
    """ConversionPair under euler (rhs = 0, one channel with the columns [-sigma, +sigma]): at every stored point A + B equals its
    initial value within 2 n_steps 2^-23 max(|A|, |B|), the rounding of the two fused multiply-adds per step, and A itself moves
    by at least 1 % of its range.  A kernel that ignored the hook fails the second, one that drew per species the first."""
    B, S = shape
    cls = CM.ConversionPair
    pb = CM.problem(cls, B, S)
    traj = _run(cls, "euler", pb, with_gradient=False)["traj"].double()
    A, Bs = traj[:, :, 0], traj[:, :, 1]
    steps = CM.n_steps(cls, pb["T"])
    drift = ((A + Bs) - (A + Bs)[..., :1]).abs()
    bound = 2 * steps * 2.0 ** -23 * torch.maximum(A.abs(), Bs.abs())  # (at every stored point, from that point's own values)
    moved = float((A - A[..., :1]).abs().max() / (A.max() - A.min()))
    print("ConversionPair %dx%d: A + B drifts by at most %.2e (%.2f of its bound at that point, smallest bound %.2e); A moves by "
          "%.1f %% of its range" % (B, S, float(drift.max()), float((drift / bound).max()), float(bound.min()), 100 * moved))
    assert bool((drift <= bound).all())
    assert moved >= 0.01
    assert float(traj[:, :, 2:].std(dim=-1).max()) == 0.0  # (the species no channel enters stay where they are)


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def test_the_statistics_of_the_shared_channel():
    """SharedChannel with euler at B=4, S=4096 (n = 16 384 trajectories), T=9 on the ragged grid, every trajectory with the same
    parameters and start: at the last point the sample means, variances and the cross-species covariance lie within 5 standard
    errors of the exact linear recursions (CM.shared_statistics: Var_j' = c^2 Var_j + (s^2 + s_j^2) h, Cov' = c^2 Cov + s^2 h), and
    the increment correlations between the channel combinations, consecutive steps and neighbouring trajectories are below
    5 / sqrt(n).  The key CM.STAT_KEY is fixed; tests/test_modelgen_channel_host.py runs the same figures on the CPU with the
    draws of tests/sde_ref.py under that key."""
    cls, B, S = CM.SharedChannel, CM.STAT_B, CM.STAT_S
    th = {k: torch.full((B, S), v) for k, v in dict(CM.BASES[cls], **CM.STAT_THETA).items()}
    cond = torch.tensor([float(CM.STAT_KEY[0]), float(CM.STAT_KEY[1])])[None, :].expand(B, 2)
    times = torch.tensor(CM.RAGGED)
    traj = SG._launch(cls, "euler", th, cond, times, torch.zeros(B, 4, len(CM.RAGGED)))["traj"].double().reshape(B * S, 4, -1)
    mean_se, var_se, cov_se, corrs, bound = CM.shared_statistics(traj[:, :2], times)
    for j in range(2):
        print("species %d: mean off by %.2f standard errors, variance by %.2f" % (j, mean_se[j], var_se[j]))
    print("covariance off by %.2f standard errors" % cov_se)
    for what, c in corrs.items():
        print("correlation between %s: %.4f (bound %.4f)" % (what, c, bound))
    assert all(abs(v) <= 5.0 for v in mean_se + var_se + [cov_se])
    for what, c in corrs.items():
        assert abs(c) <= bound, what


# ---- smaller cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["modeuler", "rk4"])
def test_two_time_points(solver):
    """T = 2: one interval (four sub-steps of it for ExpressionCLE)."""
    for cls in (CM.ExpressionCLE, CM.Channels8):
        B, S = SHAPES[1]
        pb = CM.problem(cls, B, S, times=[0.25, 0.75])
        r64, r32, quiet = _reference(cls, pb, solver)
        _precondition(cls, pb, r64, quiet, "%s %s T=2" % (cls.__name__, solver))
        SG._compare(_run(cls, solver, pb), r64, r32, "%s %s T=2" % (cls.__name__, solver))


@pytest.mark.parametrize("cls", [CM.ExpressionCLE, CM.Channels8], ids=lambda c: c.__name__)
def test_the_first_two_rows_alone_and_the_adjoint_twice(cls):
    """The first two rows of the B = 3 problem run as a B = 2 problem with the same key give the same forward bits (the counter
    holds b * S + s, not the launch's size); and the same launch twice gives the same g_theta bit for bit (no atomics)."""
    B, S = SHAPES[1]
    pb = CM.problem(cls, B, S)
    a, again = _run(cls, "rk4", pb), _run(cls, "rk4", pb)
    two = SG._launch(cls, "rk4", {n: v[:2] for n, v in pb["th"].items()}, pb["cond"][:2], pb["times"], pb["obs"][:2], pb["G"]["logp"][:2])
    for k in ("traj", "xpred", "logp"):
        assert torch.equal(two[k], a[k][:2]), k
        assert torch.equal(again[k], a[k]), k
    for n in a["g_theta"]:
        assert torch.equal(again["g_theta"][n], a["g_theta"][n]), n
        assert torch.equal(two["g_theta"][n], a["g_theta"][n][:2]), n
    for n in CM.NOISE_PARAMETERS[cls]:
        assert float(a["g_theta"][n].abs().max()) > 0.0, n


# ---- the C API --------------------------------------------------------------------------------------------------------------------
def test_the_c_api_declines_an_adaptive_solver():
    """dopri5 (and every adaptive id) on a key with channel noise: VIHDS_E_UNSUPPORTED, nothing queued; ops.OdeProblemSpec raises
    first.  hip.GENERATED_DIFFUSION has the key."""
    cls, (B, S) = CM.Channels8, SHAPES[0]
    pb = CM.problem(cls, B, S)
    key = SG._key(cls)
    assert key in hip.GENERATED_DIFFUSION and SG._key(CM.ConversionPair) in hip.GENERATED_DIFFUSION
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

    spec = ops.OdeProblemSpec(key, "rk4", row_of, th.shape[0], C=C)
    for solver in ["dopri5"] + [s for s in hip.ADAPTIVE_SOLVERS if s != "dopri5"]:
        with pytest.raises(NotImplementedError, match="process noise"):
            ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=C)
        p = spec.bind(B, S, T)
        p.solver = hip.SOLVERS[solver]
        assert fwd(p) == hip.E_UNSUPPORTED and "process noise" in L.vihds_last_error().decode(), solver
    assert float(logp.abs().max()) == 0.0 and float(traj.abs().max()) == 0.0  # (nothing was launched)
    assert fwd(spec.bind(B, S, T)) == 0 and float(traj.abs().max()) > 0.0


# ---- training: SharedChannel through the plugin surface ---------------------------------------------------------------------------
N_PLATE = 20


def _noisy_training(monkeypatch, B, S, **over):
    import models
    from vihds import synthetic

    cls = CM.SharedChannel  # (additive noise: the gradient is finite wherever the noise takes the state)
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        spec["params"]["constant"]["init"] = 1.0
        spec["params"]["global"].update({"a": ln(float(np.log(0.8)), 0.2), "s": ln(float(np.log(0.4)), 0.2),
                                         "s0": ln(float(np.log(0.3)), 0.2), "s1": ln(float(np.log(0.5)), 0.2)})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "shared_channel", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("shared_channel",))
    out = synthetic.build("shared_channel", B, S, solver="rk4", device=DEV, seed=3, **over)
    ode = out[4].decoder.ode_model
    assert isinstance(ode, cls) and ode.has_diffusion and ode.n_noise_channels == 3
    return out


def test_training_step_eager_and_replayed(monkeypatch, tmp_path):
    """One Training.step eagerly -- the loss and every updated parameter finite, the prior rows behind the shared and a private
    amplitude moved -- and the same step captured and replayed from the same key state: the same loss.  A second replay draws
    afresh: another loss, and the key state has advanced by two."""
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
        for name in ("s", "s1"):
            kb = [d.name for d in model.encoder.glob].index(name)
            assert not torch.equal(free_before[:, kb], model.encoder.global_free.detach()[:, kb]), name
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
