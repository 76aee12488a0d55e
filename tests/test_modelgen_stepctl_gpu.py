"""GPU tests of `step_tolerance = (rtol, atol)` for generated models (ode_stepctl and ode_stepctl_vjp in the time loops of
ode_fwd_kernel and ode_bwd_kernel, csrc/vihds_ode_kernels.hpp; the rule of csrc/vihds_stepctl.hpp) against the float64
restatement of tests/modelgen_stepctl_models.py.

1. a loose tolerance (rtol 1e30): every count is 2 and every output equals the `substeps = 2` twin's bit for bit;
2. a tight one (rtol 0, atol 1e-30): every interval saturates, the row holds -M, everything equals the `substeps = M` twin's;
3. varying counts (a pulse of light, a jump, theta spread per sample): asserted first on the float64 definition alone -- three
   distinct counts among the first 64 trajectories, a saturated interval, no ratio of any test in [0.8, 1.25] -- then the
   kernel's counts equal the float64 counts exactly and states, x_predict, log-likelihood, loss and theta rows agree with the
   definition at those counts;
4. the same through beuler of order 1 and 2, and through one class with a forcing, a jump, missing observations and an
   observation map of its own;
5. modelgen.substep_counts reads the row back; the evaluation summaries of an own-precision model skip it.

Shapes: B=3, S=5 (one partly filled wavefront) and B=3, S=100 (300 trajectories: blocks that span data rows, tail lanes in the
last block), T=12 on a grid whose steps differ by a factor of six (the implicit cases: T=9, steps 0.1 .. 0.2).  Bounds: those of
`_compare` in tests/test_modelgen_substeps_gpu.py -- trajectory and x_predict 1e-5 per row, log-likelihood 1e-4, the loss within
max(1e-6, 8 x the float32 torch run's error), every theta row within max(1e-4, 8 x the float32 torch run of the same definition
at the same counts)."""
import ctypes

import pytest
import torch

from vihds import hip, modelgen, ops

from fixture_util import rel_err

import hip_util as H
import modelgen_stepctl_models as CM
from test_modelgen_substeps_gpu import _compare, _precondition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (3, 100)]
VARYING = [(CM.PulsedPrpr, "midpoint"), (CM.PulsedPrprFine, "rk4")]
COMBINED = [(CM.PrprImplicitCtl, "beuler"), (CM.PrprSdirkCtl, "beuler"), (CM.CombinedCtl, "midpoint")]
_KEYS, _REFS = {}, {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
        assert hip.GENERATED_SUBSTEPS[cls.model_key] == cls.substeps
        if cls.step_tolerance is not None:
            assert hip.GENERATED_STEP_CONTROL[cls.model_key] == (cls.substeps,) + tuple(float(v) for v in cls.step_tolerance)
        else:
            assert cls.model_key not in hip.GENERATED_STEP_CONTROL
    return _KEYS[cls]


def _rows(cls):
    return len(cls.species) + (4 if cls._precision_def is not None else 0) + (1 if cls.step_tolerance is not None else 0)


def _kernel(cls, pb, solver):
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == CM.slot_names(cls)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=pb["cond"].shape[1])
    assert spec.n_states == _rows(cls) and spec.n_species == len(cls.species)
    assert spec.n_precision_rows == (4 if cls._precision_def is not None else 0)
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"]), None, None)
    assert traj.shape[1] == _rows(cls)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {"traj": H.view_bsnt(traj).detach().cpu(), "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "loss": loss.detach().cpu(), "buffer": traj.detach(),
            "xbuffer": xpred.detach(),
            "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots}}


def _reference(cls, pb, solver):
    k = (cls, id(pb), solver)
    if k not in _REFS:
        r64 = CM.definition(cls, pb, solver, torch.float64)
        _REFS[k] = (r64, CM.definition(cls, pb, solver, torch.float32, codes=r64["codes"]))
    return _REFS[k]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver,times", CM.DEGENERATE, ids=lambda v: v if isinstance(v, str) else (v.__name__ if isinstance(v, type) else "T%d_%g" % (len(v), v[-1])))
def test_a_degenerate_tolerance_is_the_fixed_count_bit_for_bit(cls, solver, times, shape):
    """Cases 1 and 2.  Loose: every interval passes at the first test, the row holds +2.  Tight: no interval passes, the row
    holds -M -- asserted from the float64 definition too, on samples whose rungs float32 resolves (modelgen_stepctl_models.
    DEGENERATE says which ceilings that leaves the fourth-order scheme).  Species rows, x_predict, log-likelihood and loss equal
    those of the twin class with that fixed count bit for bit.  The theta rows do not, for a reason in the compiled code
    (profiles/LOG.md: the compiler contracts a * b + c into fused operations at other places of the adjoint once the count is a
    run-time value -- the two adjoints differ in their numbers of v_fma_f32 / v_mul_f32 / v_add_f32, as the fixed twins of
    different counts do among themselves); both are held to the bounds of case 3 against the float64 definition at those counts
    instead."""
    B, S = shape
    twin = CM.FIXED_TWIN[cls]
    pb = CM.problem(cls, B, S, solver, times=times)
    got, want = _kernel(cls, pb, solver), _kernel(twin, pb, solver)
    N = len(cls.species)
    expect = 2.0 if cls.step_tolerance == CM.LOOSE else -float(cls.substeps)
    assert abs(expect) == twin.substeps
    codes64 = CM.ladder(cls, pb["th"], pb["cond"], pb["times"], solver)[0]
    assert bool((codes64[1:] == expect).all()) and bool((codes64[0] == 0).all())
    row = got["traj"][:, :, N, :]
    assert bool((row[..., 0] == 0).all()) and bool((row[..., 1:] == expect).all()), row.unique().tolist()
    assert got["traj"].shape[2] == N + 1 and want["traj"].shape[2] == N
    assert torch.equal(got["traj"][:, :, :N], want["traj"])
    for k in ("xpred", "logp", "loss"):
        assert torch.equal(got[k], want[k]), k
    k = (cls, solver, shape, len(times))
    if k not in _REFS:
        _REFS[k] = tuple(CM.definition(cls, pb, solver, dt, codes=codes64) for dt in (torch.float64, torch.float32))
    r64, r32 = _REFS[k]
    label = "%s %s %dx%d" % (cls.__name__, solver, B, S)
    for who, out in (("", got), (" (the twin)", want)):  # (case 3's bound on the theta rows)
        for n, g in r64["g_theta"].items():
            if float(g.abs().max()) == 0.0:
                assert float(out["g_theta"][n].abs().max()) == 0.0, n
                continue
            e, bound = rel_err(out["g_theta"][n], g), max(1e-4, 8 * rel_err(r32["g_theta"][n], g))
            print("%s%s g_theta[%s]: %.2e (bound %.2e)" % (label, who, n, e, bound))
            assert e <= bound, (label, who, n)
    worst = max(float((got["g_theta"][n] - want["g_theta"][n]).abs().max() / want["g_theta"][n].abs().max().clamp_min(1e-30))
                for n in got["g_theta"])
    print("%s: theta rows against the twin's, largest difference relative to the row's largest entry %.2e" % (label, worst))
    counts, saturated = modelgen.substep_counts(got["buffer"], cls)
    assert counts.dtype == torch.int32 and saturated.dtype == torch.bool and tuple(counts.shape) == (pb["T"] - 1, B, S)
    assert bool((counts == twin.substeps).all()) and bool((saturated == (expect < 0)).all())


def _varying(cls, solver, shape, distinct):
    B, S = shape
    pb = CM.problem(cls, B, S, solver)
    r64, r32 = _reference(cls, pb, solver)
    label = "%s M=%d %s %dx%d" % (cls.__name__, cls.substeps, solver, B, S)
    _precondition(r64, label, solver)
    # the conditions, on the float64 definition alone
    codes = r64["codes"][1:]  # [T-1,B,S]
    flat = codes.reshape(codes.shape[0], -1)
    first = sorted(set(flat[:, :64].abs().reshape(-1).tolist()))
    hist = {v: int((codes == v).sum()) for v in sorted(set(codes.reshape(-1).tolist()))}
    print("%s: counts %s; among the first 64 trajectories %s" % (label, hist, first))
    assert len(first) >= distinct, first
    assert bool((codes < 0).any()), "no interval saturates"
    for k, c, r, looked in r64["looked_at"]:
        inside = looked & (r >= CM.BAND[0]) & (r <= CM.BAND[1])
        assert not bool(inside.any()), (k, c, r[inside].tolist())
        assert bool(torch.isfinite(r[looked]).all())
    got = _kernel(cls, pb, solver)
    N = _rows(cls) - 1
    assert torch.equal(got["traj"][:, :, N, :].double(), r64["codes"].permute(1, 2, 0)), "the kernel chose other counts"
    counts, saturated = modelgen.substep_counts(got["buffer"], cls)
    assert torch.equal(counts.cpu().double(), codes.abs()) and torch.equal(saturated.cpu(), codes < 0)
    _compare(got, r64, r32, label)
    return got, pb


@pytest.mark.parametrize("cls,solver", VARYING, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_varying_counts_against_the_definition_in_float64(cls, solver):
    """Case 3, at B=3, S=100: one wavefront holds trajectories with three different counts."""
    _varying(cls, solver, SHAPES[1], 3)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls,solver", COMBINED, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_implicit_schemes_and_the_combined_class(cls, solver, shape):
    """Case 4: backward Euler, the two-stage SDIRK, and a forcing + a jump + missing observations + an observation map of the
    model's own in one class.  Their ceiling is 4: both counts of the ladder occur among the first 64 trajectories, and some
    interval saturates."""
    _varying(cls, solver, shape, 2)


def test_summaries_of_an_own_precision_model_skip_the_count_row():
    """Case 5: ReaderCtl stores species | four precision rows | the count row.  The importance-weighted summaries with the
    species count of its spec equal, bit for bit, those of the same buffer without the last row (the uncontrolled layout)."""
    cls, solver = CM.ReaderCtl, "rk4"
    B, S = SHAPES[1]
    import modelgen_jump_models as JM
    pb = JM.problem(JM.PlateReaderDiluted, B, S)
    got = _kernel(cls, pb, solver)
    buf = got["buffer"]
    N = len(cls.species)
    assert buf.shape[1] == N + 5
    counts, saturated = modelgen.substep_counts(buf, cls)
    assert int(counts.min()) >= 2 and int(counts.max()) <= cls.substeps
    assert torch.equal(buf[1:, -1], torch.where(saturated, -counts.float(), counts.float())) and bool((buf[0, -1] == 0).all())
    counts_b, saturated_b = modelgen.substep_counts(H.view_bsnt(buf), cls)  # (the solution's layout [B,S,rows,T])
    assert torch.equal(counts_b, counts) and torch.equal(saturated_b, saturated)
    gen = torch.Generator().manual_seed(5)
    log_w = torch.randn(B, S, generator=gen).to(DEV)
    lse = torch.logsumexp(log_w, dim=1)
    a = ops.iw_summaries(log_w, lse, buf, got["xbuffer"], N)
    b = ops.iw_summaries(log_w, lse, buf[:, :-1].contiguous(), got["xbuffer"], N)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_the_c_api_declines_the_modeuler_family_and_the_adaptive_solvers():
    """vihds_ode_fwd and vihds_ode_bwd with modeuler, modeulerwhile and dopri5 on a model with step control:
    VIHDS_E_UNSUPPORTED with a message, nothing queued; ops.OdeProblemSpec declines the same by name."""
    B, S, T = 3, 5, len(CM.TIMES)
    L = hip.lib()
    cls = CM.PulsedPrpr
    key = _key(cls)
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    C = len(cls.forcings) * T
    times = torch.tensor(CM.TIMES, device=DEV)
    th = torch.full((len(slots), B, S), 0.5, device=DEV)
    N = L.vihds_model_n_states(hip.MODELS[key])
    assert N == len(cls.species) + 1 and L.vihds_model_n_species(hip.MODELS[key]) == len(cls.species)
    for solver, word in (("modeuler", "step control"), ("modeulerwhile", "step control"), ("dopri5", "substeps > 1")):
        prob = ops.OdeProblemSpec(key, "rk4", row_of, len(slots), C=C).bind(B, S, T)
        prob.solver = hip.SOLVERS[solver]
        cond, obs = torch.ones((B, C), device=DEV), torch.zeros((B, 4, T), device=DEV)
        traj, xpred = torch.zeros((T, N, B, S), device=DEV), torch.zeros((T, 4, B, S), device=DEV)
        logp, g = torch.zeros((4, B, S), device=DEV), torch.zeros_like(th)
        rc = L.vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and word in L.vihds_last_error().decode(), solver
        rc = L.vihds_ode_bwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                             hip.ptr(traj), None, None, hip.ptr(logp), hip.ptr(g), None, None, hip.current_stream())
        assert rc == hip.E_UNSUPPORTED and word in L.vihds_last_error().decode(), solver
        torch.cuda.synchronize()
        assert float(traj.abs().max()) == 0.0 and float(g.abs().max()) == 0.0  # (nothing was launched)
        with pytest.raises(NotImplementedError, match="step control|substeps = 8"):
            ops.OdeProblemSpec(key, solver, row_of, len(slots), C=C)


def test_a_forward_without_a_trajectory_buffer():
    """vihds_ode_fwd with traj == NULL integrates as it does with one (x_predict and the log-likelihood are the same bits) and
    stores no counts."""
    B, S = SHAPES[0]
    cls, solver = CM.PulsedPrpr, "midpoint"
    pb = CM.problem(cls, B, S, solver)
    got = _kernel(cls, pb, solver)
    key = _key(cls)
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    f32 = lambda v: v.float().to(DEV).contiguous()  # noqa: E731
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).contiguous()
    T = pb["T"]
    prob = ops.OdeProblemSpec(key, solver, row_of, len(slots), C=pb["cond"].shape[1]).bind(B, S, T)
    cond, times, obs = f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"])
    xpred, logp = torch.zeros((T, 4, B, S), device=DEV), torch.zeros((4, B, S), device=DEV)
    rc = hip.lib().vihds_ode_fwd(ctypes.byref(prob), hip.ptr(th), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), None,
                                 None, hip.ptr(xpred), hip.ptr(logp), hip.current_stream())
    hip.check(rc, "vihds_ode_fwd")
    torch.cuda.synchronize()
    assert torch.equal(H.view_bsnt(xpred).cpu(), got["xpred"]) and torch.equal(H.view_bs4(logp).cpu(), got["logp"])
