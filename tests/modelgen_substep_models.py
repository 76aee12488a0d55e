"""Models with `substeps = m` (vihds.modelgen: m steps of a fixed-grid scheme over each observation interval) for the tests:
subclasses of the forced, the implicit and the plate-reader test models that add the attribute and a key of their own.

The float64 yardstick of the GPU comparisons is written here, once, for the host and the GPU tests.  m sub-steps on `times`
are exactly the m = 1 scheme on the refined grid s_j, read at every m-th point; for a forced model the series on the refined
grid is the linear interpolant of the samples, which torch_problem's right-hand side already evaluates at any t.  Explicit
schemes: oracle.simulate on the refined grid with autograd through it.  beuler: modelgen_implicit_models.newton_step and
autograd_jacobian on the refined grid, the gradient by the implicit-function adjoint of modelgen_implicit_models.definition
restated so that only the observation points are scored."""
import torch

from oracle import vihds_oracle as O

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_likelihood_models as LM
from modelgen_models import PREC
from modelgen_noise_models import NOISE
from modelgen_piecewise_models import FIXED, TIMES  # noqa: F401  (for the tests)


class PrprForcedSub2(FM.PrprForced):
    model_key = "gen_prpr_constant_forced_sub2"
    substeps = 2


class PrprForcedSub4(FM.PrprForced):
    model_key = "gen_prpr_constant_forced_sub4"
    substeps = 4


class PrprImplicitSub4(IM.PrprImplicit):
    model_key = "gen_prpr_constant_implicit_sub4"
    substeps = 4


class DrImplicitSub4(IM.DrImplicit):
    model_key = "gen_dr_constant_implicit_sub4"
    substeps = 4


class PrprForcedImplicitSub2(IM.PrprForcedImplicit):
    model_key = "gen_prpr_constant_forced_implicit_sub2"
    substeps = 2


class FastBindingSub4(IM.FastBinding):
    model_key = "gen_fast_binding_sub4"
    newton_iterations = 6
    substeps = 4


class DenseEightSub8(IM.DenseEight):
    """The register and LDS worst case: eight species, every entry of the Jacobian, seven intermediate states."""
    model_key = "gen_dense_eight_sub8"
    substeps = 8


class PlateReaderSub3(LM.PlateReaderStudentT):
    """The plate reader with its own observation map, its own precision map and its own likelihood, at an odd m."""
    model_key = "gen_plate_reader_student_t_sub3"
    substeps = 3


# the class each one divides the intervals of: same definition, substeps = 1
PARENT = {PrprForcedSub2: FM.PrprForced, PrprForcedSub4: FM.PrprForced, PrprImplicitSub4: IM.PrprImplicit,
          DrImplicitSub4: IM.DrImplicit, PrprForcedImplicitSub2: IM.PrprForcedImplicit, FastBindingSub4: IM.FastBinding,
          DenseEightSub8: IM.DenseEight, PlateReaderSub3: LM.PlateReaderStudentT}
MODELS = list(PARENT)
STIFF = (FastBindingSub4,)  # beuler only: the explicit schemes blow up at its inputs
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS]

READER_BASE = {n: v for n, v in FM.READER_BASE.items()}
assert all(n in READER_BASE for n in NOISE)
_PROBLEMS = {}


def solvers_of(cls):
    """The fixed-grid solvers a test model takes."""
    if cls in STIFF:
        return ["beuler"]
    return list(FIXED) + (["beuler"] if cls.implicit else [])


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def problem(cls, B, S, times=None, **kw):
    """Inputs of one case (shared by the tests that use it; never modified): those of the class's m = 1 parent, from the
    module that defines it; the plate reader's are drawn here as modelgen_forcing_models.problem draws them."""
    parent = PARENT.get(cls, cls)
    if issubclass(parent, LM.PlateReaderStudentT):
        return _reader_problem(parent, B, S, TIMES if times is None else times)
    if parent.implicit:
        return IM.problem(parent, B, S, times=times, **kw)
    return FM.problem(parent, B, S, **({} if times is None else {"times": times}))


def _reader_problem(cls, B, S, times, seed=13):
    k = (cls, B, S, tuple(times), seed)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    assert sorted(READER_BASE) == sorted(slot_names(cls))
    th = {n: v * torch.exp(0.2 * rnd(B, S)) for n, v in READER_BASE.items()}
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    cond = torch.log1p(treatments)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        rhs, x0 = cls.torch_problem(th1, cond, None)
        xp = cls.torch_observe(O.simulate(rhs, x0, tt, "rk4"), th1, cond)
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": torch.zeros(B, 0, T, dtype=torch.float64), "treatments": treatments, "times": tt,
          "obs": obs, "W": {}, "B": B, "S": S, "T": T, "G": {"logp": rnd(B, S, 4)}}
    _PROBLEMS[k] = pb
    return pb


# ---- the definition in torch ---------------------------------------------------------------------------------------------------
def refined(times, m):
    """The grid of the sub-steps in the dtype of `times`: s_j = t_k + j (t_k+1 - t_k) / m; every m-th point is a point of
    `times` itself."""
    t = torch.as_tensor(times)
    j = torch.arange(m, dtype=t.dtype)
    inner = t[:-1, None] + j[None, :] * ((t[1:] - t[:-1]) / m)[:, None]
    return torch.cat([inner.reshape(-1), t[-1:]])


def hooks(cls, xs, th, cond, obs):
    """(trajectory rows [B,S,N(+4),T], x_predict, per-signal log-likelihood [B,S,4]) of the species xs at the observation
    points: the class's own maps where it has them (modelgen_forcing_models.forward states the same)."""
    if cls._observe_def is not None:
        xp = cls.torch_observe(xs, th, cond)
    else:
        xp = O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)
    if cls._precision_def is not None:
        prec = cls.torch_precision(xs, th, cond)
        full = torch.cat([xs, prec], dim=2)
    else:
        prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
        full = xs
    if cls._likelihood_def is not None:
        logp = cls.torch_log_likelihood(xp, obs, prec, th, cond).sum(3)
    else:
        logp = O.log_prob_observations(xp, obs, prec)
    return full, xp, logp


def _leaves(pb, dtype):
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    return {n: leaf(v) for n, v in pb["th"].items()}


def explicit_definition(cls, pb, solver, dtype, m=None):
    """An explicit scheme with m sub-steps (the class's own unless given): oracle.simulate on the refined grid, read at every
    m-th point, autograd for the gradient of sum(logp * G)."""
    m = int(cls.substeps) if m is None else m
    th = _leaves(pb, dtype)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    rhs, x0 = IM.torch_rhs(cls, th, cond, times)
    xs = O.simulate(rhs, x0, refined(times, m), solver)[..., ::m]
    full, xp, logp = hooks(cls, xs, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}}


def beuler_refined(cls, th, cond, times, m, newton=None, differentiable=False):
    """(every state of the refined grid [B,S,N,(T-1) m + 1], the refined grid, the largest last Newton increment relative to the
    state) of backward Euler with m sub-steps.  differentiable: autograd runs through the iterations."""
    rhs, x0 = IM.torch_rhs(cls, th, cond, times)
    fine = refined(times, m)
    newton = int(cls.newton_iterations) if newton is None else newton
    ys, y, worst = [x0], x0, 0.0
    with torch.enable_grad() if differentiable else torch.no_grad():
        for q in range(len(fine) - 1):
            if differentiable:
                y, d = IM.newton_step(rhs, fine[q + 1], fine[q + 1] - fine[q], y, newton,
                                      lambda f, t, z: IM.autograd_jacobian(f, t, z, create_graph=True))
            else:
                y, d = IM.newton_step(rhs, fine[q + 1], fine[q + 1] - fine[q], y, newton)
            dd, yy = d.detach(), y.detach()
            worst = max(worst, float((dd.abs().amax(-1) / yy.abs().amax(-1).clamp_min(1e-30)).max())
                        if bool(torch.isfinite(dd).all()) else float("inf"))
            ys.append(y)
    return torch.stack(ys, dim=3), fine, worst


def beuler_definition(cls, pb, dtype, m=None):
    """Backward Euler with m sub-steps in `dtype` and the gradient of sum(logp * G) by the implicit-function adjoint at the
    scheme's own iterates (modelgen_implicit_models.definition on the refined grid), with the one change that only the
    observation points are scored: dL/dy arrives at every m-th state of the refined grid and nowhere else."""
    m = int(cls.substeps) if m is None else m
    th = _leaves(pb, dtype)
    names = list(th)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    fine_xs, fine, last = beuler_refined(cls, th, cond, times, m)
    xs = fine_xs[..., ::m]
    N, F = fine_xs.shape[2], fine_xs.shape[3]
    Y = xs.detach().clone().requires_grad_(True)
    full, xp, logp = hooks(cls, Y, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    direct = torch.autograd.grad(loss, [Y] + [th[n] for n in names], allow_unused=True)
    gY = direct[0]
    g = {n: (torch.zeros_like(th[n]) if v is None else v.clone()) for n, v in zip(names, direct[1:])}
    rhs, x0 = IM.torch_rhs(cls, th, cond, times)
    eye = torch.eye(N, dtype=dtype)

    def add(outputs, seed):
        if not outputs.requires_grad:
            return
        for n, v in zip(names, torch.autograd.grad(outputs, [th[n] for n in names], grad_outputs=seed, allow_unused=True,
                                              retain_graph=True)):
            if v is not None:
                g[n] += v

    lam = gY[..., -1]
    for q in range(F - 2, -1, -1):
        t1, h = fine[q + 1], fine[q + 1] - fine[q]
        y1 = fine_xs[..., q + 1].detach()
        A = eye - h * IM.autograd_jacobian(rhs, t1, y1)
        mu = torch.linalg.solve(A.transpose(-1, -2), lam.unsqueeze(-1)).squeeze(-1)
        add(rhs(t1, y1), h * mu)
        lam = mu + gY[..., q // m] if q % m == 0 else mu
    add(x0, lam)
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "g_theta": g,
            "last_increment": last}


def definition(cls, pb, solver, dtype, m=None):
    return beuler_definition(cls, pb, dtype, m) if solver == "beuler" else explicit_definition(cls, pb, solver, dtype, m)


def beuler_by_autograd(cls, pb, newton, m=None):
    """float64: autograd through `newton` Newton iterations per sub-step -- what the restated adjoint must agree with once the
    iteration has converged."""
    m = int(cls.substeps) if m is None else m
    th = _leaves(pb, torch.float64)
    fine_xs, _, _ = beuler_refined(cls, th, pb["cond"], pb["times"], m, newton=newton, differentiable=True)
    _, _, logp = hooks(cls, fine_xs[..., ::m], th, pb["cond"], pb["obs"])
    (logp * pb["G"]["logp"]).sum().backward()
    return {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}
