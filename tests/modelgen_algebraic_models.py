"""Models with algebraic variables (`algebraic`, `constraint`, `algebraic_start` of vihds.modelgen: a fast reaction held at its
equilibrium) for the tests: BindingQss, the quasi-steady-state reduction of modelgen_implicit_models.FastBinding -- the totals
A + C and B + C and the reporter are the states, the complex C solves (At - C)(Bt - C) = Kd C --; BindingClosed, the same model
with C in closed form and no algebraic variable (the twin that pins the adjoint to plain reverse mode); Competing, two species
that compete for one partner (two unknowns, a dense 2 x 2 pattern, no closed form); ChainFour, a complex that binds three
further partners in turn (four unknowns, the cap; a lower-bidiagonal pattern: the compile-time-pattern case and the register
worst case); BindingCombined, BindingQss with two sub-steps, a dilution jump and a forcing read by the constraint.

The float64 yardstick is written here, once, for the host and the GPU tests: the explicit scheme interval by interval
(modelgen_jump_models.explicit_states: sub-steps and jumps included) on the right-hand side that solves the constraint by the
iteration exactly as include/vihds_hip.h defines it -- algebraic_iterations Newton steps from algebraic_start, autograd
Jacobians, torch.linalg.solve (pivoted) --, the implicit-function gradient (nothing differentiated through the iteration), and
`last_increment`, the largest last Newton increment relative to |z| at the trajectory's states.

Inputs: the draws of FAST_DRAWS (Kd = koff / kon = 0.125 exp(sqrt 2 eps)), every normal clipped at 3 sd; production ratios 0.5
and 0.3 keep the totals apart, so the quadratic has no near-double root (Newton converges slowly at one)."""
import math

import torch

from vihds.modelgen import GeneratedOdeModel, sqrt
from vihds.precisions import ConstantPrecisions

import modelgen_forcing_models as FM
import modelgen_jump_models as JM
import modelgen_substep_models as SM
from modelgen_implicit_models import FAST_DRAWS
from modelgen_models import PREC
from modelgen_piecewise_models import TIMES  # noqa: F401  (for the tests)


class BindingQss(GeneratedOdeModel):
    """FastBinding with the binding at equilibrium: At = A + C, Bt = B + C and R are the states, C the algebraic variable."""
    model_key = "gen_binding_qss"
    species = ["At", "Bt", "R"]
    parameters = ["kon", "koff", "prod", "deg", "a", "gain"]
    n_conditions = 0
    algebraic = ["C"]
    algebraic_iterations = 6
    Y0 = [0.5, 0.2, 0.0]

    def __init__(self, config):
        super(BindingQss, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"Kd": th.koff / th.kon, "prod": th.prod, "deg": th.deg, "a": th.a, "gain": th.gain}

    def initial_state(self, th, c):
        return list(self.Y0)

    def algebraic_start(self, y, p, c):
        return [y[0] * y[1] / (y[0] + y[1] + p.Kd)]

    def constraint(self, y, z, p, c):
        return [(y[0] - z[0]) * (y[1] - z[0]) - p.Kd * z[0]]

    def rhs(self, t, y, p, c):
        C = self.algebraic.C
        return [p.prod - p.deg * y[0], 0.5 * p.prod - p.deg * y[1], p.a * C * C / (0.25 + C * C) - p.deg * y[2]]

    def observe(self, y, p, c):
        return [y[0], y[1], p.gain * self.algebraic.C, y[2]]


def closed_form(At, Bt, Kd):
    """The smaller root of (At - C)(Bt - C) = Kd C, in the form without cancellation."""
    s = At + Bt + Kd
    return 2.0 * At * Bt / (s + sqrt(s * s - 4.0 * At * Bt))


class BindingClosed(GeneratedOdeModel):
    """BindingQss with C written in closed form: no algebraic variable, plain reverse mode."""
    model_key = "gen_binding_closed"
    species = ["At", "Bt", "R"]
    parameters = ["kon", "koff", "prod", "deg", "a", "gain"]
    n_conditions = 0
    Y0 = BindingQss.Y0

    def __init__(self, config):
        super(BindingClosed, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    prepare = BindingQss.prepare
    initial_state = BindingQss.initial_state

    def rhs(self, t, y, p, c):
        C = closed_form(y[0], y[1], p.Kd)
        return [p.prod - p.deg * y[0], 0.5 * p.prod - p.deg * y[1], p.a * C * C / (0.25 + C * C) - p.deg * y[2]]

    def observe(self, y, p, c):
        return [y[0], y[1], p.gain * closed_form(y[0], y[1], p.Kd), y[2]]


class Competing(GeneratedOdeModel):
    """A binds B into C1 and D into C2: (At - C1 - C2)(Bt - C1) = K1 C1 and (At - C1 - C2)(Dt - C2) = K2 C2."""
    model_key = "gen_competing_qss"
    species = ["At", "Bt", "Dt", "R"]
    parameters = ["K1", "K2", "prod", "deg", "a", "gain"]
    n_conditions = 0
    algebraic = ["C1", "C2"]
    algebraic_iterations = 8
    Y0 = [0.5, 0.2, 0.1, 0.0]

    def __init__(self, config):
        super(Competing, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"K1": th.K1, "K2": th.K2, "prod": th.prod, "deg": th.deg, "a": th.a, "gain": th.gain}

    def initial_state(self, th, c):
        return list(self.Y0)

    def algebraic_start(self, y, p, c):
        At, Bt, Dt = y[0], y[1], y[2]
        return [At * Bt / (At + Bt + Dt + p.K1), At * Dt / (At + Bt + Dt + p.K2)]

    def constraint(self, y, z, p, c):
        free = y[0] - z[0] - z[1]
        return [free * (y[1] - z[0]) - p.K1 * z[0], free * (y[2] - z[1]) - p.K2 * z[1]]

    def rhs(self, t, y, p, c):
        C1 = self.algebraic.C1
        return [p.prod - p.deg * y[0], 0.5 * p.prod - p.deg * y[1], 0.3 * p.prod - p.deg * y[2],
                p.a * C1 * C1 / (0.25 + C1 * C1) - p.deg * y[3]]

    def observe(self, y, p, c):
        return [y[0], p.gain * self.algebraic.C1, p.gain * self.algebraic.C2, y[3]]


class ChainFour(GeneratedOdeModel):
    """A complex that grows: A binds B into C1, C1 binds D1 into C2, C2 binds D2 into C3, C3 binds D3 into C4 (Ck counts every
    complex that holds at least k partners).  Residual k reads Ck and Ck-1 only: a lower-bidiagonal dg/dz, 7 of 16 entries."""
    model_key = "gen_chain_four_qss"
    species = ["At", "Bt", "D1", "D2", "D3", "R"]
    parameters = ["K1", "K2", "K3", "K4", "prod", "deg", "a", "gain"]
    n_conditions = 0
    algebraic = ["C1", "C2", "C3", "C4"]
    algebraic_iterations = 8
    Y0 = [0.5, 0.2, 0.12, 0.08, 0.05, 0.0]
    RATIOS = [1.0, 0.5, 0.3, 0.2, 0.12]

    def __init__(self, config):
        super(ChainFour, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"K1": th.K1, "K2": th.K2, "K3": th.K3, "K4": th.K4, "prod": th.prod, "deg": th.deg, "a": th.a, "gain": th.gain}

    def initial_state(self, th, c):
        return list(self.Y0)

    def algebraic_start(self, y, p, c):
        K, out, holder = [p.K1, p.K2, p.K3, p.K4], [], y[0]
        for k in range(4):
            holder = holder * y[k + 1] / (holder + y[k + 1] + K[k])
            out.append(holder)
        return out

    def constraint(self, y, z, p, c):
        K, holders = [p.K1, p.K2, p.K3, p.K4], [y[0], z[0], z[1], z[2]]
        return [(holders[k] - z[k]) * (y[k + 1] - z[k]) - K[k] * z[k] for k in range(4)]

    def rhs(self, t, y, p, c):
        C4 = self.algebraic.C4
        return [r * p.prod - p.deg * y[k] for k, r in enumerate(self.RATIOS)] + [p.a * C4 / (0.05 + C4) - p.deg * y[5]]

    def observe(self, y, p, c):
        z = self.algebraic
        return [y[0], p.gain * (z.C1 - z.C2), p.gain * (z.C2 - z.C3) + z.C4, y[5]]


class BindingCombined(BindingQss):
    """BindingQss with everything that must combine: two sub-steps per interval, a dilution at the row's events (the forcing
    `keep`), and a dissociation constant that follows a logged temperature (the forcing `temp`, read by the constraint and by
    algebraic_start: the interpolant in rhs, the sample in observe)."""
    model_key = "gen_binding_qss_combined"
    forcings = ["temp", "keep"]
    substeps = 2

    def algebraic_start(self, y, p, c):
        return [y[0] * y[1] / (y[0] + y[1] + p.Kd * self.forcing.temp)]

    def constraint(self, y, z, p, c):
        return [(y[0] - z[0]) * (y[1] - z[0]) - p.Kd * self.forcing.temp * z[0]]

    def jump(self, y, p, c):
        keep = self.forcing.keep
        return [y[0] * keep, y[1] * keep, y[2]]


MODELS = [BindingQss, Competing, ChainFour, BindingCombined]  # the classes with algebraic variables
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS + [BindingClosed]]
SOLVERS = ("modeuler", "modeulerwhile", "euler", "midpoint", "rk4")  # the fixed-grid explicit schemes

# ---- inputs of the numeric tests ------------------------------------------------------------------------------------------------
_NARROW = {"prod": (1.0, 0.3), "a": (1.0, 0.3), "deg": (0.3, 0.3), "gain": (1.2, 0.2)}
_PRECS = {n: FAST_DRAWS[n] for n in PREC}
DRAWS = {
    BindingQss: FAST_DRAWS, BindingClosed: FAST_DRAWS, BindingCombined: FAST_DRAWS,
    Competing: dict(_NARROW, K1=(0.125, math.sqrt(2.0)), K2=(0.3, math.sqrt(2.0)), **_PRECS),
    ChainFour: dict(_NARROW, K1=(0.125, 0.5), K2=(0.2, 0.5), K3=(0.2, 0.5), K4=(0.15, 0.5), **_PRECS),
}
CLIP = 3.0  # every normal draw is clipped at 3 sd
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + list(PREC)


def series_of(cls, B, times):
    """The forcing samples of a class [B, K, T], in the order of cls.forcings: a smooth temperature factor 0.5 .. 1.5 with a
    phase per row, and the dilution schedule of modelgen_jump_models (the rows differ)."""
    T = len(times)
    named = {"temp": FM.smooth_series(B, times), "keep": JM.schedule(B, T)[0]}
    return torch.stack([named[n] for n in cls.forcings], dim=1) if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)


def problem(cls, B, S, times=TIMES, seed=29):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, the wide cond, times,
    observations (the first sample's rk4 prediction under the definition with 5 % noise) and an upstream gradient for the
    log-likelihood.  BindingClosed takes the inputs of BindingQss."""
    cls_in = BindingQss if cls is BindingClosed else cls
    k = (cls_in, B, S, tuple(times), seed)
    if k not in _PROBLEMS:
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
        tt = torch.tensor(list(times), dtype=torch.float64)
        T = tt.shape[0]
        assert sorted(slot_names(cls_in)) == sorted(DRAWS[cls_in])
        th = {n: m * torch.exp(sd * rnd(B, S).clamp(-CLIP, CLIP)) for n, (m, sd) in DRAWS[cls_in].items()}
        series = series_of(cls_in, B, tt)
        cond = FM.wide_cond(torch.zeros(B, 0, dtype=torch.float64), series)
        with torch.no_grad():
            th1 = {n: v[:, :1] for n, v in th.items()}
            xs = JM.explicit_states(cls_in, th1, cond, tt, "rk4")
            xp = SM.hooks(cls_in, xs, th1, cond, torch.zeros(B, 4, T, dtype=torch.float64))[1]
            obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
        _PROBLEMS[k] = {"th": th, "cond": cond, "series": series, "times": tt, "obs": obs, "W": {}, "B": B, "S": S, "T": T,
                        "G": {"logp": rnd(B, S, 4)}}
    return _PROBLEMS[k]


# ---- the definition in torch ----------------------------------------------------------------------------------------------------
def last_increment(cls, xs, th, cond):
    """The largest last Newton increment relative to |z| of the class's iteration at the states xs [B,S,N,T] (a forcing is the
    sample of the time point); 0.0 for a class without algebraic variables."""
    if not cls.algebraic:
        return 0.0
    worst = 0.0
    series = cond[:, cond.shape[1] - len(cls.forcings) * xs.shape[3]:].reshape(cond.shape[0], len(cls.forcings), xs.shape[3])
    with torch.no_grad():
        for k in range(xs.shape[3]):
            forcing = [series[:, j, k, None].to(xs.dtype) for j in range(len(cls.forcings))] or None
            worst = max(worst, cls.torch_algebraic(xs[..., k].detach(), th, cond, forcing=forcing, return_increment=True)[1])
    return worst


def definition(cls, pb, solver, dtype):
    """The explicit scheme `solver` in `dtype` on the right-hand side that solves the constraint by the defined iteration, the
    class's hooks, and the gradient of sum(logp * G) with respect to theta by autograd, which meets the implicit-function
    derivative at every solve (the iteration itself is not differentiated)."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    xs = JM.explicit_states(cls, th, cond, times, solver)
    full, xp, logp = SM.hooks(cls, xs, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}, "g_w": [],
            "last_increment": last_increment(cls, xs.detach(), {n: v.detach() for n, v in th.items()}, cond)}


# ---- the unknowns by hand (independent of vihds.modelgen's torch restatement) ----------------------------------------------------
def binding_root(At, Bt, Kd):
    """The root of BindingQss's constraint in float64."""
    s = At + Bt + Kd
    return 2.0 * At * Bt / (s + torch.sqrt(s * s - 4.0 * At * Bt))


def competing_newton(At, Bt, Dt, K1, K2, iterations):
    """Competing's iteration written out: the analytic 2 x 2 Jacobian, Cramer's rule.  Returns (C1, C2, the smallest |pivot| of
    an elimination without pivoting, i.e. of dg1/dC1)."""
    C1, C2 = At * Bt / (At + Bt + Dt + K1), At * Dt / (At + Bt + Dt + K2)
    pivot = torch.full_like(At, float("inf"))
    for _ in range(iterations):
        free = At - C1 - C2
        g1, g2 = free * (Bt - C1) - K1 * C1, free * (Dt - C2) - K2 * C2
        a11, a12 = -(Bt - C1) - free - K1, -(Bt - C1)
        a21, a22 = -(Dt - C2), -(Dt - C2) - free - K2
        det = a11 * a22 - a12 * a21
        C1, C2 = C1 - (g1 * a22 - a12 * g2) / det, C2 - (a11 * g2 - a21 * g1) / det
        pivot = torch.minimum(pivot, a11.abs())
    return C1, C2, pivot
