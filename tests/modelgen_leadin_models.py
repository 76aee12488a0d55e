"""Models with a start map (`start(self, y, p, c)`) and / or a lead-in phase (`lead_in`, `lead_in_steps`) of vihds.modelgen for
the tests: the prpr restatement started from the steady state of its pre-induction system (ratios of clamped rates, a where on
a treatment, a parameter that only start reads), the same with an unscored hour before the first read during which the inducer
is absent, the forced prpr restatement with a lead-in (its forcing holds the first sample), the stiff binding model with three
backward-Euler steps before the first read, a model that combines substeps, jump, start and lead_in, a lead-in of one step (no
LDS rows) and seven species with eight steps (49 of the 56 rows).

The float64 yardstick of the GPU comparisons is written here, once, for the host and the GPU tests.  It is the plain scheme on
the time grid with lead_in_times prepended and the forcing samples padded with u_0: it starts from
torch_start(initial_state) (torch_problem's x0), takes the n lead-in steps -- modeuler with the fixed step hl, no sub-steps,
no jump --, drops those n points and goes on as modelgen_jump_models' definition does (sub-steps, torch_jump between the
intervals).  Explicit schemes: the oracle's step functions, gradients by autograd.  beuler: modelgen_implicit_models.newton_step
and the implicit-function adjoint at the scheme's own iterates, lead-in steps included.  `start=False` / `lead=False` give the
definition with the hook or the phase removed: what a tree that ignores the attribute computes."""
import numpy as np
import torch

from vihds import modelgen as G
from vihds.modelgen import GeneratedOdeModel, where
from vihds.precisions import ConstantPrecisions

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_substep_models as SM
from modelgen_models import PREC, PrprRestated
from modelgen_piecewise_models import TIMES  # noqa: F401  (for the tests)

INDUCED_ABOVE = 0.6  # the treatment above which a well was pre-induced (the rows' treatments are 0.3, 1.0, 1.7)


class PrprSteady(PrprRestated):
    """PrprRestated whose pre-induced wells start from the steady state of the pre-induction system: RFP, YFP and CFP at
    `pre` x production / (degradation + dilution), ratios of the clamped rates; the other wells from their initial state.
    `pre` is read by start alone."""
    model_key = "gen_prpr_constant_steady"
    parameters = PrprRestated.parameter_names + ["pre"]
    n_conditions = 1

    def prepare(self, th, c):
        p = PrprRestated.prepare(self, th, c)
        p["pre"] = th.pre
        return p

    def start(self, y, p, c):
        x, rfp, yfp, cfp, f530, f480 = y
        induced = c[0] > INDUCED_ABOVE
        return [x,
                where(induced, p.pre * p.rc / (p.drfp + p.r), rfp),
                where(induced, p.pre * p.rc * p.aYFP / (p.dyfp + p.r), yfp),
                where(induced, p.pre * p.rc * p.aCFP / (p.dcfp + p.r), cfp),
                f530, f480]


class PrprSteadyLead(PrprSteady):
    """PrprSteady inoculated an hour before the first read: four steps over [-1, 0] in which the inducer (the treatment, which
    scales YFP production) is absent."""
    model_key = "gen_prpr_constant_steady_lead"
    lead_in = 1.0
    lead_in_steps = 4

    def rhs(self, t, y, p, c):
        return FM._prpr_rhs(t, y, p, where(t < 0.0, 0.0, c[0]))


class PrprForcedLead(FM.PrprForced):
    """PrprForced with two steps over the 0.75 before the first read: the light holds its first sample there."""
    model_key = "gen_prpr_constant_forced_lead"
    lead_in = 0.75
    lead_in_steps = 2


class FastBindingLead(IM.FastBinding):
    """The stiff binding model with three backward-Euler steps over the 0.5 before the first read."""
    model_key = "gen_fast_binding_lead"
    newton_iterations = 6
    lead_in = 0.5
    lead_in_steps = 3


class PrprEverything(JM.PrprDiluted):
    """substeps, jump, start and lead_in together, on forcings: PrprDiluted with two sub-steps, started from an RFP level set
    by the first light sample and run for three steps over the 0.6 before the first read."""
    model_key = "gen_prpr_constant_everything"
    substeps = 2
    lead_in = 0.6
    lead_in_steps = 3

    def start(self, y, p, c):
        x, rfp, yfp, cfp, f530, f480 = y
        return [x, rfp + self.forcing.light * p.rc / (p.drfp + p.r), yfp, cfp, f530, f480]


class PrprLeadOne(PrprRestated):
    """A lead-in of one step: the adjoint keeps no intermediate state and declares no LDS."""
    model_key = "gen_prpr_constant_lead_one"
    lead_in = 0.5
    lead_in_steps = 1


class SevenLead(GeneratedOdeModel):
    """Seven species coupled through their total (modelgen_implicit_models.DenseEight with one fewer) and eight lead-in steps:
    49 rows of LDS, near the cap of 56; implicit, so that backward Euler's adjoint reads them too."""
    model_key = "gen_seven_lead"
    species = ["OD", "RFP", "YFP", "CFP", "F530", "F480", "U"]
    parameters = ["a", "b", "k", "init_x"]
    n_conditions = 0
    observe_kind = "default"
    implicit = True
    lead_in = 0.4
    lead_in_steps = 8

    def __init__(self, config):
        super(SevenLead, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"a": th.a, "b": th.b, "k": th.k}

    def initial_state(self, th, c):
        return [(1.0 + 0.1 * j) * th.init_x for j in range(7)]

    def rhs(self, t, y, p, c):
        total = y[0] + y[1] + y[2] + y[3] + y[4] + y[5] + y[6]
        return [p.a * (0.2 * (j + 1) - y[j]) - p.b * y[j] * total / (1.0 + total) + p.k * y[(j + 1) % 7] * y[(j + 3) % 7]
                for j in range(7)]


MODELS = [PrprSteady, PrprSteadyLead, PrprForcedLead, FastBindingLead, PrprEverything, PrprLeadOne, SevenLead]
STIFF = (FastBindingLead,)  # beuler only: the explicit schemes blow up at its inputs
START_ONLY = {PrprSteady: "pre", PrprSteadyLead: "pre"}  # the parameter that only start reads
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS]

BASES = {PrprSteady: dict(FM.PRPR_BASE, pre=0.7), PrprSteadyLead: dict(FM.PRPR_BASE, pre=0.7), PrprForcedLead: FM.PRPR_BASE,
         PrprEverything: dict(FM.PRPR_BASE, bolus=0.5), PrprLeadOne: FM.PRPR_BASE, SevenLead: IM.DENSE_BASE}
_PROBLEMS = {}


def solvers_of(cls):
    """The solvers the GPU tests run a model with: beuler alone for the stiff one; modeuler (its fixed step is hl in the
    lead-in), midpoint and rk4 for the others, beuler too for the implicit one."""
    if cls in STIFF:
        return ["beuler"]
    return ["modeuler", "midpoint", "rk4"] + (["beuler"] if cls.implicit else [])


def grid_of(cls):
    """SevenLead has a growing mode: the grid of the implicit tests (steps 0.1 .. 0.2), on which Newton's iteration converges."""
    return IM.GRID if cls is SevenLead else TIMES


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def lead_steps(cls):
    return int(cls.lead_in_steps) if cls.lead_in > 0 else 0


def lead_step_size(cls, t0):
    """hl as the kernels form it in float32: (t_0 - tl) * (1.f / n) -- modeuler's fixed step in the lead-in."""
    t0 = np.float32(t0)
    tl = np.float32(t0 - np.float32(cls.lead_in))
    return float(np.float32(np.float32(t0 - tl) * np.float32(np.float32(1.0) / np.float32(lead_steps(cls)))))


# ---- the definition in torch ---------------------------------------------------------------------------------------------------
def extended(cls, cond, times):
    """(lead_in_times prepended to `times`, the rows of cond with every forcing series padded with its first sample) in the
    dtype of `times`: the grid and the inputs on which the plain scheme is the definition."""
    n = lead_steps(cls)
    if not n:
        return times, cond
    lead = torch.as_tensor(G.lead_in_times(cls, float(times[0]))[:-1].astype(np.float64)).to(times.dtype)
    K, B, T = len(cls.forcings or ()), cond.shape[0], times.shape[0]
    if K:
        series = cond[:, cond.shape[1] - K * T:].reshape(B, K, T)
        padded = torch.cat([series[:, :, :1].expand(B, K, n), series], dim=2)
        cond = torch.cat([cond[:, :cond.shape[1] - K * T], padded.reshape(B, -1)], dim=1)
    return torch.cat([lead, times]), cond


def _leaves(pb, dtype):
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    return {n: leaf(v) for n, v in pb["th"].items()}


def _problem_on(cls, th, cond, times, start, lead):
    """(rhs on the extended grid, the state the integration starts from, the extended grid, the lead-in steps taken)."""
    n = lead_steps(cls) if lead else 0
    times_x, cond_x = extended(cls, cond, times) if n else (times, cond)
    rhs, x0 = cls.torch_problem(th, cond_x, None, start=start, **({"times": times_x} if cls.forcings else {}))
    return rhs, x0, times_x, n


def explicit_states(cls, th, cond, times, solver, start=True, lead=True):
    """The states at the observation points [B,S,N,T] of an explicit scheme (differentiable): the left limits where the class
    has a jump."""
    m, T = int(cls.substeps), len(times)
    rhs, y, times_x, n = _problem_on(cls, th, cond, times, start, lead)
    hl = lead_step_size(cls, float(times[0])) if n else None
    for j in range(n):  # nothing of these is kept
        y = JM.one_step(solver, rhs, times_x[j], times_x[j + 1], hl, y)
    fine = SM.refined(times, m)
    h_fixed = fine[1] - fine[0]
    states = [y]
    for k in range(T - 1):
        u = JM.jump_at(cls, y, th, cond, k, T) if cls._jump_def is not None else y
        for j in range(m):
            u = JM.one_step(solver, rhs, fine[k * m + j], fine[k * m + j + 1], h_fixed, u)
        y = u
        states.append(y)
    return torch.stack(states, dim=3)


def explicit_definition(cls, pb, solver, dtype, start=True, lead=True):
    th = _leaves(pb, dtype)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    xs = explicit_states(cls, th, cond, times, solver, start, lead)
    full, xp, logp = SM.hooks(cls, xs, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}}


def beuler_states(cls, th, cond, times, start=True, lead=True, newton=None, differentiable=False):
    """(the states at the observation points [B,S,N,T], the steps taken as (t0, t1, the state the step ended on, the
    observation point it ends on or None), the state the integration started from, the largest last Newton increment relative
    to the state -- lead-in steps included) of backward Euler."""
    m, T = int(cls.substeps), len(times)
    newton = int(cls.newton_iterations) if newton is None else newton
    rhs, x0, times_x, n = _problem_on(cls, th, cond, times, start, lead)
    fine = SM.refined(times, m)
    jac = (lambda f, t, z: IM.autograd_jacobian(f, t, z, create_graph=True)) if differentiable else IM.autograd_jacobian
    steps, worst, y, states = [], 0.0, x0, []

    def take(t0, t1, u):
        u, d = IM.newton_step(rhs, t1, t1 - t0, u, newton, jac)
        dd, uu = d.detach(), u.detach()
        rel = float((dd.abs().amax(-1) / uu.abs().amax(-1).clamp_min(1e-30)).max()) if bool(torch.isfinite(dd).all()) \
            else float("inf")
        return u, rel

    with torch.enable_grad() if differentiable else torch.no_grad():
        for j in range(n):
            y, rel = take(times_x[j], times_x[j + 1], y)
            worst = max(worst, rel)
            steps.append((times_x[j], times_x[j + 1], y, None))
        states.append(y)
        for k in range(T - 1):
            u = JM.jump_at(cls, y, th, cond, k, T) if cls._jump_def is not None else y
            for j in range(m):
                q = k * m + j
                u, rel = take(fine[q], fine[q + 1], u)
                worst = max(worst, rel)
                steps.append((fine[q], fine[q + 1], u, k + 1 if j == m - 1 else None))
            y = u
            states.append(y)
    return torch.stack(states, dim=3), steps, x0, worst


def beuler_definition(cls, pb, dtype, start=True, lead=True):
    """Backward Euler in `dtype` and the gradient of sum(logp * G) by the implicit-function adjoint at the scheme's own
    iterates (modelgen_jump_models.beuler_definition), continued through the lead-in steps to the state the integration
    started from, whose graph -- torch_start of the initial state -- takes it to theta."""
    th = _leaves(pb, dtype)
    names = list(th)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    m, T = int(cls.substeps), len(times)
    xs, steps, _, last = beuler_states(cls, th, cond, times, start, lead)
    N = xs.shape[2]
    Y = xs.detach().clone().requires_grad_(True)
    full, xp, logp = SM.hooks(cls, Y, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    direct = torch.autograd.grad(loss, [Y] + [th[n] for n in names], allow_unused=True)
    gY = direct[0]
    g = {n: (torch.zeros_like(th[n]) if v is None else v.clone()) for n, v in zip(names, direct[1:])}
    rhs, x0, _, n = _problem_on(cls, th, cond, times, start, lead)
    eye = torch.eye(N, dtype=dtype)

    def add(outputs, seed):
        if not outputs.requires_grad:
            return
        for nm, v in zip(names, torch.autograd.grad(outputs, [th[q] for q in names], grad_outputs=seed, allow_unused=True,
                                               retain_graph=True)):
            if v is not None:
                g[nm] += v

    def step_adjoint(q, lam):
        t0, t1, y1, _ = steps[q]
        y1, h = y1.detach(), t1 - t0
        A = eye - h * IM.autograd_jacobian(rhs, t1, y1)
        mu = torch.linalg.solve(A.transpose(-1, -2), lam.unsqueeze(-1)).squeeze(-1)
        add(rhs(t1, y1), h * mu)
        return mu

    lam = gY[..., T - 1]
    for k in range(T - 2, -1, -1):
        for j in range(m - 1, -1, -1):
            lam = step_adjoint(n + k * m + j, lam)
        if cls._jump_def is not None:
            yk = xs[..., k].detach().clone().requires_grad_(True)
            yj = JM.jump_at(cls, yk, th, cond, k, T)
            add(yj, lam)
            lam = torch.autograd.grad(yj, yk, grad_outputs=lam)[0]
        lam = lam + gY[..., k]
    for j in range(n - 1, -1, -1):
        lam = step_adjoint(j, lam)
    add(x0, lam)
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "g_theta": g,
            "last_increment": last}


def definition(cls, pb, solver, dtype, start=True, lead=True):
    return beuler_definition(cls, pb, dtype, start, lead) if solver == "beuler" \
        else explicit_definition(cls, pb, solver, dtype, start, lead)


def beuler_by_autograd(cls, pb, newton):
    """float64: autograd through `newton` Newton iterations per step, lead-in steps included -- what the restated adjoint must
    agree with once the iteration has converged."""
    th = _leaves(pb, torch.float64)
    xs, _, _, _ = beuler_states(cls, th, pb["cond"], pb["times"], newton=newton, differentiable=True)
    _, _, logp = SM.hooks(cls, xs, th, pb["cond"], pb["obs"])
    (logp * pb["G"]["logp"]).sum().backward()
    return {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}


# ---- inputs of the numeric tests ----------------------------------------------------------------------------------------------
def problem(cls, B, S, times=None, seed=29):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, the wide cond (treatments
    0.3, 1.0, 1.7, ... : both sides of INDUCED_ABOVE), times, observations (the first sample's prediction under the definition
    with 5 % noise) and an upstream gradient for the log-likelihood."""
    times = grid_of(cls) if times is None else times
    k = (cls, B, S, tuple(times), seed)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    if cls in STIFF:
        assert sorted(slot_names(cls)) == sorted(IM.FAST_DRAWS)
        th = {n: mu * torch.exp(sd * rnd(B, S)) for n, (mu, sd) in IM.FAST_DRAWS.items()}
    else:
        assert sorted(slot_names(cls)) == sorted(BASES[cls])
        th = {n: v * torch.exp(0.2 * rnd(B, S)) for n, v in BASES[cls].items()}
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = JM.series_of(cls, B, tt)
    cond = FM.wide_cond(treatments, series)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        xs = beuler_states(cls, th1, cond, tt)[0] if cls in STIFF else explicit_states(cls, th1, cond, tt, "rk4")
        xp = SM.hooks(cls, xs, th1, cond, torch.zeros(B, 4, T, dtype=torch.float64))[1]
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "treatments": treatments, "times": tt, "obs": obs, "W": {}, "B": B, "S": S,
          "T": T, "G": {"logp": rnd(B, S, 4)}}
    _PROBLEMS[k] = pb
    return pb
