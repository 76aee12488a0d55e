"""Models with `implicit_order = 2` (Alexander's two-stage SDIRK under the solver "beuler", csrc/vihds_implicit.hpp) for the
tests: order-2 twins of the implicit models of modelgen_implicit_models.py, and one twin each of a sub-stepped, a jump and a
lead-in class of the stiff binding model.  Their inputs are those of their order-1 twins, from the module that defines the twin.

The float64 yardstick is written here, once, for the host and the GPU tests: the scheme exactly as vihds.modelgen's docstring
defines it, with the float32 constants gamma and c widened -- NEWTON iterations per stage, the Jacobian by autograd of
torch_problem's right-hand side, the linear solves by torch.linalg.solve (pivoted) -- over the sub-steps, jumps and lead-in
steps a class has, and the written-out adjoint of the converged step: z1 kept from the forward run, A2 = I - a J(t1, y_k+1),
A2^T mu2 = lambda, A1 = I - a J(tg, z1), A1^T mu1 = c mu2, the parameter parts (a mu2)^T df/dtheta at (t1, y_k+1) and
(a mu1)^T df/dtheta at (tg, z1), lambda <- (1 - c) mu2 + mu1."""
import numpy as np
import torch

import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_leadin_models as LM
import modelgen_substep_models as SM
from modelgen_piecewise_models import TIMES  # noqa: F401  (for the tests)

GAMMA = float(np.float32(0.29289323))  # the float nearest 1 - sqrt(2)/2
C = float(np.float32(2.4142137))  # the float nearest 1 + sqrt(2)


class PrprSdirk(IM.PrprImplicit):
    model_key = "gen_prpr_constant_sdirk2"
    implicit_order = 2


class DrSdirk(IM.DrImplicit):
    """Eight species, the sparse Jacobian."""
    model_key = "gen_dr_constant_sdirk2"
    implicit_order = 2


class DenseEightSdirk(IM.DenseEight):
    """Eight species, every entry of the Jacobian a structural non-zero: the register worst case."""
    model_key = "gen_dense_eight_sdirk2"
    implicit_order = 2


class PrprForcedSdirk(IM.PrprForcedImplicit):
    """The only class whose result changes if stage 1 read its forcing at t1 in place of tg."""
    model_key = "gen_prpr_constant_forced_sdirk2"
    implicit_order = 2


class FastBindingSdirk(IM.FastBinding):
    model_key = "gen_fast_binding_sdirk2"
    implicit_order = 2


class FastBindingSdirkSub2(IM.FastBinding):
    model_key = "gen_fast_binding_sdirk2_sub2"
    implicit_order = 2
    substeps = 2


class FastBindingDosedSdirk(JM.FastBindingDosed):
    model_key = "gen_fast_binding_dosed_sdirk2"
    implicit_order = 2


class FastBindingLeadSdirk(LM.FastBindingLead):
    model_key = "gen_fast_binding_lead_sdirk2"
    implicit_order = 2


# the order-1 class whose inputs a class is tested on (and whose kernels it is compared with)
TWIN = {PrprSdirk: IM.PrprImplicit, DrSdirk: IM.DrImplicit, DenseEightSdirk: IM.DenseEight,
        PrprForcedSdirk: IM.PrprForcedImplicit, FastBindingSdirk: IM.FastBinding, FastBindingSdirkSub2: IM.FastBinding,
        FastBindingDosedSdirk: JM.FastBindingDosed, FastBindingLeadSdirk: LM.FastBindingLead}
PLAIN = [PrprSdirk, DrSdirk, DenseEightSdirk, PrprForcedSdirk, FastBindingSdirk]
COMBINED = [FastBindingSdirkSub2, FastBindingDosedSdirk, FastBindingLeadSdirk]
MODELS = PLAIN + COMBINED
STIFF = (FastBindingSdirk,) + tuple(COMBINED)  # the forward bounds follow the float32 torch run (conditioning of I - a J)
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS]


def slot_names(cls):
    return LM.slot_names(cls)


def problem(cls, B, S, times=None, **kw):
    """Inputs of one case (shared by the tests that use it; never modified): those of the class's order-1 twin on the grid the
    twin is tested on, from the module that defines the twin."""
    twin = TWIN[cls]
    if twin is JM.FastBindingDosed:
        return JM.problem(twin, B, S, **({} if times is None else {"times": times}))
    if twin is LM.FastBindingLead:
        return LM.problem(twin, B, S, times=times)
    return IM.problem(twin, B, S, times=times, **kw)


# ---- the definition of the scheme in torch -------------------------------------------------------------------------------------
def sdirk2_step(rhs, t0, t1, y, newton, jacobian=IM.autograd_jacobian):
    """One step of the scheme as defined, from y at t0 to t1.  Returns (y_k+1, z1, the larger of the two stages' last Newton
    increments per trajectory [B,S])."""
    eye = torch.eye(y.shape[-1], dtype=y.dtype)
    h = t1 - t0
    a, tg = GAMMA * h, t0 + GAMMA * h

    def stage(t, base, z):
        d = None
        for _ in range(newton):
            F = z - base - a * rhs(t, z)
            A = eye - a * jacobian(rhs, t, z)
            d = torch.linalg.solve(A, -F.unsqueeze(-1)).squeeze(-1)
            z = z + d
        return z, d.detach().abs().amax(-1)

    z1, d1 = stage(tg, y, y)
    w = y + C * (z1 - y)
    y1, d2 = stage(t1, w, z1)
    return y1, z1, torch.maximum(d1, d2)


def sdirk2_step_adjoint(rhs, t0, t1, z1, y1, lam, jacobian=IM.autograd_jacobian):
    """The written-out adjoint of one converged step: (the adjoint of y_k, mu1, mu2) from lam, the adjoint of y_k+1 = y1, and the
    step's stage value z1.  The caller adds the parameter parts (a mu2)^T df/dtheta at (t1, y1) and (a mu1)^T df/dtheta at
    (tg, z1)."""
    eye = torch.eye(y1.shape[-1], dtype=y1.dtype)
    a, tg = GAMMA * (t1 - t0), t0 + GAMMA * (t1 - t0)
    A2 = eye - a * jacobian(rhs, t1, y1)
    mu2 = torch.linalg.solve(A2.transpose(-1, -2), lam.unsqueeze(-1)).squeeze(-1)
    A1 = eye - a * jacobian(rhs, tg, z1)
    mu1 = torch.linalg.solve(A1.transpose(-1, -2), (C * mu2).unsqueeze(-1)).squeeze(-1)
    return (1.0 - C) * mu2 + mu1, mu1, mu2


def sdirk2_states(cls, th, cond, times, newton=None, differentiable=False, jacobian=None, m=None):
    """(the states at the observation points [B,S,N,T] -- the left limits where the class has a jump --, the steps taken as
    (t0, t1, the state the step started from, z1, the state it ended on), the state the integration started from, the largest
    last Newton increment of any stage relative to the state, lead-in steps included) of the scheme with the class's sub-steps
    (m, if given, in their place), jump and lead-in phase."""
    m, T = int(cls.substeps) if m is None else m, len(times)
    newton = int(cls.newton_iterations) if newton is None else newton
    rhs, x0, times_x, n = LM._problem_on(cls, th, cond, times, True, True)
    fine = SM.refined(times, m)
    if jacobian is None:
        jacobian = (lambda f, t, z: IM.autograd_jacobian(f, t, z, create_graph=True)) if differentiable else IM.autograd_jacobian
    steps, worst, y, states = [], 0.0, x0, []

    def take(t0, t1, u):
        nonlocal worst
        u1, z1, d = sdirk2_step(rhs, t0, t1, u, newton, jacobian)
        rel = float((d / u1.detach().abs().amax(-1).clamp_min(1e-30)).max()) if bool(torch.isfinite(d).all()) else float("inf")
        worst = max(worst, rel)
        steps.append((t0, t1, u, z1, u1))
        return u1

    with torch.enable_grad() if differentiable else torch.no_grad():
        for j in range(n):  # nothing of these is kept
            y = take(times_x[j], times_x[j + 1], y)
        states.append(y)
        for k in range(T - 1):
            u = JM.jump_at(cls, y, th, cond, k, T) if cls._jump_def is not None else y
            for j in range(m):
                u = take(fine[k * m + j], fine[k * m + j + 1], u)
            y = u
            states.append(y)
    return torch.stack(states, dim=3), steps, x0, worst


def definition(cls, pb, dtype):
    """The scheme in `dtype` and the gradient of sum(logp * G) with respect to theta by the written-out adjoint of the converged
    step (module docstring) at the scheme's own iterates, with torch_jump's autograd pullback between the observation
    intervals, continued through the lead-in steps to the state the integration started from."""
    th = LM._leaves(pb, dtype)
    names = list(th)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    m, T = int(cls.substeps), len(times)
    xs, steps, _, last = sdirk2_states(cls, th, cond, times)
    Y = xs.detach().clone().requires_grad_(True)
    full, xp, logp = SM.hooks(cls, Y, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    direct = torch.autograd.grad(loss, [Y] + [th[n] for n in names], allow_unused=True)
    gY = direct[0]
    g = {n: (torch.zeros_like(th[n]) if v is None else v.clone()) for n, v in zip(names, direct[1:])}
    rhs, x0, _, n = LM._problem_on(cls, th, cond, times, True, True)

    def add(outputs, seed):
        if not outputs.requires_grad:
            return
        for nm, v in zip(names, torch.autograd.grad(outputs, [th[q] for q in names], grad_outputs=seed, allow_unused=True,
                                               retain_graph=True)):
            if v is not None:
                g[nm] += v

    def step_adjoint(q, lam):
        t0, t1, _, z1, y1 = steps[q]
        z1, y1 = z1.detach(), y1.detach()
        a, tg = GAMMA * (t1 - t0), t0 + GAMMA * (t1 - t0)
        lam, mu1, mu2 = sdirk2_step_adjoint(rhs, t0, t1, z1, y1, lam)
        add(rhs(t1, y1), a * mu2)
        add(rhs(tg, z1), a * mu1)
        return lam

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
            "g_w": [], "last_increment": last}


def by_autograd(cls, pb, newton, dtype=torch.float64):
    """Autograd through `newton` Newton iterations per stage whose Jacobians are part of the graph -- sub-steps, jumps and
    lead-in steps included: what the written-out adjoint must agree with once the iteration has converged.  The same keys as
    definition()."""
    th = LM._leaves(pb, dtype)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    xs, _, _, last = sdirk2_states(cls, th, cond, times, newton=newton, differentiable=True)
    full, xp, logp = SM.hooks(cls, xs, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}, "g_w": [],
            "last_increment": last}


# ---- FastBinding by hand (the refined-grid solutions of the stiff tests: no autograd in their thousands of steps) --------------
def fast_sdirk2(th, times, refine=1, newton=6):
    """FastBinding by the scheme on a grid `refine` times finer, float64, with modelgen_implicit_models' hand-written right-hand
    side and Jacobian: [B,S,4,T] at `times`."""
    y = torch.tensor(IM.FastBinding.Y0, dtype=torch.float64).expand(th["kon"].shape + (4,))
    rhs, jac = (lambda t, z: IM.fast_rhs(th, z)), (lambda f, t, z: IM.fast_jacobian(th, z))
    fine = SM.refined(torch.as_tensor(times, dtype=torch.float64), refine)
    ys = [y]
    with torch.no_grad():
        for q in range(len(fine) - 1):
            y = sdirk2_step(rhs, fine[q], fine[q + 1], y, newton, jac)[0]
            if (q + 1) % refine == 0:
                ys.append(y)
    return torch.stack(ys, dim=3)


def fast_beuler(th, times, refine=1, newton=6):
    """... by backward Euler, likewise."""
    return IM.fast_refined(th, torch.as_tensor(times, dtype=torch.float64), refine=refine, newton=newton)
