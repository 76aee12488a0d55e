"""Models with a state jump at the observation points (`jump(self, y, p, c)` of vihds.modelgen) for the tests: the forced prpr
restatement diluted and dosed on a schedule that differs from well to well, the prpr restatement as a turbidostat (a condition
on a species), the stiff binding model with a bolus of A (implicit, and its substeps = 2 twin), the plate reader with its own
observation map, precision map and Student-t likelihood diluted on a schedule, and a growth law with a network in rhs and a
bolus into its latent species.  Every one of them has a parameter that only the jump reads.

The float64 yardstick of the GPU comparisons is written here, once, for the host and the GPU tests.  It is the definition of
the module docstring of vihds.modelgen in torch: y_0 the initial state; for k = 0 .. T-1 the state y_k is kept (the left limit:
what is stored, observed and scored), and for k < T-1 the next one is Phi(t_k, t_k+1, torch_jump(y_k)), Phi the fixed-grid scheme
over one observation interval, sub-steps included.  Explicit schemes: the oracle's own step functions interval by interval,
gradients by autograd.  beuler: modelgen_implicit_models.newton_step and the implicit-function adjoint of
modelgen_implicit_models.definition, with torch_jump and its autograd pullback between the steps.  With `jump=False` both are
their parents' definitions (tests/test_modelgen_jump_host.py holds them to the last bit).

The turbidostat compares a species with a constant, so its inputs are chosen as modelgen_piecewise_models.problem chooses them:
candidates are drawn from a pool and the first S per data row kept whose float64 trajectories keep every comparison at least
2 * MARGIN wide under the solvers the tests use; no trajectory is ever left out of a comparison.  `problem` asserts, on the
float64 run alone, that in every data row at least one kept sample triggers a dilution and at least one never does."""
import torch

from oracle import vihds_oracle as O
from vihds.modelgen import Network, sigmoid, where

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_likelihood_models as LM
import modelgen_substep_models as SM
from modelgen_hybrid_models import _Growth
from modelgen_models import PREC, PrprRestated
from modelgen_piecewise_models import MARGIN, POOL, TIMES, recording, sw  # noqa: F401  (MARGIN, TIMES: for the tests)

THRESHOLD = 0.1  # the optical density above which the turbidostat dilutes


class PrprDiluted(FM.PrprForced):
    """PrprForced whose wells are diluted and dosed at some reads: every species is scaled by the point's `keep` (1.0 where
    nothing happens) and `dose * bolus` of YFP is added; `bolus` is read by the jump alone."""
    model_key = "gen_prpr_constant_diluted"
    parameters = FM.PrprForced.parameter_names + ["bolus"]
    forcings = ["light", "keep", "dose"]

    def prepare(self, th, c):
        p = FM.PrprForced.prepare(self, th, c)
        p["bolus"] = th.bolus
        return p

    def jump(self, y, p, c):
        keep = self.forcing.keep
        out = [v * keep for v in y]
        out[2] = out[2] + self.forcing.dose * p.bolus
        return out


class PrprTurbidostat(PrprRestated):
    """PrprRestated in a turbidostat: whenever the optical density at a read is above THRESHOLD every species is scaled by
    `dil`, a parameter read nowhere else.  No forcings: the event is triggered by the state."""
    model_key = "gen_prpr_constant_turbidostat"
    parameters = PrprRestated.parameter_names + ["dil"]

    def prepare(self, th, c):
        p = PrprRestated.prepare(self, th, c)
        p["dil"] = th.dil
        return p

    def jump(self, y, p, c):
        dense = sw.gt("jump OD > threshold", y[0], THRESHOLD)
        return [where(dense, v * p.dil, v) for v in y]


class FastBindingDosed(IM.FastBinding):
    """The stiff binding model with a bolus of A pipetted in at some reads: `dose * bolus` is added to A."""
    model_key = "gen_fast_binding_dosed"
    parameters = IM.FastBinding.parameter_names + ["bolus"]
    forcings = ["dose"]

    def prepare(self, th, c):
        p = IM.FastBinding.prepare(self, th, c)
        p["bolus"] = th.bolus
        return p

    def jump(self, y, p, c):
        return [y[0] + self.forcing.dose * p.bolus, y[1], y[2], y[3]]


class FastBindingDosedSub2(FastBindingDosed):
    model_key = "gen_fast_binding_dosed_sub2"
    substeps = 2


class PlateReaderDiluted(LM.PlateReaderStudentT):
    """The plate reader with its own observation map, its own precision map and its Student-t likelihood, diluted on a schedule:
    a fraction `frac` (read by the jump alone) of what the schedule removes is really removed.  The full adjoint order."""
    model_key = "gen_plate_reader_student_t_diluted"
    parameters = LM.PlateReaderStudentT.parameter_names + ["frac"]
    forcings = ["keep"]

    def prepare(self, th, c):
        p = LM.PlateReaderStudentT.prepare(self, th, c)
        p["frac"] = th.frac
        return p

    def jump(self, y, p, c):
        left = 1.0 - p.frac * (1.0 - self.forcing.keep)
        return [v * left for v in y]


class HybridDosed(_Growth):
    """The growth law of the hybrid tests with one network in rhs (a 3 -> 4 -> 1 tanh gate of the expression rate) and a bolus
    into its latent species Z1, which drives YFP: the dump form of the adjoint."""
    model_key = "gen_growth_gate_dosed"
    parameters = _Growth.parameter_names + ["bolus"]
    forcings = ["dose"]
    networks = {"gate": Network(n_inputs=3, n_hidden=4, n_outputs=1, hidden="tanh")}

    def prepare(self, th, c):
        p = _Growth.prepare(self, th, c)
        p["bolus"] = th.bolus
        return p

    def rhs(self, t, y, p, c):
        g = self.net.gate([t, y[0], y[4]])
        return self.dynamics(t, y, p, [0.5, 0.5, 0.5, 0.5], sigmoid(g[0]))

    def jump(self, y, p, c):
        return [y[0], y[1], y[2], y[3], y[4] + self.forcing.dose * p.bolus, y[5]]


MODELS = [PrprDiluted, PrprTurbidostat, FastBindingDosed, FastBindingDosedSub2, PlateReaderDiluted, HybridDosed]
STIFF = (FastBindingDosed, FastBindingDosedSub2)  # beuler only: the explicit schemes blow up at their inputs
JUMP_ONLY = {PrprDiluted: "bolus", PrprTurbidostat: "dil", FastBindingDosed: "bolus", FastBindingDosedSub2: "bolus",
             PlateReaderDiluted: "frac", HybridDosed: "bolus"}  # the parameter that only the jump reads
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS]

GROWTH_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP": 1.2, "aCFP": 0.9,
               "e76": 0.1, "init_x": 0.05, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
               "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
BASES = {PrprDiluted: dict(FM.PRPR_BASE, bolus=0.5), PrprTurbidostat: dict(FM.PRPR_BASE, dil=0.5),
         PlateReaderDiluted: dict(FM.READER_BASE, frac=0.8), HybridDosed: dict(GROWTH_BASE, bolus=0.5)}
FAST_DRAWS = dict(IM.FAST_DRAWS, bolus=(0.4, 0.2))
_PROBLEMS = {}


def solvers_of(cls):
    """The solvers the GPU tests run a model with: midpoint and rk4, modeuler too for PrprDiluted (its fixed h0), beuler for the
    implicit ones (alone for them: they are stiff at their inputs)."""
    if cls in STIFF:
        return ["beuler"]
    return (["modeuler"] if cls is PrprDiluted else []) + ["midpoint", "rk4"]


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


# ---- the schedules ----------------------------------------------------------------------------------------------------------------
def events_of(b, T):
    """The points at which data row b has an event: two or three of them, point 0 among them for every row; the rows differ, and
    every third row has one at the last point, where a jump has no effect."""
    return sorted({0, (3 + b % 3) % T, (6 + b % 3) % T}) if b % 3 else [0, 4 % T]


def schedule(B, T):
    """(keep [B,T]: 1.0 but at the row's events, where 0.5 .. 0.7 of the culture is kept; dose [B,T]: 0.0 but at the events)."""
    keep, dose = torch.ones(B, T, dtype=torch.float64), torch.zeros(B, T, dtype=torch.float64)
    for b in range(B):
        for q, k in enumerate(events_of(b, T)):
            keep[b, k] = 0.5 + 0.1 * ((b + q) % 3)
            dose[b, k] = 0.3 + 0.1 * ((b + 2 * q) % 4)
    return keep, dose


def series_of(cls, B, times):
    """The forcing samples of a class [B, K, T], in the order of cls.forcings."""
    T = len(times)
    keep, dose = schedule(B, T)
    named = {"light": FM.smooth_series(B, times), "keep": keep, "dose": dose}
    return torch.stack([named[n] for n in cls.forcings], dim=1) if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)


# ---- the definition in torch ---------------------------------------------------------------------------------------------------
def jump_at(cls, y, th, cond, k, T):
    """torch_jump at point k of T for the states y [B,S,N]: a class with forcings reads sample k of its series."""
    if cls.forcings:
        return cls.torch_jump(y.unsqueeze(-1).expand(y.shape + (T,)), th, cond)[..., k]
    return cls.torch_jump(y.unsqueeze(-1), th, cond)[..., 0]


def one_step(solver, rhs, t0, t1, h_fixed, y):
    """One step of an explicit scheme, in the oracle's own arithmetic (oracle.vihds_oracle: modified_euler_integrate with its
    fixed h, modified_euler_while, _fixed_grid with the step functions)."""
    if solver in ("modeuler", "modeulerwhile"):
        h = h_fixed if solver == "modeuler" else t1 - t0
        f1 = rhs(t0, y)
        f2 = rhs(t1, y + h * f1)
        return y + 0.5 * h * (f1 + f2)
    step = {"euler": O._euler_step, "midpoint": O._midpoint_step, "rk4": O._rk4_38_step}[solver]
    return y + step(rhs, t0, t1 - t0, y)


def _leaves(pb, dtype):
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    W = {name: tuple(leaf(w) for w in ws) for name, ws in pb["W"].items()} or None
    return th, W


def _torch_rhs(cls, th, cond, times, W):
    return cls.torch_problem(th, cond, W, **({"times": times} if cls.forcings else {}))


def explicit_states(cls, th, cond, times, solver, W=None, jump=True):
    """The left limits [B,S,N,T] of an explicit scheme (differentiable)."""
    m, T = int(cls.substeps), len(times)
    rhs, x0 = _torch_rhs(cls, th, cond, times, W)
    fine = SM.refined(times, m)
    h_fixed = fine[1] - fine[0]
    y, lefts = x0, [x0]
    for k in range(T - 1):
        u = jump_at(cls, y, th, cond, k, T) if jump and cls._jump_def is not None else y
        for j in range(m):
            u = one_step(solver, rhs, fine[k * m + j], fine[k * m + j + 1], h_fixed, u)
        y = u
        lefts.append(y)
    return torch.stack(lefts, dim=3)


def explicit_definition(cls, pb, solver, dtype, jump=True):
    """An explicit scheme interval by interval with torch_jump between, autograd for the gradient of sum(logp * G) with respect
    to theta and the network weights; in float64 the margins of its switches are recorded."""
    th, W = _leaves(pb, dtype)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    with recording() as mg:
        xs = explicit_states(cls, th, cond, times, solver, W, jump)
        full, xp, logp = SM.hooks(cls, xs, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "margins": mg,
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()},
            "g_w": [w.grad for ws in (W or {}).values() for w in ws]}


def beuler_states(cls, th, cond, times, jump=True):
    """(the left limits [B,S,N,T], every state of the refined grid as the scheme left it -- entry q + 1 is what step q of the
    refined grid ended on --, the refined grid, the largest last Newton increment relative to the state) of backward Euler."""
    m, T = int(cls.substeps), len(times)
    rhs, x0 = IM.torch_rhs(cls, th, cond, times)
    fine = SM.refined(times, m)
    y, lefts, ends, worst = x0, [x0], [x0], 0.0
    with torch.no_grad():
        for k in range(T - 1):
            u = jump_at(cls, y, th, cond, k, T) if jump and cls._jump_def is not None else y
            for j in range(m):
                q = k * m + j
                u, d = IM.newton_step(rhs, fine[q + 1], fine[q + 1] - fine[q], u, int(cls.newton_iterations))
                worst = max(worst, float((d.abs().amax(-1) / u.abs().amax(-1).clamp_min(1e-30)).max())
                            if bool(torch.isfinite(d).all()) else float("inf"))
                ends.append(u)
            y = u
            lefts.append(y)
    return torch.stack(lefts, dim=3), ends, fine, worst


def beuler_definition(cls, pb, dtype, jump=True):
    """Backward Euler in `dtype` and the gradient of sum(logp * G) by the implicit-function adjoint at the scheme's own iterates
    (modelgen_implicit_models.definition; on the refined grid as modelgen_substep_models.beuler_definition), with torch_jump's
    autograd pullback between the observation intervals: after the step adjoints of interval k, lambda is the adjoint of
    jump(y_k); its pullback through the jump is the adjoint of y_k, to which dL/dy_k of the point's hooks is added."""
    th, _ = _leaves(pb, dtype)
    names = list(th)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    m, T = int(cls.substeps), len(times)
    with recording() as mg:
        xs, ends, fine, last = beuler_states(cls, th, cond, times, jump)
    N = xs.shape[2]
    Y = xs.detach().clone().requires_grad_(True)
    full, xp, logp = SM.hooks(cls, Y, th, cond, obs)
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

    lam = gY[..., T - 1]
    for k in range(T - 2, -1, -1):
        for j in range(m - 1, -1, -1):
            q = k * m + j
            t1, h = fine[q + 1], fine[q + 1] - fine[q]
            y1 = ends[q + 1].detach()
            A = eye - h * IM.autograd_jacobian(rhs, t1, y1)
            mu = torch.linalg.solve(A.transpose(-1, -2), lam.unsqueeze(-1)).squeeze(-1)
            add(rhs(t1, y1), h * mu)
            lam = mu
        if jump and cls._jump_def is not None:
            yk = xs[..., k].detach().clone().requires_grad_(True)
            yj = jump_at(cls, yk, th, cond, k, T)
            add(yj, lam)
            lam = torch.autograd.grad(yj, yk, grad_outputs=lam)[0]
        lam = lam + gY[..., k]
    add(x0, lam)
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "g_theta": g,
            "g_w": [], "last_increment": last, "margins": mg}


def definition(cls, pb, solver, dtype, jump=True):
    return beuler_definition(cls, pb, dtype, jump) if solver == "beuler" else explicit_definition(cls, pb, solver, dtype, jump)


def triggered(cls, traj):
    """[B,S] bools: the trajectories of the turbidostat that are diluted at least once (the last point's jump does not count)."""
    assert cls is PrprTurbidostat
    return (traj[:, :, 0, :-1] > THRESHOLD).any(dim=-1)


# ---- inputs of the numeric tests: chosen on the float64 yardstick alone ------------------------------------------------------
def _draw(cls, B, n, rnd):
    if cls in STIFF:
        return {k: mu * torch.exp(sd * rnd(B, n)) for k, (mu, sd) in FAST_DRAWS.items()}
    return {k: v * torch.exp(0.2 * rnd(B, n)) for k, v in BASES[cls].items()}


def problem(cls, B, S, times=TIMES, seed=23):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, the wide cond, times, network
    weights, observations (the first sample's prediction under the definition, jumps included, with 5 % noise) and an upstream
    gradient for the log-likelihood.  The turbidostat's samples are kept from a pool (module docstring)."""
    k = (cls, B, S, tuple(times), seed)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    assert sorted(slot_names(cls)) == sorted(FAST_DRAWS if cls in STIFF else BASES[cls])
    pooled = cls is PrprTurbidostat
    th = _draw(cls, B, POOL * S if pooled else S, rnd)
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = series_of(cls, B, tt)
    cond = FM.wide_cond(treatments, series)
    W = {name: tuple(0.6 * rnd(*shape) for shape in net.tensor_shapes()) for name, net in (cls.networks or {}).items()}
    first = "beuler" if cls in STIFF else "rk4"
    if pooled:
        with torch.no_grad():
            keep = torch.ones(B, POOL * S, dtype=torch.bool)
            for solver in solvers_of(cls):
                with recording() as mg:
                    explicit_states(cls, th, cond, tt, solver)
                keep &= mg.per_trajectory >= 2.0 * MARGIN
        assert int(keep.sum(1).min()) >= S, "too few candidates keep their switches wide: %s" % keep.sum(1).tolist()
        pick = torch.stack([torch.nonzero(keep[b])[:S, 0] for b in range(B)])
        th = {name: v.gather(1, pick) for name, v in th.items()}
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        xs = beuler_states(cls, th1, cond, tt)[0] if first == "beuler" else explicit_states(cls, th1, cond, tt, first, W or None)
        xp = SM.hooks(cls, xs, th1, cond, torch.zeros(B, 4, T, dtype=torch.float64))[1]
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "treatments": treatments, "times": tt, "obs": obs, "W": W, "B": B, "S": S,
          "T": T, "G": {"logp": rnd(B, S, 4)}}
    if pooled:  # on the float64 run alone: in every data row a sample that is diluted and one that never is
        with torch.no_grad():
            for solver in solvers_of(cls):
                trig = triggered(cls, explicit_states(cls, th, cond, tt, solver))
                assert bool(trig.any(1).all()) and bool((~trig).any(1).all()), (solver, trig.sum(1).tolist())
    _PROBLEMS[k] = pb
    return pb
