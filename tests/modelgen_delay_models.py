"""Models with delayed state reads (the `delays` of vihds.modelgen) for the tests, and the float64 yardstick of the scheme.

DelayedRepressor: growth plus dR/dt = beta / (1 + (R(t - tau) / K)^n) - gamma R, the textbook delayed negative feedback, with an
observation map of its own.  DelayedRepressorFrozen: its twin without any delay machinery, R(t_0) -- the initial-state parameter
-- in place of the read: what the delay model computes once tau spans the whole grid.  TwoDelays: two reads of different species,
one forcing, and one delay shared through prepare as 2 * tau.  DelayedStart: a read in a class with a start map (the constant
history is the state after start).

The yardstick (`simulate`) is the definition of csrc/vihds_delay.hpp in plain torch: per observation interval the two lookups
H(t_k - taue) and H(min(t_k+1 - taue, t_k)) into the states so far (searchsorted, gather), the chord between them read by every
stage, the schemes of oracle.vihds_oracle stepped with it.  Autograd differentiates the interpolation weights with respect to tau
by itself."""
import torch

from oracle import vihds_oracle as O
from vihds.modelgen import GeneratedOdeModel, clamp
from vihds.precisions import ConstantPrecisions

from modelgen_models import PREC
from modelgen_piecewise_models import FIXED  # noqa: F401  (the five fixed-grid solvers, for the tests)

RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # the grid of tests/test_modelgen_forcing_gpu.py: steps 0.1 .. 1.0


def _feedback(p, r_lag):
    q = r_lag / p.K
    return p.beta / (1.0 + q * q)


class _Repressor(GeneratedOdeModel):
    species = ["OD", "R"]
    parameters = ["r", "cap", "beta", "K", "gamma", "tau", "gain", "init_x", "init_r"]

    def __init__(self, config):
        super(_Repressor, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "cap": th.cap, "beta": th.beta, "K": th.K, "gamma": th.gamma, "tau": th.tau,
                "gain": th.gain, "r0": th.init_r}

    def initial_state(self, th, c):
        return [th.init_x, th.init_r]

    def observe(self, y, p, c):
        return [y[0], p.gain * y[1], y[1] / (1.0 + y[1]), y[0] * y[1]]


class DelayedRepressor(_Repressor):
    """Delayed negative feedback: the repressor's production reads its own concentration tau ago."""
    model_key = "gen_delayed_repressor"
    delays = {"Rlag": ("R", "tau")}

    def rhs(self, t, y, p, c):
        x, r = y
        return [p.r * x * (1.0 - x / p.cap), _feedback(p, self.delayed.Rlag) - p.gamma * r]


class DelayedRepressorFrozen(_Repressor):
    """The twin without a delay: R(t_0), the initial-state parameter, in place of the read."""
    model_key = "gen_delayed_repressor_frozen"

    def rhs(self, t, y, p, c):
        x, r = y
        return [p.r * x * (1.0 - x / p.cap), _feedback(p, p.r0) - p.gamma * r]


class DelayedRepressorTreated(_Repressor):
    """The timing probe's twin: the read is a constant treatment (a class without `delays`: the parent's kernels)."""
    model_key = "gen_delayed_repressor_treated"
    n_conditions = 1

    def rhs(self, t, y, p, c):
        x, r = y
        return [p.r * x * (1.0 - x / p.cap), _feedback(p, c[0]) - p.gamma * r]


class TwoDelays(GeneratedOdeModel):
    """A relay: the sender S is driven by a forcing and by the receiver's past, the receiver Q by the sender's past; Q's lag is
    twice S's, shared through prepare."""
    model_key = "gen_two_delays"
    species = ["OD", "S", "Q", "F"]
    parameters = ["r", "cap", "a", "b", "ds", "dq", "tau", "init_x", "init_s", "init_q", "init_f"]
    observe_kind = "direct"
    forcings = ["light"]
    delays = {"Slag": ("S", "tau2"), "Qlag": ("Q", "tau")}

    def __init__(self, config):
        super(TwoDelays, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": th.r, "cap": th.cap, "a": th.a, "b": th.b, "ds": th.ds, "dq": th.dq, "tau": th.tau, "tau2": 2.0 * th.tau}

    def initial_state(self, th, c):
        return [th.init_x, th.init_s, th.init_q, th.init_f]

    def rhs(self, t, y, p, c):
        x, s, q, f = y
        slag, qlag = self.delayed.Slag, self.delayed.Qlag
        return [p.r * x * (1.0 - x / p.cap),
                p.a * self.forcing.light / (1.0 + qlag) - p.ds * s,
                p.b * slag - p.dq * q,
                slag * qlag - 0.3 * f]


class DelayedStart(_Repressor):
    """A delayed read in a class with a start map: the history before t_0 is the state after start."""
    model_key = "gen_delayed_start"
    delays = {"Rlag": ("R", "tau")}

    def start(self, y, p, c):
        return [y[0], y[1] + p.beta / (p.gamma + p.K)]

    def rhs(self, t, y, p, c):
        x, r = y
        return [p.r * x * (1.0 - x / p.cap), _feedback(p, self.delayed.Rlag) - p.gamma * r]


MODELS = [DelayedRepressor, TwoDelays, DelayedStart]
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(DelayedRepressor, False), (DelayedRepressorFrozen, False), (TwoDelays, False), (DelayedStart, False),
            (DelayedRepressorTreated, False)]

REPRESSOR_BASE = {"r": 1.0, "cap": 2.0, "beta": 1.5, "K": 0.4, "gamma": 0.6, "tau": 0.5, "gain": 1.3, "init_x": 0.05,
                  "init_r": 0.3, "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
TWO_BASE = {"r": 1.0, "cap": 2.0, "a": 1.2, "b": 0.9, "ds": 0.5, "dq": 0.4, "tau": 0.3, "init_x": 0.05, "init_s": 0.2,
            "init_q": 0.1, "init_f": 0.1, "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
BASES = {DelayedRepressor: REPRESSOR_BASE, DelayedRepressorFrozen: REPRESSOR_BASE, DelayedRepressorTreated: REPRESSOR_BASE,
         DelayedStart: REPRESSOR_BASE, TwoDelays: TWO_BASE}
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def history(xs, times, k, species, s, tau):
    """H(s) of interval k for one read: xs the states so far [>= k+1 entries of [B,S,N]], s [B,S].  The constant history
    y(t_0) for s <= t_0, else the linear interpolant of the stored points 0 .. k, its interval index clamped into [0, k-1];
    NaN where the delay is not finite."""
    y0 = xs[0][:, :, species]
    val = y0
    if k > 0:
        Y = torch.stack([x[:, :, species] for x in xs[:k + 1]])  # [k+1, B, S]
        tg = times[:k].contiguous()  # t_0 .. t_k-1
        j = (torch.searchsorted(tg, s.detach().contiguous(), right=True) - 1).clamp(0, k - 1)
        tj, tj1 = times[j], times[j + 1]
        yj, yj1 = Y.gather(0, j[None])[0], Y.gather(0, (j + 1)[None])[0]
        w = (s - tj) / (tj1 - tj)
        val = torch.where(s > times[0], yj + w * (yj1 - yj), y0)
    return torch.where(torch.isfinite(tau), val, torch.full_like(val, float("nan")))


def interval_ends(times, k, tau):
    """(s_lo, s_hi, taue) of interval k."""
    taue = torch.clamp(tau, min=0.0)
    return times[k] - taue, torch.minimum(times[k + 1] - taue, times[k].expand_as(taue)), taue


def simulate(rhs, x0, times, solver):
    """The fixed-grid schemes of oracle.vihds_oracle with the delayed reads of `rhs.delays`: [T, B, S, N]."""
    xs = [x0]
    h0 = times[1] - times[0]
    step = {"euler": O._euler_step, "midpoint": O._midpoint_step, "rk4": O._rk4_38_step}
    for k in range(len(times) - 1):
        t0, t1 = times[k], times[k + 1]
        chords = []
        for species, tau in rhs.delays:
            s_lo, s_hi, _ = interval_ends(times, k, tau)
            d_lo, d_hi = history(xs, times, k, species, s_lo, tau), history(xs, times, k, species, s_hi, tau)
            chords.append((d_lo, (d_hi - d_lo) / (t1 - t0)))

        def f(t, y, _c=chords, _t0=t0):
            return rhs(t, y, delayed=[lo + (t - _t0) * sl for lo, sl in _c])

        y = xs[-1]
        if solver in ("modeuler", "modeulerwhile"):
            h = h0 if solver == "modeuler" else t1 - t0
            f1 = f(t0, y)
            f2 = f(t1, y + h * f1)
            y = y + 0.5 * h * (f1 + f2)
        else:
            y = y + step[solver](f, t0, t1 - t0, y)
        xs.append(y)
    return torch.stack(xs)


def smooth_series(B, times):
    t = torch.as_tensor(times, dtype=torch.float64)
    return 1.0 + 0.5 * torch.sin(0.9 * t[None, :] + 0.7 * torch.arange(B, dtype=torch.float64)[:, None])


def forward(cls, th, cond, times, solver, obs=None):
    """The definition in th's dtype: species [B,S,N,T], x_predict [B,S,4,T] and, given observations, the per-signal
    log-likelihood [B,S,4] under the constant precisions."""
    kw = {"times": times} if cls.forcings else {}
    rhs, x0 = cls.torch_problem(th, cond, None, **kw)
    if cls.delays:
        xs = simulate(rhs, x0, times, solver).permute(1, 2, 3, 0)
    else:
        xs = O.simulate(rhs, x0, times, solver)
    xp = cls.torch_observe(xs, th, cond) if cls._observe_def is not None else O.observe_direct(xs)
    if obs is None:
        return xs, xp, None
    prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    return xs, xp, O.log_prob_observations(xp, obs, prec)


def delay_margin(taue, tt):
    """Per element of taue (>= 0): the distance of every s_lo and every unclamped s_hi to a grid point (to t_0 where the lookup is
    the constant history), of taue to each step length and to 0, in units of the local step -- the kinks of the tau gradient."""
    steps = tt[1:] - tt[:-1]
    out = taue / steps.min()
    right, left = torch.cat([steps, steps[-1:]]), torch.cat([steps[:1], steps])
    for k in range(len(tt) - 1):
        out = torch.minimum(out, (taue - steps[k]).abs() / steps[k])
        unclamped = (tt[k + 1] - taue) < tt[k]
        for s, use in ((tt[k] - taue, torch.ones_like(unclamped)), (tt[k + 1] - taue, unclamped)):
            d = (s[..., None] - tt).abs()
            rel = (d / torch.where(s[..., None] >= tt, right, left)).min(dim=-1).values
            rel = torch.where(s > tt[0], rel, (s - tt[0]).abs() / steps[0])
            out = torch.where(use, torch.minimum(out, rel), out)
    return out


def tau_values(B, S, times, seed, factors=(1.0,), margin=4e-3):
    """The delays of a case [B,S]: the four classes of the grid's step lengths in turn along the samples -- below the smallest
    step, between the smallest and the largest, above the largest, above the whole span -- each with a random factor.  A draw
    whose delay (times each of `factors`: the delays a class derives from it) sits within `margin` of the local step of a kink
    of the tau gradient is drawn again: precondition (b) of the GPU comparisons, arranged here on the CPU."""
    gen = torch.Generator().manual_seed(1000 + seed)
    tt = torch.as_tensor(list(times), dtype=torch.float64)
    steps = tt[1:] - tt[:-1]
    lo, hi, span = float(steps.min()), float(steps.max()), float(tt[-1] - tt[0])
    kind = (torch.arange(S)[None, :] + torch.arange(B)[:, None]) % 4
    if hi > lo:
        bands = [(0.25 * lo, 0.9 * lo), (1.1 * lo, 0.9 * hi), (1.1 * hi, 0.9 * span), (1.1 * span, 1.5 * span)]
    else:  # (one step: T = 2 -- below it, and above the span)
        bands = [(0.25 * lo, 0.9 * lo), (0.3 * lo, 0.8 * lo), (1.1 * span, 1.3 * span), (1.1 * span, 1.5 * span)]

    def draw():
        u = torch.rand(B, S, generator=gen, dtype=torch.float64)
        v = torch.zeros(B, S, dtype=torch.float64)
        for q, (a, b) in enumerate(bands):
            v = torch.where(kind == q, a + (b - a) * u, v)
        return v

    out = draw()
    for _ in range(200):
        bad = torch.zeros(B, S, dtype=torch.bool)
        for f in factors:
            bad |= delay_margin(f * out, tt) < margin
        if not bool(bad.any()):
            return out
        out = torch.where(bad, draw(), out)
    raise RuntimeError("no delays away from the kinks found")


def problem(cls, B, S, times=RAGGED, seed=11, tau=None):
    """Inputs of one case (shared by the tests that use it; never modified)."""
    k = (cls, B, S, tuple(times), seed, None if tau is None else float(tau))
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    th = {n: v * torch.exp(0.2 * rnd(B, S)) for n, v in BASES[cls].items()}
    if tau is not None:
        th["tau"] = torch.full((B, S), float(tau), dtype=torch.float64)
    elif cls is TwoDelays:  # (Slag reads 2 tau: the classes of tau_values are those of the longer lag)
        th["tau"] = 0.5 * tau_values(B, S, times, seed, factors=(1.0, 0.5))
    else:
        th["tau"] = tau_values(B, S, times, seed)
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = smooth_series(B, tt)[:, None, :] if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    cond = torch.cat([torch.log1p(treatments).reshape(B, -1), series.reshape(B, -1)], dim=1)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        _, xp, _ = forward(cls, th1, cond, tt, "rk4")
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "times": tt, "obs": obs, "B": B, "S": S, "T": T,
          # the upstream gradient of the log-likelihood: one sign, so that the loss sum(logp * G) is a well-conditioned sum (the
          # GPU tests bound it relative to its own size in float32 and assert the condition number on the float64 run)
          "G": {"logp": 0.5 + torch.rand(B, S, 4, generator=gen, dtype=torch.float64)}}
    _PROBLEMS[k] = pb
    return pb


def kink_margins(cls, pb):
    """Precondition (b) on the float64 inputs alone: the smallest delay_margin over the reads of the class as prepare hands the
    delays out; and the classes of the delays met (a): below the smallest step, between the smallest and the largest, above the
    largest, above the whole span."""
    tt = pb["times"]
    steps = tt[1:] - tt[:-1]
    rhs, _ = cls.torch_problem(pb["th"], pb["cond"], None, **({"times": tt} if cls.forcings else {}))
    smallest, classes = float("inf"), set()
    edges = [0.0, float(steps.min()), float(steps.max()), float(tt[-1] - tt[0]), float("inf")]
    for _sp, tau in rhs.delays:
        taue = torch.clamp(tau, min=0.0)
        smallest = min(smallest, float(delay_margin(taue, tt).min()))
        classes |= {q for q in range(4) if bool(((taue > edges[q]) & (taue < edges[q + 1])).any())}
    return smallest, classes
