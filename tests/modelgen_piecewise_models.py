"""Models with piecewise terms (where, minimum, maximum, abs, sqrt, erf, erfc of vihds.modelgen) for the tests: a small model
that uses every one of them in each of its five functions, the plate reader with a detector ceiling and a censored (Tobit)
likelihood, and the prpr_constant restatement with a production term that is switched on at a time given as a treatment.

Switch margins.  A float32 kernel and a float64 yardstick agree only where they take the same branches, so the models do not
compare with `<` directly: every comparison, every minimum / maximum and every abs goes through `sw` below.  On symbols
(tracing) and on float32 tensors it is the plain operation; on float64 tensors inside `recording()` it also notes the margin
|lhs - rhs| / (|lhs| + |rhs| + 1) of the switch at every point it is evaluated -- every stage of every step for rhs, every time
point for the three maps -- so a test reads the smallest margin of its yardstick's own trajectory (Margins.smallest, and per
trajectory Margins.per_trajectory [B, S]) instead of deriving the expressions again."""
import contextlib
import math

import torch

from oracle import vihds_oracle as O
from vihds import modelgen as G
from vihds.modelgen import GeneratedOdeModel, erf, erfc, log, sqrt, where

from modelgen_models import PrprRestated
from modelgen_noise_models import PlateReaderNoise
from modelgen_observe_models import PlateReader

LOG2PI = math.log(2.0 * math.pi)
SQRT1_2 = math.sqrt(0.5)
MARGIN = 1e-3  # the precondition of every numeric comparison: 100 x the 1e-5 forward tolerance


class Margins(object):
    """What recording() collects: the smallest margin per switch label, and per trajectory [B, S] over all labels."""

    def __init__(self):
        self.by_label, self.per_trajectory = {}, None

    @property
    def smallest(self):
        return min(self.by_label.values())

    def note(self, label, a, b):
        a = a if isinstance(a, torch.Tensor) else torch.tensor(float(a), dtype=torch.float64)
        b = b if isinstance(b, torch.Tensor) else torch.tensor(float(b), dtype=torch.float64)
        if a.dtype != torch.float64 and b.dtype != torch.float64:
            return
        m = ((a - b).abs() / (a.abs() + b.abs() + 1.0)).detach().double()
        m = torch.where(torch.isnan(m), torch.full_like(m, float("inf")), m)  # (a trajectory that is NaN takes no branch)
        self.by_label[label] = min(self.by_label.get(label, float("inf")), float(m.min()))
        while m.dim() > 2:  # ([B, S, T] of the three maps)
            m = m.amin(dim=-1)
        if m.dim() == 2:
            self.per_trajectory = m.clone() if self.per_trajectory is None else torch.minimum(self.per_trajectory, m)


_ACTIVE = []


@contextlib.contextmanager
def recording():
    m = Margins()
    _ACTIVE.append(m)
    try:
        yield m
    finally:
        _ACTIVE.pop()


class _Switches(object):
    """The operations that switch, with their margins noted (module docstring)."""

    @staticmethod
    def _note(label, a, b):
        if _ACTIVE and (isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor)):
            _ACTIVE[-1].note(label, a, b)

    def lt(self, label, a, b):
        self._note(label, a, b)
        return a < b

    def gt(self, label, a, b):
        self._note(label, a, b)
        return a > b

    def ge(self, label, a, b):
        self._note(label, a, b)
        return a >= b

    def minimum(self, label, a, b):
        self._note(label, a, b)
        return G.minimum(a, b)

    def maximum(self, label, a, b):
        self._note(label, a, b)
        return G.maximum(a, b)

    def abs(self, label, x):
        self._note(label, x, 0.0)
        return G.abs(x)


sw = _Switches()
T_LATE = 3.45  # (a constant switch time of EveryPiecewiseOperation: off every stage time of tests' grids)


def _tobit(x, ob, pr, ceil, label):
    """A reading at or above the ceiling says only that the signal was at least there: the Gaussian's tail mass above the
    ceiling; below it, the Gaussian density.  The tail is formed from a z that is 0 where the reading is not censored (the
    double-where idiom of the module docstring of vihds.modelgen): erfc underflows to 0 a dozen standard deviations below the
    ceiling, and the logarithm's adjoint there would be 0 * inf."""
    censored = sw.ge(label, ob, ceil)
    z = where(censored, (ceil - x) * sqrt(pr), 0.0)
    return where(censored, log(0.5 * erfc(z * SQRT1_2)), -0.5 * (LOG2PI - log(pr) + pr * (x - ob) * (x - ob)))


class EveryPiecewiseOperation(GeneratedOdeModel):
    """Every piecewise operation, in prepare (accurate maths) and in the four time-loop functions: a substrate that is dosed
    from time tau on (a condition on t against a parameter) and taken up at a saturating rate (minimum of two model
    quantities), a product whose extra source `boost` exists only late and above a density threshold (nested where, a
    condition between a species and a parameter: `boost` is read in that one branch), a square-root sink, a detector with a
    ceiling and a floor, shot noise in |signal|, and a likelihood that is censored at the ceiling and truncated at zero."""
    model_key = "gen_every_piecewise_operation"
    species = ["OD", "S", "P", "Q"]
    parameters = ["r", "K", "tau", "dose", "vmax", "km", "thr", "boost", "q", "ceil", "floor", "s0", "s1", "init_x", "init_s"]
    n_conditions = 1

    def prepare(self, th, c):
        return {"r": sw.maximum("prepare r", th.r, 0.3), "K": sqrt(sw.abs("prepare K", th.K)) + 1.0, "tau": th.tau,
                "dose": where(sw.lt("prepare c", c[0], 1.0), th.dose, 0.5 * th.dose + 0.1 * erf(th.dose)),
                "vmax": th.vmax, "km": th.km, "thr": th.thr, "boost": th.boost, "q": th.q,
                "ceil": sw.minimum("prepare ceil", th.ceil, 10.0 * erfc(th.ceil - 3.0)), "floor": th.floor, "s0": th.s0,
                "s1": th.s1}

    def initial_state(self, th, c):
        return [th.init_x, th.init_s, 0.1, 0.5]

    def rhs(self, t, y, p, c):
        x, s, pr, q = y
        early = sw.lt("rhs t < tau", t, p.tau)
        dense = sw.gt("rhs x > thr", x, p.thr)
        gate = (~early & dense) | sw.gt("rhs t > T_LATE", t, T_LATE)
        u = where(early, 0.0, p.dose)
        uptake = sw.minimum("rhs uptake", p.km * s, p.vmax)
        extra = where(early, 0.0, where(dense, p.boost * x, 0.1 * x))
        root = sqrt(p.q + pr)  # (NaN for q + P < 0, and from there on)
        return [p.r * (1.0 - x / p.K) * x,
                u - uptake - 0.3 * s,
                uptake + extra - 0.4 * pr * where(gate, 0.5, 1.0),
                sw.maximum("rhs root", root, 0.05) - 0.6 * q - 0.2 * sw.abs("rhs |S - P|", s - pr)]

    def observe(self, y, p, c):
        x, s, pr, q = y
        return [x,
                sw.minimum("observe ceiling", x * pr * 4.0, p.ceil),
                sw.maximum("observe floor", x * s, p.floor),
                where(sw.gt("observe q > s", q, s) & ~sw.gt("observe c", c[0], 1.0), sqrt(x * q), x * q)]

    def precision(self, y, x, p, c):
        shot = lambda j: 1.0 / (p.s0 * p.s0 + p.s1 * p.s1 * sw.abs("precision |x%d|" % j, x[j]))  # noqa: E731
        return [shot(0), shot(1), shot(2),
                where(sw.gt("precision x3", x[3], 0.3), shot(3), 1.0 / (p.s0 * p.s0 + 0.3 * p.s1 * p.s1))]

    def log_likelihood(self, x, obs, pr, p, c):
        gauss = lambda j: -0.5 * (LOG2PI - log(pr[j]) + pr[j] * (x[j] - obs[j]) * (x[j] - obs[j]))  # noqa: E731
        return [gauss(0), _tobit(x[1], obs[1], pr[1], p.ceil, "log_likelihood obs1 >= ceil"),
                # truncated at zero: the Gaussian over the mass it has above 0
                gauss(2) - log(0.5 * (1.0 + erf(x[2] * sqrt(pr[2]) * SQRT1_2))),
                gauss(3)]


class PlateReaderCensored(PlateReaderNoise):
    """PlateReaderNoise whose detector saturates: the three fluorescence signals are cut at the parameter `ceil`, and their
    likelihood is Tobit -- the tail mass above the ceiling for a reading at the ceiling, the Gaussian density below."""
    model_key = "gen_plate_reader_censored"
    parameters = PlateReaderNoise.parameter_names + ["ceil"]

    def prepare(self, th, c):
        p = PlateReaderNoise.prepare(self, th, c)
        p["ceil"] = th.ceil
        return p

    def observe(self, y, p, c):
        xp = PlateReader._observe_def(self, y, p, c)
        return [xp[0]] + [sw.minimum("observe ceiling %d" % j, xp[j], p.ceil) for j in (1, 2, 3)]

    def log_likelihood(self, x, obs, pr, p, c):
        return [-0.5 * (LOG2PI - log(pr[0]) + pr[0] * (x[0] - obs[0]) * (x[0] - obs[0]))] + [
            _tobit(x[j], obs[j], pr[j], p.ceil, "log_likelihood obs%d >= ceil" % j) for j in (1, 2, 3)]


class PrprDosed(PrprRestated):
    """PrprRestated with YFP production switched on at a time that is a treatment (an inducer added at hour c[0]): the
    switch time differs per data row."""
    model_key = "gen_prpr_constant_dosed"
    n_conditions = 1

    def rhs(self, t, y, p, c):
        x, rfp, yfp, cfp, f530, f480 = y
        gamma = p.r * G.sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        return [gamma * x,
                p.rc - (gamma + p.drfp) * rfp,
                p.rc * p.aYFP * where(sw.lt("rhs t < c0", t, c[0]), 0.0, 1.0) - (gamma + p.dyfp) * yfp,
                p.rc * p.aCFP - (gamma + p.dcfp) * cfp,
                p.rc * p.a530 - gamma * f530,
                p.rc * p.a480 - gamma * f480]


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(EveryPiecewiseOperation, False), (PlateReaderCensored, False), (PrprDosed, False)]


# ---- inputs of the numeric tests: chosen on the float64 yardstick alone ------------------------------------------------------
FIXED = ["modeuler", "modeulerwhile", "euler", "midpoint", "rk4"]
TIMES = [0.0, 0.3, 0.7, 1.0, 1.6, 2.0, 2.6, 3.1, 3.7]  # T = 9, steps 0.3 .. 0.6
EVERY_BASE = {"r": 1.2, "K": 2.0, "tau": 1.8, "dose": 1.5, "vmax": 0.6, "km": 1.0, "thr": 0.5, "boost": 0.8, "q": 0.5,
              "ceil": 1.5, "floor": 0.15, "s0": 0.2, "s1": 0.15, "init_x": 0.1, "init_s": 0.4}
EVERY_TREATMENT = [0.6, 1.7, 0.3]  # c[0] of the three data rows: both sides of the 1.0 that prepare and observe compare with
PRPR_DOSED_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP_PR": 1.2,
                   "aCFP_PR": 0.9, "a530": 0.4, "a480": 0.3, "init_x": 0.01, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
                   "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
# the hour the inducer is added to each data row: off every grid time of TIMES and every stage time between them (halves,
# thirds); the last row is dosed after the end, so its production stays off
PRPR_DOSED_SWITCH = [1.34, 2.35, 4.2]
POOL = 16  # candidates drawn per sample that is kept
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else ["prec_x", "prec_rfp", "prec_yfp", "prec_cfp"])


def forward(cls, th, cond, times, solver, obs=None, grid=None):
    """The float64 (or float32) definition: species [B,S,N,T], x_predict [B,S,4,T], precisions [B,S,4,T] and, given
    observations, the per-signal log-likelihood [B,S,4]."""
    rhs, x0 = cls.torch_problem(th, cond)
    xs = O.simulate(rhs, x0, times, solver, **({"grid": grid} if grid is not None else {}))
    xp = cls.torch_observe(xs, th, cond) if cls._observe_def is not None else O.observe_default(xs)
    if cls._precision_def is not None:
        prec = cls.torch_precision(xs, th, cond)
    else:
        prec = torch.stack([th[n] for n in slot_names(cls)[-4:]], dim=2)[:, :, :, None].expand_as(xp)
    if obs is None:
        return xs, xp, prec, None
    if cls._likelihood_def is not None:
        logp = cls.torch_log_likelihood(xp, obs, prec, th, cond).sum(3)
    else:
        logp = O.log_prob_observations(xp, obs, prec)
    return xs, xp, prec, logp


def _candidates(cls, B, n, gen):
    base = EVERY_BASE if cls is EveryPiecewiseOperation else PRPR_DOSED_BASE
    th = {k: v * torch.exp(0.2 * torch.randn(B, n, generator=gen, dtype=torch.float64)) for k, v in base.items()}
    if cls is EveryPiecewiseOperation:
        # the dosing time from before the first step to past the end of the grid: a trajectory dosed after TIMES[-1] never
        # reaches the branch that reads `boost`
        th["tau"] = 0.4 + 4.2 * torch.rand(B, n, generator=gen, dtype=torch.float64)
    return th


def problem(cls, B, S):
    """Inputs of one case for EveryPiecewiseOperation or PrprDosed (shared by the tests that use it; never modified): theta
    [B,S] per slot, treatments, times, observations and upstream gradients.  POOL * S candidates are drawn per data row and
    the first S kept whose float64 trajectory keeps every switch at least 2 * MARGIN wide under every fixed-grid solver --
    a property of the inputs, decided by the float64 definition alone; the tests assert MARGIN on what was kept."""
    k = (cls, B, S)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    assert B == 3
    gen = torch.Generator().manual_seed(11)
    n = POOL * S
    th = _candidates(cls, B, n, gen)
    c = torch.tensor(EVERY_TREATMENT if cls is EveryPiecewiseOperation else PRPR_DOSED_SWITCH, dtype=torch.float64)
    cond = torch.log1p(c)[:, None]
    times = torch.tensor(TIMES, dtype=torch.float64)
    T = times.shape[0]
    with torch.no_grad():
        th1 = {name: v[:, :1] for name, v in th.items()}
        _, xp, prec, _ = forward(cls, th1, cond, times, "rk4")
        obs = xp[:, 0] * (1.0 + 0.05 * torch.randn(B, 4, T, generator=gen, dtype=torch.float64))
        if cls is EveryPiecewiseOperation:
            # a detector that saturates: readings of the censored signal above 1.3 are reported as 2.0 -- above every sampled
            # ceiling (1.5 e^{0.2 z}), so the likelihood's censored branch is taken by them and by nothing else
            obs[:, 1] = torch.where(obs[:, 1] > 1.3, torch.full_like(obs[:, 1], 2.0), obs[:, 1].clamp_max(0.8))
        keep = torch.ones(B, n, dtype=torch.bool)
        for solver in FIXED:
            with recording() as m:
                forward(cls, th, cond, times, solver, obs)
            if m.per_trajectory is not None:
                keep &= m.per_trajectory >= 2.0 * MARGIN
    assert int(keep.sum(1).min()) >= S, "too few candidates keep their switches wide: %s of %d" % (keep.sum(1).tolist(), n)
    pick = torch.stack([torch.nonzero(keep[b])[:S, 0] for b in range(B)])
    N = len(cls.species)
    rows = N + (4 if cls._precision_def is not None else 0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    pb = {"th": {name: v.gather(1, pick) for name, v in th.items()}, "cond": cond, "times": times, "obs": obs, "B": B, "S": S,
          "T": T, "G": {"logp": rnd(B, S, 4), "xpred": rnd(B, S, 4, T), "traj": rnd(B, S, rows, T)}}
    _PROBLEMS[k] = pb
    return pb
