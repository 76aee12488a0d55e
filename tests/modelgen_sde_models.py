"""Models with process noise (the `diffusion` hook of vihds.modelgen) for the tests, and the float64 yardstick of the scheme.

Brownian8: eight species, rhs = 0, diffusion = 1, zero initial state and a jump that returns zeros -- on a grid of unit steps the
state stored at point k + 1 is exactly the draw xi_k: this is how the tests read the kernel's own draws.  OrnsteinUhlenbeck:
additive noise with a known variance recursion.  PrprLangevin: prpr_constant restated (tests/modelgen_models.py) plus
sigma * sqrt(max(y, 0)) on OD and RFP and 0 on the rest.  LightSub4: substeps = 4 and a forcing.  DilutedHooked: an observation
map of its own and a jump.

The yardstick (`forward`) is the definition of csrc/vihds_sde.hpp in plain torch: u' = Phi_h(u) + g(u) sqrt(h) xi per step, with
the schemes of oracle.vihds_oracle, g from torch_diffusion and the draws xi passed in as an argument."""
import torch

from oracle import vihds_oracle as O
from vihds.modelgen import GeneratedOdeModel, clamp, maximum, sigmoid, sqrt
from vihds.precisions import ConstantPrecisions

from modelgen_models import PREC, PrprRestated
from modelgen_piecewise_models import FIXED  # noqa: F401  (the five fixed-grid solvers, for the tests)

RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # the grid of tests/test_modelgen_forcing_gpu.py: steps 0.1 .. 1.0


class Brownian8(GeneratedOdeModel):
    """The probe of the kernel's draws: on a unit grid the state stored at point k + 1 is xi_k."""
    model_key = "gen_sde_brownian8"
    species = ["W0", "W1", "W2", "W3", "W4", "W5", "W6", "W7"]
    parameters = ["unused"]
    observe_kind = "direct"

    def __init__(self, config):
        super(Brownian8, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"unused": th.unused}

    def initial_state(self, th, c):
        return [0.0] * 8

    def rhs(self, t, y, p, c):
        return [0.0] * 8

    def jump(self, y, p, c):
        return [0.0] * 8

    def diffusion(self, y, p, c):
        return [1.0] * 8


class OrnsteinUhlenbeck(GeneratedOdeModel):
    """dX = -a X dt + sigma dW on four species: additive noise."""
    model_key = "gen_sde_ornstein_uhlenbeck"
    species = ["X0", "X1", "X2", "X3"]
    parameters = ["a", "sigma", "init"]
    observe_kind = "direct"

    def __init__(self, config):
        super(OrnsteinUhlenbeck, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"a": th.a, "sigma": th.sigma}

    def initial_state(self, th, c):
        return [th.init, th.init, th.init, th.init]

    def rhs(self, t, y, p, c):
        return [-p.a * v for v in y]

    def diffusion(self, y, p, c):
        return [p.sigma, p.sigma, p.sigma, p.sigma]


class PrprLangevin(PrprRestated):
    """prpr_constant restated, with demographic noise on the culture density and on RFP."""
    model_key = "gen_sde_prpr_langevin"
    parameters = list(PrprRestated.parameter_names) + ["sigma"]

    def prepare(self, th, c):
        return dict(PrprRestated.prepare(self, th, c), sigma=th.sigma)

    def diffusion(self, y, p, c):
        return [p.sigma * sqrt(maximum(y[0], 0.0)), 0.5 * p.sigma * sqrt(maximum(y[1], 0.0)), 0.0, 0.0, 0.0, 0.0]


class LightSub4(GeneratedOdeModel):
    """Four sub-steps per interval and a forcing: a light-driven reporter in a growing culture, noise on reporter and maturation."""
    model_key = "gen_sde_light_sub4"
    species = ["OD", "P", "M", "D"]
    parameters = ["r", "cap", "a", "km", "dp", "sigma", "init_x", "init_p"]
    observe_kind = "direct"
    forcings = ["light"]
    substeps = 4

    def __init__(self, config):
        super(LightSub4, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "cap": th.cap, "a": th.a, "km": th.km, "dp": th.dp, "sigma": th.sigma}

    def initial_state(self, th, c):
        return [th.init_x, th.init_p, 0.5 * th.init_p, 0.1]

    def rhs(self, t, y, p, c):
        x, q, m, d = y
        g = p.r * (1.0 - x / p.cap)
        return [g * x, p.a * self.forcing.light - (p.km + p.dp + g) * q, p.km * q - (p.dp + g) * m, 0.3 * sigmoid(t) - 0.2 * d]

    def diffusion(self, y, p, c):
        # (the amplitude of P scales with the light of the interval's first point: a forcing read in the hook)
        return [0.0, p.sigma * self.forcing.light * sqrt(maximum(y[1], 0.0)), p.sigma * y[2], 0.0]


class DilutedHooked(GeneratedOdeModel):
    """An observation map of its own and a dilution at every read; multiplicative noise on the density and the product."""
    model_key = "gen_sde_diluted_hooked"
    species = ["OD", "A", "B"]
    parameters = ["r", "cap", "k", "d", "keep", "gain", "sigma", "init_x", "init_a"]

    def __init__(self, config):
        super(DilutedHooked, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "cap": th.cap, "k": th.k, "d": th.d, "keep": th.keep, "gain": th.gain, "sigma": th.sigma}

    def initial_state(self, th, c):
        return [th.init_x, th.init_a, 0.2]

    def rhs(self, t, y, p, c):
        x, a, b = y
        return [p.r * x * (1.0 - x / p.cap), p.k * x - p.d * a, p.d * a - 0.5 * b]

    def observe(self, y, p, c):
        return [y[0], p.gain * y[1], y[2] / (1.0 + y[2]), y[0] * y[1]]

    def jump(self, y, p, c):
        return [p.keep * y[0], y[1], p.keep * y[2]]

    def diffusion(self, y, p, c):
        return [p.sigma * y[0], p.sigma * sqrt(maximum(y[1], 0.0)), 0.0]


PARITY = [PrprLangevin, LightSub4, DilutedHooked]
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(Brownian8, False), (OrnsteinUhlenbeck, False), (PrprLangevin, False), (LightSub4, False), (DilutedHooked, False)]

_P = {"prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
BASES = {
    Brownian8: dict(_P, unused=1.0),
    OrnsteinUhlenbeck: dict(_P, a=0.8, sigma=0.5, init=1.0),
    PrprLangevin: dict(_P, r=1.0, K=2.0, tlag=1.0, rc=1.0, drfp=0.3, dyfp=0.3, dcfp=0.3, aYFP_PR=0.8, aCFP_PR=0.6, a530=0.1,
                       a480=0.1, init_x=0.1, init_rfp=0.5, init_yfp=0.4, init_cfp=0.3, sigma=0.08),
    LightSub4: dict(_P, r=1.0, cap=2.0, a=1.2, km=0.7, dp=0.3, sigma=0.15, init_x=0.1, init_p=0.5),
    DilutedHooked: dict(_P, r=1.2, cap=2.0, k=0.9, d=0.5, keep=0.85, gain=1.3, sigma=0.1, init_x=0.2, init_a=0.4),
}
KEY = (0x5eed01, 0x0c0ffe)  # the noise key of the shared problems: two words below 2^24
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def n_steps(cls, T):
    """The steps a trajectory of T points draws for: (T - 1) * substeps."""
    return (T - 1) * int(cls.substeps)


def noisy_species(cls):
    """Indices of the species with an amplitude that is not the constant 0 (the struct's NOISE_MASK)."""
    return [j for j, e in enumerate(cls._trace.dif) if not (e.op == "const" and e.val == 0.0)]


def smooth_series(B, times):
    t = torch.as_tensor(times, dtype=torch.float64)
    return 1.0 + 0.5 * torch.sin(0.9 * t[None, :] + 0.7 * torch.arange(B, dtype=torch.float64)[:, None])


def _column(hook, y, k, T, th, cond):
    """A per-time-point hook (torch_jump / torch_diffusion) on the state y [B,S,N] with the forcing samples of point k."""
    return hook(y.unsqueeze(-1).expand(y.shape + (T,)), th, cond)[..., k]


def _scheme_step(rhs, solver, s0, s1, h_fixed, y):
    """One step of the fixed-grid scheme and the length h it advances by (oracle.vihds_oracle's steps)."""
    if solver in ("modeuler", "modeulerwhile"):
        h = h_fixed if solver == "modeuler" else s1 - s0
        f1 = rhs(s0, y)
        f2 = rhs(s1, y + h * f1)
        return y + 0.5 * h * (f1 + f2), h
    step = {"euler": O._euler_step, "midpoint": O._midpoint_step, "rk4": O._rk4_38_step}[solver]
    return y + step(rhs, s0, s1 - s0, y), s1 - s0


def forward(cls, th, cond, times, solver, obs, xi, starts=None):
    """The definition in th's dtype: species [B,S,N,T], x_predict [B,S,4,T] and, given observations, the per-signal
    log-likelihood [B,S,4] under the constant precisions.  xi [B,S,>=N,(T-1)*substeps]: the draws, species q of step
    k * substeps + j; cond as the kernels take it (the two key columns last; they are not read here).  starts: a list that
    receives the start state [B,S,N] of every step, sub-steps included -- where the amplitudes are evaluated."""
    kw = {"times": times} if cls.forcings else {}
    rhs, y = cls.torch_problem(th, cond, None, **kw)
    N, T, m = len(cls.species), int(times.shape[0]), int(cls.substeps)
    xi = xi.to(y.dtype)
    h0 = (times[1] - times[0]) / m
    xs = [y]
    for k in range(T - 1):
        if cls._jump_def is not None:
            y = _column(cls.torch_jump, y, k, T, th, cond)
        t0, t1 = times[k], times[k + 1]
        hs = (t1 - t0) / m
        for j in range(m):
            s0, s1 = t0 + j * hs, (t1 if j == m - 1 else t0 + (j + 1) * hs)
            if starts is not None:
                starts.append(y.detach())
            g = _column(cls.torch_diffusion, y, k, T, th, cond)
            y, h = _scheme_step(rhs, solver, s0, s1, h0, y)
            y = y + g * (torch.sqrt(h) * xi[:, :, :N, k * m + j])
        xs.append(y)
    xs = torch.stack(xs, dim=-1)
    if cls._observe_def is not None:
        xp = cls.torch_observe(xs, th, cond)
    else:
        xp = O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)
    if obs is None:
        return xs, xp, None
    prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    return xs, xp, O.log_prob_observations(xp, obs, prec)


def problem(cls, B, S, times=RAGGED, seed=17, key=KEY):
    """Inputs of one case (shared by the tests that use it; never modified).  cond is [treatments | forcing samples | key]."""
    k = (cls, B, S, tuple(times), seed, tuple(key))
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    th = {n: v * torch.exp(0.1 * rnd(B, S)) for n, v in BASES[cls].items()}
    series = smooth_series(B, tt)[:, None, :] if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    keys = torch.tensor([float(key[0]), float(key[1])], dtype=torch.float64)[None, :].expand(B, 2)
    cond = torch.cat([series.reshape(B, -1), keys], dim=1)
    with torch.no_grad():  # observations: the noise-free trajectory of the first sample, 5 % multiplicative scatter
        th1 = {n: v[:, :1] for n, v in th.items()}
        zero = torch.zeros(B, 1, len(cls.species), n_steps(cls, T), dtype=torch.float64)
        _, xp, _ = forward(cls, th1, cond, tt, "rk4", None, zero)
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "times": tt, "obs": obs, "B": B, "S": S, "T": T, "key": tuple(key),
          # the upstream gradient of the log-likelihood: one sign, so that the loss sum(logp * G) is a well-conditioned sum
          "G": {"logp": 0.5 + torch.rand(B, S, 4, generator=gen, dtype=torch.float64)}}
    _PROBLEMS[k] = pb
    return pb


def kinked_species(cls):
    """Indices of the species that an argument of a sqrt, maximum or minimum of the class's traced diffusion depends on."""
    from vihds.modelgen import _topo
    out = set()
    for n in _topo([e for e in cls._trace.dif if hasattr(e, "op")]):
        if n.op in ("sqrt", "maximum", "minimum"):
            out |= {m.val for m in _topo([a for a in n.args if hasattr(a, "op")]) if m.op == "y"}
    return sorted(out)


def kink_margin(cls, starts):
    """The smallest distance, relative to the species' largest value, from the kink at 0 of a species that a sqrt / maximum of the
    class's diffusion reads, over the step start states `starts` (what forward(..., starts=[]) collected: every state an
    amplitude is evaluated at, sub-steps included).  Every class of this module takes the root and the maximum of a species
    itself, so the argument's kink is the species' zero; inf for a class whose amplitudes have no such operation."""
    states = torch.stack(list(starts))
    out = float("inf")
    for j in kinked_species(cls):
        v = states[..., j]
        out = min(out, float((v / v.abs().max()).min()))
    return out


STAT_KEY = (20261, 1020)  # the key of the statistics test (tests/test_modelgen_sde_gpu.py; its CPU twin in the host tests)
STAT_B, STAT_S = 4, 4096
STAT_THETA = {"a": 0.8, "sigma": 0.5, "init": 1.0}


def ou_statistics(traj, times):
    """What the statistics test asserts, from the trajectories traj [n, 4, T] (float64) of OrnsteinUhlenbeck under euler with
    STAT_THETA on the float32 grid `times`: per species the distance of the last point's sample mean and variance from the exact
    recursion m' = (1 - a h) m, Var' = (1 - a h)^2 Var + sigma^2 h in standard errors (sqrt(Var / n), sqrt(2 / n) Var), and the
    correlations of the increments (x_k+1 - (1 - a h) x_k) / (sigma sqrt(h)) between two species, two consecutive steps and
    neighbouring trajectories, with their bound 5 / sqrt(n)."""
    import numpy as np

    a, sigma, x0 = STAT_THETA["a"], STAT_THETA["sigma"], STAT_THETA["init"]
    n = traj.shape[0]
    t = times.float().double()
    steps = t[1:] - t[:-1]
    m, var = x0, 0.0
    for h in steps.tolist():
        m, var = (1.0 - a * h) * m, (1.0 - a * h) ** 2 * var + sigma * sigma * h
    last = traj[:, :, -1]
    mean_se = [(float(last[:, j].mean()) - m) / (var / n) ** 0.5 for j in range(4)]
    var_se = [(float(last[:, j].var()) - var) / ((2.0 / n) ** 0.5 * var) for j in range(4)]
    xi = (traj[:, :, 1:] - (1.0 - a * steps) * traj[:, :, :-1]) / (sigma * steps.sqrt())
    corr = lambda u, v: float(np.corrcoef(u.numpy().ravel(), v.numpy().ravel())[0, 1])  # noqa: E731
    corrs = {"two species": corr(xi[:, 0, :], xi[:, 1, :]), "the first and the last species": corr(xi[:, 3, :], xi[:, 0, :]),
             "two consecutive steps": corr(xi[:, :, :-1], xi[:, :, 1:]), "neighbouring trajectories": corr(xi[:-1], xi[1:])}
    return mean_se, var_se, corrs, 5.0 / n ** 0.5
