"""Models with reaction-channel noise (`noise_channels` / `channel_noise` of vihds.modelgen) for the tests, and the float64
yardstick of the scheme.

  ConversionPair   rhs = 0 and one channel A -> B with the columns [-sigma, +sigma]: A + B is conserved by every step
  SharedChannel    two species with linear decay; one channel enters both, each has a private one: additive noise with a known
                   variance and covariance recursion (the statistics)
  ExpressionCLE    mRNA / protein / matured protein written once as reactions (langevin, langevin_drift): five channels with
                   square-root amplitudes, a forcing that gates transcription, substeps = 4
  HookedChannels   a jump, an observation map of its own, missing observations and a `where` in an amplitude
  DiagonalTwin     PrprLangevin (tests/modelgen_sde_models.py) restated with one channel per noisy species
  Channels8        eight channels that all enter all four species: the second Philox block, and the densest pattern the module
                   allows (MAX_NOISE_ENTRIES) -- the worst case of the compile test

Every class is padded to the species its observe_kind reads, as the classes of tests/modelgen_sde_models.py are.

The yardstick (`forward`) is modelgen_sde_models.forward with the channel sum in place of g * xi:
    u' = Phi_h(u) + sum_r G[:, r](u) sqrt(h) xi_r        per step, sub-steps included, G at the step's start state,
G from torch_channel_noise and the draws xi [B,S,>=R,(T-1)*substeps] passed in as an argument (channel r of step c)."""
import torch

from oracle import vihds_oracle as O
from vihds.modelgen import GeneratedOdeModel, clamp, langevin, langevin_drift, maximum, sigmoid, sqrt, where
from vihds.precisions import ConstantPrecisions

import modelgen_missing_models as MM
import modelgen_sde_models as SM
from modelgen_models import PREC
from modelgen_sde_models import FIXED, RAGGED, STAT_B, STAT_S, n_steps, slot_names, smooth_series  # noqa: F401  (for the tests)


class _Constant(GeneratedOdeModel):
    def __init__(self, config):
        super(_Constant, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)


class ConversionPair(_Constant):
    """A -> B at a constant amplitude and no drift: the two species move by the same increment, in opposite directions."""
    model_key = "gen_chan_conversion_pair"
    species = ["A", "B", "U", "V"]
    parameters = ["sigma", "init_a", "init_b"]
    observe_kind = "direct"
    noise_channels = ["convert"]

    def prepare(self, th, c):
        return {"sigma": th.sigma}

    def initial_state(self, th, c):
        return [th.init_a, th.init_b, 0.5, 0.25]

    def rhs(self, t, y, p, c):
        return [0.0, 0.0, 0.0, 0.0]

    def channel_noise(self, y, p, c):
        return [[-p.sigma, p.sigma, 0.0, 0.0]]


class SharedChannel(_Constant):
    """dX_j = -a X_j dt + s dW_shared + s_j dW_j on two species (two more decay without noise)."""
    model_key = "gen_chan_shared_channel"
    species = ["X0", "X1", "U", "V"]
    parameters = ["a", "s", "s0", "s1", "init"]
    observe_kind = "direct"
    noise_channels = ["shared", "own0", "own1"]

    def prepare(self, th, c):
        return {"a": th.a, "s": th.s, "s0": th.s0, "s1": th.s1}

    def initial_state(self, th, c):
        return [th.init, th.init, th.init, th.init]

    def rhs(self, t, y, p, c):
        return [-p.a * v for v in y]

    def channel_noise(self, y, p, c):
        return [[p.s, p.s, 0.0, 0.0], [p.s0, 0.0, 0.0, 0.0], [0.0, p.s1, 0.0, 0.0]]


class ExpressionCLE(_Constant):
    """Light-gated expression as a chemical Langevin equation: transcription, mRNA decay, translation, maturation and the decay
    of the matured protein, each a channel; `eps` is the inverse square root of the system size.  D is a deterministic fourth
    species."""
    model_key = "gen_chan_expression_cle"
    species = ["M", "P", "F", "D"]
    parameters = ["ktx", "dm", "ktl", "kmat", "df", "eps", "init_m", "init_p"]
    observe_kind = "direct"
    forcings = ["light"]
    substeps = 4
    noise_channels = ["tx", "mdeg", "tl", "mature", "fdeg"]
    STOICHIOMETRY = [[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, -1, 1, 0], [0, 0, -1, 0]]

    def prepare(self, th, c):
        return {"ktx": th.ktx, "dm": th.dm, "ktl": th.ktl, "kmat": th.kmat, "df": th.df, "eps": th.eps}

    def initial_state(self, th, c):
        return [th.init_m, th.init_p, 0.5 * th.init_p, 0.1]

    def propensities(self, y, p):
        return [p.ktx * self.forcing.light, p.dm * y[0], p.ktl * y[0], p.kmat * y[1], p.df * y[2]]

    def rhs(self, t, y, p, c):
        drift = langevin_drift(self.STOICHIOMETRY, self.propensities(y, p))
        return drift[:3] + [0.3 * sigmoid(t) - 0.2 * y[3]]

    def channel_noise(self, y, p, c):
        return [[p.eps * e for e in col] for col in langevin(self.STOICHIOMETRY, self.propensities(y, p))]


class HookedChannels(_Constant):
    """An observation map of its own, a dilution at every read and missing observations; growth noise on the density, and a
    conversion A -> B whose amplitude is the guarded root where(A > 0, sqrt(A), 0)."""
    model_key = "gen_chan_hooked_channels"
    species = ["OD", "A", "B"]
    parameters = ["r", "cap", "k", "d", "keep", "gain", "sigma", "init_x", "init_a"]
    missing_observations = True
    noise_channels = ["growth", "convert"]

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

    def channel_noise(self, y, p, c):
        root = where(y[1] > 0.0, sqrt(p.d * y[1]), 0.0)
        return [[p.sigma * y[0], 0.0, 0.0], [0.0, -p.sigma * root, p.sigma * root]]


class DiagonalTwin(SM.PrprLangevin):
    """PrprLangevin with its two noisy species written as two channels: channel r enters species r alone, with the diagonal
    model's amplitude -- the same counters, the same instructions, the same bits."""
    model_key = "gen_chan_diagonal_twin"
    diffusion = None
    noise_channels = ["od", "rfp"]

    def channel_noise(self, y, p, c):
        return [[p.sigma * sqrt(maximum(y[0], 0.0)), 0.0, 0.0, 0.0, 0.0, 0.0],
                [0.0, 0.5 * p.sigma * sqrt(maximum(y[1], 0.0)), 0.0, 0.0, 0.0, 0.0]]


_W8 = [[(0.3 + 0.1 * ((3 * q + 5 * r) % 7)) * (1.0 if (q + r) % 2 == 0 else -1.0) for q in range(4)] for r in range(8)]


class Channels8(_Constant):
    """Four species relaxing to a level, eight channels that each enter all four: 32 amplitudes, the densest pattern allowed.
    Channels 0 .. 3 scale with sigma (Philox block 0), channels 4 .. 7 with tau (block 1)."""
    model_key = "gen_chan_channels8"
    species = ["X0", "X1", "X2", "X3"]
    parameters = ["a", "level", "sigma", "tau", "init"]
    observe_kind = "direct"
    noise_channels = ["c0", "c1", "c2", "c3", "c4", "c5", "c6", "c7"]

    def prepare(self, th, c):
        return {"a": th.a, "level": th.level, "sigma": th.sigma, "tau": th.tau}

    def initial_state(self, th, c):
        return [th.init, 0.8 * th.init, 1.2 * th.init, th.init]

    def rhs(self, t, y, p, c):
        return [p.a * (p.level - v) for v in y]

    def channel_noise(self, y, p, c):
        roots = [sqrt(maximum(v, 0.0) + 0.05) for v in y]
        return [[(p.sigma if r < 4 else p.tau) * _W8[r][q] * roots[q] for q in range(4)] for r in range(8)]


PARITY = [ExpressionCLE, HookedChannels, Channels8]
TWIN = {DiagonalTwin: SM.PrprLangevin}
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(ConversionPair, False), (SharedChannel, False), (ExpressionCLE, False), (HookedChannels, False), (DiagonalTwin, False),
            (Channels8, False)]
NOISE_PARAMETERS = {ConversionPair: ["sigma"], SharedChannel: ["s", "s0", "s1"], ExpressionCLE: ["eps"], HookedChannels: ["sigma"],
                    DiagonalTwin: ["sigma"], Channels8: ["sigma", "tau"]}

_P = {"prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
BASES = {
    ConversionPair: dict(_P, sigma=0.3, init_a=1.0, init_b=0.5),
    SharedChannel: dict(_P, a=0.8, s=0.4, s0=0.3, s1=0.5, init=1.0),
    ExpressionCLE: dict(_P, ktx=1.5, dm=0.9, ktl=1.2, kmat=0.7, df=0.4, eps=0.05, init_m=1.0, init_p=1.0),
    HookedChannels: dict(_P, r=1.2, cap=2.0, k=0.9, d=0.5, keep=0.85, gain=1.3, sigma=0.1, init_x=0.2, init_a=0.4),
    DiagonalTwin: SM.BASES[SM.PrprLangevin],
    Channels8: dict(_P, a=0.6, level=1.5, sigma=0.04, tau=0.05, init=1.0),
}
KEY = (0x5eed03, 0x0c4a17)  # the noise key of the shared problems: two words below 2^24
_PROBLEMS = {}


def n_channels(cls):
    return len(cls.noise_channels)


def pattern(cls):
    """[(species q, channel r)] of the entries of G that are not the constant 0 (the struct's channel_species)."""
    R = n_channels(cls)
    return [(j // R, j % R) for j, e in enumerate(cls._trace.chan) if not (e.op == "const" and e.val == 0.0)]


def noisy_species(cls):
    return sorted({q for q, _r in pattern(cls)})


def _column(hook, y, k, T, th, cond):
    """A per-time-point hook (torch_jump / torch_channel_noise) on the state y [B,S,N] with the forcing samples of point k."""
    return hook(y.unsqueeze(-1).expand(y.shape + (T,)), th, cond)[..., k]


def forward(cls, th, cond, times, solver, obs, xi, starts=None, observed=None):
    """The definition in th's dtype: species [B,S,N,T], x_predict [B,S,4,T] and, given observations, the per-signal
    log-likelihood [B,S,4] under the constant precisions (and the mask `observed` [B,4,T] of a class with missing observations).
    xi [B,S,>=R,(T-1)*substeps]: the draws, channel r of step k * substeps + j; cond as the kernels take it (mask words and key
    columns last; they are not read here).  starts: a list that receives the start state [B,S,N] of every step."""
    kw = {"times": times} if cls.forcings else {}
    rhs, y = cls.torch_problem(th, cond, None, **kw)
    R, T, m = n_channels(cls), int(times.shape[0]), int(cls.substeps)
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
            G = _column(cls.torch_channel_noise, y, k, T, th, cond)  # [B,S,N,R]
            y, h = SM._scheme_step(rhs, solver, s0, s1, h0, y)
            y = y + (G * (torch.sqrt(h) * xi[:, :, None, :R, k * m + j])).sum(-1)
        xs.append(y)
    xs = torch.stack(xs, dim=-1)
    if cls._observe_def is not None:
        xp = cls.torch_observe(xs, th, cond)
    else:
        xp = O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)
    if obs is None:
        return xs, xp, None
    prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    if cls.missing_observations:
        seen = torch.ones(obs.shape, dtype=torch.bool) if observed is None else observed
        return xs, xp, MM.masked_sum(lambda ob: MM.gaussian_terms(xp, ob, prec), xp, obs, seen)
    return xs, xp, O.log_prob_observations(xp, obs, prec)


def cond_of(cls, series, observed, key):
    """A row of cond as the kernels take it: [forcing samples | mask words (a masked class) | key lo, key hi]."""
    B, T = series.shape[0], series.shape[2]
    parts = [series.reshape(B, -1)]
    if cls.missing_observations:
        parts.append(torch.full((B, T), 15.0, dtype=torch.float64) if observed is None else MM.words_of(observed))
    parts.append(torch.tensor([float(key[0]), float(key[1])], dtype=torch.float64)[None, :].expand(B, 2))
    return torch.cat(parts, dim=1)


def problem(cls, B, S, times=RAGGED, seed=23, key=KEY):
    """Inputs of one case (shared by the tests that use it; never modified).  A class with missing observations gets the gaps
    mask of tests/modelgen_missing_models.py and NaN / 1e30 under it."""
    k = (cls, B, S, tuple(times), seed, tuple(key))
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    assert sorted(slot_names(cls)) == sorted(BASES[cls])
    th = {n: v * torch.exp(0.1 * rnd(B, S)) for n, v in BASES[cls].items()}
    series = smooth_series(B, tt)[:, None, :] if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    observed = None
    if cls.missing_observations:
        observed = MM.gaps_mask(B, T) if T >= 9 else MM.tail_mask(B, T, lost=0)
    cond = cond_of(cls, series, observed, key)
    with torch.no_grad():  # observations: the noise-free trajectory of the first sample, 5 % multiplicative scatter
        th1 = {n: v[:, :1] for n, v in th.items()}
        zero = torch.zeros(B, 1, n_channels(cls), n_steps(cls, T), dtype=torch.float64)
        _, xp, _ = forward(cls, th1, cond, tt, "rk4", None, zero)
        clean = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "times": tt, "obs": clean if observed is None else MM.with_placeholders(clean, observed),
          "observed": observed, "B": B, "S": S, "T": T, "key": tuple(key),
          # the upstream gradient of the log-likelihood: one sign, so that the loss sum(logp * G) is a well-conditioned sum
          "G": {"logp": 0.5 + torch.rand(B, S, 4, generator=gen, dtype=torch.float64)}}
    _PROBLEMS[k] = pb
    return pb


def kinked_species(cls):
    """Indices of the species that an argument of a sqrt, maximum or minimum, or the condition of a where, of the class's traced
    channel_noise depends on."""
    from vihds.modelgen import _topo
    out = set()
    for n in _topo([e for e in cls._trace.chan if hasattr(e, "op")]):
        if n.op in ("sqrt", "maximum", "minimum"):
            out |= {m.val for m in _topo([a for a in n.args if hasattr(a, "op")]) if m.op == "y"}
        elif n.op == "where":
            out |= {m.val for m in _topo([n.args[0]]) if m.op == "y"}
    return sorted(out)


def kink_margin(cls, starts):
    """The smallest distance, relative to the species' largest value, from the kink at 0 of a species that a sqrt / maximum / where
    of the class's channel_noise reads, over the step start states `starts`.  Every class of this module takes the root, the
    maximum and the condition of a species itself (times a positive parameter, plus a floor >= 0), so the kink nearest to the
    states is the species' zero; inf for a class whose amplitudes have no such operation."""
    states = torch.stack(list(starts))
    out = float("inf")
    for j in kinked_species(cls):
        v = states[..., j]
        out = min(out, float((v / v.abs().max()).min()))
    return out


# ---- the statistics of SharedChannel ------------------------------------------------------------------------------------------------
STAT_KEY = (20263, 1021)  # the key of the statistics test (tests/test_modelgen_channel_gpu.py; its CPU twin in the host tests)
STAT_THETA = {"a": 0.8, "s": 0.4, "s0": 0.3, "s1": 0.5, "init": 1.0}


def shared_statistics(traj, times):
    """What the statistics test asserts, from the trajectories traj [n, 2, T] (float64; species X0 and X1) of SharedChannel under
    euler with STAT_THETA on the float32 grid `times`.  With c = 1 - a h the exact recursions are
        m' = c m,   Var_j' = c^2 Var_j + (s^2 + s_j^2) h,   Cov' = c^2 Cov + s^2 h.
    Returns the distances of the last point's sample means, variances and covariance from them in standard errors (sqrt(Var / n),
    sqrt(2 / n) Var, sqrt((Var_0 Var_1 + Cov^2) / n): those of Gaussian samples), and correlations of the increments
    e_j = (x_j' - c x_j) / sqrt(h) = s xi_s + s_j xi_j with their bound 5 / sqrt(n): between the channel combinations
    e_0 - e_1 (the private channels alone) and s1^2 e_0 + s0^2 e_1 (whose covariance with it is s1^2 s0^2 - s0^2 s1^2 = 0 exactly when
    the three channels are independent with unit variance), between two consecutive steps and between neighbouring
    trajectories."""
    import numpy as np

    a, s, s0, s1, x0 = (STAT_THETA[k] for k in ("a", "s", "s0", "s1", "init"))
    n = traj.shape[0]
    t = times.float().double()
    steps = t[1:] - t[:-1]
    m, var, cov = x0, [0.0, 0.0], 0.0
    for h in steps.tolist():
        c = 1.0 - a * h
        m, cov = c * m, c * c * cov + s * s * h
        var = [c * c * var[0] + (s * s + s0 * s0) * h, c * c * var[1] + (s * s + s1 * s1) * h]
    last = traj[:, :, -1]
    mean_se = [(float(last[:, j].mean()) - m) / (var[j] / n) ** 0.5 for j in range(2)]
    var_se = [(float(last[:, j].var()) - var[j]) / ((2.0 / n) ** 0.5 * var[j]) for j in range(2)]
    got_cov = float(((last[:, 0] - last[:, 0].mean()) * (last[:, 1] - last[:, 1].mean())).sum() / (n - 1))
    cov_se = (got_cov - cov) / ((var[0] * var[1] + cov * cov) / n) ** 0.5
    e = (traj[:, :, 1:] - (1.0 - a * steps) * traj[:, :, :-1]) / steps.sqrt()
    corr = lambda u, v: float(np.corrcoef(u.numpy().ravel(), v.numpy().ravel())[0, 1])  # noqa: E731
    corrs = {"the private channels and their complement": corr(e[:, 0] - e[:, 1], s1 * s1 * e[:, 0] + s0 * s0 * e[:, 1]),
             "two consecutive steps": corr(e[:, :, :-1], e[:, :, 1:]), "neighbouring trajectories": corr(e[:-1], e[1:])}
    return mean_se, var_se, cov_se, corrs, 5.0 / n ** 0.5
