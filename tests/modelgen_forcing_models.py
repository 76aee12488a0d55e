"""Models with time-varying inputs (the forcings of vihds.modelgen) for the tests: the prpr_constant restatement whose YFP
production is scaled by a light schedule read in rhs (and its twin that takes the same input as a constant treatment), the
plate reader whose gain and noise depend on a logged temperature (read by observe and precision only), and a small model
that switches on a square-wave light (a condition on a forcing), feeds a network from both of its forcings and has a
Student-t likelihood.

A row of `cond` is [n_conditions treatments as log(1 + c) | K x T forcing samples, forcing-major, raw].  The series differ
from row to row; one is smooth and one a sampled square wave whose levels (0.2 and 1.0) keep the interpolant away from the
0.5 that ForcedSwitch compares it with at every stage time of the fixed-grid schemes (fractions 0, 1/3, 1/2, 2/3, 1 of an
interval: 0.2, 0.467, 0.6, 0.733, 1.0), which the tests assert as modelgen_piecewise_models.MARGIN on the float64 run."""
import math

import torch

from oracle import vihds_oracle as O
from vihds.modelgen import GeneratedOdeModel, Network, clamp, log, sigmoid, where
from vihds.precisions import ConstantPrecisions

from modelgen_models import PREC, PrprRestated
from modelgen_noise_models import NOISE, PlateReaderNoise
from modelgen_observe_models import PlateReader
from modelgen_piecewise_models import FIXED, TIMES, recording, sw  # noqa: F401  (FIXED, recording: for the tests)

NU = 4.0
STUDENT_T_CONST = math.lgamma(0.5 * (NU + 1.0)) - math.lgamma(0.5 * NU) - 0.5 * math.log(NU * math.pi)
LOW, HIGH = 0.2, 1.0  # the square wave's levels


def _prpr_rhs(t, y, p, drive):
    x, rfp, yfp, cfp, f530, f480 = y
    gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
    return [gamma * x,
            p.rc - (gamma + p.drfp) * rfp,
            p.rc * p.aYFP * drive - (gamma + p.dyfp) * yfp,
            p.rc * p.aCFP - (gamma + p.dcfp) * cfp,
            p.rc * p.a530 - gamma * f530,
            p.rc * p.a480 - gamma * f480]


class PrprForced(PrprRestated):
    """PrprRestated with YFP production scaled by a light schedule that differs from well to well."""
    model_key = "gen_prpr_constant_forced"
    forcings = ["light"]

    def rhs(self, t, y, p, c):
        return _prpr_rhs(t, y, p, self.forcing.light)


class PrprTreated(PrprRestated):
    """The twin of PrprForced whose drive is a constant treatment."""
    model_key = "gen_prpr_constant_treated"
    n_conditions = 1

    def rhs(self, t, y, p, c):
        return _prpr_rhs(t, y, p, c[0])


class PrprRamped(PrprRestated):
    """PrprRestated whose drive is the linear function 0.4 + 0.25 t written into rhs by hand (what PrprForced computes from the
    samples of that function: the interpolant reproduces it exactly)."""
    model_key = "gen_prpr_constant_ramped"
    RAMP = (0.4, 0.25)

    def rhs(self, t, y, p, c):
        return _prpr_rhs(t, y, p, self.RAMP[0] + self.RAMP[1] * t)


class PlateReaderForced(PlateReaderNoise):
    """PlateReaderNoise in an incubator whose logged temperature changes the detector's gain and its noise: the forcing is
    read by observe and precision only, never by rhs."""
    model_key = "gen_plate_reader_forced"
    forcings = ["temp"]

    def observe(self, y, p, c):
        xp = PlateReader._observe_def(self, y, p, c)
        gain = 1.0 + 0.3 * (self.forcing.temp - 1.0)
        return [xp[0], gain * xp[1], gain * xp[2], xp[3] + 0.05 * self.forcing.temp]

    def precision(self, y, x, p, c):
        pr = PlateReaderNoise._precision_def(self, y, x, p, c)
        return [pr[0]] + [pr[j] / (1.0 + 0.5 * self.forcing.temp * self.forcing.temp) for j in (1, 2, 3)]


class ForcedSwitch(GeneratedOdeModel):
    """Light-switched expression: YFP production takes `boost` while the light is on (a condition on a forcing), a 3 -> 4 -> 1
    tanh network fed from both forcings gates the expression rate, CFP production follows a treatment, the temperature warms
    the decay; Student-t noise around the fixed 'direct' map, whose scale reads the temperature too."""
    model_key = "gen_forced_switch"
    species = ["OD", "RFP", "YFP", "CFP"]
    parameters = ["r", "K", "rc", "drfp", "dyfp", "dcfp", "aYFP", "aCFP", "boost", "init_x", "init_rfp", "init_yfp", "init_cfp"]
    n_conditions = 1
    observe_kind = "direct"
    forcings = ["light", "temp"]
    networks = {"gate": Network(n_inputs=3, n_hidden=4, n_outputs=1, hidden="tanh")}

    def __init__(self, config):
        super(ForcedSwitch, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "rc": th.rc, "drfp": th.drfp, "dyfp": th.dyfp,
                "dcfp": th.dcfp, "aYFP": th.aYFP, "aCFP": th.aCFP, "boost": th.boost}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, th.init_cfp]

    def rhs(self, t, y, p, c):
        x, rfp, yfp, cfp = y
        light, temp = self.forcing.light, self.forcing.temp
        gamma = p.r * (1.0 - x / p.K)
        rate = p.rc * sigmoid(self.net.gate([light, x, temp])[0])
        on = sw.gt("rhs light > 0.5", light, 0.5)
        return [gamma * x,
                rate - (gamma + p.drfp * temp) * rfp,
                rate * p.aYFP * where(on, p.boost, 0.2) - (gamma + p.dyfp) * yfp,
                rate * p.aCFP * c[0] / (1.0 + c[0]) - (gamma + p.dcfp) * cfp]

    def log_likelihood(self, x, obs, pr, p, c):
        def t(j):
            s = pr[j] / (1.0 + 0.2 * self.forcing.temp)
            e = x[j] - obs[j]
            return STUDENT_T_CONST + 0.5 * log(s) - 0.5 * (NU + 1.0) * log(1.0 + s * e * e / NU)
        return [t(j) for j in range(4)]


MODELS = [PrprForced, PlateReaderForced, ForcedSwitch]
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(PrprForced, False), (PlateReaderForced, False), (ForcedSwitch, False), (PrprTreated, False)]


# ---- inputs of the numeric tests ----------------------------------------------------------------------------------------------
PRPR_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP_PR": 1.2,
             "aCFP_PR": 0.9, "a530": 0.4, "a480": 0.3, "init_x": 0.01, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
             "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
READER_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "aYFP": 1.2, "gain_r": 1.3, "bg_r": 0.05,
               "sat": 0.6, "auto": 0.3, "leak": 0.2, "init_x": 0.05, "init_rfp": 0.1, "init_yfp": 0.1,
               "s0_od": 0.05, "s1_od": 0.1, "s0_r": 0.05, "s1_r": 0.1, "s0_y": 0.05, "s1_y": 0.1, "s0_c": 0.05, "s1_c": 0.1,
               "s_dens": 0.05, "s_trt": 0.05}
SWITCH_BASE = {"r": 1.0, "K": 2.0, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP": 1.2, "aCFP": 0.9, "boost": 1.5,
               "init_x": 0.05, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
               "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
BASES = {PrprForced: PRPR_BASE, PrprTreated: PRPR_BASE, PrprRamped: PRPR_BASE, PlateReaderForced: READER_BASE,
         ForcedSwitch: SWITCH_BASE}
assert all(n in READER_BASE for n in NOISE)
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def smooth_series(B, times):
    """[B, T]: 1 + 0.5 sin(0.9 t + 0.7 b), a different phase per row."""
    t = torch.as_tensor(times, dtype=torch.float64)
    return 1.0 + 0.5 * torch.sin(0.9 * t[None, :] + 0.7 * torch.arange(B, dtype=torch.float64)[:, None])


def square_series(B, T):
    """[B, T]: a square wave of period 4 samples between LOW and HIGH, shifted by one sample from row to row."""
    k = torch.arange(T)[None, :] + torch.arange(B)[:, None]
    return torch.where((k // 2) % 2 == 0, torch.tensor(HIGH, dtype=torch.float64), torch.tensor(LOW, dtype=torch.float64))


def series_of(cls, B, times):
    """The forcing samples of a class [B, K, T], in the order of cls.forcings."""
    T = len(times)
    named = {"light": square_series(B, T) if cls is ForcedSwitch else smooth_series(B, times),
             "temp": smooth_series(B, times).flip(0) if cls is ForcedSwitch else smooth_series(B, times)}
    return torch.stack([named[n] for n in cls.forcings], dim=1)


def wide_cond(treatments, series):
    """[B, C + K T]: log(1 + treatment) per treatment, then the samples, forcing-major, raw."""
    B = series.shape[0]
    return torch.cat([torch.log1p(treatments).reshape(B, -1), series.reshape(B, -1)], dim=1)


def forward(cls, th, cond, times, solver, obs=None, weights=None):
    """The float64 (or float32) definition: species [B,S,N,T], x_predict [B,S,4,T], precisions [B,S,4,T] and, given
    observations, the per-signal log-likelihood [B,S,4]."""
    kw = {"times": times} if cls.forcings else {}
    rhs, x0 = cls.torch_problem(th, cond, weights, **kw)
    xs = O.simulate(rhs, x0, times, solver)
    if cls._observe_def is not None:
        xp = cls.torch_observe(xs, th, cond)
    else:
        xp = O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)
    if cls._precision_def is not None:
        prec = cls.torch_precision(xs, th, cond)
    else:
        prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    if obs is None:
        return xs, xp, prec, None
    if cls._likelihood_def is not None:
        logp = cls.torch_log_likelihood(xp, obs, prec, th, cond).sum(3)
    else:
        logp = O.log_prob_observations(xp, obs, prec)
    return xs, xp, prec, logp


def problem(cls, B, S, times=TIMES, seed=11):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, the wide cond, times,
    network weights, observations (the first sample's prediction with 5 % noise) and an upstream gradient for the
    log-likelihood."""
    k = (cls, B, S, tuple(times), seed)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    th = {n: v * torch.exp(0.2 * rnd(B, S)) for n, v in BASES[cls].items()}
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = series_of(cls, B, tt) if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    cond = wide_cond(treatments, series)
    W = {name: tuple(0.6 * rnd(*shape) for shape in net.tensor_shapes()) for name, net in (cls.networks or {}).items()}
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        _, xp, _, _ = forward(cls, th1, cond, tt, "rk4", weights=W or None)
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "treatments": treatments, "times": tt, "obs": obs, "W": W, "B": B, "S": S,
          "T": T, "G": {"logp": rnd(B, S, 4)}}
    _PROBLEMS[k] = pb
    return pb
