"""Models with steady species (`steady_species`, `steady_rate` of vihds.modelgen: the trajectory starts at a steady state of the
model itself under the pre-culture conditions) for the tests: PrprSteadySolved, modelgen_leadin_models.PrprSteady with its
closed-form start replaced by the solve (the twin that pins the mu adjoint to plain reverse mode); ToggleSteady, two mutually
repressing species whose inducer is absent before t_0, bistable at the draws (no closed form; the guess selects the basin);
CascadeCombined, four steady species in a repression cascade with a forcing read at u_0, a treatment, a start map for the
guess, a lead-in, two sub-steps and a dilution jump; ChainEight, eight steady species coupled to their neighbours (the cap, a
tridiagonal pattern); BindingSteadyStiff, the stiff binding model of modelgen_implicit_models started from its pre-culture
equilibrium and run with backward Euler.

The float64 yardstick is modelgen_leadin_models.definition: the plain scheme from torch_problem's x0, which now includes the
solve (GeneratedOdeModel.torch_steady: the iteration as the module docstring defines it and the implicit-function gradient at
its final state).  `converged` is the precondition every comparison asserts first, on the float64 run alone."""
import torch

from vihds.modelgen import GeneratedOdeModel, where
from vihds.precisions import ConstantPrecisions

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_leadin_models as LM
import modelgen_substep_models as SM
from modelgen_models import PREC, PrprRestated
from modelgen_piecewise_models import TIMES  # noqa: F401  (for the tests)

INDUCED_ABOVE = LM.INDUCED_ABOVE


class PrprSteadySolved(PrprRestated):
    """PrprSteady with the solve in place of the closed form: a pre-induced well relaxes RFP, YFP and CFP to `pre` x production
    / (degradation + dilution); any other well to its initial state, which steady_rate reads as effective parameters of its own.
    The residuals are linear in the steady species: 9 iterations (delta 0.1 .. 6.5e3) reach the closed form to 1e-12 in float64
    (tests/test_modelgen_steady_host.py states the count)."""
    model_key = "gen_prpr_constant_steady_solved"
    parameters = LM.PrprSteady.parameter_names
    n_conditions = 1
    steady_species = ["RFP", "YFP", "CFP"]
    steady_steps = 9
    steady_first_step = 0.1
    steady_growth = 4.0

    def prepare(self, th, c):
        p = PrprRestated.prepare(self, th, c)
        p.update({"pre": th.pre, "rfp0": th.init_rfp, "yfp0": th.init_yfp, "cfp0": th.init_cfp})
        return p

    def steady_rate(self, y, p, c):
        x, rfp, yfp, cfp, f530, f480 = y
        induced = c[0] > INDUCED_ABOVE
        return [where(induced, p.pre * p.rc - (p.drfp + p.r) * rfp, p.rfp0 - rfp),
                where(induced, p.pre * p.rc * p.aYFP - (p.dyfp + p.r) * yfp, p.yfp0 - yfp),
                where(induced, p.pre * p.rc * p.aCFP - (p.dcfp + p.r) * cfp, p.cfp0 - cfp)]


class ToggleSteady(GeneratedOdeModel):
    """A toggle switch: U and V repress each other with Hill exponent 2; the inducer (the treatment) weakens V's repression of U
    and is absent in the pre-culture, where U also has a basal production `leak` that only steady_rate reads.  init_u and init_v
    only feed the guess: they say which basin the well was pre-cultured in."""
    model_key = "gen_toggle_steady"
    species = ["OD", "U", "V", "W"]
    parameters = ["r", "K", "a1", "a2", "d", "kw", "leak", "init_x", "init_u", "init_v", "init_w"]
    n_conditions = 1
    observe_kind = "direct"
    steady_species = ["U", "V"]
    steady_steps = 12
    steady_first_step = 0.1
    steady_growth = 4.0

    def __init__(self, config):
        super(ToggleSteady, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": th.r, "K": th.K, "a1": th.a1, "a2": th.a2, "d": th.d, "kw": th.kw, "leak": th.leak}

    def initial_state(self, th, c):
        return [th.init_x, th.init_u, th.init_v, th.init_w]

    def rhs(self, t, y, p, c):
        x, u, v, w = y
        ve = v / (1.0 + c[0])
        return [p.r * x * (1.0 - x / p.K),
                p.a1 / (1.0 + ve * ve) - p.d * u,
                p.a2 / (1.0 + u * u) - p.d * v,
                p.kw * u - p.d * w]

    def steady_rate(self, y, p, c):
        f = self.rhs(0.0, y, p, [0.0] * len(c))
        return [f[1] + p.leak, f[2]]


class CascadeCombined(GeneratedOdeModel):
    """A repression cascade X1 -| X2 -> X3 -| X4 driven by light and an inducer, diluted by growth: the four are steady in the
    pre-culture (the first light sample, half the inducer), start sets the guess of X1 from the light, two lead-in steps, two
    sub-steps per interval, and a dilution jump that doses the reporter."""
    model_key = "gen_cascade_steady_combined"
    species = ["OD", "X1", "X2", "X3", "X4", "F"]
    parameters = ["r", "K", "b1", "b2", "b3", "b4", "dx", "kf", "bolus", "init_x", "init_c", "init_f"]
    n_conditions = 1
    forcings = ["light", "keep", "dose"]
    steady_species = ["X1", "X2", "X3", "X4"]
    steady_steps = 12
    steady_first_step = 0.1
    steady_growth = 4.0
    substeps = 2
    lead_in = 0.5
    lead_in_steps = 2

    def __init__(self, config):
        super(CascadeCombined, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {n: getattr(th, n) for n in ("r", "K", "b1", "b2", "b3", "b4", "dx", "kf", "bolus")}

    def initial_state(self, th, c):
        return [th.init_x, th.init_c, th.init_c, th.init_c, th.init_c, th.init_f]

    def start(self, y, p, c):
        return [y[0], y[1] + self.forcing.light * p.b1 / (p.dx + p.r), y[2], y[3], y[4], y[5]]

    def rhs(self, t, y, p, c):
        x, x1, x2, x3, x4, f = y
        g = p.r * (1.0 - x / p.K)
        return [g * x,
                p.b1 * self.forcing.light * (1.0 + c[0]) - (p.dx + g) * x1,
                p.b2 / (1.0 + x1 * x1) - (p.dx + g) * x2,
                p.b3 * x2 / (1.0 + x2) - (p.dx + g) * x3,
                p.b4 / (1.0 + x3 * x3) - (p.dx + g) * x4,
                p.kf * x4 - g * f]

    def steady_rate(self, y, p, c):
        f = self.rhs(0.0, y, p, [0.5 * c[0]])
        return [f[1], f[2], f[3], f[4]]

    def observe(self, y, p, c):
        return [y[0], y[0] * y[2], y[0] * y[4], y[0] * y[5]]

    def jump(self, y, p, c):
        keep = self.forcing.keep
        out = [v * keep for v in y]
        out[5] = out[5] + self.forcing.dose * p.bolus
        return out


class ChainEight(GeneratedOdeModel):
    """Eight species in a chain, each produced at its own rate, degraded linearly and quadratically and exchanged with its
    neighbours: all eight steady in the pre-culture (a tridiagonal J), next to the density and a reporter."""
    model_key = "gen_chain_eight_steady"
    species = ["OD"] + ["S%d" % j for j in range(1, 9)] + ["R"]
    parameters = ["r", "K", "a", "b", "q", "k", "kf", "init_x", "init_s", "init_r"]
    n_conditions = 0
    steady_species = ["S%d" % j for j in range(1, 9)]
    steady_steps = 12
    steady_first_step = 0.1
    steady_growth = 4.0

    def __init__(self, config):
        super(ChainEight, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {n: getattr(th, n) for n in ("r", "K", "a", "b", "q", "k", "kf")}

    def initial_state(self, th, c):
        return [th.init_x] + [(1.0 + 0.1 * j) * th.init_s for j in range(8)] + [th.init_r]

    def rhs(self, t, y, p, c):
        s = y[1:9]
        out = [p.r * y[0] * (1.0 - y[0] / p.K)]
        for j in range(8):
            left = s[j - 1] - s[j] if j > 0 else 0.0
            right = s[j + 1] - s[j] if j < 7 else 0.0
            out.append(p.a * (0.2 * (j + 1)) - p.b * s[j] - p.q * s[j] * s[j] + p.k * (left + right))
        out.append(p.kf * s[7] - p.b * y[9])
        return out

    def steady_rate(self, y, p, c):
        return self.rhs(0.0, y, p, c)[1:9]

    def observe(self, y, p, c):
        return [y[0], y[1] + y[2], y[8], y[9]]


class ChainEightFree(ChainEight):
    """ChainEight without the solve (what the timing probe compares it with): the integration starts from the initial state."""
    model_key = "gen_chain_eight_free"
    steady_species = None


class BindingSteadyStiff(IM.FastBinding):
    """The stiff binding model started from the equilibrium of its pre-culture, where A and B are produced at `pre` x their
    rates: A, B and C are steady, the reporter starts from 0.  implicit = True; run with backward Euler."""
    model_key = "gen_fast_binding_steady"
    parameters = IM.FastBinding.parameter_names + ["pre"]
    newton_iterations = 6
    steady_species = ["A", "B", "C"]
    steady_steps = 14
    steady_first_step = 0.05
    steady_growth = 4.0

    def prepare(self, th, c):
        p = IM.FastBinding.prepare(self, th, c)
        p["pre"] = th.pre
        return p

    def steady_rate(self, y, p, c):
        A, B, C, R = y
        bind = p.kon * A * B - p.koff * C
        return [p.pre * p.prod - bind - p.deg * A, 0.5 * p.pre * p.prod - bind - p.deg * B, bind - p.deg * C]


MODELS = [PrprSteadySolved, ToggleSteady, CascadeCombined, ChainEight, BindingSteadyStiff]
STIFF = (BindingSteadyStiff,)  # beuler only: the explicit schemes blow up at its inputs
STEADY_ONLY = {PrprSteadySolved: "pre", ToggleSteady: "leak", BindingSteadyStiff: "pre"}  # read by steady_rate alone
GUESS_ONLY = {ToggleSteady: ("init_u", "init_v"), CascadeCombined: ("init_c",), ChainEight: ("init_s",)}  # slots that only feed a steady species' guess
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS + [ChainEightFree]]  # (... and the timing probe)

_PREC_BASE = {n: FM.PRPR_BASE[n] for n in PREC}
# (median, log-sd) per slot; ToggleSteady's guesses are set per data row below (the basins)
DRAWS = {
    PrprSteadySolved: {n: (v, 0.2) for n, v in dict(FM.PRPR_BASE, pre=0.7).items()},
    ToggleSteady: dict({"r": (1.0, 0.2), "K": (2.0, 0.2), "a1": (6.0, 0.05), "a2": (6.0, 0.05), "d": (1.0, 0.05), "kw": (0.5, 0.2),
                        "leak": (0.05, 0.2), "init_x": (0.05, 0.2), "init_u": (1.0, 0.1), "init_v": (1.0, 0.1), "init_w": (0.3, 0.2)},
                       **{n: (v, 0.2) for n, v in _PREC_BASE.items()}),
    CascadeCombined: dict({"r": (1.0, 0.2), "K": (2.0, 0.2), "b1": (1.2, 0.2), "b2": (2.0, 0.2), "b3": (1.5, 0.2), "b4": (1.0, 0.2),
                           "dx": (0.5, 0.2), "kf": (0.8, 0.2), "bolus": (0.5, 0.2), "init_x": (0.05, 0.2), "init_c": (0.3, 0.2),
                           "init_f": (0.2, 0.2)}, **{n: (v, 0.2) for n, v in _PREC_BASE.items()}),
    ChainEight: dict({"r": (1.0, 0.2), "K": (2.0, 0.2), "a": (1.0, 0.2), "b": (0.6, 0.2), "q": (0.3, 0.2), "k": (0.4, 0.2),
                      "kf": (0.7, 0.2), "init_x": (0.05, 0.2), "init_s": (0.3, 0.2), "init_r": (0.2, 0.2)},
                     **{n: (v, 0.2) for n, v in _PREC_BASE.items()}),
    BindingSteadyStiff: dict(IM.FAST_DRAWS, pre=(0.4, 0.2)),
}
DRAWS[ChainEightFree] = DRAWS[ChainEight]
TOGGLE_GUESS = [(3.5, 0.3), (0.3, 3.5), (4.5, 0.2)]  # (U, V) medians per data row, cyclically: rows 0 and 2 high U, row 1 high V
_PROBLEMS = {}

definition = LM.definition


def solvers_of(cls):
    """beuler alone for the stiff model; midpoint and rk4 for the others, euler and modeuler too for the twin."""
    if cls in STIFF:
        return ["beuler"]
    return ["midpoint", "rk4"] + (["euler", "modeuler"] if cls is PrprSteadySolved else [])


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def guess_and_forcing(cls, th, cond, T):
    """(the state the solve starts from [B,S,N], the first forcing samples or None) in the dtype of th: torch_problem's x0
    without the solve is not on offer, so the guess is formed as torch_problem forms it."""
    ref = next(iter(th.values()))
    _rhs, x0 = cls.torch_problem(th, cond, None, start=False, **({"times": torch.arange(T, dtype=ref.dtype)} if cls.forcings else {}))
    K = len(cls.forcings or ())
    forcing = None
    if K:
        series = cond[:, cond.shape[1] - K * T:].reshape(cond.shape[0], K, T).to(ref.dtype)
        forcing = [series[:, k, 0, None].expand_as(ref) for k in range(K)]
    if cls._start_def is not None:
        x0 = cls.torch_start(x0, th, cond, **({"n_times": T} if K else {}))
    return x0, forcing


def converged(cls, pb, dtype=torch.float64, **over):
    """(the largest last increment relative to |y_E|, the largest |steady_rate| at the final state, the final state) of the
    solve on the problem's inputs in `dtype`: the convergence precondition of the comparisons is the first at most 1e-9 in
    float64."""
    th = {n: v.to(dtype) for n, v in pb["th"].items()}
    guess, forcing = guess_and_forcing(cls, th, pb["cond"].to(dtype), pb["T"])
    with torch.no_grad():
        y, inc, res = cls.torch_steady(guess, th, pb["cond"].to(dtype), forcing=forcing, return_residual=True, **over)
    return inc, res, y


def problem(cls, B, S, times=None, seed=41):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot (every normal clipped at 3
    sd), the wide cond (treatments 0.3, 1.0, 1.7, ...), times, observations (the first sample's prediction under the definition
    with 5 % noise) and an upstream gradient for the log-likelihood."""
    times = TIMES if times is None else times
    k = (cls, B, S, tuple(times), seed)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64).clamp(-3.0, 3.0)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    assert sorted(slot_names(cls)) == sorted(DRAWS[cls])
    th = {n: m * torch.exp(sd * rnd(B, S)) for n, (m, sd) in DRAWS[cls].items()}
    if cls is ToggleSteady:
        for b in range(B):
            u, v = TOGGLE_GUESS[b % len(TOGGLE_GUESS)]
            th["init_u"][b] *= u
            th["init_v"][b] *= v
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = JM.series_of(cls, B, tt)
    cond = FM.wide_cond(treatments, series)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        xs = LM.beuler_states(cls, th1, cond, tt)[0] if cls in STIFF else LM.explicit_states(cls, th1, cond, tt, "rk4")
        xp = SM.hooks(cls, xs, th1, cond, torch.zeros(B, 4, T, dtype=torch.float64))[1]
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "treatments": treatments, "times": tt, "obs": obs, "W": {}, "B": B, "S": S,
          "T": T, "G": {"logp": rnd(B, S, 4)}}
    _PROBLEMS[k] = pb
    return pb
