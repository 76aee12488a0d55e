"""Models with `step_tolerance = (rtol, atol)` (vihds.modelgen: every trajectory picks its own number of steps per observation
interval by step doubling, 1 -> 2 -> .. -> substeps; csrc/vihds_stepctl.hpp) for the tests, their twins without the attribute,
and the float64 restatement of the rule that the host and the GPU tests share.

The restatement is written here once.  For the interval k, from y_k (after the class's jump, where it has one), Phi^c is c
steps of the scheme on s_j = t_k + j (t_k+1 - t_k) / c, s_c = t_k+1:

    coarse = Phi^1(y_k);  c = 1
    repeat:  fine = Phi^2c(y_k);  r = max_i |fine_i - coarse_i| / (atol + rtol max(|fine_i|, |coarse_i|))
             r <= 1: take fine, count 2c, passed | 2c == M: take fine, count M, saturated | else coarse = fine, c = 2c

`ladder` runs it without a graph for every trajectory at once and returns the codes (+count passed, -M saturated) and every
ratio that a test looked at; `states` then integrates again with those counts frozen -- every count that occurs is run for the
whole batch and torch.where picks per trajectory, so autograd sees the realised scheme and a count carries no gradient.  An
implicit scheme's steps are modelgen_implicit_models.newton_step / modelgen_sdirk_models.sdirk2_step with autograd through their
iterations, which is the kernels' implicit-function adjoint once the iteration has converged (the tests assert the last
increment on the float64 run)."""
import numpy as np
import torch

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_missing_models as MM
import modelgen_sdirk_models as SD
import modelgen_substep_models as SM
from modelgen_models import PREC

TOL = (1e-3, 1e-6)
LOOSE = (1e30, 0.0)   # every interval passes at the first test: every count is 2
TIGHT = (0.0, 1e-30)  # no interval passes: every count is the ceiling, saturated
BAND = (0.8, 1.25)    # no ratio of a deciding test may lie in here (float32 rounding moves it by parts in a thousand)
# a pulse of light between these times, on a grid whose steps differ by a factor of six
TIMES = [0.0, 0.3, 0.5, 1.1, 1.3, 1.6, 2.2, 2.4, 3.0, 3.6, 3.8, 4.4]
IMPLICIT_TIMES = IM.GRID[:6]  # the implicit cases: steps of 0.1 .. 0.2 (Newton converges at one step per interval too)
PULSE = (1.0, 2.3, 6.0)  # (from, to, level) of the light; 0.3 outside
POOL = 32  # candidates per kept sample (problem)


class PulsedPrpr(JM.PrprDiluted):
    """The diluted and dosed prpr model (a forcing in rhs, a jump) under a pulse of light, with step control."""
    model_key = "gen_prpr_pulsed_ctl8"
    substeps = 8
    step_tolerance = TOL


class PulsedPrprFine(JM.PrprDiluted):
    """... at a tolerance at which the fourth-order scheme's counts vary as well."""
    model_key = "gen_prpr_pulsed_ctl8_fine"
    substeps = 8
    step_tolerance = (1e-4, 1e-6)


class PulsedPrprSub8(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_sub8"
    substeps = 8


class PulsedPrprSub2(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_sub2"
    substeps = 2


class PulsedPrprSub1(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_sub1"


class PulsedPrprLoose(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_ctl8_loose"
    substeps = 8
    step_tolerance = LOOSE


class PulsedPrprTight(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_ctl8_tight"
    substeps = 8
    step_tolerance = TIGHT


class PulsedPrprTight4(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_ctl4_tight"
    substeps = 4
    step_tolerance = TIGHT


class PulsedPrprTight2(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_ctl2_tight"
    substeps = 2
    step_tolerance = TIGHT


class PulsedPrprSub4(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_sub4"
    substeps = 4


class PrprImplicitCtl(IM.PrprForcedImplicit):
    """Backward Euler under a forcing, ceiling 4."""
    model_key = "gen_prpr_forced_implicit_ctl4"
    substeps = 4
    newton_iterations = 6
    step_tolerance = (1.5e-2, 1e-6)


class PrprSdirkCtl(SD.PrprForcedSdirk):
    """The two-stage SDIRK under a forcing, ceiling 4."""
    model_key = "gen_prpr_forced_sdirk_ctl4"
    substeps = 4
    step_tolerance = (3e-4, 1e-6)


def _tinted(self, y, p, c):
    light = self.forcing.light
    return [y[0], y[0] * y[1], 1.1 * y[0] * (y[2] + y[4]), y[0] * (y[3] + y[5]) + 0.02 * light]


class CombinedCtl(JM.PrprDiluted):
    """Everything at once: a forcing in rhs, a jump, missing observations and an observation map of its own (which reads the
    forcing), with step control."""
    model_key = "gen_prpr_pulsed_masked_tinted_ctl4"
    substeps = 4
    missing_observations = True
    step_tolerance = TOL
    observe = _tinted


class CombinedSub4(JM.PrprDiluted):
    model_key = "gen_prpr_pulsed_masked_tinted_sub4"
    substeps = 4
    missing_observations = True
    observe = _tinted


class ReaderCtl(JM.PlateReaderDiluted):
    """A precision map of the model's own under step control: the count row sits behind the four precision rows."""
    model_key = "gen_plate_reader_student_t_diluted_ctl4"
    substeps = 4
    step_tolerance = TOL


class ReaderSub4(JM.PlateReaderDiluted):
    model_key = "gen_plate_reader_student_t_diluted_sub4"
    substeps = 4


class DenseEightCtl(IM.DenseEight):
    """The register and LDS worst case that fits a ceiling of 8: eight species, every entry of the Jacobian."""
    model_key = "gen_dense_eight_ctl8"
    substeps = 8
    step_tolerance = TOL


class DenseEightSdirkCtl(SD.DenseEightSdirk):
    model_key = "gen_dense_eight_sdirk_ctl8"
    substeps = 8
    step_tolerance = TOL


# the class without the attribute that generates the recorded text (its struct differs by the two STEP_ lines alone)
TWIN = {PulsedPrpr: PulsedPrprSub8, PulsedPrprFine: PulsedPrprSub8, PulsedPrprLoose: PulsedPrprSub8, PulsedPrprTight: PulsedPrprSub8,
        PulsedPrprTight4: PulsedPrprSub4, PulsedPrprTight2: PulsedPrprSub2, CombinedCtl: CombinedSub4, ReaderCtl: ReaderSub4}
# ... and the fixed count whose kernels a degenerate tolerance must reproduce bit for bit
FIXED_TWIN = {PulsedPrprLoose: PulsedPrprSub2, PulsedPrprTight: PulsedPrprSub8, PulsedPrprTight4: PulsedPrprSub4,
              PulsedPrprTight2: PulsedPrprSub2}
# The degenerate cases the GPU tests run, (class, solver, times).  "No interval passes" has a premise in float32: at every rung
# fine and coarse must differ by more than rounding, or they are the same bits, r = 0 and the rung passes.  problem() keeps, for a
# TIGHT class, only samples whose float64 rung differences are above RESOLVED float32 epsilons of the state on some species at
# every rung of every interval.  euler and midpoint meet that up to 8 steps; the fourth-order scheme does not -- on TIMES and on
# grids two and three times as coarse at most 1 candidate of 400 keeps Phi^2 and Phi^4 (let alone Phi^4 and Phi^8) apart by 32
# epsilons on all intervals of either of the first two data rows -- so its tight case is the ceiling 2 on the doubled grid, where Phi^1 and Phi^2 differ
RESOLVED = 64.0
EPS32 = float(torch.finfo(torch.float32).eps)
TIMES_X2 = [2.0 * t for t in TIMES]
DEGENERATE = ([(PulsedPrprLoose, s, TIMES) for s in ("euler", "midpoint", "rk4")]
              + [(c, s, TIMES) for c in (PulsedPrprTight, PulsedPrprTight4) for s in ("euler", "midpoint")]
              + [(PulsedPrprTight2, "rk4", TIMES_X2)])
MODELS = [PulsedPrpr, PulsedPrprFine, PulsedPrprLoose, PulsedPrprTight, PulsedPrprTight4, PulsedPrprTight2, PrprImplicitCtl, PrprSdirkCtl, CombinedCtl, ReaderCtl]
WIDEST = [DenseEightCtl, DenseEightSdirkCtl]  # compiled by the host test only
EXPLICIT = ("euler", "midpoint", "rk4")
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS + [PulsedPrprSub8, PulsedPrprSub4, PulsedPrprSub2]]
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


def solvers_of(cls):
    return ["beuler"] if cls.implicit else list(EXPLICIT)


# ---- the rule in torch -------------------------------------------------------------------------------------------------------------
def sub_times(t0, t1, c):
    """s_0 .. s_c of csrc/vihds_stepctl.hpp (SubGridN) in the dtype of t0."""
    hs = (t1 - t0) * (1.0 / c)
    return [t0 + j * hs for j in range(c)] + [t1]


def one_step(cls, solver, rhs, t0, t1, y, differentiable):
    """(the state after one step of the class's scheme, the last Newton increment relative to the state per trajectory [B,S] --
    zeros for an explicit scheme, infinity where it is not finite)."""
    if solver != "beuler":
        return JM.one_step(solver, rhs, t0, t1, None, y), torch.zeros(y.shape[:2], dtype=torch.float64)
    jac = (lambda f, t, z: IM.autograd_jacobian(f, t, z, create_graph=True)) if differentiable else IM.autograd_jacobian
    if int(cls.implicit_order) == 2:
        y1, _, d = SD.sdirk2_step(rhs, t0, t1, y, int(cls.newton_iterations), jac)
    else:
        y1, d = IM.newton_step(rhs, t1, t1 - t0, y, int(cls.newton_iterations), jac)
        d = d.detach().abs().amax(-1)
    rel = (d / y1.detach().abs().amax(-1).clamp_min(1e-30)).double()
    return y1, torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))


def phi(cls, solver, rhs, t0, t1, y, c, differentiable=False):
    s, worst = sub_times(t0, t1, c), torch.zeros(y.shape[:2], dtype=torch.float64)
    for j in range(c):
        y, d = one_step(cls, solver, rhs, s[j], s[j + 1], y, differentiable)
        worst = torch.maximum(worst, d)
    return y, worst


def ratio(fine, coarse, rtol, atol):
    """r [B,S] of the acceptance test over the species (the last axis); NaN where any term is."""
    q = (fine - coarse).abs() / (atol + rtol * torch.maximum(fine.abs(), coarse.abs()))
    r = q.amax(-1)
    return torch.where(torch.isnan(q).any(-1), torch.full_like(r, float("nan")), r)


def ratio_numpy(fine, coarse, rtol, atol):
    """The same number by numpy alone, one trajectory at a time (the independent restatement)."""
    with np.errstate(all="ignore"):
        q = np.abs(fine - coarse) / (atol + rtol * np.maximum(np.abs(fine), np.abs(coarse)))
    return float(np.max(q))  # (np.max propagates NaN)


def _rhs_of(cls, th, cond, times):
    return cls.torch_problem(th, cond, None, **({"times": times} if cls.forcings else {}))


def ladder(cls, th, cond, times, solver, tol=None, ceiling=None):
    """The rule for every trajectory at once, no graph: (codes [T,B,S] float64 -- entry k + 1 the interval k's, entry 0 zero --,
    every ratio a test looked at as a list of (interval, c, r [B,S], looked [B,S] bool), the states [B,S,N,T])."""
    rtol, atol = cls.step_tolerance if tol is None else tol
    M, T = int(cls.substeps) if ceiling is None else ceiling, len(times)
    with torch.no_grad():
        rhs, x0 = _rhs_of(cls, th, cond, times)
        y, codes, looked_at, lefts = x0, [torch.zeros(x0.shape[:2], dtype=x0.dtype)], [], [x0]
        for k in range(T - 1):
            u = JM.jump_at(cls, y, th, cond, k, T) if cls._jump_def is not None else y
            coarse = phi(cls, solver, rhs, times[k], times[k + 1], u, 1)[0]
            open_ = torch.ones(x0.shape[:2], dtype=torch.bool)
            code, nxt, c = torch.zeros(x0.shape[:2], dtype=x0.dtype), torch.zeros_like(x0), 1
            while bool(open_.any()):
                fine = phi(cls, solver, rhs, times[k], times[k + 1], u, 2 * c)[0]
                r = ratio(fine, coarse, rtol, atol)
                looked_at.append((k, c, r, open_.clone()))
                passed = open_ & (r <= 1.0)
                stop = passed | (open_ & (2 * c == M))
                code = torch.where(passed, torch.full_like(code, 2.0 * c), torch.where(stop, torch.full_like(code, -float(M)), code))
                nxt = torch.where(stop.unsqueeze(-1), fine, nxt)
                open_ = open_ & ~stop
                coarse, c = fine, 2 * c
            y = nxt
            codes.append(code)
            lefts.append(y)
    return torch.stack(codes), looked_at, torch.stack(lefts, dim=3)


def states(cls, th, cond, times, solver, codes, differentiable=True):
    """(the left limits [B,S,N,T] of the realised scheme: interval k with |codes[k + 1]| steps per trajectory, the counts frozen;
    the largest last Newton increment of a step that some trajectory's realised scheme took, relative to the state)."""
    T = len(times)
    rhs, x0 = _rhs_of(cls, th, cond, times)
    counts = codes.abs().round().to(torch.int64)
    y, lefts, worst = x0, [x0], 0.0
    for k in range(T - 1):
        u = JM.jump_at(cls, y, th, cond, k, T) if cls._jump_def is not None else y
        nxt = None
        for c in sorted(set(counts[k + 1].reshape(-1).tolist())):
            mine = counts[k + 1] == c
            yc, d = phi(cls, solver, rhs, times[k], times[k + 1], u, int(c), differentiable)
            worst = max(worst, float(d[mine].max()))
            nxt = yc if nxt is None else torch.where(mine.unsqueeze(-1), yc, nxt)
        y = nxt
        lefts.append(y)
    return torch.stack(lefts, dim=3), worst


def definition(cls, pb, solver, dtype, codes=None):
    """The float64 (or float32) definition of a case: the ladder in float64 unless the codes are given, then the realised scheme in
    `dtype` with autograd for the gradient of sum(logp * G).  `traj` carries the count row behind the species and precision rows."""
    lad = None
    if codes is None:
        th64 = {n: v.double() for n, v in pb["th"].items()}
        codes = (lad := ladder(cls, th64, pb["cond"], pb["times"], solver))[0]
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    xs, worst = states(cls, th, cond, times, solver, codes)
    full, xp, logp = SM.hooks(cls, xs, th, cond, obs)
    if pb.get("observed") is not None:  # (missing observations: the scoring rule of modelgen_missing_models, constant precisions)
        prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
        logp = MM.masked_sum(lambda ob: MM.gaussian_terms(xp, ob, prec), xp, obs, pb["observed"])
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    row = codes.to(dtype).permute(1, 2, 0).unsqueeze(2)  # [B,S,1,T]
    out = {"traj": torch.cat([full.detach(), row], dim=2), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
           "codes": codes, "last_increment": worst, "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()}}
    if lad is not None:
        out["looked_at"] = lad[1]
    return out


def in_band(looked_at):
    """[B,S] bool: the trajectories with a ratio inside BAND at a test that looked at them."""
    bad = None
    for _k, _c, r, looked in looked_at:
        hit = looked & (r >= BAND[0]) & (r <= BAND[1])
        bad = hit if bad is None else bad | hit
    return bad


# ---- inputs of the numeric tests: chosen on the float64 definition alone ----------------------------------------------------------
def pulse_series(B, times):
    """[B, T] light: PULSE[2] between PULSE[0] and PULSE[1] (shifted by 0.2 b from row to row), 0.3 outside."""
    t = torch.as_tensor(times, dtype=torch.float64)[None, :] - 0.2 * torch.arange(B, dtype=torch.float64)[:, None]
    return torch.where((t >= PULSE[0]) & (t <= PULSE[1]), torch.tensor(PULSE[2], dtype=torch.float64),
                       torch.tensor(0.3, dtype=torch.float64))


def smooth_pulse(B, times):
    """[B, T] light of the implicit cases (their grid is IMPLICIT_TIMES, 0 .. 0.7): 0.3 + 3 exp(-((t - 0.3 - 0.1 b) / 0.2)^2)."""
    t = torch.as_tensor(times, dtype=torch.float64)[None, :] - 0.1 * torch.arange(B, dtype=torch.float64)[:, None]
    return 0.3 + 3.0 * torch.exp(-((t - 0.3) / 0.2) ** 2)


def series_of(cls, B, times):
    T = len(times)
    keep, dose = JM.schedule(B, T)
    named = {"light": pulse_series(B, times) if "keep" in cls.forcings else smooth_pulse(B, times), "keep": keep, "dose": dose}
    return torch.stack([named[n] for n in cls.forcings], dim=1)


def problem(cls, B, S, solver, times=None, seed=31, spread=0.6):
    """Inputs of one case of the pulsed model (shared by the tests that use it; never modified): theta [B,S] per slot spread
    per sample by exp(spread eps) on the rates, the wide cond with the pulse, times, observations and an upstream gradient.  The
    samples are kept from a pool of POOL S candidates per row: those of which no ratio at any test of `cls`'s ladder under
    `solver` lies in BAND, on the float64 definition alone (a TIGHT class: those with every rung resolved, see DEGENERATE)."""
    times = (IMPLICIT_TIMES if cls.implicit else TIMES) if times is None else times
    k = (cls, B, S, solver, tuple(times), seed, spread)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    base = FM.PRPR_BASE if cls.implicit else JM.BASES[JM.PrprDiluted]
    assert sorted(slot_names(cls)) == sorted(base)
    wide = ("r", "rc", "drfp", "dyfp", "dcfp")
    th = {n: v * torch.exp((spread if n in wide else 0.2) * rnd(B, POOL * S)) for n, v in base.items()}
    series = series_of(cls, B, tt)
    cond = FM.wide_cond(torch.zeros(B, 0, dtype=torch.float64), series)
    observed = MM.gaps_mask(B, T) if cls.missing_observations else None
    if observed is not None:
        cond = torch.cat([cond, MM.words_of(observed)], dim=1)
    if cls.step_tolerance == TIGHT:  # (every rung resolved in float32: DEGENERATE)
        keep = (ladder(cls, th, cond, tt, solver, tol=(RESOLVED * EPS32, 0.0))[0][1:] < 0).all(0)
        assert int(keep.sum(1).min()) >= S, "too few candidates keep every rung resolved: %s" % keep.sum(1).tolist()
        pick = torch.stack([torch.nonzero(keep[b])[:S, 0] for b in range(B)])
        th = {name: v.gather(1, pick) for name, v in th.items()}
    elif cls.step_tolerance != LOOSE:
        keep = ~in_band(ladder(cls, th, cond, tt, solver)[1])
        assert int(keep.sum(1).min()) >= S, "too few candidates keep their ratios out of the band: %s" % keep.sum(1).tolist()
        pick = torch.stack([torch.nonzero(keep[b])[:S, 0] for b in range(B)])
        th = {name: v.gather(1, pick) for name, v in th.items()}
    else:
        th = {name: v[:, :S].contiguous() for name, v in th.items()}
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        first = IM.PrprForcedImplicit if cls.implicit else PulsedPrprSub8
        xs = JM.explicit_states(first, th1, cond, tt, "rk4")
        xp = SM.hooks(cls, xs, th1, cond, torch.zeros(B, 4, T, dtype=torch.float64))[1]
        obs = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "times": tt, "obs": obs, "W": {}, "B": B, "S": S, "T": T,
          "G": {"logp": rnd(B, S, 4)}, "observed": observed}
    _PROBLEMS[k] = pb
    return pb
