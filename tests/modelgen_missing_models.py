"""Models with missing observations (missing_observations = True of vihds.modelgen) for the tests, each the twin of an existing
test model, and the float64 yardstick of the scoring rule.

  PrprMasked                  PrprRestated: constant precisions, the kernels' Gaussian
  ReaderStudentForcedMasked   PlateReaderForced with a Student-t: its own observe, precision and log_likelihood, one forcing
  LightSub4Masked             LightSub4: one forcing, four sub-steps and process noise -- a row of cond is
                              [samples | mask words | key], which tests every offset
  PrprMaskedPrecisions        PrprRestatedPrecisions: NeuralPrecisions (WithPrec<> forwards the core's trait)
  PrprDilutedSub2Masked       PrprDiluted with substeps = 2: a jump and two sub-steps

A row of `cond` is [treatments as log(1 + c) | K x T forcing samples | T mask words | key lo, key hi]; word k of a row is
sum_j observed[j][k] * 2^j.  The yardstick states the rule on its own, in three lines (masked_sum): with m = observed,
ob' = where(m, obs, x_predict) and the term is where(m, term(ob'), 0) -- the placeholder under the mask never enters."""
import math

import torch

from oracle import vihds_oracle as O
from vihds.precisions import NeuralPrecisions

import modelgen_forcing_models as FM
import modelgen_jump_models as JM
import modelgen_likelihood_models as LM
import modelgen_sde_models as SDE
import sde_ref
from modelgen_models import PREC, PrprRestated, PrprRestatedPrecisions
from modelgen_piecewise_models import FIXED, TIMES  # noqa: F401  (FIXED: for the tests)
from vihds.modelgen import log

PREC_INIT = ["init_prec_x", "init_prec_rfp", "init_prec_yfp", "init_prec_cfp"]  # the slots NeuralPrecisions adds (WithPrec<>)
PREC_W = ("prod_w", "prod_b", "degr_w", "degr_b")  # the precision network's tensors in the weight buffer's order (no hidden layer)


class PrprMasked(PrprRestated):
    model_key = "gen_prpr_constant_masked"
    missing_observations = True


class ReaderStudentForced(FM.PlateReaderForced):
    """PlateReaderForced (its own observe and precision, both reading the logged temperature) with the Student-t of
    PlateReaderStudentT: the unmasked twin."""
    model_key = "gen_plate_reader_forced_student_t"

    def log_likelihood(self, x, obs, pr, p, c):
        def t(j):
            e = x[j] - obs[j]
            return LM.STUDENT_T_CONST + 0.5 * log(pr[j]) - 0.5 * (LM.NU + 1.0) * log(1.0 + pr[j] * e * e / LM.NU)
        return [t(j) for j in range(4)]


class ReaderStudentForcedMasked(ReaderStudentForced):
    model_key = "gen_plate_reader_forced_student_t_masked"
    missing_observations = True


class LightSub4Masked(SDE.LightSub4):
    model_key = "gen_sde_light_sub4_masked"
    missing_observations = True


class PrprMaskedPrecisions(PrprMasked):
    model_key = "gen_prpr_constant_masked_precisions"

    def __init__(self, config):
        super(PrprMaskedPrecisions, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)


class PrprDilutedSub2(JM.PrprDiluted):
    """PrprDiluted (three forcings, a scheduled dilution and bolus at the reads) with two sub-steps: the unmasked twin."""
    model_key = "gen_prpr_constant_diluted_sub2"
    substeps = 2


class PrprDilutedSub2Masked(PrprDilutedSub2):
    model_key = "gen_prpr_constant_diluted_sub2_masked"
    missing_observations = True


MODELS = [PrprMasked, ReaderStudentForcedMasked, LightSub4Masked, PrprMaskedPrecisions, PrprDilutedSub2Masked]
NEURAL = (PrprMaskedPrecisions, PrprRestatedPrecisions)
TWIN = {PrprMasked: PrprRestated, ReaderStudentForcedMasked: ReaderStudentForced, LightSub4Masked: SDE.LightSub4,
        PrprMaskedPrecisions: PrprRestatedPrecisions, PrprDilutedSub2Masked: PrprDilutedSub2}
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, cls in NEURAL) for cls in MODELS] + [(ReaderStudentForced, False), (PrprDilutedSub2, False)]

_PRPR_NEURAL = {k: v for k, v in FM.PRPR_BASE.items() if k not in PREC}
_PRPR_NEURAL.update(dict(zip(PREC_INIT, (50.0, 20.0, 20.0, 20.0))))  # (where the precision states start: the constant slots' values)
BASES = {PrprMasked: FM.PRPR_BASE, ReaderStudentForcedMasked: FM.READER_BASE, LightSub4Masked: SDE.BASES[SDE.LightSub4],
         PrprMaskedPrecisions: _PRPR_NEURAL, PrprDilutedSub2Masked: JM.BASES[JM.PrprDiluted]}
KEY = (0x5eed02, 0x0c0de5)  # the noise key of LightSub4Masked's problems: two words below 2^24
_PROBLEMS = {}


def slot_names(cls):
    if cls in NEURAL:
        return list(cls.parameter_names) + PREC_INIT
    return list(cls.parameter_names) + ([] if cls._precision_def is not None else list(PREC))


# ---- the masks ---------------------------------------------------------------------------------------------------------------------
EMPTY = (2, 2)  # (row, signal) that the gaps mask never observes


def gaps_mask(B=3, T=9):
    """observed [B,4,T] (bool) of the tests: row 0 fully observed; row 1 a fixed pseudo-random pattern; row 2 with signal 2 never
    observed, the last three points unobserved for every signal (a ragged tail) and the first point unobserved for signal 0.
    Rows behind the third repeat the three."""
    assert T >= 9
    gen = torch.Generator().manual_seed(20261)
    m = torch.ones(3, 4, T, dtype=torch.bool)
    m[1] = torch.rand(4, T, generator=gen) < 0.6
    m[2, 2, :] = False
    m[2, :, T - 3:] = False
    m[2, 0, 0] = False
    return m[torch.arange(B) % 3].clone()


def tail_mask(B, T, lost=3):
    """observed [B,4,T]: every row loses its last `lost` points."""
    m = torch.ones(B, 4, T, dtype=torch.bool)
    m[:, :, T - lost:] = False
    return m


def with_placeholders(obs, observed, kinds=(float("nan"), 1e30)):
    """obs with the entries under the mask replaced: kinds[0] for every other masked entry, kinds[1] for the rest."""
    out = obs.contiguous().clone(memory_format=torch.contiguous_format)
    at = torch.nonzero(~observed.contiguous().reshape(-1))[:, 0]
    flat = out.view(-1)
    flat[at[0::2]] = kinds[0]
    flat[at[1::2]] = kinds[1]
    return out


def words_of(observed):
    """[B,T] float64: sum_j observed[j][k] * 2^j, stated on its own (vihds.modelgen.mask_words is the library's)."""
    return sum(observed[:, j].double() * float(2 ** j) for j in range(4))


def masked_sum(terms_of, xp, obs, observed):
    """The scoring rule, stated on its own: sum over time of where(m, terms_of(ob'), 0) with ob' = where(m, obs, x_predict)."""
    m = observed.bool()[:, None].expand(xp.shape)
    ob = torch.where(m, obs.to(xp.dtype)[:, None].expand(xp.shape), xp.detach())
    return torch.where(m, terms_of(ob), torch.zeros((), dtype=xp.dtype)).sum(3)


def gaussian_terms(xp, ob, prec):
    return -0.5 * (math.log(2.0 * math.pi) - torch.log(prec) + prec * (xp - ob) ** 2)


def student_t_terms(xp, ob, prec):
    """ReaderStudentForced's density with torch ops: Student-t of LM.NU degrees of freedom, scale 1 / sqrt(precision)."""
    e = xp - ob
    return LM.STUDENT_T_CONST + 0.5 * torch.log(prec) - 0.5 * (LM.NU + 1.0) * torch.log(1.0 + prec * e * e / LM.NU)


# ---- the definition in torch -----------------------------------------------------------------------------------------------------
def series_of(cls, B, times):
    """The forcing samples of a class [B, K, T], in the order of cls.forcings."""
    T = len(times)
    if not cls.forcings:
        return torch.zeros(B, 0, T, dtype=torch.float64)
    if issubclass(cls, JM.PrprDiluted):
        return JM.series_of(cls, B, times)
    if issubclass(cls, SDE.LightSub4):
        return SDE.smooth_series(B, times)[:, None, :]
    return FM.series_of(cls, B, times)


def cond_of(cls, treatments, series, observed=None, key=KEY):
    """A row of cond as the kernels take it: [log(1 + treatment) | samples | mask words (a masked class) | key (process noise)].
    observed None: every point observed (word 15)."""
    B, T = series.shape[0], series.shape[2]
    parts = [torch.log1p(treatments).reshape(B, -1), series.reshape(B, -1)]
    if cls.missing_observations:
        parts.append(torch.full((B, T), 15.0, dtype=torch.float64) if observed is None else words_of(observed))
    if cls._diffusion_def is not None:
        parts.append(torch.tensor([float(key[0]), float(key[1])], dtype=torch.float64)[None, :].expand(B, 2))
    return torch.cat(parts, dim=1)


def draws_of(cls, B, S, T, key=KEY):
    """xi [B,S,N,(T-1)*substeps] of a class with process noise under `key` (tests/sde_ref.py), None for every other class."""
    if cls._diffusion_def is None:
        return None
    return torch.from_numpy(sde_ref.expected_draws(B, S, len(cls.species), SDE.n_steps(cls, T), key))


def states(cls, th, cond, times, solver, xi=None, prec_w=None):
    """The stored rows [B,S,N(+4),T] of the scheme in th's dtype (differentiable): the twins' own definitions."""
    if cls._diffusion_def is not None:
        return SDE.forward(cls, th, cond, times, solver, None, xi)[0]
    if cls._jump_def is not None or cls.substeps > 1:
        return JM.explicit_states(cls, th, cond, times, solver)
    rhs, x0 = cls.torch_problem(th, cond, None, **({"times": times} if cls.forcings else {}))
    if cls in NEURAL:
        rhs = O._with_precisions(rhs, len(cls.species), {k: v.to(x0.dtype) for k, v in prec_w.items()})
        x0 = torch.cat([x0, torch.stack([th[n] for n in PREC_INIT], dim=2)], dim=2)
    return O.simulate(rhs, x0, times, solver)


def forward(cls, th, cond, times, solver, obs=None, observed=None, xi=None, prec_w=None):
    """The float64 (or float32) definition: the stored rows [B,S,N(+4),T], x_predict [B,S,4,T] and, given observations, the
    per-signal log-likelihood [B,S,4] under the mask `observed` [B,4,T] (None: every point)."""
    sol = states(cls, th, cond, times, solver, xi, prec_w)
    xs, prec = O.split_neural_precisions(sol) if cls in NEURAL else (sol, None)
    if cls._observe_def is not None:
        xp = cls.torch_observe(xs, th, cond)
    else:
        xp = O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)
    full = sol
    if cls._precision_def is not None:
        prec = cls.torch_precision(xs, th, cond)
        full = torch.cat([xs, prec], dim=2)
    elif prec is None:
        prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    if obs is None:
        return full, xp, None
    if observed is None:
        observed = torch.ones(obs.shape, dtype=torch.bool)
    # (the densities are written out here: neither the kernels nor the library's host restatement is on this side)
    assert cls._likelihood_def is None or issubclass(cls, ReaderStudentForced)
    terms = student_t_terms if cls._likelihood_def is not None else gaussian_terms
    logp = masked_sum(lambda ob: terms(xp, ob, prec), xp, obs, observed)
    return full, xp, logp


def definition(cls, pb, solver, dtype, observed=None, obs=None):
    """The definition in `dtype` with autograd for the gradient of sum(logp * G) with respect to theta and the precision
    network's weights.  observed / obs: another mask and other observations than the problem's."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    W = {k: leaf(v) for k, v in pb["prec_w"].items()} if pb["prec_w"] else None
    observed = pb["observed"] if observed is None else observed
    cond = cond_of(cls, pb["treatments"], pb["series"], observed).to(dtype)
    full, xp, logp = forward(cls, th, cond, pb["times"].to(dtype), solver, (pb["obs"] if obs is None else obs).to(dtype), observed,
                             pb["xi"], W)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    loss.backward()
    terms = (logp * pb["G"]["logp"].to(dtype)).detach()
    return {"traj": full.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(),
            "condition": float(terms.abs().sum() / terms.sum().abs()),  # (1: no cancellation in the loss)
            "g_theta": {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in th.items()},
            "g_w": [W[k].grad for k in PREC_W] if W else []}


def problem(cls, B, S, times=TIMES, seed=29, mask=gaps_mask):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, treatments and series, the
    mask, observations (the first sample's noise-free prediction with 5 % scatter, NaN / 1e30 under the mask) and their clean
    copy, an upstream gradient for the log-likelihood of one sign, the draws of a class with process noise."""
    k = (cls, B, S, tuple(times), seed, mask.__name__)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    assert sorted(slot_names(cls)) == sorted(BASES[cls])
    spread = 0.1 if cls._diffusion_def is not None else 0.2
    th = {n: v * torch.exp(spread * rnd(B, S)) for n, v in BASES[cls].items()}
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = series_of(cls, B, tt)
    observed = mask(B, T)
    prec_w = None
    if cls in NEURAL:
        nin = len(cls.species) + 1
        prec_w = {"prod_w": 0.3 * rnd(4, nin), "prod_b": 0.3 * rnd(4), "degr_w": 0.3 * rnd(4, nin), "degr_b": 0.3 * rnd(4)}
    xi = draws_of(cls, B, S, T)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        quiet = None if xi is None else torch.zeros_like(xi[:, :1])
        _, xp, _ = forward(cls, th1, cond_of(cls, treatments, series, observed), tt, "rk4", xi=quiet, prec_w=prec_w)
        clean = xp[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "treatments": treatments, "series": series, "times": tt, "observed": observed, "clean": clean,
          "obs": with_placeholders(clean, observed), "prec_w": prec_w, "xi": xi, "B": B, "S": S, "T": T,
          "G": {"logp": 0.5 + torch.rand(B, S, 4, generator=gen, dtype=torch.float64)}}
    pb["cond"] = cond_of(cls, treatments, series, observed)
    _PROBLEMS[k] = pb
    return pb


def flat_weights(pb):
    """The precision network's weights as the kernels take them (float64, [n]); None for a class without."""
    return torch.cat([pb["prec_w"][k].reshape(-1) for k in PREC_W]) if pb["prec_w"] else None

