"""The ELBO-side kernels (csrc/vihds_elbo.hip, csrc/vihds_offset.hip) across the shapes that select their code paths, each
against a plain float64 restatement on the CPU, through the C ABI (so that a case can take the path `ops` never picks).

Which branch each case exists for
  vihds_theta_fwd   theta_fwd_lds_kernel while THETA_LDS_FIELDS * min(B, 63/S + 2) * P * 4 <= 48 KB, else theta_fwd_kernel:
                    (5,3,7) one ragged block over three rows; (30,36,1) largest S = 1 table inside the limit; (31,70,1) and
                    (40,40,2) the global-table fallback; (13,5,100) blocks that span rows with n % 64 != 0; (4,1,64) exactly
                    one full block, P = 4; (33,2,65) P % 4 = 1 with a one-trajectory last block.  Generator advance: 256
                    blocks (tickets), 257 blocks (the one-thread launch behind the kernel), the fallback's own tickets.
  vihds_theta_bwd   S 1 / 63 / 64 / 65 (a wavefront's first prefetch round: part, full, one over), 256 / 257 / 300 (four
                    rounds full, then the tail loop); P 1 / 4 / 5 / 9 (idle wavefronts in the last chunk of
                    THETA_BWD_PCHUNK); B 1 / 5; constants; g_theta_scale; q_rows + log-precision adjoint; the in-launch IWAE
                    job (loss, ticket, replay); each upstream gradient NULL once.
  vihds_iwae_*      iwae_path: "rows" (ticket, S <= 1024), "small" (no ticket, B <= 64, S <= 256), "two_launch"; both sides
                    of S 256|257, B 64|65, S 1024|1025, and S = 1, B = 1.  vihds_iwae_combine: more rows than its 16
                    wavefronts (B 40), 1 / 2 / 3 / 8 ranks.
  vihds_offset_rows_bwd   offset_bwd_path: "registers" (B <= RB * 16, S <= SC * 64) against "loop": (48,256) | (49,256),
                    (48,257), plus (3,5) and (100,70).
  vihds_device_condition  one ragged block, several blocks, 257 blocks (generator advance by the separate launch), and a
                    shard (S_total, s_offset) whose B does not divide S_total.
  vihds_gather_batch  clamped and repeated indices, C4*T = 8 (T = 2), 344 (> 256 threads), 15; n_tr / D = 0; no delta_obs.
  vihds_adam_step   tensors of 1, 1023, 1024, 1025, 2049 elements around ADAM_CHUNK with a gradient-less tensor between
                    them, grad_scale 0.125, a device learning rate that changes, 32 | 33 tensors.
The Python mirror of the host-side predicates (`theta_fwd_path`, `iwae_path`, `offset_bwd_path`; constants read from the
.hip sources) checks on the CPU that every case lands where its label says and that every branch is named by a case.

Restatements (float64 torch, CPU): `theta_ref` (anchored to oracle.sample_clip_theta / chained_log_prob on a committed
fixture), `iwae_ref`, `condition_ref` (anchored to oracle.device_conditioner), `offset_fwd_ref` / `offset_bwd_ref`,
`gather_ref`, `adam_ref`; the expected draws come from tests/philox_ref.py.

Inputs of the IWAE cases: per-signal log-likelihoods N(-200, 50^2) -- sums over a plate's time points are large and
negative, so |log w| ~ 800 and the float32 sum of six terms (<= 3 ulp(800) ~ 2e-4 absolute) stays inside 1e-6 relative --
and one set with log-weights N(-1e4, 1e3^2) for the max subtraction.  d loss / d log_w is compared with the float64
softmax at the launch's OWN float32 log-weights (which are checked on their own against the float64 sum), for the reason
given in test_encoder_tail_shapes.py: a float64 sum behind the softmax would measure the conditioning of exp, not the
kernel.  What remains is the rounding of lse = max + log(sumexp) to float32, at most ulp(|lse|)/2 = 4.9e-4 for
|lse| < 16384, under GTOL.

Tolerances the suite already has for the same quantity
  theta 1e-5 per parameter row (test_encoder_tail_shapes.py, q tables / test_oracle_golden.py forward); values (log q,
  log p) TOL 1e-4 and gradients GTOL 5e-4 per parameter row (test_hip_parity.py, test_decoder_dispatch_shapes.py); loss, lse and log-weights
  1e-6 (test_encoder_tail_shapes.py TOL_LOSS); Adam 2e-6 (test_hip_parity.py::test_adam_step_matches_torch_adam); in-kernel
  normals 1e-4 absolute against philox_ref and conditioner outputs from them 1e-4 (test_hip_parity.py: hardware log / sin /
  cos); offset-layer forward and routed gradient allclose(1e-6, 1e-6) (test_hip_parity.py::test_offset_rows_against_torch).
Quantities without one get 8 x the error of the float32 run of the same restatement against its float64 run, the largest
over this module's own cases (test_float32_run_of_the_restatements_stays_inside_a_quarter_of_the_measured_bounds
re-measures; sums are taken sequentially in float32, the least favourable legitimate order):
  row max              measured 1.37e-07  -> ROW_MAX_TOL     1.1e-06
  row sum-exp          measured 1.37e-04  -> ROW_SUMEXP_TOL  1.1e-03   (the float32 rounding of log w, ~1e-4, exponentiated)
  offset layer g_W     measured 2.59e-07  -> OFFSET_GW_TOL   2.1e-06
  offset layer g_bias  measured 1.61e-07  -> OFFSET_GB_TOL   1.3e-06
  conditioner output   measured 9.99e-08  -> COND_TOL        8.0e-07
Every GPU case prints its largest error next to its tolerance.
"""
import ctypes
import math
import os
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

from fixture_util import Fixture, rel_err
from oracle import vihds_oracle as O
from philox_ref import expected_kernel_normals, philox4x32_10

DEV = "cuda:0"
gpu = pytest.mark.gpu
NORMAL, LOGNORMAL, CONSTANT = 0, 1, 2
TOL_THETA, TOL, GTOL, TOL_LOSS, TOL_ADAM, TOL_U = 1e-5, 1e-4, 5e-4, 1e-6, 2e-6, 1e-4
ROW_MAX_TOL, ROW_SUMEXP_TOL, OFFSET_GW_TOL, OFFSET_GB_TOL, COND_TOL = 1.1e-6, 1.1e-3, 2.1e-6, 1.3e-6, 8.0e-7
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vi-hds_amd", "csrc")
SENTINEL = 1234.5
F64 = torch.float64


# ---- constants read from the sources ----------------------------------------------------------------------------------
def _grab(text, pattern, what):
    m = re.search(pattern, text)
    assert m is not None, "source changed under the mirror: %s (%r)" % (what, pattern)
    return tuple(int(g) for g in m.groups() if g)


@lru_cache(maxsize=None)
def consts():
    read = lambda f: open(os.path.join(CSRC, f)).read()  # noqa: E731
    elbo, off, api = read("vihds_elbo.hip"), read("vihds_offset.hip"), read("vihds_api.hip")
    c = {}
    for name in ("THETA_LDS_FIELDS", "RNG_TICKET_BLOCKS", "THETA_BWD_PCHUNK", "ADAM_CHUNK"):
        (c[name],) = _grab(elbo, r"constexpr int %s = (\d+);" % name, name)
    (c["OFFSET_BWD_THREADS"],) = _grab(off, r"constexpr int OFFSET_BWD_THREADS = (\d+);", "OFFSET_BWD_THREADS")
    c["RB"], c["SC"] = _grab(off, r"constexpr int RB = (\d+), SC = (\d+);", "RB, SC")
    _grab(off, r"if \(B <= RB \* \(OFFSET_BWD_THREADS / 64\) && S <= SC \* 64 && n_waves == OFFSET_BWD_THREADS / 64\)()",
          "offset_rows_bwd_kernel: register path predicate")
    c["nb"] = _grab(elbo, r"const int nb_max = min\(B, (\d+) / S \+ (\d+)\);", "launch_theta_fwd: nb_max")
    (c["theta_lds_kb"],) = _grab(elbo, r"if \(lds <= (\d+) \* 1024\) \{", "launch_theta_fwd: LDS limit")
    _grab(elbo, r"const size_t lds = \(size_t\)THETA_LDS_FIELDS \* nb_max \* P \* sizeof\(float\);()", "launch_theta_fwd: LDS bytes")
    c["theta_lds_blocks"] = _grab(elbo, r"const int blocks = \(n \+ (\d+)\) / (\d+);\s+const int advance = blocks <= RNG_TICKET_BLOCKS;",
                                  "launch_theta_fwd: blocks of the LDS kernel")
    (c["theta_global_blk"],) = _grab(elbo, r"const int n = B \* S, blk = (\d+);\s+const int nb_max", "launch_theta_fwd: blk")
    _grab(elbo, r"hipLaunchKernelGGL\(theta_fwd_kernel, dim3\(\(4 \* n \+ blk - 1\) / blk\), dim3\(blk\)()",
          "launch_theta_fwd: grid of the fallback")
    (c["bwd_prefetch"],) = _grab(elbo, r"for \(int sidx = lane \+ (\d+); sidx < S; sidx \+= 64\)", "theta_bwd_kernel: tail loop")
    (c["cond_blk"],) = _grab(elbo, r"const int n = B \* S, blk = (\d+);\s+const int blocks = \(n \+ blk - 1\) / blk;\s+"
                                   r"const int advance = blocks <= RNG_TICKET_BLOCKS;", "launch_device_condition: blk")
    (c["iwae_rows_S"],) = _grab(api, r"if \(ticket && S <= (\d+)\) \{", "vihds_iwae_loss_fwd: rows path")
    c["iwae_small"] = _grab(api, r"if \(B <= (\d+) && S <= (\d+)\) \{  // one launch, one block", "vihds_iwae_loss_fwd: small path")
    c["unit_grad"] = _grab(api, r"return \(\(with_ticket && S <= (\d+)\) \|\| \(B <= (\d+) && S <= (\d+)\)\) \? 1 : 0;",
                           "vihds_iwae_loss_unit_grad")
    (c["adam_max"],) = _grab(open(os.path.join(CSRC, "..", "..", "include", "vihds_hip.h")).read(),
                             r"#define VIHDS_ADAM_MAX_TENSORS (\d+)", "VIHDS_ADAM_MAX_TENSORS")
    return c


# ---- Python mirror of the host-side predicates ------------------------------------------------------------------------
def theta_fwd_path(P, B, S):
    """launch_theta_fwd's choice: the kernel, the data rows a block's table holds, the grid, and whether the blocks take
    tickets to advance the generator (else a one-thread launch follows)."""
    c = consts()
    n = B * S
    nb_max = min(B, c["nb"][0] // S + c["nb"][1])
    lds = c["THETA_LDS_FIELDS"] * nb_max * P * 4
    if lds <= c["theta_lds_kb"] * 1024:
        add, div = c["theta_lds_blocks"]
        blocks = (n + add) // div
        return dict(path="lds", nb_max=nb_max, blocks=blocks, tickets=blocks <= c["RNG_TICKET_BLOCKS"], lds=lds)
    blk = c["theta_global_blk"]
    return dict(path="global", nb_max=nb_max, blocks=(4 * n + blk - 1) // blk, tickets=True, lds=lds)


def iwae_path(B, S, ticket):
    c = consts()
    if ticket and S <= c["iwae_rows_S"]:
        return "rows"
    if B <= c["iwae_small"][0] and S <= c["iwae_small"][1]:
        return "small"
    return "two_launch"


def iwae_unit_grad(B, S, ticket):
    return iwae_path(B, S, ticket) != "two_launch"


def offset_bwd_path(B, S):
    c = consts()
    return "registers" if B <= c["RB"] * (c["OFFSET_BWD_THREADS"] // 64) and S <= c["SC"] * 64 else "loop"


def condition_blocks(B, S):
    return -(-B * S // consts()["cond_blk"])


# ---- the GPU cases ----------------------------------------------------------------------------------------------------
THETA_FWD_CASES = [
    # (P, B, S, kernel, what the case is for)
    (5, 3, 7, "lds", "one ragged block over three rows"),
    (30, 36, 1, "lds", "S 1: 36 rows in one block's table"),
    (31, 70, 1, "global", "S 1: 65-row table past 48 KB"),
    (40, 40, 2, "global", "33-row table past 48 KB"),
    (13, 5, 100, "lds", "blocks span rows, n % 64 != 0"),
    (4, 1, 64, "lds", "exactly one full block"),
    (33, 2, 65, "lds", "P % 4 = 1, one trajectory in the last block"),
]
THETA_ADVANCE_CASES = [
    # (P, B, S, kernel, blocks, tickets)
    (5, 128, 128, "lds", 256, True),
    (5, 257, 64, "lds", 257, False),
    (31, 70, 1, "global", 5, True),
]
THETA_BWD_S = [1, 63, 64, 65, 256, 257, 300]
THETA_BWD_B = [1, 5]
THETA_BWD_P = [1, 4, 5, 9]
IWAE_CASES = [
    # (B, S, path with a ticket, path without)
    (1, 1, "rows", "small"),
    (36, 200, "rows", "small"),
    (64, 256, "rows", "small"),
    (65, 256, "rows", "two_launch"),
    (64, 257, "rows", "two_launch"),
    (3, 1024, "rows", "two_launch"),
    (3, 1025, "two_launch", "two_launch"),
    (70, 300, "rows", "two_launch"),
]
IWAE_N_TOTAL = {(36, 200): 400}  # n_iwae_total != S once
IWAE_PAIR = (5, 300)             # vihds_iwae_fwd + vihds_iwae_bwd
COMBINE_RANKS, COMBINE_B, COMBINE_S_TOTAL = [1, 2, 3, 8], [5, 40], 48
OFFSET_CASES = [(48, 256, "registers"), (49, 256, "loop"), (48, 257, "loop"), (3, 5, "registers"), (100, 70, "loop")]
OFFSET_DN = [(1, 1), (12, 3), (1, 3), (12, 1)]
COND_CASES = [
    # (B, S, blocks, s_offset of the shard checked against the unsharded call)
    (5, 7, 1, 3),
    (7, 100, 3, 37),
    (257, 256, 257, 128),
]
COND_E, COND_D = 3, [1, 7]
GATHER_CT = [(4, 2), (4, 86), (3, 5)]
ADAM_SIZES = [1, 1023, 1024, None, 1025, 2049]  # None: the tensor without a gradient (7 elements)


# ---- float64 restatements ---------------------------------------------------------------------------------------------
def _normal_lp(mu, prec, v):
    return -math.log(2.0 * math.pi) + 0.5 * (prec + 1e-12).log() - 0.5 * prec * (mu - v) ** 2


def theta_ref(kind, q_mu, q_prec_or_log, q_rows, p_mu, p_prec, lo, hi, u, prec_is_log=False, parts=False):
    """theta [P,B,S] = clip(sample(q, u)), log q and log p [B,S] (reference distributions.py:64-85,119-142,327-381):
    q_mu / q_prec_or_log are tables [R,B]; q_rows None (parameter p = row p of both) or [2P] (rows of mu, then rows of the
    precision); u [B,S,P].  Constants give 0*u + mu, carry no trainable parameter (their value is detached: encoders.py
    :242-253) and contribute nothing to log q / log p; their clip bounds are ignored.  parts=True also returns the
    unclipped sample."""
    P = kind.shape[0]
    rows = torch.arange(P).repeat(2) if q_rows is None else q_rows.long()
    ln, cst = (kind == LOGNORMAL)[:, None, None], (kind == CONSTANT)[:, None, None]
    mu = q_mu[rows[:P]][:, :, None]
    pr = q_prec_or_log[rows[P:]][:, :, None]
    prec = torch.where(cst, torch.ones_like(pr), pr.exp() if prec_is_log else pr)
    uu = u.permute(2, 0, 1)
    z = mu + (1.0 / prec.sqrt()) * uu
    xr = torch.where(ln, torch.where(ln, z, torch.zeros_like(z)).exp(), z)
    lo3, hi3 = lo[:, None, None], hi[:, None, None]
    x = torch.where(cst, xr, torch.maximum(torch.minimum(xr, hi3), lo3))
    log_x = (torch.where(ln, x, torch.ones_like(x)) + 1e-12).log()
    v = torch.where(ln, log_x, x)
    jac = torch.where(ln, log_x, torch.zeros_like(x))
    zero = torch.zeros_like(x)
    log_q = torch.where(cst, zero, _normal_lp(mu, prec, v) - jac).sum(0)
    log_p = torch.where(cst, zero, _normal_lp(p_mu[:, None, None], p_prec[:, None, None], v) - jac).sum(0)
    theta = torch.where(cst, (0.0 * uu + mu).detach(), x)
    return (theta, log_q, log_p, xr) if parts else (theta, log_q, log_p)


def iwae_ref(logp, log_p, log_q, n_total):
    """training.py:135-149 with the kernels' order of the six-term sum: log_w, row max, row sum-exp, lse, loss and
    d loss / d log_w = -softmax / B."""
    lw = ((logp[0] + logp[1]) + logp[2]) + logp[3]
    lw = lw + (log_p if log_p is not None else 0.0) - (log_q if log_q is not None else 0.0)
    m = lw.max(1).values
    se = _seq_sum((lw - m[:, None]).exp(), 1)
    lse = m + se.log()
    loss = -_seq_sum(lse - math.log(n_total), 0) / lw.shape[0]
    return dict(log_w=lw, row_max=m, row_sumexp=se, lse=lse, loss=loss, g_logw=softmax_grad(lw, lse))


def softmax_grad(log_w, lse):
    return -(1.0 / log_w.shape[0]) * (log_w - lse[:, None]).exp()


def _seq_sum(x, dim):
    """Sum in index order (what a float32 run needs to be the least favourable legitimate order)."""
    return x.cumsum(dim).select(dim, -1)


def condition_ref(z, dev1hot, rel, is_default, w_mean, w_std, B, S, S_total=None, s_off=0):
    """OdeModel.device_conditioner applied to ones (ode.py:43-58) for E parameters: out[e][b][s] = default_e +
    relu(sum_d (w_mean + w_std z[e][d]) dev1hot[r][d] rel[e][d]), r = (b S_total + s_off + s) mod B."""
    S_total = S if S_total is None else S_total
    b, s = torch.meshgrid(torch.arange(B), torch.arange(S), indexing="ij")
    r = (b * S_total + s_off + s) % B
    hot = dev1hot[r][None] * rel[:, None, None, :]                     # [E,B,S,D]
    c = _seq_sum((w_mean + w_std * z)[:, None, None, :] * hot, 3)
    return is_default.to(c.dtype)[:, None, None] + torch.relu(c)


def offset_fwd_ref(theta, W, bias, dev1hot, src, dst):
    n = W.shape[0]
    out = theta.clone()
    off = _seq_sum(W[None] * dev1hot[:, None, :], 2) + bias[None]      # [B,n]
    out[dst:dst + n] = theta[src:src + n] + off.t()[:, :, None]
    return out


def offset_bwd_ref(g_theta, dev1hot, n, src, dst, accumulate):
    """Routed gradient [R,B,S] and the layer's (g_W [n,D], g_bias [n]); accumulate = 0 assigns the source rows."""
    out = g_theta.clone()
    g = g_theta[dst:dst + n]
    out[src:src + n] = g_theta[src:src + n] + g if accumulate else g
    rs = _seq_sum(g, 2)                                               # [n,B]
    return out, _seq_sum(rs[:, :, None] * dev1hot[None], 1), _seq_sum(rs, 1)


def gather_ref(idx, obs_src, inputs_src, dev1hot_src):
    r = idx.clamp(0, obs_src.shape[0] - 1)
    obs = obs_src[r]
    return obs, inputs_src[r], dev1hot_src[r], obs[:, :, 1:] - obs[:, :, :-1]


def adam_ref(params, grads, m, v, count, lr, beta1, beta2, eps, grad_scale, gate=None):
    """training.py:82,338 (torch.optim.Adam's arithmetic, no weight decay, no amsgrad) in place on lists of tensors; a
    tensor whose gradient is None is skipped, a non-finite gate skips the whole step.  Returns the new step count."""
    if gate is not None and not math.isfinite(gate):
        return count
    t = count + 1
    for p, g, mm, vv in zip(params, grads, m, v):
        if g is None:
            continue
        ge = g * grad_scale
        mm += (ge - mm) * (1.0 - beta1)
        vv.mul_(beta2).add_((1.0 - beta2) * ge * ge)
        p -= lr / (1.0 - beta1 ** t) * (mm / (vv.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps))
    return t


def conditioner_normals(E, D, seed, step):
    """The z the device conditioner draws (csrc/vihds_elbo.hip: counter (e D + d, 0xC04D, step, 0), first normal)."""
    idx = np.arange(E * D, dtype=np.uint64)
    r = philox4x32_10(idx, np.full_like(idx, 0xC04D), np.full_like(idx, step), np.zeros_like(idx),
                      np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    u1 = np.minimum((r[0].astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32), np.float32(0.99999994))
    u2 = (r[1].astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    z = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
    return torch.tensor(z.reshape(E, D).astype(np.float32), dtype=F64)


# ---- seeded inputs (float32 values held in float64: both sides see the same numbers) -----------------------------------
def _f32(t):
    return t.float().double()


KIND_CYCLE = (LOGNORMAL, NORMAL, CONSTANT, LOGNORMAL, NORMAL)


def theta_problem(P, B, S, seed, packed=False):
    """Mixed kinds (KIND_CYCLE), every third parameter with clip bounds at +-0.9 sigma around its centre (10-30 % of the
    samples clipped at each end), the rest at +-6 sigma.  Normal centres lie 2..3 away from 0, so no bound is near 0.
    packed: q_mu / q_prec are tables of P + 3 rows read through a permuted q_rows, the precision table holds logs."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=F64)    # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    kind = torch.tensor([KIND_CYCLE[p % 5] for p in range(P)])
    ln, cst = kind == LOGNORMAL, kind == CONSTANT
    sign = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0).double()
    centre = torch.where(ln, 2.0 * rand(P) - 1.0, sign * (2.0 + rand(P)))
    sigma = 0.2 + 0.3 * rand(P)
    mu = centre[:, None] + 0.1 * sigma[:, None] * randn(P, B)
    prec = (1.0 / sigma ** 2)[:, None] * (0.1 * randn(P, B)).exp()
    mu[cst] = rand(int(cst.sum()), B)
    prec[cst] = 1.0
    tight = (torch.arange(P) % 3 == 0) & ~cst
    width = torch.where(tight, 0.9, 6.0) * sigma
    lo, hi = centre - width, centre + width
    lo, hi = torch.where(ln, lo.exp(), lo), torch.where(ln, hi.exp(), hi)
    lo[cst] = 0.0
    hi[cst] = 0.0
    pr = dict(P=P, B=B, S=S, kind=kind, tight=tight, packed=packed, p_mu=_f32(centre + 0.3 * sigma * randn(P)),
              p_prec=_f32(1.0 / (2.0 * sigma) ** 2), lo=_f32(lo), hi=_f32(hi), u=_f32(randn(B, S, P)), seed=seed)
    if packed:
        R = P + 3
        rows = torch.cat([torch.randperm(R, generator=g)[:P], torch.randperm(R, generator=g)[:P]])
        q_mu, q_pr = randn(R, B), randn(R, B)
        q_mu[rows[:P]] = mu
        q_pr[rows[P:]] = prec.log()
        pr.update(q_rows=rows, q_mu=_f32(q_mu), q_prec=_f32(q_pr))
    else:
        pr.update(q_rows=None, q_mu=_f32(mu), q_prec=_f32(prec))
    return pr


def theta_eval(pr, dtype=F64, grad=False, u=None):
    """theta_ref on a problem; grad=True: the q tables are leaves."""
    c = lambda k: pr[k].to(dtype)  # noqa: E731
    q_mu, q_prec = c("q_mu").clone().requires_grad_(grad), c("q_prec").clone().requires_grad_(grad)
    out = theta_ref(pr["kind"], q_mu, q_prec, pr["q_rows"], c("p_mu"), c("p_prec"), c("lo"), c("hi"),
                    (pr["u"] if u is None else u).to(dtype), prec_is_log=pr["packed"], parts=True)
    return out + (q_mu, q_prec)


def near_a_bound(pr):
    """[B,S,P] mask: the float64 unclipped sample lies within 1e-4 relative of a clip bound (constants have none)."""
    xr = theta_eval(pr)[3]
    lo, hi = pr["lo"][:, None, None], pr["hi"][:, None, None]
    near = ((xr - lo).abs() <= 1e-4 * lo.abs()) | ((xr - hi).abs() <= 1e-4 * hi.abs())
    return (near & (pr["kind"] != CONSTANT)[:, None, None]).permute(1, 2, 0)


def settle_draws(pr):
    """Resample (fixed seed) the draws whose float64 sample sits within 1e-4 relative of a clip bound: a float32 sample
    there may fall on the other side, where the clamp's derivative jumps.  No sample is excluded from any comparison."""
    g = torch.Generator().manual_seed(pr["seed"] + 1000)
    n_resampled = 0
    for _ in range(50):
        near = near_a_bound(pr)
        if not bool(near.any()):
            break
        n_resampled += int(near.sum())
        pr["u"][near] = _f32(torch.randn(int(near.sum()), generator=g, dtype=F64))
    return n_resampled


def clipped_fractions(pr):
    """Fractions of the tight parameters' samples clipped at the lower and at the upper bound (float64)."""
    if not bool(pr["tight"].any()):
        return None
    xr = theta_eval(pr)[3][pr["tight"]]
    lo, hi = pr["lo"][pr["tight"]][:, None, None], pr["hi"][pr["tight"]][:, None, None]
    return float((xr < lo).double().mean()), float((xr > hi).double().mean()), xr.numel()


def iwae_inputs(B, S, seed, wide=False):
    """logp [4,B,S], log_p, log_q [B,S].  wide: log-weights N(-1e4, 1e3^2), else per-signal N(-200, 50^2)."""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    logp = (-2500.0 + 500.0 * randn(4, B, S)) if wide else (-200.0 + 50.0 * randn(4, B, S))
    return _f32(logp), _f32(-30.0 + 5.0 * randn(B, S)), _f32(-25.0 + 5.0 * randn(B, S))


def offset_inputs(B, S, D, n, seed):
    g = torch.Generator().manual_seed(seed)
    R, src, dst = 2 * n + 3, 1, n + 2
    dev = torch.zeros(B, D, dtype=F64)
    dev[torch.arange(B), torch.arange(B) % D] = 1.0
    dev = _f32(dev + 0.1 * torch.rand(B, D, generator=g, dtype=F64))
    return dict(R=R, src=src, dst=dst, dev=dev, W=_f32(torch.randn(n, D, generator=g, dtype=F64)),
                bias=_f32(torch.randn(n, generator=g, dtype=F64)), theta=_f32(torch.randn(R, B, S, generator=g, dtype=F64)),
                g_theta=_f32(torch.randn(R, B, S, generator=g, dtype=F64)))


def condition_inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.zeros(B, D, dtype=F64)
    dev[torch.arange(B), torch.randint(0, D, (B,), generator=g)] = 1.0
    dev = _f32(dev + 0.05 * torch.rand(B, D, generator=g, dtype=F64))
    rel = torch.tensor([[1.0 if (d + e) % 3 != 1 else 0.0 for d in range(D)] for e in range(COND_E)], dtype=F64)
    dflt = torch.tensor([1, 0, 1], dtype=torch.int32)
    return dev, rel, dflt, _f32(torch.randn(COND_E, D, generator=g, dtype=F64))


# ---- 0. CPU: constants, mirror, branch coverage ------------------------------------------------------------------------
def test_source_constants_are_read_and_consistent():
    """Every constant and formula the mirror uses is found in the sources (a changed source fails here, not silently in the
    GPU cases' labels), and the pieces fit each other."""
    c = consts()
    assert c["theta_lds_blocks"] == (c["nb"][0], c["nb"][0] + 1) and c["theta_global_blk"] == c["nb"][0] + 1
    assert c["THETA_LDS_FIELDS"] == 10 and c["theta_lds_kb"] <= 64 and c["RNG_TICKET_BLOCKS"] >= 1
    assert c["bwd_prefetch"] == 4 * 64 and c["THETA_BWD_PCHUNK"] == 4
    assert c["unit_grad"] == (c["iwae_rows_S"],) + c["iwae_small"]
    assert c["OFFSET_BWD_THREADS"] % 64 == 0 and c["adam_max"] == 32 and c["ADAM_CHUNK"] == 1024 and c["cond_blk"] == 256


def test_every_gpu_case_lands_in_the_branch_it_names_and_every_branch_is_named():
    c = consts()
    seen = set()
    for P, B, S, path, _ in THETA_FWD_CASES:
        br = theta_fwd_path(P, B, S)
        assert br["path"] == path, (P, B, S, br)
        seen.add(("theta", path))
    assert theta_fwd_path(30, 36, 1)["lds"] <= 48 * 1024 < theta_fwd_path(31, 70, 1)["lds"]
    assert theta_fwd_path(13, 5, 100)["nb_max"] == 2 and (5 * 100) % 64 != 0 and theta_fwd_path(5, 3, 7)["nb_max"] == 3
    assert theta_fwd_path(4, 1, 64)["blocks"] == 1 and theta_fwd_path(33, 2, 65)["blocks"] == 3
    for P, B, S, path, blocks, tickets in THETA_ADVANCE_CASES:
        br = theta_fwd_path(P, B, S)
        assert (br["path"], br["blocks"], br["tickets"]) == (path, blocks, tickets), (P, B, S, br)
        seen.add(("theta advance", path, tickets))
    assert {k for k in seen if k[0] == "theta"} == {("theta", "lds"), ("theta", "global")}
    assert {k[1:] for k in seen if k[0] == "theta advance"} == {("lds", True), ("lds", False), ("global", True)}
    assert [case[4] for case in THETA_ADVANCE_CASES][:2] == [c["RNG_TICKET_BLOCKS"], c["RNG_TICKET_BLOCKS"] + 1]
    # theta_bwd: both sides of the first prefetch round and of the four rounds; a last chunk with idle wavefronts
    assert {c["bwd_prefetch"], c["bwd_prefetch"] + 1, 63, 64, 65, 1} <= set(THETA_BWD_S)
    assert any(P % c["THETA_BWD_PCHUNK"] for P in THETA_BWD_P) and any(P % c["THETA_BWD_PCHUNK"] == 0 for P in THETA_BWD_P)
    assert any(P > c["THETA_BWD_PCHUNK"] for P in THETA_BWD_P)
    paths = set()
    for B, S, with_ticket, without in IWAE_CASES:
        assert iwae_path(B, S, True) == with_ticket and iwae_path(B, S, False) == without, (B, S)
        paths |= {with_ticket, without}
    assert paths == {"rows", "small", "two_launch"}
    assert iwae_path(*IWAE_PAIR, False) == "two_launch" and max(COMBINE_B) > 16 and all(COMBINE_S_TOTAL % n == 0 for n in COMBINE_RANKS)
    assert {offset_bwd_path(B, S) for B, S, _ in OFFSET_CASES} == {"registers", "loop"}
    for B, S, path in OFFSET_CASES:
        assert offset_bwd_path(B, S) == path, (B, S)
    for B, S, blocks, s_off in COND_CASES:
        assert condition_blocks(B, S) == blocks and 0 < s_off < S and S % B != 0, (B, S)
    assert COND_CASES[-1][2] == c["RNG_TICKET_BLOCKS"] + 1
    assert any(ct[0] * ct[1] > 256 for ct in GATHER_CT) and any(ct[1] == 2 for ct in GATHER_CT)
    sizes = [s for s in ADAM_SIZES if s is not None]
    assert {c["ADAM_CHUNK"] - 1, c["ADAM_CHUNK"], c["ADAM_CHUNK"] + 1, 2 * c["ADAM_CHUNK"] + 1, 1} <= set(sizes)
    assert None in ADAM_SIZES[1:-1]


def test_iwae_mirror_agrees_with_the_library_predicate():
    """vihds_iwae_loss_unit_grad is the one predicate the library exports: the mirror answers as it does on both sides of
    every boundary (host-side arithmetic only: no GPU needed)."""
    from vihds import hip

    L = hip.lib()
    shapes = [(B, S) for B, S, _, _ in IWAE_CASES] + [(64, 1024), (65, 1024), (1, 1025), (0, 5), (5, 0)]
    for B, S in shapes:
        for ticket in (0, 1):
            want = int(B > 0 and S > 0 and iwae_unit_grad(B, S, bool(ticket)))
            assert L.vihds_iwae_loss_unit_grad(B, S, ticket) == want, (B, S, ticket)


# ---- 0b. CPU: the restatements against the oracle and against their float32 runs ---------------------------------------
def test_theta_restatement_equals_the_oracle_on_a_fixture():
    """theta_ref == oracle.sample_clip_theta + chained_log_prob in float64 on dr_constant_icml_tiny_modeuler's q, prior and
    draws: theta, log q, log p and the gradient of a random functional of them in q's means and precisions (constants:
    exactly zero here).  condition_ref == oracle.device_conditioner on its [B,S] tiling."""
    fx = Fixture("dr_constant_icml_tiny_modeuler")
    d = lambda k: fx.t(k, dtype=F64)  # noqa: E731
    kind = torch.tensor(fx.kinds)
    P, B = d("q_mu").shape
    u = d("u")
    S = u.shape[1]
    sigma = 1.0 / d("p_prec").sqrt()
    lo, hi = d("p_mu") - 4.0 * sigma, d("p_mu") + 4.0 * sigma
    ln = kind == LOGNORMAL
    lo, hi = torch.where(ln, lo.exp(), lo), torch.where(ln, hi.exp(), hi)
    assert {LOGNORMAL, CONSTANT} <= set(fx.kinds)
    g = torch.Generator().manual_seed(2)
    w_th, w_q, w_p = (torch.randn(s, generator=g, dtype=F64) for s in ((P, B, S), (B, S), (B, S)))
    qm, qp = d("q_mu").requires_grad_(True), d("q_prec").requires_grad_(True)
    th, lq, lp = theta_ref(kind, qm, qp, None, d("p_mu"), d("p_prec"), lo, hi, u)
    ((w_th * th).sum() + (w_q * lq).sum() + (w_p * lp).sum()).backward()
    qm_o = [d("q_mu")[i][:, None].requires_grad_(True) for i in range(P)]
    qp_o = [d("q_prec")[i][:, None].requires_grad_(True) for i in range(P)]
    pm, pp = [d("p_mu")[i] for i in range(P)], [d("p_prec")[i] for i in range(P)]
    th_o = O.sample_clip_theta(fx.names, fx.kinds, qm_o, qp_o, pm, pp, u)
    vals = list(th_o.values())
    lq_o = O.chained_log_prob(fx.kinds, qm_o, qp_o, vals)
    lp_o = O.chained_log_prob(fx.kinds, pm, pp, vals)
    ((w_th * torch.stack(vals)).sum() + (w_q * lq_o).sum() + (w_p * lp_o).sum()).backward()
    assert rel_err(th, torch.stack(vals), dim=0) < 1e-12
    assert rel_err(lq, lq_o) < 1e-12 and rel_err(lp, lp_o) < 1e-12
    assert rel_err(th.float(), fx.t("theta"), dim=0) < 1e-5  # (and the reference's own recorded theta)
    n_live = 0
    for i in range(P):
        if fx.kinds[i] == CONSTANT:
            assert float(qm.grad[i].abs().max()) == 0.0 and float(qp.grad[i].abs().max()) == 0.0
            continue
        n_live += 1
        assert rel_err(qm.grad[i], qm_o[i].grad[:, 0]) < 1e-10 and rel_err(qp.grad[i], qp_o[i].grad[:, 0]) < 1e-10, i
    assert n_live > 0 and float(qm.grad.abs().max()) > 0
    # the conditioner: one parameter at a time through the oracle's own tiling
    B, S, D = 5, 7, 6
    dev, rel, dflt, z = condition_inputs(B, D, 3)
    got = condition_ref(z, dev, rel, dflt, 2.0, 1.5, B, S)
    for e in range(COND_E):
        want = O.device_conditioner((2.0 + 1.5 * z[e])[None], torch.ones(B, S, dtype=F64), rel[e], dev, bool(dflt[e]))
        assert rel_err(got[e], want) < 1e-13, e


def measure_float32_runs():
    """Largest error of the float32 run of each restatement against its float64 run over this module's own cases, for the
    quantities whose bound is derived from it (module docstring)."""
    worst = dict(row_max=0.0, row_sumexp=0.0, offset_gw=0.0, offset_gb=0.0, cond=0.0)
    shapes = [(B, S) for B, S, _, _ in IWAE_CASES] + [IWAE_PAIR] + [(B, COMBINE_S_TOTAL) for B in COMBINE_B]
    for B, S in shapes:
        for wide in (False, True):
            logp, lp, lq = iwae_inputs(B, S, 7, wide)
            r64, r32 = iwae_ref(logp, lp, lq, S), iwae_ref(logp.float(), lp.float(), lq.float(), S)
            worst["row_max"] = max(worst["row_max"], rel_err(r32["row_max"], r64["row_max"]))
            worst["row_sumexp"] = max(worst["row_sumexp"], each_rel_err(r32["row_sumexp"], r64["row_sumexp"]))
    for B, S, _ in OFFSET_CASES:
        for D, n in OFFSET_DN:
            t = offset_inputs(B, S, D, n, 4)
            _, gw64, gb64 = offset_bwd_ref(t["g_theta"], t["dev"], n, t["src"], t["dst"], 1)
            _, gw32, gb32 = offset_bwd_ref(t["g_theta"].float(), t["dev"].float(), n, t["src"], t["dst"], 1)
            worst["offset_gw"] = max(worst["offset_gw"], rel_err(gw32, gw64, dim=0))
            worst["offset_gb"] = max(worst["offset_gb"], rel_err(gb32, gb64))
    for B, S, _, _ in COND_CASES:
        for D in COND_D:
            dev, rel, dflt, z = condition_inputs(B, D, 3)
            o64 = condition_ref(z, dev, rel, dflt, 2.0, 1.5, B, S)
            o32 = condition_ref(z.float(), dev.float(), rel.float(), dflt, 2.0, 1.5, B, S)
            worst["cond"] = max(worst["cond"], rel_err(o32, o64, dim=0))
    return worst


def each_rel_err(a, b):
    """Largest elementwise relative error (for quantities bounded away from 0, such as a row's sum-exp >= 1)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def test_float32_run_of_the_restatements_stays_inside_a_quarter_of_the_measured_bounds():
    """The bounds without a precedent in the suite are 8 x the float32 restatement's own error (module docstring): the
    re-measured error stays within a quarter of each, and the float32 runs of the restatements with a precedent stay within
    theirs (so every bound measures float32 rounding, not a defect of the restatement)."""
    w = measure_float32_runs()
    print("float32 runs: " + "  ".join("%s %.2e" % kv for kv in sorted(w.items())))
    bounds = dict(row_max=ROW_MAX_TOL, row_sumexp=ROW_SUMEXP_TOL, offset_gw=OFFSET_GW_TOL, offset_gb=OFFSET_GB_TOL, cond=COND_TOL)
    for k, b in bounds.items():
        assert 0.0 < w[k] <= b / 4.0, (k, w[k], b)
    pr = theta_problem(13, 5, 100, 1)
    settle_draws(pr)
    th64, lq64, lp64 = theta_eval(pr)[:3]
    th32, lq32, lp32 = theta_eval(pr, torch.float32)[:3]
    assert rel_err(th32, th64, dim=0) < TOL_THETA and rel_err(lq32, lq64) < TOL and rel_err(lp32, lp64) < TOL
    g = torch.Generator().manual_seed(3)
    ups = [_f32(torch.randn(s, generator=g, dtype=F64)) for s in ((13, 5, 100), (5, 100), (5, 100))]
    g64, g32 = _theta_bwd_reference(pr, *ups), _theta_bwd_reference(pr, *ups, dtype=torch.float32)
    live = pr["kind"] != CONSTANT
    assert rel_err(g32[0][live], g64[0][live], dim=0) < GTOL and rel_err(g32[1][live], g64[1][live], dim=0) < GTOL
    assert float(g64[0][~live].abs().max()) == 0.0 and float(g64[0][live].abs().min()) > 0.0


# ---- GPU plumbing -----------------------------------------------------------------------------------------------------
def _dev(t, dtype=torch.float32):
    return None if t is None else t.detach().to(dtype).to(DEV).contiguous()


def _new_rng(seed):
    from vihds import ops

    return ops.KernelNormal.new_state(seed, DEV)


class ThetaCall:
    """One problem's device buffers and the two theta entry points on them."""

    def __init__(self, pr):
        self.pr = pr
        self.P, self.B, self.S = pr["P"], pr["B"], pr["S"]
        self.d = {k: _dev(pr[k]) for k in ("q_mu", "q_prec", "p_mu", "p_prec", "lo", "hi")}
        self.kind = _dev(pr["kind"], torch.int32)
        self.rows = _dev(pr["q_rows"], torch.int32)

    def opts(self, rng=None, S_total=0, s_off=0, scale=None, job=None):
        from vihds import hip

        o = hip.ThetaOpts()
        o.q_rows, o.q_prec_is_log = hip.ptr(self.rows), int(self.pr["packed"])
        o.rng, o.S_total, o.s_offset = hip.ptr(rng), S_total, s_off
        o.g_theta_scale = hip.ptr(scale)
        if job is not None:
            o.iwae = ctypes.pointer(job)
        return o

    def fwd(self, u=None, rng=None, S=None, S_total=0, s_off=0, logs=True):
        from vihds import hip

        S = self.S if S is None else S
        d = self.d
        u = torch.full((self.B, S, self.P), SENTINEL, device=DEV) if u is None else u
        theta = torch.full((self.P, self.B, S), SENTINEL, device=DEV)
        lq, lp = (torch.full((self.B, S), SENTINEL, device=DEV) for _ in range(2)) if logs else (None, None)
        o = self.opts(rng, S_total, s_off)
        hip.check(hip.lib().vihds_theta_fwd(self.P, self.B, S, hip.ptr(self.kind), hip.ptr(d["q_mu"]), hip.ptr(d["q_prec"]),
                                            hip.ptr(d["p_mu"]), hip.ptr(d["p_prec"]), hip.ptr(d["lo"]), hip.ptr(d["hi"]),
                                            hip.ptr(u), hip.ptr(theta), hip.ptr(lq), hip.ptr(lp), ctypes.byref(o),
                                            hip.current_stream()), "vihds_theta_fwd")
        torch.cuda.synchronize()
        return u, theta, lq, lp

    def bwd(self, g_theta, g_lq, g_lp, scale=None, job=None):
        from vihds import hip

        d = self.d
        u = _dev(self.pr["u"])
        g_mu, g_pr = (torch.full_like(d[k], SENTINEL) for k in ("q_mu", "q_prec"))
        o = self.opts(scale=scale, job=job)
        hip.check(hip.lib().vihds_theta_bwd(self.P, self.B, self.S, hip.ptr(self.kind), hip.ptr(d["q_mu"]), hip.ptr(d["q_prec"]),
                                            hip.ptr(d["p_mu"]), hip.ptr(d["p_prec"]), hip.ptr(d["lo"]), hip.ptr(d["hi"]),
                                            hip.ptr(u), hip.ptr(g_theta), hip.ptr(g_lq), hip.ptr(g_lp), hip.ptr(g_mu),
                                            hip.ptr(g_pr), ctypes.byref(o), hip.current_stream()), "vihds_theta_bwd")
        torch.cuda.synchronize()
        return g_mu.cpu(), g_pr.cpu()


def _check_theta_values(label, pr, u, theta, lq, lp):
    """theta / log q / log p of a forward launch against theta_ref at the draws the launch used."""
    th64, lq64, lp64 = theta_eval(pr, u=u.cpu().double())[:3]
    errs = dict(theta=rel_err(theta, th64, dim=0))
    cst = pr["kind"] == CONSTANT
    if bool(cst.any()):  # constants: 0 * u + value, exactly
        assert torch.equal(theta.cpu()[cst], th64[cst].float()), label
    if lq is not None:
        errs.update(log_q=rel_err(lq, lq64), log_p=rel_err(lp, lp64))
    return errs


# ---- 1. vihds_theta_fwd ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P,B,S,path,what", THETA_FWD_CASES, ids=["P%dxB%dxS%d-%s" % c[:4] for c in THETA_FWD_CASES])
def test_theta_fwd_both_kernels_against_float64(P, B, S, path, what):
    """theta, log q and log p with given draws (identity rows; permuted q_rows + log-precisions; log_q / log_p NULL), and
    with the in-kernel generator: the written draws against philox_ref, theta / log q / log p at those draws, and a call on
    samples S.. of 2S per row against that slice of the unsharded call."""
    assert theta_fwd_path(P, B, S)["path"] == path
    worst = dict(theta=0.0, log_q=0.0, log_p=0.0, u=0.0)
    for packed in (False, True):
        pr = theta_problem(P, B, S, 11 + packed, packed)
        call = ThetaCall(pr)
        u_in = _dev(pr["u"])
        u, theta, lq, lp = call.fwd(u=u_in)
        assert torch.equal(u, _dev(pr["u"]))  # (an input: left alone)
        for k, e in _check_theta_values((what, packed), pr, u, theta, lq, lp).items():
            worst[k] = max(worst[k], e)
        frac = clipped_fractions(pr)
        if frac is not None and frac[2] >= 400:
            assert 0.1 <= frac[0] <= 0.3 and 0.1 <= frac[1] <= 0.3, frac
        if not packed:  # log_q / log_p NULL: theta alone, the same bits
            _, theta2, _, _ = call.fwd(u=u_in, logs=False)
            assert torch.equal(theta2, theta)
        # the in-kernel generator
        seed = 0x1234567890ABCDEF + P
        state = _new_rng(seed)
        u_k, th_k, lq_k, lp_k = call.fwd(rng=state, S_total=S, s_off=0)
        want = torch.tensor(expected_kernel_normals(B, S, P, seed, 0))
        worst["u"] = max(worst["u"], float((u_k.cpu() - want).abs().max()))
        assert state.cpu().tolist()[2:] == [1, 0]
        for k, e in _check_theta_values((what, packed, "rng"), pr, u_k, th_k, lq_k, lp_k).items():
            worst[k] = max(worst[k], e)
        # S sharded: samples S..2S-1 of a 2S-sample row are that slice of the same global draw
        full = _new_rng(seed)
        u_f, th_f, lq_f, lp_f = call.fwd(rng=full, S=2 * S, S_total=2 * S, s_off=0)
        part = _new_rng(seed)
        u_p, th_p, lq_p, lp_p = call.fwd(rng=part, S=S, S_total=2 * S, s_off=S)
        assert torch.equal(u_p, u_f[:, S:]), (what, packed)
        want2 = torch.tensor(expected_kernel_normals(B, 2 * S, P, seed, 0))
        worst["u"] = max(worst["u"], float((u_f.cpu() - want2).abs().max()))
        if theta_fwd_path(P, B, 2 * S)["path"] == path:  # the same kernel: the same bits
            assert torch.equal(th_p, th_f[:, :, S:]) and torch.equal(lq_p, lq_f[:, S:]) and torch.equal(lp_p, lp_f[:, S:])
        else:
            assert rel_err(th_p, th_f[:, :, S:], dim=0) < TOL_THETA and rel_err(lq_p, lq_f[:, S:]) < TOL
    print("theta_fwd P%d B%d S%d %-6s %-45s theta %.1e (tol %.0e)  log_q %.1e  log_p %.1e (tol %.0e)  u %.1e (tol %.0e)"
          % (P, B, S, path, what, worst["theta"], TOL_THETA, worst["log_q"], worst["log_p"], TOL, worst["u"], TOL_U))
    assert worst["theta"] < TOL_THETA and worst["log_q"] < TOL and worst["log_p"] < TOL and worst["u"] < TOL_U, worst


@gpu
@pytest.mark.parametrize("P,B,S,path,blocks,tickets", THETA_ADVANCE_CASES,
                         ids=["%s-%dblocks" % (c[3], c[4]) for c in THETA_ADVANCE_CASES])
def test_theta_fwd_generator_advance_on_both_paths(P, B, S, path, blocks, tickets):
    """Two launches in a row on one generator state: the state words are [1, 0] and [2, 0], with block tickets (<= 256
    blocks, and the fallback kernel) and with the separate one-thread launch (257 blocks); the draws are those of steps 0
    and 1."""
    br = theta_fwd_path(P, B, S)
    assert (br["path"], br["blocks"], br["tickets"]) == (path, blocks, tickets)
    pr = theta_problem(P, B, S, 21)
    call = ThetaCall(pr)
    seed = 0x0FEDCBA987654321
    state = _new_rng(seed)
    worst = dict(theta=0.0, log_q=0.0, log_p=0.0, u=0.0)
    for step in (0, 1):
        u, theta, lq, lp = call.fwd(rng=state, S_total=S, s_off=0)
        assert state.cpu().tolist()[2:] == [step + 1, 0], (path, blocks, step)
        want = torch.tensor(expected_kernel_normals(B, S, P, seed, step))
        worst["u"] = max(worst["u"], float((u.cpu() - want).abs().max()))
        for k, e in _check_theta_values((path, blocks), pr, u, theta, lq, lp).items():
            worst[k] = max(worst[k], e)
    print("theta_fwd advance %-6s %3d blocks: theta %.1e (tol %.0e)  log_q %.1e  log_p %.1e (tol %.0e)  u %.1e (tol %.0e)"
          % (path, blocks, worst["theta"], TOL_THETA, worst["log_q"], worst["log_p"], TOL, worst["u"], TOL_U))
    assert worst["theta"] < TOL_THETA and worst["log_q"] < TOL and worst["log_p"] < TOL and worst["u"] < TOL_U, worst


# ---- 2. vihds_theta_bwd ------------------------------------------------------------------------------------------------
def _theta_bwd_reference(pr, g_theta, g_lq, g_lp, scale=None, dtype=F64):
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    th, lq, lp, _, q_mu, q_prec = theta_eval(pr, dtype, grad=True)
    loss = th.sum() * 0.0
    if g_theta is not None:
        loss = loss + (c(g_theta) * (c(scale) if scale is not None else 1.0) * th).sum()
    if g_lq is not None:
        loss = loss + (c(g_lq) * lq).sum()
    if g_lp is not None:
        loss = loss + (c(g_lp) * lp).sum()
    loss.backward()
    return q_mu.grad, q_prec.grad, lq.detach(), lp.detach()


def _theta_job_reference(pr, g_theta, has_lp, has_lq, log_w, n_iwae, dtype=F64):
    """Gradients of the in-launch IWAE loss in the q tables, taken at the given log-weights (module docstring)."""
    th, lq, lp, _, q_mu, q_prec = theta_eval(pr, dtype, grad=True)
    dlw = (g_theta.to(dtype) * th).sum(0) + (lp if has_lp else 0.0) - (lq if has_lq else 0.0)
    lw = log_w.to(dtype) + (dlw - dlw.detach())
    (-(torch.logsumexp(lw, 1) - math.log(n_iwae)).mean()).backward()
    return q_mu.grad, q_prec.grad


def _compare_q_grads(label, pr, got, ref64):
    """Referenced rows against the float64 gradient: per parameter, the largest error relative to the row's float64 maximum
    (rel_err's per-row norm); a row whose float64 gradient is exactly 0 -- a constant, or at S = 1 a clipped sample without
    an upstream log q gradient -- must come back exactly 0.  Every other row of the tables: untouched."""
    P = pr["P"]
    rows = torch.arange(P).repeat(2) if pr["q_rows"] is None else pr["q_rows"]
    worst = 0.0
    for g, r64, rws in ((got[0], ref64[0], rows[:P]), (got[1], ref64[1], rows[P:])):
        other = torch.ones(g.shape[0], dtype=torch.bool)
        other[rws] = False
        assert bool((g[other] == SENTINEL).all()), label
        for p in range(P):
            scale = float(r64[rws[p]].abs().max())
            assert scale == 0.0 or int(pr["kind"][p]) != CONSTANT, (label, p)
            if scale == 0.0:
                assert float(g[rws[p]].abs().max()) == 0.0, (label, p)
            else:
                worst = max(worst, float((g[rws[p]].double() - r64[rws[p]]).abs().max()) / scale)
    return worst


@gpu
@pytest.mark.parametrize("S", THETA_BWD_S)
def test_theta_bwd_against_autograd_of_the_float64_restatement(S):
    """vihds_theta_bwd on its own for B in {1, 5} x P in {1, 4, 5, 9} at one S: random upstream gradients (each NULL once),
    g_theta_scale, permuted q_rows with the log-precision adjoint, and the in-launch IWAE job (loss, log_w, lse, ticket, a
    bit-identical replay; log_p / log_q NULL in the job once) against autograd of theta_ref.  Draws whose float64 sample
    lies within 1e-4 relative of a clip bound are resampled first; nothing is excluded."""
    from vihds import hip

    worst = dict(plain=0.0, null=0.0, scale=0.0, rows=0.0, iwae=0.0, log_w=0.0, lse=0.0, loss=0.0)
    n_clipped = n_total = n_resampled = 0
    k = 0
    for B in THETA_BWD_B:
        for P in THETA_BWD_P:
            k += 1
            label = "P%d B%d S%d" % (P, B, S)
            g = torch.Generator().manual_seed(100 * S + 10 * B + P)
            randn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=F64))  # noqa: E731
            for packed in (False, True):
                pr = theta_problem(P, B, S, 31 + k + 50 * packed, packed)
                n_resampled += settle_draws(pr)
                assert not bool(near_a_bound(pr).any()), label
                xr = theta_eval(pr)[3]
                live = pr["kind"] != CONSTANT
                out = (xr < pr["lo"][:, None, None]) | (xr > pr["hi"][:, None, None])
                n_clipped += int(out[live].sum())
                n_total += int(out[live].numel())
                call = ThetaCall(pr)
                g_th, g_lq, g_lp, scale = randn(P, B, S), randn(B, S), randn(B, S), randn(B, S)

                def check(key, tag, got, *ups):
                    r64 = _theta_bwd_reference(pr, *ups)
                    worst[key] = max(worst[key], _compare_q_grads(label + tag, pr, got, r64))
                    return r64

                if packed:
                    check("rows", " rows", call.bwd(_dev(g_th), _dev(g_lq), _dev(g_lp)), g_th, g_lq, g_lp)
                    continue
                ref = check("plain", "", call.bwd(_dev(g_th), _dev(g_lq), _dev(g_lp)), g_th, g_lq, g_lp)
                ups = [g_th, g_lq, g_lp]
                ups[k % 3] = None  # each upstream gradient NULL in turn
                check("null", " null", call.bwd(*[_dev(t) for t in ups]), *ups)
                check("scale", " scale", call.bwd(_dev(g_th), _dev(g_lq), _dev(g_lp), scale=_dev(scale)), g_th, g_lq, g_lp, scale)
                # the IWAE job: log q / log p as the forward would hand them over (float32 of the restatement's)
                logp, _, _ = iwae_inputs(B, S, 300 + k)
                lq32, lp32 = _f32(ref[2]), _f32(ref[3])
                has_lp, has_lq = k % 4 != 1, k % 4 != 3
                n_iwae = S if k % 2 else 2 * S
                bufs = dict(logp=_dev(logp), log_p=_dev(lp32) if has_lp else None, log_q=_dev(lq32) if has_lq else None,
                            log_w=torch.full((B, S), SENTINEL, device=DEV), lse=torch.full((B,), SENTINEL, device=DEV),
                            loss=torch.full((1,), SENTINEL, device=DEV), ticket=torch.zeros(1, dtype=torch.int32, device=DEV))
                job = hip.IwaeJob()
                for name, t in bufs.items():
                    setattr(job, name, hip.ptr(t))
                job.n_iwae_total = n_iwae
                # (g_log_q / g_log_p / g_theta_scale are ignored with a job: hand in garbage)
                got = call.bwd(_dev(g_th), _dev(g_lq), _dev(g_lp), scale=_dev(scale), job=job)
                first = {n: bufs[n].clone() for n in ("log_w", "lse", "loss")}
                assert int(bufs["ticket"].item()) == 0, label
                again = call.bwd(_dev(g_th), None, None, job=job)
                assert int(bufs["ticket"].item()) == 0, label
                assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), label
                assert all(torch.equal(first[n], bufs[n]) for n in first), label
                r64 = iwae_ref(logp, lp32 if has_lp else None, lq32 if has_lq else None, n_iwae)
                worst["log_w"] = max(worst["log_w"], rel_err(bufs["log_w"], r64["log_w"], dim=0))
                worst["lse"] = max(worst["lse"], rel_err(bufs["lse"], r64["lse"]))
                worst["loss"] = max(worst["loss"], rel_err(bufs["loss"][0], r64["loss"]))
                lw_gpu = bufs["log_w"].cpu()  # gradients at the launch's own float32 log-weights (module docstring)
                j64 = _theta_job_reference(pr, g_th, has_lp, has_lq, lw_gpu, n_iwae)
                worst["iwae"] = max(worst["iwae"], _compare_q_grads(label + " iwae", pr, got, j64))
    keys = ("plain", "null", "scale", "rows", "iwae")
    print("theta_bwd S %3d: grads " % S + "  ".join("%s %.1e" % (kk, worst[kk]) for kk in keys)
          + " (tol %.0e)  job log_w %.1e  lse %.1e  loss %.1e (tol %.0e)  clipped %d of %d samples, %d resampled"
          % (GTOL, worst["log_w"], worst["lse"], worst["loss"], TOL_LOSS, n_clipped, n_total, n_resampled))
    assert n_clipped > 0.05 * n_total  # (pass = 0 is exercised)
    for key in keys:
        assert worst[key] < GTOL, (key, worst)
    for key in ("log_w", "lse", "loss"):
        assert worst[key] < TOL_LOSS, (key, worst)


# ---- 3. IWAE -----------------------------------------------------------------------------------------------------------
def _iwae_buffers(B, S, unit):
    b = dict(log_w=torch.full((B, S), SENTINEL, device=DEV), row_max=torch.full((B,), SENTINEL, device=DEV),
             row_sumexp=torch.full((B,), SENTINEL, device=DEV), lse=torch.full((B,), SENTINEL, device=DEV),
             loss=torch.full((1,), SENTINEL, device=DEV))
    b["unit"] = torch.full((B, S), SENTINEL, device=DEV) if unit else None
    b["unit_neg"] = torch.full((B, S), SENTINEL, device=DEV) if unit else None
    return b


def _iwae_loss_fwd(B, S, n_total, d, b, ticket):
    from vihds import hip

    rc = hip.lib().vihds_iwae_loss_fwd(B, S, n_total, hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), hip.ptr(b["log_w"]),
                                       hip.ptr(b["row_max"]), hip.ptr(b["row_sumexp"]), hip.ptr(b["lse"]), hip.ptr(b["loss"]),
                                       hip.ptr(b["unit"]), hip.ptr(b["unit_neg"]), hip.ptr(ticket), hip.current_stream())
    torch.cuda.synchronize()
    return rc


def _iwae_errors(b, r64):
    return dict(log_w=rel_err(b["log_w"], r64["log_w"], dim=0), row_max=rel_err(b["row_max"], r64["row_max"]),
                row_sumexp=each_rel_err(b["row_sumexp"], r64["row_sumexp"]), lse=rel_err(b["lse"], r64["lse"]),
                loss=rel_err(b["loss"][0], r64["loss"]))


IWAE_BOUNDS = dict(log_w=TOL_LOSS, row_max=ROW_MAX_TOL, row_sumexp=ROW_SUMEXP_TOL, lse=TOL_LOSS, loss=TOL_LOSS, unit=GTOL)


@gpu
@pytest.mark.parametrize("with_ticket", [True, False], ids=["ticket", "no-ticket"])
@pytest.mark.parametrize("B,S,p_ticket,p_none", IWAE_CASES, ids=["B%dxS%d" % c[:2] for c in IWAE_CASES])
def test_iwae_loss_fwd_on_every_path_against_float64(B, S, p_ticket, p_none, with_ticket):
    """vihds_iwae_loss_fwd with and without a ticket: log_w, row max, row sum-exp, lse and loss against iwae_ref on both
    input sets; the unit-gradient outputs equal vihds_iwae_loss_bwd at g_loss = 1 bit for bit and the float64 softmax where
    vihds_iwae_loss_unit_grad says 1, and asking for them elsewhere is VIHDS_E_UNSUPPORTED; the ticket is back at 0 and a
    second launch gives the same bits."""
    from vihds import hip

    L = hip.lib()
    path = iwae_path(B, S, with_ticket)
    assert path == (p_ticket if with_ticket else p_none)
    unit = bool(L.vihds_iwae_loss_unit_grad(B, S, int(with_ticket)))
    assert unit == iwae_unit_grad(B, S, with_ticket)
    n_total = IWAE_N_TOTAL.get((B, S), S)
    worst = {k: 0.0 for k in IWAE_BOUNDS}
    for wide in (False, True):
        logp, lp, lq = iwae_inputs(B, S, 7, wide)
        d = [_dev(t) for t in (logp, lp, lq)]
        r64 = iwae_ref(logp, lp, lq, n_total)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV) if with_ticket else None
        if not unit:  # declined before anything is queued: outputs untouched
            b = _iwae_buffers(B, S, True)
            assert _iwae_loss_fwd(B, S, n_total, d, b, ticket) == hip.E_UNSUPPORTED
            assert all(bool((t == SENTINEL).all()) for t in b.values())
        b = _iwae_buffers(B, S, unit)
        assert _iwae_loss_fwd(B, S, n_total, d, b, ticket) == 0, L.vihds_last_error()
        for k, e in _iwae_errors(b, r64).items():
            worst[k] = max(worst[k], e)
        if with_ticket:
            assert int(ticket.item()) == 0
        first = {k: (None if t is None else t.clone()) for k, t in b.items()}
        assert _iwae_loss_fwd(B, S, n_total, d, b, ticket) == 0
        assert all(t is None or torch.equal(t, b[k]) for k, t in first.items())
        if with_ticket:
            assert int(ticket.item()) == 0
        if unit:
            g_logw, g_neg = torch.full((B, S), SENTINEL, device=DEV), torch.full((B, S), SENTINEL, device=DEV)
            one = torch.ones(1, device=DEV)
            hip.check(L.vihds_iwae_loss_bwd(B, S, hip.ptr(b["log_w"]), hip.ptr(b["lse"]), hip.ptr(one), hip.ptr(g_logw),
                                            hip.ptr(g_neg), hip.current_stream()), "vihds_iwae_loss_bwd")
            torch.cuda.synchronize()
            assert torch.equal(b["unit"], g_logw) and torch.equal(b["unit_neg"], g_neg) and torch.equal(g_neg, -g_logw)
            lw = b["log_w"].cpu().double()  # (the softmax at the launch's own log-weights: module docstring)
            worst["unit"] = max(worst["unit"], rel_err(b["unit"], softmax_grad(lw, torch.logsumexp(lw, 1)), dim=0))
    print("iwae_loss_fwd B%d S%d %-10s " % (B, S, path)
          + "  ".join("%s %.1e (%.1e)" % (k, worst[k], IWAE_BOUNDS[k]) for k in IWAE_BOUNDS))
    for k, bound in IWAE_BOUNDS.items():
        assert worst[k] < bound, (k, worst)


@gpu
def test_iwae_fwd_and_bwd_pair_against_float64():
    """vihds_iwae_fwd + vihds_iwae_bwd at (5, 300) with a random g_lse."""
    from vihds import hip

    L = hip.lib()
    B, S = IWAE_PAIR
    logp, lp, lq = iwae_inputs(B, S, 9)
    d = [_dev(t) for t in (logp, lp, lq)]
    r64 = iwae_ref(logp, lp, lq, S)
    b = _iwae_buffers(B, S, False)
    hip.check(L.vihds_iwae_fwd(B, S, hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), hip.ptr(b["log_w"]), hip.ptr(b["row_max"]),
                               hip.ptr(b["row_sumexp"]), hip.current_stream()), "vihds_iwae_fwd")
    torch.cuda.synchronize()
    errs = dict(log_w=rel_err(b["log_w"], r64["log_w"], dim=0), row_max=rel_err(b["row_max"], r64["row_max"]),
                row_sumexp=each_rel_err(b["row_sumexp"], r64["row_sumexp"]))
    lse = (b["row_max"].cpu().double() + b["row_sumexp"].cpu().double().log()).float()  # (the host's finish)
    g_lse = _f32(torch.randn(B, generator=torch.Generator().manual_seed(1), dtype=F64))
    g_logw = torch.full((B, S), SENTINEL, device=DEV)
    d_lse, d_g = _dev(lse), _dev(g_lse)
    hip.check(L.vihds_iwae_bwd(B, S, hip.ptr(b["log_w"]), hip.ptr(d_lse), hip.ptr(d_g), hip.ptr(g_logw),
                               hip.current_stream()), "vihds_iwae_bwd")
    torch.cuda.synchronize()
    lw = b["log_w"].cpu().double()
    want = g_lse[:, None] * (lw - torch.logsumexp(lw, 1)[:, None]).exp()
    errs["g_logw"] = rel_err(g_logw, want, dim=0)
    print("iwae_fwd + iwae_bwd B%d S%d: log_w %.1e (%.0e)  row_max %.1e (%.1e)  row_sumexp %.1e (%.1e)  g_logw %.1e (%.0e)"
          % (B, S, errs["log_w"], TOL_LOSS, errs["row_max"], ROW_MAX_TOL, errs["row_sumexp"], ROW_SUMEXP_TOL, errs["g_logw"], GTOL))
    assert errs["log_w"] < TOL_LOSS and errs["row_max"] < ROW_MAX_TOL and errs["row_sumexp"] < ROW_SUMEXP_TOL
    assert errs["g_logw"] < GTOL


@gpu
@pytest.mark.parametrize("B", COMBINE_B)
@pytest.mark.parametrize("n_ranks", COMBINE_RANKS)
def test_iwae_combine_over_ranks_against_the_unsharded_float64_result(n_ranks, B):
    """vihds_iwae_combine fed by vihds_iwae_fwd on the S-slices of one problem: lse, loss and every rank's unit gradient
    equal the unsharded float64 result; unit_g_logw without log_w is rejected."""
    from vihds import hip

    L = hip.lib()
    S_total = COMBINE_S_TOTAL
    S = S_total // n_ranks
    worst = dict(lse=0.0, loss=0.0, unit=0.0)
    for wide in (False, True):
        logp, lp, lq = iwae_inputs(B, S_total, 13, wide)
        r64 = iwae_ref(logp, lp, lq, S_total)
        gathered = torch.full((n_ranks, 2, B), SENTINEL, device=DEV)
        log_ws = []
        for r in range(n_ranks):
            sl = slice(r * S, (r + 1) * S)
            d = [_dev(logp[:, :, sl]), _dev(lp[:, sl]), _dev(lq[:, sl])]
            log_w = torch.full((B, S), SENTINEL, device=DEV)
            hip.check(L.vihds_iwae_fwd(B, S, hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), hip.ptr(log_w),
                                       gathered[r, 0].data_ptr(), gathered[r, 1].data_ptr(), hip.current_stream()), "vihds_iwae_fwd")
            torch.cuda.synchronize()
            log_ws.append(log_w)
        lw_all = torch.cat(log_ws, 1).cpu().double()
        assert rel_err(lw_all, r64["log_w"], dim=0) < TOL_LOSS
        want_unit = softmax_grad(lw_all, torch.logsumexp(lw_all, 1))
        for r in range(n_ranks):
            lse, loss = torch.full((B,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
            unit, neg = torch.full((B, S), SENTINEL, device=DEV), torch.full((B, S), SENTINEL, device=DEV)
            hip.check(L.vihds_iwae_combine(n_ranks, B, S, S_total, hip.ptr(gathered), hip.ptr(log_ws[r]), hip.ptr(lse),
                                           hip.ptr(loss), hip.ptr(unit), hip.ptr(neg), hip.current_stream()), "vihds_iwae_combine")
            torch.cuda.synchronize()
            worst["lse"] = max(worst["lse"], rel_err(lse, r64["lse"]))
            worst["loss"] = max(worst["loss"], rel_err(loss[0], r64["loss"]))
            worst["unit"] = max(worst["unit"], rel_err(unit, want_unit[:, r * S:(r + 1) * S], dim=0))
            assert torch.equal(neg, -unit)
        assert L.vihds_iwae_combine(n_ranks, B, S, S_total, hip.ptr(gathered), None, hip.ptr(lse), hip.ptr(loss),
                                    hip.ptr(unit), None, hip.current_stream()) < 0
        # without the unit outputs log_w is not needed
        hip.check(L.vihds_iwae_combine(n_ranks, B, S, S_total, hip.ptr(gathered), None, hip.ptr(lse), hip.ptr(loss), None, None,
                                       hip.current_stream()), "vihds_iwae_combine")
        torch.cuda.synchronize()
        worst["lse"] = max(worst["lse"], rel_err(lse, r64["lse"]))
    print("iwae_combine ranks %d B %2d: lse %.1e  loss %.1e (tol %.0e)  unit gradient %.1e (tol %.0e)"
          % (n_ranks, B, worst["lse"], worst["loss"], TOL_LOSS, worst["unit"], GTOL))
    assert worst["lse"] < TOL_LOSS and worst["loss"] < TOL_LOSS and worst["unit"] < GTOL, worst


# ---- 4. the offset layer -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,S,path", OFFSET_CASES, ids=["B%dxS%d-%s" % c for c in OFFSET_CASES])
def test_offset_rows_both_backward_paths_against_float64(B, S, path):
    """vihds_offset_rows_fwd and _bwd for D in {1, 12} x n in {1, 3}: accumulate 0 (source rows pre-filled with NaN) and 1,
    with and without g_wb; the routed gradient, g_W and g_bias against float64, every other row untouched."""
    from vihds import hip

    L = hip.lib()
    assert offset_bwd_path(B, S) == path
    worst = dict(fwd=0.0, routed=0.0, g_w=0.0, g_b=0.0)
    for D, n in OFFSET_DN:
        t = offset_inputs(B, S, D, n, 4)
        R, src, dst = t["R"], t["src"], t["dst"]
        dev, W, bias = _dev(t["dev"]), _dev(t["W"]), _dev(t["bias"])
        theta = _dev(t["theta"])
        hip.check(L.vihds_offset_rows_fwd(B, S, D, n, R, src, dst, hip.ptr(W), hip.ptr(bias), hip.ptr(dev), hip.ptr(theta),
                                          hip.current_stream()), "vihds_offset_rows_fwd")
        torch.cuda.synchronize()
        want = offset_fwd_ref(t["theta"], t["W"], t["bias"], t["dev"], src, dst)
        assert torch.allclose(theta.cpu().double(), want, rtol=1e-6, atol=1e-6), (D, n)
        keep = torch.ones(R, dtype=torch.bool)
        keep[dst:dst + n] = False
        assert torch.equal(theta.cpu()[keep], t["theta"].float()[keep])
        worst["fwd"] = max(worst["fwd"], float((theta.cpu().double() - want).abs().max()))
        for accumulate in (0, 1):
            for with_wb in (True, False):
                g_in = t["g_theta"].clone()
                if not accumulate:
                    g_in[src:src + n] = float("nan")
                g_theta = _dev(g_in)
                g_wb = torch.full((n * D + n + 8,), SENTINEL, device=DEV) if with_wb else None
                hip.check(L.vihds_offset_rows_bwd(B, S, D, n, R, src, dst, accumulate, hip.ptr(dev), hip.ptr(g_theta),
                                                  hip.ptr(g_wb), hip.current_stream()), "vihds_offset_rows_bwd")
                torch.cuda.synchronize()
                routed, gw, gb = offset_bwd_ref(t["g_theta"], t["dev"], n, src, dst, accumulate)
                got = g_theta.cpu()
                label = (D, n, accumulate, with_wb)
                assert bool(torch.isfinite(got).all()), label
                assert torch.allclose(got.double(), routed, rtol=1e-6, atol=1e-6), label
                if not accumulate:  # an assignment: the same bits
                    assert torch.equal(got[src:src + n], got[dst:dst + n]), label
                keep = torch.ones(R, dtype=torch.bool)
                keep[src:src + n] = False
                assert torch.equal(got[keep], t["g_theta"].float()[keep]), label
                worst["routed"] = max(worst["routed"], float((got.double() - routed).abs().max()))
                if with_wb:
                    out = g_wb.cpu()
                    assert bool((out[n * D + n:] == SENTINEL).all()), label
                    worst["g_w"] = max(worst["g_w"], rel_err(out[: n * D].reshape(n, D), gw, dim=0))
                    worst["g_b"] = max(worst["g_b"], rel_err(out[n * D: n * D + n], gb))
    print("offset_rows B%d S%d %-9s fwd max|d| %.1e  routed max|d| %.1e (allclose 1e-6)  g_W %.1e (tol %.1e)  g_bias %.1e (tol %.1e)"
          % (B, S, path, worst["fwd"], worst["routed"], worst["g_w"], OFFSET_GW_TOL, worst["g_b"], OFFSET_GB_TOL))
    assert worst["g_w"] < OFFSET_GW_TOL and worst["g_b"] < OFFSET_GB_TOL, worst


# ---- 5. the device conditioner -----------------------------------------------------------------------------------------
def _device_condition(B, S, S_total, s_off, D, z, rng, dev, rel, dflt):
    from vihds import hip

    out = torch.full((COND_E, B, S), SENTINEL, device=DEV)
    hip.check(hip.lib().vihds_device_condition(COND_E, B, S, S_total, s_off, D, 2.0, 1.5, hip.ptr(z), hip.ptr(rng), hip.ptr(dev),
                                               hip.ptr(rel), hip.ptr(dflt), hip.ptr(out), hip.current_stream()),
              "vihds_device_condition")
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("D", COND_D)
@pytest.mark.parametrize("B,S,blocks,s_off", COND_CASES, ids=["B%dxS%d" % c[:2] for c in COND_CASES])
def test_device_condition_shapes_shards_and_generator(B, S, blocks, s_off, D):
    """vihds_device_condition with given z against condition_ref; a call on samples s_off.. of S per row equals that slice
    of the unsharded output (B does not divide S, so the tiling index matters); with the generator, the outputs at the
    philox_ref draws of steps 0 and 1 and the state words [step + 1, 0] (tickets up to 256 blocks, the one-thread launch
    at 257)."""
    assert condition_blocks(B, S) == blocks
    dev, rel, dflt, z = condition_inputs(B, D, 3)
    d_dev, d_rel, d_dflt, d_z = _dev(dev), _dev(rel), _dev(dflt, torch.int32), _dev(z)
    out = _device_condition(B, S, S, 0, D, d_z, None, d_dev, d_rel, d_dflt)
    e_z = rel_err(out, condition_ref(z, dev, rel, dflt, 2.0, 1.5, B, S), dim=0)
    part = _device_condition(B, S - s_off, S, s_off, D, d_z, None, d_dev, d_rel, d_dflt)
    assert torch.equal(part, out[:, :, s_off:])
    assert torch.equal(_device_condition(B, S, 0, 0, D, d_z, None, d_dev, d_rel, d_dflt), out)  # S_total <= 0: S_total = S
    seed = 0x3EDCBA9876543210
    state = _new_rng(seed)
    e_rng, outs = 0.0, []
    for step in (0, 1):
        o = _device_condition(B, S, S, 0, D, None, state, d_dev, d_rel, d_dflt)
        assert state.cpu().tolist()[2:] == [step + 1, 0], (blocks, step)
        e_rng = max(e_rng, rel_err(o, condition_ref(conditioner_normals(COND_E, D, seed, step), dev, rel, dflt, 2.0, 1.5, B, S), dim=0))
        outs.append(o)
    assert not torch.equal(outs[0], outs[1])
    shard_state = _new_rng(seed)
    part = _device_condition(B, S - s_off, S, s_off, D, None, shard_state, d_dev, d_rel, d_dflt)
    assert torch.equal(part, outs[0][:, :, s_off:]) and shard_state.cpu().tolist()[2:] == [1, 0]
    print("device_condition B%d S%d D%d (%d blocks): given z %.1e (tol %.1e)  generator %.1e (tol %.0e)"
          % (B, S, D, blocks, e_z, COND_TOL, e_rng, TOL_U))
    assert e_z < COND_TOL and e_rng < TOL_U


# ---- 6. the batch gather -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C4,T", GATHER_CT, ids=["C%dxT%d" % c for c in GATHER_CT])
def test_gather_batch_bit_for_bit(C4, T):
    """vihds_gather_batch from 11 source rows for B in {1, 7} (repeats, indices below 0 and past the set clamped to the
    ends), n_tr in {0, 2}, D in {0, 7}, with and without delta_obs: every output bit for bit, nothing written past it."""
    from vihds import hip

    L = hip.lib()
    n_src, pad = 11, 64
    g = torch.Generator().manual_seed(6)
    obs_src = torch.randn(n_src, C4, T, generator=g)
    n_checked = 0
    for B, idx in ((1, [-3]), (1, [4]), (7, [10, 3, 3, -1, 11, 0, 1 << 40])):
        for n_tr in (0, 2):
            for D in (0, 7):
                for with_delta in (True, False):
                    inputs_src, dev_src = torch.randn(n_src, n_tr, generator=g), torch.randn(n_src, D, generator=g)
                    idx_t = torch.tensor(idx, dtype=torch.int64)
                    want = gather_ref(idx_t, obs_src, inputs_src, dev_src)
                    sizes = [B * C4 * T, B * n_tr, B * D, B * C4 * (T - 1)]
                    outs = [torch.full((sz + pad,), SENTINEL, device=DEV) for sz in sizes]
                    d_src = [_dev(obs_src), _dev(inputs_src) if n_tr else None, _dev(dev_src) if D else None]
                    d_idx = idx_t.to(DEV)
                    hip.check(L.vihds_gather_batch(B, n_src, C4, T, n_tr, D, hip.ptr(d_idx), *[hip.ptr(t) for t in d_src],
                                                   hip.ptr(outs[0]), hip.ptr(outs[1]) if n_tr else None,
                                                   hip.ptr(outs[2]) if D else None, hip.ptr(outs[3]) if with_delta else None,
                                                   hip.current_stream()), "vihds_gather_batch")
                    torch.cuda.synchronize()
                    for k, (o, w, sz) in enumerate(zip(outs, want, sizes)):
                        o = o.cpu()
                        assert bool((o[sz:] == SENTINEL).all()), (B, n_tr, D, with_delta, k)
                        if k == 3 and not with_delta:
                            assert bool((o == SENTINEL).all())
                        else:
                            assert torch.equal(o[:sz], w.reshape(-1)), (B, n_tr, D, with_delta, k)
                        n_checked += 1
    print("gather_batch C4 %d T %d: %d outputs bit for bit" % (C4, T, n_checked))


# ---- 7. Adam -----------------------------------------------------------------------------------------------------------
@gpu
def test_adam_step_around_the_chunk_size_against_float64():
    """vihds_adam_step over 3 steps on tensors of 1, 1023, 1024, 1025 and 2049 elements with a gradient-less tensor between
    them (its parameter and moments stay bit for bit; the moments of the tensors behind it sit past its slot), grad_scale
    0.125, a device learning rate changed between steps, the step count and ticket words after each launch, a gated step,
    and the table limit (32 tensors accepted, 33 rejected)."""
    from vihds import hip

    L = hip.lib()
    f32c = lambda x: float(np.float32(x))  # noqa: E731  (the hyper-parameters as the float arguments carry them)
    lr0, lr1, b1, b2, eps, gs = f32c(0.01), f32c(0.002), f32c(0.9), f32c(0.999), f32c(1e-8), 0.125
    g = torch.Generator().manual_seed(8)
    sizes = [7 if s is None else s for s in ADAM_SIZES]
    no_grad = ADAM_SIZES.index(None)
    p64 = [_f32(torch.randn(s, generator=g, dtype=F64)) for s in sizes]
    m64, v64 = [torch.zeros(s, dtype=F64) for s in sizes], [torch.zeros(s, dtype=F64) for s in sizes]
    p_dev = [_dev(p) for p in p64]
    total = sum(sizes)
    m_dev, v_dev = torch.zeros(total + 16, device=DEV), torch.zeros(total + 16, device=DEV)
    m_dev[total:] = SENTINEL
    v_dev[total:] = SENTINEL
    state = torch.zeros(2, device=DEV)
    lr_dev = torch.tensor([lr0], device=DEV)
    count, worst = 0, 0.0

    def launch(grads_dev, gate=None, n=None):
        t = hip.AdamTensors()
        t.n = len(sizes) if n is None else n
        for k in range(min(t.n, hip.ADAM_MAX_TENSORS)):
            j = k % len(sizes)
            t.size[k], t.param[k], t.grad[k] = sizes[j], hip.ptr(p_dev[j]), hip.ptr(grads_dev[j])
        rc = L.vihds_adam_step(ctypes.byref(t), hip.ptr(m_dev), hip.ptr(v_dev), hip.ptr(state), hip.ptr(lr_dev), 123.0, b1, b2,
                               eps, gs, hip.ptr(gate), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    for it in range(3):
        lr = lr0 if it < 2 else lr1
        lr_dev.fill_(lr)
        grads = [None if k == no_grad else _f32((1.0 + it) * 8.0 * torch.randn(s, generator=g, dtype=F64)) for k, s in enumerate(sizes)]
        count = adam_ref(p64, grads, m64, v64, count, lr, b1, b2, eps, gs)
        assert launch([_dev(t) for t in grads]) == 0, L.vihds_last_error()
        assert state.cpu().tolist() == [float(it + 1), 0.0]
        for k in range(len(sizes)):
            if k != no_grad:
                worst = max(worst, rel_err(p_dev[k], p64[k]))
    off = sum(sizes[:no_grad])
    assert torch.equal(p_dev[no_grad].cpu(), p64[no_grad].float())
    m_all, v_all = m_dev.cpu(), v_dev.cpu()
    assert bool((m_all[off: off + 7] == 0).all()) and bool((v_all[off: off + 7] == 0).all())
    assert bool((m_all[total:] == SENTINEL).all()) and bool((v_all[total:] == SENTINEL).all())
    e_m, e_v = rel_err(m_all[:total], torch.cat(m64)), rel_err(v_all[:total], torch.cat(v64))
    # a gated step: a non-finite loss switches the launch off, the count stays
    before = [p.clone() for p in p_dev]
    grads = [_dev(torch.ones(s)) for s in sizes]
    assert launch(grads, gate=torch.tensor([float("nan")], device=DEV)) == 0
    assert state.cpu().tolist() == [3.0, 0.0] and all(torch.equal(a, b) for a, b in zip(before, p_dev))
    assert adam_ref(p64, grads, m64, v64, count, lr1, b1, b2, eps, gs, gate=float("nan")) == count
    # the table limit: 32 tensors run (and count as one step), 33 are rejected before anything is queued
    m_big, v_big = torch.zeros(6 * total, device=DEV), torch.zeros(6 * total, device=DEV)
    m_dev, v_dev = m_big, v_big
    none = [None] * len(sizes)  # (no gradients: nothing is updated, the step still counts)
    assert launch(none, n=consts()["adam_max"]) == 0, L.vihds_last_error()
    assert state.cpu().tolist() == [4.0, 0.0]
    assert launch(none, n=consts()["adam_max"] + 1) < 0
    assert state.cpu().tolist() == [4.0, 0.0] and all(torch.equal(a, b) for a, b in zip(before, p_dev))
    print("adam_step sizes %s: params %.1e  m %.1e  v %.1e (tol %.0e)" % (sizes, worst, e_m, e_v, TOL_ADAM))
    assert worst < TOL_ADAM and e_m < TOL_ADAM and e_v < TOL_ADAM
