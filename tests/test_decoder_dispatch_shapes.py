"""The fused decoder launches (csrc/vihds_dr_scan.hpp: vihds_ode_logp_grad and vihds_theta_ode_logp_grad) and dr_blackbox's
split forward fallback (csrc/ode_dr_blackbox.hip) across the shapes that select their code paths, each against a float64
restatement on the CPU.

The time-parallel kernel family is instantiated per ITEMS = ceil((T - 1) / 32) in 1..4 (steps per lane), per solver and
with or without the sampling stage (THETA); its dynamic LDS grows with ITEMS and the solver's stage count, and past 64 KB
the launcher opts the kernel in to more.  The rest of the suite launches it at T = 2, 31, 86, 100, 129 against the lane
kernels' float32 forward + adjoint, which share the adjoint's algebra with it.  So every case below names its
(solver, ITEMS) and its side of the opt-in, and the Python mirror of the host-side choices (`scan_branches`,
`bb_fwd_branches`, constants read from the headers) checks that the case really lands there.

The restatement is the oracle (oracle/vihds_oracle.py) in float64:
  * theta = clip(sample(q, u)) with O.sample_clip_theta, the device-conditioner rows with O.device_conditioner (the
    reference's .repeat tiling), log q / log p with O.chained_log_prob;
  * O.decode -> O.log_prob_observations for the per-signal log-likelihood, and the unit-weight theta gradient by
    autograd of its sum over signals.  It is evaluated at theta rounded to float32, the numbers the plain entry point is
    handed; the fused entry point samples its own theta, equal to that to float32 rounding.
  * Yardstick (test_hip_parity.py::test_all_solvers_match_oracle_forward_and_gradient): per parameter, the error relative
    to the float64 maximum must stay under max(floor, 8 x the float32 oracle's own error there).  A kernel has to be as
    good as float32 arithmetic allows, not better.
References are cached per (model, solver, T, B, S, seed) and shared by the two entry points; the plain entry point's
three shapes are slices of one 9 x 4 batch (trajectories are independent).

dr_blackbox: the split MFMA forward stages 4 T (1 + 4 rows) bytes, rows = min(B, (TPW - 1) / S + 2); above 48 KB it
declines and the thread-per-trajectory forward runs, followed by the split MFMA adjoint.  (The shape first suggested for
this, B = 5, S = 1..2, T ~ 256, stages 21.5 KB and stays on the split forward; the boundaries are in BB_TABLE.)

Every GPU case prints its worst error next to its bound.
"""
import math
import os
import re
from functools import lru_cache

import pytest
import torch

from fixture_util import Fixture, rel_err
from oracle import vihds_oracle as O

DEV = "cuda:0"
gpu = pytest.mark.gpu
TOL, GTOL = 1e-4, 5e-4  # (test_hip_parity's: values, gradients)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vi-hds_amd", "csrc")
SOLVERS = ["modeuler", "modeulerwhile", "euler", "midpoint", "rk4"]
FIXTURE_OF = {"dr_constant": "dr_constant_icml_tiny_modeuler", "dr_constant_v2": "dr_constant_v2_tiny_modeuler"}


# ---- constants and formulas read from the headers ---------------------------------------------------------------------
def _grab(text, pattern, what):
    m = re.search(pattern, text)
    assert m is not None, "header changed under the mirror: %s (%r)" % (what, pattern)
    return tuple(int(g) for g in m.groups() if g)


@lru_cache(maxsize=None)
def header():
    read = lambda f: open(os.path.join(CSRC, f)).read()  # noqa: E731
    scan, mfma, split = read("vihds_dr_scan.hpp"), read("vihds_blackbox_mfma.hpp"), read("vihds_blackbox_split.hpp")
    h = {}
    (h["tpb"],) = _grab(scan, r"#define VIHDS_SCAN_TPB (\d+)", "DR_SCAN_TPB")
    (h["lanes"],) = _grab(scan, r"constexpr int DR_SCAN_THREADS = (\d+) \* DR_SCAN_TPB;", "DR_SCAN_THREADS")
    (h["nacc"],) = _grab(scan, r"constexpr int DR_SCAN_NACC = (\d+);", "DR_SCAN_NACC")
    (h["red_pad"],) = _grab(scan, r"constexpr int DR_SCAN_RED_STRIDE = DR_SCAN_THREADS \+ (\d+);", "DR_SCAN_RED_STRIDE")
    h["ns"] = _grab(scan, r"NS = SOLVER == VIHDS_SOLVER_EULER \? (\d+) : \(SOLVER == VIHDS_SOLVER_RK4 \? (\d+) : (\d+)\);",
                    "Rk<SOLVER>::NS")
    h["step"] = _grab(scan, r"steps = \(size_t\)\((\d+) \* Rk<SOLVER>::NS \+ (\d+)\) \* items \* DR_SCAN_THREADS;",
                      "dr_scan_lds_floats: per-step floats")
    (h["gout"],) = _grab(scan, r"red = \(size_t\)DR_SCAN_NACC \* DR_SCAN_RED_STRIDE \+ DR_SCAN_TPB \* DR_SCAN_NACC \+ "
                               r"DR_SCAN_TPB \* (\d+);", "dr_scan_lds_floats: reduction overlay")
    h["grid"] = _grab(scan, r"\(steps > red \? steps : red\) \+ \(size_t\)\((\d+) \* items \+ (\d+)\) \+ DR_SCAN_TPB;",
                      "dr_scan_lds_floats: time grid")
    _grab(scan, r"return \(size_t\)E \* D \+ \(size_t\)DR_SCAN_TPB \* D \+ \(size_t\)E;()", "dr_scan_theta_floats")
    h["items"] = _grab(scan, r"const int items = \(K \+ (\d+)\) / (\d+);", "ITEMS")
    (h["items_max"],) = _grab(scan, r"if \(items > (\d+)\) return VIHDS_E_UNSUPPORTED;", "ITEMS limit")
    (h["nb_pad"],) = _grab(scan, r"const int nb_max = min\(a\.B, \(DR_SCAN_TPB - 1\) / a\.S \+ (\d+)\);", "nb_max")
    h["theta_lim"] = _grab(scan, r"if \(ts->P > (\d+) \|\| ts->n_rows > (\d+) \|\| ts->E > (\d+)\) return VIHDS_E_UNSUPPORTED;",
                           "theta-stage P / n_rows / E limits")
    (h["ed_lim"],) = _grab(scan, r"if \(ts->E \* a\.D > (\d+)\) return VIHDS_E_UNSUPPORTED;", "theta-stage E*D limit")
    (h["slot_lim"],) = _grab(scan, r"if \(a\.slot_row\[q\] >= (\d+)\) return VIHDS_E_UNSUPPORTED;", "slot_row limit")
    _grab(scan, r"dr_scan_lds_floats<SV>\(IT\) \+ \(ts \? dr_scan_theta_floats\(ts->E, a\.D\) : 0\)\) \* sizeof\(float\)()",
          "launch LDS = scan + theta floats")
    (h["optin_kb"],) = _grab(scan, r"if \(lds > (\d+) \* 1024 && !have\)", "LDS opt-in threshold")
    (h["tpw"],) = _grab(mfma, r"static constexpr int TPW = (\d+),", "BbMfma::TPW")
    (h["bb_pad"],) = _grab(split, r"const int rows = min\(a\.B, \(K::TPW - 1\) / a\.S \+ (\d+)\);", "bb_fwd_stage_rows")
    (h["bb_sig"],) = _grab(split, r"\*bytes = sizeof\(float\) \* \(\(size_t\)a\.T \+ \(size_t\)rows \* (\d+) \* a\.T\);",
                           "bb_fwd_stage_rows: bytes")
    (h["bb_kb"],) = _grab(split, r"if \(\*bytes > (\d+) \* 1024\) \{ \*bytes = 0; return 0; \}", "bb_fwd_stage_rows: limit")
    return h


# ---- Python mirror of the host-side choices ---------------------------------------------------------------------------
def solver_ns(solver):
    euler, rk4, other = header()["ns"]
    return euler if solver == "euler" else (rk4 if solver == "rk4" else other)


def scan_branches(T, B, S, solver, theta_stage=None, max_slot_row=0):
    """launch_dr_scan_train's choices.  theta_stage: None, or dict(P, n_rows, E, D) of the sampling stage
    (vihds_theta_ode_logp_grad); max_slot_row: the largest row of theta a model slot reads."""
    h = header()
    add, div = h["items"]
    items = (T - 1 + add) // div
    threads = h["lanes"] * h["tpb"]
    a, b = h["step"]
    steps = (a * solver_ns(solver) + b) * items * threads
    red = h["nacc"] * (threads + h["red_pad"]) + h["tpb"] * h["nacc"] + h["tpb"] * h["gout"]
    g1, g0 = h["grid"]
    floats = max(steps, red) + g1 * items + g0 + h["tpb"]
    reason = None
    if items > h["items_max"]:
        reason = "ITEMS %d > %d" % (items, h["items_max"])
    if theta_stage is not None:
        ts = theta_stage
        lp, lr, le = h["theta_lim"]
        E, D = ts["E"], ts["D"]
        floats += E * D + h["tpb"] * D + E
        if reason is None and (ts["P"] > lp or ts["n_rows"] > lr or E > le):
            reason = "P / n_rows / E past %d / %d / %d" % (lp, lr, le)
        if reason is None and E * D > h["ed_lim"]:
            reason = "E*D %d > %d" % (E * D, h["ed_lim"])
    if reason is None and max_slot_row >= h["slot_lim"]:
        reason = "slot row >= %d" % h["slot_lim"]
    nbytes = 4 * floats
    return dict(items=items, nb_max=min(B, (h["tpb"] - 1) // S + h["nb_pad"]), lds_bytes=nbytes,
                steps_dominate=steps > red, optin=nbytes > h["optin_kb"] * 1024, supported=reason is None, reason=reason)


def bb_fwd_branches(B, S, T):
    """bb_fwd_stage_rows: the split MFMA forward's staged rows and bytes; split=False -> the thread-per-trajectory forward."""
    h = header()
    rows = min(B, (h["tpw"] - 1) // S + h["bb_pad"])
    nbytes = 4 * (T + rows * h["bb_sig"] * T)
    return dict(rows=rows, bytes=nbytes, split=nbytes <= h["bb_kb"] * 1024)


# (S, B) -> (last T on the split forward, first T on the thread-per-trajectory forward)
BB_TABLE = {(1, 17): (178, 179), (1, 5): (585, 586), (2, 9): (332, 333), (16, 2): (1365, 1366)}


def test_header_constants_are_read_and_consistent():
    """Every constant and formula the mirror uses is found in the headers (a changed header fails here, not silently in
    the GPU cases' labels), and the pieces fit each other: two trajectories per wavefront, ceil((T - 1) / 32)."""
    h = header()
    assert (h["lanes"] * h["tpb"]) % 64 == 0 and h["items"][1] == h["lanes"] and h["items"][0] == h["lanes"] - 1
    assert h["grid"][0] == h["lanes"] and h["nacc"] >= 29 and h["ns"] == tuple(solver_ns(s) for s in ("euler", "rk4", "midpoint"))
    assert h["ed_lim"] > 0 and h["optin_kb"] > h["bb_kb"] and h["tpw"] > 1


def test_scan_lds_layout_per_solver_and_items():
    """The dynamic LDS of every (solver, ITEMS) pair: the reduction overlay dominates at ITEMS 1 (and at 2 for euler), the
    per-step area grows by (3 NS + 14) floats per lane-step, and both sides of the 64 KB opt-in occur -- the GPU cases
    below launch every pair through both entry points."""
    h = header()
    threads = h["lanes"] * h["tpb"]
    rows = []
    for solver in SOLVERS:
        for items in range(1, h["items_max"] + 1):
            T = 32 * items + 1
            br = scan_branches(T, 9, 4, solver)
            br_t = scan_branches(T, 9, 4, solver, dict(P=35, n_rows=37, E=2, D=7))
            assert br["items"] == items and br["supported"] and br_t["supported"]
            assert br_t["lds_bytes"] == br["lds_bytes"] + 4 * (2 * 7 + h["tpb"] * 7 + 2)
            rows.append((solver, items, br["lds_bytes"], br["optin"], br_t["optin"]))
            print("%-13s ITEMS %d  LDS %6d B (%s)  opt-in %s / THETA %s" % (solver, items, br["lds_bytes"],
                  "steps" if br["steps_dominate"] else "reduction", br["optin"], br_t["optin"]))
        per_items = (3 * solver_ns(solver) + 14) * threads * 4
        assert not scan_branches(33, 9, 4, solver)["steps_dominate"]
        assert scan_branches(129, 9, 4, solver)["lds_bytes"] - scan_branches(97, 9, 4, solver)["lds_bytes"] == per_items + 4 * 32
    assert {r[3] for r in rows} == {False, True} and {r[4] for r in rows} == {False, True}
    # per lane-step: euler 17 floats, the two-stage schemes 20, rk4 26 -> per ITEMS 17 / 20 / 26 KB at 8 trajectories
    assert [(3 * solver_ns(s) + 14) * threads * 4 // 1024 for s in ("euler", "midpoint", "rk4")] == [17, 20, 26]
    assert not scan_branches(130, 9, 4, "rk4")["supported"] and scan_branches(129, 9, 4, "rk4")["supported"]


def test_theta_stage_decline_edges_in_the_mirror():
    """E*D = 128 accepted, 130 (D = 65) declined; P = 64 (n_rows 64) accepted, 65 declined; a slot row of 64 declined."""
    ok = lambda m=0, **kw: scan_branches(34, 9, 4, "rk4", dict(dict(P=35, n_rows=37, E=2, D=7), **kw), m)["supported"]  # noqa: E731
    assert ok(D=64) and not ok(D=65)
    assert ok(P=64, n_rows=64, E=0, D=7) and not ok(P=65, n_rows=65, E=0, D=7)
    assert ok(E=32, D=4, n_rows=64, P=32) and not ok(E=33, D=1, n_rows=64, P=31)
    assert not ok(64) and ok(63)


def test_blackbox_split_forward_boundaries_come_out_of_the_mirror():
    """The last T on the split MFMA forward and the first on the thread-per-trajectory forward, per (S, B); the shape
    first suggested for the fallback (B 5, S 1..2, T 256) stays on the split forward."""
    for (S, B), (last, first) in BB_TABLE.items():
        assert bb_fwd_branches(B, S, last)["split"] and not bb_fwd_branches(B, S, first)["split"], (S, B)
    assert bb_fwd_branches(40, 1, 178)["rows"] == 17 and bb_fwd_branches(100, 32, 1365)["rows"] == 2
    for S in (1, 2):
        assert bb_fwd_branches(5, S, 256)["split"]


# ---- problems and float64 references ----------------------------------------------------------------------------------
UB, US = 9, 4  # the union batch of the plain entry point's shapes (and the fused entry point's shape)
A_SHAPES = [("partial block B3xS4", 3, 4), ("S 1: B9xS1", 9, 1), ("single trajectory", 1, 1)]


@lru_cache(maxsize=None)
def make_problem(model, T, B, S, seed, D=7):
    """Seeded inputs on the CPU (float32 values): q tables around the reference fixture's (local parameters jittered per
    row), draws u, treatments, a jittered time grid (modeuler's fixed h differs from the per-step h), observations, the
    device matrix and conditioner (weights w_mean + w_std z, relevance, defaults), and the weights of the q-gradient's
    loss (sum_bs wl sum_signals logp + a log q + c log p)."""
    fx = Fixture(FIXTURE_OF[model])
    g = torch.Generator().manual_seed(seed)
    P = len(fx.names)
    cols = torch.arange(B) % fx.B
    glob = fx.t("q_is_global").bool()[:, None]
    q_mu = fx.t("q_mu")[:, cols]
    q_mu = torch.where(glob, q_mu, q_mu + 0.05 * torch.randn(P, B, generator=g))
    q_lp = fx.t("q_prec")[:, cols].log()
    q_lp = torch.where(glob, q_lp, q_lp + 0.1 * torch.randn(P, B, generator=g))
    E = len(fx.extra_names)
    if D == 7:
        rel = torch.tensor([fx.cfg["relevance"][n] for n in fx.extra_names])
    else:
        rel = (torch.rand(E, D, generator=g) < 0.7).float()
    dev = torch.rand(B, D, generator=g)
    dev[torch.rand(B, D, generator=g) < 0.5] = 0.0
    return dict(
        model=model, names=list(fx.names), extra=list(fx.extra_names), kinds=list(fx.kinds), B=B, S=S, T=T, D=D,
        q_mu=q_mu.float(), q_lp=q_lp.float(), p_mu=fx.t("p_mu"), p_prec=fx.t("p_prec"),
        u=torch.randn(B, S, P, generator=g), cond=torch.log1p(torch.rand(B, 2, generator=g) * 1000.0),
        times=torch.arange(T, dtype=torch.float32) * 0.1933 + 0.003 * torch.rand(T, generator=g),
        obs=torch.rand(B, 4, T, generator=g), dev=dev, rel=rel, dflt=torch.tensor([1, 0][:E], dtype=torch.int32),
        z=torch.randn(E, D, generator=g), w_mean=0.3, w_std=1.7,
        wl=torch.rand(B, S, generator=g), wa=torch.randn(B, S, generator=g), wc=torch.randn(B, S, generator=g))


def _sample(pr, dtype):
    """theta (P names + conditioner rows) in `dtype` from q leaves; returns (theta dict, q leaves, log q, log p)."""
    P = len(pr["names"])
    qm = pr["q_mu"].to(dtype).clone().requires_grad_(True)
    ql = pr["q_lp"].to(dtype).clone().requires_grad_(True)
    mus, precs = [qm[p][:, None] for p in range(P)], [ql[p][:, None].exp() for p in range(P)]
    pm, pp = [pr["p_mu"][p].to(dtype) for p in range(P)], [pr["p_prec"][p].to(dtype) for p in range(P)]
    th = O.sample_clip_theta(pr["names"], pr["kinds"], mus, precs, pm, pp, pr["u"].to(dtype))
    vals = [th[n] for n in pr["names"]]
    log_q = O.chained_log_prob(pr["kinds"], mus, precs, vals)
    log_p = O.chained_log_prob(pr["kinds"], pm, pp, vals)
    ones = torch.ones(pr["B"], pr["S"], dtype=dtype)
    for e, n in enumerate(pr["extra"]):
        w = (pr["w_mean"] + pr["w_std"] * pr["z"][e].to(dtype))[None, :]
        th[n] = O.device_conditioner(w, ones, pr["rel"][e].to(dtype), pr["dev"].to(dtype), bool(pr["dflt"][e]))
    return th, (qm, ql), log_q, log_p


@lru_cache(maxsize=None)
def reference(model, solver, T, B, S, seed, D=7):
    """Per dtype (float64, float32): theta, the per-signal log-likelihood [B,S,4] and unit-weight theta gradient at
    theta rounded to float32 (the values the plain entry point is handed), log q / log p, and the q-table gradients of
    sum(wl * sum_signals logp + wa * log q + wc * log p) -- the decoder term as its linearisation g_unit . theta, which is
    what the theta adjoint consumes."""
    pr = make_problem(model, T, B, S, seed, D)
    out = {}
    th64, _, _, _ = _sample(pr, torch.float64)
    theta_r = {n: v.detach().float() for n, v in th64.items()}  # the float32 theta of both entry points
    for dtype in (torch.float64, torch.float32):
        leaves = {n: v.to(dtype).clone().requires_grad_(True) for n, v in theta_r.items()}
        _, xp, prec = O.decode(model, leaves, pr["cond"].to(dtype), pr["times"].to(dtype), solver)
        lpo = O.log_prob_observations(xp, pr["obs"].to(dtype), prec)
        names = list(leaves)
        g_unit = dict(zip(names, torch.autograd.grad(lpo.sum(), [leaves[n] for n in names], allow_unused=True)))
        g_unit = {n: (torch.zeros(B, S, dtype=dtype) if v is None else v) for n, v in g_unit.items()}
        th, (qm, ql), log_q, log_p = _sample(pr, dtype)
        lin = sum((g_unit[n].detach() * pr["wl"].to(dtype) * th[n]).sum() for n in pr["names"])
        loss = lin + (pr["wa"].to(dtype) * log_q).sum() + (pr["wc"].to(dtype) * log_p).sum()
        gm, gl = torch.autograd.grad(loss, [qm, ql])
        out[dtype] = dict(lpo=lpo.detach(), g_unit=g_unit, log_q=log_q.detach(), log_p=log_p.detach(), g_mu=gm, g_lp=gl,
                          theta={n: v.detach() for n, v in th.items()})
    out["theta_r"] = theta_r
    return pr, out


def yardstick(got, r64, r32, floor):
    """(error, bound) relative to the float64 maximum; bound = max(floor, 8 x the float32 oracle's own error).  A slice whose
    float64 value is exactly 0 must come back exactly 0 (bound 0, error = max |got|)."""
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    scale = float(r64.abs().max())
    if scale == 0.0:
        return float(got.abs().max()), 0.0
    return float((got - r64).abs().max()) / scale, max(floor, 8.0 * float((r32 - r64).abs().max()) / scale)


class Report:
    """Worst error / bound per quantity; check() asserts and prints one line."""

    def __init__(self, label):
        self.label, self.items = label, {}

    def add(self, key, err, bound, where=None):
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        if key not in self.items or ratio > self.items[key][2]:
            self.items[key] = (err, bound, ratio, where)

    def per_row(self, key, got, r64, r32, floor):
        for k in range(r64.shape[0]):
            self.add(key, *yardstick(got[k], r64[k], r32[k], floor), where=k)

    def check(self):
        print("%-58s " % self.label + "  ".join("%s %.1e (%.0e)" % (k, v[0], v[1]) for k, v in sorted(self.items.items())))
        bad = {k: v for k, v in self.items.items() if not v[0] <= v[1]}
        assert not bad, (self.label, bad)


def _slot_rows(model, holes):
    """row_of of the kernel's theta buffer: the model's slots in order with unused rows at `holes` (the kernel must leave
    them alone; the product path hands them back as zeros)."""
    from vihds import hip

    slots = hip.model_slots(model)
    n_rows = len(slots) + len(holes)
    free = [r for r in range(n_rows) if r not in holes]
    return slots, {n: free[k] for k, n in enumerate(slots)}, n_rows


# ---- 0. the oracle against its own float32 run (CPU) ------------------------------------------------------------------
def test_float64_reference_agrees_with_its_float32_run():
    """At one shape (rk4, T 34: ITEMS 2, the union batch) the float64 and float32 restatements agree to float32 accuracy:
    the per-signal log-likelihood, every slot's unit-weight gradient, log q / log p and the q-table gradients (so the
    yardstick measures float32 conditioning, not a bug in the reference)."""
    pr, ref = reference("dr_constant", "rk4", 34, UB, US, 1)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert rel_err(r32["lpo"], r64["lpo"], dim=2) < 1e-5
    assert rel_err(r32["log_q"], r64["log_q"]) < 1e-5 and rel_err(r32["log_p"], r64["log_p"]) < 1e-5
    for n, g in r64["g_unit"].items():
        e, _ = yardstick(r32["g_unit"][n], g, g, 0.0)
        assert e < GTOL, n
    live = torch.tensor([k != O.CONSTANT for k in pr["kinds"]])
    assert rel_err(r32["g_mu"][live], r64["g_mu"][live], dim=0) < GTOL
    assert rel_err(r32["g_lp"][live], r64["g_lp"][live], dim=0) < GTOL
    assert float(r64["g_unit"]["r"].abs().max()) > 0 and float(r64["g_mu"][live].abs().max()) > 0


# ---- A. vihds_ode_logp_grad, kernel_variant 3 (GPU) -------------------------------------------------------------------
A_T = [2, 33, 34, 65, 66, 97, 98, 129]
A_CASES = ([("dr_constant", s, T) for T in A_T for s in SOLVERS]
           + [("dr_constant_v2", s, T) for T in (34, 66, 98, 129) for s in SOLVERS])


def _a_id(c):
    model, solver, T = c
    br = scan_branches(T, UB, US, solver)
    return "%s-%s-T%d-ITEMS%d-%s" % (model, solver, T, br["items"], "optin" if br["optin"] else "lds64k")


@gpu
@pytest.mark.parametrize("model,solver,T", A_CASES, ids=[_a_id(c) for c in A_CASES])
def test_logp_grad_kernel_against_float64(model, solver, T):
    """ops.OdeLogLikFused (vihds_ode_logp_grad, kernel_variant 3) at a partial block (B*S not a multiple of 8), S 1 (up to
    nb_max = 9 data rows per block) and a single trajectory: per-signal log-likelihood and unit-weight gradient of every
    slot against float64; rows of the theta buffer that are not slots come back exactly 0."""
    from vihds import ops

    pr, ref = reference(model, solver, T, UB, US, 1)
    slots, row_of, n_rows = _slot_rows(model, (0, 7))
    rep = Report("A %s %s" % (_a_id((model, solver, T)), "partial/S1/single"))
    for label, B, S in A_SHAPES:
        br = scan_branches(T, B, S, solver, max_slot_row=n_rows - 1)
        assert br["supported"] and br["items"] == scan_branches(T, UB, US, solver)["items"], (label, br)
        assert br["optin"] == scan_branches(T, UB, US, solver)["optin"]
        theta = torch.full((n_rows, B, S), 777.0)
        for n in slots:
            theta[row_of[n]] = ref["theta_r"][n][:B, :S]
        spec = ops.OdeProblemSpec(model, solver, row_of, n_rows, C=2, kernel_variant=3)
        th = theta.to(DEV).requires_grad_(True)
        logp = ops.OdeLogLikFused.apply(spec, th, pr["cond"][:B].to(DEV), pr["times"].to(DEV), pr["obs"][:B].to(DEV), None)
        g_unit = logp.grad_fn.saved_tensors[5].cpu()
        torch.cuda.synchronize()
        logp = logp.detach().cpu().permute(1, 2, 0)  # [B,S,4]
        r64, r32 = ref[torch.float64], ref[torch.float32]
        rep.per_row("logp", logp.permute(2, 0, 1), r64["lpo"][:B, :S].permute(2, 0, 1), r32["lpo"][:B, :S].permute(2, 0, 1), TOL)
        got = torch.stack([g_unit[row_of[n]] for n in slots])
        rep.per_row("g_unit", got, torch.stack([r64["g_unit"][n][:B, :S] for n in slots]),
                    torch.stack([r32["g_unit"][n][:B, :S] for n in slots]), GTOL)
        rep.add("holes", float(g_unit[[0, 7]].abs().max()), 0.0)
    rep.check()


# ---- B. ops.DecoderStepFused: the sampling stage and the conditioner in the same launch (GPU) -------------------------
def _q_layout(P, seed):
    """q_all rows in a shuffled order (q_rows maps parameter p to its mu row and P + p to its log-precision row)."""
    perm = torch.randperm(2 * P, generator=torch.Generator().manual_seed(seed))
    return perm, torch.argsort(perm)  # q_all[k] = [mu; log prec][perm[k]];  q_rows[j] = position of entry j


def _decoder_step(pr, solver):
    """One DecoderStepFused forward + backward at problem `pr` (the union shape); returns the outputs on the CPU."""
    import hip_util as H
    from vihds import ops

    P, E, B, S = len(pr["names"]), len(pr["extra"]), pr["B"], pr["S"]
    perm, q_rows = _q_layout(P, 3)
    q_all = torch.cat([pr["q_mu"], pr["q_lp"]], 0)[perm].contiguous().to(DEV).requires_grad_(True)
    kind = torch.tensor(pr["kinds"], dtype=torch.int32, device=DEV)
    lo, hi = H.clip_bounds(pr["kinds"], pr["p_mu"], pr["p_prec"], 4.0)
    row_of = {n: k for k, n in enumerate(pr["names"] + pr["extra"])}
    spec = ops.OdeProblemSpec(pr["model"], solver, row_of, P + E, C=2, D=pr["D"], kernel_variant=3)
    cond_job = (E, P, pr["w_mean"], pr["w_std"], pr["z"].to(DEV), None, pr["rel"].to(DEV), pr["dflt"].to(DEV))
    theta, log_q, log_p, _u, logp = ops.DecoderStepFused.apply(
        q_all, kind, pr["p_mu"].to(DEV), pr["p_prec"].to(DEV), lo.to(DEV), hi.to(DEV), pr["u"].to(DEV), P + E,
        q_rows.to(torch.int32).to(DEV), spec, pr["cond"].to(DEV), pr["times"].to(DEV), pr["obs"].to(DEV),
        pr["dev"].to(DEV), cond_job)
    g_unit = logp.grad_fn.saved_tensors[8].detach().cpu()
    wl = pr["wl"].to(DEV)
    torch.autograd.backward([logp, log_q, log_p], [wl[None].expand(4, B, S), pr["wa"].to(DEV), pr["wc"].to(DEV)])
    torch.cuda.synchronize()
    g = q_all.grad.cpu()[q_rows]
    return dict(theta=theta.detach().cpu(), log_q=log_q.detach().cpu(), log_p=log_p.detach().cpu(),
                logp=logp.detach().cpu(), g_unit=g_unit, g_mu=g[:P], g_lp=g[P:])


def _check_decoder_step(label, pr, ref, out):
    P = len(pr["names"])
    r64, r32 = ref[torch.float64], ref[torch.float32]
    names = pr["names"] + pr["extra"]
    rep = Report(label)
    # theta: the kernel's own float32 sample (1e-5, as the fixture test) -- the conditioner rows to 1e-6
    rep.add("theta", rel_err(out["theta"][:P], torch.stack([r64["theta"][n] for n in pr["names"]]), dim=0), 1e-5)
    rep.add("theta_cond", rel_err(out["theta"][P:], torch.stack([r64["theta"][n] for n in pr["extra"]]), dim=0), 1e-6)
    rep.add("log_q", *yardstick(out["log_q"], r64["log_q"], r32["log_q"], TOL))
    rep.add("log_p", *yardstick(out["log_p"], r64["log_p"], r32["log_p"], TOL))
    rep.per_row("logp", out["logp"], r64["lpo"].permute(2, 0, 1), r32["lpo"].permute(2, 0, 1), TOL)
    rep.per_row("g_unit", out["g_unit"], torch.stack([r64["g_unit"][n] for n in names]),
                torch.stack([r32["g_unit"][n] for n in names]), GTOL)
    live = torch.tensor([k != O.CONSTANT for k in pr["kinds"]])
    rep.per_row("dL/dq_mu", out["g_mu"][live], r64["g_mu"][live], r32["g_mu"][live], GTOL)
    rep.per_row("dL/dq_logprec", out["g_lp"][live], r64["g_lp"][live], r32["g_lp"][live], GTOL)
    rep.check()


B_CASES = [(s, T) for T in A_T for s in SOLVERS]


def _b_id(c):
    solver, T = c
    br = scan_branches(T, UB, US, solver, dict(P=35, n_rows=37, E=2, D=7))
    return "dr_constant-%s-T%d-ITEMS%d-%s" % (solver, T, br["items"], "optin" if br["optin"] else "lds64k")


@gpu
@pytest.mark.parametrize("solver,T", B_CASES, ids=[_b_id(c) for c in B_CASES])
def test_decoder_step_kernel_against_float64(solver, T):
    """ops.DecoderStepFused (vihds_theta_ode_logp_grad: THETA on) at 9 rows x 4 samples (a partial last block, global q
    parameters, q rows shuffled, the conditioner with E = 2): theta (conditioner rows included), log q, log p, the
    per-signal log-likelihood and the unit-weight gradient, then through vihds_theta_bwd d loss / d q_mu and
    d loss / d log-precision, all against float64 on the references the plain entry point's cases use."""
    pr, ref = reference("dr_constant", solver, T, UB, US, 1)
    br = scan_branches(T, UB, US, solver, dict(P=len(pr["names"]), n_rows=len(pr["names"]) + 2, E=2, D=pr["D"]))
    assert br["supported"] and br["nb_max"] == 3
    _check_decoder_step("B " + _b_id((solver, T)), pr, ref, _decoder_step(pr, solver))


@gpu
def test_decoder_step_theta_stage_edges():
    """E*D = 128 (E 2, D 64) is the widest conditioner the launch takes: accepted and correct; D = 65 is declined
    (FusedTrainingUnsupported) before anything runs."""
    from vihds import ops

    solver, T = "rk4", 34
    pr, ref = reference("dr_constant", solver, T, UB, US, 1, 64)
    assert scan_branches(T, UB, US, solver, dict(P=35, n_rows=37, E=2, D=64))["supported"]
    _check_decoder_step("B E*D 128 (D 64) rk4 T34", pr, ref, _decoder_step(pr, solver))
    pr65 = make_problem("dr_constant", T, UB, US, 1, 65)
    assert not scan_branches(T, UB, US, solver, dict(P=35, n_rows=37, E=2, D=65))["supported"]
    with pytest.raises(ops.FusedTrainingUnsupported):
        _decoder_step(pr65, solver)


@gpu
@pytest.mark.parametrize("P", [64, 65])
def test_decoder_step_at_the_parameter_count_limit(P):
    """P = 64 sampled parameters (the 35 of dr_constant, aR / aS sampled too, 27 more that no slot reads; n_rows 64, every
    slot row < 64, no conditioner) is accepted: theta against the float64 sample, and the slots' log-likelihood against
    the float64 decode of that theta.  P = 65 is declined."""
    import hip_util as H
    from vihds import hip, ops

    solver, T, B, S = "midpoint", 34, 3, 4
    base = make_problem("dr_constant", T, B, S, 5)
    g = torch.Generator().manual_seed(9)
    n_more = P - len(base["names"]) - 2
    names = base["names"] + ["aR", "aS"] + ["extra%d" % k for k in range(n_more)]
    kinds = base["kinds"] + [O.LOGNORMAL, O.LOGNORMAL] + [O.NORMAL] * n_more
    q_mu = torch.cat([base["q_mu"], torch.full((2, B), 0.0), torch.randn(n_more, B, generator=g)])
    q_lp = torch.cat([base["q_lp"], torch.full((2, B), 4.0), torch.zeros(n_more, B)])
    p_mu = torch.cat([base["p_mu"], torch.zeros(2 + n_more)])
    p_prec = torch.cat([base["p_prec"], torch.ones(2 + n_more)])
    u = torch.randn(B, S, P, generator=g)
    assert scan_branches(T, B, S, solver, dict(P=P, n_rows=P, E=0, D=0))["supported"] == (P <= 64)
    spec = ops.OdeProblemSpec("dr_constant", solver, {n: k for k, n in enumerate(names)}, P, C=2, kernel_variant=3)
    lo, hi = H.clip_bounds(kinds, p_mu, p_prec, 4.0)
    args = (torch.cat([q_mu, q_lp]).to(DEV), torch.tensor(kinds, dtype=torch.int32, device=DEV), p_mu.to(DEV),
            p_prec.to(DEV), lo.to(DEV), hi.to(DEV), u.to(DEV), P, torch.arange(2 * P, dtype=torch.int32, device=DEV), spec,
            base["cond"].to(DEV), base["times"].to(DEV), base["obs"].to(DEV), None, None)
    if P > 64:
        with pytest.raises(ops.FusedTrainingUnsupported):
            ops.DecoderStepFused.apply(*args)
        return
    with torch.no_grad():
        theta, _lq, _lp, _u, logp = ops.DecoderStepFused.apply(*args)
    torch.cuda.synchronize()
    th64 = O.sample_clip_theta(names, kinds, [q_mu[p].double()[:, None] for p in range(P)],
                               [q_lp[p].double().exp()[:, None] for p in range(P)], [p_mu[p].double() for p in range(P)],
                               [p_prec[p].double() for p in range(P)], u.double())
    rep = Report("B P %d (n_rows 64, no conditioner) %s T%d" % (P, solver, T))
    rep.add("theta", rel_err(theta.cpu(), torch.stack([th64[n] for n in names]), dim=0), 1e-5)
    lp = {}
    for dtype in (torch.float64, torch.float32):
        th = {n: th64[n].float().to(dtype) for n in hip.model_slots("dr_constant")}
        _, xp, prec = O.decode("dr_constant", th, base["cond"].to(dtype), base["times"].to(dtype), solver)
        lp[dtype] = O.log_prob_observations(xp, base["obs"].to(dtype), prec).permute(2, 0, 1)
    rep.per_row("logp", logp.cpu(), lp[torch.float64], lp[torch.float32], TOL)
    rep.check()


# ---- C. time grids past the fused kernels: declines and the two-kernel path (GPU) -------------------------------------
@lru_cache(maxsize=None)
def reference_full(model, solver, T, B, S, seed):
    """float64 / float32 trajectories, predictions, log-likelihood and the theta gradient of
    1e-2 sum(traj ct0) + 1e-2 sum(xpred ct1) + 1e-3 sum(logp ct2) at theta rounded to float32."""
    pr, ref = reference(model, solver, T, B, S, seed)
    g = torch.Generator().manual_seed(seed + 100)
    ct = [torch.randn(B, S, 8, T, generator=g), torch.randn(B, S, 4, T, generator=g), torch.randn(B, S, 4, generator=g)]
    out = {}
    for dtype in (torch.float64, torch.float32):
        leaves = {n: v.to(dtype).clone().requires_grad_(True) for n, v in ref["theta_r"].items()}
        xs, xp, prec = O.decode(model, leaves, pr["cond"].to(dtype), pr["times"].to(dtype), solver)
        lpo = O.log_prob_observations(xp, pr["obs"].to(dtype), prec)
        f = 1e-2 * (xs * ct[0].to(dtype)).sum() + 1e-2 * (xp * ct[1].to(dtype)).sum() + 1e-3 * (lpo * ct[2].to(dtype)).sum()
        names = list(leaves)
        gs = torch.autograd.grad(f, [leaves[n] for n in names], allow_unused=True)
        out[dtype] = dict(xs=xs.detach(), xp=xp.detach(), lpo=lpo.detach(),
                          g={n: (torch.zeros(B, S, dtype=dtype) if v is None else v) for n, v in zip(names, gs)})
    return pr, ref, ct, out


@gpu
@pytest.mark.parametrize("T", [130, 135])
@pytest.mark.parametrize("solver", SOLVERS)
def test_grids_past_the_fused_kernels_decline_and_the_two_kernel_path_holds(solver, T):
    """T = 130 / 135 (ITEMS 5; real plate data reach 135 points): OdeLogLikFused and DecoderStepFused raise
    FusedTrainingUnsupported; OdeSolveObserve with kernel_variant 0 (lane kernels) and 1 (one thread per trajectory)
    matches float64 on traj, x_predict, logp and the theta gradient of cotangents on all three."""
    import hip_util as H
    from vihds import ops

    B, S = 3, 4
    pr, ref, ct, full = reference_full("dr_constant", solver, T, B, S, 2)
    assert not scan_branches(T, B, S, solver)["supported"]
    slots, row_of, n_rows = _slot_rows("dr_constant", ())
    theta = torch.stack([ref["theta_r"][n] for n in slots]).to(DEV)
    cond, times, obs = pr["cond"].to(DEV), pr["times"].to(DEV), pr["obs"].to(DEV)
    spec3 = ops.OdeProblemSpec("dr_constant", solver, row_of, n_rows, C=2, kernel_variant=3)
    with pytest.raises(ops.FusedTrainingUnsupported):
        ops.OdeLogLikFused.apply(spec3, theta.clone().requires_grad_(True), cond, times, obs, None)
    with pytest.raises(ops.FusedTrainingUnsupported):
        _decoder_step(pr, solver)
    r64, r32 = full[torch.float64], full[torch.float32]
    for variant in (0, 1):
        spec = ops.OdeProblemSpec("dr_constant", solver, row_of, n_rows, C=2, kernel_variant=variant)
        th = theta.clone().requires_grad_(True)
        traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, cond, times, obs, None, None)
        (1e-2 * (H.view_bsnt(traj) * ct[0].to(DEV)).sum() + 1e-2 * (H.view_bsnt(xpred) * ct[1].to(DEV)).sum()
         + 1e-3 * (H.view_bs4(logp) * ct[2].to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        rep = Report("C dr_constant %s T%d kernel_variant %d" % (solver, T, variant))
        rep.per_row("traj", H.view_bsnt(traj).cpu().permute(2, 0, 1, 3), r64["xs"].permute(2, 0, 1, 3),
                    r32["xs"].permute(2, 0, 1, 3), TOL)
        rep.per_row("xpred", H.view_bsnt(xpred).cpu().permute(2, 0, 1, 3), r64["xp"].permute(2, 0, 1, 3),
                    r32["xp"].permute(2, 0, 1, 3), TOL)
        rep.per_row("logp", H.view_bs4(logp).cpu().permute(2, 0, 1), r64["lpo"].permute(2, 0, 1), r32["lpo"].permute(2, 0, 1), TOL)
        rep.per_row("g_theta", th.grad.cpu(), torch.stack([r64["g"][n] for n in slots]),
                    torch.stack([r32["g"][n] for n in slots]), GTOL)
        rep.check()


@gpu
def test_training_step_at_135_points_takes_the_two_kernel_path(monkeypatch):
    """Eager Training.steps of the synthetic dr_constant_icml plate at 135 time points (real plates reach that): both
    declines cached after the first step (the fused decoder step, the fused log-likelihood), no decoder_step or
    ode_logp_grad launch asked for in the second, and its loss and the theta gradient that reaches the integrator's input
    match a float64 recomputation from the theta it was handed.
    (fused_step_tail off: the theta gradient is autograd's, observable at the integrator's input.)"""
    from vihds import ops, synthetic

    spec_fn, _ = synthetic.WORKLOADS["dr_constant_icml"]
    monkeypatch.setitem(synthetic.WORKLOADS, "dr_constant_icml", (spec_fn, 135))
    _, _, _, _, model, training = synthetic.build(
        "dr_constant_icml", 4, 6, solver="rk4", device=DEV, seed=3, u_rng="kernel", conditioner_rng="kernel",
        nan_check_every=0, fused_ode_training=True, fused_decoder_step=True, fused_step_tail=False)
    model.train()
    cap = {}
    orig_apply, orig_iwae = ops.OdeSolveObserve.apply, ops.iwae_loss

    def apply(spec, theta, cond, times, obs, *rest):
        cap.update(spec=spec, theta=theta.detach().clone(), cond=cond.detach().clone(), times=times.detach().clone(),
                   obs=obs.detach().clone())
        theta.register_hook(lambda g: cap.__setitem__("g_theta", g.detach().clone()))
        return orig_apply(spec, theta, cond, times, obs, *rest)

    def iwae_loss(logp, log_p, log_q, *args, **kw):
        cap.update(log_p=log_p.detach().clone(), log_q=log_q.detach().clone())
        return orig_iwae(logp, log_p, log_q, *args, **kw)

    monkeypatch.setattr(ops.OdeSolveObserve, "apply", apply)
    monkeypatch.setattr(ops, "iwae_loss", iwae_loss)
    # the first step asks for both fused launches (declined on the host, nothing queued) and caches the declines ...
    training.step(training.train_data, zero_grad=True)
    declined = model.decoder.ode_model._fused_declined  # (one cache, keyed by route and shape)
    assert {key[0] for key, value in declined.items() if value is True} == {"DecoderStepFused", "OdeLogLikFused"}
    # ... so the second one does not ask again; it is the step checked against float64
    cap.clear()
    rec = ops.LaunchRecorder()
    ops.TIMER = rec
    try:
        loss = float(training.step(training.train_data, zero_grad=True))
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    assert "decoder_step" not in rec.calls and "ode_logp_grad" not in rec.calls, list(rec.calls)
    assert "ode_fwd" in rec.calls and "ode_bwd" in rec.calls, list(rec.calls)
    spec = cap["spec"]
    assert cap["times"].shape[0] == 135 and not scan_branches(135, 4, 6, "rk4")["supported"]
    rows = [spec.proto.slot_row[q] for q in range(len(spec.slots))]
    res = {}
    for dtype in (torch.float64, torch.float32):
        th = {n: cap["theta"][r].to("cpu", dtype).clone().requires_grad_(True) for n, r in zip(spec.slots, rows)}
        _, xp, prec = O.decode("dr_constant", th, cap["cond"].to("cpu", dtype), cap["times"].to("cpu", dtype), "rk4")
        lpo = O.log_prob_observations(xp, cap["obs"].to("cpu", dtype), prec)
        l, _ = O.iwae_loss(lpo, cap["log_p"].to("cpu", dtype), cap["log_q"].to("cpu", dtype))
        gs = torch.autograd.grad(l, [th[n] for n in spec.slots])
        res[dtype] = (float(l), torch.stack(gs))
    rep = Report("C Training.step dr_constant_icml rk4 T135 B4xS6")
    rep.add("loss", abs(loss - res[torch.float64][0]) / abs(res[torch.float64][0]), TOL)
    g = cap["g_theta"].cpu()[rows]
    rep.per_row("g_theta", g, res[torch.float64][1], res[torch.float32][1], GTOL)
    rep.check()


# ---- D. dr_blackbox: the split forward's staging limit (GPU) ----------------------------------------------------------
BB_ORDER = ("hid_w", "hid_b", "prod_w", "prod_b", "degr_w", "degr_b")


@lru_cache(maxsize=None)
def bb_problem(B, S, T, seed):
    """test_hip_parity._blackbox_problem's inputs on the CPU (ICML sizes: 2 latent species, 25 / 20 hidden units,
    1 760 weights), with the weights also as the oracle's dicts."""
    from vihds import hip

    g = torch.Generator().manual_seed(seed)
    slots = hip.model_slots("dr_blackbox")
    th = {n: (torch.full((B, S), 0.002 if n == "init_x" else 0.0) if n.startswith("init_")
              else torch.randn(B, S, generator=g)) for n in slots}
    C, D, L, HS, HP = 2, 7, 2, 25, 20
    NX, nc = 4 + L, 12 + C + D
    wts = torch.randn(1760, generator=g) * 0.3
    shapes = {"states": [(HS, NX + nc), (HS,), (NX, HS), (NX,), (NX, HS), (NX,)],
              "prec": [(HP, 1 + NX + nc), (HP,), (4, HP), (4,), (4, HP), (4,)]}
    cond = torch.log1p(torch.rand(B, C, generator=g) * 1000.0)
    dev = torch.nn.functional.one_hot(torch.arange(B) % D, D).float()
    times = torch.arange(T, dtype=torch.float32) * 0.1933
    obs = torch.rand(B, 4, T, generator=g)
    return dict(slots=slots, th=th, wts=wts, shapes=shapes, cond=cond, dev=dev, times=times, obs=obs, C=C, D=D,
                n_const=nc)


@lru_cache(maxsize=None)
def bb_reference(B, S, T, seed, solver):
    """float64 / float32: states + precisions [B,S,N,T], x_predict, log-likelihood and the gradients (theta rows, the
    twelve weight tensors) of 1e-2 sum(traj ct0) + 1e-2 sum(xpred ct1) + 1e-3 sum(logp ct2)."""
    bp = bb_problem(B, S, T, seed)
    g = torch.Generator().manual_seed(seed + 7)
    ct = [torch.randn(B, S, 10, T, generator=g), torch.randn(B, S, 4, T, generator=g), torch.randn(B, S, 4, generator=g)]
    out = {}
    for dtype in (torch.float64, torch.float32):
        th = {n: v.to(dtype).clone().requires_grad_(True) for n, v in bp["th"].items()}
        blocks, o = {}, 0
        for net in ("states", "prec"):
            for k, shp in zip(BB_ORDER, bp["shapes"][net]):
                n = int(torch.tensor(shp).prod())
                blocks[(net, k)] = bp["wts"][o: o + n].reshape(shp).to(dtype).clone().requires_grad_(True)
                o += n
        assert o == 1760
        bb = dict(dev_1hot=bp["dev"].to(dtype), states_w={k: blocks[("states", k)] for k in BB_ORDER},
                  prec_w={k: blocks[("prec", k)] for k in BB_ORDER}, n_x=5, n_y=2, n_z=5, n_latent_species=2,
                  init_latent_species=0.001, init_prec=1e-5)
        xs, xp, prec = O.decode("dr_blackbox", th, bp["cond"].to(dtype), bp["times"].to(dtype), solver, blackbox=bb)
        lpo = O.log_prob_observations(xp, bp["obs"].to(dtype), prec)
        full = torch.cat([xs, prec], 2)
        f = 1e-2 * (full * ct[0].to(dtype)).sum() + 1e-2 * (xp * ct[1].to(dtype)).sum() + 1e-3 * (lpo * ct[2].to(dtype)).sum()
        leaves = [th[n] for n in bp["slots"]] + list(blocks.values())
        gs = torch.autograd.grad(f, leaves, allow_unused=True)
        gs = [torch.zeros_like(v) if gv is None else gv for v, gv in zip(leaves, gs)]
        ns = len(bp["slots"])
        out[dtype] = dict(traj=full.detach(), xp=xp.detach(), lpo=lpo.detach(), g_theta=torch.stack(gs[:ns]),
                          g_w=dict(zip(blocks, gs[ns:])))
    return bp, ct, out


BB_CASES = [(B, S, T, solver) for (S, B), (last, first) in BB_TABLE.items() if (S, B) != (1, 5)
            for T in (last, first) for solver in ("midpoint", "rk4")]


def _bb_id(c):
    B, S, T, solver = c
    return "B%d-S%d-T%d-%s-%s" % (B, S, T, solver, "split-fwd" if bb_fwd_branches(B, S, T)["split"] else "valu-fwd")


@gpu
@pytest.mark.parametrize("B,S,T,solver", BB_CASES, ids=[_bb_id(c) for c in BB_CASES])
def test_blackbox_forward_on_both_sides_of_the_staging_limit(B, S, T, solver):
    """kernel_variant 0 at the last T of the split MFMA forward and the first T past its 48 KB staging (then the
    thread-per-trajectory forward runs, followed by the split MFMA adjoint): traj, x_predict, logp, d / d theta and all
    1 760 weight gradients against float64.  Past the limit the forward trajectory is bit-identical to kernel_variant 1's
    (both are launch_ode<BB>) and the forward with the sampling stage in front (vihds_theta_ode_fwd) declines; before it,
    that launch runs."""
    import hip_util as H
    from vihds import ops

    br = bb_fwd_branches(B, S, T)
    bp, ct, ref = bb_reference(B, S, T, 4, solver)
    slots = bp["slots"]
    row_of = {n: k for k, n in enumerate(slots)}
    dev = lambda t: t.to(DEV)  # noqa: E731
    theta0 = torch.stack([bp["th"][n] for n in slots])
    res = {}
    for variant in (0, 1):
        spec = ops.OdeProblemSpec("dr_blackbox", solver, row_of, len(slots), C=bp["C"], D=bp["D"], n_hidden_prec=20,
                                   n_hidden_states=25, n_latent_states=2, n_const=bp["n_const"], init_latent=0.001,
                                   init_prec=1e-5, kernel_variant=variant)
        th = dev(theta0).requires_grad_(True)
        w = dev(bp["wts"]).requires_grad_(True)
        traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, dev(bp["cond"]), dev(bp["times"]), dev(bp["obs"]),
                                                      dev(bp["dev"]), w)
        if variant == 1:
            res[1] = traj.detach().cpu()
            break
        (1e-2 * (H.view_bsnt(traj) * dev(ct[0])).sum() + 1e-2 * (H.view_bsnt(xpred) * dev(ct[1])).sum()
         + 1e-3 * (H.view_bs4(logp) * dev(ct[2])).sum()).backward()
        torch.cuda.synchronize()
        res[0] = (traj.detach().cpu(), xpred.detach().cpu(), logp.detach().cpu(), th.grad.cpu(), w.grad.cpu())
        # the sampling stage in front of the forward: every slot sampled (Normal, the init_ rows constant)
        P = len(slots)
        kinds = [O.CONSTANT if n.startswith("init_") else O.NORMAL for n in slots]
        q_all = torch.cat([theta0[:, :, 0], torch.full((P, B), 2.0)]).contiguous()
        lo, hi = torch.full((P,), -50.0), torch.full((P,), 50.0)
        args = (dev(q_all), torch.tensor(kinds, dtype=torch.int32, device=DEV), dev(torch.zeros(P)), dev(torch.ones(P)),
                dev(lo), dev(hi), dev(torch.zeros(B, S, P)), P, torch.arange(2 * P, dtype=torch.int32, device=DEV), spec,
                dev(bp["cond"]), dev(bp["times"]), dev(bp["obs"]), dev(bp["dev"]), w.detach(), None, None, None)
        if br["split"]:
            with torch.no_grad():
                ops.ThetaOdeFused.apply(*args)
            torch.cuda.synchronize()
        else:
            with pytest.raises(ops.FusedTrainingUnsupported):
                ops.ThetaOdeFused.apply(*args)
    traj, xpred, logp, g_th, g_w = res[0]
    r64, r32 = ref[torch.float64], ref[torch.float32]
    rep = Report("D %s (%d staged rows, %d B)" % (_bb_id((B, S, T, solver)), br["rows"], br["bytes"]))
    rep.per_row("traj", H.view_bsnt(traj).permute(2, 0, 1, 3), r64["traj"].permute(2, 0, 1, 3),
                r32["traj"].permute(2, 0, 1, 3), TOL)
    rep.per_row("xpred", H.view_bsnt(xpred).permute(2, 0, 1, 3), r64["xp"].permute(2, 0, 1, 3),
                r32["xp"].permute(2, 0, 1, 3), TOL)
    rep.per_row("logp", H.view_bs4(logp).permute(2, 0, 1), r64["lpo"].permute(2, 0, 1), r32["lpo"].permute(2, 0, 1), TOL)
    rep.per_row("g_theta", g_th, r64["g_theta"], r32["g_theta"], GTOL)
    o = 0
    for key, blk in r64["g_w"].items():
        n = blk.numel()
        rep.add("g_w", *yardstick(g_w[o: o + n], blk.reshape(-1), r32["g_w"][key].reshape(-1), GTOL), where=key)
        o += n
    assert o == g_w.numel() == 1760
    rep.add("valu-fwd traj != variant 1 bitwise", 0.0 if br["split"] or torch.equal(traj, res[1]) else 1.0, 0.0)
    rep.check()
