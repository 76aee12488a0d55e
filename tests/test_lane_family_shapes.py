"""The white-box ODE kernels behind BASELINE config 5 -- one lane per state (csrc/vihds_relay_lanes.hpp:
relay_lane_fwd_kernel, relay_lane_theta_fwd_kernel, relay_lane_bwd_kernel, relay_lane_wreduce_kernel) and one thread per
trajectory (csrc/vihds_ode_kernels.hpp: launch_fwd_s, launch_bwd_s, pick_block) -- across the shapes that select their code
paths, each against the oracle (oracle/vihds_oracle.py) in float64.

The launchers decide on the host: whether the per-trajectory sigmoid table fits LDS (`sig_tab`), how much LDS a block asks
for (dynamic, next to the kernels' static arrays), whether the sampling stage in front of the forward is accepted, which
family runs (16 384 trajectories), whether the thread-per-trajectory forward stages its inputs (32 KB) and its block size
(2^18 trajectories).  `lane_branches`, `tpt_branches`, `lane_family` and `xcd_block` below restate those choices with the
constants read from the headers; every GPU case asserts through them that it lands on the side it is named for.

Reference: O.decode -> O.log_prob_observations in float64 at the float32 theta the kernels are handed; gradients by
autograd with random upstream gradients on all three outputs (trajectory, x_predict, log-likelihood), cached per
(model, solver, B, S, T, seed) and shared by the kernel variants.  Yardstick: test_config5_parity's -- values within TOL =
1e-4 per species / signal, every theta gradient and every precision-network weight gradient within max(GTOL = 5e-4, 8 x the
float32 oracle's own error against float64) per parameter (_assert_theta_grads, imported, not restated).  Inputs follow
test_hip_parity._relay_problem's recipe (on the CPU, so that the references need no GPU) with dt scaled so that a long grid
spans what config 5's does.  Every GPU case prints its worst error next to its bound.

Cases and the branch each takes:
  A  sig_tab on both sides of its line (forward and adjoint, kernel_variant 0; the same shapes through kernel_variant 1
     against the same reference): relay_constant_precisions B17xS1 (two blocks, sixteen data rows staged in one) at rk4 T 92 |
     93, midpoint and modeulerwhile 121 | 122, euler 144 | 145; B3xS17 (blocks span rows, last block partial) rk4 169 | 170;
     degrader_constant (three treatments, no network), auto_constant_precisions (four species, lanes 8..15 idle, the direct
     observation map) rk4 92 | 93; prpr_constant (no treatment read) midpoint 122.
  B  static + dynamic LDS past 64 KB: relay_constant_precisions rk4 adjoint at B17xS1 T 86 (table), B3xS17 T 160 (table),
     B17xS1 T 170 (no table); forward at B17xS1 T 230.
  C  the block permutation xcd_block at nblk 9 and 18 (nblk % 8 != 0, partial last block, S = 20 / 21): relay_constant and
     degrader_constant_precisions, T 12, midpoint, every trajectory compared.
  D  16 384 | 16 385 trajectories (B128xS128 | B5xS3277), relay_constant_precisions T 3 modeuler: lanes with 1 024 partial
     rows (relay_lane_wreduce_kernel's second pass) | thread-per-trajectory with the dump contracted by vihds_gram_blocks.
  E  thread-per-trajectory (kernel_variant 1): relay_constant_precisions and degrader_constant B36xS1 at T 56 (staged) | 57
     (unstaged forward), rk4 and modeuler; auto_constant T 3 euler at 2^18 - 1 | 2^18 trajectories (64 | 256 threads).
  F  the sampling stage inside the forward launch (vihds_theta_ode_fwd), relay_constant_precisions rk4 B17xS1: accepted at
     T 55 (table) and 106 (no table), declined at 56 and 107; accepted ragged B3xS17 T 40.
  G  forward only without observations (a.obs null, x_predict alone) on the no-table path.
"""
import ctypes
import os
import re
from functools import lru_cache

import pytest
import torch

from fixture_util import Fixture, rel_err
from oracle import vihds_oracle as O
from test_config5_parity import GTOL, KEYS, TOL, _assert_theta_grads
from test_hip_parity import _synthetic_theta
from test_launch_modes import _prior_of

DEV = "cuda:0"
gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vi-hds_amd", "csrc")
F64, F32 = torch.float64, torch.float32
KB = 1024
LANE_STRUCT = {"relay": "RlRelay", "degrader": "RlDegrader", "prpr": "RlPrpr", "auto": "RlAuto"}
FIXED_GRID = ("modeuler", "modeulerwhile", "euler", "midpoint", "rk4")  # VIHDS_SOLVER_MODEULER .. VIHDS_SOLVER_RK4
RELAY_P = "relay_constant_precisions"


# ---- constants and formulas read from the headers ---------------------------------------------------------------------
def _grab(text, pattern, what):
    m = re.search(pattern, text, re.S)
    assert m is not None, "header changed under the mirror: %s (%r)" % (what, pattern)
    return tuple(int(g) for g in m.groups() if g)


@lru_cache(maxsize=None)
def header():
    read = lambda f: open(os.path.join(CSRC, f)).read()  # noqa: E731
    rl, tpt, wave, stage = (read(f) for f in ("vihds_relay_lanes.hpp", "vihds_ode_kernels.hpp", "vihds_wave.hpp",
                                              "vihds_theta_stage.hpp"))
    h = {}
    (h["G"],) = _grab(rl, r"constexpr int RL_G = (\d+);", "RL_G")
    (h["T"],) = _grab(rl, r"constexpr int RL_T = (\d+);", "RL_T")
    _grab(rl, r"constexpr int RL_TR = RL_T / RL_G;()", "RL_TR")
    (h["patch"],) = _grab(rl, r"constexpr int RL_PATCH = (\d+);", "RL_PATCH")
    h["nwrow"] = _grab(rl, r"rl_nwrow\(int nin\) \{ return (\d+) \* nin \+ (\d+); \}", "rl_nwrow")
    (h["nwg"],) = _grab(rl, r"rl_nwg\(int nin\) \{ return (\d+) \* rl_nwrow\(nin\); \}", "rl_nwg")
    h["stages"] = _grab(rl, r"S = SOLVER == VIHDS_SOLVER_EULER \? (\d+) : \(SOLVER == VIHDS_SOLVER_RK4 \? (\d+) : (\d+)\);",
                        "RlTab<SOLVER>::S")
    for fam, st in LANE_STRUCT.items():
        (h["nsp_" + fam],) = _grab(rl, r"struct %s \{[^}]*?static constexpr int NSP = (\d+)," % st, st + "::NSP")
    # static LDS: the forward's patch; the adjoint's patch, tab and wred
    assert len(re.findall(r"__shared__ __attribute__\(\(aligned\(16\)\)\) float patch\[RL_TR\]\[RL_PATCH\];", rl)) == 2, "patch"
    (h["tab"],) = _grab(rl, r"__shared__ float tab\[RL_TR\]\[RL_G\]\[(\d+)\];", "tab extent")
    _grab(rl, r"__shared__ float wred\[PREC \? RL_TR : 1\]\[PREC \? NWG : 1\];()", "wred")
    assert len(re.findall(r"__shared__", rl)) == 6, "the lane kernels declare LDS the mirror does not count"  # (4 static + extern x 2)
    # relay_lanes_launch_s
    (h["nb_pad"],) = _grab(rl, r"const int nb_max = min\(a\.B, \(RL_TR - 1\) / a\.S \+ (\d+)\);", "nb_max")
    (h["sig"],) = _grab(rl, r"lds_in = sizeof\(float\) \* \(\(size_t\)a\.T \+ \(size_t\)nb_max \* (\d+) \* a\.T\);", "lds_in")
    _grab(rl, r"lds_sg = sizeof\(float\) \* \(size_t\)RL_TR \* \(a\.T - 1\) \* RlTab<SOLVER>::S;()", "lds_sg")
    (h["tab_kb"],) = _grab(rl, r"const int sig_tab = lds_in \+ lds_sg <= (\d+) \* 1024 \? 1 : 0;", "sig_tab limit")
    _grab(rl, r"const size_t lds = lds_in \+ \(sig_tab \? lds_sg : 0\);()", "dynamic bytes")
    _grab(rl, r"lds_t = lds \+ sizeof\(float\) \* theta_stage_lds_floats\(nb_max, ts->P, RL_TR\);()", "theta-stage bytes")
    (h["theta_kb"],) = _grab(rl, r"if \(backward \|\| lds_t > (\d+) \* 1024\) return VIHDS_E_UNSUPPORTED;", "theta-stage limit")
    h["theta_fl"] = _grab(stage, r"return \(size_t\)(\d+) \* nb_max \* P \+ \(size_t\)(\d+) \* ntraj \* \(\(P \+ (\d+)\) / (\d+)\);",
                          "theta_stage_lds_floats")
    (h["lane_max_n"],) = _grab(rl, r"return kernel_variant != 1 && n <= (\d+) && solver >= VIHDS_SOLVER_MODEULER && "
                                   r"solver <= VIHDS_SOLVER_RK4 &&\s+n_hidden_prec < 1;", "relay_lanes_applicable")
    h["wred_pass"] = _grab(rl, r"for \(int b0 = 0; b0 < nblocks; b0 \+= (\d+) \* (\d+)\)", "wreduce outer loop")
    # thread per trajectory
    h["pick"] = _grab(tpt, r"inline int pick_block\(int n\) \{ return n >= \(1 << (\d+)\) \? (\d+) : (\d+); \}", "pick_block")
    (h["tpt_pad"],) = _grab(tpt, r"const int nb = min\(a\.B, \(blk - 1\) / a\.S \+ (\d+)\);", "launch_fwd_s: rows")
    (h["tpt_sig"],) = _grab(tpt, r"lds = \(\(size_t\)a\.T \+ \(size_t\)nb \* (\d+) \* a\.T\) \* sizeof\(float\);", "launch_fwd_s: bytes")
    (h["tpt_kb"],) = _grab(tpt, r"if \(lds <= (\d+) \* 1024\)\s+hipLaunchKernelGGL\(\(ode_fwd_kernel<M, SOLVER, true>\)",
                           "launch_fwd_s: staging limit")
    # xcd_block
    (h["nxcd"],) = _grab(wave, r"xcd_block\(int wg, int nblk\) \{\s+constexpr int NXCD = (\d+);", "NXCD")
    _grab(wave, r"const int x = wg % NXCD, local = wg / NXCD;\s+const int q = nblk / NXCD, r = nblk % NXCD;\s+"
                r"return x \* q \+ \(x < r \? x : r\) \+ local;()", "xcd_block")
    return h


# ---- Python mirror of the host-side choices ---------------------------------------------------------------------------
def n_stages(solver):
    euler, rk4, other = header()["stages"]
    return euler if solver == "euler" else (rk4 if solver == "rk4" else other)


def n_species(model):
    return header()["nsp_" + model.split("_")[0]]


def lane_family(n, solver, kernel_variant=0, n_hidden_prec=0):
    """relay_lanes_applicable: True -> one lane per state, False -> one thread per trajectory."""
    return kernel_variant != 1 and n <= header()["lane_max_n"] and solver in FIXED_GRID and n_hidden_prec < 1


def lane_branches(model, solver, B, S, T, backward, theta_P=None):
    """relay_lanes_launch_s's choices.  theta_P: the sampled parameters of the sampling stage in front of the forward
    (vihds_theta_ode_fwd), None for the plain launches.  `accepted`: False -> VIHDS_E_UNSUPPORTED (the sampling stage only; a
    plain launch is never declined).  `static`: the LDS arrays the kernel declares itself, which the launcher does not count;
    `past_64kb`: static + dynamic exceed 64 KB, what a block could have before gfx950 and the line at which
    launch_dr_scan_train opts its kernel in -- the lane launcher does not, and the launch is accepted as it is (measured:
    cases B)."""
    h = header()
    tr = h["T"] // h["G"]
    prec = model.endswith("_precisions")
    nblk = (B * S + tr - 1) // tr
    nb_max = min(B, (tr - 1) // S + h["nb_pad"])
    lds_in = 4 * (T + nb_max * h["sig"] * T)
    lds_sg = 4 * tr * (T - 1) * n_stages(solver)
    sig_tab = lds_in + lds_sg <= h["tab_kb"] * KB
    dynamic = lds_in + (lds_sg if sig_tab else 0)
    nin = 1 + n_species(model)
    nwg = h["nwg"] * (h["nwrow"][0] * nin + h["nwrow"][1])
    static = 4 * tr * h["patch"]
    if backward:
        static += 4 * tr * h["G"] * h["tab"] + 4 * (tr * nwg if prec else 1)
    accepted = True
    if theta_P is not None:
        a, b, c, d = h["theta_fl"]
        dynamic += 4 * (a * nb_max * theta_P + b * tr * ((theta_P + c) // d))
        accepted = not backward and dynamic <= h["theta_kb"] * KB
    total = dynamic + static
    return dict(nblk=nblk, nb_max=nb_max, lds_in=lds_in, lds_sg=lds_sg, sig_tab=sig_tab, dynamic=dynamic, static=static,
                total=total, past_64kb=total > 64 * KB, accepted=accepted,
                wreduce_passes=-(-nblk // (h["wred_pass"][0] * h["wred_pass"][1])) if (backward and prec) else 0)


def tpt_branches(B, S, T):
    """pick_block and launch_fwd_s: threads per block, blocks, the forward's staged bytes and whether it stages at all."""
    h = header()
    shift, big, small = h["pick"]
    n = B * S
    blk = big if n >= (1 << shift) else small
    nb = min(B, (blk - 1) // S + h["tpt_pad"])
    lds = 4 * (T + nb * h["tpt_sig"] * T)
    return dict(block=blk, nblk=(n + blk - 1) // blk, nb=nb, lds=lds, staged=lds <= h["tpt_kb"] * KB)


def xcd_block(wg, nblk):
    """vihds_wave.hpp: hardware workgroup id -> logical block (neighbouring logical blocks on one XCD)."""
    nx = header()["nxcd"]
    x, local = wg % nx, wg // nx
    q, r = nblk // nx, nblk % nx
    return x * q + min(x, r) + local


def _edges(pred, lo, hi):
    """The (last T, first T) pairs at which pred changes over lo..hi."""
    vals = [pred(T) for T in range(lo, hi + 1)]
    return [(lo + k, lo + k + 1) for k in range(len(vals) - 1) if vals[k] != vals[k + 1]]


# (B, S, solver) -> (last T with the sigmoid table, first T without)
SIG_TABLE = {(17, 1, "rk4"): (92, 93), (17, 1, "midpoint"): (121, 122), (17, 1, "modeuler"): (121, 122),
             (17, 1, "modeulerwhile"): (121, 122), (17, 1, "euler"): (144, 145), (40, 1, "rk4"): (92, 93),
             (3, 17, "rk4"): (169, 170), (3, 17, "midpoint"): (300, 301), (3, 17, "euler"): (492, 493),
             (36, 200, "rk4"): (169, 170)}


# ---- CPU: the mirror ---------------------------------------------------------------------------------------------------
def test_header_constants_are_read_and_consistent():
    """Every constant and formula the mirror uses is found in the headers (a changed header fails here, not silently in the
    GPU cases' labels), and the pieces fit each other."""
    h = header()
    assert h["T"] % h["G"] == 0 and h["T"] // h["G"] == 16 and h["G"] == 16 and h["patch"] == 3 * h["G"]
    assert [n_stages(s) for s in ("euler", "modeuler", "modeulerwhile", "midpoint", "rk4")] == [1, 2, 2, 2, 4]
    assert [n_species(m) for m in ("relay_constant", "degrader_constant", "prpr_constant", "auto_constant")] == [12, 11, 6, 4]
    assert h["tpt_kb"] < h["tab_kb"] < h["theta_kb"] < 64
    assert h["lane_max_n"] == 16384 and h["pick"] == (18, 256, 64) and h["nxcd"] == 8
    # relay: 112 weight-gradient numbers per block row; static LDS of the adjoint 3 072 + 10 240 + 7 168 bytes
    br = lane_branches(RELAY_P, "rk4", 17, 1, 50, True)
    assert br["static"] == 3072 + 10240 + 7168 == 20480 and lane_branches(RELAY_P, "rk4", 17, 1, 50, False)["static"] == 3072
    assert lane_branches("relay_constant", "rk4", 17, 1, 50, True)["static"] == 3072 + 10240 + 4


def test_sigmoid_table_boundaries_come_out_of_the_mirror():
    """Item 1: per (B, S, solver) the one T at which relay_lanes_launch_s drops the sigmoid table, forward and adjoint alike;
    nb_max is 17 from B = 17 on at S = 1 and 2 from S = 15 on."""
    for (B, S, solver), pair in SIG_TABLE.items():
        for backward in (False, True):
            edges = _edges(lambda T: lane_branches(RELAY_P, solver, B, S, T, backward)["sig_tab"], 2, 600)
            assert edges == [pair], (B, S, solver, edges)
    assert lane_branches(RELAY_P, "rk4", 17, 1, 92, True)["nb_max"] == 17 == lane_branches(RELAY_P, "rk4", 99, 1, 92, True)["nb_max"]
    assert [lane_branches(RELAY_P, "rk4", 36, S, 99, True)["nb_max"] for S in (14, 15, 16, 17, 200)] == [3, 3, 2, 2, 2]
    # (the issue's "nb_max = 2 (S >= 15)": at S = 15 a block of sixteen can touch three rows -- 15 / 15 + 2 -- and nb_max is 3;
    # it is 2 from S = 16 on.  The cases below use S = 17.)
    # a relay model evaluated at S = 1 on a 99-point grid with rk4 already runs without the table
    assert not lane_branches(RELAY_P, "rk4", 36, 1, 99, False)["sig_tab"]


def test_total_lds_zones_past_64_kb_come_out_of_the_mirror():
    """Item 2: where dynamic + static LDS of a relay_constant_precisions rk4 launch passes 64 KB: the table's last lengths,
    and on the no-table path -- where lds_in has no upper check -- every length from 164 (adjoint) / 227 (forward) on."""
    over = lambda B, S, backward: [T for T in range(2, 601)  # noqa: E731
                                   if lane_branches(RELAY_P, "rk4", B, S, T, backward)["past_64kb"]]
    assert over(3, 17, True) == list(range(156, 170))  # (the table's last fourteen lengths; without it 36 T bytes: not below T 601)
    z = over(17, 1, True)
    assert [T for T in z if T <= 92] == list(range(86, 93)) and [T for T in z if T > 92][0] == 164  # (86: the plate's grid)
    assert over(17, 1, False)[0] == 227
    for B, S, T, backward in B_CASES:
        br = lane_branches(RELAY_P, "rk4", B, S, T, backward)
        assert br["past_64kb"] and br["accepted"], (B, S, T)
    assert lane_branches(RELAY_P, "rk4", 17, 1, 230, False)["lds_in"] == 276 * 230  # (no-table path, B >= 17, S = 1: 276 T bytes)


def test_config5_shape_keeps_its_branch():
    """BASELINE config 5 (relay_constant_precisions, 36 x 200 x 99, midpoint): the table in LDS, 16 108 dynamic bytes, 450
    blocks, under 64 KB in all -- forward and adjoint.  The benchmarked shape must not move to another branch."""
    for backward in (False, True):
        br = lane_branches(RELAY_P, "midpoint", 36, 200, 99, backward)
        assert br["sig_tab"] and br["dynamic"] == 16108 and br["nblk"] == 450 and br["nb_max"] == 2
        assert br["accepted"] and not br["past_64kb"] and br["total"] == 16108 + (20480 if backward else 3072)
    assert lane_family(7200, "midpoint") and lane_branches(RELAY_P, "midpoint", 36, 200, 99, True)["wreduce_passes"] == 1


def test_family_and_block_size_lines_come_out_of_the_mirror():
    """Items 4 and 5: lanes up to 16 384 trajectories; the weight reduction's second pass above 512 blocks = 8 192
    trajectories; the unstaged thread-per-trajectory forward from T = 57 at B36xS1; 256 threads from 2^18 trajectories."""
    assert _edges(lambda n: lane_family(n, "modeuler"), 16000, 17000) == [(16384, 16385)]
    assert not lane_family(100, "modeuler", kernel_variant=1) and not lane_family(100, "dopri5")
    assert not lane_family(100, "rk4", n_hidden_prec=5)
    assert _edges(lambda n: lane_branches(RELAY_P, "modeuler", n, 1, 3, True)["wreduce_passes"], 8000, 16384) == [(8192, 8193)]
    assert lane_branches(RELAY_P, "modeuler", 128, 128, 3, True)["wreduce_passes"] == 2
    assert _edges(lambda T: tpt_branches(36, 1, T)["staged"], 2, 300) == [(56, 57)]
    assert _edges(lambda n: tpt_branches(1, n, 3)["block"], (1 << 18) - 100, (1 << 18) + 100) == [((1 << 18) - 1, 1 << 18)]
    assert tpt_branches(1, (1 << 18) - 1, 3)["nblk"] == 4096 and tpt_branches(64, 4096, 3)["nblk"] == 1024


def test_sampling_stage_accept_line_is_not_monotonic_in_the_mirror():
    """Item 6: relay (P = 45), B >= 17, S = 1, rk4: accepted up to T 55, declined 56..92 (table plus stage scratch),
    accepted again 93..106 (no table), declined from 107."""
    from vihds import hip

    P = len(hip.model_slots(RELAY_P))
    assert P == 45
    acc = lambda T: lane_branches(RELAY_P, "rk4", 17, 1, T, False, theta_P=P)["accepted"]  # noqa: E731
    assert _edges(acc, 2, 400) == [(55, 56), (92, 93), (106, 107)] and acc(2)
    assert not lane_branches(RELAY_P, "rk4", 17, 1, 40, True, theta_P=P)["accepted"]  # (no sampling stage in an adjoint)
    for B, S, T, accepted in F_CASES:
        assert lane_branches(RELAY_P, "rk4", B, S, T, False, theta_P=P)["accepted"] == accepted


def test_xcd_block_is_a_permutation():
    """Item 3: for every nblk in 1..64 and 449..451 the block map is a bijection of range(nblk), and consecutive hardware
    ids (one per XCD in turn) land in eight contiguous runs."""
    for nblk in list(range(1, 65)) + [449, 450, 451, 1024, 1025]:
        image = [xcd_block(wg, nblk) for wg in range(nblk)]
        assert sorted(image) == list(range(nblk)), nblk
        for x in range(min(8, nblk)):
            run = image[x::8]
            assert run == list(range(run[0], run[0] + len(run))), (nblk, x)


# ---- problems and float64 references ----------------------------------------------------------------------------------
SPAN = 99 * 0.17  # config 5's grid: 99 points, dt 0.17 (test_relay_lane_kernels_at_config5_size)


@lru_cache(maxsize=None)
def problem(model, B, S, T, seed):
    """test_hip_parity._relay_problem's inputs on the CPU (float32): synthetic theta in the model's slot order, treatments over
    five magnitudes, an uneven grid (modeuler's fixed h and the per-step h differ) with dt = min(0.25, SPAN / T), observations,
    the precision network's weights."""
    from vihds import hip

    slots = hip.model_slots(model)
    th = _synthetic_theta(slots, B, S, seed)
    for n in slots:
        if n.startswith("init_prec"):
            th[n] = torch.exp(3.0 + 0.3 * torch.randn(B, S, generator=torch.Generator().manual_seed(9)))
    g = torch.Generator().manual_seed(seed + 1)
    C = 3 if model.startswith("degrader") else 2
    cond = torch.log1p(torch.tensor([0.0, 5.0, 250.0, 5000.0, 25000.0])[torch.arange(B) % 5][:, None].repeat(1, C) *
                       torch.rand(B, C, generator=g))
    dt = min(0.25, SPAN / T)
    times = torch.arange(T, dtype=torch.float32) * dt + 0.12 * dt * torch.rand(T, generator=g).cumsum(0)
    obs = torch.rand(B, 4, T, generator=g)
    wts = None
    if model.endswith("_precisions"):
        wts = torch.randn(2 * (4 * (1 + n_species(model)) + 4), generator=g) * 0.2
    N = n_species(model) + (4 if wts is not None else 0)
    gu = torch.Generator().manual_seed(seed + 2)
    up = (torch.randn(T, N, B, S, generator=gu) * 1e-3, torch.randn(T, 4, B, S, generator=gu) * 1e-3,
          torch.randn(4, B, S, generator=gu) * 1e-3)  # upstream gradients: non-zero on every trajectory
    return dict(model=model, slots=slots, theta=torch.stack([th[n] for n in slots]), cond=cond, times=times, obs=obs, wts=wts,
                up=up, B=B, S=S, T=T, N=N)


def _split_weights(model, wts, dtype):
    n_in = 1 + n_species(model)
    parts = torch.split(wts, [4 * n_in, 4, 4 * n_in, 4])
    shapes = [(4, n_in), (4,), (4, n_in), (4,)]
    return {k: p.reshape(s).to(dtype).clone().requires_grad_(True) for k, p, s in zip(KEYS, parts, shapes)}


def _oracle(pr, solver, dtype, theta=None, with_grads=True):
    """The oracle in `dtype`: [B,S,N,T] trajectory (precision states behind the species), [B,S,4,T] x_predict, [B,S,4]
    log-likelihood; gradients of sum(traj up0 + x_predict up1 + logp up2) per slot and per weight tensor."""
    model = pr["model"]
    theta = pr["theta"] if theta is None else theta
    leaves = [theta[i].to(dtype).clone().requires_grad_(with_grads) for i in range(len(pr["slots"]))]
    w = _split_weights(model, pr["wts"], dtype) if pr["wts"] is not None else None
    with torch.set_grad_enabled(with_grads):
        xs, xp, prec = O.decode(model, dict(zip(pr["slots"], leaves)), pr["cond"].to(dtype), pr["times"].to(dtype), solver,
                                prec_w=w)
        lpo = O.log_prob_observations(xp, pr["obs"].to(dtype), prec)
        traj = torch.cat([xs, prec], 2) if w is not None else xs
        out = dict(traj=traj.detach(), xp=xp.detach(), lpo=lpo.detach())
        if with_grads:
            u0, u1, u2 = (u.to(dtype) for u in pr["up"])
            loss = (traj * u0.permute(2, 3, 1, 0)).sum() + (xp * u1.permute(2, 3, 1, 0)).sum() + (lpo * u2.permute(1, 2, 0)).sum()
            wl = [w[k] for k in KEYS] if w is not None else []
            gr = torch.autograd.grad(loss, leaves + wl, allow_unused=True)
            zero = torch.zeros(pr["B"], pr["S"], dtype=dtype)
            out["th"] = [zero if g_ is None else g_ for g_ in gr[: len(leaves)]]
            out["w"] = [g_.reshape(-1) for g_ in gr[len(leaves):]]
    return out


@lru_cache(maxsize=None)
def reference(model, solver, B, S, T, seed):
    pr = problem(model, B, S, T, seed)
    return pr, {dtype: _oracle(pr, solver, dtype) for dtype in (F64, F32)}


def _worst(names, got, r32, r64):
    """(name, error, bound) of the parameter nearest to (or furthest past) the yardstick -- for the printed line only; the
    assertion is _assert_theta_grads'."""
    worst = ("-", 0.0, GTOL)
    for n, g, a, b in zip(names, got, r32, r64):
        scale = float(b.abs().max())
        if scale == 0.0:
            continue
        e32 = float((a.double() - b).abs().max()) / scale
        e = float((g.double() - b).abs().max()) / scale
        bound = max(GTOL, 8.0 * e32)
        if e / bound >= worst[1] / worst[2]:
            worst = (n, e, bound)
    return worst


def _hip(pr, solver, variant, backward=True):
    """The kernels through ops.OdeSolveObserve (every launch through hip.check): outputs as the oracle lays them out."""
    from vihds import ops

    slots = pr["slots"]
    th = pr["theta"].to(DEV).requires_grad_(backward)
    w = pr["wts"].to(DEV).requires_grad_(backward) if pr["wts"] is not None else None
    spec = ops.OdeProblemSpec(pr["model"], solver, {n: i for i, n in enumerate(slots)}, len(slots), C=pr["cond"].shape[1],
                              kernel_variant=variant)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, pr["cond"].to(DEV), pr["times"].to(DEV), pr["obs"].to(DEV), None, w)
    out = dict(traj=traj.detach().permute(2, 3, 1, 0).cpu(), xp=xpred.detach().permute(2, 3, 1, 0).cpu(),
               lpo=logp.detach().permute(1, 2, 0).cpu())
    if backward:
        u0, u1, u2 = (u.to(DEV) for u in pr["up"])
        ((traj * u0).sum() + (xpred * u1).sum() + (logp * u2).sum()).backward()
        out["th"] = list(th.grad.cpu())
        if w is not None:
            n_in = 1 + n_species(pr["model"])
            out["w"] = list(torch.split(w.grad.cpu(), [4 * n_in, 4, 4 * n_in, 4]))
    torch.cuda.synchronize()
    return out


def _check(label, out, pr, ref):
    """Print the worst errors next to their bounds, then assert the yardstick."""
    r64, r32 = ref[F64], ref[F32]
    vals = {"traj": rel_err(out["traj"], r64["traj"]), "xp": rel_err(out["xp"], r64["xp"]),
            "logp": rel_err(out["lpo"], r64["lpo"], dim=2)}
    line = "%-62s " % label + "  ".join("%s %.1e (%.0e)" % (k, v, TOL) for k, v in vals.items())
    if "th" in out:
        line += "  theta-grad %s %.1e (%.1e)" % _worst(pr["slots"], out["th"], r32["th"], r64["th"])
    if "w" in out:
        line += "  weight-grad %s %.1e (%.1e)" % _worst(KEYS, out["w"], r32["w"], r64["w"])
    print(line)
    assert all(torch.isfinite(out[k]).all() for k in ("traj", "xp", "lpo"))
    assert all(v < TOL for v in vals.values()), vals
    if "th" in out:
        _assert_theta_grads(pr["slots"], out["th"], r32["th"], r64["th"], pr["B"], pr["S"])
    if "w" in out:
        _assert_theta_grads(KEYS, out["w"], r32["w"], r64["w"], pr["B"], pr["S"])


# ---- the cases ---------------------------------------------------------------------------------------------------------
SEED = 21
# A: (model, solver, B, S, T, sigmoid table in LDS)
A_CASES = ([(RELAY_P, s, 17, 1, T, T == last) for s, last in (("rk4", 92), ("midpoint", 121), ("modeulerwhile", 121),
                                                                ("euler", 144)) for T in (last, last + 1)]
           + [(RELAY_P, "rk4", 3, 17, 169, True), (RELAY_P, "rk4", 3, 17, 170, False)]
           + [(m, "rk4", 17, 1, T, T == 92) for m in ("degrader_constant", "auto_constant_precisions") for T in (92, 93)]
           + [("prpr_constant", "midpoint", 17, 1, 122, False)])
# B: (B, S, T, adjoint) of relay_constant_precisions, rk4: total LDS past 64 KB
B_CASES = [(17, 1, 86, True), (3, 17, 160, True), (17, 1, 170, True), (17, 1, 230, False)]
# C: (model, B, S): nblk 9 and 18
C_CASES = [(m, B, S) for m in ("relay_constant", "degrader_constant_precisions") for B, S in ((7, 20), (13, 21))]
# D: (B, S, lanes)
D_CASES = [(128, 128, True), (5, 3277, False)]
# E: thread per trajectory
E_CASES = [(m, s, 36, 1, T) for m in (RELAY_P, "degrader_constant") for s in ("rk4", "modeuler") for T in (56, 57)]
E_BIG = [(1, (1 << 18) - 1, 64), (64, 4096, 256)]
# F: (B, S, T, accepted) of the sampling stage, relay_constant_precisions, rk4
F_CASES = [(17, 1, 55, True), (17, 1, 106, True), (17, 1, 56, False), (17, 1, 107, False), (3, 17, 40, True)]

REFERENCES = sorted(set(
    [(m, s, B, S, T) for m, s, B, S, T, _ in A_CASES] + [(RELAY_P, "rk4", B, S, T) for B, S, T, _ in B_CASES]
    + [(m, "midpoint", B, S, 12) for m, B, S in C_CASES] + [(RELAY_P, "modeuler", B, S, 3) for B, S, _ in D_CASES]
    + E_CASES + [("auto_constant", "euler", B, S, 3) for B, S, _ in E_BIG]))


def _id(case):
    return "-".join(str(v) for v in case)


# ---- 0. the oracle against its own float32 run (CPU) ------------------------------------------------------------------
@pytest.mark.parametrize("case", REFERENCES, ids=_id)
def test_float64_reference_agrees_with_its_float32_run(case):
    """On every case's inputs the oracle's float32 and float64 runs are finite and agree to float32 accuracy -- values to
    1e-5 per species / signal, every gradient to GTOL of its float64 maximum (degrader's nA: see below) -- so the yardstick measures float32
    conditioning on a well-posed problem, not a runaway trajectory on the longer grids or a bug in the reference."""
    pr, ref = reference(*case, SEED)
    r64, r32 = ref[F64], ref[F32]
    for k in ("traj", "xp", "lpo"):
        assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), k
    assert rel_err(r32["traj"], r64["traj"]) < 1e-5 and rel_err(r32["xp"], r64["xp"]) < 1e-5
    assert rel_err(r32["lpo"], r64["lpo"], dim=2) < 1e-5
    names = list(pr["slots"]) + (list(KEYS) if pr["wts"] is not None else [])
    worst = _worst(names, r32["th"] + r32["w"], r64["th"] + r64["w"], r64["th"] + r64["w"])
    print("%-50s float32 oracle: worst gradient %s %.1e" % (_id(case), worst[0], worst[1]))
    for n, a, b in zip(names, r32["th"] + r32["w"], r64["th"] + r64["w"]):
        scale = float(b.abs().max())
        # (degrader's arabinose Hill exponent nA: d PBAD / d nA is the difference of the numerator's and the denominator's
        # derivative, two nearly equal terms, and float32 loses the digits they share -- 1e-2, the bound
        # test_relay_lane_kernels_match_thread_per_trajectory documents for the same parameter.  This loosens the self-check
        # alone: the kernels' bound for nA is the yardstick's, 8 x this very error.)
        bound = 1e-2 if (case[0].startswith("degrader") and n == "nA") else GTOL
        assert torch.isfinite(b).all() and (scale == 0.0 or float((a.double() - b).abs().max()) / scale < bound), n


def test_sampling_stage_inputs_stay_finite_and_resolved():
    """The accepted cases of F on the CPU: theta = clip(sample(q, u)) from the tables below (O.sample_clip_theta) integrates
    to finite values over the whole grid, float32 within 1e-5 of float64."""
    for B, S, T, accepted in F_CASES:
        if not accepted:
            continue
        pr, tab = problem(RELAY_P, B, S, T, SEED), _tables(B, S, 5)
        P, kinds = tab["P"], [int(k) for k in tab["kind"]]
        col = lambda t: [t[p][:, None].double() for p in range(P)]  # noqa: E731
        th = O.sample_clip_theta(pr["slots"], kinds, col(tab["q_mu"]), col(tab["q_prec"]), list(tab["p_mu"].double()),
                                 list(tab["p_prec"].double()), tab["u"].double())
        theta = torch.stack([th[n].expand(B, S) for n in pr["slots"]]).float()
        r64, r32 = (_oracle(pr, "rk4", dt, theta=theta, with_grads=False) for dt in (F64, F32))
        assert all(torch.isfinite(v).all() for v in r64.values())
        assert rel_err(r32["traj"], r64["traj"]) < 1e-5 and rel_err(r32["lpo"], r64["lpo"], dim=2) < 1e-5


# ---- A. the sigmoid table on both sides of its line --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", A_CASES, ids=_id)
def test_sigmoid_table_switch_forward_and_adjoint(case, variant):
    """Item 1.  kernel_variant 0: the lane kernels with the table in LDS | with the stage sigmoids evaluated in place (another
    LDS layout in forward and adjoint); kernel_variant 1: the same shape on the thread-per-trajectory kernels, same reference."""
    model, solver, B, S, T, table = case
    for backward in (False, True):
        br = lane_branches(model, solver, B, S, T, backward)
        assert br["sig_tab"] == table and br["accepted"] and br["nblk"] == (2 if S == 1 else 4)
    assert lane_family(B * S, solver, variant) == (variant == 0)
    pr, ref = reference(model, solver, B, S, T, SEED)
    _check("A %s v%d table %d" % (_id(case[:5]), variant, table), _hip(pr, solver, variant), pr, ref)


# ---- B. static + dynamic LDS past 64 KB ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", B_CASES, ids=_id)
def test_total_lds_past_64_kb_launches(case):
    """Item 2.  The adjoint's static arrays (patch, tab, wred: 20 480 bytes for relay_constant_precisions) come on top of the
    dynamic block the launcher sizes; these four shapes ask for more than 64 KB in all (forward: T 230), and the launcher
    never opts the kernel in to more.  Each must return VIHDS_OK (hip.check inside ops.OdeSolveObserve raises otherwise) and
    meet the yardstick on the lane kernels.  Measured on an MI355X: none is refused -- a gfx950 block may have up to 160 KB
    and the runtime asks for no opt-in below that -- so the launcher stands as it is."""
    B, S, T, adjoint = case
    br = lane_branches(RELAY_P, "rk4", B, S, T, adjoint)
    assert br["past_64kb"] and br["accepted"] and lane_family(B * S, "rk4")
    pr, ref = reference(RELAY_P, "rk4", B, S, T, SEED)
    out = _hip(pr, "rk4", 0, backward=adjoint)
    _check("B %s %s total LDS %d B, table %d" % (_id(case[:3]), "adjoint" if adjoint else "forward", br["total"], br["sig_tab"]),
           out, pr, ref)


# ---- C. the block permutation -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", C_CASES, ids=_id)
def test_block_map_covers_every_trajectory(case):
    """Item 3.  nblk 9 and 18: more blocks than XCDs, nblk % 8 != 0, a partial last block, S neither dividing nor divided by
    16.  Every trajectory's outputs and gradients are compared: a block map that is no bijection leaves some unwritten."""
    model, B, S = case
    br = lane_branches(model, "midpoint", B, S, 12, True)
    assert br["nblk"] == {140: 9, 273: 18}[B * S] and br["nblk"] % 8 != 0 and (B * S) % 16 != 0 and S % 16 != 0 and 16 % S != 0
    pr, ref = reference(model, "midpoint", B, S, 12, SEED)
    _check("C %s nblk %d" % (_id(case), br["nblk"]), _hip(pr, "midpoint", 0), pr, ref)


# ---- D. 16 384 | 16 385 trajectories ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", D_CASES, ids=_id)
def test_family_choice_at_16384_trajectories(case):
    """Item 4.  At 16 384 trajectories the lane kernels run and leave 1 024 partial weight-gradient rows that
    relay_lane_wreduce_kernel adds up in two passes; at 16 385 the thread-per-trajectory adjoint dumps [fields][E][n] and the
    caller contracts it (vihds_gram_blocks).  Upstream gradients are non-zero on every trajectory; the oracle runs them all."""
    from vihds import hip, ops

    B, S, lanes = case
    T, solver = 3, "modeuler"
    pr, ref = reference(RELAY_P, solver, B, S, T, SEED)
    spec = ops.OdeProblemSpec(RELAY_P, solver, {n: i for i, n in enumerate(pr["slots"])}, len(pr["slots"]), C=2)
    pp = ctypes.byref(spec.bind(B, S, T))
    L = hip.lib()
    assert lane_family(B * S, solver) == lanes and bool(L.vihds_ode_bwd_reduces_weights(pp)) == lanes
    br = lane_branches(RELAY_P, solver, B, S, T, True)
    n_fields = 8 + 1 + n_species(RELAY_P)  # the dump: eight pre-activation adjoints and the network's inputs
    want_aux = br["nblk"] * 112 if lanes else n_fields * (T - 1) * n_stages(solver) * B * S
    assert int(L.vihds_ode_bwd_aux_floats(pp)) == want_aux
    assert br["nblk"] == (1024 if lanes else 1025) and (br["wreduce_passes"] == 2 or not lanes)
    _check("D %s n %d %s" % (_id(case[:2]), B * S, "lanes" if lanes else "thread per trajectory"), _hip(pr, solver, 0), pr, ref)


# ---- E. thread per trajectory ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", E_CASES, ids=_id)
def test_thread_per_trajectory_staged_and_unstaged_forward(case):
    """Item 5.  kernel_variant 1 at B36xS1: T 56 stages the time grid and the 36 observation rows in LDS (32 480 bytes), T 57
    does not (ode_fwd_kernel<..., LDS_IN = false>, which had only ever run for dr_constant)."""
    model, solver, B, S, T = case
    assert tpt_branches(B, S, T)["staged"] == (T == 56) and not lane_family(B * S, solver, 1)
    pr, ref = reference(model, solver, B, S, T, SEED)
    _check("E %s staged %d" % (_id(case), T == 56), _hip(pr, solver, 1), pr, ref)


@gpu
@pytest.mark.parametrize("case", E_BIG, ids=_id)
def test_thread_per_trajectory_block_size_at_2_to_the_18(case):
    """Item 5.  pick_block: 64 threads below 2^18 trajectories, 256 from there on (auto_constant, T 3, euler); the oracle on
    all trajectories."""
    B, S, block = case
    assert tpt_branches(B, S, 3)["block"] == block and not lane_family(B * S, "euler")
    pr, ref = reference("auto_constant", "euler", B, S, 3, SEED)
    _check("E auto_constant %s block %d" % (_id(case[:2]), block), _hip(pr, "euler", 0), pr, ref)


# ---- F. the sampling stage inside the forward launch ---------------------------------------------------------------------
SENTINEL = -777.0


@lru_cache(maxsize=None)
def _tables(B, S, seed):
    """q and p tables of relay_constant_precisions' 45 parameters (test_launch_modes' priors; q a quarter as wide as p around
    a jittered mean, constants at their values), clip bounds and host draws."""
    import hip_util as H
    from vihds import hip

    slots = hip.model_slots(RELAY_P)
    fx = Fixture("relay_constant_precisions_tiny_modeuler")
    rows = [_prior_of(fx, n) for n in slots]
    g = torch.Generator().manual_seed(seed)
    P = len(slots)
    p_mu, p_prec = torch.tensor([r[1] for r in rows]), torch.tensor([r[2] for r in rows])
    lo, hi = H.clip_bounds([r[0] for r in rows], p_mu, p_prec, 4.0)
    sampled = torch.tensor([r[0] != O.CONSTANT for r in rows])[:, None]  # (a constant's value is its q_mu: the initial states)
    q_mu = p_mu[:, None] + sampled * 0.1 * torch.randn(P, B, generator=g) / p_prec.sqrt()[:, None]
    q_prec = 16.0 * p_prec[:, None] * torch.exp(0.1 * torch.randn(P, B, generator=g))
    return dict(P=P, kind=torch.tensor([r[0] for r in rows], dtype=torch.int32), p_mu=p_mu, p_prec=p_prec, lo=lo, hi=hi,
                q_mu=q_mu.contiguous(), q_prec=q_prec.contiguous(), u=torch.randn(B, S, P, generator=g))


def _sampling_launches(pr, tab, fused, rng_seed):
    """vihds_theta_ode_fwd (fused) or vihds_theta_fwd + vihds_ode_fwd on the same tables; outputs pre-filled with SENTINEL.
    rng_seed None: the host's u; else the in-kernel generator from a fresh state of that seed (u is then an output)."""
    from vihds import hip, ops

    L = hip.lib()
    B, S, T, P, N = pr["B"], pr["S"], pr["T"], tab["P"], pr["N"]
    d = {k: v.to(DEV) for k, v in tab.items() if k != "P"}
    cond, times, obs, w = (pr[k].to(DEV) for k in ("cond", "times", "obs", "wts"))
    fill = lambda *shape: torch.full(shape, SENTINEL, device=DEV)  # noqa: E731
    o = dict(theta=fill(P, B, S), log_q=fill(B, S), log_p=fill(B, S), traj=fill(T, N, B, S), xp=fill(T, 4, B, S), lpo=fill(4, B, S))
    opts = None
    if rng_seed is None:
        u = d["u"].clone()
    else:
        u = o["u"] = fill(B, S, P)
        state = ops.KernelNormal.new_state(rng_seed, DEV)
        opts = ctypes.byref(hip.ThetaOpts(None, 0, state.data_ptr(), S, 0, None, None))  # (S_total = S: vihds_theta_fwd asks for it)
    spec = ops.OdeProblemSpec(RELAY_P, "rk4", {n: i for i, n in enumerate(pr["slots"])}, P, C=2)
    pp = ctypes.byref(spec.bind(B, S, T))
    st = hip.current_stream()
    head = (hip.ptr(d["kind"]), hip.ptr(d["q_mu"]), hip.ptr(d["q_prec"]), hip.ptr(d["p_mu"]), hip.ptr(d["p_prec"]),
            hip.ptr(d["lo"]), hip.ptr(d["hi"]), hip.ptr(u))
    if fused:
        rc = int(L.vihds_theta_ode_fwd(pp, P, *head, opts, None, hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), hip.ptr(w),
                                       hip.ptr(o["theta"]), hip.ptr(o["log_q"]), hip.ptr(o["log_p"]), hip.ptr(o["traj"]),
                                       hip.ptr(o["xp"]), hip.ptr(o["lpo"]), st))
    else:
        rc = int(L.vihds_theta_fwd(P, B, S, *head, hip.ptr(o["theta"]), hip.ptr(o["log_q"]), hip.ptr(o["log_p"]), opts, st))
        hip.check(rc, "vihds_theta_fwd")
        rc = int(L.vihds_ode_fwd(pp, hip.ptr(o["theta"]), hip.ptr(cond), None, hip.ptr(times), hip.ptr(obs), hip.ptr(w),
                                 hip.ptr(o["traj"]), hip.ptr(o["xp"]), hip.ptr(o["lpo"]), st))
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in o.items()}


@gpu
@pytest.mark.parametrize("case", F_CASES, ids=_id)
def test_sampling_stage_in_front_of_the_lane_forward(case):
    """Item 6.  Accepted (with the table, without it, ragged): theta, u, log q, log p and the ODE outputs equal the separate
    vihds_theta_fwd + vihds_ode_fwd launches' on the same draws -- the host's u and the in-kernel generator -- and the ODE
    outputs meet the float64 oracle at the sampled theta.  Declined: VIHDS_E_UNSUPPORTED and no output buffer touched.
    Fused against separate is float32 against float32 of the same formulas: a few units in the last place for theta and u
    (1e-6), 1e-5 for the 45-term sums log q / log p and for the ODE outputs (the bound of the lane kernels against the
    thread-per-trajectory ones)."""
    from vihds import hip

    B, S, T, accepted = case
    pr = problem(RELAY_P, B, S, T, SEED)
    tab = _tables(B, S, 5)
    br = lane_branches(RELAY_P, "rk4", B, S, T, False, theta_P=tab["P"])
    assert br["accepted"] == accepted and br["sig_tab"] == (T < 93) and (not accepted or not br["past_64kb"])
    for rng_seed in (None, 0x5EED5EED1234):
        rc, got = _sampling_launches(pr, tab, True, rng_seed)
        if not accepted:
            assert rc == hip.E_UNSUPPORTED, (rc, hip.lib().vihds_last_error().decode())
            assert all(bool((v == SENTINEL).all()) for v in got.values()), [k for k, v in got.items() if not (v == SENTINEL).all()]
            print("F %s declined (%d), %d output buffers untouched" % (_id(case[:3]), rc, len(got)))
            continue
        hip.check(rc, "vihds_theta_ode_fwd")
        rc2, sep = _sampling_launches(pr, tab, False, rng_seed)
        hip.check(rc2, "vihds_ode_fwd")
        errs = {k: rel_err(got[k], sep[k], **({"dim": 0} if k == "theta" else {})) for k in got}
        print("F %s %s  fused against separate: %s" % (_id(case[:3]), "host u" if rng_seed is None else "in-kernel generator",
                                                       "  ".join("%s %.1e" % kv for kv in sorted(errs.items()))))
        assert all(torch.isfinite(v).all() and not bool((v == SENTINEL).any()) for v in got.values())
        assert errs["theta"] < 1e-6 and errs.get("u", 0.0) < 1e-6
        assert all(errs[k] < 1e-5 for k in ("log_q", "log_p", "traj", "xp", "lpo")), errs
        r64 = _oracle(pr, "rk4", F64, theta=got["theta"], with_grads=False)
        vals = {"traj": rel_err(got["traj"].permute(2, 3, 1, 0), r64["traj"]), "xp": rel_err(got["xp"].permute(2, 3, 1, 0), r64["xp"]),
                "logp": rel_err(got["lpo"].permute(1, 2, 0), r64["lpo"], dim=2)}
        print("F %s against the float64 oracle at the sampled theta: %s" % (
            _id(case[:3]), "  ".join("%s %.1e (%.0e)" % (k, v, TOL) for k, v in vals.items())))
        assert all(v < TOL for v in vals.values()), vals


# ---- G. forward without observations ------------------------------------------------------------------------------------
@gpu
def test_forward_without_observations_on_the_no_table_path():
    """a.obs null and no log-likelihood requested: obs_on comes from x_predict alone and the observation rows are not staged
    (relay_constant_precisions B17xS1 T 93 rk4: no sigmoid table)."""
    from vihds import hip, ops

    B, S, T = 17, 1, 93
    assert not lane_branches(RELAY_P, "rk4", B, S, T, False)["sig_tab"]
    pr, ref = reference(RELAY_P, "rk4", B, S, T, SEED)
    spec = ops.OdeProblemSpec(RELAY_P, "rk4", {n: i for i, n in enumerate(pr["slots"])}, len(pr["slots"]), C=2)
    theta, cond, times, w = (pr[k].to(DEV) for k in ("theta", "cond", "times", "wts"))
    traj, xp = torch.full((T, pr["N"], B, S), SENTINEL, device=DEV), torch.full((T, 4, B, S), SENTINEL, device=DEV)
    hip.check(hip.lib().vihds_ode_fwd(ctypes.byref(spec.bind(B, S, T)), hip.ptr(theta), hip.ptr(cond), None, hip.ptr(times), None,
                                      hip.ptr(w), hip.ptr(traj), hip.ptr(xp), None, hip.current_stream()), "vihds_ode_fwd")
    torch.cuda.synchronize()
    r64 = ref[F64]
    vals = {"traj": rel_err(traj.permute(2, 3, 1, 0), r64["traj"]), "xp": rel_err(xp.permute(2, 3, 1, 0), r64["xp"])}
    print("G 17-1-93 without observations: " + "  ".join("%s %.1e (%.0e)" % (k, v, TOL) for k, v in vals.items()))
    assert all(v < TOL for v in vals.values()), vals
