"""CPU tests of the delayed reads of vihds.modelgen (`delays`, read as self.delayed.<name> in rhs): every refusal by its
message, the generated text and its digests (and the unchanged digests of every class without the attribute), the float64
yardstick itself (the frozen twin, the order of the scheme, the gradient with respect to tau), csrc/vihds_delay.hpp in a
stand-alone host program under the address and undefined-behaviour sanitizers, and compilation for gfx950 (scratch and VGPRs of
every fixed-grid kernel of the test models)."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G
from vihds.utils import attrify

import modelgen_delay_models as DM
import modelgen_models as MM
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
ALL = [DM.DelayedRepressor, DM.TwoDelays, DM.DelayedStart, DM.DelayedRepressorFrozen, DM.DelayedRepressorTreated]
GOLDEN = os.path.join(ROOT, "tests", "golden", "modelgen_delay_source_sha256.json")


def _lagged(name, **body):
    """_define's six-species model with the effective parameter `tau` and one delayed read of OD in rhs."""
    attrs = dict(parameters=["r", "tau", "init_x"], delays={"lag": ("OD", "tau")},
                 prepare=lambda self, th, c: {"r": th.r, "tau": th.tau},
                 rhs=lambda self, t, y, p, c: [p.r * self.delayed.lag] + [0.0] * 5)
    attrs.update(body)
    return _define(name, **attrs)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ok = _lagged("lag_ok")
    assert ok._trace.delays == [("lag", "OD", "tau")] and G.GeneratedOdeModel.delays is None and G.MAX_DELAYS == 4
    for what, match in ((dict(implicit=True), "delays and implicit = True"), (dict(substeps=2), "delays and substeps = 2"),
                        (dict(lead_in=0.5), "delays and lead_in = 0.5"),
                        (dict(jump=lambda self, y, p, c: list(y)), r"delays and jump\(self, y, p, c\)"),
                        (dict(networks={"n": G.Network(1, 2, 1)}), "delays and networks"),
                        (dict(algebraic=["z0"], algebraic_start=lambda self, y, p, c: [p.r],
                              constraint=lambda self, y, z, p, c: [z[0] - p.r]), "delays and algebraic variables")):
        with pytest.raises(G.ModelDefinitionError, match=match + ".*declined in this version"):
            _lagged("lag_with_%s" % sorted(what)[0], **what)
    with pytest.raises(G.ModelDefinitionError, match="declares delays.*does not take NeuralPrecisions"):
        G.generate_source(ok, True)
    four = {"l%d" % k: ("OD", "tau") for k in range(4)}
    assert "N_DELAYS = 4" in G.generate_source(_lagged("lag_four", delays=four,
                                                       rhs=lambda self, t, y, p, c: [p.r * self.delayed.l3] + [0.0] * 5))
    with pytest.raises(G.ModelDefinitionError, match="5 delays.*at most 4"):
        _lagged("lag_five", delays=dict(four, l4=("OD", "tau")))
    with pytest.raises(G.ModelDefinitionError, match="'lag' reads the unknown species 'nope'"):
        _lagged("lag_species", delays={"lag": ("nope", "tau")})
    with pytest.raises(G.ModelDefinitionError, match="names the delay 'nope', which is no effective parameter"):
        _lagged("lag_parameter", delays={"lag": ("OD", "nope")})
    with pytest.raises(G.ModelDefinitionError, match="names the delay 'init_x', which is no effective parameter"):
        _lagged("lag_theta_not_effective", delays={"lag": ("OD", "init_x")})  # (a key of what prepare returns, not of theta)
    for clash, extra in (("OD", {}), ("r", {}), ("light", dict(forcings=["light"]))):
        with pytest.raises(G.ModelDefinitionError, match="also a species, a parameter, a forcing or an algebraic variable"):
            _lagged("lag_clash_%s" % clash, delays={clash: ("OD", "tau")}, **extra)
    with pytest.raises(G.ModelDefinitionError, match="delays must be a dict"):
        _lagged("lag_list", delays=[("lag", "OD", "tau")])
    with pytest.raises(G.ModelDefinitionError, match="unknown delayed read 'other'"):
        _lagged("lag_unknown", rhs=lambda self, t, y, p, c: [p.r * self.delayed.other] + [0.0] * 5)


def test_where_a_delayed_read_may_be_read():
    for hook, definition in (("prepare", lambda self, th, c: {"r": th.r * self.delayed.lag, "tau": th.tau}),
                             ("initial_state", lambda self, th, c: [th.init_x * self.delayed.lag] + [0.0] * 5),
                             ("start", lambda self, y, p, c: [y[0] + self.delayed.lag] + list(y[1:])),
                             ("observe", lambda self, y, p, c: [self.delayed.lag] * 4),
                             ("precision", lambda self, y, x, p, c: [1.0 + self.delayed.lag] * 4),
                             ("log_likelihood", lambda self, x, obs, pr, p, c: [self.delayed.lag * (x[j] - obs[j]) for j in range(4)])):
        with pytest.raises(G.ModelDefinitionError, match="delayed read 'lag' read in %s" % hook):
            _lagged("lag_in_%s" % hook, **{hook: definition})
    # network-free expressions and where conditions in rhs
    ok = _lagged("lag_where", rhs=lambda self, t, y, p, c: [G.where(self.delayed.lag > 0.5, p.r, 2.0 * p.r) * y[0]
                                                            + G.sqrt(1.0 + self.delayed.lag * self.delayed.lag)] + [0.0] * 5)
    assert "N_DELAYS = 1" in G.generate_source(ok)


def _config(solver, n_conditions):
    return SimpleNamespace(device="cpu", params=attrify({"solver": solver}),
                           data=SimpleNamespace(device_depth=1, conditions=["c%d" % k for k in range(n_conditions)],
                                                relevance_vectors={}, default_devices=[]))


def test_host_checks_run_before_anything_is_built(monkeypatch):
    """An adaptive solver and the implicit solver raise from solve, ahead of the library build and of every launch."""
    def no_build(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(G, "register_kernel", no_build)
    times = torch.tensor(DM.RAGGED)
    for solver in hip.ADAPTIVE_SOLVERS:
        model = DM.DelayedRepressor(_config(solver, 0))
        with pytest.raises(NotImplementedError, match="declares delays.*adaptive solver '%s'" % solver):
            model.solve(_config(solver, 0), times, None, torch.zeros(3, 0), None)
    model = DM.DelayedRepressor(_config("beuler", 0))
    with pytest.raises(NotImplementedError, match="needs a generated model with implicit = True"):
        model.solve(_config("beuler", 0), times, None, torch.zeros(3, 0), None)


# ---- the generated text -------------------------------------------------------------------------------------------------------
def test_generated_text():
    src = G.generate_source(DM.DelayedRepressor)
    tr = DM.DelayedRepressor._trace
    D0 = tr.D0
    assert D0 == tr.NP == len(tr.p_names) == 8  # (no treatment read, no forcing: the reads' slots follow the named parameters)
    for line in ("static constexpr int N_DELAYS = 1;  // Rlag = R(t - tau): p[8 ..] values, p[9 ..] slopes, p[10] the interval start",
                 "static constexpr int DELAY_SLOT = 8;", "static constexpr int NP = 11;",
                 "static constexpr int delay_species(int e) { return 1; }",
                 "static constexpr int delay_param(int e) { return 5; }",
                 "static void set_delay(float* p, float t_lo, float inv_dt, const float* d_lo, const float* d_hi) {",
                 "    p[8] = d_lo[0];", "    p[9] = (d_hi[0] - d_lo[0]) * inv_dt;", "    p[10] = t_lo;",
                 "(p[8] + (t - p[10]) * p[9])", "pb[8] +=", "pb[9] +="):
        assert line in src, line
    assert "pb[10]" not in src  # (the interval start has no adjoint)
    prepare = src[src.index("static void prepare("):src.index("static void prepare_vjp(")]
    prepare_vjp = src[src.index("static void prepare_vjp("):src.index("static void init(")]
    for k in (8, 9, 10):  # prepare writes none of the reserved entries and prepare_vjp leaves their adjoints alone
        assert "p[%d]" % k not in prepare and "pb[%d]" % k not in prepare_vjp
    two = G.generate_source(DM.TwoDelays)
    t2 = DM.TwoDelays._trace
    assert t2.F0 == 8 and t2.D0 == 11  # (one forcing: value, slope, interval start; the reads' slots behind them)
    for line in ("static constexpr int N_FORCINGS = 1;", "static constexpr int N_DELAYS = 2;", "static constexpr int DELAY_SLOT = 11;",
                 "static constexpr int NP = 16;", "delay_species(int e) { return e == 0 ? 1 : 2; }",
                 "delay_param(int e) { return e == 0 ? 7 : 6; }", "    p[13] = (d_hi[0] - d_lo[0]) * inv_dt;",
                 "    p[14] = (d_hi[1] - d_lo[1]) * inv_dt;", "    p[15] = t_lo;", "(p[12] + (t - p[15]) * p[14])"):
        assert line in two, line
    started = G.generate_source(DM.DelayedStart)
    assert "N_DELAYS = 1" in started and "static void start(" in started
    for cls in (DM.DelayedRepressorFrozen, DM.DelayedRepressorTreated):
        text = G.generate_source(cls)  # (module and key carry the word: the members are what must be absent)
        assert "N_DELAYS" not in text and "DELAY_SLOT" not in text and "set_delay" not in text and "delay_species" not in text


def test_classes_without_delays_generate_the_recorded_text():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        for key, digest in json.load(f).items():
            cname, neural = key.split(":")
            text = G.generate_source(getattr(MM, cname), bool(int(neural)))
            assert hashlib.sha256(text.encode()).hexdigest() == digest, key
            assert "DELAY" not in text and "delay" not in text
    n = 0
    for name in ("modelgen_source_sha256_all.json", "modelgen_algebraic_source_sha256.json"):
        with open(os.path.join(ROOT, "tests", "golden", name)) as f:
            recorded = json.load(f)
        for key, digest in recorded.items():
            path, neural = key.split(":")
            if "." in path:
                module, cname = path.rsplit(".", 1)
            else:
                module, cname = "modelgen_algebraic_models", path
            text = G.generate_source(getattr(importlib.import_module(module), cname), bool(int(neural)))
            assert hashlib.sha256(text.encode()).hexdigest() == digest, key
            assert "DELAY" not in text and "delay" not in text
            n += 1
    assert n >= 34


def test_new_classes_generate_the_recorded_text():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted("%s:0" % c.__name__ for c in ALL)
    for cls in ALL:
        text = G.generate_source(cls)
        assert hashlib.sha256(text.encode()).hexdigest() == recorded["%s:0" % cls.__name__], cls.__name__


def test_documents_have_the_paragraph():
    for word in ("Delayed reads.", "self.delayed.Rlag", "MAX_DELAYS", "set_delay", "fmaxf(tau, 0", "vihds_delay.hpp"):
        assert word in G.__doc__, word
    with open(os.path.join(CSRC, "vihds_delay.hpp")) as f:
        header = f.read()
    for word in ("s_hi = fminf(t_k+1 - taue, t_k)", "clamped into [0, k-1] before any load", "no atomics"):
        assert word in header, word
    for name, words in (("DESIGN.md", ("Delayed reads", "sub-steps with delays", "state-dependent delays", "non-constant initial history")),
                        ("INTEGRATION.md", ("Delayed reads",)), ("README.md", ("delays",))):
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        for word in words:
            assert word in text, (name, word)


# ---- the yardstick itself, in float64 -----------------------------------------------------------------------------------------
def _theta(cls, B, S, times, **over):
    pb = DM.problem(cls, B, S, times)
    th = {n: v.clone() for n, v in pb["th"].items()}
    for n, v in over.items():
        th[n] = torch.full_like(th[n], v) if not isinstance(v, torch.Tensor) else v
    return pb, th


@pytest.mark.parametrize("solver", DM.FIXED)
def test_a_delay_over_the_whole_span_is_the_frozen_twin(solver):
    """With tau >= t_end - t_0 every lookup is the constant history R(t_0): the yardstick equals the frozen twin, which reads the
    initial-state parameter, to rounding; the gradient with respect to tau is exactly 0."""
    tt = torch.tensor(DM.RAGGED, dtype=F64)
    span = float(tt[-1] - tt[0])
    for tau in (span, 1.5 * span):
        pb, th = _theta(DM.DelayedRepressor, 3, 5, DM.RAGGED, tau=tau)
        th = {n: v.requires_grad_(True) for n, v in th.items()}
        xs, xp, logp = DM.forward(DM.DelayedRepressor, th, pb["cond"], tt, solver, pb["obs"])
        fs, fp, flogp = DM.forward(DM.DelayedRepressorFrozen, th, pb["cond"], tt, solver, pb["obs"])
        e = float((xs - fs).detach().abs().max() / fs.detach().abs().max())
        print("%s tau %.2f: delayed against frozen %.2e" % (solver, tau, e))
        assert e <= 1e-14 and float((logp - flogp).detach().abs().max()) <= 1e-11 * float(flogp.detach().abs().max())
        (logp * pb["G"]["logp"]).sum().backward()
        assert float(th["tau"].grad.abs().max()) == 0.0 and float(th["init_r"].grad.abs().max()) > 0.0


def _refined(times, m):
    t = np.asarray(times, dtype=np.float64)
    return np.concatenate([np.linspace(t[k], t[k + 1], m, endpoint=False) for k in range(len(t) - 1)] + [t[-1:]]).tolist()


def test_rk4_is_of_second_order_with_a_delay_above_the_step():
    """DelayedRepressor, rk4, every tau at least the largest step (so no read is clamped to the start of its step): the error
    against the same scheme on grids refined 2, 4 and 8 times falls by more than 3 per halving (the linear interpolant of the
    history caps the order at 2: a factor 4)."""
    base = [0.25 * k for k in range(17)]  # (t = 0 .. 4 in steps of 0.25)
    B, S = 2, 3
    pb, th = _theta(DM.DelayedRepressor, B, S, base)
    th["tau"] = 0.5 + 0.9 * torch.rand(B, S, generator=torch.Generator().manual_seed(4), dtype=F64)  # (0.5 .. 1.4: at least twice the step)
    ends = {}
    with torch.no_grad():
        for m in (1, 2, 4, 8, 16):
            tt = torch.tensor(_refined(base, m), dtype=F64)
            xs, _, _ = DM.forward(DM.DelayedRepressor, th, pb["cond"], tt, "rk4")
            ends[m] = xs[:, :, :, ::m]
    errs = [float((ends[m] - ends[2 * m]).abs().max()) for m in (1, 2, 4, 8)]
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("rk4 with a delay: differences between successive refinements %s, ratios %s"
          % (", ".join("%.3e" % e for e in errs), ", ".join("%.2f" % r for r in ratios)))
    assert all(r > 3.0 for r in ratios), ratios


@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_the_gradient_with_respect_to_tau_agrees_with_a_central_difference(cls):
    """At inputs away from the kinks (precondition (b) of the GPU tests: 1e-3 of the local step), midpoint and rk4."""
    B, S = 3, 5
    pb = DM.problem(cls, B, S)
    margin, classes = DM.kink_margins(cls, pb)
    print("%s: smallest kink margin %.2e, delay classes %s" % (cls.__name__, margin, sorted(classes)))
    assert margin >= 1e-3 and classes == {0, 1, 2, 3}
    tt = pb["times"]

    def loss(tau, solver):
        th = dict(pb["th"], tau=tau)
        _, _, logp = DM.forward(cls, th, pb["cond"], tt, solver, pb["obs"])
        return (logp * pb["G"]["logp"]).sum()

    for solver in ("midpoint", "rk4"):
        tau = pb["th"]["tau"].clone().requires_grad_(True)
        loss(tau, solver).backward()
        h = 1e-6
        fd = torch.zeros_like(tau)
        with torch.no_grad():
            for b in range(B):
                for s in range(S):
                    d = torch.zeros_like(tau)
                    d[b, s] = h
                    fd[b, s] = (loss(pb["th"]["tau"] + d, solver) - loss(pb["th"]["tau"] - d, solver)) / (2 * h)
        e = float((tau.grad - fd).abs().max() / fd.abs().max())
        print("%s %s: d loss / d tau against the central difference %.2e (largest %.3e)" % (cls.__name__, solver, e, float(fd.abs().max())))
        assert float(fd.abs().max()) > 0.0 and e <= 1e-6


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every fixed-grid solver compile for gfx950 and spill nothing
    (VGPRs printed; recorded in DESIGN.md)."""
    header = tmp_path / "delay.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(n_delays<VIHDS_GEN_CORE>::value == %d);" % len(cls.delays),
             "static_assert(n_delays<PrprConstant>::value == 0 && n_delays<WithPrec<PrprConstant>>::value == 0);"]
    for solver in DM.FIXED:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "delay"), "_ZN5vihds")
    assert len(usage) == 15, sorted(usage)
    for solver in DM.FIXED:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d" % (cls.__name__, solver, min(fwd), max(fwd), bwd[0]))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


# ---- csrc/vihds_delay.hpp in a stand-alone host program under sanitizers ----------------------------------------------------------
PROGRAM = r"""
// reads "T, t[T], y[T]" and then cases "tau g_lo g_hi".  Per case it walks the intervals k = 0 .. T-2 upwards with the forward's
// cursor and downwards with the adjoint's, the history of interval k in a heap array of exactly k + 1 floats (a load behind the
// points stored so far is a heap overflow) and its adjoint column likewise, and prints per k:
//   k j_lo j_hi (forward walk) j_lo j_hi (adjoint walk) d_lo d_hi taub A[0 .. k]
#include <cstdio>
#include <memory>
#include <vector>
#include "vihds_delay.hpp"
using namespace vihds;
struct Out { int jl, jh; float dlo, dhi, taub; std::vector<float> A; };
static Out interval(const float* t, const std::vector<float>& yall, int k, float tau, float g_lo, float g_hi, int& cur, bool up) {
  std::unique_ptr<float[]> y(new float[k + 1]), A(new float[k + 1]);
  for (int q = 0; q <= k; ++q) { y[q] = yall[q]; A[q] = 0.f; }
  auto time_at = [&](int q) { return t[q]; };
  auto y_at = [&](int q) { return y[q]; };
  auto a_at = [&](int q) -> float& { return A[q]; };
  const DelayEnds en = delay_ends(t[k], t[k + 1], tau);
  cur = up ? delay_seek_up(time_at, cur, k, en.s_lo) : delay_seek_down(time_at, cur, k, en.s_lo);
  const DelayHit lo = delay_lookup(time_at, y_at, cur, en.s_lo, t[0], y[0], tau);
  const int jh = delay_seek_up(time_at, cur, k, en.s_hi);
  const DelayHit hi = delay_lookup(time_at, y_at, jh, en.s_hi, t[0], y[0], tau);
  Out o{cur, jh, lo.value, hi.value, 0.f, {}};
  o.taub = delay_scatter(a_at, lo, g_lo, true) + delay_scatter(a_at, hi, g_hi, !en.clamped);
  o.A.assign(A.get(), A.get() + k + 1);
  return o;
}
int main() {
  int T;
  if (std::scanf("%d", &T) != 1 || T < 2) return 2;
  std::unique_ptr<float[]> t(new float[T]);
  std::vector<float> y(T);
  for (int q = 0; q < T; ++q) if (std::scanf("%f", &t[q]) != 1) return 2;
  for (float& v : y) if (std::scanf("%f", &v) != 1) return 2;
  float tau, g_lo, g_hi;
  while (std::scanf("%f %f %f", &tau, &g_lo, &g_hi) == 3) {
    std::vector<Out> up(T - 1), down(T - 1);
    int cur = 0;
    for (int k = 0; k < T - 1; ++k) up[k] = interval(t.get(), y, k, tau, g_lo, g_hi, cur, true);
    cur = T - 2;
    for (int k = T - 2; k >= 0; --k) down[k] = interval(t.get(), y, k, tau, g_lo, g_hi, cur, false);
    for (int k = 0; k < T - 1; ++k) {
      std::printf("%d %d %d %d %d %.9g %.9g %.9g", k, up[k].jl, up[k].jh, down[k].jl, down[k].jh, up[k].dlo, up[k].dhi, up[k].taub);
      for (float v : up[k].A) std::printf(" %.9g", v);
      std::printf("\n");
    }
  }
  return 0;
}
"""


def _host_compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) or (name if os.path.exists(name) else None)
        if path:
            return path
    return None


def _restate(times, y, k, tau, g_lo, g_hi, dt):
    """The definition of vihds_delay.hpp for interval k in numpy scalars of type dt, operation for operation (float32: a fused
    multiply-add is the float64 product and sum rounded once): (j_lo, j_hi, d_lo, d_hi, taub, A[0 .. k])."""
    t, y = times.astype(dt), y.astype(dt)
    fma = (lambda a, b, c: np.float32(np.float64(a) * np.float64(b) + np.float64(c))) if dt is np.float32 else (lambda a, b, c: a * b + c)
    tau, g_lo, g_hi = dt(tau), dt(g_lo), dt(g_hi)
    taue = tau if tau > 0 else dt(0.0)  # fmaxf(tau, 0): 0 for a NaN
    finite = bool(np.isfinite(tau))
    A, taub = np.zeros(k + 1, dtype=dt), dt(0.0)
    with np.errstate(invalid="ignore"):
        s_lo, s = dt(t[k] - taue), dt(t[k + 1] - taue)
    clamped = not (s < t[k])
    out = []
    for s_, g, moves in ((s_lo, g_lo, True), (t[k] if clamped else s, g_hi, not clamped)):
        below = [q for q in range(k) if t[q] <= s_]
        j = max(below) if below else 0
        if not (s_ > t[0]):
            value = y[0]
            A[0] = dt(A[0] + g)
        else:
            step, dy = dt(t[j + 1] - t[j]), dt(y[j + 1] - y[j])
            w, slope = dt(dt(s_ - t[j]) / step), dt(dy / step)
            value = fma(w, dy, y[j])
            A[j] = dt(A[j] + fma(-w, g, g))
            A[j + 1] = dt(A[j + 1] + dt(w * g))
            if moves:
                taub = dt(taub + dt(-slope * g))
        out.append((j, value if finite else dt(np.nan)))
    return out[0][0], out[1][0], out[0][1], out[1][1], taub, A


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
@pytest.mark.parametrize("grid", ["ragged", "two"])
def test_lookup_and_scatter_in_a_host_program_under_sanitizers(tmp_path, grid):
    """csrc/vihds_delay.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own.  Every k of the
    ragged grid of 9 points and of T = 2; tau NaN, +inf, -1, 0, below the smallest step, between steps, exactly a step, above the
    whole span, and delays that put s exactly on grid points.  A clean sanitizer run; the forward's and the adjoint's cursor walks
    give the same indices; value, scatter weights and the tau term within 8 x the distance of a float32 numpy restatement from
    the float64 one (largest figures printed)."""
    src, exe = tmp_path / "delay.cpp", tmp_path / "delay"
    src.write_text(PROGRAM)
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    times = np.array(DM.RAGGED if grid == "ragged" else [0.25, 0.75], dtype=np.float32)
    T = len(times)
    rng = np.random.RandomState(3)
    y = (0.5 + rng.rand(T)).astype(np.float32)
    steps = np.diff(times.astype(np.float64))
    taus = [float("nan"), float("inf"), -1.0, 0.0, 0.37 * steps.min(), 0.5 * (steps.min() + steps.max()) if T > 2 else 0.61 * steps[0],
            float(steps.max()), float(steps.min()), 1.25 * float(times[-1] - times[0]), 1e30]
    # s exactly on grid points: differences of grid points (float32 differences of these grids are exact or land within an ulp)
    taus += sorted({float(np.float32(times[a]) - np.float32(times[b])) for a in range(T) for b in range(a)})
    cases = [(np.float32(tau), np.float32(rng.randn()), np.float32(rng.randn())) for tau in taus]
    text = "%d\n%s\n%s\n" % (T, " ".join("%.9g" % v for v in times), " ".join("%.9g" % v for v in y))
    text += "".join("%.9g %.9g %.9g\n" % c for c in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(cases) * (T - 1)
    worst = {"value": (0.0, 0.0), "scatter": (0.0, 0.0), "tau term": (0.0, 0.0)}
    on_grid = 0
    for c, (tau, g_lo, g_hi) in enumerate(cases):
        for k in range(T - 1):
            f = rows[c * (T - 1) + k].split()
            assert int(f[0]) == k
            j32 = _restate(times, y, k, tau, g_lo, g_hi, np.float32)
            r64 = _restate(times, y, k, tau, g_lo, g_hi, np.float64)
            ju, jhu, jd, jhd = (int(v) for v in f[1:5])
            assert (ju, jhu) == (jd, jhd) == (j32[0], j32[1]), (tau, k, f[1:5], j32[:2])
            assert 0 <= ju <= max(k - 1, 0) and 0 <= jhu <= max(k - 1, 0)
            f32 = lambda v: np.float64(np.float32(float(v)))  # noqa: E731  (nine digits name a float32; its value is that float32)
            got = (np.array([f32(f[5]), f32(f[6])]), np.array([f32(f[7])]), np.array([f32(v) for v in f[8:]]))
            assert len(got[2]) == k + 1
            if not np.isfinite(tau):
                assert np.isnan(got[0]).all() and np.isnan(np.array(j32[2:4], dtype=np.float64)).all(), (tau, k)
            s_lo = np.float32(times[k] - (tau if tau > 0 else np.float32(0)))
            on_grid += int(np.isfinite(tau) and s_lo in times)
            for name, g, r32_, r64_ in (("value", got[0], np.array(j32[2:4], dtype=np.float64), np.array(r64[2:4])),
                                        ("tau term", got[1], np.array([j32[4]], dtype=np.float64), np.array([r64[4]])),
                                        ("scatter", got[2], j32[5].astype(np.float64), r64[5])):
                if name == "value" and not np.isfinite(tau):
                    continue
                scale = max(float(np.abs(r64_).max()), 1e-30)
                e_got, e_32 = float(np.abs(g - r64_).max()) / scale, float(np.abs(r32_ - r64_).max()) / scale
                if e_got > worst[name][0]:
                    worst[name] = (e_got, e_32)
                assert e_got <= 8.0 * e_32, (name, float(tau), k, e_got, e_32)
    assert on_grid >= T - 1
    for name, (e_got, e_32) in worst.items():
        print("%s grid, %s: largest distance to float64 %.2e (the float32 restatement's there %.2e)" % (grid, name, e_got, e_32))
