"""CPU tests of `step_tolerance = (rtol, atol)` in vihds.modelgen and of the host-side parts of the step control: validation and
every refusal with its message, the generated text (two lines, recorded digests, the twin without the attribute), the host
declines before anything is built or queued, the float64 restatement of the rule checked against an independent numpy loop, the
preconditions the GPU tests assert, the read-out, compilation for gfx950 (scratch, VGPRs and LDS of every new kernel; the kernel
set of a controlled launcher), and csrc/vihds_stepctl.hpp in a stand-alone host program under the address and
undefined-behaviour sanitizers."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G, ops

import modelgen_jump_models as JM
import modelgen_stepctl_models as CM
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_substeps_host import SOLVER_ENUM, _config, _host_compiler, _usage_with_lds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "modelgen_stepctl_source_sha256.json")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
six = lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5  # noqa: E731


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_validation():
    assert G.GeneratedOdeModel.step_tolerance is None and G.STEP_CONTROL_CEILINGS == (2, 4, 8)
    for m in (2, 4, 8):
        cls = _define("ctl_ok_%d" % m, substeps=m, step_tolerance=(1e-3, 1e-6), rhs=six)
        assert cls.step_tolerance == (1e-3, 1e-6) and cls(_config("rk4", 0)).has_step_control
    assert not _define("ctl_none", substeps=4, rhs=six)(_config("rk4", 0)).has_step_control
    for m in (1, 3, 5, 6, 7):
        with pytest.raises(G.ModelDefinitionError, match=r"step_tolerance and substeps = %d.*ceiling.*2, 4, 8" % m):
            _define("ctl_bad_m_%d" % m, substeps=m, step_tolerance=(1e-3, 1e-6), rhs=six)
    for k, bad in enumerate(((0.0, 0.0), (-1e-3, 1e-6), (1e-3, -1.0), (float("nan"), 1e-6), (1e-3, float("inf")), (1e39, 0.0),
                             1e-3, (1e-3,), (1e-3, 1e-6, 0.0), ("1e-3", 1e-6), (True, 1e-6))):
        with pytest.raises(G.ModelDefinitionError, match=r"step_tolerance = .*\(rtol, atol\).*not both\s+0"):
            _define("ctl_bad_tol_%d" % k, substeps=4, step_tolerance=bad, rhs=six)
    for good in ((1e30, 0.0), (0.0, 1e-30), [1e-3, 1e-6], (np.float32(1e-3), 0), (1, 0)):  # (very large values are legal)
        _define("ctl_good_tol_%d" % abs(hash(str(good))), substeps=2, step_tolerance=good, rhs=six)
    # the adjoint's LDS: (M - 1) * species rows, as for substeps
    wide = dict(species=["s%d" % k for k in range(9)], initial_state=lambda self, th, c: [th.init_x] + [0.0] * 8,
                rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 8)
    assert _define("ctl_nine_4", substeps=4, step_tolerance=CM.TOL, **wide).substeps == 4
    with pytest.raises(G.ModelDefinitionError, match="MAX_SUBSTEP_ROWS"):
        _define("ctl_nine_8", substeps=8, step_tolerance=CM.TOL, **wide)


def test_refusals_when_the_class_is_defined():
    with pytest.raises(G.ModelDefinitionError, match="step_tolerance and networks.*declined in this version"):
        _define("ctl_net", substeps=2, step_tolerance=CM.TOL, networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match=r"has delays and step_tolerance = \(0.001, 1e-06\).*declined in this version"):
        _define("ctl_delay", substeps=2, step_tolerance=CM.TOL, parameters=["r", "tau", "init_x"],
                prepare=lambda self, th, c: {"r": th.r, "tau": th.tau}, delays={"lag": ("OD", "tau")},
                rhs=lambda self, t, y, p, c: [p.r * self.delayed.lag] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match=r"step_tolerance and diffusion\(self, y, p, c\).*declined in this version"):
        _define("ctl_noise", substeps=2, step_tolerance=CM.TOL, rhs=six,
                diffusion=lambda self, y, p, c: [0.1 * y[0]] + [0.0] * 5)
    ok = _define("ctl_for_neural", substeps=2, step_tolerance=CM.TOL, rhs=six)
    with pytest.raises(G.ModelDefinitionError, match=r"step_tolerance = \(0.001, 1e-06\).*precision network"):
        G.generate_source(ok, True)


def test_docstring_has_a_step_control_paragraph():
    for word in ("Error-controlled sub-steps.", "step_tolerance = ", "STEP_RTOL", "saturated", "substep_counts", "1e-5"):
        assert word in G.__doc__, word


# ---- generated text -------------------------------------------------------------------------------------------------------------
def test_generated_text_and_digests():
    """A controlled class generates its twin's text plus the two STEP_ lines behind SUBSTEPS; the twin without the attribute
    generates what a class that never heard of it does; the digests of the new models' text are recorded."""
    for cls, twin in CM.TWIN.items():
        a = G.generate_source(twin).replace(twin.model_key, "KEY").replace(twin.__qualname__, "NAME").splitlines()
        text = G.generate_source(cls)
        assert text == G.generate_source(cls)
        b = text.replace(cls.model_key, "KEY").replace(cls.__qualname__, "NAME").splitlines()
        added = [ln for ln in b if "STEP_" in ln]
        assert len(added) == 2 and len(b) == len(a) + 2 and not any("STEP_" in ln for ln in a)
        at = b.index(added[0])
        assert b[at - 1] == "  static constexpr int SUBSTEPS = %d;" % cls.substeps and b[at + 1] == added[1]
        assert added[0].startswith("  static constexpr float STEP_RTOL = %s;" % G._lit(cls.step_tolerance[0]))
        assert added[1] == "  static constexpr float STEP_ATOL = %s;" % G._lit(cls.step_tolerance[1])
        assert [ln for ln in b if ln not in added] == a, cls.__name__
    # (the attribute written out as None: byte for byte the text of the class without it)
    plain = G.generate_source(CM.PulsedPrprSub8)
    restated = type("PulsedPrprSub8", (JM.PrprDiluted,), {"model_key": CM.PulsedPrprSub8.model_key, "substeps": 8,
                                                          "step_tolerance": None, "__module__": CM.PulsedPrprSub8.__module__,
                                                          "__qualname__": "PulsedPrprSub8"})
    assert G.generate_source(restated) == plain
    assert G.generate_source(JM.PrprDiluted).count("STEP_") == 0
    with open(GOLDEN) as f:
        recorded = json.load(f)
    classes = CM.MODELS + CM.WIDEST + [CM.PulsedPrprSub8, CM.PulsedPrprSub4, CM.PulsedPrprSub2, CM.CombinedSub4, CM.ReaderSub4]
    digests = {cls.model_key: hashlib.sha256(G.generate_source(cls).encode()).hexdigest() for cls in classes}
    assert digests == recorded, json.dumps(digests, indent=1, sort_keys=True)


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def test_host_declines_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hip, "lib", no_library)
    monkeypatch.setattr(G, "register_kernel", no_library)
    assert G.STEP_CONTROL_DECLINED_SOLVERS == ("modeuler", "modeulerwhile")
    cls = CM.PulsedPrpr
    key = cls.model_key
    monkeypatch.setitem(hip.MODELS, key, 1024)
    monkeypatch.setitem(hip.GENERATED_SUBSTEPS, key, cls.substeps)
    monkeypatch.setitem(hip.GENERATED_STEP_CONTROL, key, (8,) + CM.TOL)  # (what register_kernel records)
    for solver in ("modeuler", "modeulerwhile"):
        with pytest.raises(NotImplementedError, match=r"step control \(step_tolerance\).*'%s'.*fixed step h0" % solver):
            ops.OdeProblemSpec(key, solver, {}, 1, C=0)
        with pytest.raises(NotImplementedError, match=r"step_tolerance = \(0.001, 1e-06\).*'%s'.*fixed step\s+h0.*solvers with "
                                                      r"step control: beuler, euler, midpoint, rk4" % solver):
            cls(_config(solver, 0)).solve(_config(solver, 0), torch.tensor(CM.TIMES), None, torch.zeros(3, 0), None)
    for solver in hip.ADAPTIVE_SOLVERS:
        with pytest.raises(NotImplementedError, match=r"substeps = 8.*fixed-grid solvers"):
            ops.OdeProblemSpec(key, solver, {}, 1, C=0)
        with pytest.raises(NotImplementedError, match=r"substeps = 8.*'%s'" % solver):
            cls(_config(solver, 0)).solve(_config(solver, 0), torch.tensor(CM.TIMES), None, torch.zeros(3, 0), None)
    # the twin without the attribute takes modeuler as before
    twin = CM.PulsedPrprSub8
    monkeypatch.setitem(hip.MODELS, twin.model_key, 1025)
    monkeypatch.setitem(hip.GENERATED_SUBSTEPS, twin.model_key, 8)
    with pytest.raises(AssertionError, match="the library was asked for"):
        ops.OdeProblemSpec(twin.model_key, "modeuler", {}, 1, C=0)


def test_the_read_out_and_the_precision_split():
    """substep_counts on both layouts; expand_precisions of an own-precision controlled model hands back the species and the four
    precision rows, never the count row; a model without the attribute is refused by name."""
    cls = CM.ReaderCtl
    N, T, B, S = len(cls.species), 5, 2, 3
    gen = torch.Generator().manual_seed(3)
    buf = torch.rand(T, N + 5, B, S, generator=gen)
    code = torch.tensor([2.0, -4.0, 4.0, 2.0])[:, None, None].expand(T - 1, B, S)
    buf[0, -1], buf[1:, -1] = 0.0, code
    for traj in (buf, buf.permute(2, 3, 1, 0)):
        counts, saturated = G.substep_counts(traj, cls)
        assert counts.dtype == torch.int32 and saturated.dtype == torch.bool
        assert torch.equal(counts, code.abs().to(torch.int32)) and torch.equal(saturated, code < 0)
    model = cls(_config("rk4", 0))
    assert model.has_step_control and torch.equal(G.substep_counts(buf, model)[0], counts)
    sol = buf.permute(2, 3, 1, 0)
    xs, prec = model.expand_precisions(None, list(range(T)), sol)
    assert torch.equal(xs, sol[:, :, :N]) and torch.equal(prec, sol[:, :, N:N + 4])
    with pytest.raises(G.ModelDefinitionError, match="ReaderSub4 has no step_tolerance"):
        G.substep_counts(buf, CM.ReaderSub4)
    with pytest.raises(RuntimeError, match=r"\[T, %d, B, S\]" % (N + 5)):
        G.substep_counts(buf[:, :-1], cls)


# ---- the definition checks itself -----------------------------------------------------------------------------------------------
def _numpy_ladder(cls, th, cond, times, solver):
    """The rule, one trajectory at a time with Python control flow and numpy's ratio: codes [T,B,S]."""
    rtol, atol = cls.step_tolerance
    M, T = int(cls.substeps), len(times)
    B, S = next(iter(th.values())).shape
    codes = np.zeros((T, B, S))
    with torch.no_grad():
        for b in range(B):
            for s in range(S):
                th1 = {n: v[b:b + 1, s:s + 1] for n, v in th.items()}
                rhs, y = cls.torch_problem(th1, cond[b:b + 1], None, times=times)
                for k in range(T - 1):
                    u = JM.jump_at(cls, y, th1, cond[b:b + 1], k, T)
                    coarse, c = CM.phi(cls, solver, rhs, times[k], times[k + 1], u, 1)[0], 1
                    while True:
                        fine = CM.phi(cls, solver, rhs, times[k], times[k + 1], u, 2 * c)[0]
                        r = CM.ratio_numpy(fine[0, 0].numpy(), coarse[0, 0].numpy(), rtol, atol)
                        if r <= 1.0:
                            y, codes[k + 1, b, s] = fine, 2 * c
                            break
                        if 2 * c == M:
                            y, codes[k + 1, b, s] = fine, -M
                            break
                        coarse, c = fine, 2 * c
    return codes


def test_the_restatement_against_an_independent_numpy_loop():
    cls, solver = CM.PulsedPrpr, "midpoint"
    pb = CM.problem(cls, 3, 5, solver)
    codes, looked, xs = CM.ladder(cls, pb["th"], pb["cond"], pb["times"], solver)
    assert np.array_equal(codes.numpy(), _numpy_ladder(cls, pb["th"], pb["cond"], pb["times"], solver))
    assert len(set(codes[1:].reshape(-1).tolist())) >= 3
    # the realised scheme at those counts ends where the ladder ended, and its gradient exists and is finite
    d = CM.definition(cls, pb, solver, F64)
    assert torch.equal(d["codes"], codes) and float((d["traj"][:, :, :6] - xs).abs().max()) <= 1e-12
    assert torch.equal(d["traj"][:, :, 6], codes.permute(1, 2, 0))
    assert all(bool(torch.isfinite(g).all()) for g in d["g_theta"].values()) and float(d["g_theta"]["r"].abs().max()) > 0
    # frozen counts: the definition at the fixed count of a degenerate tolerance is the twin's own definition
    for tol, m, twin in ((CM.LOOSE, 2, CM.PulsedPrprSub2), (CM.TIGHT, 8, CM.PulsedPrprSub8)):
        c2 = CM.ladder(cls, pb["th"], pb["cond"], pb["times"], solver, tol=tol)[0]
        assert bool((c2[1:] == (2.0 if tol == CM.LOOSE else -8.0)).all())
        a = CM.definition(cls, pb, solver, F64, codes=c2)
        b = JM.explicit_definition(twin, pb, solver, F64)
        assert float((a["traj"][:, :, :6] - b["traj"]).abs().max()) <= 1e-12 * float(b["traj"].abs().max())
        for n, g in b["g_theta"].items():
            assert float((a["g_theta"][n] - g).abs().max()) <= 1e-10 * max(float(g.abs().max()), 1e-30), n


def test_the_ratio_of_the_restatement():
    rows = _RATIO_TABLE
    for fine, coarse, rtol, atol in rows:
        want = CM.ratio_numpy(np.float64(fine), np.float64(coarse), rtol, atol)
        got = float(CM.ratio(torch.tensor([[fine]], dtype=F64), torch.tensor([[coarse]], dtype=F64), rtol, atol))
        assert (np.isnan(want) and np.isnan(got)) or want == got, (fine, coarse, rtol, atol, want, got)


@pytest.mark.parametrize("cls,solver,shape", [(CM.PulsedPrpr, "midpoint", (3, 100)), (CM.PulsedPrprFine, "rk4", (3, 100)),
                                              (CM.PrprImplicitCtl, "beuler", (3, 5)), (CM.PrprSdirkCtl, "beuler", (3, 5)),
                                              (CM.CombinedCtl, "midpoint", (3, 100))],
                         ids=lambda v: v if isinstance(v, str) else (v.__name__ if isinstance(v, type) else "%dx%d" % v))
def test_the_inputs_keep_every_ratio_out_of_the_band(cls, solver, shape):
    """What the GPU tests assert first, on the float64 definition alone."""
    pb = CM.problem(cls, shape[0], shape[1], solver)
    codes, looked, xs = CM.ladder(cls, pb["th"], pb["cond"], pb["times"], solver)
    assert bool(torch.isfinite(xs).all()) and not bool(CM.in_band(looked).any())
    first = set(codes[1:].reshape(codes.shape[0] - 1, -1)[:, :64].abs().reshape(-1).tolist())
    print("%s %s: counts among the first 64 trajectories %s" % (cls.__name__, solver, sorted(first)))
    assert len(first) >= (3 if cls.substeps == 8 else 2) and bool((codes < 0).any())


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", [CM.PulsedPrpr, CM.PrprImplicitCtl, CM.PrprSdirkCtl, CM.CombinedCtl, CM.ReaderCtl] + CM.WIDEST,
                         ids=lambda c: c.__name__)
def test_step_control_kernels_compile_without_scratch(tmp_path, cls):
    """The staged forward, the unstaged forward and the adjoint of every solver in scope compile for gfx950 and spill nothing;
    the adjoint's static LDS is (M - 1) * N rows of 256 floats as under `substeps = M`, the forwards declare none (coarse and
    fine live in registers).  VGPRs and LDS are printed (DESIGN.md quotes them)."""
    header = tmp_path / "ctl.hpp"
    header.write_text(G.generate_source(cls))
    solvers = ["euler", "midpoint", "rk4"] + (["beuler"] if cls.implicit else [])
    rows_total = len(cls.species) + (4 if cls._precision_def is not None else 0) + 1
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(step_control<VIHDS_GEN_CORE>::value && !step_control<WithPrec<VIHDS_GEN_CORE>>::value);",
             "static_assert(!step_control<PrprConstant>::value && !step_control<BlackboxIcml>::value);",
             "static_assert(substeps<VIHDS_GEN_CORE>::value == %d && traj_rows<VIHDS_GEN_CORE>::value == %d);"
             % (cls.substeps, rows_total),
             "static_assert(traj_rows<PrprConstant>::value == PrprConstant::N);"]
    for s in solvers:
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s]]
    usage = _usage_with_lds(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "ctl"))
    assert len(usage) == 3 * len(solvers), sorted(usage)
    rows = (cls.substeps - 1) * len(cls.species)
    for s in solvers:
        tag = "Li%dELb" % hip.SOLVERS[s]
        fwd = [v for n, v in usage.items() if "ode_fwd_kernel" in n and tag in n]
        (bwd,) = [v for n, v in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s M=%d %s: forward %d / %d VGPRs, adjoint %d VGPRs and %d bytes of LDS"
              % (cls.__name__, cls.substeps, s, fwd[0][0], fwd[1][0], bwd[0], bwd[2]))
        assert len(fwd) == 2 and all(v[2] == 0 for v in fwd)
        assert bwd[2] == rows * 256 * 4
    for name, (vgpr, scratch, lds) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_controlled_launcher_holds_no_kernel_of_the_modeuler_family(tmp_path):
    """launch_ode with every solver in one unit: the twin holds the fifteen fixed-grid kernels, the controlled class the nine of
    euler, midpoint and rk4 -- no modeuler, no modeulerwhile, no adaptive pair, no one-pass summaries."""
    names = {}
    for cls in (CM.PulsedPrprSub8, CM.PulsedPrpr):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        struct = "GenModel_" + G._ident(cls.model_key)
        names[cls] = sorted(n.replace("%d%s" % (len(struct), struct), "M") for n in usage)
        assert all("ode_fwd_kernel" in n or "ode_bwd_kernel" in n for n in names[cls]), names[cls]
    family = ("Li%dELb" % hip.SOLVERS["modeuler"], "Li%dELb" % hip.SOLVERS["modeulerwhile"])
    assert len(names[CM.PulsedPrprSub8]) == 15 and len(names[CM.PulsedPrpr]) == 9
    assert names[CM.PulsedPrpr] == [n for n in names[CM.PulsedPrprSub8] if not any(t in n for t in family)]


# ---- csrc/vihds_stepctl.hpp in a stand-alone host program under sanitizers -------------------------------------------------------
_RATIO_TABLE = [
    ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 1e-3, 1e-6),            # equal states
    ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1e-3, 1e-6),            # zero states
    ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1e-3, 0.0),             # ... with atol = 0: 0 / 0
    ([1.0, 2.0, 3.0], [1.001, 2.0, 2.9], 1e-3, 1e-6),
    ([1.0, -2.0, 3.0], [1.0, 2.0, 3.0], 1e-3, 1e-6),
    ([1.0, float("nan"), 3.0], [1.0, 2.0, 3.5], 1e-3, 1e-6),   # a NaN species among larger terms
    ([1.0, 2.0, 3.0], [float("nan"), 2.0, 3.0], 1e-3, 1e-6),
    ([1.0, float("inf"), 3.0], [1.0, 2.0, 3.0], 1e-3, 1e-6),   # inf / inf
    ([1.0, float("inf"), 3.0], [1.0, 2.0, 3.0], 0.0, 1e-6),    # inf / atol
    ([1.0, 2.0, 3.0], [1.5, 2.5, 3.5], 1e30, 0.0),             # the loose tolerance of the tests
    ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0000002], 0.0, 1e-30),      # the tight one
    ([1e-20, 2.0, 3.0], [3e-20, 2.0, 3.0], 1e-3, 0.0),
]
PROGRAM = r"""
// mode "g": reads intervals "t0 t1" and prints, for c = 1, 2, 4, 8, "c equal s_0 .. s_c" -- equal: SubGridN(c) has the bits of
// SubGrid<c> at every j (and hs).  mode "r": reads "rtol atol f0 f1 f2 c0 c1 c2" and prints step_ratio<3> and whether r <= 1.f.
// mode "c": reads "code ceiling" and prints step_count_of.
#include <cstdio>
#include <cstring>
#include "vihds_stepctl.hpp"
template <int C>
static void grid(float t0, float t1) {
  const vihds::SubGrid<C> a(t0, t1);
  const vihds::SubGridN b(t0, t1, C);
  bool equal = std::memcmp(&a.hs, &b.hs, sizeof(float)) == 0;
  std::printf("%d", C);
  for (int j = 0; j <= C; ++j) {
    const float x = a.at(j), y = b.at(j);
    equal = equal && std::memcmp(&x, &y, sizeof(float)) == 0;
  }
  std::printf(" %d", equal ? 1 : 0);
  for (int j = 0; j <= C; ++j) std::printf(" %.9g", b.at(j));
  std::printf("\n");
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (argv[1][0] == 'g') {
    float t0, t1;
    while (std::scanf("%f %f", &t0, &t1) == 2) { grid<1>(t0, t1); grid<2>(t0, t1); grid<4>(t0, t1); grid<8>(t0, t1); }
  } else if (argv[1][0] == 'r') {
    float rtol, atol, f[3], c[3];
    while (std::scanf("%f %f %f %f %f %f %f %f", &rtol, &atol, &f[0], &f[1], &f[2], &c[0], &c[1], &c[2]) == 8) {
      const float r = vihds::step_ratio<3>(f, c, rtol, atol);
      std::printf("%.9g %d\n", r, r <= 1.f ? 1 : 0);
    }
  } else {
    float code;
    int ceiling;
    while (std::scanf("%f %d", &code, &ceiling) == 2) std::printf("%d\n", vihds::step_count_of(code, ceiling));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if _host_compiler() is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("stepctl")
    src, exe = d / "stepctl.cpp", d / "stepctl"
    src.write_text(PROGRAM)
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]

    def run(mode, text):
        out = subprocess.run([str(exe), mode], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]
        return out.stdout.strip().splitlines()

    return run


def test_the_run_time_sub_grid_is_the_compile_time_one_bit_for_bit(program):
    """SubGridN(c) against SubGrid<c> for c = 1, 2, 4, 8 over a sweep of intervals: the same float32 bits at every s_j; s_0 == t0 and
    s_c == t1 exactly; the times strictly increase."""
    from test_modelgen_substeps_host import RAGGED
    grids = [np.float32(RAGGED), np.float32(CM.TIMES), np.float32(0.06) * np.arange(200, dtype=np.float32),
             np.float32([1e3, 1e3 + 1e-3, 1e3 + 0.5]), np.float32([-3.7, -1.1, 0.3, 1e-3 + 0.3])]
    cases = [(g[k], g[k + 1]) for g in grids for k in range(len(g) - 1)]
    rows = program("g", "".join("%.9g %.9g\n" % c for c in cases))
    assert len(rows) == 4 * len(cases)
    for q, row in enumerate(rows):
        t0, t1 = cases[q // 4]
        v = row.split()
        c, equal, s = int(v[0]), int(v[1]), np.float32(v[2:])
        assert c == (1, 2, 4, 8)[q % 4] and len(s) == c + 1
        assert equal == 1, (t0, t1, c)
        assert s[0] == t0 and s[c] == t1 and bool((s[1:] > s[:-1]).all()), (t0, t1, c, s)


def test_the_ratio_function_against_numpy(program):
    """step_ratio on a table with NaN, infinity, equal states and zero states: numpy's value in float32 arithmetic to one
    rounding, NaN exactly where numpy says NaN, and the test r <= 1.f fails for every NaN and every infinity."""
    text = "".join("%.9g %.9g %s %s\n" % (rtol, atol, " ".join("%.9g" % x for x in f), " ".join("%.9g" % x for x in c))
                   for f, c, rtol, atol in _RATIO_TABLE)
    rows = program("r", text)
    assert len(rows) == len(_RATIO_TABLE)
    for (f, c, rtol, atol), row in zip(_RATIO_TABLE, rows):
        r, passed = row.split()
        r = float(r)
        want = CM.ratio_numpy(np.float32(f), np.float32(c), np.float32(rtol), np.float32(atol))
        if np.isnan(want):
            assert np.isnan(r) and passed == "0", (f, c, r)
        elif np.isinf(want):
            assert np.isinf(r) and passed == "0", (f, c, r)
        else:
            assert abs(r - want) <= 4 * float(np.spacing(np.float32(want))) and passed == ("1" if want <= 1.0 else "0"), (f, c, r, want)


def test_the_count_the_adjoint_uses_is_clamped(program):
    """step_count_of: |code| into 1 .. ceiling for every float a zeroed or foreign row may hold."""
    codes = [0.0, -0.0, 1.0, 2.0, -2.0, 4.0, -8.0, 8.0, 9.0, 1e9, -1e30, 3e38, float("inf"), float("-inf"), float("nan"), 0.5,
             -0.99, 2.7, 1e-40]
    cases = [(x, m) for x in codes for m in (2, 4, 8)]
    rows = program("c", "".join("%r %d\n" % c for c in cases))
    assert len(rows) == len(cases)
    for (x, m), row in zip(cases, rows):
        want = 1 if not abs(x) >= 1.0 else min(int(min(abs(x), 1e6)), m)
        assert int(row) == want and 1 <= int(row) <= m, (x, m, row)
