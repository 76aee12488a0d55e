"""CPU tests of `substeps = m` in vihds.modelgen and of the host-side parts of the sub-stepped time loops: validation, the
generated text (one line, and none at m = 1), the host declines before anything is built or queued, the float64 yardstick
of the GPU comparisons checked against itself (autograd through the Newton iteration on the refined grid against the
restated implicit-function adjoint; the refined explicit definition against the oracle's own grid), the preconditions the GPU
tests assert, compilation for gfx950 (scratch, VGPRs and LDS of every new kernel; the kernel set of a sub-stepped launcher),
and csrc/vihds_substeps.hpp in a stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vihds_oracle as O
from vihds import hip, modelgen as G, ops
from vihds.utils import attrify

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_substep_models as SM
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # (tests/test_modelgen_forcing_gpu.py: steps 0.1 .. 1.0)
SOLVER_ENUM = {"modeuler": "VIHDS_SOLVER_MODEULER", "modeulerwhile": "VIHDS_SOLVER_MODEULERWHILE",
               "euler": "VIHDS_SOLVER_EULER", "midpoint": "VIHDS_SOLVER_MIDPOINT", "rk4": "VIHDS_SOLVER_RK4",
               "beuler": "VIHDS_SOLVER_BEULER"}
six = lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5  # noqa: E731


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_validation():
    assert G.MAX_SUBSTEPS == 8 and G.GeneratedOdeModel.substeps == 1
    for bad in (0, 9, 2.0, True, -1, None, "2"):
        with pytest.raises(G.ModelDefinitionError, match=r"substeps = .*1 \.\. 8"):
            _define("substeps_bad_%s" % bad, substeps=bad, rhs=six)
    for good in (1, 2, 8, np.int64(3)):
        assert _define("substeps_ok_%d" % good, substeps=good, rhs=six).substeps == good
    with pytest.raises(G.ModelDefinitionError, match="substeps = 2 and networks"):
        _define("substeps_net", substeps=2, networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    ok = _define("substeps_for_neural", substeps=2, rhs=six)
    with pytest.raises(G.ModelDefinitionError, match="substeps = 2.*precision network"):
        G.generate_source(ok, True)
    assert "#define VIHDS_GEN_NEURAL 1" in G.generate_source(_define("substeps_one_neural", substeps=1, rhs=six), True)  # (m = 1 may)
    # the adjoint's LDS: (m - 1) * species rows
    wide = dict(species=["s%d" % k for k in range(9)], initial_state=lambda self, th, c: [th.init_x] + [0.0] * 8,
                rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 8)
    assert _define("substeps_nine_7", substeps=7, **wide).substeps == 7  # 54 rows
    with pytest.raises(G.ModelDefinitionError, match="MAX_SUBSTEP_ROWS"):
        _define("substeps_nine_8", substeps=8, **wide)  # 63 rows
    assert (G.MAX_SUBSTEPS - 1) * G.MAX_IMPLICIT_STATES == G.MAX_SUBSTEP_ROWS == 56
    for cls, parent in SM.PARENT.items():
        assert cls.substeps > 1 and parent.substeps == 1 and cls.model_key != parent.model_key
    assert SM.FastBindingSub4.newton_iterations == 6 and SM.PlateReaderSub3.substeps == 3
    assert all(SM.PlateReaderSub3.__dict__.get(a) is None and getattr(SM.PlateReaderSub3, a) is not None
               for a in ("_observe_def", "_precision_def", "_likelihood_def"))


def test_docstring_has_a_substeps_paragraph():
    for word in ("Sub-steps.", "substeps = ", "MAX_SUBSTEPS", "fmaf", "SUBSTEPS", "recomputes"):
        assert word in G.__doc__, word


# ---- generated text -------------------------------------------------------------------------------------------------------------
def _twin(parent, m):
    """`parent` restated under its own name and key with substeps = m written out."""
    return type(parent.__name__, (parent,), {"model_key": parent.model_key, "substeps": m, "__module__": parent.__module__,
                                             "__qualname__": parent.__qualname__})


def test_generated_text():
    for cls, parent in SM.PARENT.items():
        plain = G.generate_source(parent)
        assert "SUBSTEPS" not in plain
        assert G.generate_source(_twin(parent, 1)) == plain  # substeps = 1 written out: byte for byte
        line = "  static constexpr int SUBSTEPS = %d;" % cls.substeps
        a, b = plain.splitlines(), G.generate_source(_twin(parent, cls.substeps)).splitlines()
        assert len(b) == len(a) + 1 and b.count(line) == 1  # the one line, and nothing else
        b.remove(line)
        assert a == b, cls.__name__
        text = G.generate_source(cls)
        assert text == G.generate_source(cls) and text.count(line) == 1 and text.count("SUBSTEPS") == 1
        assert len(text.splitlines()) == len(a) + 1


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def _config(solver, n_conditions):
    return SimpleNamespace(device="cpu", params=attrify({"solver": solver}),
                           data=SimpleNamespace(device_depth=1, conditions=["c%d" % k for k in range(n_conditions)],
                                                relevance_vectors={}, default_devices=[]))


def test_host_declines_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hip, "lib", no_library)
    monkeypatch.setattr(G, "register_kernel", no_library)
    before = (dict(hip.SOLVERS), hip.IMPLICIT_SOLVERS, hip.ADAPTIVE_SOLVERS)
    assert before == ({"modeuler": 0, "modeulerwhile": 1, "euler": 2, "midpoint": 3, "rk4": 4, "dopri5": 5, "bosh3": 6,
                       "adaptive_heun": 7, "dopri8": 8, "beuler": 9}, ("beuler",), ("dopri5", "bosh3", "adaptive_heun", "dopri8"))
    for cls in (SM.PrprImplicitSub4, SM.PlateReaderSub3):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        monkeypatch.setitem(hip.GENERATED_SUBSTEPS, key, cls.substeps)  # (what register_kernel records)
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"substeps = %d.*fixed-grid solvers: beuler, euler, midpoint, modeuler, "
                                                          r"modeulerwhile, rk4" % cls.substeps):
                ops.OdeProblemSpec(key, solver, {}, 1, C=0)
    for cls in (SM.PrprImplicitSub4, SM.PrprForcedSub2):
        model = cls(_config("dopri5", 0))
        with pytest.raises(NotImplementedError, match=r"substeps = %d.*'dopri5'.*fixed-grid solvers: beuler, euler" % cls.substeps):
            model.solve(_config("dopri5", 0), torch.tensor(SM.TIMES), None, torch.zeros(3, 0), None)
    # a model without sub-steps is not declined here
    monkeypatch.setitem(hip.MODELS, IM.PrprImplicit.model_key, 1025)
    monkeypatch.setitem(hip.GENERATED_SUBSTEPS, IM.PrprImplicit.model_key, 1)
    with pytest.raises(AssertionError, match="the library was asked for"):
        ops.OdeProblemSpec(IM.PrprImplicit.model_key, "dopri5", {}, 1, C=0)


# ---- the definition checks itself -----------------------------------------------------------------------------------------------
def test_the_refined_grid():
    t = torch.tensor(RAGGED, dtype=F64)
    for m in range(1, 9):
        fine = SM.refined(t, m)
        assert fine.shape[0] == (len(RAGGED) - 1) * m + 1 and torch.equal(fine[::m], t)
        assert bool((fine[1:] > fine[:-1]).all())
    assert torch.equal(SM.refined(t, 1), t)


def test_one_substep_is_the_parents_definition():
    """m = 1 of the restated definitions is the definition the earlier tests hold the kernels to."""
    pb = SM.problem(SM.PrprForcedSub4, 2, 3)
    a = SM.explicit_definition(FM.PrprForced, pb, "rk4", F64, m=1)
    xs, xp, _, logp = FM.forward(FM.PrprForced, pb["th"], pb["cond"], pb["times"], "rk4", pb["obs"])
    assert torch.equal(a["traj"], xs) and torch.equal(a["xpred"], xp) and torch.equal(a["logp"], logp)
    pb = SM.problem(SM.PrprImplicitSub4, 2, 3)
    a, b = SM.beuler_definition(IM.PrprImplicit, pb, F64, m=1), IM.definition(IM.PrprImplicit, pb, F64)
    assert torch.equal(a["traj"], b["traj"]) and torch.equal(a["logp"], b["logp"])
    for n in b["g_theta"]:
        assert torch.equal(a["g_theta"][n], b["g_theta"][n]), n


def test_the_interpolant_on_the_refined_grid_is_what_rhs_reads():
    """A forced model on the refined grid: the right-hand side of torch_problem built on `times` reads, at a sub-step time, the
    linear interpolant of the samples -- the same series the m = 1 class would be given on the refined grid."""
    cls, m = SM.PrprForcedSub4, 4
    pb = SM.problem(cls, 3, 4)
    fine = SM.refined(pb["times"], m)
    series = pb["series"][:, 0]  # [B, T]
    k = torch.arange(len(fine) - 1) // m
    lo, hi = pb["times"][k], pb["times"][k + 1]
    interp = series[:, k] + (fine[:-1] - lo) * (series[:, k + 1] - series[:, k]) / (hi - lo)
    interp = torch.cat([interp, series[:, -1:]], dim=1)
    coarse = SM.explicit_definition(cls, pb, "rk4", F64)["traj"]
    rhs, x0 = FM.PrprForced.torch_problem(pb["th"], FM.wide_cond(torch.zeros(3, 0), interp[:, None, :]), None, times=fine)
    twin = O.simulate(rhs, x0, fine, "rk4")[..., ::m]
    assert float((twin - coarse).abs().max() / coarse.abs().max()) <= 1e-13


def test_restated_adjoint_equals_autograd_through_the_newton_iteration():
    """float64, FastBindingSub4: the yardstick's gradient (implicit-function theorem at every sub-step's iterate, only the
    observation points scored) against autograd through 30 unrolled Newton iterations per sub-step: 1e-8 relative per
    parameter, the bound of the m = 1 test of the same kind."""
    cls = SM.FastBindingSub4
    pb = SM.problem(cls, 2, 3, times=SM.TIMES[:3])
    ref = SM.beuler_definition(cls, pb, F64)
    assert ref["last_increment"] <= 1e-9
    auto = SM.beuler_by_autograd(cls, pb, 30)
    for n, g in auto.items():
        e = float((ref["g_theta"][n] - g).abs().max() / g.abs().max())
        print("g_theta[%s]: restated adjoint against autograd through Newton %.2e" % (n, e))
        assert e <= 1e-8, n


@pytest.mark.parametrize("cls", [SM.PrprImplicitSub4, SM.DrImplicitSub4], ids=lambda c: c.__name__)
def test_substeps_make_newton_converge_on_the_piecewise_grid(cls):
    """What the GPU test asserts first, on the float64 yardstick alone: on the piecewise TIMES (steps of 0.3 .. 0.6) the last
    Newton increment is at most 1e-9 with m = 4 and above 1e-3 with m = 1."""
    pb = SM.problem(cls, 3, 100, times=SM.TIMES)
    worst = {m: SM.beuler_refined(cls, pb["th"], pb["cond"], pb["times"], m)[2] for m in (1, 4)}
    print("%s: last Newton increment %.2e at m = 1, %.2e at m = 4" % (cls.__name__, worst[1], worst[4]))
    assert worst[4] <= 1e-9 and worst[1] > 1e-3


def test_substeps_halve_the_error_of_the_stiff_model():
    cls = SM.FastBindingSub4
    pb = SM.problem(cls, 3, 5)  # (the GPU test asserts the same at 3 x 100: 1.09e-1 against 2.8e-2)
    fine = IM.fast_refined(pb["th"], pb["times"])
    err = {m: float((SM.beuler_refined(cls, pb["th"], pb["cond"], pb["times"], m)[0][..., ::m] - fine).abs().max()) for m in (1, 4)}
    print("FastBinding against the 400 times finer grid: %.3e at m = 1, %.3e at m = 4" % (err[1], err[4]))
    assert err[4] < 0.5 * err[1]


# ---- compilation ----------------------------------------------------------------------------------------------------------------
def _usage_with_lds(text):
    """{kernel: (vgprs, scratch, static LDS bytes)} from the kernel-resource-usage remarks."""
    out, lds, cur = _resource_usage(text, "_ZN5vihds"), {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur in out:
            lds[cur] = int(m.group(1))
    return {k: (v[0], v[1], lds[k]) for k, v in out.items()}


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", SM.MODELS, ids=lambda c: c.__name__)
def test_substep_kernels_compile_without_scratch(tmp_path, cls):
    """The staged forward, the unstaged forward and the adjoint of every fixed-grid solver the model takes compile for gfx950
    and spill nothing; the adjoint's static LDS is (m - 1) * N rows of 256 floats, the forwards declare
    none.  VGPRs and LDS are printed (DESIGN.md quotes them).  DenseEightSub8 is the worst case MAX_SUBSTEPS stands for."""
    header = tmp_path / "sub.hpp"
    header.write_text(G.generate_source(cls))
    solvers = SM.solvers_of(cls)
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(substeps<VIHDS_GEN_CORE>::value == %d && substeps<WithPrec<VIHDS_GEN_CORE>>::value == 1);" % cls.substeps,
             "static_assert(substeps<PrprConstant>::value == 1 && substeps<BlackboxIcml>::value == 1);",
             "static_assert(kMaxSubsteps == %d);" % G.MAX_SUBSTEPS]
    for s in solvers:
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s]]
    usage = _usage_with_lds(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "sub"))
    assert len(usage) == 3 * len(solvers), sorted(usage)
    rows = (cls.substeps - 1) * len(cls.species)
    for s in solvers:
        tag = "Li%dELb" % hip.SOLVERS[s]
        fwd = [v for n, v in usage.items() if "ode_fwd_kernel" in n and tag in n]
        (bwd,) = [v for n, v in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s m=%d %s: forward %d / %d VGPRs, adjoint %d VGPRs and %d bytes of LDS"
              % (cls.__name__, cls.substeps, s, fwd[0][0], fwd[1][0], bwd[0], bwd[2]))
        assert len(fwd) == 2 and all(v[2] == 0 for v in fwd)
        assert bwd[2] == rows * 256 * 4
    for name, (vgpr, scratch, lds) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_substepped_launcher_holds_the_fixed_grid_kernels_only(tmp_path):
    """launch_ode with every solver in one unit.  PrprForcedSub4 holds the fifteen kernel names of PrprForced and
    PrprForcedImplicitSub2 the eighteen of PrprForcedImplicit (the struct's name aside); a sub-stepped model without forcings
    holds fifteen too -- no kernel of an adaptive pair, no one-pass summaries."""
    names = {}
    for cls in (FM.PrprForced, SM.PrprForcedSub4, IM.PrprForcedImplicit, SM.PrprForcedImplicitSub2, SM.PlateReaderSub3):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        struct = "GenModel_" + G._ident(cls.model_key)
        assert all(struct in n for n in usage)
        names[cls] = sorted(n.replace("%d%s" % (len(struct), struct), "M") for n in usage)
        assert all("ode_fwd_kernel" in n or "ode_bwd_kernel" in n for n in names[cls]), names[cls]
    assert len(names[FM.PrprForced]) == 15 and names[SM.PrprForcedSub4] == names[FM.PrprForced]
    assert len(names[IM.PrprForcedImplicit]) == 18 and names[SM.PrprForcedImplicitSub2] == names[IM.PrprForcedImplicit]
    assert names[SM.PlateReaderSub3] == names[FM.PrprForced]


# ---- the sub-step times, in a stand-alone host program under sanitizers ----------------------------------------------------------
PROGRAM = r"""
// reads intervals "t0 t1 h0" and prints, for m = 1 .. 8, one line "m fixed_step s_0 .. s_m"
#include <cstdio>
#include "vihds_substeps.hpp"
template <int MS>
static void run(float t0, float t1, float h0) {
  const vihds::SubGrid<MS> sg(t0, t1);
  std::printf("%d %.9g", MS, vihds::SubGrid<MS>::fixed_step(h0));
  for (int j = 0; j <= MS; ++j) std::printf(" %.9g", sg.at(j));
  std::printf("\n");
}
int main() {
  static_assert(vihds::kMaxSubsteps == 8, "one call per m below");
  float t0, t1, h0;
  while (std::scanf("%f %f %f", &t0, &t1, &h0) == 3) {
    run<1>(t0, t1, h0); run<2>(t0, t1, h0); run<3>(t0, t1, h0); run<4>(t0, t1, h0);
    run<5>(t0, t1, h0); run<6>(t0, t1, h0); run<7>(t0, t1, h0); run<8>(t0, t1, h0);
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


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_substep_times_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/vihds_substeps.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own.  On the
    ragged grid, the piecewise grid and a long uniform one, for m = 1 .. 8: s_0 == t_k and s_m == t_k+1 exactly (float32
    bits), the times strictly increase, each is within one float32 rounding of t_k + j (t_k+1 - t_k) / m, and modeuler's
    fixed step is h0 * (1.f / m)."""
    src, exe = tmp_path / "subgrid.cpp", tmp_path / "subgrid"
    src.write_text(PROGRAM)
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    grids = [np.float32(RAGGED), np.float32(SM.TIMES), np.float32(0.06) * np.arange(200, dtype=np.float32),
             np.float32([1e3, 1e3 + 1e-3, 1e3 + 0.5])]
    cases = [(g[k], g[k + 1], g[1] - g[0]) for g in grids for k in range(len(g) - 1)]
    text = "".join("%.9g %.9g %.9g\n" % c for c in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == 8 * len(cases)
    for q, row in enumerate(rows):
        t0, t1, h0 = cases[q // 8]
        v = row.split()
        m, fixed, s = int(v[0]), np.float32(v[1]), np.float32(v[2:])
        assert m == q % 8 + 1 and len(s) == m + 1
        assert s[0] == t0 and s[m] == t1, (t0, t1, m, s)
        assert bool((s[1:] > s[:-1]).all()), (t0, t1, m, s)
        assert fixed == np.float32(h0 * (np.float32(1.0) / np.float32(m)))
        exact = float(t0) + np.arange(m + 1) * (float(t1) - float(t0)) / m
        assert float(np.abs(s.astype(np.float64) - exact).max()) <= 2.0 * float(np.spacing(np.float32(max(abs(t0), abs(t1)))))
