"""CPU tests of `implicit_order = 2` in vihds.modelgen and of the two-stage SDIRK's host-side parts: the attribute's refusals,
the generated text (one more line, and the unchanged text of every class without it), the unchanged solver tables, the order of
the float64 definition, its written-out adjoint against autograd through the Newton iterations, the preconditions of the GPU
comparisons on the float64 yardstick alone, compilation for gfx950 (scratch and VGPRs of the kernels of solver 9; the kernel
set of a launcher), and sdirk2_step / sdirk2_step_vjp of csrc/vihds_implicit.hpp in a stand-alone host program under the
address and undefined-behaviour sanitizers."""
import hashlib
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G

import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_leadin_models as LM
import modelgen_sdirk_models as DM
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_implicit_host import CSRC, HIPCC, RAGGED, RAGGED_R, ROOT, _host_compiler

F64 = torch.float64
EARLIER_MODULES = ["modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models",
                   "modelgen_implicit_models", "modelgen_substep_models"]
SIX = lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5  # noqa: E731


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _digest(cls, neural=False):
    return hashlib.sha256(G.generate_source(cls, neural).encode()).hexdigest()


# ---- the attribute ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    assert G.GeneratedOdeModel.implicit_order == 1
    assert _define("sdirk_ok", implicit=True, implicit_order=2, rhs=SIX).implicit_order == 2
    assert _define("sdirk_one", implicit=True, implicit_order=1, rhs=SIX).implicit_order == 1
    assert _define("sdirk_explicit_one", implicit_order=1, rhs=SIX).implicit is False
    with pytest.raises(G.ModelDefinitionError, match="implicit_order = 2 without implicit = True"):
        _define("sdirk_explicit", implicit_order=2, rhs=SIX)
    for implicit in (True, False):
        for bad in (True, False, 0, 3, -1, 2.0, 1.0, "2", None):
            with pytest.raises(G.ModelDefinitionError, match="implicit_order"):
                _define("sdirk_bad_%s_%s" % (implicit, bad), implicit=implicit, implicit_order=bad, rhs=SIX)
    # everything `implicit` refuses stays refused
    with pytest.raises(G.ModelDefinitionError, match="implicit = True and networks"):
        _define("sdirk_net", implicit=True, implicit_order=2, networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="precision ODE of NeuralPrecisions has no generated Jacobian"):
        G.generate_source(_define("sdirk_for_neural", implicit=True, implicit_order=2, rhs=SIX), True)
    with pytest.raises(G.ModelDefinitionError, match="at most 8"):
        _define("sdirk_nine", implicit=True, implicit_order=2, species=["s%d" % k for k in range(9)],
                initial_state=lambda self, th, c: [th.init_x] + [0.0] * 8, rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 8)
    for bad in (0, 9):
        with pytest.raises(G.ModelDefinitionError, match="newton_iterations"):
            _define("sdirk_newton_%d" % bad, implicit=True, implicit_order=2, newton_iterations=bad, rhs=SIX)


def test_docstring_describes_the_order():
    for word in ("implicit_order = 2", "SDIRK", "L-stable", "fmaf(gamma, h, t0)", "fmaf(c, z1 - y_k, y_k)", "mu1", "mu2",
                 "GENERATED_IMPLICIT_ORDER", "IMPLICIT_ORDER = 2"):
        assert word in G.__doc__, word


def test_generated_text():
    """One more line, IMPLICIT_ORDER = 2, and only at order 2: apart from it (and the names) the text is the order-1 twin's."""
    line = "  static constexpr int IMPLICIT_ORDER = 2;  // the two-stage SDIRK of vihds_implicit.hpp\n"
    for cls in DM.MODELS:
        src, twin = G.generate_source(cls), G.generate_source(DM.TWIN[cls])
        assert src == G.generate_source(cls)
        assert src.count("IMPLICIT_ORDER") == 1 and src.count(line) == 1 and "IMPLICIT_ORDER" not in twin
        assert "static constexpr int NEWTON = %d;" % cls.newton_iterations in src
        rest = src.replace(line, "")
        if cls is DM.FastBindingSdirkSub2:
            rest = rest.replace("  static constexpr int SUBSTEPS = 2;\n", "")
        same = lambda text, c: text.replace(c.__qualname__, "X").replace(c.model_key, "X")  # noqa: E731
        strip = lambda text, c: "\n".join(l for l in same(text, c).splitlines() if not l.startswith("//"))  # noqa: E731
        assert strip(rest, cls) == strip(twin, DM.TWIN[cls]), cls.__name__
    a = G.generate_source(_define("sdirk_text", implicit=True, implicit_order=2, rhs=SIX))
    b = G.generate_source(_define("sdirk_text", implicit=True, rhs=SIX))
    assert a.replace(line, "") == b and a != b
    recorded = _golden("modelgen_sdirk_source_sha256.json")
    assert sorted(recorded) == sorted(cls.__name__ for cls in DM.MODELS)
    for cls in DM.MODELS:
        assert _digest(cls) == recorded[cls.__name__], cls.__name__


def test_classes_without_the_attribute_generate_the_recorded_text():
    """Every (class, neural) of the earlier PREBUILT lists generates the text it generated: the digests recorded before the
    attribute existed (tests/golden/modelgen_jump_source_sha256.json, "without" and "with", and modelgen_leadin_source_sha256.json)."""
    jump, lead = _golden("modelgen_jump_source_sha256.json"), _golden("modelgen_leadin_source_sha256.json")
    seen = set()
    for m in EARLIER_MODULES:
        for cls, neural in importlib.import_module(m).PREBUILT:
            key = "%s.%s:%d" % (m, cls.__name__, int(neural))
            assert _digest(cls, neural) == jump["without"][key], key
            assert "IMPLICIT_ORDER" not in G.generate_source(cls, neural)
            seen.add(key)
    assert seen == set(jump["without"]) and len(seen) == 39
    for cls, neural in JM.PREBUILT:
        assert not neural and _digest(cls) == jump["with"][cls.__name__], cls.__name__
    assert sorted(jump["with"]) == sorted(cls.__name__ for cls in JM.MODELS)
    for cls, neural in LM.PREBUILT:
        assert not neural and _digest(cls) == lead[cls.__name__], cls.__name__
    assert sorted(lead) == sorted(cls.__name__ for cls in LM.MODELS)


def test_the_solver_tables_are_unchanged():
    assert hip.SOLVERS == {"modeuler": 0, "modeulerwhile": 1, "euler": 2, "midpoint": 3, "rk4": 4, "dopri5": 5, "bosh3": 6,
                           "adaptive_heun": 7, "dopri8": 8, "beuler": 9}
    assert hip.IMPLICIT_SOLVERS == ("beuler",)
    assert hip.ADAPTIVE_SOLVERS == ("dopri5", "bosh3", "adaptive_heun", "dopri8")
    assert isinstance(hip.GENERATED_IMPLICIT_ORDER, dict) and isinstance(hip.GENERATED_IMPLICIT, set)


def test_register_kernel_records_the_order(monkeypatch):
    class _Lib:
        def vihds_model_register(self, path):
            return 1500

    monkeypatch.setattr(G, "ensure_library", lambda source: "/nowhere/lib.so")
    monkeypatch.setattr(hip, "lib", lambda: _Lib())
    for name in ("MODELS", "GENERATED_NETWORKS", "GENERATED_SUBSTEPS", "GENERATED_IMPLICIT_ORDER", "GENERATED_LEAD_IN"):
        monkeypatch.setattr(hip, name, dict(getattr(hip, name)))
    for name in ("GENERATED_IMPLICIT", "GENERATED_OWN_PRECISION", "GENERATED_JUMP", "GENERATED_START"):
        monkeypatch.setattr(hip, name, set(getattr(hip, name)))
    monkeypatch.setattr(G, "_REGISTERED", {})
    two = _define("sdirk_registered_two", implicit=True, implicit_order=2, rhs=SIX)
    one = _define("sdirk_registered_one", implicit=True, rhs=SIX)
    none = _define("sdirk_registered_none", rhs=SIX)
    for cls in (two, one, none):
        assert G.register_kernel(cls) == 1500
    assert hip.GENERATED_IMPLICIT_ORDER == {"sdirk_registered_two": 2, "sdirk_registered_one": 1}
    assert hip.GENERATED_IMPLICIT == {"sdirk_registered_two", "sdirk_registered_one"}


# ---- the float64 definition -------------------------------------------------------------------------------------------------------
def test_the_definition_is_second_order():
    """PrprSdirk (not stiff) on the first four intervals of its grid refined 2, 4 and 8 times, against the same scheme on the grid
    refined 64 times: halving the step divides the error by 3.5 .. 4.5, twice.  (The ratio tends to 4 as the step shrinks: on the
    grid itself, steps of up to 0.2, the third-order term still shows and the first ratio is 4.8 -- printed.)"""
    cls = DM.PrprSdirk
    pb = DM.problem(cls, 3, 5)
    times = pb["times"][:5]
    run = lambda m: DM.sdirk2_states(cls, pb["th"], pb["cond"], times, newton=8, m=m)[0]  # noqa: E731
    fine = run(64)
    err = [float((run(m) - fine).abs().max()) for m in (1, 2, 4, 8)]
    print("error at m = 1, 2, 4, 8: %.3e %.3e %.3e %.3e (ratios %.2f, %.2f, %.2f)"
          % (tuple(err) + (err[0] / err[1], err[1] / err[2], err[2] / err[3])))
    assert 3.5 <= err[1] / err[2] <= 4.5 and 3.5 <= err[2] / err[3] <= 4.5


def test_the_constants():
    g, c = np.float32(1.0 - np.sqrt(2.0) / 2.0), np.float32(1.0 + np.sqrt(2.0))
    assert DM.GAMMA == float(g) and DM.C == float(c)
    assert "%.8g" % g == "0.29289323" and "%.8g" % c == "2.4142137"
    with open(os.path.join(CSRC, "vihds_implicit.hpp")) as f:
        text = f.read()
    assert "kSdirk2Gamma = 0.29289323f;" in text and "kSdirk2C = 2.4142137f;" in text


@pytest.mark.parametrize("cls", [DM.FastBindingSdirk, DM.PrprForcedSdirk] + DM.COMBINED, ids=lambda c: c.__name__)
def test_written_out_adjoint_equals_autograd_through_the_newton_iteration(cls):
    """float64: the yardstick's gradient (the written-out adjoint at the iterate, first derivatives only) against autograd through
    12 Newton iterations per stage whose Jacobians are part of the graph: 1e-8 relative per theta row."""
    pb = DM.problem(cls, 2, 3)
    ref, auto = DM.definition(cls, pb, F64), DM.by_autograd(cls, pb, 12)
    assert ref["last_increment"] <= 1e-9 and float((auto["traj"] - ref["traj"]).abs().max()) <= 1e-12
    for n, g in auto["g_theta"].items():
        if float(g.abs().max()) == 0.0:
            assert float(ref["g_theta"][n].abs().max()) == 0.0, n
            continue
        e = float((ref["g_theta"][n] - g).abs().max() / g.abs().max())
        print("%s g_theta[%s]: written-out adjoint against autograd through Newton %.2e" % (cls.__name__, n, e))
        assert e <= 1e-8, n


@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_newton_has_converged_at_the_test_inputs(cls):
    """The precondition of the GPU comparisons on the float64 run alone, at both of their shapes: every stage's last Newton
    increment is at most 1e-9 of the state and everything is finite."""
    for B, S in ((3, 5), (3, 100)):
        pb = DM.problem(cls, B, S)
        xs, _, _, last = DM.sdirk2_states(cls, pb["th"], pb["cond"], pb["times"])
        print("%s %dx%d: last Newton increment %.2e, smallest state %.2e" % (cls.__name__, B, S, last, float(xs.min())))
        assert bool(torch.isfinite(xs).all()) and last <= 1e-9
    if cls is DM.PrprForcedSdirk:
        pb = DM.problem(cls, 3, 100, times=RAGGED, r_scale=RAGGED_R)
        assert DM.sdirk2_states(cls, pb["th"], pb["cond"], pb["times"])[3] <= 1e-9


def test_the_hand_written_stiff_run_is_the_definition_and_is_not_backward_euler():
    """fast_sdirk2 (the refined solutions of the GPU tests) is the generic definition; against its 64 times refined run the
    definition is at least 4 times closer than backward Euler on the same grid."""
    cls = DM.FastBindingSdirk
    pb = DM.problem(cls, 3, 100)
    xs = DM.sdirk2_states(cls, pb["th"], pb["cond"], pb["times"])[0]
    assert float((DM.fast_sdirk2(pb["th"], pb["times"]) - xs).abs().max()) <= 1e-12
    fine = DM.fast_sdirk2(pb["th"], pb["times"], refine=64, newton=3)  # (three iterations there leave 4e-8)
    e2 = float((xs - fine).abs().max())
    e1 = float((IM.beuler(IM.FastBinding, pb["th"], pb["cond"], pb["times"])[0] - fine).abs().max())
    print("against the 64x refined solution: SDIRK2 %.3e, backward Euler %.3e" % (e2, e1))
    assert e1 >= 4.0 * e2


# ---- compilation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", DM.MODELS, ids=lambda c: c.__name__)
def test_sdirk_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of solver 9 compile for gfx950 for an order-2 class and spill nothing
    (VGPRs printed; recorded in DESIGN.md).  DenseEightSdirk is the worst case."""
    header = tmp_path / "sdirk.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(implicit_order<VIHDS_GEN_CORE>::value == 2 && has_jacobian<VIHDS_GEN_CORE>::value);",
             "static_assert(implicit_order<WithPrec<VIHDS_GEN_CORE>>::value == 0);",
             "static_assert(implicit_order<PrprConstant>::value == 0 && implicit_order<BlackboxIcml>::value == 0);",
             "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, true>(OdeArgs);",
             "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, false>(OdeArgs);",
             "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, false>(OdeArgs);", "}"]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", "sdirk"), "_ZN5vihds")
    assert len(usage) == 3, sorted(usage)
    for kind in ("ode_fwd_kernel", "ode_bwd_kernel"):
        vgprs = [v for name, (v, _) in usage.items() if kind in name]
        print("%s %s sdirk2: %d .. %d VGPRs" % (cls.__name__, kind, min(vgprs), max(vgprs)))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_an_order_two_model_holds_the_kernels_of_its_twin(tmp_path):
    """launch_ode with every solver in one unit: the same 18 kernels, 3 of them of solver 9, at either order; an order-1 model's
    struct answers implicit_order 1."""
    names = {}
    for cls in (IM.PrprForcedImplicit, DM.PrprForcedSdirk):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
                "static_assert(implicit_order<VIHDS_GEN_CORE>::value == %d);\n"
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % (header, cls.implicit_order))
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        assert all("ode_fwd_kernel" in n or "ode_bwd_kernel" in n for n in usage), sorted(usage)
        assert all(scratch == 0 for _, scratch in usage.values())
        sname = G.generate_source(cls).split("struct ")[1].split(" ")[0]
        names[cls] = sorted(n.replace(sname, "M").replace(str(len(sname)) + "M", "M") for n in usage)
        assert (len(usage), sum("Li%dELb" % hip.SOLVERS["beuler"] in n for n in usage)) == (18, 3), cls.__name__
    assert names[IM.PrprForcedImplicit] == names[DM.PrprForcedSdirk]


# ---- the step and its adjoint, in a stand-alone host program under sanitizers -----------------------------------------------------
PROGRAM = r"""
// reads cases "kind n t0 t1, q[..], y[n], lam[n]" and prints y_k+1, z1, the adjoint of y_k, mu1 and mu2 of one step
//   kind 0: f_i(t, z) = sum_j M_ij z_j - 0.1 z_i^3 + (1 + t) b_i, q = M[n n] b[n], the dense pattern, 4 Newton iterations
//   kind 1: FastBinding's right-hand side and Jacobian, q = kon koff prod deg a, the model's own pattern, 6 iterations
#include <cstdio>
#include <vector>
#include "vihds_implicit.hpp"
template <int N, int NEWTON, unsigned long long NZ, class F, class JF>
static void run(float t0, float t1, std::vector<float>& y, std::vector<float>& lam, F f, JF jac) {
  std::vector<float> y0(y), z1(N), mu1(N), mu2(N);
  vihds::sdirk2_step<N, NEWTON, NZ>(t0, t1, y.data(), f, jac);
  vihds::sdirk2_step_vjp<N, NEWTON, NZ>(t0, t1, y0.data(), y.data(), lam.data(), z1.data(), mu1.data(), mu2.data(), f, jac);
  const std::vector<float>* out[] = {&y, &z1, &lam, &mu1, &mu2};
  for (int k = 0; k < 5; ++k)
    for (int i = 0; i < N; ++i) std::printf("%.9g%c", (*out[k])[i], k == 4 && i + 1 == N ? '\n' : ' ');
}
template <int N>
static void run_cubic(float t0, float t1, const std::vector<float>& q, std::vector<float>& y, std::vector<float>& lam) {
  const float* M = q.data();
  const float* b = q.data() + N * N;
  run<N, 4, vihds::dense_pattern(N)>(
      t0, t1, y, lam,
      [=](float t, const float* z, float* out) {
        for (int i = 0; i < N; ++i) {
          float s = (1.f + t) * b[i] - 0.1f * z[i] * z[i] * z[i];
          for (int j = 0; j < N; ++j) s += M[i * N + j] * z[j];
          out[i] = s;
        }
      },
      [=](float, const float* z, float* J) {
        for (int i = 0; i < N; ++i)
          for (int j = 0; j < N; ++j) J[i * N + j] = M[i * N + j] - (i == j ? 0.3f * z[i] * z[i] : 0.f);
      });
}
static void run_fast(float t0, float t1, const std::vector<float>& q, std::vector<float>& y, std::vector<float>& lam) {
  const float kon = q[0], koff = q[1], prod = q[2], deg = q[3], a = q[4];
  run<4, 6, FAST_MASK>(
      t0, t1, y, lam,
      [=](float, const float* z, float* out) {
        const float bind = kon * z[0] * z[1] - koff * z[2];
        out[0] = prod - bind - deg * z[0];
        out[1] = 0.5f * prod - bind - deg * z[1];
        out[2] = bind - deg * z[2];
        out[3] = a * z[2] * z[2] / (0.25f + z[2] * z[2]) - deg * z[3];
      },
      [=](float, const float* z, float* J) {
        const float den = 0.25f + z[2] * z[2];
        const float rows[16] = {-kon * z[1] - deg, -kon * z[0], koff, 0.f, -kon * z[1], -kon * z[0] - deg, koff, 0.f,
                                kon * z[1], kon * z[0], -koff - deg, 0.f, 0.f, 0.f, a * 0.5f * z[2] / (den * den), -deg};
        for (int k = 0; k < 16; ++k) J[k] = rows[k];
      });
}
int main() {
  int kind, n;
  float t0, t1;
  while (std::scanf("%d %d %f %f", &kind, &n, &t0, &t1) == 4) {
    if (n != 1 && n != 2 && n != 4 && n != 8) return 3;
    std::vector<float> q(kind ? 5 : n * n + n), y(n), lam(n);
    for (float& v : q) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : y) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : lam) if (std::scanf("%f", &v) != 1) return 2;
    if (kind == 1 && n == 4) run_fast(t0, t1, q, y, lam);
    else if (kind != 0) return 3;
    else if (n == 1) run_cubic<1>(t0, t1, q, y, lam);
    else if (n == 2) run_cubic<2>(t0, t1, q, y, lam);
    else if (n == 4) run_cubic<4>(t0, t1, q, y, lam);
    else run_cubic<8>(t0, t1, q, y, lam);
  }
  return 0;
}
"""


def _torch_step(kind, n, t0, t1, q, y, lam, dtype):
    """The definition of modelgen_sdirk_models for one case of the program, in `dtype`: y_k+1, z1, adjoint of y_k, mu1, mu2."""
    as_t = lambda v: torch.tensor(np.asarray(v, dtype=np.float32)).to(dtype)  # noqa: E731  (the program's inputs, exactly)
    q, y, lam, t0, t1 = as_t(q), as_t(y)[None, None], as_t(lam)[None, None], as_t(t0), as_t(t1)
    if kind:
        th = {k: v.reshape(1, 1) for k, v in zip(("kon", "koff", "prod", "deg", "a"), q)}
        rhs, jac, newton = (lambda t, z: IM.fast_rhs(th, z)), (lambda f, t, z: IM.fast_jacobian(th, z)), 6
    else:
        M, b = q[:n * n].reshape(n, n), q[n * n:]
        rhs = lambda t, z: z @ M.T - 0.1 * z ** 3 + (1.0 + t) * b  # noqa: E731
        jac = lambda f, t, z: M - torch.diag_embed(0.3 * z ** 2)  # noqa: E731
        newton = 4
    y1, z1, _ = DM.sdirk2_step(rhs, t0, t1, y, newton, jac)
    lam0, mu1, mu2 = DM.sdirk2_step_adjoint(rhs, t0, t1, z1, y1, lam, jac)
    return torch.cat([v.reshape(-1) for v in (y1, z1, lam0, mu1, mu2)]).double().numpy()


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_step_and_adjoint_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/vihds_implicit.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own, which takes one
    step and its adjoint for N = 1, 2, 4, 8 on a cubic right-hand side with a dominant diagonal and for FastBinding's
    right-hand side and Jacobian written in C, at the model's stiff inputs.  Against the torch definition in float64; the bound
    per case is 8 x the error of the float32 torch run of the definition (pivoted solves), floored at 1e-6 -- both printed."""
    pattern = G.jacobian_pattern(IM.FastBinding)
    mask = sum(1 << (i * 4 + j) for i in range(4) for j in range(4) if pattern[i][j])
    src, exe = tmp_path / "step.cpp", tmp_path / "step"
    src.write_text(PROGRAM)
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-DFAST_MASK=0x%xull" % mask, "-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    rng = np.random.RandomState(4)
    cases = []
    for n in (1, 2, 4, 8):
        for _ in range(4):
            M = rng.randn(n, n) - np.diag(n + 3.0 * rng.rand(n))
            t0 = rng.rand()
            cases.append((0, n, t0, t0 + 0.1 + 0.5 * rng.rand(), np.concatenate([M.reshape(-1), rng.randn(n)]),
                          0.2 + rng.rand(n), rng.randn(n)))
    pb = DM.problem(DM.FastBindingSdirk, 3, 100)
    xs = DM.sdirk2_states(DM.FastBindingSdirk, pb["th"], pb["cond"], pb["times"])[0].reshape(-1, 4, pb["T"]).numpy()
    q_all = np.stack([pb["th"][k].reshape(-1).numpy() for k in ("kon", "koff", "prod", "deg", "a")], axis=1)
    order = np.argsort(-q_all[:, 0])
    for row in list(order[:4]) + list(order[-2:]):  # (the stiffest rows and the mildest)
        for k in (0, 3, 7):
            cases.append((1, 4, float(pb["times"][k]), float(pb["times"][k + 1]), q_all[row], xs[row, :, k], rng.randn(4)))
    text = "".join("%d %d %.9g %.9g\n%s\n" % (kind, n, t0, t1, "\n".join(" ".join("%.9g" % v for v in np.asarray(a, dtype=np.float32))
                                                                       for a in (q, y, lam)))
                   for kind, n, t0, t1, q, y, lam in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(cases)
    worst = (0.0, 0.0)
    for case, row in zip(cases, rows):
        got = np.array([float(v) for v in row.split()])
        exact, single = _torch_step(*case, dtype=F64), _torch_step(*case, dtype=torch.float32)
        assert got.shape == exact.shape == (5 * case[1],) and np.isfinite(got).all()
        for part in range(5):  # y_k+1, z1, the adjoint of y_k, mu1, mu2: each against its own size
            sl = slice(part * case[1], (part + 1) * case[1])
            scale = np.abs(exact[sl]).max()
            e_got, e_32 = np.abs(got[sl] - exact[sl]).max() / scale, np.abs(single[sl] - exact[sl]).max() / scale
            if e_got > worst[0]:
                worst = (e_got, e_32)
            assert e_got <= max(1e-6, 8.0 * e_32), (case[:4], part, e_got, e_32)
    print("%d steps: worst float32 error of the program %.2e (the float32 torch run there: %.2e)" % ((len(cases),) + worst))
