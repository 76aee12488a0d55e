"""CPU tests of `implicit = True` in vihds.modelgen and of the backward-Euler solver's host-side parts: the generated Jacobian
against autograd, the generated text (and the unchanged text of every class without it), the refusals, compilation for
gfx950 (scratch and VGPRs of the implicit kernels; the kernel set of a launcher without them), the elimination of
csrc/vihds_implicit.hpp in a stand-alone host program under the address and undefined-behaviour sanitizers, the
implicit-function adjoint against autograd through the unrolled Newton iteration, the preconditions of the GPU comparisons
on the float64 yardstick alone, and the host checks that run before anything is built or queued."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G, ops
from vihds.utils import attrify

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_models as MM
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_observe_host import _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


class EveryImplicit(MM.EveryOperation):
    """Every operation's adjoint rule inside a Jacobian."""
    model_key = "gen_every_operation_implicit"
    implicit = True


EVERY_BASE = {"r": 0.5, "k": 1.2, "n": 1.5, "h": 0.3, "init_x": 0.4}


# ---- the generated Jacobian -----------------------------------------------------------------------------------------------------
def _jacobian_errors(cls, th, cond, times, states):
    rhs, _ = IM.torch_rhs(cls, th, cond, times)
    worst = 0.0
    for t, y in states:
        auto = IM.autograd_jacobian(rhs, t, y)
        gen = cls.torch_jacobian(y, th, cond, t=t, times=times if cls.forcings else None)
        assert gen.shape == auto.shape == y.shape + (y.shape[-1],)
        scale = auto.abs().amax((-1, -2), keepdim=True)
        assert float(scale.min()) > 0.0
        worst = max(worst, float(((gen - auto).abs() / scale).max()))
    return worst


@pytest.mark.parametrize("cls", IM.MODELS, ids=lambda c: c.__name__)
def test_generated_jacobian_equals_autograd(cls):
    """torch_jacobian (the DAG nodes rhs_jac is emitted from) against autograd of torch_problem's right-hand side in float64,
    at random states and at the states of a short backward-Euler trajectory, between and on grid points: 1e-12 of each
    trajectory's largest entry."""
    B, S = 3, 7
    pb = IM.problem(cls, B, S)
    N = len(cls.species)
    gen = torch.Generator().manual_seed(5)
    xs, _ = IM.beuler(cls, pb["th"], pb["cond"], pb["times"][:4])
    states = [(pb["times"][k], xs[..., k]) for k in range(4)]
    states += [(0.5 * (pb["times"][k] + pb["times"][k + 1]), 0.1 + torch.rand(B, S, N, generator=gen, dtype=F64)) for k in (0, 2, 6)]
    e = _jacobian_errors(cls, pb["th"], pb["cond"], pb["times"], states)
    print("%s: generated Jacobian against autograd %.2e" % (cls.__name__, e))
    assert e <= 1e-12


def test_generated_jacobian_of_every_operation():
    B, S = 2, 6
    gen = torch.Generator().manual_seed(6)
    th = {n: v * torch.exp(0.2 * torch.randn(B, S, generator=gen, dtype=F64)) for n, v in EVERY_BASE.items()}
    cond = torch.log1p(torch.tensor([[0.4], [1.1]], dtype=F64))
    states = [(torch.tensor(t, dtype=F64), lo + (hi - lo) * torch.rand(B, S, 4, generator=gen, dtype=F64))
              for t, lo, hi in ((0.0, 0.1, 0.9), (0.7, -0.9, 0.9), (1.3, 1.1, 2.0))]  # (inside, across and outside clamp's bounds)
    states = [(t, torch.cat([y[..., :1].abs() + 0.1, y[..., 1:]], dim=-1)) for t, y in states]  # (pow's base stays positive)
    e = _jacobian_errors(EveryImplicit, th, cond, None, states)
    print("EveryOperation: generated Jacobian against autograd %.2e" % e)
    assert e <= 1e-12


def test_structural_non_zeros():
    counts = {cls.__name__: sum(map(sum, G.jacobian_pattern(cls))) for cls in (IM.PrprImplicit, IM.DrImplicit, EveryImplicit)}
    assert counts == {"PrprImplicit": 11, "DrImplicit": 19, "EveryImplicit": 7}
    assert sum(map(sum, G.jacobian_pattern(IM.DenseEight))) == 64 and sum(map(sum, G.jacobian_pattern(IM.FastBinding))) == 11


# ---- generated text -------------------------------------------------------------------------------------------------------------
def test_generated_text():
    for cls in IM.MODELS + [EveryImplicit]:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)
        N = len(cls.species)
        pattern = G.jacobian_pattern(cls)
        mask = sum(1 << (i * N + j) for i in range(N) for j in range(N) if pattern[i][j])
        assert "static constexpr int NEWTON = %d;" % cls.newton_iterations in src
        assert "static constexpr unsigned long long JAC_NZ = 0x%xull;" % mask in src
        assert "__device__ static void rhs_jac(float t, const float* y, const float* p, const float*, float* J) {" in src
        body = _member(src, "rhs_jac")
        for i in range(N):
            for j in range(N):
                zero = "J[%d] = 0.f;" % (i * N + j)
                assert (zero in body) != pattern[i][j], (cls.__name__, i, j)
                assert body.count("J[%d] = " % (i * N + j)) == 1
        # without the three additions the text is the parent's, with its key
        parent = [k for k in cls.__mro__[1:] if k.__dict__.get("model_key")]
        if parent and not parent[0].implicit:
            plain = G.generate_source(parent[0])
            assert "rhs_jac" not in plain and "NEWTON" not in plain and "JAC_NZ" not in plain
            for m in ("rhs", "rhs_vjp", "prepare", "prepare_vjp", "init", "init_vjp"):
                assert _member(src, m) == _member(plain, m), (cls.__name__, m)
    assert IM.FastBinding.newton_iterations == 6 and IM.PrprImplicit.newton_iterations == 4 and not G.GeneratedOdeModel.implicit
    # the forced model's Jacobian reads the interpolant as rhs does
    tr = IM.PrprForcedImplicit._trace
    at_t = "(p[%d] + (t - p[%d]) * p[%d])" % (tr.F0, tr.F0 + 2, tr.F0 + 1)
    assert at_t in _member(G.generate_source(IM.PrprForcedImplicit), "rhs")
    assert "p[%d]" % tr.F0 not in _member(G.generate_source(IM.PrprForcedImplicit), "rhs_jac")  # (dYFP/dy does not read the light)


def test_classes_without_implicit_generate_the_recorded_text():
    import importlib

    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        for key, digest in json.load(f).items():
            cname, neural = key.split(":")
            text = G.generate_source(getattr(MM, cname), bool(int(neural)))
            assert hashlib.sha256(text.encode()).hexdigest() == digest, key
            assert "rhs_jac" not in text and "NEWTON" not in text and "JAC_NZ" not in text
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256_all.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 29
    for key, digest in recorded.items():
        path, neural = key.split(":")
        module, cname = path.rsplit(".", 1)
        text = G.generate_source(getattr(importlib.import_module(module), cname), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "rhs_jac" not in text and "NEWTON" not in text


def test_refusals():
    six = lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5  # noqa: E731
    assert _define("implicit_ok", implicit=True, rhs=six).implicit is True
    with pytest.raises(G.ModelDefinitionError, match="implicit = True and networks"):
        _define("implicit_net", implicit=True, networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    ok = _define("implicit_for_neural", implicit=True, rhs=six)
    with pytest.raises(G.ModelDefinitionError, match="precision ODE of NeuralPrecisions has no generated Jacobian"):
        G.generate_source(ok, True)
    assert G.MAX_IMPLICIT_STATES == 8
    nine = dict(species=["s%d" % k for k in range(9)], initial_state=lambda self, th, c: [th.init_x] + [0.0] * 8,
                rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 8)
    assert _define("nine_explicit", **nine).implicit is False
    with pytest.raises(G.ModelDefinitionError, match="at most 8"):
        _define("nine_implicit", implicit=True, **nine)
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(G.ModelDefinitionError, match="newton_iterations"):
            _define("implicit_newton_%s" % bad, implicit=True, newton_iterations=bad, rhs=six)
    for good in (1, 8):
        assert "NEWTON = %d;" % good in G.generate_source(_define("implicit_newton_ok_%d" % good, implicit=True,
                                                                   newton_iterations=good, rhs=six))
    with pytest.raises(G.ModelDefinitionError, match="implicit must be True or False"):
        _define("implicit_int", implicit=1, rhs=six)
    _define("explicit_any_newton", newton_iterations=99, rhs=six)  # (read by an implicit class only)


def test_docstring_has_an_implicit_paragraph():
    for word in ("Implicit models.", "implicit = True", "newton_iterations", "rhs_jac", "beuler", "MAX_IMPLICIT_STATES",
                 "torch_jacobian", "pivot"):
        assert word in G.__doc__, word


# ---- the preconditions of the GPU comparisons, on the float64 yardstick alone ---------------------------------------------------
@pytest.mark.parametrize("cls", IM.MODELS, ids=lambda c: c.__name__)
def test_newton_has_converged_at_the_test_inputs(cls):
    """The kernel's adjoint is that of the CONVERGED step; the yardstick's iterate is its own.  They are the same number where
    the last of the NEWTON increments is at rounding level: at most 1e-9 of the state, at both shapes of the GPU tests."""
    for B, S in ((3, 5), (3, 100)):
        pb = IM.problem(cls, B, S)
        xs, last = IM.beuler(cls, pb["th"], pb["cond"], pb["times"])
        print("%s %dx%d: last Newton increment %.2e" % (cls.__name__, B, S, last))
        assert bool(torch.isfinite(xs).all()) and last <= 1e-9
    pb = IM.problem(IM.PrprForcedImplicit, 3, 100, times=RAGGED, r_scale=RAGGED_R)
    assert IM.beuler(IM.PrprForcedImplicit, pb["th"], pb["cond"], pb["times"])[1] <= 1e-9


RAGGED = [0.0, 0.1, 0.7, 0.9, 1.9, 2.0, 2.8, 3.0, 3.7]  # (tests/test_modelgen_forcing_gpu.py)
RAGGED_R = 0.25  # growth rates of 0.25 exp(0.2 eps): h * rate stays below 0.5 on steps of up to 1.0


def test_the_stiff_inputs_are_stiff():
    """FastBinding at its draws on TIMES: the 3/8 rule is non-finite in every row, backward Euler finite everywhere; fewer
    Newton iterations than its six are not converged."""
    cls = IM.FastBinding
    assert IM.grid_of(cls) is IM.TIMES
    for B, S in ((3, 5), (3, 100)):
        pb = IM.problem(cls, B, S)
        rhs, x0 = IM.torch_rhs(cls, pb["th"], pb["cond"], pb["times"])
        explicit = IM.rk4_38(rhs, x0, pb["times"])
        assert not bool(torch.isfinite(explicit).all(3).all(2).any())
        assert float(pb["th"]["kon"].max() / pb["th"]["kon"].min()) > 10.0
    worst = {k: IM.beuler(cls, pb["th"], pb["cond"], pb["times"], newton=k)[1] for k in (3, 4, 6)}
    print("last increment after 3 / 4 / 6 iterations: %.1e / %.1e / %.1e" % (worst[3], worst[4], worst[6]))
    assert worst[6] <= 1e-12 < worst[3]


def test_the_hand_written_fast_binding_is_the_model():
    pb = IM.problem(IM.FastBinding, 3, 5)
    rhs, x0 = IM.torch_rhs(IM.FastBinding, pb["th"], pb["cond"], pb["times"])
    y = torch.rand(3, 5, 4, generator=torch.Generator().manual_seed(2), dtype=F64)
    assert torch.allclose(IM.fast_rhs(pb["th"], y), rhs(0.0, y), rtol=1e-13, atol=0.0)
    assert torch.allclose(IM.fast_jacobian(pb["th"], y), IM.autograd_jacobian(rhs, 0.0, y), rtol=1e-12, atol=1e-13)
    assert torch.equal(x0, torch.tensor(IM.FastBinding.Y0, dtype=F64).expand(3, 5, 4))


# ---- the formula of the adjoint -------------------------------------------------------------------------------------------------
def test_implicit_function_adjoint_equals_autograd_through_the_newton_iteration():
    """float64, FastBinding: the yardstick's gradient (implicit-function theorem at the iterate, first derivatives only) against
    autograd through 30 unrolled Newton iterations per step whose Jacobians are part of the graph: 1e-8 relative per
    parameter."""
    cls = IM.FastBinding
    pb = IM.problem(cls, 2, 3, times=IM.TIMES[:5])
    ref = IM.definition(cls, pb, F64)
    th = {n: v.detach().clone().requires_grad_(True) for n, v in pb["th"].items()}
    rhs, x0 = IM.torch_rhs(cls, th, pb["cond"], pb["times"])
    jac = functools.partial(IM.autograd_jacobian, create_graph=True)
    ys, y = [x0], x0
    for k in range(pb["T"] - 1):
        y, d = IM.newton_step(rhs, pb["times"][k + 1], pb["times"][k + 1] - pb["times"][k], y, 30, jac)
        ys.append(y)
    xs = torch.stack(ys, dim=3)
    assert float((xs.detach() - ref["traj"]).abs().max()) <= 1e-13
    _, logp = IM.log_likelihood(cls, xs, th, pb["cond"], pb["obs"])
    loss = (logp * pb["G"]["logp"]).sum()
    loss.backward()
    for n, v in th.items():
        e = float((ref["g_theta"][n] - v.grad).abs().max() / v.grad.abs().max())
        print("g_theta[%s]: implicit-function adjoint against autograd through Newton %.2e" % (n, e))
        assert e <= 1e-8, n


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
    assert hip.SOLVERS["beuler"] == 9 and hip.IMPLICIT_SOLVERS == ("beuler",) and "beuler" not in hip.ADAPTIVE_SOLVERS
    message = "solver 'beuler' needs a generated model with implicit = True"
    with pytest.raises(NotImplementedError, match=message):
        ops.OdeProblemSpec("dr_constant", "beuler", {}, 1, C=2)
    monkeypatch.setitem(hip.MODELS, MM.PrprRestated.model_key, 1024)  # (a registered model without a Jacobian)
    with pytest.raises(NotImplementedError, match=message):
        ops.OdeProblemSpec(MM.PrprRestated.model_key, "beuler", {}, 1, C=0)
    for cls in (MM.PrprRestated, FM.PrprForced):
        model = cls(_config("beuler", 0))
        with pytest.raises(NotImplementedError, match=message):
            model.solve(_config("beuler", 0), torch.tensor(IM.TIMES), None, torch.zeros(3, 0), None)
    assert MM.PrprRestated.model_key not in hip.GENERATED_IMPLICIT


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", IM.MODELS, ids=lambda c: c.__name__)
def test_implicit_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of VIHDS_SOLVER_BEULER compile for gfx950 and spill nothing (VGPRs
    printed; recorded in DESIGN.md).  DenseEight is the worst case the cap MAX_IMPLICIT_STATES stands for."""
    header = tmp_path / "implicit.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(has_jacobian<VIHDS_GEN_CORE>::value && !has_jacobian<WithPrec<VIHDS_GEN_CORE>>::value);",
             "static_assert(!has_jacobian<PrprConstant>::value && !has_jacobian<BlackboxIcml>::value);",
             "static_assert(solver_is_implicit(VIHDS_SOLVER_BEULER) && !solver_is_adaptive(VIHDS_SOLVER_BEULER));",
             "static_assert(VIHDS_GEN_CORE::N <= kMaxImplicitStates && kMaxImplicitStates == %d);" % G.MAX_IMPLICIT_STATES,
             "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, true>(OdeArgs);",
             "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, false>(OdeArgs);",
             "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_BEULER, false>(OdeArgs);", "}"]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", "implicit"), "_ZN5vihds")
    assert len(usage) == 3, sorted(usage)
    for kind in ("ode_fwd_kernel", "ode_bwd_kernel"):
        vgprs = [v for name, (v, _) in usage.items() if kind in name]
        print("%s %s beuler: %d .. %d VGPRs" % (cls.__name__, kind, min(vgprs), max(vgprs)))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_only_an_implicit_model_holds_the_implicit_kernels(tmp_path):
    """launch_ode with every solver in one unit: PrprForced holds the fifteen fixed-grid kernels it held before, none of solver
    9; PrprForcedImplicit holds those and three more."""
    counts = {}
    for cls in (FM.PrprForced, IM.PrprForcedImplicit):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        assert all("ode_fwd_kernel" in n or "ode_bwd_kernel" in n for n in usage), sorted(usage)
        counts[cls] = (len(usage), sum("Li%dELb" % hip.SOLVERS["beuler"] in n for n in usage))
    assert counts == {FM.PrprForced: (15, 0), IM.PrprForcedImplicit: (18, 3)}, counts


# ---- the elimination, in a stand-alone host program under sanitizers -------------------------------------------------------------
PROGRAM = r"""
// reads cases "N sparse transpose h, J[N N], b[N]" and prints the solution of (I - h J) x = b (transpose: of its transpose)
#include <cstdio>
#include <vector>
#include "vihds_implicit.hpp"
template <int N, unsigned long long NZ>
static void run(bool transpose, float h, const std::vector<float>& J, std::vector<float>& b) {
  if (transpose) vihds::implicit_solve<N, NZ, true>(h, J.data(), b.data());
  else vihds::implicit_solve<N, NZ, false>(h, J.data(), b.data());
}
int main() {
  int n, sparse, transpose;
  float h;
  while (std::scanf("%d %d %d %f", &n, &sparse, &transpose, &h) == 4) {
    std::vector<float> J(n * n), b(n);
    for (float& v : J) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : b) if (std::scanf("%f", &v) != 1) return 2;
    if (sparse && n == 4) run<4, FAST_MASK>(transpose != 0, h, J, b);
    else if (n == 1) run<1, vihds::dense_pattern(1)>(transpose != 0, h, J, b);
    else if (n == 2) run<2, vihds::dense_pattern(2)>(transpose != 0, h, J, b);
    else if (n == 4) run<4, vihds::dense_pattern(4)>(transpose != 0, h, J, b);
    else if (n == 8) run<8, vihds::dense_pattern(8)>(transpose != 0, h, J, b);
    else return 3;
    for (int i = 0; i < n; ++i) std::printf("%.9g%c", b[i], i + 1 < n ? ' ' : '\n');
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
def test_elimination_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/vihds_implicit.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own, which solves
    (I - h J) x = b and the transposed system for N = 1, 2, 4, 8 on diagonally dominant random matrices and on FastBinding's
    Newton matrices (dense pattern and the model's own sparse one).  Against numpy in float64; the bound per case is 8 x the
    error of numpy's float32 solve (pivoted), floored at 1e-6 -- both printed."""
    pattern = G.jacobian_pattern(IM.FastBinding)
    mask = sum(1 << (i * 4 + j) for i in range(4) for j in range(4) if pattern[i][j])
    src, exe = tmp_path / "solve.cpp", tmp_path / "solve"
    src.write_text(PROGRAM)
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-DFAST_MASK=0x%xull" % mask, "-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    rng = np.random.RandomState(3)
    cases = []
    for n in (1, 2, 4, 8):
        for transpose in (0, 1):
            for _ in range(4):
                J = rng.randn(n, n) - np.diag(n + 3.0 * rng.rand(n))  # (I - h J: dominant diagonal)
                cases.append((n, 0, transpose, 0.1 + 0.5 * rng.rand(), J, rng.randn(n)))
    pb = IM.problem(IM.FastBinding, 3, 100)
    xs, _ = IM.beuler(IM.FastBinding, pb["th"], pb["cond"], pb["times"])
    rhs, _ = IM.torch_rhs(IM.FastBinding, pb["th"], pb["cond"], pb["times"])
    for k in (1, 4, 8):
        J = IM.autograd_jacobian(rhs, pb["times"][k], xs[..., k]).reshape(-1, 4, 4).numpy()
        order = np.argsort(-np.abs(J).max((1, 2)))
        for row in list(order[:3]) + list(order[-2:]):  # (the stiffest rows and the mildest)
            for sparse in (0, 1):
                for transpose in (0, 1):
                    cases.append((4, sparse, transpose, float(pb["times"][k] - pb["times"][k - 1]), J[row], rng.randn(4)))
    text = "".join("%d %d %d %.9g\n%s\n%s\n" % (n, sp, tr, h, " ".join("%.9g" % v for v in J.reshape(-1)),
                                                " ".join("%.9g" % v for v in b)) for n, sp, tr, h, J, b in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(cases)
    worst = (0.0, 0.0)
    for (n, sp, tr, h, J, b), row in zip(cases, rows):
        J32, b32, h32 = J.astype(np.float32), b.astype(np.float32), np.float32(h)  # (the program's inputs, exactly)
        A = np.eye(n) - float(h32) * J32.astype(np.float64)
        A = A.T if tr else A
        exact = np.linalg.solve(A, b32.astype(np.float64))
        pivoted = np.linalg.solve(A.astype(np.float32), b32).astype(np.float64)
        got = np.array([float(v) for v in row.split()])
        scale = np.abs(exact).max()
        e_got, e_piv = np.abs(got - exact).max() / scale, np.abs(pivoted - exact).max() / scale
        if e_got > worst[0]:
            worst = (e_got, e_piv)
        assert e_got <= max(1e-6, 8.0 * e_piv), (n, sp, tr, e_got, e_piv)
    print("%d solves: worst unpivoted float32 error %.2e (numpy's pivoted float32 solve there: %.2e)" % ((len(cases),) + worst))
