"""CPU tests of algebraic variables in vihds.modelgen (`algebraic`, `constraint`, `algebraic_start`) and of the host-side parts
of csrc/vihds_algebraic.hpp: the refusals, the generated dg/dz and its pattern against autograd, the generated text (and the
unchanged text of every class without algebraic variables), torch_algebraic against the roots written out by hand and its
precondition at the inputs of the GPU tests, the implicit-function gradient against plain autograd of the closed-form twin,
compilation for gfx950 (scratch and VGPRs of every explicit fixed-grid kernel), and the Newton loop and both solves in a
stand-alone host program under the address and undefined-behaviour sanitizers."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G

import modelgen_algebraic_models as AM
import modelgen_models as MM
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_observe_host import _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SHAPES = [(3, 5), (3, 100)]
ALL = AM.MODELS + [AM.BindingClosed]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _qss(name, **body):
    """A six-species model whose first derivative reads one algebraic variable z0 with z0 (1 + y0) = r."""
    attrs = dict(algebraic=["z0"],
                 algebraic_start=lambda self, y, p, c: [p.r],
                 constraint=lambda self, y, z, p, c: [z[0] * (1.0 + y[0]) - p.r],
                 rhs=lambda self, t, y, p, c: [p.r * y[0] - self.algebraic.z0] + [0.0] * 5)
    attrs.update(body)
    return _define(name, **attrs)


def test_refusals():
    ok = _qss("alg_ok")
    assert "N_ALGEBRAIC = 1" in G.generate_source(ok) and G.MAX_ALGEBRAIC == 4
    with pytest.raises(G.ModelDefinitionError, match="algebraic variables and implicit = True.*f_y - f_z g_z\\^-1 g_y"):
        _qss("alg_implicit", implicit=True)
    with pytest.raises(G.ModelDefinitionError, match="algebraic variables and networks"):
        _qss("alg_net", networks={"n": G.Network(1, 2, 1)},
             rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0] - self.algebraic.z0] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
        G.generate_source(ok, True)
    two = lambda n: dict(algebraic=["z%d" % k for k in range(n)],  # noqa: E731
                         algebraic_start=lambda self, y, p, c: [p.r] * n,
                         constraint=lambda self, y, z, p, c: [z[k] * (1.0 + y[0]) - p.r for k in range(n)])
    assert "N_ALGEBRAIC = 4" in G.generate_source(_qss("alg_four", **two(4)))
    with pytest.raises(G.ModelDefinitionError, match="5 algebraic variables.*at most 4"):
        _qss("alg_five", **two(5))
    with pytest.raises(G.ModelDefinitionError, match="without constraint"):
        _qss("alg_no_constraint", constraint=None)
    with pytest.raises(G.ModelDefinitionError, match="without algebraic_start"):
        _qss("alg_no_start", algebraic_start=None)
    with pytest.raises(G.ModelDefinitionError, match="constraint must return a list of 1 entries"):
        _qss("alg_long_constraint", constraint=lambda self, y, z, p, c: [z[0] - p.r, z[0]])
    with pytest.raises(G.ModelDefinitionError, match="algebraic_start must return a list of 1 entries"):
        _qss("alg_long_start", algebraic_start=lambda self, y, p, c: [p.r, p.r])
    with pytest.raises(G.ModelDefinitionError, match="constraint must be a function constraint\\(self, y, z, p, c\\)"):
        _qss("alg_bad_signature", constraint=lambda self, t, y, z, p, c: [z[0] - p.r])
    with pytest.raises(G.ModelDefinitionError, match="no residual depends on the algebraic variable 'z1'.*zero column"):
        _qss("alg_zero_column", **dict(two(2), constraint=lambda self, y, z, p, c: [z[0] - p.r, z[0] * y[0] - p.r]))
    with pytest.raises(G.ModelDefinitionError, match="residual 1 depends on no algebraic variable.*zero row"):
        _qss("alg_zero_row", **dict(two(2), constraint=lambda self, y, z, p, c: [z[0] + z[1] - p.r, y[0] - p.r]))
    with pytest.raises(G.ModelDefinitionError, match="pivot 0 would be a structural zero"):
        _qss("alg_zero_pivot", **dict(two(2), constraint=lambda self, y, z, p, c: [z[1] - p.r, z[0] - p.r]))
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(G.ModelDefinitionError, match="algebraic_iterations"):
            _qss("alg_iterations_%s" % bad, algebraic_iterations=bad)
    for good in (1, 8):
        assert "ALG_ITER = %d;" % good in G.generate_source(_qss("alg_iterations_ok_%d" % good, algebraic_iterations=good))
    with pytest.raises(G.ModelDefinitionError, match="algebraic must be a list of names"):
        _qss("alg_names", algebraic=["not a name"])
    with pytest.raises(G.ModelDefinitionError, match="also a species, a parameter or a forcing"):
        _qss("alg_clash", algebraic=["OD"])


def test_where_an_algebraic_variable_may_be_read():
    for hook, definition in (("prepare", lambda self, th, c: {"r": th.r * self.algebraic.z0}),
                             ("initial_state", lambda self, th, c: [self.algebraic.z0] + [0.0] * 5),
                             ("start", lambda self, y, p, c: [self.algebraic.z0] + [0.0] * 5),
                             ("jump", lambda self, y, p, c: [self.algebraic.z0] + [0.0] * 5),
                             ("precision", lambda self, y, x, p, c: [self.algebraic.z0] * 4),
                             ("log_likelihood", lambda self, x, obs, pr, p, c: [self.algebraic.z0] * 4)):
        with pytest.raises(G.ModelDefinitionError, match="read in %s: .*read in rhs\\(self, t, y, p, c\\) and in "
                                                         "observe\\(self, y, p, c\\) only" % hook):
            _qss("alg_read_in_%s" % hook, **{hook: definition})
    both = _qss("alg_read_in_observe", observe=lambda self, y, p, c: [y[0], self.algebraic.z0, y[1], y[2]])
    src = G.generate_source(both)
    assert "algebraic(y, p, u, z);" in _member(src, "observe") and "algebraic_vjp(y, z, p, u, zb, yb, pb);" in _member(src, "observe_vjp")
    with pytest.raises(G.ModelDefinitionError, match="unknown algebraic variable 'nope' .*declares: z0"):
        _qss("alg_unknown", rhs=lambda self, t, y, p, c: [self.algebraic.nope] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="unknown algebraic variable 'C' .*declares: none"):
        _define("alg_undeclared", rhs=lambda self, t, y, p, c: [self.algebraic.C] + [0.0] * 5)


# ---- the generated dg/dz ---------------------------------------------------------------------------------------------------------
def _states(cls, B=3, S=7):
    pb = AM.problem(cls, B, S)
    gen = torch.Generator().manual_seed(11)
    y = 0.2 + 3.0 * torch.rand(B, S, len(cls.species), generator=gen, dtype=F64)
    z = 0.05 + torch.rand(B, S, len(cls.algebraic), generator=gen, dtype=F64)
    forcing = [0.5 + torch.rand(B, S, generator=gen, dtype=F64) for _ in cls.forcings] or None
    return pb, y, z, forcing


@pytest.mark.parametrize("cls", AM.MODELS, ids=lambda c: c.__name__)
def test_generated_constraint_jacobian_equals_autograd(cls):
    """torch_constraint_jacobian (the DAG nodes constraint_jac is emitted from) against autograd of the class's constraint in
    float64 at random states: 1e-13 of each matrix's largest entry; the pattern is autograd's."""
    pb, y, z, forcing = _states(cls)
    gen = cls.torch_constraint_jacobian(y, z, pb["th"], pb["cond"], forcing=forcing)
    inst = cls.__new__(cls)
    if cls.forcings:
        object.__setattr__(inst, "forcing", G._Forcings(cls, lambda k, _n: forcing[k]))
    p = G._Named(inst.prepare(G._Named(pb["th"].items(), "parameter"), G._Conditions([])).items(), "effective parameter")
    zz = z.clone().requires_grad_(True)
    res = inst.constraint(list(y.unbind(-1)), list(zz.unbind(-1)), p, G._Conditions([]))
    auto = torch.stack([torch.autograd.grad(r.sum(), zz, retain_graph=True)[0] for r in res], dim=-2)
    e = float(((gen - auto).abs() / auto.abs().amax((-1, -2), keepdim=True)).max())
    print("%s: generated dg/dz against autograd %.2e" % (cls.__name__, e))
    assert e <= 1e-13
    pattern = torch.tensor(G.constraint_pattern(cls))
    assert torch.equal(pattern, (auto != 0.0).any(0).any(0))


def test_structural_patterns():
    count = lambda cls: sum(map(sum, G.constraint_pattern(cls)))  # noqa: E731
    assert [count(c) for c in AM.MODELS] == [1, 4, 7, 1]
    assert G.constraint_pattern(AM.ChainFour) == [[i == j or i == j + 1 for j in range(4)] for i in range(4)]


# ---- generated text -------------------------------------------------------------------------------------------------------------
def test_generated_text():
    for cls in AM.MODELS:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)
        M = len(cls.algebraic)
        pattern = G.constraint_pattern(cls)
        mask = sum(1 << (i * M + j) for i in range(M) for j in range(M) if pattern[i][j])
        for line in ("static constexpr int N_ALGEBRAIC = %d;" % M, "static constexpr int ALG_ITER = %d;" % cls.algebraic_iterations,
                     "static constexpr unsigned ALG_NZ = 0x%xu;" % mask):
            assert line in src, line
        body = _member(src, "constraint_jac")
        for i in range(M):
            for j in range(M):
                assert body.count("A[%d] = " % (i * M + j)) == (1 if pattern[i][j] else 0)
        for m in ("rhs", "observe"):
            assert "    float z[%d];\n    algebraic(y, p, u, z);" % M in _member(src, m), m
        for m in ("rhs_vjp", "observe_vjp"):
            assert _member(src, m).rstrip().endswith("algebraic_vjp(y, z, p, u, zb, yb, pb);"), m
        for m in ("algebraic_start", "constraint", "constraint_vjp", "algebraic", "algebraic_vjp"):
            assert "__device__ static void %s(" % m in src
    # the forcing a constraint reads: the interpolant at the stage time in rhs, the sample of the point in observe
    cls = AM.BindingCombined
    tr, src = cls._trace, G.generate_source(cls)
    assert "const float u[2] = {(p[%d] + (t - p[%d]) * p[%d])," % (tr.F0, tr.F0 + 4, tr.F0 + 2) in _member(src, "rhs")
    assert "const float u[2] = {p[%d], p[%d]};" % (tr.F0, tr.F0 + 1) in _member(src, "observe")
    assert "u[0]" in _member(src, "constraint") and "SUBSTEPS = 2" in src and "OWN_JUMP" in src
    assert "const float* u = nullptr;" in _member(G.generate_source(AM.BindingQss), "rhs")
    # the closed-form twin has nothing of it
    closed = G.generate_source(AM.BindingClosed)
    assert "N_ALGEBRAIC" not in closed and "algebraic(" not in closed and "constraint" not in closed and "fsqrt" in closed


def test_classes_without_algebraic_variables_generate_the_recorded_text():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        for key, digest in json.load(f).items():
            cname, neural = key.split(":")
            text = G.generate_source(getattr(MM, cname), bool(int(neural)))
            assert hashlib.sha256(text.encode()).hexdigest() == digest, key
            assert "ALGEBRAIC" not in text and "algebraic" not in text
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256_all.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 29
    for key, digest in recorded.items():
        path, neural = key.split(":")
        module, cname = path.rsplit(".", 1)
        text = G.generate_source(getattr(importlib.import_module(module), cname), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "ALGEBRAIC" not in text and "algebraic" not in text


def test_new_classes_generate_the_recorded_text():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_algebraic_source_sha256.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted("%s:0" % c.__name__ for c in ALL)
    for cls in ALL:
        text = G.generate_source(cls)
        assert hashlib.sha256(text.encode()).hexdigest() == recorded["%s:0" % cls.__name__], cls.__name__


def test_documents_have_the_paragraph():
    for word in ("Algebraic variables.", "algebraic_iterations", "algebraic_start", "constraint(self, y, z, p, c)",
                 "torch_algebraic", "MAX_ALGEBRAIC", "pivot", "implicit-function"):
        assert word in G.__doc__, word
    with open(os.path.join(CSRC, "vihds_algebraic.hpp")) as f:
        header = f.read()
    for word in ("algebraic_start", "ALG_ITER times", "A^T mu = zb", "WITHOUT pivoting"):
        assert word in header, word
    assert hip.GENERATED_ALGEBRAIC == {} or all(isinstance(v, int) for v in hip.GENERATED_ALGEBRAIC.values())


# ---- the iteration on the host ----------------------------------------------------------------------------------------------------
def _trajectory(cls, pb):
    with torch.no_grad():
        return AM.JM.explicit_states(cls, pb["th"], pb["cond"], pb["times"], "rk4")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls", AM.MODELS, ids=lambda c: c.__name__)
def test_newton_has_converged_at_the_test_inputs(cls, shape):
    """The kernel's adjoint is that of the CONVERGED solution: on the float64 run alone, the last of the algebraic_iterations
    increments is at most 1e-9 of |z| at every state of the rk4 trajectory, at both shapes of the GPU tests."""
    pb = AM.problem(cls, *shape)
    xs = _trajectory(cls, pb)
    last = AM.last_increment(cls, xs, pb["th"], pb["cond"])
    print("%s %dx%d: last Newton increment %.2e" % ((cls.__name__,) + shape + (last,)))
    assert bool(torch.isfinite(xs).all()) and last <= 1e-9


def test_torch_algebraic_is_the_root_written_out_by_hand():
    """BindingQss against the closed form, Competing against its iteration written out with the analytic Jacobian and Cramer's
    rule (1e-13 relative); no pivot of Competing's unpivoted elimination is small at the test inputs."""
    pb = AM.problem(AM.BindingQss, 3, 100)
    xs = _trajectory(AM.BindingQss, pb)
    for k in (0, 4, 8):
        z = AM.BindingQss.torch_algebraic(xs[..., k], pb["th"], pb["cond"])
        root = AM.binding_root(xs[:, :, 0, k], xs[:, :, 1, k], pb["th"]["koff"] / pb["th"]["kon"])
        assert z.shape == (3, 100, 1) and float(((z[..., 0] - root).abs() / root).max()) <= 1e-13
    pb = AM.problem(AM.Competing, 3, 100)
    xs = _trajectory(AM.Competing, pb)
    smallest = float("inf")
    for k in (0, 4, 8):
        z, last = AM.Competing.torch_algebraic(xs[..., k], pb["th"], pb["cond"], return_increment=True)
        C1, C2, pivot = AM.competing_newton(xs[:, :, 0, k], xs[:, :, 1, k], xs[:, :, 2, k], pb["th"]["K1"], pb["th"]["K2"], 8)
        assert float(((z[..., 0] - C1).abs() / C1).max()) <= 1e-13 and float(((z[..., 1] - C2).abs() / C2).max()) <= 1e-13
        assert last <= 1e-9
        smallest = min(smallest, float(pivot.min()))
    print("Competing: smallest |dg1/dC1| over the iterations %.3f" % smallest)
    assert smallest >= 0.1
    with pytest.raises(G.ModelDefinitionError, match="declares no algebraic variables"):
        AM.BindingClosed.torch_algebraic(xs[..., 0], pb["th"], pb["cond"])


def test_torch_algebraic_keeps_the_iterate_and_carries_the_implicit_function_gradient():
    """One iteration is not converged: the value is still exactly the iterate's (no correction is added to it), and the
    gradient is -A^-1 dg/d(y, p) at that iterate -- against the closed form's autograd at the converged count."""
    pb = AM.problem(AM.BindingQss, 3, 5)
    y = _trajectory(AM.BindingQss, pb)[..., 4]
    th = {n: v.clone().requires_grad_(True) for n, v in pb["th"].items()}
    yy = y.clone().requires_grad_(True)
    z = AM.BindingQss.torch_algebraic(yy, th, pb["cond"])
    with torch.no_grad():
        assert torch.equal(z, AM.BindingQss.torch_algebraic(y, pb["th"], pb["cond"]))
    w = torch.randn(z.shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    got = torch.autograd.grad((z * w).sum(), [yy, th["kon"], th["koff"]])
    y2 = y.clone().requires_grad_(True)
    th2 = {n: v.clone().requires_grad_(True) for n, v in pb["th"].items()}
    root = AM.binding_root(y2[..., 0], y2[..., 1], th2["koff"] / th2["kon"])
    want = torch.autograd.grad((root * w[..., 0]).sum(), [y2, th2["kon"], th2["koff"]])
    for a, b in zip(got, want):
        assert float((a - b).abs().max() / b.abs().max()) <= 1e-12


def test_implicit_function_gradient_equals_autograd_of_the_closed_form():
    """float64, rk4, 3 x 100: the definition of BindingQss (Newton, implicit-function gradient) against plain autograd of
    BindingClosed's definition: trajectories, log-likelihood and every theta gradient to 1e-8 relative -- the level the
    precondition (last increment <= 1e-9) implies."""
    pb = AM.problem(AM.BindingQss, 3, 100)
    a, b = AM.definition(AM.BindingQss, pb, "rk4", F64), AM.definition(AM.BindingClosed, pb, "rk4", F64)
    assert a["last_increment"] <= 1e-9 and b["last_increment"] == 0.0
    worst = 0.0
    for k in ("traj", "xpred", "logp"):
        e = float((a[k] - b[k]).abs().max() / b[k].abs().max())
        print("%s: quasi-steady-state definition against the closed form %.2e" % (k, e))
        worst = max(worst, e)
    for n, g in b["g_theta"].items():
        if float(g.abs().max()) == 0.0:
            assert float(a["g_theta"][n].abs().max()) == 0.0
            continue
        e = float((a["g_theta"][n] - g).abs().max() / g.abs().max())
        print("g_theta[%s]: implicit-function gradient against autograd of the closed form %.2e" % (n, e))
        worst = max(worst, e)
    assert worst <= 1e-8


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.__name__)
def test_explicit_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every explicit fixed-grid solver compile for gfx950 and spill
    nothing (VGPRs printed; recorded in DESIGN.md).  ChainFour is the worst case the cap MAX_ALGEBRAIC stands for."""
    header = tmp_path / "algebraic.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(kMaxAlgebraic == %d);" % G.MAX_ALGEBRAIC]
    for solver in AM.SOLVERS:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "algebraic"), "_ZN5vihds")
    assert len(usage) == 15, sorted(usage)
    for solver in AM.SOLVERS:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d" % (cls.__name__, solver, min(fwd), max(fwd), bwd[0]))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


# ---- the Newton loop and both solves, in a stand-alone host program under sanitizers ----------------------------------------------
PROGRAM = r"""
// reads cases "m pattern transpose newton, A[m m], b[m]".  newton = 0: prints the solution of A x = b (transpose: A^T x = b,
// through algebraic_adjoint, whose sign is undone here).  newton > 0: prints z after that many Newton iterations from b on
// g(z) = A z + 0.5 z * z - 1 (componentwise square), whose Jacobian A + diag(z) has A's pattern plus the diagonal.
#include <cstdio>
#include <vector>
#include "vihds_algebraic.hpp"
template <int M, unsigned NZ>
static void run(int transpose, int newton, const std::vector<float>& A, std::vector<float>& b) {
  if (newton == 0 && !transpose) vihds::dense_solve<M, NZ, false>(A.data(), b.data());
  else if (newton == 0) {
    vihds::algebraic_adjoint<M, NZ>(b.data(), [&](float* J) { for (int k = 0; k < M * M; ++k) if ((NZ >> k) & 1u) J[k] = A[k]; });
    for (float& v : b) v = -v;
  } else {
    auto g = [&](const float* z, float* G) {
      for (int i = 0; i < M; ++i) {
        float s = 0.5f * z[i] * z[i] - 1.f;
        for (int j = 0; j < M; ++j) if ((NZ >> (i * M + j)) & 1u) s += A[i * M + j] * z[j];
        G[i] = s;
      }
    };
    auto jac = [&](const float* z, float* J) {
      for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j) if ((NZ >> (i * M + j)) & 1u) J[i * M + j] = A[i * M + j] + (i == j ? z[i] : 0.f);
    };
    if (newton == 3) vihds::algebraic_newton<M, 3, NZ>(b.data(), g, jac);
    else vihds::algebraic_newton<M, 8, NZ>(b.data(), g, jac);
  }
}
int main() {
  int m, pattern, transpose, newton;
  while (std::scanf("%d %d %d %d", &m, &pattern, &transpose, &newton) == 4) {
    std::vector<float> A(m * m), b(m);
    for (float& v : A) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : b) if (std::scanf("%f", &v) != 1) return 2;
    if (m == 1) run<1, 0x1u>(transpose, newton, A, b);
    else if (m == 2 && pattern == 0) run<2, 0xfu>(transpose, newton, A, b);
    else if (m == 2) run<2, MASK_2_1>(transpose, newton, A, b);        // lower triangular
    else if (m == 3 && pattern == 0) run<3, 0x1ffu>(transpose, newton, A, b);
    else if (m == 3) run<3, MASK_3_1>(transpose, newton, A, b);        // arrowhead (first row, first column): fills in everywhere
    else if (m == 4 && pattern == 0) run<4, 0xffffu>(transpose, newton, A, b);
    else if (m == 4 && pattern == 1) run<4, MASK_4_1>(transpose, newton, A, b);   // lower bidiagonal (ChainFour)
    else if (m == 4) run<4, MASK_4_2>(transpose, newton, A, b);        // arrowhead (last row, last column): no fill-in
    else return 3;
    for (int i = 0; i < m; ++i) std::printf("%.9g%c", b[i], i + 1 < m ? ' ' : '\n');
  }
  return 0;
}
"""


def _mask(m, entry):
    return sum(1 << (i * m + j) for i in range(m) for j in range(m) if i == j or entry(i, j))


MASKS = {(1, 0): 0x1, (2, 0): 0xf, (2, 1): _mask(2, lambda i, j: j < i), (3, 0): 0x1ff, (3, 1): _mask(3, lambda i, j: i == 0 or j == 0),
         (4, 0): 0xffff, (4, 1): _mask(4, lambda i, j: i == j + 1), (4, 2): _mask(4, lambda i, j: i == 3 or j == 3)}


def _host_compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) or (name if os.path.exists(name) else None)
        if path:
            return path
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_newton_and_both_solves_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/vihds_algebraic.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own, which runs
    dense_solve, the adjoint's transposed solve and the Newton loop for 1 to 4 unknowns on dense and sparse patterns (lower
    triangular, ChainFour's lower bidiagonal, arrowheads) with diagonally dominant matrices.  Against numpy in float64 (pivoted
    solves; Newton iterated in float64 with the same count); the bound per case is 8 x the error of the same computation with
    numpy's pivoted float32 solve, floored at 1e-6 -- both printed."""
    chain = G.constraint_pattern(AM.ChainFour)
    masks = dict(MASKS)
    assert masks[(4, 1)] == sum(1 << (i * 4 + j) for i in range(4) for j in range(4) if chain[i][j])
    src, exe = tmp_path / "algebraic.cpp", tmp_path / "algebraic"
    src.write_text(PROGRAM)
    defines = ["-DMASK_%d_%d=0x%xu" % (m, pt, masks[(m, pt)]) for m, pt in sorted(masks) if pt]
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined"] + defines + ["-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    rng = np.random.RandomState(5)
    cases = []
    for (m, pattern), mask in sorted(masks.items()):
        keep = np.array([[(mask >> (i * m + j)) & 1 for j in range(m)] for i in range(m)], dtype=np.float64)
        assert keep.diagonal().all()
        for transpose, newton in ((0, 0), (1, 0), (0, 3), (0, 8)):
            for _ in range(3):
                A = (rng.randn(m, m) + np.diag(m + 2.0 + 3.0 * rng.rand(m))) * keep
                b = rng.randn(m) if newton == 0 else 0.1 + 0.2 * rng.rand(m)
                cases.append((m, pattern, transpose, newton, A, b))
    text = "".join("%d %d %d %d\n%s\n%s\n" % (m, pt, tr, nw, " ".join("%.9g" % v for v in A.reshape(-1)),
                                              " ".join("%.9g" % v for v in b)) for m, pt, tr, nw, A, b in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(cases)

    def compute(A, b, transpose, newton, dtype):
        A, b = A.astype(dtype), b.astype(dtype)
        if newton == 0:
            return np.linalg.solve(A.T if transpose else A, b)
        z = b
        for _ in range(newton):
            G_ = (A @ z + dtype(0.5) * z * z - dtype(1.0)).astype(dtype)
            z = (z + np.linalg.solve(A + np.diag(z), -G_)).astype(dtype)
        return z

    worst = (0.0, 0.0)
    for (m, pt, tr, nw, A, b), row in zip(cases, rows):
        A32, b32 = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)  # (the program's inputs)
        exact = compute(A32, b32, tr, nw, np.float64)
        pivoted = compute(A32, b32, tr, nw, np.float32).astype(np.float64)
        got = np.array([float(v) for v in row.split()])
        scale = np.abs(exact).max()
        e_got, e_piv = np.abs(got - exact).max() / scale, np.abs(pivoted - exact).max() / scale
        if e_got > worst[0]:
            worst = (e_got, e_piv)
        assert e_got <= max(1e-6, 8.0 * e_piv), (m, pt, tr, nw, e_got, e_piv)
    print("%d cases: worst unpivoted float32 error %.2e (numpy's pivoted float32 computation there: %.2e)" % ((len(cases),) + worst))
