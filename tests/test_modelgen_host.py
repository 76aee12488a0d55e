"""CPU tests of vihds.modelgen: the operations' reverse mode against torch.autograd in float64, the prpr_constant
restatement against the oracle, deterministic generation, definition errors, compilation for gfx950 (scratch and VGPRs of the
generated kernels) and vihds_model_register's refusal of a missing library."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from fixture_util import Fixture
from oracle import vihds_oracle as O
from vihds import hip
from vihds import modelgen as G

import modelgen_models as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")


def _check_vjp(fn, xs, seed=0):
    """fn(*args) -> one value; compare the generated VJP (evaluated in float64) with torch.autograd."""
    g = G.Graph()
    leaves = [g.leaf("th", k) for k in range(len(xs))]
    out = fn(*leaves)
    assert isinstance(out, G.Sym)
    seed_leaf = g.leaf("seed", 0)
    adj = G.vjp(g, [out], [seed_leaf])
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(xs[0].shape, dtype=torch.float64, generator=gen)
    env = {("th", k): x for k, x in enumerate(xs)}
    env[("seed", 0)] = w
    nodes = [out] + [adj.get(l.id, g.const(0.0)) for l in leaves]
    vals = G.evaluate(nodes, env)
    xt = [x.clone().requires_grad_(True) for x in xs]
    ref = fn(*xt)
    assert torch.allclose(vals[0], ref, rtol=1e-12, atol=1e-12)
    grads = torch.autograd.grad(ref, xt, w, allow_unused=True)
    for k, (a, b) in enumerate(zip(vals[1:], grads)):
        b = torch.zeros_like(xs[k]) if b is None else b
        a = a.expand_as(b)
        err = ((a - b).abs() / (1.0 + b.abs())).max().item()
        assert err <= 1e-12, (k, err)


def _rand(n=64, lo=0.2, hi=2.0, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=gen)


@pytest.mark.parametrize("name,fn,n_args", [
    ("add", lambda a, b: a + b, 2),
    ("sub", lambda a, b: a - b, 2),
    ("mul", lambda a, b: a * b, 2),
    ("div", lambda a, b: a / b, 2),
    ("neg", lambda a: -a, 1),
    ("numbers", lambda a: 3.0 - 2.0 * a / 4.0 + 1.0 / a, 1),
    ("exp", lambda a: G.exp(a), 1),
    ("log", lambda a: G.log(a), 1),
    ("pow_const", lambda a: G.pow(a, 2.5), 1),
    ("pow_square", lambda a: G.pow(a, 2.0), 1),
    ("pow_symbolic_exponent", lambda a, n: G.pow(a, n), 2),
    ("pow_symbolic_exponent_const_base", lambda n: G.pow(1.7, n), 1),
    ("sigmoid", lambda a: G.sigmoid(a), 1),
    ("tanh", lambda a: G.tanh(a), 1),
    ("clamp", lambda a: G.clamp(a, 0.5, 1.5), 1),
    ("hill", lambda n, k6, k12: (G.pow(G.clamp(k6, 1e-12, 1.0) * 3.0, G.clamp(n, 0.5, 3.0))
                                 + G.pow(G.clamp(k12, 1e-12, 1.0) * 0.5, G.clamp(n, 0.5, 3.0)))
     / G.pow(1.0 + G.clamp(k6, 1e-12, 1.0) * 3.0 + G.clamp(k12, 1e-12, 1.0) * 0.5, G.clamp(n, 0.5, 3.0)), 3),
    ("growth", lambda r, K, x, t: G.clamp(r, 0.0, 4.0) * G.sigmoid(4.0 * (t - 1.0)) * (1.0 - x / K) * x, 4),
    ("promoter", lambda e, k, b: (e + k * b * b) / (1.0 + k * b * b) * G.tanh(b) - G.exp(-b), 3),
])
def test_operation_vjp_matches_autograd(name, fn, n_args):
    xs = [_rand(seed=7 * k + 1) for k in range(n_args)]
    _check_vjp(fn, xs)


def test_clamp_vjp_at_the_bounds():
    """torch.clamp's gradient flows where lo <= x <= hi, the bounds themselves included (csrc clamp_pass)."""
    x = torch.tensor([0.25, 0.5, 1.0, 1.5, 1.75], dtype=torch.float64)
    _check_vjp(lambda a: G.clamp(a, 0.5, 1.5), [x])
    g = G.Graph()
    a = g.leaf("th", 0)
    adj = G.vjp(g, [G.clamp(a, 0.5, 1.5)], [1.0])
    (d,) = G.evaluate([adj[a.id]], {("th", 0): x})
    assert d.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


def test_torch_backend_dispatch():
    x = torch.tensor([0.5, 2.0], dtype=torch.float64)
    assert torch.equal(G.clamp(x, 0.6, 1.0), torch.clamp(x, 0.6, 1.0))
    assert torch.equal(G.pow(x, x), torch.pow(x, x))
    assert G.exp(0.0) == 1.0 and G.sigmoid(0.0) == 0.5


def test_prpr_restatement_matches_oracle_in_float64():
    """Through the torch backend, the API's restatement of prpr_constant gives the RHS, x0 and trajectory of
    oracle.make_prpr_constant exactly, on the prpr_constant_tiny_modeuler fixture's theta."""
    fx = Fixture("prpr_constant_tiny_modeuler")
    th = {k: v.double() for k, v in fx.theta_dict().items()}
    cond = fx.t("inputs").double()
    times = fx.t("times").double()
    rhs_a, x0_a = MM.PrprRestated.torch_problem(th, cond)
    rhs_b, x0_b = O.make_prpr_constant(th, cond)
    assert torch.equal(x0_a, x0_b.double())
    for t in (0.0, 1.3, 7.9):
        tt = torch.tensor(t, dtype=torch.float64)
        assert torch.equal(rhs_a(tt, x0_a), rhs_b(tt, x0_b.double()))
    xs_a = O.simulate(rhs_a, x0_a, times, "modeuler")
    xs_b = O.simulate(rhs_b, x0_b.double(), times, "modeuler")
    assert torch.equal(xs_a, xs_b)


def test_generated_source_is_deterministic():
    for cls, neural in MM.PREBUILT:
        a = G.generate_source(cls, neural)
        b = G.generate_source(cls, neural)
        assert a == b
        assert G.library_tag(a) == G.library_tag(b)
    # a fresh trace of the same definition gives the same text too
    cls = type("PrprAgain", (MM.PrprRestated,), {"model_key": "gen_prpr_constant"})
    assert G.generate_source(cls).split("\n", 1)[1] == G.generate_source(MM.PrprRestated).split("\n", 1)[1]
    assert "asm" not in G.generate_source(MM.LuxReceiver)


def _define(name, **body):
    attrs = dict(model_key=name, species=["OD", "RFP", "YFP", "CFP", "F530", "F480"], parameters=["r", "init_x"],
                 n_conditions=0, observe_kind="default",
                 prepare=lambda self, th, c: {"r": th.r},
                 initial_state=lambda self, th, c: [th.init_x, 0.0, 0.0, 0.0, 0.0, 0.0],
                 rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5)
    attrs.update(body)
    return type(name, (G.GeneratedOdeModel,), attrs)


def test_definition_errors_are_raised_when_the_class_is_defined():
    assert _define("ok_model").model_key == "ok_model"

    def branchy(self, t, y, p, c):
        if y[0] > 1.0:
            return [y[0]] * 6
        return [p.r] * 6

    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("bad_if", rhs=branchy)
    with pytest.raises(G.ModelDefinitionError, match="not available"):
        _define("bad_op", rhs=lambda self, t, y, p, c: [G.op.sin(y[0])] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="model quantity"):
        _define("bad_torch", rhs=lambda self, t, y, p, c: [torch.sin(y[0])] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="VIHDS_MAX_SLOTS"):
        _define("too_many", parameters=["q%d" % k for k in range(61)])
    with pytest.raises(G.ModelDefinitionError, match="at most"):
        _define("too_many_states", species=["s%d" % k for k in range(G.MAX_STATES + 1)])
    with pytest.raises(G.ModelDefinitionError, match="unknown parameter"):
        _define("bad_name", prepare=lambda self, th, c: {"r": th.nope})
    with pytest.raises(G.ModelDefinitionError, match="out of range"):
        _define("bad_cond", prepare=lambda self, th, c: {"r": th.r * c[0]})
    with pytest.raises(G.ModelDefinitionError, match="affine"):
        _define("bad_init", initial_state=lambda self, th, c: [G.exp(th.init_x), 0.0, 0.0, 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="reads 6 species"):
        _define("bad_obs", species=["OD", "RFP"], initial_state=lambda self, th, c: [th.init_x, 0.0],
                rhs=lambda self, t, y, p, c: [y[0], y[1]])


def test_register_refuses_a_missing_library():
    lib = hip.lib()
    rc = lib.vihds_model_register(b"/nonexistent/libvihds_gen_0000.so")
    assert rc < 0
    assert "no such file" in lib.vihds_last_error().decode()


def _resource_usage(text, kernel_prefix):
    """{kernel: (vgprs, scratch)} from -Rpass-analysis=kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        if cur and cur.startswith(kernel_prefix):
            m = re.search(r"VGPRs: (\d+)", line)
            if m and "AGPR" not in line:
                out.setdefault(cur, [0, 0])[0] = int(m.group(1))
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m:
                out.setdefault(cur, [0, 0])[1] = int(m.group(1))
    return out


def _compile_usage(tmp_path, source_text, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / (name + ".hip")
    src.write_text(source_text)
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c", str(src), "-o", str(tmp_path / (name + ".o"))],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return res.stdout


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_generated_prpr_compiles_without_scratch_and_within_the_builtin_vgprs(tmp_path):
    """The generated struct compiles for gfx950; its thread-per-trajectory kernels (midpoint) spill nothing and use at
    most 16 VGPRs more than the same kernels instantiated for the hand-written PrprConstant."""
    header = tmp_path / "gen.hpp"
    header.write_text(G.generate_source(MM.PrprRestated))
    inst = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
            "template __global__ void ode_fwd_kernel<%s, VIHDS_SOLVER_MIDPOINT, true>(OdeArgs);\n"
            "template __global__ void ode_bwd_kernel<%s, VIHDS_SOLVER_MIDPOINT, false>(OdeArgs);\n}\n")
    gen = _resource_usage(_compile_usage(tmp_path, inst % (header, "VIHDS_GEN_CORE", "VIHDS_GEN_CORE"), "gen"), "_ZN5vihds")
    ref = _resource_usage(_compile_usage(tmp_path, inst % (header, "PrprConstant", "PrprConstant"), "ref"), "_ZN5vihds")
    pick = lambda d, k: [v for n, v in d.items() if k in n]  # noqa: E731
    for kind in ("ode_fwd_kernel", "ode_bwd_kernel"):
        (g_vgpr, g_scr), = pick(gen, kind)
        (r_vgpr, r_scr), = pick(ref, kind)
        print("%s: generated %d VGPRs / %d B scratch, built-in PrprConstant %d VGPRs / %d B scratch"
              % (kind, g_vgpr, g_scr, r_vgpr, r_scr))
        assert g_scr == 0
        assert g_vgpr <= r_vgpr + 16


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_every_operation_compiles_in_prepare_and_rhs(tmp_path):
    """exp, log, pow, sigmoid, tanh, clamp and division, emitted in the accurate form (prepare, init) and with the time-loop
    helpers (rhs and its adjoint), compile for gfx950 into the forward and adjoint kernels, on their own and in WithPrec<>."""
    src = G.generate_source(MM.EveryOperation)
    for form in ("expf(", "logf(", "powf(", "tanhf(", "fexp(", "ftanh(", "sigmoid_f(", "fdiv(", "frcp(", "clampf(",
                 "clamp_pass("):
        assert form in src, form
    header = tmp_path / "ops.hpp"
    header.write_text(src)
    inst = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
            "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_RK4, true>(OdeArgs);\n"
            "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_RK4, false>(OdeArgs);\n"
            "template __global__ void ode_bwd_kernel<WithPrec<VIHDS_GEN_CORE>, VIHDS_SOLVER_MIDPOINT, false>(OdeArgs);\n}\n")
    usage = _resource_usage(_compile_usage(tmp_path, inst % header, "ops"), "_ZN5vihds")
    assert len(usage) == 3 and all(scr == 0 for _, scr in usage.values()), usage


def test_library_tag_follows_every_file_of_the_layout_guard():
    """The cache key of a generated library covers the files whose checksum vihds_model_register compares (the Makefile's
    HDRS: csrc/*.hpp and include/vihds_hip.h), so an edit to any of them names a new library instead of finding one the
    main library refuses."""
    import inspect

    body = inspect.getsource(G._kernel_headers_digest)
    assert "vihds_hip.h" in body
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "HDRS = $(wildcard *.hpp) ../../include/vihds_hip.h" in mk


def test_declared_parameter_names_leave_the_module_parameters_method_alone():
    """`parameters = [...]` in a model class is the list of theta names; the class keeps nn.Module.parameters() (the
    optimiser and the general training step walk the decoder's tensors through it) and the names as parameter_names."""
    import torch.nn as nn

    for cls in (MM.PrprRestated, MM.PrprRestatedPrecisions, MM.DrRestated):
        assert cls.parameters is nn.Module.parameters
        assert cls.parameter_names[:2] == ["r", "K"]
