"""CPU tests of a generated model's own observation map (GeneratedOdeModel.observe): definition errors, torch_observe, the
traced map's reverse mode against torch.autograd in float64, the generated text, and compilation for gfx950 (no scratch in
the forward and adjoint kernels of every fixed-grid solver, plain and inside WithPrec<>)."""
import hashlib
import json
import os
import re
import shutil

import pytest
import torch

from vihds import modelgen as G
from vihds.modelgen import Network

import modelgen_models as MM
import modelgen_observe_models as OM
from test_modelgen_host import _compile_usage, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name, **body):
    attrs = dict(model_key=name, species=["OD", "RFP"], parameters=["r", "gain", "init_x"], n_conditions=1,
                 prepare=lambda self, th, c: {"r": th.r, "gain": th.gain},
                 initial_state=lambda self, th, c: [th.init_x, 0.0],
                 rhs=lambda self, t, y, p, c: [p.r * y[0], -y[1]],
                 observe=lambda self, y, p, c: [y[0], p.gain * y[0] * y[1], c[0] * y[1], 1.0])
    attrs.update(body)
    return type(name, (G.GeneratedOdeModel,), attrs)


def test_a_class_with_observe_has_the_custom_kind_and_keeps_the_instance_method():
    from vihds.ode import OdeModel

    cls = _define("obs_ok")  # (two species: the species count of the fixed kinds does not apply)
    assert cls.observe_kind == "custom" and cls.observe is OdeModel.observe
    one = _define("obs_one_species", species=["OD"], initial_state=lambda self, th, c: [th.init_x],
                  rhs=lambda self, t, y, p, c: [p.r * y[0]], observe=lambda self, y, p, c: [y[0], p.gain * y[0], 0.0, c[0]])
    assert one.observe_kind == "custom"
    # a subclass inherits the map; the classes without one keep their fixed kind
    sub = type("ObsSub", (OM.PrprOwnMap,), {"model_key": "obs_sub"})
    assert sub.observe_kind == "custom" and "OBS_CUSTOM" in G.generate_source(sub)
    assert MM.PrprRestated.observe_kind == "default" and MM.EveryOperation.observe_kind == "direct"
    with pytest.raises(G.ModelDefinitionError, match="defines no observe"):
        MM.PrprRestated.torch_observe(torch.zeros(1, 1, 6, 2), {}, torch.zeros(1, 0))


def test_definition_errors_of_observe_are_raised_when_the_class_is_defined():
    with pytest.raises(G.ModelDefinitionError, match="observe must return a list of 4"):
        _define("obs_three", observe=lambda self, y, p, c: [y[0], y[1], y[0]])
    with pytest.raises(G.ModelDefinitionError, match="observe must return a list of 4"):
        _define("obs_scalar", observe=lambda self, y, p, c: y[0])
    with pytest.raises(G.ModelDefinitionError, match="called from observe: networks are evaluated in rhs only"):
        _define("obs_net", networks={"f": Network(2, 3, 1)},
                rhs=lambda self, t, y, p, c: [self.net.f([y[0], y[1]])[0], -y[1]],
                observe=lambda self, y, p, c: [self.net.f([y[0], y[1]])[0], y[0], y[1], 0.0])
    with pytest.raises(G.ModelDefinitionError, match="unknown effective parameter 'nope'"):
        _define("obs_name", observe=lambda self, y, p, c: [y[0], p.nope, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="out of range"):
        _define("obs_cond", observe=lambda self, y, p, c: [y[0], c[1], 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("obs_if", observe=lambda self, y, p, c: [y[0] if y[0] > 0.0 else y[1], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="defines observe and observe_kind = 'direct'"):
        _define("obs_kind", observe_kind="direct")
    with pytest.raises(G.ModelDefinitionError, match="defines observe and observe_kind = 'direct'"):
        type("ObsKindSub", (OM.PrprOwnMap,), {"model_key": "obs_kind_sub", "observe_kind": "direct"})
    with pytest.raises(G.ModelDefinitionError, match="must be one of"):
        _define("obs_custom_without_a_map", observe=None, observe_kind="custom", species=["a", "b", "c", "d", "e", "f"],
                initial_state=lambda self, th, c: [th.init_x] + [0.0] * 5, rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 5)


def _rand(shape, lo, hi, seed):
    gen = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, generator=gen)


def _reader_inputs(B=6, S=5, T=4):
    cls = OM.PlateReader
    th = {n: _rand((B, S), 0.2, 1.5, 3 + k) for k, n in enumerate(cls.parameter_names)}
    th["leak"] = _rand((B, S), -0.3, 0.9, 90)  # clamp(leak, 0, 0.5) in prepare: below, inside and above the bounds
    assert bool((th["leak"] < 0).any()) and bool((th["leak"] > 0.5).any()) and bool(((th["leak"] > 0) & (th["leak"] < 0.5)).any())
    cond = torch.log1p(_rand((B, 1), 0.1, 3.0, 91))
    y = _rand((B, S, 3, T), 0.1, 2.0, 92)
    return cls, th, cond, y


def test_torch_observe_of_a_restated_map_against_the_expression():
    """torch_observe applies prepare and evaluates the definition in the caller's dtype: the default map restated, the
    inducer map, and the reader's map against its formula written out with torch."""
    y6 = _rand((3, 4, 10, 5), 0.1, 2.0, 1)  # (ten states: whatever is stored behind the species is ignored)
    th = {n: _rand((3, 4), 0.2, 1.5, 2) for n in OM.PrprOwnMap.parameter_names}
    got = OM.PrprOwnMap.torch_observe(y6, th, torch.zeros(3, 0, dtype=torch.float64))
    x = y6[:, :, 0]
    ref = torch.stack([x, x * y6[:, :, 1], x * (y6[:, :, 2] + y6[:, :, 4]), x * (y6[:, :, 3] + y6[:, :, 5])], dim=2)
    assert got.dtype == torch.float64 and got.shape == (3, 4, 4, 5) and torch.equal(got, ref)
    thi = {n: _rand((3, 4), 0.2, 1.5, 5) for n in OM.InducerRestated.parameter_names}
    got = OM.InducerRestated.torch_observe(y6, thi, torch.zeros(3, 1, dtype=torch.float64))
    ref = torch.stack([x, x * y6[:, :, 1], x * (y6[:, :, 2] + y6[:, :, 3]), x * y6[:, :, 4]], dim=2)
    assert torch.equal(got, ref)
    cls, th, cond, y = _reader_inputs()
    got = cls.torch_observe(y, th, cond)
    x, rfp, yfp = y[:, :, 0], y[:, :, 1], y[:, :, 2]
    bs = lambda v: v[:, :, None]  # noqa: E731
    c0 = torch.clamp(torch.exp(cond) - 1.0, 1e-12, 1e6)[:, :, None]
    leak = torch.clamp(bs(th["leak"]), 0.0, 0.5)
    ref = torch.stack([x, bs(th["gain_r"]) * x * rfp + bs(th["bg_r"]),
                       x * yfp / (1.0 + bs(th["sat"]) * yfp) + leak * x * rfp,
                       x * bs(th["auto"]) * c0 * torch.sigmoid(x - 1.0) + torch.exp(-x) * leak], dim=2)
    assert got.dtype == torch.float64 and torch.allclose(got, ref, rtol=1e-14, atol=1e-14)
    assert cls.torch_observe(y.float(), th, cond).dtype == torch.float32


def test_traced_observe_vjp_matches_autograd():
    """The reader's map (/, sigmoid, exp, a parameter clamped in prepare, a treatment): observe_vjp as the generator derives
    it -- reverse mode over the DAG, evaluated in float64 by the DAG evaluation of test_operation_vjp_matches_autograd --
    followed by prepare_vjp, as the adjoint kernel chains them, against torch.autograd through torch_observe."""
    cls, th, cond, y = _reader_inputs()
    tr = cls._trace
    g = tr.g
    N, P, NPU = len(cls.species), cls.parameter_names, len(tr.p_names)
    B, S, _, T = y.shape
    W = torch.randn(B, S, 4, T, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    c0 = torch.clamp(torch.exp(cond) - 1.0, 1e-12, 1e6)[:, :, None]  # [B,1,1]
    env_th = {("th", s): th[n][:, :, None] for s, n in enumerate(P)}
    env_th[("c", 0)] = c0
    pvals = G.evaluate(tr.p_exprs, env_th)
    # observe and its adjoint
    seeds = [g.leaf("seed", j) for j in range(4)]
    adj = G.vjp(g, tr.obs, seeds)
    y_leaves, p_leaves = [g.leaf("y", j) for j in range(N)], [g.leaf("p", k) for k in range(NPU)]
    env = {("y", j): y[:, :, j] for j in range(N)}
    env.update({("p", k): pvals[k] for k in range(NPU)})
    env[("p", NPU)] = c0  # (the treatment as observe reads it: one more parameter behind the named ones)
    env.update({("seed", j): W[:, :, j] for j in range(4)})
    nodes = list(tr.obs) + [adj.get(l.id, g.const(0.0)) for l in y_leaves + p_leaves]
    vals = G.evaluate(nodes, env)
    xp = torch.stack([v.expand(B, S, T) for v in vals[:4]], dim=2)
    yb = [v.expand(B, S, T) for v in vals[4:4 + N]]
    pb = [v.expand(B, S, T).sum(2, keepdim=True) for v in vals[4 + N:]]  # (one parameter per trajectory: summed over time)
    read_by_observe = {tr.p_names[k] for k, l in enumerate(p_leaves) if l.id in adj}
    assert read_by_observe == {"gain_r", "bg_r", "sat", "auto", "leak"}
    # ... then prepare's adjoint with pb as its seed
    adj_p = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    env_th.update({("seed", k): pb[k] for k in range(NPU)})
    thb = G.evaluate([adj_p.get(g.leaf("th", s).id, g.const(0.0)) for s in range(len(P))], env_th)
    # autograd
    yt = y.clone().requires_grad_(True)
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    ref = cls.torch_observe(yt, tht, cond)
    assert torch.allclose(xp, ref, rtol=1e-12, atol=1e-12)
    grads = torch.autograd.grad(ref, [yt] + [tht[n] for n in P], W, allow_unused=True)
    err = lambda a, b: ((a - b).abs() / (1.0 + b.abs())).max().item()  # noqa: E731
    for j in range(N):
        assert err(yb[j], grads[0][:, :, j]) <= 1e-12, j
    for s, n in enumerate(P):
        want = grads[1 + s] if grads[1 + s] is not None else torch.zeros(B, S, dtype=torch.float64)
        assert err(thb[s].expand(B, S, 1)[:, :, 0], want) <= 1e-12, n
    # the comparison is not vacuous: the observe-only parameters have a gradient, the clamped one only inside its bounds
    for n in ("gain_r", "bg_r", "sat", "auto"):
        assert float(grads[1 + P.index(n)].abs().min()) > 0.0, n
    gl = grads[1 + P.index("leak")]
    inside = (th["leak"] >= 0.0) & (th["leak"] <= 0.5)
    assert bool((gl[inside] != 0).all()) and bool((gl[~inside] == 0).all())


def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def test_generated_text_of_a_custom_map():
    src = G.generate_source(OM.PlateReader)
    assert "static constexpr int OBS = OBS_CUSTOM;" in src
    assert "__device__ static void observe(const float* y, const float* p, float* xp) {" in src
    assert ("__device__ static void observe_vjp(const float* y, const float* p, const float* xpb, float* yb, float* pb) {"
            in src)
    assert src == G.generate_source(OM.PlateReader)
    again = type("ReaderAgain", (OM.PlateReader,), {"model_key": OM.PlateReader.model_key})
    assert G.generate_source(again).split("\n", 1)[1] == src.split("\n", 1)[1]
    for cls, neural in OM.PREBUILT:
        a = G.generate_source(cls, neural)
        assert a == G.generate_source(cls, neural) and G.library_tag(a) == G.library_tag(a) and "OBS_CUSTOM" in a
    tr = OM.PlateReader._trace
    NPU = len(tr.p_names)
    # the treatment (read by prepare and by observe, not by rhs) is one more parameter, copied by prepare, without adjoint
    assert tr.c_in_rhs == [0] and "    p[%d] = c[0];" % NPU in _member(src, "prepare")
    assert "p[%d]" % NPU in _member(src, "observe") and "p[%d]" % NPU not in _member(src, "rhs")
    body = _member(src, "observe_vjp")
    written = sorted(int(k) for k in re.findall(r"pb\[(\d+)\] \+=", body))
    assert written == sorted(tr.p_names.index(n) for n in ("gain_r", "bg_r", "sat", "auto", "leak"))
    assert all(k < NPU for k in written) and " = " not in re.sub(r"const float v\d+ = ", "", body)  # (it adds, never assigns)
    assert sorted(int(j) for j in re.findall(r"yb\[(\d+)\] \+=", body)) == [0, 1, 2]
    # both members use the time-loop helpers (they run once per time point), not the accurate forms of prepare
    both = _member(src, "observe") + body
    assert "fdiv(" in both and "sigmoid_f(" in both and "fexp(" in both and "expf(" not in both and " / " not in both
    # a map without parameters writes no pb at all
    assert not re.search(r"(?<!x)pb\[", _member(G.generate_source(OM.PrprOwnMap), "observe_vjp"))


def test_a_class_without_observe_generates_the_text_it_did():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        recorded = json.load(f)
    for neural in (0, 1):
        text = G.generate_source(MM.PrprRestated, bool(neural))
        assert hashlib.sha256(text.encode()).hexdigest() == recorded["PrprRestated:%d" % neural]
        assert "OBS_CUSTOM" not in text and "observe" not in text


FIXED = ["MODEULER", "MODEULERWHILE", "EULER", "MIDPOINT", "RK4"]


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
@pytest.mark.parametrize("wrapped", [False, True])
def test_custom_map_compiles_without_scratch_for_every_fixed_grid_solver(tmp_path, wrapped):
    """Forward and adjoint kernels of the reader model, plain and inside WithPrec<> (where the core's species lead y and its
    parameters lead p), for every fixed-grid solver: they compile for gfx950 and spill nothing.  (VGPRs printed, recorded
    in profiles/LOG.md.)"""
    header = tmp_path / "reader.hpp"
    header.write_text(G.generate_source(OM.PlateReader, wrapped))
    model = "WithPrec<VIHDS_GEN_CORE>" if wrapped else "VIHDS_GEN_CORE"
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {"]
    for s in FIXED:
        lines.append("template __global__ void ode_fwd_kernel<%s, VIHDS_SOLVER_%s, true>(OdeArgs);" % (model, s))
        lines.append("template __global__ void ode_bwd_kernel<%s, VIHDS_SOLVER_%s, false>(OdeArgs);" % (model, s))
        if wrapped:  # (the adjoint that dumps for the weight gradient)
            lines.append("template __global__ void ode_bwd_kernel<%s, VIHDS_SOLVER_%s, true>(OdeArgs);" % (model, s))
    lines.append("}")
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", "reader"), "_ZN5vihds")
    assert len(usage) == len(FIXED) * (3 if wrapped else 2), sorted(usage)
    for name, (vgpr, scratch) in sorted(usage.items()):
        print("%s: %d VGPRs, %d B scratch" % (name, vgpr, scratch))
        assert scratch == 0, name
