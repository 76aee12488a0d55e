"""CPU tests of a generated model's own precision map (GeneratedOdeModel.precision): definition errors, the instance's
precisions attribute, the generated text, torch_precision against finite differences in float64, the traced adjoint against
autograd, and compilation for gfx950 (no scratch in the forward and adjoint kernels of every fixed-grid solver)."""
import hashlib
import json
import os
import re
import shutil

import pytest
import torch

from vihds import hip
from vihds import modelgen as G
from vihds.modelgen import Network
from vihds.precisions import ConstantPrecisions, ModelPrecisions, NeuralPrecisions

import modelgen_models as MM
import modelgen_noise_models as NM
from test_modelgen_host import _compile_usage, _resource_usage
from test_modelgen_nn_host import _config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_ONLY = NM.NOISE


def _define(name, **body):
    attrs = dict(model_key=name, species=["OD", "RFP"], parameters=["r", "s0", "s1", "init_x"], n_conditions=1,
                 prepare=lambda self, th, c: {"r": th.r, "s0": th.s0, "s1": th.s1},
                 initial_state=lambda self, th, c: [th.init_x, 0.0],
                 rhs=lambda self, t, y, p, c: [p.r * y[0], -y[1]],
                 observe=lambda self, y, p, c: [y[0], y[0] * y[1], y[1], 1.0],
                 precision=lambda self, y, x, p, c: [1.0 / (p.s0 * p.s0 + G.pow(p.s1 * x[0], 2.0)), 1.0 / (p.s0 + c[0]),
                                                     G.exp(-y[1]), 4.0])
    attrs.update(body)
    return type(name, (G.GeneratedOdeModel,), attrs)


def test_a_class_with_precision_is_traced_and_owns_its_precisions():
    cls = _define("noise_ok")
    tr = cls._trace
    assert tr.prec is not None and len(tr.prec) == 4 and tr.prec[3].op == "const"  # (a Python number is a constant precision)
    assert tr.c_in_rhs == [0]  # (the treatment precision reads is copied by prepare: the union with rhs and observe)
    src = G.generate_source(cls)
    assert "static constexpr bool OWN_PREC = true;" in src and "    p[3] = c[0];" in src
    sub = type("NoiseSub", (NM.PlateReaderNoise,), {"model_key": "noise_sub"})  # (a subclass inherits the map)
    assert sub._trace.prec is not None and "OWN_PREC" in G.generate_source(sub)
    assert MM.PrprRestated._trace.prec is None
    with pytest.raises(G.ModelDefinitionError, match="defines no precision"):
        MM.PrprRestated.torch_precision(torch.zeros(1, 1, 6, 2), {}, torch.zeros(1, 0))


def test_definition_errors_of_precision_are_raised_when_the_class_is_defined():
    with pytest.raises(G.ModelDefinitionError, match="precision must return a list of 4"):
        _define("noise_three", precision=lambda self, y, x, p, c: [1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="precision must return a list of 4"):
        _define("noise_scalar", precision=lambda self, y, x, p, c: 1.0 / x[0])
    with pytest.raises(G.ModelDefinitionError, match="called from precision: networks are evaluated in rhs only"):
        _define("noise_net", networks={"f": Network(2, 3, 1)},
                rhs=lambda self, t, y, p, c: [self.net.f([y[0], y[1]])[0], -y[1]],
                precision=lambda self, y, x, p, c: [G.exp(self.net.f([y[0], x[1]])[0]), 1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="unknown effective parameter 'nope'"):
        _define("noise_name", precision=lambda self, y, x, p, c: [p.nope, 1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="out of range"):
        _define("noise_cond", precision=lambda self, y, x, p, c: [c[1], 1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("noise_if", precision=lambda self, y, x, p, c: [x[0] if x[0] > 0.0 else 1.0, 1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="precision must be a function"):
        _define("noise_not_callable", precision=[1.0, 1.0, 1.0, 1.0])
    with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
        G.generate_source(NM.PlateReaderNoise, neural=True)


def test_the_slot_limit_relaxes_to_all_slots_for_a_model_with_its_own_precisions():
    """Such a model has no prec_* / init_prec_* slots, so all VIHDS_MAX_SLOTS slots are its own; every other model keeps
    four of them for the precisions."""
    names = ["q%d" % k for k in range(hip.VIHDS_MAX_SLOTS)]
    body = dict(parameters=names, prepare=lambda self, th, c: {"q0": th.q0, "q1": th.q1},
                rhs=lambda self, t, y, p, c: [p.q0 * y[0], -y[1]], initial_state=lambda self, th, c: [th.q2, 0.0],
                observe=None)
    own = dict(body, precision=lambda self, y, x, p, c: [p.q1, p.q1, p.q1, p.q1])
    _define("noise_all_slots", species=["OD", "RFP", "a", "b", "c", "d"],
            **dict(own, initial_state=lambda self, th, c: [th.q2] + [0.0] * 5,
                   rhs=lambda self, t, y, p, c: [p.q0 * y[0]] + [0.0] * 5))
    with pytest.raises(G.ModelDefinitionError, match="at most %d slots" % hip.VIHDS_MAX_SLOTS):
        _define("noise_too_many", species=["OD", "RFP", "a", "b", "c", "d"],
                **dict(own, parameters=names + ["one_more"], initial_state=lambda self, th, c: [th.q2] + [0.0] * 5,
                       rhs=lambda self, t, y, p, c: [p.q0 * y[0]] + [0.0] * 5))
    with pytest.raises(G.ModelDefinitionError, match="4 of them for the precisions"):
        _define("noise_fixed_limit", species=["OD", "RFP", "a", "b", "c", "d"],
                **dict(body, precision=None, parameters=names[:-3], initial_state=lambda self, th, c: [th.q2] + [0.0] * 5,
                       rhs=lambda self, t, y, p, c: [p.q0 * y[0]] + [0.0] * 5))


_Config = _config(n_hidden_decoder_precisions=0)


def test_the_instance_has_model_precisions_and_refuses_another_kind():
    m = NM.PlateReaderNoise(_Config)
    assert isinstance(m.precisions, ModelPrecisions) and m.precisions.dynamic and m.precision_kind == "custom"
    assert m._neural() is False and m.neural_weights() is None and m.flat_weight_tensors() == []
    assert list(m.precisions.parameters()) == []
    states = torch.arange(2 * 3 * 7 * 5, dtype=torch.float32).reshape(2, 3, 7, 5)  # (3 species + 4 precision rows)
    xs, prec = m.expand_precisions(None, [0.0] * 5, states)
    assert torch.equal(xs, states[:, :, :3]) and torch.equal(prec, states[:, :, 3:])
    assert prec.data_ptr() == states[:, :, 3:].data_ptr()  # (a view of the stored rows)
    with pytest.raises(G.ModelDefinitionError, match="must not assign self.precisions"):
        m.precisions = ConstantPrecisions(MM.PREC)
    with pytest.raises(G.ModelDefinitionError, match="must not assign self.precisions"):
        m.precisions = NeuralPrecisions(3, 0, 4)
    # the hybrid model keeps its networks' weights and nothing else
    h = NM.GrowthWithLatentsNoise(_Config)
    assert isinstance(h.precisions, ModelPrecisions)
    assert sum(t.numel() for t in h.flat_weight_tensors()) == sum(n.n_weights for n in h.networks.values())
    # a model without the method is what it was
    assert MM.PrprRestated(_Config).precision_kind == "fixed"


def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def test_generated_text_of_a_precision_map():
    cls = NM.PlateReaderNoise
    src = G.generate_source(cls)
    assert "__device__ static void precision(const float* y, const float* xp, const float* p, float* pr) {" in src
    assert re.search(r"static void precision_vjp\(const float\* y, const float\* xp, const float\* p, const float\* prb, "
                     r"float\* yb,\s+float\* xpb, float\* pb\) \{", src)
    # deterministic across two traces
    assert src == G.generate_source(cls)
    again = type("NoiseAgain", (cls,), {"model_key": cls.model_key})
    assert again._trace is not cls._trace and G.generate_source(again).split("\n", 1)[1] == src.split("\n", 1)[1]
    for c, neural in NM.PREBUILT:
        a = G.generate_source(c, neural)
        assert a == G.generate_source(c, neural) and G.library_tag(a) == G.library_tag(a) and "OWN_PREC" in a
    tr = cls._trace
    NPU = len(tr.p_names)
    fwd, body = _member(src, "precision"), _member(src, "precision_vjp")
    # exactly the parameters precision reads appear in its pb writes; the treatment has no adjoint
    written = sorted(int(k) for k in re.findall(r"(?<!x)pb\[(\d+)\] \+=", body))
    assert written == sorted(tr.p_names.index(n) for n in NOISE_ONLY) and all(k < NPU for k in written)
    assert "p[%d]" % NPU in fwd  # (the treatment, copied by prepare behind the named parameters)
    # the adjoint adds and never assigns; it reaches the species it reads and all four predicted signals
    assert " = " not in re.sub(r"const float v\d+ = ", "", body)
    assert sorted(int(j) for j in re.findall(r"yb\[(\d+)\] \+=", body)) == [0]
    assert sorted(int(j) for j in re.findall(r"xpb\[(\d+)\] \+=", body)) == [0, 1, 2, 3]
    # both members use the time-loop helpers (they run once per time point), not the accurate forms of prepare
    both = fwd + body
    assert "frcp(" in both and "fdiv(" in both and " / " not in both and "expf(" not in both and "tanhf(" not in both
    every = _define("noise_every_helper", precision=lambda self, y, x, p, c: [
        G.exp(-x[0]) / p.s0, G.sigmoid(x[1]) + p.s1, 1.0 + G.tanh(y[1]) * G.tanh(y[1]), G.clamp(p.s0, 0.1, 2.0)])
    both = _member(G.generate_source(every), "precision") + _member(G.generate_source(every), "precision_vjp")
    for helper in ("fexp(", "fdiv(", "sigmoid_f(", "ftanh(", "clampf(", "clamp_pass("):
        assert helper in both, helper
    assert " / " not in both and "expf(" not in both and "tanhf(" not in both
    # the pass-through model: four copies forward, four additions back
    pt = G.generate_source(NM.PrprPassThrough)
    k0 = NM.PrprPassThrough._trace.p_names.index("pt_x")
    assert _member(pt, "precision").split() == " ".join("pr[%d] = p[%d];" % (j, k0 + j) for j in range(4)).split()
    assert _member(pt, "precision_vjp").split() == " ".join("pb[%d] += prb[%d];" % (k0 + j, j) for j in range(4)).split()
    assert "slot_name" in pt and '"prec_x"' not in pt and '"pt_x"' in pt


def test_a_class_without_precision_generates_the_text_it_did():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        recorded = json.load(f)
    classes = {c.__name__: c for c in (MM.DrRestated, MM.EveryOperation, MM.LuxReceiver, MM.LuxReceiverPrecisions,
                                       MM.PrprRestated, MM.PrprRestatedPrecisions)}
    for key, digest in recorded.items():
        name, neural = key.split(":")
        text = G.generate_source(classes[name], bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "OWN_PREC" not in text and "void precision" not in text


def _rand(shape, lo, hi, seed):
    gen = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, generator=gen)


def _inputs(cls, B=3, S=2, T=3):
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    cond = torch.log1p(_rand((B, 1), 0.1, 3.0, 91))
    y = _rand((B, S, len(cls.species) + 4, T), 0.2, 1.5, 92)  # (four rows behind the species: ignored)
    return th, cond, y


def test_torch_precision_against_the_expression_and_finite_differences():
    """torch_precision applies prepare and the model's observation map, then the definition, in the caller's dtype; its
    autograd gradient agrees with central differences in float64 for every noise parameter, a map parameter the precisions
    reach only through x, and the species."""
    cls = NM.PlateReaderNoise
    th, cond, y = _inputs(cls)
    got = cls.torch_precision(y, th, cond)
    x = cls.torch_observe(y, th, cond)
    bs = lambda n: th[n][:, :, None]  # noqa: E731
    c0 = torch.clamp(torch.exp(cond) - 1.0, 1e-12, 1e6)[:, :, None]
    var = lambda a, b, j: bs(a) ** 2 + (bs(b) * x[:, :, j]) ** 2  # noqa: E731
    ref = torch.stack([1.0 / var("s0_od", "s1_od", 0), 1.0 / (var("s0_r", "s1_r", 1) + (bs("s_dens") * y[:, :, 0]) ** 2),
                       1.0 / var("s0_y", "s1_y", 2), 1.0 / (var("s0_c", "s1_c", 3) + bs("s_trt") ** 2 * c0 / (1.0 + c0))], dim=2)
    assert got.dtype == torch.float64 and got.shape == (3, 2, 4, 3) and torch.allclose(got, ref, rtol=1e-13, atol=0)
    assert bool((got > 0).all())
    assert cls.torch_precision(y.float(), th, cond).dtype == torch.float32
    # the fixed maps in front of the definition
    th6, cond6, y6 = _inputs(NM.PrprPassThrough)
    pt = NM.PrprPassThrough.torch_precision(y6, th6, torch.zeros(3, 0, dtype=torch.float64))
    assert torch.equal(pt, torch.stack([th6[n] for n in NM.PASS_THROUGH], dim=2)[:, :, :, None].expand(3, 2, 4, 3))
    thh, condh, yh = _inputs(NM.GrowthWithLatentsNoise)
    xh = yh[:, :, 0:1] * torch.cat([torch.ones_like(yh[:, :, :1]), yh[:, :, 1:4]], dim=2)  # the 'direct' map
    ph = NM.GrowthWithLatentsNoise.torch_precision(yh, thh, condh)
    assert torch.allclose(ph[:, :, 0], 1.0 / (thh["s0_od"][:, :, None] ** 2 + (thh["s1_od"][:, :, None] * xh[:, :, 0]) ** 2),
                          rtol=1e-13, atol=0)
    # gradient against central differences
    W = torch.randn(got.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    loss = lambda t, yy: (cls.torch_precision(yy, t, cond) * W).sum()  # noqa: E731
    names = NOISE_ONLY + ["gain_r", "sat"]
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    grads = torch.autograd.grad(loss(tht, yt), [tht[n] for n in names] + [yt])
    h = 1e-6
    for n, g in zip(names, grads):
        assert float(g.abs().max()) > 0.0, n
        for idx in [(0, 0), (2, 1)]:
            up, dn = dict(th), dict(th)
            up[n], dn[n] = th[n].clone(), th[n].clone()
            up[n][idx] += h
            dn[n][idx] -= h
            fd = float(loss(up, y) - loss(dn, y)) / (2 * h)
            assert abs(fd - float(g[idx])) <= 1e-6 * (1.0 + abs(fd)), (n, idx, fd, float(g[idx]))
    for idx in [(0, 0, 0, 0), (1, 1, 2, 2), (2, 0, 1, 1)]:
        up, dn = y.clone(), y.clone()
        up[idx] += h
        dn[idx] -= h
        fd = float(loss(th, up) - loss(th, dn)) / (2 * h)
        assert abs(fd - float(grads[-1][idx])) <= 1e-6 * (1.0 + abs(fd)), (idx, fd)
    assert float(grads[-1][:, :, 3:].abs().max()) == 0.0  # (the rows behind the species are not read)


def test_traced_precision_vjp_matches_autograd():
    """precision_vjp as the generator derives it (reverse mode over the DAG, evaluated in float64) against torch.autograd
    through the same definition with y, x and the effective parameters as independent inputs."""
    cls = NM.PlateReaderNoise
    tr = cls._trace
    g = tr.g
    N, NPU = len(cls.species), len(tr.p_names)
    B, S, T = 3, 2, 3
    y, x = _rand((B, S, N, T), 0.2, 1.5, 1), _rand((B, S, 4, T), 0.2, 1.5, 2)
    pv = [_rand((B, S, 1), 0.3, 1.2, 10 + k) for k in range(NPU)]
    c0 = _rand((B, 1, 1), 0.2, 2.0, 3)
    W = torch.randn(B, S, 4, T, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    adj = G.vjp(g, tr.prec, [g.leaf("seed", j) for j in range(4)])
    leaves = [g.leaf("y", j) for j in range(N)] + [g.leaf("x", j) for j in range(4)] + [g.leaf("p", k) for k in range(NPU)]
    env = {("y", j): y[:, :, j] for j in range(N)}
    env.update({("x", j): x[:, :, j] for j in range(4)})
    env.update({("p", k): pv[k] for k in range(NPU)})
    env[("p", NPU)] = c0
    env.update({("seed", j): W[:, :, j] for j in range(4)})
    vals = G.evaluate(list(tr.prec) + [adj.get(l.id, g.const(0.0)) for l in leaves], env)
    assert {tr.p_names[k] for k in range(NPU) if g.leaf("p", k).id in adj} == set(NOISE_ONLY)
    yt, xt = y.clone().requires_grad_(True), x.clone().requires_grad_(True)
    pt = [v.clone().requires_grad_(True) for v in pv]
    inst = cls.__new__(cls)
    pr = cls._precision_def(inst, list(torch.unbind(yt, 2)), list(torch.unbind(xt, 2)),
                            G._Named(zip(tr.p_names, pt), "effective parameter"), G._Conditions([c0]))
    pr = torch.stack([v.expand(B, S, T) for v in pr], dim=2)
    assert torch.allclose(torch.stack([v.expand(B, S, T) for v in vals[:4]], dim=2), pr, rtol=1e-13, atol=0)
    ref = torch.autograd.grad(pr, [yt, xt] + pt, W, allow_unused=True)
    err = lambda a, b: ((a - b).abs() / (1.0 + b.abs())).max().item()  # noqa: E731
    for j in range(N):
        assert err(vals[4 + j].expand(B, S, T), ref[0][:, :, j]) <= 1e-12, j
    for j in range(4):
        assert float(ref[1][:, :, j].abs().min()) > 0.0 and err(vals[4 + N + j].expand(B, S, T), ref[1][:, :, j]) <= 1e-12, j
    for k in range(NPU):
        want = ref[2 + k] if ref[2 + k] is not None else torch.zeros(B, S, 1, dtype=torch.float64)
        assert err(vals[8 + N + k].expand(B, S, T).sum(2, keepdim=True), want) <= 1e-12, tr.p_names[k]


FIXED = ["MODEULER", "MODEULERWHILE", "EULER", "MIDPOINT", "RK4"]


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
@pytest.mark.parametrize("which", ["reader", "hybrid"])
def test_precision_map_compiles_without_scratch_for_every_fixed_grid_solver(tmp_path, which):
    """Forward and adjoint kernels of the plate reader with its own noise (its own observe too) and of the hybrid model with
    the same noise (networks in rhs: the adjoint with and without the dump), for every fixed-grid solver: they compile for
    gfx950 and spill nothing.  (VGPRs printed, recorded in DESIGN.md section 4.7.)"""
    cls = NM.PlateReaderNoise if which == "reader" else NM.GrowthWithLatentsNoise
    header = tmp_path / "noise.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(own_prec<VIHDS_GEN_CORE>::value && traj_rows<VIHDS_GEN_CORE>::value == VIHDS_GEN_CORE::N + 4);",
             "static_assert(!own_prec<PrprConstant>::value && traj_rows<WithPrec<PrprConstant>>::value == 10);"]
    for s in FIXED:
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
        lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
        if which == "hybrid":  # (the adjoint that dumps for the networks' weight gradient)
            lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
    lines.append("}")
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", which), "_ZN5vihds")
    assert len(usage) == len(FIXED) * (3 if which == "hybrid" else 2), sorted(usage)
    for name, (vgpr, scratch) in sorted(usage.items()):
        print("%s: %d VGPRs, %d B scratch" % (name, vgpr, scratch))
        assert scratch == 0, name
