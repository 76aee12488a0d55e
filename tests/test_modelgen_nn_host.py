"""CPU tests of the networks of vihds.modelgen: definition errors, unchanged source for models without networks, the
generated adjoint of a network node against torch.autograd in float64, the weights as parameters of the model instance,
compilation of the largest supported networks for gfx950 without scratch, and no inline assembly beyond the empty memory
clobber."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import types
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from vihds import modelgen as G
from vihds.modelgen import Network

import modelgen_hybrid_models as HM
import modelgen_models as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
HAVE_HIPCC = bool(shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"))


def _define(name, **body):
    attrs = dict(model_key=name, species=["OD", "RFP", "YFP", "CFP"], parameters=["r", "init_x"], n_conditions=1,
                 observe_kind="direct", networks={"f": Network(2, 3, 1)},
                 prepare=lambda self, th, c: {"r": th.r},
                 initial_state=lambda self, th, c: [th.init_x, 0.0, 0.0, 0.0],
                 rhs=lambda self, t, y, p, c: [p.r * y[0] * self.net.f([y[0], t])[0], 0.0, 0.0, 0.0])
    attrs.update(body)
    return type(name, (G.GeneratedOdeModel,), attrs)


def test_network_definition_errors_are_raised_when_the_class_is_defined():
    ok = _define("nn_ok")
    assert "static constexpr int NW = 13;" in G.generate_source(ok)
    with pytest.raises(G.ModelDefinitionError, match="takes a list of 2 inputs"):
        _define("nn_inputs", rhs=lambda self, t, y, p, c: [self.net.f([y[0]])[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="unknown network 'g'"):
        _define("nn_unknown", rhs=lambda self, t, y, p, c: [self.net.g([y[0], t])[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="never called"):
        _define("nn_unused", rhs=lambda self, t, y, p, c: [p.r * y[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="at most once per rhs"):
        _define("nn_twice", rhs=lambda self, t, y, p, c: [self.net.f([y[0], t])[0] + self.net.f([y[1], t])[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="rhs only"):
        _define("nn_prepare", prepare=lambda self, th, c: {"r": self.net.f([th.r, th.r])[0]})
    with pytest.raises(G.ModelDefinitionError, match="rhs only"):
        _define("nn_init", initial_state=lambda self, th, c: [self.net.f([th.r, th.r])[0], 0.0, 0.0, 0.0])
    for what, net, top in (("n_inputs", Network(17, 3, 1), 16), ("n_hidden", Network(2, 33, 1), 32),
                           ("n_outputs", Network(2, 3, 9), 8), ("n_hidden", Network(2, 0, 1), 32)):
        with pytest.raises(G.ModelDefinitionError, match=r"%s = \d+; supported: 1 \.\. %d" % (what, top)):
            _define("nn_size", networks={"f": net})
    with pytest.raises(G.ModelDefinitionError, match="at most 2"):
        _define("nn_three", networks={k: Network(2, 3, 1) for k in "fgh"})
    with pytest.raises(G.ModelDefinitionError, match="relu, tanh"):
        _define("nn_act", networks={"f": Network(2, 3, 1, hidden="gelu")})
    # inputs may be any model quantity: states, t, prepared parameters, treatments, expressions of them
    mixed = _define("nn_mixed", rhs=lambda self, t, y, p, c: [self.net.f([G.exp(-y[0]) * p.r + c[0], t * 2.0])[0], 0.0, 0.0, 0.0])
    assert "net0_forward" in G.generate_source(mixed)


def test_models_without_networks_generate_the_parent_commits_text():
    """tests/golden/modelgen_source_sha256.json holds sha256(generate_source(cls, neural)) of every model of
    tests/modelgen_models.py as the commit before networks existed produced it."""
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 12
    for key, digest in recorded.items():
        name, neural = key.split(":")
        text = G.generate_source(getattr(MM, name), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "NET_FIELDS" not in text and "static constexpr int NW = 0;" in text


def _weights(net, gen, scale=0.7):
    return tuple(scale * torch.randn(shape, dtype=torch.float64, generator=gen) for shape in net.tensor_shapes())


@pytest.mark.parametrize("hidden", ["relu", "tanh"])
@pytest.mark.parametrize("sizes", [(5, 8, 4), (3, 4, 1), (16, 32, 8)])
def test_generated_network_adjoint_matches_autograd(hidden, sizes):
    """Outputs, input adjoints and the four weight adjoints of a network node (evaluate / vjp of the DAG, the formulas the
    kernel and the dump's contraction implement) against float64 autograd of the torch form of the same call: 1e-12
    relative, the bound of the operation-VJP tests.  Inputs are expressions of the leaves, outputs go through heads."""
    net = Network(*sizes, hidden=hidden)
    I, H, O = sizes
    gen = torch.Generator().manual_seed(I * 100 + H)
    W = _weights(net, gen)
    xs = [torch.randn(48, dtype=torch.float64, generator=gen) for _ in range(I)]
    seeds = [torch.randn(48, dtype=torch.float64, generator=gen) for _ in range(O)]

    def model(leaves, call):
        ins = [leaves[0] * leaves[i] if i % 2 else G.tanh(leaves[i]) + 0.5 for i in range(I)]
        out = call(ins)
        return [G.sigmoid(out[j]) * leaves[j % I] if j % 2 else out[j] for j in range(O)]

    g = G.Graph([net])
    leaves = [g.leaf("y", k) for k in range(I)]
    outs = model(leaves, lambda ins: g.net(0, ins))
    seed_leaves = [g.leaf("seed", j) for j in range(O)]
    adj = G.vjp(g, outs, seed_leaves)
    env = {("y", k): x for k, x in enumerate(xs)}
    env.update({("seed", j): s for j, s in enumerate(seeds)})
    env[("w", 0)] = W
    env["wgrad"] = {}
    vals = G.evaluate(outs + [adj[l.id] for l in leaves], env)
    # torch form
    xt = [x.clone().requires_grad_(True) for x in xs]
    Wt = tuple(w.clone().requires_grad_(True) for w in W)
    call = G.GeneratedOdeModel._torch_call(lambda: {"n": Wt})
    ref = model(xt, lambda ins: call(0, "n", net, ins))
    grads = torch.autograd.grad(ref, xt + list(Wt), seeds)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()  # noqa: E731
    for j in range(O):
        assert rel(vals[j], ref[j].detach()) <= 1e-12, ("output", j)
    for k in range(I):
        assert rel(vals[O + k], grads[k]) <= 1e-12, ("input adjoint", k)
    for k, name in enumerate(("W1", "b1", "W2", "b2")):
        assert env["wgrad"][0][k].shape == W[k].shape
        assert rel(env["wgrad"][0][k], grads[I + k]) <= 1e-12, name


def test_relu_passes_no_gradient_at_a_preactivation_of_exactly_zero():
    """Hidden unit 0 has pre-activation exactly 0 for every sample (zero weights and bias): its adjoint is 0, as torch's
    relu backward gives; the other units are unaffected."""
    net = Network(3, 4, 2, hidden="relu")
    gen = torch.Generator().manual_seed(9)
    W1, b1, W2, b2 = _weights(net, gen)
    W1[0], b1[0] = 0.0, 0.0
    x = torch.randn(20, 3, dtype=torch.float64, generator=gen)
    ob = torch.randn(20, 2, dtype=torch.float64, generator=gen)
    z, _h, _o = G.net_forward_ref(net, (W1, b1, W2, b2), x)
    assert bool((z[:, 0] == 0).all())
    xb, (gW1, gb1, gW2, gb2) = G.net_vjp_ref(net, (W1, b1, W2, b2), x, ob)
    xt = x.clone().requires_grad_(True)
    Wt = [w.clone().requires_grad_(True) for w in (W1, b1, W2, b2)]
    out = torch.relu(xt @ Wt[0].t() + Wt[1]) @ Wt[2].t() + Wt[3]
    ref = torch.autograd.grad(out, [xt] + Wt, ob)
    assert bool((gW1[0] == 0).all()) and gb1[0] == 0 and bool((ref[1][0] == 0).all()) and ref[2][0] == 0
    for a, b in zip([xb, gW1, gb1, gW2, gb2], ref):
        assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-12
    assert "(z > 0.f ? hub : 0.f)" in G.generate_source(HM.GrowthWithLatents)


class _Params(dict):
    __getattr__ = dict.__getitem__


def _config(**params):
    data = types.SimpleNamespace(device_depth=2, conditions=["C6"], relevance_vectors=None, default_devices=None)
    return types.SimpleNamespace(data=data, params=_Params(params), device=torch.device("cpu"))


@pytest.mark.parametrize("cls,hidden_prec", [(HM.GrowthWithLatents, None), (HM.GrowthWithLatentsPrecisions, 0),
                                              (HM.GrowthWithLatentsPrecisions, 20)])
def test_network_weights_are_parameters_of_the_instance_in_buffer_order(cls, hidden_prec):
    torch.manual_seed(3)
    model = cls(_config(n_hidden_decoder_precisions=hidden_prec))
    torch.manual_seed(3)
    again = cls(_config(n_hidden_decoder_precisions=hidden_prec))
    named = dict(model.named_parameters())
    assert list(named)[:8] == ["nets.latent.hidden.weight", "nets.latent.hidden.bias", "nets.latent.out.weight",
                               "nets.latent.out.bias", "nets.gate.hidden.weight", "nets.gate.hidden.bias",
                               "nets.gate.out.weight", "nets.gate.out.bias"]
    params = list(model.parameters())
    assert len({id(p) for p in params}) == len(params)  # each exactly once
    flat = model.flat_weight_tensors()
    assert [tuple(t.shape) for t in flat[:8]] == [(8, 5), (8,), (4, 8), (4,), (4, 3), (4,), (1, 4), (1,)]
    assert all(a is b for a, b in zip(flat, params))  # the tail's Adam walks them as ONE run of parameters()
    n_prec = 0 if hidden_prec is None else sum(t.numel() for t in model.precisions.weight_tensors())
    w = model.neural_weights()
    assert w.numel() == 105 + n_prec == sum(t.numel() for t in flat)
    assert torch.equal(w.detach(), torch.cat([t.detach().reshape(-1) for t in flat]))
    for a, b in zip(flat, again.flat_weight_tensors()):
        assert torch.equal(a, b)  # seeded by the caller's torch.manual_seed, like every other module
    # xavier_uniform_ on the matrices (bound sqrt(6 / (fan_in + fan_out))), nn.Linear's default on the biases
    W1 = model.nets["latent"].hidden.weight
    assert float(W1.abs().max()) <= (6.0 / (5 + 8)) ** 0.5 and float(W1.abs().max()) > 0.3
    assert float(model.nets["latent"].hidden.bias.abs().max()) <= 5 ** -0.5


def test_the_definition_runs_eagerly_in_float64_with_autograd_weight_gradients():
    B, S = 3, 2
    gen = torch.Generator().manual_seed(1)
    th = {n: 0.5 + torch.rand(B, S, dtype=torch.float64, generator=gen) for n in HM.GrowthWithLatents.parameter_names}
    cond = torch.rand(B, 1, dtype=torch.float64, generator=gen)
    with pytest.raises(ValueError, match="weights="):
        HM.GrowthWithLatents.torch_problem(th, cond)
    W = {name: tuple(w.requires_grad_(True) for w in _weights(net, gen))
         for name, net in HM.GrowthWithLatents.networks.items()}
    rhs, x0 = HM.GrowthWithLatents.torch_problem(th, cond, weights=W)
    dy = rhs(torch.tensor(0.3, dtype=torch.float64), x0 + 0.1)
    assert dy.shape == (B, S, 6) and dy.dtype == torch.float64
    grads = torch.autograd.grad(dy.sum(), [w for ws in W.values() for w in ws])
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # with W2 = 0, b2 = 0 the heads are sigmoid(0): the network-free twin
    Z = {name: (ws[0], ws[1], torch.zeros_like(ws[2]), torch.zeros_like(ws[3])) for name, ws in W.items()}
    rhs0, _ = HM.GrowthWithLatents.torch_problem(th, cond, weights=Z)
    rhs1, x1 = HM.GrowthWithoutNetworks.torch_problem(th, cond)
    assert torch.equal(x0, x1)
    assert torch.allclose(rhs0(0.3, x0 + 0.1), rhs1(0.3, x0 + 0.1), rtol=1e-15, atol=0)
    # an instance's own parameters drive the same definition
    torch.manual_seed(0)
    model = HM.GrowthWithLatents(_config())
    rhs2, _ = HM.GrowthWithLatents.torch_problem({k: v.float() for k, v in th.items()}, cond.float(), model.network_weights())
    assert rhs2(0.3, x0.float()).dtype == torch.float32


def _resource_usage(text):
    """{kernel: (vgprs, agprs, scratch)} from -Rpass-analysis=kernel-resource-usage remarks."""
    out = {}
    for block in re.split(r"Function Name: ", text)[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", block).group(1))  # noqa: E731
        out[block.split()[0]] = (g(r" VGPRs"), g(r"AGPRs"), g(r"ScratchSize \[bytes/lane\]"))
    return out


SOLVERS = ["VIHDS_SOLVER_MODEULER", "VIHDS_SOLVER_MODEULERWHILE", "VIHDS_SOLVER_EULER", "VIHDS_SOLVER_MIDPOINT", "VIHDS_SOLVER_RK4"]


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not installed")
def test_largest_networks_compile_for_every_fixed_grid_solver_without_scratch(tmp_path):
    """Two 16 -> 32 -> 8 networks (ReLU and tanh), with constant precisions and inside WithPrec<>: the forward kernel and
    the adjoint kernel in both of its forms (with the weight-gradient dump, and without an aux buffer) of every fixed-grid
    solver report 0 bytes of scratch.  The register counts are printed and carried in the assertion message."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

    def compile_one(job):
        cls, neural, solver = job
        name = "%s_%s" % (cls.__name__, solver)
        header = tmp_path / (name + ".hpp")
        header.write_text(G.generate_source(cls, neural))
        M = "WithPrec<VIHDS_GEN_CORE>" if neural else "VIHDS_GEN_CORE"
        src = tmp_path / (name + ".hip")
        src.write_text('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n' % header
                       + "template __global__ void ode_fwd_kernel<%s, %s, true>(OdeArgs);\n" % (M, solver)
                       + "template __global__ void ode_bwd_kernel<%s, %s, true>(OdeArgs);\n" % (M, solver)
                       + "template __global__ void ode_bwd_kernel<%s, %s, false>(OdeArgs);\n}\n" % (M, solver))
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c", str(src), "-o",
                              str(tmp_path / (name + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout[-3000:]
        return job, _resource_usage(res.stdout)

    jobs = [(cls, neural, s) for cls, neural in ((HM.LargestNetworks, False), (HM.LargestNetworksPrecisions, True))
            for s in SOLVERS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(compile_one, jobs))
    report = []
    for (cls, neural, solver), usage in results:
        assert len(usage) == 3, usage
        for kernel, (vgpr, agpr, scratch) in sorted(usage.items()):
            kind = "fwd" if "ode_fwd" in kernel else ("bwd+dump" if "Lb1EEEv" in kernel else "bwd")
            report.append("%s %s %s: %d VGPRs, %d AGPRs, %d B scratch" % (cls.__name__, solver[13:].lower(), kind, vgpr, agpr, scratch))
    text = "\n".join(report)
    print(text)
    assert all(line.endswith(" 0 B scratch") for line in report), text


def test_generated_text_has_no_inline_assembly_beyond_the_empty_memory_clobber():
    clobber = '__asm__ volatile("" ::: "memory");'
    for cls, neural in ((HM.GrowthWithLatents, False), (HM.GrowthWithLatentsPrecisions, True), (HM.LargestNetworks, False)):
        text = G.generate_source(cls, neural)
        assert clobber in text
        rest = text.replace(clobber, "")
        assert "asm" not in rest.lower() and "__builtin_amdgcn" not in rest and "atomic" not in rest.lower()
    # weights are read through the constant address space only (scalar loads), never written
    text = G.generate_source(HM.GrowthWithLatents)
    assert "typedef const __attribute__((address_space(4))) float* weights_ptr;" in text
    assert not re.search(r"\b[Wwb][12]?\[[^\]]*\]\s*[-+*]?=[^=]", text)
