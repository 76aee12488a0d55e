"""CPU tests of a generated model's own observation log density (GeneratedOdeModel.log_likelihood): definition errors, the
generated text, torch_log_likelihood, the traced adjoint chained with the precision map's, the observation map's and
prepare's against autograd in float64, the host paths that restate the Gaussian, and compilation for gfx950 (no scratch in the
forward and adjoint kernels of every fixed-grid solver)."""
import hashlib
import json
import math
import os
import re
import shutil
from types import SimpleNamespace

import pytest
import torch

from vihds import modelgen as G
from vihds import training as TR
from vihds.modelgen import Network

import modelgen_likelihood_models as LM
import modelgen_models as MM
import modelgen_noise_models as NM
from test_modelgen_host import _compile_usage, _resource_usage
from test_modelgen_nn_host import _config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_Config = _config(n_hidden_decoder_precisions=0)
_GAUSS = lambda self, x, obs, pr, p, c: [  # noqa: E731
    -0.5 * (LM.LOG2PI - G.log(pr[j]) + pr[j] * (x[j] - obs[j]) * (x[j] - obs[j])) for j in range(4)]


def _define(name, **body):
    attrs = dict(model_key=name, species=["OD", "RFP"], parameters=["r", "nu", "init_x"], n_conditions=1,
                 prepare=lambda self, th, c: {"r": th.r, "nu": th.nu},
                 initial_state=lambda self, th, c: [th.init_x, 0.0],
                 rhs=lambda self, t, y, p, c: [p.r * y[0], -y[1]],
                 observe=lambda self, y, p, c: [y[0], y[0] * y[1], y[1], 1.0],
                 log_likelihood=_GAUSS)
    attrs.update(body)
    return type(name, (G.GeneratedOdeModel,), attrs)


def test_a_class_with_log_likelihood_is_traced():
    cls = _define("lik_ok", log_likelihood=lambda self, x, obs, pr, p, c: [
        -p.nu * (x[0] - obs[0]) * (x[0] - obs[0]), G.log(pr[1]) - c[0] * x[1], obs[2], 0.0])
    tr = cls._trace
    assert tr.lik is not None and len(tr.lik) == 4 and tr.lik[3].op == "const" and tr.lik[2].op == "ob"
    assert tr.c_in_rhs == [0]  # (the treatment log_likelihood reads is copied by prepare: the union with the other functions)
    src = G.generate_source(cls)
    assert "static constexpr bool OWN_LIK = true;" in src and "    p[2] = c[0];" in src
    sub = type("LikSub", (LM.PlateReaderStudentT,), {"model_key": "lik_sub"})  # (a subclass inherits the definition)
    assert sub._trace.lik is not None and "OWN_LIK" in G.generate_source(sub) and "OWN_PREC" in G.generate_source(sub)
    assert MM.PrprRestated._trace.lik is None and NM.PlateReaderNoise._trace.lik is None
    back = type("LikBack", (LM.PlateReaderStudentT,), {"model_key": "lik_back", "log_likelihood": None})  # (the Gaussian again)
    assert back._trace.lik is None and "OWN_LIK" not in G.generate_source(back) and LM.PlateReaderStudentT._trace.lik is not None
    helper = _define("lik_helper_argument", log_likelihood=lambda self, x, obs, pr, p, c, scale=2.0, *, shift=0.0: [
        scale * (x[j] - obs[j]) + shift for j in range(4)])  # (arguments with defaults are the author's own)
    assert helper._trace.lik is not None
    assert MM.PrprRestated(_Config).likelihood_kind == "gaussian"
    assert LM.PrprContaminated(_Config).likelihood_kind == "custom"
    assert LM.PlateReaderStudentT(_Config).likelihood_kind == "custom"
    assert LM.PlateReaderStudentT(_Config).precision_kind == "custom"
    with pytest.raises(G.ModelDefinitionError, match="defines no log_likelihood"):
        MM.PrprRestated.torch_log_likelihood(torch.zeros(1, 1, 4, 2), torch.zeros(1, 4, 2), torch.ones(1, 1, 4, 2), {},
                                             torch.zeros(1, 0))


def test_definition_errors_of_log_likelihood_are_raised_when_the_class_is_defined():
    with pytest.raises(G.ModelDefinitionError, match="log_likelihood must return a list of 4"):
        _define("lik_three", log_likelihood=lambda self, x, obs, pr, p, c: [x[0], x[1], x[2]])
    with pytest.raises(G.ModelDefinitionError, match="log_likelihood must return a list of 4"):
        _define("lik_scalar", log_likelihood=lambda self, x, obs, pr, p, c: x[0] - obs[0])
    with pytest.raises(G.ModelDefinitionError, match="called from log_likelihood: networks are evaluated in rhs only"):
        _define("lik_net", networks={"f": Network(2, 3, 1)},
                rhs=lambda self, t, y, p, c: [self.net.f([y[0], y[1]])[0], -y[1]],
                log_likelihood=lambda self, x, obs, pr, p, c: [self.net.f([x[0], obs[0]])[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="no t and no species"):
        _define("lik_t", log_likelihood=lambda self, t, x, obs, pr, p, c: [t * x[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="unknown effective parameter 'nope'"):
        _define("lik_name", log_likelihood=lambda self, x, obs, pr, p, c: [p.nope * x[0], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="out of range"):
        _define("lik_cond", log_likelihood=lambda self, x, obs, pr, p, c: [c[1], 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("lik_if", log_likelihood=lambda self, x, obs, pr, p, c: [x[0] if x[0] > obs[0] else 0.0, 0.0, 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="log_likelihood must be a function"):
        _define("lik_not_callable", log_likelihood=[0.0, 0.0, 0.0, 0.0])
    for cls in (LM.PrprGaussianThrough, LM.PlateReaderStudentT):
        with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
            G.generate_source(cls, neural=True)


def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def test_generated_text_of_a_log_likelihood():
    for cls in (LM.PrprGaussianThrough, LM.PlateReaderStudentT, LM.PrprContaminated, LM.PrprLogNormal):
        src = G.generate_source(cls)
        assert "__device__ static void loglik(const float* xp, const float* ob, const float* pr, const float* p, float* ll) {" in src
        assert re.search(r"static void loglik_vjp\(const float\* xp, const float\* ob, const float\* pr, const float\* p, "
                         r"const float\* llb,\s+float\* xpb, float\* prb, float\* pb\) \{", src)
        assert src == G.generate_source(cls)  # deterministic
        tr = cls._trace
        NPU = len(tr.p_names)
        fwd, body = _member(src, "loglik"), _member(src, "loglik_vjp")
        # the adjoint adds and never assigns; the observations are data and get no adjoint
        assert " = " not in re.sub(r"const float v\d+ = ", "", body)
        assert "obb" not in src and not re.search(r"\bob\[\d\] \+?= ", src)
        adj = G.vjp(tr.g, tr.lik, [tr.g.leaf("seed", j) for j in range(4)])
        assert all(tr.g.leaf("ob", j).id not in adj for j in range(4))
        assert sorted(int(j) for j in re.findall(r"xpb\[(\d+)\] \+=", body)) == [0, 1, 2, 3]
        assert sorted(int(j) for j in re.findall(r"prb\[(\d+)\] \+=", body)) == [0, 1, 2, 3]
        # pb is written exactly for the parameters the definition reads
        written = sorted(int(k) for k in re.findall(r"(?<![xr])pb\[(\d+)\] \+=", body))
        reads = [tr.p_names.index(n) for n in ("w", "kappa")] if cls is LM.PrprContaminated else []
        assert written == sorted(reads) and all(k < NPU for k in written)
        # both members use the time-loop helpers, not the accurate forms of prepare
        both = fwd + body
        assert "fdiv(" in both and " / " not in both and "expf(" not in both and "tanhf(" not in both
        assert ("OWN_PREC" in src) == (cls is LM.PlateReaderStudentT)
    both = _member(G.generate_source(LM.PrprContaminated), "loglik") + _member(G.generate_source(LM.PrprContaminated), "loglik_vjp")
    assert "fexp(" in both and "logf(" in both
    every = _define("lik_every_helper", log_likelihood=lambda self, x, obs, pr, p, c: [
        G.exp(-x[0]) / p.nu, G.sigmoid(x[1] - obs[1]), G.tanh(pr[2]) * G.tanh(x[2]), G.clamp(x[3], 0.1, 2.0) / pr[3]])
    both = _member(G.generate_source(every), "loglik") + _member(G.generate_source(every), "loglik_vjp")
    for helper in ("fexp(", "fdiv(", "sigmoid_f(", "ftanh(", "clampf(", "clamp_pass("):
        assert helper in both, helper
    assert " / " not in both and "expf(" not in both and "tanhf(" not in both
    # a nonlinear operation on the forward-only leaf
    assert "logf(ob[0])" in _member(G.generate_source(LM.PrprLogNormal), "loglik")
    # the Student-t's constants are numbers in the text
    assert G._lit(LM.STUDENT_T_CONST) in _member(G.generate_source(LM.PlateReaderStudentT), "loglik")
    for c, neural in LM.PREBUILT:
        a = G.generate_source(c, neural)
        assert G.library_tag(a) == G.library_tag(a) and "OWN_LIK" in a


def test_a_class_without_log_likelihood_generates_the_text_it_did():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        recorded = json.load(f)
    classes = {c.__name__: c for c in (MM.DrRestated, MM.EveryOperation, MM.LuxReceiver, MM.LuxReceiverPrecisions,
                                       MM.PrprRestated, MM.PrprRestatedPrecisions)}
    assert recorded
    for key, digest in recorded.items():
        name, neural = key.split(":")
        text = G.generate_source(classes[name], bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "OWN_LIK" not in text and "loglik" not in text
    for c, neural in NM.PREBUILT:
        text = G.generate_source(c, neural)
        assert "OWN_LIK" not in text and "loglik" not in text


def _rand(shape, lo, hi, seed):
    gen = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, generator=gen)


def _default_map(y):
    return [y[:, :, 0], y[:, :, 0] * y[:, :, 1], y[:, :, 0] * (y[:, :, 2] + y[:, :, 4]), y[:, :, 0] * (y[:, :, 3] + y[:, :, 5])]


def _inputs(cls, B=3, S=2, T=3):
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    cond = torch.log1p(_rand((B, int(cls.n_conditions)), 0.1, 3.0, 91))
    y = _rand((B, S, len(cls.species), T), 0.2, 1.5, 92)
    ob = _rand((B, 4, T), 0.2, 1.5, 93)
    prec = _rand((B, S, 4, 1), 5.0, 50.0, 94)
    W = torch.randn(B, S, 4, T, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    return th, cond, y, ob, prec, W


def _chain(cls, th, cond, y, ob, prec, W):
    """What the kernels compute, from the traced DAG in float64: prepare, the observation map, the precisions, loglik; then
    loglik_vjp, precision_vjp, observe_vjp (each adding into what the one before left) and prepare_vjp on pb summed over the
    time points.  -> ll, the log density's own xpb and prb, yb (None with a fixed map), {parameter: thb}."""
    tr = cls._trace
    g = tr.g
    B, S, N, T = y.shape
    NPU, C = len(tr.p_names), int(cls.n_conditions)
    full = lambda v: v.expand(B, S, T)  # noqa: E731
    seeds4 = [g.leaf("seed", j) for j in range(4)]
    c = torch.clamp(torch.exp(cond) - 1.0, 1e-12, 1e6)
    env0 = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
    env0.update({("c", q): c[:, q:q + 1].expand(B, S) for q in range(C)})
    pv = G.evaluate(tr.p_exprs, env0)
    env = {("p", k): pv[k].expand(B, S)[:, :, None] for k in range(NPU)}
    env.update({("p", NPU + q): env0[("c", q)][:, :, None] for q in range(C)})
    env.update({("y", j): y[:, :, j] for j in range(N)})
    x = G.evaluate(tr.obs, env) if tr.obs is not None else _default_map(y)
    env.update({("x", j): full(x[j]) for j in range(4)})
    pr = G.evaluate(tr.prec, env) if tr.prec is not None else [prec[:, :, j] for j in range(4)]
    env.update({("pr", j): full(pr[j]) for j in range(4)})
    env.update({("ob", j): ob[:, None, j, :] for j in range(4)})
    ll = torch.stack([full(v) for v in G.evaluate(tr.lik, env)], dim=2)

    def pull(outputs, seed_values, leaves):
        adj = G.vjp(g, outputs, seeds4 if len(outputs) == 4 else [g.leaf("seed", k) for k in range(len(outputs))])
        e = dict(env)
        e.update({("seed", j): v for j, v in enumerate(seed_values)})
        vals = G.evaluate([adj.get(l.id, g.const(0.0)) for l in leaves], e)
        return [full(v) for v in vals]

    xl, prl, pl, yl = ([g.leaf("x", j) for j in range(4)], [g.leaf("pr", j) for j in range(4)],
                       [g.leaf("p", k) for k in range(NPU)], [g.leaf("y", j) for j in range(N)])
    out = pull(tr.lik, [W[:, :, j] for j in range(4)], xl + prl + pl)
    xpb, prb, pb = out[:4], out[4:8], out[8:]
    own = ([v.clone() for v in xpb], [v.clone() for v in prb])
    yb = None
    if tr.prec is not None:
        out = pull(tr.prec, prb, yl + xl + pl)
        yb = out[:N]
        xpb = [a + b for a, b in zip(xpb, out[N:N + 4])]
        pb = [a + b for a, b in zip(pb, out[N + 4:])]
    if tr.obs is not None:
        out = pull(tr.obs, xpb, yl + pl)
        yb = [a + b for a, b in zip(yb, out[:N])] if yb is not None else out[:N]
        pb = [a + b for a, b in zip(pb, out[N:])]
    adj = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    e = dict(env0)
    e.update({("seed", k): pb[k].sum(2) for k in range(NPU)})
    tl = [g.leaf("th", s) for s in range(len(cls.parameter_names))]
    thb = G.evaluate([adj.get(l.id, g.const(0.0)) for l in tl], e)
    return ll, own, yb, {n: v.expand(B, S) for n, v in zip(cls.parameter_names, thb)}


_err = lambda a, b: ((a - b).abs() / (1.0 + b.abs())).max().item()  # noqa: E731


def test_traced_adjoint_of_the_student_t_chained_through_precision_observe_and_prepare_matches_autograd():
    """PlateReaderStudentT: loglik_vjp, then precision_vjp, then observe_vjp, then prepare_vjp as the generator derives them,
    against autograd through torch_observe, torch_precision and torch_log_likelihood with the species and theta as inputs."""
    cls = LM.PlateReaderStudentT
    th, cond, y, ob, prec, W = _inputs(cls)
    ll, _own, yb, thb = _chain(cls, th, cond, y, ob, prec, W)
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    x, pr = cls.torch_observe(yt, tht, cond), cls.torch_precision(yt, tht, cond)
    ref = cls.torch_log_likelihood(x, ob, pr, tht, cond)
    assert ref.dtype == torch.float64 and ref.shape == W.shape and _err(ll, ref.detach()) <= 1e-12
    e = x.detach() - ob[:, None]
    want = (LM.STUDENT_T_CONST + 0.5 * pr.detach().log() - 2.5 * torch.log1p(pr.detach() * e * e / 4.0))
    assert torch.allclose(ref.detach(), want, rtol=1e-12, atol=1e-12)
    names = list(cls.parameter_names)
    grads = torch.autograd.grad((ref * W).sum(), [yt] + [tht[n] for n in names], allow_unused=True)
    for j in range(len(cls.species)):
        assert _err(yb[j], grads[0][:, :, j]) <= 1e-11, j
    for n, gr in zip(names, grads[1:]):
        want = gr if gr is not None else torch.zeros_like(th[n])
        assert _err(thb[n], want) <= 1e-11, n
    for n in NM.NOISE + ["gain_r", "sat"]:  # (reached only through the precision map or the observation map)
        assert float(grads[1 + names.index(n)].abs().min()) > 0.0, n
    assert cls.torch_log_likelihood(x.detach().float(), ob, pr.detach(), th, cond).dtype == torch.float32


@pytest.mark.parametrize("cls", [LM.PrprContaminated, LM.PrprLogNormal, LM.PrprGaussianThrough], ids=lambda c: c.__name__)
def test_traced_adjoint_with_constant_precisions_matches_autograd(cls):
    """Constant precisions and the fixed map: xpb, prb (what the kernel adds into precb) and, through prepare_vjp, the
    likelihood-only parameters against autograd through torch_log_likelihood."""
    th, cond, y, ob, prec, W = _inputs(cls)
    ll, (xpb, prb), yb, thb = _chain(cls, th, cond, y, ob, prec, W)
    assert yb is None
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    xt = torch.stack(_default_map(y), dim=2).requires_grad_(True)
    pt = prec.clone().requires_grad_(True)
    ref = cls.torch_log_likelihood(xt, ob, pt, tht, cond)
    assert _err(ll, ref.detach()) <= 1e-12
    names = list(cls.parameter_names)
    grads = torch.autograd.grad((ref * W).sum(), [xt, pt] + [tht[n] for n in names], allow_unused=True)
    for j in range(4):
        assert _err(xpb[j], grads[0][:, :, j]) <= 1e-11 and float(grads[0][:, :, j].abs().min()) > 0.0, j
        assert _err(prb[j].sum(2, keepdim=True), grads[1][:, :, j]) <= 1e-11, j
    for n, gr in zip(names, grads[2:]):
        want = gr if gr is not None else torch.zeros_like(th[n])
        assert _err(thb[n], want) <= 1e-11, n
    e = xt.detach() - ob[:, None]
    gauss = TR.log_prob_gaussian(ob[:, None], xt.detach(), prec)
    if cls is LM.PrprGaussianThrough:
        assert torch.allclose(ref.detach(), gauss, rtol=1e-13, atol=1e-13)
    elif cls is LM.PrprContaminated:
        for n in LM.CONTAMINATION:
            assert float(grads[2 + names.index(n)].abs().min()) > 0.0, n
        w, k = torch.sigmoid(th["eps"])[:, :, None, None], th["kappa"][:, :, None, None]
        wide = TR.log_prob_gaussian(ob[:, None], xt.detach(), prec / (k * k))
        want = torch.logaddexp(torch.log1p(-w) + gauss, torch.log(w) + wide)
        assert torch.allclose(ref.detach(), want, rtol=1e-12, atol=1e-12)
    else:
        le = xt.detach().log() - ob[:, None].log()
        want = -0.5 * (math.log(2 * math.pi) - prec.log() + prec * le * le) - ob[:, None].log()
        assert torch.allclose(ref.detach(), want, rtol=1e-12, atol=1e-12)
    assert e.abs().max() > 0.0


def test_host_paths_take_the_model_definition():
    """training.log_prob_observations (the plugin fallback of Training.cost) evaluates a custom model's own log density with
    theta and the treatments of the last solve; a model without the method keeps the Gaussian."""
    cls = LM.PrprContaminated
    th, cond, y, ob, prec, _W = _inputs(cls)
    x = torch.stack(_default_map(y), dim=2)
    m = cls(_Config)
    wrap = SimpleNamespace(decoder=SimpleNamespace(ode_model=m))
    with pytest.raises(RuntimeError, match="nothing has been solved yet"):
        TR.log_prob_observations(wrap, x, ob, prec)
    names = list(cls.parameter_names)
    m._last_inputs = (torch.stack([th[n] for n in names]), {n: i for i, n in enumerate(names)}, cond)
    got = TR.log_prob_observations(wrap, x, ob, prec)
    want = cls.torch_log_likelihood(x, ob, prec, th, cond).sum(3)
    assert got.shape == (3, 2, 4) and torch.equal(got, want)
    gauss = TR.log_prob_gaussian(ob[:, None], x, prec).sum(3)
    assert float((got - gauss).abs().min()) > 0.0
    plain = SimpleNamespace(decoder=SimpleNamespace(ode_model=MM.PrprRestated(_Config)))
    assert torch.equal(TR.log_prob_observations(plain, x, ob, prec), gauss)
    assert torch.equal(TR.log_prob_observations(None, x, ob, prec), gauss)
    with pytest.raises(NotImplementedError):
        TR.log_prob_observations(wrap, x, ob, prec, use_laplace=True)


FIXED = ["MODEULER", "MODEULERWHILE", "EULER", "MIDPOINT", "RK4"]


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
@pytest.mark.parametrize("which", ["student_t", "contaminated"])
def test_log_likelihood_compiles_without_scratch_for_every_fixed_grid_solver(tmp_path, which):
    """Forward and adjoint kernels of PlateReaderStudentT (its own observe and precision too) and of PrprContaminated
    (constant precisions, two likelihood-only parameters), for every fixed-grid solver: they compile for gfx950 and spill
    nothing.  (VGPRs printed, recorded in DESIGN.md section 4.7.)"""
    cls = LM.PlateReaderStudentT if which == "student_t" else LM.PrprContaminated
    header = tmp_path / "lik.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(own_lik<VIHDS_GEN_CORE>::value && own_prec<VIHDS_GEN_CORE>::value == %s);" % (
                 "true" if which == "student_t" else "false"),
             "static_assert(!own_lik<PrprConstant>::value && !own_lik<WithPrec<PrprConstant>>::value);"]
    for s in FIXED:
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
        lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
    lines.append("}")
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", which), "_ZN5vihds")
    assert len(usage) == len(FIXED) * 3, sorted(usage)
    for name, (vgpr, scratch) in sorted(usage.items()):
        print("%s: %d VGPRs, %d B scratch" % (name, vgpr, scratch))
        assert scratch == 0, name
