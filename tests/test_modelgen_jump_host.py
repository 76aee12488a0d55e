"""CPU tests of the state jump of vihds.modelgen (`jump(self, y, p, c)`) and of the host-side parts around it: definition
errors, the generated text (nothing changes without the hook; the members and the switch with it), the traced hook and its
reverse-mode adjoint against torch_jump and autograd in float64, the host declines an adaptive solver before any library call,
the float64 yardstick of the GPU comparisons checked against itself (with the hook returning y unchanged it is its parents'
definition to the last bit; its restated implicit-function adjoint against autograd through the Newton iteration), and
compilation for gfx950: scratch and VGPRs of the staged and unstaged forward, the adjoint and its dump form, and the kernel set
of a launcher."""
import hashlib
import importlib
import json
import os
import re
import shutil
from types import SimpleNamespace

import pytest
import torch

from vihds import hip, modelgen as G, ops
from vihds.utils import attrify

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_substep_models as SM
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SOLVER_ENUM = {"modeuler": "VIHDS_SOLVER_MODEULER", "modeulerwhile": "VIHDS_SOLVER_MODEULERWHILE",
               "euler": "VIHDS_SOLVER_EULER", "midpoint": "VIHDS_SOLVER_MIDPOINT", "rk4": "VIHDS_SOLVER_RK4",
               "beuler": "VIHDS_SOLVER_BEULER"}
# the modules whose PREBUILT lists existed before the hook
EARLIER_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models",
                   "modelgen_implicit_models", "modelgen_substep_models")
halve = lambda self, y, p, c: [0.5 * v for v in y]  # noqa: E731


# ---- definition -----------------------------------------------------------------------------------------------------------------
def test_the_hook_record():
    h = G.HOOKS[-1]
    assert h is G.HOOK["jump"] and [r.name for r in G.HOOKS] == ["observe", "precision", "log_likelihood", "jump"]
    assert h.groups == ("y",) and h.n_outputs == "species" and h.count(6) == 6 and h.count(3) == 3
    assert h.checks_arguments and h.none_resets and not h.hides_method and h.switch == "OWN_JUMP"
    assert h.targets == [("y", "yb"), ("p", "pb")]
    assert all(r.n_outputs == 4 and r.count(6) == 4 for r in G.HOOKS[:-1])


def test_definition_errors_are_raised_when_the_class_is_defined():
    ok = _define("jump_ok", jump=halve)
    assert ok._jump_def is halve and ok._trace.jmp is not None and len(ok._trace.jmp) == 6
    for bad in (lambda self, y, p, c: [y[0]] * 4, lambda self, y, p, c: [y[0]] * 7, lambda self, y, p, c: y[0]):
        with pytest.raises(G.ModelDefinitionError, match="jump must return a list of 6 entries"):
            _define("jump_wrong_length", jump=bad)
    three = dict(species=["OD", "A", "B"], observe=lambda self, y, p, c: [y[0], y[1], y[2], y[0]],
                 initial_state=lambda self, th, c: [th.init_x, 0.0, 0.0], rhs=lambda self, t, y, p, c: [p.r * y[0], 0.0, 0.0])
    with pytest.raises(G.ModelDefinitionError, match="jump must return a list of 3 entries"):
        _define("jump_four_of_three", jump=lambda self, y, p, c: [y[0]] * 4, **three)
    assert len(_define("jump_three", jump=lambda self, y, p, c: [y[0], y[1], y[2] + p.r], **three)._trace.jmp) == 3
    for bad in (lambda self, t, y, p, c: list(y), lambda self, y, p: list(y), lambda self, y, x, p, c: list(y)):
        with pytest.raises(G.ModelDefinitionError, match=r"jump must be a function jump\(self, y, p, c\).*no t"):
            _define("jump_wrong_arguments", jump=bad)
    with pytest.raises(G.ModelDefinitionError, match="jump must be a function"):
        _define("jump_not_callable", jump=[0.0] * 6)
    assert _define("jump_with_default", jump=lambda self, y, p, c, scale=0.5: [scale * v for v in y])._trace.jmp is not None
    with pytest.raises(G.ModelDefinitionError, match="network 'n' called from jump"):
        _define("jump_net", networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5,
                jump=lambda self, y, p, c: [self.net.n([y[0]])[0]] + list(y[1:]))
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("jump_if", jump=lambda self, y, p, c: [v * 0.5 if y[0] > 1.0 else v for v in y])
    with pytest.raises(G.ModelDefinitionError, match="unknown effective parameter 'nope'"):
        _define("jump_unknown", jump=lambda self, y, p, c: [p.nope * v for v in y])
    # NeuralPrecisions: WithPrec<> does not forward the members
    with pytest.raises(G.ModelDefinitionError, match=r"defines jump\(self, y, p, c\).*does not take NeuralPrecisions"):
        G.generate_source(ok, neural=True)
    for cls in JM.MODELS:
        with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
            G.generate_source(cls, True)
    # jump = None in a subclass removes the hook: the parent's text but for the names
    off = type("JumpOff", (ok,), {"model_key": "jump_off", "jump": None})
    assert off._jump_def is None and off._trace.jmp is None and "OWN_JUMP" not in G.generate_source(off)
    assert "yj[" not in G.generate_source(off) and "jump_vjp" not in G.generate_source(off)
    again = type("JumpOffOn", (off,), {"model_key": "jump_off_on", "jump": halve})
    assert again._trace.jmp is not None and "OWN_JUMP" in G.generate_source(again)
    # a treatment the hook reads becomes one more effective parameter
    treated = _define("jump_treated", n_conditions=2, jump=lambda self, y, p, c: [v * c[1] for v in y])
    assert treated._trace.c_in_rhs == [1] and treated._trace.NP == 2
    assert "yj[0] = " in G.generate_source(treated) and "p[1]" in _member(G.generate_source(treated), "jump")
    # a forcing is not read before the first time point, and the jump reads the sample of the point
    assert "p[%d]" % JM.PrprDiluted._trace.F0 in _member(G.generate_source(JM.PrprDiluted), "rhs")


def test_docstring_has_a_state_jumps_paragraph():
    for word in ("State jumps.", "def jump(self, y, p, c)", "LEFT limit", "not evaluated", "OWN_JUMP", "jump_vjp", "torch_jump",
                 "jump = None", "fixed-grid solvers only"):
        assert word in G.__doc__, word


# ---- generated text -------------------------------------------------------------------------------------------------------------
def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def _digests():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_jump_source_sha256.json")) as f:
        return json.load(f)


def test_classes_without_the_hook_generate_the_recorded_text():
    """Every (class, neural) of the PREBUILT lists that existed before the hook generates the text it generated: the digests of
    tests/golden/modelgen_jump_source_sha256.json "without" were taken from the commit before the hook (those of the six older
    modules are the entries of modelgen_source_sha256_all.json)."""
    recorded = _digests()["without"]
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256_all.json")) as f:
        older = json.load(f)
    seen = set()
    for m in EARLIER_MODULES:
        for cls, neural in importlib.import_module(m).PREBUILT:
            key = "%s.%s:%d" % (m, cls.__name__, int(neural))
            text = G.generate_source(cls, neural)
            assert hashlib.sha256(text.encode()).hexdigest() == recorded[key], key
            assert "jump" not in text.lower() and "OWN_JUMP" not in text, key
            if key in older:
                assert older[key] == recorded[key], key
            seen.add(key)
    assert seen == set(recorded) and len(seen) == 39


def test_generated_text_of_a_jump():
    recorded = _digests()["with"]
    assert sorted(recorded) == sorted(cls.__name__ for cls in JM.MODELS)
    for cls in JM.MODELS:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)  # deterministic
        assert hashlib.sha256(src.encode()).hexdigest() == recorded[cls.__name__], cls.__name__
        assert src.count("  static constexpr bool OWN_JUMP = true;  // the state jumps at the observation points: jump / jump_vjp\n") == 1
        assert "  __device__ static void jump(const float* y, const float* p, float* yj) {" in src
        assert "  __device__ static void jump_vjp(const float* y, const float* p, const float* yjb, float* yb, float* pb) {" in src
        # the hook is emitted last, after log_likelihood
        assert src.index("OWN_JUMP") > max(src.find(s) for s in ("loglik_vjp", "precision_vjp", "observe_vjp", "rhs_vjp"))
        tr, N = cls._trace, len(cls.species)
        fwd, body = _member(src, "jump"), _member(src, "jump_vjp")
        assert sorted(int(j) for j in re.findall(r"yj\[(\d+)\] = ", fwd)) == list(range(N))
        # the adjoint adds and never assigns; it writes yb of every species and pb of the named parameters only
        assert " = " not in re.sub(r"const (float|bool) v\d+ = ", "", body)
        assert sorted(set(int(j) for j in re.findall(r"yb\[(\d+)\] \+=", body))) == list(range(N))
        written = sorted(int(k) for k in re.findall(r"(?<![y])pb\[(\d+)\] \+=", body))
        assert written == [tr.p_names.index(JM.JUMP_ONLY[cls])], cls.__name__
        # the parameter the jump alone reads is read by no other member of the time loop
        slot = "p[%d]" % tr.p_names.index(JM.JUMP_ONLY[cls])
        assert slot in fwd and all(slot not in _member(src, m) for m in ("rhs", "rhs_vjp"))
        # the time-loop helpers, not the accurate forms of prepare
        assert " / " not in fwd + body and "expf(" not in fwd + body
        if cls.forcings:  # the sample of the point, never the interpolant
            assert "(t - p[" not in fwd + body and "p[%d]" % (tr.F0 + len(cls.forcings) - 1) in fwd
    # without the hook: the parent's text, but for the names and the parameter
    twin = type("PrprTurbidostat", (JM.PrprTurbidostat,), {"model_key": JM.PrprTurbidostat.model_key, "jump": None,
                                                           "__module__": JM.PrprTurbidostat.__module__})
    a, b = G.generate_source(twin).splitlines(), G.generate_source(JM.PrprTurbidostat).splitlines()
    assert a[2:-4] == b[2:len(a) - 4] and "OWN_JUMP" in b[len(a) - 4]
    turbid = _member(G.generate_source(JM.PrprTurbidostat), "jump")
    assert re.search(r"const bool v\d+ = %s < y\[0\];" % re.escape(G._lit(JM.THRESHOLD)), turbid) and turbid.count("fsel(") == 6


# ---- the torch restatement and the traced adjoint ---------------------------------------------------------------------------------
def _rand(shape, lo, hi, seed):
    return lo + (hi - lo) * torch.rand(shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("cls", [JM.PrprDiluted, JM.PrprTurbidostat, JM.PlateReaderDiluted, JM.HybridDosed],
                         ids=lambda c: c.__name__)
def test_traced_jump_and_its_adjoint_match_torch_jump_and_autograd(cls):
    """float64: evaluate of the traced nodes equals torch_jump, and the reverse-mode adjoint the generator emits as jump_vjp
    (then prepare_vjp) equals autograd through torch_jump, for the species and for every parameter.  Bound 1e-12."""
    tr = cls._trace
    g = tr.g
    B, S, T, N = 3, 2, 4, len(cls.species)
    NPU, C, K = len(tr.p_names), int(cls.n_conditions), len(cls.forcings)
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    treat = _rand((B, C), 0.1, 3.0, 91)
    series = _rand((B, K, T), 0.2, 1.5, 95)
    cond = FM.wide_cond(treat, series)
    y = _rand((B, S, N, T), 0.02, 0.3, 92)  # (optical densities on both sides of the turbidostat's threshold)
    W = torch.randn(B, S, N, T, dtype=F64, generator=torch.Generator().manual_seed(8))
    # the traced DAG
    c = torch.clamp(torch.exp(cond[:, :C]) - 1.0, 1e-12, 1e6)
    env0 = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
    env0.update({("c", q): c[:, q:q + 1].expand(B, S) for q in range(C)})
    pv = G.evaluate(tr.p_exprs, env0)
    env = {("p", k): pv[k].expand(B, S)[:, :, None] for k in range(NPU)}
    env.update({("p", NPU + q): env0[("c", q)][:, :, None] for q in range(C)})
    env.update({("y", j): y[:, :, j] for j in range(N)})
    env.update({("f", k): series[:, k, None, :] for k in range(K)})
    full = lambda v: v.expand(B, S, T) if isinstance(v, torch.Tensor) else torch.full((B, S, T), float(v), dtype=F64)  # noqa: E731
    traced = torch.stack([full(v) for v in G.evaluate(tr.jmp, env)], dim=2)
    adj = G.vjp(g, tr.jmp, [g.leaf("seed", j) for j in range(N)])
    e = dict(env)
    e.update({("seed", j): W[:, :, j] for j in range(N)})
    leaves = [g.leaf("y", j) for j in range(N)] + [g.leaf("p", k) for k in range(NPU)]
    out = [full(v) for v in G.evaluate([adj.get(l.id, g.const(0.0)) for l in leaves], e)]
    yb, pb = torch.stack(out[:N], dim=2), out[N:]
    adjp = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    e0 = dict(env0)
    e0.update({("seed", k): pb[k].sum(2) for k in range(NPU)})
    thb = G.evaluate([adjp.get(g.leaf("th", s).id, g.const(0.0)) for s in range(len(cls.parameter_names))], e0)
    # torch_jump and autograd
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    ref = cls.torch_jump(yt, tht, cond)
    assert ref.shape == (B, S, N, T)
    (ref * W).sum().backward()
    err = lambda a, b: float(((a - b).abs() / (1.0 + b.abs())).max())  # noqa: E731
    assert err(traced, ref.detach()) <= 1e-12 and err(yb, yt.grad) <= 1e-12
    for n, v in zip(cls.parameter_names, thb):
        want = tht[n].grad if tht[n].grad is not None else torch.zeros(B, S, dtype=F64)
        got = v.expand(B, S) if isinstance(v, torch.Tensor) else torch.full((B, S), float(v), dtype=F64)
        assert err(got, want) <= 1e-12, n
    assert float(tht[JM.JUMP_ONLY[cls]].grad.abs().max()) > 0.0
    if cls is JM.PrprTurbidostat:
        dense = y[:, :, 0] > JM.THRESHOLD
        assert bool(dense.any()) and bool((~dense).any())
        assert torch.equal(ref.detach()[:, :, 1][~dense], y[:, :, 1][~dense])
    with pytest.raises(G.ModelDefinitionError, match="defines no jump"):
        FM.PrprForced.torch_jump(y, th, cond)


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
    assert hip.GENERATED_JUMP == set() or all(isinstance(k, str) for k in hip.GENERATED_JUMP)
    fixed = "fixed-grid solvers: beuler, euler, midpoint, modeuler, modeulerwhile, rk4"
    for cls in (JM.PrprTurbidostat, JM.FastBindingDosed):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        monkeypatch.setattr(hip, "GENERATED_JUMP", hip.GENERATED_JUMP | {key})  # (what register_kernel records)
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"state jump.*'%s'.*%s" % (solver, fixed)):
                ops.OdeProblemSpec(key, solver, {}, 1, C=0)
    for cls in (JM.PrprTurbidostat, JM.PrprDiluted, JM.FastBindingDosed):
        model = cls(_config("dopri5", int(cls.n_conditions)))
        assert model.has_jump
        with pytest.raises(NotImplementedError, match=r"defines jump\(self, y, p, c\).*'dopri5'.*%s" % fixed):
            model.solve(_config("dopri5", 0), torch.tensor(JM.TIMES), None, torch.zeros(3, 0), None)
    # a model without the hook is not declined here
    assert not FM.PrprTreated(_config("rk4", 1)).has_jump
    monkeypatch.setitem(hip.MODELS, FM.PrprTreated.model_key, 1025)
    with pytest.raises(AssertionError, match="the library was asked for"):
        ops.OdeProblemSpec(FM.PrprTreated.model_key, "dopri5", {}, 1, C=1)


def test_evaluation_stores_x_predict_for_a_model_with_a_jump():
    from vihds import ode

    request = SimpleNamespace(general_tail=False)
    config = SimpleNamespace(params=attrify({"lazy_x_predict": True}))
    with torch.no_grad():
        assert ode.x_predict_on_demand(request, FM.PrprTreated(_config("rk4", 1)), config)
        assert not ode.x_predict_on_demand(request, JM.PrprTurbidostat(_config("rk4", 0)), config)


# ---- the definition checks itself -----------------------------------------------------------------------------------------------
def _identity_twin(cls):
    """`cls` with a hook that returns y unchanged, under a key of its own."""
    return type(cls.__name__ + "Identity", (cls,), {"model_key": cls.model_key + "_identity", "jump": lambda self, y, p, c: list(y)})


def test_an_identity_jump_is_the_parents_definition_to_the_last_bit():
    """With the hook returning y unchanged the yardstick of the GPU tests is the definition the earlier tests hold the kernels
    to: modelgen_forcing_models.forward for the explicit schemes (modeuler's fixed h0 included), modelgen_implicit_models
    .definition for beuler, modelgen_substep_models.beuler_definition with sub-steps -- values bit for bit, and so are the
    gradients of the restated implicit adjoint; those autograd forms through the explicit schemes agree to 1e-13 relative."""
    pb = FM.problem(FM.PrprForced, 2, 3)
    twin = _identity_twin(FM.PrprForced)
    for solver in FM.FIXED:
        a = JM.explicit_definition(twin, pb, solver, F64)
        xs, xp, _, logp = FM.forward(FM.PrprForced, pb["th"], pb["cond"], pb["times"], solver, pb["obs"])
        assert torch.equal(a["traj"], xs) and torch.equal(a["xpred"], xp) and torch.equal(a["logp"], logp), solver
        b = SM.explicit_definition(FM.PrprForced, pb, solver, F64, m=1)
        for n, v in b["g_theta"].items():  # (autograd adds a leaf's parts in the order of its graph: the last bits may differ)
            assert float((a["g_theta"][n] - v).abs().max()) <= 1e-13 * float(v.abs().max()), (solver, n)
    pb = IM.problem(IM.FastBinding, 2, 3)
    a, b = JM.beuler_definition(_identity_twin(IM.FastBinding), pb, F64), IM.definition(IM.FastBinding, pb, F64)
    assert torch.equal(a["traj"], b["traj"]) and torch.equal(a["logp"], b["logp"]) and a["last_increment"] == b["last_increment"]
    for n in b["g_theta"]:
        assert torch.equal(a["g_theta"][n], b["g_theta"][n]), n
    pb = SM.problem(SM.FastBindingSub4, 2, 3)
    a, b = JM.beuler_definition(_identity_twin(SM.FastBindingSub4), pb, F64), SM.beuler_definition(SM.FastBindingSub4, pb, F64)
    assert torch.equal(a["traj"], b["traj"]) and torch.equal(a["logp"], b["logp"])
    for n in b["g_theta"]:
        assert torch.equal(a["g_theta"][n], b["g_theta"][n]), n
    # and `jump=False` of a model with the hook is its hookless parent's definition
    pb = JM.problem(JM.PrprDiluted, 2, 3)
    a = JM.explicit_definition(JM.PrprDiluted, pb, "rk4", F64, jump=False)
    th = {n: v for n, v in pb["th"].items() if n != "bolus"}
    xs = FM.forward(FM.PrprForced, th, FM.wide_cond(torch.zeros(2, 0), pb["series"][:, :1]), pb["times"], "rk4")[0]
    assert torch.equal(a["traj"], xs)


def test_restated_adjoint_with_jumps_equals_autograd_through_the_newton_iteration():
    """float64, FastBindingDosedSub2: the yardstick's gradient (implicit-function theorem at every sub-step's iterate, the
    jump's pullback between the intervals) against autograd through 30 unrolled Newton iterations per sub-step and through
    torch_jump: 1e-8 relative per parameter, the bound of the tests of the same kind without jumps."""
    cls = JM.FastBindingDosedSub2
    pb = JM.problem(cls, 2, 3)
    pb = dict(pb, times=pb["times"][:4], obs=pb["obs"][..., :4],
              cond=FM.wide_cond(torch.zeros(2, 0), pb["series"][..., :4]))
    ref = JM.beuler_definition(cls, pb, F64)
    assert ref["last_increment"] <= 1e-9
    th = {n: v.detach().clone().requires_grad_(True) for n, v in pb["th"].items()}
    times, cond, T, m = pb["times"], pb["cond"], 4, 2
    rhs, x0 = IM.torch_rhs(cls, th, cond, times)
    fine = SM.refined(times, m)
    y, lefts = x0, [x0]
    for k in range(T - 1):
        u = JM.jump_at(cls, y, th, cond, k, T)
        for j in range(m):
            q = k * m + j
            u, _ = IM.newton_step(rhs, fine[q + 1], fine[q + 1] - fine[q], u, 30,
                                  lambda f, t, z: IM.autograd_jacobian(f, t, z, create_graph=True))
        y = u
        lefts.append(y)
    _, _, logp = SM.hooks(cls, torch.stack(lefts, dim=3), th, cond, pb["obs"])
    (logp * pb["G"]["logp"]).sum().backward()
    for n, v in th.items():
        e = float((ref["g_theta"][n] - v.grad).abs().max() / v.grad.abs().max())
        print("g_theta[%s]: restated adjoint against autograd through Newton and the jump %.2e" % (n, e))
        assert e <= 1e-8, n
    assert float(th["bolus"].grad.abs().max()) > 0.0


def test_the_inputs_of_the_gpu_tests():
    """What the GPU tests assert first, on the float64 yardstick alone, at both of their shapes: the schedules (two or three
    events per row, point 0 among them, rows differ), Newton converged, the turbidostat's comparisons at least MARGIN wide with a
    diluted and an undiluted sample in every data row, and the hook matters: without it the trajectory differs by more than
    100 x 1e-5 and the gradient of the parameter only the jump reads by more than 100 x 1e-4."""
    T = len(JM.TIMES)
    ev = [JM.events_of(b, T) for b in range(3)]
    assert all(0 in e and len(e) in (2, 3) for e in ev) and len({tuple(e) for e in ev}) == 3 and T - 1 in ev[2]
    keep, dose = JM.schedule(3, T)
    assert all(sorted(torch.nonzero(keep[b] != 1.0)[:, 0].tolist()) == ev[b] == sorted(torch.nonzero(dose[b])[:, 0].tolist())
               for b in range(3))
    for cls in JM.MODELS:
        assert cls._jump_def is not None and JM.JUMP_ONLY[cls] in cls.parameter_names
        for B, S in ((3, 5), (3, 100)):
            pb = JM.problem(cls, B, S)
            assert JM.problem(cls, B, S) is pb
            for solver in JM.solvers_of(cls):
                r = JM.definition(cls, pb, solver, F64)
                r0 = JM.definition(cls, pb, solver, F64, jump=False)
                assert all(bool(torch.isfinite(r[k]).all()) for k in ("traj", "xpred", "logp"))
                if solver == "beuler":
                    assert r["last_increment"] <= 1e-9
                if r["margins"].by_label:
                    assert cls is JM.PrprTurbidostat and r["margins"].smallest >= JM.MARGIN
                    trig = JM.triggered(cls, r["traj"])
                    assert bool(trig.any(1).all()) and bool((~trig).any(1).all())
                gap = float((r0["traj"] - r["traj"]).abs().amax(dim=(0, 1, 3)).div(r["traj"].abs().amax(dim=(0, 1, 3))).max())
                name = JM.JUMP_ONLY[cls]
                print("%s %s %dx%d: without the hook the trajectory differs by %.2e; |g_theta[%s]| up to %.2e"
                      % (cls.__name__, solver, B, S, gap, name, float(r["g_theta"][name].abs().max())))
                assert gap > 100 * 1e-5 and float(r0["g_theta"][name].abs().max()) == 0.0
                assert float(r["g_theta"][name].abs().max(dim=1).values.min()) > 0.0


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", JM.MODELS, ids=lambda c: c.__name__)
def test_jump_kernels_compile_without_scratch(tmp_path, cls):
    """The staged forward, the unstaged forward, the adjoint and, for the model with a network, the dump form of the adjoint
    compile for gfx950 and spill nothing, for every fixed-grid solver (and beuler where the model is implicit).  VGPRs are
    printed (DESIGN.md quotes them).  The trait is false for the hand-written models and for WithPrec<>."""
    header = tmp_path / "jump.hpp"
    header.write_text(G.generate_source(cls))
    solvers = list(FM.FIXED) + (["beuler"] if cls.implicit else [])
    dump = bool(cls.networks)
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(has_jump<VIHDS_GEN_CORE>::value && !has_jump<WithPrec<VIHDS_GEN_CORE>>::value);",
             "static_assert(!has_jump<PrprConstant>::value && !has_jump<DrConstant<1>>::value && !has_jump<BlackboxIcml>::value);"]
    for s in solvers:
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s]]
        if dump:
            lines += ["template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % SOLVER_ENUM[s]]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "jump"), "_ZN5vihds")
    assert len(usage) == (4 if dump else 3) * len(solvers), sorted(usage)
    for s in solvers:
        tag = "Li%dELb" % hip.SOLVERS[s]
        fwd = sorted(v[0] for n, v in usage.items() if "ode_fwd_kernel" in n and tag in n)
        bwd = [v[0] for n, v in sorted(usage.items()) if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %s VGPRs (staged / unstaged in either order), adjoint %s VGPRs%s"
              % (cls.__name__, s, " / ".join(map(str, fwd)), " / ".join(map(str, bwd)), " (plain / dump)" if dump else ""))
        assert len(fwd) == 2 and len(bwd) == (2 if dump else 1)
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_launcher_with_a_jump_holds_the_fixed_grid_kernels_only(tmp_path):
    """launch_ode with every solver in one unit.  PrprDiluted holds exactly the fifteen kernel names of PrprForced and
    FastBindingDosed eighteen (the struct's name aside); PrprTurbidostat, which has neither forcings nor sub-steps, holds the
    fifteen too -- no kernel of an adaptive pair, no one-pass summaries."""
    names = {}
    for cls in (FM.PrprForced, JM.PrprDiluted, IM.PrprForcedImplicit, JM.FastBindingDosed, JM.PrprTurbidostat):
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
    assert len(names[FM.PrprForced]) == 15 and names[JM.PrprDiluted] == names[FM.PrprForced]
    assert len(names[IM.PrprForcedImplicit]) == 18 and names[JM.FastBindingDosed] == names[IM.PrprForcedImplicit]
    assert names[JM.PrprTurbidostat] == names[FM.PrprForced]
