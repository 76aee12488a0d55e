"""CPU tests of the start map and the lead-in phase of vihds.modelgen (`start(self, y, p, c)`, `lead_in`, `lead_in_steps`) and of
the host-side parts around them: definition errors, the generated text (nothing changes without them; the members, the switch
and the two constants with them), torch_start and the traced adjoint against autograd in float64, lead_in_times, the host
declines an adaptive solver before any library call, the float64 yardstick of the GPU comparisons checked against itself, and
compilation for gfx950: scratch and VGPRs of the staged and unstaged forward and of the adjoint, and the kernel set of a
launcher."""
import hashlib
import importlib
import json
import os
import re
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G, ops
from vihds.utils import attrify

import modelgen_forcing_models as FM
import modelgen_implicit_models as IM
import modelgen_jump_models as JM
import modelgen_leadin_models as LM
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SOLVER_ENUM = {"modeuler": "VIHDS_SOLVER_MODEULER", "modeulerwhile": "VIHDS_SOLVER_MODEULERWHILE",
               "euler": "VIHDS_SOLVER_EULER", "midpoint": "VIHDS_SOLVER_MIDPOINT", "rk4": "VIHDS_SOLVER_RK4",
               "beuler": "VIHDS_SOLVER_BEULER"}
# the modules whose PREBUILT lists existed before the two attributes
EARLIER_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models",
                   "modelgen_implicit_models", "modelgen_substep_models")
double = lambda self, y, p, c: [2.0 * v for v in y]  # noqa: E731


# ---- definition -----------------------------------------------------------------------------------------------------------------
def test_the_hook_record():
    h = G.START_HOOK
    assert h is G.HOOK["start"] and G.ALL_HOOKS == (h,) + G.HOOKS and h not in G.HOOKS
    assert h.groups == ("y",) and h.n_outputs == "species" and h.count(6) == 6 and h.count(3) == 3
    assert h.checks_arguments and h.none_resets and not h.hides_method and h.switch == "OWN_START"
    assert h.targets == [("y", "yb"), ("p", "pb")]
    assert G.MAX_LEAD_IN_STEPS == 8 and G.GeneratedOdeModel.lead_in == 0.0 and G.GeneratedOdeModel.lead_in_steps == 1


def test_start_definition_errors_are_raised_when_the_class_is_defined():
    ok = _define("start_ok", start=double)
    assert ok._start_def is double and ok._trace.start is not None and len(ok._trace.start) == 6
    for bad in (lambda self, y, p, c: [y[0]] * 4, lambda self, y, p, c: [y[0]] * 7, lambda self, y, p, c: y[0]):
        with pytest.raises(G.ModelDefinitionError, match="start must return a list of 6 entries"):
            _define("start_wrong_length", start=bad)
    for bad in (lambda self, t, y, p, c: list(y), lambda self, y, p: list(y), lambda self, y, x, p, c: list(y)):
        with pytest.raises(G.ModelDefinitionError, match=r"start must be a function start\(self, y, p, c\).*no t"):
            _define("start_wrong_arguments", start=bad)
    with pytest.raises(G.ModelDefinitionError, match="start must be a function"):
        _define("start_not_callable", start=[0.0] * 6)
    with pytest.raises(G.ModelDefinitionError, match="network 'n' called from start: networks are evaluated in rhs only"):
        _define("start_net", networks={"n": G.Network(1, 2, 1)},
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5,
                start=lambda self, y, p, c: [self.net.n([y[0]])[0]] + list(y[1:]))
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("start_if", start=lambda self, y, p, c: [v * 0.5 if y[0] > 1.0 else v for v in y])
    with pytest.raises(G.ModelDefinitionError, match="unknown effective parameter 'nope'"):
        _define("start_unknown", start=lambda self, y, p, c: [p.nope * v for v in y])
    # start combines with networks in rhs
    hybrid = _define("start_hybrid", networks={"n": G.Network(1, 2, 1)},
                     rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5, start=double)
    assert "OWN_START" in G.generate_source(hybrid) and "NET_FIELDS" in G.generate_source(hybrid)
    # NeuralPrecisions: WithPrec<> does not forward the members
    with pytest.raises(G.ModelDefinitionError, match=r"defines start\(self, y, p, c\).*does not take NeuralPrecisions"):
        G.generate_source(ok, neural=True)
    # start = None in a subclass removes the hook
    off = type("StartOff", (ok,), {"model_key": "start_off", "start": None})
    assert off._start_def is None and off._trace.start is None and "OWN_START" not in G.generate_source(off)
    assert "ys[" not in G.generate_source(off) and "start_vjp" not in G.generate_source(off)
    again = type("StartOffOn", (off,), {"model_key": "start_off_on", "start": double})
    assert again._trace.start is not None and "OWN_START" in G.generate_source(again)
    # a treatment the hook reads becomes one more effective parameter; a parameter may be read by start alone
    treated = _define("start_treated", n_conditions=2, start=lambda self, y, p, c: [v * c[1] for v in y])
    assert treated._trace.c_in_rhs == [1] and treated._trace.NP == 2
    assert "p[1]" in _member(G.generate_source(treated), "start")
    src = G.generate_source(LM.PrprSteady)
    slot = "p[%d]" % LM.PrprSteady._trace.p_names.index("pre")
    assert slot in _member(src, "start") and all(slot not in _member(src, m) for m in ("rhs", "rhs_vjp"))


def test_the_initial_state_stays_affine_and_its_message_points_to_start():
    """initial_state keeps its refusal and its wording (tests/test_modelgen_host.py and test_modelgen_piecewise_host.py match
    it); the message ends with a pointer to start, and the same map is accepted there."""
    steady = lambda self, th, c: [th.init_x, th.r / (1.0 + th.r), 0.0, 0.0, 0.0, 0.0]  # noqa: E731
    with pytest.raises(G.ModelDefinitionError, match=r"affine.*where, minimum, maximum.*goes into start\(self, y, p, c\)"):
        _define("init_ratio", initial_state=steady)
    ok = _define("start_ratio", start=lambda self, y, p, c: [y[0], p.r / (1.0 + p.r)] + list(y[2:]))
    assert "fdiv(" in _member(G.generate_source(ok), "start") or "frcp(" in _member(G.generate_source(ok), "start")


def test_lead_in_definition_errors_are_raised_when_the_class_is_defined():
    ok = _define("lead_ok", lead_in=1.5, lead_in_steps=3)
    src = G.generate_source(ok)
    assert "  static constexpr int LEAD_STEPS = 3;" in src and "  static constexpr float LEAD_TIME = 1.5f;\n" in src
    assert _define("lead_int", lead_in=2).lead_in == 2 and "LEAD_TIME = 2.0f;" in G.generate_source(_define("lead_int2", lead_in=2))
    for bad in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), "1.0", None, True, [1.0], 1e-60, 1e60):
        with pytest.raises(G.ModelDefinitionError, match=r"lead_in = .*a number above 0"):
            _define("lead_bad", lead_in=bad)
    for bad in (0, 9, -1, 2.0, True, "2", None):
        with pytest.raises(G.ModelDefinitionError, match=r"lead_in_steps = .*1 \.\. 8 \(MAX_LEAD_IN_STEPS\)"):
            _define("lead_steps_bad", lead_in=1.0, lead_in_steps=bad)
    for zero in ({}, {"lead_in": 0.0}, {"lead_in": 0}):
        with pytest.raises(G.ModelDefinitionError, match="lead_in_steps = 2 without lead_in"):
            _define("lead_steps_alone", lead_in_steps=2, **zero)
    with pytest.raises(G.ModelDefinitionError, match=r"lead_in = 1.0 and networks.*\(T-1\) x stages"):
        _define("lead_net", networks={"n": G.Network(1, 2, 1)}, lead_in=1.0,
                rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match=r"lead_in = 1.5.*does not take\s+NeuralPrecisions"):
        G.generate_source(ok, neural=True)
    # the LDS rows: (lead_in_steps - 1) * species at most MAX_SUBSTEP_ROWS = 56
    nine = dict(species=["OD", "RFP", "YFP", "CFP", "F530", "F480", "U", "V", "W"],
                initial_state=lambda self, th, c: [th.init_x] + [0.0] * 8, rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 8)
    assert G.MAX_STATES >= 9
    with pytest.raises(G.ModelDefinitionError, match=r"lead_in_steps = 8 and 9 species.*at most 56 \(MAX_SUBSTEP_ROWS\)"):
        _define("lead_rows", lead_in=1.0, lead_in_steps=8, **nine)
    assert _define("lead_rows_ok", lead_in=1.0, lead_in_steps=7, **nine).lead_in_steps == 7  # 54 rows
    assert (LM.SevenLead.lead_in_steps - 1) * len(LM.SevenLead.species) == 49
    # every new model: no NeuralPrecisions
    for cls in LM.MODELS:
        with pytest.raises(G.ModelDefinitionError, match="NeuralPrecisions"):
            G.generate_source(cls, True)
    # a subclass returns to no lead-in with the default
    off = type("LeadOff", (ok,), {"model_key": "lead_off", "lead_in": 0.0, "lead_in_steps": 1})
    assert "LEAD_" not in G.generate_source(off)


def test_docstring_has_a_paragraph_on_where_the_trajectory_starts():
    for word in ("Where the trajectory starts.", "def start(self, y, p, c)", "lead_in = 6.0", "lead_in_steps = 4", "OWN_START",
                 "start_vjp", "LEAD_STEPS", "LEAD_TIME", "lead_in_times", "torch_start", "start = None", "Fixed-grid solvers only"):
        assert word in G.__doc__, word


# ---- generated text -------------------------------------------------------------------------------------------------------------
def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def test_classes_without_the_attributes_generate_the_recorded_text():
    """Every (class, neural) of the PREBUILT lists that existed before generates the text it generated: the digests of
    tests/golden/modelgen_jump_source_sha256.json, "without" and "with", were recorded before the two attributes existed."""
    recorded = _golden("modelgen_jump_source_sha256.json")
    seen = set()
    for m in EARLIER_MODULES:
        for cls, neural in importlib.import_module(m).PREBUILT:
            key = "%s.%s:%d" % (m, cls.__name__, int(neural))
            text = G.generate_source(cls, neural)
            assert hashlib.sha256(text.encode()).hexdigest() == recorded["without"][key], key
            assert "OWN_START" not in text and "LEAD_" not in text and " start(" not in text and "start_vjp" not in text, key
            seen.add(key)
    assert seen == set(recorded["without"]) and len(seen) == 39
    for cls in JM.MODELS:
        text = G.generate_source(cls)
        assert hashlib.sha256(text.encode()).hexdigest() == recorded["with"][cls.__name__], cls.__name__
        assert "OWN_START" not in text and "LEAD_" not in text


def test_generated_text_of_the_new_models():
    recorded = _golden("modelgen_leadin_source_sha256.json")
    assert sorted(recorded) == sorted(cls.__name__ for cls in LM.MODELS)
    for cls in LM.MODELS:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)  # deterministic
        assert hashlib.sha256(src.encode()).hexdigest() == recorded[cls.__name__], cls.__name__
        has_start, n = cls._start_def is not None, LM.lead_steps(cls)
        assert src.count("  static constexpr bool OWN_START = true;") == int(has_start)
        assert src.count("  static constexpr int LEAD_STEPS = %d;" % n) == int(n > 0) and src.count("LEAD_STEPS") == int(n > 0)
        assert src.count("  static constexpr float LEAD_TIME = %s;\n" % G._lit(cls.lead_in)) == int(n > 0)
        if not has_start:
            assert " start(" not in src and "start_vjp" not in src
            continue
        assert "  __device__ static void start(const float* y, const float* p, float* ys) {" in src
        assert "  __device__ static void start_vjp(const float* y, const float* p, const float* ysb, float* yb, float* pb) {" in src
        N = len(cls.species)
        fwd, body = _member(src, "start"), _member(src, "start_vjp")
        assert sorted(int(j) for j in re.findall(r"ys\[(\d+)\] = ", fwd)) == list(range(N))
        # the adjoint adds and never assigns; it writes pb of the named parameters only
        assert " = " not in re.sub(r"const (float|bool) v\d+ = ", "", body)
        assert all(int(k) < len(cls._trace.p_names) for k in re.findall(r"(?<![y])pb\[(\d+)\] \+=", body))
        if cls.forcings:  # the first sample, never the interpolant
            assert "(t - p[" not in fwd + body and "p[%d]" % cls._trace.F0 in fwd
    steady = _member(G.generate_source(LM.PrprSteady), "start")
    assert re.search(r"const bool v\d+ = %s < p\[\d+\];" % re.escape(G._lit(LM.INDUCED_ABOVE)), steady) and steady.count("fsel(") == 3
    # without the attributes: the parent's text but for the names
    twin = type("PrprSteadyLead", (LM.PrprSteadyLead,), {"model_key": LM.PrprSteadyLead.model_key, "start": None, "lead_in": 0.0,
                                                          "lead_in_steps": 1, "__module__": LM.PrprSteadyLead.__module__})
    a, b = G.generate_source(twin).splitlines(), G.generate_source(LM.PrprSteadyLead).splitlines()
    assert [l for l in b if "LEAD_" not in l][:len(a) - 4] == a[:-4]


# ---- lead_in_times --------------------------------------------------------------------------------------------------------------
def test_lead_in_times_are_the_kernels_grid():
    """n + 1 float32 times that end on t_0 exactly and start at t_0 - L; strictly increasing; the inner ones a single rounding of
    j * hl + tl (checked against exact rational arithmetic)."""
    from fractions import Fraction

    for cls in LM.MODELS + [FM.PrprForced]:
        for t0 in (0.0, 0.3, 1.7, -2.25, 1e3):
            t = G.lead_in_times(cls, t0)
            n = LM.lead_steps(cls)
            assert t.dtype == np.float32 and t.shape == (n + 1,) and t[-1] == np.float32(t0)
            if not n:
                continue
            tl = np.float32(np.float32(t0) - np.float32(cls.lead_in))
            hl = np.float32(np.float32(np.float32(t0) - tl) * np.float32(np.float32(1.0) / np.float32(n)))
            assert t[0] == tl and bool(np.all(np.diff(t.astype(np.float64)) > 0))
            assert LM.lead_step_size(cls, t0) == float(hl)
            for j in range(n):
                exact = Fraction(j) * Fraction(float(hl)) + Fraction(float(tl))
                lo, hi = np.nextafter(t[j], np.float32(-np.inf)), np.nextafter(t[j], np.float32(np.inf))
                err = abs(Fraction(float(t[j])) - exact)
                assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (cls.__name__, t0, j)
    assert G.lead_in_times(LM.PrprSteadyLead, 0.0).tolist() == [-1.0, -0.75, -0.5, -0.25, 0.0]


# ---- the torch restatement and the traced adjoint ---------------------------------------------------------------------------------
def _rand(shape, lo, hi, seed):
    return lo + (hi - lo) * torch.rand(shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("cls", [LM.PrprSteady, LM.PrprEverything], ids=lambda c: c.__name__)
def test_traced_start_and_its_adjoint_match_torch_start_and_autograd(cls):
    """float64: evaluate of the traced nodes equals torch_start, and the reverse-mode adjoint the generator emits as start_vjp
    (then prepare_vjp) equals autograd through torch_start, for the state and for every parameter.  Bound 1e-12.  torch_problem's
    x0 includes the hook."""
    tr = cls._trace
    g = tr.g
    B, S, T, N = 3, 2, 4, len(cls.species)
    NPU, C, K = len(tr.p_names), int(cls.n_conditions), len(cls.forcings or ())
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    treat = torch.tensor([[0.3], [1.0], [1.7]], dtype=F64)[:, :C]
    series = _rand((B, K, T), 0.2, 1.5, 95)
    cond = FM.wide_cond(treat, series)
    y = _rand((B, S, N), 0.02, 0.3, 92)
    W = torch.randn(B, S, N, dtype=F64, generator=torch.Generator().manual_seed(8))
    c = torch.clamp(torch.exp(cond[:, :C]) - 1.0, 1e-12, 1e6)
    env0 = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
    env0.update({("c", q): c[:, q:q + 1].expand(B, S) for q in range(C)})
    pv = G.evaluate(tr.p_exprs, env0)
    env = {("p", k): pv[k].expand(B, S) for k in range(NPU)}
    env.update({("p", NPU + q): env0[("c", q)] for q in range(C)})
    env.update({("y", j): y[:, :, j] for j in range(N)})
    env.update({("f", k): series[:, k, :1].expand(B, S) for k in range(K)})  # (the first sample)
    full = lambda v: v.expand(B, S) if isinstance(v, torch.Tensor) else torch.full((B, S), float(v), dtype=F64)  # noqa: E731
    traced = torch.stack([full(v) for v in G.evaluate(tr.start, env)], dim=2)
    adj = G.vjp(g, tr.start, [g.leaf("seed", j) for j in range(N)])
    e = dict(env)
    e.update({("seed", j): W[:, :, j] for j in range(N)})
    leaves = [g.leaf("y", j) for j in range(N)] + [g.leaf("p", k) for k in range(NPU)]
    out = [full(v) for v in G.evaluate([adj.get(l.id, g.const(0.0)) for l in leaves], e)]
    yb, pb = torch.stack(out[:N], dim=2), out[N:]
    adjp = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    e0 = dict(env0)
    e0.update({("seed", k): pb[k] for k in range(NPU)})
    thb = G.evaluate([adjp.get(g.leaf("th", s).id, g.const(0.0)) for s in range(len(cls.parameter_names))], e0)
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    ref = cls.torch_start(yt, tht, cond)
    assert ref.shape == (B, S, N)
    (ref * W).sum().backward()
    err = lambda a, b: float(((a - b).abs() / (1.0 + b.abs())).max())  # noqa: E731
    assert err(traced, ref.detach()) <= 1e-12 and err(yb, yt.grad) <= 1e-12
    for n, v in zip(cls.parameter_names, thb):
        want = tht[n].grad if tht[n].grad is not None else torch.zeros(B, S, dtype=F64)
        assert err(full(v), want) <= 1e-12, n
    if cls in LM.START_ONLY:
        gp = tht[LM.START_ONLY[cls]].grad
        assert float(gp[0].abs().max()) == 0.0 and float(gp[1:].abs().min()) > 0.0  # (row 0 is not induced)
        assert torch.equal(ref.detach()[0], y[0]) and not torch.equal(ref.detach()[1], y[1])
    # torch_problem starts from it (start=False: the initial state alone)
    kw = {"times": torch.arange(T, dtype=F64)} if K else {}
    x0 = cls.torch_problem(th, cond, None, **kw)[1]
    xi = cls.torch_problem(th, cond, None, start=False, **kw)[1]
    assert torch.equal(x0, cls.torch_start(xi, th, cond)) and not torch.equal(x0, xi)
    with pytest.raises(G.ModelDefinitionError, match="defines no start"):
        FM.PrprForced.torch_start(y, th, cond)


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
    fixed = "fixed-grid solvers: beuler, euler, midpoint, modeuler, modeulerwhile, rk4"
    for cls, word in ((LM.PrprSteady, r"start map \(start\)"), (LM.PrprLeadOne, r"lead-in phase \(lead_in\)"),
                      (LM.PrprSteadyLead, r"start map \(start\) and a lead-in phase \(lead_in\)")):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        if cls._start_def is not None:  # (what register_kernel records)
            monkeypatch.setattr(hip, "GENERATED_START", hip.GENERATED_START | {key})
        if cls.lead_in > 0:
            monkeypatch.setattr(hip, "GENERATED_LEAD_IN", dict(hip.GENERATED_LEAD_IN, **{key: (cls.lead_in, cls.lead_in_steps)}))
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"%s.*'%s'.*%s" % (word, solver, fixed)):
                ops.OdeProblemSpec(key, solver, {}, 1, C=0)
    for cls, word in ((LM.PrprSteady, r"defines start\(self, y, p, c\)"), (LM.PrprLeadOne, "has lead_in = 0.5"),
                      (LM.FastBindingLead, "has lead_in = 0.5"), (LM.PrprSteadyLead, r"defines start\(self, y, p, c\)")):
        model = cls(_config("dopri5", int(cls.n_conditions)))
        assert model.has_start == (cls._start_def is not None) and model.has_lead_in == (cls.lead_in > 0)
        with pytest.raises(NotImplementedError, match=r"%s.*'dopri5'.*%s" % (word, fixed)):
            model.solve(_config("dopri5", 0), torch.tensor(LM.TIMES), None, torch.zeros(3, 0), None)
    # a model without the attributes is not declined here
    plain = FM.PrprTreated(_config("rk4", 1))
    assert not plain.has_start and not plain.has_lead_in
    monkeypatch.setitem(hip.MODELS, FM.PrprTreated.model_key, 1025)
    with pytest.raises(AssertionError, match="the library was asked for"):
        ops.OdeProblemSpec(FM.PrprTreated.model_key, "dopri5", {}, 1, C=1)


def test_evaluation_stores_x_predict_for_these_models():
    from vihds import ode

    request = SimpleNamespace(general_tail=False)
    config = SimpleNamespace(params=attrify({"lazy_x_predict": True}))
    with torch.no_grad():
        assert ode.x_predict_on_demand(request, FM.PrprTreated(_config("rk4", 1)), config)
        assert not ode.x_predict_on_demand(request, LM.PrprSteady(_config("rk4", 1)), config)
        assert not ode.x_predict_on_demand(request, LM.PrprLeadOne(_config("rk4", 0)), config)


# ---- the definition checks itself -----------------------------------------------------------------------------------------------
def test_without_the_attributes_the_definition_is_the_parents_to_the_last_bit():
    """`start=False, lead=False` of the yardstick is the definition the earlier tests hold the kernels to: modelgen_jump_models'
    for PrprEverything's parent with two sub-steps, modelgen_implicit_models.definition for FastBinding."""
    pb = LM.problem(LM.PrprEverything, 2, 3)
    twin = type("PrprDilutedSub2", (JM.PrprDiluted,), {"model_key": "gen_prpr_constant_diluted_sub2_twin", "substeps": 2})
    for solver in ("modeuler", "rk4"):
        a = LM.explicit_definition(LM.PrprEverything, pb, solver, F64, start=False, lead=False)
        b = JM.explicit_definition(twin, pb, solver, F64)
        assert torch.equal(a["traj"], b["traj"]) and torch.equal(a["logp"], b["logp"]), solver
        for n, v in b["g_theta"].items():
            assert float((a["g_theta"][n] - v).abs().max()) <= 1e-13 * max(float(v.abs().max()), 1e-300), (solver, n)
    pb = IM.problem(IM.FastBinding, 2, 3)
    a, b = LM.beuler_definition(LM.FastBindingLead, pb, F64, lead=False), IM.definition(IM.FastBinding, pb, F64)
    assert torch.equal(a["traj"], b["traj"]) and torch.equal(a["logp"], b["logp"]) and a["last_increment"] == b["last_increment"]
    for n in b["g_theta"]:
        assert torch.equal(a["g_theta"][n], b["g_theta"][n]), n


def test_the_definition_is_the_plain_scheme_on_the_extended_grid():
    """PrprForcedLead under rk4: the oracle's own simulate on lead_in_times + times with the series padded with u_0, the leading
    n points dropped, is the yardstick bit for bit (the lead-in has no scheme of its own)."""
    from oracle import vihds_oracle as O

    cls = LM.PrprForcedLead
    pb = LM.problem(cls, 2, 3)
    times_x, cond_x = LM.extended(cls, pb["cond"], pb["times"])
    n = LM.lead_steps(cls)
    assert times_x.shape[0] == pb["T"] + n and torch.equal(times_x[n:], pb["times"]) and float(times_x[0]) == -0.75
    assert cond_x.shape[1] == pb["cond"].shape[1] + n and torch.equal(cond_x[:, :n + 1], pb["cond"][:, :1].expand(2, n + 1))
    rhs, x0 = cls.torch_problem(pb["th"], cond_x, None, times=times_x)
    for solver in ("midpoint", "rk4"):
        xs = O.simulate(rhs, x0, times_x, solver)[..., n:]
        assert torch.equal(LM.explicit_states(cls, pb["th"], pb["cond"], pb["times"], solver), xs), solver


def test_restated_adjoint_with_a_lead_in_equals_autograd_through_the_newton_iteration():
    """float64: the yardstick's gradient (implicit-function theorem at every step's iterate, lead-in steps included) against
    autograd through 30 unrolled Newton iterations per step: 1e-8 relative per parameter."""
    for cls in (LM.FastBindingLead, LM.SevenLead):
        pb = LM.problem(cls, 2, 3)
        pb = dict(pb, times=pb["times"][:4], obs=pb["obs"][..., :4])
        ref = LM.beuler_definition(cls, pb, F64)
        assert ref["last_increment"] <= 1e-9
        auto = LM.beuler_by_autograd(cls, pb, 30)
        for n, v in auto.items():
            if float(v.abs().max()) == 0.0:
                assert float(ref["g_theta"][n].abs().max()) == 0.0, n
                continue
            e = float((ref["g_theta"][n] - v).abs().max() / v.abs().max())
            print("%s g_theta[%s]: restated adjoint against autograd through Newton %.2e" % (cls.__name__, n, e))
            assert e <= 1e-8, (cls.__name__, n)


def test_the_inputs_of_the_gpu_tests():
    """What the GPU tests assert first, on the float64 yardstick alone, at their shapes: everything finite, Newton converged
    (lead-in steps included), the hook and the phase matter (without either the trajectory differs by more than 100 x 1e-5), the
    gradient of the start-only parameter is not zero, and both sides of the induction threshold occur."""
    cases = [(cls, (3, 5), None) for cls in LM.MODELS] + [(cls, (3, 100), None) for cls in (LM.PrprSteadyLead, LM.FastBindingLead)]
    cases += [(cls, (3, 5), [0.0, 0.3]) for cls in (LM.PrprSteadyLead, LM.PrprEverything, LM.FastBindingLead)]
    for cls, (B, S), times in cases:
        pb = LM.problem(cls, B, S, times=times)
        assert LM.problem(cls, B, S, times=times) is pb
        if cls.n_conditions:
            assert bool((pb["treatments"] < LM.INDUCED_ABOVE).any()) and bool((pb["treatments"] > LM.INDUCED_ABOVE).any())
        for solver in LM.solvers_of(cls):
            r = LM.definition(cls, pb, solver, F64)
            assert all(bool(torch.isfinite(r[k]).all()) for k in ("traj", "xpred", "logp"))
            assert all(bool(torch.isfinite(v).all()) for v in r["g_theta"].values())
            if solver == "beuler":
                assert r["last_increment"] <= 1e-9
            scale = r["traj"].abs().amax(dim=(0, 1, 3))
            for has, kw in ((cls._start_def is not None, {"start": False}), (cls.lead_in > 0, {"lead": False})):
                if has:
                    r0 = LM.definition(cls, pb, solver, F64, **kw)
                    gap = float((r0["traj"] - r["traj"]).abs().amax(dim=(0, 1, 3)).div(scale).max())
                    print("%s %s %dx%d T=%d: without %s the trajectory differs by %.2e"
                          % (cls.__name__, solver, B, S, pb["T"], list(kw)[0], gap))
                    assert gap > 100 * 1e-5
                    if cls in LM.START_ONLY and "start" in kw:
                        assert float(r0["g_theta"][LM.START_ONLY[cls]].abs().max()) == 0.0
            if cls in LM.START_ONLY:
                assert float(r["g_theta"][LM.START_ONLY[cls]].abs().max()) > 0.0


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", LM.MODELS, ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged forward, the unstaged forward and the adjoint compile for gfx950 and spill nothing, for every solver the model
    takes.  VGPRs are printed (DESIGN.md quotes them).  The traits are off for the hand-written models and for WithPrec<>."""
    header = tmp_path / "leadin.hpp"
    header.write_text(G.generate_source(cls))
    solvers = LM.solvers_of(cls)
    n, has = LM.lead_steps(cls), "" if cls._start_def is not None else "!"
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(%shas_start<VIHDS_GEN_CORE>::value && lead_in<VIHDS_GEN_CORE>::value == %d);" % (has, n),
             "static_assert(!has_start<WithPrec<VIHDS_GEN_CORE>>::value && lead_in<WithPrec<VIHDS_GEN_CORE>>::value == 0);",
             "static_assert(!has_start<PrprConstant>::value && !has_start<DrConstant<1>>::value && !has_start<BlackboxIcml>::value);",
             "static_assert(lead_in<PrprConstant>::value == 0 && lead_in<DrConstant<1>>::value == 0 && lead_in<BlackboxIcml>::value == 0);",
             "static_assert(substate_rows<VIHDS_GEN_CORE>() == %d);"
             % (max(int(cls.substeps) - 1, n - 1, 0) * len(cls.species))]
    for s in solvers:
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s],
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % SOLVER_ENUM[s]]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "leadin"), "_ZN5vihds")
    assert len(usage) == 3 * len(solvers), sorted(usage)
    for s in solvers:
        tag = "Li%dELb" % hip.SOLVERS[s]
        fwd = sorted(v[0] for k, v in usage.items() if "ode_fwd_kernel" in k and tag in k)
        bwd = [v[0] for k, v in sorted(usage.items()) if "ode_bwd_kernel" in k and tag in k]
        print("%s %s: forward %s VGPRs (staged / unstaged in either order), adjoint %s VGPRs"
              % (cls.__name__, s, " / ".join(map(str, fwd)), " / ".join(map(str, bwd))))
        assert len(fwd) == 2 and len(bwd) == 1
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_launcher_holds_the_fixed_grid_kernels_only(tmp_path):
    """launch_ode with every solver in one unit.  PrprSteady (a start map, nothing else) and PrprLeadOne (a lead-in, nothing
    else) hold exactly the fifteen kernel names of PrprForced, FastBindingLead the eighteen of an implicit model (the struct's
    name aside) -- no kernel of an adaptive pair, no one-pass summaries."""
    names = {}
    for cls in (FM.PrprForced, LM.PrprSteady, LM.PrprLeadOne, IM.PrprForcedImplicit, LM.FastBindingLead):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        struct = "GenModel_" + G._ident(cls.model_key)
        assert all(struct in k for k in usage)
        names[cls] = sorted(k.replace("%d%s" % (len(struct), struct), "M") for k in usage)
        assert all("ode_fwd_kernel" in k or "ode_bwd_kernel" in k for k in names[cls]), names[cls]
    assert len(names[FM.PrprForced]) == 15 and names[LM.PrprSteady] == names[FM.PrprForced]
    assert names[LM.PrprLeadOne] == names[FM.PrprForced]
    assert len(names[IM.PrprForcedImplicit]) == 18 and names[LM.FastBindingLead] == names[IM.PrprForcedImplicit]
