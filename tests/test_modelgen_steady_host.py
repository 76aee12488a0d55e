"""CPU tests of pre-equilibration in vihds.modelgen (`steady_species`, `steady_rate`, `steady_steps`, `steady_first_step`,
`steady_growth`) and of the host-side parts of csrc/vihds_steady.hpp: the refusals, the generated text (and the unchanged text of
every class without steady species), the generated Jacobian and its pattern against autograd, torch_steady's implicit-function
gradient against gradcheck of a run of 40 pure Newton iterations, the solved twin against its closed form, the toggle's two
basins against a long float64 integration of the pre-culture system, the convergence precondition at the inputs of the GPU
tests, the host's refusal of an adaptive solver, the iteration and the adjoint solve in a stand-alone host program under the
address and undefined-behaviour sanitizers, and compilation for gfx950 (scratch and VGPRs of the staged and unstaged forward and
of the adjoint; the kernel set of a launcher)."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G, ops

import modelgen_forcing_models as FM
import modelgen_leadin_models as LM
import modelgen_steady_models as SS
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_leadin_host import _config, _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SHAPES = [(3, 5), (3, 100)]
ALL = SS.MODELS + [SS.ChainEightFree]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _steady(name, **body):
    """A six-species model whose RFP and YFP relax to r / (1 + OD) and r in the pre-culture."""
    attrs = dict(steady_species=["RFP", "YFP"],
                 steady_rate=lambda self, y, p, c: [p.r - (1.0 + y[0]) * y[1], p.r * y[1] - y[2]])
    attrs.update(body)
    return _define(name, **attrs)


def test_refusals():
    ok = _steady("steady_ok")
    src = G.generate_source(ok)
    assert "N_STEADY = 2" in src and G.MAX_STEADY == 8 and G.MAX_STEADY_STEPS == 16
    E = G.ModelDefinitionError
    with pytest.raises(E, match="steady_species: 'LuxR' is no species of the model"):
        _steady("steady_unknown", steady_species=["RFP", "LuxR"])
    with pytest.raises(E, match="steady_species has duplicates"):
        _steady("steady_twice", steady_species=["RFP", "RFP"])
    nine = dict(species=["OD"] + ["S%d" % k for k in range(9)], initial_state=lambda self, th, c: [th.init_x] + [0.0] * 9,
                rhs=lambda self, t, y, p, c: [p.r * y[0]] + [0.0] * 9, observe_kind="direct")
    eight = _steady("steady_eight", steady_species=["S%d" % k for k in range(8)],
                    steady_rate=lambda self, y, p, c: [p.r - y[1 + k] for k in range(8)], **nine)
    assert "N_STEADY = 8" in G.generate_source(eight)
    with pytest.raises(E, match="9 steady species.*at most 8"):
        _steady("steady_nine", steady_species=["S%d" % k for k in range(9)],
                steady_rate=lambda self, y, p, c: [p.r - y[1 + k] for k in range(9)], **nine)
    with pytest.raises(E, match="steady_rate must return a list of 2 entries"):
        _steady("steady_short", steady_rate=lambda self, y, p, c: [p.r - y[1]])
    with pytest.raises(E, match="steady_rate must return a list of 2 entries"):
        _steady("steady_scalar", steady_rate=lambda self, y, p, c: p.r - y[1])
    with pytest.raises(E, match=r"steady_rate must be a function steady_rate\(self, y, p, c\).*no t"):
        _steady("steady_t", steady_rate=lambda self, t, y, p, c: [p.r - y[1], p.r - y[2]])
    with pytest.raises(E, match="without steady_rate"):
        _steady("steady_none", steady_rate=None)
    net = dict(networks={"n": G.Network(1, 2, 1)}, rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5)
    with pytest.raises(E, match="network 'n' called from steady_rate"):
        _steady("steady_net", steady_rate=lambda self, y, p, c: [self.net.n([y[1]])[0] - y[1], p.r - y[2]], **net)
    with pytest.raises(E, match="network 'n' called from steady_rate"):  # (through the model's own rhs)
        _steady("steady_net_rhs", steady_rate=lambda self, y, p, c: [self.rhs(0.0, y, p, c)[0] - y[1], p.r - y[2]], **net)
    alg = dict(algebraic=["z0"], algebraic_start=lambda self, y, p, c: [p.r],
               constraint=lambda self, y, z, p, c: [z[0] * (1.0 + y[0]) - p.r],
               rhs=lambda self, t, y, p, c: [p.r * y[0] - self.algebraic.z0] + [0.0] * 5)
    with pytest.raises(E, match="algebraic variables and steady_species"):
        _steady("steady_alg", **alg)
    lag = dict(delays={"late": ("RFP", "tau")}, prepare=lambda self, th, c: {"r": th.r, "tau": th.r},
               rhs=lambda self, t, y, p, c: [p.r * y[0], self.delayed.late - y[1]] + [0.0] * 4)
    with pytest.raises(E, match="delayed read 'late' read in steady_rate"):
        _steady("steady_delay", steady_rate=lambda self, y, p, c: [self.delayed.late - y[1], p.r - y[2]], **lag)
    with pytest.raises(E, match="delayed read 'late' read in steady_rate"):  # (through the model's own rhs)
        _steady("steady_delay_rhs", steady_rate=lambda self, y, p, c: [self.rhs(0.0, y, p, c)[1], p.r - y[2]], **lag)
    for bad in (0, 17, 4.0, True, "4"):
        with pytest.raises(E, match=r"steady_steps = .*an int in 1 \.\. 16"):
            _steady("steady_steps_bad", steady_steps=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True, 1e-60):
        with pytest.raises(E, match="steady_first_step = .*finite number above 0"):
            _steady("steady_first_bad", steady_first_step=bad)
    for bad in (0.5, float("inf"), float("nan"), "2", False):
        with pytest.raises(E, match="steady_growth = .*finite factor of at least 1"):
            _steady("steady_growth_bad", steady_growth=bad)
    assert "STEADY_GROWTH = 1.0f" in G.generate_source(_steady("steady_growth_one", steady_growth=1))
    for attr, value in (("steady_steps", 4), ("steady_first_step", 0.5), ("steady_growth", 2.0),
                        ("steady_rate", lambda self, y, p, c: [p.r - y[1]])):
        with pytest.raises(E, match="sets %s without steady_species" % attr):
            _define("steady_lonely_" + attr, **{attr: value})
    with pytest.raises(E, match="sets steady_steps without steady_species"):  # (an emptied list does not excuse it)
        _define("steady_lonely_emptied", steady_species=[], steady_steps=4)
    # a structurally singular Jacobian, in the wording of the constraint's check
    with pytest.raises(E, match="no residual depends on the steady species 'YFP'.*zero column"):
        _steady("steady_column", steady_rate=lambda self, y, p, c: [p.r - y[1], p.r - 2.0 * y[1]])
    with pytest.raises(E, match="residual 1 depends on no steady species.*zero row"):
        _steady("steady_row", steady_rate=lambda self, y, p, c: [p.r - y[1] - y[2], p.r - y[0]])
    with pytest.raises(E, match="residual 0 does not depend on the steady species 'RFP'.*pivot 0.*order the residuals"):
        _steady("steady_pivot", steady_rate=lambda self, y, p, c: [p.r - y[2], p.r - y[1]])
    with pytest.raises(E, match="does not take NeuralPrecisions"):
        G.generate_source(ok, True)
    # None or [] in a subclass removes it: the text is the parent's without the attribute
    plain = _define("steady_plain")
    for k, empty in enumerate((None, [])):
        gone = type("steady_gone_%d" % k, (ok,), {"model_key": "steady_plain", "steady_species": empty})
        assert gone._trace.steady == [] and "STEADY" not in G.generate_source(gone)
        assert G.generate_source(gone).split("\n", 1)[1] == G.generate_source(plain).split("\n", 1)[1]


def test_where_steady_rate_may_read():
    """It reads a forcing's first sample and a treatment (one more effective parameter), and a parameter of its own."""
    cls = SS.CascadeCombined
    tr, src = cls._trace, G.generate_source(cls)
    body = _member(src, "steady_rate")
    assert "p[%d]" % tr.F0 in body and "p[%d]" % (tr.F0 + 3) not in body  # (the value entry of `light`, never a slope)
    assert tr.c_in_rhs == [0] and "p[%d]" % len(tr.p_names) in body
    tg = SS.ToggleSteady._trace
    leak = tg.p_names.index("leak")
    assert "p[%d]" % leak in _member(G.generate_source(SS.ToggleSteady), "steady_rate")
    assert "p[%d]" % leak not in _member(G.generate_source(SS.ToggleSteady), "rhs")


# ---- generated text -------------------------------------------------------------------------------------------------------------
def test_generated_text():
    for cls in SS.MODELS:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)
        M = len(cls.steady_species)
        pattern = G.steady_pattern(cls)
        mask = sum(1 << (i * M + j) for i in range(M) for j in range(M) if pattern[i][j])
        for line in ("static constexpr int N_STEADY = %d;" % M, "static constexpr int STEADY_STEPS = %d;" % cls.steady_steps,
                     "static constexpr float STEADY_DELTA0 = %s;" % G._lit(cls.steady_first_step),
                     "static constexpr float STEADY_GROWTH = %s;" % G._lit(cls.steady_growth),
                     "static constexpr unsigned long long STEADY_NZ = 0x%xull;" % mask,
                     "static constexpr int steady_species(int e)"):
            assert line in src, line
        body = _member(src, "steady_jac")
        for i in range(M):
            for j in range(M):
                assert body.count("A[%d] = " % (i * M + j)) == (1 if pattern[i][j] else 0)
        idx = [cls.species.index(s) for s in cls.steady_species]
        vjp_body = _member(src, "steady_rate_vjp")
        assert not any("yb[%d] +=" % j in vjp_body for j in idx)  # (the steady species' adjoint is cleared, never added to)
        adj = _member(src, "steady_vjp")
        assert all("lam[%d] = 0.f;" % j in adj for j in idx) and adj.rstrip().endswith("steady_rate_vjp(y, p, mu, lam, pb);")
        assert "steady_iterate<N_STEADY, STEADY_STEPS, STEADY_NZ>(" in src and "steady_adjoint<N_STEADY, STEADY_NZ>(" in src
    assert "OWN_START" in G.generate_source(SS.CascadeCombined) and "LEAD_STEPS = 2" in G.generate_source(SS.CascadeCombined)
    assert "STEADY" not in G.generate_source(SS.ChainEightFree) and "steady" not in G.generate_source(SS.ChainEightFree).split("\n", 2)[2]
    assert "STEADY" not in G.generate_source(LM.PrprSteady)


def test_structural_patterns():
    count = lambda cls: sum(map(sum, G.steady_pattern(cls)))  # noqa: E731
    assert [count(c) for c in SS.MODELS] == [3, 4, 7, 22, 9]
    assert G.steady_pattern(SS.ChainEight) == [[abs(i - j) <= 1 for j in range(8)] for i in range(8)]
    assert G.steady_pattern(SS.CascadeCombined) == [[i == j or i == j + 1 for j in range(4)] for i in range(4)]


def test_classes_without_steady_species_generate_the_recorded_text():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256_all.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 29
    for key, digest in recorded.items():
        path, neural = key.split(":")
        module, cname = path.rsplit(".", 1)
        text = G.generate_source(getattr(importlib.import_module(module), cname), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key
        assert "STEADY" not in text and "steady(" not in text


def test_new_classes_generate_the_recorded_text():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_steady_source_sha256.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted("%s:0" % c.__name__ for c in ALL)
    for cls in ALL:
        text = G.generate_source(cls)
        assert hashlib.sha256(text.encode()).hexdigest() == recorded["%s:0" % cls.__name__], cls.__name__


def test_documents_have_the_paragraph():
    for word in ("Pre-equilibration.", "steady_species", "steady_steps", "steady_first_step", "steady_growth",
                 "def steady_rate(self, y, p, c)", "torch_steady", "torch_steady_jacobian", "MAX_STEADY", "MAX_STEADY_STEPS",
                 "implicit-function", "exactly 0", "return_residual"):
        assert word in G.__doc__, word
    with open(os.path.join(CSRC, "vihds_steady.hpp")) as f:
        header = f.read()
    for word in ("pseudo-transient", "J(y*)^T mu = lam_E", "WITHOUT pivoting", "__builtin_fmaf"):
        assert word in header, word
    for doc, word in (("INTEGRATION.md", "steady_species"), ("DESIGN.md", "steady_species"), ("README.md", "modelgen_steady")):
        with open(os.path.join(ROOT, doc)) as f:
            assert word in f.read(), doc
    assert hip.GENERATED_STEADY == {} or all(isinstance(v, int) for v in hip.GENERATED_STEADY.values())


# ---- the generated Jacobian ---------------------------------------------------------------------------------------------------------
def _state_and_inputs(cls, B=3, S=5):
    pb = SS.problem(cls, B, S)
    guess, forcing = SS.guess_and_forcing(cls, pb["th"], pb["cond"], pb["T"])
    return pb, guess, forcing


def _residual(cls, y, th, cond, forcing):
    """steady_rate of the class at the states y [B,S,N] with torch ops: the class's own function, called as the tests call rhs."""
    inst = cls.__new__(cls)
    ref = y[:, :, 0]
    cs = G._treatments_torch(cls, cond, ref, ref.shape[1])
    if forcing is not None:
        object.__setattr__(inst, "forcing", G._Forcings(cls, lambda k, _name: forcing[k]))
    thn = G._Named([(n, th[n]) for n in cls.parameter_names], "parameter")
    p = G._Named(inst.prepare(thn, G._Conditions(cs)).items(), "effective parameter")
    out = inst.steady_rate(list(torch.unbind(y, dim=2)), p, G._Conditions(cs))
    return torch.stack([v.expand_as(ref) for v in out], dim=2)


@pytest.mark.parametrize("cls", SS.MODELS, ids=lambda c: c.__name__)
def test_generated_jacobian_equals_autograd(cls):
    """torch_steady_jacobian (the DAG nodes steady_jac is emitted from) against autograd of the class's steady_rate in float64,
    1e-13 relative; the structural pattern is exactly the set of entries autograd finds non-zero at generic states."""
    pb, guess, forcing = _state_and_inputs(cls)
    y = (guess * (1.0 + 0.1 * torch.rand(guess.shape, generator=torch.Generator().manual_seed(3), dtype=F64))).requires_grad_(True)
    J = cls.torch_steady_jacobian(y.detach(), pb["th"], pb["cond"], forcing=forcing)
    F = _residual(cls, y, pb["th"], pb["cond"], forcing)
    idx = [cls.species.index(s) for s in cls.steady_species]
    M = len(idx)
    rows = [torch.autograd.grad(F[:, :, i].sum(), y, retain_graph=True)[0][:, :, idx] for i in range(M)]
    auto = torch.stack(rows, dim=2)
    assert J.shape == auto.shape == (3, 5, M, M)
    assert float((J - auto).abs().max() / auto.abs().max()) <= 1e-13
    pattern = torch.tensor(G.steady_pattern(cls))
    assert torch.equal((auto.abs().amax((0, 1)) > 0), pattern)


# ---- the solve on the host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SS.ToggleSteady, SS.CascadeCombined], ids=lambda c: c.__name__)
def test_implicit_function_gradient_passes_gradcheck_on_forty_newton_iterations(cls):
    """float64: torch_steady run as 40 pure Newton iterations (first step 1e12, growth 1: I - delta J is -delta J to rounding)
    from a guess near the root.  gradcheck differentiates that run numerically -- the guess of a steady species moves nothing,
    the other species and theta move the root -- and the custom backward, the implicit-function step, must agree."""
    pb, guess, forcing = _state_and_inputs(cls, 2, 2)
    with torch.no_grad():
        root = cls.torch_steady(guess, pb["th"], pb["cond"], forcing=forcing)
    names = list(cls.parameter_names)
    idx = [cls.species.index(s) for s in cls.steady_species]
    bump = torch.zeros_like(root)
    bump[:, :, idx] = 0.02 * torch.randn(root[:, :, idx].shape, generator=torch.Generator().manual_seed(5), dtype=F64)
    start = (root * (1.0 + bump)).requires_grad_(True)  # (the steady species' guesses moved off the root by 2 %)
    thetas = [pb["th"][n].clone().requires_grad_(True) for n in names]

    def run(y, *ths):
        th = dict(pb["th"], **dict(zip(names, ths)))
        return cls.torch_steady(y, th, pb["cond"], forcing=forcing, steps=40, first_step=1e12, growth=1.0)

    out, inc, res = cls.torch_steady(start.detach(), pb["th"], pb["cond"], forcing=forcing, return_residual=True, steps=40,
                                     first_step=1e12, growth=1.0)
    print("%s: 40 Newton iterations end with an increment of %.2e, |F| %.2e" % (cls.__name__, inc, res))
    assert inc <= 1e-12 and float((out - root).abs().max() / root.abs().max()) <= 1e-10
    assert torch.autograd.gradcheck(run, [start] + thetas, eps=1e-6, atol=1e-6, rtol=1e-5)
    # the guess of a steady species receives exactly 0, the species held fixed what the root's dependence on them gives
    g = torch.autograd.grad(run(start, *thetas).sum(), start)[0]
    assert float(g[:, :, idx].abs().max()) == 0.0 and float(g[:, :, 0].abs().min()) > 0.0


def test_torch_steady_keeps_the_iterate_and_returns_the_residual():
    """Too few steps are not converged: the value is still the iterate's, the last increment and |F| say so; torch_problem's x0
    includes the solve (start=False: the initial state alone); a class without steady species has no torch_steady."""
    cls = SS.ToggleSteady
    pb, guess, forcing = _state_and_inputs(cls)
    y3, inc3, res3 = cls.torch_steady(guess, pb["th"], pb["cond"], return_residual=True, steps=3)
    y12, inc12, res12 = cls.torch_steady(guess, pb["th"], pb["cond"], return_residual=True)
    assert inc3 > 1e-3 and res3 > 1e-3 and inc12 <= 1e-9 and res12 <= 1e-12
    assert torch.equal(y12[:, :, [0, 3]], guess[:, :, [0, 3]]) and not torch.equal(y12[:, :, 1:3], guess[:, :, 1:3])
    x0 = cls.torch_problem(pb["th"], pb["cond"], None)[1]
    xi = cls.torch_problem(pb["th"], pb["cond"], None, start=False)[1]
    assert torch.equal(x0, y12) and torch.equal(xi, guess)
    with pytest.raises(G.ModelDefinitionError, match="declares no steady_species"):
        SS.ChainEightFree.torch_steady(guess, pb["th"], pb["cond"])
    with pytest.raises(ValueError, match=r"needs forcing=\[light, keep, dose\]"):
        pc, gc, _ = _state_and_inputs(SS.CascadeCombined)
        SS.CascadeCombined.torch_steady(gc, pc["th"], pc["cond"])


def test_the_solved_twin_reaches_the_closed_form():
    """PrprSteadySolved against PrprSteady's start map in float64 on the same inputs, 3 x 100: 1e-12 relative at 9 steps -- the
    class's steady_steps -- and not at 8 (both printed)."""
    cls = SS.PrprSteadySolved
    assert cls.steady_steps == 9 and cls.parameter_names == LM.PrprSteady.parameter_names
    pb = SS.problem(cls, 3, 100)
    closed = LM.PrprSteady.torch_problem(pb["th"], pb["cond"], None)[1]
    guess, _ = SS.guess_and_forcing(cls, pb["th"], pb["cond"], pb["T"])
    errs = {}
    for n in (8, 9):
        y = cls.torch_steady(guess, pb["th"], pb["cond"], steps=n)
        errs[n] = float(((y - closed).abs() / closed.abs().clamp_min(1e-30)).max())
        print("PrprSteadySolved: %d steps are within %.2e of the closed form" % (n, errs[n]))
    assert errs[9] <= 1e-12 < errs[8]
    assert torch.equal(cls.torch_problem(pb["th"], pb["cond"], None)[1], cls.torch_steady(guess, pb["th"], pb["cond"]))
    assert not torch.equal(closed[0], guess[0]) or not torch.equal(closed[1], guess[1])


def test_the_twins_float64_definitions_agree():
    """float64, rk4, 3 x 5: the definition of PrprSteadySolved (the solve, the implicit-function gradient) against plain
    autograd of PrprSteady's (the closed form): trajectory, log-likelihood and every theta gradient to 1e-9 relative."""
    pb = SS.problem(SS.PrprSteadySolved, 3, 5)
    a, b = SS.definition(SS.PrprSteadySolved, pb, "rk4", F64), LM.definition(LM.PrprSteady, pb, "rk4", F64)
    worst = 0.0
    for k in ("traj", "xpred", "logp"):
        worst = max(worst, float((a[k] - b[k]).abs().max() / b[k].abs().max()))
    for n, g in b["g_theta"].items():
        e = float((a["g_theta"][n] - g).abs().max() / g.abs().max())
        print("g_theta[%s]: the solve's implicit-function gradient against autograd of the closed form %.2e" % (n, e))
        worst = max(worst, e)
    assert worst <= 1e-9


def _integrate(f, y, t_end, n):
    h = t_end / n
    for _ in range(n):
        k1 = f(y)
        k2 = f(y + 0.5 * h * k1)
        k3 = f(y + 0.5 * h * k2)
        k4 = f(y + h * k3)
        y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return y


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_toggle_lands_in_the_basin_of_its_guess(shape):
    """float64: rows 0 and 2 (guesses with U high) end at the state with U high, row 1 at the one with V high, and each agrees
    with the pre-culture system d y_E / dt = steady_rate integrated by rk4 from the same guess over 80 time units -- refined
    (800, 1600, 3200 steps) until two refinements agree to 1e-8 -- to 1e-8 relative.  The convergence precondition holds for
    every row."""
    cls = SS.ToggleSteady
    pb = SS.problem(cls, *shape)
    inc, res, y = SS.converged(cls, pb)
    print("ToggleSteady %dx%d: last increment %.2e, |F| %.2e" % (shape + (inc, res)))
    assert inc <= 1e-9
    guess, _ = SS.guess_and_forcing(cls, pb["th"], pb["cond"], pb["T"])

    def flow(z):
        full = torch.cat([guess[:, :, :1], z, guess[:, :, 3:]], dim=2)
        return _residual(cls, full, pb["th"], pb["cond"], None)

    prev, steps, agreed = None, 800, None
    with torch.no_grad():
        while steps <= 3200:
            cur = _integrate(flow, guess[:, :, 1:3], 80.0, steps)
            if prev is not None:
                agreed = float(((cur - prev).abs() / cur.abs()).max())
                print("rk4 with %d steps against %d: %.2e" % (steps, steps // 2, agreed))
                if agreed <= 1e-8:
                    break
            prev, steps = cur, steps * 2
    assert agreed is not None and agreed <= 1e-8
    high_u = y[:, :, 1] > y[:, :, 2]
    assert bool(high_u[0].all()) and bool((~high_u[1]).all()) and (shape[0] < 3 or bool(high_u[2].all()))
    assert float((y[0, :, 1] / y[0, :, 2]).min()) > 5.0 and float((y[1, :, 2] / y[1, :, 1]).min()) > 5.0  # (two different states)
    gap = float(((y[:, :, 1:3] - cur).abs() / cur.abs()).max())
    print("ToggleSteady %dx%d: the solve against the long integration %.2e" % (shape + (gap,)))
    assert gap <= 1e-8


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cls", SS.MODELS, ids=lambda c: c.__name__)
def test_the_iteration_has_converged_at_the_test_inputs(cls, shape):
    """The kernel's adjoint is that of the CONVERGED solution: on the float64 run alone, the last of the steady_steps increments
    is at most 1e-9 of |y_E| in every row, at both shapes of the GPU tests, and no pivot of the unpivoted eliminations is
    small: the float32 run of the same iteration ends within 1e-5 of it."""
    pb = SS.problem(cls, *shape)
    inc, res, y = SS.converged(cls, pb)
    inc32, _res32, y32 = SS.converged(cls, pb, torch.float32)
    e32 = float(((y32.double() - y).abs() / y.abs().clamp_min(1e-3)).max())
    print("%s %dx%d: last increment %.2e, |F| %.2e; float32 run: last increment %.2e, %.2e from the float64 state"
          % ((cls.__name__,) + shape + (inc, res, inc32, e32)))
    assert bool(torch.isfinite(y).all()) and inc <= 1e-9 and e32 <= 1e-5


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def test_host_declines_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hip, "lib", no_library)
    monkeypatch.setattr(G, "register_kernel", no_library)
    fixed = "fixed-grid solvers: beuler, euler, midpoint, modeuler, modeulerwhile, rk4"
    for cls in (SS.ToggleSteady, SS.ChainEight):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        monkeypatch.setattr(hip, "GENERATED_STEADY", dict(hip.GENERATED_STEADY, **{key: len(cls.steady_species)}))
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"steady species \(steady_species\).*'%s'.*%s" % (solver, fixed)):
                ops.OdeProblemSpec(key, solver, {}, 1, C=0)
        model = cls(_config("dopri5", int(cls.n_conditions)))
        assert model.n_steady_species == len(cls.steady_species)
        with pytest.raises(NotImplementedError, match=r"declares steady_species.*'dopri5'.*%s" % fixed):
            model.solve(_config("dopri5", 0), torch.tensor(SS.TIMES), None, torch.zeros(3, 0), None)
    plain = SS.ChainEightFree(_config("rk4", 0))
    assert plain.n_steady_species == 0
    monkeypatch.setitem(hip.MODELS, SS.ChainEightFree.model_key, 1025)
    with pytest.raises(AssertionError, match="the library was asked for"):
        ops.OdeProblemSpec(SS.ChainEightFree.model_key, "dopri5", {}, 1, C=0)


def test_evaluation_stores_x_predict_for_these_models():
    from types import SimpleNamespace

    from vihds import ode
    from vihds.utils import attrify

    request = SimpleNamespace(general_tail=False)
    config = SimpleNamespace(params=attrify({"lazy_x_predict": True}))
    with torch.no_grad():
        assert ode.x_predict_on_demand(request, FM.PrprTreated(_config("rk4", 1)), config)
        assert not ode.x_predict_on_demand(request, SS.ToggleSteady(_config("rk4", 1)), config)


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", SS.MODELS, ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every solver the class is tested with compile for gfx950 and
    spill nothing (VGPRs printed; recorded in DESIGN.md).  ChainEight is the worst case the cap MAX_STEADY stands for."""
    header = tmp_path / "steady.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(kMaxSteady == %d && kMaxSteadySteps == %d);" % (G.MAX_STEADY, G.MAX_STEADY_STEPS),
             "static_assert(has_steady<VIHDS_GEN_CORE>::value == %d);" % len(cls.steady_species)]
    solvers = SS.solvers_of(cls)
    for solver in solvers:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "steady"), "_ZN5vihds")
    assert len(usage) == 3 * len(solvers), sorted(usage)
    for solver in solvers:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d" % (cls.__name__, solver, min(fwd), max(fwd), bwd[0]))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


def _dense_eight(n_species):
    """Eight steady species coupled through their total (a dense 8 x 8 J, all 64 bits of the pattern), sixteen iterations, beside
    n_species - 9 further species in a chain that reads them: the register worst case the caps MAX_STEADY and MAX_STEADY_STEPS
    stand for."""
    def rhs(self, t, y, p, c):
        total = sum(y[2:9], y[1])
        out = [p.r * y[0]]
        for j in range(8):
            out.append(p.r * 0.2 * (j + 1) - (1.0 + 0.1 * j) * y[1 + j] - p.r * y[1 + j] * total / (1.0 + total))
        for j in range(9, n_species):
            out.append(p.r * y[j - 1] - y[j] * y[(j * 7) % n_species] / (1.0 + y[j]))
        return out

    return type("steady_dense_%d" % n_species, (G.GeneratedOdeModel,), dict(
        model_key="steady_dense_%d" % n_species, species=["OD"] + ["S%d" % k for k in range(1, n_species)], parameters=["r", "init_x"],
        n_conditions=0, observe_kind="direct", prepare=lambda self, th, c: {"r": th.r},
        initial_state=lambda self, th, c: [th.init_x] * n_species, rhs=rhs, steady_species=["S%d" % k for k in range(1, 9)],
        steady_steps=16, steady_rate=lambda self, y, p, c: self.rhs(0.0, y, p, c)[1:9]))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_dense_pattern_beside_a_large_state_compiles_without_scratch(tmp_path):
    """The caps at once: 8 steady species with a dense J (64 non-zeros, full fill-in), 16 iterations, beside 24 species in all.
    The staged and the unstaged forward and the adjoint of midpoint and rk4 compile for gfx950 without scratch (VGPRs printed;
    DESIGN.md records them, and what a state of 32 species does with and without the solve)."""
    cls = _dense_eight(24)
    assert G.steady_pattern(cls) == [[True] * 8] * 8 and "STEADY_NZ = 0xffffffffffffffffull" in G.generate_source(cls)
    header = tmp_path / "dense.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {"]
    for name in ("VIHDS_SOLVER_MIDPOINT", "VIHDS_SOLVER_RK4"):
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "dense"), "_ZN5vihds")
    assert len(usage) == 6, sorted(usage)
    for name, (vgpr, scratch) in sorted(usage.items()):
        print("%s: %d VGPRs, %d B scratch" % (name, vgpr, scratch))
        assert scratch == 0, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_a_launcher_holds_the_fixed_grid_kernels_only(tmp_path):
    """launch_ode with every solver in one unit: ToggleSteady (steady species, nothing else) holds exactly the fifteen kernel
    names of PrprForced, BindingSteadyStiff the eighteen of an implicit model (the struct's name aside) -- no kernel of an
    adaptive pair, no one-pass summaries."""
    import modelgen_implicit_models as IM

    names = {}
    for cls in (FM.PrprForced, SS.ToggleSteady, IM.PrprForcedImplicit, SS.BindingSteadyStiff):
        header = tmp_path / ("%s.hpp" % cls.__name__)
        header.write_text(G.generate_source(cls))
        text = ('#include "vihds_ode_kernels.hpp"\n#include "vihds_gen_model.hpp"\n#include "%s"\nnamespace vihds {\n'
                "int a_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
                "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
        usage = _resource_usage(_compile_usage(tmp_path, text, "launch_" + cls.__name__), "_ZN5vihds")
        struct = "GenModel_" + G._ident(cls.model_key)
        assert all(struct in k for k in usage)
        names[cls] = sorted(k.replace("%d%s" % (len(struct), struct), "M") for k in usage)
        assert all("ode_fwd_kernel" in k or "ode_bwd_kernel" in k for k in names[cls]), names[cls]
        assert all(scratch == 0 for _v, scratch in usage.values())
    assert len(names[FM.PrprForced]) == 15 and names[SS.ToggleSteady] == names[FM.PrprForced]
    assert len(names[IM.PrprForcedImplicit]) == 18 and names[SS.BindingSteadyStiff] == names[IM.PrprForcedImplicit]


# ---- the iteration and the adjoint solve, in a stand-alone host program under sanitizers ----------------------------------------
PROGRAM = r"""
// reads cases "m pattern mode, A[m m], b[m], z[m]".  mode 0: prints z after 12 iterations (delta 0.1, growth 4) on
// F(z) = b - A z - 0.5 z * z (componentwise square), whose Jacobian -(A + diag(z)) has A's pattern (which holds the diagonal).
// mode 1: prints steady_adjoint's -J^-T b for J = -(A + diag(z)).
#include <cstdio>
#include <vector>
#include "vihds_steady.hpp"
template <int M, unsigned long long NZ>
static void run(int mode, const std::vector<float>& A, const std::vector<float>& b, std::vector<float>& z) {
  auto f = [&](const float* s, float* F) {
    for (int i = 0; i < M; ++i) {
      float v = b[i] - 0.5f * s[i] * s[i];
      for (int j = 0; j < M; ++j) if ((NZ >> (i * M + j)) & 1ull) v -= A[i * M + j] * s[j];
      F[i] = v;
    }
  };
  auto jac = [&](const float* s, float* J) {
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < M; ++j) if ((NZ >> (i * M + j)) & 1ull) J[i * M + j] = -(A[i * M + j] + (i == j ? s[i] : 0.f));
  };
  if (mode == 0) {
    vihds::steady_iterate<M, 12, NZ>(0.1f, 4.f, z.data(), f, jac);
  } else {
    std::vector<float> mu(b);
    vihds::steady_adjoint<M, NZ>(mu.data(), [&](float* J) { jac(z.data(), J); });
    z = mu;
  }
}
int main() {
  int m, pattern, mode;
  while (std::scanf("%d %d %d", &m, &pattern, &mode) == 3) {
    std::vector<float> A(m * m), b(m), z(m);
    for (float& v : A) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : b) if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : z) if (std::scanf("%f", &v) != 1) return 2;
    if (m == 1) run<1, 0x1ull>(mode, A, b, z);
    else if (m == 2 && pattern == 0) run<2, 0xfull>(mode, A, b, z);
    else if (m == 2) run<2, MASK_2_1>(mode, A, b, z);
    else if (m == 4 && pattern == 0) run<4, 0xffffull>(mode, A, b, z);
    else if (m == 4) run<4, MASK_4_1>(mode, A, b, z);
    else if (m == 8 && pattern == 0) run<8, 0xffffffffffffffffull>(mode, A, b, z);
    else if (m == 8) run<8, MASK_8_1>(mode, A, b, z);
    else return 3;
    for (int i = 0; i < m; ++i) std::printf("%.9g%c", z[i], i + 1 < m ? ' ' : '\n');
  }
  return 0;
}
"""


def _tridiagonal(m):
    return sum(1 << (i * m + j) for i in range(m) for j in range(m) if abs(i - j) <= 1)


MASKS = {(1, 0): 0x1, (2, 0): 0xf, (2, 1): sum(1 << (i * 2 + j) for i in range(2) for j in range(2) if j <= i),
         (4, 0): 0xffff, (4, 1): _tridiagonal(4), (8, 0): (1 << 64) - 1, (8, 1): _tridiagonal(8)}


def _host_compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) or (name if os.path.exists(name) else None)
        if path:
            return path
    return None


def _gauss(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A (float64: the yardstick; float32: the error to expect)."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        q = k + int(np.argmax(np.abs(A[k:, k])))
        if q != k:
            A[[k, q]], b[[k, q]] = A[[q, k]], b[[q, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] = A[i, k:] - m * A[k, k:]
            b[i] = b[i] - m * b[k]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_iteration_and_adjoint_solve_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/vihds_steady.hpp compiled as plain C++ with -fsanitize=address,undefined into a program of its own, which runs
    steady_iterate (12 iterations, delta 0.1, growth 4) and steady_adjoint for 1, 2, 4 and 8 unknowns on dense and sparse patterns
    (lower triangular, ChainEight's tridiagonal) with diagonally dominant matrices.  Against the same computation in float64
    with the Gaussian elimination above (the deltas formed in float32, as the header forms them); the bound per case is 8 x the
    error of that computation in float32, floored at 1e-6 -- both printed."""
    chain = G.steady_pattern(SS.ChainEight)
    assert MASKS[(8, 1)] == sum(1 << (i * 8 + j) for i in range(8) for j in range(8) if chain[i][j])
    src, exe = tmp_path / "steady.cpp", tmp_path / "steady"
    src.write_text(PROGRAM)
    defines = ["-DMASK_%d_%d=0x%xull" % (m, pt, MASKS[(m, pt)]) for m, pt in sorted(MASKS) if pt]
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined"] + defines + ["-I", CSRC, str(src), "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    rng = np.random.RandomState(7)
    cases = []
    for (m, pattern), mask in sorted(MASKS.items()):
        keep = np.array([[(mask >> (i * m + j)) & 1 for j in range(m)] for i in range(m)], dtype=np.float64)
        assert keep.diagonal().all()
        for mode in (0, 1):
            for _ in range(3):
                A = (0.5 * rng.randn(m, m) + np.diag(m + 1.0 + 2.0 * rng.rand(m))) * keep
                cases.append((m, pattern, mode, A, 1.0 + rng.rand(m), 0.1 + 0.5 * rng.rand(m)))
    fmt = lambda v: " ".join("%.9g" % x for x in np.asarray(v).reshape(-1))  # noqa: E731
    text = "".join("%d %d %d\n%s\n%s\n%s\n" % (m, pt, mode, fmt(A), fmt(b), fmt(z)) for m, pt, mode, A, b, z in cases)
    run = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(cases)

    def compute(A, b, z, mode, dtype):
        A, b, z = A.astype(dtype), b.astype(dtype), z.astype(dtype)
        if mode == 1:
            return -_gauss(-(A + np.diag(z)).T.copy(), b)
        delta = np.float32(0.1)
        for _ in range(12):
            F = (b - A @ z - dtype(0.5) * z * z).astype(dtype)
            J = -(A + np.diag(z))
            d = _gauss((np.eye(len(b), dtype=dtype) - dtype(delta) * J).astype(dtype), (dtype(delta) * F).astype(dtype))
            z = (z + d).astype(dtype)
            delta = np.float32(delta * np.float32(4.0))
        return z

    worst = (0.0, 0.0)
    for (m, pt, mode, A, b, z), row in zip(cases, rows):
        r32 = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731  (the program's inputs)
        exact = compute(r32(A), r32(b), r32(z), mode, np.float64)
        single = compute(r32(A), r32(b), r32(z), mode, np.float32).astype(np.float64)
        got = np.array([float(v) for v in row.split()])
        scale = np.abs(exact).max()
        e_got, e_single = np.abs(got - exact).max() / scale, np.abs(single - exact).max() / scale
        if e_got > worst[0]:
            worst = (e_got, e_single)
        assert e_got <= max(1e-6, 8.0 * e_single), (m, pt, mode, e_got, e_single)
    print("%d cases: worst unpivoted float32 error %.2e (the pivoted float32 computation there: %.2e)" % ((len(cases),) + worst))
