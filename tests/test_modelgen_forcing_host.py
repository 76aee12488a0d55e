"""CPU tests of the forcings of vihds.modelgen (time-varying inputs read as self.forcing.<name>): tracing and validation
errors, the generated text, the unchanged text of models without forcings, the torch restatement against a linear function
written into rhs by hand, the host-side checks that run before anything is built or queued, the batch plumbing, the
precondition of the GPU comparisons, and compilation for gfx950 (scratch and VGPRs of every fixed-grid kernel of the three
test models)."""
import hashlib
import json
import os
import re
import shutil
from types import SimpleNamespace

import pytest
import torch

from oracle import vihds_oracle as O
from vihds import modelgen as G
from vihds import training
from vihds.utils import attrify

import modelgen_forcing_models as FM
import modelgen_models as MM
import modelgen_piecewise_models as PM
from test_modelgen_host import _compile_usage, _define, _resource_usage
from test_modelgen_observe_host import _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _with_light(name, **body):
    """_define's six-species model with one forcing, read in rhs unless `body` says otherwise."""
    attrs = dict(forcings=["light"], rhs=lambda self, t, y, p, c: [p.r * y[0] * self.forcing.light] + [0.0] * 5)
    attrs.update(body)
    return _define(name, **attrs)


# ---- tracing and validation ---------------------------------------------------------------------------------------------------
def test_definition_errors():
    ok = _with_light("forced_ok")
    assert ok._trace.forcings == ["light"] and G.GeneratedOdeModel.forcings == ()
    with pytest.raises(G.ModelDefinitionError, match="forcing 'light' read in prepare"):
        _with_light("forced_in_prepare", prepare=lambda self, th, c: {"r": th.r * self.forcing.light})
    with pytest.raises(G.ModelDefinitionError, match="forcing 'light' read in initial_state"):
        _with_light("forced_in_init", initial_state=lambda self, th, c: [th.init_x * self.forcing.light] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="also a species or a parameter"):
        _with_light("forced_clash_parameter", forcings=["r"])
    with pytest.raises(G.ModelDefinitionError, match="also a species or a parameter"):
        _with_light("forced_clash_species", forcings=["OD"])
    with pytest.raises(G.ModelDefinitionError, match="at most %d" % G.MAX_FORCINGS):
        _with_light("forced_five", forcings=["f%d" % k for k in range(G.MAX_FORCINGS + 1)])
    assert G.MAX_FORCINGS == 4
    with pytest.raises(G.ModelDefinitionError, match="valid identifiers"):
        _with_light("forced_bad_name", forcings=["not a name"])
    with pytest.raises(G.ModelDefinitionError, match="duplicates"):
        _with_light("forced_twice", forcings=["light", "light"])
    with pytest.raises(G.ModelDefinitionError, match="unknown forcing 'temp'"):
        _with_light("forced_unknown", rhs=lambda self, t, y, p, c: [p.r * self.forcing.temp] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="read-only"):
        def assigns(self, t, y, p, c):
            self.forcing.light = 1.0
            return [p.r] * 6
        _with_light("forced_assigned", rhs=assigns)


def test_a_forcing_is_a_leaf_without_adjoint():
    g = G.Graph()
    f, a = g.leaf("f", 0), g.leaf("th", 0)
    adj = G.vjp(g, [f * a + G.exp(f)], [1.0])
    assert f.id not in adj and adj[a.id] is f
    assert "f" in G._NO_ADJOINT and "ob" in G._NO_ADJOINT


def _config(solver, n_conditions):
    return SimpleNamespace(device="cpu", params=attrify({"solver": solver}),
                           data=SimpleNamespace(device_depth=1, conditions=["c%d" % k for k in range(n_conditions)],
                                                relevance_vectors={}, default_devices=[]))


def test_host_checks_run_before_anything_is_built(monkeypatch):
    """An adaptive solver and a wrong cond width raise from solve, ahead of the library build and of every launch."""
    def no_build(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(G, "register_kernel", no_build)
    times = torch.tensor(PM.TIMES)
    for cls in (FM.PrprForced, FM.ForcedSwitch):
        K, C, T = len(cls.forcings), int(cls.n_conditions), len(PM.TIMES)
        model = cls(_config("dopri5", C))
        good = torch.zeros(3, C + K * T)
        with pytest.raises(NotImplementedError, match="adaptive solver 'dopri5'"):
            model.solve(model_config(model, "dopri5"), times, None, good, None)
        model = cls(_config("rk4", C))
        with pytest.raises(ValueError, match=r"must hold %d samples behind its %d treatment\(s\), and holds %d" % (K * T, C, K * T - 1)):
            model.solve(model_config(model, "rk4"), times, None, good[:, :-1], None)
        assert model.cond_width(T) == C + K * T
        with pytest.raises(RuntimeError, match="number of time points"):
            model.cond_width()
    plain = MM.PrprRestated(_config("rk4", 0))
    assert plain.cond_width() == 0 and plain.cond_width(9) == 0


def model_config(model, solver):
    return _config(solver, model.n_treatments)


def test_row_inputs_and_the_batch_plumbing():
    B, T = 3, len(PM.TIMES)
    cls = FM.ForcedSwitch
    model = cls(_config("rk4", 1))
    series = FM.series_of(cls, B, torch.tensor(PM.TIMES, dtype=F64)).float()
    items = [{"devices": 0, "dev_1hot": torch.ones(1), "inputs": torch.full((1,), 0.1 * b), "observations": torch.zeros(4, T),
              "forcings": series[b]} for b in range(B)]
    batch = training.collate_merged(torch.tensor(PM.TIMES), "cpu", items)
    assert torch.equal(batch.forcings, series) and batch.forcings.dtype == torch.float32
    wide = model.row_inputs(batch)
    assert wide.shape == (B, 1 + 2 * T)
    assert torch.equal(wide[:, :1], batch.inputs) and torch.equal(wide[:, 1:].reshape(B, 2, T), series)
    # a batch without the key is what it was, and a model without forcings reads data.inputs itself
    plain = training.collate_merged(torch.tensor(PM.TIMES), "cpu", [{k: v for k, v in it.items() if k != "forcings"} for it in items])
    assert "forcings" not in plain and sorted(plain) == ["dev_1hot", "devices", "inputs", "observations", "times"]
    assert MM.PrprRestated(_config("rk4", 1)).row_inputs(plain) is plain.inputs
    with pytest.raises(RuntimeError, match="every batch needs 'forcings'"):
        model.row_inputs(plain)
    with pytest.raises(RuntimeError, match="must be"):
        model.row_inputs(attrify(dict(plain, forcings=series[:, :1])))


# ---- generated text -----------------------------------------------------------------------------------------------------------
def test_generated_text():
    cls = FM.ForcedSwitch
    src = G.generate_source(cls)
    assert src == G.generate_source(cls)
    tr = cls._trace
    K, F0 = 2, tr.F0
    assert F0 == tr.NP == len(tr.p_names) + 1  # (the named parameters, then the treatment rhs reads)
    assert "static constexpr int N_FORCINGS = 2;" in src and "static constexpr int NP = %d;" % (F0 + 2 * K + 1) in src
    si, sp = _member(src, "set_interval"), _member(src, "set_point")
    for k in range(K):
        assert "p[%d] = u_lo[%d];" % (F0 + k, k) in si and "p[%d] = (u_hi[%d] - u_lo[%d]) * inv_dt;" % (F0 + K + k, k, k) in si
        assert "p[%d] = u[%d];" % (F0 + k, k) in sp and "p[%d] = 0.f;" % (F0 + K + k) in sp
    assert "p[%d] = t_lo;" % (F0 + 2 * K) in si and "t_lo" not in sp
    # rhs and its adjoint read the interpolant at t, the hooks the value
    at_t = ["(p[%d] + (t - p[%d]) * p[%d])" % (F0 + k, F0 + 2 * K, F0 + K + k) for k in range(K)]
    for m in ("rhs", "rhs_vjp"):
        body = _member(src, m)
        assert all(text in body for text in at_t), m
    for m in ("loglik", "loglik_vjp"):
        body = _member(src, m)
        assert "p[%d]" % (F0 + 1) in body and "(t - " not in body and "p[%d]" % (F0 + K + 1) not in body, m
    # nothing of the forcing entries is prepared, and no adjoint is formed for them
    slots = ["p[%d]" % k for k in range(F0, F0 + 2 * K + 1)] + ["pb[%d]" % k for k in range(F0, F0 + 2 * K + 1)]
    for m in ("prepare", "prepare_vjp", "init", "init_vjp"):
        assert not any(s in _member(src, m) for s in slots), m
    for m in ("rhs_vjp", "loglik_vjp"):
        assert not any(s in _member(src, m) for s in slots[2 * K + 1:]), m
    # the network takes the interpolants as inputs; the condition compares one
    assert re.search(r"const float n0_x\[3\] = \{\(p\[%d\] \+ " % F0, _member(src, "rhs"))
    assert re.search(r"const bool v\d+ = 0\.5f < \(p\[%d\] \+ " % F0, _member(src, "rhs"))
    # a forcing read by the hooks only
    reader = G.generate_source(FM.PlateReaderForced)
    f0 = FM.PlateReaderForced._trace.F0
    assert "p[%d]" % f0 not in _member(reader, "rhs") and "p[%d]" % f0 in _member(reader, "observe")
    assert "p[%d]" % f0 in _member(reader, "precision_vjp") and "pb[%d]" % f0 not in reader


def test_models_without_forcings_generate_the_recorded_text():
    for name in ("modelgen_source_sha256.json", "modelgen_source_sha256_all.json"):
        with open(os.path.join(ROOT, "tests", "golden", name)) as f:
            recorded = json.load(f)
        if name.endswith("_all.json"):
            continue  # (checked entry by entry in tests/test_modelgen_tables_host.py: the file must exist unchanged)
        for key, digest in recorded.items():
            cname, neural = key.split(":")
            text = G.generate_source(getattr(MM, cname), bool(int(neural)))
            assert hashlib.sha256(text.encode()).hexdigest() == digest, key
            assert "N_FORCINGS" not in text and "set_interval" not in text and "set_point" not in text
    twin = G.generate_source(FM.PrprTreated)
    assert "N_FORCINGS" not in twin and "set_point" not in twin


def test_docstring_has_a_forcings_paragraph():
    doc = G.__doc__
    for word in ("Forcings.", "self.forcing.", "forcings = [", "linear interpolant", "MAX_FORCINGS", "adaptive", "row_inputs",
                 "no gradient"):
        assert word in doc, word


# ---- the torch restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", FM.FIXED)
def test_a_linear_forcing_equals_the_line_written_into_rhs(solver):
    """float64 torch_problem of PrprForced with samples of 0.4 + 0.25 t against PrprRamped, which has that line in rhs: the
    interpolant reproduces a linear function exactly.  Bound 1e-12 relative."""
    B, S = 3, 4
    pb = FM.problem(FM.PrprRamped, B, S)
    times = pb["times"]
    a0, a1 = FM.PrprRamped.RAMP
    series = (a0 + a1 * times)[None, None, :].expand(B, 1, -1)
    wide = FM.wide_cond(torch.zeros(B, 0, dtype=F64), series)
    xs, _, _, logp = FM.forward(FM.PrprForced, pb["th"], wide, times, solver, pb["obs"])
    ref_xs, _, _, ref_logp = FM.forward(FM.PrprRamped, pb["th"], pb["cond"], times, solver, pb["obs"])
    e_xs = float(((xs - ref_xs).abs() / ref_xs.abs().clamp_min(1e-300)).max())
    e_lp = float(((logp - ref_logp).abs() / ref_logp.abs()).max())
    print("%s: trajectory %.2e, log-likelihood %.2e" % (solver, e_xs, e_lp))
    assert e_xs <= 1e-12 and e_lp <= 1e-12
    assert float((xs[:, :, 2] - FM.forward(MM.PrprRestated, pb["th"], pb["cond"], times, solver)[0][:, :, 2]).abs().max()) > 1e-3


def test_torch_restatements_take_the_wide_cond():
    cls = FM.ForcedSwitch
    pb = FM.problem(cls, 3, 5)
    with pytest.raises(ValueError, match="needs times="):
        cls.torch_problem(pb["th"], pb["cond"], pb["W"])
    with pytest.raises(ValueError, match="must hold 18 samples behind its 1 treatment"):
        cls.torch_problem(pb["th"], pb["cond"][:, :-1], pb["W"], times=pb["times"])
    rhs, x0 = cls.torch_problem(pb["th"], pb["cond"], pb["W"], times=pb["times"])
    # at a grid point the interpolant is the sample, from either side; between two points it is their mean at the middle
    y = x0 + 0.3
    light, temp = pb["series"][:, 0], pb["series"][:, 1]

    def by_hand(k, lam):
        one = dict(pb, series=None)
        u = [(1 - lam) * s[:, k] + lam * s[:, k + 1] for s in (light, temp)]
        flat = torch.stack([u[0], u[1]], dim=1)[:, :, None].expand(3, 2, pb["T"])
        r, _ = cls.torch_problem(pb["th"], FM.wide_cond(one["treatments"], flat), pb["W"], times=pb["times"])
        return r(pb["times"][0], y)

    for k, lam in ((2, 0.0), (2, 0.5), (7, 1.0)):
        t = (1 - lam) * pb["times"][k] + lam * pb["times"][k + 1]
        assert torch.allclose(rhs(t, y), by_hand(k, lam), rtol=1e-13, atol=0.0)
    # the hooks see the samples themselves: a likelihood evaluated on a series that is constant in time at point k's values
    xs, xp, prec, logp = FM.forward(cls, pb["th"], pb["cond"], pb["times"], "rk4", pb["obs"], pb["W"])
    ll = cls.torch_log_likelihood(xp, pb["obs"], prec, pb["th"], pb["cond"])
    k = 4
    flat = pb["series"][:, :, k:k + 1].expand(3, 2, pb["T"])
    ll_k = cls.torch_log_likelihood(xp, pb["obs"], prec, pb["th"], FM.wide_cond(pb["treatments"], flat))
    assert torch.equal(ll[..., k], ll_k[..., k]) and not torch.equal(ll[..., k + 1], ll_k[..., k + 1])
    # a NaN sample propagates
    bad = pb["cond"].clone()
    bad[1, 1 + 3] = float("nan")
    xs_bad = FM.forward(cls, pb["th"], bad, pb["times"], "rk4", weights=pb["W"])[0]
    assert bool(torch.isnan(xs_bad[1, :, 2, 4:]).all()) and bool(torch.isfinite(xs_bad[0]).all())


@pytest.mark.parametrize("solver", FM.FIXED)
def test_the_float64_yardstick_keeps_the_light_switch_wide(solver):
    """The precondition of the GPU comparisons on the yardstick alone, at both of their shapes: the interpolated square wave
    stays at least 1e-3 (relative margin) away from 0.5 at every stage time, and both sides occur."""
    cls = FM.ForcedSwitch
    for B, S in ((3, 5), (3, 100)):
        pb = FM.problem(cls, B, S)
        with FM.recording() as m:
            xs, xp, prec, logp = FM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], pb["W"])
        print("%s %dx%d: smallest margin %.2e" % (solver, B, S, m.smallest))
        assert m.smallest >= PM.MARGIN and bool(torch.isfinite(logp).all())
    light = pb["series"][:, 0]
    assert bool((light > 0.5).any()) and bool((light < 0.5).any())
    assert not torch.equal(light[0], light[1]) and not torch.equal(light[1], light[2])
    assert float(pb["series"].abs().max()) <= 2.0 and float(pb["series"].abs().min()) >= 0.1  # O(1)


# ---- compilation --------------------------------------------------------------------------------------------------------------
SOLVERS = ["MODEULER", "MODEULERWHILE", "EULER", "MIDPOINT", "RK4"]


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
@pytest.mark.parametrize("cls", FM.MODELS, ids=lambda c: c.__name__)
def test_forcing_models_compile_without_scratch_for_every_fixed_grid_solver(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint (for the model with a network also its dump form) of the three
    models for every fixed-grid solver: they compile for gfx950 and spill nothing.  (VGPR ranges printed, recorded in
    DESIGN.md.)  The traits say what the kernels see."""
    header = tmp_path / "forcing.hpp"
    header.write_text(G.generate_source(cls))
    K = len(cls.forcings)
    dump = bool(cls.networks)
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(n_forcings<VIHDS_GEN_CORE>::value == %d && n_forcings<WithPrec<VIHDS_GEN_CORE>>::value == %d);" % (K, K),
             "static_assert(n_forcings<PrprConstant>::value == 0 && n_forcings<WithPrec<PrprConstant>>::value == 0);",
             "static_assert(n_forcings<BlackboxIcml>::value == 0);"]
    for s in SOLVERS:
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
        lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
        if dump:
            lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
    lines.append("}")
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", "forcing"), "_ZN5vihds")
    assert len(usage) == (4 if dump else 3) * len(SOLVERS), sorted(usage)
    for kind in ("ode_fwd_kernel", "ode_bwd_kernel"):
        vgprs = [v for name, (v, _) in usage.items() if kind in name]
        print("%s %s: %d .. %d VGPRs" % (cls.__name__, kind, min(vgprs), max(vgprs)))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_launcher_of_a_forced_model_holds_no_adaptive_or_summary_kernel(tmp_path):
    """launch_ode of a model with forcings, all solvers in one unit: the only kernels it instantiates are the fixed-grid
    forward and adjoint -- no trial, grid-barrier or summaries kernel."""
    header = tmp_path / "forcing.hpp"
    header.write_text(G.generate_source(FM.PrprForced))
    text = ('#include "vihds_ode_kernels.hpp"\n#include "%s"\nnamespace vihds {\n'
            "int forced_launch(bool b, int s, const OdeArgs& a, hipStream_t st, const LaunchMode& m) {\n"
            "  return launch_ode<VIHDS_GEN_CORE, -1>(b, s, a, st, m);\n}\n}\n" % header)
    usage = _resource_usage(_compile_usage(tmp_path, text, "forced_launch"), "_ZN5vihds")
    assert len(usage) == 3 * len(SOLVERS), sorted(usage)  # (staged forward, unstaged forward, adjoint)
    assert all("ode_fwd_kernel" in n or "ode_bwd_kernel" in n for n in usage), sorted(usage)
