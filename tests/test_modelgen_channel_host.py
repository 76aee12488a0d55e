"""CPU tests of the reaction-channel noise of vihds.modelgen (`noise_channels` / `channel_noise`): the hook record beside the
pinned tuples, every refusal by its message, the generated text (members, constants, the fold of structural zeros) and its
digests, the unchanged text of every class without the attribute, the langevin helpers against hand-written columns, the traced
amplitudes and their adjoint against torch_channel_noise and autograd, the host's declines and the key columns, the inputs and
the statistics key of the GPU tests on the float64 definition, the documents, compilation for gfx950 without scratch, and the
host part of csrc/vihds_sde.hpp with a CPU restatement of the accumulation in a stand-alone program under sanitizers."""
import glob
import hashlib
import importlib
import json
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vihds import hip, modelgen as G, ops
from vihds.utils import attrify

import modelgen_channel_models as CM
import modelgen_sde_models as SM
import sde_ref
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
ALL = [c for c, _ in CM.PREBUILT]
GOLDEN = os.path.join(ROOT, "tests", "golden", "modelgen_channel_source_sha256.json")
# the modules whose PREBUILT lists existed before the hook
EARLIER_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models", "modelgen_implicit_models",
                   "modelgen_substep_models", "modelgen_jump_models", "modelgen_leadin_models", "modelgen_sdirk_models",
                   "modelgen_algebraic_models", "modelgen_delay_models", "modelgen_sde_models", "modelgen_missing_models",
                   "modelgen_stepctl_models")
one = lambda self, y, p, c: [[p.r, -p.r, 0.0, 0.0, 0.0, 0.0]]  # noqa: E731


def _chan(name, channel_noise=one, noise_channels=("flow",), **body):
    return _define(name, channel_noise=channel_noise, noise_channels=list(noise_channels), **body)


# ---- definition -----------------------------------------------------------------------------------------------------------------
def test_the_hook_record_stands_beside_the_pinned_tuples():
    h = G.HOOK["channel_noise"]
    assert h is G.CHANNEL_NOISE_HOOK and h not in G.TRACED_HOOKS and G.MODEL_HOOKS == G.TRACED_HOOKS + (h,)
    assert G.TRACED_HOOKS == G.ALL_HOOKS + (G.DIFFUSION_HOOK,) and G.ALL_HOOKS == (G.START_HOOK,) + G.HOOKS
    assert [r.name for r in G.HOOKS] == ["observe", "precision", "log_likelihood", "jump"]
    assert G.NOISE_HOOKS == (G.DIFFUSION_HOOK, h) and sorted(G.HOOK) == sorted(r.name for r in G.MODEL_HOOKS)
    assert h.groups == ("y",) and h.n_outputs == "channels" and h.count(6, 3) == 18 and h.count(4, 8) == 32
    assert h.checks_arguments and h.none_resets and not h.hides_method and h.skips_zero and h.switch == "HAS_DIFFUSION"
    assert h.targets == [("y", "yb"), ("p", "pb")] and h.excludes_neural
    assert "t" not in re.findall(r"\w+", h.signature)[1:]
    assert G.MAX_NOISE_CHANNELS == 8 and G.MAX_NOISE_ENTRIES == 32


def test_refusals_name_their_reason():
    ok = _chan("chan_ok")
    assert ok._channel_noise_def is one and ok._diffusion_def is None and len(ok._trace.chan) == 6 and ok._trace.n_channels == 1
    assert CM.pattern(ok) == [(0, 0), (1, 0)] and ok._trace.dif is None
    # together with diffusion; one without the other
    with pytest.raises(G.ModelDefinitionError, match=r"channel_noise\(self, y, p, c\) together with diffusion\(self, y, p, c\): a model has one noise term"):
        _chan("chan_both", diffusion=lambda self, y, p, c: [p.r] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="declares noise_channels without channel_noise"):
        _define("chan_names_only", noise_channels=["a"])
    with pytest.raises(G.ModelDefinitionError, match=r"defines channel_noise\(self, y, p, c\) without noise_channels"):
        _define("chan_hook_only", channel_noise=one)
    # arity: there is no t to read, and nothing else to take
    for bad in (lambda self, t, y, p, c: [list(y)], lambda self, y, p: [list(y)], lambda self, y, x, p, c: [list(y)]):
        with pytest.raises(G.ModelDefinitionError, match=r"channel_noise must be a function channel_noise\(self, y, p, c\).*no t"):
            _chan("chan_wrong_arguments", channel_noise=bad)
    with pytest.raises(G.ModelDefinitionError, match="channel_noise must be a function"):
        _chan("chan_not_callable", channel_noise=[[0.0] * 6])
    # the number of channels, and of entries per channel
    for bad in (lambda self, y, p, c: [[p.r] * 6] * 2, lambda self, y, p, c: [], lambda self, y, p, c: p.r):
        with pytest.raises(G.ModelDefinitionError, match=r"channel_noise must return a list of 1 lists, one per noise channel \(flow\)"):
            _chan("chan_wrong_channels", channel_noise=bad)
    for bad in (lambda self, y, p, c: [[p.r] * 5], lambda self, y, p, c: [[p.r] * 7], lambda self, y, p, c: [p.r]):
        with pytest.raises(G.ModelDefinitionError, match="channel 'flow' must be a list of 6 entries"):
            _chan("chan_wrong_entries", channel_noise=bad)
    with pytest.raises(G.ModelDefinitionError, match="channel 'idle' enters no species"):
        _chan("chan_empty_column", noise_channels=["flow", "idle"],
              channel_noise=lambda self, y, p, c: [[p.r] + [0.0] * 5, [0.0 * p.r] + [0.0] * 5])
    # names
    for names, why in ((["OD"], "'OD' is also a species"), (["r"], "'r' is also a species, a parameter"), (["a", "a"], "duplicates"),
                       (["not a name"], "valid identifiers"), ([3], "valid identifiers")):
        with pytest.raises(G.ModelDefinitionError, match="noise_channels.*%s" % why):
            _chan("chan_bad_names", noise_channels=names, channel_noise=lambda self, y, p, c: [[p.r] + [0.0] * 5] * len(names))
    with pytest.raises(G.ModelDefinitionError, match="'u' is also a species, a parameter, a forcing"):
        _chan("chan_forcing_name", noise_channels=["u"], forcings=["u"])
    with pytest.raises(G.ModelDefinitionError, match=r"9 noise channels.*at most 8 \(MAX_NOISE_CHANNELS"):
        _chan("chan_nine", noise_channels=["c%d" % r for r in range(9)],
              channel_noise=lambda self, y, p, c: [[p.r] + [0.0] * 5] * 9)
    with pytest.raises(G.ModelDefinitionError, match=r"36 entries that are not the constant 0.*at most 32 \(MAX_NOISE_ENTRIES\)"):
        _chan("chan_dense", noise_channels=["c%d" % r for r in range(6)],
              channel_noise=lambda self, y, p, c: [[p.r * v for v in y]] * 6)
    # what diffusion refuses, for the same reasons
    for has, reason in ((dict(implicit=True), r"implicit = True: a drift-implicit step"),
                        (dict(lead_in=0.5), r"lead_in = 0.5: the steps before the first observation point"),
                        (dict(networks={"n": G.Network(1, 2, 1)}, rhs=lambda self, t, y, p, c: [self.net.n([y[0]])[0]] + [0.0] * 5),
                         r"networks: the adjoint's dump"),
                        (dict(parameters=["r", "tau", "init_x"], delays={"lag": ("OD", "tau")},
                              prepare=lambda self, th, c: {"r": th.r, "tau": th.tau},
                              rhs=lambda self, t, y, p, c: [p.r * self.delayed.lag] + [0.0] * 5), r"delays: the stored history"),
                        (dict(algebraic=["Z"], constraint=lambda self, y, z, p, c: [z[0] - y[0]],
                              algebraic_start=lambda self, y, p, c: [y[0]],
                              rhs=lambda self, t, y, p, c: [p.r * self.algebraic.Z] + [0.0] * 5), r"algebraic variables: the amplitude")):
        with pytest.raises(G.ModelDefinitionError, match=r"defines channel_noise\(self, y, p, c\) and has %s.*declined in this version" % reason):
            _chan("chan_refused", **has)
    with pytest.raises(G.ModelDefinitionError, match=r"step_tolerance and channel_noise\(self, y, p, c\).*two noisy trial solutions"):
        _chan("chan_step_control", step_tolerance=(1e-3, 1e-6), substeps=4)
    with pytest.raises(G.ModelDefinitionError, match=r"defines channel_noise\(self, y, p, c\).*process noise of its own does not take NeuralPrecisions"):
        G.generate_source(ok, neural=True)
    for cls in ALL:
        with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
            G.generate_source(cls, True)
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _chan("chan_if", channel_noise=lambda self, y, p, c: [[p.r if y[0] > 1.0 else 0.0] + [0.0] * 5])
    with pytest.raises(G.ModelDefinitionError, match="noise_seed"):
        _chan("chan_bad_seed", noise_seed=-1)
    # channel_noise = None in a subclass removes the hook (and the inherited names with it)
    off = type("ChanOff", (ok,), {"model_key": "chan_off", "channel_noise": None})
    assert off._channel_noise_def is None and off._trace.chan is None and off.noise_channels == ()
    assert not any(w in G.generate_source(off) for w in ("channel_noise", "NOISE_CHANNELS", "channel_species", "HAS_DIFFUSION"))
    # what combines: forcings, substeps, jump, start, the observation hooks, missing observations, piecewise operations
    both = _chan("chan_combined", forcings=["u"], substeps=3, jump=lambda self, y, p, c: [0.5 * v for v in y],
                 start=lambda self, y, p, c: [v + 1.0 for v in y], observe=lambda self, y, p, c: [y[0], y[1], y[2], y[3]],
                 precision=lambda self, y, x, p, c: [1.0 + x[0]] * 4, missing_observations=True,
                 log_likelihood=lambda self, x, obs, pr, p, c: [-(x[j] - obs[j]) * (x[j] - obs[j]) * pr[j] for j in range(4)],
                 noise_channels=["a", "b"],
                 channel_noise=lambda self, y, p, c: [
                     [p.r * self.forcing.u * G.sqrt(G.maximum(y[0], 0.0)), G.where(y[1] > 0.5, p.r, 0.1), 0.0, 0.0, 0.0, 0.0],
                     [0.0, G.abs(y[1]), G.minimum(y[2], 1.0), 0.0, 0.0, 0.0]])
    src = G.generate_source(both)
    assert "NOISE_CHANNELS = 2" in src and "r == 0 ? 0x3u : 0x6u" in src and "SUBSTEPS = 3" in src and "OWN_JUMP" in src
    assert "OWN_START" in src and "MASKED_OBS" in src
    # a treatment the hook reads becomes one more effective parameter
    treated = _chan("chan_treated", n_conditions=2, channel_noise=lambda self, y, p, c: [[p.r * c[1], 0.0, 0.0, 0.0, 0.0, 0.0]])
    assert treated._trace.c_in_rhs == [1] and "p[1]" in _member(G.generate_source(treated), "channel_noise")


def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def test_generated_text_of_the_channels():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(c.__name__ for c in ALL)
    enters = {CM.ConversionPair: [0x3], CM.SharedChannel: [0x3, 0x1, 0x2], CM.ExpressionCLE: [0x1, 0x1, 0x2, 0x6, 0x4],
              CM.HookedChannels: [0x1, 0x6], CM.DiagonalTwin: [0x1, 0x2], CM.Channels8: [0xf] * 8}
    for cls in ALL:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)  # deterministic
        assert hashlib.sha256(src.encode()).hexdigest() == recorded[cls.__name__], cls.__name__
        N, R = len(cls.species), CM.n_channels(cls)
        pattern = CM.pattern(cls)
        assert [sum(1 << q for q, r_ in pattern if r_ == r) for r in range(R)] == enters[cls]
        assert src.count("  static constexpr bool HAS_DIFFUSION = true;") == 1 and "NOISE_MASK" not in src
        assert "  static constexpr int NOISE_CHANNELS = %d;" % R in src
        assert "  static constexpr int NOISE_ENTRIES = %d;" % len(pattern) in src
        picks = " : ".join(["r == %d ? 0x%xu" % (r, m) for r, m in enumerate(enters[cls][:-1])] + ["0x%xu" % enters[cls][-1]])
        assert "  __host__ __device__ static constexpr unsigned channel_species(int r) { return %s; }" % picks in src
        assert "  __device__ static void channel_noise(const float* y, const float* p, float* G) {" in src
        assert "  __device__ static void channel_noise_vjp(const float* y, const float* p, const float* Gb, float* yb, float* pb) {" in src
        assert " diffusion(" not in src and "diffusion_vjp" not in src
        # emitted last, after every other hook
        assert src.index("HAS_DIFFUSION") > max(src.find(s) for s in ("jump_vjp", "loglik_vjp", "precision_vjp", "observe_vjp", "rhs_vjp"))
        fwd = _member(src, "channel_noise")
        flat = sorted(q * R + r for q, r in pattern)
        assert sorted(int(j) for j in re.findall(r"G\[(\d+)\] = ", fwd)) == flat  # (a structural zero is not written ...)
        body = _member(src, "channel_noise_vjp")
        assert " = " not in re.sub(r"const (float|bool) v\d+ = ", "", body)  # the adjoint adds and never assigns
        assert sorted(set(int(j) for j in re.findall(r"Gb\[(\d+)\]", body))) == flat  # (... and its seed is not read)
        assert " / " not in fwd + body and "sqrtf(" not in fwd + body
        if cls.forcings:  # the sample of the interval's first point, never the interpolant
            assert "(t - p[" not in fwd + body and "p[%d]" % cls._trace.F0 in fwd
    # the diagonal twin's amplitudes are the diagonal class's, statement for statement
    twin, diag = G.generate_source(CM.DiagonalTwin), G.generate_source(SM.PrprLangevin)
    rename = lambda text: text.replace("G[0]", "g[0]").replace("G[3]", "g[1]").replace("Gb[0]", "gb[0]").replace("Gb[3]", "gb[1]")  # noqa: E731
    assert rename(_member(twin, "channel_noise")) == _member(diag, "diffusion")
    assert rename(_member(twin, "channel_noise_vjp")) == _member(diag, "diffusion_vjp")


def test_classes_without_the_attribute_generate_the_recorded_text():
    """Every (class, neural) of the PREBUILT lists that existed before the hook generates a text whose digest is among those
    recorded in tests/golden/modelgen_*_sha256*.json by the earlier pull requests, and none of the hook's words."""
    recorded = set()

    def collect(d):
        for v in d.values():
            collect(v) if isinstance(v, dict) else recorded.add(v)

    for path in glob.glob(os.path.join(ROOT, "tests", "golden", "modelgen_*sha256*.json")):
        if path != GOLDEN:
            with open(path) as f:
                collect(json.load(f))
    seen = 0
    for m in EARLIER_MODULES:
        for cls, neural in importlib.import_module(m).PREBUILT:
            text = G.generate_source(cls, neural)
            assert not any(w in text for w in ("channel_noise", "NOISE_CHANNELS", "NOISE_ENTRIES", "channel_species")), cls.__name__
            assert hashlib.sha256(text.encode()).hexdigest() in recorded, "%s.%s:%d" % (m, cls.__name__, int(neural))
            seen += 1
    assert seen == 95


# ---- the helpers ------------------------------------------------------------------------------------------------------------------
def test_the_langevin_helpers_against_hand_written_columns():
    nu = [[1, 0, 0], [-1, 1, 0], [0, -2, 3]]
    a = [torch.tensor([4.0, 9.0], dtype=F64), torch.tensor([1.0, -1.0], dtype=F64), torch.tensor([0.25, 16.0], dtype=F64)]
    cols = G.langevin(nu, a)
    r = [torch.sqrt(torch.clamp(v, min=0.0)) for v in a]
    want = [[r[0], 0.0, 0.0], [-r[1], r[1], 0.0], [0.0, -2.0 * r[2], 3.0 * r[2]]]
    for got_col, want_col in zip(cols, want):
        for g, w in zip(got_col, want_col):
            assert (isinstance(g, float) and g == 0.0) if isinstance(w, float) else torch.equal(g, w)
    assert float(cols[1][1][1]) == 0.0  # (a negative propensity is clamped to 0 under the root)
    floored = G.langevin(nu, a, floor=0.5)
    assert torch.equal(floored[1][1], torch.sqrt(torch.clamp(a[1], min=0.0) + 0.5))
    drift = G.langevin_drift(nu, a)
    assert torch.equal(drift[0], a[0] - a[1]) and torch.equal(drift[1], a[1] + (-2.0) * a[2]) and torch.equal(drift[2], 3.0 * a[2])
    assert G.langevin_drift([[0, 1]], [a[0]])[0] == 0.0
    # numbers stay numbers; model quantities fold the zeros into structural zeros
    assert G.langevin([[1, -1]], [4.0]) == [[2.0, -2.0]] and G.langevin_drift([[1, -1]], [4.0]) == [4.0, -4.0]
    cle = CM.ExpressionCLE
    assert CM.pattern(cle) == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 3), (2, 4)]
    assert "fsqrt(" in _member(G.generate_source(cle), "channel_noise")
    for bad, why in ((([[1, 0]], [1.0, 2.0]), "one row of stoichiometry per propensity"), (([[1, 0], [1]], [1.0, 2.0]), "same number"),
                     (([[0.5, 0]], [1.0]), "integers"), (([[True, 0]], [1.0]), "integers"), (([], []), "at least one")):
        with pytest.raises(G.ModelDefinitionError, match=why):
            G.langevin(*bad)
        with pytest.raises(G.ModelDefinitionError, match=why):
            G.langevin_drift(*bad)
    with pytest.raises(G.ModelDefinitionError, match="floor"):
        G.langevin([[1]], [1.0], floor=-1.0)


# ---- the torch restatement and the traced adjoint ---------------------------------------------------------------------------------
def _rand(shape, lo, hi, seed):
    return lo + (hi - lo) * torch.rand(shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.__name__)
def test_traced_channels_and_their_adjoint_match_torch_channel_noise_and_autograd(cls):
    """float64: evaluate of the traced nodes equals torch_channel_noise, and the reverse-mode adjoint the generator emits as
    channel_noise_vjp (then prepare_vjp) equals autograd through torch_channel_noise, for the species and every parameter.
    Bound 1e-12."""
    tr = cls._trace
    g = tr.g
    B, S, T, N, R = 3, 2, 4, len(cls.species), CM.n_channels(cls)
    NPU, K = len(tr.p_names), len(cls.forcings)
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    series = _rand((B, K, T), 0.2, 1.5, 95)
    words = [torch.full((B, T), 15.0, dtype=F64)] if cls.missing_observations else []
    cond = torch.cat([series.reshape(B, -1)] + words + [torch.tensor([[3.0, 5.0]], dtype=F64).expand(B, 2)], dim=1)
    y = _rand((B, S, N, T), 0.05, 0.9, 92)
    W = torch.randn(B, S, N, R, T, dtype=F64, generator=torch.Generator().manual_seed(8))
    env0 = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
    pv = G.evaluate(tr.p_exprs, env0)
    env = {("p", k): pv[k].expand(B, S)[:, :, None] for k in range(NPU)}
    env.update({("y", j): y[:, :, j] for j in range(N)})
    env.update({("f", k): series[:, k, None, :] for k in range(K)})
    full = lambda v: v.expand(B, S, T) if isinstance(v, torch.Tensor) else torch.full((B, S, T), float(v), dtype=F64)  # noqa: E731
    traced = torch.stack([full(v) for v in G.evaluate(tr.chan, env)], dim=2).reshape(B, S, N, R, T)  # (flat index q * R + r)
    adj = G.vjp(g, tr.chan, [g.leaf("seed", j) for j in range(N * R)])
    e = dict(env)
    e.update({("seed", q * R + r): W[:, :, q, r] for q in range(N) for r in range(R)})
    leaves = [g.leaf("y", j) for j in range(N)] + [g.leaf("p", k) for k in range(NPU)]
    out = [full(v) for v in G.evaluate([adj.get(l.id, g.const(0.0)) for l in leaves], e)]
    yb, pb = torch.stack(out[:N], dim=2), out[N:]
    adjp = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    e0 = dict(env0)
    e0.update({("seed", k): pb[k].sum(2) for k in range(NPU)})
    thb = G.evaluate([adjp.get(g.leaf("th", s).id, g.const(0.0)) for s in range(len(cls.parameter_names))], e0)
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    ref = cls.torch_channel_noise(yt, tht, cond)
    assert ref.shape == (B, S, N, R, T)
    (ref * W).sum().backward()
    err = lambda a, b: float(((a - b).abs() / (1.0 + b.abs())).max())  # noqa: E731
    assert err(traced, ref.detach()) <= 1e-12
    assert err(yb, yt.grad if yt.grad is not None else torch.zeros_like(y)) <= 1e-12
    for n, v in zip(cls.parameter_names, thb):
        want = tht[n].grad if tht[n].grad is not None else torch.zeros(B, S, dtype=F64)
        got = v.expand(B, S) if isinstance(v, torch.Tensor) else torch.full((B, S), float(v), dtype=F64)
        assert err(got, want) <= 1e-12, n
    for n in CM.NOISE_PARAMETERS[cls]:
        assert float(tht[n].grad.abs().max()) > 0.0, n
    # outside the pattern the restatement is 0, inside it is not
    inside = torch.zeros(N, R, dtype=torch.bool)
    for q, r in CM.pattern(cls):
        inside[q, r] = True
    assert float(ref.detach()[:, :, ~inside].abs().max() if bool((~inside).any()) else 0.0) == 0.0
    assert all(float(ref.detach()[:, :, q, r].abs().max()) > 0.0 for q, r in CM.pattern(cls))
    with pytest.raises(G.ModelDefinitionError, match="defines no channel_noise"):
        SM.PrprLangevin.torch_channel_noise(y, th, cond)
    with pytest.raises(G.ModelDefinitionError, match="defines no diffusion"):
        cls.torch_diffusion(y, th, cond)


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def _config(solver, n_conditions=0):
    return SimpleNamespace(device="cpu", params=attrify({"solver": solver}),
                           data=SimpleNamespace(device_depth=1, conditions=["c%d" % k for k in range(n_conditions)],
                                                relevance_vectors={}, default_devices=[]))


def test_host_declines_before_any_library_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hip, "lib", no_library)
    monkeypatch.setattr(G, "register_kernel", no_library)
    fixed = "fixed-grid solvers: beuler, euler, midpoint, modeuler, modeulerwhile, rk4"
    for cls in (CM.ConversionPair, CM.Channels8):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        monkeypatch.setattr(hip, "GENERATED_DIFFUSION", hip.GENERATED_DIFFUSION | {key})  # (what register_kernel records)
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"process noise.*'%s'.*%s" % (solver, fixed)):
                ops.OdeProblemSpec(key, solver, {}, 1, C=2)
        model = cls(_config("dopri5"))
        assert model.has_diffusion and model.n_noise_channels == CM.n_channels(cls)
        with pytest.raises(NotImplementedError, match=r"defines channel_noise\(self, y, p, c\).*'dopri5'.*%s" % fixed):
            model.solve(_config("dopri5"), torch.tensor(CM.RAGGED), None, torch.zeros(3, 2), None)
    # a cond without the two key columns is refused before anything is built
    with pytest.raises(ValueError, match="2 noise-key columns"):
        CM.ExpressionCLE(_config("rk4")).solve(_config("rk4"), torch.tensor(CM.RAGGED), None, torch.zeros(3, 9), None)
    assert SM.PrprLangevin(_config("rk4")).n_noise_channels == 0 and SM.PrprLangevin(_config("rk4")).has_diffusion
    from modelgen_models import PrprRestated
    plain = PrprRestated(_config("rk4"))
    assert not plain.has_diffusion and plain.n_noise_channels == 0
    with pytest.raises(AttributeError):
        CM.Channels8(_config("rk4")).n_noise_channels = 3  # (read-only)


def test_row_inputs_the_key_state_and_stored_evaluations():
    from vihds import ode

    B, T = 3, 9
    plain = SimpleNamespace(inputs=torch.zeros(B, 0))
    model = CM.Channels8(_config("rk4"))
    assert model.cond_width(T) == 2 and CM.ExpressionCLE(_config("rk4")).cond_width(T) == T + 2
    assert CM.HookedChannels(_config("rk4")).cond_width(T) == T + 2  # (the mask words, then the key)
    rows = model.row_inputs(SimpleNamespace(inputs=plain.inputs, noise_key=(7, 16777215)))
    assert rows.shape == (B, 2) and rows.dtype == torch.float32 and rows.tolist() == [[7.0, 16777215.0]] * B
    seeded = type("Seeded", (CM.Channels8,), {"model_key": None, "noise_seed": (5 << 24) + (1 << 24) - 1})(_config("rk4"))
    seeded.train()
    assert [seeded.row_inputs(plain)[0].tolist() for _ in range(2)] == [[16777215.0, 5.0], [0.0, 6.0]]
    seeded.eval()
    assert seeded.row_inputs(plain)[0].tolist() == [16777215.0, 5.0]
    assert seeded.state_dict()["noise_key_state"].tolist() == [1.0, 6.0]
    request = SimpleNamespace(general_tail=False)
    config = SimpleNamespace(params=attrify({"lazy_x_predict": True}))
    with torch.no_grad():
        assert not ode.x_predict_on_demand(request, model, config)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------
def _preconditions(cls, pb, solver, xi):
    starts = []
    with torch.no_grad():
        xs, xp, lp = CM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], xi, starts, pb["observed"])
        quiet, _, _ = CM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], torch.zeros_like(xi), None, pb["observed"])
    assert bool(torch.isfinite(xs).all() and torch.isfinite(lp).all())
    assert len(starts) == CM.n_steps(cls, pb["T"])
    margin = CM.kink_margin(cls, starts)
    moved = min(float((xs[:, :, j] - quiet[:, :, j]).abs().max() / (quiet[:, :, j].max() - quiet[:, :, j].min()))
                for j in CM.noisy_species(cls))
    terms = lp * pb["G"]["logp"]
    return margin, moved, float(terms.abs().sum() / terms.sum().abs())


def test_the_inputs_of_the_gpu_tests():
    """The preconditions of the GPU comparisons, on the float64 run with the restatement's draws: every state finite, every
    argument of a sqrt / maximum and every condition of a where at least 1e-3 (relative) away from its kink, the noise moves
    every noisy species by at least 1 % of its range, the loss is no cancelling sum, and the gradient row of every noise parameter
    is not zero.  (DiagonalTwin runs on its twin's problem, whose inputs tests/test_modelgen_sde_host.py checks.)"""
    cases = [(cls, B, S, CM.RAGGED) for cls in CM.PARITY for B, S in ((3, 5), (3, 100))]
    cases += [(cls, 3, 100, [0.25, 0.75]) for cls in (CM.ExpressionCLE, CM.Channels8)]  # (the T = 2 cases)
    for cls, B, S, grid in cases:
        pb = CM.problem(cls, B, S, times=grid)
        xi = torch.from_numpy(sde_ref.expected_draws(B, S, 8, CM.n_steps(cls, pb["T"]), pb["key"])).to(F64)
        for solver in (CM.FIXED if len(grid) > 2 else ("modeuler", "rk4")):
            margin, moved, condition = _preconditions(cls, pb, solver, xi)
            print("%s %s %dx%d T=%d: kink margin %.2e, noise moves %.1f %% of the range, condition %.2f"
                  % (cls.__name__, solver, B, S, pb["T"], margin, 100 * moved, condition))
            assert margin >= 1e-3 and moved >= 0.01 and condition <= 4.0
        th = {n: v.clone().requires_grad_(True) for n, v in pb["th"].items()}
        _, _, lp = CM.forward(cls, th, pb["cond"], pb["times"], "rk4", pb["obs"], xi, None, pb["observed"])
        (lp * pb["G"]["logp"]).sum().backward()
        for n in CM.NOISE_PARAMETERS[cls]:
            assert float(th[n].grad.abs().max()) > 0.0, (cls.__name__, n)
    assert CM.kinked_species(CM.ExpressionCLE) == [0, 1, 2] and CM.kinked_species(CM.HookedChannels) == [1]
    assert CM.kinked_species(CM.Channels8) == [0, 1, 2, 3] and CM.kinked_species(CM.SharedChannel) == []
    # ConversionPair under euler: the definition conserves A + B, and A moves
    pb = CM.problem(CM.ConversionPair, 3, 100)
    xi = torch.from_numpy(sde_ref.expected_draws(3, 100, 8, 8, pb["key"])).to(F64)
    xs, _, _ = CM.forward(CM.ConversionPair, pb["th"], pb["cond"], pb["times"], "euler", None, xi)
    total = xs[:, :, 0] + xs[:, :, 1]
    assert float((total - total[..., :1]).abs().max()) <= 1e-14
    assert float((xs[:, :, 0] - xs[:, :, 0, :1]).abs().max()) > 0.1


def test_the_definition_with_a_diagonal_pattern_is_the_diagonal_definition():
    """CM.forward on DiagonalTwin equals SM.forward on PrprLangevin, given the same draws: the channel sum restates g * xi."""
    pb = SM.problem(SM.PrprLangevin, 3, 5)
    xi = torch.from_numpy(sde_ref.expected_draws(3, 5, 8, 8, pb["key"])).to(F64)
    for solver in ("euler", "rk4"):
        a = SM.forward(SM.PrprLangevin, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], xi)
        b = CM.forward(CM.DiagonalTwin, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], xi)
        for u, v in zip(a, b):
            assert float((u - v).abs().max()) <= 1e-13 * float(u.abs().max())


def test_the_statistics_key_passes_with_the_draws_of_the_restatement():
    """What tests/test_modelgen_channel_gpu.py asserts of the kernels under CM.STAT_KEY, here in float64 with the draws of
    sde_ref under the same key: the key was chosen so that both pass (largest deviation printed)."""
    cls, B, S = CM.SharedChannel, CM.STAT_B, CM.STAT_S
    times = torch.tensor(CM.RAGGED).float().double()
    th = {k: torch.full((B, S), v, dtype=F64) for k, v in dict(CM.BASES[cls], **CM.STAT_THETA).items()}
    xi = torch.from_numpy(sde_ref.expected_draws(B, S, 4, len(CM.RAGGED) - 1, CM.STAT_KEY)).to(F64)
    with torch.no_grad():
        xs, _, _ = CM.forward(cls, th, torch.zeros(B, 2, dtype=F64), times, "euler", None, xi)
    mean_se, var_se, cov_se, corrs, bound = CM.shared_statistics(xs.reshape(B * S, 4, -1)[:, :2], times)
    print("mean %s, variance %s, covariance %.2f standard errors; correlations %s (bound %.4f)" % (
        ["%.2f" % v for v in mean_se], ["%.2f" % v for v in var_se], cov_se, {k: round(v, 4) for k, v in corrs.items()}, bound))
    assert all(abs(v) <= 5.0 for v in mean_se + var_se + [cov_se]) and all(abs(c) <= bound for c in corrs.values())
    # the statistic notices what it is for: per-species draws (no shared channel) miss the covariance by many standard errors
    with torch.no_grad():
        apart = SM.forward(SM.OrnsteinUhlenbeck, {k: torch.full((B, S), v, dtype=F64) for k, v in dict(
            SM.BASES[SM.OrnsteinUhlenbeck], a=0.8, sigma=0.5, init=1.0).items()}, torch.zeros(B, 2, dtype=F64), times, "euler", None, xi)[0]
    assert abs(CM.shared_statistics(apart.reshape(B * S, 4, -1)[:, :2], times)[2]) > 20.0


# ---- documents ------------------------------------------------------------------------------------------------------------------
def test_the_documents_have_the_paragraph():
    for word in ("Noise channels.", "noise_channels = [", "def channel_noise(self, y, p, c)", "chemical Langevin", "structural zero",
                 "NOISE_CHANNELS", "channel_species", "channel_noise_vjp", "torch_channel_noise", "langevin_drift", "MAX_NOISE_CHANNELS",
                 "MAX_NOISE_ENTRIES", "MODEL_HOOKS", "tau-leaping", "more than 8 channels", "non-diagonal noise", "Milstein",
                 "drift-implicit", "noise in the lead-in", "sharded"):
        assert word in G.__doc__, word
    assert G.__doc__.index("Noise channels.") > G.__doc__.index("Process noise.")
    read = lambda name: open(os.path.join(ROOT, name)).read()  # noqa: E731
    assert "channel_noise(self, y, p, c)" in read("README.md")
    for name in ("INTEGRATION.md", "DESIGN.md"):
        text = read(name)
        assert "channel_noise(self, y, p, c)" in text and "noise_channels" in text and "langevin" in text, name
    design = read("DESIGN.md")
    for word in ("non-diagonal noise", "Milstein", "drift-implicit", "noise in the lead-in", "tau-leaping", "more than 8 channels"):
        assert word in design[design.index("## 8"):], word
    assert "MAX_NOISE_ENTRIES" in design and "VGPR" in design[design.index("MAX_NOISE_ENTRIES"):]


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", [CM.Channels8, CM.ExpressionCLE, CM.HookedChannels], ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every fixed-grid solver compile for gfx950 and spill nothing
    (VGPRs printed; recorded in DESIGN.md).  Channels8 is the worst case: eight channels at MAX_NOISE_ENTRIES entries."""
    if cls is CM.Channels8:
        assert len(CM.pattern(cls)) == G.MAX_NOISE_ENTRIES and CM.n_channels(cls) == G.MAX_NOISE_CHANNELS
    header = tmp_path / "chan.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(has_diffusion<VIHDS_GEN_CORE>::value && cond_tail<VIHDS_GEN_CORE>() == 2);",
             "static_assert(noise_channels<VIHDS_GEN_CORE>::value == %d);" % CM.n_channels(cls),
             "static_assert(noise_channels<PrprConstant>::value == 0 && noise_channels<WithPrec<PrprConstant>>::value == 0);"]
    for solver in CM.FIXED:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "chan"), "_ZN5vihds")
    assert len(usage) == 15, sorted(usage)
    for solver in CM.FIXED:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d" % (cls.__name__, solver, min(fwd), max(fwd), bwd[0]))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


# ---- the host part of csrc/vihds_sde.hpp in a stand-alone program under sanitizers -----------------------------------------------
PROGRAM = r"""
// prints: block, lane and counter of channels 0 .. 7; which Philox blocks R channels draw; the accumulation over a structural
// pattern (3 species, 4 channels) from a heap array of G that holds EXACTLY the flat entries up to the last one of the pattern --
// a read of a structural zero behind it is a heap overflow -- beside a restatement written out by hand; and the seeds of the
// adjoint, written into a heap array of the same size filled with a sentinel
#include <cmath>
#include <cstdio>
#include <memory>
#include "vihds_sde.hpp"
using namespace vihds;
struct Pattern {  // species 0 <- channels 0, 2;  species 1 <- channels 0, 1, 3;  species 2 <- channel 3
  static constexpr int N = 3;
  static constexpr int NOISE_CHANNELS = 4;
  static constexpr unsigned channel_species(int r) { return r == 0 ? 0x3u : r == 1 ? 0x2u : r == 2 ? 0x1u : 0x6u; }
};
int main() {
  for (int r = 0; r < 8; ++r) {
    const SdeCounter c = sde_channel_counter(1234u, r, 11u);
    std::printf("channel %d %u %d %u %u %u %u\n", r, sde_channel_block(r), sde_channel_lane(r), c.c0, c.c1, c.c2, c.c3);
  }
  for (int R = 1; R <= 8; ++R)
    std::printf("blocks %d %d %d\n", R, (int)sde_block_drawn(sde_channel_mask(R), 0), (int)sde_block_drawn(sde_channel_mask(R), 1));
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 3; ++q) std::printf("enters %d %d %d\n", r, q, (int)sde_channel_enters<Pattern>(r, q));
  constexpr int R = Pattern::NOISE_CHANNELS, LAST = 2 * R + 3;  // the last entry of the pattern: species 2, channel 3
  std::unique_ptr<float[]> G(new float[LAST + 1]), Gb(new float[LAST + 1]);
  for (int j = 0; j <= LAST; ++j) { G[j] = 0.25f * (float)(j + 1); Gb[j] = -77.f; }
  const float dw[R] = {0.5f, -1.5f, 2.f, 0.125f};
  float y[3] = {1.f, 2.f, 3.f};
  sde_channel_accumulate<Pattern>(G.get(), dw, y);
  float w[3] = {1.f, 2.f, 3.f};  // by hand, channel by channel
  w[0] = std::fmaf(G[0 * R + 0], dw[0], w[0]); w[1] = std::fmaf(G[1 * R + 0], dw[0], w[1]);
  w[1] = std::fmaf(G[1 * R + 1], dw[1], w[1]);
  w[0] = std::fmaf(G[0 * R + 2], dw[2], w[0]);
  w[1] = std::fmaf(G[1 * R + 3], dw[3], w[1]); w[2] = std::fmaf(G[2 * R + 3], dw[3], w[2]);
  for (int q = 0; q < 3; ++q) std::printf("y %d %.9g %.9g\n", q, (double)y[q], (double)w[q]);
  const float lam[3] = {2.f, -3.f, 0.5f};
  sde_channel_seed<Pattern>(lam, dw, Gb.get());
  for (int j = 0; j <= LAST; ++j) std::printf("seed %d %.9g\n", j, (double)Gb[j]);
  return 0;
}
"""


def _host_compiler():
    return shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_the_channel_helpers_in_a_host_program_under_sanitizers(tmp_path):
    src, exe = tmp_path / "chan_host.cpp", tmp_path / "chan_host"
    src.write_text(PROGRAM)
    subprocess.check_call([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    channels = [[int(v) for v in l.split()[1:]] for l in out if l.startswith("channel ")]
    for r, (q, block, lane, c0, c1, c2, c3) in enumerate(channels):
        (r0, r1, r2, r3), rl = sde_ref.counter(1234, r, 11)
        assert (q, block, lane, c0, c1, c2, c3) == (r, r >> 2, r & 3, r0, r1, r2, r3) and lane == rl
    assert len(channels) == 8
    blocks = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in out if l.startswith("blocks ")}
    assert blocks == {R: (1, 1 if R > 4 else 0) for R in range(1, 9)}
    pattern = {(0, 0), (0, 1), (1, 1), (2, 0), (3, 1), (3, 2)}  # (channel, species)
    enters = {(int(l.split()[1]), int(l.split()[2])): int(l.split()[3]) for l in out if l.startswith("enters ")}
    assert enters == {(r, q): int((r, q) in pattern) for r in range(4) for q in range(3)}
    ys = [l.split() for l in out if l.startswith("y ")]
    assert len(ys) == 3 and all(a == b for _, _, a, b in ys) and [float(v[2]) for v in ys] != [1.0, 2.0, 3.0]
    # the same accumulation in numpy's float32, fused by hand through float64 (a product of two float32 is exact in float64)
    G_ = [np.float32(0.25 * (j + 1)) for j in range(12)]
    dw = [np.float32(v) for v in (0.5, -1.5, 2.0, 0.125)]
    want = [np.float32(1.0), np.float32(2.0), np.float32(3.0)]
    for r, q in sorted(pattern):
        want[q] = np.float32(np.float64(G_[q * 4 + r]) * np.float64(dw[r]) + np.float64(want[q]))
    assert [float(v[2]) for v in ys] == [float(v) for v in want]
    seeds = [float(l.split()[2]) for l in out if l.startswith("seed ")]
    lam = (2.0, -3.0, 0.5)
    assert seeds == [lam[j // 4] * float(dw[j % 4]) if (j % 4, j // 4) in pattern else -77.0 for j in range(12)]
