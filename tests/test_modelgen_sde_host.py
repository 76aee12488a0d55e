"""CPU tests of the process noise of vihds.modelgen (the `diffusion` hook): the hook record, every refusal by its message, the
host's declines, the generated text and its digests (and the unchanged text of every class without the hook), the traced
amplitudes and their adjoint against torch_diffusion and autograd, the key columns of row_inputs and the key state, the strong
order of the float64 definition, the documents, compilation for gfx950 without scratch, and the host part of csrc/vihds_sde.hpp in
a stand-alone program under the address and undefined-behaviour sanitizers."""
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

import modelgen_sde_models as SM
import sde_ref
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
ALL = [c for c, _ in SM.PREBUILT]
GOLDEN = os.path.join(ROOT, "tests", "golden", "modelgen_sde_source_sha256.json")
# the modules whose PREBUILT lists existed before the hook
EARLIER_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models", "modelgen_implicit_models",
                   "modelgen_substep_models", "modelgen_jump_models", "modelgen_leadin_models", "modelgen_sdirk_models",
                   "modelgen_algebraic_models", "modelgen_delay_models")
unit = lambda self, y, p, c: [p.r, 0.0, 0.0, 0.0, 0.0, 0.0]  # noqa: E731


# ---- definition -----------------------------------------------------------------------------------------------------------------
def test_the_hook_record():
    h = G.HOOK["diffusion"]
    assert h is G.DIFFUSION_HOOK and G.TRACED_HOOKS == G.ALL_HOOKS + (h,) and h not in G.ALL_HOOKS
    assert h.groups == ("y",) and h.n_outputs == "species" and h.count(6) == 6 and h.count(3) == 3
    assert h.checks_arguments and h.none_resets and not h.hides_method and h.skips_zero and h.switch == "HAS_DIFFUSION"
    assert h.targets == [("y", "yb"), ("p", "pb")] and h.excludes_neural
    assert "t" not in re.findall(r"\w+", h.signature)[1:] and not any(r.skips_zero for r in G.ALL_HOOKS)


def test_refusals_name_their_reason():
    ok = _define("sde_ok", diffusion=unit)
    assert ok._diffusion_def is unit and len(ok._trace.dif) == 6 and SM.noisy_species(ok) == [0]
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
        with pytest.raises(G.ModelDefinitionError, match=r"defines diffusion\(self, y, p, c\) and has %s.*declined in this version" % reason):
            _define("sde_refused", diffusion=unit, **has)
    with pytest.raises(G.ModelDefinitionError, match=r"defines diffusion\(self, y, p, c\).*process noise of its own does not take NeuralPrecisions"):
        G.generate_source(ok, neural=True)
    for cls in ALL:
        with pytest.raises(G.ModelDefinitionError, match="does not take NeuralPrecisions"):
            G.generate_source(cls, True)
    # arity: there is no t to read, and nothing else to take
    for bad in (lambda self, t, y, p, c: list(y), lambda self, y, p: list(y), lambda self, y, x, p, c: list(y)):
        with pytest.raises(G.ModelDefinitionError, match=r"diffusion must be a function diffusion\(self, y, p, c\).*no t"):
            _define("sde_wrong_arguments", diffusion=bad)
    with pytest.raises(G.ModelDefinitionError, match="diffusion must be a function"):
        _define("sde_not_callable", diffusion=[0.0] * 6)
    for bad in (lambda self, y, p, c: [p.r] * 4, lambda self, y, p, c: [p.r] * 7, lambda self, y, p, c: p.r):
        with pytest.raises(G.ModelDefinitionError, match="diffusion must return a list of 6 entries"):
            _define("sde_wrong_length", diffusion=bad)
    with pytest.raises(G.ModelDefinitionError, match="returns the constant 0 for every species"):
        _define("sde_all_zero", diffusion=lambda self, y, p, c: [0.0] * 6)
    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("sde_if", diffusion=lambda self, y, p, c: [p.r if y[0] > 1.0 else 0.0] + [0.0] * 5)
    for seed in (-1, 1 << 48, 0.5, True):
        with pytest.raises(G.ModelDefinitionError, match="noise_seed"):
            _define("sde_bad_seed", diffusion=unit, noise_seed=seed)
    # diffusion = None in a subclass removes the hook
    off = type("SdeOff", (ok,), {"model_key": "sde_off", "diffusion": None})
    assert off._diffusion_def is None and off._trace.dif is None and "diffusion" not in G.generate_source(off).lower()
    # what combines: forcings, substeps, jump, start, the observation hooks, piecewise operations
    both = _define("sde_combined", forcings=["u"], substeps=3, jump=lambda self, y, p, c: [0.5 * v for v in y],
                   start=lambda self, y, p, c: [v + 1.0 for v in y], observe=lambda self, y, p, c: [y[0], y[1], y[2], y[3]],
                   precision=lambda self, y, x, p, c: [1.0 + x[0]] * 4,
                   log_likelihood=lambda self, x, obs, pr, p, c: [-(x[j] - obs[j]) * (x[j] - obs[j]) * pr[j] for j in range(4)],
                   diffusion=lambda self, y, p, c: [p.r * self.forcing.u * G.sqrt(G.maximum(y[0], 0.0)), G.where(y[1] > 0.5, p.r, 0.1),
                                                    0.0, 0.0, 0.0, 0.0])
    src = G.generate_source(both)
    assert "NOISE_MASK = 0x3u" in src and "SUBSTEPS = 3" in src and "OWN_JUMP" in src and "OWN_START" in src


def _member(src, name):
    m = re.search(r"__device__ static void %s\((.*?)\) \{\n(.*?)\n  \}" % name, src, re.S)
    assert m, name
    return m.group(2)


def test_generated_text_of_a_diffusion():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(c.__name__ for c in ALL)
    masks = {SM.Brownian8: 0xff, SM.OrnsteinUhlenbeck: 0xf, SM.PrprLangevin: 0x3, SM.LightSub4: 0x6, SM.DilutedHooked: 0x3}
    for cls in ALL:
        src = G.generate_source(cls)
        assert src == G.generate_source(cls)  # deterministic
        assert hashlib.sha256(src.encode()).hexdigest() == recorded[cls.__name__], cls.__name__
        assert src.count("  static constexpr bool HAS_DIFFUSION = true;") == 1
        assert "  static constexpr unsigned NOISE_MASK = 0x%xu;" % masks[cls] in src
        assert "  __device__ static void diffusion(const float* y, const float* p, float* g) {" in src
        assert "  __device__ static void diffusion_vjp(const float* y, const float* p, const float* gb, float* yb, float* pb) {" in src
        # emitted last, after every other hook
        assert src.index("HAS_DIFFUSION") > max(src.find(s) for s in ("jump_vjp", "loglik_vjp", "precision_vjp", "observe_vjp", "rhs_vjp"))
        noisy = SM.noisy_species(cls)
        fwd = _member(src, "diffusion")
        assert sorted(int(j) for j in re.findall(r"g\[(\d+)\] = ", fwd)) == noisy  # (a zero amplitude is not written ...)
        if cls in (SM.Brownian8, SM.OrnsteinUhlenbeck):  # (constant amplitudes: no state adjoint)
            continue
        body = _member(src, "diffusion_vjp")
        # the adjoint adds and never assigns, reads the seeds of the noisy species only, uses the time-loop helpers
        assert " = " not in re.sub(r"const (float|bool) v\d+ = ", "", body)
        assert sorted(set(int(j) for j in re.findall(r"gb\[(\d+)\]", body))) == noisy  # (... and its seed is not read)
        assert " / " not in fwd + body and "sqrtf(" not in fwd + body and "fsqrt(" in fwd
        if cls.forcings:  # the sample of the interval's first point, never the interpolant
            assert "(t - p[" not in fwd + body and "p[%d]" % cls._trace.F0 in fwd
    assert "diffusion_vjp(const float* y, const float* p, const float* gb, float* yb, float* pb) {\n  }" in G.generate_source(SM.Brownian8)
    # without the hook: the parent's text, but for the names and the parameter
    twin = type("PrprLangevin", (SM.PrprLangevin,), {"model_key": SM.PrprLangevin.model_key, "diffusion": None,
                                                     "__module__": SM.PrprLangevin.__module__})
    a, b = G.generate_source(twin).splitlines(), G.generate_source(SM.PrprLangevin).splitlines()
    assert a[2:-4] == b[2:len(a) - 4] and "HAS_DIFFUSION" in b[len(a) - 4]


def test_classes_without_the_hook_generate_the_recorded_text():
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
            assert "diffusion" not in text.lower() and "NOISE_MASK" not in text, cls.__name__
            assert hashlib.sha256(text.encode()).hexdigest() in recorded, "%s.%s:%d" % (m, cls.__name__, int(neural))
            seen += 1
    assert seen == 70


# ---- the torch restatement and the traced adjoint ---------------------------------------------------------------------------------
def _rand(shape, lo, hi, seed):
    return lo + (hi - lo) * torch.rand(shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("cls", SM.PARITY + [SM.OrnsteinUhlenbeck], ids=lambda c: c.__name__)
def test_traced_diffusion_and_its_adjoint_match_torch_diffusion_and_autograd(cls):
    """float64: evaluate of the traced nodes equals torch_diffusion, and the reverse-mode adjoint the generator emits as
    diffusion_vjp (then prepare_vjp) equals autograd through torch_diffusion, for the species and every parameter.  Bound 1e-12."""
    tr = cls._trace
    g = tr.g
    B, S, T, N = 3, 2, 4, len(cls.species)
    NPU, K = len(tr.p_names), len(cls.forcings)
    th = {n: _rand((B, S), 0.3, 1.2, 3 + k) for k, n in enumerate(cls.parameter_names)}
    series = _rand((B, K, T), 0.2, 1.5, 95)
    cond = torch.cat([series.reshape(B, -1), torch.tensor([[3.0, 5.0]], dtype=F64).expand(B, 2)], dim=1)
    y = _rand((B, S, N, T), 0.05, 0.9, 92)
    W = torch.randn(B, S, N, T, dtype=F64, generator=torch.Generator().manual_seed(8))
    env0 = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
    pv = G.evaluate(tr.p_exprs, env0)
    env = {("p", k): pv[k].expand(B, S)[:, :, None] for k in range(NPU)}
    env.update({("y", j): y[:, :, j] for j in range(N)})
    env.update({("f", k): series[:, k, None, :] for k in range(K)})
    full = lambda v: v.expand(B, S, T) if isinstance(v, torch.Tensor) else torch.full((B, S, T), float(v), dtype=F64)  # noqa: E731
    traced = torch.stack([full(v) for v in G.evaluate(tr.dif, env)], dim=2)
    adj = G.vjp(g, tr.dif, [g.leaf("seed", j) for j in range(N)])
    e = dict(env)
    e.update({("seed", j): W[:, :, j] for j in range(N)})
    leaves = [g.leaf("y", j) for j in range(N)] + [g.leaf("p", k) for k in range(NPU)]
    out = [full(v) for v in G.evaluate([adj.get(l.id, g.const(0.0)) for l in leaves], e)]
    yb, pb = torch.stack(out[:N], dim=2), out[N:]
    adjp = G.vjp(g, tr.p_exprs, [g.leaf("seed", k) for k in range(NPU)])
    e0 = dict(env0)
    e0.update({("seed", k): pb[k].sum(2) for k in range(NPU)})
    thb = G.evaluate([adjp.get(g.leaf("th", s).id, g.const(0.0)) for s in range(len(cls.parameter_names))], e0)
    tht = {n: v.clone().requires_grad_(True) for n, v in th.items()}
    yt = y.clone().requires_grad_(True)
    ref = cls.torch_diffusion(yt, tht, cond)
    assert ref.shape == (B, S, N, T)
    (ref * W).sum().backward()
    err = lambda a, b: float(((a - b).abs() / (1.0 + b.abs())).max())  # noqa: E731
    assert err(traced, ref.detach()) <= 1e-12
    assert err(yb, yt.grad if yt.grad is not None else torch.zeros_like(y)) <= 1e-12
    for n, v in zip(cls.parameter_names, thb):
        want = tht[n].grad if tht[n].grad is not None else torch.zeros(B, S, dtype=F64)
        got = v.expand(B, S) if isinstance(v, torch.Tensor) else torch.full((B, S), float(v), dtype=F64)
        assert err(got, want) <= 1e-12, n
    assert float(tht["sigma"].grad.abs().max()) > 0.0
    quiet = [j for j in range(N) if j not in SM.noisy_species(cls)]
    assert float(ref.detach()[:, :, quiet].abs().max() if quiet else 0.0) == 0.0
    from modelgen_models import PrprRestated
    with pytest.raises(G.ModelDefinitionError, match="defines no diffusion"):
        PrprRestated.torch_diffusion(y, th, cond)


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
    for cls in (SM.PrprLangevin, SM.LightSub4):
        key = cls.model_key
        monkeypatch.setitem(hip.MODELS, key, 1024)
        monkeypatch.setattr(hip, "GENERATED_DIFFUSION", hip.GENERATED_DIFFUSION | {key})  # (what register_kernel records)
        for solver in hip.ADAPTIVE_SOLVERS:
            with pytest.raises(NotImplementedError, match=r"process noise.*'%s'.*%s" % (solver, fixed)):
                ops.OdeProblemSpec(key, solver, {}, 1, C=2)
    for cls in (SM.PrprLangevin, SM.OrnsteinUhlenbeck):  # (a class with a jump or sub-steps is declined for those first)
        model = cls(_config("dopri5"))
        assert model.has_diffusion
        with pytest.raises(NotImplementedError, match=r"defines diffusion\(self, y, p, c\).*'dopri5'.*%s" % fixed):
            model.solve(_config("dopri5"), torch.tensor(SM.RAGGED), None, torch.zeros(3, 2), None)
    # a cond without the two key columns is refused before anything is built
    with pytest.raises(ValueError, match="2 noise-key columns"):
        SM.LightSub4(_config("rk4")).solve(_config("rk4"), torch.tensor(SM.RAGGED), None, torch.zeros(3, 9), None)
    from modelgen_models import PrprRestated
    assert not PrprRestated(_config("rk4")).has_diffusion


def test_evaluation_stores_x_predict_for_a_model_with_process_noise():
    from vihds import ode
    from modelgen_models import PrprRestated

    request = SimpleNamespace(general_tail=False)
    config = SimpleNamespace(params=attrify({"lazy_x_predict": True}))
    with torch.no_grad():
        assert ode.x_predict_on_demand(request, PrprRestated(_config("rk4")), config)
        assert not ode.x_predict_on_demand(request, SM.PrprLangevin(_config("rk4")), config)


def test_row_inputs_and_the_key_state():
    B, T = 3, 9
    plain = SimpleNamespace(inputs=torch.zeros(B, 0))
    model = SM.PrprLangevin(_config("rk4"))
    assert model.cond_width(T) == 2 and model.cond_width() == 2
    forced = SM.LightSub4(_config("rk4"))
    assert forced.cond_width(T) == T + 2
    # a batch's own key: one pair, or one pair per row
    rows = model.row_inputs(SimpleNamespace(inputs=plain.inputs, noise_key=(7, 16777215)))
    assert rows.shape == (B, 2) and rows.dtype == torch.float32 and rows.tolist() == [[7.0, 16777215.0]] * B
    per_row = [[1, 2], [3, 4], [5, 6]]
    assert model.row_inputs(SimpleNamespace(inputs=plain.inputs, noise_key=torch.tensor(per_row))).tolist() == [[float(v) for v in r] for r in per_row]
    series = torch.arange(B * T, dtype=torch.float32).reshape(B, 1, T)
    wide = forced.row_inputs(SimpleNamespace(inputs=torch.zeros(B, 0), forcings=series, noise_key=np.array([9, 8])))
    assert wide.shape == (B, T + 2) and torch.equal(wide[:, :T], series[:, 0]) and wide[:, T:].tolist() == [[9.0, 8.0]] * B
    assert torch.equal(G._forcing_series(SM.LightSub4, wide, wide, T)[:, 0], series[:, 0])
    # bad keys are refused on the host
    for bad, why in (((1 << 24, 0), r"\[0, 2\^24\)"), ((-1, 0), r"\[0, 2\^24\)"), ((0.5, 1), "integers"), ((1, 2, 3), "one pair"),
                     ([[1, 2]] * (B + 1), "one pair"), ((float("nan"), 0), "integers"), ("ab", "integers")):
        with pytest.raises(ValueError, match=why):
            model.row_inputs(SimpleNamespace(inputs=plain.inputs, noise_key=bad))
    # without a key: training mode reads the state and advances it, evaluation mode keeps the seed's key
    cls = type("Seeded", (SM.PrprLangevin,), {"model_key": None, "noise_seed": (5 << 24) + (1 << 24) - 2})
    seeded = cls(_config("rk4"))
    seeded.train()
    keys = [seeded.row_inputs(plain)[0].tolist() for _ in range(3)]
    assert keys == [[16777214.0, 5.0], [16777215.0, 5.0], [0.0, 6.0]]  # (the counter carries into the second word at 2^24)
    assert seeded.row_inputs(plain).tolist() == [[1.0, 6.0]] * B
    seeded.eval()
    assert [seeded.row_inputs(plain)[0].tolist() for _ in range(2)] == [[16777214.0, 5.0]] * 2
    seeded.train()
    assert seeded.row_inputs(plain)[0].tolist() == [2.0, 6.0]  # (evaluations did not advance it)
    model.eval()
    assert model.row_inputs(plain).tolist() == [[0.0, 0.0]] * B  # (noise_seed = 0 by default)
    # the state is a buffer: saved with the model, moved (not seeded again) with it, and a loaded state continues the stream
    saved = seeded.state_dict()
    assert saved["noise_key_state"].tolist() == [3.0, 6.0] and "noise_eval_key" not in saved
    fresh = cls(_config("rk4"))
    fresh.load_state_dict(saved)
    fresh.train()
    assert fresh.row_inputs(plain)[0].tolist() == [3.0, 6.0] and fresh.noise_state("cpu") is fresh._buffers["noise_key_state"]
    from modelgen_models import PrprRestated
    assert "noise_key_state" not in PrprRestated(_config("rk4")).state_dict()
    hi = type("Wrap", (SM.PrprLangevin,), {"model_key": None, "noise_seed": (1 << 48) - 1})(_config("rk4"))
    hi.train()
    assert [hi.row_inputs(plain)[0].tolist() for _ in range(2)] == [[16777215.0, 16777215.0], [0.0, 0.0]]


# ---- the definition checks itself -----------------------------------------------------------------------------------------------
def test_halving_the_step_halves_the_strong_error_of_the_additive_noise_model():
    """OrnsteinUhlenbeck in float64 with euler on [0, 2]: levels of 8, 16, 32, 64 and 512 steps driven by the SAME Brownian path
    (the coarse increments are sums of the finest ones, passed as xi = dW / sqrt(h)).  Additive noise: Euler-Maruyama has strong
    order 1 here, so the root-mean-square error against the finest level halves per level; the test derives its margin from its
    own two finer levels -- the ratio of the two coarse errors lies within the deviation from 2 that the two finer ones show,
    doubled, and no less than 2 +- 0.25."""
    cls, B, S, fine = SM.OrnsteinUhlenbeck, 1, 2000, 512
    gen = torch.Generator().manual_seed(5)
    th = {n: torch.full((B, S), v, dtype=F64) for n, v in SM.BASES[cls].items()}
    cond = torch.zeros(B, 2, dtype=F64)
    dW = torch.randn(B, S, 4, fine, generator=gen, dtype=F64) * (2.0 / fine) ** 0.5

    def end_state(n):
        inc = dW.reshape(B, S, 4, n, fine // n).sum(-1)
        times = torch.linspace(0.0, 2.0, n + 1, dtype=F64)
        xs, _, _ = SM.forward(cls, th, cond, times, "euler", None, inc / (2.0 / n) ** 0.5)
        return xs[..., -1]

    ref = end_state(fine)
    err = {n: float(((end_state(n) - ref) ** 2).mean().sqrt()) for n in (8, 16, 32, 64)}
    print("strong errors: %s" % ", ".join("%d steps %.3e" % kv for kv in sorted(err.items())))
    fine_ratios = [err[16] / err[32], err[32] / err[64]]
    margin = max(0.25, 2.0 * max(abs(r - 2.0) for r in fine_ratios))
    print("ratios %.3f (coarse), %.3f, %.3f; margin %.3f" % (err[8] / err[16], fine_ratios[0], fine_ratios[1], margin))
    assert abs(err[8] / err[16] - 2.0) <= margin and margin <= 0.5
    # ... and the noise matters: a scheme that ignored it would be off by the order of the process's own spread, sigma /
    # sqrt(2 a) = 0.4, several times the coarsest level's error
    quiet, _, _ = SM.forward(cls, th, cond, torch.linspace(0.0, 2.0, 65, dtype=F64), "euler", None, torch.zeros(B, S, 4, 64, dtype=F64))
    assert float(((quiet[..., -1] - ref) ** 2).mean().sqrt()) > 4 * err[8]


def test_the_draws_of_the_restatement():
    """sde_ref: the counter layout, the disjoint theta stream, keys and rows."""
    assert sde_ref.counter(7, 5, 11) == ((7, 1, 11, sde_ref.STREAM_TAG), 1) and sde_ref.STREAM_TAG != 0
    assert sde_ref.step_index(2, 4, 3) == 11 and sde_ref.step_index(5, 1, 0) == 5
    a = sde_ref.expected_draws(3, 5, 8, 6, SM.KEY)
    assert a.shape == (3, 5, 8, 6) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, sde_ref.expected_draws(3, 5, 8, 6, SM.KEY))
    assert not np.array_equal(a, sde_ref.expected_draws(3, 5, 8, 6, (SM.KEY[0] + 1, SM.KEY[1])))
    # the first two rows of a B = 3 problem are the B = 2 problem's; more steps extend the draws
    assert np.array_equal(a[:2], sde_ref.expected_draws(2, 5, 8, 6, SM.KEY)) and np.array_equal(a, sde_ref.expected_draws(3, 5, 8, 9, SM.KEY)[..., :6])
    # the theta stream at the same trajectory, block, step and key differs (its fourth counter word is 0)
    from philox_ref import expected_kernel_normals
    theta = expected_kernel_normals(3, 5, 8, SM.KEY[0] | (SM.KEY[1] << 32), 0)
    assert not np.array_equal(theta, a[..., 0])
    big = sde_ref.expected_draws(4, 4096, 4, 8, (11, 22)).astype(np.float64)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1.0) < 5 * np.sqrt(2.0 / big.size)


def test_the_inputs_of_the_gpu_tests():
    """The preconditions of the GPU comparisons, on the float64 run with the restatement's draws: every state finite, every
    argument of a sqrt / maximum at least 1e-3 (relative) above its kink, the noise moves every noisy species by at least 1 % of
    its range, and the loss is no cancelling sum."""
    cases = [(cls, B, S, SM.RAGGED) for cls in SM.PARITY for B, S in ((3, 5), (3, 100))]
    cases += [(cls, 3, 100, [0.25, 0.75]) for cls in (SM.PrprLangevin, SM.LightSub4)]  # (the T = 2 cases)
    for cls, B, S, grid in cases:
        pb = SM.problem(cls, B, S, times=grid)
        xi = torch.from_numpy(sde_ref.expected_draws(B, S, 8, SM.n_steps(cls, pb["T"]), pb["key"])).to(F64)
        for solver in (SM.FIXED if len(grid) > 2 else ("modeuler", "rk4")):
            starts = []
            with torch.no_grad():
                xs, xp, lp = SM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], xi, starts)
                quiet, _, _ = SM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"], torch.zeros_like(xi))
            assert bool(torch.isfinite(xs).all() and torch.isfinite(lp).all())
            assert len(starts) == SM.n_steps(cls, pb["T"])
            margin = SM.kink_margin(cls, starts)
            moved = min(float((xs[:, :, j] - quiet[:, :, j]).abs().max() / (quiet[:, :, j].max() - quiet[:, :, j].min()))
                        for j in SM.noisy_species(cls))
            terms = lp * pb["G"]["logp"]
            condition = float(terms.abs().sum() / terms.sum().abs())
            print("%s %s %dx%d T=%d: kink margin %.2e, noise moves %.1f %% of the range, condition %.2f"
                  % (cls.__name__, solver, B, S, pb["T"], margin, 100 * moved, condition))
            assert margin >= 1e-3 and moved >= 0.01 and condition <= 4.0


def test_the_statistics_key_passes_with_the_draws_of_the_restatement():
    """What tests/test_modelgen_sde_gpu.py asserts of the kernels under SM.STAT_KEY, here in float64 with the draws of sde_ref
    under the same key: the key was chosen so that both pass (largest deviation printed)."""
    cls, B, S = SM.OrnsteinUhlenbeck, SM.STAT_B, SM.STAT_S
    times = torch.tensor(SM.RAGGED).float().double()
    th = {k: torch.full((B, S), v, dtype=F64) for k, v in dict(SM.BASES[cls], **SM.STAT_THETA).items()}
    xi = torch.from_numpy(sde_ref.expected_draws(B, S, 4, len(SM.RAGGED) - 1, SM.STAT_KEY)).to(F64)
    with torch.no_grad():
        xs, _, _ = SM.forward(cls, th, torch.zeros(B, 2, dtype=F64), times, "euler", None, xi)
    mean_se, var_se, corrs, bound = SM.ou_statistics(xs.reshape(B * S, 4, -1), times)
    print("mean %s, variance %s standard errors; correlations %s (bound %.4f)" % (
        ["%.2f" % v for v in mean_se], ["%.2f" % v for v in var_se], {k: round(v, 4) for k, v in corrs.items()}, bound))
    assert all(abs(v) <= 5.0 for v in mean_se + var_se) and all(abs(c) <= bound for c in corrs.values())
    assert SM.kinked_species(SM.PrprLangevin) == [0, 1] and SM.kinked_species(SM.LightSub4) == [1]
    assert SM.kinked_species(SM.DilutedHooked) == [1] and SM.kinked_species(cls) == []


# ---- documents ------------------------------------------------------------------------------------------------------------------
def test_the_documents_have_the_paragraph():
    for word in ("Process noise.", "def diffusion(self, y, p, c)", "Euler-Maruyama", "strong order 1/2", "the IWAE bound gains no term",
                 "HAS_DIFFUSION", "diffusion_vjp", "torch_diffusion", "noise_key", "noise_seed", "2^24", "non-diagonal noise", "Milstein",
                 "drift-implicit", "noise in the lead-in", "sharded"):
        assert word in G.__doc__, word
    read = lambda name: open(os.path.join(ROOT, name)).read()  # noqa: E731
    assert "diffusion(self, y, p, c)" in read("README.md")
    for name in ("INTEGRATION.md", "DESIGN.md"):
        text = read(name)
        assert "diffusion(self, y, p, c)" in text and "vihds_sde.hpp" in text and "noise_key" in text, name
    design = read("DESIGN.md")
    for word in ("non-diagonal noise", "Milstein", "drift-implicit", "noise in the lead-in"):
        assert word in design[design.index("## 8"):], word


# ---- compilation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every fixed-grid solver compile for gfx950 and spill nothing
    (VGPRs printed; recorded in DESIGN.md)."""
    header = tmp_path / "sde.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "static_assert(has_diffusion<VIHDS_GEN_CORE>::value && cond_tail<VIHDS_GEN_CORE>() == 2);",
             "static_assert(!has_diffusion<PrprConstant>::value && !has_diffusion<WithPrec<PrprConstant>>::value && cond_tail<PrprConstant>() == 0);"]
    for solver in SM.FIXED:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, %s, false>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "sde"), "_ZN5vihds")
    assert len(usage) == 15, sorted(usage)
    for solver in SM.FIXED:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d" % (cls.__name__, solver, min(fwd), max(fwd), bwd[0]))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


# ---- the host part of csrc/vihds_sde.hpp in a stand-alone program under sanitizers -----------------------------------------------
PROGRAM = r"""
// prints: per solver id the step length for (t0, t1, h0) = (0.5, 0.75, 0.125); the step indices of a grid of 3 intervals with 4
// sub-steps, written into a heap array of exactly 12 entries (an index outside it is a heap overflow); block, lane and counter
// of species 0 .. 7; key words from floats
#include <cstdio>
#include <memory>
#include "vihds_sde.hpp"
using namespace vihds;
int main() {
  for (int solver = 0; solver < 5; ++solver) std::printf("h %d %.9g\n", solver, (double)sde_step_length(solver, 0.5f, 0.75f, 0.125f));
  const int T = 4, MS = 4;
  std::unique_ptr<int[]> seen(new int[(T - 1) * MS]);
  for (int q = 0; q < (T - 1) * MS; ++q) seen[q] = 0;
  for (int k = 0; k < T - 1; ++k)
    for (int j = 0; j < MS; ++j) seen[sde_step_index(k, MS, j)] += 1;
  for (int q = 0; q < (T - 1) * MS; ++q) std::printf("step %d %d\n", q, seen[q]);
  std::printf("single %u %u\n", sde_step_index(0, 1, 0), sde_step_index(7, 1, 0));
  for (int s = 0; s < 8; ++s) {
    const SdeCounter c = sde_counter(1234u, s, 11u);
    std::printf("species %d %u %d %u %u %u %u\n", s, sde_block(s), sde_lane(s), c.c0, c.c1, c.c2, c.c3);
  }
  std::printf("drawn %d %d %d %d\n", (int)sde_block_drawn(0x3u, 0), (int)sde_block_drawn(0x3u, 1), (int)sde_block_drawn(0x30u, 0),
              (int)sde_block_drawn(0x30u, 1));
  const float words[] = {0.f, 1.f, 16777215.f, 16777216.f, -3.f, 2.75f};
  for (float w : words) std::printf("key %u\n", sde_key_word(w));
  return 0;
}
"""


def _host_compiler():
    return shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_the_header_in_a_host_program_under_sanitizers(tmp_path):
    src, exe = tmp_path / "sde_host.cpp", tmp_path / "sde_host"
    src.write_text(PROGRAM)
    subprocess.check_call([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    h = {int(l.split()[1]): float(l.split()[2]) for l in out if l.startswith("h ")}
    assert h == {hip.SOLVERS["modeuler"]: 0.125, hip.SOLVERS["modeulerwhile"]: 0.25, hip.SOLVERS["euler"]: 0.25,
                 hip.SOLVERS["midpoint"]: 0.25, hip.SOLVERS["rk4"]: 0.25}
    steps = [l.split() for l in out if l.startswith("step ")]
    assert [int(s[1]) for s in steps] == list(range(12)) and all(int(s[2]) == 1 for s in steps)  # each index once: k * m + j
    assert [l for l in out if l.startswith("single ")] == ["single 0 7"]
    species = [[int(v) for v in l.split()[1:]] for l in out if l.startswith("species ")]
    for s, (q, block, lane, c0, c1, c2, c3) in enumerate(species):
        (r0, r1, r2, r3), rl = sde_ref.counter(1234, s, 11)
        assert (q, block, lane, c0, c1, c2, c3) == (s, s >> 2, s & 3, r0, r1, r2, r3) and lane == rl
    assert len(species) == 8 and [l for l in out if l.startswith("drawn ")] == ["drawn 1 0 0 1"]
    assert [int(l.split()[1]) for l in out if l.startswith("key ")] == [0, 1, 16777215, 16777215, 0, 2]
