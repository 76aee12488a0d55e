"""CPU tests of the missing observations of vihds.modelgen (missing_observations = True, the batch key "observed"): definition
errors and refusals by their message, the generated text and its digests (and the unchanged text of every class without the
attribute), the layout of a row of cond and the word encoding, the float64 definition of the scoring rule and the host paths that
restate it, fill_unobserved, load_csv with blank cells and `merge: union`, the batch plumbing, the documents, compilation for
gfx950 without scratch, and csrc/vihds_mask.hpp in a stand-alone program under the address and undefined-behaviour sanitizers."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vihds import datasets, hip, modelgen as G, ode, ops, training
from vihds.utils import attrify

import modelgen_missing_models as XM
import modelgen_models as MM
from test_modelgen_host import _compile_usage, _define, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-hds_amd", "csrc")
F64 = torch.float64
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
GOLDEN = os.path.join(ROOT, "tests", "golden", "modelgen_missing_source_sha256.json")
# the modules whose PREBUILT lists existed before the attribute
EARLIER_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                   "modelgen_likelihood_models", "modelgen_piecewise_models", "modelgen_forcing_models", "modelgen_implicit_models",
                   "modelgen_substep_models", "modelgen_jump_models", "modelgen_leadin_models", "modelgen_sdirk_models",
                   "modelgen_algebraic_models", "modelgen_delay_models", "modelgen_sde_models")
T9 = len(XM.TIMES)


def _config(solver, n_conditions):
    return SimpleNamespace(device="cpu", params=attrify({"solver": solver, "n_hidden_decoder_precisions": 0}),
                           data=SimpleNamespace(device_depth=1, conditions=["c%d" % k for k in range(n_conditions)],
                                                relevance_vectors={}, default_devices=[]))


# ---- definition and refusals ------------------------------------------------------------------------------------------------------
def test_the_attribute_is_a_bool():
    assert G.GeneratedOdeModel.missing_observations is False
    assert _define("missing_ok", missing_observations=True).missing_observations is True
    assert _define("missing_off", missing_observations=False).missing_observations is False
    for bad in (1, 0, "yes", None, [True]):
        with pytest.raises(G.ModelDefinitionError, match=r"missing_observations = .*it is True or False"):
            _define("missing_bad", missing_observations=bad)


def test_bad_masks_raise_on_the_host():
    good = XM.gaps_mask()
    for ok in (good, good.float(), good.double().numpy(), good.int().tolist()):
        m = G.observed_mask(ok, 3, T9)
        assert m.dtype == torch.float32 and torch.equal(m.bool(), good)
    for value in (0.5, 2.0, -1.0, float("nan"), float("inf")):
        bad = good.float()
        bad[1, 2, 3] = value
        with pytest.raises(ValueError, match="must hold 0 / 1"):
            G.observed_mask(bad, 3, T9)
    for shape in ((3, T9), (3, 3, T9), (3, 4, T9 - 1), (2, 4, T9), (3, 4, T9, 1)):
        with pytest.raises(ValueError, match=r"'observed' must be \[3 rows, 4 signals, 9 time points\]"):
            G.observed_mask(torch.ones(shape), 3, T9)
    # ... from the batch plumbing too, before anything is uploaded
    item = {"devices": 0, "dev_1hot": torch.ones(1), "inputs": torch.zeros(1), "observations": torch.zeros(4, T9),
            "observed": torch.full((4, T9), 0.5)}
    with pytest.raises(ValueError, match="must hold 0 / 1"):
        training.collate_merged(torch.tensor(XM.TIMES), "cpu", [item])


def test_host_checks_run_before_anything_is_built(monkeypatch):
    """An adaptive solver and a wrong cond width raise from solve, ahead of the library build and of every launch; a spec of a
    registered masked model declines the adaptive solvers by name."""
    def no_build(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(G, "register_kernel", no_build)
    times = torch.tensor(XM.TIMES)
    for cls in XM.MODELS:
        K, C = len(cls.forcings), int(cls.n_conditions)
        width = C + (K + 1) * T9 + (2 if cls._diffusion_def is not None else 0)
        for solver in sorted(hip.ADAPTIVE_SOLVERS):
            model = cls(_config(solver, C))
            with pytest.raises(NotImplementedError, match="adaptive solver '%s'" % solver):
                model.solve(_config(solver, C), times, None, torch.zeros(3, width), None)
        model = cls(_config("rk4", C))
        assert model.cond_width(T9) == width
        with pytest.raises(ValueError, match=r"its %d mask words behind them.*\(width %d\)" % (T9, width - 1)):
            model.solve(_config("rk4", C), times, None, torch.zeros(3, width - 1), None)
        with pytest.raises(RuntimeError, match="number of time points"):
            model.cond_width()
    monkeypatch.setattr(hip, "GENERATED_MASKED", {"gen_registered_masked"})
    monkeypatch.setitem(hip.MODELS, "gen_registered_masked", 1 << 20)
    for solver in sorted(hip.ADAPTIVE_SOLVERS):
        with pytest.raises(NotImplementedError, match=r"has missing observations \(missing_observations = True\).*adaptive solver '%s'" % solver):
            ops.OdeProblemSpec("gen_registered_masked", solver, {}, 0, C=9)


def _batch(B=3, observed=None, **more):
    d = {"inputs": torch.zeros(B, 0), "observations": torch.zeros(B, 4, T9), "times": torch.tensor(XM.TIMES)}
    if observed is not None:
        d["observed"] = observed
    d.update(more)
    return attrify(d)


def test_a_model_without_the_attribute_refuses_the_key():
    mask = XM.gaps_mask().float()
    builtin = ode.OdeModel.__new__(ode.OdeModel)
    with pytest.raises(RuntimeError, match="carries 'observed'.*OdeModel is not a generated model with missing_observations = True"):
        ode.OdeModel.row_inputs(builtin, _batch(observed=mask))
    plain = MM.PrprRestated(_config("rk4", 0))
    with pytest.raises(RuntimeError, match="carries 'observed'.*PrprRestated does not set missing_observations = True"):
        plain.row_inputs(_batch(observed=mask))
    b = _batch()
    assert plain.row_inputs(b) is b.inputs and ode.OdeModel.row_inputs(builtin, b) is b.inputs  # (today's path without the key)
    with pytest.raises(RuntimeError, match="carries 'observed'"):
        training.log_prob_observations(SimpleNamespace(decoder=SimpleNamespace(ode_model=plain)), torch.ones(3, 2, 4, T9),
                                       torch.ones(3, 4, T9), torch.ones(3, 2, 4, 1), observed=mask)
    with pytest.raises(RuntimeError, match="carries 'observed'"):
        XM.ReaderStudentForced.torch_log_likelihood(torch.ones(3, 2, 4, T9), torch.ones(3, 4, T9), torch.ones(3, 2, 4, T9), {}, None,
                                                    observed=mask)


# ---- generated text ---------------------------------------------------------------------------------------------------------------
def test_generated_text_of_a_masked_class():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted("%s:%d" % (c.__name__, int(n)) for c, n in XM.PREBUILT)
    line = "  static constexpr bool MASKED_OBS = true;"
    for cls, neural in XM.PREBUILT:
        src = G.generate_source(cls, neural)
        assert src == G.generate_source(cls, neural)  # deterministic
        assert hashlib.sha256(src.encode()).hexdigest() == recorded["%s:%d" % (cls.__name__, int(neural))], cls.__name__
        assert src.count(line) == (1 if cls.missing_observations else 0) and src.count("MASKED_OBS") == src.count(line)
    # the attribute adds that one line and nothing else (the key and the struct's name apart)
    for cls, twin in ((XM.ReaderStudentForcedMasked, XM.ReaderStudentForced), (XM.PrprDilutedSub2Masked, XM.PrprDilutedSub2)):
        a, b = G.generate_source(cls).splitlines(), G.generate_source(twin).splitlines()
        extra = [l for l in a if l.startswith(line)]
        a.remove(extra[0])
        same = [x for x, y in zip(a, b) if x == y]
        assert len(a) == len(b) and len(extra) == 1 and len(same) >= len(a) - 4


def test_classes_without_the_attribute_generate_the_recorded_text():
    recorded = set()
    for name in sorted(os.listdir(os.path.join(ROOT, "tests", "golden"))):
        if name.startswith("modelgen") and "sha256" in name and name.endswith(".json") and name != os.path.basename(GOLDEN):
            with open(os.path.join(ROOT, "tests", "golden", name)) as f:
                stack = [json.load(f)]
            while stack:  # (a file may group its digests)
                for v in stack.pop().values():
                    if isinstance(v, dict):
                        stack.append(v)
                    else:
                        recorded.add(v)
    seen = 0
    for m in EARLIER_MODULES:
        for cls, neural in importlib.import_module(m).PREBUILT:
            text = G.generate_source(cls, neural)
            assert "MASKED_OBS" not in text, cls.__name__
            assert hashlib.sha256(text.encode()).hexdigest() in recorded, "%s.%s:%d" % (m, cls.__name__, int(neural))
            seen += 1
    assert seen == 75


# ---- the layout of a row of cond --------------------------------------------------------------------------------------------------
def test_all_sixteen_words_round_trip():
    flags = torch.tensor([[(w >> j) & 1 for w in range(16)] for j in range(4)], dtype=torch.float32)[None]  # [1, 4, 16]
    words = G.mask_words(flags)
    assert words.dtype == torch.float32 and words.tolist() == [[float(w) for w in range(16)]]
    assert torch.equal(G.mask_bits(words), flags.bool())
    assert torch.equal(words.double(), XM.words_of(flags.bool()))
    g = XM.gaps_mask()
    assert torch.equal(G.mask_bits(G.mask_words(g.float())), g) and G.mask_words(g.float())[0].tolist() == [15.0] * T9


def test_the_mask_of_the_tests():
    """Row 0 fully observed, row 1 a fixed pattern, row 2 with its three gaps; every (row, signal) other than the deliberately
    empty one keeps at least two observed points; NaN under half of the masked entries and 1e30 under the rest."""
    m = XM.gaps_mask()
    assert m.shape == (3, 4, T9) and bool(m[0].all()) and not bool(m[1].all()) and torch.equal(m, XM.gaps_mask())
    assert not bool(m[2, 2].any()) and not bool(m[2, :, T9 - 3:].any()) and not bool(m[2, 0, 0]) and bool(m[2, 1, 0])
    counts = m.sum(-1)
    for b in range(3):
        for j in range(4):
            assert (int(counts[b, j]) == 0) if (b, j) == XM.EMPTY else (int(counts[b, j]) >= 2), (b, j)
    pb = XM.problem(XM.PrprMasked, 3, 5)
    under = pb["obs"][~m]
    assert int(torch.isnan(under).sum()) == (under.numel() + 1) // 2 and int((under == 1e30).sum()) == under.numel() // 2
    assert torch.equal(pb["obs"][m], pb["clean"][m]) and bool(torch.isfinite(pb["clean"]).all())


def test_row_inputs_and_cond_width():
    """[n_conditions treatments | K x T samples | T mask words | key lo, key hi], for every class of the tests."""
    B = 3
    mask = XM.gaps_mask()
    for cls in XM.MODELS:
        K, C = len(cls.forcings), int(cls.n_conditions)
        model = cls(_config("rk4", C))
        model.eval()
        series = XM.series_of(cls, B, torch.tensor(XM.TIMES, dtype=F64)).float()
        more = {"forcings": series} if K else {}
        if cls._diffusion_def is not None:
            more["noise_key"] = XM.KEY
        inputs = 0.1 * torch.arange(B * C, dtype=torch.float32).reshape(B, C)
        for given in (mask, mask.float()):
            wide = model.row_inputs(_batch(observed=given, inputs=inputs, **more))
            assert wide.shape == (B, model.cond_width(T9)) and wide.dtype == torch.float32
            o = C
            assert torch.equal(wide[:, :o], inputs)
            assert torch.equal(wide[:, o:o + K * T9].reshape(B, K, T9), series)
            o += K * T9
            assert torch.equal(wide[:, o:o + T9].double(), XM.words_of(mask))
            o += T9
            if cls._diffusion_def is not None:
                assert wide[:, o:].tolist() == [[float(XM.KEY[0]), float(XM.KEY[1])]] * B
                o += 2
            assert o == wide.shape[1]
            # ... which is the row the tests' own cond_of builds
            assert torch.equal(wide.double(), XM.cond_of(cls, torch.expm1(inputs.double()), series.double(), mask).float().double())
        # without the key every point counts as observed
        full = model.row_inputs(_batch(inputs=inputs, **more))
        assert full.shape == wide.shape and full[:, C + K * T9:C + (K + 1) * T9].tolist() == [[15.0] * T9] * B
        with pytest.raises(ValueError, match="'observed' must be"):
            model.row_inputs(_batch(observed=mask[:2], inputs=inputs, **more))
        with pytest.raises(ValueError, match="must hold 0 / 1"):
            model.row_inputs(_batch(observed=2.0 * mask.float(), inputs=inputs, **more))


def test_batches_carry_the_mask():
    mask = XM.gaps_mask()
    items = [{"devices": 0, "dev_1hot": torch.ones(1), "inputs": torch.full((1,), 0.1 * b), "observations": torch.zeros(4, T9),
              "observed": mask[b]} for b in range(3)]
    batch = training.collate_merged(torch.tensor(XM.TIMES), "cpu", items)
    assert batch.observed.dtype == torch.float32 and torch.equal(batch.observed.bool(), mask) and batch.observed.is_contiguous()
    plain = training.collate_merged(torch.tensor(XM.TIMES), "cpu", [{k: v for k, v in it.items() if k != "observed"} for it in items])
    assert "observed" not in plain and sorted(plain) == ["dev_1hot", "devices", "inputs", "observations", "times"]
    d = training.batch_to_device(torch.tensor(XM.TIMES), "cpu", {"dev_1hot": torch.ones(3, 1), "inputs": torch.zeros(3, 1),
                                                                 "observations": torch.zeros(3, 4, T9), "observed": mask.numpy()})
    assert torch.equal(d.observed, mask.float())


# ---- the float64 definition ---------------------------------------------------------------------------------------------------------
def _logp(cls, pb, obs, observed, grad=False):
    th = {n: v.detach().clone().requires_grad_(grad) for n, v in pb["th"].items()}
    W = {k: v.clone() for k, v in pb["prec_w"].items()} if pb["prec_w"] else None
    cond = XM.cond_of(cls, pb["treatments"], pb["series"], observed)
    _, _, logp = XM.forward(cls, th, cond, pb["times"], "rk4", obs, observed, pb["xi"], W)
    return logp, th


@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_the_float64_definition(cls):
    pb = XM.problem(cls, 3, 5)
    m = pb["observed"]
    with torch.no_grad():
        logp, _ = _logp(cls, pb, pb["obs"], m)
        assert bool(torch.isfinite(logp).all())
        # a fully masked signal: exactly 0.0
        assert torch.equal(logp[XM.EMPTY[0], :, XM.EMPTY[1]], torch.zeros(5, dtype=F64))
        # changing the placeholders changes nothing
        for kinds in ((1e30, float("nan")), (0.0, 0.0), (float("inf"), -7.0)):
            other, _ = _logp(cls, pb, XM.with_placeholders(pb["clean"], m, kinds), m)
            assert torch.equal(other, logp), kinds
        # a masked entry contributes exactly 0.0: masking one more entry removes exactly its own term
        b, j, k = 1, 0, int(torch.nonzero(m[1, 0])[0, 0])
        less = m.clone()
        less[b, j, k] = False
        one_less, _ = _logp(cls, pb, pb["obs"], less)
        full, xp, _ = XM.forward(cls, pb["th"], pb["cond"], pb["times"], "rk4", xi=pb["xi"], prec_w=pb["prec_w"])
        keep = torch.ones(3, 4, dtype=torch.bool)
        keep[b, j] = False
        assert torch.equal(one_less[keep[:, None].expand(3, 5, 4)], logp[keep[:, None].expand(3, 5, 4)])
        assert bool((one_less[b, :, j] != logp[b, :, j]).all())
        # a fully observed mask is the unmasked definition of the twin, exactly
        twin = XM.TWIN[cls]
        ones = torch.ones_like(m)
        masked_full, _ = _logp(cls, pb, pb["clean"], ones)
        twin_full, _ = _logp(twin, pb, pb["clean"], None)
        assert torch.equal(masked_full, twin_full)
    # autograd gradients are finite with NaN placeholders, and a never-observed signal's constant precision has none
    logp, th = _logp(cls, pb, XM.with_placeholders(pb["clean"], m, (float("nan"), float("nan"))), m, grad=True)
    (logp * pb["G"]["logp"]).sum().backward()
    for n, v in th.items():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), n
    if "prec_yfp" in th:
        assert torch.equal(th["prec_yfp"].grad[XM.EMPTY[0]], torch.zeros(5, dtype=F64)) and bool((th["prec_yfp"].grad[0] != 0).all())


def test_the_host_paths_restate_the_rule():
    """training.log_prob_observations (the Gaussian and a model's own density) and torch_log_likelihood against the tests' own
    three-line statement: bit for bit in float64."""
    pb = XM.problem(XM.PrprMasked, 3, 5)
    m = pb["observed"]
    with torch.no_grad():
        full, xp, want = XM.forward(XM.PrprMasked, pb["th"], pb["cond"], pb["times"], "rk4", pb["obs"], m)
        prec = torch.stack([pb["th"][n] for n in XM.PREC], dim=2)[:, :, :, None]
        model = SimpleNamespace(decoder=SimpleNamespace(ode_model=XM.PrprMasked(_config("rk4", 0))))
        got = training.log_prob_observations(model, xp, pb["obs"], prec, observed=m)
        assert torch.equal(got, want)
        assert torch.equal(training.log_prob_observations(model, xp, pb["obs"], prec, observed=m.float()), want)
        # without the mask: today's expression (NaN under the placeholders, as before)
        plain = training.log_prob_observations(model, xp, pb["clean"], prec)
        assert torch.equal(plain, torch.sum(training.log_prob_gaussian(pb["clean"][:, None], xp, prec), 3))
        # a model's own density
        cls = XM.ReaderStudentForcedMasked
        pr = XM.problem(cls, 3, 5)
        _, xq, want_t = XM.forward(cls, pr["th"], pr["cond"], pr["times"], "rk4", pr["obs"], pr["observed"])
        prec_t = cls.torch_precision(XM.states(cls, pr["th"], pr["cond"], pr["times"], "rk4"), pr["th"], pr["cond"])
        terms = cls.torch_log_likelihood(xq, pr["obs"], prec_t, pr["th"], pr["cond"], observed=pr["observed"])
        assert torch.equal(terms.sum(3), want_t) and bool((terms[~pr["observed"][:, None].expand(terms.shape)] == 0.0).all())
        twin_terms = XM.ReaderStudentForced.torch_log_likelihood(
            xq, pr["clean"], prec_t, pr["th"], XM.cond_of(XM.ReaderStudentForced, pr["treatments"], pr["series"]))
        sel = pr["observed"][:, None].expand(terms.shape)
        assert torch.equal(terms[sel], twin_terms[sel])


# ---- the dataset ------------------------------------------------------------------------------------------------------------------
def test_fill_unobserved():
    times = np.array([0.0, 1.0, 3.0, 4.0, 8.0], dtype=np.float32)
    obs = np.zeros((2, 4, 5), dtype=np.float32)
    seen = np.ones((2, 4, 5), dtype=bool)
    obs[0, 0] = [1.0, np.nan, 7.0, 1e30, 5.0]       # interior: one gap between 0 and 3, one between 3 and 8
    seen[0, 0] = [True, False, True, False, True]
    obs[0, 1] = [np.nan, np.nan, 2.0, 4.0, np.nan]  # both ends: the nearest observed value
    seen[0, 1] = [False, False, True, True, False]
    obs[0, 2] = np.nan                              # an empty signal
    seen[0, 2] = False
    obs[1, 3] = [3.0, 2.0, 1.0, 0.5, 0.25]
    out = datasets.fill_unobserved(times, obs, seen)
    assert out.dtype == np.float32 and np.isfinite(out).all() and out is not obs
    np.testing.assert_allclose(out[0, 0], [1.0, 3.0, 7.0, 6.6, 5.0], rtol=1e-6)
    assert out[0, 1].tolist() == [2.0, 2.0, 2.0, 4.0, 4.0] and out[0, 2].tolist() == [0.0] * 5
    assert np.array_equal(out[seen], obs[seen]) and np.array_equal(out[1], obs[1])
    # fully observed input is returned unchanged
    whole = np.arange(40, dtype=np.float32).reshape(2, 4, 5)
    assert datasets.fill_unobserved(times, whole, np.ones_like(whole, dtype=bool)) is whole


SIGNALS = ["OD", "mRFP1", "EYFP", "ECFP"]


def _write_plate(path, times, rows):
    """A plate-reader file in the loader's layout: five leading columns, then one reading column per signal and time; the first
    row holds the time of every reading column.  rows: [(device, condition text, {signal: [cells]})]."""
    cols = ["Device", "a", "b", "c", "Condition"] + ["Raw Data (%s) %d" % (s, k) for s in SIGNALS for k in range(len(times))]
    lines = [",".join(cols), ",".join(["", "", "", "", ""] + [repr(float(t)) for _s in SIGNALS for t in times])]
    for dev, cond, cells in rows:
        lines.append(",".join([dev, "", "", "", cond] + [str(v) for s in SIGNALS for v in cells[s]]))
    path.write_text("\n".join(lines) + "\n")


def _settings(tmp_path, files, **more):
    return attrify(dict(data_dir=str(tmp_path), files=files, devices=["D1"], device_map={"D1": 0}, conditions=["C6"],
                        signals=SIGNALS, normalize=None, subtract_background=True, device_idx_to_device_name=["D1"],
                        component_maps={"g": {"D1": 0}}, **more))


def _two_plates(tmp_path):
    """Two files of different length with one shared time (1.0); the first has a blank and a 'nan' cell."""
    ta, tb = [0.0, 1.0, 2.0, 3.0], [0.5, 1.0, 2.5]
    a = {s: [1.0 + k + 0.1 * j for k in range(4)] for j, s in enumerate(SIGNALS)}
    a["OD"][2] = ""
    a["EYFP"][0] = "nan"
    b = {s: [2.0 + k + 0.1 * j for k in range(3)] for j, s in enumerate(SIGNALS)}
    _write_plate(tmp_path / "a.csv", ta, [("D1", "C6=5", a), ("D1", "C6=1", {s: [3.0 + k for k in range(4)] for s in SIGNALS})])
    _write_plate(tmp_path / "b.csv", tb, [("D1", "C6=2", b)])
    return ta, tb


def test_load_csv_takes_blank_cells(tmp_path):
    ta, _ = _two_plates(tmp_path)
    devices, treatments, times, obs = datasets.load_csv("a.csv", _settings(tmp_path, ["a.csv"]))
    assert times.tolist() == ta and obs.shape == (2, 4, 4) and obs.dtype == np.float32 and treatments.tolist() == [[5.0], [1.0]]
    gone = np.zeros((2, 4, 4), dtype=bool)
    gone[0, 0, 2] = gone[0, 2, 0] = True
    assert np.array_equal(np.isnan(obs), gone) and obs[0, 0].tolist()[:2] == [1.0, 2.0] and obs[0, 1, 2] == np.float32(3.1)
    # the dataset keeps the mask and hands the encoder nothing that is not finite
    ds = datasets.TimeSeriesDataset(_settings(tmp_path, ["a.csv"]), None)
    ds.init_single("a.csv")
    assert torch.equal(ds.observed.bool(), torch.from_numpy(~gone)) and bool(torch.isfinite(ds.observations).all())
    item = ds[0]
    assert sorted(item) == ["dev_1hot", "devices", "inputs", "observations", "observed"] and item["observed"].shape == (4, 4)
    delta = training._delta_obs(ds.observations)
    assert bool(torch.isfinite(delta).all())
    # a complete file: no mask, today's items
    ds2 = datasets.TimeSeriesDataset(_settings(tmp_path, ["b.csv"]), None)
    ds2.init_single("b.csv")
    assert ds2.observed is None and sorted(ds2[0]) == ["dev_1hot", "devices", "inputs", "observations"]


def test_merge_union(tmp_path):
    ta, tb = _two_plates(tmp_path)
    loaded = [datasets.load_csv(f, _settings(tmp_path, [])) for f in ("a.csv", "b.csv")]
    times_list, obs_list = [l[2] for l in loaded], [l[3] for l in loaded]
    # the default merge is what it was: the shortest file's grid by nearest time
    chosen, merged = datasets.merge_observations(list(times_list), list(obs_list))
    assert chosen.tolist() == tb and merged.shape == (3, 4, 3)
    assert np.array_equal(merged[2], obs_list[1][0]) and merged[1, 0].tolist() == [3.0, 4.0, 5.0]  # (nearest of 0.5: 0.0; of 2.5: 2.0)
    same, merged2 = datasets.merge_observations(list(times_list), list(obs_list), True, 0.0)
    assert same.tolist() == tb and np.array_equal(np.isnan(merged), np.isnan(merged2))
    # the union: sorted, the shared time once, every file observed at its own points only
    union, wide = datasets.merge_observations(list(times_list), list(obs_list), "union")
    assert union.tolist() == [0.0, 0.5, 1.0, 2.0, 2.5, 3.0] and wide.shape == (3, 4, 6)
    at_a, at_b = [0, 2, 3, 5], [1, 2, 4]
    seen = ~np.isnan(wide)
    assert seen[1].all(axis=0).tolist() == [k in at_a for k in range(6)] and seen[2].all(axis=0).tolist() == [k in at_b for k in range(6)]
    assert not seen[2][:, [0, 3, 5]].any() and np.array_equal(wide[1][:, at_a], obs_list[0][1]) and np.array_equal(wide[2][:, at_b], obs_list[1][0])
    assert not seen[0, 0, 3] and not seen[0, 2, 0]  # (the file's own blank cells stay unobserved)
    # times within the tolerance are one point
    near, wide2 = datasets.merge_observations([np.array([0.0, 1.0], np.float32), np.array([0.02, 1.01, 2.0], np.float32)],
                                              [np.ones((1, 4, 2), np.float32), 2 * np.ones((1, 4, 3), np.float32)], "union", 0.05)
    assert near.tolist() == [0.0, 1.0, 2.0] and not np.isnan(wide2[:, :, :2]).any() and np.isnan(wide2[0, :, 2]).all()
    exact, _ = datasets.merge_observations([np.array([0.0, 1.0], np.float32), np.array([0.02, 1.0], np.float32)],
                                           [np.ones((1, 4, 2), np.float32), np.ones((1, 4, 2), np.float32)], "union")
    assert [round(float(t), 2) for t in exact] == [0.0, 0.02, 1.0]
    # through the dataset: the spec's data block says merge: union
    ds = datasets.TimeSeriesDataset(_settings(tmp_path, ["a.csv", "b.csv"], merge="union", merge_tolerance=0.0), None)
    ds.init_multiple_merge()
    assert ds.times.tolist() == union.tolist() and ds.observed.shape == (3, 4, 6) and torch.equal(ds.observed.bool(), torch.from_numpy(seen))
    assert bool(torch.isfinite(ds.observations).all()) and "observed" in ds[2]
    ds0 = datasets.TimeSeriesDataset(_settings(tmp_path, ["a.csv", "b.csv"], merge=True), None)
    ds0.init_multiple_merge()
    assert ds0.times.tolist() == tb


# ---- documents --------------------------------------------------------------------------------------------------------------------
def test_the_documents_have_the_paragraph():
    for word in ("Missing observations.", "missing_observations = True", "'observed'", "MASKED_OBS", "mask words", "2^j",
                 "fill_unobserved", "merge: union", "adaptive", "An encoder that reads the mask"):
        assert word in G.__doc__, word
    read = lambda name: open(os.path.join(ROOT, name)).read()  # noqa: E731
    assert "missing_observations" in read("README.md")
    for name in ("INTEGRATION.md", "DESIGN.md"):
        text = read(name)
        assert "missing_observations" in text and "vihds_mask.hpp" in text and "mask words" in text, name
    design = read("DESIGN.md")
    open_items = " ".join(design[design.index("## 8"):].split())  # (line breaks apart)
    for word in ("time-parallel decoder", "an encoder that reads the mask", "per-row time grids without a union grid",
                 "skipping integration steps", "adaptive solvers for masked models"):
        assert word in open_items, word


# ---- compilation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("cls", XM.MODELS, ids=lambda c: c.__name__)
def test_kernels_compile_without_scratch(tmp_path, cls):
    """The staged and the unstaged forward and the adjoint of every fixed-grid solver compile for gfx950 and spill nothing (VGPRs
    printed; recorded in profiles/LOG.md).  The class under NeuralPrecisions is instantiated as WithPrec<>, which forwards the
    trait, with the adjoint's dump form beside the plain one."""
    neural = cls in XM.NEURAL
    header = tmp_path / "missing.hpp"
    header.write_text(G.generate_source(cls, neural))
    model = "WithPrec<VIHDS_GEN_CORE>" if neural else "VIHDS_GEN_CORE"
    tail = 2 if cls._diffusion_def is not None else 0
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "vihds_gen_model.hpp"', '#include "%s"' % header, "namespace vihds {",
             "using MaskedM = %s;" % model,
             "static_assert(masked_obs<MaskedM>::value && masked_obs<VIHDS_GEN_CORE>::value);",
             "static_assert(cond_tail<MaskedM>() == %d && cond_mask_words<MaskedM>(9) == 9);" % tail,
             "static_assert(!masked_obs<PrprConstant>::value && !masked_obs<WithPrec<PrprConstant>>::value && "
             "cond_mask_words<PrprConstant>(9) == 0);"]
    for solver in XM.FIXED:
        name = "VIHDS_SOLVER_" + solver.upper()
        lines += ["template __global__ void ode_fwd_kernel<MaskedM, %s, true>(OdeArgs);" % name,
                  "template __global__ void ode_fwd_kernel<MaskedM, %s, false>(OdeArgs);" % name,
                  "template __global__ void ode_bwd_kernel<MaskedM, %s, false>(OdeArgs);" % name]
        if neural:
            lines += ["template __global__ void ode_bwd_kernel<MaskedM, %s, true>(OdeArgs);" % name]
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines + ["}"]) + "\n", "missing"), "_ZN5vihds")
    assert len(usage) == (20 if neural else 15), sorted(usage)
    for solver in XM.FIXED:
        tag = "Li%dELb" % hip.SOLVERS[solver]
        fwd = [v for n, (v, _) in usage.items() if "ode_fwd_kernel" in n and tag in n]
        bwd = [v for n, (v, _) in usage.items() if "ode_bwd_kernel" in n and tag in n]
        print("%s %s: forward %d .. %d VGPRs, adjoint %d .. %d" % (cls.__name__, solver, min(fwd), max(fwd), min(bwd), max(bwd)))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name


# ---- csrc/vihds_mask.hpp in a stand-alone program under sanitizers ------------------------------------------------------------------
PROGRAM = r"""
// prints: for every word 0 .. 15 and a few values no host writes, the four flags; the selects on a NaN placeholder, written into
// a heap array of exactly 16 x 4 entries (an index outside it is a heap overflow); the words of all sixteen flag sets
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include "vihds_mask.hpp"
using namespace vihds;
int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  std::unique_ptr<float[]> out(new float[16 * kMaskSignals]);
  for (int w = 0; w < 16; ++w) {
    const ObsMask m((float)w);
    std::printf("word %d %d%d%d%d\n", w, (int)m.observed(0), (int)m.observed(1), (int)m.observed(2), (int)m.observed(3));
    for (int j = 0; j < kMaskSignals; ++j) out[w * kMaskSignals + j] = m.gate(j, m.read(j, nan, 2.f + j) - (2.f + j) + 1.f);
  }
  for (int q = 0; q < 16 * kMaskSignals; ++q) std::printf("sel %d %.9g\n", q, (double)out[q]);
  const float odd[] = {nan, inf, -inf, -1.f, 16.f, 1e30f, 3.75f, -0.f};
  for (float w : odd) {
    const ObsMask m(w);
    std::printf("odd %d\n", m.bits);
  }
  const ObsMask all;
  std::printf("default %d\n", all.bits);
  for (int w = 0; w < 16; ++w) std::printf("enc %d %.9g\n", w, (double)mask_word(w & 1, w & 2, w & 4, w & 8));
  const ObsMask half(5.f);
  std::printf("read %.9g %.9g gate %.9g %.9g\n", (double)half.read(0, 7.f, nan), (double)half.read(1, inf, 3.f), (double)half.gate(2, 9.f),
              (double)half.gate(3, nan));
  return 0;
}
"""


def _host_compiler():
    return shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler")
def test_the_header_in_a_host_program_under_sanitizers(tmp_path):
    src, exe = tmp_path / "mask_host.cpp", tmp_path / "mask_host"
    src.write_text(PROGRAM)
    subprocess.check_call([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    words = {int(l.split()[1]): l.split()[2] for l in out if l.startswith("word ")}
    assert words == {w: "".join(str((w >> j) & 1) for j in range(4)) for w in range(16)}
    sel = [float(l.split()[2]) for l in out if l.startswith("sel ")]
    # observed: the NaN read enters (NaN); unobserved: the predicted signal stands in and the gate gives exactly 0
    assert len(sel) == 64
    for w in range(16):
        for j in range(4):
            v = sel[w * 4 + j]
            assert np.isnan(v) if (w >> j) & 1 else (v == 0.0 and not np.signbit(v)), (w, j, v)
    assert [int(l.split()[1]) for l in out if l.startswith("odd ")] == [0, 0, 0, 0, 0, 0, 3, 0]
    assert [l for l in out if l.startswith("default ")] == ["default 15"]
    assert [float(l.split()[2]) for l in out if l.startswith("enc ")] == [float(w) for w in range(16)]
    assert [l for l in out if l.startswith("read ")] == ["read 7 3 gate 9 0"]
