"""CPU tests of the two tables of vihds.modelgen: the generated text of every model of the test suite is what it was before
the tables existed (its digest names the compiled library, so the kernels are the same files), and every record of the
operation table is complete and folds constants to what it evaluates on tensors."""
import hashlib
import importlib
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from vihds import modelgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_MODULES = ("modelgen_models", "modelgen_hybrid_models", "modelgen_observe_models", "modelgen_noise_models",
                 "modelgen_likelihood_models", "modelgen_piecewise_models")
NAN = float("nan")
POINTS = (-1.5, 0.0, 0.5, 1.0, 2.0, NAN)
BOUNDS = (0.0, 1.0)  # of clamp and cpass
# the arguments that are conditions (every other argument is a value)
CONDITION_ARGUMENTS = {"and": (0, 1), "or": (0, 1), "not": (0,), "where": (0,)}
SPACINGS = 4  # float64 spacings of the larger magnitude: 1 was measured (tanh, sqrt, erfc), the rest is for another libm


def test_every_recorded_source_digest_is_unchanged():
    """tests/golden/modelgen_source_sha256_all.json holds sha256(generate_source(cls, neural)), keyed module.Class:neural, of
    the (class, neural) pairs of every PREBUILT list and of the classes of modelgen_source_sha256.json, as the commit before
    the operation and hook tables produced them."""
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256_all.json")) as f:
        recorded = json.load(f)
    prebuilt = {"%s.%s:%d" % (m, cls.__name__, int(neural))
                for m in MODEL_MODULES for cls, neural in importlib.import_module(m).PREBUILT}
    assert len(prebuilt) == 22 and prebuilt <= set(recorded), sorted(prebuilt - set(recorded))
    assert "modelgen_models.EveryOperation:0" in recorded
    for key, digest in recorded.items():
        path, neural = key.split(":")
        module, name = path.split(".")
        text = G.generate_source(getattr(importlib.import_module(module), name), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key


def test_operations_are_the_public_records_and_module_attributes():
    assert G.OPERATIONS == tuple(r.name for r in G.OP_TABLE.values() if r.public)
    for name in G.OPERATIONS:
        assert getattr(G.op, name) is getattr(G, name) and callable(getattr(G, name)), name


@pytest.mark.parametrize("rec", list(G.OP_TABLE.values()), ids=lambda r: r.name)
def test_every_operation_record_is_complete_and_its_fold_agrees_with_its_torch_evaluation(rec):
    """The record has a fold, a torch evaluation, C spellings for the time loop and for prepare / init that take the node's
    arguments (and constants), and an adjoint rule -- none for conditions and pass nodes.  Then _fold on constants against
    evaluate on leaves in float64 at every combination of POINTS (conditions: both truth values): conditions agree exactly
    as bools, NaN and +-inf fall in the same places, finite values agree within SPACINGS float64 spacings."""
    assert G.OP_TABLE[rec.name] is rec and rec.arity >= 1 and rec.kind in ("value", "condition", "pass")
    assert callable(rec.fold) and callable(rec.torch) and callable(rec.number)
    assert len(rec.c) == 2 and all(isinstance(t, str) and t.count("%s") == rec.arity + (2 if rec.val else 0) for t in rec.c)
    assert rec.peephole is None or callable(rec.peephole)
    assert callable(rec.adjoint) if rec.kind == "value" else rec.adjoint is None

    g = G.Graph()
    is_condition = [i in CONDITION_ARGUMENTS.get(rec.name, ()) for i in range(rec.arity)]
    combos = list(itertools.product(*[(True, False) if c else POINTS for c in is_condition]))
    # a condition argument is the node y[i] < 0.5 on a leaf that holds 0 (true) or 1 (false)
    leaves = [g.leaf("y", i) for i in range(rec.arity)]
    args = [leaf < 0.5 if c else leaf for leaf, c in zip(leaves, is_condition)]
    val = BOUNDS if rec.val else None
    node = g._intern(rec.name, tuple(args), val)
    assert isinstance(node, G.Cond) == (rec.kind == "condition")
    env = {("y", i): torch.tensor([(0.0 if v else 1.0) if c else v for v in column], dtype=torch.float64)
           for i, (column, c) in enumerate(zip(zip(*combos), is_condition))}
    got = G.evaluate([node], env)[0]
    assert got.shape == (len(combos),) and got.dtype == (torch.bool if rec.kind == "condition" else torch.float64)
    worst = 0.0
    for point, e in zip(combos, got.tolist()):
        f = G._fold(rec.name, *point, val=val)
        if rec.kind == "condition":
            assert isinstance(f, bool) and isinstance(e, bool) and f is e, (rec.name, point, f, e)
            continue
        assert isinstance(f, float)
        if math.isnan(f) or math.isnan(e) or math.isinf(f) or math.isinf(e):
            assert (math.isnan(f) and math.isnan(e)) or f == e, (rec.name, point, f, e)
            continue
        spacings = abs(f - e) / float(np.spacing(max(abs(f), abs(e)))) if f != e else 0.0
        worst = max(worst, spacings)
        assert spacings <= SPACINGS, (rec.name, point, f, e, spacings)
    print("%s: %d points, fold vs evaluate worst %.1f spacings" % (rec.name, len(combos), worst))
