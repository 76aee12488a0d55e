"""The size and capability queries of the C ABI -- pure host code, nothing is launched and no GPU is needed -- for every
case of test_launch_modes.CASES (every built-in model, the lane `_precisions` models with a hidden layer, one registered
generated model, one sized dr_blackbox side library), over every solver id, kernel_variant 0 / 1 and three shapes, against
the table recorded in tests/golden/problem_query_table.json.  (90, 200, 5) is 18 000 trajectories: above the lane-split
limit that vihds_ode_bwd_reduces_weights and the summaries query switch on.

Three more dr_blackbox problems pin how a size set is resolved, with return codes and messages: the built-in network sizes
with another latent width (a side library is looked for, the built-in kernels do not match), a size set nobody built, and
an n_const that does not cover the treatments and the device one-hot.

Record the table (against the library the table is to pin):  python tests/test_problem_queries.py --out <file>"""
import ctypes
import json
import os
import re
import sys
from functools import lru_cache

import pytest

if __name__ == "__main__":  # the recorder runs outside pytest: the paths tests/conftest.py sets up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "vi-hds_amd"), os.path.join(_ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import test_launch_modes as LM  # noqa: E402  (its CASES and the problem descriptor of each)
from fixture_util import GOLDEN  # noqa: E402

TABLE_FILE = os.path.join(GOLDEN, "problem_query_table.json")
SHAPES = ((2, 3, 5), (36, 200, 86), (90, 200, 5))
SOLVER_IDS = tuple(range(9))
VARIANTS = (0, 1)
# one column of a table row each, in this order
QUERIES = ("vihds_model_n_weights", "vihds_ode_bwd_aux_floats", "vihds_ode_bwd_reduces_weights", "vihds_problem_n_states",
           "vihds_problem_n_slots", "vihds_problem_dump_fields", "vihds_blackbox_gram_on_chip",
           "vihds_blackbox_tail_offset_floats", "vihds_ode_fwd_summaries_supported",
           "vihds_ode_fwd_summaries_workspace_floats", "vihds_ode_adaptive_workspace_floats",
           "vihds_ode_adaptive_tape_floats")
# the queries that resolve a dr_blackbox size set (the extra problems call these)
BLACKBOX_QUERIES = ("vihds_model_n_weights", "vihds_ode_bwd_aux_floats", "vihds_problem_n_states", "vihds_problem_n_slots",
                    "vihds_problem_dump_fields", "vihds_blackbox_gram_on_chip", "vihds_blackbox_tail_offset_floats")


def _query(L, name, pp):
    if name == "vihds_ode_adaptive_tape_floats":
        return int(L.vihds_ode_adaptive_tape_floats(pp, LM.MAX_STEPS))
    return int(getattr(L, name)(pp))


def case_table(case):
    from vihds import hip

    L = hip.lib()
    out = {"queries": {}}
    for variant in VARIANTS:
        spec, _, _ = LM._spec(case, variant, "rk4")
        for B, S, T in SHAPES:
            rows = out["queries"].setdefault("B %d S %d T %d" % (B, S, T), {})
            for solver in SOLVER_IDS:
                prob = spec.bind(B, S, T)
                prob.solver = solver
                rows["kernel_variant %d / solver %d" % (variant, solver)] = [_query(L, q, ctypes.byref(prob)) for q in QUERIES]
    m = spec.proto.model
    n_slots = int(L.vihds_model_n_slots(m))
    out["model"] = {"n_states": int(L.vihds_model_n_states(m)), "n_species": int(L.vihds_model_n_species(m)), "n_slots": n_slots,
                    "slot_names": [L.vihds_model_slot_name(m, s).decode() for s in range(n_slots)]}
    return out


def _extra_problems():
    spec, _, _ = LM._spec("dr_blackbox", 0, "rk4")
    C, D = spec.proto.C, spec.proto.D
    out = {}
    for name, (n_latent, n_hidden, n_hidden_prec, n_const) in (
            ("built-in network sizes, 11 latent inputs", (2, 25, 20, 11 + C + D)),
            ("4_7_3_9: no library built", (4, 7, 3, 9 + C + D)),
            ("n_const below C + D", (2, 25, 20, C + D - 1))):
        prob = spec.bind(2, 3, 5)
        prob.n_latent_states, prob.n_hidden_states, prob.n_hidden_prec, prob.n_const = n_latent, n_hidden, n_hidden_prec, n_const
        out[name] = prob
    return out


def extra_table():
    from vihds import hip

    L = hip.lib()
    out = {}
    for name, prob in _extra_problems().items():
        out[name] = {}
        for q in BLACKBOX_QUERIES:
            L.vihds_rng_advance(None, None)  # (leaves "null rng" in the sticky error string: a query without a message shows as that)
            rc = _query(L, q, ctypes.byref(prob))
            out[name][q] = {"rc": rc, "error": L.vihds_last_error().decode()}
    return out


@lru_cache(maxsize=None)
def _golden():
    with open(TABLE_FILE) as f:
        return json.load(f)


def test_the_table_covers_every_case_and_query():
    assert _golden()["queries"] == list(QUERIES)
    assert sorted(_golden()["cases"]) == sorted(LM.CASES)
    for case in _golden()["cases"].values():
        assert sorted(case["queries"]) == sorted("B %d S %d T %d" % s for s in SHAPES)
        for rows in case["queries"].values():
            assert len(rows) == len(VARIANTS) * len(SOLVER_IDS)


@pytest.mark.parametrize("case", sorted(LM.CASES))
def test_queries_match_the_recorded_table(case):
    got = json.loads(json.dumps(case_table(case)))
    want = _golden()["cases"][case]
    assert got["model"] == want["model"]
    for shape in sorted(want["queries"]):
        for key in sorted(want["queries"][shape]):
            g, w = got["queries"].get(shape, {}).get(key), want["queries"][shape][key]
            assert g == w, "%s, %s, %s: %s" % (case, shape, key, [(q, a, b) for q, a, b in zip(QUERIES, g or (), w) if a != b])
    assert got == want


def test_blackbox_size_sets_resolve_as_recorded():
    assert json.loads(json.dumps(extra_table())) == _golden()["dr_blackbox problems"]


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    table = {"queries": list(QUERIES), "cases": {c: case_table(c) for c in sorted(LM.CASES)},
             "dr_blackbox problems": extra_table()}
    text = json.dumps(table, indent=1, sort_keys=True)
    text = re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text)  # (one row per line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("wrote %s" % args.out)
