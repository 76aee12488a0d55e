"""Which launches a training step, an evaluation pass and a plain forward + cost + backward ask for, per model and switch:
the ordered list of C ABI entry points that queue work (the vihds_* entry points of include/vihds_hip.h whose prototype ends in
`void* stream`), against the table recorded in tests/golden/step_route_table.json.

A route is chosen by model, switch and purpose, never by size, so the tiny golden fixtures take every branch at their own
shapes.  A training case records three consecutive Training.step calls (a decline is remembered, and the sampling stage
moves into the forward launch, only from the second step on) and then one model() + cost() + backward() outside
Training.step; an evaluation case records one eager Training.evaluate at kernel_variant 1 (how a small batch reaches the
summaries-on-the-way form: vihds_ode_fwd_summaries_supported).  The calls are observed by replacing hip.lib for the
duration of a case with a proxy that notes the attribute name and returns the real function: what is listed is what the
host asked the library for.  An entry point that declines on the host before it queues anything is listed too (the
declined vihds_theta_ode_fwd in step 2 of gen_prpr_constant), so a decline that is remembered shows as a name that is gone
from the next step.

Record the table (on a GPU, against the tree the table is to pin):  python tests/test_step_routes.py --out <file>"""
import json
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # the recorder runs outside pytest: the paths tests/conftest.py sets up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "vi-hds_amd"), os.path.join(_ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from fixture_util import GOLDEN, Fixture  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE_FILE = os.path.join(GOLDEN, "step_route_table.json")
HEADER = os.path.join(os.path.dirname(GOLDEN), "..", "include", "vihds_hip.h")
N_STEPS = 3

# model -> (fixture, params of the model itself, switches turned off one at a time)
MODELS = {
    "dr_constant_icml_tiny_modeuler": ("dr_constant_icml_tiny_modeuler", {},
                                       ["fused_step_tail", "fused_iwae_backward", "fused_decoder_step", "fused_ode_training"]),
    "relay_constant_precisions_tiny_modeuler": ("relay_constant_precisions_tiny_modeuler", {},
                                                ["fused_theta_ode", "fused_step_tail", "inkernel_iwae", "lazy_x_predict"]),
    "dr_blackbox_icml_tiny_modeuler": ("dr_blackbox_icml_tiny_modeuler", {}, ["fused_theta_ode"]),
    "prpr_constant_tiny_modeuler": ("prpr_constant_tiny_modeuler", {}, []),
    "dr_constant_precisions_tiny_modeuler": ("dr_constant_precisions_tiny_modeuler", {}, []),
    "gen_prpr_constant": ("prpr_constant_tiny_modeuler", {}, []),
    "auto_constant_tiny_modeuler/dopri5": ("auto_constant_tiny_modeuler", {"solver": "dopri5"}, ["adaptive_device"]),
}


EVALUATION_SWITCHES = ("lazy_x_predict", "adaptive_device")  # (the others act on training steps only)


def _cases():
    out = {}
    for model, (_, _, switches) in MODELS.items():
        for off in [None] + switches:
            out["%s train %s" % (model, "defaults" if off is None else off + "=false")] = (model, "train", off)
        for off in [None, "online_summaries"] + [s for s in switches if s in EVALUATION_SWITCHES]:
            out["%s evaluate %s" % (model, "defaults" if off is None else off + "=false")] = (model, "evaluate", off)
    return out


CASES = _cases()


@lru_cache(maxsize=None)
def queueing_calls():
    """The entry points of the C ABI that queue work: the prototypes of include/vihds_hip.h that end in `void* stream`."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(vihds_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", header, flags=re.S)
    return frozenset(name for name, args in protos if re.search(r"void\s*\*\s*stream\s*$", args))


class _Noting(object):
    """Stands in for the loaded library: notes the queueing entry points asked for, hands out the real functions."""

    def __init__(self, real, calls):
        self._real, self._calls, self._queueing = real, calls, queueing_calls()

    def __getattr__(self, name):
        if name in self._queueing:
            self._calls.append(name)
        return getattr(self._real, name)


def _recorded(fn):
    """fn() with hip.lib replaced by the noting proxy; returns (fn's value, the calls noted)."""
    from vihds import hip

    calls, real_lib = [], hip.lib
    proxy = _Noting(real_lib(), calls)
    hip.lib = lambda: proxy
    try:
        out = fn()
    finally:
        hip.lib = real_lib
    return out, calls


def _build(model, purpose, off):
    import e2e_util as E
    import models
    from vihds.config import Config
    from vihds.parameters import Parameters
    from vihds.training import Training
    from vihds.vae import build_model

    fixture, over, _ = MODELS[model]
    over = dict(over, hip_graph=False, eval_graph=False)
    if off is not None:
        over[off] = False
    if purpose == "evaluate":
        over["kernel_variant"] = 1
    fx = Fixture(fixture)
    if model == "gen_prpr_constant":  # a registered generated model on the prpr fixture's data (tests/test_modelgen_gpu.py)
        import modelgen_models as MM

        spec = json.loads(str(fx.z["spec_json"]))
        spec["model"] = MM.PrprRestated.model_key
        spec["params"]["solver"] = fx.solver
        spec["params"].update(over)
        models.LOOKUP[MM.PrprRestated.model_key] = MM.PrprRestated
        args = E.make_args(fx.S, seed=fx.cfg["seed"], gpu=0)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        settings = Config(args=None, spec=spec)
        settings.device = torch.device("cuda:0")
        settings.seed = args.seed
        data = E._Pair(E._FakeDataset(fx), settings)
        parameters = Parameters(settings.params)
    else:
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, **over)
    model_ = build_model(args, settings, data, parameters)
    training = Training(args, settings, data, parameters, model_)
    return fx, args, model_, training, E.batch_from_fixture(fx, settings.device)


def run_case(case):
    """{phase: [call, ...]} of one case."""
    import models

    model, purpose, off = CASES[case]
    try:
        fx, args, net, training, batch = _build(model, purpose, off)
        np.random.seed(fx.cfg["seed"] + 1)
        torch.manual_seed(fx.cfg["seed"] + 1)
        out = {}
        if purpose == "evaluate":
            net.eval()
            _, out["evaluate"] = _recorded(lambda: training.evaluate(training.valid_data, args.test_samples))
        else:
            net.train()
            for k in range(N_STEPS):
                _, out["step %d" % (k + 1)] = _recorded(lambda: training.step(batch))
            assert training.optimizer.step_count() == N_STEPS

            def plain():
                results, theta, q, p = net(batch, args.train_samples)
                training.cost(batch, results, theta, q, p).elbo.backward()

            _, out["model, cost, backward"] = _recorded(plain)
            training.optimizer.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        return out
    finally:
        models.LOOKUP.pop("gen_prpr_constant", None)


def write_table(table, path):
    """One phase per line: call names only."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            " %s: {\n%s\n }" % (json.dumps(c), ",\n".join("  %s: %s" % (json.dumps(ph), json.dumps(table[c][ph]))
                                                           for ph in sorted(table[c])))
            for c in sorted(table)) + "\n}\n")


@lru_cache(maxsize=None)
def _golden():
    with open(TABLE_FILE) as f:
        return json.load(f)


def test_the_table_covers_every_case():
    assert sorted(_golden()) == sorted(CASES)


def test_the_queueing_calls_are_parsed_from_the_header():
    calls = queueing_calls()
    assert {"vihds_ode_fwd", "vihds_step_tail", "vihds_rng_advance", "vihds_adam_step"} <= calls
    assert not calls & {"vihds_step_tail_supported", "vihds_ode_fwd_summaries_supported", "vihds_last_error"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_step_routes_match_the_recorded_table(case):
    got = run_case(case)
    want = _golden()[case]
    for phase in sorted(set(got) | set(want)):
        print("%-70s %-22s %s" % (case, phase, " ".join(got.get(phase, ["-"]))))
    assert got == want


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    args_ = ap.parse_args()
    table = {}
    for c in sorted(CASES):
        table[c] = run_case(c)
        print(c, flush=True)
    write_table(table, args_.out)
    print("wrote %s" % args_.out)
