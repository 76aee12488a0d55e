"""Forward / adjoint launch times of generated models with steady species (`steady_species`, `steady_rate`: a fixed number of
pseudo-transient iterations once per trajectory before the first step, the adjoint repeating them and solving J^T mu = lam_E)
against the same model without the solve.  B=36, S=200, T=86, rk4 -- the inputs and the measurement of
tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, the variants alternating over several rounds in one
process):
  PrprSteadySolved (3 steady species, 9 iterations)   against PrprSteady, its closed-form twin: the cost of the solve
  ChainEight       (8 steady species, 12 iterations)  against ChainEightFree, the same class with steady_species = None
There is no threshold: the ratios are a finding.  A select chooses between the two residuals of the twin (where on the
treatment), so its arithmetic does not depend on the rows' treatments.
    python tests/probe/modelgen_steady_timing.py [--reps 200] [--rounds 5]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import modelgen_substeps_timing as ST  # noqa: E402
import torch  # noqa: E402

from vihds import hip, modelgen  # noqa: E402
import modelgen_leadin_models as LM  # noqa: E402
import modelgen_steady_models as SS  # noqa: E402

CASES = (("PrprSteadySolved", "rk4", SS.PrprSteadySolved, LM.PrprSteady, "closed form"),
         ("ChainEight", "rk4", SS.ChainEight, SS.ChainEightFree, "no solve"))


def measure(a, name, solver, solved, plain, label):
    for cls in (solved, plain):
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(solved.model_key)
    assert slots == hip.model_slots(plain.model_key)
    theta, _, times, obs = AB.problem(slots)
    variants = {"solve": ST._launches(solved, solver, theta, times, None, obs),
                label: ST._launches(plain, solver, theta, times, None, obs)}
    for v in variants.values():
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(v[kind](), kind)
    torch.cuda.synchronize()
    print("%s %s: finite share of the trajectory %s" % (name, solver, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in variants.items())))
    d = (variants["solve"]["traj"][0] - variants[label]["traj"][0]).abs().max()
    print("%s %s: largest difference of the first stored state to the launch with %s %.2e" % (name, solver, label, float(d)))
    res = {}
    for _ in range(a.rounds):
        for kind in ("fwd", "bwd"):
            for key, v in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    v[kind]()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((key, kind), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    med = {k: sorted(v) for k, v in res.items()}
    mid = lambda k: med[k][len(med[k]) // 2]  # noqa: E731
    for kind in ("fwd", "bwd"):
        print("%s %s %s: %s  [%d rounds x %d launches]" % (name, solver, kind, ", ".join(
            "%s %.1f us (%.1f .. %.1f)" % (key, mid((key, kind)), med[(key, kind)][0], med[(key, kind)][-1]) for key in variants),
            a.rounds, a.reps))
        print("%s %s %s: solve / %s %.2f" % (name, solver, kind, label, mid(("solve", kind)) / mid((label, kind))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for case in CASES:
        measure(a, *case)


if __name__ == "__main__":
    main()
