"""Forward / adjoint launch times of the two-stage SDIRK (`implicit_order = 2` under the solver "beuler": two stage solves of
NEWTON Newton iterations per step; the adjoint recomputes stage 1, then two Jacobians, two transposed solves and two rhs_vjp
per step) against what the same class had before it: backward Euler at m = 1 and with `substeps = 2`, and rk4.  B=36, S=200,
T=86 -- the inputs and the measurement of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, every
variant alternating over several rounds in one process, one line per class and launch kind):
  PrprImplicit   6 species, 11 of 36 Jacobian entries structurally non-zero
  DrImplicit     8 species (the cap), 19 of 64
There is no threshold: the ratios order 2 / order 1 are findings (expected before the measurement: forward about 2, adjoint
about one stage-1 recompute plus twice backward Euler's adjoint).
    python tests/probe/modelgen_sdirk_timing.py [--reps 200] [--rounds 5]"""
import argparse
import ctypes
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_implicit_models as IM  # noqa: E402
import modelgen_sdirk_models as DM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV


class PrprImplicitSub2(IM.PrprImplicit):
    model_key = "gen_prpr_constant_implicit_sub2"
    substeps = 2


class DrImplicitSub2(IM.DrImplicit):
    model_key = "gen_dr_constant_implicit_sub2"
    substeps = 2


# (the two Sub2 classes are the ones here that no test module builds: their libraries are compiled on the probe's first run)
CASES = (("PrprImplicit", (("sdirk2", DM.PrprSdirk, "beuler"), ("beuler m=1", IM.PrprImplicit, "beuler"),
                           ("beuler m=2", PrprImplicitSub2, "beuler"), ("rk4", IM.PrprImplicit, "rk4"))),
         ("DrImplicit", (("sdirk2", DM.DrSdirk, "beuler"), ("beuler m=1", IM.DrImplicit, "beuler"),
                         ("beuler m=2", DrImplicitSub2, "beuler"), ("rk4", IM.DrImplicit, "rk4"))))


def measure(a, name, variants):
    slots = None
    for _, cls, _ in variants:
        modelgen.register_kernel(cls, False)
        assert slots in (None, hip.model_slots(cls.model_key))  # (the same theta rows through every variant)
        slots = hip.model_slots(cls.model_key)
    assert hip.GENERATED_IMPLICIT_ORDER[variants[0][1].model_key] == 2 and hip.GENERATED_IMPLICIT_ORDER[variants[1][1].model_key] == 1
    row_of = {n: i for i, n in enumerate(slots)}
    theta, _, times, obs = AB.problem(slots)
    cond = torch.full((B, max(int(variants[0][1].n_conditions), 1)), math.log1p(0.5), device=DEV)
    L, st = hip.lib(), hip.current_stream()
    launches = {}
    for key, cls, solver in variants:
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        traj = torch.empty((T, len(cls.species), B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
        g_theta = torch.zeros_like(theta)

        def fwd(prob=prob, traj=traj, xpred=xpred, logp=logp):
            return L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

        def bwd(prob=prob, traj=traj, g_logp=g_logp, g_theta=g_theta):
            return L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), None, None, g_logp.data_ptr(),
                                   g_theta.data_ptr(), None, None, st)

        launches[key] = {"fwd": fwd, "bwd": bwd, "traj": traj}
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[key][kind](), kind)
    torch.cuda.synchronize()
    print("%s: finite share of the trajectory %s" % (name, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in launches.items())))
    res = {}
    for _ in range(a.rounds):
        for kind in ("fwd", "bwd"):
            for key, v in launches.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    v[kind]()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((key, kind), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    for kind in ("fwd", "bwd"):
        med = {k: sorted(res[(k, kind)]) for k in launches}
        mid = {k: v[len(v) // 2] for k, v in med.items()}
        print("%s %s: %s  [sdirk2 / beuler m=1 %.2f, sdirk2 / beuler m=2 %.2f, sdirk2 / rk4 %.2f; %d rounds x %d launches]" % (
            name, kind, ", ".join("%s %.1f us (%.1f .. %.1f)" % (k, mid[k], v[0], v[-1]) for k, v in med.items()),
            mid["sdirk2"] / mid["beuler m=1"], mid["sdirk2"] / mid["beuler m=2"], mid["sdirk2"] / mid["rk4"], a.rounds, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for name, variants in CASES:
        measure(a, name, variants)


if __name__ == "__main__":
    main()
