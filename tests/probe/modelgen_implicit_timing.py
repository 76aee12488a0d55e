"""Forward / adjoint launch times of the backward-Euler solver ("beuler": NEWTON = 4 Newton iterations per step, each a
right-hand side, a generated Jacobian and an unpivoted elimination in registers; the adjoint one Jacobian, one transposed
solve and one rhs_vjp per step) against rk4 and midpoint for the same class, B=36, S=200, T=86 -- the inputs and the
measurement of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, the solvers alternating over
several rounds in one process, one line per class and launch kind):
  PrprImplicit   6 species, 11 of 36 Jacobian entries structurally non-zero
  DrImplicit     8 species (the cap), 19 of 64
There is no threshold: this records what a Newton step costs in this kernel family.
    python tests/probe/modelgen_implicit_timing.py [--reps 200] [--rounds 5]"""
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

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
SOLVERS = ("beuler", "rk4", "midpoint")


def measure(a, cls):
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    theta, _, times, obs = AB.problem(slots)
    C = int(cls.n_conditions)
    cond = torch.full((B, max(C, 1)), math.log1p(0.5), device=DEV)
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for solver in SOLVERS:
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

        launches[solver] = {"fwd": fwd, "bwd": bwd, "traj": traj}
        for name in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[solver][name](), name)
    torch.cuda.synchronize()
    finite = {s: float(torch.isfinite(launches[s]["traj"]).float().mean()) for s in SOLVERS}
    print("%s: finite share of the trajectory %s" % (cls.__name__, ", ".join("%s %.3f" % kv for kv in finite.items())))
    res = {}
    for _ in range(a.rounds):
        for name in ("fwd", "bwd"):
            for solver in SOLVERS:
                fn = launches[solver][name]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((solver, name), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    for name in ("fwd", "bwd"):
        med = {s: sorted(res[(s, name)]) for s in SOLVERS}
        print("%s %s: %s  [beuler / rk4 %.2f, beuler / midpoint %.2f; %d rounds x %d launches]" % (
            cls.__name__, name, ", ".join("%s %.1f us (%.1f .. %.1f)" % (s, v[len(v) // 2], v[0], v[-1]) for s, v in med.items()),
            med["beuler"][len(med["beuler"]) // 2] / med["rk4"][len(med["rk4"]) // 2],
            med["beuler"][len(med["beuler"]) // 2] / med["midpoint"][len(med["midpoint"]) // 2], a.rounds, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for cls in (IM.PrprImplicit, IM.DrImplicit):
        measure(a, cls)


if __name__ == "__main__":
    main()
