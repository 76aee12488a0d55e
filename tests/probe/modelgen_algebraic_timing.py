"""Forward / adjoint launch times of a generated model with an algebraic variable against its closed-form twin: BindingQss (six
Newton iterations on one unknown inside every rhs / observe evaluation, the mu step in both adjoints) and BindingClosed (one
sqrt, plain reverse mode) of tests/modelgen_algebraic_models.py compute the same model, so the difference is the price of the
iteration.  Competing (two unknowns, eight iterations, a dense 2 x 2 solve; no closed form exists) is timed alone.  B=36, S=200,
T=86 -- the inputs and the measurement of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, the
variants alternating over several rounds in one process, one line per solver and launch kind).  There is no threshold: the
ratios are findings.
    python tests/probe/modelgen_algebraic_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_algebraic_models as AM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
VARIANTS = (("qss", AM.BindingQss), ("closed", AM.BindingClosed), ("competing", AM.Competing))


def measure(a, solver):
    L, st = hip.lib(), hip.current_stream()
    launches = {}
    for key, cls in VARIANTS:
        modelgen.register_kernel(cls, False)
        slots = hip.model_slots(cls.model_key)
        row_of = {n: i for i, n in enumerate(slots)}
        theta, cond, times, obs = AB.problem(slots)
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        traj = torch.empty((T, len(cls.species), B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
        g_theta = torch.zeros_like(theta)
        keep = (theta, cond, times, obs, xpred, logp, g_logp, g_theta)

        def fwd(prob=prob, k=keep, traj=traj):
            return L.vihds_ode_fwd(ctypes.byref(prob), k[0].data_ptr(), k[1].data_ptr(), None, k[2].data_ptr(), k[3].data_ptr(),
                                   None, traj.data_ptr(), k[4].data_ptr(), k[5].data_ptr(), st)

        def bwd(prob=prob, k=keep, traj=traj):
            return L.vihds_ode_bwd(ctypes.byref(prob), k[0].data_ptr(), k[1].data_ptr(), None, k[2].data_ptr(), k[3].data_ptr(),
                                   None, traj.data_ptr(), None, None, k[6].data_ptr(), k[7].data_ptr(), None, None, st)

        launches[key] = {"fwd": fwd, "bwd": bwd, "traj": traj, "g": g_theta}
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[key][kind](), kind)
    torch.cuda.synchronize()
    print("%s: finite share of trajectory / theta gradient %s; largest |qss - closed| on the trajectory %.2e" % (
        solver, ", ".join("%s %.3f / %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean()),
                                             float(torch.isfinite(v["g"]).float().mean())) for k, v in launches.items()),
        float((launches["qss"]["traj"] - launches["closed"]["traj"]).abs().max())))
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
        print("%s %s: %s  [qss / closed %.2f; %d rounds x %d launches]" % (
            solver, kind, ", ".join("%s %.1f us (%.1f .. %.1f)" % (k, mid[k], v[0], v[-1]) for k, v in med.items()),
            mid["qss"] / mid["closed"], a.rounds, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solvers", default="midpoint,rk4")
    a = ap.parse_args()
    for solver in a.solvers.split(","):
        measure(a, solver)


if __name__ == "__main__":
    main()
