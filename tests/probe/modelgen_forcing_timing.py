"""Forward / adjoint launch times of a generated model with a forcing against the same model with that input as a constant
treatment, B=36, S=200, T=86 -- the measurement of tests/probe/modelgen_ab_timing.py (its inputs, HIP events around
back-to-back launches, the two routes alternating over several rounds, one line per solver and launch kind) for two routes
that differ in their rows of cond, which that probe's cases do not:
  constant treatment   PrprTreated (tests/modelgen_forcing_models.py): YFP production scaled by c[0] = 1.5 -- one more
                       effective parameter that prepare copies; cond [B, 1], C = 1
  forcing              PrprForced: the same input as a forcing whose T samples are all 1.5 (n_forcings<> = 1: the samples
                       staged in LDS by the forward and requested one interval ahead by the adjoint, set_interval -- a
                       subtraction, a reciprocal and a multiply -- and set_point per interval, one subtraction and one FMA
                       per rhs evaluation); cond [B, T] (samples are used raw), C = T
    python tests/probe/modelgen_forcing_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_forcing_models as FM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
DRIVE = 1.5
LABELS = ("constant treatment", "forcing")


def measure(a, solver):
    routes = (("treated", FM.PrprTreated), ("forced", FM.PrprForced))
    for _, cls in routes:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(FM.PrprTreated.model_key)
    assert hip.model_slots(FM.PrprForced.model_key) == slots  # (the same theta rows through both routes)
    row_of = {n: i for i, n in enumerate(slots)}
    theta, treatment, times, obs = AB.problem(slots, DRIVE)
    conds = {"treated": treatment, "forced": torch.full((B, T), DRIVE, device=DEV)}
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls in routes:
        cond = conds[route]
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        traj = torch.empty((T, len(cls.species), B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
        g_theta = torch.zeros_like(theta)

        def fwd(prob=prob, cond=cond, traj=traj, xpred=xpred, logp=logp):
            return L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

        def bwd(prob=prob, cond=cond, traj=traj, g_logp=g_logp, g_theta=g_theta):
            return L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), None, None, g_logp.data_ptr(),
                                   g_theta.data_ptr(), None, None, st)

        launches[route] = {"fwd": fwd, "bwd": bwd, "logp": logp}
        for name in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[route][name](), name)
    torch.cuda.synchronize()
    # the two routes compute the same thing: the interpolant of a constant series is that constant
    worst = float(((launches["forced"]["logp"] - launches["treated"]["logp"]).abs()
                   / launches["treated"]["logp"].abs().clamp_min(1.0)).max())
    print("%s: log-likelihood of the two routes agrees to %.1e" % (solver, worst))
    res = {}
    for _ in range(a.rounds):
        for name in ("fwd", "bwd"):
            for route, _cls in routes:
                fn = launches[route][name]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((route, name), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    for name in ("fwd", "bwd"):
        f, o = sorted(res[("treated", name)]), sorted(res[("forced", name)])
        print("%s %s: %s %.1f us (%.1f .. %.1f), %s %.1f us (%.1f .. %.1f), ratio of medians %.3f  [%d rounds x %d launches]"
              % (solver, name, LABELS[0], f[len(f) // 2], f[0], f[-1], LABELS[1], o[len(o) // 2], o[0], o[-1],
                 o[len(o) // 2] / f[len(f) // 2], a.rounds, a.reps))


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
