"""Forward / adjoint launch times of a generated model with a delayed read against the same model with that read as a constant
treatment, B=36, S=200, T=86 -- the measurement of tests/probe/modelgen_forcing_timing.py (HIP events around back-to-back
launches, the routes alternating over several rounds, one line per solver and launch kind):
  constant treatment   DelayedRepressorTreated (tests/modelgen_delay_models.py): the repressor's production reads c[0] -- a class
                       without `delays`, so its code objects are what the kernel headers gave before delays existed
  delayed read         DelayedRepressor, tau = the theta row (0.5 .. 1.5 time units = 2 .. 6 steps of the grid): per interval
                       two lookups into the stored trajectory (a cursor walk over the times, two loads of the species, a
                       division and an FMA each) and set_delay; in the adjoint also two scatters into the history adjoint (read-
                       modify-write of two floats each), one load of A[.][k] per point, and the column's zeroing (T stores) up front
  delayed read, past   the same kernels with every tau = 100 (above the span): the lookups return the constant history without a
                       load of the trajectory and the scatters add to A[.][0] alone -- what is left is the walk, the branches and
                       the column
The difference between the last two is what the history loads and the two-point scatters cost.
    python tests/probe/modelgen_delay_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_delay_models as DM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
ROUTES = (("treated", DM.DelayedRepressorTreated, "constant treatment"), ("delayed", DM.DelayedRepressor, "delayed read"),
          ("past", DM.DelayedRepressor, "delayed read, past"))


def measure(a, solver):
    for _, cls, _label in ROUTES:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(DM.DelayedRepressor.model_key)
    assert hip.model_slots(DM.DelayedRepressorTreated.model_key) == slots  # (the same theta rows through every route)
    row_of = {n: i for i, n in enumerate(slots)}
    theta, treatment, times, obs = AB.problem(slots, 0.3)
    theta_past = theta.clone()
    theta_past[row_of["tau"]] = 100.0
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls, _label in ROUTES:
        th = theta_past if route == "past" else theta
        cond = treatment if route == "treated" else torch.empty((B, 0), device=DEV)
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        n_aux = int(L.vihds_ode_bwd_aux_floats(ctypes.byref(prob)))
        assert n_aux == (T * B * S if cls.delays else 0)
        aux = torch.empty(max(n_aux, 1), device=DEV)
        traj = torch.empty((T, len(cls.species), B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
        g_theta = torch.zeros_like(theta)
        cond_ptr = cond.data_ptr() if cond.shape[1] else None

        def fwd(prob=prob, th=th, cond_ptr=cond_ptr, traj=traj, xpred=xpred, logp=logp):
            return L.vihds_ode_fwd(ctypes.byref(prob), th.data_ptr(), cond_ptr, None, times.data_ptr(), obs.data_ptr(), None,
                                   traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

        def bwd(prob=prob, th=th, cond_ptr=cond_ptr, traj=traj, g_logp=g_logp, g_theta=g_theta, aux=aux, n_aux=n_aux):
            return L.vihds_ode_bwd(ctypes.byref(prob), th.data_ptr(), cond_ptr, None, times.data_ptr(), obs.data_ptr(), None,
                                   traj.data_ptr(), None, None, g_logp.data_ptr(), g_theta.data_ptr(), None,
                                   aux.data_ptr() if n_aux else None, st)

        launches[route] = {"fwd": fwd, "bwd": bwd, "logp": logp, "g_theta": g_theta}
        for name in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[route][name](), name)
    torch.cuda.synchronize()
    for route in launches:
        assert bool(torch.isfinite(launches[route]["logp"]).all()) and bool(torch.isfinite(launches[route]["g_theta"]).all()), route
    res = {}
    for _ in range(a.rounds):
        for name in ("fwd", "bwd"):
            for route, _cls, _label in ROUTES:
                fn = launches[route][name]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((route, name), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    for name in ("fwd", "bwd"):
        med = {}
        parts = []
        for route, _cls, label in ROUTES:
            v = sorted(res[(route, name)])
            med[route] = v[len(v) // 2]
            parts.append("%s %.1f us (%.1f .. %.1f)" % (label, med[route], v[0], v[-1]))
        print("%s %s: %s  [%d rounds x %d launches]" % (solver, name, ", ".join(parts), a.rounds, a.reps))
        print("%s %s: delayed - treated %.1f us per launch = %.0f ns per interval; of it the history loads%s %.1f us, the rest "
              "(cursor walk, branches%s) %.1f us" % (
                  solver, name, med["delayed"] - med["treated"], 1000.0 * (med["delayed"] - med["treated"]) / (T - 1),
                  " and two-point scatters" if name == "bwd" else "", med["delayed"] - med["past"],
                  ", the column's zeroing, A[.][k] loads" if name == "bwd" else "", med["past"] - med["treated"]))


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
