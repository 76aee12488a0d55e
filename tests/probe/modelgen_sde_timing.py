"""Forward / adjoint launch times of a generated model with process noise against its noise-free twin, B=36, S=200, T=86 -- the
measurement of tests/probe/modelgen_delay_timing.py (HIP events around back-to-back launches, the routes alternating over several
rounds, one line per solver and launch kind):
  noise-free twin   PrprRestated (tests/modelgen_models.py): a class without `diffusion`, so its code objects are what the kernel
                    headers gave before the hook existed
  process noise     PrprLangevin (tests/modelgen_sde_models.py): the twin plus sigma sqrt(max(y, 0)) on OD and RFP.  Both noisy
                    species sit in the first block of four: per step one Philox4x32-10 evaluation (ten rounds) and two
                    Box-Muller pairs, of which two normals are used, the two amplitudes and two FMAs; in the adjoint the same
                    draws again, diffusion_vjp and N additions
The ratio to the twin is what ten Philox rounds and a Box-Muller pair per four species and step cost next to the rhs evaluations
of the scheme (two for midpoint, four for rk4; twice as many again in the adjoint).
    python tests/probe/modelgen_sde_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_models as MM  # noqa: E402
import modelgen_sde_models as SM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
ROUTES = (("twin", MM.PrprRestated, "noise-free twin"), ("noisy", SM.PrprLangevin, "process noise"))


def measure(a, solver):
    for _, cls, _label in ROUTES:
        modelgen.register_kernel(cls, False)
    twin_slots = hip.model_slots(MM.PrprRestated.model_key)
    theta, _treatment, times, obs = AB.problem(twin_slots)
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls, _label in ROUTES:
        slots = hip.model_slots(cls.model_key)
        row_of = {n: i for i, n in enumerate(slots)}
        # the twin's theta rows through both routes; sigma = 0.05 for the noisy one
        th = torch.stack([theta[twin_slots.index(n)] if n in twin_slots else torch.full((B, S), 0.05, device=DEV) for n in slots]).contiguous()
        cond = torch.tensor([[12345.0, 678.0]], device=DEV).expand(B, 2).contiguous() if route == "noisy" else torch.empty((B, 0), device=DEV)
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        assert int(L.vihds_ode_bwd_aux_floats(ctypes.byref(prob))) == 0  # (nothing is stored for the backward pass)
        traj = torch.empty((T, len(cls.species), B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
        g_theta = torch.zeros_like(th)
        cond_ptr = cond.data_ptr() if cond.shape[1] else None

        def fwd(prob=prob, th=th, cond_ptr=cond_ptr, traj=traj, xpred=xpred, logp=logp):
            return L.vihds_ode_fwd(ctypes.byref(prob), th.data_ptr(), cond_ptr, None, times.data_ptr(), obs.data_ptr(), None,
                                   traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

        def bwd(prob=prob, th=th, cond_ptr=cond_ptr, traj=traj, g_logp=g_logp, g_theta=g_theta):
            return L.vihds_ode_bwd(ctypes.byref(prob), th.data_ptr(), cond_ptr, None, times.data_ptr(), obs.data_ptr(), None,
                                   traj.data_ptr(), None, None, g_logp.data_ptr(), g_theta.data_ptr(), None, None, st)

        launches[route] = {"fwd": fwd, "bwd": bwd, "logp": logp, "g_theta": g_theta, "keep": (th, cond)}
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
        med, parts = {}, []
        for route, _cls, label in ROUTES:
            v = sorted(res[(route, name)])
            med[route] = v[len(v) // 2]
            parts.append("%s %.1f us (%.1f .. %.1f)" % (label, med[route], v[0], v[-1]))
        print("%s %s: %s  [%d rounds x %d launches]" % (solver, name, ", ".join(parts), a.rounds, a.reps))
        print("%s %s: noisy / twin %.3f; noisy - twin %.1f us per launch = %.0f ns per step" % (
            solver, name, med["noisy"] / med["twin"], med["noisy"] - med["twin"], 1000.0 * (med["noisy"] - med["twin"]) / (T - 1)))


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
