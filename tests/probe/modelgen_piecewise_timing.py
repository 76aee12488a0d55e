"""Forward / adjoint launch times of a right-hand side with a switch (the same thread-per-trajectory kernel template): the
prpr_constant restatement vs its subclass PrprDosed, whose YFP production is multiplied by where(t < c[0], 0, 1) -- one
comparison and one select per rhs evaluation, one more select in rhs_vjp, one more effective parameter (the treatment).  The
switch time is 10 of the 20 hours, so half of the steps run on either side.  B=36, S=200, T=86, midpoint and rk4.  HIP events
around back-to-back launches, the two routes alternating over several rounds; prints one line per solver and launch kind.
    python tests/probe/modelgen_piecewise_timing.py [--reps 200] [--rounds 5]"""
import argparse
import ctypes
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "vi-hds_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_models as MM  # noqa: E402
import modelgen_piecewise_models as PM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solvers", default="midpoint,rk4")
    a = ap.parse_args()
    for solver in a.solvers.split(","):
        measure(a, solver)


def measure(a, solver):
    B, S, T, dev = 36, 200, 86, "cuda:0"
    routes = (("fixed", MM.PrprRestated), ("own", PM.PrprDosed))
    for _, cls in routes:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(MM.PrprRestated.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    assert hip.model_slots(PM.PrprDosed.model_key) == slots  # (the same theta rows through both routes)
    gen = torch.Generator(device=dev).manual_seed(0)
    theta = 0.5 + torch.rand((len(slots), B, S), device=dev, generator=gen)
    cond = torch.full((B, 1), math.log1p(10.0), device=dev)  # (c[0] = 10: the inducer is added half way)
    times = torch.linspace(0.0, 20.0, T, device=dev)
    obs = torch.rand((B, 4, T), device=dev, generator=gen)
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls in routes:
        spec = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=1)
        prob = spec.bind(B, S, T)
        N = spec.n_states
        traj = torch.empty((T, N, B, S), device=dev)
        xpred = torch.empty((T, 4, B, S), device=dev)
        logp = torch.empty((4, B, S), device=dev)
        g_logp = torch.ones((4, B, S), device=dev)
        g_theta = torch.zeros_like(theta)

        def fwd(prob=prob, traj=traj, xpred=xpred, logp=logp):
            return L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

        def bwd(prob=prob, traj=traj, g_logp=g_logp, g_theta=g_theta):
            return L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),
                                   obs.data_ptr(), None, traj.data_ptr(), None, None, g_logp.data_ptr(),
                                   g_theta.data_ptr(), None, None, st)

        launches[route] = {"fwd": fwd, "bwd": bwd}
        for name in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[route][name](), name)
    torch.cuda.synchronize()
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
        f, o = sorted(res[("fixed", name)]), sorted(res[("own", name)])
        print("%s %s: PrprRestated %.1f us (%.1f .. %.1f), PrprDosed %.1f us (%.1f .. %.1f), ratio of medians %.3f  [%d rounds x %d launches]"
              % (solver, name, f[len(f) // 2], f[0], f[-1], o[len(o) // 2], o[0], o[-1], o[len(o) // 2] / f[len(f) // 2],
                 a.rounds, a.reps))


if __name__ == "__main__":
    main()
