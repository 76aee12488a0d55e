"""Forward / adjoint launch times of a generated model with missing observations under a fully observed mask against its
unmasked twin, B=36, S=200, T=86 -- the measurement of tests/probe/modelgen_forcing_timing.py (HIP events around back-to-back
launches, the two routes alternating over several rounds, one line per solver and launch kind) for two routes that differ in the
mask words of their rows of cond and in the selects at the scoring point:
  unmasked twin        PrprRestated (tests/modelgen_models.py): cond [B, 0], C = 0
  fully observed mask  PrprMasked (tests/modelgen_missing_models.py): masked_obs<> -- T mask words per data row (all 15), staged
                       in LDS by the forward (nb x T more floats) and requested one point ahead by the adjoint, one word decode and
                       four pairs of selects per time point; cond [B, T], C = T
    python tests/probe/modelgen_missing_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_missing_models as XM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
LABELS = ("unmasked twin", "fully observed mask")


def measure(a, solver):
    routes = (("plain", XM.TWIN[XM.PrprMasked]), ("masked", XM.PrprMasked))
    for _, cls in routes:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(routes[0][1].model_key)
    assert hip.model_slots(XM.PrprMasked.model_key) == slots  # (the same theta rows through both routes)
    row_of = {n: i for i, n in enumerate(slots)}
    theta, _treatment, times, obs = AB.problem(slots)
    conds = {"plain": torch.zeros((B, 1), device=DEV), "masked": torch.full((B, T), 15.0, device=DEV)}
    widths = {"plain": 0, "masked": T}
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls in routes:
        cond = conds[route]
        prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=widths[route]).bind(B, S, T)
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

        launches[route] = {"fwd": fwd, "bwd": bwd, "logp": logp, "g_theta": g_theta}
        for name in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(launches[route][name](), name)
    torch.cuda.synchronize()
    # the two routes compute the same thing: under a fully observed mask every select takes the read and the term
    worst = float(((launches["masked"]["logp"] - launches["plain"]["logp"]).abs()
                   / launches["plain"]["logp"].abs().clamp_min(1.0)).max())
    worst_g = float(((launches["masked"]["g_theta"] - launches["plain"]["g_theta"]).abs()
                     / launches["plain"]["g_theta"].abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)).max())
    print("%s: log-likelihood of the two routes agrees to %.1e, g_theta to %.1e" % (solver, worst, worst_g))
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
        f, o = sorted(res[("plain", name)]), sorted(res[("masked", name)])
        fm, om = f[len(f) // 2], o[len(o) // 2]
        print("%s %s: %s %.1f us (%.1f .. %.1f), %s %.1f us (%.1f .. %.1f), ratio of medians %.3f, masked - twin %.1f us per launch "
              "[%d rounds x %d launches]" % (solver, name, LABELS[0], fm, f[0], f[-1], LABELS[1], om, o[0], o[-1], om / fm, om - fm,
                                             a.rounds, a.reps))


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
