"""Forward / adjoint launch times of sub-stepped generated models (`substeps = m`: m steps of the scheme per observation
interval in one launch, the adjoint recomputing the interval's m - 1 intermediate states into LDS) against the only way to get
the same accuracy without them: the m = 1 class on the m-times refined grid (T' = (T - 1) m + 1 points, a forcing's samples
interpolated onto it), which does the same steps and stores, observes and scores m times as many points.  B=36, S=200, T=86 --
the inputs and the measurement of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, every variant
alternating over several rounds in one process):
  PrprForced    rk4      m = 1, 2, 4
  PrprImplicit  beuler   m = 1, 2, 4
There is no threshold: the ratio sub-stepped / refined is a finding.
    python tests/probe/modelgen_substeps_timing.py [--reps 200] [--rounds 5]"""
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
import modelgen_implicit_models as IM  # noqa: E402
import modelgen_substep_models as SM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV


class PrprImplicitSub2(IM.PrprImplicit):
    model_key = "gen_prpr_constant_implicit_sub2"
    substeps = 2


CASES = (("PrprForced", "rk4", {1: FM.PrprForced, 2: SM.PrprForcedSub2, 4: SM.PrprForcedSub4}),
         ("PrprImplicit", "beuler", {1: IM.PrprImplicit, 2: PrprImplicitSub2, 4: SM.PrprImplicitSub4}))
# (PrprImplicitSub2 is the one class here that no test module builds: its library is compiled on the probe's first run)


def _launches(cls, solver, theta, times, series, obs):
    """fwd / bwd closures of one class on one grid; series [B, K, len(times)] or None."""
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    Tg = times.shape[0]
    cond = series.reshape(B, -1).contiguous() if series is not None else torch.zeros((B, 1), device=DEV)
    prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, Tg)
    traj = torch.empty((Tg, len(cls.species), B, S), device=DEV)
    xpred = torch.empty((Tg, 4, B, S), device=DEV)
    logp = torch.empty((4, B, S), device=DEV)
    g_logp = torch.ones((4, B, S), device=DEV)
    g_theta = torch.zeros_like(theta)
    L, st = hip.lib(), hip.current_stream()

    def fwd():
        return L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(), obs.data_ptr(), None,
                               traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)

    def bwd():
        return L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(), obs.data_ptr(), None,
                               traj.data_ptr(), None, None, g_logp.data_ptr(), g_theta.data_ptr(), None, None, st)

    keep = (prob, cond, xpred, logp, g_logp, g_theta, times, obs)  # (alive as long as the closures)
    return {"fwd": fwd, "bwd": bwd, "traj": traj, "keep": keep}


def measure(a, name, solver, classes):
    slots = None
    variants = {}
    for m, cls in classes.items():
        modelgen.register_kernel(cls, False)
        assert slots in (None, hip.model_slots(cls.model_key))
        slots = hip.model_slots(cls.model_key)
    theta, _, times, obs = AB.problem(slots)
    forced = bool(classes[1].forcings)
    series = (1.0 + 0.5 * torch.sin(0.9 * times[None, :] + 0.7 * torch.arange(B, device=DEV)[:, None]))[:, None, :] if forced else None
    for m, cls in classes.items():
        variants["m=%d" % m] = _launches(cls, solver, theta, times, series, obs)
        if m > 1:  # the yardstick: the m = 1 class on the refined grid, observations and samples interpolated onto it
            fine = SM.refined(times.double().cpu(), m).float().to(DEV)
            k = torch.arange(fine.shape[0] - 1, device=DEV) // m
            w = torch.cat([(fine[:-1] - times[k]) / (times[k + 1] - times[k]), torch.zeros(1, device=DEV)])
            k = torch.cat([k, torch.tensor([T - 2], device=DEV)])
            w[-1] = 1.0
            lerp = lambda v: v[..., k] + w * (v[..., k + 1] - v[..., k])  # noqa: E731
            variants["refined x%d" % m] = _launches(classes[1], solver, theta, fine, lerp(series) if forced else None,
                                                    lerp(obs).contiguous())
    for v in variants.values():
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(v[kind](), kind)
    torch.cuda.synchronize()
    print("%s %s: finite share of the trajectory %s" % (name, solver, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in variants.items())))
    for m in classes:  # the sub-stepped launch computes the refined launch's states at the observation points
        if m > 1:
            d = (variants["m=%d" % m]["traj"] - variants["refined x%d" % m]["traj"][::m]).abs().max()
            print("%s %s m=%d: largest difference to the refined-grid launch at the observation points %.2e (largest value %.2f)"
                  % (name, solver, m, float(d), float(variants["m=%d" % m]["traj"].abs().max())))
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
        print("%s %s %s: %s" % (name, solver, kind, ", ".join(
            "m=%d / refined x%d %.2f, m=%d / m=1 %.2f" % (m, m, mid(("m=%d" % m, kind)) / mid(("refined x%d" % m, kind)), m,
                                                         mid(("m=%d" % m, kind)) / mid(("m=1", kind))) for m in classes if m > 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for name, solver, classes in CASES:
        measure(a, name, solver, classes)


if __name__ == "__main__":
    main()
