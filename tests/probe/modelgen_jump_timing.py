"""Forward / adjoint launch times of a generated model with a state jump (`jump(self, y, p, c)`: M::jump at the end of a time
point's iteration of the forward, its recomputation and M::jump_vjp in the adjoint) against the same model without the hook
(`jump = None`: the struct has no new member, so its kernels are what the commit before the hook compiled).  The model is
tests/modelgen_jump_models.PrprDiluted -- the forced prpr restatement, every species scaled by the point's `keep` and
`dose * bolus` added to YFP --, for beuler its `implicit = True` subclass.  B=36, S=200, T=86 -- the inputs and the measurement
of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, both routes alternating over several rounds in
one process), the schedule of modelgen_jump_models.schedule (two or three events per data row):
  midpoint, rk4   PrprDiluted          with / without the hook
  beuler          PrprDilutedImplicit  with / without the hook
There is no threshold: the difference per launch is a finding.
    python tests/probe/modelgen_jump_timing.py [--reps 200] [--rounds 5]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_jump_models as JM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV


class PrprDilutedPlain(JM.PrprDiluted):
    model_key = "gen_prpr_constant_diluted_plain"
    jump = None


class PrprDilutedImplicit(JM.PrprDiluted):
    model_key = "gen_prpr_constant_diluted_implicit"
    implicit = True


class PrprDilutedImplicitPlain(PrprDilutedImplicit):
    model_key = "gen_prpr_constant_diluted_implicit_plain"
    jump = None


# (the three classes above are the ones no test module builds: their libraries are compiled on the probe's first run)
CASES = (("midpoint", JM.PrprDiluted, PrprDilutedPlain), ("rk4", JM.PrprDiluted, PrprDilutedPlain),
         ("beuler", PrprDilutedImplicit, PrprDilutedImplicitPlain))


def _launches(cls, solver, theta, times, cond, obs):
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    prob = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
    traj = torch.empty((T, len(cls.species), B, S), device=DEV)
    xpred = torch.empty((T, 4, B, S), device=DEV)
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
    return {"fwd": fwd, "bwd": bwd, "traj": traj, "g_theta": g_theta, "keep": keep}


def measure(a, solver, with_hook, without):
    for cls in (with_hook, without):
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(with_hook.model_key)
    assert hip.model_slots(without.model_key) == slots  # (the same theta rows through both routes)
    assert with_hook.model_key in hip.GENERATED_JUMP and without.model_key not in hip.GENERATED_JUMP
    theta, _, times, obs = AB.problem(slots)
    cond = JM.series_of(with_hook, B, times.double().cpu()).float().reshape(B, -1).contiguous().to(DEV)
    variants = {"with the hook": _launches(with_hook, solver, theta, times, cond, obs),
                "without": _launches(without, solver, theta, times, cond, obs)}
    for v in variants.values():
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(v[kind](), kind)
    torch.cuda.synchronize()
    print("%s: finite share of the trajectory %s; the two routes differ by up to %.2e of %.2f" % (solver, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in variants.items()),
        float((variants["with the hook"]["traj"] - variants["without"]["traj"]).abs().max()),
        float(variants["without"]["traj"].abs().max())))
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
        w, wo = mid(("with the hook", kind)), mid(("without", kind))
        print("%s %s: %s; difference %+.1f us per launch (%+.1f %%)  [%d rounds x %d launches]" % (solver, kind, ", ".join(
            "%s %.1f us (%.1f .. %.1f)" % (key, mid((key, kind)), med[(key, kind)][0], med[(key, kind)][-1]) for key in variants),
            w - wo, 100.0 * (w - wo) / wo, a.rounds, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for solver, with_hook, without in CASES:
        measure(a, solver, with_hook, without)


if __name__ == "__main__":
    main()
