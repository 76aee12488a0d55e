"""Forward / adjoint launch times of a generated model with step control (`step_tolerance`: every trajectory picks 2, 4 or 8
steps per observation interval by step doubling, csrc/vihds_stepctl.hpp) against its fixed twins, alternating in one process at
B=36, S=200, T=86 on the pulsed prpr model of tests/modelgen_stepctl_models.py (a pulse of light over a seventh of the grid, a
dilution and a dose at two or three reads per row):
  PulsedPrpr      M = 8, (rtol, atol) = (1e-3, 1e-6)    the controlled class
  PulsedPrprSub8  substeps = 8                          the yardstick: the only way to the same accuracy without the control
  PulsedPrprSub1  substeps = 1                          one step per interval
The measurement is that of tests/probe/modelgen_ab_timing.py (HIP events around back-to-back launches, the variants alternating
over several rounds).  It prints the histogram of the chosen counts; passing at the first test costs 1 + 2 = 3 steps for a count
of 2, a saturated interval 1 + 2 + 4 + 8 = 15 for 8, and a wavefront runs as long as its slowest lane.  There is no threshold:
the ratio controlled / fixed 8 is a finding, whichever way it falls.
    python tests/probe/modelgen_stepctl_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
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
import modelgen_stepctl_models as CM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
VARIANTS = (("controlled M=8", CM.PulsedPrpr), ("substeps=8", CM.PulsedPrprSub8), ("substeps=1", CM.PulsedPrprSub1))


def _launches(cls, solver, theta, times, cond, obs):
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    spec = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=cond.shape[1])
    prob = spec.bind(B, S, T)
    traj = torch.empty((T, spec.n_states, B, S), device=DEV)
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
    return {"fwd": fwd, "bwd": bwd, "traj": traj, "keep": keep}


def measure(a, solver):
    for _, cls in VARIANTS:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(CM.PulsedPrpr.model_key)
    assert all(hip.model_slots(cls.model_key) == slots for _, cls in VARIANTS)
    theta, _, times, obs = AB.problem(slots)
    t = times.cpu().double()
    light = torch.where((t >= 5.0) & (t <= 8.0), torch.tensor(6.0, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64))
    keep, dose = JM.schedule(B, T)
    series = torch.stack([light[None, :].expand(B, T), keep, dose], dim=1)  # (the order of PrprDiluted.forcings)
    assert list(CM.PulsedPrpr.forcings) == ["light", "keep", "dose"]
    cond = series.reshape(B, -1).float().to(DEV).contiguous()
    variants = {name: _launches(cls, solver, theta, times, cond, obs) for name, cls in VARIANTS}
    for v in variants.values():
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(v[kind](), kind)
    torch.cuda.synchronize()
    print("%s: finite share of the trajectory %s" % (solver, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in variants.items())))
    counts, saturated = modelgen.substep_counts(variants["controlled M=8"]["traj"], CM.PulsedPrpr)
    n = counts.numel()
    hist = {c: int(((counts == c) & ~saturated).sum()) for c in (2, 4, 8)}
    print("%s: chosen counts over %d intervals: %s, saturated %d (%.1f %%); share that passed at the first test %.3f"
          % (solver, n, ", ".join("%d: %d" % kv for kv in hist.items()), int(saturated.sum()), 100.0 * float(saturated.sum()) / n,
             hist[2] / n))
    steps = hist[2] * 3 + hist[4] * 7 + (hist[8] + int(saturated.sum())) * 15
    per_wave = counts.reshape(T - 1, -1)
    pad = (-per_wave.shape[1]) % 64
    waves = torch.nn.functional.pad(per_wave, (0, pad)).reshape(T - 1, -1, 64).amax(-1)
    wave_steps = sum({2: 3, 4: 7, 8: 15}[int(c)] for c in waves.reshape(-1).tolist())
    print("%s: forward steps per interval and trajectory %.2f (fixed 8: 8); per wavefront, the slowest lane's %.2f"
          % (solver, steps / n, wave_steps / waves.numel()))
    d = (variants["controlled M=8"]["traj"][:, :-1] - variants["substeps=8"]["traj"]).abs().max()
    print("%s: largest difference of the controlled states to the fixed-8 states %.2e (largest value %.2f)"
          % (solver, float(d), float(variants["substeps=8"]["traj"].abs().max())))
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
        print("%s %s: %s  [%d rounds x %d launches]" % (solver, kind, ", ".join(
            "%s %.1f us (%.1f .. %.1f)" % (key, mid((key, kind)), med[(key, kind)][0], med[(key, kind)][-1]) for key in variants),
            a.rounds, a.reps))
        print("%s %s: controlled / substeps=8 %.2f, controlled / substeps=1 %.2f" % (
            solver, kind, mid(("controlled M=8", kind)) / mid(("substeps=8", kind)),
            mid(("controlled M=8", kind)) / mid(("substeps=1", kind))))
    print("%s fwd + bwd: controlled / substeps=8 %.2f" % (
        solver, (mid(("controlled M=8", "fwd")) + mid(("controlled M=8", "bwd")))
        / (mid(("substeps=8", "fwd")) + mid(("substeps=8", "bwd")))))


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
