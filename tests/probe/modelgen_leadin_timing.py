"""Forward / adjoint launch times of generated models with a lead-in phase (`lead_in = L`, `lead_in_steps = n`: n unscored steps
of the scheme before the first observation point, the adjoint recomputing the n - 1 intermediate states into LDS) against the
only way to get the same states without it: the same class with no lead-in on the grid with the n lead-in times prepended (T + n
points, a forcing's series padded with its first sample), which does the same arithmetic and also stores, observes and scores
the extra points.  B=36, S=200, T=86 -- the inputs and the measurement of tests/probe/modelgen_ab_timing.py (HIP events around
back-to-back launches, every variant alternating over several rounds in one process):
  PrprForced    rk4      n = 4
  PrprImplicit  beuler   n = 4
There is no threshold: the ratio lead-in / prepended is a finding.
    python tests/probe/modelgen_leadin_timing.py [--reps 200] [--rounds 5]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import modelgen_substeps_timing as ST  # noqa: E402
import torch  # noqa: E402

from vihds import hip, modelgen  # noqa: E402
import modelgen_forcing_models as FM  # noqa: E402
import modelgen_implicit_models as IM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV
LEAD, STEPS = 0.94, 4  # (four steps of about the grid's own 20 / 85)


class PrprForcedLead4(FM.PrprForced):
    model_key = "gen_prpr_constant_forced_lead4"
    lead_in = LEAD
    lead_in_steps = STEPS


class PrprImplicitLead4(IM.PrprImplicit):
    model_key = "gen_prpr_constant_implicit_lead4"
    lead_in = LEAD
    lead_in_steps = STEPS


# (the two classes with a lead-in are built by no test module: their libraries are compiled on the probe's first run)
CASES = (("PrprForced", "rk4", FM.PrprForced, PrprForcedLead4), ("PrprImplicit", "beuler", IM.PrprImplicit, PrprImplicitLead4))


def measure(a, name, solver, plain, lead):
    for cls in (plain, lead):
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(plain.model_key)
    assert slots == hip.model_slots(lead.model_key)
    theta, _, times, obs = AB.problem(slots)
    n = int(lead.lead_in_steps)
    forced = bool(plain.forcings)
    series = (1.0 + 0.5 * torch.sin(0.9 * times[None, :] + 0.7 * torch.arange(B, device=DEV)[:, None]))[:, None, :] if forced else None
    front = torch.as_tensor(modelgen.lead_in_times(lead, float(times[0]))[:-1]).to(DEV)
    long_times = torch.cat([front, times]).contiguous()
    pad = lambda v: torch.cat([v[..., :1].expand(v.shape[:-1] + (n,)), v], dim=-1).contiguous()  # noqa: E731
    variants = {"lead-in": ST._launches(lead, solver, theta, times, series, obs),
                "prepended": ST._launches(plain, solver, theta, long_times, pad(series) if forced else None, pad(obs)),
                "none": ST._launches(plain, solver, theta, times, series, obs)}
    for v in variants.values():
        for kind in ("fwd", "bwd"):  # (warm-up; the adjoint reads the trajectory the forward launch left)
            hip.check(v[kind](), kind)
    torch.cuda.synchronize()
    print("%s %s: finite share of the trajectory %s" % (name, solver, ", ".join(
        "%s %.3f" % (k, float(torch.isfinite(v["traj"]).float().mean())) for k, v in variants.items())))
    d = (variants["lead-in"]["traj"] - variants["prepended"]["traj"][n:]).abs().max()
    print("%s %s: largest difference to the prepended-grid launch at the observation points %.2e (largest value %.2f)"
          % (name, solver, float(d), float(variants["lead-in"]["traj"].abs().max())))
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
        print("%s %s %s: lead-in / prepended %.2f, lead-in / none %.2f" % (
            name, solver, kind, mid(("lead-in", kind)) / mid(("prepended", kind)), mid(("lead-in", kind)) / mid(("none", kind))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for name, solver, plain, lead in CASES:
        measure(a, name, solver, plain, lead)


if __name__ == "__main__":
    main()
