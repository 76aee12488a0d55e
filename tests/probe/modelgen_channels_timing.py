"""Forward launch and training-step (forward + adjoint launch) times of generated models with reaction-channel noise against a
diagonal twin and a noise-free twin of the same drift, B=36, S=200, T=86 -- the measurement of tests/probe/modelgen_sde_timing.py
(HIP events around back-to-back launches, the routes alternating over several rounds, one line per class, solver and kind):
  channels      ExpressionCLE (5 channels, 6 entries, four sub-steps, one forcing) and Channels8 (8 channels, 32 entries) of
                tests/modelgen_channel_models.py: two Philox4x32-10 blocks per step each (channels 0..3 and 4..7)
  diagonal      the same class with channel_noise = None and diffusion(self, y, p, c) = the root of the row sums of G^2: the same
                marginal variance per species from one Wiener process per species.  Four species: ONE Philox block per step -- a
                diagonal model of four species cannot draw more, so the twin has the same number of NOISY SPECIES, not of blocks;
                the difference to it is one more block plus the extra amplitudes and FMAs
  noise-free    the same class with channel_noise = None
    python tests/probe/modelgen_channels_timing.py [--reps 200] [--rounds 5] [--solvers midpoint,rk4]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import modelgen_ab_timing as AB  # noqa: E402  (puts the repository, the package and tests/ on the path)
import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
from vihds.modelgen import sqrt  # noqa: E402
import modelgen_channel_models as CM  # noqa: E402

B, S, T, DEV = AB.B, AB.S, AB.T, AB.DEV


def _diagonal(self, y, p, c):
    cols = type(self).__mro__[1].channel_noise(self, y, p, c)  # (the channel class's own columns)
    out = []
    for q in range(len(y)):
        total = 0.0
        for col in cols:
            total = total + col[q] * col[q]
        out.append(sqrt(total) if not isinstance(total, float) else total)
    return out


def twins(cls):
    quiet = type(cls.__name__ + "Quiet", (cls,), {"model_key": cls.model_key + "_quiet", "channel_noise": None, "__module__": cls.__module__})
    diag = type(cls.__name__ + "Diagonal", (cls,), {"model_key": cls.model_key + "_diagonal", "channel_noise": None,
                                                    "diffusion": _diagonal, "__module__": cls.__module__})
    return (("quiet", quiet, "noise-free"), ("diag", diag, "diagonal"), ("chan", cls, "channels"))


def measure(a, cls, solver):
    routes = twins(cls)
    for _, c, _label in routes:
        modelgen.register_kernel(c, False)
    times = torch.linspace(0.0, 4.0, T, device=DEV)
    series = CM.smooth_series(B, times.cpu().double())[:, None, :] if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    obs = torch.ones((B, 4, T), device=DEV)
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, c, _label in routes:
        slots = hip.model_slots(c.model_key)
        row_of = {n: i for i, n in enumerate(slots)}
        th = torch.stack([torch.full((B, S), float(CM.BASES[cls][n]), device=DEV) for n in slots]).contiguous()
        parts = [series.reshape(B, -1).float()]
        if route != "quiet":
            parts.append(torch.tensor([[12345.0, 678.0]]).expand(B, 2))
        cond = torch.cat(parts, dim=1).to(DEV).contiguous()
        prob = ops.OdeProblemSpec(c.model_key, solver, row_of, len(slots), C=cond.shape[1]).bind(B, S, T)
        assert int(L.vihds_ode_bwd_aux_floats(ctypes.byref(prob))) == 0  # (nothing is stored for the backward pass)
        traj = torch.empty((T, len(c.species), B, S), device=DEV)
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

        def step(fwd=fwd, bwd=bwd):  # (the model's part of a training step: the forward launch, then the adjoint)
            fwd()
            return bwd()

        launches[route] = {"fwd": fwd, "step": step, "logp": logp, "g_theta": g_theta, "keep": (th, cond)}
        hip.check(fwd(), "fwd")  # (warm-up; the adjoint reads the trajectory the forward launch left)
        hip.check(bwd(), "bwd")
    torch.cuda.synchronize()
    for route in launches:
        assert bool(torch.isfinite(launches[route]["logp"]).all()) and bool(torch.isfinite(launches[route]["g_theta"]).all()), route
    res = {}
    for _ in range(a.rounds):
        for name in ("fwd", "step"):
            for route, _c, _label in routes:
                fn = launches[route][name]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _k in range(a.reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                res.setdefault((route, name), []).append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    n_steps = (T - 1) * int(cls.substeps)
    for name in ("fwd", "step"):
        med, parts = {}, []
        for route, _c, label in routes:
            v = sorted(res[(route, name)])
            med[route] = v[len(v) // 2]
            parts.append("%s %.1f us (%.1f .. %.1f)" % (label, med[route], v[0], v[-1]))
        print("%s %s %s: %s  [%d rounds x %d launches]" % (cls.__name__, solver, name, ", ".join(parts), a.rounds, a.reps))
        print("%s %s %s: channels / diagonal %.3f, channels / noise-free %.3f; channels - diagonal %.1f us = %.0f ns per step" % (
            cls.__name__, solver, name, med["chan"] / med["diag"], med["chan"] / med["quiet"], med["chan"] - med["diag"],
            1000.0 * (med["chan"] - med["diag"]) / n_steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solvers", default="midpoint,rk4")
    a = ap.parse_args()
    for cls in (CM.ExpressionCLE, CM.Channels8):
        for solver in a.solvers.split(","):
            measure(a, cls, solver)


if __name__ == "__main__":
    main()
