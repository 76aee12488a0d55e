"""Forward / adjoint launch times of a generated model against the hand-written one (the same thread-per-trajectory kernel
template): prpr_constant restated with vihds.modelgen vs the built-in prpr_constant at kernel_variant=1, B=36, S=200, T=86,
midpoint.  HIP events around back-to-back launches; prints one line per launch kind.
    python tests/probe/modelgen_timing.py [--reps 200]"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "vi-hds_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from vihds import hip, modelgen, ops  # noqa: E402
import modelgen_models as MM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--solver", default="midpoint")
    a = ap.parse_args()
    B, S, T, dev = 36, 200, 86, "cuda:0"
    modelgen.register_kernel(MM.PrprRestated, False)
    slots = hip.model_slots("prpr_constant")
    row_of = {n: i for i, n in enumerate(slots)}
    gen = torch.Generator(device=dev).manual_seed(0)
    theta = 0.5 + torch.rand((len(slots), B, S), device=dev, generator=gen)
    cond = torch.zeros((B, 1), device=dev)
    times = torch.linspace(0.0, 20.0, T, device=dev)
    obs = torch.rand((B, 4, T), device=dev, generator=gen)
    L = hip.lib()
    res = {}
    for key, kv in (("prpr_constant", 1), (MM.PrprRestated.model_key, 0)):
        spec = ops.OdeProblemSpec(key, a.solver, row_of, len(slots), C=1, kernel_variant=kv)
        prob = spec.bind(B, S, T)
        N = spec.n_states
        traj = torch.empty((T, N, B, S), device=dev)
        xpred = torch.empty((T, 4, B, S), device=dev)
        logp = torch.empty((4, B, S), device=dev)
        g_logp = torch.ones((4, B, S), device=dev)
        g_theta = torch.zeros_like(theta)
        st = hip.current_stream()
        fwd = lambda: L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),  # noqa: E731
                                      obs.data_ptr(), None, traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(), st)
        bwd = lambda: L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), None, times.data_ptr(),  # noqa: E731
                                      obs.data_ptr(), None, traj.data_ptr(), None, None, g_logp.data_ptr(),
                                      g_theta.data_ptr(), None, None, st)
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            hip.check(fn(), name)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            res[(key, name)] = t0.elapsed_time(t1) * 1000.0 / a.reps
    for name in ("fwd", "bwd"):
        b, g = res[("prpr_constant", name)], res[(MM.PrprRestated.model_key, name)]
        print("%s %s: built-in %.1f us, generated %.1f us, ratio %.3f" % (a.solver, name, b, g, g / b))


if __name__ == "__main__":
    main()
