"""Forward / adjoint launch times of a generated model with networks (tests/modelgen_hybrid_models.py: GrowthWithLatents,
5 -> 8 -> 4 ReLU and 3 -> 4 -> 1 tanh) at B=36, S=200, T=86, midpoint; the contraction of its adjoint dump into the weight
gradient (vihds_gram_blocks per network + the bias row sums: ops.decoder_weight_grads) and the dump's size; and the built-in
dr_blackbox at kernel_variant=1 -- the same thread-per-trajectory template -- at the same shape.  HIP events around
back-to-back launches; one line per figure.
    python tests/probe/modelgen_nn_timing.py [--reps 200]"""
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
import modelgen_hybrid_models as HM  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / reps


def launches(spec, B, S, T, theta, cond, dev1hot, times, obs, weights):
    L = hip.lib()
    prob = spec.bind(B, S, T)
    N = spec.n_states
    traj = torch.empty((T, N, B, S), device=theta.device)
    xpred = torch.empty((T, 4, B, S), device=theta.device)
    logp = torch.empty((4, B, S), device=theta.device)
    g_logp = torch.ones((4, B, S), device=theta.device)
    g_theta = torch.zeros_like(theta)
    n_aux = int(L.vihds_ode_bwd_aux_floats(ctypes.byref(prob)))
    aux = torch.empty(max(n_aux, 1), device=theta.device)
    g_w = torch.zeros_like(weights)
    st = hip.current_stream()
    fwd = lambda: hip.check(L.vihds_ode_fwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), hip.ptr(dev1hot),  # noqa: E731
                                            times.data_ptr(), obs.data_ptr(), weights.data_ptr(), traj.data_ptr(),
                                            xpred.data_ptr(), logp.data_ptr(), st), "fwd")
    bwd = lambda: hip.check(L.vihds_ode_bwd(ctypes.byref(prob), theta.data_ptr(), cond.data_ptr(), hip.ptr(dev1hot),  # noqa: E731
                                            times.data_ptr(), obs.data_ptr(), weights.data_ptr(), traj.data_ptr(), None, None,
                                            g_logp.data_ptr(), g_theta.data_ptr(), g_w.data_ptr(), aux.data_ptr(), st), "bwd")
    return prob, fwd, bwd, aux, g_w, n_aux


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--solver", default="midpoint")
    a = ap.parse_args()
    B, S, T, dev = 36, 200, 86, "cuda:0"
    cls = HM.GrowthWithLatents
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    gen = torch.Generator(device=dev).manual_seed(0)
    theta = 0.5 + torch.rand((len(slots), B, S), device=dev, generator=gen)
    cond = torch.rand((B, 1), device=dev, generator=gen)
    times = torch.linspace(0.0, 17.0, T, device=dev)
    obs = torch.rand((B, 4, T), device=dev, generator=gen)
    spec = ops.OdeProblemSpec(cls.model_key, a.solver, row_of, len(slots), C=1)
    n_w = hip.lib().vihds_model_n_weights(ctypes.byref(spec.bind(B, S, T)))
    weights = 0.5 * torch.randn(n_w, device=dev, generator=gen)
    prob, fwd, bwd, aux, g_w, n_aux = launches(spec, B, S, T, theta, cond, None, times, obs, weights)
    print("%s hybrid (%s, %d weights) fwd: %.1f us" % (a.solver, cls.model_key, n_w, timed(fwd, a.reps)))
    print("%s hybrid bwd (with the weight-gradient dump): %.1f us" % (a.solver, timed(bwd, a.reps)))
    print("%s hybrid weight-gradient contraction (2 x vihds_gram_blocks + 4 row sums): %.1f us" % (
        a.solver, timed(lambda: ops.decoder_weight_grads(spec, prob, aux, g_w), a.reps)))
    stages = {"euler": 1, "rk4": 4}.get(a.solver, 2)
    fields = sum(i + 2 * h + o for i, h, o in spec.networks)
    assert n_aux == fields * (T - 1) * stages * B * S
    print("%s hybrid aux: %d floats = %.1f MB (%d fields x %d evaluations x %d trajectories)" % (
        a.solver, n_aux, 4e-6 * n_aux, fields, (T - 1) * stages, B * S))
    # the built-in dr_blackbox, thread per trajectory
    from test_hip_parity import _blackbox_problem

    bspec, btheta, bw, bcond, bdev, btimes, bobs = _blackbox_problem(B, S, T, seed=0, solver=a.solver, variant=1)
    _, bfwd, bbwd, _, _, b_aux = launches(bspec, B, S, T, btheta, bcond, bdev, btimes, bobs, bw)
    print("%s dr_blackbox kernel_variant=1 (%d weights) fwd: %.1f us" % (a.solver, bw.numel(), timed(bfwd, a.reps)))
    print("%s dr_blackbox kernel_variant=1 bwd: %.1f us (aux %.1f MB)" % (a.solver, timed(bbwd, a.reps), 4e-6 * b_aux))


if __name__ == "__main__":
    main()
