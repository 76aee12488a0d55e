"""Forward / adjoint launch times of generated models, one case per feature of vihds.modelgen, B=36, S=200, T=86.  The A/B
cases (AB_CASES) time the same problem through two routes of the same thread-per-trajectory kernel template: the
prpr_constant restatement (tests/modelgen_models.py: PrprRestated) and a subclass of it that routes one piece through the
generated struct.  HIP events around back-to-back launches, the two routes alternating over several rounds; one line per
solver and launch kind.  The case `nn` times a model with networks and the contraction of its adjoint dump.
    python tests/probe/modelgen_ab_timing.py --case {nn,observe,noise,likelihood,piecewise} [--reps 200] [--rounds 5]
                                             [--solvers midpoint,rk4]"""
import argparse
import ctypes
import importlib
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

B, S, T, DEV = 36, 200, 86, "cuda:0"


def _alias_pass_through(row_of, own_module):
    """PrprPassThrough names its four noise parameters itself: the same theta rows through both routes."""
    row_of.update({a: row_of[b] for a, b in zip(own_module.PASS_THROUGH, MM.PREC)})


# case -> own: (module, class) of the second route; labels: how the printed line names the two routes; solvers: the
# default of --solvers; c0: the treatment c[0] of every row; rows: an adjustment of the theta rows, where the second route
# names some differently (otherwise both routes must have the same slots)
AB_CASES = {
    # the same observation map: observe_kind "default" (the kernels' fixed map) vs the default map written as the model's
    # own observe (OBS_CUSTOM: the generated struct's observe / observe_vjp)
    "observe": dict(own=("modelgen_observe_models", "PrprOwnMap"), labels=("fixed map", "own map"), solvers="midpoint"),
    # the same precisions: ConstantPrecisions (four theta rows, log 2 pi - log prec folded once per trajectory, no precision
    # rows in the trajectory) vs a precision() that returns four parameters unchanged (own_prec<>: the generated struct's
    # precision / precision_vjp per time point, four more rows stored per time point)
    "noise": dict(own=("modelgen_noise_models", "PrprPassThrough"), labels=("constant precisions", "own precision map"),
                  rows=_alias_pass_through),
    # the same Gaussian log-likelihood: the kernels' own term (log 2 pi - log prec folded once per trajectory) vs a
    # log_likelihood() that writes the same formula out (own_lik<>: the generated struct's loglik / loglik_vjp per time
    # point, a logf per signal and time point)
    "likelihood": dict(own=("modelgen_likelihood_models", "PrprGaussianThrough"), labels=("built-in Gaussian", "own log_likelihood")),
    # a right-hand side with a switch: PrprDosed multiplies the YFP production by where(t < c[0], 0, 1) -- one comparison and
    # one select per rhs evaluation, one more select in rhs_vjp, one more effective parameter (the treatment).  The switch
    # time is 10 of the 20 hours (c[0] = 10: the inducer is added half way), so half of the steps run on either side
    "piecewise": dict(own=("modelgen_piecewise_models", "PrprDosed"), labels=("PrprRestated", "PrprDosed"), c0=10.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["nn"] + list(AB_CASES))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solvers", default=None)
    a = ap.parse_args()
    if a.case == "nn":
        for solver in (a.solvers or "midpoint").split(","):
            measure_networks(a, solver)
        return
    case = AB_CASES[a.case]
    for solver in (a.solvers or case.get("solvers", "midpoint,rk4")).split(","):
        measure_ab(a, case, solver)


def problem(slots, c0=0.0):
    """theta [slots,B,S], cond [B,1] (log(1 + c0), as the data holds a treatment), times [T], observations [B,4,T]."""
    gen = torch.Generator(device=DEV).manual_seed(0)
    theta = 0.5 + torch.rand((len(slots), B, S), device=DEV, generator=gen)
    cond = torch.full((B, 1), math.log1p(c0), device=DEV)
    times = torch.linspace(0.0, 20.0, T, device=DEV)
    obs = torch.rand((B, 4, T), device=DEV, generator=gen)
    return theta, cond, times, obs


def measure_ab(a, case, solver):
    own_module = importlib.import_module(case["own"][0])
    routes = (("fixed", MM.PrprRestated), ("own", getattr(own_module, case["own"][1])))
    for _, cls in routes:
        modelgen.register_kernel(cls, False)
    slots = hip.model_slots(MM.PrprRestated.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    if "rows" in case:
        case["rows"](row_of, own_module)
    else:
        assert hip.model_slots(routes[1][1].model_key) == slots  # (the same theta rows through both routes)
    theta, cond, times, obs = problem(slots, case.get("c0", 0.0))
    L = hip.lib()
    st = hip.current_stream()
    launches = {}
    for route, cls in routes:
        spec = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=1)
        prob = spec.bind(B, S, T)
        N = spec.n_states
        traj = torch.empty((T, N, B, S), device=DEV)
        xpred = torch.empty((T, 4, B, S), device=DEV)
        logp = torch.empty((4, B, S), device=DEV)
        g_logp = torch.ones((4, B, S), device=DEV)
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
        print("%s %s: %s %.1f us (%.1f .. %.1f), %s %.1f us (%.1f .. %.1f), ratio of medians %.3f  [%d rounds x %d launches]"
              % (solver, name, case["labels"][0], f[len(f) // 2], f[0], f[-1], case["labels"][1], o[len(o) // 2], o[0], o[-1],
                 o[len(o) // 2] / f[len(f) // 2], a.rounds, a.reps))


# ---- nn: a generated model with networks (tests/modelgen_hybrid_models.py: GrowthWithLatents, 5 -> 8 -> 4 ReLU and 3 -> 4 -> 1
# tanh); the contraction of its adjoint dump into the weight gradient (vihds_gram_blocks per network + the bias row sums:
# ops.decoder_weight_grads) and the dump's size; and the built-in dr_blackbox at kernel_variant=1 -- the same
# thread-per-trajectory template -- at the same shape.  One line per figure (--rounds is not used)
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


def network_launches(spec, theta, cond, dev1hot, times, obs, weights):
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


def measure_networks(a, solver):
    import modelgen_hybrid_models as HM

    cls = HM.GrowthWithLatents
    modelgen.register_kernel(cls, False)
    slots = hip.model_slots(cls.model_key)
    row_of = {n: i for i, n in enumerate(slots)}
    gen = torch.Generator(device=DEV).manual_seed(0)
    theta = 0.5 + torch.rand((len(slots), B, S), device=DEV, generator=gen)
    cond = torch.rand((B, 1), device=DEV, generator=gen)
    times = torch.linspace(0.0, 17.0, T, device=DEV)
    obs = torch.rand((B, 4, T), device=DEV, generator=gen)
    spec = ops.OdeProblemSpec(cls.model_key, solver, row_of, len(slots), C=1)
    n_w = hip.lib().vihds_model_n_weights(ctypes.byref(spec.bind(B, S, T)))
    weights = 0.5 * torch.randn(n_w, device=DEV, generator=gen)
    prob, fwd, bwd, aux, g_w, n_aux = network_launches(spec, theta, cond, None, times, obs, weights)
    print("%s hybrid (%s, %d weights) fwd: %.1f us" % (solver, cls.model_key, n_w, timed(fwd, a.reps)))
    print("%s hybrid bwd (with the weight-gradient dump): %.1f us" % (solver, timed(bwd, a.reps)))
    print("%s hybrid weight-gradient contraction (2 x vihds_gram_blocks + 4 row sums): %.1f us" % (
        solver, timed(lambda: ops.decoder_weight_grads(spec, prob, aux, g_w), a.reps)))
    stages = {"euler": 1, "rk4": 4}.get(solver, 2)
    fields = sum(i + 2 * h + o for i, h, o in spec.networks)
    assert n_aux == fields * (T - 1) * stages * B * S
    print("%s hybrid aux: %d floats = %.1f MB (%d fields x %d evaluations x %d trajectories)" % (
        solver, n_aux, 4e-6 * n_aux, fields, (T - 1) * stages, B * S))
    # the built-in dr_blackbox, thread per trajectory
    from test_hip_parity import _blackbox_problem

    bspec, btheta, bw, bcond, bdev, btimes, bobs = _blackbox_problem(B, S, T, seed=0, solver=solver, variant=1)
    _, bfwd, bbwd, _, _, b_aux = network_launches(bspec, btheta, bcond, bdev, btimes, bobs, bw)
    print("%s dr_blackbox kernel_variant=1 (%d weights) fwd: %.1f us" % (solver, bw.numel(), timed(bfwd, a.reps)))
    print("%s dr_blackbox kernel_variant=1 bwd: %.1f us (aux %.1f MB)" % (solver, timed(bbwd, a.reps), 4e-6 * b_aux))


if __name__ == "__main__":
    main()
