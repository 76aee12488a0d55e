"""Which model launcher accepts which launch mode: every mode-carrying ODE entry point of the C ABI (the plain forward, the
sampling stage in front of it, the evaluation's second pass, the host-driven and the device-resident adaptive controllers)
and the two backward entry points (vihds_ode_bwd at rk4, vihds_ode_bwd_elbo at both solvers, on the trajectory the plain
forward just wrote) called for every built-in model, one registered generated model and one sized dr_blackbox side library, at kernel_variant
0 / 1 and rk4 / dopri5, against the table recorded in tests/golden/launch_mode_table.json.

The launchers decide on model, variant, solver and mode, never on size, so the smallest legal shape (B 2, S 3, T 5) takes
every branch.  Parameters sit at their prior locations (q = p, u = 0 through the library's own sampling stage), every call
gets real device buffers of the sizes the library's own queries ask for, and outputs start as NaN: "finite" means written
and finite.  (g_weights is the one output the kernels ADD to: it starts as zero like its callers', "finite" covers it, and
"g_weights_written" records whether anything arrived in it -- dr_blackbox leaves it alone, its gradients come from aux.)
A launcher that accepts a mode it used to decline therefore shows up as a table mismatch, not as a fault.

Record the table (on a GPU, against the library the table is to pin):  python tests/test_launch_modes.py --out <file>"""
import ctypes
import json
import os
import sys
from functools import lru_cache

import pytest
import torch

if __name__ == "__main__":  # the recorder runs outside pytest: the paths tests/conftest.py sets up
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "vi-hds_amd"), os.path.join(_ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from fixture_util import GOLDEN, Fixture  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, T, D = 2, 3, 5, 7
TABLE_FILE = os.path.join(GOLDEN, "launch_mode_table.json")
VARIANTS = (0, 1)
SOLVERS = ("rk4", "dopri5")
RTOL, ATOL, MAX_GRID, MAX_STEPS = 1e-4, 1e-6, 4096, 512
FALLBACK_FLOATS = 1 << 20  # workspace of a call whose size query declines (the call then declines before any launch)

# model key -> (fixture whose prior table holds the model's parameters, treatments per data row)
PRIORS = {
    "dr_constant": ("dr_constant_icml_tiny_modeuler", 2),
    "dr_constant_v2": ("dr_constant_v2_tiny_modeuler", 2),
    "auto_constant": ("auto_constant_tiny_modeuler", 2),
    "prpr_constant": ("prpr_constant_tiny_modeuler", 2),
    "relay_constant": ("relay_constant_precisions_tiny_modeuler", 2),
    "degrader_constant": ("degrader_constant_precisions_tiny_modeuler", 3),
    "dr_constant_precisions": ("dr_constant_precisions_tiny_modeuler", 2),
    "dr_constant_precisions_v2": ("dr_constant_v2_tiny_modeuler", 2),
    "auto_constant_precisions": ("auto_constant_precisions_tiny_modeuler", 2),
    "prpr_constant_precisions": ("prpr_constant_precisions_tiny_modeuler", 2),
    "relay_constant_precisions": ("relay_constant_precisions_tiny_modeuler", 2),
    "degrader_constant_precisions": ("degrader_constant_precisions_tiny_modeuler", 3),
    "dr_blackbox": ("dr_blackbox_icml_tiny_modeuler", 2),
    "inducer_constant": ("inducer_constant_precisions_tiny_modeuler", 2),
    "inducer_constant_precisions": ("inducer_constant_precisions_tiny_modeuler", 2),
    "debug_constant": ("dr_constant_icml_tiny_modeuler", 2),
}
LANE_PRECISIONS = ("auto_constant_precisions", "prpr_constant_precisions", "relay_constant_precisions",
                   "degrader_constant_precisions")
# case name -> (model key, hidden units of the precision network)
CASES = {m: (m, 0) for m in PRIORS}
CASES.update({m + "/hidden5": (m, 5) for m in LANE_PRECISIONS})  # (a hidden layer changes the lane launchers' choice)
CASES["generated:gen_prpr_constant"] = ("generated", 0)
CASES["dr_blackbox/sized_3_12_6_8"] = ("sized", 0)


def _prior_of(fx, name):
    """(kind, mu, precision) of one parameter: the fixture's prior row, or a benign log-normal for a row it has not (the
    conditioner's rows, a model without a fixture)."""
    if name in fx.names:
        k = fx.names.index(name)
        prec = float(fx.z["p_prec"][k])
        return fx.kinds[k], float(fx.z["p_mu"][k]), prec if 0.0 < prec < float("inf") else 1.0
    if name.startswith("init_prec_"):
        return 1, 2.3, 4.0
    if name.startswith("init_"):
        return 1, -4.6, 4.0
    if name.startswith("prec_"):
        return 1, 3.0, 4.0
    return 1, -1.0, 4.0


def _spec(case, variant, solver):
    from vihds import hip, modelgen, ops

    model, hidden = CASES[case]
    kw = dict(kernel_variant=variant)
    if model == "generated":
        import modelgen_models as MM

        modelgen.register_kernel(MM.PrprRestated, False)
        model, fixture, C = MM.PrprRestated.model_key, "prpr_constant_tiny_modeuler", 2
        slots = hip.model_slots(model)
        kw.update(D=D)
    elif model == "sized":
        model, fixture, C = "dr_blackbox", "dr_blackbox_sized_tiny_modeuler", 2
        slots = ["z1", "z2", "z3", "z4", "x1", "x2", "x3", "y1", "init_x", "init_rfp", "init_yfp", "init_cfp"]
        kw.update(D=D, n_hidden_prec=6, n_hidden_states=12, n_latent_states=3, n_const=8 + C + D, slots=slots)
    else:
        fixture, C = PRIORS[model]
        slots = hip.model_slots(model)
        if model == "dr_blackbox":
            kw.update(D=D, n_hidden_prec=20, n_hidden_states=25, n_latent_states=2, n_const=12 + C + D, slots=slots)
        else:
            kw.update(D=D, n_hidden_prec=hidden)
    row_of = {n: i for i, n in enumerate(slots)}
    return ops.OdeProblemSpec(model, solver, row_of, len(slots), C=C, **kw), fixture, slots


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _finite(*tensors):
    return bool(all(torch.isfinite(t).all() for t in tensors))


@lru_cache(maxsize=None)
def _inputs(case):
    """Seeded inputs of one case, shared by its variants and solvers: the prior tables, theta at the prior locations (the
    library's own sampling stage with q = p and u = 0), treatments, one-hot devices, times, observations, weights."""
    from vihds import hip
    import hip_util as H

    spec, fixture, slots = _spec(case, 0, "rk4")
    fx = Fixture(fixture)
    rows = [_prior_of(fx, n) for n in slots]
    P = len(slots)
    kind = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=DEV)
    p_mu = torch.tensor([r[1] for r in rows], device=DEV)
    p_prec = torch.tensor([r[2] for r in rows], device=DEV)
    lo, hi = H.clip_bounds([r[0] for r in rows], p_mu.cpu(), p_prec.cpu(), 4.0)
    tab = dict(P=P, kind=kind, p_mu=p_mu, p_prec=p_prec, lo=lo.to(DEV), hi=hi.to(DEV),
               q_mu=p_mu[:, None].repeat(1, B).contiguous(), q_prec=p_prec[:, None].repeat(1, B).contiguous(),
               u=torch.zeros(B, S, P, device=DEV))
    theta, log_q, log_p = _nan(P, B, S), _nan(B, S), _nan(B, S)
    L = hip.lib()
    hip.check(L.vihds_theta_fwd(P, B, S, hip.ptr(kind), hip.ptr(tab["q_mu"]), hip.ptr(tab["q_prec"]), hip.ptr(p_mu),
                                hip.ptr(p_prec), hip.ptr(tab["lo"]), hip.ptr(tab["hi"]), hip.ptr(tab["u"]), hip.ptr(theta),
                                hip.ptr(log_q), hip.ptr(log_p), None, hip.current_stream()), "vihds_theta_fwd")
    torch.cuda.synchronize()
    assert _finite(theta), "theta at the prior locations must be finite"
    g = torch.Generator().manual_seed(7)
    C = spec.proto.C
    n_w = int(L.vihds_model_n_weights(ctypes.byref(spec.bind(B, S, T))))
    return dict(tab=tab, theta=theta, cond=torch.log1p(torch.rand(B, C, generator=g) * 1000.0).to(DEV),
                dev1hot=torch.eye(D)[torch.arange(B) % D].contiguous().to(DEV),
                times=torch.arange(T, dtype=torch.float32) * 0.25, obs=torch.rand(B, 4, T, generator=g).to(DEV),
                weights=(0.1 * torch.randn(n_w, generator=g)).to(DEV) if n_w > 0 else None,
                log_w=torch.zeros(B, S, device=DEV), lse=torch.full((B,), float(torch.tensor(float(S)).log()), device=DEV))


def _call(L, fn, outputs):
    """One entry point: (return code, the library's message when it declined, every output written and finite when it ran)."""
    L.vihds_rng_advance(None, None)  # (leaves "null rng" in the sticky error string: a decline without a message shows as that)
    rc = int(fn())
    torch.cuda.synchronize()
    if rc < 0:
        return {"rc": rc, "error": L.vihds_last_error().decode()}
    return {"rc": 0, "finite": _finite(*outputs())}


def _backward(L, x, pp, name, times, traj, logp, with_aux=True):
    """One backward entry point on the forward's trajectory: aux and g_weights of the sizes the library's queries return."""
    from vihds import hip

    n_aux, n_w = int(L.vihds_ode_bwd_aux_floats(pp)), int(L.vihds_model_n_weights(pp))
    aux = torch.zeros(n_aux, device=DEV) if with_aux and n_aux > 0 else None
    g_w = torch.zeros(n_w, device=DEV) if n_w > 0 else None
    g_theta = _nan(*x["theta"].shape)
    head = (pp, hip.ptr(x["theta"]), hip.ptr(x["cond"]), hip.ptr(x["dev1hot"]), hip.ptr(times), hip.ptr(x["obs"]),
            hip.ptr(x["weights"]), hip.ptr(traj))
    if name == "vihds_ode_bwd":
        grads = (torch.full_like(traj, 0.01), torch.full((T, 4, B, S), 0.01, device=DEV), torch.ones(4, B, S, device=DEV))
    else:  # (the log-likelihood gradient is formed in the kernel from logp, log_p, log_q)
        grads = (logp, torch.zeros(B, S, device=DEV), torch.zeros(B, S, device=DEV))
    row = _call(L, lambda: getattr(L, name)(*head, *(hip.ptr(g) for g in grads), hip.ptr(g_theta), hip.ptr(g_w), hip.ptr(aux),
                                            hip.current_stream()),
                lambda: (g_theta,) + ((g_w,) if g_w is not None else ()))
    if row["rc"] == 0 and g_w is not None:
        row["g_weights_written"] = bool((g_w != 0).any())
    return row


def _run(case, variant, solver):
    from vihds import hip

    L = hip.lib()
    spec, _, _ = _spec(case, variant, solver)
    x = _inputs(case)
    tab, theta, cond, dev1hot, obs, w = x["tab"], x["theta"], x["cond"], x["dev1hot"], x["obs"], x["weights"]
    times = x["times"].to(DEV)
    prob = spec.bind(B, S, T)
    pp = ctypes.byref(prob)
    N = int(L.vihds_problem_n_states(pp))
    assert N > 0
    st = hip.current_stream()
    out = {}

    traj, xpred, logp = _nan(T, N, B, S), _nan(T, 4, B, S), _nan(4, B, S)
    out["vihds_ode_fwd"] = _call(L, lambda: L.vihds_ode_fwd(
        pp, hip.ptr(theta), hip.ptr(cond), hip.ptr(dev1hot), hip.ptr(times), hip.ptr(obs), hip.ptr(w), hip.ptr(traj),
        hip.ptr(xpred), hip.ptr(logp), st), lambda: (traj, xpred, logp))

    for name in (("vihds_ode_bwd",) if solver == "rk4" else ()) + ("vihds_ode_bwd_elbo",):
        out[name] = _backward(L, x, pp, name, times, traj, logp)
        if spec.model == "dr_blackbox":  # (refused before any launch)
            out[name + " without aux"] = _backward(L, x, pp, name, times, traj, logp, with_aux=False)

    traj, xpred, logp = _nan(T, N, B, S), _nan(T, 4, B, S), _nan(4, B, S)
    th2, log_q, log_p = theta.clone(), _nan(B, S), _nan(B, S)
    out["vihds_theta_ode_fwd"] = _call(L, lambda: L.vihds_theta_ode_fwd(
        pp, tab["P"], hip.ptr(tab["kind"]), hip.ptr(tab["q_mu"]), hip.ptr(tab["q_prec"]), hip.ptr(tab["p_mu"]),
        hip.ptr(tab["p_prec"]), hip.ptr(tab["lo"]), hip.ptr(tab["hi"]), hip.ptr(tab["u"]), None, None, hip.ptr(cond),
        hip.ptr(dev1hot), hip.ptr(times), hip.ptr(obs), hip.ptr(w), hip.ptr(th2), hip.ptr(log_q), hip.ptr(log_p),
        hip.ptr(traj), hip.ptr(xpred), hip.ptr(logp), st), lambda: (th2, log_q, log_p, traj, xpred, logp))

    n_ws = int(L.vihds_ode_fwd_summaries_workspace_floats(pp))
    ws = _nan(max(n_ws, FALLBACK_FLOATS))
    mu, sd, states, var = _nan(B, 4, T), _nan(B, 4, T), _nan(B, N, T), _nan(B, 4, T)
    n_species = int(spec.n_species)
    out["vihds_ode_fwd_summaries"] = _call(L, lambda: L.vihds_ode_fwd_summaries(
        pp, hip.ptr(theta), hip.ptr(cond), hip.ptr(dev1hot), hip.ptr(times), hip.ptr(w), hip.ptr(x["log_w"]),
        hip.ptr(x["lse"]), hip.ptr(ws), hip.ptr(mu), hip.ptr(sd), hip.ptr(states), hip.ptr(var), st),
        lambda: (mu, sd, states.reshape(-1)[: B * n_species * T], var))
    out["vihds_ode_fwd_summaries"]["supported"] = int(L.vihds_ode_fwd_summaries_supported(pp))
    out["vihds_ode_fwd_summaries"]["workspace_query"] = min(n_ws, 0)

    n_ws = int(L.vihds_ode_adaptive_workspace_floats(pp))
    ws = _nan(max(n_ws, FALLBACK_FLOATS))
    grid, index = torch.full((MAX_GRID,), float("nan")), torch.zeros(T, dtype=torch.int32)
    n_grid = []

    def adaptive_grid():
        rc = L.vihds_ode_adaptive_grid(pp, hip.ptr(theta), hip.ptr(cond), hip.ptr(dev1hot), hip.ptr(w),
                                       x["times"].data_ptr(), RTOL, ATOL, hip.ptr(ws), grid.data_ptr(), MAX_GRID,
                                       index.data_ptr(), st)
        n_grid.append(rc)
        return min(rc, 0)  # (success returns the grid's length)

    out["vihds_ode_adaptive_grid"] = _call(L, adaptive_grid, lambda: (grid[: n_grid[0]],))
    if n_grid[0] > 0:
        out["vihds_ode_adaptive_grid"]["covers_the_output_times"] = bool(
            n_grid[0] >= T and torch.equal(grid[index.long()], x["times"]))

    n_tape = int(L.vihds_ode_adaptive_tape_floats(pp, MAX_STEPS))
    for name in ("vihds_ode_adaptive_fwd",) + (("vihds_ode_adaptive_fwd_w",) if w is not None else ()):
        tape, traj = torch.zeros(max(n_tape, FALLBACK_FLOATS), device=DEV), _nan(T, N, B, S)
        if name == "vihds_ode_adaptive_fwd":
            fn = lambda: L.vihds_ode_adaptive_fwd(pp, hip.ptr(theta), hip.ptr(cond), hip.ptr(dev1hot), hip.ptr(times),  # noqa: E731
                                                  RTOL, ATOL, MAX_STEPS, hip.ptr(tape), hip.ptr(traj), st)
        else:
            fn = lambda: L.vihds_ode_adaptive_fwd_w(pp, hip.ptr(theta), hip.ptr(cond), hip.ptr(dev1hot), hip.ptr(w),  # noqa: E731
                                                    hip.ptr(times), RTOL, ATOL, MAX_STEPS, hip.ptr(tape), hip.ptr(traj), st)
        out[name] = _call(L, fn, lambda: (traj,))
        out[name]["tape_query"] = min(n_tape, 0)
        if out[name]["rc"] == 0:
            out[name]["device_error"] = int(tape[:4].view(torch.int32)[1])  # (ops.ADAPTIVE_DEVICE_ERRORS; 0: none)
    return out


def case_table(case):
    return {"kernel_variant %d / %s" % (v, s): _run(case, v, s) for v in VARIANTS for s in SOLVERS}


@lru_cache(maxsize=None)
def _golden():
    with open(TABLE_FILE) as f:
        return json.load(f)


def test_the_table_covers_every_case():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_modes_match_the_recorded_table(case):
    got = json.loads(json.dumps(case_table(case)))
    want = _golden()[case]
    for key in sorted(want):
        for entry in sorted(want[key]):
            print("%-45s %-22s %-28s %s" % (case, key, entry, json.dumps(got.get(key, {}).get(entry), sort_keys=True)))
    assert got == want


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    table = {}
    for c in sorted(CASES):
        table[c] = case_table(c)
        print(c, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % args.out)
