"""GPU tests of a generated model's own precision map (GeneratedOdeModel.precision, own_prec<> in the kernels): four
parameters handed through against the same numbers as constant precisions, a signal-dependent noise model against its own
definition in float64, the same noise on a model with networks in rhs, an evaluation pass and one training step.

Shapes (B, S): (3, 5) one partly filled wavefront; (5, 26) rows that straddle wavefronts, three 64-thread blocks; (3, 100)
300 trajectories, so that a data row straddles two blocks of the LDS-staged forward.  T=7 on a non-uniform grid."""
import ctypes

import numpy as np
import pytest
import torch

from fixture_util import rel_err
from oracle import vihds_oracle as O
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_hybrid_models as HM
import modelgen_models as MM
import modelgen_noise_models as NM
from test_modelgen_observe_gpu import PRPR_BASE, READER_BASE, TIMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXED = ["modeuler", "modeulerwhile", "euler", "midpoint", "rk4"]
SHAPES = [(3, 5), (5, 26), (3, 100)]
TOL, GTOL = 1e-4, 5e-4  # forward per signal, gradients per parameter
_KEYS = {}


def _key(cls):
    if cls not in _KEYS:
        modelgen.register_kernel(cls, False)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _spread(base, B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: (v * torch.exp(0.2 * torch.randn(B, S, generator=gen, dtype=torch.float64))) for k, v in base.items()}


# ---- pass-through ---------------------------------------------------------------------------------------------------
def _run_shared(spec, th, cond, times, obs, n_species, seed=5):
    """forward + adjoint with upstream gradients on the log-likelihood, x_predict and the species rows of the trajectory."""
    th = th.detach().clone().requires_grad_(True)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, cond, times, obs, None, None)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    loss = (logp * torch.randn(logp.shape, device=DEV, generator=gen)).sum()
    loss = loss + (xpred * torch.randn(xpred.shape, device=DEV, generator=gen)).sum()
    species = traj[:, :n_species]
    loss = loss + (species * torch.randn(species.shape, device=DEV, generator=gen)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return traj.detach(), xpred.detach(), logp.detach(), th.grad


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("solver", FIXED + ["dopri5"])
def test_pass_through_precisions_against_constant_precisions(solver, shape):
    """PrprPassThrough (precision returns four parameters unchanged) and PrprRestated on ConstantPrecisions read the SAME theta
    buffer -- the pass-through slots name the rows of prec_x .. prec_cfp -- so every row of g_theta compares, the pass-through
    parameters' with the prec_* rows'.  Log-likelihood, species rows, x_predict and g_theta within 1e-5 (two float32 routes:
    the constant branch folds log 2 pi - log prec once, the own branch forms it per time point); the stored precision rows
    equal the parameters at every time point; dopri5: the two accepted grids are identical (the precision rows do not enter
    the controller's error norm), then both integrate on it with the log-likelihood formed by the host (ode.py) from the
    rows."""
    B, S = shape
    ref_key, own_key = _key(MM.PrprRestated), _key(NM.PrprPassThrough)
    slots = hip.model_slots(ref_key)
    own_slots = hip.model_slots(own_key)
    assert own_slots == slots[:-4] + NM.PASS_THROUGH and slots[-4:] == MM.PREC
    row_of = {n: i for i, n in enumerate(slots)}
    own_rows = dict(row_of, **{a: row_of[b] for a, b in zip(NM.PASS_THROUGH, MM.PREC)})
    th64 = _spread(PRPR_BASE, B, S, 3)
    th = torch.stack([th64[n] for n in slots]).float().to(DEV)
    cond = torch.zeros((B, 1), device=DEV)
    times = torch.tensor(TIMES, device=DEV)
    obs = (0.05 + torch.rand(B, 4, len(TIMES), generator=torch.Generator().manual_seed(4))).to(DEV)
    ref_spec = ops.OdeProblemSpec(ref_key, solver, row_of, th.shape[0], C=1)
    own_spec = ops.OdeProblemSpec(own_key, solver, own_rows, th.shape[0], C=1)
    assert (ref_spec.n_states, ref_spec.n_species) == (6, 6) and (own_spec.n_states, own_spec.n_species) == (10, 6)
    assert own_spec.own_precision and not ref_spec.own_precision
    prec_rows = [row_of[n] for n in MM.PREC]
    if solver == "dopri5":
        grid, index = ops.adaptive_grid(ref_spec, th, cond, times, None, None)
        grid_own, index_own = ops.adaptive_grid(own_spec, th, cond, times, None, None)
        assert torch.equal(grid, grid_own) and torch.equal(index, index_own)
        times = grid.to(DEV)
        obs = (0.05 + torch.rand(B, 4, times.shape[0], generator=torch.Generator().manual_seed(4))).to(DEV)
    ref = _run_shared(ref_spec, th, cond, times, obs, 6)
    got = _run_shared(own_spec, th, cond, times, obs, 6)
    figures = {"traj": rel_err(H.view_bsnt(got[0][:, :6]), H.view_bsnt(ref[0])),
               "xpred": rel_err(H.view_bsnt(got[1]), H.view_bsnt(ref[1])),
               "logp": rel_err(H.view_bs4(got[2]), H.view_bs4(ref[2]), dim=2),
               "g_theta": rel_err(got[3], ref[3], dim=0)}
    print("%s n=%d: %s" % (solver, B * S, "  ".join("%s %.2e" % kv for kv in figures.items())))
    assert float(ref[3][prec_rows].abs().amax(dim=(1, 2)).min()) > 0.0  # (every prec_* row has a gradient to compare)
    stored = got[0][:, 6:]  # [T,4,B,S]
    assert torch.equal(stored, th[prec_rows][None].expand_as(stored))
    for name, e in figures.items():
        assert e < 1e-5, (name, e)


# ---- the model's own definition in float64 -------------------------------------------------------------------------------
NOISE_BASE = {"s0_od": 0.14, "s1_od": 0.10, "s0_r": 0.20, "s1_r": 0.15, "s0_y": 0.22, "s1_y": 0.12, "s0_c": 0.21,
              "s1_c": 0.18, "s_dens": 0.25, "s_trt": 0.16}
GROWTH_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP": 1.2, "aCFP": 0.9,
               "e76": 0.5, "init_x": 0.05, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1}
_PROBLEMS, _REFS = {}, {}


def _problem(cls, B, S):
    """Inputs of one case (shared by the tests that use it; never modified)."""
    k = (cls, B, S)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    hybrid = cls is NM.GrowthWithLatentsNoise
    base = dict(GROWTH_BASE if hybrid else {n: v for n, v in READER_BASE.items() if not n.startswith("prec_")}, **NOISE_BASE)
    assert sorted(base) == sorted(cls.parameter_names)
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    N, T = len(cls.species), len(TIMES)
    pb = {"th": _spread(base, B, S, 6), "cond": torch.log1p(2.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64)),
          "times": torch.tensor(TIMES, dtype=torch.float64), "B": B, "S": S,
          "W": {name: tuple(0.6 * rnd(*shape) for shape in net.tensor_shapes()) for name, net in cls.networks.items()}
          if hybrid else None}
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in pb["th"].items()}
        xs, xp, prec = _forward(cls, th1, pb["cond"], pb["times"], "rk4", pb["W"])
        pb["obs"] = xp[:, 0] + rnd(B, 4, T) / prec[:, 0].sqrt()  # (noise of the model's own size)
    pb["G"] = {"logp": rnd(B, S, 4), "xpred": rnd(B, S, 4, T), "traj": rnd(B, S, N + 4, T)}
    _PROBLEMS[k] = pb
    return pb


def _forward(cls, th, cond, times, solver, W):
    rhs, x0 = cls.torch_problem(th, cond, W) if W else cls.torch_problem(th, cond)
    xs = O.simulate(rhs, x0, times, solver)
    xp = cls.torch_observe(xs, th, cond) if cls._observe_def is not None else O.observe_direct(xs)
    return xs, xp, cls.torch_precision(xs, th, cond)


def _reference(cls, B, S, solver, upstream):
    """torch_problem integrated by the oracle's step functions, torch_observe, torch_precision, autograd -- in float64, once
    per case."""
    k = (cls, B, S, solver, upstream)
    if k not in _REFS:
        pb = _problem(cls, B, S)
        leaf = lambda v: v.detach().clone().requires_grad_(True)  # noqa: E731
        th = {n: leaf(v) for n, v in pb["th"].items()}
        W = {name: tuple(leaf(w) for w in ws) for name, ws in pb["W"].items()} if pb["W"] else None
        xs, xp, prec = _forward(cls, th, pb["cond"], pb["times"], solver, W)
        lpo = O.log_prob_observations(xp, pb["obs"], prec)
        loss = (lpo * pb["G"]["logp"]).sum()
        if upstream:
            loss = loss + (xp * pb["G"]["xpred"]).sum() + (torch.cat([xs, prec], dim=2) * pb["G"]["traj"]).sum()
        loss.backward()
        _REFS[k] = {"traj": xs.detach(), "xpred": xp.detach(), "prec": prec.detach(), "logp": lpo.detach(),
                    "g_theta": {n: v.grad for n, v in th.items()},
                    "g_w": [w.grad for ws in W.values() for w in ws] if W else []}
    return _REFS[k]


def _kernel(cls, B, S, solver, upstream):
    pb = _problem(cls, B, S)
    key = _key(cls)
    slots = hip.model_slots(key)
    assert slots == cls.parameter_names  # (no prec_* / init_prec_* slots behind the model's own)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([pb["th"][n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=1)
    N = len(cls.species)
    assert (spec.n_states, spec.n_species) == (N + 4, N)
    w = None
    if pb["W"]:
        w = torch.cat([t.reshape(-1) for ws in pb["W"].values() for t in ws]).float().to(DEV).requires_grad_(True)
    prob = spec.bind(B, S, len(TIMES))
    assert hip.lib().vihds_model_n_weights(ctypes.byref(prob)) == (0 if w is None else w.numel())
    f32 = lambda v: v.float().to(DEV)  # noqa: E731
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, f32(pb["cond"]), f32(pb["times"]), f32(pb["obs"]), None, w)
    loss = (H.view_bs4(logp) * f32(pb["G"]["logp"])).sum()
    if upstream:
        loss = loss + (H.view_bsnt(xpred) * f32(pb["G"]["xpred"])).sum() + (H.view_bsnt(traj) * f32(pb["G"]["traj"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    full = H.view_bsnt(traj).detach().cpu()
    return {"traj": full[:, :, :N], "prec": full[:, :, N:], "xpred": H.view_bsnt(xpred).detach().cpu(),
            "logp": H.view_bs4(logp).detach().cpu(), "g_theta": {n: th.grad[row_of[n]].cpu() for n in slots},
            "g_w": None if w is None else w.grad.cpu(), "spec": spec, "prob": prob}


def _compare(got, ref, label):
    """Prints every figure, then asserts the bounds of DESIGN.md section 2."""
    lines, bad = [], []
    for k in ("traj", "xpred", "prec", "logp"):
        e = rel_err(got[k], ref[k], dim=2)
        lines.append("%s %s: %.2e (bound %.0e)" % (label, k, e, TOL))
        if not e <= TOL:
            bad.append(lines[-1])
    for n, g in ref["g_theta"].items():
        assert g is not None, n
        e = rel_err(got["g_theta"][n], g)
        lines.append("%s g_theta[%s]: %.2e (bound %.0e)" % (label, n, e, GTOL))
        if not e <= GTOL:
            bad.append(lines[-1])
    o = 0
    for k, g in enumerate(ref["g_w"]):
        e = rel_err(got["g_w"][o:o + g.numel()].view(g.shape), g)
        o += g.numel()
        lines.append("%s weight tensor %d %s: %.2e (bound %.0e)" % (label, k, tuple(g.shape), e, GTOL))
        if not e <= GTOL:
            bad.append(lines[-1])
    print("\n".join(lines))
    for n in NM.NOISE:  # (the precision-only parameters: the comparison of their rows is not vacuous)
        assert float(ref["g_theta"][n].abs().min()) > 0.0, n
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("solver", ["rk4", "modeuler"])
@pytest.mark.parametrize("upstream", [False, True])
def test_signal_dependent_noise_against_its_own_definition_in_float64(solver, upstream, shape):
    """PlateReaderNoise (its own observe; per signal a floor and a part proportional to the predicted signal, one precision
    reads a species, one a treatment): species, x_predict, the stored precision rows and the log-likelihood within 1e-4 per
    signal, every row of g_theta within 5e-4, of torch_problem + the oracle's steps + torch_observe + torch_precision with
    autograd in float64.  `upstream`: gradients arrive on x_predict and on all rows of the trajectory, the four precision
    rows included."""
    B, S = shape
    got = _kernel(NM.PlateReaderNoise, B, S, solver, upstream)
    _compare(got, _reference(NM.PlateReaderNoise, B, S, solver, upstream), "%s upstream=%s n=%d" % (solver, upstream, B * S))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("solver", ["rk4", "modeuler"])
@pytest.mark.parametrize("upstream", [False, True])
def test_noise_model_with_networks_in_rhs(solver, upstream, shape):
    """GrowthWithLatentsNoise: the same comparison, with the gradient of the eight network tensors; two runs give
    bit-identical weight gradients; the adjoint's aux buffer holds the networks' fields alone."""
    B, S = shape
    cls = NM.GrowthWithLatentsNoise
    got = _kernel(cls, B, S, solver, upstream)
    _compare(got, _reference(cls, B, S, solver, upstream), "hybrid %s upstream=%s n=%d" % (solver, upstream, B * S))
    again = _kernel(cls, B, S, solver, upstream)
    assert torch.equal(got["g_w"], again["g_w"]) and float(got["g_w"].abs().max()) > 0.0
    fields = sum(net.n_fields for net in cls.networks.values())
    stages = {"rk4": 4, "modeuler": 2}[solver]
    assert hip.lib().vihds_ode_bwd_aux_floats(ctypes.byref(got["prob"])) == fields * (len(TIMES) - 1) * stages * B * S
    plain = ops.OdeProblemSpec(_key(HM.GrowthWithLatents), solver, {n: i for i, n in enumerate(
        hip.model_slots(_key(HM.GrowthWithLatents)))}, len(HM.GrowthWithLatents.parameter_names) + 4, C=1)
    assert (hip.lib().vihds_ode_bwd_aux_floats(ctypes.byref(plain.bind(B, S, len(TIMES))))
            == hip.lib().vihds_ode_bwd_aux_floats(ctypes.byref(got["prob"])))


# ---- evaluation and training through the host path ---------------------------------------------------------------------
N_PLATE = 20


def _reader_training(monkeypatch, B, S, **over):
    """Config -> Parameters -> model -> Training on a synthetic plate of N_PLATE time points (the encoder's convolution and
    pooling windows need 15 or more) whose spec names PlateReaderNoise and gives every parameter it reads a prior; the
    plate's observations are simulated from the model itself."""
    import models
    from vihds import synthetic

    cls = NM.PlateReaderNoise
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)

    def spec_fn(solver):
        spec = synthetic.dr_constant_icml_spec(solver)
        spec["model"] = cls.model_key
        ln = synthetic._ln
        glob = spec["params"]["global"]
        glob.update({"gain_r": ln(0.3, 0.2), "bg_r": ln(-3.0, 0.2), "sat": ln(-0.5, 0.2), "auto": ln(-1.2, 0.2),
                     "leak": ln(-1.0, 0.2)})
        glob.update({n: ln(float(np.log(v)), 0.2) for n, v in NOISE_BASE.items()})
        return spec

    monkeypatch.setitem(synthetic.WORKLOADS, "reader_noise", (spec_fn, N_PLATE))
    monkeypatch.setattr(synthetic, "MODEL_SIMULATED", synthetic.MODEL_SIMULATED + ("reader_noise",))
    out = synthetic.build("reader_noise", B, S, solver="rk4", device=DEV, seed=3, **over)
    assert isinstance(out[4].decoder.ode_model, cls)
    return out


def _samples(cls, theta, q, p):
    """The samples of one pass and their log-densities, copied to the host in float64."""
    return ({n: getattr(theta, n).detach().double().cpu() for n in cls.parameter_names},
            p.log_prob(theta).detach().double().cpu(), q.log_prob(theta).detach().double().cpu())


def _float64_pass(cls, samples, batch, solver):
    """The decoder and the importance weights in float64 from the samples of one pass."""
    th, log_p, log_q = samples
    cond, times = batch.inputs.double().cpu(), batch.times.double().cpu()
    xs, xp, prec = _forward(cls, th, cond, times, solver, None)
    lpo = O.log_prob_observations(xp, batch.observations.double().cpu(), prec)
    return xs, xp, prec, lpo, lpo.sum(2) + log_p - log_q


def test_evaluation_of_a_model_with_its_own_precisions(monkeypatch, tmp_path):
    """Training.evaluate on PlateReaderNoise at B=3, S=5: the pass stores the trajectory and x_predict, the summaries come
    from vihds_iw_summaries with the precision rows of the trajectory, and iw_variance / iw_predict_std (and the other two)
    equal the importance-weighted values formed in float64 from the same samples within 1e-4 per signal.  The one-pass
    summaries decline the model.  Decoder.forward returns the precisions as a view of the stored rows."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _reader_training(monkeypatch, B, S, hip_graph=False)
    cls = NM.PlateReaderNoise
    ode = model.decoder.ode_model
    model.eval()
    seen = {}
    cost = training.cost

    def spy(batch, results, theta, q, p, **kw):
        seen.update(batch=batch, results=results, theta=theta, q=q, p=p)
        return cost(batch, results, theta, q, p, **kw)

    monkeypatch.setattr(training, "cost", spy)
    res = training.evaluate(training.train_data, S)
    sol = seen["results"].solution
    assert sol.has_x_predict and getattr(sol, "online_summaries", None) is None
    assert sol.traj_buffer.shape[1] == len(cls.species) + 4
    spec = next(iter(ode._spec_cache.values()))
    assert hip.lib().vihds_ode_fwd_summaries_supported(ctypes.byref(spec.bind(B, S, N_PLATE))) == 0
    x_states, x_predict, precisions = seen["results"]
    assert precisions.shape == (B, S, 4, N_PLATE) and x_states.shape[2] == len(cls.species)
    assert precisions.data_ptr() == sol.sol[:, :, len(cls.species):].data_ptr()
    xs, xp, prec, lpo, log_w = _float64_pass(cls, _samples(cls, seen["theta"], seen["q"], seen["p"]), seen["batch"], "rk4")
    w = torch.softmax(log_w, dim=1)[:, :, None, None]
    mu = (w * xp).sum(1)
    ref = {"iw_predict_mu": mu, "iw_predict_std": ((w * (xp ** 2 + 1.0 / prec)).sum(1) - mu ** 2).sqrt(),
           "iw_states": (w * xs).sum(1), "iw_variance": (w / prec).sum(1)}
    e = rel_err(precisions, prec)
    print("precisions %.2e" % e)
    errs = {k: rel_err(torch.as_tensor(np.asarray(getattr(res, k))), v, dim=1) for k, v in ref.items()}
    print("  ".join("%s %.2e" % kv for kv in errs.items()))
    assert e <= TOL
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_one_training_step_through_the_general_path(monkeypatch, tmp_path):
    """One Training.step on PlateReaderNoise through the general five-launch step (ops.GeneralTail, vihds_ode_bwd_elbo) with
    fixed draws: the loss equals the -ELBO formed in float64 from the step's own samples within 1e-4, and the encoder /
    global tensor of every precision-only parameter changes."""
    monkeypatch.chdir(tmp_path)
    B, S = 3, 5
    args, settings, data, parameters, model, training = _reader_training(monkeypatch, B, S, hip_graph=False)
    cls = NM.PlateReaderNoise
    batch = training.train_data
    model.train()
    seen = {}
    tail = training._general_tail

    def spy(results, theta, q, p):  # (the step's own samples, copied before the tail's launches update anything)
        seen["samples"] = _samples(cls, theta, q, p)
        return tail(results, theta, q, p)

    monkeypatch.setattr(training, "_general_tail", spy)
    enc = model.encoder
    glob_names = [d.name for d in enc.glob]
    assert all(n in glob_names for n in NM.NOISE)
    before = enc.global_free.detach().clone()  # [2, n_global]: mu and log-precision of every global parameter
    np.random.seed(21)
    torch.manual_seed(21)
    loss = float(training.step(batch))
    torch.cuda.synchronize()
    assert training._gtail_ok is True, "the general step did not take the model"
    xs, xp, prec, lpo, log_w = _float64_pass(cls, seen["samples"], batch, "rk4")
    ref = -float((torch.logsumexp(log_w, dim=1) - np.log(S)).mean())
    print("loss %.6f, float64 %.6f" % (loss, ref))
    assert abs(loss - ref) <= TOL * abs(ref)
    after = enc.global_free.detach()
    for n in NM.NOISE:  # (read by precision only: their gradient reaches the encoder through precision_vjp and prepare_vjp)
        k = glob_names.index(n)
        assert not torch.equal(before[:, k], after[:, k]), n
