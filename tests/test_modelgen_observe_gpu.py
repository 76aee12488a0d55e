"""GPU tests of a generated model's own observation map (GeneratedOdeModel.observe, OBS_CUSTOM in the kernels): the default
map through both routes, inducer_constant_precisions restated against the built-in kernels and its reference fixture, a map
with parameters against its own definition in float64, the evaluation summaries, and the summaries kernel's refusal.

Shapes: B=3, S=5 (15 trajectories: one partly filled wavefront, the adjoint's tail lanes shadow the last trajectory) and
B=5, S=26 (130: three 64-thread blocks, the last with 2 live lanes, data rows that straddle block boundaries), T=7 on a
non-uniform grid."""
import ctypes

import pytest
import torch

from fixture_util import Fixture, rel_err
from oracle import vihds_oracle as O
from vihds import hip, modelgen, ops

import hip_util as H
import modelgen_models as MM
import modelgen_observe_models as OM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXED = ["modeuler", "modeulerwhile", "euler", "midpoint", "rk4"]
SHAPES = [(3, 5), (5, 26)]
TIMES = [0.0, 0.4, 0.6, 1.5, 2.1, 3.3, 3.7]  # (steps 0.2 .. 1.2: inside every scheme's stability region for these rates)
_KEYS = {}


def _key(cls, neural):
    """Every model is registered once per module."""
    if cls not in _KEYS:
        modelgen.register_kernel(cls, neural)
        _KEYS[cls] = cls.model_key
    return _KEYS[cls]


def _run(spec, th, cond, times, obs, weights, upstream=False):
    """forward + adjoint of one launch pair: random upstream gradients on the log-likelihood and, `upstream`, on x_predict
    and the trajectory too."""
    th = th.detach().clone().requires_grad_(True)
    w = None if weights is None else weights.detach().clone().requires_grad_(True)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, cond, times, obs, None, w)
    gen = torch.Generator(device=DEV).manual_seed(5)
    loss = (logp * torch.randn(logp.shape, device=DEV, generator=gen)).sum()
    if upstream:
        loss = loss + (xpred * torch.randn(xpred.shape, device=DEV, generator=gen)).sum()
        loss = loss + (traj * torch.randn(traj.shape, device=DEV, generator=gen)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return traj.detach(), xpred.detach(), logp.detach(), th.grad, (None if w is None else w.grad)


def _agree(got, ref, rows, neural, tol=1e-5):
    assert rel_err(H.view_bsnt(got[0]), H.view_bsnt(ref[0])) < tol
    assert rel_err(H.view_bsnt(got[1]), H.view_bsnt(ref[1])) < tol
    assert rel_err(H.view_bs4(got[2]), H.view_bs4(ref[2]), dim=2) < tol
    assert rel_err(got[3][rows], ref[3][rows], dim=0) < tol
    if neural:
        assert rel_err(got[4], ref[4]) < tol


def _spread(base, B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: (v * torch.exp(0.2 * torch.randn(B, S, generator=gen, dtype=torch.float64))) for k, v in base.items()}


PRPR_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "dcfp": 0.25, "aYFP_PR": 1.2, "aCFP_PR": 0.9,
             "a530": 0.4, "a480": 0.3, "init_x": 0.01, "init_rfp": 0.1, "init_yfp": 0.1, "init_cfp": 0.1,
             "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0,
             "init_prec_x": 10.0, "init_prec_rfp": 10.0, "init_prec_yfp": 10.0, "init_prec_cfp": 10.0}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("solver", FIXED + ["dopri5"])
@pytest.mark.parametrize("prec", ["constant", "neural_h0", "neural_h3"])
def test_the_default_map_through_both_routes(solver, prec, shape):
    """PrprRestated (observe_kind "default": the kernels' fixed map) and its subclass that writes the same map as its own
    observe (OBS_CUSTOM: the struct's members): trajectory, x_predict, log-likelihood, g_theta and g_weights agree to 1e-5,
    with upstream gradients on all three outputs.  dopri5: one accepted grid handed to both."""
    B, S = shape
    neural = prec != "constant"
    hidden = 3 if prec == "neural_h3" else 0
    fixed_key = _key(MM.PrprRestatedPrecisions if neural else MM.PrprRestated, neural)
    own_key = _key(OM.PrprOwnMapPrecisions if neural else OM.PrprOwnMap, neural)
    slots = hip.model_slots(fixed_key)
    assert slots == hip.model_slots(own_key)
    row_of = {n: i for i, n in enumerate(slots)}
    th64 = _spread(PRPR_BASE, B, S, 3)
    th = torch.stack([th64[n] for n in slots]).float().to(DEV)
    cond = torch.zeros((B, 1), device=DEV)  # (prpr_constant reads no treatment)
    times = torch.tensor(TIMES, device=DEV)
    gen = torch.Generator().manual_seed(4)
    obs = (0.05 + torch.rand(B, 4, len(TIMES), generator=gen)).to(DEV)
    mk = lambda key: ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=1, n_hidden_prec=hidden)  # noqa: E731
    fixed_spec, own_spec = mk(fixed_key), mk(own_key)
    weights = None
    if neural:
        n_w = hip.lib().vihds_model_n_weights(fixed_spec.bind(B, S, len(TIMES)))
        assert n_w == hip.lib().vihds_model_n_weights(own_spec.bind(B, S, len(TIMES))) > 0
        weights = 0.3 * torch.randn(n_w, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    if solver == "dopri5":
        grid, _ = ops.adaptive_grid(fixed_spec, th, cond, times, None, weights)
        grid_own, _ = ops.adaptive_grid(own_spec, th, cond, times, None, weights)  # (the custom-map model's controller runs)
        assert grid_own.shape[0] >= times.shape[0] and bool(torch.isfinite(grid_own).all())
        times = grid.to(DEV)
        obs = torch.zeros((B, 4, times.shape[0]), device=DEV)
    ref = _run(fixed_spec, th, cond, times, obs, weights, upstream=True)
    got = _run(own_spec, th, cond, times, obs, weights, upstream=True)
    _agree(got, ref, sorted(set(row_of[s] for s in own_spec.slots)), neural)


def test_inducer_constant_restated_against_the_builtin_and_its_fixture():
    """inducer_constant_precisions, whose map [OD, OD*RFP, OD*(YFP+F530), OD*F480] is neither fixed kind a generated model
    can name, restated with observe: against the built-in kernels (kernel_variant=1) all five outputs within 1e-5, and the
    log-likelihood within 1e-4 of the reference fixture."""
    fx = Fixture("inducer_constant_precisions_tiny_modeuler")
    key = _key(OM.InducerRestated, True)
    th, row_of = H.pack_theta(fx, DEV)
    cond, times, obs = fx.t("inputs", DEV), fx.t("times", DEV), fx.t("observations", DEV)
    ref_spec = H.spec_for(fx, row_of, th.shape[0], kernel_variant=1)
    assert ref_spec.model == "inducer_constant_precisions"
    gen_spec = ops.OdeProblemSpec(key, fx.solver, row_of, th.shape[0], C=cond.shape[1], D=ref_spec.proto.D,
                                  n_hidden_prec=ref_spec.proto.n_hidden_prec)
    assert gen_spec.slots == ref_spec.slots
    prec_w, _, _ = fx.decoder_weights(DEV)
    order = (("hid_w", "hid_b") if "hid_w" in prec_w else ()) + ("prod_w", "prod_b", "degr_w", "degr_b")
    weights = torch.cat([prec_w[k].reshape(-1) for k in order])
    ref = _run(ref_spec, th, cond, times, obs, weights)
    got = _run(gen_spec, th, cond, times, obs, weights)
    _agree(got, ref, sorted(set(row_of[s] for s in gen_spec.slots)), True)
    for name, out in (("built-in", ref), ("generated", got)):
        e = rel_err(H.view_bs4(out[2]), fx.t("log_p_by_species"), dim=2)
        print("%s log-likelihood against the fixture: %.2e" % (name, e))
        assert e < 1e-4, name


READER_BASE = {"r": 1.0, "K": 2.0, "tlag": 0.8, "rc": 0.8, "drfp": 0.2, "dyfp": 0.3, "aYFP": 1.2, "gain_r": 1.5, "bg_r": 0.05,
               "sat": 0.6, "auto": 0.3, "leak": 0.4, "init_x": 0.05, "init_rfp": 0.1, "init_yfp": 0.1,
               "prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
OBSERVE_ONLY = ("gain_r", "bg_r", "sat", "auto", "leak")
_READER_REF = {}


def _reader_problem(B, S):
    gen = torch.Generator().manual_seed(7)
    th64 = _spread(READER_BASE, B, S, 6)
    assert bool((th64["leak"] > 0.5).any()) and bool((th64["leak"] < 0.5).any())  # (clamp(leak, 0, 0.5): both sides)
    cond = torch.log1p(2.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64))
    times = torch.tensor(TIMES, dtype=torch.float64)
    with torch.no_grad():
        th_obs = {k: v[:, :1] for k, v in th64.items()}
        rhs, x0 = OM.PlateReader.torch_problem(th_obs, cond)
        xp = OM.PlateReader.torch_observe(O.simulate(rhs, x0, times, "rk4"), th_obs, cond)[:, 0]
        obs = xp * (1.0 + 0.05 * torch.randn(B, 4, len(TIMES), generator=gen, dtype=torch.float64))
    G = {"logp": torch.randn(B, S, 4, generator=gen, dtype=torch.float64),
         "xpred": torch.randn(B, S, 4, len(TIMES), generator=gen, dtype=torch.float64),
         "traj": torch.randn(B, S, 3, len(TIMES), generator=gen, dtype=torch.float64)}
    return th64, cond, times, obs, G


def _reader_oracle(B, S, solver, upstream, dtype):
    """torch_problem + torch_observe integrated by the oracle's step functions (computed once per case and dtype)."""
    k = (B, S, solver, upstream, dtype)
    if k not in _READER_REF:
        th64, cond, times, obs, G = _reader_problem(B, S)
        th = {n: v.to(dtype).detach().clone().requires_grad_(True) for n, v in th64.items()}
        rhs, x0 = OM.PlateReader.torch_problem(th, cond.to(dtype))
        xs = O.simulate(rhs, x0, times.to(dtype), solver)
        xp = OM.PlateReader.torch_observe(xs, th, cond.to(dtype))
        lpo = O.log_prob_observations(xp, obs.to(dtype), O.expand_constant_precisions(th, len(TIMES)))
        loss = (lpo * G["logp"].to(dtype)).sum()
        if upstream:
            loss = loss + (xp * G["xpred"].to(dtype)).sum() + (xs * G["traj"].to(dtype)).sum()
        loss.backward()
        _READER_REF[k] = (xp.detach(), lpo.detach(), {n: v.grad for n, v in th.items()})
    return _READER_REF[k]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("solver", ["rk4", "modeuler"])
@pytest.mark.parametrize("upstream", [False, True])
def test_a_map_with_parameters_against_its_own_definition_in_float64(solver, upstream, shape):
    """PlateReader: gain, offset, saturation, a treatment and a clamped parameter read by observe only.  x_predict, the
    log-likelihood and every row of g_theta against torch_problem + torch_observe in float64, within max(floor, 8x the
    float32 oracle's own error) -- the bounds of test_generated_receiver_against_its_own_definition_in_float64 (floor 1e-6
    for values, 1e-4 for gradients).  `upstream`: gradients arrive on x_predict and on the trajectory as well, so the
    injection goes through observe_vjp."""
    B, S = shape
    key = _key(OM.PlateReader, False)
    th64, cond, times, obs, G = _reader_problem(B, S)
    xp64, lp64, g64 = _reader_oracle(B, S, solver, upstream, torch.float64)
    xp32, lp32, g32 = _reader_oracle(B, S, solver, upstream, torch.float32)
    slots = hip.model_slots(key)
    row_of = {n: i for i, n in enumerate(slots)}
    th = torch.stack([th64[n] for n in slots]).float().to(DEV).requires_grad_(True)
    spec = ops.OdeProblemSpec(key, solver, row_of, th.shape[0], C=1)
    traj, xpred, logp = ops.OdeSolveObserve.apply(spec, th, cond.float().to(DEV), times.float().to(DEV), obs.float().to(DEV),
                                                  None, None)
    loss = (H.view_bs4(logp) * G["logp"].float().to(DEV)).sum()
    if upstream:
        loss = loss + (H.view_bsnt(xpred) * G["xpred"].float().to(DEV)).sum()
        loss = loss + (H.view_bsnt(traj) * G["traj"].float().to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    e, e32 = rel_err(H.view_bsnt(xpred), xp64), rel_err(xp32, xp64)
    print("%s upstream=%s n=%d: x_predict %.2e (fp32 oracle %.2e)" % (solver, upstream, B * S, e, e32))
    assert e <= max(1e-6, 8 * e32)
    e, e32 = rel_err(H.view_bs4(logp), lp64, dim=2), rel_err(lp32, lp64, dim=2)
    print("%s upstream=%s n=%d: log-likelihood %.2e (fp32 oracle %.2e)" % (solver, upstream, B * S, e, e32))
    assert e <= max(1e-6, 8 * e32)
    for n in OBSERVE_ONLY:  # (the comparison of their rows is not vacuous)
        assert g64[n] is not None and float(g64[n].abs().max()) > 0.0, n
    inside = th64["leak"] <= 0.5
    assert bool((g64["leak"][~inside] == 0).all()) and bool((g64["leak"][inside] != 0).all())
    for n in slots:
        ref = g64[n]
        assert ref is not None, n
        ge, ge32 = rel_err(th.grad[row_of[n]].cpu(), ref), rel_err(g32[n], ref)
        print("  d/d%-8s %.2e (fp32 oracle %.2e)" % (n, ge, ge32))
        assert ge <= max(1e-4, 8 * ge32), (n, ge, ge32)


def test_evaluation_summaries_of_a_custom_map(monkeypatch):
    """A spec naming the restated inducer model: the forward launch of an evaluation pass stores x_predict (never the lazy
    form), Training.cost(full_output=...) forms its summaries from that buffer, and they equal the plain torch formula of
    training.py applied to the stored buffers within 1e-5 -- as does cost's fallback branch, handed the three tensors.
    OdeModel.observe on another tensor evaluates the map with torch ops; Training.evaluate runs."""
    import numpy as np
    import e2e_util as E
    import models
    from test_modelgen_gpu import _build_named

    cls = OM.InducerRestated
    monkeypatch.setitem(models.LOOKUP, cls.model_key, cls)
    fx = Fixture("inducer_constant_precisions_tiny_modeuler")
    args, settings, model, training = _build_named(fx, cls.model_key, hip_graph=False)
    ode = model.decoder.ode_model
    assert isinstance(ode, cls) and ode.observe_kind == "custom"
    model.eval()
    batch = E.batch_from_fixture(fx, settings.device)
    with torch.no_grad():
        results, theta, q, p = model(batch, fx.S)
        elbo, summ = training.cost(batch, results, theta, q, p, full_output="device")
        sol = results.solution
        assert sol.has_x_predict, "a custom-map model took the lazy x_predict path"
        x_states, precisions = ode.expand_precisions(theta, batch.times, sol.sol)
        x_predict = sol.x_predict
        _, log_w, lse = ops.iwae_loss(sol.logp_buffer, p.log_prob(theta), q.log_prob(theta))
        w = (log_w - lse[:, None]).exp()[:, :, None, None]
        mu = (w * x_predict).sum(1)
        plain = (mu, ((w * (x_predict ** 2 + 1.0 / precisions)).sum(1) - mu ** 2).sqrt(), (w * x_states).sum(1),
                 (w / precisions).sum(1))
        for name, a, b in zip(("iw_predict_mu", "iw_predict_std", "iw_states", "iw_variance"), summ, plain):
            assert rel_err(a, b, dim=1) < 1e-5, name
        elbo_f, summ_f = training.cost(batch, (x_states, x_predict, precisions), theta, q, p, full_output="device")
        assert abs(float(elbo_f) - float(elbo)) <= 1e-5 * abs(float(elbo))
        for name, a, b in zip(("iw_predict_mu", "iw_predict_std", "iw_states", "iw_variance"), summ_f, plain):
            assert rel_err(a, b, dim=1) < 1e-5, name
        # the map with torch ops on a tensor that is not the last solution (theta and treatments of the last solve)
        again = ode.observe(sol.sol.clone(), theta)
        assert again.shape == x_predict.shape and rel_err(again, x_predict) < 1e-5
        # without the stored buffer the summaries kernel would have to form the map itself: it refuses
        with pytest.raises(RuntimeError, match="passes its stored x_predict"):
            ops.iw_summaries(log_w, lse, sol.traj_buffer, None, sol.traj_buffer.shape[1] - 4, observe_kind="custom")
    res = training.evaluate(training.train_data, fx.S)
    T = fx.z["times"].shape[0]
    assert res.iw_predict_mu.shape == (fx.B, 4, T) and res.iw_states.shape == (fx.B, len(cls.species), T)
    assert np.isfinite(res.iw_predict_mu).all() and np.isfinite(res.iw_states).all() and np.isfinite(float(res.elbo))


def test_the_states_summaries_refuse_a_custom_map():
    """vihds_iw_summaries_states forms the observed signals from the states by one of the fixed maps; VIHDS_OBS_CUSTOM is
    VIHDS_E_BADARG with a message that says where such a model's x_predict comes from."""
    assert ops.OBSERVE_KINDS["custom"] == 3
    B, S, T, N = 2, 4, 3, 6
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    rows = (ctypes.c_int * 4)(0, 1, 2, 3)
    out = [z(B, 4, T), z(B, 4, T), z(B, N, T), z(B, 4, T)]
    L = hip.lib()
    rc = L.vihds_iw_summaries_states(B, S, T, N, N, 3, hip.ptr(z(B, S)), hip.ptr(z(B)), hip.ptr(z(T, N, B, S)),
                                     hip.ptr(z(4, B, S)), rows, hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(out[2]),
                                     hip.ptr(out[3]), hip.current_stream())
    assert rc == -1  # VIHDS_E_BADARG
    msg = L.vihds_last_error().decode()
    assert "VIHDS_OBS_CUSTOM" in msg and "passes its stored x_predict" in msg
