"""Pin the CPU oracle (oracle/vihds_oracle.py) against outputs of the reference itself.

The fixtures under tests/golden/ were produced by running /root/reference (see make_fixtures.py for the
exact provenance).  Everything here is CPU-only and exact-or-nearly-exact: the oracle restates the same
fp32 op sequence, so forward values agree to rounding of BLAS/reduction order only."""
import pytest
import torch

from fixture_util import ALL_FIXTURES as _PINNED, PATCHED_FIXTURES, Fixture, rel_err
from oracle import vihds_oracle as O

ALL_FIXTURES = _PINNED + PATCHED_FIXTURES  # the second list: the MODIFIED reference (fixture_util.PATCHED_FIXTURES)


def _blackbox_kwargs(fx, th, prec_w, states_w):
    p = fx.cfg["params"]
    return dict(dev_1hot=fx.t("dev_1hot"), states_w=states_w, prec_w=prec_w, n_x=p["n_x"], n_y=p["n_y"], n_z=p["n_z"],
                n_latent_species=p["n_latent_species"], init_latent_species=p["init_latent_species"],
                init_prec=p["init_prec"])


def _run_oracle(fx, th):
    prec_w, states_w, offset = fx.decoder_weights()
    for w in (prec_w, states_w):
        if w:
            for v in w.values():
                v.requires_grad_(True)
    qm, qp = fx.q_params()
    pm, pp = fx.p_params()
    th_sim = th
    blackbox = None
    if fx.model == "dr_blackbox":
        # condition_theta (dr_blackbox.py:86-96) re-binds the y attributes only: the ODE sees y + offset,
        # log q / log p (which iterate theta.samples) still see the un-offset y.
        th_sim = dict(th)
        ow, ob = offset
        ow.requires_grad_(True), ob.requires_grad_(True)
        off = torch.nn.functional.linear(fx.t("dev_1hot").unsqueeze(1).repeat([1, fx.S, 1]), ow, ob)
        for i in range(fx.cfg["params"]["n_y"]):
            th_sim["y%d" % (i + 1)] = th["y%d" % (i + 1)] + off[:, :, i]
        blackbox = _blackbox_kwargs(fx, th_sim, prec_w, states_w)
    xs, xp, prec = O.decode(fx.model, th_sim, fx.t("inputs"), fx.t("times"), fx.solver, prec_w=prec_w,
                            blackbox=blackbox)
    lpo = O.log_prob_observations(xp, fx.t("observations"), prec)
    vals = [th[n] for n in fx.names]
    log_q = O.chained_log_prob(fx.kinds, qm, qp, vals)
    log_p = O.chained_log_prob(fx.kinds, pm, pp, vals)
    loss, log_w = O.iwae_loss(lpo, log_p, log_q)
    return dict(xs=xs, xp=xp, prec=prec, lpo=lpo, log_q=log_q, log_p=log_p, loss=loss, prec_w=prec_w,
                states_w=states_w, offset=offset)


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_sample_and_clip_match_reference(name):
    fx = Fixture(name)
    qm, qp = fx.q_params()
    pm, pp = fx.p_params()
    th = O.sample_clip_theta(fx.names, fx.kinds, qm, qp, pm, pp, fx.t("u"))
    got = torch.stack([th[n] for n in fx.names])
    ref = fx.t("theta")
    # exp / sqrt of identical fp32 inputs: identical up to libm ulp differences between runs
    assert rel_err(got, ref) < 1e-6
    assert torch.allclose(got, ref, rtol=2e-6, atol=0)


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_forward_matches_reference(name):
    fx = Fixture(name)
    th = fx.theta_dict()
    with torch.no_grad():
        out = _run_oracle(fx, th)
    st = int(fx.z["sample_stride"])
    assert rel_err(out["xs"][:, ::st], fx.t("x_states")) < 1e-5
    assert rel_err(out["xp"][:, ::st], fx.t("x_predict")) < 1e-5
    assert rel_err(out["prec"][:, ::st], fx.t("precisions")) < 1e-5
    assert rel_err(out["xs"].double().sum(1), fx.t("x_states_sum_over_samples", dtype=torch.float64), dim=1) < 1e-5
    assert rel_err(out["lpo"], fx.t("log_p_by_species"), dim=2) < 1e-5
    assert rel_err(out["log_q"], fx.t("log_q")) < 1e-5
    assert rel_err(out["log_p"], fx.t("log_p")) < 1e-5
    assert rel_err(out["loss"], fx.t("loss")) < 1e-5


@pytest.mark.parametrize("name", [n for n in ALL_FIXTURES if "full" not in n])
def test_theta_and_weight_gradients_match_reference(name):
    fx = Fixture(name)
    th = fx.theta_dict(requires_grad=True)
    out = _run_oracle(fx, th)
    out["loss"].backward()
    got = torch.stack([th[n].grad if th[n].grad is not None else torch.zeros_like(th[n]) for n in fx.names])
    # Constant-kind entries (init_x ...) carry no grad in the reference (distributions.py:241-242)
    live = torch.tensor([k != O.CONSTANT for k in fx.kinds])
    assert rel_err(got[live], fx.t("theta_grad")[live], dim=0) < 2e-4
    ref = fx.decoder_weight_grads()
    key = {"prod_w": "prec_production.weight", "prod_b": "prec_production.bias", "degr_w": "prec_degradation.weight",
           "degr_b": "prec_degradation.bias", "hid_w": "prec_hidden.weight", "hid_b": "prec_hidden.bias"}
    if out["prec_w"]:
        for k, v in out["prec_w"].items():
            assert rel_err(v.grad, ref["ode_model.precisions." + key[k]]) < 2e-4
    if out["states_w"]:
        skey = {"prod_w": "states_production.weight", "prod_b": "states_production.bias",
                "degr_w": "states_degradation.weight", "degr_b": "states_degradation.bias",
                "hid_w": "states_hidden.weight", "hid_b": "states_hidden.bias"}
        for k, v in out["states_w"].items():
            assert rel_err(v.grad, ref["ode_model.neural_states." + skey[k]]) < 2e-4
        assert rel_err(out["offset"][0].grad, ref["ode_model.offset_layer.weight"]) < 2e-4


@pytest.mark.parametrize("name", ["dr_constant_icml_tiny_modeuler", "dr_blackbox_icml_tiny_modeuler",
                                  "dr_constant_one_s5_modeulerwhile"])
def test_q_parameter_gradients_match_reference(name):
    """d loss / d (mu, log_prec) of q through sample -> clip -> decode -> cost."""
    fx = Fixture(name)
    qm0 = fx.t("q_mu")
    qlp0 = fx.t("q_prec").log()
    qm_leaf = qm0.clone().requires_grad_(True)
    qlp_leaf = qlp0.clone().requires_grad_(True)
    P = len(fx.names)
    qm = [qm_leaf[i][:, None] for i in range(P)]
    qp = [qlp_leaf[i][:, None].exp() for i in range(P)]
    pm, pp = fx.p_params()
    th = O.sample_clip_theta(fx.names, fx.kinds, qm, qp, pm, pp, fx.t("u"))
    if fx.extra_names:
        ex = fx.t("extra_theta")
        for i, n in enumerate(fx.extra_names):
            th[n] = ex[i]
    prec_w, states_w, offset = fx.decoder_weights()
    th_sim, blackbox = th, None
    if fx.model == "dr_blackbox":
        th_sim = dict(th)
        off = torch.nn.functional.linear(fx.t("dev_1hot").unsqueeze(1).repeat([1, fx.S, 1]), *offset)
        for i in range(fx.cfg["params"]["n_y"]):
            th_sim["y%d" % (i + 1)] = th["y%d" % (i + 1)] + off[:, :, i]
        blackbox = _blackbox_kwargs(fx, th_sim, prec_w, states_w)
    xs, xp, prec = O.decode(fx.model, th_sim, fx.t("inputs"), fx.t("times"), fx.solver, prec_w=prec_w, blackbox=blackbox)
    lpo = O.log_prob_observations(xp, fx.t("observations"), prec)
    vals = [th[n] for n in fx.names]
    loss, _ = O.iwae_loss(lpo, O.chained_log_prob(fx.kinds, pm, pp, vals), O.chained_log_prob(fx.kinds, qm, qp, vals))
    loss.backward()
    glob = fx.t("q_is_global").bool()
    gm, gl = qm_leaf.grad.clone(), qlp_leaf.grad.clone()
    # fixture stores the TOTAL grad for global (size-1) q tensors, broadcast over B
    gm[glob] = gm[glob].sum(1, keepdim=True).expand(-1, fx.B)
    gl[glob] = gl[glob].sum(1, keepdim=True).expand(-1, fx.B)
    live = torch.tensor([k != O.CONSTANT for k in fx.kinds])
    assert rel_err(gm[live], fx.t("q_mu_grad")[live], dim=0) < 2e-4
    assert rel_err(gl[live], fx.t("q_logprec_grad")[live], dim=0) < 2e-4


def test_config3_training_shape_against_the_reference():
    """BASELINE config 3's training shape -- 36 rows x 1 000 importance samples -- recorded from the reference itself
    (tests/golden/dr_constant_icml_s1000_light_modeuler.npz: the four sample-sized input arrays are left out; u is the
    reference's own draw regenerated from the recorded seed).  u -> sample / clip -> decode -> cost: log q, log p, the
    log-likelihoods, every 125th sample's trajectory, the loss and d loss / d (mu, log_prec) of q."""
    from fixture_util import LIGHT_FIXTURE_S1000

    fx = Fixture(LIGHT_FIXTURE_S1000)
    assert (fx.B, fx.S) == (36, 1000)
    qm_leaf = fx.t("q_mu").clone().requires_grad_(True)
    qlp_leaf = fx.t("q_prec").log().clone().requires_grad_(True)
    P = len(fx.names)
    qm = [qm_leaf[i][:, None] for i in range(P)]
    qp = [qlp_leaf[i][:, None].exp() for i in range(P)]
    pm, pp = fx.p_params()
    th = O.sample_clip_theta(fx.names, fx.kinds, qm, qp, pm, pp, fx.t("u"))
    ex = fx.t("extra_theta")
    for i, n in enumerate(fx.extra_names):
        th[n] = ex[i]
    xs, xp, prec = O.decode(fx.model, th, fx.t("inputs"), fx.t("times"), fx.solver)
    lpo = O.log_prob_observations(xp, fx.t("observations"), prec)
    vals = [th[n] for n in fx.names]
    log_p, log_q = O.chained_log_prob(fx.kinds, pm, pp, vals), O.chained_log_prob(fx.kinds, qm, qp, vals)
    loss, _ = O.iwae_loss(lpo, log_p, log_q)
    st = int(fx.z["sample_stride"])
    assert rel_err(xs.detach()[:, ::st], fx.t("x_states")) < 1e-5
    assert rel_err(xp.detach()[:, ::st], fx.t("x_predict")) < 1e-5
    assert rel_err(xs.detach().double().sum(1), fx.t("x_states_sum_over_samples", dtype=torch.float64), dim=1) < 1e-5
    assert rel_err(lpo.detach(), fx.t("log_p_by_species"), dim=2) < 1e-5
    assert rel_err(log_q.detach(), fx.t("log_q")) < 1e-5
    assert rel_err(log_p.detach(), fx.t("log_p")) < 1e-5
    assert rel_err(loss.detach(), fx.t("loss")) < 1e-5
    loss.backward()
    glob = fx.t("q_is_global").bool()
    gm, gl = qm_leaf.grad.clone(), qlp_leaf.grad.clone()
    gm[glob] = gm[glob].sum(1, keepdim=True).expand(-1, fx.B)
    gl[glob] = gl[glob].sum(1, keepdim=True).expand(-1, fx.B)
    live = torch.tensor([k != O.CONSTANT for k in fx.kinds])
    assert rel_err(gm[live], fx.t("q_mu_grad")[live], dim=0) < 2e-4
    assert rel_err(gl[live], fx.t("q_logprec_grad")[live], dim=0) < 2e-4


def test_unpinned_solvers_meet_reference_cv_criterion():
    """tests/test_ode_solvers.py:83-89 of the reference: final state across solvers within 5 % CV.
    midpoint/rk4/euler are restated from torchdiffeq==0.1 (absent) -- this is the only reference-anchored
    check available for them; parity otherwise unpinned."""
    fx = Fixture("dr_constant_one_s5_modeulerwhile")
    th = fx.theta_dict()
    finals = []
    with torch.no_grad():
        for solver in ["modeuler", "modeulerwhile", "midpoint", "rk4"]:
            xs, _, _ = O.decode(fx.model, th, fx.t("inputs"), fx.t("times"), solver)
            finals.append(xs[:, :, :, -1])
    sol = torch.stack(finals).double()
    ok = sol.mean(0).abs() > 1e-8
    cv = (sol.std(0, unbiased=False) / sol.mean(0))[ok]
    assert float(cv.abs().max()) < 0.05


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_importance_weighted_summaries_match_reference(name):
    """Results.init (reference utils.py:79-99 via Training.cost(full_output=True)): pins
    oracle.importance_weighted_summaries, the checker of vihds_iw_summaries."""
    fx = Fixture(name)
    with torch.no_grad():
        out = _run_oracle(fx, fx.theta_dict())
        log_w = out["lpo"].sum(2) + out["log_p"] - out["log_q"]
        mu, std, states, var = O.importance_weighted_summaries(log_w, out["xp"], out["xs"], out["prec"])
    assert rel_err(mu, fx.t("iw_predict_mu"), dim=1) < 1e-5
    assert rel_err(states, fx.t("iw_states"), dim=1) < 1e-5
    assert rel_err(var, fx.t("iw_variance"), dim=1) < 1e-5
    ref_std = fx.t("iw_predict_std")
    ok = torch.isfinite(ref_std) & torch.isfinite(std)  # (sqrt of a rounding-negative difference is NaN in both)
    assert ok.float().mean() > 0.9
    assert float(((std - ref_std)[ok]).abs().max() / ref_std[ok].abs().max()) < 1e-3


@pytest.mark.parametrize("solver", ["dopri5", "bosh3", "adaptive_heun", "dopri8"])
def test_adaptive_oracle_solvers_agree_with_the_pinned_scheme(solver):
    """The oracle's restatement of torchdiffeq's adaptive pairs (parity unpinned: the dependency is absent) against the
    pinned modified-Euler fixture, by the reference's own criterion (tests/test_ode_solvers.py:83-89: final states within
    5 %), and against a finely resolved rk4 solution to the tolerance asked for; the accepted grid contains every output
    time."""
    fx = Fixture("dr_constant_icml_tiny_modeuler")
    th = fx.theta_dict()
    rhs, x0 = O.MODEL_TABLE[fx.model][0](th, fx.t("inputs"))
    rtol, atol = (1e-6, 1e-8) if solver in ("dopri5", "dopri8") else (1e-4, 1e-6)
    grid, index = O.adaptive_grid(solver, rhs, x0, fx.t("times"), rtol, atol)
    assert [float(torch.tensor(grid[i], dtype=torch.float32)) for i in index] == [float(v) for v in fx.t("times")]
    assert all(b > a for a, b in zip(grid, grid[1:]))
    sol = O.simulate(rhs, x0, fx.t("times"), solver, grid=(grid, index))  # [B,S,N,T]
    assert rel_err(sol[..., -1], fx.t("x_states")[..., -1], dim=2) < 0.05
    t = fx.t("times").double()
    fine = torch.cat([(t[:-1, None] + (t[1:, None] - t[:-1, None]) * torch.arange(16).double()[None] / 16).reshape(-1), t[-1:]])
    th64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in th.items()}
    rhs64, x064 = O.MODEL_TABLE[fx.model][0](th64, fx.t("inputs").double())
    ref = O.simulate(rhs64, x064, fine, "rk4")[..., ::16].float()
    assert rel_err(sol, ref) < (5e-4 if solver in ("dopri5", "dopri8") else 5e-3)  # (rtol 1e-6 / 1e-4; per-species max-norm)


# ---------------------------------------------------------------------------------------------------------------
# the committed fixture recipe itself (run_training_trace referenced a name that was not in scope)
def _load_recipe():
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_fixtures.py")
    spec = importlib.util.spec_from_file_location("make_fixtures", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, path


def test_fixture_recipe_has_no_unbound_names():
    """Every function of tests/golden/make_fixtures.py compiles and only reads names that are parameters, locals,
    module globals or builtins (the defect was a NameError at run time, invisible to an import)."""
    import builtins
    import inspect

    mod, _ = _load_recipe()
    sig = inspect.signature(mod.run_training_trace)
    assert "params_override" in sig.parameters and sig.parameters["params_override"].default is None
    assert "params_override" in inspect.signature(mod.run_case).parameters
    for name, fn in inspect.getmembers(mod, inspect.isfunction):
        if fn.__module__ != mod.__name__:
            continue
        stack = [fn.__code__]
        while stack:  # nested functions / lambdas / comprehensions too
            code = stack.pop()
            stack += [c for c in code.co_consts if inspect.iscode(c)]
            for g in code.co_names:
                if g in code.co_varnames or g in code.co_freevars or g in code.co_cellvars:
                    continue
                ok = hasattr(builtins, g) or g in vars(mod)
                # attribute names and imported-module members also live in co_names: only flag what looks like a bare
                # global read, i.e. a name some LOAD_GLOBAL instruction refers to
                if not ok:
                    import dis

                    loads = {i.argval for i in dis.get_instructions(code) if i.opname == "LOAD_GLOBAL"}
                    assert g not in loads, "%s reads the undefined global %r" % (name, g)


@pytest.mark.parametrize("solver", ["dopri5", "bosh3", "adaptive_heun"])
def test_dependency_algorithm_steps_past_output_times_and_interpolates(solver):
    """`odeint_adaptive`: the restatement of torchdiffeq 0.1's own adaptive driver (no clipping to the output times; the
    quartic `_interp_fit` interpolant of the accepted step that contains an output time).  Properties of that algorithm:
    it takes fewer accepted steps than the output grid forces on a clipped controller when the tolerance is loose; its
    solution still meets the tolerance against a finely resolved rk4; the interpolant reproduces both ends of a step."""
    fx = Fixture("dr_constant_icml_tiny_modeuler")
    th = fx.theta_dict()
    rhs, x0 = O.MODEL_TABLE[fx.model][0](th, fx.t("inputs"))
    rtol, atol = (1e-6, 1e-8) if solver == "dopri5" else (1e-4, 1e-6)
    sol, n_acc, n_rej = O.odeint_adaptive(solver, rhs, x0, fx.t("times"), rtol, atol)
    assert sol.shape[0] == fx.t("times").shape[0] and n_acc > 0
    grid, _ = O.adaptive_grid(solver, rhs, x0, fx.t("times"), rtol, atol)
    if solver == "dopri5":  # the 5th-order pair wants steps longer than the output spacing: clipping adds steps
        assert n_acc < len(grid) - 1, (n_acc, len(grid))
    t = fx.t("times").double()
    fine = torch.cat([(t[:-1, None] + (t[1:, None] - t[:-1, None]) * torch.arange(16).double()[None] / 16).reshape(-1), t[-1:]])
    th64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in th.items()}
    rhs64, x064 = O.MODEL_TABLE[fx.model][0](th64, fx.t("inputs").double())
    ref = O.simulate(rhs64, x064, fine, "rk4")[..., ::16].float()
    assert rel_err(sol.permute(1, 2, 3, 0), ref) < (5e-4 if solver == "dopri5" else 5e-3)
    y0, y1, f0, f1 = torch.randn(3), torch.randn(3), torch.randn(3), torch.randn(3)
    coef = O._interp_fit(y0, y1, 0.5 * (y0 + y1), f0, f1, 0.3)
    assert torch.allclose(O._interp_evaluate(coef, 1.0, 1.3, 1.0), y0, atol=1e-6)
    assert torch.allclose(O._interp_evaluate(coef, 1.0, 1.3, 1.3), y1, atol=1e-5)


@pytest.mark.parametrize("name", PATCHED_FIXTURES)
def test_rhs_forward_matches_the_modified_references_own_forward(name):
    """The first evaluation of Relay_Constant_RHS.forward / Degrader_Constant_RHS.forward / ... themselves (recorded by a
    forward hook in `make_fixtures.py --patched`: MODIFIED REFERENCE, construction defects repaired, equations untouched;
    models/relay_constant.py:91-134, degrader_constant.py:103-143, inducer_constant.py, prpr_constant.py) against the
    oracle's RHS closure on the recorded (t, state), and the initial state against initialize_state."""
    fx = Fixture(name)
    prec_w, _, _ = fx.decoder_weights()
    maker, _, neural = O.MODEL_TABLE[fx.model]
    assert neural
    rhs, x0 = maker(fx.theta_dict(), fx.t("inputs"), prec_w=prec_w)
    state = fx.t("rhs_state")
    assert torch.equal(x0, state)  # the integrators' first call is f(times[0], x0)
    assert float(fx.t("rhs_t")) == float(fx.t("times")[0])
    with torch.no_grad():
        out = rhs(fx.t("rhs_t"), state)
    assert rel_err(out, fx.t("rhs_out"), dim=2) < 1e-6


def test_patched_fixtures_say_so():
    for name in PATCHED_FIXTURES:
        assert str(Fixture(name).z["provenance"]).startswith("MODIFIED REFERENCE")
    for name in _PINNED:
        assert "MODIFIED REFERENCE" not in str(Fixture(name).z["provenance"])
