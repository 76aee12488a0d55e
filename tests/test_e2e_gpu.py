"""GPU end-to-end parity: the host package (Config -> Encoder -> fused theta kernel -> Decoder/fused ODE kernel
-> Training.cost -> backward) on the fixture's batch, with the reference's RNG streams (host numpy u, CPU-drawn
DeviceConditioner weights), against what the reference itself produced for the same seed: loss (= -ELBO),
trajectories, and d loss / d (every encoder parameter)."""
import os
import numpy as np
import pytest
import torch

from fixture_util import PATCHED_FIXTURES, Fixture, rel_err

pytestmark = pytest.mark.gpu

CASES = ["dr_constant_one_modeuler", "dr_constant_one_s5_modeulerwhile", "dr_constant_icml_tiny_modeuler",
         "dr_constant_icml_tiny_modeulerwhile", "dr_constant_icml_full_modeuler", "dr_constant_v2_tiny_modeuler",
         "auto_constant_tiny_modeuler", "prpr_constant_tiny_modeuler", "dr_constant_precisions_tiny_modeuler",
         "auto_constant_precisions_tiny_modeuler", "dr_blackbox_icml_tiny_modeuler",
         "dr_constant_precisions_hidden20_tiny_modeuler", "dr_blackbox_sized_tiny_modeuler", "dr_blackbox_icml_full_modeuler"]
# + the MODIFIED reference (construction defects repaired, fixture_util.PATCHED_FIXTURES): the relay / degrader / inducer /
# prpr *_precisions plugins end to end, BASELINE config 5's model among them
CASES = CASES + PATCHED_FIXTURES


def _ref_encoder_grads(fx, enc):
    """The reference's per-head gradients, arranged like the batched heads."""
    ref = {k[len("encoder_grad/"):]: fx.t(k) for k in fx.z.files if k.startswith("encoder_grad/")}
    out = {"conditional.conv.weight": ref["conditional.conv.weight"], "conditional.conv.bias": ref["conditional.conv.bias"],
           "conditional.lin.weight": ref["conditional.lin.weight"], "conditional.lin.bias": ref["conditional.lin.bias"]}
    if enc.local:
        w, b = [], []
        for free in ("mu", "log_prec"):  # heads are stored [all mu ; all log_prec]
            for d in enc.local:
                w.append(ref["q_local_defs.%s.layers.%s.weight" % (d.name, free)])
                b.append(ref["q_local_defs.%s.layers.%s.bias" % (d.name, free)])
        out["local_heads.weight"], out["local_heads.bias"] = torch.cat(w, 0), torch.cat(b, 0)
    if enc.gcond:
        out["gcond_heads.weight"] = torch.cat([ref["q_global_cond_defs.%s.layers.%s.weight" % (d.name, f)]
                                               for f in ("mu", "log_prec") for d in enc.gcond], 0)
    if enc.glob:
        out["global_free"] = torch.stack([torch.cat([ref["q_global_defs.%s.free_params.mu" % d.name],
                                                     ref["q_global_defs.%s.free_params.log_prec" % d.name]])
                                          for d in enc.glob]).t()
    return out


@pytest.mark.parametrize("name", CASES)
def test_training_step_matches_reference(name):
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture(name)
    args, settings, data, parameters = E.build_from_fixture(fx, gpu=0)
    model = build_model(args, settings, data, parameters)
    training = Training(args, settings, data, parameters, model)
    model.train()
    batch = E.batch_from_fixture(fx, settings.device)
    np.random.seed(fx.cfg["seed"] + 1)
    torch.manual_seed(fx.cfg["seed"] + 1)
    results, theta, q, p = model(batch, args.train_samples)
    x_states, x_predict, precisions = results
    loss = training.cost(batch, results, theta, q, p).elbo
    loss.backward()

    st = int(fx.z["sample_stride"])
    assert rel_err(torch.stack([theta.samples[n] for n in fx.names]), fx.t("theta"), dim=0) < 1e-5
    assert rel_err(x_states[:, ::st], fx.t("x_states")) < 1e-4
    assert rel_err(x_predict[:, ::st], fx.t("x_predict")) < 1e-4
    assert rel_err(precisions[:, ::st], fx.t("precisions")) < 1e-5
    assert rel_err(q.log_prob(theta), fx.t("log_q")) < 1e-4
    assert rel_err(p.log_prob(theta), fx.t("log_p")) < 1e-4
    assert rel_err(loss, fx.t("loss")) < 1e-4
    ref = _ref_encoder_grads(fx, model.encoder)
    got = dict(model.encoder.named_parameters())
    for k, g in ref.items():
        assert rel_err(got[k].grad, g) < 1e-3, k
    dref = {k[len("decoder_grad/"):]: fx.t(k) for k in fx.z.files if k.startswith("decoder_grad/")}
    for k, v in model.decoder.named_parameters():  # neural-precision weights
        assert rel_err(v.grad, dref[k]) < 1e-3, k


def test_reference_api_compat_paths():
    """q.sample / p.clip / q.log_prob / simulate / observe / expand_precisions used one by one (the call sequence
    of the reference's tests/test_ode_solvers.py:58-66) give the same numbers as the fused path."""
    import e2e_util as E
    from vihds.training import log_prob_observations
    from vihds.vae import build_model

    fx = Fixture("dr_constant_icml_tiny_modeuler")
    args, settings, data, parameters = E.build_from_fixture(fx, gpu=0)
    model = build_model(args, settings, data, parameters)
    model.n_theta = len(fx.names)
    batch = E.batch_from_fixture(fx, settings.device)
    q = model.encoder(batch)
    theta = q.sample(fx.t("u"), model.device)
    assert rel_err(torch.stack(theta.get_tensors()), fx.t("theta_unclipped"), dim=0) < 1e-5
    clipped = model.encoder.p.clip(theta, stddevs=4)
    assert rel_err(torch.stack(clipped.get_tensors()), fx.t("theta"), dim=0) < 1e-5
    assert rel_err(q.log_prob(clipped), fx.t("log_q")) < 1e-4
    assert rel_err(model.encoder.p.log_prob(clipped), fx.t("log_p")) < 1e-4
    ode = model.decoder.ode_model
    clipped.aR = fx.t("extra_theta", settings.device)[0]
    clipped.aS = fx.t("extra_theta", settings.device)[1]
    sol = ode.simulate(settings, batch.times, clipped, batch.inputs, batch.dev_1hot, condition_on_device=False)
    assert tuple(sol.shape) == (fx.B, fx.S, 8, len(fx.z["times"]))
    xs, prec = ode.expand_precisions(clipped, batch.times, sol)
    xp = ode.observe(xs, clipped)
    assert rel_err(xs, fx.t("x_states")) < 1e-4 and rel_err(xp, fx.t("x_predict")) < 1e-4
    lpo = log_prob_observations(None, xp, batch.observations, prec)
    assert rel_err(lpo, fx.t("log_p_by_species"), dim=2) < 1e-4
    # a caller-supplied state tensor goes through the generic observe
    xp2 = ode.observe(xs.contiguous(), clipped)
    assert rel_err(xp2, fx.t("x_predict")) < 1e-4


def test_evaluation_results_and_graph_step():
    """full_output=True path (Results with device-side IW summaries) and the hipGraph-captured training step."""
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture("dr_constant_icml_tiny_modeuler")
    args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, u_rng="device", conditioner_rng="device",
                                                            hip_graph=True)
    model = build_model(args, settings, data, parameters)
    training = Training(args, settings, data, parameters, model)
    batch = E.batch_from_fixture(fx, settings.device)
    model.eval()
    with torch.no_grad():
        results, theta, q, p = model(batch, args.train_samples)
        out = training.cost(batch, results, theta, q, p, full_output=True)
    assert out.iw_predict_mu.shape == (fx.B, 4, 86) and out.iw_states.shape == (fx.B, 8, 86)
    assert np.isfinite(out.elbo) and np.isfinite(out.iw_predict_mu).all()
    model.train()
    before = [p_.detach().clone() for p_ in model.parameters()]
    losses = [float(training.graph_step(batch)) for _ in range(5)]
    assert all(np.isfinite(losses))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # eager and graph steps draw different random numbers, so only check the graph step keeps optimising
    eager = float(training.step(batch))
    assert np.isfinite(eager)


@pytest.mark.parametrize("name", ["dr_constant_icml_tiny_modeuler", "auto_constant_tiny_modeuler",
                                  "dr_constant_precisions_tiny_modeuler", "dr_blackbox_icml_tiny_modeuler"])
def test_evaluation_without_a_stored_x_predict_gives_the_same_results(name):
    """params.lazy_x_predict (evaluation passes leave x_predict to the summaries kernel) against the pass that stores it:
    the same Results, and the (x_states, x_predict, precisions) tuple a plugin reads from the decoder is the stored one."""
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture(name)
    outs, tuples = [], []
    for lazy in (False, True):
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, lazy_x_predict=lazy)
        model = build_model(args, settings, data, parameters)
        training = Training(args, settings, data, parameters, model)
        batch = E.batch_from_fixture(fx, settings.device)
        model.eval()
        np.random.seed(11)
        torch.manual_seed(11)
        with torch.no_grad():
            results, theta, q, p = model(batch, args.train_samples)
            assert results.solution.has_x_predict == (not lazy)
            outs.append(training.cost(batch, results, theta, q, p, full_output=True))
            assert results.solution.has_x_predict == (not lazy)  # (the summaries did not materialise it)
            tuples.append(tuple(results))
    a, b = outs
    assert a.elbo == b.elbo
    for k in ("iw_predict_mu", "iw_predict_std", "iw_states", "iw_variance"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for x, y in zip(tuples[0], tuples[1]):
        assert x.shape == y.shape and torch.equal(x, y)


@pytest.mark.parametrize("name", ["dr_constant_icml_tiny_modeuler", "dr_constant_precisions_tiny_modeuler",
                                  "dr_blackbox_icml_tiny_modeuler"])
def test_evaluation_replayed_from_a_graph_gives_the_eager_results(name):
    """Training.evaluate with params.eval_graph (the device side of the pass captured once, replayed per evaluation) against
    the eager pass from the same generator states: six consecutive evaluations each, every member of Results identical,
    a Results kept from an earlier replay not disturbed by later ones, and parameters changed in between picked up."""
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture(name)
    runs = []
    for graph in (False, True):
        # (draws inside the kernels: their generator states are rolled back after the capture's warm-up passes, so both
        # runs see the same sequence; torch's device generator, "device", is consumed by the warm-up)
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, u_rng="kernel", conditioner_rng="kernel",
                                                                hip_graph=True, eval_graph=graph)
        model = build_model(args, settings, data, parameters)
        training = Training(args, settings, data, parameters, model)
        batch = E.batch_from_fixture(fx, settings.device)
        model.eval()
        outs = []
        for k in range(6):  # (more passes than host staging buffers: the first Results outlive their buffer's reuse)
            if k == 2:
                with torch.no_grad():
                    for p_ in model.parameters():
                        p_.mul_(1.01)
            outs.append(training.evaluate(batch, args.train_samples))
        assert (len(training._eval_graphs) == 1) == graph
        # (read AFTER all passes, without copying at the time of the pass: views of a reused buffer would show here)
        runs.append([(float(o.elbo), o.iw_predict_mu, o.iw_predict_std, o.iw_states, o.iw_variance,
                      [np.asarray(v) for v in o.q_values], o) for o in outs])
    for a, b in zip(*runs):
        assert a[0] == b[0]
        for x, y in zip(a[1:5], b[1:5]):
            assert np.array_equal(x, y)
        for x, y in zip(a[5], b[5]):
            assert np.array_equal(x, y)
    # theta is read last: the first replay's samples must have survived the two replays behind it
    for a, b in zip(*runs):
        assert np.array_equal(a[6].theta, b[6].theta)
    assert runs[1][0][0] != runs[1][1][0]  # (fresh draws per replay)


@pytest.mark.parametrize("name", ["dr_constant_icml_tiny_modeuler", "dr_constant_precisions_tiny_modeuler",
                                  "dr_blackbox_icml_tiny_modeuler", "relay_constant_precisions_tiny_modeuler",
                                  "auto_constant_tiny_modeuler"])
def test_default_graph_replay_with_the_reference_streams_equals_eager(name):
    """An UNCHANGED spec on the GPU (round 4): hip_graph is automatic and the reference's host-side streams (numpy u, CPU-drawn
    conditioner weights) are staged into the replayed step and the replayed evaluation (vihds/hostdraws.py).  Against
    hip_graph: false from the same seeds: five training steps through Training._run_batch (the second half with the next
    step's numpy draw prefetched), then an evaluation, a step, an evaluation -- every loss and ELBO equal, both generators left
    in the same state."""
    import e2e_util as E
    from vihds.training import Training
    from vihds.utils import TrainingLogData
    from vihds.vae import build_model

    fx = Fixture(name)
    runs = {}
    for graph in (False, None):
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, hip_graph=graph)
        model = build_model(args, settings, data, parameters)
        training = Training(args, settings, data, parameters, model)
        assert training.use_graph == (graph is None)
        batch = E.batch_from_fixture(fx, settings.device)
        log = TrainingLogData()
        np.random.seed(21)
        torch.manual_seed(21)
        out = []

        def step(nxt):
            model.train()
            assert training._run_batch(0.0, batch, log, next_batch=nxt)
            out.append(float(training._pending_elbo) if training._pending_elbo is not None else float(training.last_elbo))

        orig_step = training.step

        def keeping(b, *a, **k):  # (the eager path hands the loss back through _run_batch's local only)
            training.last_elbo = orig_step(b, *a, **k)
            return training.last_elbo

        training.step = keeping
        for k in range(5):
            step(batch if k >= 2 and k < 4 else None)
        model.eval()
        out.append(float(training.evaluate(batch, fx.S).elbo))
        step(None)
        model.eval()
        out.append(float(training.evaluate(batch, fx.S).elbo))
        runs[graph] = (out, np.random.rand(), float(torch.rand(1)))
    a, b = runs[False], runs[None]
    assert a[1] == b[1] and a[2] == b[2], "the host generators were consumed differently"
    for x, y in zip(a[0], b[0]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (a[0], b[0])


def test_kept_elbo_scalars_survive_later_graph_evaluations():
    """_evaluate_elbo_and_plot keeps bare `out.elbo` values (max_val_elbo, the elbo lists) while the Results they
    came from die; with the captured evaluation pass those used to be views of a pinned ring slot a later pass rewrites.
    More passes than ring slots, keeping ONLY the scalars: every kept value must still be the value of its own pass."""
    import gc
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture("dr_constant_icml_tiny_modeuler")
    args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, u_rng="kernel", conditioner_rng="kernel",
                                                            hip_graph=True, eval_graph=True)
    model = build_model(args, settings, data, parameters)
    training = Training(args, settings, data, parameters, model)
    batch = E.batch_from_fixture(fx, settings.device)
    model.eval()
    kept, at_the_time = [], []
    for k in range(11):
        out = training.evaluate(batch, args.train_samples)
        kept.append(out.elbo)  # the bare member, as the reference's loop keeps it
        at_the_time.append(float(out.elbo))
        del out
        gc.collect()
    assert len(set(at_the_time)) == 11  # (fresh draws per pass)
    assert [float(v) for v in kept] == at_the_time


class _TraceDataset(torch.utils.data.Dataset):
    def __init__(self, z):
        self.times = torch.tensor(z["times"])
        self.n_times, self.n_species = len(self.times), 4
        self.devices = np.asarray(z["devices"])
        self.dev_1hot = torch.tensor(z["dev_1hot"])
        self.inputs = torch.tensor(z["inputs"])
        self.observations = torch.tensor(z["observations"])

    def __len__(self):
        return len(self.devices)

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        return {"devices": self.devices[idx], "dev_1hot": self.dev_1hot[idx], "inputs": self.inputs[idx],
                "observations": self.observations[idx]}


def _drive_reference_trace(name, tmp_path, monkeypatch):
    """Training.run() driven through the same seeds as the reference's run_on_split (same CV split, DataLoader shuffles,
    host-numpy u, CPU-drawn conditioner weights, Adam, MultiStepLR) on the processed dataset the reference trained on.
    Returns (losses of every step, the reference's recorded losses, run()'s result, the trace file)."""
    import json
    import os

    import e2e_util as E
    from vihds.config import Config
    from vihds.datasets import split_dataset
    from vihds.parameters import Parameters
    from vihds.training import Training
    from vihds.vae import build_model

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    cfg = json.loads(str(z["config_json"]))
    spec = json.loads(str(z["spec_json"]))
    spec["params"]["solver"] = cfg["solver"]
    args = E.make_args(cfg["n_iwae"], seed=cfg["seed"], gpu=0)
    args.epochs = args.test_epoch = cfg["epochs"]
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    settings = Config(args=None, spec=spec)
    settings.device = torch.device("cuda:0")
    data = split_dataset(_TraceDataset(z), args, settings.data)
    assert np.array_equal(np.asarray(data.train.indices), z["train_ids"])
    parameters = Parameters(settings.params)
    model = build_model(args, settings, data, parameters)
    training = Training(args, settings, data, parameters, model)
    losses = []
    orig = training.step_rows

    def recording_step(rows, next_rows=None, ahead=1):  # (run() replays its steps from hipGraphs by default: the loss is what a step hands back)
        out = orig(rows, next_rows, ahead)
        losses.append(float(out))
        return out

    training.step_rows = recording_step
    orig_epoch = training.epoch_rows

    def recording_epoch(batches):  # (an epoch of a single batch is one graph launch even with the per-step NaN check)
        out = orig_epoch(batches)
        losses.extend(float(v) for v in out)
        return out

    training.epoch_rows = recording_epoch
    assert training.use_graph and settings.params.u_rng == "numpy" and settings.params.conditioner_rng == "cpu"
    monkeypatch.chdir(tmp_path)
    result = training.run()
    return np.array(losses), z["step_losses"], result, z


@pytest.mark.parametrize("name", ["trace_dr_constant_icml_modeuler", "trace_auto_constant_modeuler"])
def test_training_run_tracks_reference_trace(name, tmp_path, monkeypatch):
    """Drop-in check of the whole loop: the loss of every training step and the final validation ELBO against what the
    reference recorded (4 / 6 epochs at n_iwae = 20)."""
    losses, ref, result, z = _drive_reference_trace(name, tmp_path, monkeypatch)
    assert len(losses) == len(ref)
    rel = np.abs(np.array(losses) - ref) / np.abs(ref)
    print("per-step relative deviation from the reference:", np.array2string(rel, precision=2))
    assert rel[0] < 1e-4
    assert rel[: min(7, len(rel))].max() < 1e-3   # first epoch
    assert rel.max() < 5e-2                        # fp32 rounding differences grow through Adam, slowly
    assert result is not None
    assert abs(float(result.elbo) - float(z["valid_elbo"][-1])) / abs(float(z["valid_elbo"][-1])) < 5e-2


def test_long_reference_trace_at_the_headline_sample_count(tmp_path, monkeypatch):
    """The reference's own run at the headline's sample count and the spec's learning rate: dr_constant_icml, n_iwae = 200, lr 0.01,
    modeuler, 15 epochs = 105 steps (tests/golden/trace_dr_constant_icml_s200_modeuler.npz, round 5).  At this learning rate the
    training dynamics amplify rounding differences by roughly 7x per step (measured: 0, 2e-7, 3e-6, 1.5e-5, 1e-4, 1e-2, ...: the
    IWAE weights concentrate on a few samples), so a step-by-step comparison is meaningful for the first steps only; after that
    the check is that the run lands where the reference's does -- a finite objective of the same size -- and neither stalls nor
    runs away (the reference: last loss -522.5, validation ELBO 579.2).  (Run-aways do exist at this learning rate, in the reference
    as here: of its seeds 0..17 one -- seed 12 -- ends at -7.6e17, profiles/r05_reference_runaway_seeds.log; of the same eighteen runs
    through this package one -- seed 8 -- does, tests/probe/ref_seed_compare.py.  Seed 0, recorded here, is not among them.)"""
    losses, ref, result, z = _drive_reference_trace("trace_dr_constant_icml_s200_modeuler", tmp_path, monkeypatch)
    assert len(losses) == len(ref) == 105
    rel = np.abs(losses - ref) / np.abs(ref)
    print("first steps, relative deviation from the reference:", np.array2string(rel[:8], precision=2))
    assert rel[0] < 1e-4 and rel[:5].max() < 1e-3
    assert np.isfinite(losses).all() and np.abs(losses).max() < 1e5
    # the last epoch's mean loss and the validation ELBO: the reference's magnitude (chaotic, not step-exact)
    ours_end, ref_end = losses[-7:].mean(), ref[-7:].mean()
    print("last epoch mean loss: ours %.1f, reference %.1f; validation ELBO ours %.1f, reference %.1f"
          % (ours_end, ref_end, float(result.elbo), float(z["valid_elbo"][-1])))
    assert ours_end < 0 and abs(ours_end - ref_end) < 0.5 * abs(ref_end)
    assert result is not None and abs(float(result.elbo) - float(z["valid_elbo"][-1])) < 0.4 * abs(float(z["valid_elbo"][-1]))


def _run_worker(mode, steps, s_total, ranks):
    import json
    import socket
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "two_rank_worker.py")
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None), env.pop("LOCAL_RANK", None)
    if ranks == 1:
        cmd = [sys.executable, worker, mode, str(steps), str(s_total)]
    else:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        # both ranks share the one GPU of the test box; gloo because a communicator cannot hold one device twice
        env.update(VIHDS_DIST_BACKEND="gloo", VIHDS_FORCE_DEVICE="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
               "--master-addr", "127.0.0.1", "--master-port", str(port), worker, mode, str(steps), str(s_total)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("LOSSES ")][-1]
    return json.loads(line[len("LOSSES "):])


def test_two_ranks_sharded_step_matches_single_process_and_segmented_graph_matches_eager():
    """S sharded over two ranks (one process per rank, both on this box's one GPU, gloo): (a) the loss trajectory equals
    the single-process run over the same global sample set (in-kernel RNG is shard-consistent, the row statistics and
    the gradients are exchanged); (b) the captured step -- hipGraph segments with the collectives run eagerly in
    between -- reproduces the eager steps one for one (the three warm-up steps before the capture are rolled back:
    parameters, Adam state and generator counters)."""
    S = 16
    single = _run_worker("eager", 8, S, 1)
    eager2 = _run_worker("eager", 8, S, 2)
    graph2 = _run_worker("graph", 5, S, 2)
    for a, b in zip(single, eager2):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (single, eager2)
    for k in range(5):
        assert abs(graph2[k] - eager2[k]) <= 2e-4 * max(1.0, abs(eager2[k])), (graph2, eager2)
    assert single[-1] < single[0]  # and it trains


@pytest.mark.parametrize("decoder_step", [False, True])
def test_fused_training_path_matches_two_kernel_path(decoder_step):
    """params.fused_ode_training: one launch (vihds_ode_logp_grad) gives the log-likelihood and the unit-weight
    adjoint, the theta gradient is scaled by the IWAE weights afterwards, and x_states / x_predict are only computed
    if somebody unpacks the decoder result.  Loss and every encoder-parameter gradient must equal the two-kernel path's
    on the reference fixture, and the lazily built outputs must equal the fixture's trajectories.
    decoder_step: sampling and device conditioning run inside the same launch too (vihds_theta_ode_logp_grad)."""
    import e2e_util as E
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture("dr_constant_icml_tiny_modeuler")
    outs = {}
    for fused in (False, True):
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, fused_ode_training=fused,
                                                               fused_decoder_step=decoder_step)
        model = build_model(args, settings, data, parameters)
        training = Training(args, settings, data, parameters, model)
        model.train()
        batch = E.batch_from_fixture(fx, "cuda:0")
        np.random.seed(fx.cfg["seed"] + 1)
        torch.manual_seed(fx.cfg["seed"] + 1)
        batch_results, theta, q, p = model(batch, fx.S)
        if fused:
            from vihds.decoders import LazyDecoderResult

            assert isinstance(batch_results, LazyDecoderResult) and batch_results._items is None
        elbo = training.cost(batch, batch_results, theta, q, p).elbo
        elbo.backward()
        if fused:
            assert batch_results._items is None  # training never asked for the trajectories
            x_states, x_predict, _prec = batch_results
            assert rel_err(x_states, fx.t("x_states")) < 1e-4 and rel_err(x_predict, fx.t("x_predict")) < 1e-4
        outs[fused] = (float(elbo), {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None})
    assert abs(outs[True][0] - outs[False][0]) <= 1e-6 * abs(outs[False][0])
    assert abs(outs[True][0] - float(fx.t("loss"))) <= 1e-4 * abs(float(fx.t("loss")))
    for k, g in outs[False][1].items():
        assert rel_err(outs[True][1][k], g) < 1e-5, k


@pytest.mark.parametrize("seed_kind", ["unit", "ones"])
def test_iwae_loss_inside_the_theta_adjoint_matches_separate_launch(seed_kind):
    """params.fused_iwae_backward: Training.cost launches nothing for the loss; the decoder step's backward forms the
    importance weights, the loss value, log_w and lse inside the theta-adjoint launch (vihds_iwae_job).  With the unit
    seed Training.step uses, loss and every encoder gradient must equal the separate-launch path; a backward seeded any
    other way falls back to the ordinary IWAE launch and must give the same numbers too."""
    import e2e_util as E
    from vihds import ops
    from vihds.training import Training
    from vihds.vae import build_model

    fx = Fixture("dr_constant_icml_tiny_modeuler")
    outs = {}
    for fused_iwae in (False, True):
        args, settings, data, parameters = E.build_from_fixture(fx, gpu=0, fused_ode_training=True, fused_decoder_step=True,
                                                               fused_iwae_backward=fused_iwae)
        model = build_model(args, settings, data, parameters)
        training = Training(args, settings, data, parameters, model)
        model.train()
        batch = E.batch_from_fixture(fx, "cuda:0")
        np.random.seed(fx.cfg["seed"] + 1)
        torch.manual_seed(fx.cfg["seed"] + 1)
        batch_results, theta, q, p = model(batch, fx.S)
        eager = training.cost(batch, batch_results, theta, q, p).elbo  # outside Training.step: never deferred
        assert not ops._PENDING_IWAE and abs(float(eager) - float(fx.t("loss"))) <= 1e-4 * abs(float(fx.t("loss")))
        elbo = training.cost(batch, batch_results, theta, q, p, defer_iwae=True).elbo  # as Training.step calls it
        if fused_iwae:
            assert len(ops._PENDING_IWAE) == 1  # nothing launched for the loss yet
        elbo.backward(ops.unit_gradient(elbo.device) if seed_kind == "unit" else torch.ones_like(elbo))
        assert not ops._PENDING_IWAE
        outs[fused_iwae] = (float(elbo), {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None})
    assert abs(outs[True][0] - outs[False][0]) <= 1e-6 * abs(outs[False][0])
    assert abs(outs[True][0] - float(fx.t("loss"))) <= 1e-4 * abs(float(fx.t("loss")))
    for k, g in outs[False][1].items():
        assert rel_err(outs[True][1][k], g) < 1e-5, k


def test_two_replicas_row_data_parallel_plumbing():
    """--shard rows: every rank runs the whole step on its own rows and the gradients are averaged (one all-reduce, the
    1/world factor applied inside the Adam kernel).  With both replicas fed the SAME rows and draws the averaged step
    must reproduce the single-process step exactly -- eager and as hipGraph segments around the collective -- and
    with different rows per replica it must still train."""
    S = 16
    single = _run_worker("eager", 8, S, 1)
    same_eager = _run_worker("dp-same-eager", 8, S, 2)
    same_graph = _run_worker("dp-same-graph", 5, S, 2)
    for a, b in zip(single, same_eager):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (single, same_eager)
    for k in range(5):
        assert abs(same_graph[k] - same_eager[k]) <= 2e-4 * max(1.0, abs(same_eager[k])), (same_graph, same_eager)
    diff = _run_worker("dp-diff-graph", 30, S, 2)
    assert all(np.isfinite(diff)) and min(diff[-5:]) < diff[0]


def test_one_rank_rccl_job_with_the_collective_inside_the_graph():
    """The multi-GPU path on the one GPU of the test box: a ONE-rank job over RCCL (VIHDS_FORCE_DIST=1: communicator,
    RowReplica, gradient all-reduce) must walk the single-process loss trajectory -- eagerly, with one step per captured
    graph and with four steps per graph launch, which needs the all-reduce recorded INSIDE the hipGraph
    (parallel.collectives_capturable: probed in a child process; where the stack cannot, the step is cut at the collective
    and `graph4` is refused -- then this test checks the refusal instead)."""
    import json
    import socket
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "two_rank_worker.py")

    def run(mode, steps, dist):
        env = dict(os.environ)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "VIHDS_DIST_BACKEND"):
            env.pop(k, None)
        if dist:
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       VIHDS_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = subprocess.run([sys.executable, worker, mode, str(steps), "16"], env=env, capture_output=True, text=True, timeout=900)
        return out

    def losses(out):
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("LOSSES ")][-1]
        cap = [ln for ln in out.stdout.splitlines() if ln.startswith("CAPTURED ")][-1]
        return json.loads(line[len("LOSSES "):]), int(cap.split()[1])

    single, _ = losses(run("eager", 8, False))
    eager, _ = losses(run("dp-same-eager", 8, True))
    graph, captured = losses(run("dp-same-graph", 8, True))
    for a, b in zip(single, eager):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (single, eager)
    for a, b in zip(eager, graph):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (eager, graph)
    out4 = run("dp-same-graph4", 8, True)
    if captured:
        g4, cap4 = losses(out4)
        assert cap4 == 1
        for a, b in zip(eager, g4):
            assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (eager, g4)
    else:
        assert out4.returncode != 0 and "collectives inside the graph" in out4.stderr


@pytest.mark.parametrize("solver,tail", [("rk4", False), ("rk4", True), ("modeuler", True)])
def test_headline_decoder_launch_matches_oracle_at_bench_shape(solver, tail):
    """The launch bench.py times, checked directly: synthetic dr_constant_icml batch, B=36, S=200, T=86, in-kernel
    Philox for u and the conditioner weights, vihds_theta_ode_logp_grad (sampling + conditioning + integration +
    log-likelihood + unit-weight adjoint in one launch) -> IWAE loss -> theta adjoint -> encoder adjoint, once
    eagerly and once replayed from the step's hipGraph.  The draws u and the conditioner rows aR / aS the kernel
    wrote out are handed to the oracle (reference vae.py:26-36 + training.py:127-149 restated op by op on the CPU,
    fed by a CPU twin of the encoder holding the same weights): theta, log q, log p, the per-signal log-likelihoods,
    the loss and the gradient of every encoder parameter must agree.  rk4 is the bench's solver (torchdiffeq 0.1's
    tableau restated: parity unpinned, see oracle header); modeuler is the reference's own integrator."""
    from oracle import vihds_oracle as O
    from vihds import ops, synthetic

    B, S = 36, 200
    # tail: the rest of the step as vihds_step_tail's two launches (bench.py's default) instead of theta adjoint + encoder
    # adjoint + Adam as five; the encoder gradients it leaves in .grad are checked against the same oracle numbers
    kw = dict(solver=solver, seed=1, u_rng="kernel", conditioner_rng="kernel", nan_check_every=0, learning_rate=0.001,
              fused_ode_training=True, fused_iwae_backward=tail, fused_step_tail=tail)
    twin = None
    for graph in (False, True):
        args, settings, data, parameters, model, training = synthetic.build(
            "dr_constant_icml", B, S, device="cuda:0", hip_graph=graph, **kw)
        model.train()
        batch = training.train_data
        stash = {}
        orig_cost = training.cost

        def cost(b, results, theta, q, p, _o=orig_cost, _s=stash, **k):
            _s.update(results=results, theta=theta, q=q)
            return _o(b, results, theta, q, p, **k)

        training.cost = cost
        rec = ops.LaunchRecorder()
        if graph:
            training.graph_step(batch)  # warm-up (rolled back), capture, first replay
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            loss = training.graph_step(batch)  # the replay under test
        else:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            ops.TIMER = rec
            try:
                loss = training.step(batch, zero_grad=False)
            finally:
                ops.TIMER = None
            assert "decoder_step" in rec.calls, "the fused decoder launch did not run: %s" % list(rec.calls)
        torch.cuda.synchronize()
        theta, q, results = stash["theta"], stash["q"], stash["results"]
        enc = model.encoder
        names = list(enc.names)
        got_theta = torch.stack([theta.samples[n] for n in names]).cpu()
        u = theta._u.detach().cpu()
        aR, aS = theta.aR.detach().cpu(), theta.aS.detach().cpu()
        got_logq, got_logp = q.log_prob(theta).detach().cpu(), enc.p.log_prob(theta).detach().cpu()
        got_lpo = results.solution.logp_buffer.detach().cpu().permute(1, 2, 0)
        got_grads = {k: v.grad.detach().cpu().clone() for k, v in model.named_parameters() if v.grad is not None}
        assert u.shape == (B, S, len(names)) and abs(float(u.mean())) < 0.01 and abs(float(u.std()) - 1.0) < 0.01

        # ---- oracle on the same draws
        if twin is None:
            twin = synthetic.build("dr_constant_icml", B, S, device="cpu", observations=batch.observations.cpu(), **kw)
        c_model, c_training = twin[4], twin[5]
        c_model.load_state_dict({k: v.cpu() for k, v in state.items()})
        c_model.zero_grad(set_to_none=True)
        c_enc, cb = c_model.encoder, c_training.train_data
        assert torch.equal(cb.observations, batch.observations.cpu()) and torch.equal(cb.inputs, batch.inputs.cpu())
        kinds = [d.kind for d in c_enc.descs]
        _, pm, pp = c_enc.p.image("cpu", 1)
        p_mu, p_prec = [pm[i, 0] for i in range(len(names))], [pp[i, 0] for i in range(len(names))]
        cq = c_enc(cb)
        _, q_mu, q_prec = cq.image("cpu", B)
        qm = [q_mu[i][:, None] for i in range(len(names))]
        qp = [q_prec[i][:, None] for i in range(len(names))]
        th = O.sample_clip_theta(names, kinds, qm, qp, p_mu, p_prec, u)
        th["aR"], th["aS"] = aR, aS
        out = O.elbo_from_theta("dr_constant", names, kinds, th, qm, qp, p_mu, p_prec, cb.inputs, cb.times,
                                cb.observations, solver)
        out["loss"].backward()
        tag = "graph replay" if graph else "eager"
        assert rel_err(got_theta, torch.stack([th[n] for n in names]), dim=0) < 1e-5, tag
        assert rel_err(got_logq, out["log_q"]) < 1e-4 and rel_err(got_logp, out["log_p"]) < 1e-4, tag
        assert rel_err(got_lpo, out["log_p_by_species"], dim=2) < 1e-4, tag
        assert rel_err(loss, out["loss"]) < 1e-4, tag
        ref_grads = {k: v.grad for k, v in c_model.named_parameters() if v.grad is not None}
        assert set(ref_grads) == set(got_grads), tag
        errs = {k: float(rel_err(got_grads[k], g)) for k, g in ref_grads.items()}
        print("encoder-gradient errors vs oracle (%s, %s): %s" % (solver, tag, {k: "%.1e" % v for k, v in errs.items()}))
        for k, e in errs.items():
            assert e < 2e-5, (tag, k, errs)


def _tail_run(tail, graph, n_steps, B=8, S=24, poison_at=None, **extra):
    """n_steps training steps of the synthetic dr_constant_icml plate through Training.step / graph_step with the bench's
    fast keys; returns (losses, last gradients, parameters after, optimizer step count, kernel names of one step)."""
    from vihds import ops, synthetic

    kw = dict(solver="rk4", seed=3, u_rng="kernel", conditioner_rng="kernel", nan_check_every=0, learning_rate=0.01,
              fused_ode_training=True, fused_decoder_step=True, fused_iwae_backward=True, fused_step_tail=tail)
    kw.update(extra)
    args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", B, S, device="cuda:0",
                                                                        hip_graph=graph, **kw)
    model.train()
    batch = training.train_data
    losses, launched = [], []
    clean = batch.observations.clone()
    for k in range(n_steps):
        if poison_at is not None:
            # (in place: a captured step reads the batch from the buffers it was staged in)
            batch.observations.copy_(clean)
            if k == poison_at:
                batch.observations[1, 2, 5] = float("nan")
            training._staged.clear()
        if graph:
            loss = training.graph_step(batch)
        else:
            rec = ops.LaunchRecorder()
            ops.TIMER = rec
            try:  # (zero_grad only on the last step: autograd ACCUMULATES into .grad when it is left standing)
                loss = training.step(batch, zero_grad=k < n_steps - 1)
            finally:
                ops.TIMER = None
            launched = list(rec.calls)
        losses.append(float(loss))
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    return losses, grads, params, training.optimizer.step_count(), launched


@pytest.mark.parametrize("graph", [False, True])
def test_step_tail_matches_the_five_launch_path(graph):
    """params.fused_step_tail: IWAE loss + theta adjoint + encoder adjoint + Adam as vihds_step_tail's two launches
    (row blocks, then gradient sums with the update applied in place) against the same step as vihds_theta_bwd (with the
    IWAE job) + vihds_encoder_bwd (two launches) + vihds_adam_step: same draws (in-kernel generators, same seeds), so the
    loss of every step, the last step's gradient of every encoder parameter, every parameter after 5 Adam steps and the
    step counter must agree -- eagerly and replayed from the step's hipGraph."""
    # ONE step from the same initial state: the tail's own arithmetic (v_exp / v_log / v_rcp in the theta adjoint, DPP
    # scan sums) against the five-launch path's, before any Adam step can amplify a rounding difference
    ref1 = _tail_run(False, graph, 1)
    got1 = _tail_run(True, graph, 1)
    assert abs(ref1[0][0] - got1[0][0]) <= 1e-6 * abs(ref1[0][0])
    assert set(ref1[1]) == set(got1[1])
    for k, g in ref1[1].items():
        assert rel_err(got1[1][k], g) < 1e-5, k
    for k, v in ref1[2].items():
        assert rel_err(got1[2][k], v) < 1e-6, k
    # five steps: Adam's first updates are lr * sign-like (m / sqrt(v)), so rounding-level gradient differences show up
    # at the 1e-6 .. 1e-5 level in later losses
    ref = _tail_run(False, graph, 5)
    got = _tail_run(True, graph, 5)
    if not graph:
        assert "step_tail" in got[4] and "step_tail" not in ref[4], (got[4], ref[4])
    for a, b in zip(ref[0], got[0]):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (ref[0], got[0])
    assert set(ref[1]) == set(got[1])
    for k, g in ref[1].items():
        assert rel_err(got[1][k], g) < 2e-4, k
    for k, v in ref[2].items():
        assert rel_err(got[2][k], v) < 1e-4, k
    assert ref[3] == got[3] == 5


@pytest.mark.parametrize("tail", [False, True])
def test_non_finite_loss_skips_the_whole_update(tail):
    """The reference stops before optimizer.step on a NaN ELBO (training.py:331-334).  Here the launches of the step are
    already queued when the host could look, so the update is gated on the device: a step whose loss is not finite leaves
    every parameter, both Adam moments and the step count exactly as they were -- all or nothing -- with the separate Adam
    launch (vihds_adam_step's `gate`) and with vihds_step_tail alike; the next finite step trains on."""
    clean = _tail_run(tail, False, 2)
    bad = _tail_run(tail, False, 3, poison_at=1)
    assert np.isfinite(bad[0][0]) and not np.isfinite(bad[0][1]) and np.isfinite(bad[0][2]), bad[0]
    assert bad[3] == 2  # the poisoned step did not count
    # step 0 (finite) + step 1 (skipped) + step 2 (finite, same draws as the clean run's step... no: the generators moved
    # on during the skipped step, so only the FIRST step is comparable value for value)
    assert abs(bad[0][0] - clean[0][0]) <= 1e-6 * max(1.0, abs(clean[0][0]))
    for k, v in bad[2].items():
        assert torch.isfinite(v).all(), k
    one = _tail_run(tail, False, 1)
    two = _tail_run(tail, False, 2, poison_at=1)
    for k, v in one[2].items():
        assert torch.equal(two[2][k], v), k  # bit for bit what the single finite step left
    assert two[3] == 1


@pytest.mark.parametrize("tail", [False, True])
def test_multi_step_graph_matches_one_step_graphs(tail):
    """graph_step(batch, repeat=3): three consecutive training steps captured into ONE hipGraph (what bench.py replays to
    amortise the idle time between graph launches).  Two launches of it must walk the same loss sequence, and leave the
    same parameters and step count, as six launches of the one-step graph -- with the five-launch tail (whose autograd
    gradients must not accumulate from one captured step into the next) and with vihds_step_tail."""
    from vihds import synthetic

    kw = dict(solver="rk4", seed=3, u_rng="kernel", conditioner_rng="kernel", nan_check_every=0, learning_rate=0.01,
              fused_ode_training=True, fused_decoder_step=True, fused_iwae_backward=True, fused_step_tail=tail)
    runs = {}
    for repeat in (1, 3):
        args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 8, 24, device="cuda:0",
                                                                            hip_graph=True, **kw)
        model.train()
        batch = training.train_data
        losses = []
        for _ in range(6 // repeat):
            last = training.graph_step(batch, repeat=repeat)
            losses += [float(x) for x in training.last_losses] if repeat > 1 else [float(last)]
        torch.cuda.synchronize()
        runs[repeat] = (losses, {k: v.detach().clone() for k, v in model.named_parameters()}, training.optimizer.step_count())
    assert len(runs[3][0]) == 6 and runs[1][2] == runs[3][2] == 6
    for a, b in zip(runs[1][0], runs[3][0]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (runs[1][0], runs[3][0])
    for k, v in runs[1][1].items():
        assert rel_err(runs[3][1][k], v) < 1e-6, k


def test_bench_gpus_2_self_launch_on_one_device():
    """The driver's plain command for a scaling run, `python bench.py --gpus N`, with N = 2 ranks sharing this box's one GPU
    over gloo: bench.py starts the ranks itself, rank 0 prints ONE JSON line whose value counts both replicas' steps, names
    the world size and every rank's device, and (--full) carries the strong-scaling leg (config 3's one batch, sample-sharded)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(VIHDS_DIST_BACKEND="gloo", VIHDS_FORCE_DEVICE="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "10", "--warmup", "2",
                        "--full", "--roofline-steps", "0", "--no-cpu-baseline"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.strip()] == lines, r.stdout[-3000:]  # the line and nothing else on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and np.isfinite(out["final_loss"])
    # the strong-scaling legs: ONE batch, its IWAE-sample axis sharded over the two ranks -- config 3 and config 5
    for leg, per_rank in (("strong_scaling_config3", 500), ("strong_scaling_config5", 100)):
        assert out[leg]["scaling"] == "strong" and out[leg]["n_iwae_per_gpu"] == per_rank, out[leg]
        assert out[leg]["value"] > 0 and np.isfinite(out[leg]["final_loss"]), out[leg]
    assert out["eager_ms_per_step"] > 0  # (the safe measurement that precedes the captured one)


@pytest.mark.parametrize("graph", [False, True])
def test_step_rows_gathers_on_the_device_what_the_host_loader_would_stack(graph):
    """Device-resident batching (Training.step_rows / vihds_gather_batch): a step on rows picked by index from the resident
    training set -- eagerly, and as one hipGraph per batch size holding gather + step, full and ragged batches alternating
    -- must walk the loss sequence of steps on the same batches built on the host (index, copy, delta_obs with torch ops)."""
    from vihds import synthetic
    from vihds.utils import attrify

    kw = dict(solver="rk4", seed=5, u_rng="kernel", conditioner_rng="kernel", nan_check_every=0, learning_rate=0.01,
              fused_ode_training=True, fused_decoder_step=True, fused_iwae_backward=True, fused_step_tail=True, n_batch=8)
    g = torch.Generator().manual_seed(0)
    picks = [torch.randperm(20, generator=g)[:n] for n in (8, 8, 4, 8, 4, 8)]
    runs = {}
    for mode in ("host", "rows"):
        args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                            hip_graph=graph and mode == "rows", **kw)
        model.train()
        src = training.train_data
        losses = []
        for rows in picks:
            if mode == "rows":
                losses.append(float(training.step_rows(rows)))
            else:
                r = rows.to("cuda:0")
                obs = src.observations[r].contiguous()
                batch = attrify({"observations": obs, "inputs": src.inputs[r].contiguous(),
                                 "dev_1hot": src.dev_1hot[r].contiguous(), "times": src.times, "devices": None,
                                 "delta_obs": (obs[:, :, 1:] - obs[:, :, :-1]).contiguous()})
                losses.append(float(training.step(batch)))
        runs[mode] = (losses, {k: v.detach().clone() for k, v in model.named_parameters()})
    for a, b in zip(runs["host"][0], runs["rows"][0]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (runs["host"][0], runs["rows"][0])
    for k, v in runs["host"][1].items():
        assert rel_err(runs["rows"][1][k], v) < 1e-6, k


def test_epoch_graph_walks_the_same_steps_as_one_graph_per_step():
    """Training.epoch_rows (what run() uses with hip_graph when the NaN check is at most once per epoch): all the steps of
    an epoch -- full batches and the ragged one, gather + step each -- in ONE hipGraph launch fed by one copy of the epoch's
    row indices, against the same batches through Training.step_rows (one graph launch per step): same losses, same
    parameters after two epochs; and run() itself takes that path and counts the steps."""
    from vihds import synthetic

    kw = dict(solver="rk4", seed=5, u_rng="kernel", conditioner_rng="kernel", learning_rate=0.01, hip_graph=True,
              fused_ode_training=True, fused_decoder_step=True, fused_iwae_backward=True, fused_step_tail=True, n_batch=8)
    g = torch.Generator().manual_seed(1)
    epochs = [list(torch.randperm(20, generator=g).split(8)) for _ in range(2)]  # 8 + 8 + 4 rows, twice
    runs = {}
    for mode in ("steps", "epoch"):
        args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                            nan_check_every=0, **kw)
        model.train()
        losses = []
        for batches in epochs:
            if mode == "epoch":
                losses += [float(l) for l in training.epoch_rows(batches)]
            else:
                losses += [float(training.step_rows(rows)) for rows in batches]
        runs[mode] = (losses, {k: v.detach().clone() for k, v in model.named_parameters()})
    assert len(runs["epoch"][0]) == 6
    for a, b in zip(runs["steps"][0], runs["epoch"][0]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (runs["steps"][0], runs["epoch"][0])
    for k, v in runs["steps"][1].items():
        assert rel_err(runs["epoch"][1][k], v) < 1e-6, k
    # run(): three epochs of three batches, NaN check once per epoch -> three graph launches, nine steps
    args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                        nan_check_every=3, **kw)
    args.epochs, args.test_epoch, args.test_samples = 3, 3, 32
    assert training.epoch_graph
    out = training.run()
    assert training._steps == 9 and any(k[0] == "epoch" for k in training._graphs if isinstance(k[0], str))
    assert out is not None and np.isfinite(float(out.elbo))


@pytest.mark.parametrize("model_name,graph", [("dr_constant_icml", False), ("dr_constant_icml", True),
                                              ("relay_constant_precisions", False)])
def test_evaluation_with_online_summaries_gives_the_two_kernel_results(model_name, graph):
    """params.online_summaries (default: the evaluation's forward launch writes the log-likelihoods only, the summaries come
    from a second forward launch that adds them up on the way: no trajectory through HBM) against the pass that stores the
    trajectory and streams it back, at an evaluation-sized launch (24 rows x 1 000 samples), from the same generator
    states: the same ELBO and theta samples bit for bit, the summaries to rounding (another summation order); eagerly and
    from the captured evaluation graph; a plugin that asks for the trajectory after all gets it."""
    from vihds import synthetic

    outs = []
    for online in (True, False):
        args, settings, data, parameters, model, training = synthetic.build(
            model_name, 24, 16, solver="rk4", device="cuda:0", seed=3, u_rng="kernel", conditioner_rng="kernel",
            hip_graph=graph, nan_check_every=0, learning_rate=0.001, online_summaries=online)
        model.eval()
        res = [training.evaluate(training.train_data, 1000) for _ in range(2)]
        sol = model.decoder.ode_model._last
        assert (getattr(sol, "online_summaries", None) is not None) == online
        outs.append(res[-1])
        if online and not graph:
            with torch.no_grad():
                results, theta, q, p = model(training.train_data, 1000)
                x_states, x_predict, precisions = tuple(results)
            assert x_states.shape[:2] == (24, 1000) and torch.isfinite(x_states).all()
    a, b = outs
    assert float(a.elbo) == float(b.elbo)
    for k in ("iw_predict_mu", "iw_states", "iw_variance"):
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.shape == y.shape and np.abs(x - y).max() <= 2e-5 * np.abs(y).max(), k
    # iw_predict_std = sqrt(sum_s w (x^2 + 1 / prec) - mu^2) as the reference forms it (utils.py:92-96): where ONE sample holds
    # nearly all the weight and x^2 >> 1 / prec the difference of the two float32 terms can round below zero and the root is
    # NaN -- in the reference's expression as in both kernel forms, at the same (row, signal, time) entries up to rounding.
    # The two forms must agree wherever both are finite, and on (almost) the same set of entries.
    x, y = np.asarray(a.iw_predict_std), np.asarray(b.iw_predict_std)
    ok = np.isfinite(x) & np.isfinite(y)
    assert ok.mean() > 0.95 and (np.isfinite(x) != np.isfinite(y)).mean() < 0.01
    assert np.abs(x[ok] - y[ok]).max() <= 2e-3 * np.abs(y[ok]).max()


def test_run_with_epoch_lookahead_walks_the_same_steps_and_notices_a_nan():
    """params.epoch_lookahead (run() queues an epoch's graph launch BEFORE it looks at the previous epoch's losses: the look
    is one flag per epoch in pinned memory behind an event): the same steps -- parameters and validation ELBOs bit for bit --
    as the loop that looks first; and a NaN loss still ends the run (one epoch later at most), with every NaN step a no-op."""
    from vihds import synthetic

    kw = dict(solver="rk4", seed=5, u_rng="kernel", conditioner_rng="kernel", learning_rate=0.01, hip_graph=True, nan_check_every=3,
              fused_ode_training=True, fused_decoder_step=True, fused_iwae_backward=True, fused_step_tail=True, n_batch=8)
    runs = {}
    for look in (False, True):
        args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                            epoch_lookahead=look, **kw)
        args.epochs, args.test_epoch, args.test_samples = 6, 3, 32
        assert training.epoch_graph and training.epoch_lookahead == look
        out = training.run()
        assert training._steps == 18
        runs[look] = ({k: v.detach().clone() for k, v in model.named_parameters()}, [float(e) for e in out.elbo_list])
    for k, v in runs[False][0].items():
        assert torch.equal(runs[True][0][k], v), k
    assert runs[True][1] == runs[False][1]
    # a NaN in the data: the run stops, the parameters are those of before (every step's update is gated on its own loss)
    args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                        epoch_lookahead=True, **kw)
    args.epochs, args.test_epoch, args.test_samples = 6, 3, 32
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    training.train_data.observations[:, 0, 5] = float("nan")
    training.run()
    assert training._steps <= 2 * 3  # (noticed after the second epoch was queued at the latest)
    for k, v in before.items():
        assert torch.equal(dict(model.named_parameters())[k].detach(), v), k
    # a NaN in ONE row: exactly one batch of every epoch has a non-finite loss.  Documented semantics
    # (INTEGRATION.md section 7): that batch's step is a no-op on the device, the finite batches of the epoch(s) already queued
    # still apply their updates (the reference would have stopped before them), and the run ends within two epochs.
    args, settings, data, parameters, model, training = synthetic.build("dr_constant_icml", 20, 16, device="cuda:0",
                                                                        epoch_lookahead=True, **kw)
    args.epochs, args.test_epoch, args.test_samples = 6, 3, 32
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    training.train_data.observations[7, 0, 5] = float("nan")
    training.run()
    assert training._steps <= 2 * 3
    after = {k: v.detach() for k, v in model.named_parameters()}
    assert all(torch.isfinite(v).all() for v in after.values())  # the NaN step touched nothing
    assert any(not torch.equal(after[k], before[k]) for k in before)  # ... and the finite steps beside it did train
