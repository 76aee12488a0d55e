#!/usr/bin/env python3
"""Headline benchmark: ELBO training steps/sec on dr_constant_icml (B=36 rows, n_iwae=200, T=86, RK4), fp32.

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = Training._run_batch semantics (reference vihds/training.py:324-340): draw u -> encoder -> sample/clip
theta + log q/log p (theta kernel) -> integrate + observe + log-likelihood (ODE kernel) -> IWAE loss -> backward
through all three hand-written adjoints and the encoder -> Adam.  Inputs (the 36-row batch) are resident in HBM;
u is drawn on the device inside the step.  N > 1 (weak scaling, `value` counts N step-equivalents per iteration):
--shard rows (default) = data parallel, every rank runs the whole step on its own 36 rows x 200 samples and the
parameter gradients are averaged with ONE all-reduce per step (global batch 36*N rows at n_iwae = 200);
--shard samples = every rank holds the same 36 rows and 200 of the 200*N samples per row, the row (max, sum-exp)
pairs are all-gathered and one all-reduce sums the gradients.

Prints ONE JSON line (< 6 KB: compact_line) on rank 0.  A plain run sets up, warms up, times the K steps and prints the
line (`roofline` and `cpu_baseline` null).  `--full` also measures `roofline` for the dominant kernel (the decoder launch)
and `cpu_baseline` (the oracle's op-by-op CPU restatement of the same step, timed here) and writes everything to
bench_extra.json; `--all-legs` (implies --full) also runs the other BASELINE configurations and the Training.run() /
unchanged-spec legs.  `--dump-outputs DIR` writes the last timed step's loss and the trained parameters to DIR."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "vi-hds_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B_ROWS, N_IWAE, N_TIMES, N_STATES, N_PARAMS = 36, 200, 86, 8, 35
SETUP_STEPS = int(os.environ.get("VIHDS_BENCH_SETUP_STEPS", "4096"))  # untimed graph-replayed steps ahead of the W warm-up steps
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs
MULTI_RANK_WATCHDOG_S = 300  # a multi-rank graph path that has not finished by then gives way to the eager line taken before it
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


_OUT = None  # the process's real stdout once `__main__` has routed everything else to stderr


def emit(obj):
    """The bench line (and nothing else) on stdout."""
    out = _OUT if _OUT is not None else sys.stdout
    out.write(json.dumps(obj) + "\n")
    out.flush()


LINE_LIMIT = 6144  # bytes: the driver keeps only the tail of stdout (r05's 28 KB line was cut mid-object and parsed as nothing)
EXTRA_FILE = "bench_extra.json"  # everything that is not the headline measurement (written next to bench.py, named in the line)

_LINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "value_long", "steps_long", "final_loss", "rows_per_step", "n_ranks_seen",
              "eager_ms_per_step", "note")
_CONFIG_KEYS = ("workload", "solver", "launch", "steps_per_graph_launch", "setup_seconds", "parallelism", "world_size", "dist_backend",
                "collectives_in_graph", "rows_global", "n_iwae_global")
_ROOFLINE_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source",
                  "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch", "mean_us", "launches_timed")
_CPU_KEYS = ("value", "unit", "cores", "ms_per_step", "kind", "sample", "rows_steps_per_s", "reference_over_oracle",
             "value_scaled_to_reference_best")


def _short(v, n=200):
    return v if not isinstance(v, str) or len(v) <= n else v[: n - 3] + "..."


def compact_line(full, extra_path=None):
    """The driver's line: the headline measurement, `roofline` and `cpu_baseline` with their contract keys and nothing nested
    beyond them.  Every other leg / note of `full` stays in the side file `extra_path` names."""
    line = {k: _short(full[k]) for k in _LINE_KEYS if k in full and (full[k] is not None or k == "vs_baseline")}
    cfg = full.get("config") or {}
    line["config"] = {k: _short(cfg[k], 260) for k in _CONFIG_KEYS if cfg.get(k) is not None}
    rf = full.get("roofline")
    if rf is not None:
        r = {k: _short(rf[k], 160) for k in _ROOFLINE_KEYS if k in rf and (rf[k] is not None or k == "traffic")}
        ib = rf.get("issue_bound")
        if isinstance(ib, dict):
            r["issue_bound"] = {k: ib[k] for k in ("frac", "frac_at_residency", "issue_time_us", "valu_insts_per_launch", "source")
                                if k in ib}
        line["roofline"] = r
    else:
        line["roofline"] = None
    cb = full.get("cpu_baseline")
    line["cpu_baseline"] = {k: _short(cb[k], 320) for k in _CPU_KEYS if k in cb} if cb is not None else None
    for k in ("strong_scaling_config3", "strong_scaling_config5"):
        leg = full.get(k)
        if isinstance(leg, dict):
            line[k] = {j: _short(leg[j], 120) for j in ("value", "unit", "ms_per_step", "steps", "scaling", "workload", "n_iwae_per_gpu",
                                                        "final_loss", "error", "skipped")
                       if j in leg}
    if extra_path is not None:
        line["extra"] = extra_path
    text = json.dumps(line, allow_nan=False)
    if len(text) >= LINE_LIMIT:  # (cannot happen with the keys above; a line that would be cut is worth less than a short one)
        for k in ("strong_scaling_config3", "strong_scaling_config5", "note"):
            line.pop(k, None)
        line["config"] = {k: line["config"][k] for k in ("workload", "solver", "launch") if k in line["config"]}
    return line


def emit_line(full):
    """Write the full result to EXTRA_FILE (best effort) and print the compact line."""
    path = os.path.join(ROOT, EXTRA_FILE)
    try:
        with open(path, "w") as f:
            json.dump(full, f, indent=1, default=str)
        named = EXTRA_FILE
    except OSError:
        named = None
    emit(compact_line(full, named))


def dump_outputs(path, loss, model):
    """--dump-outputs DIR: what a caller of the timed step holds after its last step -- the loss (-ELBO) and every trained
    parameter after that step's Adam update -- as DIR/<name>.npy in float32, so that two builds can be compared output for
    output on the same seeded inputs."""
    arrays = {"loss": loss}
    arrays.update(model.named_parameters())
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes of outputs, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def load_pmc(path):
    """A committed PMC reduction (profiles/make_pmc_*.py) and whether it was measured on THIS tree's kernel sources."""
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    from srcsha import csrc_sha16

    d = json.load(open(path))
    return d["kernels"], d.get("csrc_sha16") == csrc_sha16()


def algorithmic_bytes(B, S, T=N_TIMES, N=N_STATES, P=N_PARAMS):
    """fwd = read theta + write trajectory + write x_predict; bwd = read trajectory + write d theta."""
    fwd = 4 * (P * B * S + B * S * N * T + B * S * 4 * T)
    bwd = 4 * (B * S * N * T + P * B * S)
    return fwd, bwd


def ode_kernel_times(model, settings, batch, n_iwae, n_launch):
    """Average duration of the two ODE kernels of the training step, measured live: the step's own theta / inputs,
    `n_launch` back-to-back launches of vihds_ode_fwd (resp. vihds_ode_bwd, fed the broadcast [B,S] gradient the
    IWAE loss hands it in training) between ONE pair of HIP events recorded on the stream the launches go to.
    Back-to-back launches overlap their launch latency, so total / n_launch is the kernel's duration (this is what
    `rocprofv3 --kernel-trace --stats` reports for the same kernels: profiles/)."""
    import ctypes

    from vihds import hip

    with torch.no_grad():
        _results, theta, _q, _p = model(batch, n_iwae)
    ode = model.decoder.ode_model
    slots = hip.model_slots(ode.model_key)
    packed, row_of = theta.pack(slots)
    spec = ode._spec(settings, row_of, packed.shape[0])
    B, S, T = packed.shape[1], packed.shape[2], batch.times.shape[0]
    prob = spec.bind(B, S, T)
    prob.logp_grad_broadcast = 1
    dev = packed.device
    traj = torch.empty((T, spec.n_states, B, S), device=dev)
    xpred = torch.empty((T, 4, B, S), device=dev)
    logp = torch.empty((4, B, S), device=dev)
    g_logp = torch.full((B, S), -1.0 / (B * S), device=dev)
    g_theta = torch.empty_like(packed)
    L, st = hip.lib(), torch.cuda.current_stream()
    args = (packed.data_ptr(), batch.inputs.data_ptr(), batch.dev_1hot.data_ptr(), batch.times.data_ptr(),
            batch.observations.data_ptr(), None)

    def fwd():
        return L.vihds_ode_fwd(ctypes.byref(prob), *args, traj.data_ptr(), xpred.data_ptr(), logp.data_ptr(),
                               st.cuda_stream)

    def bwd():
        return L.vihds_ode_bwd(ctypes.byref(prob), *args, traj.data_ptr(), None, None, g_logp.data_ptr(),
                               g_theta.data_ptr(), None, None, st.cuda_stream)

    def fused():
        return L.vihds_ode_logp_grad(ctypes.byref(prob), *args[:5], logp.data_ptr(), g_theta.data_ptr(), st.cuda_stream)

    out = {}
    for name, fn in (("ode_fwd", fwd), ("ode_bwd", bwd), ("ode_fused", fused)):
        for _ in range(3):
            hip.check(fn(), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(n_launch):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        out[name] = {"mean_us": e0.elapsed_time(e1) * 1e3 / n_launch, "launches": n_launch}
    assert torch.isfinite(g_theta).all()
    return out


def make_oracle_step(solver, observations=None, n_iwae=N_IWAE, workload="dr_constant_icml", mode="train", rows=B_ROWS):
    """One full training step -- or, mode="eval", one evaluation pass (forward without grad + Results.init's summaries,
    reference training.py:283-307, utils.py:79-99) -- of the oracle (oracle/vihds_oracle.py: per-op [B,S] tensors, python
    time loop, autograd, Adam) on the bench workload, as a closure returning its wall time.  Shared by `cpu_baseline`
    below and by oracle/time_vs_reference.py (which times the imported reference beside it in the build container)."""
    from oracle import vihds_oracle as O
    from vihds import synthetic

    args, settings, data, parameters, model, training = synthetic.build(
        workload, rows, n_iwae, solver=solver, device="cpu", seed=0, observations=observations)
    N_IWAE_, B_ = n_iwae, rows
    enc = model.encoder
    model_key = settings.model
    ode = model.decoder.ode_model
    # relay_constant_precisions (config 5): aR / aS are sampled parameters (no device conditioner) and the precision network's
    # two Linear layers train with the encoder
    conditioned = [k for k in ("aR", "aS") if k not in enc.names and model_key != "dr_blackbox"]
    prec = getattr(ode, "precisions", None)
    prec_w = None
    if getattr(prec, "dynamic", False):
        prec_w = {"prod_w": prec.prec_production.weight, "prod_b": prec.prec_production.bias,
                  "degr_w": prec.prec_degradation.weight, "degr_b": prec.prec_degradation.bias}
        if getattr(prec, "n_hidden", 0) >= 1:
            prec_w.update({"hid_w": prec.prec_hidden.weight, "hid_b": prec.prec_hidden.bias})
    blackbox_kw, decoder_params = None, (list(prec.parameters()) if prec_w is not None else [])
    if model_key == "dr_blackbox":  # config 4: NeuralStates + NeuralPrecisions + the y offset layer (models/dr_blackbox.py)
        ns = ode.neural_states
        states_w = {"hid_w": ns.states_hidden.weight, "hid_b": ns.states_hidden.bias,
                    "prod_w": ns.states_production.weight, "prod_b": ns.states_production.bias,
                    "degr_w": ns.states_degradation.weight, "degr_b": ns.states_degradation.bias}
        blackbox_kw = dict(states_w=states_w, prec_w=prec_w, n_x=ode.n_x, n_y=ode.n_y, n_z=ode.n_z,
                           n_latent_species=ode.n_latent_species, init_latent_species=ode.init_latent_species,
                           init_prec=ode.init_prec)
        decoder_params = list(ode.parameters())
    opt = torch.optim.Adam(list(enc.parameters()) + decoder_params, lr=0.01)
    batch = training.train_data
    names = enc.names
    kinds = [d.kind for d in enc.descs]
    _, pm, pp = enc.p.image("cpu", 1)
    p_mu, p_prec = [pm[i, 0] for i in range(len(names))], [pp[i, 0] for i in range(len(names))]
    rel = {k: torch.tensor(v) for k, v in settings.data.relevance_vectors.items()}

    def forward():
        u = torch.tensor(np.random.randn(B_, N_IWAE_, len(names)).astype(np.float32))
        q = enc(batch)
        _, q_mu, q_prec = q.image("cpu", B_)
        qm = [q_mu[i][:, None] for i in range(len(names))]
        qp = [q_prec[i][:, None] for i in range(len(names))]
        th = O.sample_clip_theta(names, kinds, qm, qp, p_mu, p_prec, u)
        ones = torch.ones(B_, N_IWAE_)
        for k in conditioned:
            w = 2.0 + 1.5 * torch.randn(1, batch.dev_1hot.shape[1])
            th[k] = O.device_conditioner(w, ones, rel[k], batch.dev_1hot, True)
        th_sim, bb = th, None
        if blackbox_kw is not None:  # condition_theta: the ODE sees y + offset_layer(dev_1hot), log q / log p the sampled y
            th_sim = dict(th)
            off = ode.offset_layer(batch.dev_1hot.unsqueeze(1).repeat([1, N_IWAE_, 1]))
            for i in range(ode.n_y):
                th_sim["y%d" % (i + 1)] = th["y%d" % (i + 1)] + off[:, :, i]
            bb = dict(blackbox_kw, dev_1hot=batch.dev_1hot)
        xs, xp, prc = O.decode(model_key, th_sim, batch.inputs, batch.times, solver, prec_w=prec_w, blackbox=bb)
        lpo = O.log_prob_observations(xp, batch.observations, prc)
        vals = [th[n] for n in names]
        loss, log_w = O.iwae_loss(lpo, O.chained_log_prob(kinds, p_mu, p_prec, vals), O.chained_log_prob(kinds, qm, qp, vals))
        return loss, log_w, xs, xp, prc

    def one_step():
        t0 = time.perf_counter()
        if mode == "eval":
            with torch.no_grad():
                loss, log_w, xs, xp, prc = forward()
                O.importance_weighted_summaries(log_w, xp, xs, prc)
        else:
            loss = forward()[0]
            loss.backward()
            opt.step()
            opt.zero_grad()
        return time.perf_counter() - t0

    return one_step


def cpu_baseline(solver, observations, seconds_budget=20.0, max_steps=8, n_iwae=N_IWAE, workload="dr_constant_icml",
                 n_times=None, mode="train", rows=B_ROWS, probe_threads=None):
    """The oracle timed on this box's host cores on the same workload.  Checker code used as a *reported baseline*
    only.  Rows for 1 thread, 8 threads and all host threads; `value` is the best of them.  `fidelity` echoes
    oracle/cpu_fidelity.json: the same oracle step timed against the imported reference in the build container."""
    all_threads = torch.get_num_threads()
    one_step = make_oracle_step(solver, observations, n_iwae, workload, mode, rows)
    # the tensors are tiny (7 200 elements), so more threads is not faster: probe 1 / 8 / all host threads and time
    # the baseline with whichever is quickest on this box (probe_threads: a fixed list, for the bounded legs)
    probe = {}
    for n in sorted(set(probe_threads) if probe_threads else {1, min(8, all_threads), all_threads}):
        torch.set_num_threads(n)
        if not probe_threads:
            one_step()
        probe[n] = one_step()
    threads = min(probe, key=probe.get)
    torch.set_num_threads(threads)
    times_s = []
    t_all = time.perf_counter()
    while len(times_s) < max_steps and (time.perf_counter() - t_all) < seconds_budget:
        times_s.append(one_step())
    steps = len(times_s)
    torch.set_num_threads(all_threads)
    med = float(np.median(times_s))
    out = {"value": 1.0 / med, "unit": "steps/s" if mode == "train" else "passes/s", "cores": threads, "kind": "port",
           "sample": "%d %s of the same workload (B=%d, n_iwae=%d, T=%d, %s), median; eager PyTorch "
                     "CPU restatement of the reference path (oracle/); %d threads chosen from a probe of %s "
                     "(s/step); box has %d host threads"
                     % (steps, "full training steps" if mode == "train" else "evaluation passes (forward without grad + "
                        "Results.init summaries)", rows, n_iwae, n_times or N_TIMES, solver, threads,
                        {k: round(v, 2) for k, v in probe.items()}, all_threads),
           "ms_per_step": 1e3 * med,
           "rows_steps_per_s": {("%d thread%s" % (k, "" if k == 1 else "s")): round(1.0 / v, 3) for k, v in probe.items()}}
    fid = os.path.join(ROOT, "oracle", "cpu_fidelity.json")
    if os.path.exists(fid) and workload == "dr_constant_icml":
        fidelity = json.load(open(fid))
        out["fidelity"] = fidelity
        # how the timed restatement stands against the imported reference (build container, oracle/time_vs_reference.py):
        # per thread count, and best thread count of each against the other's best -- the reference's own op program is quickest on
        # ONE thread, the oracle's on eight, and best against best the reference is the faster (ratio < 1)
        rows_f = fidelity["rows"]
        ref_best = min(r["reference_modeuler_s_per_step"] for r in rows_f.values())
        ora_best = min(r["oracle_modeuler_s_per_step"] for r in rows_f.values())
        out["reference_over_oracle"] = dict({k: r["reference_over_oracle_modeuler"] for k, r in rows_f.items()},
                                            best_vs_best=round(ref_best / ora_best, 4), solver="modeuler",
                                            source="oracle/cpu_fidelity.json")
        out["value_scaled_to_reference_best"] = out["value"] * ora_best / ref_best
    if workload == "relay_constant_precisions":
        out["note"] = ("no reference timing exists beside this one: the reference's classes for this model raise at "
                       "construction (relay_constant.py:17,201); the oracle restates its equations and is pinned on the "
                       "MODIFIED reference's outputs (tests/golden/make_fixtures.py --patched)")
    return out


# ---- the other BASELINE configurations: same JSON contract, `--workload NAME` ------------------------
ISSUE_CYCLES_FULL_SIMD, ISSUE_CYCLES_TWO_WAVES = 3.0, 3.6  # measured: profiles/r04_issue_rate.log (see issue_bound)
MFMA_F32_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32 MFMA peak (no TF32 on gfx950)
BLACKBOX_FLOP_PER_EVAL = 3390  # 2 (27 25 + 2 25 6) + 2 (28 20 + 2 20 4) per RHS evaluation and trajectory
WORKLOAD_TABLE = {
    # name: (synthetic workload, rows, n_iwae, solver, mode, bound, what BASELINE.json calls it)
    "config2": ("dr_constant_icml", 36, 200, "rk4", "train", "hbm", "configs[1]"),
    "config3_train": ("dr_constant_icml", 36, 1000, "rk4", "train", "hbm", "configs[2], training shape (one batch, n_iwae=1000)"),
    "config3_eval": ("dr_constant_icml", 234, 1000, "rk4", "eval", "hbm", "configs[2], evaluation shape (all 234 rows, n_iwae=1000)"),
    "config3_eval_stored": ("dr_constant_icml", 234, 1000, "rk4", "eval", "hbm",
                            "configs[2], evaluation shape, params.online_summaries: false -- the trajectory through HBM"),
    "config4": ("dr_blackbox_icml", 36, 200, "midpoint", "train", "mfma", "configs[3]"),
    "config5": ("relay_constant_precisions", 36, 200, "midpoint", "train", "hbm", "configs[4]"),
    # the dr_blackbox kernels with the chip FULL (2 250 groups of 16 trajectories on 1 024 SIMDs; configs[3] itself is 450): what
    # their matrix-core utilisation is when every SIMD has work
    "config4_s1000": ("dr_blackbox_icml", 36, 1000, "midpoint", "train", "mfma", "configs[3] at n_iwae=1000"),
}
LAUNCH_KERNELS = {  # launch name (ops._launch) -> substrings of the kernels it can run, for the PMC lookup
    "decoder_step": ["dr_scan_train_theta_kernel"],
    "ode_logp_grad": ["dr_scan_train_kernel"],
    "ode_fwd": ["bb_split_fwd_kernel", "bb_mfma_fwd_kernel", "relay_lane_fwd_kernel", "dr_lane_fwd_kernel", "ode_fwd_kernel"],
    "ode_bwd": ["bb_split_bwd_kernel", "bb_mfma_bwd_kernel", "relay_lane_bwd_kernel", "dr_lane_bwd_kernel", "ode_bwd_kernel"],
    "ode_fwd_summaries": ["ode_fwd_summ_kernel"],
}


def time_launch(fn, n):
    st = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(n):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def run_workload(a, name, min_seconds=None, bounded_cpu=False):
    """Returns the JSON object of one of BASELINE.json's other configurations (None on ranks other than 0).  min_seconds:
    the timed window is sized from a short trial instead of --steps (the `--all-legs` legs: >= that many seconds
    each).  bounded_cpu: the cpu_baseline leg runs at 8 threads without the thread probe, two samples.
    One of BASELINE.json's other configurations through the same host path: timed loop (barrier + synchronize on
    both sides, max over ranks), then the step's own ODE launches re-issued back to back between one HIP event pair for
    the roofline object.  N > 1: --shard samples splits the ONE batch's IWAE-sample axis over the ranks (strong
    scaling, the partitioning BASELINE config 3 names); --shard rows replicates the batch per rank (weak)."""
    from vihds import hip, ops, parallel, synthetic

    wl, B, S, solver, mode, bound, cfg_note = WORKLOAD_TABLE[name]
    if a.solver_given:
        solver = a.solver
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run --nproc-per-node N)"
                         % (a.gpus, world))
    shard = parallel.init_from_env()
    rank = shard.rank if shard is not None else 0
    replica = None
    strong = shard is not None and a.shard == "samples" and mode == "train"
    if shard is not None and not strong:
        replica, shard = parallel.RowReplica(shard.rank, shard.world, shard.group), None
    if strong and S % world:
        raise SystemExit("n_iwae=%d does not split over %d ranks" % (S, world))
    multi = world > 1
    local_rank = int(os.environ.get("VIHDS_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local_rank)
    dev = "cuda:%d" % local_rank
    use_graph = not a.eager
    extra = {}
    if a.stored_trajectory_eval or name.endswith("_stored"):
        extra["online_summaries"] = False
    if wl == "dr_constant_icml":
        extra["fused_ode_training"] = not a.two_kernel_ode
        extra["fused_iwae_backward"] = not a.no_fused_iwae
        extra["fused_step_tail"] = not a.no_step_tail
    args, settings, data, parameters, model, training = synthetic.build(
        wl, B, S, solver=solver, device=dev, seed=a.seed, shard=shard, replica=replica, u_rng=a.device_rng,
        conditioner_rng=a.device_rng, hip_graph=use_graph, nan_check_every=0, learning_rate=a.lr, **extra)
    batch = training.train_data
    if mode == "train":
        model.train()
        step = training.graph_step if use_graph else training.step
    else:
        model.eval()

        def step(bt):  # training.py:183-215 (_evaluate_elbo_and_plot): forward without grad + Results.init summaries
            return training.evaluate(bt, S).elbo  # (Results on the host, every pass; replayed from a hipGraph unless --eager)

    def barrier():
        torch.cuda.synchronize()
        if multi:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    if use_graph:
        step(batch)
    n_steps, n_warm = a.steps, a.warmup
    if min_seconds is not None:
        for _ in range(5):
            step(batch)
        barrier()
        t0 = time.perf_counter()
        for _ in range(20):
            step(batch)
        barrier()
        per = (time.perf_counter() - t0) / 20
        n_steps, n_warm = max(50, int(math.ceil(min_seconds / per))), 20
    for _ in range(n_warm):
        loss = step(batch)
    barrier()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        loss = step(batch)
    barrier()
    elapsed = time.perf_counter() - t0
    if multi:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt)
    final = float(torch.as_tensor(loss).float().mean())
    if mode == "train" and (not np.isfinite(final) or final < -1e6):  # (the headline's own guard, on every training leg)
        raise SystemExit("degenerate objective %r after the timed steps (training ran away): not a valid bench run" % final)
    if not np.isfinite(final):
        raise SystemExit("non-finite objective %r after the timed passes: not a valid bench run" % final)

    # ---- roofline (--full): the step's own ODE launches, re-issued back to back -------------------------------------
    rec = ops.LaunchRecorder()
    if a.full:
        ops.TIMER = rec
        if mode == "train":
            training.step(batch)
        else:
            training._evaluation_device_side(batch, S)  # (the pass's own launches, eager: a graph replay records none)
        ops.TIMER = None
    ode = model.decoder.ode_model
    T = int(batch.times.shape[0])
    P = len(model.encoder.names)
    N = int(hip.lib().vihds_model_n_states(hip.MODELS[ode.model_key]))
    s_local = S // world if strong else S
    # (evaluation passes with params.lazy_x_predict: vihds_ode_fwd is handed xpred == NULL, so x_predict leaves the numerator)
    stores_xpred = not (mode == "eval" and bool(settings.params.get("lazy_x_predict", True)))
    fwd_b = 4 * (P * B * s_local + B * s_local * N * T + (B * s_local * 4 * T if stores_xpred else 0))
    bwd_b = 4 * (B * s_local * N * T + P * B * s_local)
    theta_b = 4 * (2 * P * B * s_local + 2 * B * s_local)
    n_eval = (T - 1) * {"euler": 1, "rk4": 4}.get(solver, 2)
    fwd_f = BLACKBOX_FLOP_PER_EVAL * n_eval * B * s_local
    work = {"decoder_step": (fwd_b + bwd_b + theta_b, 3 * fwd_f), "ode_logp_grad": (fwd_b + bwd_b, 3 * fwd_f),
            "ode_fwd": (fwd_b, fwd_f), "ode_bwd": (bwd_b, 2 * fwd_f),
            # (the evaluation's second forward pass: the same fixed numerator -- what the pair "forward with the trajectory
            # through HBM" moves per pass -- although this kernel itself moves theta and 26 MB of partial sums: see traffic)
            "ode_fwd_summaries": (fwd_b, fwd_f)}
    timed = {k: time_launch(fn, max(10, a.roofline_steps // 2)) for k, fn in rec.calls.items() if k in work}
    import glob
    pmc = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc_hbm_traffic.json" % name)), reverse=True):
        ks, fresh = load_pmc(f)
        pmc = {"file": os.path.basename(f), "kernels": ks if fresh else {}, "stale": not fresh}
        break

    def traffic_of(launch):
        # (the profiled run also holds a few launches of other kernel families -- warm-ups, the roofline leg's probes: the
        # workload's own kernel is the candidate with the most dispatches)
        best = None
        for sub in LAUNCH_KERNELS[launch]:
            for k, v in pmc.get("kernels", {}).items():
                if sub in k and (best is None or v.get("dispatches", 0) > best[1].get("dispatches", 0)):
                    best = (k, v)
        return (best[0], best[1]["hbm_bytes_corrected"]) if best else (None, None)

    def entry(k):
        us = timed[k]
        kname, tr = traffic_of(k)
        if bound == "mfma":
            ach, unit, peak, num = work[k][1] / (us * 1e-6) / 1e12, "TFLOP/s", MFMA_F32_PEAK_TFLOPS, work[k][1]
        else:
            ach, unit, peak, num = work[k][0] / (us * 1e-6) / 1e9, "GB/s", HBM_PEAK_GBS, work[k][0]
        return {"launch": k, "kernel": kname, "mean_us": us, "achieved": ach, "unit": unit, "peak": peak,
                "frac": ach / peak, "algorithmic_%s_per_launch" % ("flops" if bound == "mfma" else "bytes"): num,
                "traffic": tr}

    if rank != 0:
        return None
    roofline = None
    if timed:
        dom = max(timed, key=timed.get)
        d = entry(dom)
        roofline = {"bound": bound, "kernel": d["kernel"] or dom, "launch": dom, "achieved": d["achieved"],
                    "peak": d["peak"], "unit": d["unit"], "frac": d["frac"], "traffic": d["traffic"],
                    "traffic_source": ("profiles/%s" % pmc["file"]) if d["traffic"] is not None else None,
                    "mean_us": d["mean_us"], "launches_timed": max(10, a.roofline_steps // 2),
                    "timing": "back-to-back launches of the step's own launch closure between one HIP event pair on the "
                              "launch stream",
                    "numerator_note": ("SURVEY 8d: %d flop per RHS evaluation and trajectory x %d evaluations x %d "
                                       "trajectories forward, backward counted as 2x forward" % (BLACKBOX_FLOP_PER_EVAL, n_eval, B * s_local))
                    if bound == "mfma" else ("SURVEY 8d fixed numerator: fwd = theta + trajectory + x_predict, bwd = trajectory + d theta"
                                                            if stores_xpred else
                                                            "SURVEY 8d numerator without the x_predict term (fwd = theta + trajectory): "
                                                            "the evaluation pass does not store x_predict (params.lazy_x_predict)"),
                    "other_kernels": [entry(k) for k in timed if k != dom]}
        mf = os.path.join(ROOT, "profiles", "%s_mfma_busy.json" % name)
        if not os.path.exists(mf):  # (per-round files: the newest r*_<name>_mfma_busy.json)
            cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_mfma_busy.json" % name)), reverse=True)
            mf = cand[0] if cand else mf
        if bound == "mfma" and os.path.exists(mf):
            roofline["mfma_busy"] = json.load(open(mf))
    what = "training steps" if mode == "train" else "evaluation passes"
    scale = 1 if (strong or not multi) else world
    out = {
        "metric": "ELBO %s/sec (%s, n_iwae=%d)" % (what, wl, S), "value": scale * n_steps / elapsed,
        "unit": "steps/s" if mode == "train" else "passes/s", "n_gpus": world, "steps": n_steps, "warmup": n_warm,
        "ms_per_step": 1e3 * elapsed / n_steps, "higher_is_better": True,
        "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s (BASELINE.json %s): B=%d rows x n_iwae=%d, N=%d states, T=%d, P=%d, %s, %s"
                               % (wl, cfg_note, B, S, N, T, P, solver,
                                  "full training step (encoder+theta+ODE+IWAE fwd/bwd+Adam)" if mode == "train" else
                                  "evaluation pass (forward without grad writing the log-likelihoods only, the importance-weighted summaries from a second forward launch that adds them up on the way: no trajectory through HBM; the [B,.,T] summaries, q and the ELBO are copied to the host, the theta samples [P,B,S] stay on the device until Results.theta / dump() reads them)"
                                  if bool(settings.params.get("online_summaries", True)) else
                                  "evaluation pass (forward without grad, trajectories through HBM, IW summaries on device; the [B,.,T] summaries, q and the ELBO are copied to the host, the theta samples [P,B,S] stay on the device until Results.theta / dump() reads them)"),
                   "name": name, "solver": solver, "n_iwae_per_gpu": s_local, "n_iwae_global": S,
                   "rows_global": B * (world if replica is not None else 1),
                   "launch": "hipGraph replay" if use_graph else "eager", "learning_rate": a.lr,
                   "batch_staging": "the batch is resident in HBM; its staging copies and delta_obs (reference "
                                    "encoders.py:385) are outside the replayed step",
                   "parallelism": ("single GPU" if world == 1 else
                                   "iwae-sample shard x%d of ONE batch (all-gather of row statistics + one gradient all-reduce "
                                   "per step)" % world if strong else
                                   "data parallel over rows x%d (one gradient all-reduce per step)" % world)},
        "final_objective": final, "roofline": roofline,
    }
    if a.full and world == 1 and not a.no_cpu_baseline:
        # the oracle on this box's host cores: a training step (white-box models and, since round 4, dr_blackbox) or an
        # evaluation pass; the evaluation shape's sample is 36 of its 234 rows (the pass is row-wise independent; 234 rows
        # x 1000 samples of eager [B,S] tensors would be minutes), scaled to passes of the full shape
        cpu_rows = B if mode == "train" else min(B, 36)
        obs_cpu = batch.observations.detach().cpu()[:cpu_rows].contiguous()
        cb = cpu_baseline(solver, obs_cpu, n_iwae=S, max_steps=2 if bounded_cpu else 4, workload=wl, n_times=T, mode=mode,
                          rows=cpu_rows, probe_threads=[min(8, torch.get_num_threads())] if bounded_cpu else None,
                          seconds_budget=15.0 if bounded_cpu else 20.0)
        if cpu_rows != B:
            cb["value"] *= cpu_rows / B
            cb["ms_per_step"] *= B / cpu_rows
            cb["sample"] += "; timed on %d of the %d rows (row-wise independent work), value scaled by %d/%d" % (cpu_rows, B, cpu_rows, B)
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu_restatement"] = out["value"] / cb["value"]
    else:
        out["cpu_baseline"] = None
    return out


def newton_summary(hist):
    """{mean, p99, max, ...} of the time-parallel decoder kernel's Newton walks per wavefront (vihds_debug_newton_hist)."""
    h = [int(v) for v in hist[:33]]
    n = sum(h)
    if n == 0:
        return None
    cum, p99 = 0, 0
    for w, c in enumerate(h):
        cum += c
        if cum >= 0.99 * n:
            p99 = w
            break
    return {"wavefront_launches": n, "mean": sum(w * c for w, c in enumerate(h)) / n, "p99": p99,
            "max": max(w for w, c in enumerate(h) if c), "hist": {str(w): c for w, c in enumerate(h) if c},
            "first_order_exit_frac": int(hist[33]) / n,
            "note": "walks of the OD chain per wavefront (two trajectories) of dr_scan_train_theta_kernel's Newton iteration; "
                    "1 = the closed-form guess was already settled, 2 = the usual case"}


REAL_PLATE_NPZ = os.path.join(ROOT, "tests", "golden", "trace_dr_constant_icml_modeuler.npz")


def run_loop_legs(a, plate="synthetic", leg_names=None, epochs=None, telemetry=True, stream_seed=None):
    """`Training.run()` itself -- the loop a user of run_xval.py runs (reference training.py:342-383) -- on a dr_constant_icml
    plate of the reference's size: 234 training rows in batches of 36 (six full batches and a ragged one of 18 per epoch,
    shuffled by the reference's own DataLoader sampler), n_iwae = 200, evaluation of the training and the validation rows at
    1000 samples every `test_epoch` epochs (the reference's default, 20), with the fast keys of the headline bench.
    plate = "synthetic": the seeded synthetic plate at --lr; "real": the reference's processed plate (the 312 wells recorded in
    tests/golden/trace_dr_constant_icml_modeuler.npz, its own 234 / 78 split) with the spec's learning_rate 0.01 and MultiStepLR
    [250, 1000] unchanged.  value = optimizer steps / wall time of run(), evaluations and host work included.  Legs: one graph
    launch per epoch (run()'s default with hip_graph when the NaN check is at most once per epoch), one per step with the same
    check, one per step with the check after every step as the reference has it.  telemetry: the decoder kernel's Newton walks."""
    import contextlib
    import io

    from vihds import hip, synthetic

    torch.cuda.set_device(0)
    solver = a.solver or "rk4"
    n_rows, n_batch, S, S_eval = 234, 36, 200, 1000
    epochs = epochs or max(100, a.steps // 7)
    test_epoch = 20
    all_legs = (("epoch_graph_nan_check_per_epoch", 7, True), ("step_graphs_nan_check_per_epoch", 7, False),
                ("step_graphs_nan_check_every_step", 1, False))
    legs = {}
    for name, check, epoch_graph in all_legs:
        if leg_names is not None and name not in leg_names:
            continue
        keys = dict(u_rng=a.device_rng, conditioner_rng=a.device_rng, hip_graph=not a.eager, nan_check_every=check,
                    epoch_graph=epoch_graph, lazy_cache_dump=epoch_graph, epoch_lookahead=epoch_graph, fused_ode_training=True,
                    fused_iwae_backward=True, fused_step_tail=not a.no_step_tail)
        hist = torch.zeros(34, dtype=torch.int32, device="cuda:0") if telemetry else None
        hip.lib().vihds_debug_newton_hist(hip.ptr(hist))  # (before the captures: a captured launch keeps its pointer)
        try:
            if plate == "real":
                args, settings, data, parameters, model, training = synthetic.build_recorded_plate(
                    REAL_PLATE_NPZ, S, solver=solver, device="cuda:0", seed=0, **keys)
            else:
                args, settings, data, parameters, model, training = synthetic.build(
                    "dr_constant_icml", n_rows, S, solver=solver, device="cuda:0", seed=a.seed, n_batch=n_batch,
                    learning_rate=a.lr, **keys)
            if stream_seed is not None:
                # the split and the initial weights stay the recorded ones (seed 0: the reference's); only the run's random
                # streams -- the draws u, the conditioner's weights, the loader's shuffles -- start somewhere else
                np.random.seed(1000 + stream_seed)
                torch.manual_seed(1000 + stream_seed)
            args.epochs, args.test_epoch, args.test_samples = 2, 1, S_eval
            with contextlib.redirect_stdout(io.StringIO()):
                training.run()  # captures, allocator warm-up, one evaluation: not timed
            if hist is not None:
                torch.cuda.synchronize()
                hist.zero_()
            args.epochs, args.test_epoch = epochs, test_epoch
            steps_per_epoch = (len(data.train) + n_batch - 1) // n_batch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                out = training.run()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        finally:
            hip.lib().vihds_debug_newton_hist(None)
        n_steps, n_eval = epochs * steps_per_epoch, epochs // test_epoch
        stopped = "Cannot proceed" in buf.getvalue()
        legs[name] = {"value": n_steps / el, "ms_per_step": 1e3 * el / n_steps, "wall_s": el, "epochs": epochs, "steps": n_steps,
                      "evaluations": n_eval, "final_validation_elbo": float(out.elbo) if out is not None else None,
                      "stopped_on_nan": stopped, "learning_rate": float(settings.params.learning_rate),
                      "learning_boundaries": list(settings.params.learning_boundaries),
                      "newton_iters": newton_summary(hist.cpu().tolist()) if hist is not None else None}
        del training, model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return legs


def run_loop_workload(a):
    """--workload run_loop: the three legs of run_loop_legs on the synthetic plate, as a line of its own."""
    if int(os.environ.get("WORLD_SIZE", "1")) != 1 or a.gpus != 1:
        raise SystemExit("--workload run_loop is a single-process measurement")
    legs = run_loop_legs(a, "synthetic")
    best = legs["epoch_graph_nan_check_per_epoch"]
    emit(({
        "metric": "ELBO training steps/sec through Training.run() (dr_constant_icml, n_iwae=200)", "value": best["value"],
        "unit": "steps/s", "n_gpus": 1, "steps": best["steps"], "warmup": 2 * 7, "ms_per_step": best["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "Training.run(): 234 rows in batches of 36 (ragged last batch of 18), n_iwae=200, T=86, %s, "
                               "evaluation of train + validation rows at n_iwae=1000 every 20 epochs; rows resident in HBM, "
                               "batches gathered on the device by row index (vihds_gather_batch), one hipGraph per EPOCH "
                               "holding its seven gather + step pairs, fed by one copy of the epoch's row indices"
                               % (a.solver or "rk4"),
                   "name": "run_loop", "launch": "eager" if a.eager else "hipGraph replay (one epoch = 7 steps per launch)",
                   "learning_rate": a.lr},
        "legs": legs, "roofline": None, "cpu_baseline": None,
        "note": "end-to-end loop figure next to the headline's resident-batch replay (python bench.py): the difference is the "
                "per-step host work (sampler, index copy, graph launch), the ragged batch and the evaluations"}))


def loop_legs_for_default_line(a):
    """`run_loop` (synthetic plate, --lr) and `real_plate` (the reference's processed plate at the spec's own learning rate and
    schedule) for `--all-legs` (bench_extra.json): Training.run() end to end, one graph launch per epoch, with the decoder kernel's Newton
    telemetry.  A failure is reported in the object, never raised."""
    out = {}
    for key, plate, epochs in (("run_loop", "synthetic", 200), ("real_plate", "real", 300)):
        t0 = time.perf_counter()
        try:
            name = "epoch_graph_nan_check_per_epoch"
            if plate == "real":
                # The spec's learning rate (0.01) on this objective is not stable for every random stream: the reference's own
                # clip-after-sample log q lets q collapse onto a clipped sample (-ELBO -> -1e19) for some draws -- with the
                # reference's own keys (numpy stream, modeuler) as with these; tests/probe/runaway_seeds.py, DESIGN.md.  Four
                # streams are run and every final validation ELBO is reported.
                runs = [run_loop_legs(a, plate, leg_names=(name,), epochs=epochs, stream_seed=k)[name] for k in range(4)]

                def ran_away(r):
                    v = r["final_validation_elbo"]
                    return v is None or not np.isfinite(v) or abs(v) > 1e6

                # (a stream whose objective ran away measures nothing: `value` is the median throughput of the streams that
                # stayed finite, the others are counted and listed -- VERDICT r05 weak #10)
                finite = [r for r in runs if not ran_away(r)]
                pool = sorted(finite or runs, key=lambda r: r["value"])
                leg = dict(pool[len(pool) // 2])
                leg["final_validation_elbo_by_stream"] = [r["final_validation_elbo"] for r in runs]
                leg["value_by_stream"] = [r["value"] for r in runs]
                leg["runaway_streams"] = len(runs) - len(finite)
                leg["value_is_median_of"] = "%d finite streams" % len(finite) if finite else "all streams (every one ran away)"
            else:
                leg = run_loop_legs(a, plate, leg_names=(name,), epochs=epochs)[name]
            leg["unit"] = "steps/s"
            leg["data"] = ("synthetic plate (vihds/synthetic.py), 234 rows" if plate == "synthetic" else
                           "the reference's processed ICML plate: 312 wells from data/*.csv through datasets.py:173-224, recorded "
                           "in tests/golden/trace_dr_constant_icml_modeuler.npz; 234 train / 78 validation rows (its own split)")
            leg["workload"] = ("Training.run(): batches of 36 (ragged last 18), n_iwae=200, rk4, evaluation of train + validation "
                               "rows at n_iwae=1000 every 20 epochs, one hipGraph launch per epoch queued ahead of the look at the previous epoch's losses, fast keys")
            out[key] = leg
        except BaseException as exc:  # noqa: BLE001
            out[key] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
        out[key]["leg_wall_s"] = time.perf_counter() - t0
    return out


def strong_scaling_leg(a, dev, world, rank, workload="dr_constant_icml", S=1000, solver=None, label="config3_train"):
    """BASELINE config 3's partitioning next to the headline's weak-scaling line: ONE batch (36 rows, n_iwae = 1000) with its
    IWAE-sample axis sharded over the ranks (all-gather of the row statistics + one gradient all-reduce per step; same code
    as `--workload config3_train --shard samples`).  Returned as an object of the same JSON line; a failure is reported
    in it, never raised (the headline line must come out)."""
    from vihds import parallel, synthetic

    try:
        if S % world:
            return {"skipped": "n_iwae=%d does not split over %d ranks" % (S, world)}
        shard = parallel.SampleShard(rank, world)
        extra = {"fused_ode_training": not a.two_kernel_ode} if workload == "dr_constant_icml" else {}
        args, settings, data, parameters, model, training = synthetic.build(
            workload, B_ROWS, S, solver=solver or a.solver, device=dev, seed=a.seed, shard=shard, u_rng=a.device_rng,
            conditioner_rng=a.device_rng, hip_graph=not a.eager, nan_check_every=0, learning_rate=a.lr, **extra)
        model.train()
        batch = training.train_data
        step = training.step if a.eager else training.graph_step
        step(batch)
        for _ in range(5):
            step(batch)
        n = 50
        torch.cuda.synchronize()
        torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = step(batch)
        torch.cuda.synchronize()
        torch.distributed.barrier()
        el = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(el, op=torch.distributed.ReduceOp.MAX)
        el = float(el)
        return {"workload": "%s: ONE batch of 36 rows, n_iwae=%d sharded over the ranks (--shard samples)" % (label, S),
                "scaling": "strong", "value": n / el, "unit": "steps/s", "ms_per_step": 1e3 * el / n, "steps": n,
                "n_iwae_per_gpu": S // world, "final_loss": float(loss)}
    except Exception as e:  # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def unchanged_spec_leg(a, dev, min_seconds):
    """The headline workload with NONE of this implementation's opt-in keys: what `run_xval.py --gpu 0 <spec>.yaml` runs
    when the YAML is the reference's own -- u from numpy's global RandomState (vae.py:22-24; drawn by vihds/nprand.py, the
    same numbers), the conditioner's weights from torch's CPU generator, the reference's look at every step's ELBO
    (training.py:331-334).  Round 4: the value-preserving fast keys are on by default (fused decoder step, step tail, graph
    replay with the host draws staged).  rk4 like the headline (the spec's own default solver is midpoint)."""
    from vihds import synthetic

    args, settings, data, parameters, model, training = synthetic.build(
        "dr_constant_icml", B_ROWS, N_IWAE, solver=a.solver, device=dev, seed=a.seed, learning_rate=a.lr)
    model.train()
    batch = training.train_data

    from vihds.utils import TrainingLogData

    log = TrainingLogData()

    def step():  # the body of Training.run()'s loop for one resident batch: the step and the reference's per-step NaN check
        if not training._run_batch(time.time(), batch, log, next_batch=batch, ahead=2):  # (the same resident batch follows, twice)
            raise SystemExit("NaN objective in the unchanged-spec leg")

    for _ in range(50):  # (the capture and its warm-up steps happen in here; the helper thread and its pool come up)
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        step()
    torch.cuda.synchronize()
    n = max(500, int(math.ceil(min_seconds / ((time.perf_counter() - t0) / 100))))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    loss = training._pending_elbo if training._pending_elbo is not None else torch.tensor(float("nan"))
    p = settings.params
    return {"metric": "ELBO training steps/sec (dr_constant_icml, n_iwae=200), reference-default keys", "value": n / el,
            "unit": "steps/s", "steps": n, "ms_per_step": 1e3 * el / n, "final_loss": float(loss),
            "config": {"workload": "the headline workload with no opt-in key set (params.fast off)", "solver": a.solver,
                       "u_rng": p.u_rng, "conditioner_rng": p.conditioner_rng, "hip_graph": p.hip_graph,
                       "graph_replay": bool(training.use_graph), "nan_check_every": int(p.nan_check_every),
                       "learning_rate": a.lr,
                       "launch": "Training._run_batch per step: the reference's RNG streams (numpy u from native code, bit for "
                                 "bit; CPU-drawn conditioner weights) staged into the replayed step, the loss of every step "
                                 "read on the host (one step late)"}}


def distributed_path_leg(a, plain_ms):
    """The headline workload as a ONE-rank job through the distributed path (torch.distributed over RCCL, RowReplica: the
    gradient all-reduce, the captured step with the collective inside the graph or cut at it) next to the plain one-process
    number: what the multi-GPU machinery costs per step before any wire latency.  A child process (its own communicator)."""
    import socket
    import subprocess

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               VIHDS_FORCE_DIST="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", "2000", "--warmup", "200", "--no-cpu-baseline",
           "--no-other-configs", "--no-strong-leg", "--roofline-steps", "0", "--seed", str(a.seed), "--lr", str(a.lr)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if not line:
        return {"error": "rc %d: %s" % (out.returncode, (out.stderr or out.stdout)[-300:])}
    d = json.loads(line[-1])  # (a child that died in the process group's teardown behind its line has still measured)
    keep = {k: d.get(k) for k in ("value", "ms_per_step", "steps", "launch", "world_size", "dist_backend",
                                  "collectives_in_graph", "steps_per_graph_launch")}
    keep["overhead_us_per_step_vs_plain"] = 1e3 * (d["ms_per_step"] - plain_ms)
    keep["ratio_to_plain"] = plain_ms / d["ms_per_step"]
    return keep


def other_config_legs(a, dev):
    """The other single-GPU BASELINE configurations and the unchanged-spec path, each timed for >= --leg-seconds inside the
    `--all-legs` command, written to bench_extra.json under `other_configs` (never into the driver's line).  A leg that fails reports its
    error; it never takes the headline line with it."""
    legs = {}
    for name in ("config3_train", "config3_eval", "config3_eval_stored", "config4", "config5", "config4_s1000"):
        t0 = time.perf_counter()
        try:
            # (no CPU leg: 36 000 trajectories of eager [B,S] tensors would be a minute per step; config3_eval has the pass's)
            no_cpu = name in ("config4_s1000", "config3_eval_stored")
            if no_cpu:
                keep_cb, a.no_cpu_baseline = a.no_cpu_baseline, True
            out = run_workload(a, name, min_seconds=a.leg_seconds, bounded_cpu=True)
            if no_cpu:
                a.no_cpu_baseline = keep_cb
            keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "config", "final_objective", "roofline",
                    "cpu_baseline", "speedup_vs_cpu_restatement")
            legs[name] = {k: out[k] for k in keep if k in out}
        except BaseException as exc:  # noqa: BLE001 (SystemExit included: a leg must not end the run)
            legs[name] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
        legs[name]["leg_wall_s"] = time.perf_counter() - t0
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    t0 = time.perf_counter()
    try:
        legs["unchanged_spec"] = unchanged_spec_leg(a, dev, a.leg_seconds)
    except BaseException as exc:  # noqa: BLE001
        legs["unchanged_spec"] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
    legs["unchanged_spec"]["leg_wall_s"] = time.perf_counter() - t0
    return legs


def distributed_leg_guarded(a, plain_ms):
    t0 = time.perf_counter()
    try:
        leg = distributed_path_leg(a, plain_ms)
    except BaseException as exc:  # noqa: BLE001
        leg = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
    leg["leg_wall_s"] = time.perf_counter() - t0
    return leg


def issue_bound(kernel_name, mean_us):
    """HBM is demonstrably not what bounds the headline launch (measured traffic is ~10x below the algorithmic bytes: the
    trajectory stays in LDS), VALU issue is the nearer ceiling: instructions per launch (rocprofv3 --pmc SQ_INSTS_VALU, a pass
    of its own; newest profiles/r*_pmc_valu.json holding this kernel) / 1024 SIMDs x the measured issue interval of a SIMD.
    ONE constant, measured (tests/micro/issue_rate.hip, output committed as profiles/r04_issue_rate.log; independent FMAs at
    2.4 GHz): a SIMD retires one wavefront-instruction per 3.0 cycles with 4 wavefronts resident, per 3.6 cycles with 2, per
    5.9 cycles with 1 (9.8 when each depends on the last).  `frac` uses the full-SIMD figure (3.0: the kernel's ceiling);
    `frac_at_residency` the figure at the kernel's own two wavefronts per SIMD (3.6)."""
    import glob

    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_valu.json")), reverse=True):
        ks, fresh = load_pmc(f)
        if kernel_name in ks and not fresh:
            return None  # (an instruction count of other kernel code)
        if kernel_name in ks:
            insts = ks[kernel_name]["SQ_INSTS_VALU"]
            cyc, cyc2, clk, simds = ISSUE_CYCLES_FULL_SIMD, ISSUE_CYCLES_TWO_WAVES, 2.4e9, 1024
            t_us = insts / simds * cyc / clk * 1e6
            return {"valu_insts_per_launch": insts, "simds": simds, "cycles_per_inst": cyc, "clock_hz": clk,
                    "issue_time_us": t_us, "frac": t_us / mean_us, "cycles_per_inst_at_two_waves_per_simd": cyc2,
                    "frac_at_residency": insts / simds * cyc2 / clk * 1e6 / mean_us,
                    "constants_source": "profiles/r04_issue_rate.log (tests/micro/issue_rate.hip)",
                    "source": "profiles/" + os.path.basename(f),
                    "note": "fraction of the launch that pure VALU issue on all 1024 SIMDs would take: the kernel's distance "
                            "from its own (instruction-count) ceiling; the rest is serial phases and idle SIMDs"}
    return None


def headline_roofline(a, model, settings, batch, training, n_iwae_model):
    """`--full`: the decoder launch and the ODE kernels of the headline step, re-issued back to back between HIP events,
    against SURVEY 8d's fixed byte numerator (`roofline` in the line)."""
    from vihds import ops

    # (training.step needs a live autograd graph; the direct launches below reuse the resident batch and the model)
    kt = ode_kernel_times(model, settings, batch, n_iwae_model, a.roofline_steps)
    # the step's own decoder launch (sampling + conditioning + sweeps), re-issued back to back with its own arguments
    rec = ops.LaunchRecorder()
    ops.TIMER = rec
    training.step(batch)
    ops.TIMER = None
    step_launch = rec.calls.get("decoder_step")
    if step_launch is not None:
        st = torch.cuda.current_stream()
        for _ in range(3):
            step_launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.roofline_steps):
            step_launch()
        e1.record(st)
        torch.cuda.synchronize()
        kt["ode_step"] = {"mean_us": e0.elapsed_time(e1) * 1e3 / a.roofline_steps, "launches": a.roofline_steps}
    fwd_b, bwd_b = algorithmic_bytes(B_ROWS, N_IWAE)
    solver_id = {"modeuler": 0, "modeulerwhile": 1, "euler": 2, "midpoint": 3, "rk4": 4}[a.solver]
    lanes = B_ROWS * N_IWAE <= 16384  # the library's automatic choice (vihds_dr_lanes.hpp)
    kname = {k: ("void vihds::dr_lane_%s_kernel<1, %d, true>(vihds::OdeArgs)" % (k[4:], solver_id)) if lanes else
                ("void vihds::%s_kernel<vihds::DrConstant<1>, %d>(vihds::OdeArgs)" % (k, solver_id))
             for k in ("ode_fwd", "ode_bwd")}
    # the decoder launch: the time-parallel kernel (csrc/vihds_dr_scan.hpp), ITEMS = steps per lane
    scan_items = (N_TIMES - 1 + 31) // 32
    kname["ode_fused"] = "void vihds::dr_scan_train_kernel<1, %d, %d>(vihds::OdeArgs)" % (solver_id, scan_items)
    kname["ode_step"] = ("void vihds::dr_scan_train_theta_kernel<1, %d, %d>(vihds::OdeArgs, int, "
                         "vihds::ThetaStageArgs)" % (solver_id, scan_items))
    theta_b = 4 * (2 * N_PARAMS * B_ROWS * N_IWAE + 2 * B_ROWS * N_IWAE)  # the sampling stage's u, theta, log q, log p
    # SURVEY 8d's fixed numerator for every form of the decoder launch: 30 729 600 + 20 822 400 = 51 552 000 B; the
    # sampling stage's bytes (theta_b) are reported next to it, never added to it
    nbytes = {"ode_fwd": fwd_b, "ode_bwd": bwd_b, "ode_fused": fwd_b + bwd_b, "ode_step": fwd_b + bwd_b}

    def gbs(nb, us):
        return nb / (us * 1e-6) / 1e9

    # HBM traffic per launch from the PMC passes committed under profiles/ (newest set that has this kernel)
    import glob
    pmc_kernels, pmc_name, pmc_stale = {}, None, None
    for pmc_file in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")), reverse=True):
        ks, fresh = load_pmc(pmc_file)
        if kname["ode_step" if "ode_step" in kt else "ode_fused"] in ks:
            if fresh:
                pmc_kernels, pmc_name = ks, os.path.basename(pmc_file)
            else:  # counters of other kernel code are not this kernel's traffic
                pmc_stale = os.path.basename(pmc_file)
            break

    def entry(k):
        pmc = pmc_kernels.get(kname[k])
        return {"kernel": kname[k], "mean_us": kt[k]["mean_us"], "achieved": gbs(nbytes[k], kt[k]["mean_us"]),
                "algorithmic_bytes_per_launch": nbytes[k], "traffic": pmc["hbm_bytes_corrected"] if pmc else None}

    fused_step = not a.two_kernel_ode and lanes
    if fused_step and "ode_step" in kt:
        dom, others = "ode_step", ["ode_fused", "ode_fwd", "ode_bwd"]
    elif fused_step:
        dom, others = "ode_fused", ["ode_fwd", "ode_bwd"]
    else:
        dom = "ode_bwd" if kt["ode_bwd"]["mean_us"] >= kt["ode_fwd"]["mean_us"] else "ode_fwd"
        others = ["ode_fwd" if dom == "ode_bwd" else "ode_bwd", "ode_fused"]
    others = [k for k in others if k in kt]
    d = entry(dom)
    roofline = {
        "bound": "hbm", "kernel": d["kernel"], "achieved": d["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": d["achieved"] / HBM_PEAK_GBS, "traffic": d["traffic"],
        "traffic_source": ("profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same workload, same "
                           "kernel sources: csrc_sha16 checked)" % pmc_name) if d["traffic"] is not None else
                          ("none: newest profiles/%s was measured on other kernel sources (csrc_sha16 differs); re-run "
                           "tests/probe/profile_set.sh" % pmc_stale) if pmc_stale else None,
        "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"], "mean_us": d["mean_us"],
        "launches_timed": kt[dom]["launches"],
        "timing": "back-to-back launches of the kernel between one HIP event pair on the launch stream",
        "numerator_note": ("fixed SURVEY 8d numerator: the bytes the forward + adjoint pair moves when the trajectory "
                           "goes through HBM (30 729 600 + 20 822 400 B).  The fused kernel keeps the trajectory in LDS and "
                           "itself moves only the draws, theta, the log-probabilities and d theta (see traffic); the "
                           "sampling stage that runs in the same launch is NOT in the numerator (theta_stage_bytes)")
        if fused_step else None,
        "theta_stage_bytes": theta_b if (fused_step and "ode_step" in kt) else None,
        "issue_bound": issue_bound(d["kernel"], d["mean_us"]),
        "other_kernels": [entry(k) for k in others],
        "step_algorithmic_bytes": fwd_b + bwd_b,
    }
    return roofline


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (defaults: a timed window of ~0.35 s at the headline -- a 200-step window is 17 ms, in which one 4 ms hiccup of the
    # host or the clocks is a 20 % error: measured, profiles/r03_h_bench.json's first version)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--solver", default=None)
    ap.add_argument("--workload", choices=sorted(WORKLOAD_TABLE) + ["run_loop"], default="config2",
                    help="which BASELINE.json configuration: config2 (headline, default), config3_train / config3_eval "
                         "(n_iwae=1000), config4 (dr_blackbox, MFMA roofline), config5 (relay)")
    ap.add_argument("--eager", action="store_true", help="launch every kernel from python instead of replaying a hipGraph")
    ap.add_argument("--host-rng", action="store_true", help="draw u with host numpy as the reference does (vae.py:22-24)")
    ap.add_argument("--device-rng", choices=["kernel", "device"], default="kernel",
                    help="kernel: u and the conditioner weights are drawn inside the HIP kernels (counter-based "
                         "Philox); device: torch.randn on the GPU")
    ap.add_argument("--shard", choices=["rows", "samples"], default="rows",
                    help="N > 1: 'rows' = data parallel, every GPU its own 36 rows x 200 samples, gradients averaged with "
                         "one all-reduce per step; 'samples' = the same 36 rows on every GPU, the IWAE-sample axis split "
                         "(200 per GPU), row statistics all-gathered + one gradient all-reduce")
    ap.add_argument("--two-kernel-ode", action="store_true",
                    help="integrate and differentiate with vihds_ode_fwd + vihds_ode_bwd (trajectory through HBM) "
                         "instead of the fused vihds_ode_logp_grad")
    ap.add_argument("--stored-trajectory-eval", action="store_true",
                    help="evaluation pass: write the trajectory (644 MB at config 3's evaluation shape) and stream it back "
                         "through vihds_iw_summaries_states instead of the second forward launch that adds the summaries up "
                         "on the way (params.online_summaries: false)")
    ap.add_argument("--no-fused-iwae", action="store_true",
                    help="keep the IWAE loss as its own launch instead of forming it inside the theta-adjoint launch")
    ap.add_argument("--no-step-tail", action="store_true",
                    help="keep IWAE loss + theta adjoint, the encoder adjoint (two launches) and Adam as the five launches of "
                         "round 2 instead of vihds_step_tail's two")
    ap.add_argument("--steps-per-graph", type=int, default=32,
                    help="consecutive training steps captured into one hipGraph (single process, resident batch); 1 = one "
                         "graph launch per step as in round 2")
    ap.add_argument("--no-strong-leg", dest="strong_leg", action="store_false",
                    help="N > 1 with --full: skip the extra strong-scaling measurement (config 3's one batch, n_iwae=1000, "
                         "sample-sharded) that is otherwise added to the line as `strong_scaling_config3`")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--all-legs", action="store_true",
                    help="N = 1: after the headline, also time the other single-GPU BASELINE configurations (config3_train, "
                         "config3_eval, config4, config5), the unchanged-spec path, Training.run() end to end and the per-rank "
                         "shard shapes.  They go to bench_extra.json, never into the line (the driver's line stays < 6 KB)")
    ap.add_argument("--no-other-configs", dest="other_configs", action="store_false",
                    help="--all-legs: skip the legs of the other single-GPU BASELINE configurations and the unchanged-spec path")
    ap.add_argument("--leg-seconds", type=float, default=0.6, help="timed window of each `other_configs` leg")
    ap.add_argument("--roofline-steps", type=int, default=100,
                    help="launches of each ODE kernel timed for the roofline object (0: skip)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.001,
                    help="Adam learning rate.  The reference spec's 0.01 makes the objective run away on the synthetic "
                         "plate within a few hundred steps on some seeds (q collapses onto a clipped sample: -ELBO "
                         "-> -1e20 / nan, DESIGN.md section 2, profiles/LOG.md); the arithmetic per step does not depend on it.  On the "
                         "real plate data 0.01 trains for 3 000 steps without incident (tests/probe/real_data_long_run.py)")
    ap.add_argument("--no-loop-legs", dest="loop_legs", action="store_false",
                    help="--all-legs: skip the `run_loop` / `real_plate` legs (Training.run() end to end)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline legs, the CPU baseline, the long window behind a "
                         "short one and (N > 1) the strong-scaling legs, and write bench_extra.json.  Without it a run sets up, "
                         "warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="headline workload: after the timed steps write the last step's loss and the trained parameters as "
                         "DIR/<name>.npy (float32)")
    a = ap.parse_args()
    a.full = a.full or a.all_legs
    if a.dump_outputs and a.workload != "config2":
        ap.error("--dump-outputs writes the headline workload's outputs (--workload config2)")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as typed: start the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1) and
        # hand the same arguments on; rank 0 of that job prints the line
        import socket
        import subprocess

        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env, stdout=_OUT))  # (the ranks inherit the REAL stdout for their one line)
    a.solver_given = a.solver is not None
    if a.workload != "config2":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
        if a.workload == "run_loop":
            return run_loop_workload(a)
        out = run_workload(a, a.workload)
        if out is not None:
            emit(out)
        return
    a.solver = a.solver or "rk4"

    from vihds import parallel, synthetic

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run --nproc-per-node N)"
                         % (a.gpus, world))
    shard = parallel.init_from_env()
    rank = shard.rank if shard is not None else 0
    replica = None
    if shard is not None and a.shard == "rows":  # data parallel over rows: replicas + one gradient all-reduce
        replica, shard = parallel.RowReplica(shard.rank, shard.world, shard.group), None
    multi = shard is not None or replica is not None
    if multi:
        # (backstop behind the watchdog below: a multi-rank run that stops making progress says where it stands and ends)
        import faulthandler

        faulthandler.dump_traceback_later(MULTI_RANK_WATCHDOG_S + 60, exit=True)
    local_rank = int(os.environ.get("VIHDS_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local_rank)
    dev = "cuda:%d" % local_rank
    use_graph = not a.eager and not a.host_rng
    if multi and os.environ.get("VIHDS_BENCH_MULTI_EAGER"):
        use_graph = False  # (multi-rank steps are captured as hipGraph segments with eager collectives in between)
    # every rank: same seed => same encoder init; --shard samples: same draws too (each rank takes its slice);
    # --shard rows: own plate rows and own draws per rank
    n_iwae_model = N_IWAE * world if shard is not None else N_IWAE
    args, settings, data, parameters, model, training = synthetic.build(
        "dr_constant_icml", B_ROWS, n_iwae_model, solver=a.solver, device=dev, seed=a.seed, shard=shard, replica=replica,
        u_rng="numpy" if a.host_rng else a.device_rng, conditioner_rng="cpu" if a.host_rng else a.device_rng,
        hip_graph=use_graph, nan_check_every=0, learning_rate=a.lr, fused_ode_training=not a.two_kernel_ode,
        fused_iwae_backward=not a.no_fused_iwae, fused_step_tail=not a.no_step_tail)
    model.train()
    batch = training.train_data
    step = training.graph_step if use_graph else training.step
    launch_mode = "hipGraph replay" if use_graph else "eager"
    def barrier():
        torch.cuda.synchronize()
        if multi:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    # Several ranks: the SAFE measurement first -- eager launches, eager collectives, nothing captured -- so that a valid line
    # exists before anything that has never run on more than one GPU is tried (the captured step with RCCL's kernels inside
    # the hipGraph, the capture probe's child processes).  A watchdog then guards the graph path: if it has not finished within
    # MULTI_RANK_WATCHDOG_S seconds, rank 0 prints the eager line (marked as such) and every rank leaves with exit code 0 -- the
    # scaling record is never lost to a hang (VERDICT r04 #2d: the old behaviour was a traceback after twenty minutes).
    watchdog = None
    if multi:
        import threading

        for _ in range(10):
            training.step(batch)
        barrier()
        t0 = time.perf_counter()
        n_eager = max(20, min(a.steps, 200))
        for _ in range(n_eager):
            loss_e = training.step(batch)
        barrier()
        te = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
        el_e = float(te)
        fallback = {
            "metric": "ELBO training steps/sec (dr_constant_icml, n_iwae=200)", "value": world * n_eager / el_e, "unit": "steps/s",
            "n_gpus": world, "steps": n_eager, "warmup": 10, "ms_per_step": 1e3 * el_e / n_eager, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "dr_constant_icml: B=36 rows x n_iwae=200 per GPU, N=8 species, T=86, P=35, %s, full training "
                                   "step (encoder+theta+ODE+IWAE fwd/bwd+Adam)" % a.solver, "launch": "eager (fallback line)",
                       "world_size": world, "parallelism": "data parallel over rows" if replica is not None else "iwae-sample shard"},
            "final_loss": float(loss_e), "roofline": None, "cpu_baseline": None,
            "note": "FALLBACK: the hipGraph-replayed multi-rank measurement did not finish within %d s; this is the eager "
                    "measurement taken before it" % MULTI_RANK_WATCHDOG_S}

        def fire():
            if rank == 0:
                emit_line(fallback)
            os._exit(0)

        watchdog = threading.Timer(MULTI_RANK_WATCHDOG_S, fire)
        watchdog.daemon = True
        watchdog.start()

    # steps per graph launch: between two graph launches the GPU idles 6-8 us (measured: rocprofv3 kernel trace), so the
    # resident-batch replay captures G consecutive steps per graph; K timed steps = K // G launches of that graph plus
    # one launch of a graph holding the K % G remaining steps -- exactly K optimizer steps either way
    # (several ranks: only data-parallel replicas, and only when the communicator records into the capture -- the gradient
    # all-reduce then sits inside the graph between the step's kernels; the sample-sharded step keeps one step per graph)
    G = 1
    if use_graph and (not multi or (replica is not None and parallel.collectives_capturable(replica.group))):
        G = max(1, a.steps_per_graph)

    def run_steps(k):
        out = None
        for _ in range(k // G):
            out = training.graph_step(batch, repeat=G) if G > 1 else step(batch)
        rest = k % G if G > 1 else 0
        if rest > 1:
            out = training.graph_step(batch, repeat=rest)  # (the remainder as ONE graph of its own, captured during setup)
        elif rest == 1:
            out = step(batch)
        return out

    setup_seconds = 0.0
    if use_graph:
        capture_error = None
        try:
            step(batch)  # setup, not a measured or warm-up step: allocator warm-up + hipGraph capture happen on first use
            if G > 1:
                training.graph_step(batch, repeat=G)  # (same for the G-step graph: G untimed steps)
                for k in sorted({a.warmup % G, a.steps % G}):  # (and for the graphs that hold the remainders)
                    if k > 1:
                        # (setup, like the capture itself -- not among the W warm-up or the K timed steps: the graph that holds the
                        # remainder is launched for SETUP_STEPS steps, ~0.3 s of device time.  A launch after an idle stretch
                        # runs below the steady rate: the driver's 20-step window measured 13.5-14.1k steps/s behind two such
                        # launches, 14.4-14.6k behind 32 (profiles/r06_setup_launches.log), 14.9k in a long run.  Reported as
                        # config.setup_seconds)
                        # (a FIXED number of launches, never a time: the timed steps then start from the same model state on every
                        # run, which --dump-outputs relies on; several ranks: 32 launches -- every launch holds collectives)
                        t_setup = time.perf_counter()
                        for _round in range(4 if multi else -(-SETUP_STEPS // (8 * k))):
                            for _ in range(8):
                                training.graph_step(batch, repeat=k)
                            torch.cuda.synchronize()
                        setup_seconds += time.perf_counter() - t_setup
        except Exception as exc:  # noqa: BLE001 -- (reported in the line; the run goes on with eager launches)
            if not multi:
                raise
            capture_error = repr(exc)[:300]
        if multi:
            # a multi-rank step is captured as hipGraph segments around its collectives; should that fail on ANY rank (it
            # has only ever run over gloo and over RCCL with one rank: no multi-GPU node was available), every rank
            # falls back to eager launches rather than losing the scaling line
            flag = torch.tensor([0.0 if capture_error is None else 1.0], device=dev)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
            if float(flag) > 0:
                torch.cuda.synchronize()
                training.use_graph = False
                use_graph, G = False, 1
                step = training.step
                launch_mode = "eager (hipGraph capture of the multi-rank step failed on a rank: %s)" % (capture_error or "another rank")
                step(batch)
    loss = run_steps(a.warmup)
    barrier()
    t0 = time.perf_counter()
    loss = run_steps(a.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if multi:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, loss, model)
    # --full: a short timed window (the driver's --steps 20 is ~2 ms) is also reported over >= 0.5 s of the same replay
    long_run = None
    if a.full and use_graph and elapsed < 0.25:
        n_long = int(math.ceil(0.5 / max(elapsed / a.steps, 1e-6) / G)) * G
        barrier()
        t1 = time.perf_counter()
        loss = run_steps(n_long)
        barrier()
        el = time.perf_counter() - t1
        if multi:
            tl = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(tl, op=torch.distributed.ReduceOp.MAX)
            el = float(tl)
        long_run = {"steps": n_long, "value": world * n_long / el, "ms_per_step": 1e3 * el / n_long}
    final_loss = float(loss)
    if not np.isfinite(final_loss) or final_loss < -1e6:
        raise SystemExit("degenerate loss %r after the timed steps (training ran away): not a valid bench run"
                         % final_loss)

    rank_devices = ["rank 0: %s (%s)" % (dev, torch.cuda.get_device_name(local_rank))]
    strong = strong5 = None
    if multi:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, "rank %d: %s (%s)" % (rank, dev, torch.cuda.get_device_name(local_rank)))
        rank_devices = gathered
        if a.full and a.strong_leg:
            strong = strong_scaling_leg(a, dev, world, rank)
            strong5 = strong_scaling_leg(a, dev, world, rank, "relay_constant_precisions", 200, "midpoint", "config5")
    eager_ms = None
    if watchdog is not None:
        watchdog.cancel()
        eager_ms = fallback["ms_per_step"]
    # ---- roofline leg (--full): the same step, eager, with HIP events around every ODE kernel launch -----------
    if a.full and a.roofline_steps <= 0:
        if rank == 0:
            short = {"metric": "ELBO training steps/sec (dr_constant_icml, n_iwae=200)",
                              "value": world * a.steps / elapsed, "unit": "steps/s", "n_gpus": world, "steps": a.steps,
                              "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps, "launch": launch_mode,
                              "final_loss": final_loss, "world_size": world, "rank_devices": rank_devices,
                              "value_long": long_run["value"] if long_run else None,
                              "strong_scaling_config3": strong, "strong_scaling_config5": strong5, "scaling": "weak",
                              "steps_per_graph_launch": G,
                              "dist_backend": torch.distributed.get_backend() if multi else None,
                              "collectives_in_graph": bool(getattr(training, "collectives_captured", False)) if multi else None,
                              "eager_ms_per_step": eager_ms,
                              "note": "roofline leg skipped (--roofline-steps 0)"}
            if multi and eager_ms is not None and fallback["steps"] == a.steps and eager_ms < short["ms_per_step"]:
                # (as in the full line below: both are exactly K steps; the faster measurement is the line's)
                short["graph_replay"] = {"value": short["value"], "ms_per_step": short["ms_per_step"], "launch": launch_mode}
                short["value"], short["ms_per_step"] = fallback["value"], eager_ms
                short["launch"] = "eager (faster than the hipGraph replay on this run: see graph_replay)"
            short["config"] = {"workload": "dr_constant_icml: B=36 rows x n_iwae=200 per GPU, T=86, %s" % a.solver,
                               "solver": a.solver, "launch": short.pop("launch"), "world_size": world}
            emit_line(short)
        return
    roofline = headline_roofline(a, model, settings, batch, training, n_iwae_model) if a.full else None
    if rank != 0:
        return
    out = {
        "metric": "ELBO training steps/sec (dr_constant_icml, n_iwae=200)",
        "value": world * a.steps / elapsed, "unit": "steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        # what ONE counted step is at N > 1: row replicas (--shard rows) put 36 rows per rank through one Adam step on the
        # averaged gradient -- `value` counts that as N steps of the named 36-row configuration (weak scaling), and says so here
        "rows_per_step": B_ROWS * (world if replica is not None else 1),
        "n_ranks_seen": torch.distributed.get_world_size() if multi else 1,
        "value_long": long_run["value"] if long_run else None,
        "ms_per_step_long": long_run["ms_per_step"] if long_run else None,
        "steps_long": long_run["steps"] if long_run else None,
        "config": {"workload": "dr_constant_icml: B=36 rows x n_iwae=200 per GPU, N=8 species, T=86, P=35, %s, "
                               "full training step (encoder+theta+ODE+IWAE fwd/bwd+Adam)" % a.solver,
                   "solver": a.solver, "n_iwae_per_gpu": N_IWAE, "n_iwae_global": n_iwae_model,
                   "rows_global": B_ROWS * (world if replica is not None else 1),
                   "launch": launch_mode, "steps_per_graph_launch": G, "learning_rate": a.lr,
                   "setup_seconds": (setup_seconds if not multi else "32 launches per remainder graph") if use_graph else 0.0,
                   "world_size": torch.distributed.get_world_size() if multi else 1, "rank_devices": rank_devices,
                   "dist_backend": torch.distributed.get_backend() if multi else None,
                   "collectives_in_graph": bool(getattr(training, "collectives_captured", False)) if multi else None,
                   "batch_staging": "the batch is resident in HBM; its staging copies and delta_obs (reference "
                                    "encoders.py:385) are outside the replayed step",
                   "ode": "vihds_ode_fwd + vihds_ode_bwd" if a.two_kernel_ode else "vihds_theta_ode_logp_grad (sampling + conditioning + ODE + adjoint in one launch)", "tail": "loss + backward + Adam: five launches" if (a.no_step_tail or multi) else "vihds_step_tail (IWAE loss + theta adjoint + encoder adjoint + Adam in two launches)", "u_rng": "host numpy" if a.host_rng else ("in-kernel philox" if a.device_rng == "kernel" else "torch device philox"),
                   "parallelism": ("single GPU" if world == 1 else
                                   "data parallel over rows x%d (36 rows per GPU, one gradient all-reduce per step)" % world
                                   if replica is not None else "iwae-sample shard x%d (all-gather of row statistics + "
                                   "one gradient all-reduce per step)" % world)},
        "final_loss": final_loss, "roofline": roofline, "strong_scaling_config3": strong,
        "strong_scaling_config5": strong5, "eager_ms_per_step": eager_ms,
    }
    if not a.full:
        out["note"] = "roofline, cpu_baseline and the other legs: --full"
    if multi and eager_ms is not None and fallback["steps"] == a.steps and eager_ms < out["ms_per_step"]:
        # Several ranks: BOTH measurements are exactly K steps of the same workload between the same barriers -- the eager one
        # taken first, the hipGraph replay after it.  The captured multi-rank step has never run on more than one GPU; should
        # it turn out the slower of the two there (over gloo, with its collectives outside the graph segments, it is), the
        # line carries the faster measurement and says so.
        out["graph_replay"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "launch": launch_mode,
                               "steps_per_graph_launch": G}
        out["value"], out["ms_per_step"] = fallback["value"], eager_ms
        out["config"]["launch"] = "eager (faster than the hipGraph replay on this run: see graph_replay)"
    if a.full and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.solver, batch.observations.detach().cpu())
        out["speedup_vs_cpu_restatement"] = out["value"] / out["cpu_baseline"]["value"]
    if world == 1 and a.all_legs and a.other_configs and not (a.eager or a.host_rng or a.two_kernel_ode):
        del model, training, step
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        out["other_configs"] = other_config_legs(a, dev)
        out["other_configs"]["distributed_path_world1"] = distributed_leg_guarded(a, out["ms_per_step"])
        if a.loop_legs:
            loops = loop_legs_for_default_line(a)
            out["run_loop"], out["real_plate"] = loops["run_loop"], loops["real_plate"]
            out["newton_iters"] = {k: (loops[k] or {}).get("newton_iters") for k in ("run_loop", "real_plate")}
    if a.full:
        emit_line(out)
    else:  # (a plain run writes no side file: the line is all it measured)
        emit(compact_line(out))
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() == 1:
        try:  # (the one-rank legs: a group left alive aborted in RCCL's teardown now and then, behind the line)
            torch.cuda.synchronize()
            torch.distributed.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass



if __name__ == "__main__":
    # The contract is ONE line on stdout.  The package mirrors the reference's console messages ("Initialising encoder" ...) and
    # libraries print what they like: everything but the line goes to stderr, from python and from native code alike.
    _OUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    sys.stdout = sys.stderr
    main()
