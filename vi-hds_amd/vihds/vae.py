"""BaseVAE glue (counterpart of the reference's vihds/vae.py): sample u -> encoder -> q.sample -> p.clip ->
decoder.  The sample/clip/log-prob chain is one kernel; the decoder is one kernel."""
import numpy as np
import torch
import torch.nn as nn

from vihds import ode as O
from vihds import ops
from vihds.decoders import Decoder, on_demand_result
from vihds.encoders import Encoder
from vihds.utils import default_get_value


class BaseVAE(nn.Module):
    def __init__(self, encoder, decoder, device, u_rng="numpy", shard=None):
        super(BaseVAE, self).__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.device = device
        self.n_theta = None
        self.u_rng = u_rng
        self.shard = shard  # vihds.parallel.SampleShard or None
        self._rng_state = None
        self._u_staging = {}

    def sample_u(self, n_batch, n_samples, device=None):
        """Standard-normal draws u [B,S,P].  "numpy" = the reference's host RNG stream (vae.py:22-24);
        "device" = torch's Philox generator on the GPU (graph-capturable, no host->device copy);
        "kernel" = drawn inside the theta kernel (counter-based Philox, vihds_theta_opts.rng): no launch of its own,
        and under S-sharding each rank draws only its slice of the same global stream."""
        if self.u_rng == "device":
            return torch.randn((n_batch, n_samples, self.n_theta), device=self.device)
        if self.u_rng == "kernel":
            if self._rng_state is None:  # seeded once from torch's generator so torch.manual_seed controls it
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                self._rng_state = ops.KernelNormal.new_state(seed, self.device)
            return ops.KernelNormal((n_batch, n_samples, self.n_theta), self._rng_state)
        # The reference's stream (np.random.randn of the global RandomState), bit for bit, from native code (vihds/nprand.py:
        # 2.3 ms of numpy per draw at B=36, S=200 otherwise), straight into one of a few pinned staging buffers -- used in
        # turn, each reused only after the copy that read it has run -- and on to the device without waiting.
        from vihds import hostdraws, nprand

        shape = (int(n_batch), int(n_samples), int(self.n_theta))
        if hostdraws.capturing():  # a captured step: the draw happens before every replay (vihds/hostdraws.py)
            return hostdraws.ACTIVE.add(shape, self.device, nprand.Draw(shape), prefetchable=True)
        hostdraws.note(shape)
        if not (torch.cuda.is_available() and torch.device(self.device).type == "cuda"):
            return torch.from_numpy(nprand.randn_f32(shape)).to(self.device)
        n = shape[0] * shape[1] * shape[2]
        ring = self._u_staging.get(n)
        if ring is None:
            ring = self._u_staging[n] = {"bufs": [torch.empty(n, dtype=torch.float32).pin_memory() for _ in range(4)],
                                         "events": [None] * 4, "pos": 0}
        k = ring["pos"]
        ring["pos"] = (k + 1) % 4
        if ring["events"][k] is not None:
            ring["events"][k].synchronize()
        host = ring["bufs"][k]
        nprand.randn_f32(shape, out=host.numpy())
        u = host.view(shape).to(self.device, non_blocking=True)
        if ring["events"][k] is None:
            ring["events"][k] = torch.cuda.Event()
        ring["events"][k].record()
        return u

    def forward(self, data, samples, writer=None, epoch=None, request=None):
        """reference vae.py:26-37.  `request` (ode.ForwardRequest): what the caller will do with the forward; None asks for
        nothing.  Which launches run is ode.sampling_route's answer; a route that declines is remembered and the next one
        tried."""
        request = request or O.PLAIN_FORWARD
        u = self.sample_u(len(data.inputs), samples)
        if self.shard is not None:
            u = self.shard.take(u)  # every rank drew the same full u; keep this rank's slice of S
        q = self.encoder(data)
        p = self.encoder.p
        ode_model = self.decoder.ode_model
        n_extra = len(ode_model.extra_theta_names) if self.decoder.condition_on_device else 0
        attempts = ((O.DECODER_STEP_FUSED, self._decoder_step_fused), (O.THETA_ODE_FUSED, self._theta_ode_fused))
        for route, attempt in attempts:
            if O.sampling_route(request, self, q, data, samples) != route:
                continue
            try:
                fused = attempt(data, samples, u, q, p, n_extra)
            except ops.FusedTrainingUnsupported:  # (remembered: this shape does not ask for the route again)
                shape = (tuple(data.observations.shape), samples, self.decoder.config.params.solver)
                ode_model._fused_declined[(route,) + shape] = True
                continue
            if fused is not None:
                return fused + (q, p)
        clipped_theta = q.sample_clip_log_prob(u, p, stddevs=4, n_extra_rows=n_extra)
        if self.shard is not None:
            lo, _ = self.shard.bounds(samples)
            object.__setattr__(clipped_theta, "_sample_window", (samples, lo))
        result, conditioned_theta = self.decoder(clipped_theta, data, writer, epoch, request=request)
        return result, conditioned_theta, q, p

    def _decoder_step_fused(self, data, samples, u, q, p, n_extra):
        """Training fast path (params.fused_ode_training): sampling, device conditioning, log-likelihood and the
        unit-weight adjoint in ONE launch (ops.DecoderStepFused).  None when it turns out not to apply after all."""
        dec = self.decoder
        ode, cfg, obs = dec.ode_model, dec.config, data.observations
        extra = list(ode.extra_theta_names) if n_extra else []
        window = None
        if self.shard is not None:
            lo, _ = self.shard.bounds(samples)
            window = (samples, lo)

        def spec_of(names):
            row_of = {n: k for k, n in enumerate(list(names) + extra)}
            return ode._spec(cfg, row_of, len(names) + len(extra), len(data.times))

        n_q = len(q.names())
        cond_job = None
        if extra:
            rel, dflt, z, mean, std, rng_state = ode.conditioner_job(extra, data.dev_1hot)
            cond_job = (len(extra), n_q, mean, std, z, rng_state, rel, dflt)
        if window is not None and not isinstance(u, ops.KernelNormal):
            return None  # (the conditioner tiling needs the window; only the in-kernel draw carries it)
        theta, logp = q.decoder_step_fused(u, p, 4, n_extra, spec_of, ode.row_inputs(data), data.times.to(obs.device), obs,
                                           data.dev_1hot, cond_job)
        for k, n in enumerate(extra):
            theta.bind_reserved_row(n, n_q + k)
        if window is not None:
            object.__setattr__(theta, "_sample_window", window)
        if hasattr(ode, "aR") and extra:
            ode.aR, ode.aS = getattr(theta, "aR", None), getattr(theta, "aS", None)
        # params.fused_iwae_backward: Training.cost may leave the IWAE loss to this step's theta-adjoint launch
        defer = bool(default_get_value(cfg.params, "fused_iwae_backward", True)) and self.shard is None
        sol = O.LazySolution(logp, O.ForwardRecord(O.DECODER_STEP_FUSED, logp.grad_fn, defer_iwae=defer),
                             lambda: ode.solve(cfg, data.times, theta, ode.row_inputs(data), data.dev_1hot, obs))
        ode._last = sol
        return on_demand_result(ode, theta, data.times, sol), theta

    def _theta_ode_fused(self, data, samples, u, q, p, n_extra):
        """Training steps whose backward is ops.GeneralTail and whose request allows it (fuse_sampling): the sampling stage,
        for dr_blackbox also condition_theta, runs inside the ODE forward launch (ops.ThetaOdeFused, vihds_theta_ode_fwd).
        ode.sampling_route says for which models."""
        dec = self.decoder
        ode, cfg, obs = dec.ode_model, dec.config, data.observations
        blackbox = ode.model_key == "dr_blackbox"
        extra = list(ode.extra_theta_names) if (blackbox and n_extra) else []
        n_q = len(q.names())
        offset = None
        if blackbox and ode.n_y > 0:
            offset = (ode.offset_layer.weight, ode.offset_layer.bias, (ode.offset_source_row(q.names()), n_q, ode.n_y))

        def spec_of(names):
            row_of = {n: k for k, n in enumerate(list(names) + extra)}
            if blackbox:  # the integrator reads the device-conditioned rows (condition_theta re-binds y1.. to them)
                for i in range(ode.n_y):
                    row_of["y%d" % (i + 1)] = n_q + i
            return ode._spec(cfg, row_of, len(names) + len(extra), len(data.times))

        theta, traj, logp = q.theta_ode_fused(u, p, 4, len(extra), spec_of, ode.row_inputs(data), data.times.to(obs.device), obs,
                                              data.dev_1hot, ode.neural_weights(), offset)
        if blackbox:
            for i in range(ode.n_y):  # (what condition_theta does: the attribute now names the conditioned row)
                theta.bind_reserved_row("y%d" % (i + 1), n_q + i)
        node = logp.grad_fn
        sol = O.DecodedSolution(traj, None, logp, O.ForwardRecord(O.THETA_ODE_FUSED, node, node, node.rng_state),
                                observe=lambda s_: ode._observe_map(s_))
        ode._last = sol
        return on_demand_result(ode, theta, data.times, sol), theta


def build_model(args, settings, dataset, parameters, shard=None):
    """reference vae.py:39-51.  Construction order (encoder, then decoder) matches the reference so that the
    same torch seed gives the same initial weights."""
    encoder = Encoder(parameters, dataset, getattr(args, "verbose", False), device=settings.device)
    if settings.data.device_depth > 1:
        decoder_condition_on_device = True
    else:
        print("- Only a single device being considered, so disabling device-conditioning in the decoder")
        decoder_condition_on_device = False
    decoder = Decoder(settings, decoder_condition_on_device).to(settings.device)
    return BaseVAE(encoder, decoder, settings.device, u_rng=default_get_value(settings.params, "u_rng", "numpy"),
                   shard=shard)
