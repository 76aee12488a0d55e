"""OdeModel: the plugin base class of models.LOOKUP (counterpart of the reference's vihds/ode.py).

`simulate` keeps the reference signature and return value ([B,S,N,T], a strided view) but runs the whole time
loop -- and, fused in the same kernel, observe + the Gaussian log-likelihood -- as ONE HIP kernel
(vihds_ode_fwd) with a hand-written discrete adjoint (vihds_ode_bwd).  There is no torchdiffeq and no CPU path.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from vihds import ops
from vihds.utils import default_get_value


PLAIN, TRAIN, EVALUATE = "plain", "train", "evaluate"

# What the caller will do with a forward, passed down as `request=` (None: PLAIN_FORWARD, a call that asks for nothing):
# purpose; general_tail: the step's backward is ops.GeneralTail, so nobody reads x_predict; fuse_sampling: the sampling
# stage may run inside the forward launch; online_summaries: the summaries-on-the-way evaluation form is allowed
ForwardRequest = namedtuple("ForwardRequest", "purpose general_tail fuse_sampling online_summaries",
                            defaults=(PLAIN, False, False, False))
PLAIN_FORWARD = ForwardRequest()

# the routes that produce a log-likelihood, named by the ops entry that launches them
DECODER_STEP_FUSED, THETA_ODE_FUSED, ODE_SOLVE_OBSERVE, ODE_LOGLIK_FUSED, ODE_LOGP_ONLY, ADAPTIVE_HOST, ADAPTIVE_DEVICE = (
    "DecoderStepFused", "ThetaOdeFused", "OdeSolveObserve", "OdeLogLikFused", "ode_logp_only", "adaptive_grid",
    "AdaptiveOdeSolve")
GENERAL_TAIL = "GeneralTail"  # (not a forward route: the key of the step tail's declines in the same cache)

# What a forward ran, written where it is known and handed to the solution's constructor: the route, its autograd nodes
# (the outputs' grad_fn at the .apply call site; theta_node: the sampling launch's, ThetaOdeFused's own node when it held
# the sampling stage), the generator state a fused forward left for the tail to step, and what Training.cost may do
ForwardRecord = namedtuple("ForwardRecord", "route ode_node theta_node rng_state has_logp defer_iwae online_summaries",
                           defaults=(None, None, None, None, True, False, None))


class DecodedSolution(object):
    """What one fused kernel launch produced for a batch: views in the reference's layouts."""

    def __init__(self, traj, xpred, logp, record, observe=None):
        self.traj_buffer, self._xpred, self.logp_buffer = traj, xpred, logp  # [T,N,B,S], [T,4,B,S], [4,B,S]
        self.sol = traj.permute(2, 3, 1, 0)          # [B,S,N,T]  (reference ode.py:82)
        self.log_p_by_species = logp.permute(1, 2, 0)  # [B,S,4] (reference training.py:24-33)
        self.record, self.has_logp, self.online_summaries = record, record.has_logp, record.online_summaries
        self._observe = observe  # xpred None (params.lazy_x_predict): the map that forms it from `sol` if somebody asks

    @property
    def has_x_predict(self):
        return self._xpred is not None

    @property
    def xpred_buffer(self):
        if self._xpred is None:
            self._xpred = self._observe(self.sol).permute(3, 2, 0, 1).contiguous()
        return self._xpred

    @property
    def x_predict(self):
        return self.xpred_buffer.permute(2, 3, 1, 0)   # [B,S,4,T]  (reference ode.py:84-93)


class LazySolution(object):
    """What the fused training kernel produced: the per-species log-likelihood only.  Trajectory and x_predict are
    computed (by the ordinary forward kernel, as a fresh autograd node on the same theta) if and when somebody asks."""

    def __init__(self, logp, record, materialise):
        self.logp_buffer = logp
        self.log_p_by_species = logp.permute(1, 2, 0)
        self.record, self.has_logp, self.online_summaries = record, record.has_logp, record.online_summaries
        self._materialise, self._full = materialise, None

    def full(self):
        if self._full is None:
            self._full = self._materialise()
        return self._full

    traj_buffer = property(lambda self: self.full().traj_buffer)
    xpred_buffer = property(lambda self: self.full().xpred_buffer)
    sol = property(lambda self: self.full().sol)
    x_predict = property(lambda self: self.full().x_predict)


def sampling_route(request, vae, q, data, samples):
    """The launch that holds the sampling stage of a forward under autograd -- DECODER_STEP_FUSED or THETA_ODE_FUSED -- or
    None: the sampling kernel on its own, then the decoder (likelihood_route).  A route that raises
    ops.FusedTrainingUnsupported is entered into `_fused_declined` by BaseVAE.forward, which asks again."""
    import vihds.hip as hip

    ode, prm = vae.decoder.ode_model, vae.decoder.config.params
    obs = data.get("observations", None) if hasattr(data, "get") else None
    if (not torch.is_grad_enabled() or obs is None or not obs.is_cuda or getattr(q, "_packed_q", None) is None
            or prm.solver in hip.ADAPTIVE_SOLVERS):
        return None
    declined, shape = ode._fused_declined, (tuple(obs.shape), samples, prm.solver)
    if (default_get_value(prm, "fused_ode_training", True) and default_get_value(prm, "fused_decoder_step", True)
            and ode.model_key in ode.fused_training_keys and not declined.get((DECODER_STEP_FUSED,) + shape)):
        return DECODER_STEP_FUSED
    # the models whose forward kernels carry the sampling stage: relay / degrader / prpr / auto_constant (+ _precisions) --
    # a device conditioner is no stage of theirs -- and dr_blackbox at the built-in sizes, whose condition_theta is one when
    # it runs on the device and the offset layer's source rows sit back to back
    if not request.fuse_sampling or vae.shard is not None or declined.get((THETA_ODE_FUSED,) + shape):
        return None
    if ode.model_key != "dr_blackbox":
        return None if getattr(ode, "extra_theta_names", ()) else THETA_ODE_FUSED
    if ode.n_y > 0 and (not vae.decoder.condition_on_device or ode.offset_source_row(q.names()) < 0):
        return None
    return THETA_ODE_FUSED


def likelihood_route(request, ode, config, theta, times, observations):
    """(route, packed theta, spec) of a forward once theta is sampled.  Under autograd ODE_LOGLIK_FUSED where the model has
    that launch; under no_grad ODE_LOGP_ONLY, the summaries-on-the-way form, which is opt-in per call (Training.evaluate
    asks for it): any other forward under no_grad -- plots, xval scripts, plugin code that reads x_states / x_predict --
    keeps the stored trajectory, for which the lazy solution's full solve would be a THIRD integration.  Otherwise
    (ODE_SOLVE_OBSERVE, None, None): the ordinary forward.  theta is packed only where a route gets that far."""
    import vihds.hip as hip

    prm, grad, plain = config.params, torch.is_grad_enabled(), (ODE_SOLVE_OBSERVE, None, None)
    if grad:
        fits = ode.model_key in ode.fused_training_keys and default_get_value(prm, "fused_ode_training", True)
    else:
        fits = (request.purpose == EVALUATE and request.online_summaries and default_get_value(prm, "online_summaries", True)
                and default_get_value(prm, "lazy_x_predict", True) and not getattr(theta, "_row_offset", None))
    if not fits or observations is None or prm.solver in hip.ADAPTIVE_SOLVERS:
        return plain
    packed, row_of = theta.pack(ode.kernel_slots())
    if not packed.is_cuda or (grad and not packed.requires_grad):
        return plain
    spec, shape = ode._spec(config, row_of, packed.shape[0], times.shape[0]), (packed.shape[1], packed.shape[2], times.shape[0])
    if grad:
        fits = not ode._fused_declined.get((ODE_LOGLIK_FUSED,) + shape + (prm.solver,))
    else:
        fits = ops.ode_fwd_summaries_supported(spec, *shape)
    return (ODE_LOGLIK_FUSED if grad else ODE_LOGP_ONLY, packed, spec) if fits else plain


def x_predict_on_demand(request, ode, config):
    """Whether the ordinary forward leaves x_predict to whoever asks for it.  Evaluation passes (no graph to differentiate)
    do: Training.cost's summaries form it inside their kernel, plugin code reading DecoderResult gets it from the
    observation map; so do training steps whose backward is ops.GeneralTail (request.general_tail): nobody reads it there.
    A map of the model's own -- observe_kind "custom", vihds/modelgen.py -- exists in its kernels only and may read theta:
    such a model always stores x_predict, and the summaries take it from that buffer; so does a model with a precision map
    of its own -- its precision rows go to vihds_iw_summaries, which takes x_predict as a buffer -- and a model with a state
    jump (has_jump, vihds/modelgen.py): what is read afterwards is the buffer its kernel scored, the left limits.  A model
    with a start map, steady species or a lead-in phase (has_start / n_steady_species / has_lead_in) likewise: its evaluation
    stores what its kernel scored; a
    model with process noise (has_diffusion) likewise: the stored buffers are the realisation its kernel scored."""
    return ((not torch.is_grad_enabled() or request.general_tail)
            and bool(default_get_value(config.params, "lazy_x_predict", True)) and ode.observe_kind != "custom"
            and ode.precision_kind != "custom" and not getattr(ode, "has_jump", False)
            and not getattr(ode, "has_start", False) and not getattr(ode, "has_lead_in", False)
            and not getattr(ode, "n_steady_species", 0)
            and not getattr(ode, "has_diffusion", False))


class DeviceConditioner(nn.Module):
    """Linear(D,1) -> ReLU with weights ~ N(2, 1.5) (reference ode.py:99-116)."""

    def __init__(self, n_inputs, use_bias=False, activation="relu"):
        super(DeviceConditioner, self).__init__()
        self.cond = nn.Linear(n_inputs, 1, use_bias)
        nn.init.xavier_uniform_(self.cond.weight)
        nn.init.normal_(self.cond.weight, mean=2.0, std=1.5)
        self.act = nn.ReLU()

    def forward(self, x):
        return self.act(self.cond(x))


class OdeModel(nn.Module):
    """Plugin interface (reference ode.py:28-96): subclasses set `species`, `n_species`, `precisions`,
    `model_key` (the models.LOOKUP key = the kernel to run) and may override condition_theta / observe."""

    model_key = None
    observe_kind = "default"
    precision_kind = "fixed"  # "custom": a generated model's own precision map (vihds/modelgen.py)
    likelihood_kind = "gaussian"  # "custom": a generated model's own observation log density (vihds/modelgen.py)

    def __init__(self, config):
        super(OdeModel, self).__init__()
        self.device_depth = config.data.device_depth
        self.n_treatments = len(config.data.conditions)
        self.use_laplace = default_get_value(config.params, "use_laplace", False, verbose=True)
        if self.use_laplace:
            raise NotImplementedError("use_laplace: the reference's Laplace log-prob (training.py:36-38) cannot "
                                      "run (torch.log of a float); only the Gaussian likelihood is implemented")
        self.precisions = None
        self.species = None
        self.n_species = None
        self.relevance = config.data.relevance_vectors
        self.default_devices = config.data.default_devices
        self.device = config.device
        self.conditioner_rng = default_get_value(config.params, "conditioner_rng", "cpu")
        self._spec_cache = {}
        self._tile_index = {}
        self._relevance_dev = {}
        self._rng_state = None
        self._fused_declined = {}  # (route, shape...) -> True: what a launch has declined once is not asked for again
        self._last = None
        self._last_inputs = None  # (packed theta, row_of, treatments) of the last solve: what a custom observation map reads

    # ---- device conditioning (reference ode.py:43-58) ----------------------------------------------
    def device_conditioner(self, param, param_name, dev_1hot, use_bias=False, activation="relu"):
        """NB reference behaviour kept: a NEW DeviceConditioner with fresh N(2,1.5) weights on every call
         -- the weights are not trained."""
        n_batch, n_iwae = param.shape[0], param.shape[1]
        n_inputs = dev_1hot.shape[1]
        if self.conditioner_rng in ("device", "kernel") and dev_1hot.is_cuda:
            weight = 2.0 + 1.5 * torch.randn((1, n_inputs), device=dev_1hot.device)
        else:
            weight = DeviceConditioner(n_inputs, use_bias=use_bias, activation=activation).cond.weight.detach()
            weight = weight.to(dev_1hot.device)
        rkey = (param_name, str(dev_1hot.device))
        if rkey not in self._relevance_dev:  # uploaded once: no host->device copy inside a captured step
            self._relevance_dev[rkey] = torch.as_tensor(self.relevance[param_name], device=dev_1hot.device)
        rel = self._relevance_dev[rkey]
        cond = torch.relu(torch.nn.functional.linear(dev_1hot * rel, weight)).reshape(-1)  # [B]
        # Reference quirk kept on purpose (ode.py:46,52-57): `param` is flattened row-major (k = b*S+s) but the
        # conditioner output is tiled with .repeat([S,1]) (k -> cond[k mod B]), so entry (b,s) is scaled by the
        # value of row (b*S+s) mod B, not row b.
        window = getattr(param, "_sample_window", None) or (n_iwae, 0)  # (S_total, s_offset) under S-sharding
        key = (n_batch, n_iwae, window, str(dev_1hot.device))
        if key not in self._tile_index:
            b = torch.arange(n_batch, device=dev_1hot.device)[:, None]
            sidx = torch.arange(n_iwae, device=dev_1hot.device)[None, :]
            self._tile_index[key] = (b * window[0] + window[1] + sidx) % n_batch
        param_cond = cond[self._tile_index[key]]
        if param_name in self.default_devices:
            return param * (1.0 + param_cond)
        return param * param_cond

    # names of attributes condition_theta adds to theta (rows reserved behind the sampled parameters)
    extra_theta_names = ()

    def conditioner_job(self, names, dev_1hot):
        """(relevance [E,D], is_default [E], z or None, w_mean, w_std, rng_state or None) for the conditioner kernel:
        a fresh N(2, 1.5) weight draw per call as in the reference (ode.py:48), on the stream `conditioner_rng` names."""
        dev = dev_1hot.device
        key = (tuple(names), str(dev))
        if key not in self._relevance_dev:
            rel = torch.tensor(np.stack([self.relevance[n] for n in names]), dtype=torch.float32, device=dev)
            dflt = torch.tensor([1 if n in self.default_devices else 0 for n in names], dtype=torch.int32, device=dev)
            self._relevance_dev[key] = (rel, dflt)
        rel, dflt = self._relevance_dev[key]
        D = dev_1hot.shape[1]
        rng_state = None
        if self.conditioner_rng == "kernel":  # drawn inside the kernel (no launch for the draw, graph-capturable)
            if self._rng_state is None:
                self._rng_state = ops.KernelNormal.new_state(int(torch.randint(0, 2 ** 62, (1,)).item()), dev)
            z, mean, std, rng_state = None, 2.0, 1.5, self._rng_state
        elif self.conditioner_rng == "device":
            z, mean, std = torch.randn((len(names), D), device=dev), 2.0, 1.5
        else:  # the reference's stream: a fresh DeviceConditioner per name, drawn on the host
            from vihds import hostdraws

            def draw(host=None, k=len(names)):
                # what constructing k DeviceConditioner(D) modules draws from torch's CPU generator, without the modules:
                # nn.Linear's own initialisation and xavier_uniform_ (a uniform_ of the weight each: the stream advances by
                # the same amount whatever the bounds), then the N(2, 1.5) weights that are kept
                w = torch.empty((k, D)) if host is None else torch.from_numpy(host).view(k, D)
                for row in w:
                    row = row.view(1, D)
                    row.uniform_()
                    row.uniform_()
                    row.normal_(mean=2.0, std=1.5)
                return w

            if hostdraws.capturing():  # a captured step: drawn before every replay (vihds/hostdraws.py)
                z = hostdraws.ACTIVE.add((len(names), D), dev, draw)
            else:
                hostdraws.note((len(names), D))
                z = draw().to(dev)
            mean, std = 0.0, 1.0
        return rel, dflt, z, mean, std, rng_state

    def condition_ones(self, theta, names, dev_1hot):
        """theta.<name> = device_conditioner(ones, name, dev_1hot) for several names in ONE kernel launch, written
        straight into rows reserved in theta's packed buffer (falls back to the op-by-op path when theta has no
        reserved rows, e.g. when it was built by hand)."""
        n_batch, n_iwae = theta.get_n_batch(), theta.get_n_samples()
        base = len(theta.samples)
        if theta.n_reserved_rows() < len(names) or not dev_1hot.is_cuda:
            ones = torch.ones((n_batch, n_iwae), device=dev_1hot.device)
            for n in names:
                setattr(theta, n, self.device_conditioner(ones, n, dev_1hot))
            return theta
        rel, dflt, z, mean, std, rng_state = self.conditioner_job(names, dev_1hot)
        with torch.no_grad():
            ops.device_condition(z, dev_1hot, rel, dflt, theta._packed[base: base + len(names)], mean, std,
                                 rng_state, getattr(theta, "_sample_window", None))
        for j, n in enumerate(names):
            theta.bind_reserved_row(n, base + j)
        return theta

    def condition_theta(self, theta, dev_1hot, writer, epoch):
        raise NotImplementedError("TODO: write your condition_theta")

    # ---- kernel problem description -----------------------------------------------------------------
    def neural_weights(self):
        """Flat weight buffer for models with neural blocks (None for white-box models)."""
        return None

    def flat_weight_tensors(self):
        """The nn.Parameters behind neural_weights(), in the flat buffer's order ([] for white-box models): what
        ops.GeneralTail updates in the step's last launch."""
        prec = self.precisions
        return list(prec.weight_tensors()) if getattr(prec, "dynamic", False) else []

    def problem_kwargs(self, config):
        return {}

    def kernel_slots(self):
        """Parameter names in the order the kernel reads them (the library's table; dr_blackbox builds its own from
        n_z / n_x / n_y)."""
        import vihds.hip as hip

        return hip.model_slots(self.model_key)

    def row_inputs(self, data):
        """The rows of `cond` the kernels read for a batch: the treatments.  (A generated model with forcings appends their
        samples, vihds/modelgen.py; callers that solve for a batch pass this, not data.inputs.)  A batch with 'observed' -- a
        mask of missing observations -- is for a generated model with missing_observations = True alone: these kernels would
        score the placeholders, so it is refused here (a look at the batch's keys: nothing is read back from the device)."""
        observed = data.get("observed", None) if hasattr(data, "get") else getattr(data, "observed", None)
        if observed is not None:
            raise RuntimeError("the batch carries 'observed' (a mask of missing observations), and %s is not a generated model "
                               "with missing_observations = True: only such a model scores by it -- every other model's "
                               "kernels would score the placeholders" % type(self).__name__)
        return data.inputs

    def cond_width(self, n_times=None):
        """Floats per row of cond (the problem's C) on a grid of n_times points."""
        return self.n_treatments

    def _spec(self, config, row_of, n_rows, n_times=None):
        C = self.cond_width(n_times)
        key = (config.params.solver, n_rows, tuple(sorted(row_of.items())), C)
        if key not in self._spec_cache:
            # params.adjoint_solver (reference ode.py:80: torchdiffeq.odeint_adjoint, the continuous adjoint) selects
            # nothing here: every solver differentiates through the discrete adjoint of its own accepted steps, which is
            # the gradient of what was actually computed
            kw = dict(self.problem_kwargs(config))
            # params.kernel_variant: 0 = the library's choice, 1 thread-per-trajectory, 2 lane-split, 3 time-parallel
            kw.setdefault("kernel_variant", int(default_get_value(config.params, "kernel_variant", 0)))
            self._spec_cache[key] = ops.OdeProblemSpec(self.model_key, config.params.solver, row_of, n_rows,
                                                       C=C, D=self.device_depth, **kw)
        return self._spec_cache[key]

    def solve(self, config, times, theta, conditions, dev_1hot, observations=None, request=None):
        """One fused launch: trajectory, observed signals and (if observations are given) the per-species
        log-likelihood.  Returns a DecodedSolution."""
        import vihds.hip as hip

        request = request or PLAIN_FORWARD
        slots = self.kernel_slots()
        packed, row_of = theta.pack(slots)
        self._last_inputs = (packed, row_of, conditions)
        spec = self._spec(config, row_of, packed.shape[0], len(times))
        dev = packed.device
        times = times.to(dev)
        if config.params.solver in hip.ADAPTIVE_SOLVERS:
            return self._solve_adaptive(config, spec, packed, row_of, times, theta, conditions, dev_1hot, observations)
        obs = observations
        if obs is None:  # likelihood not requested: feed zeros (logp output is then meaningless and unused)
            obs = torch.zeros((packed.shape[1], 4, times.shape[0]), device=dev)
        row_offset, row_offset_map = getattr(theta, "_row_offset", None) or (None, None)
        lazy = x_predict_on_demand(request, self, config)
        traj, xpred, logp = ops.OdeSolveObserve.apply(spec, packed, conditions.to(dev), times, obs.to(dev),
                                                      dev_1hot.to(dev) if dev_1hot is not None else None,
                                                      self.neural_weights(), row_offset, row_offset_map, not lazy)
        record = ForwardRecord(ODE_SOLVE_OBSERVE, logp.grad_fn, getattr(theta, "_node", None),
                               has_logp=observations is not None)
        self._last = DecodedSolution(traj, xpred, logp, record, observe=lambda sol: self._observe_map(sol))
        return self._last

    @staticmethod
    def _with_room(config, rtol, atol, size, overflow, run):
        """run(size), with the caller-sized buffer quadrupled up to 2^17 points while run raises `overflow(exc)`: only the
        controller running out of its buffer is worth a larger one; anything else is re-raised as it is."""
        while True:
            try:
                return run(size)
            except RuntimeError as e:
                if not overflow(e):
                    raise
                if size >= (1 << 17):
                    raise RuntimeError(
                        "solver %r with rtol=%g, atol=%g needs more than %d accepted steps on this batch: in fp32 a relative "
                        "tolerance below ~1e-6 is at rounding level for a low-order pair -- raise params.solver_rtol / "
                        "solver_atol (or params.solver_max_grid)" % (config.params.solver, rtol, atol, size)) from e
                size *= 4

    def _adaptive_solution(self, route, spec, packed, row_of, traj, xpred, observations):
        """The DecodedSolution of an adaptive route: the log-likelihood at the output times with torch ops (observations
        exist there only) from the precision rows -- autograd then hands the adjoint kernel its upstream gradients."""
        if observations is not None:
            if spec.n_precision_rows:  # neural precisions: the four states behind the species (reference precisions.py:89-94)
                prec = traj[:, spec.n_species:spec.n_species + 4, :, :]
            else:  # constant precisions: four theta rows broadcast over time (reference precisions.py:31-35)
                rows = [row_of[n] for n in spec.slots[-4:]]
                prec = packed[rows][None]
            if self.likelihood_kind == "custom":
                # the model's own log density (vihds/modelgen.py) on the gathered rows, with theta and the treatments of this
                # solve: [T,4,B,S] -> [B,S,4,T] and back, summed over time
                ll = self._log_likelihood_map(xpred.permute(2, 3, 1, 0), observations, prec.permute(2, 3, 1, 0))
                logp = ll.sum(3).permute(2, 0, 1)
            else:
                err = xpred - observations.to(packed.device).permute(2, 1, 0)[:, :, :, None]
                logp = (-0.5 * (math.log(2 * math.pi) - torch.log(prec) + prec * err * err)).sum(0)  # training.py:24-44
        else:
            logp = torch.zeros((4,) + tuple(packed.shape[1:]), device=packed.device)
        self._last = DecodedSolution(traj, xpred, logp, ForwardRecord(route, has_logp=observations is not None))
        return self._last

    def _solve_adaptive(self, config, spec, packed, row_of, times, theta, conditions, dev_1hot, observations):
        """torchdiffeq's adaptive pairs (reference ode.py:79-81; dopri5 / bosh3 / adaptive_heun): the controller picks ONE
        accepted grid for the batch (ops.adaptive_grid), the ordinary kernels integrate on it with the pair's
        higher-order tableau, the rows of the output times are gathered, and the log-likelihood is evaluated on the
        gathered x_predict (_adaptive_solution)."""
        dev = packed.device
        cond = conditions.to(dev)
        d1 = dev_1hot.to(dev) if dev_1hot is not None else None
        weights = self.neural_weights()
        rtol = float(default_get_value(config.params, "solver_rtol", 1e-7))  # torchdiffeq.odeint defaults
        atol = float(default_get_value(config.params, "solver_atol", 1e-9))
        # The accepted grid lives in a caller-sized buffer: params.solver_max_grid (default 4096 points); when the controller
        # runs out of it the buffer is quadrupled (_with_room) before giving up with a message that names the cause --
        # all arithmetic is fp32, so tolerances near its epsilon (torchdiffeq's defaults 1e-7 / 1e-9 with a low-order pair
        # such as adaptive_heun) ask for step sizes the state cannot resolve
        max_grid = int(default_get_value(config.params, "solver_max_grid", 4096))
        # torchdiffeq's own algorithm, resident on the device (round 4): steps run past the output times, outputs come from
        # the accepted step's quartic interpolant, the adjoint walks the logged accepted steps -- models without shared
        # neural weights; params.adaptive_device: false keeps the clipped-grid controller below for them too
        B, S = packed.shape[1], packed.shape[2]
        # (round 5: also the *_precisions models without a hidden layer -- the library says which problems it takes)
        if (bool(default_get_value(config.params, "adaptive_device", True))
                and ops.adaptive_device_supported(spec, B, S, int(times.shape[0]), max_grid) is not None):
            return self._solve_adaptive_device(config, spec, packed, row_of, times, cond, d1, observations, rtol, atol, max_grid,
                                               weights)
        # (the C ABI's message for the controller running out of its buffer; step-size underflow, a non-finite error estimate
        # or bad arguments are re-raised as they are)
        grid, index = self._with_room(
            config, rtol, atol, max_grid, lambda e: "does not fit max_grid" in str(e),
            lambda n: ops.adaptive_grid(spec, packed, cond, times, d1, weights, rtol, atol, max_grid=n))
        self.last_adaptive_grid = grid
        dummy = torch.zeros((packed.shape[1], 4, grid.shape[0]), device=dev)
        row_offset, row_offset_map = getattr(theta, "_row_offset", None) or (None, None)
        traj_g, xpred_g, _ = ops.OdeSolveObserve.apply(spec, packed, cond, grid, dummy, d1, weights, row_offset,
                                                       row_offset_map)
        traj, xpred = traj_g.index_select(0, index), xpred_g.index_select(0, index)  # [T,N,B,S], [T,4,B,S]
        return self._adaptive_solution(ADAPTIVE_HOST, spec, packed, row_of, traj, xpred, observations)

    def _solve_adaptive_device(self, config, spec, packed, row_of, times, cond, d1, observations, rtol, atol, max_steps,
                               weights=None):
        """ops.AdaptiveOdeSolve + the observation map and the log-likelihood with torch ops on the solution at the output
        times (autograd hands the adjoint kernel the upstream gradient of the trajectory)."""
        check = bool(default_get_value(config.params, "adaptive_check", True))  # False: no synchronisation (capturable)
        stats = [0, 0, 0]
        traj = self._with_room(
            config, rtol, atol, max_steps, lambda e: isinstance(e, ops.GridOverflow),
            lambda n: ops.AdaptiveOdeSolve.apply(spec, packed, cond, times, d1, rtol, atol, n, check, stats, weights))
        self.last_adaptive_stats = {"accepted": stats[1], "rejected": stats[2]}
        self.last_adaptive_grid = None
        xpred = self._observe_map(traj.permute(2, 3, 1, 0)).permute(3, 2, 0, 1).contiguous()  # [B,S,N,T] -> [T,4,B,S]
        return self._adaptive_solution(ADAPTIVE_DEVICE, spec, packed, row_of, traj, xpred, observations)

    fused_training_keys = ("dr_constant", "dr_constant_v2")

    def solve_for_training(self, config, times, theta, conditions, dev_1hot, observations, request=None):
        """The forward that leaves the trajectory out, where the request and the model allow one (likelihood_route): under autograd ONE launch gives the log-likelihood and the unit-weight adjoint
        (params.fused_ode_training, ops.OdeLogLikFused); under no_grad the evaluation without the trajectory's round trip
        (_solve_for_evaluation).  Returns a LazySolution, or None when neither applies (then use solve)."""
        route, packed, spec = likelihood_route(request or PLAIN_FORWARD, self, config, theta, times, observations)
        if route == ODE_SOLVE_OBSERVE:
            return None
        dev = packed.device
        args = (packed, conditions.to(dev), times.to(dev), dev_1hot.to(dev) if dev_1hot is not None else None)
        full = lambda: self.solve(config, times, theta, conditions, dev_1hot, observations)  # noqa: E731
        if route == ODE_LOGP_ONLY:
            return self._solve_for_evaluation(spec, args + (self.neural_weights(),), observations.to(dev), full)
        try:
            logp = ops.OdeLogLikFused.apply(spec, args[0], args[1], args[2], observations.to(dev), args[3])
        except ops.FusedTrainingUnsupported:
            self._fused_declined[(route, packed.shape[1], packed.shape[2], times.shape[0], config.params.solver)] = True
            return None
        self._last = LazySolution(logp, ForwardRecord(route, logp.grad_fn), full)
        return self._last

    def _solve_for_evaluation(self, spec, args, observations, full):
        """Evaluation without the trajectory's round trip (params.online_summaries, default on): the forward launch writes
        the log-likelihoods ONLY, and Results' importance-weighted summaries come from a second forward launch that adds
        them up on the way (ops.ode_fwd_summaries) -- the trajectory (644 MB at 234 rows x 1 000 samples) is neither
        allocated, written nor read back: 1.33 GB -> 0.12 GB of HBM traffic for the two launches, at the same time per pass
        (0.68 ms either way: the integration is VALU-bound, the second one costs what streaming the trajectory back did;
        DESIGN.md section 1; profiles/LOG.md, round 5).  `online_summaries: false` keeps the stored form.
        Returns a LazySolution whose record carries `online_summaries(log_w, lse)`; trajectory and x_predict are computed
        (the ordinary forward launch, `full`) only if somebody asks.  likelihood_route says where the form applies (not
        dr_blackbox, the adaptive solvers, launches below the evaluation size, which run other kernel families)."""
        logp = ops.ode_logp_only(spec, args[0], args[1], args[2], observations, args[3], args[4])
        online = lambda log_w, lse: ops.ode_fwd_summaries(spec, *args, log_w, lse)  # noqa: E731
        self._last = LazySolution(logp, ForwardRecord(ODE_LOGP_ONLY, online_summaries=online), full)
        return self._last

    # ---- reference entry points ---------------------------------------------------------------------
    def simulate(self, config, times, theta, conditions, dev_1hot, condition_on_device=True, observations=None,
                 request=None):
        """reference ode.py:66-82 -> [B,S,N,T].  `request`: what the caller will do with the forward (ForwardRequest);
        an override that does not pass it on gets the plain forward, which is correct and stores x_predict."""
        return self.solve(config, times, theta, conditions, dev_1hot, observations, request=request).sol

    def expand_precisions(self, theta, times, x_states):
        return self.precisions.expand(theta, len(times), x_states)

    def observe(self, x_sample, _theta):
        """reference ode.py:84-93.  When x_sample is (a view of) the solution just simulated, the fused
        kernel's x_predict is returned; otherwise the observation map is evaluated with torch ops (a generated model's own
        map: GeneratedOdeModel.torch_observe with theta and the treatments of the last solve)."""
        last = self._last
        if last is not None and x_sample.data_ptr() == last.sol.data_ptr() and x_sample.shape[3] == last.sol.shape[3]:
            return last.x_predict
        return self._observe_map(x_sample)

    def _observe_map(self, x_sample):
        x0 = x_sample[:, :, 0, :]
        if self.observe_kind == "default":
            xp = [x0, x0 * x_sample[:, :, 1, :], x0 * (x_sample[:, :, 2, :] + x_sample[:, :, 4, :]),
                  x0 * (x_sample[:, :, 3, :] + x_sample[:, :, 5, :])]
        elif self.observe_kind == "inducer":  # models/inducer_constant.py:106-114
            xp = [x0, x0 * x_sample[:, :, 1, :], x0 * (x_sample[:, :, 2, :] + x_sample[:, :, 3, :]),
                  x0 * x_sample[:, :, 4, :]]
        else:
            xp = [x0, x0 * x_sample[:, :, 1, :], x0 * x_sample[:, :, 2, :], x0 * x_sample[:, :, 3, :]]
        return torch.stack(xp, dim=-1).permute(0, 1, 3, 2)

    def summaries(self, writer, epoch):
        pass
