"""Models with `implicit = True` (the generated Jacobian of vihds.modelgen and the backward-Euler solver "beuler") for the
tests: the prpr_constant and dr_constant restatements and the forced prpr model as implicit subclasses (DrImplicit has the
cap's eight species and a sparse Jacobian), a four-species binding model that is stiff at the inputs drawn for it, and an
eight-species model whose every derivative reads every species (the register worst case).

The float64 yardstick of the GPU comparisons is written here, once, for the host and the GPU tests: the scheme exactly as
include/vihds_hip.h defines it -- NEWTON iterations from y_k, the Jacobian by autograd of torch_problem's right-hand side,
the linear solve by torch.linalg.solve (pivoted) -- and the implicit-function adjoint at its own iterate."""
import torch

from oracle import vihds_oracle as O
from vihds.modelgen import GeneratedOdeModel
from vihds.precisions import ConstantPrecisions

from modelgen_forcing_models import PRPR_BASE, PrprForced, series_of, wide_cond
from modelgen_models import PREC, DrRestated, PrprRestated
from modelgen_piecewise_models import TIMES  # noqa: F401  (for the tests)


class PrprImplicit(PrprRestated):
    model_key = "gen_prpr_constant_implicit"
    implicit = True


class DrImplicit(DrRestated):
    """Eight species: the cap.  19 of the 64 entries of its Jacobian are structural non-zeros."""
    model_key = "gen_dr_constant_implicit"
    implicit = True


class PrprForcedImplicit(PrprForced):
    model_key = "gen_prpr_constant_forced_implicit"
    implicit = True


class FastBinding(GeneratedOdeModel):
    """A and B are produced and bind reversibly into C, which drives a reporter R through a Hill term; everything decays.  With
    kon of a few hundred the binding equilibrates in milliseconds: on a grid of steps 0.3 .. 0.6 the explicit schemes blow up."""
    model_key = "gen_fast_binding"
    species = ["A", "B", "C", "R"]
    parameters = ["kon", "koff", "prod", "deg", "a", "gain"]
    n_conditions = 0
    implicit = True
    newton_iterations = 6
    Y0 = [0.5, 0.2, 0.0, 0.0]

    def __init__(self, config):
        super(FastBinding, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"kon": th.kon, "koff": th.koff, "prod": th.prod, "deg": th.deg, "a": th.a, "gain": th.gain}

    def initial_state(self, th, c):
        return list(self.Y0)

    def rhs(self, t, y, p, c):
        A, B, C, R = y
        bind = p.kon * A * B - p.koff * C
        return [p.prod - bind - p.deg * A,
                0.5 * p.prod - bind - p.deg * B,
                bind - p.deg * C,
                p.a * C * C / (0.25 + C * C) - p.deg * R]

    def observe(self, y, p, c):
        A, B, C, R = y
        return [A + C, B + C, p.gain * C, R]


class DenseEight(GeneratedOdeModel):
    """Eight species coupled through their total: every entry of the Jacobian is a structural non-zero."""
    model_key = "gen_dense_eight"
    species = ["OD", "RFP", "YFP", "CFP", "F530", "F480", "U", "V"]
    parameters = ["a", "b", "k", "init_x"]
    n_conditions = 0
    observe_kind = "default"
    implicit = True

    def __init__(self, config):
        super(DenseEight, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"a": th.a, "b": th.b, "k": th.k}

    def initial_state(self, th, c):
        return [(1.0 + 0.1 * j) * th.init_x for j in range(8)]

    def rhs(self, t, y, p, c):
        total = y[0] + y[1] + y[2] + y[3] + y[4] + y[5] + y[6] + y[7]
        return [p.a * (0.2 * (j + 1) - y[j]) - p.b * y[j] * total / (1.0 + total) + p.k * y[(j + 1) % 8] * y[(j + 3) % 8]
                for j in range(8)]


MODELS = [PrprImplicit, DrImplicit, PrprForcedImplicit, FastBinding, DenseEight]
# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(cls, False) for cls in MODELS]

# ---- inputs of the numeric tests ----------------------------------------------------------------------------------------------
_PREC_BASE = {"prec_x": 50.0, "prec_rfp": 20.0, "prec_yfp": 20.0, "prec_cfp": 20.0}
DR_BASE = dict(PRPR_BASE, dR=0.4, dS=0.5, e76=0.1, e81=0.15, KGR_76=0.8, KGS_76=0.3, KGR_81=0.2, KGS_81=0.9, aYFP=1.2,
               aCFP=0.9, aR=0.7, aS=0.6, nR=1.5, nS=1.2, KR6=0.3, KR12=0.05, KS6=0.04, KS12=0.4, init_luxR=0.1, init_lasR=0.1)
for _n in ("aYFP_PR", "aCFP_PR"):
    del DR_BASE[_n]
DENSE_BASE = dict(_PREC_BASE, a=0.8, b=0.5, k=0.3, init_x=0.1)
# FastBinding: (median, log-sd) -- kon = 400 exp(eps), koff = 50 exp(eps), the others narrow
FAST_DRAWS = dict({"kon": (400.0, 1.0), "koff": (50.0, 1.0), "prod": (1.0, 0.3), "a": (1.0, 0.3), "deg": (0.3, 0.3),
                   "gain": (1.2, 0.2)}, **{n: (v, 0.2) for n, v in _PREC_BASE.items()})
# The grid of the models with a growth term (every model but FastBinding): steps 0.1 .. 0.15 .. 0.2, not uniform.  Newton's
# iteration from y_k solves the step of a GROWING mode only while h * rate stays well below 1 (at h * rate = 1 the matrix
# I - h J is singular): on modelgen_piecewise_models.TIMES (steps up to 0.6, growth rates up to 1.8) four iterations leave
# increments of order 1, here they reach 1e-16.  The tests assert that as their precondition.
GRID = [0.0, 0.1, 0.25, 0.35, 0.55, 0.7, 0.9, 1.05, 1.25]
BASES = {PrprImplicit: PRPR_BASE, PrprForcedImplicit: PRPR_BASE, DrImplicit: DR_BASE, DenseEight: DENSE_BASE}
_PROBLEMS = {}


def slot_names(cls):
    return list(cls.parameter_names) + list(PREC)


def grid_of(cls):
    return TIMES if cls is FastBinding else GRID


def problem(cls, B, S, times=None, seed=17, r_scale=1.0):
    """Inputs of one case (shared by the tests that use it; never modified): theta [B,S] per slot, cond (the wide rows of the
    forced model), times (grid_of(cls) unless given), observations (the first sample's backward-Euler prediction with 5 %
    noise) and an upstream gradient for the log-likelihood.  r_scale scales the growth rate (a grid with long steps)."""
    times = grid_of(cls) if times is None else times
    k = (cls, B, S, tuple(times), seed, r_scale)
    if k in _PROBLEMS:
        return _PROBLEMS[k]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    tt = torch.tensor(list(times), dtype=torch.float64)
    T = tt.shape[0]
    if cls is FastBinding:
        th = {n: m * torch.exp(sd * rnd(B, S)) for n, (m, sd) in FAST_DRAWS.items()}
    else:
        th = {n: v * torch.exp(0.2 * rnd(B, S)) * (r_scale if n == "r" else 1.0) for n, v in BASES[cls].items()}
    treatments = 0.3 + 0.7 * torch.arange(B, dtype=torch.float64)[:, None].expand(B, int(cls.n_conditions))
    series = series_of(cls, B, tt) if cls.forcings else torch.zeros(B, 0, T, dtype=torch.float64)
    cond = wide_cond(treatments, series)
    with torch.no_grad():
        th1 = {n: v[:, :1] for n, v in th.items()}
        xs = beuler(cls, th1, cond, tt)[0]
        obs = signals(cls, xs, th1, cond)[:, 0] * (1.0 + 0.05 * rnd(B, 4, T))
    pb = {"th": th, "cond": cond, "series": series, "times": tt, "obs": obs, "W": {}, "B": B, "S": S, "T": T,
          "G": {"logp": rnd(B, S, 4)}}
    _PROBLEMS[k] = pb
    return pb


# ---- the definition of the scheme in torch -------------------------------------------------------------------------------------
def torch_rhs(cls, th, cond, times):
    kw = {"times": times} if cls.forcings else {}
    return cls.torch_problem(th, cond, None, **kw)


def autograd_jacobian(rhs, t, z, create_graph=False):
    """[B,S,N,N] with entry [i][j] = d f_i / d z_j of rhs(t, .) at z [B,S,N] (trajectories do not interact: the gradient of a
    component's sum over the batch is that component's row for every trajectory)."""
    with torch.enable_grad():
        z = z if z.requires_grad else z.detach().requires_grad_(True)
        f = rhs(t, z)
        rows = []
        for i in range(z.shape[-1]):
            fi = f[..., i].sum()
            g = torch.autograd.grad(fi, z, create_graph=create_graph, retain_graph=True, allow_unused=True)[0] \
                if fi.requires_grad else None
            rows.append(torch.zeros_like(z) if g is None else g)
    J = torch.stack(rows, dim=-2)
    return J if create_graph else J.detach()


def newton_step(rhs, t1, h, y, newton, jacobian=autograd_jacobian):
    """One step of the scheme as defined: z = y; `newton` times F = z - y - h f(t1, z), A = I - h J(t1, z), solve A d = -F,
    z += d.  Returns (z, the last increment d)."""
    eye = torch.eye(y.shape[-1], dtype=y.dtype)
    z, d = y, None
    for _ in range(newton):
        F = z - y - h * rhs(t1, z)
        A = eye - h * jacobian(rhs, t1, z)
        d = torch.linalg.solve(A, -F.unsqueeze(-1)).squeeze(-1)
        z = z + d
    return z, d


def beuler(cls, th, cond, times, newton=None):
    """(species [B,S,N,T], the largest last Newton increment relative to the state's size) of the scheme on `times`."""
    rhs, x0 = torch_rhs(cls, th, cond, times)
    newton = int(cls.newton_iterations) if newton is None else newton
    ys, y, worst = [x0], x0, 0.0
    with torch.no_grad():
        for k in range(len(times) - 1):
            y, d = newton_step(rhs, times[k + 1], times[k + 1] - times[k], y, newton)
            worst = max(worst, float((d.abs().amax(-1) / y.abs().amax(-1).clamp_min(1e-30)).max()) if bool(torch.isfinite(d).all())
                        else float("inf"))
            ys.append(y)
    return torch.stack(ys, dim=3), worst


def signals(cls, xs, th, cond):
    if cls._observe_def is not None:
        return cls.torch_observe(xs, th, cond)
    return O.observe_direct(xs) if cls.observe_kind == "direct" else O.observe_default(xs)


def log_likelihood(cls, xs, th, cond, obs):
    """(x_predict [B,S,4,T], per-signal log-likelihood [B,S,4]) of the species xs: the model's map and constant precisions."""
    xp = signals(cls, xs, th, cond)
    prec = torch.stack([th[n] for n in PREC], dim=2)[:, :, :, None].expand_as(xp)
    return xp, O.log_prob_observations(xp, obs, prec)


def definition(cls, pb, dtype):
    """The scheme in `dtype` and the gradient of sum(logp * G) with respect to theta by the implicit-function adjoint at the
    scheme's own iterate: lambda_T-1 = dL/dy_T-1; per step, last to first, A = I - h J(t1, y_k+1), A^T mu = lambda, the
    parameter part (h mu)^T df/dtheta at (t1, y_k+1), lambda = mu + dL/dy_k; the initial state's part last."""
    leaf = lambda v: v.to(dtype).detach().clone().requires_grad_(True)  # noqa: E731
    th = {n: leaf(v) for n, v in pb["th"].items()}
    names = list(th)
    cond, times, obs = pb["cond"].to(dtype), pb["times"].to(dtype), pb["obs"].to(dtype)
    xs, last = beuler(cls, th, cond, times)
    T, N = xs.shape[3], xs.shape[2]
    Y = xs.detach().clone().requires_grad_(True)
    xp, logp = log_likelihood(cls, Y, th, cond, obs)
    loss = (logp * pb["G"]["logp"].to(dtype)).sum()
    direct = torch.autograd.grad(loss, [Y] + [th[n] for n in names], allow_unused=True)
    gY = direct[0]
    g = {n: (torch.zeros_like(th[n]) if v is None else v.clone()) for n, v in zip(names, direct[1:])}
    rhs, x0 = torch_rhs(cls, th, cond, times)
    eye = torch.eye(N, dtype=dtype)

    def add(outputs, seed):
        if not outputs.requires_grad:
            return
        for n, v in zip(names, torch.autograd.grad(outputs, [th[n] for n in names], grad_outputs=seed, allow_unused=True,
                                              retain_graph=True)):  # (prepare's graph is shared by every step)
            if v is not None:
                g[n] += v

    lam = gY[..., T - 1]
    for k in range(T - 2, -1, -1):
        t1, h = times[k + 1], times[k + 1] - times[k]
        y1 = xs[..., k + 1].detach()
        A = eye - h * autograd_jacobian(rhs, t1, y1)
        mu = torch.linalg.solve(A.transpose(-1, -2), lam.unsqueeze(-1)).squeeze(-1)
        add(rhs(t1, y1), h * mu)
        lam = mu + gY[..., k]
    add(x0, lam)
    return {"traj": xs.detach(), "xpred": xp.detach(), "logp": logp.detach(), "loss": loss.detach(), "g_theta": g,
            "g_w": [], "last_increment": last}


# ---- FastBinding by hand (the refined-grid solution of the stiff test: no autograd in its 3 200 steps) ------------------------
def fast_rhs(th, y):
    A, B, C, R = y.unbind(-1)
    bind = th["kon"] * A * B - th["koff"] * C
    return torch.stack([th["prod"] - bind - th["deg"] * A, 0.5 * th["prod"] - bind - th["deg"] * B, bind - th["deg"] * C,
                        th["a"] * C * C / (0.25 + C * C) - th["deg"] * R], dim=-1)


def fast_jacobian(th, y):
    A, B, C, R = y.unbind(-1)
    kon, koff, deg, a = th["kon"], th["koff"], th["deg"], th["a"]
    z = torch.zeros_like(A)
    hill = a * 0.5 * C / (0.25 + C * C) ** 2
    rows = [[-kon * B - deg, -kon * A, koff + z, z], [-kon * B, -kon * A - deg, koff + z, z],
            [kon * B, kon * A, -koff - deg, z], [z, z, hill, -deg + z]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def fast_refined(th, times, refine=400, newton=2):
    """FastBinding on a grid `refine` times finer (backward Euler, `newton` iterations per small step): [B,S,4,T] at `times`."""
    y = torch.tensor(FastBinding.Y0, dtype=torch.float64).expand(th["kon"].shape + (4,))
    rhs, jac = (lambda t, z: fast_rhs(th, z)), (lambda f, t, z: fast_jacobian(th, z))
    ys = [y]
    for k in range(len(times) - 1):
        h = (times[k + 1] - times[k]) / refine
        for _ in range(refine):
            y, _d = newton_step(rhs, None, h, y, newton, jac)
        ys.append(y)
    return torch.stack(ys, dim=3)


def rk4_38(rhs, x0, times):
    """The 3/8 rule on `times` (what "rk4" is here) -> [B,S,N,T]."""
    return O.simulate(rhs, x0, times, "rk4")
