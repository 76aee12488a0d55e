"""New ODE models defined in Python and run on generated HIP kernels.

A model is one subclass of GeneratedOdeModel (the plugin surface of the reference's vihds/ode.py:20-96):

    class MyModel(GeneratedOdeModel):
        model_key = "my_model"
        species = ["OD", "RFP", ...]                 # ODE states, in order
        parameters = ["r", "K", ..., "init_x"]       # theta names the kernel reads, in slot order
        n_conditions = 0                             # treatments read per data row
        observe_kind = "default"                     # or "direct" (the fixed maps of the kernels), or define observe

        def __init__(self, config):
            super().__init__(config)
            self.precisions = ConstantPrecisions([...])   # or NeuralPrecisions(...), as the built-in models do

        def prepare(self, th, c):          # reference <Model>_RHS.__init__: named effective parameters
            return {"r": clamp(th.r, 0.0, 4.0), ...}
        def initial_state(self, th, c):    # reference initialize_state: one entry per species
            return [th.init_x, ..., 0.0]
        def rhs(self, t, y, p, c):         # reference OdeFunc.forward: one entry per species
            return [...]
        def observe(self, y, p, c):        # optional; reference observe(x_sample, theta): the OD, RFP, YFP, CFP signals
            return [y[0], p.gain * y[0] * y[1] + p.bg, ...]
        def precision(self, y, x, p, c):   # optional; the precisions of the four signals (then no self.precisions above)
            return [1.0 / (p.s0_od * p.s0_od + pow(p.s1_od * x[0], 2.0)), ...]
        def log_likelihood(self, x, obs, pr, p, c):   # optional; the four log densities of one time point
            return [C + 0.5 * log(pr[j]) - 0.5 * (NU + 1.0) * log(1.0 + pr[j] * (x[j] - obs[j]) * (x[j] - obs[j]) / NU) ...]

`c` holds the treatments after clamp(exp(cond) - 1, 1e-12, 1e6) (the c[] contract of csrc/vihds_models.hpp).  The
functions use + - * / (unary minus, Python numbers) and the operations of this module: exp, log, pow, sigmoid, tanh, clamp
(constant bounds), and the piecewise ones: where(cond, a, b), minimum(a, b), maximum(a, b), abs(x) (Python's abs() too),
sqrt(x), erf(x), erfc(x).  Each of them dispatches on its arguments:
  - symbols (when the class is defined): an expression DAG, from which the model struct of vihds_models.hpp and its
    reverse-mode adjoint are generated as HIP C++ (generate_source);
  - torch tensors: torch ops, eagerly -- the same definition is then a float64 PyTorch right-hand side (torch_problem).
On first use the struct is compiled for gfx950 into the side library vi-hds_amd/lib/libvihds_gen_<tag>.so, registered
with the C ABI (vihds_model_register) and its key added to hip.MODELS: the general training / evaluation path takes it from
there like any built-in key.  Neural precisions wrap the generated struct in WithPrec<> (nothing generated).

The adjoint of each operation is torch autograd's formula, with one exception kept on purpose: the exponent adjoint of
pow(a, n) is g * a^n * log(a) everywhere, as csrc pow_vjp computes it for the built-in models.  At a = 0 that is NaN
(0 * -inf) where autograd masks it to 0 (pow_backward_exponent, base 0 and exponent >= 0); clamp the base away from 0
(as the reference models do: clamp(K, 1e-12, 1) * c) when the exponent is a parameter.

Piecewise terms.  A comparison a < b, a <= b, a > b, a >= b between model quantities and / or Python numbers gives a
CONDITION; conditions combine with & | ~ (not with and / or / not, which are Python control flow and raise, as `if` does) and
select in where(cond, a, b).  A condition is not a number -- arithmetic on one raises; write where(cond, 1.0, 0.0) for an
indicator -- and == / != stay refused.  A Python bool as cond selects when the model is traced.  Conditions may read any leaf
(t in rhs: where(t < p.tau, 0.0, p.dose) is an input switched on at tau; the observations in log_likelihood: a censored
density).  minimum / maximum take two quantities or numbers; a symbolic bound for clamp is minimum(maximum(x, lo), hi).  The
forward semantics are torch's, NaN included: a NaN operand makes every comparison false, minimum / maximum return the NaN (so
a trajectory that has gone NaN stays NaN and the non-finite-loss exit sees it), sqrt of a negative value is NaN.  All of them
are emitted as selects, never as branches.  The adjoints are torch autograd's: where passes the gradient to the branch taken
BY A SELECT (the other branch gets exactly 0, whatever it holds); minimum / maximum pass it to the selected argument, half to
each at a tie; abs: g sign(x), sign(0) = 0; sqrt: g / (2 sqrt(x)), infinite at 0; erf: g 2 / sqrt(pi) exp(-x^2), erfc its
negative.  They are allowed in prepare, rhs (network inputs included), observe, precision and log_likelihood; initial_state
stays affine in theta (a where, minimum, maximum, abs, sqrt of a parameter or treatment there is refused).  Two traps:
  - the double-where idiom.  where(x > 0, log(x), 0) has the right value, but its adjoint forms 0 / x in the branch not
    taken: 0 * inf = NaN at x = 0 (and log's value there may be -inf or NaN, which the select hides only in the forward
    pass).  Make the argument safe with an inner where: where(x > 0, log(where(x > 0, x, 1.0)), 0) -- as with torch.where.
  - a switch time or a threshold gets no gradient through the condition itself: conditions carry no adjoint, so in
    where(t < p.tau, 0.0, p.dose) the gradient reaches dose, never tau (the true derivative with respect to a switch time is
    a jump term no fixed-grid scheme resolves); a parameter that is only ever compared is not learned from the data.

The observation map.  Without `observe` the four signals are one of the kernels' fixed maps of the species by position
(observe_kind: "default" [y0, y0 y1, y0 (y2 + y4), y0 (y3 + y5)], "direct" [y0, y0 y1, y0 y2, y0 y3]).  A model that defines
observe(y, p, c) -> list of 4 has observe_kind "custom": the map is traced into the same DAG (the same operations, no t, no
network calls), sees the species, the effective parameters of prepare and the treatments, and is emitted with its
reverse-mode adjoint as two more members of the struct, called once per time point by the forward and the adjoint kernel.
A parameter may be read by observe only; a treatment it reads is copied by prepare like one rhs reads.  On instances
`observe` stays OdeModel.observe(x_sample, theta) (the definition is kept as the class's map, as `parameters` is kept as
parameter_names); torch_observe evaluates it with torch ops.

The observation noise.  Without `precision` the precisions are what the instance's `precisions` says: four constant theta
entries (ConstantPrecisions: the slots prec_x .. prec_cfp behind the model's own) or the reference's precision ODE
(NeuralPrecisions).  A model that defines precision(y, x, p, c) -> list of 4 owns them: the method is traced into the same DAG
(the operations and limits of observe: no t, no network calls) and sees the species, the four predicted signals x of that time
point (from the model's observe, or from the fixed map of its observe_kind), the effective parameters and the treatments.  It
is emitted with its reverse-mode adjoint as the members precision / precision_vjp, called once per time point; the forward
kernel stores the four values as four rows behind the species in the trajectory (the layout of a NeuralPrecisions model, so
expand_precisions and the evaluation summaries read them unchanged).  Such a model has no prec_* or init_prec_* slots -- its
noise parameters are ordinary entries of `parameters`, which may then be as many as VIHDS_MAX_SLOTS (not VIHDS_MAX_SLOTS - 4)
-- and its `precisions` attribute is a ModelPrecisions the base class creates; assigning another kind raises, and it does not
combine with NeuralPrecisions.  POSITIVITY IS THE AUTHOR'S RESPONSIBILITY: the log-likelihood takes logf of each value, so a
non-positive precision gives NaN exactly as a non-positive constant precision does; no clamp is inserted (write
1 / (s0^2 + (s1 x)^2), exp(.), or clamp(., 1e-6, 1e6) where the expression could reach 0).  torch_precision evaluates the
definition with torch ops.

The observation likelihood.  Without `log_likelihood` the density that joins prediction, observation and precision is the
kernels' Gaussian, -0.5 (log 2 pi - log pr + pr (x - obs)^2) per signal and time point.  A model that defines
log_likelihood(x, obs, pr, p, c) -> list of 4 owns it (likelihood_kind "custom", otherwise "gaussian"): the method is traced
into the same DAG (the operations and limits of observe: no t, no network calls, no species) with two more leaf kinds -- the
four observations of the time point, which are data and get no adjoint, and the four precisions (the constant slots, or the
values of the model's own precision) -- and returns the four per-signal log densities of that time point; the kernel sums
them over time into logp[j].  It is emitted with its reverse-mode adjoint as the members loglik / loglik_vjp (time-loop
helpers; the adjoint adds into the predicted signals', the precisions' and the parameters' adjoints).  The adjoint kernel runs
the three adjoints in the order likelihood, precision, observation map.  A parameter may be read by log_likelihood only (a
mixing weight, a width); a treatment it reads is copied by prepare.  Normalising constants are Python numbers (math.lgamma).
It composes with constant precisions, an own precision, an own observe and networks in rhs, not with NeuralPrecisions; a
subclass returns to the Gaussian with `log_likelihood = None`.
torch_log_likelihood evaluates the definition with torch ops; the host paths that restate the Gaussian (the host-driven
adaptive route, training.log_prob_observations) take it for such a model.  WHAT STAYS GAUSSIAN: everything downstream of
logp is untouched, and the evaluation summaries (iw_variance, iw_predict_std) keep reading the precision rows as inverse
variances.  For a Student-t with nu degrees of freedom and scale 1 / sqrt(pr) the variance is nu / (nu - 2) / pr (nu > 2), so
those two summaries understate the spread by that factor unless the model's precision already carries it.

Forcings.  An input that changes over the experiment and differs from well to well -- a light or inducer schedule, a logged
temperature, the measured OD as a growth driver -- is declared by name and read as an attribute:

        forcings = ["light", "temp"]                 # at most MAX_FORCINGS; identifiers, no species or parameter name

        def rhs(self, t, y, p, c):
            drive = p.aYFP * self.forcing.light      # ... where(self.forcing.light > 0.5, ...), self.net.gate([self.forcing.temp, ...])

Every data row brings one sample per forcing and time point of the observation grid (the batch key "forcings", [rows, K, T]).
In rhs the value at stage time t is the linear interpolant of the row's samples -- on [t_k, t_k+1] that is u_k + (t - t_k)
(u_k+1 - u_k) / (t_k+1 - t_k), continuous, so a stage on a grid point is unambiguous; in observe, precision and log_likelihood
it is exactly the sample u_k of the time point.  Values are used raw (no log1p / exp round trip as the treatments have), a NaN
sample propagates.  A forcing may be a network input and may be compared; reading one in prepare or initial_state raises (they
run once, before the first time point).  It is data, like the observations: a leaf of the DAG with no adjoint -- no gradient
with respect to the samples exists.  The samples travel in the rows of `cond`, behind the treatments: [n_conditions
treatments | K x T samples, forcing-major], so the problem's C is n_conditions + K T (the data's treatment count, where the
data carry more treatments than the model reads: the samples are the last K T entries of a row) and the C ABI has no new field;
OdeModel.row_inputs(data) builds those rows for a batch (data.inputs for every other model) and solve checks the width.  The
encoder does not see forcings.  In the kernels the generated struct keeps 2 K + 1 more entries of p (per forcing a value and a
slope, and the interval's start) that its members set_interval / set_point write from the time loop; rhs reads p[v] + (t -
p[t0]) p[s].  The adaptive solvers integrate on a grid that is not the observation grid: a model with forcings declines them
(solve raises before anything is queued, the library answers VIHDS_E_UNSUPPORTED), as it declines the one-pass summaries.
torch_problem takes the wide cond and `times`, the torch hooks cut the samples from the wide cond.

Implicit models.  A kinetic model with one fast reaction is stiff, and the wide priors draw stiff samples even where the
posterior mean is not: beyond h |lambda| of about 2.8 rk4 blows up on the observation grid, the loss goes non-finite and the
step is skipped.  A class that sets

        implicit = True                              # default False
        newton_iterations = 4                        # 1 .. MAX_NEWTON_ITERATIONS, read by an implicit class only

gets the Jacobian of rhs generated beside its adjoint -- the DAG differentiated row by row with constant one-hot seeds
(jacobian_nodes; vjp itself is unchanged), emitted as the member rhs_jac(t, y, p, wg, J), J[i N + j] = d dy_i / d y_j, with the
forcing reads of rhs, a structural zero as the literal 0.f, and the constants NEWTON and JAC_NZ (the structural pattern: the
elimination leaves out every operation on a structural zero at compile time) -- and takes the solver "beuler" (hip.IMPLICIT_SOLVERS):
backward Euler on the observation grid, y' = y + h f(t1, y'), by exactly NEWTON Newton iterations from y (no convergence test),
each linear solve by Gaussian elimination without a pivot search in registers (a zero pivot gives inf / NaN, which reaches the
non-finite-loss exit like any blow-up); the adjoint is the implicit-function theorem's at the stored y' and needs first
derivatives only.  A step evaluates rhs at t1, where a forcing's interpolant is the sample u_k+1.  What it cannot do: Newton
from y solves the step of a GROWING mode only while h times its rate stays well below 1 (I - h J is singular at 1) -- backward
Euler is for fast DECAY; too few iterations leave a step that is not the converged one, and the adjoint is then not the
gradient of what was computed (FastBinding of the tests needs 6).  It composes with observe, precision, log_likelihood, piecewise
terms and forcings.  Refused in this version: together with networks (the Jacobian of a network with respect to its inputs is
not generated), with NeuralPrecisions (the precision ODE has no Jacobian), with more than MAX_IMPLICIT_STATES = 8 species
(the matrix lives in registers).  Any other model given "beuler" raises before anything is queued; the implicit model keeps
every explicit solver.  A class without `implicit` generates byte for byte the text it generated before.  torch_jacobian
evaluates the same DAG nodes with torch ops, to check the generator against autograd.

Backward Euler is first order: `substeps` buys accuracy linearly.  An implicit class that also sets

        implicit_order = 2                           # the int 1 (default) or 2; 2 needs implicit = True

runs Alexander's two-stage SDIRK under the same solver name -- "beuler" is the implicit scheme of the model; there is no new
solver id, hip.GENERATED_IMPLICIT_ORDER[key] tells which scheme a registered model runs.  It is order 2, L-stable and stiffly
accurate (stability function (1 + (1 - 2 gamma) z) / (1 - gamma z)^2).  With gamma the float nearest 1 - sqrt(2)/2, c the
float nearest 1 + sqrt(2), h = t1 - t0, a = gamma * h and tg = fmaf(gamma, h, t0), in float32: stage 1 starts at z = y_k and
runs NEWTON times  F = z - y_k - a f(tg, z), A = I - a J(tg, z), solve A d = -F, z += d  to z1; the base of stage 2 is
w = fmaf(c, z1 - y_k, y_k), which is y_k + (1 - gamma) h f(tg, z1) without another evaluation of a stiff f; stage 2 starts at
z = z1 and runs NEWTON times  F = z - w - a f(t1, z), A = I - a J(t1, z), solve A d = -F, z += d  to y_k+1.
newton_iterations is the count per stage; no convergence test, as above.  A forcing is read at tg and at t1 from the
interval's interpolant.  The adjoint is the converged step's, first derivatives only: z1 is recomputed by the forward's
stage-1 call (registers, no LDS), A2 = I - a J(t1, y_k+1), A2^T mu2 = lambda;  A1 = I - a J(tg, z1), A1^T mu1 = c mu2;  the
parameter adjoint gains (a mu2)^T df/dp at (t1, y_k+1) and (a mu1)^T df/dp at (tg, z1);  lambda <- (1 - c) mu2 + mu1.  The
stage matrix is I - gamma h J: Newton from y_k on a growing mode reaches steps about 3.4 times longer than backward Euler's.
The order combines with everything `implicit` combines with (forcings, substeps, jump, start, lead_in, the hooks), whose
definitions are written over the one-step map; what `implicit` refuses stays refused.  The generated struct gains the one
line IMPLICIT_ORDER = 2 (none at order 1: such a class generates byte for byte the text it generated before).

Sub-steps.  The observation grid is the plate reader's, not the model's: a fixed-grid solver takes one step per interval of it.
A class that sets

        substeps = 4                                 # 1 .. MAX_SUBSTEPS = 8, an int; default 1

has every fixed-grid solver (modeuler, modeulerwhile, euler, midpoint, rk4, beuler) take that many steps of its own scheme
over each observation interval [t_k, t_k+1]: with hs = (t_k+1 - t_k) * (1.f / m), sub-step j runs from s_j to s_j+1, where
s_j = fmaf((float)j, hs, t_k) for j < m and s_m = t_k+1 exactly; modeuler's fixed step h0 becomes h0 * (1.f / m); beuler starts
each sub-step's Newton iteration from the previous sub-state, so a growing mode needs h * rate / m well below 1, not h * rate.
Only the states at the observation points are stored, observed and scored: traj, x_predict and logp keep their shapes, and the
float64 meaning is exactly the m = 1 scheme on the refined grid read at every m-th point.  A forcing's set_interval stays one
call per observation interval: a sub-step reads the linear interpolant of the samples inside it.  The generated struct gains the
one line SUBSTEPS = m (none at m = 1: such a class generates byte for byte the text it generated before); the kernels' time
loops run a rolled loop of m steps, and the adjoint, which finds only y_k stored, recomputes the interval's m - 1 intermediate
states into LDS ((m - 1) * species rows of 256 floats per block, at most MAX_SUBSTEP_ROWS = 56) before it runs the m step
adjoints last to first.  Such a model takes the fixed-grid solvers only: an adaptive solver chooses its own steps and is
declined (solve raises before anything is queued, the library answers VIHDS_E_UNSUPPORTED).  Refused in this version: together
with networks and with NeuralPrecisions (the adjoint's dump holds one evaluation per stage and observation interval).

Error-controlled sub-steps.  One `substeps` for every trajectory and every interval is paid for on every quiet interval and says
nothing where it was too small.  A class that also sets

        substeps = 8                                 # now the ceiling of the ladder: 2, 4 or 8
        step_tolerance = (1e-3, 1e-6)                # (rtol, atol) on the species: finite floats >= 0, not both 0

has every trajectory pick its own number of steps for every observation interval by step doubling (csrc/vihds_stepctl.hpp has the
rule, exactly): with Phi^c the c steps of the scheme from y_k on the sub-grid of c steps, coarse = Phi^1, then fine = Phi^2c and
r = max over the species of |fine - coarse| / (atol + rtol max(|fine|, |coarse|)); r <= 1 accepts fine with count 2c, otherwise
c doubles, and at 2c = substeps fine is taken all the same and the interval counts as saturated.  A NaN or infinite r fails the
test.  Only species enter r (algebraic unknowns and precision rows do not); jump applies to the accepted state afterwards, the
steps of a lead-in phase are not controlled, and beuler starts each sub-step's Newton iteration from the previous sub-state as
under `substeps`.  The choice is made in registers, with no barrier and no atomics; passing at the first test costs three steps
for a count of 2.  The solution gains one row per time point, the last one (behind the four precision rows of a model with a
precision map of its own): at point k + 1 the count of the interval that ended there as a float, +count where the test passed
and -substeps where the ladder was exhausted, 0 at point 0.  substep_counts(traj, model) reads it back as (counts int32
[T-1, B, S], saturated bool [T-1, B, S]); `saturated` means the tolerance was NOT met there.  expand_precisions and the
evaluation summaries leave the row out.  The adjoint reads the row from the stored trajectory (clamped into 1 .. substeps before
it bounds a loop or indexes LDS), never repeats the ladder, and runs the interval adjoint of `substeps` at that count: it is the
exact discrete adjoint of the realised scheme, and a count carries no gradient, as a `where` condition carries none.  The struct
gains STEP_RTOL and STEP_ATOL beside SUBSTEPS (a class without the attribute generates the text it generated before).  In float32
a relative tolerance much below 1e-5 measures rounding, not truncation error.  Solvers: euler, midpoint, rk4 and beuler (either
implicit_order); modeuler and modeulerwhile, whose fixed step h0 is not the interval, and the adaptive solvers are declined
before anything is built or queued.  Combines with forcings, jump, start / lead_in, algebraic, missing_observations and the three
observation hooks; refused in this version: networks, NeuralPrecisions, delays, diffusion.

State jumps.  A discontinuity of the state at an observation point -- a culture diluted at a read, a bolus pipetted into a
well, a turbidostat that dilutes above a threshold, a dose -- is neither a term of rhs nor a forcing (both change the
derivative, not the state).  A class may define

        def jump(self, y, p, c):                     # -> list of len(species): the state right after the time point
            keep = self.forcing.keep                 # per well, per time point; 1.0 where nothing happens
            return [y[0] * keep, y[1] * keep + p.bolus * self.forcing.dose, ...]

With Phi the chosen fixed-grid scheme over one observation interval (sub-steps included): y_0 is the initial state; for k = 0 ..
T-1 the state y_k is stored, observed and scored (traj, x_predict and logp hold the LEFT limit at t_k), and for k < T-1 the next
interval starts from the jump, y_k+1 = Phi(t_k, t_k+1, jump(y_k; p, c, u_k)), u_k the forcing samples of the point as the other
hooks read them.  A jump at the last point has no effect and is not evaluated.  The hook has no t: an event schedule travels as
a forcing (which may differ from well to well), a state-triggered event is a where on y -- its condition carries no adjoint, as
for every where: there is no gradient with respect to an event time or a trigger threshold.  Like log_likelihood it takes
exactly its arguments, `jump = None` in a subclass removes it, and a treatment it reads becomes one more effective parameter.
The struct gains OWN_JUMP, jump(y, p, yj) and jump_vjp(y, p, yjb, yb, pb) (reverse mode, forward values recomputed, it adds);
the forward kernel calls jump last in a time point's iteration, the adjoint recomputes it from the stored left limit, runs the
step adjoint from there and chains jump_vjp into the trajectory adjoint ahead of the point's hook adjoints.  modeuler's fixed
h0 and the sub-step grid are untouched.  Networks in rhs, forcings, implicit, substeps and the other hooks all combine with it.
Such a model takes the fixed-grid solvers only (an adaptive solver is declined: solve raises before anything is queued, the
library answers VIHDS_E_UNSUPPORTED) and no NeuralPrecisions (generate_source(cls, neural=True) raises).  A class without the hook
generates byte for byte the text it generated before.  torch_jump restates the hook with torch ops.

Where the trajectory starts.  initial_state stays affine in theta (init_vjp sees no theta) and the time loop begins at the first
read.  Two optional attributes lift both limits:

        def start(self, y, p, c):                    # -> list of len(species): the state the integration starts from
            rfp0 = p.rc / (p.drfp + p.r)             # y is what initial_state returned; p, c as in jump; self.forcing.<name>
            return [y[0], where(c[0] > 0.5, rfp0, y[1]), ...]              # reads the first sample u_0
        lead_in = 6.0                                # L > 0, in the units of `times`: an unscored phase before t_0
        lead_in_steps = 4                            # n, 1 .. MAX_LEAD_IN_STEPS = 8, an int; default 1

y_start = start(initial_state(th, c); p, c, u_0); with no lead-in y_0 = y_start.  start has the rules of jump (all operations of
the model language, no t, no network call, exactly its arguments, `start = None` in a subclass removes it, a treatment it reads
becomes one more effective parameter, a parameter may be read by it alone).  With a lead-in, tl = t_0 - L (formed in float32),
hl = (t_0 - tl) * (1.f / n), s_j = fmaf(j, hl, tl) for j < n and s_n = t_0 exactly (lead_in_times returns them); u_0 = y_start,
u_j+1 = Phi(s_j, s_j+1, u_j) with Phi one step of the chosen fixed-grid scheme, y_0 = u_n.  Nothing of the lead-in is stored,
observed or scored: traj[0], x_predict[0] and logp begin at y_0.  rhs sees the true t < t_0 there -- where(t < 0.0, 0.0, c[0]) is
an inducer absent before the first read --, a forcing holds its first sample, modeuler's fixed step is hl, beuler starts each
step's Newton iteration from u_j, substeps do not divide these steps and jump is not applied.  The struct gains OWN_START, start
and start_vjp, LEAD_STEPS and LEAD_TIME; the adjoint kernel, after its time loop, recomputes init, start and the lead-in's
intermediate states (into the LDS rows of the sub-steps: (n - 1) * species at most MAX_SUBSTEP_ROWS), runs the n step adjoints
last to first, then start_vjp ahead of prepare_vjp, and hands the state part to the unchanged init_vjp.  Fixed-grid solvers only
(an adaptive solver is declined: solve raises before anything is queued, the library answers VIHDS_E_UNSUPPORTED), no
NeuralPrecisions; a lead-in takes no networks (the dump is sized (T-1) x stages), start combines with networks in rhs.  A class
with neither generates byte for byte the text it generated before.  torch_start restates the hook with torch ops.

Pre-equilibration.  Cells are pre-cultured until the circuit has relaxed, and only then induced and read: the right initial state
is a steady state of the model itself under the pre-culture conditions, a function of the parameters being inferred.  start
covers it where the steady state has a closed form; a toggle switch, a repressilator, a cascade with Hill repression have none:

        steady_species = ["U", "V"]                  # 1 .. MAX_STEADY = 8 names out of `species`
        steady_steps = 12                            # an int, 1 .. MAX_STEADY_STEPS = 16: a fixed count
        steady_first_step = 0.1                      # the pseudo-time step delta_0 > 0, in the units of `times`
        steady_growth = 4.0                          # delta_k+1 = delta_k * steady_growth, at least 1
        def steady_rate(self, y, p, c):              # -> one residual per steady species: their d/dt in the pre-culture
            f = self.rhs(0.0, y, p, [0.0] * len(c))  # e.g. the model's own rhs with the inducers absent
            return [f[1], f[2]]

steady_rate has the rules of start (no t, no network call, self.forcing.<name> is the first sample u_0, a treatment it reads
becomes one more effective parameter, a parameter may be read by it alone); y is the full state, and the species not named are
inputs held fixed (the cell density grows and is at no steady state).  A self.rhs(...) it calls is traced as part of it: where
that rhs calls a network or reads self.algebraic / self.delayed the read raises and names steady_rate.  The value, exactly: from
y_s = start(initial_state(...)) (initial_state(...) without a start), with E the steady species, F = steady_rate, J = dF/dy_E
(generated from the DAG like rhs_jac, its structural pattern STEADY_NZ known at compile time) and delta_0 = steady_first_step,
for k = 0 .. steady_steps - 1: solve (I - delta_k J(y)) d = delta_k F(y), y_E += d, delta_k+1 = delta_k * steady_growth in
float32.  Each iteration is one Newton iteration of a backward-Euler step in pseudo-time (pseudo-transient continuation): the
early ones follow the flow from the guess, so a bistable model lands in the basin its guess is in; the late ones are Newton's
method up to 1 / delta_k.  No convergence test, no data-dependent branch.  The order is initial_state, start, the solve, the
lead-in, the scored time loop; nothing of the solve is stored or scored, traj[0] is what follows it (or the lead-in), and a
delayed read's history before t_0 is that stored y_0.  The adjoint is the implicit-function theorem's at the final state y*: with
lam the adjoint of y*, solve J(y*)^T mu = lam_E (J itself, not I - delta J), add steady_rate's vector-Jacobian product seeded
with -mu into the adjoint of the other species and of p, set lam_E = 0.  Nothing is differentiated through the iteration, so
the guess of a steady species receives exactly 0 gradient: an init_* parameter that only feeds such a guess is learned from its
prior alone (INTEGRATION.md lists this trap).  Too few steps leave a y* that is no root, and the adjoint is then not the gradient
of what was computed: choose the count on torch_steady(y, theta, cond, forcing=None, return_residual=True), which runs the same
iteration in y's dtype, carries the implicit-function gradient through a custom autograd function and also returns the last
increment relative to |y_E| and |F(y*)|.  torch_problem's x0 includes the solve; torch_steady_jacobian evaluates the generated J
from the same DAG nodes.  The solves eliminate without a pivot search (csrc/vihds_steady.hpp): residual i must depend on steady
species i; a zero column or row of J and a structurally zero pivot after fill-in are refused when the class is defined.  The
struct gains N_STEADY, STEADY_STEPS, STEADY_DELTA0, STEADY_GROWTH, STEADY_NZ, steady_species(e), steady_rate, steady_jac,
steady_rate_vjp, steady and steady_vjp.  It combines with start, lead_in, forcings, an own observe / precision / log_likelihood,
piecewise terms, substeps, step_tolerance, jump, missing_observations, implicit (both orders), delays, diffusion / noise_channels
and networks in rhs.  Refused in this version: together with `algebraic`, with NeuralPrecisions, more than MAX_STEADY names.
Fixed-grid solvers only, as for start (an adaptive solver is declined: solve and ops.OdeProblemSpec raise before anything is
queued, the library answers VIHDS_E_UNSUPPORTED).  `steady_species = None` (or []) in a subclass removes it; a class without it
generates byte for byte the text it generated before.

Algebraic variables.  A fast reaction held at its equilibrium -- binding and unbinding of a repressor, an inducer, a dimer, orders
of magnitude faster than expression and dilution -- is the reduction modellers reach for before a stiff solver: the TOTALS stay
ODE states and the complex is defined by a constraint g(y, z, p) = 0 (quasi-steady state, rapid equilibrium).  A class declares

        algebraic = ["C"]                            # 1 .. MAX_ALGEBRAIC = 4 unknowns z; identifiers of their own
        algebraic_iterations = 6                     # 1 .. MAX_NEWTON_ITERATIONS, an int: a fixed Newton count
        def algebraic_start(self, y, p, c):          # -> the iteration's starting value, one entry per unknown
            return [y[0] * y[1] / (y[0] + y[1] + p.Kd)]
        def constraint(self, y, z, p, c):            # -> one residual per unknown; z solves constraint(...) == 0
            return [(y[0] - z[0]) * (y[1] - z[0]) - p.Kd * z[0]]

and reads self.algebraic.C in rhs and in observe (reading it in prepare, initial_state, start, precision, log_likelihood or jump
raises and says so).  constraint and algebraic_start have no t and call no network; they read the species, the effective
parameters, the treatments and the forcings -- in rhs a forcing is the interpolant at the stage time, in observe the sample of
the time point.  The value, exactly: z = algebraic_start(y, p); algebraic_iterations times G = g(y, z, p), A = dg/dz (y, z, p),
solve A d = -G, z += d; then rhs / observe are evaluated with that z.  No convergence test, no data-dependent branch; the solve
is Gaussian elimination without a pivot search on the structural pattern of dg/dz (ALG_NZ; csrc/vihds_algebraic.hpp), so
residual i must depend on unknown i (a structurally zero pivot, column or row is refused when the class is defined; a pivot
that vanishes numerically gives inf / NaN, which reaches the non-finite-loss exit).  The adjoint repeats the value pass (the
same bits), takes the adjoint zb of z from reverse mode over rhs / observe, solves A^T mu = zb with A at the final z and
subtracts (dg/dy)^T mu from the state adjoint and (dg/dp)^T mu from the parameter adjoint -- one vjp of the constraint seeded
with -mu.  That is the implicit-function derivative of the CONVERGED solution: nothing is differentiated through the iteration
or through algebraic_start, so too few iterations (or a start near a double root, where Newton converges slowly) leave an
adjoint that is not the gradient of what was computed.  A treatment or forcing read by the constraint has no adjoint.  The
closure lives inside the struct's rhs / rhs_vjp and observe / observe_vjp (the members algebraic_start, constraint,
constraint_jac, constraint_vjp, algebraic, algebraic_vjp and the constants N_ALGEBRAIC, ALG_ITER, ALG_NZ): every explicit
solver runs such a model with unchanged kernels, and substeps, jump, start, lead_in, forcings, an own precision and an own
log_likelihood combine with it.  Refused in this version: together with implicit = True (the reduced Jacobian f_y - f_z
g_z^-1 g_y is not generated), with networks, with NeuralPrecisions, more than MAX_ALGEBRAIC unknowns.  A class without
`algebraic` generates byte for byte the text it generated before.  torch_algebraic(y, theta, cond) returns z by the same
iteration with torch ops (autograd Jacobians, a pivoted solve); it keeps the iterate's value and carries the implicit-function
gradient, and torch_problem's right-hand side and torch_observe use it, so autograd through the host paths stays correct;
torch_constraint_jacobian evaluates the generated dg/dz, to check the generator against autograd.

Delayed reads.  A right-hand side may read a species at an earlier time, y_i(t - tau) -- transcription, translation and
maturation lags, delayed negative feedback, a signal relay -- with the delay an effective parameter like any other:

        delays = {"Rlag": ("R", "tau")}              # name -> (species, key of what prepare returns); at most MAX_DELAYS

        def rhs(self, t, y, p, c):
            production = p.beta / (1.0 + (self.delayed.Rlag / p.K) ** 2)     # R at t - p.tau

self.delayed.Rlag is readable in rhs only (arithmetic, where conditions; a read in prepare, initial_state, start or a hook
raises and names the place).  The delay is in the units of `times`; being a key of prepare's dict it may be clamped, scaled or
shared, and its gradient reaches theta through prepare_vjp.  The value, defined per observation interval k = [t_k, t_k+1] with
taue = fmaxf(tau, 0.f) (csrc/vihds_delay.hpp): s_lo = t_k - taue and s_hi = fminf(t_k+1 - taue, t_k) -- the history is known up
to the start of the step only --; H(s) is the stored state at t_0 (after start, where the class has one) for s <= t_0, a constant
history, and otherwise the linear interpolant fmaf(w, y_j+1 - y_j, y_j) of the float32 states stored at the observation points,
j the largest index of [0, k-1] with t_j <= s; every stage of the step reads the chord from H(s_lo) to H(s_hi).  The struct
reserves 2 E + 1 more entries of p behind the forcings' (values, slopes, the interval start) that its member set_delay writes from
the time loop; rhs reads p[v] + (t - p[t0]) p[s] as it reads a forcing, and -- the difference -- rhs_vjp adds the read's adjoint
to pb[v] and pb[s].  The adjoint kernel repeats the lookups, scatters those adjoints back to the earlier time points with the
interpolation weights (a per-trajectory history adjoint in its aux buffer, no atomics, the same bits run to run) and adds
-(y_j+1 - y_j) / (t_j+1 - t_j) times each to the adjoint of tau where the lookup moves with it.  Consequences: the interpolant
is linear, so a scheme's order is capped at 2; for taue below the step the read lags by up to h - taue -- the term is then
treated like explicit Euler (sub-steps would be the remedy and are not combined yet); at s on a grid point, and at taue equal to
a step, the gradient with respect to tau jumps.  A delay that is not finite makes the read NaN.  Combines with start, forcings,
piecewise terms and the hooks; declined in this version: implicit = True, substeps > 1, lead_in, jump, networks, algebraic,
NeuralPrecisions, the adaptive solvers (solve raises before anything is queued) and the one-pass summaries.  torch_problem's rhs
takes the values as rhs(t, state, delayed=[...]) and lists (species index, delay) per read as rhs.delays; the integration loop
that looks them up is the caller's (tests/modelgen_delay_models.py has the float64 definition).

Process noise.  Well-to-well scatter that enters the state and is propagated by the dynamics -- intrinsic fluctuations of
expression and growth -- is neither observation noise nor a parameter: the model is dX = f dt + g dW.  A class may define

        def diffusion(self, y, p, c):                # -> one amplitude per species, like rhs; 0.0 for a species without noise
            return [p.sigma * sqrt(maximum(y.X, 0.0)), 0.0, ...]

Diagonal Ito noise: one independent Wiener process per species.  For every step the scheme takes -- every sub-step when
substeps > 1 -- from the state u over a step of length h,  u' = Phi_h(u) + g(u, p) * (sqrt(h) * xi),  Phi the unchanged step of
the chosen fixed-grid solver, g evaluated at the step's START state, xi ~ N(0,1) per species, h the length the scheme itself
advances by (modeuler: its fixed step, as the step uses it; every other solver: t1 - t0).  This is Euler-Maruyama for euler;
for the other schemes it is a drift / noise splitting of the same strong order 1/2 (the drift's higher order buys nothing
pathwise).  The noise path is sampled from its prior: it is not a variational parameter, so the IWAE bound gains no term -- the
bound averages over the path as it does over theta's samples.  The hook has no t and is read-only; a forcing reads the sample
of the interval's first point, as in jump.  The struct gains HAS_DIFFUSION, NOISE_MASK, diffusion(y, p, g) and
diffusion_vjp(y, p, gb, yb, pb) (reverse mode, forward values recomputed, it adds); a species whose amplitude folds to the
constant 0 draws nothing and has no adjoint.  The draws are stored nowhere (csrc/vihds_sde.hpp): xi of species q at step
k * substeps + j of trajectory b * S + s is normal q & 3 of the Philox4x32-10 block at the counter (b * S + s, q >> 2,
k * substeps + j, a non-zero tag -- the theta stream has 0 there), keyed by two 24-bit words per data row that travel as the
last two floats of the row of cond: [n_conditions | K x T | key lo, key hi].  The adjoint regenerates each draw from its
counter (gb = lam' sqrt(h) xi, diffusion_vjp, the scheme's step adjoint, lam += yb): no atomics, gradients repeat bit for bit.
row_inputs appends the key columns and cond_width counts them.  A batch may carry 'noise_key' (one pair of ints or [rows, 2],
each in [0, 2^24), checked on the host); without it the model keeps a two-word state on the device, seeded from the class
attribute noise_seed: in training mode row_inputs reads it and advances it in place (a captured step draws afresh on every
replay; the counter wraps at 2^24 into the second word), in evaluation mode the key is the seed's, so evaluations repeat.
The state is the buffer noise_key_state: it is saved in state_dict (a resumed run continues the stream), moved by Module.to, and
moved as it stands -- never seeded again -- when a batch arrives on another device.  The hook's record, DIFFUSION_HOOK, stands
beside HOOKS and ALL_HOOKS rather than inside HOOKS: those two tuples are pinned by earlier tests as the per-time-point hooks and
the start map, and this hook is called per step of the scheme; TRACED_HOOKS = ALL_HOOKS + (DIFFUSION_HOOK,) is what tracing, code
generation and the capture of the definitions walk.
One trap: the derivative of sqrt is infinite at 0, so a species with the amplitude sigma * sqrt(maximum(y, 0.0)) that starts at
0 (or is driven there) has a gradient that is not finite, and the training step skips its update; start it above 0 or put a
floor under the root, sqrt(maximum(y, 0.0) + eps).
Combines with forcings, substeps, jump, start, the three observation hooks and the piecewise operations.  Refused at class
definition, each with its reason: implicit = True, networks, NeuralPrecisions, algebraic, delays, lead_in > 0, a wrong arity
(there is no t to read) or a wrong number of returned values.  Such a model takes the fixed-grid solvers only (solve and
ops.OdeProblemSpec raise NotImplementedError before anything is built or queued; the library answers VIHDS_E_UNSUPPORTED).
Open: Milstein or Stratonovich schemes, drift-implicit steps, the refused combinations, S sharded over ranks (the trajectory
index is the launch's), noise in the lead-in; non-diagonal noise is built as channels (next paragraph), a dense correlated
matrix beyond them is not.  torch_diffusion restates the hook with torch ops; tests/modelgen_sde_models.py has the float64
definition of the scheme, which takes the draws as an argument.

Noise channels.  The intrinsic noise of a reaction network is not diagonal: in the chemical Langevin equation every REACTION has
a Wiener process of its own, which enters every species the reaction touches through the stoichiometry,
dX = sum_r nu_r a_r(X) dt + sum_r nu_r sqrt(a_r(X)) dW_r.  A conversion A -> B moves A down and B up by the same increment (the
total is conserved); a species that is produced and degraded has two channels whose variances add; mRNA and protein, immature and
matured fluorophore are correlated.  In place of diffusion a class may declare

        noise_channels = ["tx", "deg", "mature"]     # 1 .. MAX_NOISE_CHANNELS = 8 identifiers, names of their own
        def channel_noise(self, y, p, c):            # -> one list per channel, each with one amplitude per species
            a_tx = sqrt(maximum(p.k * y.M, 0.0))
            return [[a_tx, 0.0, ...], [-a_deg, 0.0, ...], [0.0, -a_m, a_m, ...]]

Entry [r][q] is G[q][r], the amplitude with which channel r enters species q.  The hook has the rules of diffusion: no t, exactly
its arguments, every operation of the model language (the piecewise ones included), self.forcing.<name> reads the sample of the
interval's first point, channel_noise = None in a subclass removes it (and the inherited names), a treatment it reads becomes
one more effective parameter.  An entry that folds to the constant 0 is a structural zero: it draws nothing, costs nothing and
has no adjoint.  The scheme, exactly: for every step the fixed-grid scheme takes (every sub-step when substeps > 1) from the
state u over the length h of the diagonal scheme,  dw[r] = sqrtf(h) * xi_r;  u' = Phi_h(u);  then for r = 0 .. R-1 ascending
and every species q of channel r's pattern, ascending,  u'[q] = fmaf(G[q][r], dw[r], u'[q]),  G evaluated at the step's start
state.  xi_r is normal r & 3 of the Philox block at the counter (b * S + s, r >> 2, k * substeps + j, the stream's tag) under the
row's key: the layout of the diagonal hook with the channel index where the species index stood -- the tag, the key columns,
noise_key, noise_seed and noise_key_state are the same, and a class with one channel per species and the diagonal amplitudes
repeats its diffusion twin bit for bit.  The adjoint regenerates dw, seeds Gb[q][r] = lam'[q] * dw[r] on the pattern, runs
channel_noise_vjp (reverse mode, forward values recomputed, it adds), the scheme's own step adjoint on lam, then lam += yb: no
atomics, nothing stored, gradients repeat bit for bit.  The struct gains HAS_DIFFUSION (so everything that asks for a noisy model
-- the key, the width of cond, the declined solvers -- holds unchanged), NOISE_CHANNELS, NOISE_ENTRIES, channel_species(r) (bit
q: channel r enters species q), channel_noise(y, p, G) and channel_noise_vjp(y, p, Gb, yb, pb), G the flat array
G[q * R + r]; the kernels' trait is noise_channels<M> (csrc/vihds_sde.hpp).  On instances has_diffusion is true and
n_noise_channels is R (0 for every other model).
Written once: langevin(stoichiometry, propensities, floor=0.0) returns the columns nu_r[q] * sqrt(maximum(a_r, 0.0) + floor)
for channel_noise and langevin_drift(stoichiometry, propensities) the sums sum_r nu_r[q] * a_r for rhs; stoichiometry[r][q] is an
integer, and a 0 is a structural zero.  Both are plain Python over this module's operations (symbols, tensors and numbers alike).
The trap of the diagonal hook holds here too: the derivative of sqrt is infinite at 0, so a propensity that starts at 0 or is
driven there gives a gradient that is not finite and the training step skips its update -- give langevin a floor > 0, or start
the species above 0.
Refused at class definition, each with its reason: channel_noise together with diffusion; noise_channels without the hook or
the hook without noise_channels; a wrong arity; a wrong number of channels or of entries per channel; a channel that enters no
species; a name that is also a species, a parameter, a forcing, an algebraic variable or a delay; more than MAX_NOISE_CHANNELS
channels; more than MAX_NOISE_ENTRIES = 32 entries that are not structurally zero (each is a register held across the scheme's
step: eight channels into four species, which compiles without scratch); what diffusion refuses, for its reasons (implicit =
True, networks, NeuralPrecisions, algebraic, delays, lead_in > 0); and step_tolerance (two noisy trial solutions differ by the
noise).  It combines with what diffusion combines with: forcings, substeps, jump, start, the three observation hooks,
missing_observations and the piecewise operations; the fixed-grid solvers only, declined as for diffusion.  The hook's record,
CHANNEL_NOISE_HOOK, stands beside the pinned tuples: MODEL_HOOKS = TRACED_HOOKS + (CHANNEL_NOISE_HOOK,) is what tracing, code
generation and the capture of the definitions walk.  torch_channel_noise restates the hook with torch ops ([B,S,N,R,T]);
tests/modelgen_channel_models.py has the float64 definition, which takes the draws as an argument.
Open: more than 8 channels (a dense correlated matrix over many species), tau-leaping (Poisson increments in place of normal
ones), Milstein or Stratonovich schemes (the channels do not commute: Levy areas), drift-implicit steps, S sharded over ranks,
noise in the lead-in.

Missing observations.  Plate-reader data has dropped and saturated reads, plates of different duration and channels that a plate
does not record; the kernels' data contract is otherwise a complete rectangle of finite reads.  A class may set

        missing_observations = True                  # a bool; default False

and a batch may then carry 'observed', [rows, 4, T] of 0 / 1 as bool or float, 1 where the read exists (anything else raises on
the host: observed_mask checks shape and values wherever the data is still there -- training.batch_to_device does before it
uploads; a tensor that is on a device already is taken as it is, reading it back would stall the queue).  Without the key every
point counts as observed.  Defined exactly, at time point k and signal j with m = observed[j][k] and x the predicted signal:
ob' = m ? obs[j][k] : x[j] -- the predicted signal stands in for the placeholder, the residual-0 point of any density, so what
stands under the mask (NaN, inf, a saturated value) never enters the arithmetic --, the signal's term is formed from ob' (the
constant-precision Gaussian, the Gaussian of NeuralPrecisions or of an own precision with its log pr part, the model's own
log_likelihood), and logp[j] += m ? term : 0.  The adjoint seeds the point with m ? g_logp[j] : 0 and forms its residuals from
ob'; what arrives for x_predict and the trajectory is not masked, and the in-kernel importance weight is formed as before.
Everything is a select: nothing is multiplied by 0 and no branch depends on the data.  The trajectory, x_predict and the
precision rows are stored at every point as before.  The struct gains one line, MASKED_OBS = true (vihds_models.hpp:
masked_obs<M>, false for every hand-written model; WithPrec<> forwards its core's value, so NeuralPrecisions takes such a
model); a class without the attribute generates byte for byte the text it generated before.  The mask travels in the rows of
cond like the forcings and the noise key: [n_conditions treatments | K x T forcing samples | T mask words | key lo, key hi],
mask word k of a row the float sum_j observed[j][k] * 2^j -- an integer 0 .. 15, exact in float32, one float per time point
(mask_words; csrc/vihds_mask.hpp decodes it and holds the selects, __host__ __device__).  row_inputs builds the words and
cond_width counts them; solve checks the width before anything is queued; OdeArgs and the C ABI get no field.  The staged forward
keeps the words in LDS beside the observations, the unstaged forward and the adjoint fetch them one point ahead.  The mask is
read at the scoring point only, so it combines with every other feature of this module.  Refused: the adaptive solvers (solve and
ops.OdeProblemSpec raise NotImplementedError before anything is built or queued, the library answers VIHDS_E_UNSUPPORTED -- the
words live on the observation grid, as forcing samples do); a batch with 'observed' that reaches any other model raises in
row_inputs (a look at the batch's keys, nothing is read back).  The host paths that restate the likelihood take the mask with
the same selects: training.log_prob_observations(..., observed=), torch_log_likelihood(..., observed=), masked_terms.  The encoder
is not told about the mask and must never see a NaN: a dataset with missing entries stores datasets.fill_unobserved(times,
observations, observed) -- linear interpolation in time between observed neighbours, the nearest observed value before the first
and after the last, 0 for a signal without any -- as 'observations' and the mask as 'observed'; datasets.load_csv reads a blank or
'nan' cell as unobserved, and the spec's data block takes merge: union (with merge_tolerance), the sorted union of the files'
time points with each file observed at its own, where the default resamples every file onto the shortest one's grid.
Open: masks for the built-in models' kernels (the time-parallel decoder, the lane kernels, dr_blackbox).
An encoder that reads the mask.  Per-row time grids without a union grid.
Skipping integration steps for rows whose remaining points are all unobserved.  Adaptive solvers for masked models.
tests/modelgen_missing_models.py has the float64 definition.

Learned terms.  A model may declare small networks and call each of them (at most once) inside rhs:

        networks = {"latent": Network(n_inputs=5, n_hidden=8, n_outputs=4, hidden="relu")}     # hidden: "relu" | "tanh"

        def rhs(self, t, y, p, c):
            o = self.net.latent([y[4], y[5], y[0], p.a, c[0]])      # list of n_outputs values, LINEAR output layer

A network is Linear(n_inputs, n_hidden) -> activation -> Linear(n_hidden, n_outputs) with biases; heads and gates are
composed from the operations above (the reference's NeuralStates, vihds/ode.py:119-138, is sigmoid(o[j]) - sigmoid(o[k]) * z).
Its weights are nn.Parameters of the model instance (nets.<name>.hidden / .out); neural_weights() is one flat buffer: all
networks in declaration order, each W1 [H][I], b1 [H], W2 [O][H], b2 [O], then the NeuralPrecisions weights when the model
uses them.  The generated struct then has NW > 0: the forward MLP and its adjoint are emitted into it, weights are read as
scalars through the constant address space, and the weight gradient comes from a field-major dump of the adjoint kernel
(per evaluation and network: inputs [I], hidden pre-activation adjoints [H], hidden activations [H], output adjoints [O])
contracted by vihds_gram_blocks -- fixed summation order, no atomics (ops.decoder_weight_grads).
"""
import hashlib
import inspect
import math
import operator
import os
import sys

import numpy as np
import torch

from vihds import hip
from vihds.ode import OdeModel

MAX_STATES = 32  # ODE states of a generated model (all of them live in registers of one thread)
OBSERVE_KINDS = {"default": ("OBS_DEFAULT", 6), "direct": ("OBS_DIRECT", 4)}  # kernel enum, species observe() reads
OBSERVE_CUSTOM = "custom"  # observe_kind of a class that defines observe(y, p, c): the struct's own map, OBS_CUSTOM
# networks of a generated model (the hidden layer is walked one unit at a time, the inputs and outputs live in registers)
MAX_NETWORKS, MAX_NET_INPUTS, MAX_NET_HIDDEN, MAX_NET_OUTPUTS = 2, 16, 32, 8
MAX_DELAYS = 4  # delayed reads of a generated model (each costs the kernels two lookups per interval and three registers)
MAX_FORCINGS = 4  # time-varying inputs of a generated model (each costs the kernels two registers and a sample in flight)
NET_ACTIVATIONS = ("relu", "tanh")
# species of a model with `implicit = True`: the N x N matrix of a Newton step lives in registers beside the states, and its
# structural pattern is one 64-bit constant.  Eight is what compiles without scratch when every species is in every
# derivative (tests/test_modelgen_implicit_host.py builds that worst case)
MAX_IMPLICIT_STATES = 8
MAX_NEWTON_ITERATIONS = 8
# steps of a fixed-grid scheme per observation interval (`substeps`).  The adjoint keeps the interval's intermediate states in
# LDS, (substeps - 1) * species rows of 256 floats per block: eight species at 8 need 56 KB, which is what builds
# (tests/test_modelgen_substeps_host.py compiles that worst case without scratch)
MAX_SUBSTEPS = 8
MAX_SUBSTEP_ROWS = 56  # (substeps - 1) * species: a block's static LDS ends at 64 KB
# `step_tolerance = (rtol, atol)`: the ceilings of the ladder 1 -> 2 -> 4 -> 8 that `substeps` may name (csrc/vihds_stepctl.hpp),
# and the fixed-grid solvers that decline such a model -- their fixed step h0 is not the observation interval
STEP_CONTROL_CEILINGS = (2, 4, 8)
_F32_MAX = float(np.finfo(np.float32).max)
STEP_CONTROL_DECLINED_SOLVERS = ("modeuler", "modeulerwhile")
# steps of the lead-in phase before the first observation point (`lead_in_steps`).  The adjoint keeps its intermediate states in
# the LDS rows the sub-steps use (never both at once): (lead_in_steps - 1) * species rows, at most MAX_SUBSTEP_ROWS
MAX_LEAD_IN_STEPS = 8
# unknowns of a model with `algebraic` variables: the matrix of a Newton step on the constraint lives in registers beside the
# states, its structural pattern is one 16-bit constant (tests/test_modelgen_algebraic_host.py compiles four without scratch)
MAX_ALGEBRAIC = 4
# reaction channels of a model with `noise_channels` (each a Wiener process of its own: two Philox blocks of four normals), and
# the entries of channel_noise that are not the constant 0: every one is an amplitude that lives in a register across the scheme's
# step, beside the states, the parameters and the stages.  Four entries per channel on average is what compiles without scratch
# with rk4 (tests/test_modelgen_channel_host.py builds that worst case; DESIGN.md 4.7 has the compiler's figures)
MAX_NOISE_CHANNELS = 8
MAX_NOISE_ENTRIES = 32
# species a model with `steady_species` solves for before the first step: the matrix of an iteration lives in registers beside
# the states, its structural pattern is one 64-bit constant (csrc/vihds_steady.hpp; tests/test_modelgen_steady_host.py compiles
# eight without scratch); and the iterations it may ask for (`steady_steps`, a fixed count)
MAX_STEADY = 8
MAX_STEADY_STEPS = 16


class ModelDefinitionError(TypeError):
    """A generated model's definition cannot be traced or breaks a limit of the kernels."""


class Network(object):
    """Linear(n_inputs, n_hidden) -> relu | tanh -> Linear(n_hidden, n_outputs), biases in both layers, raw outputs."""

    def __init__(self, n_inputs, n_hidden, n_outputs, hidden="relu"):
        self.n_inputs, self.n_hidden, self.n_outputs, self.hidden = n_inputs, n_hidden, n_outputs, hidden

    @property
    def sizes(self):
        return (int(self.n_inputs), int(self.n_hidden), int(self.n_outputs))

    @property
    def n_weights(self):
        I, H, O = self.sizes
        return H * I + H + O * H + O

    @property
    def n_fields(self):  # floats the adjoint dumps per evaluation: x [I], hidden pre-activation adjoints [H], h [H], output adjoints [O]
        I, H, O = self.sizes
        return I + 2 * H + O

    def tensor_shapes(self):
        I, H, O = self.sizes
        return [(H, I), (H,), (O, H), (O,)]

    def __repr__(self):
        return "Network(%d, %d, %d, hidden=%r)" % (self.sizes + (self.hidden,))


def _class_networks(cls):
    nets = getattr(cls, "networks", None)
    return dict(nets) if nets else {}


# ---------------------------------------------------------------------------------------------------------------------
# expression DAG
# ---------------------------------------------------------------------------------------------------------------------
_LEAVES = ("const", "th", "c", "y", "p", "t", "seed", "x")  # (x: the predicted signals precision() reads)
# ... and the two leaf kinds only log_likelihood() reads: the observations of the time point (forward only: data have no
# adjoint) and the precisions (the constant slots or the values of the model's own precision map)
_LEAVES += ("ob", "pr")
# ... and the forcings (rhs and the hooks): per-row time series, data like the observations
_LEAVES += ("f",)
# ... and the algebraic variables (rhs and observe): the unknowns z of the class's constraint, solved for where they are read
_LEAVES += ("z",)
# ... and the delayed reads (rhs only): the trajectory's own past, y_i(t - tau) -- a leaf WITH an adjoint, which rhs_vjp adds to
# the value and slope entries of the read's reserved slots ("dt": the stage time minus the interval start, its helper leaf)
_LEAVES += ("d", "dt")
_NO_ADJOINT = ("ob", "f", "dt")


def _control_flow(*_args, **_kw):
    raise ModelDefinitionError(
        "a generated model's functions are traced once, symbolically: Python control flow on a model quantity (if, "
        "and/or/not, bool(), float(), math.*) is not possible -- a comparison a < b gives a condition: combine conditions "
        "with & | ~ and select with where(cond, a, b); the operations are %s (clamp, minimum, maximum for bounds)"
        % ", ".join(OPERATIONS))


def _no_equality(*_args, **_kw):
    raise ModelDefinitionError(
        "== and != on a model quantity are not available to generated models: equality of floating-point values is not a "
        "condition to build a model on (conditions are a < b, a <= b, a > b, a >= b, combined with & | ~)")


def _condition_arithmetic(*_args, **_kw):
    raise ModelDefinitionError(
        "arithmetic on a condition: a condition (a < b, c1 & c2, ...) is not a number -- it combines with & | ~ and selects "
        "with where(cond, a, b); write where(cond, 1.0, 0.0) for an indicator")


class Sym(object):
    """A node of the expression DAG (interned by its graph: equal expressions are one node)."""

    __slots__ = ("g", "op", "args", "val", "id")

    def __init__(self, g, op, args, val, nid):
        self.g, self.op, self.args, self.val, self.id = g, op, args, val, nid

    def __add__(self, o):
        return self.g.make("add", (self, o))

    def __radd__(self, o):
        return self.g.make("add", (o, self))

    def __sub__(self, o):
        return self.g.make("sub", (self, o))

    def __rsub__(self, o):
        return self.g.make("sub", (o, self))

    def __mul__(self, o):
        return self.g.make("mul", (self, o))

    def __rmul__(self, o):
        return self.g.make("mul", (o, self))

    def __truediv__(self, o):
        return self.g.make("div", (self, o))

    def __rtruediv__(self, o):
        return self.g.make("div", (o, self))

    def __neg__(self):
        return self.g.make("neg", (self,))

    def __pos__(self):
        return self

    def __pow__(self, o):
        return self.g.make("pow", (self, o))

    def __rpow__(self, o):
        return self.g.make("pow", (o, self))

    def __abs__(self):
        return self.g.make("abs", (self,))

    def __lt__(self, o):
        return self.g.compare("lt", self, o)

    def __le__(self, o):
        return self.g.compare("le", self, o)

    def __gt__(self, o):
        return self.g.compare("lt", o, self)

    def __ge__(self, o):
        return self.g.compare("le", o, self)

    def __and__(self, o):
        return self.g.logic("and", (self, o))

    __rand__ = __and__

    def __or__(self, o):
        return self.g.logic("or", (self, o))

    __ror__ = __or__

    def __invert__(self):
        return self.g.logic("not", (self,))

    __bool__ = __float__ = __int__ = __index__ = _control_flow
    __eq__ = __ne__ = _no_equality
    __hash__ = object.__hash__

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        raise ModelDefinitionError("%s on a model quantity: a generated model can only use + - * / and %s"
                                   % (getattr(func, "__name__", func), ", ".join(OPERATIONS)))

    def __repr__(self):
        return "Sym(%s#%d)" % (self.op, self.id)


class Cond(Sym):
    """A condition node: a comparison of two quantities or a combination of conditions.  It selects in where(cond, a, b); it
    is no number (arithmetic and comparisons on it raise), and bool() of it -- if, and, or, not -- is Python control flow."""

    __slots__ = ()

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = _condition_arithmetic
    __neg__ = __pos__ = __pow__ = __rpow__ = __abs__ = _condition_arithmetic
    __lt__ = __le__ = __gt__ = __ge__ = _condition_arithmetic

    def __repr__(self):
        return "Cond(%s#%d)" % (self.op, self.id)


# ---------------------------------------------------------------------------------------------------------------------
# the operation table
# ---------------------------------------------------------------------------------------------------------------------
class Operation(object):
    """One operation of the DAG and everything that is known about it.  TO ADD AN OPERATION, ADD ONE RECORD to OP_TABLE:
    constant folding, the torch evaluation, the emitter, reverse mode, the module-level function and `op.<name>` all look
    it up here.
      arity      number of argument nodes
      val        True when the node carries constants in `val` (clamp's bounds); fold, torch and c then take them last
      fold       the operation on numpy float64 scalars (bools for the arguments that are conditions)
      torch      the operation on tensors (evaluate, and the module-level function on tensors)
      number     the module-level function on Python numbers, where it is not the fold (math.exp raises where the fold
                 gives inf)
      c          the C spelling, or (time loop, prepare / init) where the fast helpers of vihds_models.hpp differ from the
                 IEEE ones; %s per argument, then per constant of val
      peephole   (node, argument texts, fast) -> a cheaper spelling for this node, or None
      adjoint    (g, node, args, gb, acc): calls acc(argument, contribution) for each argument IN TURN -- vjp's output
                 depends on the order in which nodes are created, so a contribution is built right before it is
                 accumulated (a tuple's entries are evaluated left to right); None for the kinds without one
      kind       "value"; "condition" (a bool: selects in where, no adjoint, no arithmetic); "pass" (a node only vjp
                 builds -- the backward weight of clamp, minimum / maximum, abs: piecewise constant, no adjoint)
      public     a name of the model language: listed in OPERATIONS, a module attribute and an attribute of `op`"""

    __slots__ = ("name", "arity", "val", "fold", "torch", "number", "c", "peephole", "adjoint", "kind", "commutative", "public")

    def __init__(self, name, arity, fold, torch, c, adjoint=None, kind="value", val=False, commutative=False, public=False,
                 number=None, peephole=None):
        self.name, self.arity, self.fold, self.torch, self.adjoint, self.kind = name, arity, fold, torch, adjoint, kind
        self.val, self.commutative, self.public, self.peephole = val, commutative, public, peephole
        self.c = (c, c) if isinstance(c, str) else c
        self.number = number or (lambda *a: _fold(name, *a))


def _is_const(n, v):
    return n.op == "const" and n.val == v


def _like(v, other):
    """A Python number as a tensor beside `other` (torch.minimum / maximum / where want tensors)."""
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(float(v), dtype=other.dtype, device=other.device)


def _both_tensors(f):
    return lambda a, b: f(_like(a, b if isinstance(b, torch.Tensor) else a), _like(b, a if isinstance(a, torch.Tensor) else b))


def _pass_weight(a, b, beaten):
    """The backward weight of minimum / maximum for a: 0 where b wins (`beaten`), 1/2 at a tie, else 1 (NaN included)."""
    return torch.where(a == b, 0.5, 1.0).masked_fill(beaten, 0.0).to(a.dtype)


_TWO_OVER_SQRT_PI = 2.0 / math.sqrt(math.pi)
_O = Operation
OP_TABLE = {r.name: r for r in (
    _O("add", 2, operator.add, operator.add, "%s + %s", lambda g, n, a, gb, acc: (acc(a[0], gb), acc(a[1], gb)),
       commutative=True),
    _O("sub", 2, operator.sub, operator.sub, "%s - %s", lambda g, n, a, gb, acc: (acc(a[0], gb), acc(a[1], -gb))),
    _O("mul", 2, operator.mul, operator.mul, "%s * %s", lambda g, n, a, gb, acc: (acc(a[0], gb * a[1]), acc(a[1], gb * a[0])),
       commutative=True),
    # torch: grad / other, -grad * ((self / other) / other)
    _O("div", 2, operator.truediv, operator.truediv, ("fdiv(%s, %s)", "%s / %s"),
       lambda g, n, a, gb, acc: (acc(a[0], gb / a[1]), acc(a[1], -(gb * (n / a[1])))),
       peephole=lambda n, a, fast: "frcp(%s)" % a[1] if fast and _is_const(n.args[0], 1.0) else None),
    _O("neg", 1, operator.neg, operator.neg, "-%s", lambda g, n, a, gb, acc: acc(a[0], -gb)),
    _O("exp", 1, np.exp, torch.exp, ("fexp(%s)", "expf(%s)"), lambda g, n, a, gb, acc: acc(a[0], gb * n),
       public=True, number=math.exp),
    _O("log", 1, np.log, torch.log, "logf(%s)", lambda g, n, a, gb, acc: acc(a[0], gb / a[0]), public=True, number=math.log),
    # pow_vjp: g n a^(n-1), g a^n log(a)  (unmasked at a = 0: see the module docstring)
    _O("pow", 2, np.power, torch.pow, "powf(%s, %s)",
       lambda g, n, a, gb, acc: (acc(a[0], gb * (a[1] * g.make("pow", (a[0], a[1] - 1.0)))),
                                 acc(a[1], gb * (n * g.make("log", (a[0],))))),
       public=True, number=math.pow,
       peephole=lambda n, a, fast: "%s * %s" % (a[0], a[0]) if _is_const(n.args[1], 2.0) else None),
    _O("sigmoid", 1, lambda a: 1.0 / (1.0 + np.exp(-a)), torch.sigmoid, ("sigmoid_f(%s)", "1.f / (1.f + expf(-%s))"),
       lambda g, n, a, gb, acc: acc(a[0], gb * (n * (1.0 - n))), public=True, number=lambda x: 1.0 / (1.0 + math.exp(-x))),
    _O("tanh", 1, np.tanh, torch.tanh, ("ftanh(%s)", "tanhf(%s)"), lambda g, n, a, gb, acc: acc(a[0], gb * (1.0 - n * n)),
       public=True, number=math.tanh),
    # (clamp and where are public with functions written out below: their arguments are checked)
    _O("clamp", 1, lambda a, v: min(max(a, v[0]), v[1]) if a == a else a, lambda a, v: torch.clamp(a, v[0], v[1]),
       "clampf(%s, %s, %s)", lambda g, n, a, gb, acc: acc(a[0], gb * g.make("cpass", (a[0],), n.val)), val=True, public=True),
    _O("cpass", 1, lambda a, v: 1.0 if v[0] <= a <= v[1] else 0.0, lambda a, v: ((a >= v[0]) & (a <= v[1])).to(a.dtype),
       "clamp_pass(%s, %s, %s)", kind="pass", val=True),
    # conditions: a < b and a <= b (a > b and a >= b are the same two with the arguments swapped) and their combinations;
    # a NaN operand makes every comparison false.  They are bools in C, where is a select (one v_cndmask_b32): straight-line
    # code, no branch
    _O("lt", 2, operator.lt, operator.lt, "%s < %s", kind="condition"),
    _O("le", 2, operator.le, operator.le, "%s <= %s", kind="condition"),
    _O("and", 2, operator.and_, operator.and_, "%s && %s", kind="condition"),
    _O("or", 2, operator.or_, operator.or_, "%s || %s", kind="condition"),
    _O("not", 1, operator.not_, operator.invert, "!%s", kind="condition"),
    # a select of the adjoint, never a product with a mask: what the other branch holds is not touched
    _O("where", 3, lambda c, a, b: a if c else b, torch.where, "fsel(%s, %s, %s)",
       lambda g, n, a, gb, acc: (acc(a[1], g.where(a[0], gb, g.const(0.0))), acc(a[2], g.where(a[0], g.const(0.0), gb))),
       public=True),
    # np.minimum / np.maximum propagate NaN, as torch's; the adjoint: g to the selected argument, g / 2 to each at a tie
    _O("minimum", 2, np.minimum, _both_tensors(torch.minimum), "fmin_nan(%s, %s)",
       lambda g, n, a, gb, acc: (acc(a[0], gb * g.make("minpass", (a[0], a[1]))), acc(a[1], gb * g.make("minpass", (a[1], a[0])))),
       public=True),
    _O("maximum", 2, np.maximum, _both_tensors(torch.maximum), "fmax_nan(%s, %s)",
       lambda g, n, a, gb, acc: (acc(a[0], gb * g.make("maxpass", (a[0], a[1]))), acc(a[1], gb * g.make("maxpass", (a[1], a[0])))),
       public=True),
    _O("minpass", 2, lambda a, b: 0.0 if a > b else (0.5 if a == b else 1.0), lambda a, b: _pass_weight(a, b, a > b),
       "min_pass(%s, %s)", kind="pass"),
    _O("maxpass", 2, lambda a, b: 0.0 if a < b else (0.5 if a == b else 1.0), lambda a, b: _pass_weight(a, b, a < b),
       "max_pass(%s, %s)", kind="pass"),
    # g sign(x), sign(0) = 0
    _O("abs", 1, np.abs, torch.abs, "fabsf(%s)", lambda g, n, a, gb, acc: acc(a[0], gb * g.make("sign", (a[0],))), public=True),
    _O("sign", 1, lambda a: 1.0 if a > 0.0 else (-1.0 if a < 0.0 else 0.0), torch.sign, "fsign(%s)", kind="pass"),
    # g / (2 sqrt(x)): infinite at 0, as torch's; the value is NaN below 0, as the kernels' and torch's
    _O("sqrt", 1, np.sqrt, torch.sqrt, ("fsqrt(%s)", "sqrtf(%s)"), lambda g, n, a, gb, acc: acc(a[0], gb / (2.0 * n)),
       public=True),
    _O("erf", 1, math.erf, torch.erf, "erff(%s)",
       lambda g, n, a, gb, acc: acc(a[0], gb * (_TWO_OVER_SQRT_PI * g.make("exp", (-(a[0] * a[0]),)))), public=True),
    _O("erfc", 1, math.erfc, torch.erfc, "erfcf(%s)",
       lambda g, n, a, gb, acc: acc(a[0], -(gb * (_TWO_OVER_SQRT_PI * g.make("exp", (-(a[0] * a[0]),))))), public=True),
)}
del _O
OPERATIONS = tuple(r.name for r in OP_TABLE.values() if r.public)
_COMMUTATIVE = tuple(r.name for r in OP_TABLE.values() if r.commutative)
# ("cconst": the constant conditions that folding leaves -- a leaf, like "const")
_CONDITIONS = tuple(r.name for r in OP_TABLE.values() if r.kind == "condition") + ("cconst",)


def _fold(op, *args, val=None):
    """Constant folding in float64 (IEEE semantics: inf / NaN instead of exceptions); a condition folds to a bool."""
    rec = OP_TABLE[op]
    with np.errstate(all="ignore"):
        args = [a if isinstance(a, (bool, np.bool_)) else np.float64(a) for a in args]
        v = rec.fold(*args, val) if rec.val else rec.fold(*args)
    return bool(v) if rec.kind == "condition" else float(v)


class Graph(object):
    """Hash-consed expression DAG: building a node that exists returns that node (common-subexpression elimination);
    operations on constants are folded; x+0, x*1, x*0, x/1, -(-x), pow(x, 1), where(c, a, a), minimum(a, a) simplify.
    Conditions (compare, logic) are nodes of their own class, Cond; where() selects between two values by one."""

    def __init__(self, networks=()):
        self.nodes = []
        self._table = {}
        self.networks = list(networks)  # Network objects; a "net" node's val is its index here

    def _intern(self, op, args, val):
        key = (op, tuple(a.id for a in args), val)
        n = self._table.get(key)
        if n is None:
            n = (Cond if op in _CONDITIONS else Sym)(self, op, tuple(args), val, len(self.nodes))
            self.nodes.append(n)
            self._table[key] = n
        return n

    def const(self, v):
        v = float(v)
        return self._intern("const", (), 0.0 if v == 0.0 else v)  # (one zero: -0.0 and 0.0 fold together)

    def leaf(self, kind, index):
        return self._intern(kind, (), index)

    def _arg(self, a):
        if isinstance(a, Cond):
            _condition_arithmetic()
        if isinstance(a, Sym):
            if a.g is not self:
                raise ModelDefinitionError("a model quantity from another trace was used")
            return a
        if isinstance(a, (bool, np.bool_)) or not isinstance(a, (int, float, np.integer, np.floating)):
            raise ModelDefinitionError("unsupported operand %r of type %s in a generated model (Python numbers and model "
                                       "quantities only)" % (a, type(a).__name__))
        return self.const(a)

    def net(self, k, inputs):
        """Network k applied to `inputs`: the call node and one node per output (never folded or simplified)."""
        call = self._intern("net", tuple(self._arg(a) for a in inputs), k)
        return [self._intern("netout", (call,), j) for j in range(self.networks[k].sizes[2])]

    def compare(self, op, a, b):
        """The condition a < b ("lt") or a <= b ("le"); constant operands fold to a constant condition."""
        a, b = self._arg(a), self._arg(b)
        if a.op == "const" and b.op == "const":
            return self._intern("cconst", (), _fold(op, a.val, b.val))
        return self._intern(op, (a, b), None)

    def _condition(self, c, what):
        if isinstance(c, Cond):
            if c.g is not self:
                raise ModelDefinitionError("a model quantity from another trace was used")
            return c
        if isinstance(c, (bool, np.bool_)):
            return self._intern("cconst", (), bool(c))
        raise ModelDefinitionError("%s takes conditions (a < b, a <= b, a > b, a >= b and their combinations with & | ~) or a "
                                   "Python bool, not %s" % (what, "a model quantity" if isinstance(c, Sym) else type(c).__name__))

    def logic(self, op, args):
        """c1 & c2 ("and"), c1 | c2 ("or"), ~c ("not"); constant conditions fold, c & c, c | c and ~~c simplify."""
        args = tuple(self._condition(c, {"and": "&", "or": "|", "not": "~"}[op]) for c in args)
        if op == "not":
            if args[0].op == "cconst": return self._intern("cconst", (), _fold(op, args[0].val))
            if args[0].op == "not": return args[0].args[0]
            return self._intern(op, args, None)
        absorbing = op == "or"  # (the constant that decides the result: True for |, False for &)
        for k in (0, 1):
            if args[k].op == "cconst":
                return args[k] if args[k].val == absorbing else args[1 - k]
        if args[0] is args[1]:
            return args[0]
        if args[0].id > args[1].id:
            args = (args[1], args[0])
        return self._intern(op, args, None)

    def where(self, c, a, b):
        """a where the condition holds, else b (a select: the value not taken may be anything, NaN and inf included)."""
        c = self._condition(c, "where(cond, a, b): cond")
        a, b = self._arg(a), self._arg(b)
        if c.op == "cconst":
            return a if c.val else b
        if a is b:
            return a
        return self._intern("where", (c, a, b), None)

    def make(self, op, args, val=None):
        args = tuple(self._arg(a) for a in args)
        if all(a.op == "const" for a in args):
            return self.const(_fold(op, *[a.val for a in args], val=val))
        zero = lambda s: s.op == "const" and s.val == 0.0  # noqa: E731
        one = lambda s: s.op == "const" and s.val == 1.0  # noqa: E731
        if op == "add":
            if zero(args[0]): return args[1]
            if zero(args[1]): return args[0]
        elif op == "sub":
            if zero(args[1]): return args[0]
            if zero(args[0]): return self.make("neg", (args[1],))
        elif op == "mul":
            if zero(args[0]) or zero(args[1]): return self.const(0.0)
            if one(args[0]): return args[1]
            if one(args[1]): return args[0]
            if args[0].op == "const" and args[0].val == -1.0: return self.make("neg", (args[1],))
            if args[1].op == "const" and args[1].val == -1.0: return self.make("neg", (args[0],))
        elif op == "div":
            if one(args[1]): return args[0]
            if zero(args[0]): return self.const(0.0)
        elif op == "neg":
            if args[0].op == "neg": return args[0].args[0]
        elif op == "pow":
            if one(args[1]): return args[0]
        elif op in ("minimum", "maximum"):
            if args[0] is args[1]: return args[0]
        if op in _COMMUTATIVE and args[0].id > args[1].id:
            args = (args[1], args[0])
        return self._intern(op, args, val)


# ---------------------------------------------------------------------------------------------------------------------
# the operation namespace (dispatch on argument type)
# ---------------------------------------------------------------------------------------------------------------------
def _sym_of(args):
    for a in args:
        if isinstance(a, Sym):
            return a.g
    return None


def _tensor_of(args):
    return any(isinstance(a, torch.Tensor) for a in args)


def _number(x, what):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ModelDefinitionError("%s must be a Python number (got %s)" % (what, type(x).__name__))
    return float(x)


def clamp(x, lo, hi):
    lo, hi = _number(lo, "clamp's lower bound"), _number(hi, "clamp's upper bound")
    if not lo <= hi:
        raise ModelDefinitionError("clamp: lower bound %g above upper bound %g" % (lo, hi))
    g = _sym_of((x,))
    if g: return g.make("clamp", (x,), (lo, hi))
    if _tensor_of((x,)):
        return torch.clamp(x, lo, hi)
    return min(max(x, lo), hi)


def where(cond, a, b):
    """a where cond holds, else b.  cond is a condition (a comparison of model quantities / numbers, combined with & | ~) or
    a Python bool, which selects when the model is traced."""
    g = _sym_of((cond, a, b))
    if g: return g.where(cond, a, b)
    if isinstance(cond, (bool, np.bool_)):
        return a if cond else b
    if not (isinstance(cond, torch.Tensor) and cond.dtype == torch.bool):
        raise ModelDefinitionError("where(cond, a, b): cond must be a condition (a < b, ... combined with & | ~) or a Python "
                                   "bool, not %s" % type(cond).__name__)
    ta, tb = isinstance(a, torch.Tensor), isinstance(b, torch.Tensor)
    if ta or tb:
        return torch.where(cond, _like(a, b if tb else a), _like(b, a if ta else b))
    # two Python numbers: nothing says which float type the caller computes in.  Numbers that float32 holds exactly (0.0 and
    # 1.0 of a switch) stay float32, which every tensor they meet promotes; any other pair is kept in float64
    a, b = _number(a, "where's value"), _number(b, "where's value")
    exact = all(float(np.float32(v)) == v or v != v for v in (a, b))
    dtype = torch.float32 if exact else torch.float64
    return torch.where(cond, torch.tensor(a, dtype=dtype, device=cond.device), torch.tensor(b, dtype=dtype, device=cond.device))


def _dispatching(rec):
    """The module-level function of a table record: symbols build the node, tensors take torch, numbers take math."""
    def f(*args):
        if len(args) != rec.arity:
            raise TypeError("%s() takes %d positional argument(s) but %d were given" % (rec.name, rec.arity, len(args)))
        g = _sym_of(args)
        if g: return g.make(rec.name, args)
        return rec.torch(*args) if _tensor_of(args) else rec.number(*args)

    f.__name__ = f.__qualname__ = rec.name
    return f


# exp, log, pow, sigmoid, tanh, minimum, maximum, abs (Python's abs() on a model quantity comes here too), sqrt, erf, erfc
globals().update((r.name, _dispatching(r)) for r in OP_TABLE.values() if r.public and r.name not in globals())


class _Namespace(object):
    """`op.exp(x)` ...: the operations as one object; any other name is refused with the list."""

    def __getattr__(self, name):
        if name in OPERATIONS:
            return globals()[name]
        raise ModelDefinitionError("operation '%s' is not available to generated models (available: + - * / and %s)"
                                   % (name, ", ".join(OPERATIONS)))


op = _Namespace()


# ---------------------------------------------------------------------------------------------------------------------
# reverse mode
# ---------------------------------------------------------------------------------------------------------------------
def _topo(roots):
    """Nodes reachable from roots, every node after its arguments (deterministic: roots and arguments in order)."""
    seen, order = set(), []
    for r in roots:
        stack = [(r, False)]
        while stack:
            n, done = stack.pop()
            if done:
                order.append(n)
                continue
            if n.id in seen:
                continue
            seen.add(n.id)
            stack.append((n, True))
            for a in reversed(n.args):
                if a.id not in seen:
                    stack.append((a, False))
    return order


def vjp(g, outputs, seeds):
    """Reverse-mode derivative of the DAG: {leaf node id: adjoint node} for sum_k seeds[k] * d outputs[k] / d leaf.  Each
    operation's rule is torch autograd's formula (clamp: gradient where lo <= x <= hi; pow: csrc pow_vjp, unmasked at a
    zero base -- module docstring)."""
    adj = {}
    net_adj = {}  # "net" node id -> {output index: adjoint}

    def acc(node, contrib):
        if node.op == "const" or node.op in _NO_ADJOINT:
            return
        adj[node.id] = g.make("add", (adj[node.id], contrib)) if node.id in adj else contrib

    for o, s in zip(outputs, seeds):
        if isinstance(o, Sym):
            acc(o, g._arg(s))
    order = _topo([o for o in outputs if isinstance(o, Sym)])
    for n in reversed(order):
        if n.op == "net":
            # every output node has been visited: one adjoint node for the call (the kernel's net<k>_vjp, which also dumps
            # what the weight gradient is contracted from) and one node per input adjoint
            ob = net_adj.get(n.id)
            if ob is not None:
                I, _H, O = g.networks[n.val].sizes
                back = g._intern("netbwd", n.args + tuple(ob.get(j, g.const(0.0)) for j in range(O)), n.val)
                for i in range(I):
                    acc(n.args[i], g._intern("netbwd_in", (back,), i))
            continue
        if n.id not in adj or n.op in _LEAVES:
            continue
        gb = adj[n.id]
        a = n.args
        if n.op == "netout":
            net_adj.setdefault(a[0].id, {})[n.val] = gb
        elif n.op in ("netbwd", "netbwd_in"):
            raise ModelDefinitionError("second derivatives of a network are not generated")
        elif OP_TABLE[n.op].adjoint is not None:  # (conditions and pass nodes: piecewise constant)
            OP_TABLE[n.op].adjoint(g, n, a, gb, acc)
    return adj


def _net_act(net, z):
    return torch.relu(z) if net.hidden == "relu" else torch.tanh(z)


def net_forward_ref(net, W, x):
    """The network on x [..., I] with W = (W1, b1, W2, b2): (hidden pre-activations, hidden activations, outputs)."""
    W1, b1, W2, b2 = W
    z = x @ W1.t() + b1
    h = _net_act(net, z)
    return z, h, h @ W2.t() + b2


def net_vjp_ref(net, W, x, ob):
    """What the generated adjoint computes, formula by formula: the input adjoint xb [..., I] and the four weight adjoints
    as the contraction of the dump forms them (hidden pre-activation adjoints x inputs, output adjoints x hidden
    activations, row sums for the biases).  ReLU passes the gradient where the pre-activation is > 0 (0 at 0, as torch)."""
    W1, _b1, W2, _b2 = W
    z, h, _ = net_forward_ref(net, W, x)
    ob = ob.expand(x.shape[:-1] + ob.shape[-1:])
    hb = ob @ W2
    zb = hb * ((z > 0).to(z.dtype) if net.hidden == "relu" else (1.0 - h * h))
    flat = lambda v: v.reshape(-1, v.shape[-1])  # noqa: E731
    return zb @ W1, (flat(zb).t() @ flat(x), flat(zb).sum(0), flat(ob).t() @ flat(h), flat(ob).sum(0))


def evaluate(outputs, env):
    """Evaluate DAG nodes with torch (float64 in the tests): env maps (leaf kind, index) -> value; ("w", k) -> the (W1, b1,
    W2, b2) of network k; the weight adjoints a "netbwd" node forms are left in env["wgrad"][k] when that dict exists."""
    vals = {}
    stack = lambda a: torch.stack(torch.broadcast_tensors(*a), dim=-1)  # noqa: E731
    for n in _topo([o for o in outputs if isinstance(o, Sym)]):
        a = [vals[x.id] for x in n.args]
        if n.op == "const": v = torch.tensor(n.val, dtype=torch.float64)
        elif n.op in _LEAVES: v = env[(n.op, n.val)]
        elif n.op == "net": v = net_forward_ref(n.g.networks[n.val], env[("w", n.val)], stack(a))[2]
        elif n.op == "netout": v = a[0][..., n.val]
        elif n.op == "netbwd":
            I = n.g.networks[n.val].sizes[0]
            v, wg = net_vjp_ref(n.g.networks[n.val], env[("w", n.val)], stack(a[:I]), stack(a[I:]))
            if "wgrad" in env:
                env["wgrad"][n.val] = wg
        elif n.op == "netbwd_in": v = a[0][..., n.val]
        elif OP_TABLE[n.op].val: v = OP_TABLE[n.op].torch(*a, n.val)
        else: v = OP_TABLE[n.op].torch(*a)
        vals[n.id] = v
    return [vals[o.id] if isinstance(o, Sym) else torch.tensor(float(o), dtype=torch.float64) for o in outputs]


# ---------------------------------------------------------------------------------------------------------------------
# tracing
# ---------------------------------------------------------------------------------------------------------------------
class _Named(object):
    """th / p: quantities by attribute (th.r) or by key (th["aYFP_PR"])."""

    def __init__(self, values, what):
        object.__setattr__(self, "_v", dict(values))
        object.__setattr__(self, "_what", what)

    def __getattr__(self, name):
        try:
            return self._v[name]
        except KeyError:
            raise ModelDefinitionError("unknown %s '%s' (defined: %s)" % (self._what, name, ", ".join(self._v))) from None

    __getitem__ = __getattr__

    def __setattr__(self, name, value):
        raise ModelDefinitionError("%s are read-only" % self._what)


class _Conditions(object):
    def __init__(self, values):
        self._v = list(values)

    def __getitem__(self, q):
        if not isinstance(q, int) or not 0 <= q < len(self._v):
            raise ModelDefinitionError("treatment c[%r] out of range: the model declares n_conditions = %d" % (q, len(self._v)))
        return self._v[q]

    def __len__(self):
        return len(self._v)


class _Networks(object):
    """`self.net` of the instance the three functions run on: one callable per declared network, `self.net.<name>(inputs)`
    -> list of n_outputs values.  call(k, name, network, inputs) does the work (symbolic or torch)."""

    def __init__(self, cls, call):
        object.__setattr__(self, "_nets", _class_networks(cls))
        object.__setattr__(self, "_call", call)
        object.__setattr__(self, "_cls", cls.__name__)

    def __getattr__(self, name):
        nets = self._nets
        if name not in nets:
            raise ModelDefinitionError("unknown network '%s' (%s.networks declares: %s)"
                                       % (name, self._cls, ", ".join(nets) or "none"))
        k, net = list(nets).index(name), nets[name]

        def apply(inputs):
            if not isinstance(inputs, (list, tuple)) or len(inputs) != net.sizes[0]:
                raise ModelDefinitionError("network '%s' takes a list of %d inputs (got %s)" % (
                    name, net.sizes[0], len(inputs) if isinstance(inputs, (list, tuple)) else type(inputs).__name__))
            return self._call(k, name, net, list(inputs))

        return apply

    __getitem__ = __getattr__

    def __setattr__(self, name, value):
        raise ModelDefinitionError("networks are read-only")


def _class_forcings(cls):
    return list(getattr(cls, "forcings", None) or ())


class _Forcings(object):
    """`self.forcing` of the instance the functions run on: `self.forcing.<name>` is the value of that forcing where the
    function is evaluated.  read(k, name) does the work (symbolic or torch)."""

    def __init__(self, cls, read):
        object.__setattr__(self, "_names", _class_forcings(cls))
        object.__setattr__(self, "_read", read)
        object.__setattr__(self, "_cls", cls.__name__)

    def __getattr__(self, name):
        if name not in self._names:
            raise ModelDefinitionError("unknown forcing '%s' (%s.forcings declares: %s)"
                                       % (name, self._cls, ", ".join(self._names) or "none"))
        return self._read(self._names.index(name), name)

    __getitem__ = __getattr__

    def __setattr__(self, name, value):
        raise ModelDefinitionError("forcings are read-only")


def _class_delays(cls):
    """[(name, species, effective parameter)] of the class's delayed reads, in declaration order."""
    d = getattr(cls, "delays", None) or {}
    return [(k, v[0], v[1]) for k, v in d.items()] if isinstance(d, dict) else []


class _Delayed(object):
    """`self.delayed` of the instance the functions run on: `self.delayed.<name>` is that species at t - tau where rhs is
    evaluated.  read(e, name) does the work (symbolic or torch)."""

    def __init__(self, cls, read):
        object.__setattr__(self, "_names", [d[0] for d in _class_delays(cls)])
        object.__setattr__(self, "_read", read)
        object.__setattr__(self, "_cls", cls.__name__)

    def __getattr__(self, name):
        if name not in self._names:
            raise ModelDefinitionError("unknown delayed read '%s' (%s.delays declares: %s)"
                                       % (name, self._cls, ", ".join(self._names) or "none"))
        return self._read(self._names.index(name), name)

    __getitem__ = __getattr__

    def __setattr__(self, name, value):
        raise ModelDefinitionError("delayed reads are read-only")


def _delay_misread(name, where):
    raise ModelDefinitionError(
        "delayed read '%s' read in %s: a delayed read is the trajectory's own past at the stage time of a step, so it is read "
        "in rhs(self, t, y, p, c) only (not in prepare, initial_state, start, constraint or any hook)" % (name, where))


def _class_algebraic(cls):
    return list(getattr(cls, "algebraic", None) or ())


class _Algebraic(object):
    """`self.algebraic` of the instance the functions run on: `self.algebraic.<name>` is that unknown of the constraint at the
    state where the function is evaluated.  read(i, name) does the work (symbolic or torch)."""

    def __init__(self, cls, read):
        object.__setattr__(self, "_names", _class_algebraic(cls))
        object.__setattr__(self, "_read", read)
        object.__setattr__(self, "_cls", cls.__name__)

    def __getattr__(self, name):
        if name not in self._names:
            raise ModelDefinitionError("unknown algebraic variable '%s' (%s.algebraic declares: %s)"
                                       % (name, self._cls, ", ".join(self._names) or "none"))
        return self._read(self._names.index(name), name)

    __getitem__ = __getattr__

    def __setattr__(self, name, value):
        raise ModelDefinitionError("algebraic variables are read-only")

    def __len__(self):
        return len(self._names)

    def __iter__(self):
        return iter(self._names)


def _class_steady(cls):
    return list(getattr(cls, "steady_species", None) or ())


_ALGEBRAIC_READERS = ("rhs", "observe")  # the functions that may read self.algebraic.<name>


def _algebraic_misread(name, where):
    raise ModelDefinitionError(
        "algebraic variable '%s' read in %s: the constraint is solved where rhs and observe are evaluated -- an algebraic "
        "variable is read in rhs(self, t, y, p, c) and in observe(self, y, p, c) only (constraint receives the unknowns as its "
        "argument z)" % (name, where))


# ---------------------------------------------------------------------------------------------------------------------
# the hook table
# ---------------------------------------------------------------------------------------------------------------------
def _settle_observe_kind(cls):
    """A class with a map of its own (defined here or inherited) has observe_kind "custom", and none of the fixed kinds."""
    if getattr(cls, "_observe_def", None) is None:
        return
    for k in cls.__mro__:
        kind = k.__dict__.get("observe_kind", "default")
        if kind != "default" and not (kind == OBSERVE_CUSTOM and k.__dict__.get("_observe_kind_set")):
            raise ModelDefinitionError("%s defines observe and observe_kind = %r: a model has either a map of its "
                                       "own or one of the fixed kinds (leave observe_kind at 'default')"
                                       % (cls.__name__, kind))
        if k is GeneratedOdeModel:
            break
    cls.observe_kind, cls._observe_kind_set = OBSERVE_CUSTOM, True


_GROUP_ADJOINT = {"y": "yb", "x": "xpb", "pr": "prb", "p": "pb"}  # leaf kind -> the kernel's adjoint array ("ob": data, none)


class Hook(object):
    """One optional function of a model that the kernels call once per time point, inside the time loop; it returns four
    values (n_outputs says otherwise), is traced into the model's DAG (the operations of rhs: no t, no network calls) and is emitted with its
    reverse-mode adjoint as two members of the struct.  TO ADD A HOOK, ADD ONE RECORD to HOOKS (in the order in which the
    forward kernel calls them) and its call site in the kernels; tracing, code generation, the capture of the definition
    when a class is defined and the torch restatement walk this table.
      name, signature    the Python method, and how error messages spell it
      groups             the lists of leaves it receives, in order, from "y" (the N species), "x" (the 4 predicted
                         signals), "ob" (the 4 observations), "pr" (the 4 precisions); p and c always follow.  The adjoint
                         adds into the adjoint array of each group that has one (_GROUP_ADJOINT), in this order, and last
                         into pb of the named effective parameters (a treatment has no adjoint)
      outputs            what the four returned values are, in error messages
      n_outputs          how many values it returns: 4, "species" (one per species: the state jump) or "channels" (one list
                         per noise channel, each with one value per species: the reaction-channel noise, kept as the flat
                         list G[q * R + r] of species q and channel r)
      attr, traced       the class attribute that holds the definition; the Trace attribute that holds its four nodes
      c_out, seed        the C arrays of the values and of their adjoints
      c_forward, c_adjoint   the members' signatures
      switch, switch_note    what tells the kernels that the struct has the members: the value of OBS, or a constant of
                         its own declared with this comment
      excludes_neural    what the model then owns that NeuralPrecisions would own too (None: they combine)
    and how the definition is taken from a class body (GeneratedOdeModel.__init_subclass__):
      note               what the "must be a function" error adds to the signature
      hides_method       the definition is removed from the class (observe would hide OdeModel.observe(x_sample, theta), the
                         entry point the decoder calls on instances: the definition is kept as the class's map)
      none_resets        `name = None` in a subclass returns to the kernels' default
      checks_arguments   the definition must take exactly the arguments of the signature (more with defaults, and
                         keyword-only helpers, are the author's own)
      settle             called for every subclass after the capture
      skips_zero         an output that folds to the constant 0 is not written and its seed is not read; the struct declares
                         NOISE_MASK, bit j set for every output that is left (process noise)"""

    switch_note = excludes_neural = settle = None
    note = ""
    n_outputs = 4
    hides_method = none_resets = checks_arguments = skips_zero = False

    def __init__(self, name, **fields):
        self.name = name
        self.__dict__.update(fields)

    @property
    def targets(self):
        return [(k, _GROUP_ADJOINT[k]) for k in self.groups + ("p",) if k in _GROUP_ADJOINT]

    def count(self, n_species, n_channels=0):
        """The number of values the hook returns for a model of n_species species (and n_channels noise channels)."""
        if self.n_outputs == "channels":
            return n_species * n_channels
        return n_species if self.n_outputs == "species" else self.n_outputs


# the start map: called once per trajectory, after init and before the first step -- not inside the time loop, so it is a record
# of its own beside HOOKS (ALL_HOOKS, below, is what tracing, code generation and the capture of the definitions walk); sees what
# initial_state returned, the effective parameters and the treatments -- no t; a forcing reads its first sample.  It returns the
# state the integration starts from, one value per species
START_HOOK = \
    Hook("start", signature="start(self, y, p, c)", groups=("y",), outputs="the state the integration starts from, one value per species",
         n_outputs="species", attr="_start_def", traced="start", c_out="ys", seed="ysb",
         switch="OWN_START", switch_note="the integration starts from start(init): start / start_vjp",
         c_forward=["  __device__ static void start(const float* y, const float* p, float* ys) {"],
         c_adjoint=["  __device__ static void start_vjp(const float* y, const float* p, const float* ysb, float* yb, float* pb) {"],
         excludes_neural="start map", none_resets=True, checks_arguments=True,
         note=": it sees what initial_state returned, the effective parameters and the treatments -- no t "
              "(or None in a subclass, for no start map)")

HOOKS = (
    # the observation map: sees the species, the effective parameters and the treatments, like rhs without t
    Hook("observe", signature="observe(self, y, p, c)", groups=("y",), outputs="the OD, RFP, YFP and CFP signals",
         attr="_observe_def", traced="obs", c_out="xp", seed="xpb", switch="OBS_CUSTOM",
         c_forward=["  __device__ static void observe(const float* y, const float* p, float* xp) {"],
         c_adjoint=["  __device__ static void observe_vjp(const float* y, const float* p, const float* xpb, float* yb, float* pb) {"],
         hides_method=True, settle=_settle_observe_kind),
    # the observation noise: sees the species, the four predicted signals, the effective parameters and the treatments.  Its
    # adjoint adds into xpb too (the predicted signals' adjoint, which observe_vjp then pulls back)
    Hook("precision", signature="precision(self, y, x, p, c)", groups=("y", "x"),
         outputs="the precisions of the OD, RFP, YFP and CFP signals", attr="_precision_def", traced="prec", c_out="pr", seed="prb",
         switch="OWN_PREC", switch_note="the precisions are this struct's map: no prec_* / init_prec_* slots",
         c_forward=["  __device__ static void precision(const float* y, const float* xp, const float* p, float* pr) {"],
         c_adjoint=["  __device__ static void precision_vjp(const float* y, const float* xp, const float* p, const float* prb, float* yb,",
                    "                                       float* xpb, float* pb) {"],
         excludes_neural="precision map"),
    # the observation log density: sees the four predicted signals, the four observations (data: no adjoint) and the four
    # precisions of the time point, the effective parameters and the treatments -- no species, no t
    Hook("log_likelihood", signature="log_likelihood(self, x, obs, pr, p, c)", groups=("x", "ob", "pr"),
         outputs="the log densities of the OD, RFP, YFP and CFP signals at one time point", attr="_likelihood_def", traced="lik",
         c_out="ll", seed="llb", switch="OWN_LIK", switch_note="the observation log density is this struct's: loglik / loglik_vjp",
         c_forward=["  __device__ static void loglik(const float* xp, const float* ob, const float* pr, const float* p, float* ll) {"],
         c_adjoint=["  __device__ static void loglik_vjp(const float* xp, const float* ob, const float* pr, const float* p, const float* llb,",
                    "                                    float* xpb, float* prb, float* pb) {"],
         excludes_neural="likelihood", none_resets=True, checks_arguments=True,
         note=": it sees the predicted signals, the observations and the precisions of one time point, the effective parameters "
              "and the treatments -- no t and no species (or None in a subclass, for the Gaussian)"),
    # the state jump: called last, after the point's state is stored, observed and scored; sees the species (the left limit),
    # the effective parameters and the treatments -- no t: an event schedule travels as a forcing, a state-triggered event is a
    # where on y.  It returns the state right after the time point, one value per species; the next interval starts there
    Hook("jump", signature="jump(self, y, p, c)", groups=("y",), outputs="the state right after the time point, one value per species",
         n_outputs="species", attr="_jump_def", traced="jmp", c_out="yj", seed="yjb",
         switch="OWN_JUMP", switch_note="the state jumps at the observation points: jump / jump_vjp",
         c_forward=["  __device__ static void jump(const float* y, const float* p, float* yj) {"],
         c_adjoint=["  __device__ static void jump_vjp(const float* y, const float* p, const float* yjb, float* yb, float* pb) {"],
         excludes_neural="state jump", none_resets=True, checks_arguments=True,
         note=": it sees the species at one time point (the left limit), the effective parameters and the treatments -- no t "
              "(or None in a subclass, for no jump)"),
)
# process noise: called once per step of the scheme (every sub-step), on the step's start state -- not once per time point, so it
# is a record of its own beside HOOKS, as the start map is (TRACED_HOOKS, below, is what tracing, code generation and the capture
# of the definitions walk); sees the species, the effective parameters and the treatments -- no t; a forcing reads the sample of
# the interval's first point, as jump does.  It returns one noise amplitude per species; one that folds to the constant 0 is not
# written, draws nothing and has no adjoint (skips_zero: the struct's NOISE_MASK says which are left)
DIFFUSION_HOOK = \
    Hook("diffusion", signature="diffusion(self, y, p, c)", groups=("y",),
         outputs="the noise amplitude of each species, one value per species; 0.0 for a species without noise",
         n_outputs="species", attr="_diffusion_def", traced="dif", c_out="g", seed="gb",
         switch="HAS_DIFFUSION", switch_note="process noise, u' = Phi_h(u) + g(u) sqrt(h) xi per step: diffusion / diffusion_vjp (vihds_sde.hpp)",
         c_forward=["  __device__ static void diffusion(const float* y, const float* p, float* g) {"],
         c_adjoint=["  __device__ static void diffusion_vjp(const float* y, const float* p, const float* gb, float* yb, float* pb) {"],
         excludes_neural="process noise", none_resets=True, checks_arguments=True, skips_zero=True,
         note=": it sees the species at a step's start, the effective parameters and the treatments -- no t "
              "(or None in a subclass, for no process noise)")

# reaction-channel noise: the other form of the scheme's noise term, called where diffusion is (a class has one of the two).  It
# returns one list per declared channel (noise_channels), each with one amplitude per species: entry [r][q] is G[q][r], the
# amplitude with which the Wiener process of channel r enters species q.  The traced outputs are the flat list G[q * R + r]; an
# entry that folds to the constant 0 is a structural zero (skips_zero: not written, no draw, no adjoint), and the struct's
# channel_species(r) says which species channel r enters
CHANNEL_NOISE_HOOK = \
    Hook("channel_noise", signature="channel_noise(self, y, p, c)", groups=("y",),
         outputs="one list per noise channel, each with the amplitude of that channel in every species; 0.0 where it does not enter",
         n_outputs="channels", attr="_channel_noise_def", traced="chan", c_out="G", seed="Gb",
         switch="HAS_DIFFUSION", switch_note="process noise by reaction channels, u' = Phi_h(u) + G(u) sqrt(h) xi per step: channel_noise / channel_noise_vjp (vihds_sde.hpp)",
         c_forward=["  __device__ static void channel_noise(const float* y, const float* p, float* G) {"],
         c_adjoint=["  __device__ static void channel_noise_vjp(const float* y, const float* p, const float* Gb, float* yb, float* pb) {"],
         excludes_neural="process noise", none_resets=True, checks_arguments=True, skips_zero=True,
         note=": it sees the species at a step's start, the effective parameters and the treatments -- no t "
              "(or None in a subclass, for no channel noise)")

ALL_HOOKS = (START_HOOK,) + HOOKS  # in the order in which the forward kernel calls them
TRACED_HOOKS = ALL_HOOKS + (DIFFUSION_HOOK,)  # ... and the hook of the scheme's step behind them
# ... and its channel form: what tracing, code generation and the capture of the definitions walk (the three tuples above are
# pinned by earlier tests as they stand)
MODEL_HOOKS = TRACED_HOOKS + (CHANNEL_NOISE_HOOK,)
NOISE_HOOKS = (DIFFUSION_HOOK, CHANNEL_NOISE_HOOK)  # the two forms of process noise
HOOK = {h.name: h for h in MODEL_HOOKS}


def _class_noise_channels(cls):
    return list(getattr(cls, "noise_channels", None) or ())


def _channel_entries(cls, g, out, N):
    """What channel_noise returned -- one list per declared channel, each with one amplitude per species -- as the flat list of
    nodes G[q * R + r] (species q, channel r), checked: the number of channels, the entries per channel, no channel without a
    species, at most MAX_NOISE_ENTRIES entries that are not the constant 0."""
    names = _class_noise_channels(cls)
    R = len(names)
    if not isinstance(out, (list, tuple)) or len(out) != R:
        raise ModelDefinitionError("%s.channel_noise must return a list of %d lists, one per noise channel (%s), and returned %s"
                                   % (cls.__name__, R, ", ".join(names),
                                      "%d" % len(out) if isinstance(out, (list, tuple)) else type(out).__name__))
    for r, col in enumerate(out):
        if not isinstance(col, (list, tuple)) or len(col) != N:
            raise ModelDefinitionError("%s.channel_noise: channel '%s' must be a list of %d entries, the amplitude with which it "
                                       "enters each species (0.0 where it does not), and is %s"
                                       % (cls.__name__, names[r], N,
                                          "a list of %d" % len(col) if isinstance(col, (list, tuple)) else type(col).__name__))
    G = [g._arg(out[r][q]) for q in range(N) for r in range(R)]
    for r in range(R):
        if all(_is_const(G[q * R + r], 0.0) for q in range(N)):
            raise ModelDefinitionError("%s.channel_noise: channel '%s' enters no species (every entry folds to the constant 0): a "
                                       "channel without a species draws for nothing -- remove it from noise_channels"
                                       % (cls.__name__, names[r]))
    nz = sum(1 for e in G if not _is_const(e, 0.0))
    if nz > MAX_NOISE_ENTRIES:
        raise ModelDefinitionError("%s.channel_noise has %d entries that are not the constant 0: every one is an amplitude held in a "
                                   "register across the scheme's step, at most %d (MAX_NOISE_ENTRIES)"
                                   % (cls.__name__, nz, MAX_NOISE_ENTRIES))
    return G


class Trace(object):
    """The functions of a model class (prepare, initial_state, rhs and, when defined, start, observe, precision, log_likelihood
    and jump) traced into one Graph."""

    def __init__(self, cls):
        inst = cls.__new__(cls)  # (the functions are methods; nothing of nn.Module is touched by them)
        self.cls = cls
        self.networks = _class_networks(cls)
        self.g = g = Graph(self.networks.values())
        self._phase, self._called = "prepare", {}

        def call(k, name, net, inputs):
            if self._phase != "rhs":
                raise ModelDefinitionError("network '%s' called from %s: networks are evaluated in rhs only (not in "
                                           "prepare, initial_state, observe or precision, nor in log_likelihood, jump, start or steady_rate)" % (name, self._phase))
            if name in self._called:
                raise ModelDefinitionError("network '%s' is called twice: a network may be called at most once per rhs "
                                           "evaluation (its adjoint dump has one slot per evaluation)" % name)
            self._called[name] = True
            return g.net(k, inputs)

        object.__setattr__(inst, "net", _Networks(cls, call))
        self.forcings = _class_forcings(cls)

        def read(k, name):
            if self._phase in ("prepare", "initial_state"):
                raise ModelDefinitionError(
                    "forcing '%s' read in %s: a forcing changes over the experiment, and %s is evaluated once, before the "
                    "first time point -- forcings are read in rhs (the interpolant at the stage time), observe, precision, "
                    "log_likelihood and jump (the sample of the time point) and in start (the first sample)"
                    % (name, self._phase, self._phase))
            return g.leaf("f", k)

        object.__setattr__(inst, "forcing", _Forcings(cls, read))
        self.algebraic = _class_algebraic(cls)

        def read_z(i, name):
            if self._phase not in _ALGEBRAIC_READERS:
                _algebraic_misread(name, self._phase)
            return g.leaf("z", i)

        object.__setattr__(inst, "algebraic", _Algebraic(cls, read_z))
        self.delays = _class_delays(cls)

        def read_d(e, name):
            if self._phase != "rhs":
                _delay_misread(name, self._phase)
            return g.leaf("d", e)

        object.__setattr__(inst, "delayed", _Delayed(cls, read_d))
        N, P, C = len(cls.species), list(cls.parameter_names), int(cls.n_conditions)
        th = _Named([(n, g.leaf("th", s)) for s, n in enumerate(P)], "parameter")
        cs = [g.leaf("c", q) for q in range(C)]
        prepared = inst.prepare(th, _Conditions(cs))
        if not isinstance(prepared, dict) or not all(isinstance(k, str) for k in prepared):
            raise ModelDefinitionError("%s.prepare must return a dict {name: value}" % cls.__name__)
        self.p_names = list(prepared)
        self.p_exprs = [g._arg(prepared[k]) for k in self.p_names]
        for name, _sp, par in self.delays:
            if par not in self.p_names:
                raise ModelDefinitionError("%s.delays: '%s' names the delay '%s', which is no effective parameter (prepare "
                                           "returns: %s)" % (cls.__name__, name, par, ", ".join(self.p_names)))
        self._phase = "initial_state"
        y0 = inst.initial_state(th, _Conditions(cs))
        self.y0 = self._state_list(y0, "initial_state", N)
        self._phase = "rhs"
        # rhs sees the effective parameters and the treatments; the kernel's rhs has no c[], so each treatment it reads is
        # one more effective parameter (copied by prepare, no adjoint)
        NPU = len(self.p_names)
        p = _Named([(n, g.leaf("p", k)) for k, n in enumerate(self.p_names)], "effective parameter")
        # the algebraic variables: the start of the iteration and the constraint, which see the species, the effective
        # parameters, the treatments and the forcings -- no t (a class without them traces nothing here)
        self.z0 = self.con = None
        M = len(self.algebraic)
        if M:
            ys, cz = [g.leaf("y", j) for j in range(N)], _Conditions([g.leaf("p", NPU + q) for q in range(C)])
            self._phase = "algebraic_start"
            self.z0 = self._unknown_list(inst.algebraic_start(ys, p, cz), "algebraic_start", M)
            self._phase = "constraint"
            self.con = self._unknown_list(inst.constraint(ys, [g.leaf("z", i) for i in range(M)], p, cz), "constraint", M)
            self._phase = "rhs"
        self.dy = self._state_list(inst.rhs(g.leaf("t", 0), [g.leaf("y", j) for j in range(N)], p,
                                            _Conditions([g.leaf("p", NPU + q) for q in range(C)])), "rhs", N)
        reached = {n.val for n in _topo(self.dy) if n.op == "net"}
        for k, name in enumerate(self.networks):
            if k not in reached:
                raise ModelDefinitionError("%s: network '%s' is declared but %s" % (
                    cls.__name__, name, "no derivative depends on its outputs" if name in self._called
                    else "never called in rhs"))
        # the hooks (optional) see their groups of leaves, the effective parameters and the treatments
        self.n_channels = 0  # (noise channels: the R of channel_noise's R x N entries)
        for h in MODEL_HOOKS:
            setattr(self, h.traced, None)
            definition = getattr(cls, h.attr, None)
            if definition is not None:
                self._phase = h.name
                out = definition(inst, *[[g.leaf(k, j) for j in range(N if k == "y" else 4)] for k in h.groups], p,
                                 _Conditions([g.leaf("p", NPU + q) for q in range(C)]))
                if h.n_outputs == "channels":
                    out = _channel_entries(cls, g, out, N)
                    self.n_channels = len(out) // N
                elif not isinstance(out, (list, tuple)) or len(out) != h.count(N):
                    raise ModelDefinitionError("%s.%s must return a list of %d entries (%s)"
                                               % (cls.__name__, h.name, h.count(N), h.outputs))
                setattr(self, h.traced, [g._arg(x) for x in out])
        # the steady species: steady_rate, traced last (a class without them traces nothing here and keeps the numbering of its
        # nodes).  It sees what start sees -- no t, no network call, a forcing's first sample; a self.rhs(...) it calls is traced
        # in its phase, so whatever that rhs does that steady_rate may not do raises here and names steady_rate
        self.steady, self.srate = _class_steady(cls), None
        if self.steady:
            self._phase = "steady_rate"
            out = inst.steady_rate([g.leaf("y", j) for j in range(N)], p, _Conditions([g.leaf("p", NPU + q) for q in range(C)]))
            if not isinstance(out, (list, tuple)) or len(out) != len(self.steady):
                raise ModelDefinitionError("%s.steady_rate must return a list of %d entries (one residual per steady species: %s)"
                                           % (cls.__name__, len(self.steady), ", ".join(self.steady)))
            self.srate = [g._arg(x) for x in out]
            bad = sorted({n.op for n in _topo(self.srate) if n.op in ("t", "net", "z", "d", "dt")})
            if bad:
                raise ModelDefinitionError("%s.steady_rate reads %s: it sees the species, the effective parameters, the treatments "
                                           "and the forcings' first samples only" % (cls.__name__, ", ".join(bad)))
        used = {n.val for n in _topo(self.dy + [x for h in MODEL_HOOKS for x in getattr(self, h.traced) or []]
                                     + (self.z0 or []) + (self.con or []) + (self.srate or [])) if n.op == "p"}
        self.c_in_rhs = [q for q in range(C) if NPU + q in used]  # (read by rhs, by observe, by precision or by log_likelihood)
        # remap the treatments rhs / observe / precision read to consecutive parameter indices behind the named ones
        self.NP = NPU + len(self.c_in_rhs)
        self.c_slot = {NPU + q: NPU + k for k, q in enumerate(self.c_in_rhs)}
        # the forcings' entries of p follow: K values, K slopes, one interval start (the struct's set_interval / set_point)
        self.F0 = self.NP
        # ... and the delayed reads' behind them: E values, E slopes, one interval start (the struct's set_delay)
        self.D0 = self.F0 + (2 * len(self.forcings) + 1 if self.forcings else 0)

    def _unknown_list(self, v, what, M):
        if not isinstance(v, (list, tuple)) or len(v) != M:
            raise ModelDefinitionError("%s.%s must return a list of %d entries (one per algebraic variable: %s)"
                                       % (self.cls.__name__, what, M, ", ".join(self.algebraic)))
        return [self.g._arg(x) for x in v]

    def _state_list(self, v, what, N):
        if not isinstance(v, (list, tuple)) or len(v) != N:
            raise ModelDefinitionError("%s.%s must return a list of %d entries (one per species)" % (self.cls.__name__, what, N))
        return [self.g._arg(x) for x in v]


# ---------------------------------------------------------------------------------------------------------------------
# code generation
# ---------------------------------------------------------------------------------------------------------------------
def _lit(v):
    f = float(np.float32(v))
    if math.isnan(f): return "__builtin_nanf(\"\")"
    if math.isinf(f): return "__builtin_inff()" if f > 0 else "(-__builtin_inff())"
    s = repr(f)
    if "e" not in s and "." not in s:
        s += ".0"
    return s + "f"


class _Emitter(object):
    """Straight-line C++ for some DAG outputs: one `const float` per operation node (`const bool` per condition).  fast=True
    is the time loop (frcp, fdiv, fexp, sigmoid_f, ftanh, fsqrt); fast=False is prepare / init (IEEE division, expf, tanhf,
    sqrtf); both use powf / logf / erff / erfcf and the selects of vihds_models.hpp (fsel, fmin_nan, fmax_nan and their
    pass weights, fsign): no branch is ever emitted."""

    def __init__(self, fast, leaf_names, p_map=None):
        self.fast, self.leaf_names, self.p_map = fast, leaf_names, p_map or {}
        self.lines, self.names = [], {}

    def ref(self, n):
        if n.op == "const": return _lit(n.val)
        if n.op == "f":  # (a forcing: the text of its value where this function is evaluated)
            return self.leaf_names["f"][n.val]
        if n.op == "d":  # (a delayed read: the chord of the interval at the stage time)
            return self.leaf_names["d"][n.val]
        if n.op == "dt":
            return self.leaf_names["dt"]
        if n.op in _LEAVES:
            base = self.leaf_names[n.op]
            idx = self.p_map.get(n.val, n.val) if n.op == "p" else n.val
            return base if n.op == "t" else "%s[%d]" % (base, idx)
        return self.names[n.id]

    def expr(self, n):
        rec, a = OP_TABLE[n.op], [self.ref(x) for x in n.args]
        text = rec.peephole(n, a, self.fast) if rec.peephole else None
        if text is None:
            text = rec.c[0 if self.fast else 1] % tuple(a + [_lit(v) for v in (n.val if rec.val else ())])
        return text

    def emit(self, assignments):
        """assignments: [(lhs, '=' or '+=', node)] -> body lines."""
        for n in _topo([x for _, _, x in assignments]):
            if n.op in _LEAVES or n.id in self.names:
                continue
            if n.op in ("net", "netout", "netbwd", "netbwd_in"):
                self._emit_net(n)
                continue
            name = "v%d" % len(self.names)
            self.lines.append("    const %s %s = %s;" % ("bool" if isinstance(n, Cond) else "float", name, self.expr(n)))
            self.names[n.id] = name
        for lhs, how, n in assignments:
            self.lines.append("    %s %s %s;" % (lhs, how, self.ref(n)))
        return self.lines

    def _emit_net(self, n):
        """Network nodes: the call nodes become one call of the struct's net<k>_forward / net<k>_vjp on small register arrays,
        the output / input-adjoint nodes are elements of those arrays."""
        k = n.val if n.op in ("net", "netbwd") else n.args[0].val
        if n.op == "netout":
            self.names[n.id] = "n%d_o[%d]" % (k, n.val)
        elif n.op == "netbwd_in":
            self.names[n.id] = "n%d_xb[%d]" % (k, n.val)
        else:
            I, _H, O = n.g.networks[k].sizes
            refs = [self.ref(x) for x in n.args]
            if n.op == "net":
                self.lines += ["    const float n%d_x[%d] = {%s};" % (k, I, ", ".join(refs)),
                               "    float n%d_o[%d];" % (k, O),
                               "    net%d_forward(w, n%d_x, n%d_o);" % (k, k, k)]
            else:
                self.lines += ["    const float n%d_bx[%d] = {%s};" % (k, I, ", ".join(refs[:I])),
                               "    const float n%d_ob[%d] = {%s};" % (k, O, ", ".join(refs[I:])),
                               "    float n%d_xb[%d];" % (k, I),
                               "    net%d_vjp<Ctx::DUMP>(w, n%d_bx, n%d_ob, n%d_xb, D, fs);" % (k, k, k, k)]
            self.names[n.id] = "n%d" % k


def _network_functions(networks):
    """net<k>_forward / net<k>_vjp of every network as struct members: the hidden layer one unit at a time (register use
    does not grow with n_hidden), the weights by uniform index through the constant address space (scalar loads)."""
    out, w0, f0 = [], 0, 0
    for k, net in enumerate(networks):
        I, H, O = net.sizes
        act = "fmaxf(z, 0.f)" if net.hidden == "relu" else "ftanh(z)"
        dact = "(z > 0.f ? hub : 0.f)" if net.hidden == "relu" else "hub * (1.f - hu * hu)"
        head = ["    const weights_ptr W1 = w + %d, b1 = W1 + %d, W2 = b1 + %d, b2 = W2 + %d;" % (w0, H * I, H, O * H)]
        unit = ["      float z = b1[u];",
                "      VIHDS_UNROLL for (int i = 0; i < %d; ++i) z = fmaf(W1[u * %d + i], x[i], z);" % (I, I),
                "      const float hu = %s;" % act]
        out += [
            "  // network %d: %d -> %d (%s) -> %d; weights at %d (W1 [%d][%d], b1, W2 [%d][%d], b2), dump fields from %d" % (
                k, I, H, net.hidden, O, w0, H, I, O, H, f0),
            "  __device__ static void net%d_forward(weights_ptr w, const float* x, float* o) {" % k,
            "    __asm__ volatile(\"\" ::: \"memory\");  // keep the weight loads inside the time loop (no hoist-and-spill)",
        ] + head + [
            "    VIHDS_UNROLL for (int j = 0; j < %d; ++j) o[j] = b2[j];" % O,
            "    _Pragma(\"nounroll\") for (int u = 0; u < %d; ++u) {" % H,
        ] + unit + [
            "      VIHDS_UNROLL for (int j = 0; j < %d; ++j) o[j] = fmaf(W2[j * %d + u], hu, o[j]);" % (O, H),
            "    }",
            "  }",
            "  // input adjoint xb; DUMP: fields x [%d] | hidden pre-activation adjoints [%d] | hidden activations [%d] | output" % (I, H, H),
            "  // adjoints [%d] of this evaluation (D = its first float, fs = floats between fields)" % O,
            "  template <bool DUMP>",
            "  __device__ static void net%d_vjp(weights_ptr w, const float* x, const float* ob, float* xb, float* D, size_t fs) {" % k,
            "    __asm__ volatile(\"\" ::: \"memory\");",
        ] + head + [
            "    VIHDS_UNROLL for (int i = 0; i < %d; ++i) xb[i] = 0.f;" % I,
            "    if constexpr (DUMP) {",
            "      VIHDS_UNROLL for (int i = 0; i < %d; ++i) D[(size_t)(%d + i) * fs] = x[i];" % (I, f0),
            "      VIHDS_UNROLL for (int j = 0; j < %d; ++j) D[(size_t)(%d + j) * fs] = ob[j];" % (O, f0 + I + 2 * H),
            "    }",
            "    _Pragma(\"nounroll\") for (int u = 0; u < %d; ++u) {" % H,
        ] + unit + [
            "      float hub = 0.f;",
            "      VIHDS_UNROLL for (int j = 0; j < %d; ++j) hub = fmaf(W2[j * %d + u], ob[j], hub);" % (O, H),
            "      const float zub = %s;" % dact,
            "      VIHDS_UNROLL for (int i = 0; i < %d; ++i) xb[i] = fmaf(W1[u * %d + i], zub, xb[i]);" % (I, I),
            "      if constexpr (DUMP) {",
            "        D[(size_t)(%d + u) * fs] = zub;" % (f0 + I),
            "        D[(size_t)(%d + u) * fs] = hu;" % (f0 + I + H),
            "      }",
            "    }",
            "  }",
        ]
        w0 += net.n_weights
        f0 += net.n_fields
    return out


def jacobian_nodes(cls):
    """The Jacobian of rhs as DAG nodes, row by row: J[i][j] = d dy_i / d y_j, by reverse mode with constant one-hot seeds
    (one vjp per row; nothing of vjp is special to it).  A structural zero is the constant 0."""
    tr = cls._trace
    g, N = tr.g, len(cls.species)
    rows = []
    for i in range(N):
        adj = vjp(g, tr.dy, [1.0 if k == i else 0.0 for k in range(N)])
        rows.append([adj.get(g.leaf("y", j).id, g.const(0.0)) for j in range(N)])
    return rows


def jacobian_pattern(cls):
    """[N][N] bools: the entries of the Jacobian that are not structurally zero."""
    return [[not _is_const(e, 0.0) for e in row] for row in jacobian_nodes(cls)]


def constraint_jacobian_nodes(cls):
    """dg/dz of the class's constraint as DAG nodes, row by row: A[i][j] = d g_i / d z_j, by reverse mode with constant one-hot
    seeds (as jacobian_nodes does for rhs).  A structural zero is the constant 0."""
    tr = cls._trace
    g, M = tr.g, len(tr.algebraic)
    rows = []
    for i in range(M):
        adj = vjp(g, tr.con, [1.0 if k == i else 0.0 for k in range(M)])
        rows.append([adj.get(g.leaf("z", j).id, g.const(0.0)) for j in range(M)])
    return rows


def constraint_pattern(cls):
    """[M][M] bools: the entries of dg/dz that are not structurally zero."""
    return [[not _is_const(e, 0.0) for e in row] for row in constraint_jacobian_nodes(cls)]


def _check_constraint_pattern(cls):
    """A structurally singular dg/dz is refused when the class is defined: an unknown no residual depends on, a residual that
    depends on no unknown, and -- the elimination has no pivot search -- a pivot that is a structural zero after fill-in."""
    names, pat = _class_algebraic(cls), [list(r) for r in constraint_pattern(cls)]
    M = len(names)
    for j in range(M):
        if not any(pat[i][j] for i in range(M)):
            raise ModelDefinitionError("%s.constraint: no residual depends on the algebraic variable '%s' -- dg/dz has a zero "
                                       "column and is structurally singular" % (cls.__name__, names[j]))
    for i in range(M):
        if not any(pat[i]):
            raise ModelDefinitionError("%s.constraint: residual %d depends on no algebraic variable -- dg/dz has a zero row and "
                                       "is structurally singular" % (cls.__name__, i))
    for k in range(M):
        if not pat[k][k]:
            raise ModelDefinitionError(
                "%s.constraint: residual %d does not depend on the algebraic variable '%s' (not even after the elimination's "
                "fill-in) -- the solve eliminates without a pivot search, so pivot %d would be a structural zero: order the "
                "residuals so that residual i depends on unknown i" % (cls.__name__, k, names[k], k))
        for i in range(k + 1, M):
            if pat[i][k]:
                for j in range(k + 1, M):
                    pat[i][j] = pat[i][j] or pat[k][j]


def steady_jacobian_nodes(cls):
    """J = d steady_rate / d y_E of the class as DAG nodes, row by row: J[i][j] = d F_i / d y[steady species j], by reverse mode
    with constant one-hot seeds (as jacobian_nodes does for rhs).  A structural zero is the constant 0."""
    tr = cls._trace
    g, M = tr.g, len(tr.steady)
    idx = [list(cls.species).index(s) for s in tr.steady]
    rows = []
    for i in range(M):
        adj = vjp(g, tr.srate, [1.0 if k == i else 0.0 for k in range(M)])
        rows.append([adj.get(g.leaf("y", j).id, g.const(0.0)) for j in idx])
    return rows


def steady_pattern(cls):
    """[M][M] bools: the entries of d steady_rate / d y_E that are not structurally zero."""
    return [[not _is_const(e, 0.0) for e in row] for row in steady_jacobian_nodes(cls)]


def _check_steady_pattern(cls):
    """A structurally singular J is refused when the class is defined, as _check_constraint_pattern does for dg/dz: a steady
    species no residual depends on, a residual that depends on no steady species, and -- the adjoint's elimination has no pivot
    search -- a pivot that is a structural zero after fill-in."""
    names, pat = _class_steady(cls), [list(r) for r in steady_pattern(cls)]
    M = len(names)
    for j in range(M):
        if not any(pat[i][j] for i in range(M)):
            raise ModelDefinitionError("%s.steady_rate: no residual depends on the steady species '%s' -- d steady_rate / d y_E "
                                       "has a zero column and is structurally singular" % (cls.__name__, names[j]))
    for i in range(M):
        if not any(pat[i]):
            raise ModelDefinitionError("%s.steady_rate: residual %d depends on no steady species -- d steady_rate / d y_E has a "
                                       "zero row and is structurally singular" % (cls.__name__, i))
    for k in range(M):
        if not pat[k][k]:
            raise ModelDefinitionError(
                "%s.steady_rate: residual %d does not depend on the steady species '%s' (not even after the elimination's "
                "fill-in) -- the solve eliminates without a pivot search, so pivot %d would be a structural zero: order the "
                "residuals so that residual i depends on steady species i" % (cls.__name__, k, names[k], k))
        for i in range(k + 1, M):
            if pat[i][k]:
                for j in range(k + 1, M):
                    pat[i][j] = pat[i][j] or pat[k][j]


def _leaf_free(node, allowed):
    return all(n.op not in _LEAVES or n.op == "const" or n.op in allowed for n in _topo([node]))


def generate_source(cls, neural=False):
    """The C++ header of one model: the struct of the vihds_models.hpp contract (adjoints by reverse mode, forward values
    recomputed inside them) and the switches csrc/generated/ode_generated_model.hip reads.  Deterministic: the same
    definition gives byte-identical text; its hash (with the kernel headers') names the library."""
    tr = cls._trace
    for h in MODEL_HOOKS:
        if neural and h.excludes_neural and getattr(tr, h.traced) is not None:
            raise ModelDefinitionError("%s defines %s: a model with a %s of its own does not take NeuralPrecisions"
                                       % (cls.__name__, h.signature, h.excludes_neural))
    if neural and cls.implicit:
        raise ModelDefinitionError("%s has implicit = True: the precision ODE of NeuralPrecisions has no generated Jacobian, so an "
                                   "implicit model takes constant precisions or a precision map of its own" % cls.__name__)
    if neural and cls.step_tolerance is not None:
        raise ModelDefinitionError("%s has step_tolerance = %r: the adjoint's dump of the precision network holds one evaluation "
                                   "per stage and observation interval, and the count row is the last row of a trajectory whose "
                                   "precision states WithPrec<> integrates -- a model with step control takes constant precisions "
                                   "or a precision map of its own" % (cls.__name__, cls.step_tolerance))
    if neural and cls.substeps > 1:
        raise ModelDefinitionError("%s has substeps = %d: the adjoint's dump of the precision network holds one evaluation per "
                                   "stage and observation interval, so a sub-stepped model takes constant precisions or a "
                                   "precision map of its own" % (cls.__name__, cls.substeps))
    if neural and cls.lead_in > 0:
        raise ModelDefinitionError("%s has lead_in = %r: the adjoint's dump of the precision network holds one evaluation per "
                                   "stage and observation interval, so a model with a lead-in phase does not take "
                                   "NeuralPrecisions (constant precisions, or a precision map of its own)"
                                   % (cls.__name__, cls.lead_in))
    if neural and tr.algebraic:
        raise ModelDefinitionError("%s declares algebraic variables: WithPrec<> evaluates the precision ODE beside a rhs that has no "
                                   "unknowns, so a model with algebraic variables does not take NeuralPrecisions (constant "
                                   "precisions, or a precision map of its own)" % cls.__name__)
    if neural and tr.delays:
        raise ModelDefinitionError("%s declares delays: WithPrec<> forwards neither the reserved slots nor set_delay, so a model "
                                   "with delayed reads does not take NeuralPrecisions (constant precisions, or a precision map "
                                   "of its own)" % cls.__name__)
    if neural and tr.steady:
        raise ModelDefinitionError("%s declares steady_species: WithPrec<> does not forward steady / steady_vjp, so a model with "
                                   "steady species does not take NeuralPrecisions (constant precisions, or a precision map of "
                                   "its own)" % cls.__name__)
    g = tr.g
    N, P, C = len(cls.species), list(cls.parameter_names), int(cls.n_conditions)
    NPU = len(tr.p_names)
    obs_enum = HOOK["observe"].switch if tr.obs is not None else OBSERVE_KINDS[cls.observe_kind][0]
    sname = "GenModel_" + _ident(cls.model_key)

    def pull(adj, targets):
        """`target[j] += adjoint of leaf j` for the leaves of each (leaf kind, adjoint array) that the outputs depend on;
        of p only the named effective parameters (a treatment has no adjoint)."""
        return [("%s[%d]" % (target, j), "+=", adj[g.leaf(kind, j).id])
                for kind, target in targets for j in range({"y": N, "p": NPU}.get(kind, 4)) if g.leaf(kind, j).id in adj]

    # prepare: named parameters, then the treatments rhs reads
    prep = [("p[%d]" % k, "=", e) for k, e in enumerate(tr.p_exprs)]
    prep += [("p[%d]" % (NPU + k), "=", g.leaf("c", q)) for k, q in enumerate(tr.c_in_rhs)]
    # prepare_vjp: overwrites every slot (a slot prepare does not read gets 0)
    pb = [g.leaf("seed", k) for k in range(NPU)]
    adj = vjp(g, tr.p_exprs, pb)
    prep_vjp = [("thb[%d]" % s, "=", adj.get(g.leaf("th", s).id, g.const(0.0))) for s in range(len(P))]
    # init / init_vjp: the kernel calls init_vjp(yb, thb) after prepare_vjp, without theta or treatments -- so it adds,
    # and the initial state must be affine in theta with constant coefficients (it is a copy in every reference model)
    init = [("y[%d]" % j, "=", e) for j, e in enumerate(tr.y0)]
    yb = [g.leaf("seed", j) for j in range(N)]
    adj0 = vjp(g, tr.y0, yb)
    init_vjp = []
    for s in range(len(P)):
        e = adj0.get(g.leaf("th", s).id)
        if e is None:
            continue
        if not _leaf_free(e, ("seed",)):
            raise ModelDefinitionError(
                "%s.initial_state: the derivative with respect to '%s' depends on theta or the treatments; the kernels' "
                "init_vjp sees the state adjoint only, so the initial state must be affine in the parameters with constant "
                "coefficients (move nonlinear maps into prepare... or into a parameter of its own; where, minimum, maximum, "
                "abs and sqrt of a parameter or a treatment are such maps: a condition on theta is refused here too); a "
                "nonlinear start -- a steady state, a ratio of rates, a where on a treatment -- goes into start(self, y, p, c), "
                "which maps what initial_state returns and reads the effective parameters"
                % (cls.__name__, P[s]))
        init_vjp.append(("thb[%d]" % s, "+=", e))
    # rhs / rhs_vjp
    rhs = [("dy[%d]" % j, "=", e) for j, e in enumerate(tr.dy)]
    v = [g.leaf("seed", j) for j in range(N)]
    adj1 = vjp(g, tr.dy, v)
    rhs_vjp = pull(adj1, [("y", "yb"), ("p", "pb")])
    # delayed reads: entries D0 .. of p hold E values, E slopes and the interval start (set_delay); rhs reads the chord at its
    # stage time, and -- unlike a forcing -- the read has an adjoint: rhs_vjp adds it to pb of the value and the slope entry
    E, D0 = len(tr.delays), tr.D0
    d_at_t = ["(p[%d] + (t - p[%d]) * p[%d])" % (D0 + e, D0 + 2 * E, D0 + E + e) for e in range(E)]
    for e in range(E):
        db = adj1.get(g.leaf("d", e).id)
        if db is not None:
            rhs_vjp += [("pb[%d]" % (D0 + e), "+=", db), ("pb[%d]" % (D0 + E + e), "+=", db * g.leaf("dt", 0))]

    # forcings: entries F0 .. of p hold K values, K slopes and the interval start; rhs (and its adjoint) reads the interpolant
    # at its stage time, a hook the value (set_point: the sample of the time point)
    K, F0 = len(tr.forcings), tr.F0
    f_at_t = ["(p[%d] + (t - p[%d]) * p[%d])" % (F0 + k, F0 + 2 * K, F0 + K + k) for k in range(K)]
    f_at_point = ["p[%d]" % (F0 + k) for k in range(K)]

    def body(assign, fast, seed, p_map=None, forcing=None):
        names = {"th": "th", "c": "c", "y": "y", "p": "p", "t": "t", "seed": seed, "x": "xp", "ob": "ob", "pr": "pr",
                 "f": forcing, "z": "z", "d": d_at_t, "dt": "(t - p[%d])" % (D0 + 2 * E)}
        return "\n".join(_Emitter(fast, names, p_map).emit(assign))

    # algebraic variables: a member that reads them opens with the solve, its adjoint repeats the solve and closes with the mu
    # step (csrc/vihds_algebraic.hpp).  `u` holds the forcings' values where the member is evaluated
    M = len(tr.algebraic)

    def reads_z(outs):
        return M > 0 and any(n.op == "z" for n in _topo([o for o in outs if isinstance(o, Sym)]))

    def solve_z(forcing):
        head = ["    const float u[%d] = {%s};" % (K, ", ".join(forcing))] if K else ["    const float* u = nullptr;"]
        return head + ["    float z[%d];" % M, "    algebraic(y, p, u, z);"]

    def pull_z(adj):
        return [("zb[%d]" % i, "=", adj.get(g.leaf("z", i).id, g.const(0.0))) for i in range(M)]

    names = ", ".join('"%s"' % n for n in P)
    key = cls.model_key
    nets = list(tr.networks.values())
    NW = sum(net.n_weights for net in nets)
    if nets:
        rhs_sig = ["  __device__ static void rhs(float t, const float* y, const float* p, const float* wg, float* dy) {",
                   "    const weights_ptr w = (weights_ptr)wg;"]
        # (Ctx: the adjoint kernel's context; Ctx::DUMP says whether this launch collects the weight gradient)
        vjp_sig = ["  template <class Ctx>",
                   "  __device__ static void rhs_vjp(float t, const float* y, const float* p, const float* wg, const float* v, float* yb,",
                   "                                 float* pb, Ctx& ctx) {",
                   "    const weights_ptr w = (weights_ptr)wg;",
                   "    float* D = nullptr;",
                   "    size_t fs = 0;",
                   "    if constexpr (Ctx::DUMP) {",
                   "      D = ctx.net_dump + (size_t)ctx.net_e * ctx.n;",
                   "      fs = ctx.fstride;",
                   "      ctx.net_e += 1;",
                   "    }"]
        net_decl = ["  static constexpr int NET_FIELDS = %d;  // floats the adjoint dumps per evaluation and trajectory" % sum(
            net.n_fields for net in nets),
                    "  typedef const __attribute__((address_space(4))) float* weights_ptr;"] + _network_functions(nets)
    else:
        rhs_sig = ["  __device__ static void rhs(float t, const float* y, const float* p, const float*, float* dy) {"]
        vjp_sig = ["  __device__ static void rhs_vjp(float t, const float* y, const float* p, const float*, const float* v, float* yb,",
                   "                                 float* pb) {"]
        net_decl = []
    # the hooks a model defines: value and adjoint run once per time point inside the time loop
    hook_decl = []
    for h in MODEL_HOOKS:
        outs = getattr(tr, h.traced)
        if outs is None:
            continue
        kept = [(j, e) for j, e in enumerate(outs) if not (h.skips_zero and _is_const(e, 0.0))]
        if not kept:
            raise ModelDefinitionError("%s.%s returns the constant 0 for every species: a model without noise defines no %s"
                                       % (cls.__name__, h.name, h.name))
        adj = vjp(g, [e for _j, e in kept], [g.leaf("seed", j) for j, _e in kept])
        if h.switch_note:
            hook_decl.append("  static constexpr bool %s = true;  // %s" % (h.switch, h.switch_note))
        if h.n_outputs == "channels":
            # entry j = q * R + r of the flat list: species q, channel r.  channel_species(r): bit q set where the entry is kept
            R, chans = tr.n_channels, _class_noise_channels(cls)
            enters = [sum(1 << (j // R) for j, _e in kept if j % R == r) for r in range(R)]
            hook_decl += [
                "  static constexpr int NOISE_CHANNELS = %d;  // %s: one Wiener process each; G[q * %d + r] is the amplitude of channel r in species q"
                % (R, ", ".join(chans), R),
                "  static constexpr int NOISE_ENTRIES = %d;  // entries of G that are not structurally zero, of %d" % (len(kept), N * R),
                "  // bit q: channel r enters species q (the other entries of G are structural zeros: never written, never read)",
                "  __host__ __device__ static constexpr unsigned channel_species(int r) { return %s; }" % " : ".join(
                    ["r == %d ? 0x%xu" % (r, m) for r, m in enumerate(enters[:-1])] + ["0x%xu" % enters[-1]])]
        elif h.skips_zero:
            hook_decl.append("  static constexpr unsigned NOISE_MASK = 0x%xu;  // bit j: species j has noise (%s)" % (
                sum(1 << j for j, _e in kept), ", ".join(cls.species[j] for j, _e in kept)))
        with_z = reads_z(outs)  # (observe alone may: a class without algebraic variables emits what it emitted before)
        hook_decl += h.c_forward + (solve_z(f_at_point) if with_z else []) + [
            body([("%s[%d]" % (h.c_out, j), "=", e) for j, e in kept], True, h.seed, tr.c_slot, f_at_point), "  }"]
        hook_decl += h.c_adjoint + (solve_z(f_at_point) + ["    float zb[%d];" % M] if with_z else []) + [
            body(pull(adj, h.targets) + (pull_z(adj) if with_z else []), True, h.seed, tr.c_slot, f_at_point)] + (
            ["    algebraic_vjp(y, z, p, u, zb, yb, pb);"] if with_z else []) + ["  }"]
    forcing_decl = []
    if K:
        forcing_decl = [
            "  static constexpr int N_FORCINGS = %d;  // %s: p[%d ..] values, p[%d ..] slopes, p[%d] the interval start" % (
                K, ", ".join(tr.forcings), F0, F0 + K, F0 + 2 * K),
            "  __device__ static void set_interval(float* p, float t_lo, float inv_dt, const float* u_lo, const float* u_hi) {",
        ] + ["    p[%d] = u_lo[%d];" % (F0 + k, k) for k in range(K)] + [
            "    p[%d] = (u_hi[%d] - u_lo[%d]) * inv_dt;" % (F0 + K + k, k, k) for k in range(K)] + [
            "    p[%d] = t_lo;" % (F0 + 2 * K),
            "  }",
            "  __device__ static void set_point(float* p, const float* u) {",
        ] + ["    p[%d] = u[%d];" % (F0 + k, k) for k in range(K)] + [
            "    p[%d] = 0.f;" % (F0 + K + k) for k in range(K)] + [
            "  }",
        ]
    delay_decl = []
    if E:
        sp = [cls.species.index(d[1]) for d in tr.delays]
        tau = [tr.p_names.index(d[2]) for d in tr.delays]
        pick = lambda v: " : ".join(["e == %d ? %d" % (e, x) for e, x in enumerate(v[:-1])] + ["%d" % v[-1]])  # noqa: E731
        delay_decl = [
            "  static constexpr int N_DELAYS = %d;  // %s: p[%d ..] values, p[%d ..] slopes, p[%d] the interval start" % (
                E, ", ".join("%s = %s(t - %s)" % d for d in tr.delays), D0, D0 + E, D0 + 2 * E),
            "  static constexpr int DELAY_SLOT = %d;  // the first reserved entry of p (and of pb: value and slope adjoints)" % D0,
            "  __host__ __device__ static constexpr int delay_species(int e) { return %s; }" % pick(sp),
            "  __host__ __device__ static constexpr int delay_param(int e) { return %s; }  // the delay's entry of p" % pick(tau),
            "  __device__ static void set_delay(float* p, float t_lo, float inv_dt, const float* d_lo, const float* d_hi) {",
        ] + ["    p[%d] = d_lo[%d];" % (D0 + e, e) for e in range(E)] + [
            "    p[%d] = (d_hi[%d] - d_lo[%d]) * inv_dt;" % (D0 + E + e, e, e) for e in range(E)] + [
            "    p[%d] = t_lo;" % (D0 + 2 * E),
            "  }",
        ]
    # implicit = True: the Jacobian of rhs for the Newton step of the implicit solvers and for their adjoint (after everything
    # above, so that the text of rhs and rhs_vjp is what the class generates without it)
    implicit_decl, jac_decl = [], []
    if cls.implicit:
        J = jacobian_nodes(cls)
        nz = [(i, j) for i in range(N) for j in range(N) if not _is_const(J[i][j], 0.0)]
        mask = sum(1 << (i * N + j) for i, j in nz)
        implicit_decl = [
            "  static constexpr int NEWTON = %d;" % int(cls.newton_iterations),
            "  static constexpr unsigned long long JAC_NZ = 0x%xull;  // structural non-zeros of rhs_jac, bit i * N + j: %d of %d" % (
                mask, len(nz), N * N)]
        # implicit_order = 2: the one line the kernels read (vihds_models.hpp implicit_order<>); none at order 1
        if cls.implicit_order == 2:
            implicit_decl += ["  static constexpr int IMPLICIT_ORDER = 2;  // the two-stage SDIRK of vihds_implicit.hpp"]
        jac_decl = ["  // J[i * N + j] = d dy[i] / d y[j]; a structural zero is the literal 0.f",
                    "  __device__ static void rhs_jac(float t, const float* y, const float* p, const float*, float* J) {",
                    body([("J[%d]" % (i * N + j), "=", J[i][j]) for i, j in nz], True, "v", tr.c_slot, f_at_t)]
        jac_decl += ["    J[%d] = 0.f;" % (i * N + j) for i in range(N) for j in range(N) if (i, j) not in nz]
        jac_decl += ["  }"]
    # algebraic variables: the constants, the three traced members (time-loop helpers, like rhs), the constraint's adjoint
    # product and the two members every reader calls; rhs / rhs_vjp open with the solve where rhs reads an unknown
    algebraic_decl, rhs_open, vjp_open, vjp_pull, vjp_close = [], [], [], [], []
    if M:
        A = constraint_jacobian_nodes(cls)
        anz = [(i, j) for i in range(M) for j in range(M) if not _is_const(A[i][j], 0.0)]
        u_names = ["u[%d]" % k for k in range(K)]
        zargs = "const float* y, const float* z, const float* p, const float* u"
        cadj = vjp(g, tr.con, [g.leaf("seed", i) for i in range(M)])
        algebraic_decl = [
            "  static constexpr int N_ALGEBRAIC = %d;  // %s: the unknowns z of constraint(y, z, p) = 0 (vihds_algebraic.hpp)" % (
                M, ", ".join(tr.algebraic)),
            "  static constexpr int ALG_ITER = %d;  // Newton iterations from algebraic_start, a fixed count" % int(cls.algebraic_iterations),
            "  static constexpr unsigned ALG_NZ = 0x%xu;  // structural non-zeros of constraint_jac, bit i * N_ALGEBRAIC + j: %d of %d" % (
                sum(1 << (i * M + j) for i, j in anz), len(anz), M * M),
            "  // u: the forcings' values where the caller is evaluated (rhs: the interpolant at t; observe: the point's sample)",
            "  __device__ static void algebraic_start(const float* y, const float* p, const float* u, float* z) {",
            body([("z[%d]" % i, "=", e) for i, e in enumerate(tr.z0)], True, "v", tr.c_slot, u_names),
            "  }",
            "  __device__ static void constraint(%s, float* G) {" % zargs,
            body([("G[%d]" % i, "=", e) for i, e in enumerate(tr.con)], True, "v", tr.c_slot, u_names),
            "  }",
            "  // A[i * N_ALGEBRAIC + j] = d G[i] / d z[j]; a structural zero is not written (and not read by the solve)",
            "  __device__ static void constraint_jac(%s, float* A) {" % zargs,
            body([("A[%d]" % (i * M + j), "=", A[i][j]) for i, j in anz], True, "v", tr.c_slot, u_names),
            "  }",
            "  // yb, pb += v^T dG/dy, v^T dG/dp (the adjoint passes v = -mu)",
            "  __device__ static void constraint_vjp(%s, const float* v, float* yb, float* pb) {" % zargs,
            body(pull(cadj, [("y", "yb"), ("p", "pb")]), True, "v", tr.c_slot, u_names),
            "  }",
            "  __device__ static void algebraic(const float* y, const float* p, const float* u, float* z) {",
            "    algebraic_start(y, p, u, z);",
            "    algebraic_newton<N_ALGEBRAIC, ALG_ITER, ALG_NZ>(",
            "        z, [&](const float* s, float* G) { constraint(y, s, p, u, G); },",
            "        [&](const float* s, float* A) { constraint_jac(y, s, p, u, A); });",
            "  }",
            "  // zb: the adjoint of z from the reader's reverse mode; A^T mu = zb at the final z, then the constraint's product with -mu",
            "  __device__ static void algebraic_vjp(%s, float* zb, float* yb, float* pb) {" % zargs,
            "    algebraic_adjoint<N_ALGEBRAIC, ALG_NZ>(zb, [&](float* A) { constraint_jac(y, z, p, u, A); });",
            "    constraint_vjp(y, z, p, u, zb, yb, pb);",
            "  }",
        ]
        if reads_z(tr.dy):
            rhs_open = solve_z(f_at_t)
            vjp_open = rhs_open + ["    float zb[%d];" % M]
            vjp_pull = pull_z(adj1)
            vjp_close = ["    algebraic_vjp(y, z, p, u, zb, yb, pb);"]
    # steady species: the constants, the three traced members and the two the time loops call once per trajectory
    # (csrc/vihds_steady.hpp); a forcing is its first sample, as in start.  None without them
    steady_decl = []
    MS = len(tr.steady)
    if MS:
        sidx = [list(cls.species).index(sp) for sp in tr.steady]
        SJ = steady_jacobian_nodes(cls)
        snz = [(i, j) for i in range(MS) for j in range(MS) if not _is_const(SJ[i][j], 0.0)]
        sadj = vjp(g, tr.srate, [g.leaf("seed", i) for i in range(MS)])
        others = [j for j in range(N) if j not in sidx]
        svjp = [("yb[%d]" % j, "+=", sadj[g.leaf("y", j).id]) for j in others if g.leaf("y", j).id in sadj]
        svjp += [("pb[%d]" % k, "+=", sadj[g.leaf("p", k).id]) for k in range(NPU) if g.leaf("p", k).id in sadj]
        put = " ".join("u[%d] = s[%d];" % (j, e) for e, j in enumerate(sidx))
        steady_decl = [
            "  static constexpr int N_STEADY = %d;  // %s: solved for before the first step (vihds_steady.hpp); the other species are held" % (
                MS, ", ".join(tr.steady)),
            "  static constexpr int STEADY_STEPS = %d;  // pseudo-transient iterations from the guess, a fixed count" % int(cls.steady_steps),
            "  static constexpr float STEADY_DELTA0 = %s;  // the first pseudo-time step" % _lit(cls.steady_first_step),
            "  static constexpr float STEADY_GROWTH = %s;  // delta_k+1 = delta_k * STEADY_GROWTH" % _lit(cls.steady_growth),
            "  static constexpr unsigned long long STEADY_NZ = 0x%xull;  // structural non-zeros of steady_jac, bit i * N_STEADY + j: %d of %d" % (
                sum(1 << (i * MS + j) for i, j in snz), len(snz), MS * MS),
            "  __host__ __device__ static constexpr int steady_species(int e) { return %s; }" % " : ".join(
                ["e == %d ? %d" % (e, j) for e, j in enumerate(sidx[:-1])] + ["%d" % sidx[-1]]),
            "  __device__ static void steady_rate(const float* y, const float* p, float* F) {",
            body([("F[%d]" % i, "=", e) for i, e in enumerate(tr.srate)], True, "v", tr.c_slot, f_at_point),
            "  }",
            "  // A[i * N_STEADY + j] = d F[i] / d y[steady_species(j)]; a structural zero is not written (and not read by the solves)",
            "  __device__ static void steady_jac(const float* y, const float* p, float* A) {",
            body([("A[%d]" % (i * MS + j), "=", SJ[i][j]) for i, j in snz], True, "v", tr.c_slot, f_at_point),
            "  }",
            "  // yb (the species that are not steady), pb += v^T dF/dy, v^T dF/dp (the adjoint passes v = -mu)",
            "  __device__ static void steady_rate_vjp(const float* y, const float* p, const float* v, float* yb, float* pb) {",
            body(svjp, True, "v", tr.c_slot, f_at_point),
            "  }",
            "  __device__ static void steady(float* y, const float* p) {",
            "    float u[%d], z[%d] = {%s};" % (N, MS, ", ".join("y[%d]" % j for j in sidx)),
        ] + ["    u[%d] = y[%d];" % (j, j) for j in others] + [
            "    steady_iterate<N_STEADY, STEADY_STEPS, STEADY_NZ>(",
            "        STEADY_DELTA0, STEADY_GROWTH, z,",
            "        [&](const float* s, float* F) { %s steady_rate(u, p, F); }," % put,
            "        [&](const float* s, float* A) { %s steady_jac(u, p, A); });" % put,
        ] + ["    y[%d] = z[%d];" % (j, e) for e, j in enumerate(sidx)] + [
            "  }",
            "  // y: the state steady returned; lam: its adjoint.  J^T mu = lam_E, then steady_rate's product with -mu; lam_E = 0",
            "  __device__ static void steady_vjp(const float* y, const float* p, float* lam, float* pb) {",
            "    float mu[%d] = {%s};" % (MS, ", ".join("lam[%d]" % j for j in sidx)),
            "    steady_adjoint<N_STEADY, STEADY_NZ>(mu, [&](float* A) { steady_jac(y, p, A); });",
        ] + ["    lam[%d] = 0.f;" % j for j in sidx] + [
            "    steady_rate_vjp(y, p, mu, lam, pb);",
            "  }",
        ]
    # substeps = m > 1: the one line the kernels' time loops read (vihds_models.hpp substeps<>); a class without it generates
    # the text it generated before
    substeps_decl = ["  static constexpr int SUBSTEPS = %d;" % int(cls.substeps)] if cls.substeps > 1 else []
    # step_tolerance = (rtol, atol): SUBSTEPS is the ceiling of the ladder, and the two lines the kernels' acceptance test reads
    # (vihds_models.hpp step_control<>, vihds_stepctl.hpp); none without it, likewise
    if cls.step_tolerance is not None:
        substeps_decl += ["  static constexpr float STEP_RTOL = %s;  // step control: 1 -> 2 -> .. -> SUBSTEPS steps per interval, "
                          "each trajectory's own (vihds_stepctl.hpp)" % _lit(cls.step_tolerance[0]),
                          "  static constexpr float STEP_ATOL = %s;" % _lit(cls.step_tolerance[1])]
    # lead_in = L > 0: the two lines the kernels read (vihds_models.hpp lead_in<>); none without it, likewise
    if cls.lead_in > 0:
        substeps_decl += ["  static constexpr int LEAD_STEPS = %d;  // steps of the scheme over [t_0 - LEAD_TIME, t_0], nothing stored"
                          % int(cls.lead_in_steps),
                          "  static constexpr float LEAD_TIME = %s;" % _lit(cls.lead_in)]
    # missing_observations = True: the one line the kernels' scoring points read (vihds_models.hpp masked_obs<>); none without it,
    # likewise
    if cls.missing_observations:
        substeps_decl += ["  static constexpr bool MASKED_OBS = true;  // a row of cond carries one mask word per time point "
                          "(vihds_mask.hpp)"]
    out = [
        "// Generated by vihds.modelgen from %s.%s (model_key %s): the model contract of vihds_models.hpp." % (
            cls.__module__, cls.__qualname__, key),
        "// Do not edit: the definition in Python is the source.",
        "#pragma once",
        "namespace vihds {",
        "struct %s {" % sname,
        "  static constexpr int N = %d;" % N,
        "  static constexpr int NS = %d;" % N,
        "  static constexpr bool NEURAL_PREC = false;",
        "  static constexpr int NW = %d;" % NW,
        "  static constexpr int NC = %d;" % C,
        "  static constexpr int OBS = %s;" % obs_enum,
        "  static constexpr int NSLOT = %d;" % len(P),
        "  static constexpr int NP = %d;" % (D0 + 2 * E + 1 if E else max(tr.NP, 1) if not K else tr.NP + 2 * K + 1),
    ] + substeps_decl + implicit_decl + forcing_decl + delay_decl + net_decl + algebraic_decl + [
        "  __host__ static const char* slot_name(int s) {",
        "    static const char* n[] = {%s};" % names,
        "    return n[s];",
        "  }",
        "  __device__ static void prepare(const float* th, const float* c, float* p) {",
        body(prep, False, "pb", tr.c_slot),
        "  }",
        "  __device__ static void prepare_vjp(const float* th, const float* c, const float* p, const float* pb, float* thb) {",
        body(prep_vjp, False, "pb"),
        "  }",
        "  __device__ static void init(const float* th, const float* c, float* y) {",
        body(init, False, "yb"),
        "  }",
        "  __device__ static void init_vjp(const float* yb, float* thb) {",
        body(init_vjp, False, "yb"),
        "  }",
    ] + rhs_sig + rhs_open + [
        body(rhs, True, "v", tr.c_slot, f_at_t),
        "  }",
    ] + vjp_sig + vjp_open + [
        body(rhs_vjp + vjp_pull, True, "v", tr.c_slot, f_at_t),
    ] + vjp_close + [
        "  }",
    ] + jac_decl + hook_decl + steady_decl + [
        "};",
        "}  // namespace vihds",
        "#define VIHDS_GEN_CORE %s" % sname,
        "#define VIHDS_GEN_NEURAL %d" % (1 if neural else 0),
        "",
    ]
    return "\n".join(line for line in out if line != "") + "\n"


def substep_counts(traj, model):
    """The step counts a model with step control chose (module docstring, "Error-controlled sub-steps"), from a stored trajectory:
    `traj` is the kernels' buffer [T, rows, B, S] (DecodedSolution.traj_buffer) or the solution [B, S, rows, T]
    (GeneratedOdeModel.simulate) -- told apart by where the rows are --, `model` the class or an instance.  Returns
    (counts int32 [T-1, B, S], saturated bool [T-1, B, S]): entry k belongs to the observation interval [t_k, t_k+1].
    `saturated` means the tolerance was NOT met there: the ladder reached its ceiling `substeps` and the interval was taken with
    that many steps all the same."""
    cls = model if isinstance(model, type) else type(model)
    if getattr(cls, "step_tolerance", None) is None:
        raise ModelDefinitionError("%s has no step_tolerance: its trajectory has no count row" % cls.__name__)
    rows = len(cls.species) + (4 if cls._precision_def is not None else 0) + 1
    if traj.dim() != 4 or rows not in (traj.shape[1], traj.shape[2]):
        raise RuntimeError("%s: a trajectory [T, %d, B, S] or a solution [B, S, %d, T] is expected, got %s"
                           % (cls.__name__, rows, rows, list(traj.shape)))
    row = traj[:, -1] if traj.shape[1] == rows else traj[:, :, -1, :].permute(2, 0, 1)  # [T, B, S]
    code = row[1:].detach()
    return code.abs().round().to(torch.int32), code < 0


def _ident(key):
    return "".join(ch if ch.isalnum() else "_" for ch in key)


# ---------------------------------------------------------------------------------------------------------------------
# the side library
# ---------------------------------------------------------------------------------------------------------------------
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")


def _kernel_headers_digest():
    """The files a generated library is compiled from: the Makefile's HDRS (csrc/*.hpp and include/vihds_hip.h, whose
    checksum is the layout guard vihds_model_register compares) and the generated translation unit."""
    paths = [os.path.join(_CSRC, n) for n in sorted(os.listdir(_CSRC)) if n.endswith(".hpp")]
    paths += [os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "vihds_hip.h"),
              os.path.join(_CSRC, "generated", "ode_generated_model.hip")]
    h = hashlib.sha256()
    for path in paths:
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    return h.hexdigest()


def library_tag(source):
    """Cache key of a generated library: the source and the kernel headers it is compiled with."""
    return hashlib.sha256(source.encode() + _kernel_headers_digest().encode()).hexdigest()[:16]


def library_path(tag):
    return os.path.join(os.path.dirname(hip.library_path()), "libvihds_gen_%s.so" % tag)


def ensure_library(source):
    """Build libvihds_gen_<tag>.so next to libvihds_hip.so when it is missing (hipcc, about a minute, once: it stays in
    vi-hds_amd/lib/), with the lock / opt-out of hip.ensure_blackbox_variant (VIHDS_BLACKBOX_JIT=0 switches building off).
    Returns the library's path."""
    tag = library_tag(source)
    path = library_path(tag)
    if os.path.exists(path):
        return path
    lib_dir = os.path.dirname(path)
    header = os.path.join(lib_dir, "generated", "gen_%s.hpp" % tag)
    cmd = ["make", "-C", _CSRC, "generated", "SRC=%s" % header, "TAG=%s" % tag]
    if (os.environ.get("VIHDS_BLACKBOX_JIT", "1") == "0" or "VIHDS_HIP_LIB" in os.environ
            or not os.path.exists(os.path.join(_CSRC, "generated", "ode_generated_model.hip"))):
        raise RuntimeError("generated model needs %s (build: %s after writing the header)" % (path, " ".join(cmd)))
    import fcntl
    import subprocess

    os.makedirs(os.path.dirname(header), exist_ok=True)
    with open(os.path.join(lib_dir, ".blackbox_build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not os.path.exists(path):
                if not os.path.exists(header) or open(header).read() != source:
                    tmp = header + ".tmp%d" % os.getpid()
                    with open(tmp, "w") as f:
                        f.write(source)
                    os.replace(tmp, header)
                sys.stderr.write("[vihds] building a generated model: %s\n" % " ".join(cmd))
                res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if res.returncode != 0 or not os.path.exists(path):
                    raise RuntimeError("building %s failed:\n%s" % (path, res.stdout[-3000:]))
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return path


_REGISTERED = {}  # model_key -> (class, neural)


def register_kernel(cls, neural=False):
    """Compile (if needed) and register the kernels of a generated model class; add its key to hip.MODELS.  Returns the
    model id.  A key is one model: registering it again with another definition or precision kind raises."""
    key = cls.model_key
    prev = _REGISTERED.get(key)
    if prev is not None:
        if prev != (cls, neural) and generate_source(*prev) != generate_source(cls, neural):
            raise ModelDefinitionError("model_key '%s' is registered already with another definition" % key)
        return hip.MODELS[key]
    if key in hip.MODELS:
        raise ModelDefinitionError("model_key '%s' is a built-in model: pick another key" % key)
    source = generate_source(cls, neural)
    path = ensure_library(source)
    mid = hip.lib().vihds_model_register(path.encode())
    if mid < 0:
        hip.check(mid, "vihds_model_register(%s)" % path)
    hip.MODELS[key] = mid
    # what ops needs to contract the adjoint's dump: the networks' sizes, in the weight buffer's order
    hip.GENERATED_NETWORKS[key] = [net.sizes for net in _class_networks(cls).values()]
    if cls._trace.prec is not None:  # (four precision rows behind the species that are no NeuralPrecisions states)
        hip.GENERATED_OWN_PRECISION.add(key)
    if cls.implicit:  # (the library holds the kernels of the implicit solvers)
        hip.GENERATED_IMPLICIT.add(key)
        hip.GENERATED_IMPLICIT_ORDER[key] = int(cls.implicit_order)
    if cls._trace.algebraic:  # (unknowns of a constraint, solved inside the struct's rhs and observe)
        hip.GENERATED_ALGEBRAIC[key] = len(cls._trace.algebraic)
    if cls._trace.delays:  # (delayed reads: the fixed-grid schemes only; the adjoint needs its history workspace)
        hip.GENERATED_DELAYS[key] = len(cls._trace.delays)
    hip.GENERATED_SUBSTEPS[key] = int(cls.substeps)  # (above 1: the library holds the fixed-grid schemes only)
    if cls.step_tolerance is not None:  # (step control: substeps is the ladder's ceiling, the trajectory has a count row)
        hip.GENERATED_STEP_CONTROL[key] = (int(cls.substeps), float(cls.step_tolerance[0]), float(cls.step_tolerance[1]))
    if cls._trace.jmp is not None:  # (a state jump at the observation points: the fixed-grid schemes only, likewise)
        hip.GENERATED_JUMP.add(key)
    if cls._trace.start is not None:  # (a start map: the fixed-grid schemes only, likewise)
        hip.GENERATED_START.add(key)
    if cls._trace.steady:  # (steady species, solved for before the first step: the fixed-grid schemes only, likewise)
        hip.GENERATED_STEADY[key] = len(cls._trace.steady)
    if cls.lead_in > 0:  # (a lead-in phase: the fixed-grid schemes only, likewise)
        hip.GENERATED_LEAD_IN[key] = (float(cls.lead_in), int(cls.lead_in_steps))
    if cls._trace.dif is not None or cls._trace.chan is not None:  # (process noise: the fixed-grid schemes only; a row of cond ends with its noise key)
        hip.GENERATED_DIFFUSION.add(key)
    if cls.missing_observations:  # (missing observations: the fixed-grid schemes only; a row of cond carries its mask words)
        hip.GENERATED_MASKED.add(key)
    _REGISTERED[key] = (cls, neural)
    return mid


# ---------------------------------------------------------------------------------------------------------------------
# reactions written once: the chemical Langevin equation from a stoichiometry and the propensities
# ---------------------------------------------------------------------------------------------------------------------
def _stoichiometry(stoichiometry, propensities, what):
    if not isinstance(stoichiometry, (list, tuple)) or not isinstance(propensities, (list, tuple)) or \
            len(stoichiometry) != len(propensities) or not stoichiometry:
        raise ModelDefinitionError("%s(stoichiometry, propensities): one row of stoichiometry per propensity (one per reaction), "
                                   "at least one" % what)
    rows = [list(nu) if isinstance(nu, (list, tuple)) else None for nu in stoichiometry]
    if any(nu is None or len(nu) != len(rows[0]) or not nu for nu in rows):
        raise ModelDefinitionError("%s: every row of the stoichiometry lists the change of each species, the same number of "
                                   "entries in every row" % what)
    for nu in rows:
        for v in nu:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ModelDefinitionError("%s: the stoichiometry holds integers (the molecules a reaction adds or removes), got %r"
                                           % (what, v))
    return rows


def langevin(stoichiometry, propensities, floor=0.0):
    """The channels of the chemical Langevin equation, for channel_noise: stoichiometry[r][q] is the integer change of species q
    in reaction r, propensities[r] the rate a_r of reaction r (a model quantity, a tensor or a number).  Returns one list per
    reaction, nu_r[q] * sqrt(maximum(a_r, 0.0) + floor); an entry with nu_r[q] == 0 is the Python float 0.0, a structural zero.
    floor > 0 keeps the root's derivative finite where a propensity reaches 0 (module docstring, "Noise channels")."""
    rows = _stoichiometry(stoichiometry, propensities, "langevin")
    floor = _number(floor, "langevin's floor")
    if floor < 0.0:
        raise ModelDefinitionError("langevin: the floor under the root is >= 0, got %g" % floor)
    out = []
    for nu, a in zip(rows, propensities):
        root = sqrt(maximum(a, 0.0) + floor if floor else maximum(a, 0.0))
        out.append([0.0 if v == 0 else (root if v == 1 else -root if v == -1 else float(v) * root) for v in nu])
    return out


def langevin_drift(stoichiometry, propensities):
    """The drift of the same reactions, for rhs: one entry per species, sum_r nu_r[q] * a_r (0.0 for a species no reaction
    changes)."""
    rows = _stoichiometry(stoichiometry, propensities, "langevin_drift")
    out = []
    for q in range(len(rows[0])):
        total = 0.0
        for nu, a in zip(rows, propensities):
            if nu[q] != 0:
                total = total + (a if nu[q] == 1 else -a if nu[q] == -1 else float(nu[q]) * a)
        out.append(total)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the plugin base class
# ---------------------------------------------------------------------------------------------------------------------
class GeneratedOdeModel(OdeModel):
    """Base class of models defined in Python (module docstring).  A subclass that sets `model_key` is traced when the
    class is defined: errors in the definition and the kernels' limits are reported there, not inside a launch.

    A class with `algebraic` variables keeps the totals of a fast reaction as species and defines the unknowns by
    constraint(self, y, z, p, c) == 0, solved by algebraic_iterations Newton steps from algebraic_start(self, y, p, c) wherever
    rhs and observe are evaluated; the adjoint is the implicit-function theorem's at the final iterate (module docstring,
    "Algebraic variables"; torch_algebraic restates the solve on the host)."""

    species = None
    parameter_names = None
    n_conditions = 0
    observe_kind = "default"
    _observe_def = _precision_def = _likelihood_def = _jump_def = None  # the definitions of the hooks the class has (HOOKS: attr)
    _start_def = None  # ... and of its start map (START_HOOK)
    _diffusion_def = None  # ... and of its process noise (HOOKS: diffusion)
    _channel_noise_def = None  # ... or of its process noise by reaction channels (CHANNEL_NOISE_HOOK)
    noise_channels = ()  # names of the noise channels channel_noise returns one list for, 1 .. MAX_NOISE_CHANNELS (module docstring)
    noise_seed = 0  # the seed of the noise key a model with process noise keeps on the device (module docstring), 0 .. 2^48 - 1
    missing_observations = False  # True: a batch may carry 'observed' [rows, 4, T], 1 where a read exists (module docstring)
    networks = None  # {name: Network}: learned terms of rhs (module docstring)
    forcings = ()  # names of the time-varying inputs, read as self.forcing.<name> (module docstring)
    delays = None  # {name: (species, effective parameter)}: delayed reads, self.delayed.<name> in rhs (module docstring)
    implicit = False  # True: the Jacobian of rhs is generated and the implicit solvers take the model (module docstring)
    newton_iterations = 4  # Newton iterations of one implicit step, 1 .. MAX_NEWTON_ITERATIONS (a fixed count, no test)
    implicit_order = 1  # the order of the implicit scheme: 1 backward Euler, 2 the two-stage SDIRK (needs implicit = True)
    substeps = 1  # steps a fixed-grid solver takes over each observation interval, 1 .. MAX_SUBSTEPS (module docstring)
    step_tolerance = None  # (rtol, atol): each trajectory picks its own steps per interval, 1 -> 2 -> .. -> substeps (module docstring)
    lead_in = 0.0  # L > 0: the length of an unscored phase before the first observation point, in the units of `times`
    lead_in_steps = 1  # steps a fixed-grid solver takes over the lead-in phase, 1 .. MAX_LEAD_IN_STEPS (module docstring)
    algebraic = ()  # names of the algebraic variables, read as self.algebraic.<name> in rhs and observe (module docstring)
    algebraic_iterations = 6  # Newton iterations on the constraint, 1 .. MAX_NEWTON_ITERATIONS (a fixed count, no test)
    constraint = None  # constraint(self, y, z, p, c) -> one residual per algebraic variable; z solves constraint(...) == 0
    algebraic_start = None  # algebraic_start(self, y, p, c) -> the iteration's starting value, one entry per algebraic variable
    steady_species = ()  # names of the species solved for before the first step, 1 .. MAX_STEADY out of `species` (module docstring)
    steady_steps = 12  # pseudo-transient iterations of that solve, 1 .. MAX_STEADY_STEPS (a fixed count, no test)
    steady_first_step = 0.1  # delta_0 > 0: the first pseudo-time step, in the units of `times`
    steady_growth = 4.0  # delta_k+1 = delta_k * steady_growth, at least 1
    steady_rate = None  # steady_rate(self, y, p, c) -> one residual per steady species: their d/dt under pre-culture conditions

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        # a subclass declares its theta names as `parameters`, which would hide nn.Module.parameters() (the optimiser and
        # the training step walk the module's tensors through it): keep the names as `parameter_names`, the method as it is
        declared = cls.__dict__.get("parameters")
        if isinstance(declared, (list, tuple)):
            cls.parameter_names = list(declared)
            del cls.parameters
        # ... and its hooks (HOOKS says how each is taken from the class body)
        for h in MODEL_HOOKS:
            definition = cls.__dict__.get(h.name)
            if definition is not None:
                ok = callable(definition)
                if ok and h.checks_arguments:
                    required = [q for q in inspect.signature(definition).parameters.values()
                                if q.default is q.empty and q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD)]
                    ok = len(required) == len(h.groups) + 3  # (self, the groups, p, c)
                if not ok:
                    raise ModelDefinitionError("%s.%s must be a function %s%s" % (cls.__name__, h.name, h.signature, h.note))
                setattr(cls, h.attr, definition)
                if h.hides_method:
                    delattr(cls, h.name)
            elif h.none_resets and h.name in cls.__dict__:
                setattr(cls, h.attr, None)
            if h.settle:
                h.settle(cls)
        if cls._channel_noise_def is None and "noise_channels" not in cls.__dict__ and "channel_noise" in cls.__dict__:
            cls.noise_channels = ()  # (channel_noise = None in a subclass: the inherited names go with the hook)
        if cls.__dict__.get("model_key") is None and getattr(cls, "_trace", None) is not None:
            cls._trace = Trace(cls)  # (a subclass that only changes __init__)
            return
        if cls.model_key is None:
            return
        _validate(cls)
        cls._trace = Trace(cls)
        if cls._trace.algebraic:
            _check_constraint_pattern(cls)
        if cls._trace.steady:
            _check_steady_pattern(cls)
        generate_source(cls)  # (the checks that need the adjoints: an initial state the kernels can differentiate)

    def __init__(self, config):
        super(GeneratedOdeModel, self).__init__(config)
        self.species = list(type(self).species)
        self.n_species = len(self.species)
        if type(self)._precision_def is not None:  # the model's own precision map: the rows the kernel stores behind the species
            from vihds.precisions import ModelPrecisions
            self.precisions = ModelPrecisions()
        if _noise_def(type(self)) is not None:
            # process noise: the two-word key state a training step reads and advances (a persistent buffer: checkpoints keep the
            # stream's position) and the fixed key of evaluation passes (derived from the seed: not saved)
            seed = int(type(self).noise_seed)
            words = torch.tensor([float(seed % NOISE_KEY_WORD), float((seed // NOISE_KEY_WORD) % NOISE_KEY_WORD)], dtype=torch.float32)
            self.register_buffer("noise_key_state", words.clone())
            self.register_buffer("noise_eval_key", words, persistent=False)
        # the networks' weights (created under the seed the caller set for the whole model, like every module here): the
        # weight matrices as the reference's NeuralStates initialises them, the biases nn.Linear's default
        nets = _class_networks(type(self))
        if nets:
            self.nets = torch.nn.ModuleDict()
            for name, net in nets.items():
                I, H, O = net.sizes
                m = torch.nn.Module()
                m.hidden, m.out = torch.nn.Linear(I, H), torch.nn.Linear(H, O)
                torch.nn.init.xavier_uniform_(m.hidden.weight)
                torch.nn.init.xavier_uniform_(m.out.weight)
                self.nets[name] = m
            self._flat_all = None
            object.__setattr__(self, "net", _Networks(type(self), self._torch_call(self.network_weights)))

    # forcings: the samples travel in the rows of cond, behind the treatments
    def row_inputs(self, data):
        rows = self._forcing_rows(data)
        observed = _batch_get(data, "observed")
        if type(self).missing_observations:
            # missing observations: one mask word per time point behind the forcing samples (csrc/vihds_mask.hpp)
            rows = torch.cat([rows, self._mask_rows(data, observed, rows)], dim=1)
        elif observed is not None:
            raise RuntimeError(_OBSERVED_WITHOUT_MASK % (type(self).__name__, "does not set missing_observations = True"))
        if _noise_def(type(self)) is None:
            return rows
        # process noise: the two words of the row's key close the row (csrc/vihds_sde.hpp)
        key = data.get("noise_key", None) if hasattr(data, "get") else getattr(data, "noise_key", None)
        B = rows.shape[0]
        if key is not None:  # (the batch's own: checked on the host, then uploaded)
            cols = noise_key_rows(key, B).to(rows.device, rows.dtype)
        else:
            cols = self._next_noise_key(rows.device).to(rows.dtype)[None, :].expand(B, NOISE_KEY_COLUMNS)
        return torch.cat([rows, cols], dim=1)

    def _mask_rows(self, data, observed, rows):
        """The mask words [rows, T] of a batch, in the dtype and on the device of `rows`: from the batch's 'observed' [rows, 4, T]
        (0/1 as bool or float; checked here where it is still on the host, see observed_mask), 15 everywhere without the key."""
        B = rows.shape[0]
        if observed is None:
            times = _batch_get(data, "times")
            T = int(times.shape[0]) if times is not None else int(data.observations.shape[-1])
            return torch.full((B, T), 15.0, dtype=rows.dtype, device=rows.device)
        return mask_words(observed_mask(observed, B)).to(rows.device, rows.dtype)

    def _next_noise_key(self, device):
        """The key [2] of a batch without 'noise_key'.  Training mode: the model's two-word state on the device, then advanced
        by one with in-place torch operations (lo + 1, carried into hi, both modulo 2^24) -- a captured step therefore draws
        afresh on every replay.  Evaluation mode: the seed's key, fixed, so evaluations repeat."""
        state = self.noise_state(device)
        if not self.training:
            return self.noise_eval_key
        key = state.clone()
        with torch.no_grad():
            state[0].add_(1.0)
            carry = (state[0] >= float(NOISE_KEY_WORD)).to(state.dtype)
            state[0].sub_(carry * float(NOISE_KEY_WORD))
            state[1].add_(carry)
            state[1].sub_((state[1] >= float(NOISE_KEY_WORD)).to(state.dtype) * float(NOISE_KEY_WORD))
        return key

    def noise_state(self, device):
        """The model's two-word key state on `device` (float32 [2]): what a training step's row_inputs reads and advances.  It is
        the buffer `noise_key_state`, seeded from noise_seed when the model is built: part of state_dict (a resumed run continues the
        stream) and moved by Module.to like every buffer; asked for on another device it is moved there as it stands (never
        seeded again), together with the evaluation key.  Training's capture warm-up snapshots and rolls it back with the other
        device-side generator states."""
        state = self._buffers["noise_key_state"]
        moved = state.to(device)  # (the tensor itself where it is there already: nothing is allocated)
        if moved is not state:
            self._buffers["noise_key_state"] = moved
            self._buffers["noise_eval_key"] = self._buffers["noise_eval_key"].to(device)
        return self._buffers["noise_key_state"]

    def _forcing_rows(self, data):
        K = len(_class_forcings(type(self)))
        if not K:
            return data.inputs
        f = data.get("forcings", None) if hasattr(data, "get") else getattr(data, "forcings", None)
        if f is None:
            raise RuntimeError("%s declares forcings %s: every batch needs 'forcings' [rows, %d, times] beside 'inputs'"
                               % (type(self).__name__, list(type(self).forcings), K))
        B = data.inputs.shape[0]
        if f.dim() != 3 or f.shape[0] != B or f.shape[1] != K:
            raise RuntimeError("%s: 'forcings' must be [%d rows, %d forcings, times], got %s"
                               % (type(self).__name__, B, K, list(f.shape)))
        return torch.cat([data.inputs, f.to(data.inputs.device, data.inputs.dtype).reshape(B, -1)], dim=1)

    def cond_width(self, n_times=None):
        K = len(_class_forcings(type(self)))
        if K and n_times is None:
            raise RuntimeError("%s declares forcings: the width of a row of cond depends on the number of time points"
                               % type(self).__name__)
        if type(self).missing_observations and n_times is None:
            raise RuntimeError("%s has missing_observations = True: the width of a row of cond depends on the number of time "
                               "points (one mask word each)" % type(self).__name__)
        return (self.n_treatments + (K * int(n_times) if K else 0) + _mask_columns(type(self), n_times)
                + _noise_key_columns(type(self)))

    def solve(self, config, times, theta, conditions, dev_1hot, observations=None, request=None):
        if config.params.solver in hip.IMPLICIT_SOLVERS and not type(self).implicit:  # (before anything is built or queued)
            raise NotImplementedError("solver '%s' needs a generated model with implicit = True (%s generates no Jacobian)"
                                      % (config.params.solver, type(self).__name__))
        if type(self).substeps > 1 and config.params.solver in hip.ADAPTIVE_SOLVERS:  # (before anything is built or queued)
            raise NotImplementedError(
                "%s has substeps = %d, which divide the observation intervals of a fixed-grid scheme: the adaptive solver '%s' "
                "chooses its own steps and is not available to it (fixed-grid solvers: %s)" % (
                    type(self).__name__, type(self).substeps, config.params.solver,
                    ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
        if type(self).step_tolerance is not None and config.params.solver in STEP_CONTROL_DECLINED_SOLVERS:  # (likewise)
            raise NotImplementedError(
                "%s has step_tolerance = %r, which divides the observation interval by step doubling: '%s' takes a fixed step "
                "h0 that is not the interval and is not available to it (solvers with step control: %s)" % (
                    type(self).__name__, type(self).step_tolerance, config.params.solver,
                    ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS) - set(STEP_CONTROL_DECLINED_SOLVERS)))))
        if type(self)._jump_def is not None and config.params.solver in hip.ADAPTIVE_SOLVERS:  # (likewise)
            raise NotImplementedError(
                "%s defines jump(self, y, p, c), a state jump applied between two steps of a fixed-grid scheme: the adaptive "
                "solver '%s' integrates on a grid of its own and is not available to it (fixed-grid solvers: %s)" % (
                    type(self).__name__, config.params.solver,
                    ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
        for has, what in ((type(self)._start_def is not None, "defines start(self, y, p, c), the state the integration starts from"),
                          (type(self).lead_in > 0, "has lead_in = %r, steps of a fixed-grid scheme before the first observation "
                                                   "point" % (type(self).lead_in,)),
                          (bool(_class_steady(type(self))), "declares steady_species, solved for before the first step")):
            if has and config.params.solver in hip.ADAPTIVE_SOLVERS:  # (likewise)
                raise NotImplementedError(
                    "%s %s: only the kernels of the fixed-grid schemes run it, the adaptive solver '%s' is not available to it "
                    "(fixed-grid solvers: %s)" % (type(self).__name__, what, config.params.solver,
                                                  ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
        if _class_delays(type(self)) and config.params.solver in hip.ADAPTIVE_SOLVERS:  # (likewise)
            raise NotImplementedError(
                "%s declares delays, which read the trajectory stored on the observation grid: the adaptive solver '%s' "
                "integrates on a grid of its own and is not available to it (fixed-grid solvers: %s)" % (
                    type(self).__name__, config.params.solver, ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
        if _noise_def(type(self)) is not None:  # (likewise)
            if config.params.solver in hip.ADAPTIVE_SOLVERS:
                raise NotImplementedError(
                    "%s defines %s, process noise drawn once per step of a fixed-grid scheme on the "
                    "observation grid: the adaptive solver '%s' chooses its own steps and is not available to it (fixed-grid "
                    "solvers: %s)" % (type(self).__name__, _noise_hook(type(self)).signature, config.params.solver,
                                      ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
            _check_forcing_width(type(self), conditions.shape[1], len(times), self.n_treatments)
        if type(self).missing_observations:  # (likewise)
            if config.params.solver in hip.ADAPTIVE_SOLVERS:
                raise NotImplementedError(
                    "%s has missing_observations = True, whose mask words live on the observation grid: the adaptive solver "
                    "'%s' integrates on a grid of its own and is not available to it (fixed-grid solvers: %s)" % (
                        type(self).__name__, config.params.solver,
                        ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
            _check_forcing_width(type(self), conditions.shape[1], len(times), self.n_treatments)
        K = len(_class_forcings(type(self)))
        if K:  # (checked before anything is built or queued)
            if config.params.solver in hip.ADAPTIVE_SOLVERS:
                raise NotImplementedError(
                    "%s declares forcings, whose samples live on the observation grid: the adaptive solver '%s' integrates on a "
                    "grid of its own and is not available to it (fixed-grid solvers: %s)" % (
                        type(self).__name__, config.params.solver, ", ".join(sorted(set(hip.SOLVERS) - set(hip.ADAPTIVE_SOLVERS)))))
            _check_forcing_width(type(self), conditions.shape[1], len(times), self.n_treatments)
        return super(GeneratedOdeModel, self).solve(config, times, theta, conditions, dev_1hot, observations, request=request)

    def __setattr__(self, name, value):
        if name == "precisions" and value is not None and type(self)._precision_def is not None:
            from vihds.precisions import ModelPrecisions
            if not isinstance(value, ModelPrecisions):
                raise ModelDefinitionError(
                    "%s defines precision(self, y, x, p, c): its precisions are that map (a ModelPrecisions the base class "
                    "creates), not %s -- a subclass __init__ must not assign self.precisions" % (
                        type(self).__name__, type(value).__name__))
        super(GeneratedOdeModel, self).__setattr__(name, value)

    @property
    def precision_kind(self):
        """'custom' for a model with a precision map of its own (module docstring), else 'fixed'."""
        return "custom" if type(self)._precision_def is not None else "fixed"

    @property
    def has_jump(self):
        """True for a model with a state jump at the observation points (module docstring)."""
        return type(self)._jump_def is not None

    @property
    def has_diffusion(self):
        """True for a model with process noise, diffusion(self, y, p, c) or channel_noise(self, y, p, c) (module docstring)."""
        return _noise_def(type(self)) is not None

    @property
    def n_noise_channels(self):
        """The number of noise channels of a model with channel_noise(self, y, p, c) (module docstring); 0 for any other."""
        return len(_class_noise_channels(type(self))) if type(self)._channel_noise_def is not None else 0

    @property
    def has_start(self):
        """True for a model with a start map, start(self, y, p, c) (module docstring)."""
        return type(self)._start_def is not None

    @property
    def n_steady_species(self):
        """The number of species a model with steady_species solves for before the first step (module docstring); 0 for any
        other."""
        return len(_class_steady(type(self)))

    @property
    def has_step_control(self):
        """True for a model with step control, step_tolerance = (rtol, atol) (module docstring): the solution has one more row
        behind the species and the precision rows, each interval's step count (substep_counts)."""
        return type(self).step_tolerance is not None

    def expand_precisions(self, theta, times, x_states):
        # (step control: the count row, the last of the solution's rows, is neither a species nor a precision)
        if type(self).step_tolerance is not None:
            x_states = x_states[:, :, :-1, :]
        return super(GeneratedOdeModel, self).expand_precisions(theta, times, x_states)

    @property
    def has_lead_in(self):
        """True for a model with a lead-in phase before the first observation point, lead_in > 0 (module docstring)."""
        return type(self).lead_in > 0

    @property
    def likelihood_kind(self):
        """'custom' for a model with an observation log density of its own (module docstring), else 'gaussian'."""
        return "custom" if type(self)._likelihood_def is not None else "gaussian"

    # the three functions of a model
    def prepare(self, th, c):
        raise NotImplementedError("prepare(th, c) -> {name: effective parameter}")

    def initial_state(self, th, c):
        raise NotImplementedError("initial_state(th, c) -> [value per species]")

    def rhs(self, t, y, p, c):
        raise NotImplementedError("rhs(t, y, p, c) -> [d species / dt]")

    def condition_theta(self, theta, dev_1hot, writer, epoch):
        return theta

    # kernels
    def _neural(self):
        return type(self)._precision_def is None and bool(getattr(self.precisions, "dynamic", False))

    def kernel_slots(self):
        register_kernel(type(self), self._neural())
        return super(GeneratedOdeModel, self).kernel_slots()

    def network_weights(self):
        """{network name: (W1, b1, W2, b2)}: the nn.Parameters, as torch_problem takes them."""
        return {name: (m.hidden.weight, m.hidden.bias, m.out.weight, m.out.bias) for name, m in self.nets.items()} \
            if _class_networks(type(self)) else {}

    def flat_weight_tensors(self):
        """The kernels' weight buffer, tensor by tensor: every network in declaration order (W1, b1, W2, b2), then the
        NeuralPrecisions weights."""
        own = [t for w in self.network_weights().values() for t in w]
        return own + super(GeneratedOdeModel, self).flat_weight_tensors()

    def neural_weights(self):
        if not _class_networks(type(self)):
            return self.precisions.flat_weights() if self._neural() else None
        if self._flat_all is None:
            from vihds import ops
            object.__setattr__(self, "_flat_all", ops.FlatParameters())
        return self._flat_all(self.flat_weight_tensors())

    def problem_kwargs(self, config):
        if self._neural():
            return {"n_hidden_prec": max(int(config.params.n_hidden_decoder_precisions), 0)}
        return {}

    def summaries(self, writer, epoch):
        if writer is not None and _class_networks(type(self)):
            from vihds.utils import variable_summaries

            for name, m in self.nets.items():
                for layer, mod in (("hidden", m.hidden), ("out", m.out)):
                    variable_summaries(writer, epoch, mod.weight, "net_%s_%s_weights" % (name, layer), False)
                    variable_summaries(writer, epoch, mod.bias, "net_%s_%s_bias" % (name, layer), False)
        if self._neural():
            self.precisions.summaries(writer, epoch)

    # the same definition as a PyTorch right-hand side
    @staticmethod
    def _torch_call(weights):
        """The eager form of a network call; `weights` returns {name: (W1, b1, W2, b2)}."""
        def call(_k, name, net, inputs):
            W1, b1, W2, b2 = weights()[name]
            xs = [v if isinstance(v, torch.Tensor) else torch.as_tensor(float(v), dtype=W1.dtype, device=W1.device)
                  for v in inputs]
            x = torch.stack(torch.broadcast_tensors(*xs), dim=-1).to(W1.dtype)
            return list(torch.unbind(net_forward_ref(net, (W1, b1, W2, b2), x)[2], dim=-1))

        return call

    @classmethod
    def torch_problem(cls, th, cond, weights=None, times=None, start=True):
        """(rhs, x0) in the convention of oracle.make_*: th maps parameter names to [B, S] tensors, cond is [B, C] (log(1 +
        treatment), as the data holds it; for a class with K forcings the wide rows [n_conditions treatments | K x T samples,
        forcing-major], and `times` [T] is then required: rhs interpolates the samples linearly at its t); rhs(t, state
        [B, S, N]) -> [B, S, N] of the species (no precision states).
        weights: {network name: (W1 [H][I], b1 [H], W2 [O][H], b2 [O])} for a model with networks (an instance's
        network_weights(), or tensors of the caller's own that require grad: autograd then gives the weight gradients).
        x0 is the state the integration starts from: a class's start map is applied to its initial state (start=False: the
        initial state alone); the steps of a lead-in phase are the caller's to take, on lead_in_times.
        A class with delayed reads: rhs(t, state, delayed=[one [B,S] tensor per entry of cls.delays]) takes the values of its
        reads as it takes a forcing's -- what they are (the lookup into the trajectory so far) is the caller's integration loop's
        to say; rhs.delays lists (species index, the delay [B,S] as prepare returned it) per entry."""
        inst = cls.__new__(cls)
        nets = _class_networks(cls)
        if nets:
            if weights is None or any(n not in weights for n in nets):
                raise ValueError("%s.torch_problem needs weights={%s}" % (cls.__name__, ", ".join("'%s': (W1, b1, W2, b2)" % n
                                                                                           for n in nets)))
            object.__setattr__(inst, "net", _Networks(cls, cls._torch_call(lambda: weights)))
        N = len(cls.species)
        B, S = th[cls.parameter_names[0]].shape
        ref = th[cls.parameter_names[0]]
        cs = _treatments_torch(cls, cond, ref, S)
        names, now = _class_forcings(cls), {}
        if names:
            if times is None:
                raise ValueError("%s.torch_problem needs times=: the class declares forcings %s, sampled on the time grid"
                                 % (cls.__name__, names))
            tg = torch.as_tensor(times).to(ref.dtype).to(ref.device)
            series = _forcing_series(cls, cond, ref, tg.shape[0])  # [B, K, T]

            def no_forcing(_k, name):
                raise ModelDefinitionError("forcing '%s' read outside rhs" % name)

            object.__setattr__(inst, "forcing", _Forcings(cls, lambda k, name: now["u"][k] if now else no_forcing(k, name)))
        thn = _Named([(n, th[n]) for n in cls.parameter_names], "parameter")
        full = lambda v: v if isinstance(v, torch.Tensor) else torch.full_like(ref, float(v))  # noqa: E731
        unknowns = _class_algebraic(cls)
        object.__setattr__(inst, "algebraic", _Algebraic(cls, lambda _i, name: _algebraic_misread(name, "prepare, initial_state or start")))
        lags, now_d = _class_delays(cls), {}
        if lags:
            object.__setattr__(inst, "delayed", _Delayed(
                cls, lambda e, name: now_d["d"][e] if now_d.get("d") is not None else _delay_misread(name, "prepare, initial_state or start")))
        p = _Named(inst.prepare(thn, _Conditions(cs)).items(), "effective parameter")
        x0 = torch.stack([full(v) for v in inst.initial_state(thn, _Conditions(cs))], dim=2)
        if start and cls._start_def is not None:  # (the state the integration starts from)
            x0 = cls.torch_start(x0, th, cond, **({"n_times": tg.shape[0]} if names else {}))
        if start and _class_steady(cls):  # (... after the solve for its steady species, which carries the implicit-function gradient)
            x0 = cls.torch_steady(x0, th, cond, forcing=[series[:, k, 0, None].expand(B, S) for k in range(len(names))] if names else None)

        def rhs(t, state, delayed=None):
            y = list(torch.unbind(state[:, :, :N], dim=2))
            if lags:
                if delayed is None or len(delayed) != len(lags):
                    raise ValueError("%s.torch_problem's rhs needs delayed=[%s]: the values of the class's delayed reads at t"
                                     % (cls.__name__, ", ".join(d[0] for d in lags)))
                now_d["d"] = list(delayed)
            if names:
                # the linear interpolant of the row's samples at t: on [t_k, t_k+1], u_k + (t - t_k) (u_k+1 - u_k) / (t_k+1 - t_k)
                tt = torch.as_tensor(t, dtype=ref.dtype, device=ref.device)
                k = int(torch.searchsorted(tg, tt.reshape(1), right=True)[0]) - 1
                k = min(max(k, 0), tg.shape[0] - 2)
                u = series[:, :, k] + (tt - tg[k]) * (series[:, :, k + 1] - series[:, :, k]) / (tg[k + 1] - tg[k])
                now["u"] = [u[:, j, None].expand(B, S) for j in range(len(names))]
            if unknowns:  # the constraint's solution at this stage state, carrying the implicit-function gradient
                z, _ = _algebraic_torch(cls, inst, y, p, _Conditions(cs))
                object.__setattr__(inst, "algebraic", _Algebraic(cls, lambda i, _name: z[i]))
            return torch.stack([full(v) for v in inst.rhs(t, y, p, _Conditions(cs))], dim=2)

        if lags:
            rhs.delays = [(list(cls.species).index(sp), full(p[par])) for _name, sp, par in lags]
        return rhs, x0

    @classmethod
    def torch_jacobian(cls, y, theta, cond, t=0.0, times=None):
        """The generated Jacobian of rhs evaluated with torch ops in y's dtype -- the SAME DAG nodes rhs_jac is emitted from
        (jacobian_nodes), not autograd: it exists to check the generator against autograd of torch_problem's rhs.  y [B,S,N]
        species, theta {parameter name: [B,S]} -- prepare is applied to it first --, cond [B,C] as the data holds it (the wide
        rows of a class with forcings, with `times` [T]: the interpolant at t) -> [B,S,N,N], entry [i][j] = d dy_i / d y_j."""
        tr = cls._trace
        N, NPU = len(cls.species), len(tr.p_names)
        ref = y[:, :, 0]
        th = {n: theta[n].to(ref.dtype) for n in cls.parameter_names}
        cs = _treatments_torch(cls, cond, ref, ref.shape[1])
        env = {("th", s): th[n] for s, n in enumerate(cls.parameter_names)}
        env.update({("c", q): v for q, v in enumerate(cs)})
        prepared = evaluate(tr.p_exprs, env)
        env.update({("p", k): v.to(ref.dtype) for k, v in enumerate(prepared)})
        env.update({("p", NPU + q): v for q, v in enumerate(cs)})  # (the treatments rhs reads sit behind the named parameters)
        env.update({("y", j): y[:, :, j] for j in range(N)})
        env[("t", 0)] = torch.as_tensor(t, dtype=ref.dtype, device=ref.device)
        names = _class_forcings(cls)
        if names:
            if times is None:
                raise ValueError("%s.torch_jacobian needs times=: the class declares forcings %s" % (cls.__name__, names))
            tg = torch.as_tensor(times).to(ref.dtype).to(ref.device)
            series = _forcing_series(cls, cond, ref, tg.shape[0])
            k = int(torch.searchsorted(tg, env[("t", 0)].reshape(1), right=True)[0]) - 1
            k = min(max(k, 0), tg.shape[0] - 2)
            u = series[:, :, k] + (env[("t", 0)] - tg[k]) * (series[:, :, k + 1] - series[:, :, k]) / (tg[k + 1] - tg[k])
            env.update({("f", j): u[:, j, None].expand_as(ref) for j in range(len(names))})
        rows = jacobian_nodes(cls)
        flat = evaluate([e for row in rows for e in row], env)
        return torch.stack([v.to(ref.dtype).expand_as(ref) for v in flat], dim=2).reshape(ref.shape + (N, N))

    @classmethod
    def torch_observe(cls, y, theta, cond):
        """The model's own observation map with torch ops in y's dtype (the float64 reference of the generated observe /
        observe_vjp, as torch_problem is for rhs): y [B,S,N,T] species (states behind them, e.g. neural precisions, are
        ignored), theta {parameter name: [B,S]} -- prepare is applied to it first -- and cond [B,C] as the data holds it
        -> x_predict [B,S,4,T]."""
        if cls._observe_def is None:
            raise ModelDefinitionError("%s defines no observe(self, y, p, c): its map is the fixed kind '%s'"
                                       % (cls.__name__, cls.observe_kind))
        return _hook_torch(cls, HOOK["observe"], cls.__new__(cls), [y[:, :, :len(cls.species), :]], theta, cond)

    @classmethod
    def torch_algebraic(cls, y, theta, cond, forcing=None, return_increment=False):
        """The algebraic variables at the states y with torch ops in y's dtype, by the iteration the kernels run (module
        docstring): z = algebraic_start(y, p); algebraic_iterations times G = g(y, z, p), A = dg/dz by autograd, A d = -G by
        torch.linalg.solve (pivoted), z += d.  y [B,S,N] species, theta {parameter name: [B,S]} -- prepare is applied to it
        first --, cond [B,C] as the data holds it, forcing: the K values the constraint reads there (tensors that broadcast to
        [B,S]) for a class with forcings -> z [B,S,M].  The value is the iterate's; its gradient is the implicit-function
        derivative of the converged solution, z_K.detach() - (s - s.detach()) with s = solve(A(z_K).detach(), g(y, z_K.detach(),
        p)): nothing is differentiated through the iteration.  return_increment: (z, the largest last Newton increment relative
        to the largest |z| of its trajectory) -- what says whether the iteration has converged."""
        if not _class_algebraic(cls):
            raise ModelDefinitionError("%s declares no algebraic variables" % cls.__name__)
        inst = cls.__new__(cls)
        ref = y[:, :, 0]
        cs = _treatments_torch(cls, cond, ref, ref.shape[1])
        thn = _Named([(n, theta[n].to(ref.dtype)) for n in cls.parameter_names], "parameter")
        p = _Named(inst.prepare(thn, _Conditions(cs)).items(), "effective parameter")
        names = _class_forcings(cls)
        if names:
            if forcing is None or len(forcing) != len(names):
                raise ValueError("%s.torch_algebraic needs forcing=[%s]: the values of the class's forcings at the states"
                                 % (cls.__name__, ", ".join(names)))
            object.__setattr__(inst, "forcing", _Forcings(cls, lambda k, _name: forcing[k]))
        z, last = _algebraic_torch(cls, inst, list(torch.unbind(y[:, :, :len(cls.species)], dim=2)), p, _Conditions(cs))
        z = torch.stack([v.expand_as(ref) for v in z], dim=2)
        return (z, last) if return_increment else z

    @classmethod
    def torch_constraint_jacobian(cls, y, z, theta, cond, forcing=None):
        """The generated dg/dz evaluated with torch ops in y's dtype -- the SAME DAG nodes constraint_jac is emitted from
        (constraint_jacobian_nodes), not autograd: it exists to check the generator against autograd of the class's constraint.
        y [B,S,N], z [B,S,M], theta, cond and forcing as torch_algebraic takes them -> [B,S,M,M], entry [i][j] = d g_i / d z_j."""
        tr = cls._trace
        N, M, NPU = len(cls.species), len(tr.algebraic), len(tr.p_names)
        ref = y[:, :, 0]
        cs = _treatments_torch(cls, cond, ref, ref.shape[1])
        env = {("th", s): theta[n].to(ref.dtype) for s, n in enumerate(cls.parameter_names)}
        env.update({("c", q): v for q, v in enumerate(cs)})
        env.update({("p", k): v.to(ref.dtype) for k, v in enumerate(evaluate(tr.p_exprs, env))})
        env.update({("p", NPU + q): v for q, v in enumerate(cs)})
        env.update({("y", j): y[:, :, j] for j in range(N)})
        env.update({("z", i): z[:, :, i] for i in range(M)})
        env.update({("f", k): v for k, v in enumerate(forcing or ())})
        flat = evaluate([e for row in constraint_jacobian_nodes(cls) for e in row], env)
        return torch.stack([v.to(ref.dtype).expand_as(ref) for v in flat], dim=2).reshape(ref.shape + (M, M))

    @classmethod
    def torch_steady(cls, y, theta, cond, forcing=None, return_residual=False, steps=None, first_step=None, growth=None):
        """The solve for the steady species with torch ops in y's dtype, by the iteration the kernels run (module docstring): from
        y [B,S,N] (what initial_state, then start returned), steady_steps times F = steady_rate(y, p), J = dF/dy_E by autograd,
        (I - delta J) d = delta F by torch.linalg.solve (pivoted), y_E += d, delta *= steady_growth (delta in float32, as the
        kernels form it).  theta {parameter name: [B,S]} -- prepare is applied to it first --, cond [B,C] as the data holds it,
        forcing: the K first samples u_0 (tensors that broadcast to [B,S]) for a class with forcings -> the state [B,S,N].  The
        value is the iterate's; a custom autograd function carries the implicit-function gradient of the converged solution at
        it: J^T mu = the adjoint of y_E, then the product of steady_rate seeded with -mu into the other species and theta, and 0
        into the guess of the steady species -- nothing is differentiated through the iteration.  return_residual: (state, the
        largest last increment relative to the largest |y_E| of its trajectory, the largest |F(y*)|) -- what says whether the
        count is enough.  steps / first_step / growth override the class's for such an experiment."""
        names_e = _class_steady(cls)
        if not names_e:
            raise ModelDefinitionError("%s declares no steady_species" % cls.__name__)
        inst = cls.__new__(cls)
        N = len(cls.species)
        idx = [list(cls.species).index(s) for s in names_e]
        y = y[:, :, :N]
        ref = y[:, :, 0]
        cs = _treatments_torch(cls, cond, ref, ref.shape[1])
        names = _class_forcings(cls)
        if names:
            if forcing is None or len(forcing) != len(names):
                raise ValueError("%s.torch_steady needs forcing=[%s]: the first samples of the class's forcings"
                                 % (cls.__name__, ", ".join(names)))
            object.__setattr__(inst, "forcing", _Forcings(cls, lambda k, _name: forcing[k]))
        object.__setattr__(inst, "algebraic", _Algebraic(cls, lambda _i, name: _algebraic_misread(name, "steady_rate")))
        if _class_delays(cls):
            object.__setattr__(inst, "delayed", _Delayed(cls, lambda _e, name: _delay_misread(name, "steady_rate")))
        pnames = list(cls.parameter_names)
        n_steps = int(cls.steady_steps if steps is None else steps)
        delta0 = np.float32(cls.steady_first_step if first_step is None else first_step)
        grow = np.float32(cls.steady_growth if growth is None else growth)

        def residual(state, thetas):
            thn = _Named([(n, v.to(ref.dtype)) for n, v in zip(pnames, thetas)], "parameter")
            p = _Named(inst.prepare(thn, _Conditions(cs)).items(), "effective parameter")
            out = inst.steady_rate(list(torch.unbind(state, dim=2)), p, _Conditions(cs))
            return torch.stack([(v if isinstance(v, torch.Tensor) else torch.full_like(ref, float(v))).expand_as(ref)
                                for v in out], dim=2)

        def linearised(state, thetas):
            """(J [B,S,M,M], F [B,S,M]) at the state, detached."""
            with torch.enable_grad():
                z = state[:, :, idx].detach().requires_grad_(True)
                full = state.detach().clone()
                cols = list(torch.unbind(full, dim=2))
                for e, j in enumerate(idx):
                    cols[j] = z[:, :, e]
                F = residual(torch.stack(cols, dim=2), [v.detach() for v in thetas])
                rows = []
                for i in range(len(idx)):
                    fi = F[:, :, i].sum()
                    row = torch.autograd.grad(fi, z, retain_graph=True, allow_unused=True)[0] if fi.requires_grad else None
                    rows.append(torch.zeros_like(z) if row is None else row)
            return torch.stack(rows, dim=2).detach(), F.detach()

        holder = {}

        class _Steady(torch.autograd.Function):
            @staticmethod
            def forward(ctx, state, *thetas):
                cur, delta = state.detach().clone(), delta0
                eye = torch.eye(len(idx), dtype=state.dtype, device=state.device)
                d = torch.zeros_like(cur[:, :, idx])
                for _ in range(n_steps):
                    J, F = linearised(cur, thetas)
                    d = torch.linalg.solve(eye - float(delta) * J, (float(delta) * F).unsqueeze(-1)).squeeze(-1)
                    cur[:, :, idx] = cur[:, :, idx] + d
                    delta = np.float32(delta * grow)
                ctx.save_for_backward(cur, *thetas)
                holder["last"] = d
                return cur

            @staticmethod
            def backward(ctx, lam):
                cur, thetas = ctx.saved_tensors[0], ctx.saved_tensors[1:]
                J, _F = linearised(cur, thetas)
                mu = torch.linalg.solve(J.transpose(-1, -2), lam[:, :, idx].unsqueeze(-1)).squeeze(-1)
                with torch.enable_grad():
                    st = cur.detach().requires_grad_(True)
                    ths = [v.detach().requires_grad_(True) for v in thetas]
                    F = residual(st, ths)
                    grads = torch.autograd.grad(F, [st] + ths, grad_outputs=-mu, allow_unused=True) if F.requires_grad \
                        else [None] * (1 + len(ths))
                gy = lam.clone()
                if grads[0] is not None:
                    gy = gy + grads[0]
                gy[:, :, idx] = 0.0
                return (gy,) + tuple(None if v is None else v for v in grads[1:])

        thetas = [theta[n].to(ref.dtype) for n in pnames]
        out = _Steady.apply(y, *thetas)
        if not return_residual:
            return out
        with torch.no_grad():
            _J, F = linearised(out, thetas)
            d = holder["last"]
            scale = out[:, :, idx].abs().amax(-1).clamp_min(1e-30)
            inc = float((d.abs().amax(-1) / scale).max()) if bool(torch.isfinite(d).all()) else float("inf")
            res = float(F.abs().max()) if bool(torch.isfinite(F).all()) else float("inf")
        return out, inc, res

    @classmethod
    def torch_steady_jacobian(cls, y, theta, cond, forcing=None):
        """The generated J = d steady_rate / d y_E evaluated with torch ops in y's dtype -- the SAME DAG nodes steady_jac is
        emitted from (steady_jacobian_nodes), not autograd: it exists to check the generator against autograd of the class's
        steady_rate.  y [B,S,N], theta, cond and forcing as torch_steady takes them -> [B,S,M,M], entry [i][j] = d F_i / d
        y[steady species j]."""
        tr = cls._trace
        N, M, NPU = len(cls.species), len(tr.steady), len(tr.p_names)
        ref = y[:, :, 0]
        cs = _treatments_torch(cls, cond, ref, ref.shape[1])
        env = {("th", s): theta[n].to(ref.dtype) for s, n in enumerate(cls.parameter_names)}
        env.update({("c", q): v for q, v in enumerate(cs)})
        env.update({("p", k): v.to(ref.dtype) for k, v in enumerate(evaluate(tr.p_exprs, env))})
        env.update({("p", NPU + q): v for q, v in enumerate(cs)})
        env.update({("y", j): y[:, :, j] for j in range(N)})
        env.update({("f", k): v for k, v in enumerate(forcing or ())})
        flat = evaluate([e for row in steady_jacobian_nodes(cls) for e in row], env)
        return torch.stack([v.to(ref.dtype).expand_as(ref) for v in flat], dim=2).reshape(ref.shape + (M, M))

    @classmethod
    def torch_precision(cls, y, theta, cond):
        """The model's own precision map with torch ops in y's dtype (the float64 reference of the generated precision /
        precision_vjp, as torch_observe is for the map): y [B,S,N,T] species (rows stored behind them are ignored), theta
        {parameter name: [B,S]} and cond [B,C] as the data holds it.  prepare and the observation map -- the model's own
        observe, or the fixed map of its observe_kind -- are applied first -> precisions [B,S,4,T]."""
        if cls._precision_def is None:
            raise ModelDefinitionError("%s defines no precision(self, y, x, p, c): its precisions are its `precisions` "
                                       "attribute's" % cls.__name__)
        inst = cls.__new__(cls)
        y = y[:, :, :len(cls.species), :]
        if cls._observe_def is not None:
            x = _hook_torch(cls, HOOK["observe"], inst, [y], theta, cond)
        else:
            fixed = OdeModel.__new__(OdeModel)  # (the fixed maps of OdeModel._observe_map read observe_kind only)
            fixed.__dict__["observe_kind"] = cls.observe_kind
            x = OdeModel._observe_map(fixed, y)
        return _hook_torch(cls, HOOK["precision"], inst, [y, x], theta, cond)

    @classmethod
    def torch_log_likelihood(cls, x, obs, prec, theta, cond, observed=None):
        """The model's own observation log density with torch ops in x's dtype (the float64 reference of the generated loglik
        / loglik_vjp): x [B,S,4,T] predicted signals, obs [B,4,T] observations, prec [B,S,4,T] precisions (anything that
        broadcasts to it), theta {parameter name: [B,S]} -- prepare is applied to it first -- and cond [B,C] as the data
        holds it -> the per-signal log densities of every time point [B,S,4,T] (the kernels sum them over time).
        observed [B,4,T] (a class with missing_observations = True; None: every point): the density is evaluated on ob' -- the
        read where there is one, x itself where there is none, so a placeholder never enters -- and an unobserved point's term is
        0.0 by a select (masked_terms)."""
        if cls._likelihood_def is None:
            raise ModelDefinitionError("%s defines no log_likelihood(self, x, obs, pr, p, c): its observation log density is "
                                       "the Gaussian's" % cls.__name__)
        if observed is not None and not cls.missing_observations:
            raise RuntimeError(_OBSERVED_WITHOUT_MASK % (cls.__name__, "does not set missing_observations = True"))
        obs, prec = obs.to(x.dtype)[:, None].expand(x.shape), prec.to(x.dtype).expand(x.shape)
        return masked_terms(lambda ob: _hook_torch(cls, HOOK["log_likelihood"], cls.__new__(cls), [x, ob, prec], theta, cond),
                            x, obs, observed)

    @classmethod
    def torch_jump(cls, y, theta, cond):
        """The model's own state jump with torch ops in y's dtype (the float64 reference of the generated jump / jump_vjp, as
        torch_observe is for the map): y [B,S,N,T] species at the time points (the left limits; rows stored behind them are
        ignored), theta {parameter name: [B,S]} -- prepare is applied to it first -- and cond [B,C] as the data holds it (the
        wide rows of a class with forcings: the jump of point k reads sample k) -> the states right after the points [B,S,N,T].
        The kernels do not evaluate the jump of the last point."""
        if cls._jump_def is None:
            raise ModelDefinitionError("%s defines no jump(self, y, p, c): its state is continuous at the observation points"
                                       % cls.__name__)
        return _hook_torch(cls, HOOK["jump"], cls.__new__(cls), [y[:, :, :len(cls.species), :]], theta, cond)

    @classmethod
    def torch_diffusion(cls, y, theta, cond, n_times=None):
        """The model's own noise amplitudes with torch ops in y's dtype (the float64 reference of the generated diffusion /
        diffusion_vjp, as torch_jump is for the jump): y [B,S,N,T] species at the start of steps (one column per time point:
        the step that starts at point k reads forcing sample k), theta {parameter name: [B,S]} -- prepare is applied to it
        first -- and cond [B,C] as the kernels take it, the two key columns last (n_times: how many samples a forcing series
        has where y holds another number of columns) -> the amplitudes [B,S,N,T]; 0 for a species without noise."""
        if cls._diffusion_def is None:
            raise ModelDefinitionError("%s defines no diffusion(self, y, p, c): its trajectories are deterministic" % cls.__name__)
        return _hook_torch(cls, HOOK["diffusion"], cls.__new__(cls), [y[:, :, :len(cls.species), :]], theta, cond, n_times)

    @classmethod
    def torch_channel_noise(cls, y, theta, cond, n_times=None):
        """The model's own channel amplitudes with torch ops in y's dtype (the float64 reference of the generated channel_noise /
        channel_noise_vjp, as torch_diffusion is for the diagonal hook): y [B,S,N,T] species at the start of steps, theta
        {parameter name: [B,S]} -- prepare is applied to it first -- and cond [B,C] as the kernels take it, the two key columns
        last (n_times as in torch_diffusion) -> G [B,S,N,R,T]: entry [.., q, r, .] is the amplitude with which channel r enters
        species q; 0 where it does not."""
        if cls._channel_noise_def is None:
            raise ModelDefinitionError("%s defines no channel_noise(self, y, p, c)" % cls.__name__)
        return _hook_torch(cls, HOOK["channel_noise"], cls.__new__(cls), [y[:, :, :len(cls.species), :]], theta, cond, n_times)

    @classmethod
    def torch_start(cls, y, theta, cond, n_times=None):
        """The model's own start map with torch ops in y's dtype (the float64 reference of the generated start / start_vjp): y
        [B,S,N] what initial_state returned, theta {parameter name: [B,S]} -- prepare is applied to it first -- and cond [B,C] as
        the data holds it (the wide rows of a class with forcings: start reads the first sample of each series; n_times says
        how many samples a series has where the rows hold more treatments than the model reads) -> the state the integration
        starts from [B,S,N]."""
        if cls._start_def is None:
            raise ModelDefinitionError("%s defines no start(self, y, p, c): its integration starts from its initial state"
                                       % cls.__name__)
        K, T = len(_class_forcings(cls)), 1
        if K:
            T = int(n_times) if n_times is not None else (cond.shape[1] - int(cls.n_conditions)) // (
                K + (1 if cls.missing_observations else 0))
        y = y[:, :, :len(cls.species)]
        return _hook_torch(cls, HOOK["start"], cls.__new__(cls), [y.unsqueeze(-1).expand(y.shape + (T,))], theta, cond)[..., 0]

    def _log_likelihood_map(self, x_predict, observations, precisions, observed=None):
        """The model's own log density on tensors of the host paths (the host-driven adaptive route, the plugin fallback of
        Training.cost), with theta and the treatments of the last solve, as _observe_map: x_predict [B,S,4,T], observations
        [B,4,T], precisions broadcastable to x_predict -> [B,S,4,T]."""
        theta, cond = self._last_theta(x_predict.device, "%s.log_likelihood reads theta and the treatments of the last solve, and "
                                       "nothing has been solved yet")
        return type(self).torch_log_likelihood(x_predict, observations.to(x_predict.device), precisions, theta, cond,
                                               observed=observed)

    def _observe_map(self, x_sample):
        """OdeModel.observe on a tensor that is not the last solution: the model's own map (torch_observe) with theta and
        the treatments of the last solve."""
        if type(self)._observe_def is None:
            return super(GeneratedOdeModel, self)._observe_map(x_sample)
        theta, cond = self._last_theta(x_sample.device, "%s.observe: the map reads theta and the treatments of the last solve, and "
                                       "nothing has been solved yet")
        return type(self).torch_observe(x_sample, theta, cond)

    def _last_theta(self, dev, nothing_solved):
        """({parameter name: [B,S]}, cond [B,C]) of the last solve on `dev`, for the host paths that evaluate a hook on
        tensors that are not the last solution."""
        if self._last_inputs is None:
            raise RuntimeError(nothing_solved % type(self).__name__)
        packed, row_of, cond = self._last_inputs
        return {n: packed[row_of[n]].to(dev) for n in type(self).parameter_names}, cond.to(dev)


def _fma32(a, b, c):
    """fmaf(a, b, c) of three float32 numbers: the exact a * b + c rounded once to float32 (to nearest, ties to even)."""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    best = np.float32(float(exact))  # (rounded twice: a neighbour may be nearer, never as near -- a tie survives both roundings)
    for other in (np.nextafter(best, np.float32(-np.inf)), np.nextafter(best, np.float32(np.inf))):
        if np.isfinite(other) and abs(Fraction(float(other)) - exact) < abs(Fraction(float(best)) - exact):
            best = other
    return np.float32(best)


def lead_in_times(cls, t0):
    """The n + 1 float32 times of the class's lead-in phase for a first observation point t0, exactly as the kernels form them
    (csrc/vihds_substeps.hpp, SubGrid<n>(tl, t0)): tl = t0 - L, hl = (t0 - tl) * (1.f / n), s_j = fmaf(j, hl, tl) for j < n and
    s_n = t0.  A numpy float32 array; [t0] alone for a class without a lead-in."""
    t0 = np.float32(t0)
    if not cls.lead_in > 0:
        return np.array([t0], dtype=np.float32)
    n = int(cls.lead_in_steps)
    tl = np.float32(t0 - np.float32(cls.lead_in))
    hl = np.float32(np.float32(t0 - tl) * np.float32(np.float32(1.0) / np.float32(n)))
    return np.array([_fma32(np.float32(j), hl, tl) for j in range(n)] + [t0], dtype=np.float32)


def _treatments_torch(cls, cond, like, S):
    """The treatments c of cond [B,C] (as the data holds it) in `like`'s dtype: C tensors [B,S]."""
    C = int(cls.n_conditions)
    tt = torch.clamp(torch.exp(cond[:, :C].to(like.dtype)) - 1.0, 1e-12, 1e6)  # (forcing samples may follow: used raw)
    return [torch.transpose(tt[:, q].repeat([S, 1]), 0, 1) for q in range(C)]


NOISE_KEY_COLUMNS = 2  # floats of a row of cond behind the forcing samples of a model with process noise: key lo, key hi
NOISE_KEY_WORD = 1 << 24  # each an integer-valued float in [0, 2^24) (csrc/vihds_sde.hpp converts by truncation)


def _noise_key_columns(cls):
    return NOISE_KEY_COLUMNS if _noise_def(cls) is not None else 0


def _noise_hook(cls):
    """The record of the form of process noise the class defines (DIFFUSION_HOOK or CHANNEL_NOISE_HOOK), or None."""
    for h in NOISE_HOOKS:
        if getattr(cls, h.attr, None) is not None:
            return h
    return None


def _noise_def(cls):
    h = _noise_hook(cls)
    return None if h is None else getattr(cls, h.attr)


def noise_key_rows(key, n_rows):
    """The two key columns [n_rows, 2] (float32, on the host) of a batch's 'noise_key': one pair of ints for every row, or
    [n_rows, 2]; each word an integer in [0, 2^24).  Checked here, before anything is uploaded."""
    if isinstance(key, torch.Tensor):
        key = key.detach().cpu().numpy()
    try:
        k = np.asarray(key).astype(np.float64)
    except (TypeError, ValueError):
        k = np.empty(0)
    if k.size == 0 or not np.all(np.isfinite(k)) or np.any(k != np.floor(k)):
        raise ValueError("noise_key must hold integers (one pair, or [rows, 2]), got %r" % (key,))
    k = k.astype(np.int64)
    if k.shape == (2,):
        k = np.broadcast_to(k, (n_rows, 2))
    if k.shape != (n_rows, 2):
        raise ValueError("noise_key must be one pair of ints or [%d rows, 2], got shape %s" % (n_rows, list(np.shape(key))))
    if k.min() < 0 or k.max() >= NOISE_KEY_WORD:
        raise ValueError("noise_key: each word is an integer in [0, 2^24) (it travels as a float32 of cond), got %d .. %d"
                         % (k.min(), k.max()))
    return torch.from_numpy(np.ascontiguousarray(k, dtype=np.float32))


_OBSERVED_WITHOUT_MASK = ("the batch carries 'observed' (a mask of missing observations), and %s %s: only a generated model "
                          "with missing_observations = True scores by it -- every other model's kernels would score the "
                          "placeholders")


def _batch_get(data, name):
    return data.get(name, None) if hasattr(data, "get") else getattr(data, name, None)


def _mask_columns(cls, n_times):
    """Floats of a row of cond behind the forcing samples of a model with missing observations: one mask word per time point."""
    return int(n_times) if getattr(cls, "missing_observations", False) else 0


def observed_mask(observed, n_rows=None, n_times=None):
    """A batch's 'observed' as a float32 tensor [rows, 4, T] of 0.0 / 1.0, where it is: 1 means the read exists.  Accepts bool or
    0/1 numbers (tensor, array or nested lists); a wrong shape raises, and so does any other value wherever the data is still
    on the host -- a numpy array, a list, a CPU tensor, which is how a dataset hands it over (training.batch_to_device checks
    before it uploads).  A tensor that is on a device already is taken as it is: reading it back would stall the queue."""
    o = observed if isinstance(observed, torch.Tensor) else torch.as_tensor(np.asarray(observed))
    if o.dim() != 3 or o.shape[1] != 4 or (n_rows is not None and o.shape[0] != n_rows) or (
            n_times is not None and o.shape[2] != n_times):
        raise ValueError("'observed' must be [%s rows, 4 signals, %s time points], got %s" % (
            "?" if n_rows is None else n_rows, "?" if n_times is None else n_times, list(o.shape)))
    if o.dtype == torch.bool:
        return o.to(torch.float32)
    if o.device.type == "cpu":
        if o.is_complex() or not bool(((o == 0) | (o == 1)).all()):
            raise ValueError("'observed' must hold 0 / 1 (1: the read exists), as bool or numbers; it holds other values "
                             "(a NaN belongs into 'observations' under a 0 here, not into the mask)")
    return o.to(torch.float32)


def mask_words(observed):
    """The mask words [rows, T] of observed [rows, 4, T] (0.0 / 1.0): word k = sum_j observed[j][k] * 2^j, an integer 0 .. 15,
    exact in float32 (csrc/vihds_mask.hpp decodes it).  Plain arithmetic on the tensor's device: nothing is uploaded, so a
    captured step may form the words of its static batch."""
    o = observed.to(torch.float32)
    return o[:, 0] + 2.0 * o[:, 1] + 4.0 * o[:, 2] + 8.0 * o[:, 3]


def mask_bits(words):
    """The inverse of mask_words: words [rows, T] -> bool [rows, 4, T], bit j of (int) word."""
    w = words.to(torch.int64)
    return torch.stack([((w >> j) & 1).bool() for j in range(4)], dim=1)


def masked_terms(terms_of, x, obs, observed):
    """The scoring rule of a model with missing observations on the host, the kernels' select for select: with m = observed
    (bool, broadcast over the samples), ob' = where(m, obs, x) -- the predicted signal stands in for the placeholder, which never
    enters the arithmetic, so no NaN reaches a gradient either --, and the result is where(m, terms_of(ob'), 0).  x [B,S,4,T];
    obs broadcastable to it; observed [B,4,T] or None (every point observed: terms_of(obs) as it is)."""
    if observed is None:
        return terms_of(obs)
    m = observed_mask(observed, x.shape[0], x.shape[-1]).to(x.device).bool()[:, None].expand(x.shape)
    # (x detached under the mask: the stand-in is a value, not a path -- the residual there is exactly 0 and carries no gradient)
    terms = terms_of(torch.where(m, obs.expand(x.shape), x.detach()))
    return torch.where(m, terms, torch.zeros((), dtype=terms.dtype, device=terms.device))


def _check_forcing_width(cls, width, n_times, n_treatments=None):
    """A row of cond is [treatments | K x T samples | T mask words | 2 key words] (the last two parts for a model with missing
    observations and one with process noise).  n_treatments: how many treatments the rows hold (an instance knows: its
    data may carry more than the n_conditions the model reads); None: at least the model's n_conditions."""
    K, C = len(_class_forcings(cls)), int(cls.n_conditions) if n_treatments is None else int(n_treatments)
    words = _mask_columns(cls, n_times)  # (the mask words of a model with missing observations follow the samples)
    tail = _noise_key_columns(cls) + words  # (the two key columns of a model with process noise close the row)
    if width - C - tail != K * n_times and (n_treatments is not None or width - tail - K * n_times < C):
        raise ValueError("%s reads %d forcing(s) on %d time points: a row of cond must hold %d samples behind its %d treatment(s)%s%s, "
                         "and holds %d (width %d)" % (cls.__name__, K, n_times, K * n_times, C,
                                                      " and its %d mask words behind them" % words if words else "",
                                                      " and its 2 noise-key columns behind them" if tail - words else "",
                                                      width - C - tail, width))


def _forcing_series(cls, cond, like, n_times):
    """The forcing samples of the wide cond [B, C] in `like`'s dtype: [B, K, T], the last K * T columns of each row, raw."""
    K = len(_class_forcings(cls))
    _check_forcing_width(cls, cond.shape[1], n_times)
    end = cond.shape[1] - _noise_key_columns(cls) - _mask_columns(cls, n_times)
    return cond[:, end - K * n_times:end].to(like.dtype).to(like.device).reshape(cond.shape[0], K, n_times)


def _algebraic_torch(cls, inst, y, p, cs):
    """(the M algebraic variables, the largest last Newton increment relative to the trajectory's largest |z|) of the class's
    constraint at the species y (a list of N tensors that broadcast together), by the iteration as the module docstring defines
    it; p the effective parameters, cs the treatments, inst.forcing the forcings' values there.  Each returned tensor has the
    iterate's value and the implicit-function gradient with respect to y, p (GeneratedOdeModel.torch_algebraic)."""
    M = len(_class_algebraic(cls))
    like = torch.broadcast_tensors(*[v for v in y if isinstance(v, torch.Tensor)])[0]
    full = lambda v: v if isinstance(v, torch.Tensor) else torch.full_like(like, float(v))  # noqa: E731
    stack = lambda vs: torch.stack(torch.broadcast_tensors(*[full(v) for v in vs]), dim=-1)  # noqa: E731
    residual = lambda zz: stack(inst.constraint(y, list(torch.unbind(zz, dim=-1)), p, cs))  # noqa: E731

    def linearised(zz):
        with torch.enable_grad():
            zz = zz.detach().requires_grad_(True)
            G = residual(zz)
            G = G.expand(torch.broadcast_shapes(G.shape, zz.shape))
            rows = []
            for i in range(M):
                gi = G[..., i].sum()
                row = torch.autograd.grad(gi, zz, retain_graph=True, allow_unused=True)[0] if gi.requires_grad else None
                rows.append(torch.zeros_like(zz) if row is None else row)
        return torch.stack(rows, dim=-2).detach(), G.detach()

    out = inst.algebraic_start(y, p, cs)
    if not isinstance(out, (list, tuple)) or len(out) != M:
        raise ModelDefinitionError("%s.algebraic_start must return a list of %d entries" % (cls.__name__, M))
    z = stack(out).detach()
    z = z.expand(torch.broadcast_shapes(z.shape, residual(z).shape)).to(like.dtype)
    d = torch.zeros_like(z)
    for _ in range(int(cls.algebraic_iterations)):
        A, G = linearised(z)
        d = torch.linalg.solve(A, -G.unsqueeze(-1)).squeeze(-1)
        z = z + d
    last = float((d.abs().amax(-1) / z.abs().amax(-1).clamp_min(1e-30)).max()) if bool(torch.isfinite(d).all()) else float("inf")
    if torch.is_grad_enabled():
        s = torch.linalg.solve(linearised(z)[0], residual(z).unsqueeze(-1)).squeeze(-1)
        z = z - (s - s.detach())
    return list(torch.unbind(z, dim=-1)), last


def _hook_torch(cls, h, inst, groups, th, cond, n_times=None):
    """The class's definition of hook h with torch ops in the dtype of its first group: groups of [B,S,.,T] tensors (in
    the hook's order), th {parameter name: [B,S]} -- prepare is applied to it -- and cond [B,C] -> [B,S,4,T] (the hook's
    n_outputs: [B,S,N,T] for the state jump)."""
    ref = groups[0][:, :, 0, :]
    cs = _treatments_torch(cls, cond, ref, ref.shape[1])
    thn = _Named([(n, th[n].to(ref.dtype)) for n in cls.parameter_names], "parameter")
    over_time = lambda v: v[:, :, None] if isinstance(v, torch.Tensor) else v  # noqa: E731
    p = _Named([(k, over_time(v)) for k, v in inst.prepare(thn, _Conditions(cs)).items()], "effective parameter")
    if _class_forcings(cls):  # the samples of every time point, [B,1,T] each
        series = _forcing_series(cls, cond, ref, ref.shape[-1] if n_times is None else int(n_times))
        object.__setattr__(inst, "forcing", _Forcings(cls, lambda k, _name: series[:, k, None, :]))
    if _class_algebraic(cls):
        if h.name in _ALGEBRAIC_READERS:  # (observe: the constraint's solution at every time point's state)
            z, _ = _algebraic_torch(cls, inst, list(torch.unbind(groups[0], dim=2)), p, _Conditions([over_time(v) for v in cs]))
            object.__setattr__(inst, "algebraic", _Algebraic(cls, lambda i, _name: z[i]))
        else:
            object.__setattr__(inst, "algebraic", _Algebraic(cls, lambda _i, name: _algebraic_misread(name, h.name)))
    out = getattr(cls, h.attr)(inst, *[list(torch.unbind(v, dim=2)) for v in groups], p, _Conditions([over_time(v) for v in cs]))
    full = lambda v: v.expand_as(ref) if isinstance(v, torch.Tensor) else torch.full_like(ref, float(v))  # noqa: E731
    if h.n_outputs == "channels":  # (one list per channel -> [B,S,N,R,T])
        return torch.stack([torch.stack([full(v) for v in col], dim=2) for col in out], dim=3)
    return torch.stack([full(v) for v in out], dim=2)


def _validate(cls):
    name = cls.__name__
    if not isinstance(cls.model_key, str) or not cls.model_key:
        raise ModelDefinitionError("%s.model_key must be a non-empty string" % name)
    if not cls.species or not all(isinstance(s, str) for s in cls.species):
        raise ModelDefinitionError("%s.species must list the ODE states" % name)
    if not cls.parameter_names or not all(isinstance(s, str) for s in cls.parameter_names):
        raise ModelDefinitionError("%s.parameters must list the theta names the kernel reads" % name)
    if len(set(cls.parameter_names)) != len(cls.parameter_names):
        raise ModelDefinitionError("%s.parameters has duplicates" % name)
    custom = getattr(cls, "_observe_def", None) is not None  # (a map of its own reads whatever species it names)
    if not custom and cls.observe_kind not in OBSERVE_KINDS:
        raise ModelDefinitionError("%s.observe_kind must be one of %s (or define observe(self, y, p, c))"
                                   % (name, sorted(OBSERVE_KINDS)))
    need = 1 if custom else OBSERVE_KINDS[cls.observe_kind][1]
    if len(cls.species) < need:
        raise ModelDefinitionError("%s: observe_kind '%s' reads %d species, the model has %d"
                                   % (name, cls.observe_kind, need, len(cls.species)))
    if len(cls.species) > MAX_STATES:
        raise ModelDefinitionError("%s: %d species; generated models hold at most %d states"
                                   % (name, len(cls.species), MAX_STATES))
    # four more slots follow the model's own: the constant precisions, or the neural precisions' initial values -- unless the
    # model has a precision map of its own (its noise parameters are among its own slots)
    n_prec_slots = 0 if getattr(cls, "_precision_def", None) is not None else 4
    if len(cls.parameter_names) + n_prec_slots > hip.VIHDS_MAX_SLOTS:
        raise ModelDefinitionError("%s: %d parameters; the kernels read at most %d slots (VIHDS_MAX_SLOTS%s)" % (
            name, len(cls.parameter_names), hip.VIHDS_MAX_SLOTS - n_prec_slots,
            ", 4 of them for the precisions" if n_prec_slots else ": a model with a precision map of its own has all of them"))
    if not isinstance(cls.n_conditions, int) or cls.n_conditions < 0:
        raise ModelDefinitionError("%s.n_conditions must be an integer >= 0" % name)
    forc = getattr(cls, "forcings", None) or ()
    if not isinstance(forc, (list, tuple)) or not all(isinstance(f, str) and f.isidentifier() for f in forc):
        raise ModelDefinitionError("%s.forcings must be a list of names (valid identifiers)" % name)
    if len(set(forc)) != len(forc):
        raise ModelDefinitionError("%s.forcings has duplicates" % name)
    clash = [f for f in forc if f in cls.species or f in cls.parameter_names]
    if clash:
        raise ModelDefinitionError("%s.forcings: %s %s also a species or a parameter; a forcing needs a name of its own"
                                   % (name, ", ".join("'%s'" % f for f in clash), "is" if len(clash) == 1 else "are"))
    if len(forc) > MAX_FORCINGS:
        raise ModelDefinitionError("%s: %d forcings; a generated model reads at most %d (MAX_FORCINGS)"
                                   % (name, len(forc), MAX_FORCINGS))
    nets = getattr(cls, "networks", None)
    alg = getattr(cls, "algebraic", None) or ()
    dl = getattr(cls, "delays", None)
    if dl:
        if not isinstance(dl, dict) or not all(
                isinstance(k, str) and k.isidentifier() and isinstance(v, (list, tuple)) and len(v) == 2
                and all(isinstance(x, str) for x in v) for k, v in dl.items()):
            raise ModelDefinitionError("%s.delays must be a dict {name: (species, effective parameter holding the delay)}" % name)
        if len(dl) > MAX_DELAYS:
            raise ModelDefinitionError("%s: %d delays; a generated model reads at most %d (MAX_DELAYS)" % (name, len(dl), MAX_DELAYS))
        clash = [k for k in dl if k in cls.species or k in cls.parameter_names or k in forc or k in alg]
        if clash:
            raise ModelDefinitionError("%s.delays: %s %s also a species, a parameter, a forcing or an algebraic variable; a "
                                       "delayed read needs a name of its own" % (name, ", ".join("'%s'" % k for k in clash),
                                                                                 "is" if len(clash) == 1 else "are"))
        for k, (sp, _par) in dl.items():
            if sp not in cls.species:
                raise ModelDefinitionError("%s.delays: '%s' reads the unknown species '%s' (species: %s)"
                                           % (name, k, sp, ", ".join(cls.species)))
        for has, what, why in (
                (cls.implicit is True, "implicit = True", "the read would be data of the implicit step, and neither the "
                                                          "Jacobian's use of it nor its adjoint is built"),
                (cls.step_tolerance is not None, "step_tolerance = %r" % (cls.step_tolerance,),
                 "the history is stored at the observation points only, and a read inside a trial step has no adjoint path"),
                (cls.substeps != 1, "substeps = %r" % (cls.substeps,), "the history is stored at the observation points only"),
                (cls.lead_in != 0, "lead_in = %r" % (cls.lead_in,), "the history before the first point is the constant stored state"),
                (getattr(cls, "_jump_def", None) is not None, "jump(self, y, p, c)", "the stored history holds the left limits"),
                (bool(nets), "networks", "the adjoint's dump of a network and the history workspace share the aux buffer"),
                (bool(alg), "algebraic variables", "the solve inside rhs_vjp does not pass the read's adjoint on")):
            if has:
                raise ModelDefinitionError("%s has delays and %s: %s -- declined in this version" % (name, what, why))
    if not isinstance(alg, (list, tuple)) or not all(isinstance(a, str) and a.isidentifier() for a in alg):
        raise ModelDefinitionError("%s.algebraic must be a list of names (valid identifiers)" % name)
    chans = getattr(cls, "noise_channels", None) or ()
    if getattr(cls, "_channel_noise_def", None) is not None and getattr(cls, "_diffusion_def", None) is not None:
        raise ModelDefinitionError("%s defines channel_noise(self, y, p, c) together with diffusion(self, y, p, c): a model has one "
                                   "noise term -- a Wiener process per species is one channel per species, so write the diagonal "
                                   "part as channels of its own (or set the inherited hook to None)" % name)
    if chans and getattr(cls, "_channel_noise_def", None) is None:
        raise ModelDefinitionError("%s declares noise_channels without channel_noise(self, y, p, c): the channels are the lists "
                                   "that hook returns, one per name" % name)
    if getattr(cls, "_channel_noise_def", None) is not None:
        if not chans:
            raise ModelDefinitionError("%s defines channel_noise(self, y, p, c) without noise_channels: the class names its "
                                       "channels, noise_channels = [\"tx\", \"deg\", ...], and the hook returns one list per name"
                                       % name)
        if not isinstance(chans, (list, tuple)) or not all(isinstance(k, str) and k.isidentifier() for k in chans):
            raise ModelDefinitionError("%s.noise_channels must be a list of names (valid identifiers)" % name)
        if len(set(chans)) != len(chans):
            raise ModelDefinitionError("%s.noise_channels has duplicates" % name)
        if len(chans) > MAX_NOISE_CHANNELS:
            raise ModelDefinitionError("%s: %d noise channels; a generated model draws for at most %d (MAX_NOISE_CHANNELS: two "
                                       "Philox blocks of four normals per step)" % (name, len(chans), MAX_NOISE_CHANNELS))
        clash = [k for k in chans if k in cls.species or k in cls.parameter_names or k in forc or k in alg or k in (dl or ())]
        if clash:
            raise ModelDefinitionError("%s.noise_channels: %s %s also a species, a parameter, a forcing, an algebraic variable or "
                                       "a delay; a noise channel needs a name of its own"
                                       % (name, ", ".join("'%s'" % k for k in clash), "is" if len(clash) == 1 else "are"))
    noise = _noise_hook(cls)
    if noise is not None:
        # process noise: what does not combine with it in this version, each with its reason
        for has, what, why in (
                (cls.implicit is True, "implicit = True", "a drift-implicit step of an SDE is a scheme of its own, and the implicit "
                                                          "step's adjoint at the stored end state does not know the noise term"),
                (bool(nets), "networks", "the adjoint's dump of a network holds one evaluation per stage, and the noisy step's "
                                         "adjoint evaluates the hook beside them"),
                (bool(alg), "algebraic variables", "the amplitude would read the constraint's solution at the step's start, "
                                                   "which only rhs and observe solve for"),
                (bool(dl), "delays", "the stored history holds one realisation's states, and the read's adjoint does not pass "
                                     "through the noise term"),
                (cls.lead_in != 0, "lead_in = %r" % (cls.lead_in,), "the steps before the first observation point have no step "
                                                                    "index in the noise stream (noise in the lead-in is open)")):
            if has:
                raise ModelDefinitionError("%s defines %s and has %s: %s -- declined in this version"
                                           % (name, noise.signature, what, why))
        seed = cls.noise_seed
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < (1 << 48):
            raise ModelDefinitionError("%s.noise_seed = %r; the seed of the noise key is an int, 0 .. 2^48 - 1 (two words of 24 bits)"
                                       % (name, seed))
    if alg:
        if len(set(alg)) != len(alg):
            raise ModelDefinitionError("%s.algebraic has duplicates" % name)
        clash = [a for a in alg if a in cls.species or a in cls.parameter_names or a in forc]
        if clash:
            raise ModelDefinitionError("%s.algebraic: %s %s also a species, a parameter or a forcing; an algebraic variable "
                                       "needs a name of its own" % (name, ", ".join("'%s'" % a for a in clash),
                                                                    "is" if len(clash) == 1 else "are"))
        if len(alg) > MAX_ALGEBRAIC:
            raise ModelDefinitionError("%s: %d algebraic variables; the matrix of a Newton step on the constraint lives in "
                                       "registers: at most %d (MAX_ALGEBRAIC)" % (name, len(alg), MAX_ALGEBRAIC))
        for what, sig, n_args in (("constraint", "constraint(self, y, z, p, c)", 5),
                                  ("algebraic_start", "algebraic_start(self, y, p, c)", 4)):
            fn = getattr(cls, what, None)
            if fn is None:
                raise ModelDefinitionError("%s declares algebraic variables without %s: the unknowns are defined by "
                                           "constraint(self, y, z, p, c) == 0 and the iteration starts from "
                                           "algebraic_start(self, y, p, c)" % (name, what))
            required = [q for q in inspect.signature(fn).parameters.values()
                        if q.default is q.empty and q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD)] if callable(fn) else []
            if len(required) != n_args:
                raise ModelDefinitionError("%s.%s must be a function %s: it sees the species, the effective parameters and the "
                                           "treatments -- no t" % (name, what, sig))
        it = cls.algebraic_iterations
        if isinstance(it, (bool, np.bool_)) or not isinstance(it, (int, np.integer)) or not 1 <= it <= MAX_NEWTON_ITERATIONS:
            raise ModelDefinitionError("%s.algebraic_iterations = %r; the constraint is solved by a fixed number of Newton "
                                       "iterations, 1 .. %d" % (name, it, MAX_NEWTON_ITERATIONS))
        if cls.implicit:
            raise ModelDefinitionError("%s has algebraic variables and implicit = True: the Jacobian of the reduced system, "
                                       "f_y - f_z g_z^-1 g_y, is not generated (an algebraic model takes the explicit solvers)" % name)
        if nets:
            raise ModelDefinitionError("%s has algebraic variables and networks: the adjoint repeats the value pass of rhs, and "
                                       "the dump of a network holds one evaluation per stage (algebraic variables are for models "
                                       "without networks)" % name)
    if not isinstance(cls.implicit, (bool, np.bool_)):
        raise ModelDefinitionError("%s.implicit must be True or False" % name)
    order = cls.implicit_order
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or order not in (1, 2):
        raise ModelDefinitionError("%s.implicit_order = %r; the order of the implicit scheme is the int 1 (backward Euler) or 2 "
                                   "(the two-stage SDIRK)" % (name, order))
    if order == 2 and not cls.implicit:
        raise ModelDefinitionError("%s has implicit_order = 2 without implicit = True: the order is that of the implicit "
                                   "scheme, which needs the generated Jacobian" % name)
    if cls.implicit:
        it = cls.newton_iterations
        if isinstance(it, bool) or not isinstance(it, (int, np.integer)) or not 1 <= it <= MAX_NEWTON_ITERATIONS:
            raise ModelDefinitionError("%s.newton_iterations = %r; an implicit step runs a fixed number of Newton iterations, "
                                       "1 .. %d" % (name, it, MAX_NEWTON_ITERATIONS))
        if nets:
            raise ModelDefinitionError("%s has implicit = True and networks: the Jacobian of a network with respect to its inputs "
                                       "is not generated (second derivatives would follow in the adjoint)" % name)
        if len(cls.species) > MAX_IMPLICIT_STATES:
            raise ModelDefinitionError("%s has implicit = True and %d species; the matrix of a Newton step lives in registers: at "
                                       "most %d (MAX_IMPLICIT_STATES)" % (name, len(cls.species), MAX_IMPLICIT_STATES))
    if not isinstance(cls.missing_observations, (bool, np.bool_)):
        raise ModelDefinitionError("%s.missing_observations = %r; it is True or False (True: a batch may carry 'observed', "
                                   "[rows, 4, T], 1 where a read exists)" % (name, cls.missing_observations))
    m = cls.substeps
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or not 1 <= m <= MAX_SUBSTEPS:
        raise ModelDefinitionError("%s.substeps = %r; a fixed-grid solver takes a whole number of steps over each observation "
                                   "interval, 1 .. %d (MAX_SUBSTEPS)" % (name, m, MAX_SUBSTEPS))
    if (m - 1) * len(cls.species) > MAX_SUBSTEP_ROWS:
        raise ModelDefinitionError("%s has substeps = %d and %d species: the adjoint keeps (substeps - 1) * species rows of an "
                                   "interval's intermediate states in LDS, at most %d (MAX_SUBSTEP_ROWS)"
                                   % (name, m, len(cls.species), MAX_SUBSTEP_ROWS))
    tol = cls.step_tolerance
    if tol is not None:
        if (not isinstance(tol, (tuple, list)) or len(tol) != 2
                or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in tol)
                or not all(math.isfinite(v) and abs(v) <= _F32_MAX and v >= 0 for v in tol)
                or not any(float(np.float32(v)) > 0 for v in tol)):
            raise ModelDefinitionError("%s.step_tolerance = %r; it is (rtol, atol), two finite float32 numbers >= 0 that are not both "
                                       "0: an interval is accepted where |fine - coarse| <= atol + rtol * max(|fine|, |coarse|) on "
                                       "every species" % (name, tol))
        if m not in STEP_CONTROL_CEILINGS:
            raise ModelDefinitionError("%s has step_tolerance and substeps = %d: with step control substeps is the ceiling of the "
                                       "ladder 1 -> 2 -> 4 -> 8 steps per observation interval, one of %s"
                                       % (name, m, ", ".join(str(c) for c in STEP_CONTROL_CEILINGS)))
        for has, what, why in (
                (bool(nets), "networks", "the adjoint's dump of a network holds one evaluation per stage and observation interval"),
                (_noise_hook(cls) is not None, getattr(_noise_hook(cls), "signature", ""),
                 "the draws are counted by the steps of a fixed count, and the difference of two noisy trial solutions measures "
                 "the noise, not the truncation error")):
            if has:
                raise ModelDefinitionError("%s has step_tolerance and %s: %s -- declined in this version" % (name, what, why))
    if m > 1 and nets:
        raise ModelDefinitionError("%s has substeps = %d and networks: the adjoint's dump of a network holds one evaluation per "
                                   "stage and observation interval (substeps > 1 is for models without networks)" % (name, m))
    L, n = cls.lead_in, cls.lead_in_steps
    if (isinstance(L, (bool, np.bool_)) or not isinstance(L, (int, float, np.integer, np.floating)) or not math.isfinite(L)
            or L < 0 or (L > 0 and not 0 < float(np.float32(L)) < float("inf"))):
        raise ModelDefinitionError("%s.lead_in = %r; the length of the lead-in phase is a number above 0 in the units of `times` "
                                   "(a float32 above 0; the default 0.0: no lead-in)" % (name, L))
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_LEAD_IN_STEPS:
        raise ModelDefinitionError("%s.lead_in_steps = %r; a fixed-grid solver takes a whole number of steps over the lead-in "
                                   "phase, 1 .. %d (MAX_LEAD_IN_STEPS)" % (name, n, MAX_LEAD_IN_STEPS))
    if not L > 0 and n != 1:
        raise ModelDefinitionError("%s has lead_in_steps = %d without lead_in: the steps divide a lead-in phase of length "
                                   "lead_in > 0" % (name, n))
    if L > 0 and (n - 1) * len(cls.species) > MAX_SUBSTEP_ROWS:
        raise ModelDefinitionError("%s has lead_in_steps = %d and %d species: the adjoint keeps (lead_in_steps - 1) * species "
                                   "rows of the lead-in's intermediate states in LDS, at most %d (MAX_SUBSTEP_ROWS)"
                                   % (name, n, len(cls.species), MAX_SUBSTEP_ROWS))
    if L > 0 and nets:
        raise ModelDefinitionError("%s has lead_in = %r and networks: the adjoint's dump of a network holds one evaluation per "
                                   "stage and observation interval, (T-1) x stages (a lead-in phase is for models without "
                                   "networks)" % (name, L))
    st = getattr(cls, "steady_species", None) or ()
    if not isinstance(st, (list, tuple)) or not all(isinstance(a, str) for a in st):
        raise ModelDefinitionError("%s.steady_species must be a list of names out of `species`" % name)
    if not st:
        # (set in this class body; one that removes an inherited solve with steady_species = None keeps what it inherits)
        own = [a for a in ("steady_steps", "steady_first_step", "steady_growth", "steady_rate") if cls.__dict__.get(a) is not None]
        if own:
            raise ModelDefinitionError("%s sets %s without steady_species: the attributes describe the solve for the species "
                                       "steady_species names" % (name, ", ".join(own)))
    else:
        unknown = [a for a in st if a not in cls.species]
        if unknown:
            raise ModelDefinitionError("%s.steady_species: %s %s no species of the model (species: %s)" % (
                name, ", ".join("'%s'" % a for a in unknown), "is" if len(unknown) == 1 else "are", ", ".join(cls.species)))
        if len(set(st)) != len(st):
            raise ModelDefinitionError("%s.steady_species has duplicates" % name)
        if len(st) > MAX_STEADY:
            raise ModelDefinitionError("%s: %d steady species; the matrix of an iteration lives in registers: at most %d "
                                       "(MAX_STEADY)" % (name, len(st), MAX_STEADY))
        fn = getattr(cls, "steady_rate", None)
        if fn is None:
            raise ModelDefinitionError("%s declares steady_species without steady_rate: the steady state is defined by "
                                       "steady_rate(self, y, p, c) == 0" % name)
        required = [q for q in inspect.signature(fn).parameters.values()
                    if q.default is q.empty and q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD)] if callable(fn) else []
        if len(required) != 4:
            raise ModelDefinitionError("%s.steady_rate must be a function steady_rate(self, y, p, c): it sees the species, the "
                                       "effective parameters and the treatments -- no t" % name)
        k = cls.steady_steps
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_STEADY_STEPS:
            raise ModelDefinitionError("%s.steady_steps = %r; the steady state is approached by a fixed number of iterations, an "
                                       "int in 1 .. %d (MAX_STEADY_STEPS)" % (name, k, MAX_STEADY_STEPS))
        for attr, low, strict, what in (("steady_first_step", 0.0, True, "the first pseudo-time step is a finite number above 0"),
                                        ("steady_growth", 1.0, False, "the pseudo-time step grows by a finite factor of at least 1")):
            v = getattr(cls, attr)
            if (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v)
                    or not math.isfinite(float(np.float32(v))) or (float(np.float32(v)) <= low if strict else float(np.float32(v)) < low)):
                raise ModelDefinitionError("%s.%s = %r; %s (as a float32)" % (name, attr, v, what))
        if getattr(cls, "algebraic", None):
            raise ModelDefinitionError("%s has algebraic variables and steady_species: steady_rate cannot read an algebraic "
                                       "variable and the two solves are not combined in this version" % name)
    if nets is None:
        return
    if not isinstance(nets, dict) or not all(isinstance(k, str) and k.isidentifier() and isinstance(v, Network)
                                             for k, v in nets.items()):
        raise ModelDefinitionError("%s.networks must be a dict {name: Network(...)}" % name)
    if len(nets) > MAX_NETWORKS:
        raise ModelDefinitionError("%s: %d networks; a generated model holds at most %d" % (name, len(nets), MAX_NETWORKS))
    for k, net in nets.items():
        for what, v, top in (("n_inputs", net.n_inputs, MAX_NET_INPUTS), ("n_hidden", net.n_hidden, MAX_NET_HIDDEN),
                             ("n_outputs", net.n_outputs, MAX_NET_OUTPUTS)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
                raise ModelDefinitionError("%s: network '%s' has %s = %r; supported: 1 .. %d" % (name, k, what, v, top))
        if net.hidden not in NET_ACTIVATIONS:
            raise ModelDefinitionError("%s: network '%s' has hidden = %r; supported: %s"
                                       % (name, k, net.hidden, ", ".join(NET_ACTIVATIONS)))
