"""Models with an observation log density of their own (GeneratedOdeModel.log_likelihood) for the tests: the Gaussian written
out on the prpr_constant restatement, a Student-t on the plate reader with its own map and its own noise, a two-component
scale mixture whose weight and width only the likelihood reads, and log-scale noise (a nonlinear operation on the
observations)."""
import math

from vihds.modelgen import exp, log, sigmoid

from modelgen_models import PrprRestated
from modelgen_noise_models import PlateReaderNoise

LOG2PI = math.log(2.0 * math.pi)
NU = 4.0  # degrees of freedom of PlateReaderStudentT
# log Gamma((nu + 1) / 2) - log Gamma(nu / 2) - log(nu pi) / 2: a Python number, folded into the generated text
STUDENT_T_CONST = math.lgamma(0.5 * (NU + 1.0)) - math.lgamma(0.5 * NU) - 0.5 * math.log(NU * math.pi)
CONTAMINATION = ["eps", "kappa"]  # (read by log_likelihood only)


class PrprGaussianThrough(PrprRestated):
    """PrprRestated (constant precisions, the default map) with the kernels' Gaussian written as the model's own."""
    model_key = "gen_prpr_constant_gaussian_through"

    def log_likelihood(self, x, obs, pr, p, c):
        return [-0.5 * (LOG2PI - log(pr[j]) + pr[j] * (x[j] - obs[j]) * (x[j] - obs[j])) for j in range(4)]


class PlateReaderStudentT(PlateReaderNoise):
    """PlateReaderNoise (its own observe, its own precision) with a Student-t of NU degrees of freedom whose scale is
    1 / sqrt(precision): heavy tails for the outliers of a plate reader."""
    model_key = "gen_plate_reader_student_t"

    def log_likelihood(self, x, obs, pr, p, c):
        def t(j):
            e = x[j] - obs[j]
            return STUDENT_T_CONST + 0.5 * log(pr[j]) - 0.5 * (NU + 1.0) * log(1.0 + pr[j] * e * e / NU)
        return [t(j) for j in range(4)]


class PrprContaminated(PrprRestated):
    """PrprRestated with a contaminated Gaussian: with probability w = sigmoid(eps) a reading comes from a Gaussian whose
    standard deviation is kappa times wider.  eps and kappa are read by log_likelihood only; the precisions stay the
    constant slots."""
    model_key = "gen_prpr_constant_contaminated"
    parameters = PrprRestated.parameter_names + CONTAMINATION

    def prepare(self, th, c):
        p = PrprRestated.prepare(self, th, c)
        p.update({"w": sigmoid(th.eps), "kappa": th.kappa})
        return p

    def log_likelihood(self, x, obs, pr, p, c):
        def mix(j):
            # log((1 - w) N(e; 1 / pr) + w N(e; kappa^2 / pr)) with the wide component factored out: the exponent left inside the
            # logarithm is <= 0 for kappa >= 1, so a residual of hundreds of standard deviations underflows to log(w / kappa), not
            # to log(0)
            q = pr[j] * (x[j] - obs[j]) * (x[j] - obs[j])
            k2 = p.kappa * p.kappa
            inner = p.w / p.kappa + (1.0 - p.w) * exp(-0.5 * q * (1.0 - 1.0 / k2))
            return 0.5 * log(pr[j]) - 0.5 * LOG2PI - 0.5 * q / k2 + log(inner)
        return [mix(j) for j in range(4)]


class PrprLogNormal(PrprRestated):
    """PrprRestated with noise on the log scale: log obs ~ Normal(log x, 1 / pr): a nonlinear operation on the
    observations, which are a forward-only leaf, and a density that is singular at obs = 0."""
    model_key = "gen_prpr_constant_log_normal"

    def log_likelihood(self, x, obs, pr, p, c):
        def ln(j):
            e = log(x[j]) - log(obs[j])
            return -0.5 * (LOG2PI - log(pr[j]) + pr[j] * e * e) - log(obs[j])
        return [ln(j) for j in range(4)]


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(PrprGaussianThrough, False), (PlateReaderStudentT, False), (PrprContaminated, False), (PrprLogNormal, False)]
