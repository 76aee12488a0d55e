"""Models with an observation map of their own (GeneratedOdeModel.observe) for the tests: the default map restated on top
of the prpr_constant restatement, inducer_constant (whose map -- models/inducer_constant.py:106-114 -- is neither of the
fixed kinds a generated model can name) and a reader model whose map has parameters."""
from vihds.modelgen import GeneratedOdeModel, clamp, exp, pow, sigmoid
from vihds.precisions import ConstantPrecisions, NeuralPrecisions

from modelgen_models import PREC, PrprRestated, PrprRestatedPrecisions


def _default_map(y):
    return [y[0], y[0] * y[1], y[0] * (y[2] + y[4]), y[0] * (y[3] + y[5])]


class PrprOwnMap(PrprRestated):
    """PrprRestated with the default map (reference ode.py:84-93) written as the model's own."""
    model_key = "gen_prpr_constant_own_map"

    def observe(self, y, p, c):
        return _default_map(y)


class PrprOwnMapPrecisions(PrprRestatedPrecisions):
    model_key = "gen_prpr_constant_precisions_own_map"

    def observe(self, y, p, c):
        return _default_map(y)


class InducerRestated(GeneratedOdeModel):
    """inducer_constant_precisions restated (csrc InducerConstant; reference models/inducer_constant.py:11-80, x0 :92-97,
    observe :106-114): five species, one treatment (arabinose), [OD, OD*RFP, OD*(YFP+F530), OD*F480]."""
    model_key = "gen_inducer_constant_precisions"
    species = ["OD", "RFP", "YFP", "F530", "F480"]
    parameters = ["r", "K", "tlag", "rc", "a530", "a480", "drfp", "dyfp", "aYFP_Inducer", "nA", "eA", "KAra",
                  "init_x", "init_rfp", "init_yfp"]
    n_conditions = 1

    def __init__(self, config):
        super(InducerRestated, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)

    def prepare(self, th, c):
        nA = clamp(th.nA, 0.5, 3.0)
        an, kn = pow(c[0], nA), pow(th.KAra, nA)
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc, "a530": th.a530,
                "a480": th.a480, "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0),
                "aYFP": th.aYFP_Inducer, "PBAD": (an + th.eA * kn) / (an + kn)}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, 0.0, 0.0]

    def rhs(self, t, y, p, c):
        x, rfp, yfp, f530, f480 = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        return [gamma * x,
                p.rc - (gamma + p.drfp) * rfp,
                p.rc * p.aYFP * p.PBAD - (gamma + p.dyfp) * yfp,
                p.rc * p.a530 - gamma * f530,
                p.rc * p.a480 - gamma * f480]

    def observe(self, y, p, c):
        x, rfp, yfp, f530, f480 = y
        return [x, x * rfp, x * (yfp + f530), x * f480]


class PlateReader(GeneratedOdeModel):
    """Three species and a plate reader: the signals have a gain, a background, a saturating response and an
    autofluorescence that scales with the treatment -- none of them an ODE state.  `gain_r`, `bg_r`, `sat`, `auto` and the
    clamped `leak` are read by observe only; the treatment is read by observe and by prepare, not by rhs."""
    model_key = "gen_plate_reader"
    species = ["OD", "RFP", "YFP"]
    parameters = ["r", "K", "tlag", "rc", "drfp", "dyfp", "aYFP", "gain_r", "bg_r", "sat", "auto", "leak",
                  "init_x", "init_rfp", "init_yfp"]
    n_conditions = 1

    def __init__(self, config):
        super(PlateReader, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc,
                "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0),
                "aYFP": th.aYFP * c[0] / (1.0 + c[0]), "gain_r": th.gain_r, "bg_r": th.bg_r, "sat": th.sat,
                "auto": th.auto, "leak": clamp(th.leak, 0.0, 0.5)}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp]

    def rhs(self, t, y, p, c):
        x, rfp, yfp = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        return [gamma * x, p.rc - (gamma + p.drfp) * rfp, p.rc * p.aYFP - (gamma + p.dyfp) * yfp]

    def observe(self, y, p, c):
        x, rfp, yfp = y
        return [x,
                p.gain_r * x * rfp + p.bg_r,
                x * yfp / (1.0 + p.sat * yfp) + p.leak * x * rfp,
                x * p.auto * c[0] * sigmoid(x - 1.0) + exp(-x) * p.leak]


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(PrprOwnMap, False), (PrprOwnMapPrecisions, True), (InducerRestated, True), (PlateReader, False)]
