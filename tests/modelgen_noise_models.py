"""Models with a precision map of their own (GeneratedOdeModel.precision) for the tests: the prpr_constant restatement with
four parameters handed through as the precisions, a plate reader whose noise has a floor and a part proportional to each
signal, and the same noise on the hybrid model with networks in rhs."""
from vihds.modelgen import GeneratedOdeModel, pow

from modelgen_hybrid_models import GrowthWithLatents, _Growth
from modelgen_models import PrprRestated
from modelgen_observe_models import PlateReader

PASS_THROUGH = ["pt_x", "pt_rfp", "pt_yfp", "pt_cfp"]  # (where PrprRestated has the slots prec_x .. prec_cfp)
NOISE = ["s0_od", "s1_od", "s0_r", "s1_r", "s0_y", "s1_y", "s0_c", "s1_c", "s_dens", "s_trt"]


def _signal_dependent(y, x, p, c):
    """Variance = floor^2 + (slope * signal)^2 per signal; the RFP channel also scatters with the cell density (a species read
    directly), the CFP channel with the treatment."""
    var = lambda s0, s1, xj: s0 * s0 + pow(s1 * xj, 2.0)  # noqa: E731
    return [1.0 / var(p.s0_od, p.s1_od, x[0]),
            1.0 / (var(p.s0_r, p.s1_r, x[1]) + pow(p.s_dens * y[0], 2.0)),
            1.0 / var(p.s0_y, p.s1_y, x[2]),
            1.0 / (var(p.s0_c, p.s1_c, x[3]) + p.s_trt * p.s_trt * c[0] / (1.0 + c[0]))]


class PrprPassThrough(PrprRestated):
    """PrprRestated with four more parameters that precision returns unchanged: the constant precisions as the model's own."""
    model_key = "gen_prpr_constant_pass_through"
    parameters = PrprRestated.parameter_names + PASS_THROUGH

    def __init__(self, config):
        GeneratedOdeModel.__init__(self, config)  # (PrprRestated's would assign ConstantPrecisions)

    def prepare(self, th, c):
        p = PrprRestated.prepare(self, th, c)
        p.update({n: th[n] for n in PASS_THROUGH})
        return p

    def precision(self, y, x, p, c):
        return [p[n] for n in PASS_THROUGH]


class PlateReaderNoise(PlateReader):
    """PlateReader (its own observe) with signal-dependent noise: every noise parameter is read by precision only."""
    model_key = "gen_plate_reader_noise"
    parameters = PlateReader.parameter_names + NOISE

    def __init__(self, config):
        GeneratedOdeModel.__init__(self, config)

    def prepare(self, th, c):
        p = PlateReader.prepare(self, th, c)
        p.update({n: th[n] for n in NOISE})
        return p

    def precision(self, y, x, p, c):
        return _signal_dependent(y, x, p, c)


class GrowthWithLatentsNoise(GrowthWithLatents):
    """The hybrid model (two networks in rhs, the fixed 'direct' map) with the plate reader's noise."""
    model_key = "gen_growth_latents_noise"
    parameters = _Growth.parameter_names + NOISE

    def __init__(self, config):
        GeneratedOdeModel.__init__(self, config)

    def prepare(self, th, c):
        p = _Growth.prepare(self, th, c)
        p.update({n: th[n] for n in NOISE})
        return p

    def precision(self, y, x, p, c):
        return _signal_dependent(y, x, p, c)


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(PrprPassThrough, False), (PlateReaderNoise, False), (GrowthWithLatentsNoise, False)]
