"""Models written with vihds.modelgen for the tests: prpr_constant and dr_constant (version 1) restated (reference
models/prpr_constant.py:13-85, models/dr_constant.py:14-150: the equations of oracle.make_prpr_constant / make_dr_constant), a
LuxR-only receiver that is not built in, and a model that uses every operation."""
from vihds.modelgen import GeneratedOdeModel, clamp, exp, log, pow, sigmoid, tanh
from vihds.precisions import ConstantPrecisions, NeuralPrecisions

PREC = ["prec_x", "prec_rfp", "prec_yfp", "prec_cfp"]


class PrprRestated(GeneratedOdeModel):
    model_key = "gen_prpr_constant"
    species = ["OD", "RFP", "YFP", "CFP", "F530", "F480"]
    parameters = ["r", "K", "tlag", "rc", "drfp", "dyfp", "dcfp", "aYFP_PR", "aCFP_PR", "a530", "a480",
                  "init_x", "init_rfp", "init_yfp", "init_cfp"]
    n_conditions = 0
    observe_kind = "default"

    def __init__(self, config):
        super(PrprRestated, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc,
                "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0),
                "dcfp": clamp(th.dcfp, 1e-12, 2.0), "aYFP": th.aYFP_PR, "aCFP": th.aCFP_PR, "a530": th.a530,
                "a480": th.a480}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, th.init_cfp, 0.0, 0.0]

    def rhs(self, t, y, p, c):
        x, rfp, yfp, cfp, f530, f480 = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        return [gamma * x,
                p.rc - (gamma + p.drfp) * rfp,
                p.rc * p.aYFP - (gamma + p.dyfp) * yfp,
                p.rc * p.aCFP - (gamma + p.dcfp) * cfp,
                p.rc * p.a530 - gamma * f530,
                p.rc * p.a480 - gamma * f480]


class PrprRestatedPrecisions(PrprRestated):
    model_key = "gen_prpr_constant_precisions"

    def __init__(self, config):
        super(PrprRestatedPrecisions, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)


class LuxReceiver(GeneratedOdeModel):
    """A LuxR-only receiver (not a built-in model): growth, LuxR expressed constitutively, and a Hill term in both
    treatments whose exponent is a parameter, driving YFP and CFP through one promoter."""
    model_key = "gen_lux_receiver"
    species = ["OD", "RFP", "YFP", "CFP", "F530", "F480", "LuxR"]
    parameters = ["r", "K", "tlag", "rc", "drfp", "dyfp", "dcfp", "dR", "aYFP", "aCFP", "a530", "a480", "aR", "e76",
                  "KGR", "nR", "KR6", "KR12", "init_x", "init_rfp", "init_yfp", "init_cfp", "init_luxR"]
    n_conditions = 2
    observe_kind = "default"

    def __init__(self, config):
        super(LuxReceiver, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        nR = clamp(th.nR, 0.5, 3.0)
        a = clamp(th.KR6, 1e-12, 1.0) * c[0]
        b = clamp(th.KR12, 1e-12, 1.0) * c[1]
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc,
                "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0),
                "dcfp": clamp(th.dcfp, 1e-12, 2.0), "dR": clamp(th.dR, 1e-12, 5.0), "aYFP": th.aYFP, "aCFP": th.aCFP,
                "a530": th.a530, "a480": th.a480, "aR": th.aR, "e76": th.e76, "KGR": th.KGR,
                "fR": (pow(a, nR) + pow(b, nR)) / pow(1.0 + a + b, nR)}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, th.init_cfp, 0.0, 0.0, th.init_luxR]

    def rhs(self, t, y, p, c):
        x, rfp, yfp, cfp, f530, f480, luxR = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        bR = luxR * luxR * p.fR
        P76 = (p.e76 + p.KGR * bR) / (1.0 + p.KGR * bR)
        return [gamma * x,
                p.rc - (gamma + p.drfp) * rfp,
                p.rc * p.aYFP * P76 - (gamma + p.dyfp) * yfp,
                p.rc * p.aCFP * P76 - (gamma + p.dcfp) * cfp,
                p.rc * p.a530 - gamma * f530,
                p.rc * p.a480 - gamma * f480,
                p.rc * p.aR - (gamma + p.dR) * luxR]


class LuxReceiverPrecisions(LuxReceiver):
    model_key = "gen_lux_receiver_precisions"

    def __init__(self, config):
        super(LuxReceiverPrecisions, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)


class DrRestated(GeneratedOdeModel):
    """dr_constant version 1 with its device conditioning: aR / aS are conditioned on the device (condition_ones, the
    reference's device_conditioner on the ones-vector, dr_constant.py:124-131) in rows reserved behind theta."""
    model_key = "gen_dr_constant"
    extra_theta_names = ("aR", "aS")
    species = ["OD", "RFP", "YFP", "CFP", "F530", "F480", "LuxR", "LasR"]
    parameters = ["r", "K", "tlag", "rc", "drfp", "dyfp", "dcfp", "dR", "dS", "e76", "e81", "KGR_76", "KGS_76", "KGR_81",
                  "KGS_81", "aYFP", "aCFP", "a530", "a480", "aR", "aS", "nR", "nS", "KR6", "KR12", "KS6", "KS12",
                  "init_x", "init_rfp", "init_yfp", "init_cfp", "init_luxR", "init_lasR"]
    n_conditions = 2
    observe_kind = "default"

    def __init__(self, config):
        super(DrRestated, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def condition_theta(self, theta, dev_1hot, writer, epoch):
        return self.condition_ones(theta, ["aR", "aS"], dev_1hot)

    def prepare(self, th, c):
        def hill(n, k6, k12):
            n = clamp(n, 0.5, 3.0)
            a, b = clamp(k6, 1e-12, 1.0) * c[0], clamp(k12, 1e-12, 1.0) * c[1]
            return (pow(a, n) + pow(b, n)) / pow(1.0 + a + b, n)

        p = {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc,
             "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0), "dcfp": clamp(th.dcfp, 1e-12, 2.0),
             "dR": clamp(th.dR, 1e-12, 5.0), "dS": clamp(th.dS, 1e-12, 5.0),
             "fR": hill(th.nR, th.KR6, th.KR12), "fS": hill(th.nS, th.KS6, th.KS12)}
        for n in ("e76", "e81", "KGR_76", "KGS_76", "KGR_81", "KGS_81", "aYFP", "aCFP", "a530", "a480", "aR", "aS"):
            p[n] = th[n]
        return p

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, th.init_cfp, 0.0, 0.0, th.init_luxR, th.init_lasR]

    def rhs(self, t, y, p, c):
        x, rfp, yfp, cfp, f530, f480, luxR, lasR = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        bR, bS = luxR * luxR * p.fR, lasR * lasR * p.fS
        P76 = (p.e76 + p.KGR_76 * bR + p.KGS_76 * bS) / (1.0 + p.KGR_76 * bR + p.KGS_76 * bS)
        P81 = (p.e81 + p.KGR_81 * bR + p.KGS_81 * bS) / (1.0 + p.KGR_81 * bR + p.KGS_81 * bS)
        return [gamma * x,
                p.rc - (gamma + p.drfp) * rfp,
                p.rc * p.aYFP * P81 - (gamma + p.dyfp) * yfp,
                p.rc * p.aCFP * P76 - (gamma + p.dcfp) * cfp,
                p.rc * p.a530 - gamma * f530,
                p.rc * p.a480 - gamma * f480,
                p.rc * p.aR - (gamma + p.dR) * luxR,
                p.rc * p.aS - (gamma + p.dS) * lasR]


class EveryOperation(GeneratedOdeModel):
    """Every operation of the namespace in prepare (accurate maths) and in rhs (the time-loop helpers)."""
    model_key = "gen_every_operation"
    species = ["OD", "A", "B", "C"]
    parameters = ["r", "k", "n", "h", "init_x"]
    n_conditions = 1
    observe_kind = "direct"

    def prepare(self, th, c):
        k = clamp(th.k, 1e-6, 10.0)
        return {"r": exp(th.r) / (1.0 + k), "k": log(1.0 + k * c[0]), "n": pow(k, th.n), "h": tanh(th.h) - sigmoid(th.h)}

    def initial_state(self, th, c):
        return [th.init_x, 0.5 * th.init_x + 1.0, 0.0, -th.init_x]

    def rhs(self, t, y, p, c):
        x, a, b, d = y
        return [p.r * x * (1.0 - x / p.n),
                exp(-a) * p.k - log(1.0 + a * a) / (1.0 + t),
                tanh(b - p.h) + sigmoid(pow(1.0 + x * x, p.n)) * c[0],
                -clamp(d, -1.0, 1.0) * pow(x, 2.0) - 1.0 / (1.0 + b * b)]


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(PrprRestated, False), (PrprRestatedPrecisions, True), (LuxReceiver, False), (LuxReceiverPrecisions, True),
            (DrRestated, False)]
