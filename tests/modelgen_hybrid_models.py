"""Hybrid models for the tests of vihds.modelgen's networks: a growth law with two latent species driven by a 5 -> 8 -> 4
ReLU network in the form of the reference's NeuralStates (vihds/ode.py:119-138: sigmoid production minus sigmoid
degradation times the state) and a 3 -> 4 -> 1 tanh network gating the mechanistic expression rate; the same class without
networks (sigmoid(0) in their place); and a model with two networks of the largest supported size."""
from vihds.modelgen import GeneratedOdeModel, Network, clamp, sigmoid
from vihds.precisions import ConstantPrecisions, NeuralPrecisions

PREC = ["prec_x", "prec_rfp", "prec_yfp", "prec_cfp"]


class _Growth(GeneratedOdeModel):
    """Shared mechanistic part (no model_key: not a model by itself)."""
    species = ["OD", "RFP", "YFP", "CFP", "Z1", "Z2"]
    parameters = ["r", "K", "tlag", "rc", "drfp", "dyfp", "dcfp", "aYFP", "aCFP", "e76",
                  "init_x", "init_rfp", "init_yfp", "init_cfp"]
    n_conditions = 1
    observe_kind = "direct"

    def __init__(self, config):
        super(_Growth, self).__init__(config)
        self.precisions = ConstantPrecisions(PREC)

    def prepare(self, th, c):
        return {"r": clamp(th.r, 0.0, 4.0), "K": clamp(th.K, 0.0, 4.0), "tlag": th.tlag, "rc": th.rc,
                "drfp": clamp(th.drfp, 1e-12, 2.0), "dyfp": clamp(th.dyfp, 1e-12, 2.0),
                "dcfp": clamp(th.dcfp, 1e-12, 2.0), "aYFP": th.aYFP, "aCFP": th.aCFP, "e76": th.e76}

    def initial_state(self, th, c):
        return [th.init_x, th.init_rfp, th.init_yfp, th.init_cfp, 0.0, 0.0]

    def dynamics(self, t, y, p, heads, gate):
        """heads: production of Z1, Z2, degradation of Z1, Z2 (each in (0, 1)); gate in (0, 1) scales the expression rate."""
        x, rfp, yfp, cfp, z1, z2 = y
        gamma = p.r * sigmoid(4.0 * (t - p.tlag)) * (1.0 - x / p.K)
        rate = p.rc * gate
        return [gamma * x,
                rate - (gamma + p.drfp) * rfp,
                rate * p.aYFP * z1 - (gamma + p.dyfp) * yfp,
                rate * p.aCFP * z2 - (gamma + p.dcfp) * cfp,
                heads[0] - heads[2] * z1,
                heads[1] - heads[3] * z2]


class GrowthWithLatents(_Growth):
    model_key = "gen_growth_latents"
    networks = {"latent": Network(n_inputs=5, n_hidden=8, n_outputs=4, hidden="relu"),
                "gate": Network(n_inputs=3, n_hidden=4, n_outputs=1, hidden="tanh")}

    def rhs(self, t, y, p, c):
        o = self.net.latent([y[4], y[5], y[0], p.e76, c[0]])
        g = self.net.gate([t, y[0], y[4]])
        return self.dynamics(t, y, p, [sigmoid(v) for v in o], sigmoid(g[0]))


class GrowthWithLatentsPrecisions(GrowthWithLatents):
    model_key = "gen_growth_latents_precisions"

    def __init__(self, config):
        super(GrowthWithLatentsPrecisions, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)


class GrowthWithoutNetworks(_Growth):
    """GrowthWithLatents with sigmoid(0) where its networks' heads are."""
    model_key = "gen_growth_no_networks"

    def rhs(self, t, y, p, c):
        return self.dynamics(t, y, p, [0.5, 0.5, 0.5, 0.5], 0.5)


class LargestNetworks(_Growth):
    """Two networks of the largest supported size (16 -> 32 -> 8), one per activation."""
    model_key = "gen_largest_networks"
    networks = {"a": Network(16, 32, 8, "relu"), "b": Network(16, 32, 8, "tanh")}

    def rhs(self, t, y, p, c):
        x = list(y) + [t, c[0], p.r, p.K, p.tlag, p.rc, p.drfp, p.dyfp, p.dcfp, p.e76]
        o = self.net.a(x)
        q = self.net.b([v * x[0] for v in x[:8]] + x[8:])
        heads = [sigmoid(o[j] + q[j + 4]) for j in range(4)]
        gate = sigmoid(o[4] * q[0] + o[5] * q[1] + o[6] * q[2] + o[7] * q[3])
        return self.dynamics(t, y, p, heads, gate)


class LargestNetworksPrecisions(LargestNetworks):
    model_key = "gen_largest_networks_precisions"

    def __init__(self, config):
        super(LargestNetworksPrecisions, self).__init__(config)
        self.precisions = NeuralPrecisions(self.n_species, config.params.n_hidden_decoder_precisions, 4)


# (class, neural precisions) of every library the GPU tests use: __graft_entry__.build() compiles them ahead
PREBUILT = [(GrowthWithLatents, False), (GrowthWithLatentsPrecisions, True), (GrowthWithoutNetworks, False)]
