"""Host model of the Temporal Fusion Transformer (arXiv 1912.09363) as the reference recipe PyTorch/Forecasting/TFT builds it.

Module names and parameter shapes are the reference's, so its state_dict loads by name (the never-used
static_encoder.vsn.joint_grn.lin_c.weight and the attention._mask buffer included).  This model is the torch-operator statement of
the network: it loads checkpoints of any hidden size and is what tft/infer.py packs its kernels' weights from.  Inference only:
every dropout of the reference is the identity here.
"""
import enum
import io
import pickle
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

LN_EPS = 1e-3


class InputTypes(enum.IntEnum):
    TARGET, OBSERVED, KNOWN, STATIC, ID, TIME = range(6)


class DataTypes(enum.IntEnum):
    CONTINUOUS, CATEGORICAL, DATE, STR = range(4)


FeatureSpec = namedtuple("FeatureSpec", ["name", "feature_type", "feature_embed_type"])


class TFTConfig:
    """One dataset configuration.  Subclasses give the columns; the sizes the model needs are derived from them."""
    features = ()
    static_categorical_inp_lens = ()
    temporal_known_categorical_inp_lens = ()
    temporal_observed_categorical_inp_lens = ()
    quantiles = (0.1, 0.5, 0.9)
    example_length = 8 * 24
    encoder_length = 7 * 24
    n_head = 4
    hidden_size = 128
    dropout = 0.1
    attn_dropout = 0.0
    dataset_stride = 1
    missing_id_strategy = None
    missing_cat_data_strategy = "encode_all"

    def __init__(self, **overrides):
        for k in ("features", "static_categorical_inp_lens", "temporal_known_categorical_inp_lens",
                  "temporal_observed_categorical_inp_lens", "quantiles"):
            setattr(self, k, list(getattr(type(self), k)))
        for k, v in overrides.items():
            setattr(self, k, v)
        self.derive()

    def _count(self, kind, embed=DataTypes.CONTINUOUS):
        return sum(1 for f in self.features if f.feature_type == kind and f.feature_embed_type == embed)

    def derive(self):
        self.temporal_known_continuous_inp_size = self._count(InputTypes.KNOWN)
        self.temporal_observed_continuous_inp_size = self._count(InputTypes.OBSERVED)
        self.static_continuous_inp_size = self._count(InputTypes.STATIC)
        self.temporal_target_size = sum(1 for f in self.features if f.feature_type == InputTypes.TARGET)
        self.num_static_vars = self.static_continuous_inp_size + len(self.static_categorical_inp_lens)
        self.num_future_vars = self.temporal_known_continuous_inp_size + len(self.temporal_known_categorical_inp_lens)
        self.num_historic_vars = (self.num_future_vars + self.temporal_observed_continuous_inp_size + self.temporal_target_size +
                                  len(self.temporal_observed_categorical_inp_lens))

    def __setstate__(self, state):
        # a pickled reference config carries its derived sizes; one written by this package may not
        self.__dict__.update(state)
        if "num_historic_vars" not in state:
            self.derive()


def _series_features(target):
    return (FeatureSpec("id", InputTypes.ID, DataTypes.CATEGORICAL),
            FeatureSpec("hours_from_start", InputTypes.TIME, DataTypes.CONTINUOUS),
            FeatureSpec(target, InputTypes.TARGET, DataTypes.CONTINUOUS))


class ElectricityConfig(TFTConfig):
    features = _series_features("power_usage") + (
        FeatureSpec("hour", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("day_of_week", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("hours_from_start", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("categorical_id", InputTypes.STATIC, DataTypes.CATEGORICAL))
    time_ids = "days_from_start"
    train_range, valid_range, test_range = (1096, 1315), (1308, 1339), (1332, 1346)
    scale_per_id = True
    static_categorical_inp_lens = (369,)
    dropout = 0.1


class TrafficConfig(TFTConfig):
    features = _series_features("values") + (
        FeatureSpec("time_on_day", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("day_of_week", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("hours_from_start", InputTypes.KNOWN, DataTypes.CONTINUOUS),
        FeatureSpec("categorical_id", InputTypes.STATIC, DataTypes.CATEGORICAL))
    time_ids = "sensor_day"
    train_range, valid_range, test_range = (0, 151), (144, 166), (159, float("inf"))
    scale_per_id = False
    static_categorical_inp_lens = (963,)
    dropout = 0.3


CONFIGS = {"electricity": ElectricityConfig, "traffic": TrafficConfig}


class MaybeLayerNorm(nn.Module):
    def __init__(self, output_size, hidden_size, eps):
        super().__init__()
        self.ln = nn.Identity() if output_size == 1 else nn.LayerNorm(output_size or hidden_size, eps=eps)

    def forward(self, x):
        return self.ln(x)


class GLU(nn.Module):
    def __init__(self, hidden_size, output_size):
        super().__init__()
        self.lin = nn.Linear(hidden_size, 2 * output_size)

    def forward(self, x):
        return F.glu(self.lin(x))


class GRN(nn.Module):
    def __init__(self, input_size, hidden_size, output_size=None, context_hidden_size=None):
        super().__init__()
        self.layer_norm = MaybeLayerNorm(output_size, hidden_size, LN_EPS)
        self.lin_a = nn.Linear(input_size, hidden_size)
        self.lin_c = nn.Linear(context_hidden_size, hidden_size, bias=False) if context_hidden_size is not None else nn.Identity()
        self.lin_i = nn.Linear(hidden_size, hidden_size)
        self.glu = GLU(hidden_size, output_size or hidden_size)
        self.out_proj = nn.Linear(input_size, output_size) if output_size else None

    def forward(self, a, c=None):
        x = self.lin_a(a)
        if c is not None:
            x = x + self.lin_c(c).unsqueeze(1)
        x = self.glu(self.lin_i(F.elu(x)))
        return self.layer_norm(x + (a if self.out_proj is None else self.out_proj(a)))


class TFTEmbedding(nn.Module):
    """Static categorical tables and the rank-1 embeddings x * vector + bias of the continuous variables."""

    def __init__(self, config):
        super().__init__()
        if config.temporal_known_categorical_inp_lens or config.temporal_observed_categorical_inp_lens:
            raise NotImplementedError("TFT: temporal categorical inputs (k_cat / o_cat) occur in neither published dataset and are not supported")
        H = config.hidden_size
        self.s_cat_embed = nn.ModuleList([nn.Embedding(n, H) for n in config.static_categorical_inp_lens]) \
            if config.static_categorical_inp_lens else None
        self.t_cat_k_embed = None
        self.t_cat_o_embed = None
        for prefix, n in (("s_cont", config.static_continuous_inp_size), ("t_cont_k", config.temporal_known_continuous_inp_size),
                          ("t_cont_o", config.temporal_observed_continuous_inp_size), ("t_tgt", config.temporal_target_size)):
            if n:
                vec = nn.Parameter(torch.empty(n, H))
                nn.init.xavier_normal_(vec)
                setattr(self, prefix + "_embedding_vectors", vec)
                setattr(self, prefix + "_embedding_bias", nn.Parameter(torch.zeros(n, H)))
            else:
                setattr(self, prefix + "_embedding_vectors", None)
                setattr(self, prefix + "_embedding_bias", None)

    def _cont(self, x, prefix):
        vec = getattr(self, prefix + "_embedding_vectors")
        if x is None or vec is None:
            return None
        return x.unsqueeze(-1) * vec + getattr(self, prefix + "_embedding_bias")

    def forward(self, batch):
        if batch.get("k_cat") is not None or batch.get("o_cat") is not None:
            raise NotImplementedError("TFT: temporal categorical inputs (k_cat / o_cat) are not supported")
        s_cat, s_cont = batch.get("s_cat"), batch.get("s_cont")
        parts = []
        if s_cat is not None and self.s_cat_embed is not None:
            parts.append(torch.stack([e(s_cat[:, 0, i]) for i, e in enumerate(self.s_cat_embed)], dim=-2))
        if s_cont is not None:
            parts.append(self._cont(s_cont[:, 0, :], "s_cont"))
        s_inp = torch.cat(parts, dim=-2)
        return s_inp, self._cont(batch.get("k_cont"), "t_cont_k"), self._cont(batch.get("o_cont"), "t_cont_o"), \
            self._cont(batch["target"], "t_tgt")


class VariableSelectionNetwork(nn.Module):
    def __init__(self, config, num_inputs):
        super().__init__()
        H = config.hidden_size
        self.joint_grn = GRN(H * num_inputs, H, output_size=num_inputs, context_hidden_size=H)
        self.var_grns = nn.ModuleList([GRN(H, H) for _ in range(num_inputs)])

    def forward(self, x, context=None):
        weights = F.softmax(self.joint_grn(torch.flatten(x, start_dim=-2), c=context), dim=-1)
        per_var = torch.stack([g(x[..., i, :]) for i, g in enumerate(self.var_grns)], dim=-1)
        return torch.matmul(per_var, weights.unsqueeze(-1)).squeeze(-1), weights


class StaticCovariateEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.vsn = VariableSelectionNetwork(config, config.num_static_vars)
        self.context_grns = nn.ModuleList([GRN(config.hidden_size, config.hidden_size) for _ in range(4)])

    def forward(self, x):
        ctx, _ = self.vsn(x)
        return tuple(g(ctx) for g in self.context_grns)           # cs, ce, ch, cc


class InterpretableMultiHeadAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        H = config.hidden_size
        if H % config.n_head:
            raise ValueError("TFT: hidden_size %d is not a multiple of n_head %d" % (H, config.n_head))
        self.n_head, self.d_head = config.n_head, H // config.n_head
        self.qkv_linears = nn.Linear(H, (2 * self.n_head + 1) * self.d_head, bias=False)
        self.out_proj = nn.Linear(self.d_head, H, bias=False)
        self.scale = self.d_head ** -0.5
        T = config.example_length
        self.register_buffer("_mask", torch.triu(torch.full((T, T), float("-inf")), 1).unsqueeze(0))

    def forward(self, x):
        B, T, _ = x.shape
        nh, dh = self.n_head, self.d_head
        q, k, v = self.qkv_linears(x).split((nh * dh, nh * dh, dh), dim=-1)
        q, k = q.view(B, T, nh, dh).transpose(1, 2), k.view(B, T, nh, dh).transpose(1, 2)
        prob = F.softmax(torch.matmul(q, k.transpose(2, 3)) * self.scale + self._mask[:, :T, :T], dim=3)
        mean_prob = prob.mean(dim=1)                                  # V is shared: mean_h(P_h V) = (mean_h P_h) V
        return self.out_proj(torch.matmul(mean_prob, v)), mean_prob


class TFTBack(nn.Module):
    def __init__(self, config):
        super().__init__()
        H = config.hidden_size
        self.encoder_length = config.encoder_length
        self.history_vsn = VariableSelectionNetwork(config, config.num_historic_vars)
        self.history_encoder = nn.LSTM(H, H, batch_first=True)
        self.future_vsn = VariableSelectionNetwork(config, config.num_future_vars)
        self.future_encoder = nn.LSTM(H, H, batch_first=True)
        self.input_gate = GLU(H, H)
        self.input_gate_ln = nn.LayerNorm(H, eps=LN_EPS)
        self.enrichment_grn = GRN(H, H, context_hidden_size=H)
        self.attention = InterpretableMultiHeadAttention(config)
        self.attention_gate = GLU(H, H)
        self.attention_ln = nn.LayerNorm(H, eps=LN_EPS)
        self.positionwise_grn = GRN(H, H)
        self.decoder_gate = GLU(H, H)
        self.decoder_ln = nn.LayerNorm(H, eps=LN_EPS)
        self.quantile_proj = nn.Linear(H, len(config.quantiles))

    def forward(self, historical_inputs, cs, ch, cc, ce, future_inputs, explain=False):
        enc = self.encoder_length
        hist_feat, hist_w = self.history_vsn(historical_inputs, cs)
        history, state = self.history_encoder(hist_feat, (ch, cc))
        fut_feat, fut_w = self.future_vsn(future_inputs, cs)
        future, _ = self.future_encoder(fut_feat, state)
        skip = torch.cat([hist_feat, fut_feat], dim=1)
        temporal = self.input_gate_ln(self.input_gate(torch.cat([history, future], dim=1)) + skip)
        enriched = self.enrichment_grn(temporal, c=ce)
        x, prob = self.attention(enriched)
        x = self.attention_ln(self.attention_gate(x[:, enc:]) + enriched[:, enc:])
        x = self.positionwise_grn(x)
        x = self.decoder_ln(self.decoder_gate(x) + temporal[:, enc:])
        out = self.quantile_proj(x)
        return (out, hist_w, fut_w, prob[:, enc:]) if explain else out


class TemporalFusionTransformer(nn.Module):
    def __init__(self, config):
        super().__init__()
        config = getattr(config, "model", config)
        self.encoder_length = config.encoder_length
        self.embedding = TFTEmbedding(config)
        self.static_encoder = StaticCovariateEncoder(config)
        self.TFTpart2 = TFTBack(config)

    def forward(self, batch, explain=False):
        enc = self.encoder_length
        s_inp, known, observed, target = self.embedding(batch)
        cs, ce, ch, cc = self.static_encoder(s_inp)
        hist = [known[:, :enc], target[:, :enc]]
        if observed is not None:
            hist.insert(0, observed[:, :enc])
        return self.TFTpart2(torch.cat(hist, dim=-2), cs, ch.unsqueeze(0), cc.unsqueeze(0), ce, known[:, enc:], explain=explain)


class _ConfigUnpickler(pickle.Unpickler):
    """The reference pickles its `configuration.*Config` object (and `data_utils` feature records) into the checkpoint; they
    resolve to this module's classes."""
    _MAP = {("configuration", "ElectricityConfig"): ElectricityConfig, ("configuration", "TrafficConfig"): TrafficConfig,
            ("data_utils", "FeatureSpec"): FeatureSpec, ("data_utils", "InputTypes"): InputTypes, ("data_utils", "DataTypes"): DataTypes}

    def find_class(self, module, name):
        return self._MAP.get((module, name)) or super().find_class(module, name)


class _PickleModule:
    __name__ = "pickle"
    Unpickler = _ConfigUnpickler
    load = staticmethod(lambda f, **kw: _ConfigUnpickler(f, **kw).load())


def load_checkpoint(path):
    """A reference checkpoint {'config': ..., 'model': state_dict, ...} -> (config, TemporalFusionTransformer in eval mode)."""
    with open(path, "rb") as f:
        ckpt = torch.load(io.BytesIO(f.read()), map_location="cpu", pickle_module=_PickleModule, weights_only=False)
    config = ckpt["config"]
    model = TemporalFusionTransformer(config)
    model.load_state_dict(ckpt["model"])
    return config, model.eval()
