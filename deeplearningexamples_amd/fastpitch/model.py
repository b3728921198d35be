"""FastPitch's parameters under the reference's names (SpeechSynthesis/FastPitch/fastpitch/model.py:112-212, transformer.py:39-193,
common/layers.py:76-88) and its configuration under the reference's keys (models.py:88-141).

A container, not a module: it holds the tensors of `FastPitch(**config).state_dict()` that inference reads --
  pitch_mean, pitch_std;  encoder.word_emb.weight;  encoder.layers.N.{dec_attn.{qkv_net.weight, qkv_net.bias, o_net.weight,
  layer_norm.*}, pos_ff.{CoreNet.0.*, CoreNet.2.*, layer_norm.*}};  speaker_emb.weight (n_speakers > 1);
  duration_predictor / pitch_predictor / energy_predictor .{layers.N.{conv.*, norm.*}, fc.*};  decoder.layers.N.*;
  pitch_emb.*, energy_emb.* (energy_conditioning);  proj.*
-- and loads what the reference's checkpoints hold: `module.` prefixes are stripped, `attention.*` (the aligner, training only)
and `*.inv_freq` (recomputed) are accepted and ignored.  The forward lives in fastpitch/infer.py.
"""
import collections

import torch

from ..utils.state import ParamTable, strip_module_prefix

# fastpitch/arg_parser.py:38-128 (and train.py's --n-speakers 1); n_symbols / padding_idx: the english_basic symbol set
DEFAULT_CONFIG = dict(
    n_mel_channels=80, n_symbols=148, padding_idx=0, symbols_embedding_dim=384,
    in_fft_n_layers=6, in_fft_n_heads=1, in_fft_d_head=64, in_fft_conv1d_kernel_size=3, in_fft_conv1d_filter_size=1536,
    in_fft_output_size=384, p_in_fft_dropout=0.1, p_in_fft_dropatt=0.1, p_in_fft_dropemb=0.0,
    out_fft_n_layers=6, out_fft_n_heads=1, out_fft_d_head=64, out_fft_conv1d_kernel_size=3, out_fft_conv1d_filter_size=1536,
    out_fft_output_size=384, p_out_fft_dropout=0.1, p_out_fft_dropatt=0.1, p_out_fft_dropemb=0.0,
    dur_predictor_kernel_size=3, dur_predictor_filter_size=256, p_dur_predictor_dropout=0.1, dur_predictor_n_layers=2,
    pitch_predictor_kernel_size=3, pitch_predictor_filter_size=256, p_pitch_predictor_dropout=0.1, pitch_predictor_n_layers=2,
    pitch_embedding_kernel_size=3,
    energy_conditioning=False, energy_predictor_kernel_size=3, energy_predictor_filter_size=256, p_energy_predictor_dropout=0.1,
    energy_predictor_n_layers=2, energy_embedding_kernel_size=3,
    n_speakers=1, speaker_emb_weight=1.0, pitch_conditioning_formants=1)
# keys a config may carry beyond those (pre_lnorm: FFTransformer's constructor argument, never set by the reference's recipes)
OPTIONAL_KEYS = ("pre_lnorm",)
LN_EPS = 1e-5                 # torch.nn.LayerNorm's default
MAX_ROWS = 1024               # rows of one utterance (text or spectrogram): the envelope of the packed attention kernel
LJSPEECH_PITCH = (218.14, 67.24)     # model.py:350-352: mean, std when the checkpoint carries none


def check_config(config):
    """The reference's keys over DEFAULT_CONFIG; an unknown key is an error."""
    cfg = dict(DEFAULT_CONFIG)
    for k, v in dict(config).items():
        if k not in cfg and k not in OPTIONAL_KEYS:
            raise ValueError("unknown FastPitch config key %r" % (k,))
        cfg[k] = v
    d = cfg["symbols_embedding_dim"]
    if cfg["in_fft_output_size"] != d or cfg["out_fft_output_size"] != d:
        raise ValueError("in_fft_output_size and out_fft_output_size must equal symbols_embedding_dim (%d)" % d)
    for k in ("in_fft_conv1d_kernel_size", "out_fft_conv1d_kernel_size", "dur_predictor_kernel_size", "pitch_predictor_kernel_size",
              "energy_predictor_kernel_size", "pitch_embedding_kernel_size", "energy_embedding_kernel_size"):
        if cfg[k] % 2 == 0:
            raise ValueError("%s must be odd (got %d): an even kernel changes the sequence length" % (k, cfg[k]))
    return cfg


def _fft_shapes(shapes, pre, n_layers, n_heads, d_head, d_model, d_inner, ksize):
    for n in range(n_layers):
        p = "%slayers.%d." % (pre, n)
        shapes[p + "dec_attn.qkv_net.weight"] = (3 * n_heads * d_head, d_model)
        shapes[p + "dec_attn.qkv_net.bias"] = (3 * n_heads * d_head,)
        shapes[p + "dec_attn.o_net.weight"] = (d_model, n_heads * d_head)
        shapes[p + "dec_attn.layer_norm.weight"] = (d_model,)
        shapes[p + "dec_attn.layer_norm.bias"] = (d_model,)
        shapes[p + "pos_ff.CoreNet.0.weight"] = (d_inner, d_model, ksize)
        shapes[p + "pos_ff.CoreNet.0.bias"] = (d_inner,)
        shapes[p + "pos_ff.CoreNet.2.weight"] = (d_model, d_inner, ksize)
        shapes[p + "pos_ff.CoreNet.2.bias"] = (d_model,)
        shapes[p + "pos_ff.layer_norm.weight"] = (d_model,)
        shapes[p + "pos_ff.layer_norm.bias"] = (d_model,)


def _predictor_shapes(shapes, pre, d_in, filt, ksize, n_layers, n_pred):
    for n in range(n_layers):
        p = "%slayers.%d." % (pre, n)
        shapes[p + "conv.weight"] = (filt, d_in if n == 0 else filt, ksize)
        shapes[p + "conv.bias"] = (filt,)
        shapes[p + "norm.weight"] = (filt,)
        shapes[p + "norm.bias"] = (filt,)
    shapes[pre + "fc.weight"] = (n_pred, filt)
    shapes[pre + "fc.bias"] = (n_pred,)


def state_shapes(config):
    """name -> shape of what inference reads of FastPitch(**config).state_dict(), in its order: the module's own buffers, then
    the children as FastPitch.__init__ registers them (`attention.*` and `*.inv_freq` left out)."""
    cfg = check_config(config)
    d = cfg["symbols_embedding_dim"]
    s = collections.OrderedDict()
    s["pitch_mean"] = (1,)
    s["pitch_std"] = (1,)
    s["encoder.word_emb.weight"] = (cfg["n_symbols"], d)
    _fft_shapes(s, "encoder.", cfg["in_fft_n_layers"], cfg["in_fft_n_heads"], cfg["in_fft_d_head"], d,
                cfg["in_fft_conv1d_filter_size"], cfg["in_fft_conv1d_kernel_size"])
    if cfg["n_speakers"] > 1:
        s["speaker_emb.weight"] = (cfg["n_speakers"], d)
    _predictor_shapes(s, "duration_predictor.", d, cfg["dur_predictor_filter_size"], cfg["dur_predictor_kernel_size"],
                      cfg["dur_predictor_n_layers"], 1)
    _fft_shapes(s, "decoder.", cfg["out_fft_n_layers"], cfg["out_fft_n_heads"], cfg["out_fft_d_head"], d,
                cfg["out_fft_conv1d_filter_size"], cfg["out_fft_conv1d_kernel_size"])
    _predictor_shapes(s, "pitch_predictor.", d, cfg["pitch_predictor_filter_size"], cfg["pitch_predictor_kernel_size"],
                      cfg["pitch_predictor_n_layers"], cfg["pitch_conditioning_formants"])
    s["pitch_emb.weight"] = (d, cfg["pitch_conditioning_formants"], cfg["pitch_embedding_kernel_size"])
    s["pitch_emb.bias"] = (d,)
    if cfg["energy_conditioning"]:
        _predictor_shapes(s, "energy_predictor.", d, cfg["energy_predictor_filter_size"], cfg["energy_predictor_kernel_size"],
                          cfg["energy_predictor_n_layers"], 1)
        s["energy_emb.weight"] = (d, 1, cfg["energy_embedding_kernel_size"])
        s["energy_emb.bias"] = (d,)
    s["proj.weight"] = (cfg["n_mel_channels"], d)
    s["proj.bias"] = (cfg["n_mel_channels"],)
    return s


def ignored_key(k):
    """Keys of the reference's state that inference does not read: the training-only aligner and the recomputed inv_freq buffers."""
    return k.startswith("attention.") or k.endswith(".inv_freq")


def normalize_keys(state):
    """`module.` prefixes stripped (models.py:226), the ignored keys dropped."""
    return collections.OrderedDict((k, v) for k, v in strip_module_prefix(state).items() if not ignored_key(k))


def positional_table(n_pos, d_model):
    """float64 [n_pos, d_model]: PositionalEmbedding (transformer.py:22-36) -- inv_freq is the module's fp32 buffer (computed in
    fp32 at construction, whatever the module is cast to afterwards), the products, sines and cosines are float64."""
    inv_freq = 1 / (10000 ** (torch.arange(0.0, d_model, 2.0) / d_model))
    sinusoid = torch.outer(torch.arange(n_pos, dtype=torch.float64), inv_freq.double())
    return torch.cat([sinusoid.sin(), sinusoid.cos()], dim=1)


class FastPitchModel(ParamTable):
    """The parameters as fp32 tensors on `device`, zero until loaded."""
    NAME = "FastPitch"
    normalize_keys = staticmethod(normalize_keys)

    def __init__(self, config, device="cpu"):
        self.cfg = check_config(config)
        super().__init__(state_shapes(self.cfg), device)
