"""float64 reference of FastPitch inference and the seeded weights of its tests (tests/ and tools/ only).

forward64: FastPitch.infer (fastpitch/model.py:327-385) for ONE utterance at a time on the CPU in float64, written for this project
from the module tree: word + positional (+ speaker) embedding; per FFT block  x1 = LN(x + o_net(softmax(q k^T / 8) v)),
x = LN(x1 + conv(relu(conv(x1))));  the temporal predictors (conv, ReLU, LN) x n, fc;  pitch_emb / energy_emb added to the encoder
output;  dur = clamp(exp(log_dur) - 1, 0, max_duration), reps = floor(dur / pace + 0.5);  every token repeated reps times + the
positional embedding;  the decoder blocks;  proj.  Run alone there are no masks: a convolution sees zeros beyond the utterance's
ends and nothing else.  dtype None: the fp32 state widened, nothing rounded -- what the reference module computes after .double()
at batch 1 (tests/test_fastpitch_host.py pins this to tests/golden/fastpitch_infer.npz).  dtype fp16 / bf16: the weights the
synthesizer holds in 16 bits (qkv_net, o_net, the convolutions, proj) are rounded to the type; emulate=True additionally rounds
wherever FastPitchSynthesizer writes a 16-bit tensor: the embedding sum, every GEMM / attention / convolution output (and the
attention probabilities, which the kernel hands to the matrix unit in 16 bits), the
residual sum inside dle_layernorm_fwd and its output, relu-LayerNorm's output (the fc reads the rounded value), the in-place
pitch / energy additions, the expanded rows, proj's output.

fill_state: every tensor from numpy's RandomState (stable across versions and machines).  Weights ~ gain N(0, 1 / fan_in), LayerNorm
gamma ~ 1 + 0.1 N, beta ~ 0.1 N, biases ~ 0.1 N, embeddings ~ N(0, 1); the duration predictor's fc comes from a stream of its own
(DUR_SEED by d_model, DUR_GAIN, DUR_BIAS), searched on the CPU so that for the texts of the tests (make_texts) the durations hold
zeros and values above 3, every dur / pace of the float64 forward lies at least 0.1 from a rounding boundary, and the forward
with rounded weights, with and without the emulated roundings, in both types, gives the same repetitions
(tests/test_fastpitch_host.py asserts all of it).
"""
import collections

import numpy as np
import torch

from deeplearningexamples_amd.fastpitch.model import LN_EPS, FastPitchModel, check_config, state_shapes

SMALL_CONFIG = dict(symbols_embedding_dim=128, in_fft_n_layers=2, in_fft_n_heads=2, in_fft_d_head=64, in_fft_conv1d_filter_size=256,
                    in_fft_output_size=128, out_fft_n_layers=2, out_fft_n_heads=2, out_fft_d_head=64, out_fft_conv1d_filter_size=256,
                    out_fft_output_size=128, dur_predictor_filter_size=64, pitch_predictor_filter_size=64,
                    energy_predictor_filter_size=64, energy_conditioning=True)
SEED = 20250
GAIN = 1.0
DUR_GAIN, DUR_BIAS = 0.9, 0.9
DUR_SEED = {128: 0, 384: 64, (128, 3): 165}      # by d_model (and n_speakers > 1); found by tools/make_fastpitch_fixture.py --search
TEXT_LENS = {"small": (9, 5, 1), "default": (9, 5)}
F64 = torch.float64


def dur_key(cfg):
    d = cfg["symbols_embedding_dim"]
    return d if cfg["n_speakers"] <= 1 else (d, cfg["n_speakers"])


def make_texts(lens, n_symbols=148, seed=SEED + 1):
    """Seeded ids in [1, n_symbols): no padding symbol inside a text."""
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randint(1, n_symbols, size=(n,))).long() for n in lens]


def fill_state(config, seed=SEED, gain=GAIN, dur_seed=None):
    """-> OrderedDict name -> fp32 tensor, the reference's names and shapes (what inference reads)."""
    cfg = check_config(config)
    rs = np.random.RandomState(seed)
    out = collections.OrderedDict()
    for k, shape in state_shapes(cfg).items():
        leaf = k.rsplit(".", 1)[-1]
        if k in ("pitch_mean", "pitch_std"):
            v = np.zeros(shape)
        elif k.endswith("word_emb.weight") or k == "speaker_emb.weight":
            v = rs.standard_normal(shape)
        elif ".layer_norm." in k or ".norm." in k:
            v = (1.0 if leaf == "weight" else 0.0) + 0.1 * rs.standard_normal(shape)
        elif leaf == "bias":
            v = 0.1 * rs.standard_normal(shape)
        else:
            fan = int(np.prod(shape[1:]))
            v = rs.standard_normal(shape) * gain * fan ** -0.5
        out[k] = torch.from_numpy(np.asarray(v)).float()
    ds = DUR_SEED[dur_key(cfg)] if dur_seed is None else dur_seed
    rd = np.random.RandomState(100000 + ds)
    w = out["duration_predictor.fc.weight"]
    out["duration_predictor.fc.weight"] = torch.from_numpy(rd.standard_normal(tuple(w.shape)) * DUR_GAIN * w.shape[1] ** -0.5).float()
    out["duration_predictor.fc.bias"] = torch.full((1,), DUR_BIAS)
    return out


def make_model(config, **kw):
    return FastPitchModel(config).load_state_dict(fill_state(config, **kw))


def positional64(n_pos, d_model):
    """transformer.py:22-36: inv_freq is an fp32 buffer, the rest float64."""
    inv_freq = (1 / (10000 ** (torch.arange(0.0, d_model, 2.0) / d_model))).double()
    s = torch.arange(n_pos, dtype=F64)[:, None] * inv_freq[None, :]
    return torch.cat([s.sin(), s.cos()], 1)


class _Net:
    """The weights as float64 (16-bit-held ones rounded to `dtype` first) and the rounding function of the emulation."""

    def __init__(self, model, dtype, emulate):
        self.cfg = model.cfg
        self.p = model.params
        self.dtype = dtype
        self.r = (lambda t: t.to(torch.float32).to(dtype).double()) if (emulate and dtype is not None) else (lambda t: t)
        self.r32 = (lambda t: t.to(torch.float32).double()) if (emulate and dtype is not None) else (lambda t: t)
        self.peak = 0.0

    def w16(self, k):
        w = self.p[k].detach().float()
        return (w if self.dtype is None else w.to(self.dtype)).double()

    def f(self, k):
        return self.p[k].detach().double()

    def see(self, t):
        if t.numel():
            self.peak = max(self.peak, float(t.abs().max()))
        return t


def _ln(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * g + b


def _conv(x, w, b):
    """x [L, C], w [Ko, C, k] -> [L, Ko]: 'same', zeros beyond the utterance."""
    ks = w.shape[2]
    return torch.nn.functional.conv1d(x.t()[None], w, b, padding=ks // 2)[0].t()


def _fft(net, x, pre, n_layers, heads):
    r, see = net.r, net.see
    for n in range(n_layers):
        p = "%slayers.%d." % (pre, n)
        qkv = see(r(x @ net.w16(p + "dec_attn.qkv_net.weight").t() + net.f(p + "dec_attn.qkv_net.bias")))
        h = heads * 64
        ctx = []
        for i in range(heads):
            q, k, v = (qkv[:, j * h + i * 64:j * h + (i + 1) * 64] for j in range(3))
            ctx.append(r(torch.softmax(q @ k.t() * 64 ** -0.5, dim=1)) @ v)
        ctx = r(torch.cat(ctx, 1))
        ao = see(r(ctx @ net.w16(p + "dec_attn.o_net.weight").t()))
        x1 = r(_ln(r(ao + x), net.f(p + "dec_attn.layer_norm.weight"), net.f(p + "dec_attn.layer_norm.bias")))
        t = see(r(_conv(x1, net.w16(p + "pos_ff.CoreNet.0.weight"), net.f(p + "pos_ff.CoreNet.0.bias"))))
        o2 = see(r(_conv(torch.relu(t), net.w16(p + "pos_ff.CoreNet.2.weight"), net.f(p + "pos_ff.CoreNet.2.bias"))))
        x = see(r(_ln(r(o2 + x1), net.f(p + "pos_ff.layer_norm.weight"), net.f(p + "pos_ff.layer_norm.bias"))))
    return x


def _predict(net, x, pre, n_layers):
    for n in range(n_layers):
        p = "%slayers.%d." % (pre, n)
        t = net.see(net.r(_conv(x, net.w16(p + "conv.weight"), net.f(p + "conv.bias"))))
        x = net.r(_ln(torch.relu(t), net.f(p + "norm.weight"), net.f(p + "norm.bias")))
    return net.r32(x @ net.f(pre + "fc.weight").t() + net.f(pre + "fc.bias"))[:, 0]


def _scalar_conv(v, w, b):
    """Conv1d(1 -> D, k) of a series v [L] -> [L, D]."""
    return torch.nn.functional.conv1d(v[None, None], w, b, padding=w.shape[2] // 2)[0].t()


def forward64(model, texts, dtype=None, emulate=False, pace=1.0, dur_tgt=None, pitch_tgt=None, energy_tgt=None,
              pitch_transform=None, max_duration=75, speaker=0, stop_after_durations=False):
    """-> (list over the utterances of dict(mel [n_mel, T], dur_pred [L], pitch_pred [L], energy_pred [L] or None, reps [L] int64,
    dur_used [L]), peak |activation|).  The overrides are per utterance: lists of 1-D float tensors (or None)."""
    cfg = model.cfg
    net = _Net(model, dtype, emulate)
    d = cfg["symbols_embedding_dim"]
    out = []
    for u, ids in enumerate(texts):
        ids = torch.as_tensor(ids).long()
        n = ids.numel()
        x = net.f("encoder.word_emb.weight")[ids] + net.r32(positional64(n, d))
        if cfg["n_speakers"] > 1:
            x = x + net.r32(net.f("speaker_emb.weight")[speaker] * cfg["speaker_emb_weight"])
        enc = _fft(net, net.r(x), "encoder.", cfg["in_fft_n_layers"], cfg["in_fft_n_heads"])
        log_dur = _predict(net, enc, "duration_predictor.", cfg["dur_predictor_n_layers"])
        dur_pred = torch.clamp(torch.exp(log_dur) - 1, 0, max_duration)
        dur = dur_pred if dur_tgt is None else torch.as_tensor(dur_tgt[u]).double()
        reps = torch.floor(dur / pace + 0.5).long()
        if stop_after_durations:
            out.append(dict(dur_pred=dur_pred, reps=reps, dur_used=dur))
            continue
        pitch_pred = _predict(net, enc, "pitch_predictor.", cfg["pitch_predictor_n_layers"])
        if pitch_transform is not None:
            std0 = float(model.params["pitch_std"][0])
            mean, std = (218.14, 67.24) if std0 == 0.0 else (float(model.params["pitch_mean"][0]), std0)
            pitch_pred = pitch_transform(pitch_pred[None, None], torch.tensor([n]), mean, std)[0, 0]
        pitch = pitch_pred if pitch_tgt is None else torch.as_tensor(pitch_tgt[u]).double()
        enc = net.r(enc + _scalar_conv(pitch, net.f("pitch_emb.weight"), net.f("pitch_emb.bias")))
        energy_pred = None
        if cfg["energy_conditioning"]:
            if energy_tgt is None:
                energy = energy_pred = _predict(net, enc, "energy_predictor.", cfg["energy_predictor_n_layers"])
            else:
                energy = torch.as_tensor(energy_tgt[u]).double()
            enc = net.r(enc + _scalar_conv(energy, net.f("energy_emb.weight"), net.f("energy_emb.bias")))
        net.see(enc)
        t = int(reps.sum())
        y = torch.repeat_interleave(enc, reps, dim=0) + net.r32(positional64(t, d))
        y = _fft(net, net.r(y), "decoder.", cfg["out_fft_n_layers"], cfg["out_fft_n_heads"])
        mel = net.r(y @ net.w16("proj.weight").t() + net.f("proj.bias")).t()
        out.append(dict(mel=mel, dur_pred=dur_pred, pitch_pred=pitch_pred, energy_pred=energy_pred, reps=reps, dur_used=dur))
    return out, net.peak


def duration_margin(dur, pace):
    """Smallest distance of dur / pace to a rounding boundary (k + 0.5)."""
    q = torch.as_tensor(dur).double() / pace
    return float(((q - torch.floor(q)) - 0.5).abs().min())
