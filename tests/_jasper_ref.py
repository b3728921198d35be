"""Float64 stand-in for the reference Jasper forward (tests/ only): SpeechRecognition/Jasper/jasper/model.py:137-171, 204-222 with
common/features.py's per-feature normalisation and inference.py:329-333's leading pad in front, restated for ONE utterance at a
time (with masked convolutions the reference's result for an utterance does not depend on its batch), and the seeded weights the
whole-network tests run on.

forward64(state, cfg, feats, dtype=None, emulate=False, lead=16)
    feats: a list of log-mel [n_feat, frames] tensors.  dtype: the 16-bit type whose rounding is applied to the WEIGHTS first (the
    weights as the recognizer holds them; the BatchNorm coefficients are the fp32 fold of utils.state.fold_bn); None: the weights
    as they are and the BatchNorm fold in float64 (the reference's module under .double()).  emulate: also round every value to
    `dtype` where the recognizer rounds -- the packed features, every sub-block's output, every link of the residual chain.
    lead: zero frames in front of the normalised features.  -> (list of float64 log-probs [out_len, n_classes], max |activation|).
forward64_both(state, cfg, feats, dtype, lead=16)
    both of them in one walk -> (exact, emulated, max |activation|).
fill_state(cfg, seed, calibrated)
    as tests/_quartznet_ref.fill_state: Xavier-uniform convolution weights, gamma U(0.5, 1.5), beta N(0, 0.2), the decoder weight
    x 4; calibrated: the BatchNorm running statistics are those of the BatchNorm's input in the float64 forward of a seeded
    randn(4, n_feat, 200) calibration input, layer by layer.  The residual sum of a block with p panes adds p + 1 unit-variance
    terms; the calibration keeps each term at unit scale, so activations grow by sqrt(p + 1) inside a block at most and are
    normalised again by the next BatchNorm.
"""
import collections

import torch

from deeplearningexamples_amd.utils.state import fold_bn
from deeplearningexamples_amd.jasper.model import BN_EPS, check_config, state_shapes
from tests._quartznet_ref import FEATURES, LABELS, clone_state, ctc_collapse, seeded_features      # noqa: F401

F64 = torch.float64


def _block(filters, repeat, k, stride=1, dilation=1, residual=True, dense=True, dropout=0.2):
    b = dict(filters=filters, repeat=repeat, kernel_size=[k], stride=[stride], dilation=[dilation], dropout=dropout, residual=residual)
    if residual and dense:
        b["residual_dense"] = True
    return b


def _config(blocks, enc_feats):
    return dict(name="Jasper", labels=list(LABELS),
                input_val=dict(audio_dataset=dict(sample_rate=16000, trim_silence=True, normalize_transcripts=True),
                               filterbank_features=dict(FEATURES)),
                jasper=dict(encoder=dict(init="xavier_uniform", in_feats=64, frame_splicing=1, activation="relu", use_conv_masks=True,
                                         blocks=blocks),
                            decoder=dict(in_feats=enc_feats, init="xavier_uniform")))


def small_config():
    """64 mel features; Conv1 64 x k 11 stride 2; dense blocks 64 k 11 x 2, 64 k 13 x 2, 128 k 17 x 2 (1, 2 and 3 panes, the last
    list of widths 64, 64, 64 in front of a 128-wide output); Conv2 128 x k 29 dilation 2; Conv3 256 x k 1."""
    blocks = [_block(64, 1, 11, stride=2, residual=False), _block(64, 2, 11), _block(64, 2, 13), _block(128, 2, 17),
              _block(128, 1, 29, dilation=2, residual=False), _block(256, 1, 1, residual=False)]
    return _config(blocks, 256)


def big_config():
    """configs/jasper10x5dr_speedp-online_speca.yaml, the part inference reads."""
    b = _block
    blocks = [b(256, 1, 11, stride=2, residual=False)]
    for filt, k, drop in ((256, 11, 0.2), (384, 13, 0.2), (512, 17, 0.2), (640, 21, 0.3), (768, 25, 0.3)):
        blocks += [b(filt, 5, k, dropout=drop) for _ in range(2)]
    blocks += [b(896, 1, 29, dilation=2, residual=False, dropout=0.4), b(1024, 1, 1, residual=False, dropout=0.4)]
    return _config(blocks, 1024)


def _rnd(t, dtype, on):
    return t.to(torch.float32).to(dtype).to(F64) if on else t


def _conv(h, w, stride, dilation):
    """h [T, C], w [Ko, C, K] float64 -> [(T - 1) // stride + 1, Ko]: one strided slice of the zero-padded rows per tap, the
    slices side by side as one [rows, C K] matrix (one large float64 product instead of K small ones)."""
    t, k = h.shape[0], w.shape[2]
    halo = (k // 2) * dilation
    ol = (t - 1) // stride + 1
    hp = torch.nn.functional.pad(h, (0, 0, halo, halo))
    cols = torch.stack([hp[j * dilation:j * dilation + stride * (ol - 1) + 1:stride] for j in range(k)], dim=2)
    return cols.reshape(ol, -1) @ w.reshape(w.shape[0], -1).t()              # both [.., C K]: the weight is not copied


def _walk(state, cfg, feats, dtype, emulate, calibrate, lead):
    _, _, blocks = check_config(cfg)
    wq = (lambda w: w.to(torch.float32).to(dtype).to(F64)) if dtype is not None else (lambda w: w.to(F64))
    peak = [0.0]

    def bn(pre, xs):
        """xs: the list of pre-BatchNorm activations [rows, C] -> scale, shift (float64 of the fp32 fold)."""
        if calibrate:
            allr = torch.cat(xs)
            state[pre + "running_mean"] = allr.mean(0).to(torch.float32)
            state[pre + "running_var"] = allr.var(0, unbiased=False).to(torch.float32)
        if dtype is None:                                                       # the reference's module in float64
            s = state[pre + "weight"].to(F64) / torch.sqrt(state[pre + "running_var"].to(F64) + BN_EPS)
            return s, state[pre + "bias"].to(F64) - state[pre + "running_mean"].to(F64) * s
        s, h = fold_bn(state[pre + "weight"], state[pre + "bias"], state[pre + "running_mean"], state[pre + "running_var"], BN_EPS)
        return s.to(F64), h.to(F64)

    def track(xs):
        peak[0] = max([peak[0]] + [float(x.abs().max()) for x in xs if x.numel()])
        return xs

    hs = []
    for f in feats:
        x = f.to(F64)
        m = x.mean(1, keepdim=True)
        s = x.std(1, unbiased=True, keepdim=True) + 1e-5
        x = _rnd(((x - m) / s).t().contiguous(), dtype, emulate[len(hs)])
        hs.append(torch.cat([torch.zeros((lead, x.shape[1]), dtype=F64), x]))
    track(hs)
    lists = [[h] for h in hs]                                                   # per utterance: the encoder's list
    for n, b in enumerate(blocks):
        pre = "encoder.layers.%d." % n
        res = None
        for j in range(len(b["panes"])):
            w = wq(state["%sres.%d.0.weight" % (pre, j)][:, :, 0])
            acc = [xs[j] @ w.t() for xs in lists]
            sc, sh = bn("%sres.%d.1." % (pre, j), acc)
            link = [sc * a + sh for a in acc]
            if res is not None:
                link = [l + q for l, q in zip(link, res)]
            res = track([_rnd(l, dtype, e) for l, e in zip(link, emulate)])
        hs = [xs[-1] for xs in lists]
        for r in range(b["repeat"]):
            w = wq(state["%sconv.%d.weight" % (pre, 4 * r)])
            acc = [_conv(h, w, b["stride"], b["dilation"]) for h in hs]
            sc, sh = bn("%sconv.%d." % (pre, 4 * r + 1), acc)
            out = [sc * a + sh for a in acc]
            if res is not None and r == b["repeat"] - 1:
                out = [o + q for o, q in zip(out, res)]
            hs = track([_rnd(o.clamp_min(0), dtype, e) for o, e in zip(out, emulate)])
        lists = [xs + [h] for xs, h in zip(lists, hs)] if b["dense"] else [[h] for h in hs]
    w = wq(state["decoder.layers.0.weight"][:, :, 0])
    bias = state["decoder.layers.0.bias"].to(torch.float32).to(F64)
    return [torch.log_softmax(xs[-1] @ w.t() + bias, dim=1) for xs in lists], peak[0]


def forward64(state, cfg, feats, dtype=None, emulate=False, lead=16):
    return _walk(state, cfg, feats, dtype, [emulate] * len(feats), False, lead)


def forward64_both(state, cfg, feats, dtype, lead=16):
    """forward64 without and with the emulated roundings in ONE walk (every weight is converted once; at 10x5dr the conversions
    of 333 M parameters are most of the time) -> (exact, emulated, max |activation| of both)."""
    n = len(feats)
    out, peak = _walk(state, cfg, list(feats) + list(feats), dtype, [False] * n + [True] * n, False, lead)
    return out[:n], out[n:], peak


def fill_state(cfg, seed, calibrated=True):
    g = torch.Generator().manual_seed(seed)
    state = collections.OrderedDict()
    for k, shape in state_shapes(cfg).items():
        if k.endswith("num_batches_tracked"):
            state[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_mean"):
            state[k] = torch.randn(shape, generator=g) * 0.2
        elif k.endswith("running_var"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        elif len(shape) == 3:                                                   # a convolution: Xavier uniform over [out, in, k]
            fan_out, fan_in = shape[0] * shape[2], shape[1] * shape[2]
            bound = (6.0 / (fan_in + fan_out)) ** 0.5
            state[k] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif k == "decoder.layers.0.bias":
            state[k] = torch.randn(shape, generator=g) * 0.1
        elif k.endswith(".weight"):                                             # gamma
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:                                                                   # beta
            state[k] = torch.randn(shape, generator=g) * 0.2
    state["decoder.layers.0.weight"] = state["decoder.layers.0.weight"] * 4
    if calibrated:
        n_feat = cfg["jasper"]["encoder"]["in_feats"]
        cal = torch.randn((4, n_feat, 200), generator=g, dtype=F64)
        _walk(state, cfg, list(cal), None, [False] * 4, True, 16)
    return state
