"""Float64 stand-in for the reference QuartzNet forward (tests/ only): SpeechRecognition/QuartzNet/quartznet/model.py:257-292,
325-364 with common/features.py:158-170 in front, restated for ONE utterance at a time (with masked convolutions the reference's
result for an utterance does not depend on its batch), and the seeded weights the whole-network tests run on.

forward64(state, cfg, feats, dtype=None, emulate=False)
    feats: a list of log-mel [n_feat, frames] tensors.  dtype: the 16-bit type whose rounding is applied to the WEIGHTS first (the
    weights as the recognizer holds them; the BatchNorm coefficients are the fp32 fold of utils.state.fold_bn); None: the weights
    as they are and the BatchNorm fold in float64 (the reference's module under .double()).  emulate: also round every value to `dtype` where the recognizer rounds -- the packed features, d, each unit's
    output, each residual branch's output.  -> (list of float64 log-probs [out_len, n_classes], max |activation|).
fill_state(cfg, seed, calibrated)
    Xavier-uniform convolution weights, gamma U(0.5, 1.5), beta N(0, 0.2), the decoder weight x 4.  calibrated: the BatchNorm
    running statistics are the actual per-channel statistics (mean, biased variance) of the BatchNorm's input in the float64 forward of
    a seeded randn(4, n_feat, 200) calibration input, layer by layer -- so activations keep unit scale through the depth and the
    argmax takes many classes.  Otherwise: running_mean N(0, 0.2), running_var U(0.5, 1.5).
"""
import collections
import copy
import itertools

import torch

from deeplearningexamples_amd.utils.state import fold_bn
from deeplearningexamples_amd.quartznet.model import BN_EPS, check_config, state_shapes

F64 = torch.float64
LABELS = [" "] + [chr(ord("a") + i) for i in range(26)] + ["'"]
FEATURES = dict(normalize="per_feature", sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", n_filt=64, n_fft=512,
                frame_splicing=1, dither=0.00001, pad_align=16)


def _block(filters, repeat, k, stride=1, dilation=1, residual=True, separable=True):
    return dict(filters=filters, repeat=repeat, kernel_size=[k], stride=[stride], dilation=[dilation], dropout=0.0, residual=residual,
                separable=separable)


def small_config():
    """64 mel features; Conv1 64 x K 11 stride 2; 3 x (64, K 13); 2 x (128, K 17); Conv2 128 x K 29 dilation 2; Conv3 256 x K 1."""
    blocks = [_block(64, 1, 11, stride=2, residual=False), _block(64, 3, 13), _block(128, 2, 17),
              _block(128, 1, 29, dilation=2, residual=False), _block(256, 1, 1, residual=False, separable=False)]
    return dict(name="QuartzNet", labels=list(LABELS),
                input_val=dict(audio_dataset=dict(sample_rate=16000, trim_silence=True, normalize_transcripts=True),
                               filterbank_features=dict(FEATURES)),
                quartznet=dict(encoder=dict(init="xavier_uniform", in_feats=64, frame_splicing=1, activation="relu", use_conv_masks=True,
                                            blocks=blocks),
                               decoder=dict(in_feats=256, init="xavier_uniform")))


def big_config():
    """configs/quartznet15x5_speedp-online-1.15_speca.yaml, the part inference reads."""
    cfg = small_config()
    b = _block
    blocks = [b(256, 1, 33, stride=2, residual=False)]
    for filt, k in ((256, 33), (256, 39), (512, 51), (512, 63), (512, 75)):
        blocks += [b(filt, 5, k) for _ in range(3)]
    blocks += [b(512, 1, 87, dilation=2, residual=False), b(1024, 1, 1, residual=False, separable=False)]
    cfg["quartznet"]["encoder"]["blocks"] = blocks
    cfg["quartznet"]["decoder"]["in_feats"] = 1024
    return cfg


def _rnd(t, dtype, on):
    return t.to(torch.float32).to(dtype).to(F64) if on else t


def _depthwise(h, w, stride, dilation):
    """h [T, C], w [C, K] float64 -> [(T - 1) // stride + 1, C]."""
    t, k = h.shape[0], w.shape[1]
    halo = (k // 2) * dilation
    ol = (t - 1) // stride + 1
    hp = torch.nn.functional.pad(h, (0, 0, halo, halo))
    d = torch.zeros((ol, h.shape[1]), dtype=F64)
    for j in range(k):
        d += w[:, j] * hp[j * dilation:j * dilation + stride * (ol - 1) + 1:stride]
    return d


def _walk(state, cfg, feats, dtype, emulate, calibrate):
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
        hs.append(_rnd(((x - m) / s).t().contiguous(), dtype, emulate))
    track(hs)
    for n, b in enumerate(blocks):
        pre = "encoder.layers.%d." % n
        res = None
        if b["residual"]:
            w = wq(state[pre + "res.0.0.weight"][:, :, 0])
            acc = [h @ w.t() for h in hs]
            sc, sh = bn(pre + "res.0.1.", acc)
            res = track([_rnd(sc * a + sh, dtype, emulate) for a in acc])
        m = 0
        for r in range(b["repeat"]):
            if b["separable"]:
                dw = wq(state["%smconv.%d.weight" % (pre, m)][:, 0, :])
                pw = wq(state["%smconv.%d.weight" % (pre, m + 1)][:, :, 0])
                bnp = "%smconv.%d." % (pre, m + 2)
                m += 5
                ds = track([_rnd(_depthwise(h, dw, b["stride"], b["dilation"]), dtype, emulate) for h in hs])
                acc = [d @ pw.t() for d in ds]
            else:
                pw = wq(state["%smconv.%d.weight" % (pre, m)][:, :, 0])
                bnp = "%smconv.%d." % (pre, m + 1)
                m += 4
                acc = [h @ pw.t() for h in hs]
            sc, sh = bn(bnp, acc)
            out = [sc * a + sh for a in acc]
            if res is not None and r == b["repeat"] - 1:
                out = [o + q for o, q in zip(out, res)]
            hs = track([_rnd(o.clamp_min(0), dtype, emulate) for o in out])
    w = wq(state["decoder.layers.0.weight"][:, :, 0])
    bias = state["decoder.layers.0.bias"].to(torch.float32).to(F64)
    return [torch.log_softmax(h @ w.t() + bias, dim=1) for h in hs], peak[0]


def forward64(state, cfg, feats, dtype=None, emulate=False):
    return _walk(state, cfg, feats, dtype, emulate, False)


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
        n_feat = cfg["quartznet"]["encoder"]["in_feats"]
        cal = torch.randn((4, n_feat, 200), generator=g, dtype=F64)
        _walk(state, cfg, list(cal), None, False, True)
    return state


def seeded_features(lens, seed, n_feat=64):
    """log-mel-like inputs: an offset larger than the spread, as the front end gives."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((n_feat, n), generator=g) * 2 - 6).to(torch.float32) for n in lens]


def ctc_collapse(ids, blank):
    """The greedy CTC reading of a row of frame ids: runs of equal ids count once, then the blanks go."""
    return [k for k, _ in itertools.groupby(ids) if k != blank]


def clone_state(state):
    return copy.deepcopy(state)
