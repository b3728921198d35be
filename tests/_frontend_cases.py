"""The cases of tests/test_gpu_frontend_bits.py and tools/make_frontend_bits.py: one call of every inference front end on the small
seeded model its own tests build, reduced to a SHA-256 of the output bytes.  The digests recorded in
tests/golden/frontend_bits.json pin what the front ends send to the library: the Python plumbing between a checkpoint and the C ABI
may be rearranged, the bits that come back may not change.

Only the front-end classes and their public methods are used, so the same file runs against any revision of the package.

Shapes: the smallest that reach the shared code's branches -- recognizers on a ragged batch of 37 and 64 frames (behind the
stride-2 first block: 19 and 32 rows), Jasper with pad_leading=16; classifiers and SSD on batch 2 with fp32 and with uint8
images at the resolution of their own tests; every class with a `graphs` option eager and captured, where the third call is the
first replay and must give the eager call's digest.
"""
import copy
import functools
import hashlib

import torch

HF, BF = torch.float16, torch.bfloat16
DEV = "cuda"
LENS = (37, 64)


def digest(outputs):
    """SHA-256 over dtype, shape and bytes of every tensor (strings: their UTF-8 bytes), in order."""
    h = hashlib.sha256()
    for t in outputs:
        if isinstance(t, str):
            h.update(t.encode() + b"\0")
            continue
        t = t.detach().cpu().contiguous()
        h.update(("%s%s" % (t.dtype, tuple(t.shape))).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _calls(fn, graphs):
    """One eager call, or three with graphs: two warm-up calls, then the capture and its first replay."""
    for _ in range(2 if graphs else 0):
        fn()
    return fn()


def _flat(out):
    return [t for t in out if t is not None]


# ------------------------------------------------------------------ the recognizers
@functools.lru_cache(maxsize=None)
def _asr(which):
    from tests import _jasper_ref, _quartznet_ref
    R = _quartznet_ref if which == "quartznet" else _jasper_ref
    cfg = R.small_config()
    return cfg, R.fill_state(cfg, 1, True), _quartznet_ref.seeded_features(LENS, 7)


def quartznet(dtype, graphs=False):
    from deeplearningexamples_amd.quartznet.infer import QuartzNetRecognizer
    cfg, state, feats = _asr("quartznet")
    texts, frames, logp = QuartzNetRecognizer(state, cfg, dtype).decode(feats, list(LENS), want_logp=True)
    return texts + frames + logp


def jasper(dtype, graphs=False):
    from deeplearningexamples_amd.jasper.infer import JasperRecognizer
    cfg, state, feats = _asr("jasper")
    texts, frames, logp = JasperRecognizer(state, cfg, dtype, pad_leading=16).decode(feats, list(LENS), want_logp=True)
    return texts + frames + logp


# ------------------------------------------------------------------ the image networks
@functools.lru_cache(maxsize=None)
def _images(size, u8):
    if u8:
        return torch.randint(0, 256, (2, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    return torch.randn((2, 3, size, size), generator=torch.Generator().manual_seed(7)).to(DEV)


@functools.lru_cache(maxsize=None)
def _cnn(net):
    """The module on the CPU (built there: the initialisation then does not depend on the device's generator)."""
    if net == "resnet50":
        from deeplearningexamples_amd.convnets.resnet import ResNet50
        from tests.test_gpu_rn50_infer import _randomise_bn
        torch.manual_seed(1234)
        m = ResNet50(num_classes=100, device="cpu")
        _randomise_bn(m, 99)
        return m
    if net == "resnext101-32x4d":
        from deeplearningexamples_amd.convnets import resnext
        from tests.test_gpu_resnext_infer import _randomise
        torch.manual_seed(4321)
        m = resnext.build(net, num_classes=100, device="cpu")
        _randomise(m, 77)
        return m
    from tests.test_gpu_efficientnet_infer import get_model
    return get_model(net)[0]


def classifier(net, dtype, u8, graphs):
    from deeplearningexamples_amd.convnets import infer
    cls = {"resnet50": infer.ResNet50Classifier, "resnext101-32x4d": infer.ResNeXtClassifier,
           "efficientnet-b0": infer.EfficientNetClassifier}[net]
    clf = cls(copy.deepcopy(_cnn(net)).to(DEV), dtype=dtype, graphs=graphs)
    return [_calls(lambda: clf.logits(_images(64, u8)), graphs)]


def ssd(dtype, u8, graphs):
    from deeplearningexamples_amd.ssd.infer import SSDDetector
    from tests.test_gpu_ssd_infer import get_images, get_model
    det = SSDDetector(copy.deepcopy(get_model(dtype)).to(DEV), dtype=dtype, graphs=graphs)
    images = _images(300, True) if u8 else get_images().to(DEV)
    raw = [t.clone() for t in _calls(lambda: det.raw(images), graphs)]
    return raw + list(_calls(lambda: det.detect(images), graphs))


# ------------------------------------------------------------------ speech synthesis, forecasting, language modelling
def hifigan(dtype, graphs):
    from deeplearningexamples_amd.hifigan.infer import HifiGanVocoder
    from tests import _hifigan_ref as H
    voc = HifiGanVocoder(H.build_model(H.SMALL_CONFIG), dtype=dtype, graphs=graphs)
    mel = H.make_mel((2, 80, 9)).to(DEV)
    return [_calls(lambda: voc.infer(mel), graphs)]


def fastpitch(dtype, graphs=False):
    from deeplearningexamples_amd.fastpitch.infer import FastPitchSynthesizer
    from tests import _fastpitch_ref as FP
    synth = FastPitchSynthesizer(FP.make_model(FP.SMALL_CONFIG), dtype=dtype)
    return _flat(synth.infer(FP.make_texts(FP.TEXT_LENS["small"])))


def tft(dtype, graphs):
    from deeplearningexamples_amd.tft import model as TM
    from deeplearningexamples_amd.tft.infer import TFTForecaster
    from tests import _tft_ref as R
    cfg = R.small_config("elec", 12, 8)
    m = TM.TemporalFusionTransformer(cfg)
    m.load_state_dict(R.seeded_state(cfg, 11))
    fc = TFTForecaster(m.eval(), dtype=dtype, graphs=graphs)
    batch = {k: (None if v is None else v.to(DEV)) for k, v in R.seeded_batch(cfg, 2, 12).items()}
    return list(_calls(lambda: fc.forecast(batch, explain=True), graphs))


def txl(dtype, graphs=False):
    from deeplearningexamples_amd.transformer_xl import model as M
    from deeplearningexamples_amd.transformer_xl.infer import TransformerXLEvaluator
    from tests import _txl_ref as R
    cfg = R.small_config()
    segments = [8, 8, 3]
    ev = TransformerXLEvaluator(M.TransformerXLModel(cfg).load_state_dict(R.fill_state(cfg, 3)), R.BATCH, dtype=dtype)
    batches = R.stream_batches(R.make_tokens(cfg, 5, R.BATCH * (sum(segments) + 1)), R.BATCH, segments)
    return [ev.segment(d.contiguous(), t.contiguous()) for d, t in batches]


def _image_cases(name, fn, dtype):
    return {"%s-%s-%s" % (name, "bf16" if dtype == BF else "fp16", "u8" if u8 else "f32"): (functools.partial(fn, dtype, u8), True)
            for u8 in (False, True)}


# id -> (fn(graphs) -> the outputs, whether the class has a `graphs` option)
CASES = {
    "quartznet-fp16": (functools.partial(quartznet, HF), False),
    "quartznet-bf16": (functools.partial(quartznet, BF), False),
    "jasper-fp16": (functools.partial(jasper, HF), False),
    "hifigan-fp16": (functools.partial(hifigan, HF), True),
    "fastpitch-fp16": (functools.partial(fastpitch, HF), False),
    "tft-fp16": (functools.partial(tft, HF), True),
    "txl-fp16": (functools.partial(txl, HF), False),
}
for _net in ("resnet50", "resnext101-32x4d", "efficientnet-b0"):
    CASES.update(_image_cases(_net, functools.partial(classifier, _net), HF))
CASES.update(_image_cases("resnet50", functools.partial(classifier, "resnet50"), BF))
CASES.update(_image_cases("ssd300", ssd, HF))

# (case id, graphs) of every run; a captured run is compared with the digest of its eager case
RUNS = [(k, g) for k, (_, has_graphs) in CASES.items() for g in ((False, True) if has_graphs else (False,))]
