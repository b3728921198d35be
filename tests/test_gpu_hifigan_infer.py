"""HifiGanVocoder (hifigan/infer.py): the whole generator against a float64 CPU forward; launch structure, graph replay, checkpoint
forms, the command line, zero-padding consistency.  GPU only.

Two configurations: the small one of tests/_hifigan_ref.py (channels 64 -> 32 -> 16 -> 8, hop 32) at mel [2, 80, 9] and V1
(512 -> 256 -> 128 -> 64 -> 32, hop 256) at mel [2, 80, 6]; fp16 and bf16; batch 2 and batch 1.

Weights (tests/_hifigan_ref.fill_state, seeded): weight_v ~ gain N(0, 1 / fan_in), weight_g = ||v||, bias ~ 0.1 N(0, 1); the gains
were chosen on the CPU so that the float64 forward alone gives max |activation| < 16384 and an audio RMS inside [0.05, 0.9] -- both
asserted here on the float64 side.  (The reference's init_weights, std 0.01, gives audio of magnitude 0.07 and would hide errors.)

Reference: tests/_hifigan_ref.forward64 over the 16-bit-rounded folded weights and spectrogram.  There is no parent path for this
network; the yardstick is the project's established one: the SAME float64 forward with each value rounded to the 16-bit type where
the vocoder rounds (the layout launch, every convolution's output after its epilogue, the leaky-ReLU operand).  With E the RMS
audio error against the unrounded float64 forward: E_new <= 1.5 E_emulated; the factor and its justification are those of
tests/test_gpu_resnext_infer.py and tests/test_gpu_rn50_infer.py (two legitimate paths that round at the same places but
accumulate differently are statistically equal).  RMS and max ratios are printed.

Zero-padding consistency.  An utterance of L frames inside a batch padded to more frames is followed by zeros in the spectrogram,
but by bias-driven activations from conv_pre on, where its batch-1 run has the zero padding of every layer.  A sample is therefore
the same in both runs -- bit for bit: the tiles and the order of every sum do not depend on T -- when its receptive field ends
before frame L at every layer.  receptive_radius() adds, from the output back, each layer's reach in output samples: 3 for
conv_post; per stage (s samples per step there) max over the blocks of the sum of its halos x s, plus one input step (u s) for
the transposed convolution, whose 3-tap form reads frames t - 1 .. t + 1; 3 hop for conv_pre.  The samples before L hop - radius
are compared, the others excluded by construction.
"""
import functools
import os
import wave

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.hifigan import inference as cli
from deeplearningexamples_amd.hifigan.infer import HifiGanVocoder
from deeplearningexamples_amd.hifigan.model import V1_CONFIG, check_config
from tests import _hifigan_ref as H
from tests._exact_grid import assert_same, bits

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DEV = "cuda"
CONFIGS = {"small": (H.SMALL_CONFIG, (2, 80, 9)), "v1": (V1_CONFIG, (2, 80, 6))}


@functools.lru_cache(maxsize=None)
def get_model(name):
    return H.build_model(CONFIGS[name][0])


@functools.lru_cache(maxsize=None)
def get_mel(name):
    return H.make_mel(CONFIGS[name][1])


@functools.lru_cache(maxsize=None)
def references(name, dtype):
    model, mel = get_model(name), get_mel(name)
    ref, peak = H.forward64(model, mel, dtype, emulate=False)
    emu, _ = H.forward64(model, mel, dtype, emulate=True)
    rms = float(ref.pow(2).mean().sqrt())
    assert peak < 16384, "max |activation| %.1f: fp16 would overflow" % peak
    assert 0.05 <= rms <= 0.9, "audio RMS %.3f: saturated or too quiet to show errors" % rms
    return ref, emu


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_audio_against_float64_and_the_emulated_roundings(name, dtype):
    ref, emu = references(name, dtype)
    voc = HifiGanVocoder(get_model(name), dtype=dtype)
    hop = int(np.prod(CONFIGS[name][0]["upsample_rates"]))
    for n in (2, 1):                                                     # the float64 rows are independent: row 0 serves batch 1
        got = voc.infer(get_mel(name)[:n].to(DEV))
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, CONFIGS[name][1][2] * hop)
        assert bool(torch.isfinite(got).all())
        d_new, d_emu = got.cpu().double() - ref[:n], emu[:n] - ref[:n]
        e_new, e_emu = _rms(d_new), _rms(d_emu)
        m_new, m_emu = float(d_new.abs().max()), float(d_emu.abs().max())
        print("%s %s batch %d: RMS audio error %.4e, emulated %.4e (ratio %.3f); max %.4e, emulated %.4e (ratio %.3f); audio RMS %.3f" % (
            name, dtype, n, e_new, e_emu, e_new / e_emu, m_new, m_emu, m_new / m_emu, _rms(ref[:n])))
        assert e_emu > 0
        assert e_new <= 1.5 * e_emu, "RMS audio error %.4e against %.4e of the emulated roundings" % (e_new, e_emu)


def test_fp32_is_rejected():
    with pytest.raises(ValueError, match="16 bits"):
        HifiGanVocoder(get_model("small"), dtype=torch.float32)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_structure(name, monkeypatch):
    """conv_pre + per stage (the upsample convolution + blocks x convolutions per block) dle_conv1d_lrelu_fwd launches, one
    dle_hfg_post_fwd, one layout launch, nothing else: V1 1 + 4 (1 + 3 x 6) = 77, the small configuration 1 + 3 (1 + 3 x 6) = 58."""
    cfg = check_config(CONFIGS[name][0])
    voc = HifiGanVocoder(get_model(name), dtype=HF)
    mel = get_mel(name).to(DEV)
    voc.infer(mel)                                                       # (first call outside the count: it allocates the buffers)
    names = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    voc.infer(mel)
    per_block = 6 if cfg["resblock"] == "1" else 2
    convs = 1 + len(cfg["upsample_rates"]) * (1 + len(cfg["resblock_kernel_sizes"]) * per_block)
    assert convs == {"v1": 77, "small": 58}[name]
    assert names.count("dle_conv1d_lrelu_fwd") == convs
    assert names.count("dle_hfg_post_fwd") == 1 and names.count("dle_nchw_to_nhwc") == 1
    assert len(names) == convs + 2, sorted(set(names))


def test_graph_replay_matches_eager():
    model = get_model("small")
    eager = HifiGanVocoder(model, dtype=HF)
    graphed = HifiGanVocoder(model, dtype=HF, graphs=True)
    for b, t in ((2, 9), (1, 5)):
        mel_a, mel_b = H.make_mel((b, 80, t), seed=71).to(DEV), H.make_mel((b, 80, t), seed=72).to(DEV)
        want_a, want_b = eager.infer(mel_a).clone(), eager.infer(mel_b).clone()
        assert not torch.equal(want_a, want_b)
        for _ in range(4):                                               # two eager warm-up calls, the capture + replay, a replay
            assert_same(bits(graphed.infer(mel_a).clone()), bits(want_a), "graph call, (B, T) = (%d, %d)" % (b, t))
        assert graphed._graphs[(b, t)].graph is not None
        # eager keeps the work buffers of the most recent shape only, a captured graph those of each of its shapes
        assert list(eager._buffers) == [(b, t)] and (b, t) in graphed._buffers
        assert_same(bits(graphed.infer(mel_b).clone()), bits(want_b), "replay with a new spectrogram, (B, T) = (%d, %d)" % (b, t))
    assert len(graphed._buffers) == 2


def _flat_keys(state):
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        if parts[0] == "resblocks":
            k = "resblocks.%d.%s" % (int(parts[1]) * 3 + int(parts[2]), ".".join(parts[3:]))
        out[k] = v
    return out


def test_from_checkpoint_forms(tmp_path):
    cfg = H.SMALL_CONFIG
    model, mel = get_model("small"), get_mel("small").to(DEV)
    state = model.state_dict()
    want = HifiGanVocoder(model, dtype=HF).infer(mel).clone()
    assert_same(bits(HifiGanVocoder(state, config=cfg, dtype=HF).infer(mel)), bits(want), "a state dict in memory")
    ema_state = H.fill_state(cfg, seed=H.SEED + 7)
    want_ema = HifiGanVocoder(ema_state, config=cfg, dtype=HF).infer(mel).clone()
    assert not torch.equal(want, want_ema)
    ckpt = {"generator": {"module." + k: v for k, v in state.items()}, "gen_ema": {"module." + k: v for k, v in ema_state.items()},
            "config": dict(cfg, mpd_periods=[2, 3, 5, 7, 11]), "train_setup": {"sampling_rate": 22050}}
    path = str(tmp_path / "hifigan_gen_checkpoint.pt")
    torch.save(ckpt, path)
    assert_same(bits(HifiGanVocoder.from_checkpoint(path, dtype=HF).infer(mel)), bits(want), "the reference's checkpoint file")
    assert_same(bits(HifiGanVocoder.from_checkpoint(path, ema=True, dtype=HF).infer(mel)), bits(want_ema), "gen_ema")
    assert_same(bits(HifiGanVocoder.from_checkpoint(ckpt, dtype=HF).infer(mel)), bits(want), "the checkpoint dict in memory")
    with pytest.raises(KeyError):
        HifiGanVocoder.from_checkpoint(dict(ckpt, gen_ema=None), ema=True, dtype=HF)
    folded = {}
    for l in model.layers:
        folded[l.name + ".weight"] = model.folded_weight(l.name)
        folded[l.name + ".bias"] = state[l.name + ".bias"]
    assert_same(bits(HifiGanVocoder(folded, config=cfg, dtype=HF).infer(mel)), bits(want), "folded weights (after remove_weight_norm)")
    assert_same(bits(HifiGanVocoder(_flat_keys(state), config=cfg, dtype=HF).infer(mel)), bits(want), "old flat resblock keys")
    assert_same(bits(HifiGanVocoder(model, dtype=HF).infer(mel.half())), bits(HifiGanVocoder(model, dtype=HF).infer(mel.half().float())),
                "a 16-bit spectrogram")


def _read_wav(path):
    with wave.open(path, "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float64), f.getframerate()


def test_inference_main_writes_trimmed_normalised_wavs(tmp_path):
    state = get_model("v1").state_dict()
    ckpt = str(tmp_path / "hifigan.pt")
    torch.save({"generator": state, "gen_ema": None, "config": V1_CONFIG, "train_setup": {}}, ckpt)
    os.makedirs(str(tmp_path / "data" / "mels"))
    lens = {"short": 5, "long": 8}
    for i, (nm, n) in enumerate(lens.items()):
        torch.save(H.make_mel((80, n), seed=90 + i), str(tmp_path / "data" / "mels" / (nm + ".pt")))
    tsv = str(tmp_path / "mels.tsv")
    open(tsv, "w").write("mel\toutput\nmels/short.pt\tshort.wav\nmels/long.pt\tlong.wav\n")
    for sub, extra in (("plain", []), ("denoised", ["-d", "0.01"])):
        out = str(tmp_path / sub)
        audios = cli.main(["-i", tsv, "--dataset-path", str(tmp_path / "data"), "--hifigan", ckpt, "-o", out, "--amp", "--cuda",
                           "-bs", "2", "--fade-out", "2"] + extra)
        assert [a.shape[0] for a in audios] == [lens["long"] * 256, lens["short"] * 256]     # longest first
        for nm, n in lens.items():
            pcm, rate = _read_wav(os.path.join(out, nm + ".wav"))
            assert rate == 22050 and pcm.shape[0] == n * 256
            assert np.isfinite(pcm).all() and np.abs(pcm).max() == 32767            # scaled to its peak
            assert pcm[-1] == 0                                                    # the fade-out ends at zero
        assert os.path.exists(os.path.join(out, "nvlog_infer.json"))
        log = open(os.path.join(out, "nvlog_infer.json")).read()
        assert "hifigan_samples/s" in log and "hifigan_latency" in log


def receptive_radius(cfg):
    """Output samples on either side of a sample that can reach it (see the module docstring)."""
    cfg = check_config(cfg)
    rates = cfg["upsample_rates"]
    radius, scale = 3, 1
    for u in reversed(rates):
        block = 0
        for k, dil in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            h = (k - 1) // 2
            reach = sum(h * d + h for d in dil[:3]) if cfg["resblock"] == "1" else sum(h * d for d in dil[:2])
            block = max(block, reach)
        radius += block * scale + u * scale
        scale *= u
    return radius + 3 * scale


def test_zero_padding_does_not_reach_the_samples_inside_the_receptive_field():
    cfg = H.SMALL_CONFIG
    hop, radius = 32, receptive_radius(cfg)
    assert radius == 3 + (60 + 2) + (120 + 4) + (240 + 32) + 96
    short, long_ = 24, 30
    keep = short * hop - radius
    assert keep >= 128
    voc = HifiGanVocoder(get_model("small"), dtype=HF)
    mel = H.make_mel((2, 80, long_), seed=81).to(DEV)
    mel[1, :, short:] = 0.0
    padded = voc.infer(mel).clone()
    alone = voc.infer(mel[1:, :, :short].contiguous()).clone()
    assert tuple(alone.shape) == (1, short * hop)
    assert_same(bits(padded[1, :keep]), bits(alone[0, :keep]), "the shorter utterance inside a padded batch")
    assert not torch.equal(padded[1, keep:short * hop], alone[0, keep:])   # (the excluded tail does differ: the margin is needed)
