"""FastPitchSynthesizer (fastpitch/infer.py): the whole network against a float64 CPU forward; the batch-1 contract, the overrides, the
one host synchronisation, the errors, the command line.  GPU only.

Two configurations: the small one of tests/_fastpitch_ref.py (d_model 128, 2 heads x 64, d_inner 256, 2 + 2 layers, predictor filters
64, energy conditioning) with the fixture texts of 9, 5 and 1 symbols, and the reference's default (6 + 6 layers, 384 / 1536, one
head) with texts of 9 and 5 symbols; fp16 and bf16.

Weights: tests/_fastpitch_ref.fill_state (seeded; gains chosen on the CPU so that the float64 forward keeps max |activation| < 16384
and the mel RMS inside [0.2, 5] -- both asserted here on the float64 side -- and so that the durations satisfy the conditions
tests/test_fastpitch_host.py asserts: zeros, values above 3, every dur / pace at least 0.1 from a rounding boundary, the same
repetitions under the emulated roundings).

Reference: tests/_fastpitch_ref.forward64 over the weights as the synthesizer holds them, each utterance ALONE (host test: equal to
the reference's own batch-1 outputs).  The yardstick is the project's established one: the SAME float64 forward with each value
rounded to the 16-bit type where the synthesizer rounds.  With E the RMS error against the unrounded float64 forward, over all
utterances of the batch: E_new <= 1.5 E_emulated for mel, dur_pred, pitch_pred and energy_pred; the factor and its justification are
those of tests/test_gpu_hifigan_infer.py.  The ratios are printed.  Integer results must be EQUAL: mel_lens and the repetitions
(no case is skipped: a flipped repetition fails the test).  Padding frames of mel hold proj.bias bit for bit; per-token outputs
are zero behind each text.  The batch-1 runs of the same utterances meet the same checks, the errors taken over the runs together
as they are over the batch (the contract: what else shares the batch does not matter; not bit for bit, because dle_gemm may route
different M to different kernels).
"""
import functools
import json
import os
import wave

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.fastpitch import inference as cli
from deeplearningexamples_amd.fastpitch.infer import FastPitchSynthesizer
from deeplearningexamples_amd.fastpitch.model import DEFAULT_CONFIG
from tests import _fastpitch_ref as FP
from tests import _hifigan_ref as H
from tests._exact_grid import assert_same, bits

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
DEV = "cuda"
CONFIGS = {"small": FP.SMALL_CONFIG, "default": DEFAULT_CONFIG, "small3": dict(FP.SMALL_CONFIG, n_speakers=3)}
TEXTS = {"small": "small", "default": "default", "small3": "small"}
KEYS = ("mel", "dur_pred", "pitch_pred", "energy_pred")


@functools.lru_cache(maxsize=None)
def get_model(name):
    return FP.make_model(CONFIGS[name])


@functools.lru_cache(maxsize=None)
def get_texts(name):
    return tuple(FP.make_texts(FP.TEXT_LENS[TEXTS[name]]))


def dur_targets(lens):
    """0, 1, 3, 4 or 5 by position (the pattern of the committed fixture; never 2: 2 / 0.8 is a rounding boundary)."""
    val = lambda i, n: 5.0 if (3 * i + n) % 5 == 2 else float((3 * i + n) % 5)
    return [torch.tensor([val(i, n) if 0 < i < n - 1 else 0.0 for i in range(n)]) if n > 1 else torch.tensor([3.0]) for n in lens]


def padded(rows, width, lead=()):
    out = torch.zeros((len(rows),) + tuple(lead) + (width,))
    for i, r in enumerate(rows):
        out[i][..., :r.numel()] = r.float()
    return out


_REF_CACHE = {}


def references(name, dtype, **kw):
    key = (name, dtype, json.dumps({k: repr(v) for k, v in kw.items()}, sort_keys=True))
    if key not in _REF_CACHE:
        model, texts = get_model(name), get_texts(name)
        ref, peak = FP.forward64(model, texts, dtype, False, **kw)
        emu, _ = FP.forward64(model, texts, dtype, True, **kw)
        rms = float(torch.cat([o["mel"].flatten() for o in ref]).pow(2).mean().sqrt())
        assert peak < 16384, "max |activation| %.1f: fp16 would overflow" % peak
        assert 0.2 <= rms <= 5.0, "mel RMS %.3f: too quiet or too loud to show errors" % rms
        for a, b in zip(ref, emu):
            assert torch.equal(a["reps"], b["reps"])
        _REF_CACHE[key] = (ref, emu)
    return _REF_CACHE[key]


def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def check_outputs(what, synth, got, idx, ref, emu, lens, errors=True):
    """got: infer()'s tuple for the utterances `idx` of the reference lists.  Integers equal, padding as promised, and (errors=True)
    E_new <= 1.5 E_emulated per output.  -> the outputs cut to each utterance's own length."""
    mel, mel_lens, dur_pred, pitch_pred, energy_pred = got
    n_mel = mel.shape[1]
    want_lens = [int(ref[i]["reps"].sum()) for i in idx]
    assert mel.dtype == torch.float32 and mel_lens.dtype == torch.int64
    assert mel_lens.tolist() == want_lens, "%s: mel_lens %s, float64 %s" % (what, mel_lens.tolist(), want_lens)
    assert tuple(mel.shape) == (len(idx), n_mel, max(want_lens))
    reps = synth.last["reps"].cpu().tolist()
    assert reps == sum((ref[i]["reps"].tolist() for i in idx), []), "%s: repetitions differ from float64" % what
    lmax = max(lens[i] for i in idx)
    assert tuple(dur_pred.shape) == (len(idx), lmax) and tuple(pitch_pred.shape) == (len(idx), 1, lmax)
    host = dict(mel=mel.cpu().double(), dur_pred=dur_pred.cpu().double(), pitch_pred=pitch_pred.cpu().double()[:, 0],
                energy_pred=None if energy_pred is None else energy_pred.cpu().double())
    bias = synth.proj_b.cpu()
    for row, i in enumerate(idx):
        t = want_lens[row]
        if t < mel.shape[2]:
            pad_frames = mel[row, :, t:].cpu()
            assert_same(bits(pad_frames), bits(bias[:, None].expand_as(pad_frames).contiguous()), "%s: padding frames of utterance %d" % (what, i))
        for k in ("dur_pred", "pitch_pred", "energy_pred"):
            if host[k] is not None:
                assert not bool(host[k][row, lens[i]:].any()), "%s: %s is not zero behind text %d" % (what, k, i)
    pieces = {}
    for k in KEYS:
        if ref[idx[0]][k] is None:
            assert host[k] is None
            continue
        pieces[k] = [(i, host[k][row, :, :ref[i][k].shape[1]] if k == "mel" else host[k][row, :ref[i][k].numel()]) for row, i in enumerate(idx)]
    if errors:
        assert_errors(what, pieces, ref, emu)
    return pieces


def assert_errors(what, pieces, ref, emu):
    """pieces: output name -> [(utterance, values)] of one run or of several.  E_new <= 1.5 E_emulated over all of them."""
    for k, parts in pieces.items():
        d_new, d_emu = [], []
        for i, g in parts:
            assert bool(torch.isfinite(g).all())
            d_new.append((g - ref[i][k]).flatten())
            d_emu.append((emu[i][k] - ref[i][k]).flatten())
        e_new, e_emu = _rms(torch.cat(d_new)), _rms(torch.cat(d_emu))
        print("%s %s: RMS error %.4e, emulated %.4e (ratio %.3f)" % (what, k, e_new, e_emu, e_new / e_emu if e_emu else float("nan")))
        assert e_emu > 0
        assert e_new <= 1.5 * e_emu, "%s %s: RMS error %.4e against %.4e of the emulated roundings" % (what, k, e_new, e_emu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["small", "default"])
def test_network_against_float64_batched_and_alone(name, dtype):
    ref, emu = references(name, dtype)
    texts = get_texts(name)
    lens = [t.numel() for t in texts]
    synth = FastPitchSynthesizer(get_model(name), dtype=dtype)
    got = synth.infer([t.to(DEV) for t in texts])
    check_outputs("%s %s batch %d" % (name, dtype, len(texts)), synth, got, list(range(len(texts))), ref, emu, lens)
    alone = {}                                                           # the contract: every utterance as if it were alone
    for i, t in enumerate(texts):
        one = check_outputs("%s %s utterance %d alone" % (name, dtype, i), synth, synth.infer([t.to(DEV)]), [i], ref, emu, lens, errors=False)
        for k, parts in one.items():
            alone.setdefault(k, []).extend(parts)
    assert_errors("%s %s the %d batch-1 runs" % (name, dtype, len(texts)), alone, ref, emu)


def test_padded_text_tensor_and_host_tensors_give_the_same_bits():
    texts = get_texts("small")
    synth = FastPitchSynthesizer(get_model("small"), dtype=HF)
    want = [t.clone() if t is not None else None for t in synth.infer([t.to(DEV) for t in texts])]
    pad = torch.zeros((3, 11), dtype=torch.int64)
    for i, t in enumerate(texts):
        pad[i, :t.numel()] = t
    for got in (synth.infer(pad, text_lens=[t.numel() for t in texts]), synth.infer(list(texts))):
        for a, b in zip(got, want):
            assert_same(a if a.dtype == torch.int64 else bits(a), b if b.dtype == torch.int64 else bits(b), "another form of the same texts")


@pytest.mark.parametrize("dtype", DTYPES)
def test_overrides_against_float64(dtype):
    texts = get_texts("small")
    lens = [t.numel() for t in texts]
    tgt = dur_targets(lens)
    g = np.random.RandomState(5)
    pitch_tgt = [torch.from_numpy(g.standard_normal(n)).float() for n in lens]
    energy_tgt = [torch.from_numpy(g.standard_normal(n)).float() for n in lens]
    dev_texts = [t.to(DEV) for t in texts]
    idx = list(range(len(texts)))
    synth = FastPitchSynthesizer(get_model("small"), dtype=dtype)
    # pace + dur_tgt (the second call of the committed fixture)
    ref, emu = references("small", dtype, pace=0.8, dur_tgt=tgt)
    assert [int(o["reps"].sum()) for o in ref] == [22, 10, 4]
    check_outputs("dur_tgt pace 0.8 %s" % dtype, synth, synth.infer(dev_texts, pace=0.8, dur_tgt=padded(tgt, 9)), idx, ref, emu, lens)
    # pace alone changes the predicted lengths (no equality demanded of the float64 side here: only that it is applied)
    slow = synth.infer(dev_texts, pace=0.5)[1].tolist()
    assert slow != synth.infer(dev_texts)[1].tolist() and sum(slow) > sum(int(o["reps"].sum()) for o in references("small", dtype)[0])
    # pitch_tgt and energy_tgt reach the network behind the duration predictor: the predicted lengths stay
    ref, emu = references("small", dtype, pitch_tgt=pitch_tgt)
    check_outputs("pitch_tgt %s" % dtype, synth, synth.infer(dev_texts, pitch_tgt=padded(pitch_tgt, 9, (1,))), idx, ref, emu, lens)
    ref, emu = references("small", dtype, energy_tgt=energy_tgt)
    got = synth.infer(dev_texts, energy_tgt=padded(energy_tgt, 9, (1,)))
    assert got[4] is None
    check_outputs("energy_tgt %s" % dtype, synth, got, idx, ref, emu, lens)
    # a pitch transform (applied in torch on the padded fp32 tensor)
    tr = cli.build_pitch_transformation(cli.parse_args(["-i", "x", "--fastpitch", "f", "--pitch-transform-amplify", "1.5", "--pitch-transform-shift", "20"]))
    ref, emu = references("small", dtype, pitch_transform=tr)
    check_outputs("pitch transform %s" % dtype, synth, synth.infer(dev_texts, pitch_transform=tr), idx, ref, emu, lens)


@pytest.mark.parametrize("dtype", DTYPES)
def test_speaker_against_float64(dtype):
    texts = get_texts("small3")
    lens = [t.numel() for t in texts]
    synth = FastPitchSynthesizer(get_model("small3"), dtype=dtype)
    dev_texts = [t.to(DEV) for t in texts]
    ref, emu = references("small3", dtype, speaker=2)
    got = synth.infer(dev_texts, speaker=2)
    check_outputs("speaker 2 %s" % dtype, synth, got, [0, 1, 2], ref, emu, lens)
    assert not torch.equal(got[2], synth.infer(dev_texts, speaker=0)[2])
    with pytest.raises(ValueError, match="speaker"):
        synth.infer(dev_texts, speaker=3)


def test_one_device_to_host_read_per_batch_and_the_launch_list(monkeypatch):
    texts = [t.to(DEV) for t in get_texts("small")]
    synth = FastPitchSynthesizer(get_model("small"), dtype=HF)
    synth.infer(texts)
    before = synth.d2h_reads
    names, copies = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (copies.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    synth.infer(texts)
    monkeypatch.undo()
    assert synth.d2h_reads == before + 1
    assert copies == ["cpu"], copies                                     # cu_out, once; nothing else leaves the device
    cfg = synth.cfg
    fft = ["dle_gemm", "dle_attention_fwd_varlen", "dle_gemm", "dle_layernorm_fwd", "dle_conv1d_packed_fwd", "dle_conv1d_packed_fwd",
           "dle_layernorm_fwd"]
    pred = ["dle_conv1d_packed_fwd", "dle_fp_relu_layernorm_fwd"] * 2
    want = (["dle_fp_embed"] + fft * cfg["in_fft_n_layers"] + pred + pred + ["dle_fp_scalar_conv_add"] + pred + ["dle_fp_scalar_conv_add"]
            + ["dle_fp_durations", "dle_fp_expand"] + fft * cfg["out_fft_n_layers"] + ["dle_gemm", "dle_fp_unpack_mel"])
    assert names == want


def test_what_is_not_built_raises():
    model = get_model("small")
    with pytest.raises(ValueError, match="16 bits"):
        FastPitchSynthesizer(model, dtype=torch.float32)
    state = model.state_dict()
    for key, val, needle in (("in_fft_d_head", 32, "64-wide"), ("pitch_conditioning_formants", 2, "pitch_conditioning_formants"),
                             ("pre_lnorm", True, "pre_lnorm")):
        cfg = dict(FP.SMALL_CONFIG, **{key: val})
        with pytest.raises(ValueError, match=needle):
            from deeplearningexamples_amd.fastpitch.model import FastPitchModel
            FastPitchSynthesizer(FastPitchModel(cfg), dtype=HF)
    synth = FastPitchSynthesizer(state, config=FP.SMALL_CONFIG, dtype=HF)
    good = torch.tensor([5, 6, 7], device=DEV)
    with pytest.raises(ValueError, match="padding_idx"):
        synth.infer([good, torch.tensor([5, 0, 7], device=DEV)])
    with pytest.raises(ValueError, match="utterance 1 has 1025"):
        synth.infer([good, torch.full((1025,), 5, dtype=torch.int64)])
    # a dur_tgt that predicts 1025 frames: the error names the utterance and its predicted length
    dur = torch.zeros((2, 3))
    dur[0] = torch.tensor([1.0, 2.0, 3.0])
    dur[1] = torch.tensor([75.0 * 13, 50.0, 0.0])
    with pytest.raises(ValueError, match="utterance 1: predicted spectrogram of 1025 frames"):
        synth.infer([good, good], dur_tgt=dur)
    dur[1, 1] = 49.0
    assert synth.infer([good, good], dur_tgt=dur)[1].tolist() == [6, 1024]


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _read_wav(path):
    with wave.open(path, "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float64), f.getframerate()


def _fastpitch_checkpoint(tmp_path):
    path = str(tmp_path / "fastpitch.pt")
    state = {"module." + k: v for k, v in get_model("small").state_dict().items()}
    state["module.attention.key_proj.0.conv.weight"] = torch.zeros(4)
    torch.save({"state_dict": state, "config": dict(FP.SMALL_CONFIG), "train_setup": {}}, path)
    return path


def _expected_lens(phrases):
    synth = FastPitchSynthesizer(get_model("small"), dtype=HF)
    ids = [torch.tensor(cli.encode_text(p, ["english_cleaners_v2"])) for p in phrases]
    return dict(zip(phrases, synth.infer(ids)[1].tolist()))


def test_inference_main_with_hifigan_writes_wavs_and_mels(tmp_path):
    fp = _fastpitch_checkpoint(tmp_path)
    hg = str(tmp_path / "hifigan.pt")
    torch.save({"generator": H.fill_state(H.SMALL_CONFIG), "gen_ema": None, "config": H.SMALL_CONFIG, "train_setup": {"hop_length": 32}}, hg)
    phrases = {"short.wav": "Hi there.", "long.wav": "The quick brown fox."}
    tsv = str(tmp_path / "phrases.tsv")
    open(tsv, "w").write("text\toutput\n" + "".join("%s\t%s\n" % (t, o) for o, t in phrases.items()))
    want = _expected_lens(list(phrases.values()))
    assert all(n > 0 for n in want.values())
    out = str(tmp_path / "out")
    res = cli.main(["-i", tsv, "--fastpitch", fp, "--hifigan", hg, "-o", out, "--amp", "--cuda", "-bs", "2", "--fade-out", "1", "--save-mels"])
    assert [a.shape[0] for a in res["audio"]] == [want[phrases["long.wav"]] * 32, want[phrases["short.wav"]] * 32]     # longest text first
    for name, text in phrases.items():
        pcm, rate = _read_wav(os.path.join(out, name))
        assert rate == 22050 and pcm.shape[0] == want[text] * 32          # mel_len * hop (the vocoder checkpoint's hop_length)
        assert np.isfinite(pcm).all() and np.abs(pcm).max() == 32767 and pcm[-1] == 0
        mel = np.load(os.path.join(out, name.replace(".wav", ".npy")))
        assert mel.shape == (want[text], 80) and np.isfinite(mel).all()
    log = open(os.path.join(out, "nvlog_infer.json")).read()
    for key in ("fastpitch_frames/s", "fastpitch_latency", "hifigan_samples/s", "hifigan_latency", "avg_fastpitch_latency", "avg_hifigan_latency"):
        assert key in log, key


def test_inference_main_with_waveglow_and_mels_only(tmp_path):
    from oracle import waveglow_oracle as WO
    fp = _fastpitch_checkpoint(tmp_path)
    wg = str(tmp_path / "waveglow.pt")
    torch.save({"state_dict": WO.seeded_state(WO.WAVEGLOW_SMALL, 7), "config": WO.WAVEGLOW_SMALL}, wg)
    txt = str(tmp_path / "phrases.txt")
    phrases = ["Hi there.", "The quick brown fox."]
    open(txt, "w").write("\n".join(phrases) + "\n")
    want = _expected_lens(phrases)
    out = str(tmp_path / "wg")
    res = cli.main(["-i", txt, "--fastpitch", fp, "--waveglow", wg, "-o", out, "--amp", "--pace", "1.0", "--fade-out", "0"])
    assert [a.shape[0] for a in res["audio"]] == [want[phrases[1]] * 256, want[phrases[0]] * 256]
    for i, n in enumerate((want[phrases[1]], want[phrases[0]])):
        pcm, rate = _read_wav(os.path.join(out, "audio_%d.wav" % i))
        assert rate == 22050 and pcm.shape[0] == n * 256 and np.abs(pcm).max() == 32767
    out2 = str(tmp_path / "mels")
    res = cli.main(["-i", txt, "--fastpitch", fp, "-o", out2, "--amp", "--save-mels", "--amp-dtype", "bf16"])
    assert res["audio"] == [] and [m.shape[1] for m in res["mels"]] == [80, 80] and all(m.shape[0] > 0 for m in res["mels"])
    assert sorted(f for f in os.listdir(out2) if f.endswith(".npy")) == ["mel_0.npy", "mel_1.npy"]
