"""JasperRecognizer (deeplearningexamples_amd/jasper/infer.py) against the float64 forward of tests/_jasper_ref.py, the launch list,
the one host synchronisation, the checkpoint forms and the errors.  GPU only.

Reference.  _jasper_ref.forward64 on the CPU over the weights as the recognizer holds them (rounded to the 16-bit type; the
BatchNorm coefficients the fp32 fold), each utterance ALONE, 16 zero frames in front of its normalised features.  Yardstick, the
project's established one: the same float64 forward with every value rounded to the 16-bit type where the recognizer rounds (the
packed features, every sub-block's output, every link of the residual chain).  With E the RMS log-prob error against the unrounded
forward over all utterances: E_new <= 1.5 E_emulated; the factor and its justification are those of
tests/test_gpu_resnext_infer.py (the recognizer's fp32 accumulations are not the emulation's float64 ones, so the two sets of
roundings fall differently: equal in distribution, not in value).

Small configuration (_jasper_ref.small_config: dense blocks of 1, 2 and 3 panes; calibrated weights fill_state(cfg, 1, True);
lengths 150, 41 and 2 frames + 16 lead frames -> 83, 29 and 9 rows), bf16 and fp16, a batch of three and each utterance alone (the
two must give the same bits).  Token check, as tests/test_gpu_quartznet_infer.py: a frame is CLEAR when its float64 top-2 gap
exceeds 4 x that frame's own max |emulated - float64|; on clear frames `ids` must equal the float64 argmax; where every frame of
an utterance is clear the transcript must be EQUAL.  Condition, asserted on the CPU-side quantities only: at least 75 % of the
frames of every utterance of >= 8 frames are clear (this seed, on the CPU: 84 % / 86 % / 78 % bf16, 99 % / 100 % / 100 % fp16;
float64 max |activation| 10.7; the argmax takes 18 distinct classes over the 83 rows of the longest utterance).

The 10x5dr YAML itself (restated in _jasper_ref.big_config: the reference's file is not part of this repository), bf16 and fp16,
lengths 120, 33 and 3 frames (68, 25 and 10 rows), uncalibrated random BatchNorm (fill_state(cfg, 99, False); float64 peak 28.1,
emulated RMS error 9.0e-2 bf16 / 1.2e-2 fp16 on the CPU; both forwards in one walk, forward64_both, about 2 s per type): the
E_new <= 1.5 E_emulated check only; the float64 side asserts max |activation| < 16384.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.jasper.infer import JasperRecognizer
from deeplearningexamples_amd.jasper.model import JasperModel, state_shapes
from tests import _jasper_ref as R

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
SMALL_LENS, BIG_LENS = (150, 41, 2), (120, 33, 3)


@functools.lru_cache(maxsize=None)
def small_case():
    cfg = R.small_config()
    return cfg, R.fill_state(cfg, 1, True), R.seeded_features(SMALL_LENS, 7)


@functools.lru_cache(maxsize=None)
def big_case():
    cfg = R.big_config()
    return cfg, R.fill_state(cfg, 99, False), R.seeded_features(BIG_LENS, 8)


@functools.lru_cache(maxsize=None)
def references(which, dtype):
    cfg, state, feats = small_case() if which == "small" else big_case()
    exact, emu, peak = R.forward64_both(state, cfg, feats, dtype)
    print("%s %s: float64 max |activation| %.4g" % (which, dtype, peak))
    assert peak < 16384
    return exact, emu


@functools.lru_cache(maxsize=None)
def recognizer(which, dtype):
    cfg, state, _ = small_case() if which == "small" else big_case()
    return JasperRecognizer(state, cfg, dtype)


def rms(a, b):
    return float((torch.cat([x.reshape(-1) for x in a]) - torch.cat([x.reshape(-1) for x in b])).pow(2).mean().sqrt())


def check_ratio(what, got, exact, emu):
    e_new, e_emu = rms(got, exact), rms(emu, exact)
    print("%s: E_new %.4e, E_emulated %.4e, ratio %.3f" % (what, e_new, e_emu, e_new / e_emu))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert e_new <= 1.5 * e_emu, "%s: RMS error %.4e against %.4e of the emulated roundings" % (what, e_new, e_emu)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_network_against_float64_batched_and_alone(dtype):
    cfg, state, feats = small_case()
    exact, emu = references("small", dtype)
    rec = recognizer("small", dtype)
    lens = list(SMALL_LENS)
    texts, frames, logp = rec.decode(feats, lens, want_logp=True)
    got = [l.cpu().double() for l in logp]
    assert [g.shape for g in got] == [e.shape for e in exact]
    assert [g.shape[0] for g in got] == [83, 29, 9]
    check_ratio("small %s batch of 3" % dtype, got, exact, emu)
    blank = len(rec.labels)
    for i, n in enumerate(lens):
        t1, f1, l1 = rec.decode([feats[i]], [n], want_logp=True)
        assert torch.equal(l1[0].cpu(), logp[i].cpu()), "utterance %d: alone and in the batch differ" % i
        assert t1[0] == texts[i] and torch.equal(f1[0], frames[i])
        # the token check
        top = exact[i].topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 4 * (emu[i] - exact[i]).abs().max(1).values
        share = float(clear.double().mean())
        print("utterance %d: %d frames, %.0f %% clear" % (i, exact[i].shape[0], 100 * share))
        if exact[i].shape[0] >= 8:
            assert share >= 0.75, "a misconfigured test: only %.0f %% of the frames are clear" % (100 * share)
        want_ids = exact[i].argmax(1)
        assert torch.equal(frames[i].long()[clear], want_ids[clear]), "utterance %d: ids differ on clear frames" % i
        assert torch.equal(logp[i].argmax(1).cpu(), frames[i].long()), "ids are not the argmax of the returned log-probs"
        assert texts[i] == "".join(rec.labels[c] for c in R.ctc_collapse(frames[i].tolist(), blank))
        if bool(clear.all()):
            assert texts[i] == "".join(rec.labels[c] for c in R.ctc_collapse(want_ids.tolist(), blank))
    alone = rec.log_probs(feats, lens)
    assert all(torch.equal(a, b) for a, b in zip(alone, logp))


@pytest.mark.parametrize("dtype", DTYPES)
def test_10x5dr_network_against_float64(dtype):
    cfg, state, feats = big_case()
    exact, emu = references("big", dtype)
    rec = recognizer("big", dtype)
    got = [l.cpu().double() for l in rec.log_probs(feats, list(BIG_LENS))]
    assert [g.shape[0] for g in got] == [68, 25, 10]
    check_ratio("10x5dr %s" % dtype, got, exact, emu)


def test_launch_structure_and_one_host_synchronisation(monkeypatch):
    cfg, state, feats = big_case()
    rec = recognizer("big", BF)
    rec.decode(feats, list(BIG_LENS))                                           # warm: nothing lazily built is counted below
    before = rec.d2h_reads
    names, copies = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (copies.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    texts, _, _ = rec.decode(feats, list(BIG_LENS))
    monkeypatch.undo()
    assert rec.d2h_reads == before + 1 and copies == ["cpu"], copies
    assert len(texts) == 3
    count = {n: names.count(n) for n in set(names)}
    assert count == {"dle_qn_normalize_pack_lead": 1, "dle_conv1d_bn_packed_fwd": 53, "dle_conv2d_fwd_affine": 55, "dle_gemm": 1,
                     "dle_ctc_greedy_packed": 1}, count
    assert names[0] == "dle_qn_normalize_pack_lead" and names[-2:] == ["dle_gemm", "dle_ctc_greedy_packed"]
    # Conv1, then per dense block its panes (1, 2, ... 10 of them) FIRST, followed by its five sub-blocks; Conv2 and Conv3 last
    want = ["dle_conv1d_bn_packed_fwd"]
    for i in range(1, 11):
        want += ["dle_conv2d_fwd_affine"] * i + ["dle_conv1d_bn_packed_fwd"] * 5
    want += ["dle_conv1d_bn_packed_fwd"] * 2
    assert names[1:-2] == want


def test_checkpoint_forms_and_errors(tmp_path):
    cfg, state, feats = small_case()
    lens = list(SMALL_LENS)
    want = recognizer("small", BF).decode(feats, lens, want_logp=True)[2]
    ema = R.clone_state(state)
    ema["decoder.layers.0.bias"] = ema["decoder.layers.0.bias"] + 1.0
    plain = JasperRecognizer.from_checkpoint(dict(state), cfg, dtype=BF)
    both = {"state_dict": {"module." + k: v for k, v in state.items()}, "ema_state_dict": ema, "epoch": 3}
    path = str(tmp_path / "jasper.pt")
    torch.save(both, path)
    from_file = JasperRecognizer.from_checkpoint(path, cfg, dtype=BF)
    from_ema = JasperRecognizer.from_checkpoint(path, cfg, ema=True, dtype=BF)
    no_ema = JasperRecognizer.from_checkpoint({"state_dict": state}, cfg, ema=True, dtype=BF)
    v1 = {k.replace("encoder.layers.", "jasper_encoder.encoder.").replace("decoder.layers.", "jasper_decoder.decoder_layers."): v
          for k, v in state.items()}
    v1["audio_preprocessor.featurizer.fb"] = torch.zeros(3)
    v1["acoustic_model.x"] = torch.zeros(3)
    assert not any(k.startswith(("encoder.", "decoder.")) for k in v1)
    from_v1 = JasperRecognizer.from_checkpoint({"state_dict": v1}, cfg, dtype=BF)
    for rec in (plain, from_file, no_ema, from_v1):
        got = rec.log_probs(feats, lens)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(from_ema.log_probs(feats, lens)[0], want[0])
    model = JasperModel(cfg).load_state_dict(state)
    assert list(model.state_dict()) == list(state_shapes(cfg))
    assert all(torch.equal(a, b) for a, b in zip(JasperRecognizer(model, dtype=BF).log_probs(feats, lens), want))
    # the lead frames count: another pad_leading gives other row counts
    assert [l.shape[0] for l in JasperRecognizer(model, dtype=BF, pad_leading=0).log_probs(feats, lens)] == [75, 21, 1]
    with pytest.raises(ValueError, match="16 bits"):
        JasperRecognizer(state, cfg, torch.float32)
    with pytest.raises(C.DleError, match="no CPU path"):
        JasperRecognizer(state, cfg, BF, device="cpu")
    with pytest.raises(ValueError, match="fewer than 2 frames"):
        plain.log_probs([feats[0][:, :1]], [1])
    with pytest.raises(ValueError, match="nemo"):
        JasperRecognizer.from_checkpoint("model.nemo", cfg)
    bad = R.small_config()
    bad["jasper"]["encoder"]["activation"] = "hardtanh"
    with pytest.raises(ValueError, match="relu"):
        JasperRecognizer(state, bad, BF)


def test_transcribe_runs_the_front_end():
    rec = recognizer("small", HF)
    g = torch.Generator().manual_seed(3)
    waves = [torch.randn(16000, generator=g) * 0.1, torch.randn(4000, generator=g) * 0.1]
    a = rec.transcribe(waves, torch.Generator().manual_seed(5))
    b = rec.transcribe(waves, torch.Generator().manual_seed(5))
    assert a == b and len(a) == 2 and all(isinstance(t, str) for t in a)


def test_inference_main_on_a_wav_and_on_a_manifest(tmp_path):
    import json

    import yaml
    from scipy.io import wavfile

    from deeplearningexamples_amd.jasper import inference as cli
    cfg, state, _ = small_case()
    cfg_path, ckpt = str(tmp_path / "small.yaml"), str(tmp_path / "jasper.pt")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({"state_dict": state}, ckpt)
    g = torch.Generator().manual_seed(9)
    names = []
    for i, n in enumerate((8000, 4800)):
        w = (torch.randn(n, generator=g) * 0.1).clamp(-1, 1)
        names.append(str(tmp_path / ("u%d.wav" % i)))
        wavfile.write(names[-1], 16000, (w * 32767).round().to(torch.int16).numpy())
    common = ["--model_config", cfg_path, "--ckpt", ckpt, "--amp", "--amp-dtype", "bf16", "--seed", "3", "-o", str(tmp_path / "out")]
    r1 = cli.main(common + ["--transcribe_wav", names[0], "--save_predictions", str(tmp_path / "p.txt"),
                            "--save_logits", str(tmp_path / "l.pt")])
    assert len(r1["preds"]) == 1 and open(str(tmp_path / "p.txt")).read() == r1["preds"][0]
    logits = torch.load(str(tmp_path / "l.pt"))
    assert isinstance(logits, list) and tuple(logits[0].shape) == (33, 29)       # 8000 samples -> 50 + 16 frames -> 33 rows
    r0 = cli.main(common + ["--transcribe_wav", names[0], "--pad_leading", "0", "--save_logits", str(tmp_path / "l0.pt")])
    assert tuple(torch.load(str(tmp_path / "l0.pt"))[0].shape) == (25, 29) and len(r0["preds"]) == 1
    from deeplearningexamples_amd.quartznet.inference import read_wav
    rec = JasperRecognizer.from_checkpoint(ckpt, cfg, dtype=BF)
    assert rec.transcribe([read_wav(names[0])], torch.Generator().manual_seed(3)) == r1["preds"]
    manifest = [{"transcript": "Ab, c", "files": [{"fname": "u0.wav"}], "original_duration": 0.5},
                {"transcript": "d", "files": [{"fname": "u1.wav"}], "original_duration": 0.3}]
    with open(str(tmp_path / "m.json"), "w") as f:
        json.dump(manifest, f)
    run = common + ["--dataset_dir", str(tmp_path), "--val_manifests", "m.json", "--dali_device", "none", "--batch_size", "2"]
    r2 = cli.main(run + ["--override_config", "input_val.audio_dataset.trim_silence=false"])
    assert len(r2["preds"]) == 2 and r2["preds"][0] == r1["preds"][0]             # the same utterance in a batch of two
    assert r2["wer"] == cli.qn.word_error_rate(r2["preds"], ["ab c", "d"])[0]
    with pytest.raises(SystemExit, match="trim_silence=false"):
        cli.main(run)
