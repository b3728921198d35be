"""QuartzNet's host side (no GPU): the parameter container against the reference's state dict, the float64 stand-in against the
reference's own float64 forward, the front end against the reference's, the CTC rule, the word error rate, the command line.

Fixtures (tools/make_quartznet_fixture.py, written from the reference's modules): tests/golden/quartznet_state_dict.json,
quartznet_cli_flags.json, quartznet_infer.npz.
"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.quartznet import inference as cli
from deeplearningexamples_amd.quartznet.features import FilterbankFeatures
from deeplearningexamples_amd.quartznet.infer import QuartzNetRecognizer
from deeplearningexamples_amd.quartznet.model import QuartzNetModel, apply_overrides, check_config, state_shapes
from oracle import _ref_import as REFI
from tests import _quartznet_ref as R

needs_ref = pytest.mark.skipif(not REFI.have_reference(), reason="reference tree not mounted")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIGS = {"15x5": R.big_config, "small": R.small_config}


def _tool():
    spec = importlib.util.spec_from_file_location("make_quartznet_fixture", os.path.join(ROOT, "tools", "make_quartznet_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_names_and_shapes_equal_the_fixture(name):
    want = json.load(open(os.path.join(GOLDEN, "quartznet_state_dict.json")))[name]
    cfg = CONFIGS[name]()
    got = state_shapes(cfg)
    assert list(got) == list(want)
    assert {k: list(v) for k, v in got.items()} == want
    model = QuartzNetModel(cfg)
    assert [(k, list(v.shape)) for k, v in model.state_dict().items()] == [(k, v) for k, v in want.items()]
    if name == "15x5":
        assert sum(1 for k in want if ".mconv." in k and k.endswith("weight") and len(want[k]) == 3 and want[k][1] == 1) == 77


@needs_ref
def test_fixtures_equal_the_reference_live():
    import yaml
    tool = _tool()
    ref_model, _ = tool.import_reference()
    want = json.load(open(os.path.join(GOLDEN, "quartznet_state_dict.json")))
    big = yaml.safe_load(open(os.path.join(tool.reference_root(), "configs", "quartznet15x5_speedp-online-1.15_speca.yaml")))
    for name, cfg in (("15x5", big), ("small", R.small_config())):
        live = {k: list(v.shape) for k, v in tool.reference_module(ref_model, cfg).state_dict().items()}
        assert list(live) == list(want[name]) and live == want[name]
    # the restated 15x5 configuration builds what the YAML builds
    assert state_shapes(R.big_config()) == state_shapes(big)
    assert check_config(R.big_config())[2] == check_config(big)[2] and check_config(big)[0] == R.LABELS
    assert tool.parser_flags() == json.load(open(os.path.join(GOLDEN, "quartznet_cli_flags.json")))


def test_forward64_equals_the_reference_float64_forward():
    z = np.load(os.path.join(GOLDEN, "quartznet_infer.npz"))
    cfg = R.small_config()
    got, peak = R.forward64(R.fill_state(cfg, 1, True), cfg, R.seeded_features((150, 41, 2), 7))
    for u, g in enumerate(got):
        want = torch.from_numpy(z["logp%d" % u])
        assert g.shape == want.shape
        assert float((g - want).abs().max()) <= 1e-12, u
    assert 1.0 < peak < 64.0


def test_front_end_against_the_reference_features():
    """Both sides are fp32 torch CPU pipelines over the same operations (the reference's FilterbankFeatures with dither 0 and the mel
    bank of this project bound in; here FilterbankFeatures.log_mel followed by the per-feature normalisation in fp32 torch).  The bar
    is 4 x the largest difference between the reference front end run in fp32 and the same arithmetic in float64, measured on the CPU
    while the fixture was made: 4.067e-05 (stored in the fixture as feat_fp32_vs_fp64), so the bar is 1.63e-04."""
    z = np.load(os.path.join(GOLDEN, "quartznet_infer.npz"))
    measured = float(z["feat_fp32_vs_fp64"])
    assert 1e-6 < measured < 1e-3
    bar = 4 * measured
    tool = _tool()
    fp = FilterbankFeatures(**dict(R.FEATURES, dither=0.0))
    for u, w in enumerate(tool.synthetic_waves()):
        mel = fp.log_mel(w)
        n = int(z["feat%d_len" % u])
        assert mel.shape == (64, n) and n == fp.get_seq_len(w.numel())
        norm = (mel - mel.mean(1, keepdim=True)) / (mel.std(1, keepdim=True) + 1e-5)
        want = torch.from_numpy(z["feat%d" % u])
        assert bool((want[:, n:] == 0).all())
        err = float((norm - want[:, :n]).abs().max())
        print("waveform %d: %d frames, max difference %.3e (bar %.3e)" % (u, n, err, bar))
        assert err <= bar
    # dither: seeded, and it changes the features
    w = tool.synthetic_waves()[2]
    fd = FilterbankFeatures(**dict(R.FEATURES, dither=1e-2))
    a, b = fd.log_mel(w, torch.Generator().manual_seed(3)), fd.log_mel(w, torch.Generator().manual_seed(3))
    assert torch.equal(a, b) and not torch.equal(a, fp.log_mel(w))


def _keep_mask(ids, blank):
    """The rule of common/helpers.py:45-61 as a predicate per position, on arrays: a frame is kept when it is no blank and differs
    from the frame in front of it (in front of the first frame stands a blank)."""
    cur = np.asarray(ids, dtype=np.int64)
    prev = np.concatenate([[blank], cur[:-1]]) if cur.size else cur
    return ((cur != prev) | (prev == blank)) & (cur != blank)


def test_ctc_rule_on_hand_made_rows_and_against_the_array_form():
    labels = R.LABELS + ["<BLANK>"]
    blank, a, b = len(labels) - 1, 1, 2
    text = lambda ids: "".join(labels[c] for c in R.ctc_collapse(ids, blank))
    assert text([a, a, blank, a, b, b]) == "aab"                       # "a a _ a b b"
    assert text([blank] * 4) == "" and text([]) == "" and text([3]) == "c"
    assert text([blank, b, b, blank, blank, b]) == "bb"
    assert text([a, blank, a]) == "aa" and text([a, a, a]) == "a" and text([0, 0, a]) == " a"
    rnd = random.Random(5)
    for _ in range(50):
        ids = [rnd.choice([blank, blank, 1, 2, 3]) for _ in range(rnd.randrange(1, 40))]
        assert R.ctc_collapse(ids, blank) == np.asarray(ids)[_keep_mask(ids, blank)].tolist()


def test_word_error_rate_on_hand_made_pairs():
    assert cli.word_error_rate(["a b c"], ["a b c"]) == (0.0, 0, 3)
    assert cli.word_error_rate(["a b c", "x"], ["a b d", "x y"]) == (0.4, 2, 5)          # one substitution, one deletion
    assert cli.word_error_rate(["the cat sat on a mat"], ["the cat sat"])[1:] == (3, 3)  # three insertions
    assert cli.word_error_rate(["", "b"], ["a", "b"]) == (0.5, 1, 2)
    assert cli.word_error_rate(["a"], [""])[0] == float("inf")
    assert cli.word_error_rate(["a", "extra"], ["a"]) == (0.0, 0, 1)                    # surplus hypotheses are cut
    with pytest.raises(ValueError):
        cli.word_error_rate(["a"], ["a", "b"])
    assert cli.normalize_transcript("Hello, World's  END", R.LABELS) == "hello world's end"
    assert cli.edit_distance(list("kitten"), list("sitting")) == 3 and cli.edit_distance([], ["a", "b"]) == 2


def test_latency_percentiles_on_a_hand_made_series():
    secs = [9.0] * 5 + [i / 1000.0 for i in range(1, 101)]              # the first five are dropped; then 1 .. 100 ms
    lat = cli.latency_percentiles(secs)
    assert lat[0.5] == pytest.approx(50.5)
    # positions int(100 (1 - a)) of 100, 99, ..., 1: 9 (1 - 0.9 is just below 0.1 in binary floating point), 5 and 1
    assert lat[0.9] == pytest.approx(91.0) and lat[0.95] == pytest.approx(95.0) and lat[0.99] == pytest.approx(99.0)


def test_every_reference_flag_parses():
    flags = json.load(open(os.path.join(GOLDEN, "quartznet_cli_flags.json")))
    assert len(flags) >= 20
    for f in flags:
        for name in f["flags"]:
            argv = ["--model_config", "cfg.yaml"] if "--model_config" not in f["flags"] else []
            val = f["choices"][0] if f["choices"] else "3"
            argv += [name] + ([] if f["values"] == 0 else [val])
            cli.parse_args(argv)
    args = cli.parse_args(["--model_config", "c", "--fp16", "--amp-dtype", "bf16", "--override_config", "a.b=1", "--override_config", "c=2"])
    assert args.amp and args.amp_dtype == "bf16" and args.override_config == ["a.b=1", "c=2"]


def _exit_message(argv, cfg=None):
    with pytest.raises(SystemExit) as e:
        cli.reject_unbuilt(cli.parse_args(["--model_config", "c"] + argv), cfg)
    msg = str(e.value)
    assert msg and "\n" not in msg, msg
    return msg


def test_each_rejection_is_one_line(monkeypatch):
    wav = ["--amp", "--transcribe_wav", "a.wav"]
    assert "--cpu" in _exit_message(["--cpu"] + wav)
    assert "TorchScript" in _exit_message(["--torchscript"] + wav)
    assert "TorchScript" in _exit_message(["--torchscript_export"] + wav)
    assert ".nemo" in _exit_message(["--ckpt", "QuartzNet.nemo"] + wav)
    assert "16 bits" in _exit_message(["--transcribe_wav", "a.wav"])
    assert "DALI" in _exit_message(["--amp", "--dataset_dir", "d", "--val_manifests", "m.json"])
    assert "no input" in _exit_message(["--amp"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "several GPUs" in _exit_message(wav)
    monkeypatch.delenv("WORLD_SIZE")
    manifest = ["--amp", "--dali_device", "none", "--dataset_dir", "d", "--val_manifests", "m.json"]
    cfg = R.small_config()
    assert "--override_config input_val.audio_dataset.trim_silence=false" in _exit_message(manifest, cfg)
    cfg = apply_overrides(R.small_config(), ["input_val.audio_dataset.trim_silence=false"])
    assert cfg["input_val"]["audio_dataset"]["trim_silence"] is False
    cli.reject_unbuilt(cli.parse_args(["--model_config", "c"] + manifest), cfg)            # now inside what is built
    cfg["input_val"]["audio_dataset"]["sample_rate"] = 8000
    assert "16 kHz" in _exit_message(wav, cfg)
    with pytest.raises(ValueError):
        apply_overrides(R.small_config(), ["no.such.section.key=1"])


def test_config_rejections_are_one_line():
    def bad(edit, word):
        cfg = R.small_config()
        edit(cfg)
        with pytest.raises(ValueError) as e:
            check_config(cfg)
        assert word in str(e.value) and "\n" not in str(e.value)
    enc = lambda c: c["quartznet"]["encoder"]
    bad(lambda c: enc(c).update(activation="hardtanh"), "relu")
    bad(lambda c: enc(c)["blocks"][1].update(normalization="group"), "batch")
    bad(lambda c: enc(c)["blocks"][1].update(groups=4), "groups")
    bad(lambda c: enc(c)["blocks"][1].update(residual_dense=True), "residual_dense")
    bad(lambda c: enc(c).update(use_conv_masks=False), "use_conv_masks")
    bad(lambda c: enc(c).update(frame_splicing=3), "frame_splicing")
    bad(lambda c: c["input_val"]["filterbank_features"].update(normalize="all_features"), "per_feature")
    bad(lambda c: enc(c)["blocks"][0].update(dilation=[2]), "stride OR dilation")
    check_config(R.small_config())


def test_fp32_is_rejected_before_any_device_is_touched():
    cfg = R.small_config()
    with pytest.raises(ValueError, match="16 bits"):
        QuartzNetRecognizer(R.fill_state(cfg, 1, False), cfg, torch.float32)


def test_product_files_do_not_import_tests():
    for name in ("model", "features", "infer", "inference"):
        src = open(os.path.join(ROOT, "deeplearningexamples_amd", "quartznet", name + ".py")).read()
        assert "import tests" not in src and "from tests" not in src
    assert "deeplearningexamples_amd.quartznet.inference" in sys.modules
