"""FastPitch, host side (no GPU): the float64 statement of the network against the reference's own outputs, the state dict, the
checkpoint forms, the command line's parser, text ids, the pitch transforms, and the duration conditions the GPU tests rely on.

tests/golden/fastpitch_infer.npz holds the reference's FastPitch.double().eval().infer outputs for the three fixture texts, EACH RUN
ALONE (tools/make_fastpitch_fixture.py); tests/_fastpitch_ref.forward64(emulate=False) must reproduce them to float64 round-off
(relative 1e-9).  That pins the project's statement of the network -- which the GPU tests compare the kernels against -- to the
reference.
"""
import ast
import json
import os

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.fastpitch import inference as cli
from deeplearningexamples_amd.fastpitch.model import (DEFAULT_CONFIG, FastPitchModel, check_config, ignored_key, normalize_keys,
                                                      positional_table, state_shapes)
from oracle import _ref_import as R
from tests import _fastpitch_ref as FP

needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference tree not mounted")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {"default": DEFAULT_CONFIG, "small": FP.SMALL_CONFIG}


def _golden():
    return np.load(os.path.join(GOLDEN, "fastpitch_infer.npz"))


def test_forward64_equals_the_reference_outputs_of_each_text_alone():
    g = _golden()
    assert json.loads(str(g["config"])) == check_config(FP.SMALL_CONFIG)
    model = FP.make_model(FP.SMALL_CONFIG)
    texts = FP.make_texts(FP.TEXT_LENS["small"])
    for u, t in enumerate(texts):
        assert np.array_equal(g["text%d" % u], t.numpy())
    tgt = [torch.from_numpy(g["b%d_dur_tgt" % u]) for u in range(3)]
    for call, kw in (("a", {}), ("b", dict(pace=0.8, dur_tgt=tgt))):
        out, _ = FP.forward64(model, texts, None, False, **kw)
        for u, o in enumerate(out):
            assert int(g["%s%d_mel_len" % (call, u)][0]) == o["mel"].shape[1] == int(o["reps"].sum())
            for k in ("mel", "dur_pred", "pitch_pred", "energy_pred"):
                ref = torch.from_numpy(g["%s%d_%s" % (call, u, k)])
                assert ref.dtype == torch.float64 and tuple(ref.shape) == tuple(o[k].shape), (call, u, k)
                err = float((o[k] - ref).abs().max()) / float(ref.abs().max())
                assert err <= 1e-9, "%s text %d %s: relative error %.3e" % (call, u, k, err)
    assert out[0]["mel"].shape[1] == 22                                  # the dur_tgt call: (0, 5, 0, 3, 1, 4, 5, 0, 0) / 0.8 -> 6 + 4 + 1 + 5 + 6


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_names_and_shapes(name):
    want = json.load(open(os.path.join(GOLDEN, "fastpitch_state_dict.json")))[name]
    assert any(k.startswith("attention.") for k in want) and any(k.endswith(".inv_freq") for k in want)
    ref = [(k, tuple(v)) for k, v in want.items() if not ignored_key(k)]
    assert ref == [(k, tuple(v)) for k, v in state_shapes(CONFIGS[name]).items()]
    assert [(k, tuple(v.shape)) for k, v in FastPitchModel(CONFIGS[name]).state_dict().items()] == ref


@needs_ref
def test_default_config_equals_the_reference_parser_defaults():
    path = os.path.join(R.REF, "PyTorch", "SpeechSynthesis", "FastPitch", "fastpitch", "arg_parser.py")
    seen = {}
    for call in ast.walk(ast.parse(open(path).read())):
        if isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and call.func.attr == "add_argument":
            flag = call.args[0].value
            kw = {k.arg: k.value for k in call.keywords}
            key = flag.lstrip("-").replace("-", "_")
            if "default" in kw:
                seen[key] = ast.literal_eval(kw["default"])
            elif isinstance(kw.get("action"), ast.Constant) and kw["action"].value == "store_true":
                seen[key] = False
    seen.pop("max_seq_len")
    for k, v in seen.items():
        assert DEFAULT_CONFIG[k] == v, k
    assert set(DEFAULT_CONFIG) - set(seen) == {"n_speakers", "pitch_conditioning_formants"}


def test_checkpoint_forms():
    state = FP.fill_state(FP.SMALL_CONFIG)
    model = FastPitchModel(FP.SMALL_CONFIG).load_state_dict(state)
    wrapped = {"module." + k: v for k, v in state.items()}
    wrapped["module.attention.key_proj.0.conv.weight"] = torch.zeros(3)
    wrapped["module.encoder.pos_emb.inv_freq"] = torch.zeros(64)
    other = FastPitchModel(FP.SMALL_CONFIG).load_state_dict(wrapped)
    for k, v in model.state_dict().items():
        assert torch.equal(other.params[k], v), k
    assert list(normalize_keys(wrapped)) == list(state)
    with pytest.raises(KeyError, match="proj.bias"):
        FastPitchModel(FP.SMALL_CONFIG).load_state_dict({k: v for k, v in state.items() if k != "proj.bias"})
    with pytest.raises(KeyError, match="stranger"):
        FastPitchModel(FP.SMALL_CONFIG).load_state_dict(dict(state, stranger=torch.zeros(1)))
    with pytest.raises(ValueError, match="shape"):
        FastPitchModel(FP.SMALL_CONFIG).load_state_dict(dict(state, **{"proj.bias": torch.zeros(81)}))
    with pytest.raises(ValueError, match="unknown"):
        check_config({"n_mels": 80})
    # a 3-speaker model has the speaker table; the default one has no energy branch
    assert "speaker_emb.weight" in state_shapes(dict(FP.SMALL_CONFIG, n_speakers=3))
    assert not any(k.startswith("energy") for k in state_shapes(DEFAULT_CONFIG))


def test_positional_table_is_the_reference_formula():
    d = 128
    inv_freq = 1 / (10000 ** (torch.arange(0.0, d, 2.0) / d))                       # transformer.py:26, fp32
    pos_seq = torch.arange(7, dtype=torch.float64)
    sinusoid = torch.matmul(pos_seq.unsqueeze(-1), inv_freq.double().unsqueeze(0))  # transformer.py:30-32 after .double()
    want = torch.cat([sinusoid.sin(), sinusoid.cos()], dim=1)
    assert torch.equal(positional_table(7, d), want)
    assert torch.equal(FP.positional64(7, d), want)


# ---- the command line -------------------------------------------------------------------------------------------------------------
REFERENCE_FLAGS = ["-i", "--input", "-o", "--output", "--log-file", "--save-mels", "--cuda", "--cudnn-benchmark", "--l2-promote",
                   "--fastpitch", "--waveglow", "-s", "--waveglow-sigma-infer", "--hifigan", "-d", "--denoising-strength",
                   "--hop-length", "--win-length", "-sr", "--sampling-rate", "--max_wav_value", "--amp", "-bs", "--batch-size",
                   "--warmup-steps", "--repeats", "--torchscript", "--checkpoint-format", "--torch-tensorrt", "--report-mel-loss",
                   "--ema", "--dataset-path", "--speaker", "--affinity", "--fade-out", "--pace", "--pitch-transform-flatten",
                   "--pitch-transform-invert", "--pitch-transform-amplify", "--pitch-transform-shift", "--pitch-transform-custom",
                   "--text-cleaners", "--symbol-set", "--p-arpabet", "--heteronyms-path", "--cmudict-path"]


def _parser_flags():
    return {s for a in cli.build_parser()._actions for s in a.option_strings}


def test_parser_flag_set_is_the_reference_list_plus_this_ports():
    assert _parser_flags() - {"-h", "--help"} == set(REFERENCE_FLAGS) | {"--amp-dtype", "--hifigan-config"}
    a = cli.parse_args(["-i", "x.txt", "--fastpitch", "f.pt", "--hifigan", "g.pt", "--amp", "--cuda", "--pace", "0.9", "-bs", "4"])
    assert (a.pace, a.batch_size, a.fade_out, a.hop_length, a.sampling_rate, a.speaker) == (0.9, 4, 10, 256, 22050, 0)
    assert a.text_cleaners == ["english_cleaners_v2"] and a.amp_dtype == "fp16"


@needs_ref
def test_reference_flag_list_equals_the_reference_file():
    path = os.path.join(R.REF, "PyTorch", "SpeechSynthesis", "FastPitch", "inference.py")
    fn = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == "parse_args")
    flags = set()
    for call in ast.walk(fn):
        if isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and call.func.attr == "add_argument":
            flags |= {a.value for a in call.args if isinstance(a, ast.Constant) and isinstance(a.value, str) and a.value.startswith("-")}
    assert flags == set(REFERENCE_FLAGS)


def test_what_is_not_built_exits_with_one_line(tmp_path):
    txt = tmp_path / "phrases.txt"
    txt.write_text("Hello world.\n")
    base = ["-i", str(txt), "--fastpitch", "f.pt", "--hifigan", "g.pt", "--amp"]
    cases = [(base + ["--torchscript"], "--torchscript"), (base + ["--torch-tensorrt"], "--torch-tensorrt"),
             (base + ["--checkpoint-format", "ts"], "--checkpoint-format ts"), (base + ["--report-mel-loss"], "--report-mel-loss"),
             (base + ["--pitch-transform-custom"], "--pitch-transform-custom"), (base + ["--p-arpabet", "0.5"], "--p-arpabet"),
             (["-i", str(txt), "--hifigan", "g.pt", "--amp"], "--fastpitch"),
             (["-i", str(txt), "--fastpitch", "f.pt", "--amp"], "--save-mels"),
             (base + ["--waveglow", "w.pt"], "single vocoder"),
             (["-i", str(txt), "--fastpitch", "f.pt", "--hifigan", "g.pt"], "16 bits")]
    for argv, needle in cases:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        msg = str(e.value)
        assert needle in msg and "\n" not in msg, (argv, msg)


def test_hifigan_entry_point_names_this_one():
    from deeplearningexamples_amd.hifigan import inference as hcli
    with pytest.raises(SystemExit) as e:
        hcli._reject_unbuilt(hcli.parse_args(["-i", "x.tsv", "--hifigan", "g.pt", "--amp", "--fastpitch", "f.pt"]), {"mel": []})
    assert "fastpitch.inference" in str(e.value) and "\n" not in str(e.value)


def test_text_ids():
    from deeplearningexamples_amd.tacotron2.text import symbols
    assert len(symbols) == 148 == DEFAULT_CONFIG["n_symbols"] and symbols[DEFAULT_CONFIG["padding_idx"]] == "_"
    ids = cli.encode_text("Hello, world.", ["english_cleaners_v2"])
    assert ids == [symbols.index(c) for c in "hello, world."]
    assert cli.encode_text("Dr. Who", ["english_cleaners_v2"]) == [symbols.index(c) for c in "doctor who"]
    assert cli.encode_text("either/or", ["english_cleaners_v2"]) == [symbols.index(c) for c in "either or"]
    arp = cli.encode_text("{HH AW1 S} now", ["english_cleaners_v2"])
    assert arp[:3] == [symbols.index("@" + s) for s in ("HH", "AW1", "S")] and arp[3:] == [symbols.index(c) for c in " now"]
    assert DEFAULT_CONFIG["padding_idx"] not in ids + arp
    with pytest.raises(ValueError, match="numbers"):
        cli.encode_text("In 1984.", ["english_cleaners_v2"])
    batches = cli.prepare_batches({"text": ["ab", "abcd", "abc"], "output": ["a.wav", "b.wav", "c.wav"]}, ["basic_cleaners"], 2)
    assert [b["text_lens"] for b in batches] == [[4, 3], [2]] and [b["output"] for b in batches] == [["b.wav", "c.wav"], ["a.wav"]]


def test_pitch_transform_closures_against_the_reference_formulas():
    pitch = torch.tensor([[[0.5, -1.25, 2.0, 0.0]]])
    lens, mean, std = torch.tensor([4]), 218.14, 67.24

    def build(*argv):
        return cli.build_pitch_transformation(cli.parse_args(["-i", "x", "--fastpitch", "f"] + list(argv)))
    assert build() is None
    # inference.py:218-233: the string the reference evals, built step by step
    assert torch.equal(build("--pitch-transform-flatten")(pitch, lens, mean, std), (pitch) * 0.0)
    assert torch.equal(build("--pitch-transform-invert")(pitch, lens, mean, std), (pitch) * -1.0)
    assert torch.equal(build("--pitch-transform-amplify", "2.5")(pitch, lens, mean, std), (pitch) * 2.5)
    assert torch.equal(build("--pitch-transform-shift", "30")(pitch, lens, mean, std), (pitch) + 30.0 / std)
    allf = build("--pitch-transform-flatten", "--pitch-transform-invert", "--pitch-transform-amplify", "1.5", "--pitch-transform-shift", "-20")
    assert torch.equal(allf(pitch, lens, mean, std), ((((pitch) * 0.0) * -1.0) * 1.5) + -20.0 / std)


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,speakers", [("small", 1), ("default", 1), ("small", 3)])
def test_duration_conditions_of_the_fixture_weights(name, speakers):
    """The integer results (mel_lens, repetitions) must be EQUAL on the GPU; for that to be a fair demand: the durations of the float64
    forward hold zeros and a value above 3, every dur / pace lies at least 0.1 from a rounding boundary -- for the unrounded weights
    and for both 16-bit weight sets -- and the forward with the emulated roundings gives the same repetitions."""
    cfg = dict(CONFIGS[name], n_speakers=speakers) if speakers > 1 else CONFIGS[name]
    model = FP.make_model(cfg)
    texts = FP.make_texts(FP.TEXT_LENS[name])
    base, peak = FP.forward64(model, texts, None, False, stop_after_durations=True)
    durs = torch.cat([o["dur_pred"] for o in base])
    assert bool((durs == 0).any()) and bool((durs > 3).any()), durs
    for dtype in (None, torch.float16, torch.bfloat16):
        for emulate in ((False,) if dtype is None else (False, True)):
            got, _ = FP.forward64(model, texts, dtype, emulate, stop_after_durations=True)
            if not emulate:
                assert min(FP.duration_margin(o["dur_pred"], 1.0) for o in got) >= 0.1, (dtype, [o["dur_pred"] for o in got])
            for a, b in zip(got, base):
                assert torch.equal(a["reps"], b["reps"]), (dtype, emulate)
    if name == "small" and speakers == 1:
        g = _golden()
        assert min(FP.duration_margin(torch.from_numpy(g["b%d_dur_tgt" % u]), 0.8) for u in range(3)) >= 0.1
