"""Jasper's host side (no GPU): the parameter container against the reference's state dict, the float64 stand-in against the
reference's own float64 forward, the dense-pane bookkeeping, the front end against the reference's, the command line.

Fixtures (tools/make_jasper_fixture.py, written from the reference's modules): tests/golden/jasper_state_dict.json,
jasper_cli_flags.json, jasper_infer.npz.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.jasper import inference as cli
from deeplearningexamples_amd.jasper.infer import JasperRecognizer
from deeplearningexamples_amd.jasper.model import (JasperModel, apply_overrides, check_config, convert_v1_state_dict, residual_panes,
                                                   state_shapes)
from deeplearningexamples_amd.quartznet.features import FilterbankFeatures
from oracle import _ref_import as REFI
from tests import _jasper_ref as R

needs_ref = pytest.mark.skipif(not REFI.have_reference(), reason="reference tree not mounted")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIGS = {"10x5dr": R.big_config, "small": R.small_config}
# the seven YAMLs under the reference's configs/ differ in the input sections and in use_conv_masks (the `_nomask` one); their
# encoder block lists are the one of _jasper_ref.big_config
YAMLS = ("jasper10x5dr_speca", "jasper10x5dr_speedp-offline", "jasper10x5dr_speedp-offline_speca",
         "jasper10x5dr_speedp-offline_speca_nomask", "jasper10x5dr_speedp-online-discrete",
         "jasper10x5dr_speedp-online-discrete_speca", "jasper10x5dr_speedp-online_speca")


def _tool():
    spec = importlib.util.spec_from_file_location("make_jasper_fixture", os.path.join(ROOT, "tools", "make_jasper_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_names_and_shapes_equal_the_fixture(name):
    want = json.load(open(os.path.join(GOLDEN, "jasper_state_dict.json")))[name]
    cfg = CONFIGS[name]()
    got = state_shapes(cfg)
    assert list(got) == list(want)
    assert {k: list(v) for k, v in got.items()} == want
    model = JasperModel(cfg)
    assert [(k, list(v.shape)) for k, v in model.state_dict().items()] == [(k, v) for k, v in want.items()]
    if name == "10x5dr":
        assert sum(1 for k in want if ".conv." in k and len(want[k]) == 3) == 53
        assert sum(1 for k in want if ".res." in k and len(want[k]) == 3) == 55


@needs_ref
def test_fixtures_equal_the_reference_live():
    import yaml
    tool = _tool()
    ref_model, _ = tool.import_reference()
    want = json.load(open(os.path.join(GOLDEN, "jasper_state_dict.json")))
    load = lambda name: json.loads(json.dumps(yaml.safe_load(open(os.path.join(tool.reference_root(), "configs", name + ".yaml")))))
    big = load("jasper10x5dr_speedp-online_speca")
    for name, cfg in (("10x5dr", big), ("small", R.small_config())):
        live = {k: list(v.shape) for k, v in tool.reference_module(ref_model, cfg).state_dict().items()}
        assert list(live) == list(want[name]) and live == want[name]
    # the restated 10x5dr configuration builds what the YAML builds, and all seven YAMLs hold that block list
    assert state_shapes(R.big_config()) == state_shapes(big)
    assert check_config(R.big_config())[2] == check_config(big)[2] and check_config(big)[0] == R.LABELS
    assert sorted(f[:-5] for f in os.listdir(os.path.join(tool.reference_root(), "configs"))) == sorted(YAMLS)
    for name in YAMLS:
        assert load(name)["jasper"]["encoder"]["blocks"] == big["jasper"]["encoder"]["blocks"], name
    assert tool.parser_flags() == json.load(open(os.path.join(GOLDEN, "jasper_cli_flags.json")))


def test_forward64_equals_the_reference_float64_forward():
    z = np.load(os.path.join(GOLDEN, "jasper_infer.npz"))
    cfg = R.small_config()
    got, peak = R.forward64(R.fill_state(cfg, 1, True), cfg, R.seeded_features((150, 41, 2), 7))
    assert [g.shape[0] for g in got] == [83, 29, 9]
    for u, g in enumerate(got):
        want = torch.from_numpy(z["logp%d" % u])
        assert g.shape == want.shape
        assert float((g - want).abs().max()) <= 1e-12, u
    assert 1.0 < peak < 64.0


def test_clear_frame_condition_of_the_gpu_test_holds_on_the_cpu():
    """What tests/test_gpu_jasper_infer.py needs of its seed, on the float64 and emulated forwards alone: at least 75 % of the
    frames of every utterance of >= 8 frames are clear."""
    cfg = R.small_config()
    state, feats = R.fill_state(cfg, 1, True), R.seeded_features((150, 41, 2), 7)
    for dtype in (torch.bfloat16, torch.float16):
        exact, _ = R.forward64(state, cfg, feats, dtype, False)
        emu, _ = R.forward64(state, cfg, feats, dtype, True)
        for e, m in zip(exact, emu):
            top = e.topk(2, dim=1).values
            clear = (top[:, 0] - top[:, 1]) > 4 * (m - e).abs().max(1).values
            assert e.shape[0] >= 8 and float(clear.double().mean()) >= 0.75


def test_pane_bookkeeping():
    blk = lambda f, residual=True, dense=True: dict(filters=f, residual=residual, **({"residual_dense": True} if dense else {}))
    # the block list of all seven reference YAMLs: Conv1, ten dense blocks, Conv2, Conv3
    for name in YAMLS:
        cfg = R.big_config()
        raw = cfg["jasper"]["encoder"]["blocks"]
        panes = residual_panes(raw, 64)
        widths = [256, 256, 256, 384, 384, 512, 512, 640, 640, 768]             # the inputs of the ten dense blocks
        assert panes[0] == [] and panes[11:] == [[], []]
        for i in range(10):
            assert panes[1 + i] == widths[:i + 1], (name, i)
        assert sum(len(p) for p in panes) == 55
        if name.endswith("_nomask"):
            cfg["jasper"]["encoder"]["use_conv_masks"] = False
            with pytest.raises(ValueError, match="use_conv_masks"):
                check_config(cfg)
        else:
            assert [b["panes"] for b in check_config(cfg)[2]] == panes
    # residual: true without residual_dense: one pane, the block's own input; the list starts again behind it and behind a
    # block without a residual
    raw = [blk(64, residual=False, dense=False), blk(96), blk(128), blk(160, dense=False), blk(192), blk(224, residual=False, dense=False),
           blk(256)]
    assert residual_panes(raw, 32) == [[], [64], [64, 96], [128], [160], [], [224]]
    small = check_config(R.small_config())[2]
    assert [b["panes"] for b in small] == [[], [64], [64, 64], [64, 64, 64], [], []]
    assert [b["dense"] for b in small] == [False, True, True, True, False, False]
    one = R.small_config()
    del one["jasper"]["encoder"]["blocks"][2]["residual_dense"]
    assert [b["panes"] for b in check_config(one)[2]] == [[], [64], [64], [64], [], []]
    assert "encoder.layers.2.res.1.0.weight" not in state_shapes(one) and "encoder.layers.2.res.0.0.weight" in state_shapes(one)


def test_front_end_against_the_reference_jasper_features():
    """The Jasper recipe's common/features.py differs from QuartzNet's in the splicing helper only, the identity at frame_splicing
    1: quartznet.features.FilterbankFeatures against the Jasper reference's output, under the bar of tests/test_quartznet_host.py
    (4 x the fp32-against-float64 difference of the reference front end measured while the fixture was made, 4.067e-05)."""
    z = np.load(os.path.join(GOLDEN, "jasper_infer.npz"))
    measured = float(z["feat_fp32_vs_fp64"])
    assert 1e-6 < measured < 1e-3
    bar = 4 * measured
    tool = _tool()
    fp = FilterbankFeatures(**dict(R.FEATURES, dither=0.0))
    for u, w in enumerate(tool.synthetic_waves()):
        mel = fp.log_mel(w)
        n = int(z["feat%d_len" % u])
        assert mel.shape == (64, n)
        norm = (mel - mel.mean(1, keepdim=True)) / (mel.std(1, keepdim=True) + 1e-5)
        want = torch.from_numpy(z["feat%d" % u])
        err = float((norm - want[:, :n]).abs().max())
        print("waveform %d: %d frames, max difference %.3e (bar %.3e)" % (u, n, err, bar))
        assert err <= bar


def test_every_reference_flag_parses():
    flags = json.load(open(os.path.join(GOLDEN, "jasper_cli_flags.json")))
    assert len(flags) >= 21 and any("--pad_leading" in f["flags"] for f in flags)
    for f in flags:
        for name in f["flags"]:
            argv = ["--model_config", "cfg.yaml"] if "--model_config" not in f["flags"] else []
            val = f["choices"][0] if f["choices"] else "3"
            argv += [name] + ([] if f["values"] == 0 else [val])
            args = cli.parse_args(argv)
            if f["values"] == "+":
                assert getattr(args, name.lstrip("-")) == [val]
            with pytest.raises(SystemExit):                                     # the arity: a flag that takes a value needs it
                cli.parse_args(argv[:-1] if f["values"] != 0 else argv + ["=surplus"])
    args = cli.parse_args(["--model_config", "c", "--fp16", "--amp-dtype", "bf16", "--override_config", "a.b=1", "--override_config", "c=2"])
    assert args.amp and args.amp_dtype == "bf16" and args.override_config == ["a.b=1", "c=2"] and args.pad_leading == 16
    assert cli.parse_args(["--model_config", "c", "--pad_leading", "0"]).pad_leading == 0


def _exit_message(argv, cfg=None):
    with pytest.raises(SystemExit) as e:
        cli.qn.reject_unbuilt(cli.parse_args(["--model_config", "c"] + argv), cfg)
    msg = str(e.value)
    assert msg and "\n" not in msg, msg
    return msg


def test_each_rejection_is_one_line(monkeypatch):
    wav = ["--amp", "--transcribe_wav", "a.wav"]
    assert "--cpu" in _exit_message(["--cpu"] + wav)
    assert "TorchScript" in _exit_message(["--torchscript"] + wav)
    assert "TorchScript" in _exit_message(["--torchscript_export"] + wav)
    assert ".nemo" in _exit_message(["--ckpt", "Jasper.nemo"] + wav)
    assert "16 bits" in _exit_message(["--transcribe_wav", "a.wav"])
    assert "DALI" in _exit_message(["--amp", "--dataset_dir", "d", "--val_manifests", "m.json"])
    assert "DALI" in _exit_message(["--amp", "--dali_device", "cpu", "--dataset_dir", "d", "--val_manifests", "m.json"])
    assert "no input" in _exit_message(["--amp"])
    # main() itself refuses before it reads a file
    for argv, word in ((["--cpu"] + wav, "--cpu"), (["--torchscript"] + wav, "TorchScript")):
        with pytest.raises(SystemExit, match=word):
            cli.main(["--model_config", "does-not-exist.yaml"] + argv)


def test_config_rejections_are_one_line():
    def bad(edit, word):
        cfg = R.small_config()
        edit(cfg)
        with pytest.raises(ValueError) as e:
            check_config(cfg)
        assert word in str(e.value) and "\n" not in str(e.value)
    enc = lambda c: c["jasper"]["encoder"]
    bad(lambda c: enc(c).update(activation="hardtanh"), "relu")
    bad(lambda c: enc(c).update(activation="selu"), "relu")
    bad(lambda c: enc(c).update(use_conv_masks=False), "use_conv_masks")
    bad(lambda c: enc(c).update(frame_splicing=3), "frame_splicing")
    bad(lambda c: c["input_val"]["filterbank_features"].update(frame_splicing=3), "frame_splicing")
    bad(lambda c: c["input_val"]["filterbank_features"].update(normalize="all_features"), "per_feature")
    bad(lambda c: enc(c)["blocks"][0].update(dilation=[2]), "stride OR dilation")
    bad(lambda c: enc(c)["blocks"][1].update(separable=True), "unknown key")
    bad(lambda c: c.pop("jasper"), "not a Jasper config")
    check_config(R.small_config())
    cfg = apply_overrides(R.small_config(), ["jasper.encoder.activation=selu"])
    with pytest.raises(ValueError, match="relu"):
        check_config(cfg)


def test_convert_v1_state_dict_rules():
    t = torch.zeros(1)
    v1 = {"jasper_encoder.encoder.0.conv.0.weight": t, "jasper_decoder.decoder_layers.0.bias": t, "acoustic_model.w": t,
          "audio_preprocessor.featurizer.window": t, "encoder.layers.3.res.1.1.bias": t,
          "x.jasper_encoder.encoder.0": t}                                      # the patterns are anchored at the start
    got = convert_v1_state_dict(v1)
    assert list(got) == ["encoder.layers.0.conv.0.weight", "decoder.layers.0.bias", "encoder.layers.3.res.1.1.bias",
                         "x.jasper_encoder.encoder.0"]
    cfg = R.small_config()
    state = R.fill_state(cfg, 1, False)
    old = {k.replace("encoder.layers.", "jasper_encoder.encoder.").replace("decoder.layers.", "jasper_decoder.decoder_layers."): v
           for k, v in state.items()}
    model = JasperModel(cfg).load_state_dict(dict(old, **{"audio_preprocessor.fb": t}))
    assert all(torch.equal(model.params[k], v) for k, v in state.items())
    with pytest.raises(KeyError, match="unexpected key"):
        JasperModel(cfg).load_state_dict(dict(state, stray=t))


def test_fp32_is_rejected_before_any_device_is_touched():
    cfg = R.small_config()
    with pytest.raises(ValueError, match="16 bits"):
        JasperRecognizer(R.fill_state(cfg, 1, False), cfg, torch.float32)


def test_product_files_do_not_import_tests():
    for name in ("model", "infer", "inference"):
        src = open(os.path.join(ROOT, "deeplearningexamples_amd", "jasper", name + ".py")).read()
        assert "import tests" not in src and "from tests" not in src
