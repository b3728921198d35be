"""Host side of the HiFi-GAN path (no GPU): the parameter container against the reference's state dict, the weight-norm fold,
the transposed-convolution packing, the float64 reference of the GPU tests against the reference's own output, the command line.

Fixtures (tools/make_hifigan_fixture.py): tests/golden/hifigan_state_dict.json -- names and shapes of the reference's Generator for
the V1 and the small configuration; tests/golden/hifigan_infer.npz -- small configuration, spectrogram [2, 80, 9], the float64 output
of the reference module after remove_weight_norm(); the weights are tests/_hifigan_ref.fill_state, repeated here.

Bar of the float64 forward against the stored output: 1e-9.  The audio is bounded by 1 and a float64 sum of at most 11 * 512 terms
of the sizes involved errs near 1e-12: about three orders of margin (measured: 3e-16).
"""
import ast
import json
import os

import numpy as np
import pytest
import torch

from oracle import _ref_import as R
from deeplearningexamples_amd import functional as F
from deeplearningexamples_amd.hifigan import inference as cli
from deeplearningexamples_amd.hifigan.model import V1_CONFIG, HifiGanGenerator, layers, state_shapes
from tests import _hifigan_ref as H

needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference tree not mounted")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {"v1": V1_CONFIG, "small": H.SMALL_CONFIG}


def test_state_dict_names_and_shapes_equal_the_fixture():
    fixture = json.load(open(os.path.join(GOLDEN, "hifigan_state_dict.json")))
    assert sorted(fixture) == ["small", "v1"]
    for name, cfg in CONFIGS.items():
        got = {k: list(v.shape) for k, v in HifiGanGenerator(cfg).state_dict().items()}
        assert got == fixture[name], name
        assert list(got) == list(fixture[name]), "%s: key order differs from the reference's state_dict()" % name
        assert got == {k: list(s) for k, s in state_shapes(cfg).items()} and list(got) == list(state_shapes(cfg))
    assert len(layers(V1_CONFIG)) == 1 + 4 + 4 * 3 * 6 + 1 and len(fixture["v1"]) == 3 * 78


@needs_ref
def test_fixture_equals_the_reference_live():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_make_hifigan_fixture", os.path.join(os.path.dirname(GOLDEN), "..", "tools",
                                                                                         "make_hifigan_fixture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    models = tool.import_reference_models()
    fixture = json.load(open(os.path.join(GOLDEN, "hifigan_state_dict.json")))
    for name, cfg in CONFIGS.items():
        live = {k: list(v.shape) for k, v in tool.reference_generator(models, cfg).state_dict().items()}
        assert live == fixture[name] and list(live) == list(fixture[name]), name
    # fold_weight_norm against remove_weight_norm, bit for bit in fp32, for a Conv1d and a ConvTranspose1d
    g = tool.reference_generator(models, H.SMALL_CONFIG, H.fill_state(H.SMALL_CONFIG))
    sd = {k: v.clone() for k, v in g.state_dict().items()}
    g.remove_weight_norm()
    for layer in ("conv_pre", "ups.0", "ups.2", "resblocks.1.2.convs1.1", "conv_post"):
        want = dict(g.named_parameters())[layer + ".weight"].detach()
        got = F.fold_weight_norm(sd[layer + ".weight_v"], sd[layer + ".weight_g"])
        assert got.dtype == torch.float32 and torch.equal(got, want), layer


@pytest.mark.parametrize("shape", [(24, 16, 7), (16, 8, 4)], ids=["conv1d", "conv_transpose1d"])
def test_fold_weight_norm_equals_the_closed_form(shape):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(shape, generator=g)
    gg = torch.rand((shape[0], 1, 1), generator=g) + 0.5
    got = F.fold_weight_norm(v, gg)
    v64 = v.double()
    want = gg.double() * v64 / v64.pow(2).sum((1, 2), keepdim=True).sqrt()
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert float((got.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())     # a division, a product, the norm
    # the norm runs over every dimension but 0: scaling one slice of dimension 0 leaves the others unchanged
    v2 = v.clone()
    v2[0] *= 3
    assert torch.equal(F.fold_weight_norm(v2, gg)[1:], got[1:])


@pytest.mark.parametrize("u,k", [(8, 16), (2, 4), (4, 8)])
def test_pack_upsample_weight_is_the_transposed_convolution(u, k):
    cin, cout, b, t = 6, 4, 2, 5
    g = torch.Generator().manual_seed(5)
    w = torch.randn((cin, cout, k), generator=g, dtype=torch.float64)
    x = torch.randn((b, cin, t), generator=g, dtype=torch.float64)
    bias = torch.randn((cout,), generator=g, dtype=torch.float64)
    packed = F.pack_upsample_weight(w, u, torch.float64)
    assert tuple(packed.shape) == (u * cout, 3, cin) and packed.dtype == torch.float64
    y = torch.nn.functional.conv1d(x, packed.permute(0, 2, 1), bias.repeat(u), padding=1)       # [B, u Cout, T]
    got = y.permute(0, 2, 1).reshape(b, t * u, cout).permute(0, 2, 1)      # [B, T, u Cout] read as [B, T u, Cout]
    want = torch.nn.functional.conv_transpose1d(x, w, bias, u, (k - u) // 2)
    assert tuple(want.shape) == (b, cout, t * u)
    assert float((got - want).abs().max()) <= 1e-12
    pad = (k - u) // 2
    for p, ko, j, c in ((0, 0, 0, 0), (u - 1, cout - 1, 2, cin - 1), (1, 2, 1, 3), (u - 1, 1, 0, 2), (0, 3, 2, 5)):
        i = (1 - j) * u + p + pad
        assert float(packed[p * cout + ko, j, c]) == (float(w[c, ko, i]) if 0 <= i < k else 0.0)
    assert F.pack_upsample_weight(w.float(), u, torch.bfloat16).dtype == torch.bfloat16


def test_pack_upsample_weight_rejects_what_the_identity_does_not_cover():
    with pytest.raises(ValueError):
        F.pack_upsample_weight(torch.zeros(4, 4, 7), 4, torch.float16)          # k - u odd
    with pytest.raises(ValueError):
        F.pack_upsample_weight(torch.zeros(4, 4, 10), 4, torch.float16)         # k > 2 u
    with pytest.raises(ValueError):
        F.pack_upsample_weight(torch.zeros(4, 4, 8), 4, torch.float32)          # a 16-bit type (or float64) only


def test_float64_forward_equals_the_reference_output():
    g = np.load(os.path.join(GOLDEN, "hifigan_infer.npz"))
    cfg = json.loads(str(g["config"]))
    assert cfg == H.SMALL_CONFIG
    mel = torch.from_numpy(g["mel"])
    assert tuple(mel.shape) == (2, 80, 9) and torch.equal(mel, H.make_mel((2, 80, 9)))
    audio, peak = H.forward64(H.build_model(cfg), mel)
    want = torch.from_numpy(g["audio"])
    assert want.dtype == torch.float64 and tuple(want.shape) == (2, 9 * 32) and float(want.abs().max()) <= 1.0
    diff = float((audio - want).abs().max())
    print("float64 forward against the stored reference output: max |diff| %.3e, max |activation| %.2f" % (diff, peak))
    assert diff <= 1e-9


def test_old_flat_resblock_keys_and_folded_weights_load_to_the_same_tensors():
    state = H.fill_state(H.SMALL_CONFIG)
    model = H.build_model(H.SMALL_CONFIG, state)
    flat = {}
    for k, v in state.items():
        parts = k.split(".")
        if parts[0] == "resblocks":
            k = "resblocks.%d.%s" % (int(parts[1]) * 3 + int(parts[2]), ".".join(parts[3:]))
        flat["module." + k] = v
    assert any(k.startswith("module.resblocks.8.") for k in flat) and all(len(k.split(".")) != 7 for k in flat)
    other = HifiGanGenerator(H.SMALL_CONFIG).load_state_dict(flat)
    assert list(other.state_dict()) == list(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(other.params[k], v), k
    folded = {}
    for l in model.layers:
        folded[l.name + ".weight"] = model.folded_weight(l.name)
        folded[l.name + ".bias"] = state[l.name + ".bias"]
    third = HifiGanGenerator(H.SMALL_CONFIG).load_state_dict(folded)
    for l in model.layers:
        assert torch.equal(third.folded_weight(l.name), model.folded_weight(l.name)), l.name
    with pytest.raises(KeyError):
        HifiGanGenerator(H.SMALL_CONFIG).load_state_dict({k: v for k, v in state.items() if k != "conv_post.bias"})


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


def test_parser_has_every_flag_of_the_reference_script():
    assert set(REFERENCE_FLAGS) <= _parser_flags()
    assert {"--hifigan-config", "--amp-dtype"} <= _parser_flags()
    a = cli.parse_args(["-i", "x.tsv", "--hifigan", "g.pt", "--amp", "--cuda", "-d", "0.01", "-bs", "4", "--ema", "--fade-out", "3"])
    assert (a.denoising_strength, a.batch_size, a.ema, a.fade_out, a.hop_length, a.sampling_rate) == (0.01, 4, True, 3, 256, 22050)


@needs_ref
def test_reference_flag_list_equals_the_reference_file():
    path = os.path.join(R.REF, "PyTorch", "SpeechSynthesis", "HiFiGAN", "inference.py")
    fn = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == "parse_args")
    flags = set()
    for call in ast.walk(fn):
        if isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and call.func.attr == "add_argument":
            flags |= {a.value for a in call.args if isinstance(a, ast.Constant) and isinstance(a.value, str) and a.value.startswith("-")}
    assert flags == set(REFERENCE_FLAGS)


def test_what_is_not_built_exits_with_one_line(tmp_path):
    tsv = tmp_path / "mels.tsv"
    tsv.write_text("mel\toutput\nmels/a.pt\ta.wav\n")
    txt = tmp_path / "phrases.txt"
    txt.write_text("Hello world.\n")
    base = ["-i", str(tsv), "--hifigan", "g.pt", "--amp"]
    cases = [(base + ["--fastpitch", "fp.pt"], "--fastpitch"), (base + ["--waveglow", "wg.pt"], "--waveglow"),
             (base + ["--torchscript"], "--torchscript"), (base + ["--torch-tensorrt"], "--torch-tensorrt"),
             (base + ["--checkpoint-format", "ts"], "--checkpoint-format ts"), (base + ["--report-mel-loss"], "--report-mel-loss"),
             (["-i", str(txt), "--hifigan", "g.pt", "--amp"], "tacotron2.inference"),
             (["-i", str(tsv), "--hifigan", "g.pt"], "16 bits")]
    for argv, needle in cases:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        msg = str(e.value)
        assert needle in msg and "\n" not in msg, (argv, msg)
