"""EfficientNet, host side (no GPU): the module tree against the reference's recorded names / shapes / scaling table, the tiny
fixtures' float64 logits, checkpoint spellings, launch arithmetic, the command line, the packed weight layout, the argument checks of
the functional wrappers, the planning entry point and the self-test of the kernel tests' derived bar.

Fixtures (tests/golden/, recorded from the reference's own EfficientNet class on the CPU): efficientnet_state_dict.json (state-dict
names and shapes of the four published architectures, the scaling table of b0..b7) and efficientnet_tiny.npz (two tiny networks on
b0's kernel / stride / expansion schedule, one per block kind, with their float64 eval() logits for a [2, 3, 33, 31] input).
"""
import json
import os

import pytest
import torch

from deeplearningexamples_amd import functional as F
from deeplearningexamples_amd.convnets import efficientnet as E
from deeplearningexamples_amd.convnets import efficientnet_eval as cli
from tests import _effnet_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF, HF = torch.bfloat16, torch.float16


def _recorded():
    return json.load(open(os.path.join(GOLDEN, "efficientnet_state_dict.json")))


tiny_model = R.tiny_model


@pytest.mark.parametrize("arch", ["efficientnet-b0", "efficientnet-b4", "efficientnet-widese-b0", "efficientnet-widese-b4"])
def test_state_dict_names_and_shapes_equal_the_reference(arch):
    rec = _recorded()["architectures"][arch]
    sd = E.build(arch, device="meta").state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == rec["state_dict"]
    assert len(sd) == rec["tensors"] and sum(v.numel() for v in sd.values()) == rec["elements"]
    assert all(m.eps == 1e-3 for m in E.build(arch, device="meta").modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_scaling_table_equals_the_reference():
    table = _recorded()["scaling"]
    assert sorted(E.ARCHS) == sorted(["efficientnet-b%d" % i for i in range(8)] + ["efficientnet-widese-b%d" % i for i in range(8)])
    for i in range(8):
        for name, wide in (("efficientnet-b%d" % i, False), ("efficientnet-widese-b%d" % i, True)):
            a, t = E.ARCHS[name], table["b%d" % i]
            assert a.widese is wide
            assert (a.stem_channels, a.feature_channels, a.default_image_size) == (t["stem_channels"], t["feature_channels"],
                                                                                   t["default_image_size"])
            for f in ("channels", "num_repeat", "kernel", "stride", "expansion"):
                assert list(getattr(a, f)) == t[f], (name, f)
            assert all(c % 8 == 0 for c in a.channels + (a.stem_channels, a.feature_channels))


@pytest.mark.parametrize("tag", ["orig", "wide"])
def test_tiny_fixture_float64_logits_are_reproduced(tag):
    """The reference's float64 eval() logits, by this project's module in float64: 1e-10 relative to max |logit| (two float64
    forwards of the same graph differ by summation order only; the bar of tests/test_txl_host.py for recorded float64 results)."""
    model, x, want = tiny_model(tag)
    with torch.no_grad():
        got = model.double().eval()(x.double())
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("%s: max |logit| %.4f, relative error %.3e" % (tag, float(want.abs().max()), err))
    assert err <= 1e-10


def test_remap_ngc_round_trip_and_arch_from_state():
    for name in ("efficientnet-b0", "efficientnet-widese-b0", "efficientnet-b4", "efficientnet-widese-b4"):
        sd = E.build(name, device="meta").state_dict()
        ngc = {("layer%d.%s" % (int(k.split(".")[1]) + 1, k.split(".", 2)[2]) if k.startswith("layers.") else k): v for k, v in sd.items()}
        assert any(k.startswith("layer1.block0.") for k in ngc) and not any(k.startswith("layers.") for k in ngc)
        back = E.remap_ngc(ngc)
        assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
        assert list(E.remap_ngc(sd)) == list(sd)                     # already in the module's spelling: untouched
        assert E.arch_from_state(back) == E.ARCHS[name]              # wide-SE recognised from the squeeze weights' shapes
    for tag in ("orig", "wide"):
        model, _, _ = tiny_model(tag)
        assert E.arch_from_state(model.state_dict()).widese is (tag == "wide")


def test_launch_count_arithmetic():
    assert E.ARCHS["efficientnet-b0"].launch_count() == 83 == E.ARCHS["efficientnet-widese-b0"].launch_count()
    assert E.ARCHS["efficientnet-b4"].launch_count() == 162 == E.ARCHS["efficientnet-widese-b4"].launch_count()
    b0 = E.ARCHS["efficientnet-b0"].blocks()
    assert len(b0) == 16 and [b[-1] for b in b0].count(1) == 1 and len(E.ARCHS["efficientnet-b4"].blocks()) == 32


def test_quant_names_are_known_and_rejected():
    with pytest.raises(ValueError, match="pytorch_quantization"):
        E.build("efficientnet-quant-b0")
    with pytest.raises(ValueError, match="unknown architecture"):
        E.build("efficientnet-b8")


def test_cli_defaults_and_rejections():
    for name, size in (("efficientnet-b0", 224), ("efficientnet-b4", 380), ("efficientnet-widese-b4", 380), ("efficientnet-b7", 600)):
        args = cli.parse_args(["--arch", name, "--amp"])
        assert args.image_size == size and args.evaluate and args.arch == name
    args = cli.parse_args(["--amp"])
    assert args.arch == "efficientnet-b0" and args.image_size == 224 and args.batch_size == 256
    assert cli.parse_args(["--amp", "--image-size", "192"]).image_size == 192
    # training flags are parsed and ignored
    assert cli.parse_args(["--amp", "--optimizer", "rmsprop", "--epochs", "400", "--use-ema", "0.999"]).evaluate
    for argv, msg in ((["--amp", "--trt", "True"], r"--trt True: the TensorRT module variants are not built"),
                      ([], r"this path computes in 16 bits: pass --amp"),
                      (["--amp", "--data-backend", "dali-gpu"], r"--data-backend dali-gpu: DALI is not part of this path"),
                      (["--amp", "--arch", "efficientnet-quant-b0"], r"--arch efficientnet-quant-b0: the quantised architectures need")):
        with pytest.raises(SystemExit, match=msg) as e:
            cli.parse_args(argv)
        assert "\n" not in str(e.value)
    with pytest.raises(SystemExit):                                   # argparse: not an EfficientNet name
        cli.parse_args(["--amp", "--arch", "resnet50"])


def test_convnets_main_still_refuses_efficientnet(capsys):
    from deeplearningexamples_amd.convnets import main as cmain
    import argparse
    with pytest.raises(SystemExit) as e:
        cmain.add_parser_arguments(argparse.ArgumentParser()).parse_args(["--arch", "efficientnet-b0"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err


def test_classifier_rejects_fp32_before_touching_a_device():
    from deeplearningexamples_amd.convnets.infer import EfficientNetClassifier
    with pytest.raises(ValueError, match="this path computes in 16 bits"):
        EfficientNetClassifier({}, dtype=torch.float32)


def test_pack_depthwise_weight_layout():
    w = torch.arange(16 * 25, dtype=torch.float32).reshape(16, 1, 5, 5) / 8
    for dtype in (BF, HF):
        p = F.pack_depthwise_weight(w, dtype)
        assert tuple(p.shape) == (5, 5, 16) and p.dtype == dtype and p.is_contiguous()
        for c, r, s in ((0, 0, 0), (3, 1, 4), (15, 4, 2)):
            assert float(p[r, s, c]) == float(w[c, 0, r, s].to(dtype))
    assert tuple(F.pack_depthwise_weight(torch.zeros(8, 1, 3), BF).shape) == (3, 8)      # the Conv1d form is unchanged
    with pytest.raises(ValueError, match="dtype must be"):
        F.pack_depthwise_weight(w, torch.float32)
    with pytest.raises(ValueError, match="expected a"):
        F.pack_depthwise_weight(torch.zeros(8, 2, 3, 3), BF)


def test_functional_argument_checks_raise_before_any_device_is_touched():
    """CPU tensors: a check that came after the device check would raise DleError (a RuntimeError), not ValueError."""
    x, w = torch.zeros(1, 4, 4, 16, dtype=BF), torch.zeros(3, 3, 16, dtype=BF)
    sc, sh = torch.ones(16), torch.zeros(16)
    bad = [((torch.zeros(1, 4, 4, 12, dtype=BF), torch.zeros(3, 3, 12, dtype=BF), torch.ones(12), torch.zeros(12)), {}, "C must be a multiple of 8"),
           ((x, torch.zeros(7, 7, 16, dtype=BF), sc, sh), {}, "k 3 or 5"),
           ((x, w, sc, sh), {"stride": 3}, "stride 1 or 2"),
           ((x.float(), w, sc, sh), {}, "16-bit activations"),
           ((x, w.to(HF), sc, sh), {}, "of x's dtype"),
           ((x, w, sc[:8], sh), {}, "scale / shift"),
           ((torch.zeros(16 * 16 + 4, dtype=BF)[4:].view(1, 4, 4, 16), w, sc, sh), {}, "x must be 16-byte aligned"),
           ((x, w, sc, sh), {"pool": torch.zeros(1, 2, 16)}, r"pool must be a contiguous, 16-byte aligned fp32 \[N,G,C\]")]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            F.dwconv2d_act_fwd(*args, **kw)
    pool, w1, b1, w2, b2 = torch.zeros(2, 3, 16), torch.zeros(4, 16), torch.zeros(4), torch.zeros(16, 4), torch.zeros(16)
    for args, kw, msg in (((pool, 1.0, w1, b1, w2, b2), {"act": "gelu"}, "act must be"),
                          ((pool.half(), 1.0, w1, b1, w2, b2), {}, "contiguous fp32"),
                          ((torch.zeros(2, 3, 12), 1.0, torch.zeros(4, 12), b1, torch.zeros(12, 4), torch.zeros(12)), {}, "multiple of 8"),
                          ((pool, 1.0, w1, b1, w2.t(), b2), {}, "weights must be"),
                          ((torch.zeros(1, 1, 16384), 1.0, torch.zeros(1, 16384), torch.zeros(1), torch.zeros(16384, 1), torch.zeros(16384)),
                           {}, r"C \+ S = 16385")):
        with pytest.raises(ValueError, match=msg):
            F.se_gate_act(*args, **kw)
    for t, msg in ((torch.zeros(2, 4, 12, dtype=BF), "multiple of 8"), (torch.zeros(2, 4, 16), "16-bit"), (torch.zeros(2, 16, dtype=BF), "16-bit")):
        with pytest.raises(ValueError, match=msg):
            F.silu_avgpool_fwd(t)


def test_pool_bands_planning_entry_point():
    """dle_dwconv2d_pool_bands (host only): G = ceil(P / T_r) * ceil(Q / T_q) for the output P x Q of the padded convolution."""
    from deeplearningexamples_amd import _cabi
    lib = _cabi.lib()
    tr, tq, chunk = R.tile_constants()
    assert (tr, tq, chunk) == (8, 16, 64)
    for h, w, k, s in ((1, 1, 3, 1), (7, 7, 5, 1), (112, 112, 3, 1), (112, 112, 3, 2), (9, 10, 3, 2), (2, 3, 5, 2), (tr + 1, tq + 1, 3, 1),
                       (190, 190, 5, 2)):
        p, q = R.out_hw(h, w, k, s)
        want = -(-p // tr) * -(-q // tq)
        assert lib.dle_dwconv2d_pool_bands(h, w, 32, k, s) == want == F.dwconv2d_pool_bands(h, w, 32, k, s)
    assert lib.dle_dwconv2d_pool_bands(112, 112, 32, 3, 1) == 14 * 7
    for bad in ((0, 4, 8, 3, 1), (4, 4, 12, 3, 1), (4, 4, 8, 7, 1), (4, 4, 8, 3, 3)):
        assert lib.dle_dwconv2d_pool_bands(*bad) == -1
    with pytest.raises(ValueError, match="ksize 3 or 5"):
        F.dwconv2d_pool_bands(4, 4, 8, 4, 1)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("in_act,out_act", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_kernel_bar_self_test(dtype, in_act, out_act):
    """The derived bar of tests/_effnet_ref.py admits an fp32 model of the kernel's arithmetic and catches the two faults it is there
    for: a dropped tap, and (with the input SiLU) an input that is not rounded to 16 bits."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((2, 9, 10, 24), generator=g) * 2).to(dtype)
    w = (torch.randn((5, 5, 24), generator=g) * 0.5).to(dtype)
    scale = (torch.rand(24, generator=g) + 0.5) * torch.where(torch.rand(24, generator=g) < 0.5, -1.0, 1.0)
    shift = torch.randn(24, generator=g)
    ref = R.dwconv_ref(x, w, scale, shift, 2, in_act, out_act)
    err = lambda y: (y.double() - ref["y64"]).abs()
    good = err(R.dwconv_model_f32(x, w, scale, shift, 2, in_act, out_act))
    print("largest use of the bar: %.3f" % float((good / ref["bar"]).max()))
    assert bool((good <= ref["bar"]).all())
    assert bool((err(R.dwconv_model_f32(x, w, scale, shift, 2, in_act, out_act, drop_tap=(4, 4))) > ref["bar"]).any())
    if in_act:
        assert bool((err(R.dwconv_model_f32(x, w, scale, shift, 2, in_act, out_act, skip_input_rounding=True)) > ref["bar"]).any())
