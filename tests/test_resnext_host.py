"""Host side of the (SE-)ResNeXt101-32x4d inference path (convnets/resnext.py, infer.py, main.py, classify.py): state-dict names,
the grouped-weight packing, command lines.  CPU only."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _ref_import as R  # noqa: E402

from deeplearningexamples_amd import functional as F  # noqa: E402
from deeplearningexamples_amd.convnets import classify, main as cmain, resnext  # noqa: E402

needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference tree not mounted")
ARCHS = ("resnext101-32x4d", "se-resnext101-32x4d")


def _fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "resnext_state_dict.json")))


@pytest.mark.parametrize("arch", ARCHS)
def test_state_dict_names_and_shapes_equal_the_fixture(arch):
    want = _fixture()[arch]
    model = resnext.build(arch, device="cpu")
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert sorted(got) == sorted(want)
    assert got == want
    # the shapes the issue names
    assert got["layers.0.0.conv2.weight"] == [128, 4, 3, 3] and got["layers.3.2.conv2.weight"] == [1024, 32, 3, 3]
    se = arch.startswith("se-")
    assert ("layers.2.22.squeeze.squeeze.weight" in got) == se == resnext.state_has_se(got)
    if se:
        assert got["layers.0.0.squeeze.squeeze.weight"] == [16, 256] and got["layers.0.0.squeeze.squeeze.bias"] == [16]
        assert got["layers.0.0.squeeze.expand.weight"] == [256, 16] and got["layers.0.0.squeeze.expand.bias"] == [256]
    assert sum(len(layer) for layer in model.layers) == 33 and len(model.bottlenecks()) == 33
    assert [blk.conv2.stride[0] for blk in model.bottlenecks()].count(2) == 3


@needs_ref
def test_fixture_equals_the_reference_live():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_resnext_state_dict_fixture as gen
    assert gen.reference_names_and_shapes() == _fixture()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ko,cg", [(128, 4), (64, 16), (1024, 32)])
def test_grouped_weight_packing_is_a_permute(ko, cg, dtype):
    w = torch.randn((ko, cg, 3, 3), generator=torch.Generator().manual_seed(ko + cg))
    for src in (w, w.contiguous(memory_format=torch.channels_last), w.double()):
        p = F.pack_grouped_weight(src, dtype)
        assert tuple(p.shape) == (ko, 3, 3, cg) and p.dtype == dtype and p.is_contiguous()
        assert torch.equal(p, w.to(dtype).permute(0, 2, 3, 1))
        # element by element: packed[k][r][s][c] is w[k][c][r][s]
        assert float(p[ko - 1, 2, 0, cg - 1]) == float(w[ko - 1, cg - 1, 2, 0].to(dtype))
    with pytest.raises(ValueError):
        F.pack_grouped_weight(torch.zeros(8, 4, 1, 1), dtype)
    with pytest.raises(ValueError):
        F.pack_grouped_weight(w, torch.float32)


def _parser():
    import argparse
    return cmain.add_parser_arguments(argparse.ArgumentParser())


@pytest.mark.parametrize("arch", ARCHS)
def test_main_accepts_the_names_and_is_inference_only(arch):
    a = _parser().parse_args(["--arch", arch, "--evaluate", "--amp"])
    assert a.arch == arch and a.evaluate
    cmain._reject_unbuilt(a)                                           # with --evaluate: accepted
    with pytest.raises(SystemExit) as e:                               # without: a one-line message, before any device is touched
        cmain.main(["--arch", arch, "--amp", "--data-backend", "synthetic"])
    msg = str(e.value)
    assert "inference-only" in msg and "resnet50" in msg and "--evaluate" in msg and "\n" not in msg, msg
    assert _parser().parse_args([]).arch == "resnet50"
    with pytest.raises(SystemExit):
        _parser().parse_args(["--arch", "efficientnet-b0"])


def test_classify_builds_se_resnext_and_points_resnext_at_main():
    import argparse
    p = classify.add_parser_arguments(argparse.ArgumentParser())
    classify.reject_unbuilt(p.parse_args(["--image", "x.npy", "--arch", "se-resnext101-32x4d"]))
    classify.reject_unbuilt(p.parse_args(["--image", "x.npy"]))
    with pytest.raises(SystemExit) as e:
        classify.reject_unbuilt(p.parse_args(["--image", "x.npy", "-a", "resnext101-32x4d"]))
    msg = str(e.value)
    assert "--evaluate" in msg and "main" in msg and "resnet50" in msg and "\n" not in msg, msg
    for arch in classify.ARCHS:
        if arch.startswith("efficientnet"):
            with pytest.raises(SystemExit):
                classify.reject_unbuilt(p.parse_args(["--image", "x.npy", "--arch", arch]))


def test_classifier_rejects_fp32():
    from deeplearningexamples_amd.convnets.infer import ResNeXtClassifier
    with pytest.raises(ValueError) as e:
        ResNeXtClassifier({}, dtype=torch.float32)
    assert "16 bits" in str(e.value)
