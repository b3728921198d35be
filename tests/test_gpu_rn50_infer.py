"""ResNet50Classifier (convnets/infer.py): the whole network with BatchNorm in the convolution epilogues, against a float64 CPU
forward and against the parent path ResNetTrainer.infer; launch structure, graph replay, checkpoint forms, predict.  GPU only.

Accuracy.  A ResNet50 whose BatchNorm running statistics, gamma (bn3 included) and beta are randomised (the default
initialisation would make the affine map trivial), batch 2 and batch 1 at 3 x 64 x 64: the stages run at 16 x 16 (halo-tile
kernel), 8 x 8, 4 x 4 and 2 x 2 (implicit-GEMM fallback).  Reference: torch float64 on the CPU over the same 16-bit-rounded weights
and images.  Yardstick: ResNetTrainer.infer on the same weights and images (two launches per unit, one more rounding per unit).  The
classifier's maximum absolute logit error may be at most 1.5 times the parent's -- the two paths round at different places, so
neither dominates element by element, but the fused path has one rounding fewer per unit.  Both errors are printed.  The argmax
must equal the float64 argmax wherever the float64 top-2 gap exceeds twice the measured error.

The same bar holds for the two routes the 64 x 64 case does not reach: the generic stem (odd stem output: 62 x 62 images) and units
routed back to the two-launch form (infer.TWO_LAUNCH_UNITS).

Measured on an MI355X (max |logit error| against float64, fused / parent): DESIGN.md section 4h.
"""
import copy

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.convnets import checkpoint2model
from deeplearningexamples_amd.convnets.engine import ResNetTrainer
from deeplearningexamples_amd.convnets.infer import ResNet50Classifier
from deeplearningexamples_amd.convnets.resnet import ResNet50
from deeplearningexamples_amd.utils import checkpoint as ckpt
from tests._exact_grid import assert_same, bits

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DEV = "cuda"
CLASSES = 100


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=g) * 0.2)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    m = ResNet50(num_classes=CLASSES, device=DEV)
    _randomise_bn(m, 99)
    return m


@pytest.fixture(scope="module")
def images():
    return torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(7)).to(DEV)


def ref_forward64(model, images, dtype):
    """float64 CPU forward under model.eval() over the 16-bit-rounded weights and images (biases and BatchNorm stay fp32 values)."""
    f = torch.nn.functional
    m = copy.deepcopy(model).cpu().double().eval()
    r16 = lambda w: w.detach().to(dtype).double()
    bn = lambda x, b: f.batch_norm(x, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)
    conv = lambda x, c: f.conv2d(x, r16(c.weight.float()), None, c.stride, c.padding)
    with torch.no_grad():
        x = images.cpu().to(dtype).double()
        x = f.max_pool2d(torch.relu(bn(conv(x, m.conv1), m.bn1)), 3, 2, 1)
        for layer in m.layers:
            for blk in layer:
                idn = x if blk.downsample is None else bn(conv(x, blk.downsample[0]), blk.downsample[1])
                o = torch.relu(bn(conv(x, blk.conv1), blk.bn1))
                o = torch.relu(bn(conv(o, blk.conv2), blk.bn2))
                x = torch.relu(bn(conv(o, blk.conv3), blk.bn3) + idn)
        return x.mean((2, 3)) @ r16(m.fc.weight.float()).t() + m.fc.bias


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_logits_against_float64_and_the_parent_path(model, images, dtype):
    ref = ref_forward64(model, images, dtype)
    clf = ResNet50Classifier(model, dtype=dtype)
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=dtype)
    for n in (2, 1):
        got = clf.logits(images[:n])
        parent = trainer.infer(images[:n])
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, CLASSES)
        assert bool(torch.isfinite(got).all())
        e_new = float((got.cpu().double() - ref[:n]).abs().max())
        e_par = float((parent.cpu().double() - ref[:n]).abs().max())
        print("%s batch %d: max |logit error| fused %.4e, parent %.4e (ratio %.3f); max |logit| %.3f" % (
            dtype, n, e_new, e_par, e_new / e_par, float(ref[:n].abs().max())))
        assert e_par > 0
        assert e_new <= 1.5 * e_par, "fused path %.4e against parent %.4e" % (e_new, e_par)
        top2 = torch.topk(ref[:n], 2, dim=1)
        clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * e_new
        assert torch.equal(got.cpu().argmax(1)[clear], top2.indices[:, 0][clear])


def _check_against_parent(clf, trainer, model, imgs, dtype, what):
    ref = ref_forward64(model, imgs, dtype)
    got, parent = clf.logits(imgs), trainer.infer(imgs)
    e_new = float((got.cpu().double() - ref).abs().max())
    e_par = float((parent.cpu().double() - ref).abs().max())
    print("%s: max |logit error| %.4e, parent %.4e (ratio %.3f)" % (what, e_new, e_par, e_new / e_par))
    assert bool(torch.isfinite(got).all()) and e_par > 0
    assert e_new <= 1.5 * e_par, "%s: %.4e against parent %.4e" % (what, e_new, e_par)


def test_generic_stem_route_on_an_odd_stem_output(model, monkeypatch):
    """62 x 62 images: the stem's output is 31 x 31, outside the pooling pass's even-size rule -- the 7x7 / 2 convolution runs through
    dle_conv2d_fwd_affine on the 8-channel image, then dle_maxpool_fwd."""
    imgs = torch.randn((2, 3, 62, 62), generator=torch.Generator().manual_seed(17)).to(DEV)
    clf = ResNet50Classifier(model, dtype=BF)
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=BF)
    _check_against_parent(clf, trainer, model, imgs, BF, "generic stem, 62 x 62")
    names = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    clf.logits(imgs)
    assert names.count("dle_conv2d_fwd_affine") == 53 and names.count("dle_maxpool_fwd") == 1
    assert "dle_stem_conv7_fwd" not in names and "dle_bn_relu_maxpool_fwd" not in names and "dle_bn_fwd_apply" not in names


def test_units_routed_back_to_two_launches(model, images, monkeypatch):
    """infer.TWO_LAUNCH_UNITS: the listed units run as dle_conv2d_fwd + dle_bn_fwd_apply on (0, scale, 1, shift); same bar."""
    from deeplearningexamples_amd.convnets import infer
    monkeypatch.setattr(infer, "TWO_LAUNCH_UNITS", frozenset({(3, 1, 64, 64), (1, 1, 64, 256), (1, 2, 256, 512)}))
    clf = ResNet50Classifier(model, dtype=BF)
    routed = sum(u.two_launch for blk in clf.blocks for u in blk if u is not None)
    assert routed == 3 + 4 + 1                # conv2 and conv3 (+ downsample) of the first stage's blocks, stage 2's downsample
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=BF)
    _check_against_parent(clf, trainer, model, images, BF, "8 units as two launches")
    names = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    clf.logits(images)
    assert names.count("dle_conv2d_fwd") == routed == names.count("dle_bn_fwd_apply") and names.count("dle_conv2d_fwd_affine") == 52 - routed


def test_channels_last_and_uint8_inputs(model, images):
    clf = ResNet50Classifier(model, dtype=BF)
    want = clf.logits(images)
    assert_same(bits(clf.logits(images.contiguous(memory_format=torch.channels_last))), bits(want), "channels_last input")
    u8 = torch.randint(0, 256, (2, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=BF)
    e = float((clf.logits(u8) - trainer.infer(u8)).abs().max())
    assert e < 0.25 * float(trainer.infer(u8).abs().max()) + 1.0       # same normalisation as the parent (a coarse sanity bar)


def test_launch_structure(model, images, monkeypatch):
    """53 convolution launches + stem pool + avgpool + fc; the halo-tile kernel takes every 3x3 stride-1 unit inside its envelope
    (at 64 x 64 input: the three conv2 of the 16 x 16 stage; the 8 x 8 ... 2 x 2 images are below its size rule H W >= 100);
    no dle_bn_fwd_apply."""
    clf = ResNet50Classifier(model, dtype=BF)
    clf.logits(images)                                                # (first call outside the count: lazy constants)
    names = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    before = int(C.lib().dle_conv3x3_affine_launch_count())
    clf.logits(images)
    halo = int(C.lib().dle_conv3x3_affine_launch_count()) - before
    assert names.count("dle_conv2d_fwd_affine") == 52 and names.count("dle_stem_conv7_fwd") == 1
    assert names.count("dle_bn_relu_maxpool_fwd") == 1 and names.count("dle_avgpool_fwd") == 1 and names.count("dle_gemm") == 1
    assert not [n for n in names if n.startswith("dle_bn_fwd_apply") or n == "dle_conv2d_fwd"], names
    assert sorted(set(names)) == ["dle_avgpool_fwd", "dle_bn_relu_maxpool_fwd", "dle_conv2d_fwd_affine", "dle_gemm", "dle_nchw_to_nhwc",
                                  "dle_stem_conv7_fwd"]
    hw = 64 // 4
    expect = 0
    for li, nblocks in enumerate((3, 4, 6, 3)):
        for b in range(nblocks):
            stride = 2 if (li > 0 and b == 0) else 1
            if stride == 2:
                hw //= 2
            expect += int(stride == 1 and hw * hw >= 100)
    assert expect == 3 and halo == expect


def test_graph_replay_matches_eager(model, images):
    eager = ResNet50Classifier(model, dtype=BF)
    graphed = ResNet50Classifier(model, dtype=BF, graphs=True)
    other = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(8)).to(DEV)
    for n in (2, 1):
        want_a, want_b = eager.logits(images[:n]).clone(), eager.logits(other[:n]).clone()
        assert not torch.equal(want_a, want_b)
        for _ in range(4):                                            # two eager warm-up calls, the capture + replay, a replay
            got = graphed.logits(images[:n]).clone()
            assert_same(bits(got), bits(want_a), "graph call, batch %d" % n)
        g = graphed._graphs[((n, 3, 64, 64), torch.float32)]
        assert g.graph is not None
        assert_same(bits(graphed.logits(other[:n]).clone()), bits(want_b), "replay with new images, batch %d" % n)
        assert_same(bits(graphed.logits(images[:n]).clone()), bits(want_a), "replay with the first images again, batch %d" % n)


def test_from_checkpoint_forms(model, images, tmp_path):
    trainer = ResNetTrainer(model, lr=0.1, compute_dtype=BF, ema=0.999)
    with torch.no_grad():                                             # an averaged model that differs from the model
        for p in trainer.ema_model.parameters():
            p.mul_(0.9)
    trainer.mark_ema_dirty()
    path = str(tmp_path / "checkpoint_0001.pth.tar")
    torch.save(ckpt.rn50_trainer_state(trainer, epoch=1, best_prec1=1.0), path)
    want = ResNet50Classifier(model, dtype=BF).logits(images)
    want_ema = ResNet50Classifier(trainer.ema_model, dtype=BF).logits(images)
    assert not torch.equal(want, want_ema)
    assert_same(bits(ResNet50Classifier.from_checkpoint(path, dtype=BF).logits(images)), bits(want), "trainer checkpoint")
    assert_same(bits(ResNet50Classifier.from_checkpoint(path, ema=True, dtype=BF).logits(images)), bits(want_ema), "averaged model")
    # the parent path on the averaged model agrees on what "the averaged weights" are
    assert float((trainer.infer(images, ema=True) - want_ema).abs().max()) < float((want - want_ema).abs().max())
    mod = str(tmp_path / "module.pth")
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, mod)
    assert_same(bits(ResNet50Classifier.from_checkpoint(mod, dtype=BF).logits(images)), bits(want), "module.-prefixed state dict")
    for ema, ref in ((False, want), (True, want_ema)):
        out = str(tmp_path / ("weights%d.pth" % ema))
        checkpoint2model.main(["--checkpoint-path", path, "--weight-path", out] + (["--ema"] if ema else []))
        assert_same(bits(ResNet50Classifier.from_checkpoint(out, dtype=BF).logits(images)), bits(ref), "checkpoint2model output")
    assert_same(bits(ResNet50Classifier(model.state_dict(), dtype=BF).logits(images)), bits(want), "a state dict in memory")


def test_predict(model, images):
    clf = ResNet50Classifier(model, dtype=HF)
    probs, top = clf.predict(images, topk=5)
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (2, CLASSES) and tuple(top.shape) == (2, 5)
    assert float((probs.double().sum(1) - 1).abs().max()) <= CLASSES * 2.0 ** -24
    p5 = probs.gather(1, top)
    assert bool((p5[:, :-1] >= p5[:, 1:]).all())
    assert torch.equal(p5, torch.topk(probs, 5, dim=1).values)
    assert torch.equal(top[:, 0], clf.logits(images).argmax(1))
