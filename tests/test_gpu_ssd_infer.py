"""SSDDetector (ssd/infer.py): the whole network and the detection against float64; launch list, host reads, graph replay,
checkpoint forms, main --mode evaluation.  GPU only.

The width = 8 network (trunk [128, 64, 64, 32, 32, 32]) on 300 x 300 images, batch 2 and batch 1, bf16 and fp16.  BatchNorm
statistics randomised as tests/test_gpu_resnext_infer.py does; the confidence heads calibrated on the test images
(tests/_ssd_ref.calibrate_heads) so that the network detects a few dozen boxes per image with no close decision.

raw().  Reference: a float64 CPU forward over the 16-bit-rounded weights and images; yardstick: the same forward with each value
rounded to the 16-bit type where the detector rounds (after every unit and after every head).  With E the RMS error of (ploc, plabel)
against the unrounded forward: E_new <= 1.5 E_emulated (the criterion and its justification are tests/test_gpu_resnext_infer.py's).

detect().  Reference: the float64 statements of tests/_ssd_ref.py applied to the detector's OWN 16-bit head outputs (raw()), so the
network's rounding is not in the comparison.  The margin condition (tests/test_ssd_host.py) is asserted on that float64 run; under
it the (box index, label) lists must be identical, boxes and scores within tests/_ssd_ref.decode_bar.
"""
import copy
import functools
import json

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.ssd import main as smain
from deeplearningexamples_amd.ssd import model as M
from deeplearningexamples_amd.ssd.infer import SSDDetector
from tests import _ssd_ref as R
from tests._exact_grid import assert_same, bits

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
DEV = "cuda"
CASES = [(0.5, 200), (0.45, 20)]


@functools.lru_cache(maxsize=None)
def get_images():
    return torch.randn((2, 3, 300, 300), generator=torch.Generator().manual_seed(7))


@functools.lru_cache(maxsize=None)
def get_model(dtype):
    torch.manual_seed(4321)
    m = R.randomise(M.SSD300(width=8).eval(), 77)
    return R.calibrate_heads(m, get_images(), dtype, 3)


@functools.lru_cache(maxsize=None)
def get_detector(dtype, graphs=False):
    return SSDDetector(copy.deepcopy(get_model(dtype)).to(DEV), dtype=dtype, graphs=graphs)


@functools.lru_cache(maxsize=None)
def references(dtype):
    out = []
    for emulate in (False, True):
        heads, peak = R.forward64(get_model(dtype), get_images(), dtype, emulate)
        assert peak < 16384
        out.append(torch.cat(R.bbox_view(heads, 81), dim=1))
    return out


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_against_float64_and_the_emulated_roundings(dtype):
    ref, emu = references(dtype)
    det = get_detector(dtype)
    both = None
    for n in (2, 1):
        ploc, plabel = det.raw(get_images()[:n].to(DEV))
        assert tuple(ploc.shape) == (n, 4, 8732) and tuple(plabel.shape) == (n, 81, 8732) and ploc.dtype == dtype
        got = torch.cat((ploc, plabel), dim=1)
        assert bool(torch.isfinite(got).all())
        e_new, e_emu = _rms(got.cpu().double() - ref[:n]), _rms(emu[:n] - ref[:n])
        print("%s batch %d: RMS error %.4e, emulated %.4e (ratio %.3f); max |value| %.2f" % (dtype, n, e_new, e_emu, e_new / e_emu, float(ref.abs().max())))
        assert e_emu > 0 and e_new <= 1.5 * e_emu, "RMS error %.4e against %.4e of the emulated roundings" % (e_new, e_emu)
        if n == 2:
            both = got
        else:
            assert_same(bits(got), bits(both[:1]), "an image alone against the same image in a batch of two")


@pytest.mark.parametrize("dtype", DTYPES)
def test_detect_against_the_float64_statements_on_its_own_head_outputs(dtype):
    det = get_detector(dtype)
    images = get_images().to(DEV)
    d = det.dboxes
    ploc, plabel = (t.cpu().float() for t in det.raw(images))
    b64, p64 = R.decode_ref(ploc.double(), plabel.double(), d("xywh"))
    box_bar, prob_bar = R.decode_bar(ploc, plabel, d("xywh"))
    for criteria, max_output in CASES:
        boxes, labels, scores, counts, index = (t.cpu() for t in det.detect(images, criteria, max_output, with_index=True))
        assert tuple(boxes.shape) == (2, max_output, 4) and labels.dtype == torch.int32 and tuple(counts.shape) == (2,)
        for i in range(2):
            margins = R.new_margins()
            idx, lab, sc, _ = R.detect_ref(b64[i], p64[i], criteria, max_output, margins=margins)
            print("%s criteria %.2f max_output %d image %d: %d detections, margins %s" % (
                dtype, criteria, max_output, i, idx.numel(), {k: "%.2e" % v for k, v in margins.items()}))
            assert R.margins_ok(margins), margins
            k = idx.numel()
            assert k >= 10, "the case detects too little to mean anything"
            assert int(counts[i]) == k
            assert list(zip(index[i, :k].tolist(), labels[i, :k].tolist())) == list(zip(idx.tolist(), lab.tolist()))
            assert bool(((boxes[i, :k].double() - b64[i][idx]).abs() <= box_bar[i][idx]).all())
            assert bool(((scores[i, :k].double() - sc).abs() <= prob_bar[i][lab, idx]).all())
            assert not bool(boxes[i, k:].any()) and not bool(labels[i, k:].any()) and not bool(scores[i, k:].any())


def test_decode_batch_is_detect_reordered_with_one_host_read(monkeypatch):
    det = get_detector(BF)
    images = get_images().to(DEV)
    boxes, labels, scores, counts = (t.cpu() for t in det.detect(images, 0.5, 200))
    reads = []
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    real_to = torch.Tensor.to

    def counted_to(self, *a, **kw):
        if self.is_cuda and any(str(x) == "cpu" for x in list(a) + list(kw.values())):
            reads.append("to")
        return real_to(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "to", counted_to)
    det.detect(images, 0.5, 200)
    assert reads == [], reads
    out = det.decode_batch(images, 0.5, 200)
    assert reads == ["cpu"], reads
    monkeypatch.undo()
    assert len(out) == 2
    for i, (bb, ll, ss) in enumerate(out):
        k = int(counts[i])
        assert tuple(bb.shape) == (k, 4) and ll.dtype == torch.int64
        assert_same(bits(bb), bits(boxes[i, :k].flip(0).contiguous()), "boxes, ascending scores")
        assert ll.tolist() == labels[i, :k].flip(0).tolist()
        assert_same(bits(ss), bits(scores[i, :k].flip(0).contiguous()), "scores, ascending")
        assert bool((ss[1:] >= ss[:-1]).all())


def test_launch_list(monkeypatch):
    """The layout pass, then 1 + 1 + 39 + 3 + 10 + 6 = 60 network launches (stem, pooling, 13 bottlenecks of 3 units, the 3
    downsample branches of layer1..layer3 -- the fourth of a ResNet-50 belongs to layer4, which SSD300 cuts --, 5 additional blocks
    of 2 units, 6 heads), then the three of the post-processing."""
    det = get_detector(BF)
    images = get_images().to(DEV)
    det.detect(images)
    names = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    det.detect(images)
    assert names[0] == "dle_nchw_to_nhwc" and names[1] == "dle_conv2d_fwd_affine" and names[2] == "dle_maxpool_fwd"
    assert names[3:61] == ["dle_conv2d_fwd_affine"] * (39 + 3 + 10 + 6)
    assert names[61:] == ["dle_ssd_decode_fwd", "dle_ssd_nms_fwd", "dle_ssd_select_fwd"]
    assert len(names) == 1 + 60 + 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_matches_eager(dtype):
    eager, graphed = get_detector(dtype), get_detector(dtype, True)
    images = get_images().to(DEV)
    other = torch.randn(tuple(images.shape), generator=torch.Generator().manual_seed(8)).to(DEV)
    want_a = [t.clone() for t in eager.detect(images, 0.5, 200, with_index=True)]
    want_b = [t.clone() for t in eager.detect(other, 0.5, 200, with_index=True)]
    for _ in range(4):                                                # two eager warm-up calls, the capture + replay, a replay
        for got, want in zip(graphed.detect(images, 0.5, 200, with_index=True), want_a):
            assert_same(bits(got.clone()), bits(want), "graph call")
    for got, want in zip(graphed.detect(other, 0.5, 200, with_index=True), want_b):
        assert_same(bits(got.clone()), bits(want), "replay with new images")
    assert all(g.graph is not None for g in graphed._graphs.values()) and len(graphed._graphs) == 1


def test_checkpoint_forms_load(tmp_path):
    model = get_model(BF)
    det = get_detector(BF)
    images = get_images().to(DEV)
    want = [t.clone() for t in det.detect(images)]
    sd = model.state_dict()
    plain, ref, mod = (str(tmp_path / n) for n in ("sd.pt", "epoch_64.pt", "module.pt"))
    torch.save(sd, plain)
    torch.save({"epoch": 65, "iteration": 1, "model": sd, "label_map": {0: "background"}}, ref)
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, mod)
    for other in (SSDDetector(sd, dtype=BF), SSDDetector.from_checkpoint(plain, dtype=BF), SSDDetector.from_checkpoint(ref, dtype=BF),
                  SSDDetector.from_checkpoint(mod, dtype=BF)):
        for got, w in zip(other.detect(images), want):
            assert_same(bits(got), bits(w), "a detector built from a checkpoint form")
    with pytest.raises(ValueError, match="16 bits"):
        SSDDetector(sd, dtype=torch.float32)


def test_main_benchmark_inference_prints_the_throughput_lines(capsys):
    assert smain.main(["--data", "unused", "--mode", "benchmark-inference", "--width", "8", "--eval-batch-size", "2", "--seed", "1",
                       "--benchmark-iterations", "2", "--benchmark-warmup", "1", "--dtype", "bf16"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Done benchmarking" in ln]
    assert len(lines) == 2 and lines[0].startswith("network:") and lines[1].startswith("network + detection:")
    for ln in lines:
        assert "Total images: 4" in ln and float(ln.split("Average images/sec: ")[1].split()[0]) > 0


def test_main_evaluation_on_a_toy_dataset(tmp_path, capsys):
    from PIL import Image
    root = tmp_path / "coco"
    (root / "val2017").mkdir(parents=True)
    (root / "annotations").mkdir()
    rng = np.random.RandomState(5)
    images, anns = [], []
    for i, (h, w) in enumerate([(240, 320), (300, 300), (128, 96)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "val2017" / ("%d.png" % i))
        images.append(dict(id=10 + i, file_name="%d.png" % i, height=h, width=w))
        anns.append(dict(image_id=10 + i, category_id=1 + i, bbox=[1, 1, 20, 20]))
    cats = [dict(id=c, name="c%d" % c) for c in range(1, 91) if c % 9][:80]
    (root / "annotations" / "instances_val2017.json").write_text(json.dumps(dict(images=images, categories=cats, annotations=anns)))
    ck, out = str(tmp_path / "ck.pt"), str(tmp_path / "det.json")
    torch.save({"model": get_model(HF).state_dict()}, ck)
    assert smain.main(["--data", str(root), "--mode", "evaluation", "--checkpoint", ck, "--eval-batch-size", "2", "--json-summary", out]) == 0
    printed = capsys.readouterr().out
    assert "Predicting Ended" in printed and ("Model precision" in printed or "pycocotools is not installed" in printed)
    rows = json.loads(open(out).read())
    ids = {c["id"] for c in cats}
    assert isinstance(rows, list)
    for r in rows:
        assert r["image_id"] in (10, 11, 12) and r["category_id"] in ids and 0.05 < r["score"] <= 1.0 and len(r["bbox"]) == 4
        assert all(np.isfinite(r["bbox"]))
