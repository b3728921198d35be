"""SSD300, host side (no GPU): the module's names and shapes, the default boxes, the float64 restatement of the post-processing
against the results recorded from the reference's own Encoder.decode_batch, the margin condition of the recorded cases, the command
line, the COCO results writer, and a self-test of the decode bar.

The margin condition.  A case's decisions (candidate or not, suppressed or not, inside the top-k or not) are demanded IDENTICAL from
every implementation only where no decision is close: the float64 run's smallest |prob - 0.05| and smallest score gap at a cut are
at least 1e-5 (absolute), its smallest |iou - criteria| at least 1e-4 of criteria -- about a thousand fp32 ulps.  It is a condition
on the INPUTS (tests/_ssd_ref.case_inputs and its seeds), asserted here.  The neighbour gaps of the final list must additionally
exceed 1e-6 (ten fp32 ulps of a probability: fp32 softmax values differ from float64 ones by a few ulps), or "the same order" would
not be a fair demand of an fp32 run.
"""
import json
import os

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.ssd import main as smain
from deeplearningexamples_amd.ssd import model as M
from tests import _ssd_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(0.45, 200), (0.5, 200), (0.45, 20), (0.5, 20)]


@pytest.fixture(scope="module")
def rec():
    return dict(np.load(os.path.join(GOLDEN, "ssd_decode.npz")))


def geometries():
    return {"full": (M.dboxes300_coco(), 81, R.FULL_SEED, True), "tiny": (M.DefaultBoxes(**R.TINY), R.TINY_LABELS, R.TINY_SEED, False)}


def test_state_dict_names_and_shapes():
    want = json.load(open(os.path.join(GOLDEN, "ssd_state_dict.json")))
    got = {k: list(v.shape) for k, v in M.SSD300().state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    blk = M.SSD300().feature_extractor.feature_extractor[6][0]
    assert blk.conv1.stride == blk.conv2.stride == blk.downsample[0].stride == (1, 1)
    assert M.SSD300().feature_extractor.feature_extractor[5][0].conv2.stride == (2, 2)


def test_width_divisor():
    m = M.SSD300(width=8)
    assert m.feature_extractor.out_channels == [128, 64, 64, 32, 32, 32]
    assert [b[0].out_channels for b in m.additional_blocks] == [32, 32, 16, 16, 16]
    # every convolution reads a multiple of 8 channels (the image aside) and every BatchNorm holds one
    assert all(p.shape[1] % 8 == 0 or p.shape[1] == 3 for p in m.parameters() if p.dim() == 4)
    assert all(b.num_features % 8 == 0 for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    loc, conf = m.eval()(torch.zeros(1, 3, 300, 300))
    assert tuple(loc.shape) == (1, 4, 8732) and tuple(conf.shape) == (1, 81, 8732)
    assert M.width_from_state(m.state_dict()) == 8


def test_other_backbones_are_turned_away():
    for name in ("resnet18", "resnet34", "resnet101", "resnet152"):
        with pytest.raises(ValueError, match="only the resnet50 backbone"):
            M.SSD300(name)


def test_default_boxes_bit_for_bit(rec):
    for name, (d, _, _, _) in geometries().items():
        for order in ("ltrb", "xywh"):
            want = rec["%s_dboxes_%s" % (name, order)]
            got = d(order).numpy()
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, order)
    assert M.dboxes300_coco().num_defaults == list(M.NUM_DEFAULTS)
    assert [M.dboxes300_coco().scale_xy, M.dboxes300_coco().scale_wh] == list(rec["scale_xy_wh"])


def test_restatement_reproduces_the_recorded_results_and_margins_hold(rec):
    for name, (d, labels, seed, big) in geometries().items():
        ploc, plabel = R.case_inputs(d("xywh").numpy(), 2, labels, seed, big)
        boxes, probs = R.decode_ref(torch.from_numpy(ploc).double(), torch.from_numpy(plabel).double(), d("xywh"))
        margins = R.new_margins()
        per_class = None
        for criteria, max_output in CASES:
            for i in range(2):
                idx, lab, sc, per_class = R.detect_ref(boxes[i], probs[i], criteria, max_output, margins=margins)
                key = "%s_c%d_m%d_i%d" % (name, round(criteria * 100), max_output, i)
                # the reference lists ascending scores
                assert np.array_equal(lab.flip(0).numpy(), rec[key + "_labels"]), key
                assert np.abs(sc.flip(0).numpy() - rec[key + "_scores"]).max() <= 1e-6, key
                assert np.abs(boxes[i][idx].flip(0).numpy() - rec[key + "_boxes"]).max() <= 1e-6, key
        print(name, {k: "%.3e" % v for k, v in margins.items()})
        assert R.margins_ok(margins), margins
        assert margins["order"] >= 1e-6, margins
        if big:      # the case is interesting: a class with more than max_num candidates, classes with none, a cut final list
            cand = (probs[0, 1:] > R.THRESHOLD).sum(1)
            assert int(cand.max()) > R.MAX_NUM and int((cand == 0).sum()) >= 1
            assert len(rec["full_c45_m200_i0_labels"]) == 200


def test_tie_rules_of_the_restatement():
    boxes = torch.tensor([[0, 0, 1, 1], [2, 2, 3, 3], [4, 4, 5, 5], [0, 0, 1, 1]], dtype=torch.float32)
    probs = torch.zeros(3, 4)
    probs[1] = torch.tensor([0.5, 0.5, 0.5, 0.5])
    probs[2] = torch.tensor([0.0, 0.5, 0.0, 0.0])
    idx, lab, sc, per = R.detect_ref(boxes, probs, 0.5, 3)
    assert per[0][1].tolist() == [0, 1, 2]                     # box 3 duplicates box 0 and loses the tie to the lower index
    assert list(zip(lab.tolist(), idx.tolist())) == [(1, 0), (1, 1), (1, 2)]      # equal scores: lower label first


def test_reference_flags_parse_and_rejections_fire(capsys):
    flags = json.load(open(os.path.join(GOLDEN, "ssd_cli_flags.json")))
    assert len(flags) >= 28
    argv = []
    for f in flags:
        value = {0: [], 1: [str(f["choices"][0]) if f["choices"] else "1"], "*": ["1", "2"]}[f["values"]]
        for spelling in f["flags"]:
            smain.make_parser().parse_args((["--data", "x"] if "--data" not in f["flags"] else []) + [spelling] + value)
        if "--no-amp" not in f["flags"] and "--no-cuda" not in f["flags"]:
            argv += [f["flags"][0]] + value
    args = smain.make_parser().parse_args(argv)
    assert args.mode == "training" and args.backbone == "resnet18" and args.evaluation == [1, 2]
    for extra, word in ((["--mode", "training"], "training is not built"), (["--mode", "benchmark-training"], "training is not built"),
                        (["--mode", "evaluation", "--backbone", "resnet101"], "only the resnet50 backbone"),
                        (["--mode", "evaluation", "--no-amp"], "16 bits")):
        assert smain.main(["--data", "x"] + extra) == 2
        out = capsys.readouterr().out.strip()
        assert word in out and len(out.splitlines()) == 1
    assert smain.reject(smain.make_parser().parse_args(["--data", "x", "--mode", "evaluation"])) is None


def test_checkpoint_forms():
    state = M.SSD300(width=8).state_dict()
    for obj in (state, {"model": state, "epoch": 3}, {"model": {"module." + k: v for k, v in state.items()}}):
        got = M.state_from_checkpoint(obj)
        assert list(got) == list(state) and all(got[k] is state[k] for k in state)
    with pytest.raises(ValueError):
        M.state_from_checkpoint([1, 2])


def test_decode_bar_admits_fp32_and_catches_faults():
    """The derived per-element bars of tests/_ssd_ref.decode_bar: an fp32 CPU model of the kernel's arithmetic stays inside; two
    deliberately faulty fp32 models do not (the location scale product rounded to bf16; one label left out of the softmax sum)."""
    d = M.DefaultBoxes(**R.TINY)
    g = torch.Generator().manual_seed(5)
    ploc = torch.randn((2, 4, 64), generator=g).to(torch.bfloat16).float()
    plabel = (3 * torch.randn((2, 5, 64), generator=g)).to(torch.bfloat16).float()
    b64, p64 = R.decode_ref(ploc.double(), plabel.double(), d("xywh"))
    box_bar, prob_bar = R.decode_bar(ploc, plabel, d("xywh"))
    b32, p32 = R.decode_ref(ploc, plabel, d("xywh"))
    assert bool(((b32.double() - b64).abs() <= box_bar).all()) and bool(((p32.double() - p64).abs() <= prob_bar).all())
    bad_loc = ploc.clone()
    bad_loc[:, :2] = ((0.1 * ploc[:, :2]).to(torch.bfloat16).float()) / 0.1
    bb, _ = R.decode_ref(bad_loc, plabel, d("xywh"))
    assert not bool(((bb.double() - b64).abs() <= box_bar).all())
    e = (plabel - plabel.max(1, keepdim=True).values).exp()
    bad_p = e / e[:, 1:].sum(1, keepdim=True)
    assert not bool(((bad_p.double() - p64).abs() <= prob_bar).all())


def test_coco_reader_and_results_writer(tmp_path):
    from PIL import Image
    root = tmp_path / "coco"
    (root / "val2017").mkdir(parents=True)
    (root / "annotations").mkdir()
    rng = np.random.RandomState(3)
    sizes = [(40, 60), (64, 48), (30, 30)]
    images = []
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "val2017" / ("%d.png" % i))
        images.append(dict(id=100 + i, file_name="%d.png" % i, height=h, width=w))
    ann = dict(images=images, categories=[dict(id=7, name="a"), dict(id=9, name="b")],
               annotations=[dict(image_id=100, category_id=7, bbox=[1, 2, 3, 4]), dict(image_id=102, category_id=9, bbox=[0, 0, 5, 5])])
    path = root / "annotations" / "instances_val2017.json"
    path.write_text(json.dumps(ann))
    coco = smain.COCODetection(str(root / "val2017"), str(path))
    assert coco.label_map == {7: 1, 9: 2} and coco.label_info == {0: "background", 1: "a", 2: "b"}
    assert coco.img_keys == [100, 102]                                     # image 101 has no annotation
    batches = list(coco.batches(8))
    assert len(batches) == 1 and tuple(batches[0][0].shape) == (2, 3, 300, 300) and batches[0][0].dtype == torch.uint8
    assert batches[0][1] == [100, 102] and batches[0][2] == [(40, 60), (30, 30)]
    decoded = [(torch.tensor([[0.1, 0.2, 0.5, 0.6]]), torch.tensor([2]), torch.tensor([0.75])),
               (torch.zeros(0, 4), torch.zeros(0, dtype=torch.long), torch.zeros(0))]
    rows = smain.results_rows(decoded, batches[0][1], batches[0][2], {v: k for k, v in coco.label_map.items()})
    assert len(rows) == 1 and rows[0][0] == 100 and rows[0][6] == 9
    assert np.allclose(rows[0][1:6], [0.1 * 60, 0.2 * 40, 0.4 * 60, 0.4 * 40, 0.75])
    out = tmp_path / "det.json"
    assert smain.write_results(rows, str(out)) == 1
    got = json.loads(out.read_text())
    assert got[0]["image_id"] == 100 and got[0]["category_id"] == 9 and len(got[0]["bbox"]) == 4 and abs(got[0]["score"] - 0.75) < 1e-6
