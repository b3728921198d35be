"""The SSD300 post-processing kernels (csrc/ssd.hip) and dle_conv2d_fwd_affine at the shapes the detector adds.  GPU only.

dle_ssd_decode_fwd.  The head tensors are built from (ploc [N,4,B], plabel [N,L,B]) by the REFERENCE's rule run backwards: the slice
of a map is reshaped to the NCHW head output [N, nd*4, H, W] / [N, nd*L, H, W] (torch.reshape, the inverse of bbox_view's) and laid
out NHWC inside the pitch, the other channels of the pitch poisoned with 1e4.  Selector inputs (one image per selector: a single
non-zero location channel, or a single hot logit) prove the channel -> (coordinate / label, anchor, box index) rule against the
formula of the header for every channel of every pixel of the tiny pyramid and for a sample of the real geometry; loc = 0 must
return the default boxes' ltrb bit for bit.  Random 16-bit inputs are checked per element against float64 under
tests/_ssd_ref.decode_bar.

dle_ssd_nms_fwd / dle_ssd_select_fwd.  fp32 boxes and probabilities go in directly; indices, order, counts, scores and boxes must
equal, bit for bit, the reference algorithm (tests/_ssd_ref.nms_ref / detect_ref, which tests/test_ssd_host.py ties to the results
recorded from the reference) run in fp32 torch on the CPU on the same arrays.

dle_conv2d_fwd_affine at 3x3 / pad 0 on 5x5 and 3x3, 3x3 / stride 2 / pad 1 on 38, 19, 10, Ko = 344 / 384 / 512 with scale 1 and
shift = bias, and the 7x7 stem at 300 x 300: float64, the bar of tests/test_gpu_rn50_infer_kernels.py.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from deeplearningexamples_amd.ssd import model as M
from tests import _ssd_ref as R
from tests._exact_grid import ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="fp16")]
DEV = "cuda"


def geometry(name):
    d = M.dboxes300_coco() if name == "full" else M.DefaultBoxes(**R.TINY)
    return d, (81 if name == "full" else R.TINY_LABELS)


def make_heads(ploc, plabel, d, pad, dtype, poison=1e4):
    """The NHWC head tensors (one per map, pitch = nd * (4 + L) rounded up to `pad`) holding ploc / plabel by the reference's reshape."""
    n, labels = ploc.shape[0], plabel.shape[1]
    heads, geom, start = [], [], 0
    for fs, nd in zip(d.feat_size, d.num_defaults):
        nb = nd * fs * fs
        loc = ploc[:, :, start:start + nb].reshape(n, 4 * nd, fs, fs)
        conf = plabel[:, :, start:start + nb].reshape(n, labels * nd, fs, fs)
        pitch = (nd * (4 + labels) + pad - 1) // pad * pad
        t = torch.full((n, fs, fs, pitch), poison, dtype=torch.float32)
        t[..., :4 * nd] = loc.permute(0, 2, 3, 1)
        t[..., 4 * nd:(4 + labels) * nd] = conf.permute(0, 2, 3, 1)
        heads.append(t.to(dtype).to(DEV).contiguous())
        geom.append((nd, 0, 4 * nd))
        start += nb
    return heads, geom


def decode(ploc, plabel, d, pad, dtype):
    heads, geom = make_heads(ploc, plabel, d, pad, dtype)
    boxes, probs = F.ssd_decode(heads, geom, d("xywh").to(DEV).contiguous(), plabel.shape[1], d.scale_xy, d.scale_wh)
    torch.cuda.synchronize()
    return boxes.cpu(), probs.cpu()


def selectors(d, labels, sample=None, seed=0):
    """One (map, channel, h, w) per image -> ploc, plabel and the (kind, coordinate / label, box index) the header's rule assigns."""
    items, start = [], 0
    for m, (fs, nd) in enumerate(zip(d.feat_size, d.num_defaults)):
        for part, nch in (("loc", 4 * nd), ("conf", labels * nd)):
            for c in range(nch):
                for h in range(fs):
                    for w in range(fs):
                        items.append((part, c // nd, start + (c % nd) * fs * fs + h * fs + w, m, c, h, w))
        start += nd * fs * fs
    if sample is not None:
        pick = torch.randperm(len(items), generator=torch.Generator().manual_seed(seed))[:sample].tolist()
        items = [items[i] for i in pick]
    heads = []
    for fs, nd in zip(d.feat_size, d.num_defaults):
        heads.append((torch.zeros(len(items), 4 * nd, fs, fs), torch.zeros(len(items), labels * nd, fs, fs)))
    for i, (part, _, _, m, c, h, w) in enumerate(items):
        heads[m][0 if part == "loc" else 1][i, c, h, w] = 2.0 if part == "loc" else 8.0
    ploc, plabel = R.bbox_view(heads, labels)
    return items, ploc, plabel


@pytest.mark.parametrize("name,sample", [("tiny", None), ("full", 12)])
def test_decode_index_rule_with_selectors(name, sample):
    d, labels = geometry(name)
    items, ploc, plabel = selectors(d, labels, sample, seed=3)
    boxes, probs = decode(ploc, plabel, d, 8, HF)
    ltrb = d("ltrb")
    b64, p64 = R.decode_ref(ploc.double(), plabel.double(), d("xywh"))
    box_bar, prob_bar = R.decode_bar(ploc, plabel, d("xywh"))
    assert bool(((boxes.double() - b64).abs() <= box_bar).all()) and bool(((probs.double() - p64).abs() <= prob_bar).all())
    uniform = 1.0 / labels
    for i, (part, which, b, *_rest) in enumerate(items):
        moved = (boxes[i] != ltrb).any(1).nonzero().flatten().tolist()
        hot = (probs[i] > 0.5).nonzero().tolist()
        if part == "loc":
            assert moved == [b], (i, part, which, b, moved)
            changed = (boxes[i, b] != ltrb[b]).nonzero().flatten().tolist()
            assert changed == ([which, which + 2] if which < 2 else [which - 2, which]), (i, which, changed)   # xy moves both edges; wh too
            assert hot == [] and abs(float(probs[i, 0, 0]) - uniform) < 1e-6
        else:
            assert moved == [] and hot == [[which, b]], (i, part, which, b, hot)


def test_decode_zero_loc_returns_the_default_boxes_exactly():
    for name in ("tiny", "full"):
        d, labels = geometry(name)
        b = d("xywh").shape[0]
        for dtype in (BF, HF):
            boxes, probs = decode(torch.zeros(1, 4, b), torch.zeros(1, labels, b), d, 8, dtype)
            assert torch.equal(boxes[0].view(torch.int32), d("ltrb").view(torch.int32))
            assert torch.equal(probs, torch.full_like(probs, float(torch.tensor(1.0) / torch.tensor(float(labels)))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,pad,n", [("tiny", 8, 3), ("tiny", 64, 3), ("full", 8, 2), ("full", 64, 2)])
def test_decode_random_inputs_per_element_bar(name, pad, n, dtype):
    d, labels = geometry(name)
    if name == "full":
        assert sorted({(nd * 85 + pad - 1) // pad * pad for nd in d.num_defaults}) == ([344, 512] if pad == 8 else [384, 512])
    b = d("xywh").shape[0]
    g = torch.Generator().manual_seed(11 + pad)
    ploc = (1.5 * torch.randn((n, 4, b), generator=g)).to(dtype).float()
    plabel = (4 * torch.randn((n, labels, b), generator=g)).to(dtype).float()
    boxes, probs = decode(ploc, plabel, d, pad, dtype)
    b64, p64 = R.decode_ref(ploc.double(), plabel.double(), d("xywh"))
    box_bar, prob_bar = R.decode_bar(ploc, plabel, d("xywh"))
    eb, ep = (boxes.double() - b64).abs(), (probs.double() - p64).abs()
    print("%s pad %d %s: boxes max err / bar %.3f, probs max err / bar %.3f" % (name, pad, dtype, float((eb / box_bar).max()), float((ep / prob_bar).max())))
    assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(probs).all())
    assert not bool((eb > box_bar).any()) and not bool((ep > prob_bar).any())


def test_decode_argument_checks():
    d, labels = geometry("tiny")
    b = d("xywh").shape[0]
    heads, geom = make_heads(torch.zeros(1, 4, b), torch.zeros(1, labels, b), d, 8, BF)
    dx = d("xywh").to(DEV).contiguous()
    with pytest.raises(ValueError):
        F.ssd_decode(heads, [(nd, 0, 4 * nd + 8) for nd, _, _ in geom], dx, labels)          # conf part past the pitch
    with pytest.raises(ValueError):
        F.ssd_decode(heads[:2], geom[:2], dx, labels)                                          # boxes of the maps != B
    with pytest.raises(ValueError):
        F.ssd_decode(heads, geom, dx, 1)                                                       # L < 2
    with pytest.raises(ValueError):
        F.ssd_decode([h.float() for h in heads], geom, dx, labels)


# ------------------------------------------------------------------------------------------------ NMS and selection
def random_case(n, labels, b, seed):
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand((n, b, 2), generator=g)
    wh = 0.05 + 0.3 * torch.rand((n, b, 2), generator=g)
    boxes = torch.cat((centre - wh / 2, centre + wh / 2), dim=2).contiguous()
    probs = 0.04 * torch.rand((n, labels, b), generator=g)
    hot = torch.rand((n, labels, b), generator=g) < 0.004
    probs[hot] = 0.05 + 0.95 * torch.rand(int(hot.sum()), generator=g)
    for i in range(n):                                   # two dense classes per image: more candidates than any max_num when b allows
        for lab in torch.randperm(labels - 1, generator=g)[:2].tolist():
            m = min(b, 300 + 40 * i)
            where = torch.randperm(b, generator=g)[:m]
            probs[i, lab + 1, where] = 0.05 + 0.95 * torch.rand(m, generator=g)
    probs[:, :, b - 1] = 0.9 * torch.rand((n, labels), generator=g) + 0.06      # a candidate at the last box index, everywhere
    return boxes, probs.contiguous()


def run_gpu(boxes, probs, criteria, max_num, max_output, threshold=R.THRESHOLD):
    bx, pr = boxes.to(DEV), probs.to(DEV)
    kept = F.ssd_nms(bx, pr, criteria=criteria, threshold=threshold, max_num=max_num)
    det = F.ssd_select(bx, *kept, max_output=max_output)
    torch.cuda.synchronize()
    return [t.cpu() for t in kept], [t.cpu() for t in det]


def check_against_reference(boxes, probs, criteria, max_num, max_output, threshold=R.THRESHOLD):
    (kept_idx, kept_score, kept_count), (det_boxes, det_label, det_score, det_idx, det_count) = run_gpu(
        boxes, probs, criteria, max_num, max_output, threshold)
    n, labels, b = probs.shape
    assert tuple(kept_idx.shape) == (n, labels - 1, max_num) and tuple(det_boxes.shape) == (n, max_output, 4)
    for i in range(n):
        idx, lab, sc, per_class = R.detect_ref(boxes[i], probs[i], criteria, max_output, threshold, max_num)
        for label, kept in per_class:
            k = kept.numel()
            what = "image %d label %d" % (i, label)
            assert int(kept_count[i, label - 1]) == k, what
            assert kept_idx[i, label - 1, :k].tolist() == kept.tolist(), what
            assert torch.equal(kept_score[i, label - 1, :k].view(torch.int32), probs[i, label][kept].view(torch.int32)), what
            assert bool((kept_idx[i, label - 1, k:] == -1).all()) and bool((kept_score[i, label - 1, k:] == 0).all()), what
        k = idx.numel()
        assert int(det_count[i]) == k
        assert det_idx[i, :k].tolist() == idx.tolist() and det_label[i, :k].tolist() == lab.tolist()
        assert torch.equal(det_score[i, :k].view(torch.int32), sc.view(torch.int32))
        assert torch.equal(det_boxes[i, :k].view(torch.int32), boxes[i][idx].view(torch.int32))
        for t in (det_boxes[i, k:], det_label[i, k:], det_score[i, k:], det_idx[i, k:]):
            assert not bool(t.view(torch.int32).any()), "rows past the count must be zero"
    return (kept_idx, kept_score, kept_count), (det_boxes, det_label, det_score, det_idx, det_count)


# every B, L, N, max_num and max_output of the grid at least once; the thresholds 200 / 201 and 256 / 257 against max_num 200 / 256
GRID = [(1, 2, 1, 1, 1), (63, 5, 3, 7, 20), (200, 5, 1, 200, 200), (201, 5, 3, 200, 20), (257, 2, 1, 256, 200), (257, 5, 3, 256, 1),
        (1000, 81, 1, 200, 200), (1000, 5, 3, 7, 200), (8732, 2, 3, 256, 200), (8732, 5, 1, 1, 20), (8732, 81, 1, 200, 200),
        (63, 81, 3, 256, 20)]


@pytest.mark.parametrize("b,labels,n,max_num,max_output", GRID)
def test_nms_and_select_bit_for_bit(b, labels, n, max_num, max_output):
    boxes, probs = random_case(n, labels, b, 100 + b + labels)
    for criteria in (0.45, 0.5):
        check_against_reference(boxes, probs, criteria, max_num, max_output)


def test_every_box_a_candidate():
    """8732 candidates in each class: the sort runs over all 16384 keys of its LDS buffer, the best 200 / 256 go on."""
    boxes, probs = random_case(1, 3, 8732, 21)
    probs[0, 1:] = 0.0501 + 0.94 * torch.rand((2, 8732), generator=torch.Generator().manual_seed(22))
    probs[0, 2, :4000] = probs[0, 2, 4000:8000]                       # and thousands of exact ties
    check_against_reference(boxes, probs, 0.5, 200, 200)
    check_against_reference(boxes, probs, 0.45, 256, 20)


def test_repeat_is_bit_identical():
    boxes, probs = random_case(2, 5, 8732, 9)
    first = run_gpu(boxes, probs, 0.5, 200, 200)
    second = run_gpu(boxes, probs, 0.5, 200, 200)
    for a, c in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def _disjoint(k):
    x = torch.arange(k, dtype=torch.float32)
    return torch.stack((x, torch.zeros(k), x + 0.5, torch.ones(k)), dim=1)


def test_constructed_cases():
    # no candidate in any class
    boxes = _disjoint(10)[None]
    probs = torch.full((1, 3, 10), 0.01)
    kept, det = check_against_reference(boxes, probs, 0.5, 7, 20)
    assert int(kept[2].sum()) == 0 and int(det[4][0]) == 0 and not bool(det[0].any())
    # exactly max_num and max_num + 1 candidates, all disjoint: all kept, the weakest cut by max_num, then by max_output
    for extra in (0, 1):
        k = 7 + extra
        boxes = _disjoint(k)[None]
        probs = torch.zeros((1, 2, k))
        probs[0, 1] = torch.linspace(0.9, 0.1, k)[torch.randperm(k, generator=torch.Generator().manual_seed(1))]
        kept, det = check_against_reference(boxes, probs, 0.5, 7, 5)
        assert int(kept[2][0, 0]) == 7 and int(det[4][0]) == 5
    # all boxes identical: one kept
    boxes = torch.tensor([0.1, 0.1, 0.6, 0.7]).repeat(1, 50, 1)
    probs = torch.zeros((1, 2, 50))
    probs[0, 1] = torch.linspace(0.2, 0.8, 50)
    kept, det = check_against_reference(boxes, probs, 0.5, 200, 200)
    assert int(kept[2][0, 0]) == 1 and kept[0][0, 0, 0] == 49
    # the chain A over B over C: B is suppressed by A, so C (which overlaps B only) is kept
    boxes = torch.tensor([[[0, 0, 1, 1], [0.4, 0, 1.4, 1], [0.8, 0, 1.8, 1]]], dtype=torch.float32)
    probs = torch.zeros((1, 2, 3))
    probs[0, 1] = torch.tensor([0.9, 0.8, 0.7])
    kept, det = check_against_reference(boxes, probs, 0.4, 200, 200)
    assert kept[0][0, 0, :2].tolist() == [0, 2] and int(kept[2][0, 0]) == 2
    # IoU exactly equal to criteria suppresses: [0,0,1,1] and [0,0,.5,1] at 0.5, exact in fp32
    boxes = torch.tensor([[[0, 0, 1, 1], [0, 0, 0.5, 1]]], dtype=torch.float32)
    probs = torch.zeros((1, 2, 2))
    probs[0, 1] = torch.tensor([0.9, 0.8])
    assert float(R.iou_ref(boxes[0, 1:], boxes[0, 0])) == 0.5
    kept, det = check_against_reference(boxes, probs, 0.5, 200, 200)
    assert int(kept[2][0, 0]) == 1
    kept, det = check_against_reference(boxes, probs, 0.5000001, 200, 200)
    assert int(kept[2][0, 0]) == 2
    # a zero-area box: against itself 0/0 (dropped from the list, kept as a candidate, as the reference does); inside another box
    # its IoU is 0 and it survives
    boxes = torch.tensor([[[0.2, 0.2, 0.2, 0.2], [0, 0, 1, 1], [0.2, 0.2, 0.2, 0.2]]], dtype=torch.float32)
    probs = torch.zeros((1, 2, 3))
    probs[0, 1] = torch.tensor([0.9, 0.8, 0.7])
    kept, det = check_against_reference(boxes, probs, 0.5, 200, 200)
    assert kept[0][0, 0, :2].tolist() == [0, 1] and int(kept[2][0, 0]) == 2       # box 2 against box 0: 0/0, suppressed
    # equal scores: the lower box index first inside a class, the lower label first in the final list
    boxes = _disjoint(6)[None]
    probs = torch.zeros((1, 3, 6))
    probs[0, 1] = 0.5
    probs[0, 2, 1] = 0.5
    kept, det = check_against_reference(boxes, probs, 0.5, 4, 5)
    assert kept[0][0, 0].tolist() == [0, 1, 2, 3] and det[1][0].tolist() == [1, 1, 1, 1, 2] and det[3][0].tolist() == [0, 1, 2, 3, 1]


def test_nms_and_select_argument_checks_without_a_launch():
    lib = C.lib()
    boxes, probs = random_case(1, 3, 16, 1)
    bx, pr = boxes.to(DEV), probs.to(DEV)
    ki = torch.zeros((1, 2, 256), dtype=torch.int32, device=DEV)
    ks = torch.zeros((1, 2, 256), device=DEV)
    kc = torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    p = C.ptr
    nms = lambda *a: lib.dle_ssd_nms_fwd(*a, C.stream())
    assert nms(p(bx), p(pr), p(ki), p(ks), p(kc), 1, 16, 3, 0.05, 0.5, 0) == -1
    assert nms(p(bx), p(pr), p(ki), p(ks), p(kc), 1, 16, 3, 0.05, 0.5, 257) == -1
    assert nms(p(bx), p(pr), p(ki), p(ks), p(kc), 1, 16, 1, 0.05, 0.5, 200) == -1
    assert nms(p(bx), p(pr), p(ki), p(ks), p(kc), 1, F.SSD_MAX_BOXES + 1, 3, 0.05, 0.5, 200) == -1
    assert nms(0, p(pr), p(ki), p(ks), p(kc), 1, 16, 3, 0.05, 0.5, 200) == -1
    assert nms(p(bx), p(pr), p(ki), p(ks), 0, 1, 16, 3, 0.05, 0.5, 200) == -1
    db = torch.zeros((1, 256, 4), device=DEV)
    dl = torch.zeros((1, 256), dtype=torch.int32, device=DEV)
    ds = torch.zeros((1, 256), device=DEV)
    sel = lambda *a: lib.dle_ssd_select_fwd(*a, C.stream())
    ok = (p(bx), p(ki), p(ks), p(kc), p(db), p(dl), p(ds), p(dl), p(kc))
    assert sel(*ok, 1, 16, 3, 0, 200) == -1 and sel(*ok, 1, 16, 3, 257, 200) == -1
    assert sel(*ok, 1, 16, 3, 200, 0) == -1 and sel(*ok, 1, 16, 3, 200, 257) == -1
    assert sel(*ok, 1, 16, 1, 200, 200) == -1
    assert sel(*ok, 1, 16, 82, 256, 256) == -1                  # 81 * 256 candidates do not fit the sort
    assert sel(0, *ok[1:], 1, 16, 3, 200, 200) == -1 and sel(*ok[:8], 0, 1, 16, 3, 200, 200) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        F.ssd_nms(bx, pr, max_num=0)
    with pytest.raises(ValueError):
        F.ssd_nms(bx, pr[:, :1].contiguous())


# ------------------------------------------------------------------------------------------------ the convolutions the model adds
def ref_conv(x, w, stride, pad):
    x, w = x.double(), w.double()
    n, h, wd, c = x.shape
    ko, r, s, _ = w.shape
    p, q = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros((n * p * q, ko), dtype=torch.float64, device=x.device)
    for i in range(r):
        for j in range(s):
            win = xp[:, i:i + stride * (p - 1) + 1:stride, j:j + stride * (q - 1) + 1:stride, :]
            y.addmm_(win.reshape(-1, c), w[:, i, j, :].t())
    return y.view(n, p, q, ko)


# name -> (N, H, W, C, Ko, R, stride, pad, scale is 1)
CONVS = {
    "pad0_5x5_128_256": (2, 5, 5, 128, 256, 3, 1, 0, False),
    "pad0_3x3_128_256": (2, 3, 3, 128, 256, 3, 1, 0, False),
    "s2_38_256_512": (1, 38, 38, 256, 512, 3, 2, 1, False),
    "s2_19_256_512": (2, 19, 19, 256, 512, 3, 2, 1, False),
    "s2_10_128_256": (2, 10, 10, 128, 256, 3, 2, 1, False),
    "head_19_512_ko344": (1, 19, 19, 512, 344, 3, 1, 1, True),
    "head_1x1_256_ko344": (2, 1, 1, 256, 344, 3, 1, 1, True),
    "width8_head_38_128_ko344": (1, 38, 38, 128, 344, 3, 1, 1, True),
    "width8_head_38_128_ko384": (2, 38, 38, 128, 384, 3, 1, 1, True),
    "head_10_512_ko512": (2, 10, 10, 512, 512, 3, 1, 1, True),
    "head_1x1_256_ko384": (2, 1, 1, 256, 384, 3, 1, 1, True),
    "stem7_300_n1": (1, 300, 300, 8, 64, 7, 2, 3, False),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CONVS))
def test_conv_affine_at_the_new_shapes(case, dtype):
    n, h, wd, c, ko, r, stride, pad, head = CONVS[case]
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, case)))
    k = r * r * c
    x = torch.randn((n, h, wd, c), generator=g, device=DEV).to(dtype)
    w = (torch.randn((ko, r, r, c), generator=g, device=DEV) / k ** 0.5).to(dtype)
    if case.startswith("stem7"):
        x[..., 3:] = 0                                  # the image's padding channels
    if head:
        scale = torch.ones(ko, device=DEV)
    else:
        scale = (0.25 + 3.75 * torch.rand((ko,), generator=g, device=DEV)) * (torch.randint(0, 2, (ko,), generator=g, device=DEV) * 2 - 1).float()
    shift = torch.randn((ko,), generator=g, device=DEV)
    relu = not head
    got = F.conv2d_fwd_affine(x, w, scale, shift, stride, pad, relu=relu).double()
    ref = scale.double() * ref_conv(x, w, stride, pad) + shift.double()
    budget = scale.double().abs() * ref_conv(x.abs(), w.abs(), stride, pad) + shift.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    assert got.shape == ref.shape
    bar = ulp16(ref, dtype) / 2 + (k + 3) * 2.0 ** -24 * budget
    err = (got - ref).abs()
    print("%s %s: max err %.3e, max err / bar %.3f" % (case, dtype, float(err.max()), float((err / bar).max())))
    assert bool(torch.isfinite(got).all())
    assert not bool((err > bar).any()), "%d of %d elements above the bar" % (int((err > bar).sum()), err.numel())
