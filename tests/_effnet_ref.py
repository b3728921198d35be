"""float64 references and DERIVED per-element bars for the EfficientNet kernels (tests/ only; CPU tensors; no conv2d and nothing
of the library): shared by tests/test_efficientnet_host.py (the bars' self-test) and tests/test_gpu_efficientnet_kernels.py.

The bars (u = 2^-24, the unit roundoff of an fp32 operation; ulp16 from tests/_exact_grid.py):
  * accumulation: a k x k fmaf chain and the BatchNorm fmaf, whatever the order: (k k + 2) u (|scale| sum |w a| + |shift|)
  * output SiLU on v: one expf within 2 ulp, an addition, a division and what the slope d silu / dv <= 1.1 carries over:
    8 u |silu(v64)| + 1.1 x (the error of v)
  * the one output rounding: ulp16(y64) / 2
  * input SiLU, rounded to 16 bits: where the float64 SiLU lies within 8 u |silu| of a rounding boundary (a NEAR-TIE) the kernel's
    fp32 SiLU may round to the other neighbour; such an input adds |scale w| ulp16(a) to the bar of exactly the outputs whose
    window holds it.  Nothing is skipped.
"""
import os
import re

import torch

from tests._exact_grid import ulp16

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_constants():
    """(T_r, T_q, C_chunk): DLE_DWCONV_TILE_ROWS / _TILE_COLS / _CHUNK of include/dle_mi355x.h."""
    src = open(os.path.join(ROOT, "include", "dle_mi355x.h")).read()
    return tuple(int(re.search(r"#define\s+DLE_DWCONV_%s\s+(\d+)" % n, src).group(1)) for n in ("TILE_ROWS", "TILE_COLS", "CHUNK"))


def tiny_model(tag):
    """tests/golden/efficientnet_tiny.npz, network `tag` ("orig" / "wide"): -> (this project's module on the CPU with the fixture's
    weights, the fixture's input [2, 3, 33, 31], the reference's float64 eval() logits)."""
    from dataclasses import replace

    import numpy as np

    from deeplearningexamples_amd.convnets import efficientnet as E
    z = np.load(os.path.join(ROOT, "tests", "golden", "efficientnet_tiny.npz"))
    arch = replace(E.ARCHS["efficientnet-b0"], widese=tag == "wide", stem_channels=int(z["stem_channels"]),
                   feature_channels=int(z["feature_channels"]), channels=tuple(int(c) for c in z["channels"]),
                   num_repeat=tuple(int(r) for r in z["num_repeat"]), default_image_size=32)
    model = E.build(arch, num_classes=int(z["num_classes"]), device="cpu")
    model.load_state_dict({k[len(tag) + 1:]: torch.from_numpy(z[k]) for k in z.files
                           if k.startswith(tag + "/") and not k.startswith(tag + "/__")})
    return model, torch.from_numpy(z[tag + "/__input"]), torch.from_numpy(z[tag + "/__logits"])


def out_hw(h, w, k, stride):
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def r16(v, dtype):
    """float64 -> the 16-bit type -> float64 (through fp32: differs from one rounding only inside a near-tie's margin)."""
    return v.float().to(dtype).double()


def silu64(v):
    return v / (1.0 + torch.exp(-v))


def near_tie(s64, dtype):
    """Where s64 lies within 8 u |s64| of the midpoint between two neighbouring values of `dtype`."""
    ulp = ulp16(s64, dtype)
    return (ulp / 2 - (s64 - r16(s64, dtype)).abs()) <= 8 * U * s64.abs()


def window_sum(a, w, k, stride):
    """sum_{r,s} w[r,s,c] a[n, p stride + r - k/2, q stride + s - k/2, c] with zero padding, by shifted slices of a padded copy.
    a [N,H,W,C], w [k,k,C], float64 -> [N,P,Q,C]."""
    n, h, wd, c = a.shape
    pad = k // 2
    p, q = out_hw(h, wd, k, stride)
    ap = torch.zeros((n, h + 2 * pad, wd + 2 * pad, c), dtype=a.dtype)
    ap[:, pad:pad + h, pad:pad + wd] = a
    acc = torch.zeros((n, p, q, c), dtype=a.dtype)
    for r in range(k):
        for s in range(k):
            acc += w[r, s] * ap[:, r:r + (p - 1) * stride + 1:stride, s:s + (q - 1) * stride + 1:stride]
    return acc


def window_terms(a, w, k, stride, n, p, q):
    """The k k products of output pixel (n, p, q), [k k, C] (a tap outside the image contributes 0)."""
    h, wd = a.shape[1:3]
    rows = []
    for r in range(k):
        for s in range(k):
            y, x = p * stride + r - k // 2, q * stride + s - k // 2
            rows.append(w[r, s] * a[n, y, x] if 0 <= y < h and 0 <= x < wd else torch.zeros_like(w[r, s]))
    return torch.stack(rows)


def dwconv_ref(x, w, scale, shift, stride, in_act, out_act):
    """x [N,H,W,C], w [k,k,C] 16-bit CPU tensors, scale / shift fp32 [C] -> dict: y64 (the unrounded float64 output), bar (per
    element, for |float(y) - y64|), a (the staged input, float64), v64, absacc (sum |w a|), ties (share of near-tie inputs)."""
    dtype, k = x.dtype, w.shape[0]
    x64, w64, sc, sh = x.double(), w.double(), scale.double(), shift.double()
    tie_bar = 0.0
    ties = 0.0
    if in_act:
        s64 = silu64(x64)
        a = r16(s64, dtype)
        near = near_tie(s64, dtype)
        ties = float(near.double().mean())
        tie_bar = sc.abs() * window_sum(near.double() * ulp16(a, dtype), w64.abs(), k, stride)
    else:
        a = x64
    acc = window_sum(a, w64, k, stride)
    absacc = window_sum(a.abs(), w64.abs(), k, stride)
    v64 = sc * acc + sh
    err_v = (k * k + 2) * U * (sc.abs() * absacc + sh.abs()) + tie_bar
    if out_act:
        y64 = silu64(v64)
        bar = ulp16(y64, dtype) / 2 + 8 * U * y64.abs() + 1.1 * err_v
    else:
        y64 = v64
        bar = ulp16(y64, dtype) / 2 + err_v
    return {"y64": y64, "bar": bar, "a": a, "v64": v64, "absacc": absacc, "ties": ties, "acc": acc}


def pool_ref(y, tr, tq):
    """Per-tile float64 sums of y [N,P,Q,C] (any float dtype), tiles of tr x tq output pixels row-major -> ([N,G,C], [N,G,C] sums of
    |y|, pixels in the largest tile)."""
    n, p, q, c = y.shape
    y64 = y.double()
    sums, mags = [], []
    for p0 in range(0, p, tr):
        for q0 in range(0, q, tq):
            t = y64[:, p0:p0 + tr, q0:q0 + tq]
            sums.append(t.sum((1, 2)))
            mags.append(t.abs().sum((1, 2)))
    return torch.stack(sums, 1), torch.stack(mags, 1), min(p, tr) * min(q, tq)


def dwconv_model_f32(x, w, scale, shift, stride, in_act, out_act, drop_tap=None, skip_input_rounding=False):
    """An fp32 CPU model of the kernel's arithmetic (not of its schedule): what the bar must admit.  drop_tap=(r, s) and
    skip_input_rounding are the two deliberate faults of the bars' self-test."""
    dtype, k = x.dtype, w.shape[0]
    a = x.float()
    if in_act:
        a = a / (1.0 + torch.exp(-a))
        if not skip_input_rounding:
            a = a.to(dtype).float()
    w32 = w.float().clone()
    if drop_tap is not None:
        w32[drop_tap] = 0
    v = scale * window_sum(a, w32, k, stride) + shift
    if out_act:
        v = v / (1.0 + torch.exp(-v))
    return v.to(dtype)


def gate_ref(pool, inv_hw, w1, b1, w2, b2, act):
    """float64 gate and the derived bar on |gate - gate64|: the fixed-order sum of G partials and the product with inv_hw
    ((G + 1) u), a C-term and an S-term fmaf chain with their biases ((C + 2) u and (S + 2) u on the sums of magnitudes), the hidden
    activation (SiLU: 8 u |h| and slope 1.1; ReLU: slope 1), all carried to the pre-sigmoid value; the sigmoid's slope <= 1/4 carries
    that to the gate, whose own expf, addition and division add 4 u."""
    p64 = pool.double()
    g = p64.shape[1]
    mean = inv_hw * p64.sum(1)
    e_mean = (g + 1) * U * inv_hw * p64.abs().sum(1)
    w1d, w2d = w1.double(), w2.double()
    c, s = w1d.shape[1], w1d.shape[0]
    z1 = mean @ w1d.t() + b1.double()
    e1 = (c + 2) * U * (mean.abs() @ w1d.abs().t() + b1.double().abs()) + e_mean @ w1d.abs().t()
    if act == "silu":
        h = silu64(z1)
        eh = 8 * U * h.abs() + 1.1 * e1
    else:
        h = torch.relu(z1)
        eh = e1
    z2 = h @ w2d.t() + b2.double()
    e2 = (s + 2) * U * (h.abs() @ w2d.abs().t() + b2.double().abs()) + eh @ w2d.abs().t()
    return torch.sigmoid(z2), e2 / 4 + 4 * U


def silu_avgpool_ref(x):
    """x [N,HW,C] 16-bit -> (mean64 of the ROUNDED SiLU values, the bar on |float(y) - mean64|, share of near-tie inputs)."""
    dtype = x.dtype
    hw = x.shape[1]
    s64 = silu64(x.double())
    a = r16(s64, dtype)
    near = near_tie(s64, dtype)
    mean = a.sum(1) / hw
    bar = ulp16(mean, dtype) / 2 + (hw + 2) * U * a.abs().sum(1) / hw + (near.double() * ulp16(a, dtype)).sum(1) / hw
    return mean, bar, float(near.double().mean())
