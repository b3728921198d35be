"""Float64 statement of the nnU-Net kernels (csrc/nnunet.hip), of the BraTS22 UNet3D forward (reference: nnunet/brats22_model.py),
of the reference's AMP arithmetic, and of the sliding-window rule.  No GPU, no product kernel, no project code: the layer walk, the
window placement and the importance maps are written out here a second time on purpose.

Kernel bars (per element, derived, never fitted):
  conv    The operand a = round16(relu?(fma(scale, x, shift))) is a correctly rounded fp32 fma followed by one rounding: reproduced
          bit for bit on the host (the float64 value of scale * x + shift is exact for the 24 + 11 bit factors of the tests,
          .float() is the fma's rounding).  acc sums K = 27 C products in fp32 in an unknown order: |acc - exact| <= (K + 2) u
          sum |w| |a|, u = 2^-24.  The stored y adds half a unit of the 16-bit type at |exact| + that bound.
  stats   (count, sum, M2) of the stored values by Welford updates and Chan merges in fp32.  With n values, m = max |y| and
          sd = sqrt(M2 / n): every update mean += d / k rounds a value bounded by m, an error of at most u m that later updates
          shrink by j / k; taken as independent and uniform (variance u^2 m^2 / 3 each, as tests/_tft_ref.py takes its roundings)
          the running mean has sigma <= u m sqrt(n) / 3, and the bar is 8 sigma plus 8 u m for the merges: bar(mean), and n
          times that for the sum.  M2 collects n products with a relative error of 4 u each and feels the running mean's error to
          first order, 2 |sum d_k delta_k| <= 2 sqrt(M2) sqrt(n) bar(mean) by Cauchy-Schwarz:
          bar(M2) = 4 (n + 8) u M2 + 2 n sd bar(mean).  There is no u n m^2 term: that is the term a sum(x^2) - n mean^2 formula
          has, and what the offset-mean test shows to be absent.
  fold    scale = gamma / sqrt(var + eps), shift = beta - mean scale from partials that are exact sums in the test (or carry the
          stats bar): first order in the bars of mean and var plus 4 u on each result.
  upsample  lambda is the correctly rounded quotient of two small integers (u relative); a lerp fma(lambda, b - a, a) of values bounded
          by m errs by u |b - a| for lambda, u |b - a| for the rounded difference and u m for the fma: 5 u m; a lerp is a convex
          combination, so the errors of its inputs pass through undiminished at most: three levels, 15 u m, stated as 16 u m,
          plus half a unit of the 16-bit type.
  head    K = C products in fp32, the bias, the weight: (C + 4) u |imp| (|b| + sum |w| |x|) per window, plus one rounding of the
          running sum per window: u |out|.
"""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as TF

U = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
FILTERS = (64, 128, 256, 512, 768, 1024, 2048)
EPS = 1e-5
TTA_FLIPS = ((), (2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4))


def to16(x, dtype):
    return x.float().to(dtype).double()


def half_ulp16(v, dtype):
    """Half the spacing of `dtype` at |v| (float64), half the subnormal spacing near 0."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype] - 1)


# ---------------------------------------------------------------------------------------------- dle_conv3d_in_fwd
def conv_operand(x, scale, shift, relu_in, dtype):
    """x [N, D, H, W, C] (16-bit values) -> the operand a as float64, bit for bit what the kernel feeds the matrix unit."""
    a = x.double()
    if scale is not None:
        a = (scale.double()[:, None, None, None, :] * a + shift.double()[:, None, None, None, :]).float()      # the fma's rounding
        if relu_in:
            a = torch.relu(a)
        a = a.to(dtype).double()
    return a


def conv3d_in(x, w, scale=None, shift=None, stride=1, relu_in=False, relu_out=True, dtype=torch.float16, pad_value_fault=False):
    """-> (exact y before the last rounding, bar of the stored y) as float64 [N, P, Q, R, Ko].  x [N, D, H, W, C], w [Ko, 3, 3, 3, C].
    pad_value_fault (the bar's self-test): normalise the padding too, as a kernel that pads in front of the norm would."""
    a = conv_operand(x, scale, shift, relu_in, dtype)
    K = 27 * a.shape[-1]
    an, wn = a.permute(0, 4, 1, 2, 3), w.double().permute(0, 4, 1, 2, 3)
    if pad_value_fault and scale is not None:
        padv = shift.double()
        padv = to16(torch.relu(padv) if relu_in else padv, dtype)
        an = TF.pad(an - padv[:, :, None, None, None], (1,) * 6) + padv[:, :, None, None, None]
        acc = TF.conv3d(an, wn, stride=stride)
        mag = TF.conv3d(an.abs(), wn.abs(), stride=stride)
    else:
        acc = TF.conv3d(an, wn, stride=stride, padding=1)
        mag = TF.conv3d(an.abs(), wn.abs(), stride=stride, padding=1)
    e = (K + 2) * U * mag
    y = torch.relu(acc) if relu_out else acc
    bar = e + half_ulp16(y.abs() + e, dtype)
    return y.permute(0, 2, 3, 4, 1).contiguous(), bar.permute(0, 2, 3, 4, 1).contiguous()


# ---------------------------------------------------------------------------------------------- statistics
def stats64(y):
    """y [N, ..., C] -> (count, sum, M2) float64 [N, C] by two passes."""
    v = y.double().reshape(y.shape[0], -1, y.shape[-1])
    n = torch.full((v.shape[0], v.shape[2]), float(v.shape[1]), dtype=torch.float64)
    s = v.sum(1)
    m2 = ((v - (s / n)[:, None, :]) ** 2).sum(1)
    return n, s, m2


def chan_merge64(part):
    """part [N, G, C, 3] -> (count, sum, M2) float64 [N, C]: Chan's formula over the bands in float64."""
    p = part.double()
    n, mean, m2 = p[:, 0, :, 0], p[:, 0, :, 1] / p[:, 0, :, 0], p[:, 0, :, 2]
    for g in range(1, p.shape[1]):
        nb, mb, m2b = p[:, g, :, 0], p[:, g, :, 1] / p[:, g, :, 0], p[:, g, :, 2]
        tot = n + nb
        d = mb - mean
        mean = mean + d * nb / tot
        m2 = m2 + m2b + d * d * n * nb / tot
        n = tot
    return n, mean * n, m2


def stats_bars(y):
    """-> (bar of sum, bar of M2) [N, C] for the statistics of y [N, ..., C]."""
    n, s, m2 = stats64(y)
    m = y.double().abs().reshape(y.shape[0], -1, y.shape[-1]).amax(1)
    mean_bar = (8 * torch.sqrt(n) / 3 + 8) * U * m
    sd = torch.sqrt(m2 / n)
    return n * mean_bar + 2.0 ** -140, 4 * (n + 8) * U * m2 + 2 * n * sd * mean_bar + 2.0 ** -140


def fold64(n, s, m2, gamma, beta, eps=EPS):
    mean, var = s / n, m2 / n
    scale = gamma.double() / torch.sqrt(var + eps)
    return scale, beta.double() - mean * scale


def fold_bars(n, s, m2, gamma, beta, sum_bar, m2_bar, eps=EPS):
    """First-order bars of (scale, shift) for partial sums within (sum_bar, m2_bar) of (s, m2), plus the fp32 evaluation: the merge
    of G bands, the division, the square root, the fma -- (G + 8) u on each, folded into 16 u with room for G <= 8."""
    mean, var = s / n, m2 / n
    scale, shift = fold64(n, s, m2, gamma, beta, eps)
    var_bar = m2_bar / n + 16 * U * var
    mean_bar = sum_bar / n + 16 * U * mean.abs()
    scale_bar = scale.abs() * (0.5 * var_bar / (var + eps) + 16 * U)
    shift_bar = mean_bar * scale.abs() + mean.abs() * scale_bar + 4 * U * (beta.double().abs() + (mean * scale).abs())
    return scale_bar, shift_bar


# ---------------------------------------------------------------------------------------------- dle_upsample3d_x2_fwd
def _axis(E):
    """Source index pair and weight of every output index of an axis of extent E (output 2 E): position i (E - 1) / (2 E - 1)."""
    i = torch.arange(2 * E, dtype=torch.int64)
    num, den = i * (E - 1), 2 * E - 1
    i0 = num // den
    lam = (num - i0 * den).double() / den
    return i0, torch.clamp(i0 + 1, max=E - 1), lam


def upsample64(x):
    """x [N, D, H, W, C] -> exact float64 [N, 2D, 2H, 2W, C] and the bar without the final rounding's half unit."""
    v = x.double()
    for ax in (1, 2, 3):
        i0, i1, lam = _axis(v.shape[ax])
        shape = [1] * 5
        shape[ax] = -1
        lam = lam.reshape(shape)
        v = v.index_select(ax, i0) * (1 - lam) + v.index_select(ax, i1) * lam
    return v


def upsample_bar(x, exact, dtype):
    m = float(x.double().abs().max())
    e = 16 * U * m
    return e + half_ulp16(exact.abs() + e, dtype)


# ---------------------------------------------------------------------------------------------- the network
def conv_order(levels):
    f = FILTERS[:levels]
    names = ["input_block.conv1", "input_block.conv2"]
    names += ["downsamples.%d" % i for i in range(levels - 2)] + ["bottleneck"] + ["upsamples.%d.conv_block" % j for j in range(levels - 1)]
    return f, names


def levels_of(sd):
    return 2 + len({k.split(".")[1] for k in sd if k.startswith("downsamples.")})


def unet3d(sd, x, mode="exact", dtype=torch.float16):
    """UNet3D.forward under eval() in float64 -> logits [N, 3, D, H, W].
    mode 'exact': nothing rounded (weights as given).
    mode 'amp': the reference's --amp arithmetic (torch.autocast): convolutions take 16-bit inputs and weights and round their
      output to 16 bits; instance_norm runs in fp32 on that (its fp32 result is kept; ReLU in fp32; the next convolution's cast
      rounds once); interpolate and cat stay in 16 bits; the output block's logits are rounded to 16 bits."""
    amp = mode == "amp"
    q = (lambda t: to16(t, dtype)) if amp else (lambda t: t)
    q32 = (lambda t: t.float().double()) if amp else (lambda t: t)
    p = lambda n: sd[n].double()
    conv = lambda t, name, stride: q(TF.conv3d(q(t), q(p(name)), stride=stride, padding=1))
    norm = lambda t, name: q32(TF.instance_norm(t, weight=p(name + ".weight"), bias=p(name + ".bias"), eps=EPS))

    def layer(t, name, stride):                     # ConvLayer: norm -> conv -> ReLU
        return torch.relu(conv(norm(t, name + ".norm"), name + ".conv.weight", stride))

    def block(t, name, stride):
        return layer(layer(t, name + ".conv1", stride), name + ".conv2", 1)

    levels = levels_of(sd)
    out = conv(x.double(), "input_block.conv1.weight", 1)
    out = torch.relu(norm(out, "input_block.norm"))
    out = torch.relu(conv(out, "input_block.conv2.weight", 1))
    enc = [out]
    for i in range(levels - 2):
        out = block(out, "downsamples.%d" % i, 2)
        enc.append(out)
    out = block(out, "bottleneck", 2)
    for j, skip in enumerate(reversed(enc)):
        up = q(TF.interpolate(out, scale_factor=2, mode="trilinear", align_corners=True))
        out = block(torch.cat((up, skip), 1), "upsamples.%d.conv_block" % j, 1)
    w = q(p("output_block.conv.weight"))
    return q(TF.conv3d(q(out), w) + p("output_block.conv.bias")[None, :, None, None, None])


# ---------------------------------------------------------------------------------------------- sliding window (the project's
# statement of MONAI's documented rule; unverified against MONAI, which cannot be run next to this project)
def windows(image, patch, overlap):
    starts = []
    for size, p in zip(image, patch):
        step = p if size == p else max(int(p * (1 - overlap)), 1)
        axis, d = [], 0
        while True:
            s = d * step
            axis.append(s - max(s + p - size, 0))
            if s + p >= size:
                break
            d += 1
        starts.append(axis)
    return list(itertools.product(*starts))


def importance(patch, blend):
    if blend == "constant":
        return torch.ones(tuple(patch), dtype=torch.float64)
    m = torch.ones((), dtype=torch.float64)
    for p in patch:
        x = torch.arange(p, dtype=torch.float64) - (p - 1) / 2
        g = torch.exp(-(x ** 2) / (2 * (0.125 * p) ** 2))
        m = m[..., None] * g
    m = m / m.max()
    m[m == 0] = m[m > 0].min()
    return m


def sliding_window(predict, volume, patch, overlap, blend):
    """volume [5, Dv, Hv, Wv] float64, predict([1, 5, *patch]) -> [1, 3, *patch]: the blended logits [3, Dv, Hv, Wv]."""
    pads = []
    for size, p in zip(volume.shape[1:], patch):
        diff = max(p - size, 0)
        pads.append((diff // 2, diff - diff // 2))
    v = TF.pad(volume, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    imp = importance(patch, blend)
    acc = torch.zeros((3,) + tuple(v.shape[1:]), dtype=torch.float64)
    tot = torch.zeros(tuple(v.shape[1:]), dtype=torch.float64)
    for d, h, w in windows(v.shape[1:], patch, overlap):
        sl = (slice(d, d + patch[0]), slice(h, h + patch[1]), slice(w, w + patch[2]))
        acc[(slice(None),) + sl] += imp * predict(v[(slice(None),) + sl][None])[0]
        tot[sl] += imp
    out = acc / tot
    D, H, W = v.shape[1:]
    return out[:, pads[0][0]:D - pads[0][1], pads[1][0]:H - pads[1][1], pads[2][0]:W - pads[2][1]]


def tta(segment, volume):
    total = 0
    for dims in TTA_FLIPS:
        ax = [d - 1 for d in dims]
        pred = segment(torch.flip(volume, ax) if ax else volume)
        total = total + (torch.flip(pred, ax) if ax else pred)
    return total / len(TTA_FLIPS)


# ---------------------------------------------------------------------------------------------- Dice (nnunet/metrics.py, brats branch)
def dice_brats(pred_logits, label):
    """pred_logits [N, 3, ...], label [N, ...] with classes 0..3 -> Dice per channel [3] in percent as compute_stats_brats counts:
    p = sigmoid > 0.5; targets whole tumour (label > 0), tumour core (label 1 or 3), enhancing (label 3); a channel without
    target scores 1 when nothing is predicted and 0 otherwise; slots as the reference fills them: (core, enhancing, whole)."""
    p = (torch.sigmoid(pred_logits.double()) > 0.5)
    y = torch.stack([label > 0, (label == 1) | (label == 3), label == 3], dim=1)
    scores = torch.zeros(3, dtype=torch.float64)
    for i in range(3):
        pi, yi = p[:, i], y[:, i]
        slot = (i - 1) % 3                          # the reference writes channel i to scores[i - 1] (metrics.py:48,53)
        if not yi.any():
            scores[slot] = 0.0 if pi.any() else 1.0
            continue
        tp = (pi & yi).sum().double()
        fn = (~pi & yi).sum().double()
        fp = (pi & ~yi).sum().double()
        scores[slot] = 2 * tp / (2 * tp + fn + fp)
    return 100 * scores


# ---------------------------------------------------------------------------------------------- seeded inputs
GEOMETRIES = {"l3": (3, (1, 5, 8, 12, 16), 11), "l2": (2, (2, 5, 4, 4, 4), 12)}          # tag -> (levels, input shape, seed)
WEIGHT_SEED = 2022


def seeded_input(shape, seed):
    """N(0, 1) values representable in fp16 (and so in fp32 and float64), as float64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(torch.float16).double()
