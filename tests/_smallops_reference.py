"""float64 statements, input builders and derived per-element bars for the small HBM-bound kernels of csrc/convnet.hip (layout,
max / average pooling, softmax cross entropy) and csrc/elementwise.hip (casts, BCE, GradScaler bookkeeping, ReLU / activation
backward, axpby, transpose).  tests/ only: no GPU and no ctypes in here.

Every statement takes the 16-bit, fp32 or u8 inputs exactly as the kernel sees them, widens them to float64 and returns the value
and a bar for every output element; the pass condition is ratio(got, ref, bar) = |got - ref| / bar <= 1 on EVERY element (a bar
of 0 demands equality, a non-finite reference demands the same non-finite class).  u = 2^-24 is one fp32 rounding, ulp16(v) the
spacing of the 16-bit output type at v: an output stored in 16 bits adds ulp16 / 2 at the far end of its fp32 bar (stored()).
Outputs that are copies, casts, maxima or flags have NO bar: they are compared as integers with the CPU's own result.

__expf(a) is exp2(a * log2(e)): the product's rounding moves the base-2 exponent by |a| log2(e) u, a relative |a| u on the result;
the fp32 constant log2(e) is off by 0.22 u (another 0.25 |a| u); where a = x - max was itself rounded, one more |a| u.  With the
hardware exp2's own relative error C_EXP u:   rel(__expf(x - max)) <= E(d) = (2.25 d + C_EXP) u,  d = |x - max|.
__logf(s) is log2(s) * ln 2: (C_LOG + 1.25) u relative on ln s next to the error s brings.  rcp: C_RCP u relative.

C_EXP, C_LOG, C_RCP are the only numbers here that are measured and not derived (the kernel guides carry no accuracy statement
for v_exp_f32 / v_log_f32 / v_rcp_f32).  They were set from one run of tests/test_gpu_smallops_reference.py on an MI355X, against
these float64 statements only, starting from 2 u each (the one-ulp figure usually quoted for these instructions); the rule is that
the largest recorded ratio of what they enter is at most 0.5.  With 2 u that run recorded (the full table is in the GPU test's
docstring):
    C_LOG   xent loss 0.083 (narrow), 0.076 (wide)                                            kept at 2
    C_RCP   act_bwd gelu, the fp32 part of the bar (the store's half ulp taken off) 0.297       kept at 2 by that run; now 3:
            the run of tests/test_gpu_tacotron2_reference.py on an MI355X recorded, on the elements of the LSTM cell state whose bar
            is at least half C_EXP / C_RCP (fast_tanh near 0, where its error is the absolute (C_EXP / 2 + 1 + C_RCP) u and the
            reciprocal has the largest share), 0.505 (fp16) and 0.493 (bf16) with 2 u; 3 u is the smallest integer that brings them
            to 0.5 or below: 0.410 and 0.400 (C_EXP = 3 instead: 0.450 and 0.439).  The figures in this module's and in the smallops
            tests' docstrings were recorded with C_RCP = 2 u; the constant enters fast_tanh_delta only, i.e. the fp32 part of act_bwd gelu.
    C_EXP   BCE loss 0.093, BCE fp32 gradient 0.420, act_bwd gelu 0.297, xent loss as above   kept at 2
            xent fp32 gradient 0.563 (narrow), 0.532 (wide): above 0.5, but not through C_EXP -- the largest ratios sit at
            elements with p << s / classes, where g = -(s / classes) gs and the bar is 4 u |g| of plain roundings; the fp32
            evaluation on the CPU, with a correctly rounded exp, reaches the same 0.563, and C_EXP = 4 moves it to 0.562.  On the
            elements where the exponential makes up at least half of the bar (grad_exp_share) the ratio is the figure the rule
            applies to; the GPU test records it as "xent ... grad fp32, exp-dominated" (CPU: 0.367 narrow, 0.329 wide).

Targets outside [0, classes) other than ignore_index are not validated by softmax_xent (nor by the reference project's loss):
they would read out of bounds and are not part of any case here.
"""
import numpy as np
import torch

F64, F32, F16, BF16, U8 = torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.uint8
U = 2.0 ** -24
C_EXP, C_LOG, C_RCP = 2.0, 2.0, 3.0
TINY = 2.0 ** -126                  # below it fp32 errors are absolute (subnormal spacing, or a flush to zero)
MANT = {F16: 10, BF16: 7, F32: 23}
EMIN = {F16: -14, BF16: -126, F32: -126}
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16", U8: "u8"}
GELU_K0, GELU_K1 = 0.7978845608028654, 0.044715


def name(dtype):
    return NAME[dtype]


def f32(x):
    """A host scalar as a C `float` parameter carries it."""
    return float(np.float32(x))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def widen(t):
    return t.detach().cpu().to(F64)


def ulp(v, dtype):
    """Spacing of `dtype` at |v| (float64), the subnormal spacing at and near 0."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype])


def stored(v, e, dtype):
    """bar of a value whose fp32 evaluation is within `e` once it is stored in `dtype`"""
    if dtype == F32:
        return e
    return e + 0.5 * ulp(v.abs() + e, dtype)


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def ratio(got, ref, bar):
    """|got - ref| / bar per element; bar 0 demands equality; a non-finite reference demands the same value (NaN for NaN)."""
    got, ref, bar = widen(got), ref.to(F64), bar.to(F64).expand_as(ref)
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    err = (got - ref).abs()
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.full_like(err, float("inf")))
    r = torch.where(torch.isfinite(ref) & torch.isfinite(got), r, torch.full_like(err, float("inf")))
    return torch.where(same, torch.zeros_like(err), r)


def worst(got, ref, bar):
    """-> (largest ratio, flat index of it); no element is left out"""
    r = ratio(got, ref, bar).reshape(-1)
    if r.numel() == 0:
        return 0.0, -1
    i = int(torch.argmax(torch.nan_to_num(r, nan=float("inf"))))
    return float(r[i]), i


def same_cast(got, want):
    """bit equality of two tensors of one dtype, except that any NaN matches any NaN (payloads are not part of the contract)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = torch.isnan(want.float())
    return bool(torch.equal(torch.isnan(got.float()), nan)) and bool(torch.equal(bits(got)[~nan], bits(want)[~nan]))


# ---------------------------------------------------------------------------------------------- casts and layout (exact)
def special_values(dtype):
    """+-0, subnormals, the fp16 limits and the tie to inf, fp32 max, +-inf, NaN, bf16 exact ties; as `dtype` holds them"""
    v = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -15, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0,
         65536.0, 3.4028234663852886e38, -3.4028234663852886e38, 3.3e38, float("inf"), -float("inf"), float("nan"),
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
         2.0 ** -126, 2.0 ** -130, 2.0 ** -149, 1e-40, 0.1, -0.3, 1.0, 6.1e-5, 5.96e-8, 2.98e-8, 2.9802325e-8]
    return torch.tensor(v, dtype=F32).to(dtype)


def cast_input(n, dtype, seed):
    """n values: the specials first (as many as fit), then N(0, 1) * 2^k over the fp16 range"""
    g = gen(seed)
    x = (torch.randn(n, generator=g) * torch.pow(2.0, torch.randint(-20, 17, (n,), generator=g).float())).to(dtype)
    s = special_values(dtype)
    m = min(n, s.numel())
    x[:m] = s[:m]
    return x


def ref_cast(x, dtype, cols_out=None):
    """torch.Tensor.to(dtype) on the CPU (round to nearest even, overflow to inf), padded columns zero"""
    y = x.cpu().to(dtype)
    if cols_out is not None and cols_out > x.shape[1]:
        y = torch.cat([y, torch.zeros(x.shape[0], cols_out - x.shape[1], dtype=dtype)], 1)
    return y


def truncating_cast(x, dtype):
    """MUTANT: chop the low bits instead of rounding (fp32 -> 16 bit)"""
    b = x.float().contiguous().view(torch.int32)
    if dtype == BF16:
        return (b >> 16).to(torch.int16).view(BF16)
    return ((b & ~0x1FFF).view(F32)).to(F16)      # 13 dropped bits of a normal fp16


def ref_nchw_to_nhwc(x, dtype, cp):
    n, c, h, w = x.shape
    y = torch.zeros(n, h, w, cp, dtype=dtype)
    y[..., :c] = x.cpu().to(dtype).permute(0, 2, 3, 1)
    return y


def ref_u8_normalize(x, mean, std, dtype, cp):
    """(x - mean[c]) / std[c]: one fp32 subtract (u |x - mean|, a relative u of the quotient), one correctly rounded divide (u),
    one store: bar = ulp16 / 2 + 4 u |ref| as the issue states it (2 u would do; the u8 -> fp32 convert is exact).  Padding
    channels are zero with bar 0."""
    n, c, h, w = x.shape
    v = (widen(x) - widen(mean).view(1, c, 1, 1)) / widen(std).view(1, c, 1, 1)
    ref = torch.zeros(n, h, w, cp, dtype=F64)
    ref[..., :c] = v.permute(0, 2, 3, 1)
    bar = stored(ref, 4 * U * ref.abs(), dtype)
    bar[..., c:] = 0
    return ref, bar


def ref_relu_bwd(g, y):
    """g's bits where y > 0, +0 elsewhere (y = 0, -0, negative or NaN)"""
    return torch.where(y.cpu().float() > 0, bits(g.cpu()), torch.zeros((), dtype=torch.int16)).view(g.dtype)


# ---------------------------------------------------------------------------------------------- max pooling
def pool_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def maxpool_route(h, w, k, s, p):
    """the kernel dle_maxpool_bwd launches, from its conditions (below 2^31 items)"""
    if (k, s, p) == (3, 2, 1) and h % 2 == 0 and w % 2 == 0:
        return "patch"
    if (k, s, p) == (3, 2, 1) and pool_out(h, k, s, p) >= 1 and pool_out(w, k, s, p) >= 1:
        return "k3s2"
    return "generic"


def maxpool_input(shape, dtype, seed, plant=True):
    """NHWC after ReLU (exact ties at 0); planted: a NaN, two NaNs in one window, +inf, a block of -inf (whole windows, one at
    the border), an all-equal block."""
    n, h, w, c = shape
    x = torch.relu(torch.randn(shape, generator=gen(seed))).to(dtype)
    if plant and h * w >= 4:
        x[0, :min(h, 5), :min(w, 5), 0] = -float("inf")          # whole windows of -inf, the corner one among them
        x[0, h - 1, w - 1, 1 % c] = float("nan")
        x[n - 1, 0, 0, 2 % c] = float("nan")
        x[n - 1, min(1, h - 1), min(1, w - 1), 2 % c] = float("nan")
        x[n - 1, h // 2, w // 2, 3 % c] = float("inf")
        x[n - 1, :, :, 4 % c] = 0.75                               # all-equal windows
        x[n - 1, :, :, 5 % c] = -float("inf")                     # every window all -inf
    return x


def ref_maxpool_fwd(x, k, s, p, last_on_ties=False, work=F64):
    """x NHWC -> (max [N, P, Q, C] in `work` precision -- a maximum of 16-bit values is exact in any of them --, uint8 code r * k + s).
    The window is scanned r-major; a tap replaces the best when `f > best || f != f` (a NaN wins, the last NaN's index is
    recorded: the kernel's rule and ATen's) and the scan starts from the first tap INSIDE the image (ATen: maxindex = the window's
    first pixel, maxval = -inf), which is what a window of -inf answers.  last_on_ties: MUTANT (>=)."""
    n, h, w, c = x.shape
    P, Q = pool_out(h, k, s, p), pool_out(w, k, s, p)
    xp = torch.full((n, h + 2 * p + s, w + 2 * p + s, c), -float("inf"), dtype=work)
    xp[:, p:p + h, p:p + w] = x.to(work)
    inside = torch.zeros(h + 2 * p + s, w + 2 * p + s, dtype=torch.bool)
    inside[p:p + h, p:p + w] = True
    best = torch.full((n, P, Q, c), -float("inf"), dtype=work)
    code = torch.zeros((n, P, Q, c), dtype=torch.uint8)
    seen = torch.zeros((1, P, Q, 1), dtype=torch.bool)
    for r in range(k):
        for t in range(k):
            f = xp[:, r:r + s * P:s, t:t + s * Q:s][:, :P, :Q]
            ok = inside[r:r + s * P:s, t:t + s * Q:s][:P, :Q].view(1, P, Q, 1)
            upd = ((f >= best) if last_on_ties else (f > best)) | (f != f) | ~seen
            upd = upd & ok
            best = torch.where(upd, f, best)
            code = torch.where(upd, torch.full_like(code, r * k + t), code)
            seen = seen | ok
    return best, code


def ref_maxpool_bwd(dy, code, hw, k, s, p, drop_tap2=False, work=F64):
    """dx[pixel] = sum of dy over the (at most ceil(k / s)^2) windows whose code names the pixel -> (ref, sum|terms|); maxpool_bwd_bar() makes the bar.  The kernels add the
    terms in fp32 starting from 0 (the first add is exact, each later one rounds) and store 16 bits:
    bar = ulp16 / 2 + 3 u sum|terms| (at most 4 terms at the geometries used: 3 roundings).  drop_tap2: MUTANT (an odd coordinate's
    tap-2 window is forgotten)."""
    n, P, Q, c = dy.shape
    h, w = hw
    dxp = torch.zeros(n, h + 2 * p + s * 2 + k, w + 2 * p + s * 2 + k, c, dtype=work)
    mag = torch.zeros_like(dxp)
    g = dy.to(work)
    for r in range(k):
        for t in range(k):
            if drop_tap2 and (r == 2 or t == 2):
                continue
            m = (code == r * k + t).to(work)
            dxp[:, r:r + s * P:s, t:t + s * Q:s][:, :P, :Q] += g * m
            mag[:, r:r + s * P:s, t:t + s * Q:s][:, :P, :Q] += g.abs() * m
    ref, mag = dxp[:, p:p + h, p:p + w].contiguous(), mag[:, p:p + h, p:p + w].contiguous()
    return ref, mag


def maxpool_bwd_bar(ref, mag, dtype):
    return stored(ref.double(), 3 * U * mag.double(), dtype)


# ---------------------------------------------------------------------------------------------- average pooling
def ref_avgpool_fwd(x, plus_one=False):
    """x [N, HW, C] 16-bit.  The kernel: a serial fp32 sum of HW terms from 0 (HW - 1 roundings), times fp32(1 / HW) (u) with one
    product rounding (u): bar = ulp16 / 2 + (HW + 2) u sum|x| / HW.  plus_one: MUTANT (divides by HW + 1)."""
    hw = x.shape[1]
    xd = widen(x)
    ref = xd.sum(1) / (hw + 1 if plus_one else hw)
    return ref, stored(ref, (hw + 2) * U * xd.abs().sum(1) / hw, x.dtype)


def ref_avgpool_bwd(dy, hw):
    """dy [N, C] -> dx [N, HW, C] = dy / HW: fp32(1 / HW) and one product, bar = ulp16 / 2 + 2 u |ref|"""
    ref = (widen(dy) / hw).unsqueeze(1).expand(dy.shape[0], hw, dy.shape[1]).contiguous()
    return ref, stored(ref, 2 * U * ref.abs(), dy.dtype)


# ---------------------------------------------------------------------------------------------- axpby
def ref_axpby(x, y, a, b):
    """a x + b y in fp32: two products and a sum (or a product and a fused multiply-add), bar = 3 u (|a x| + |b y|).  b == 0: y is
    not read and the result is the rounded product a x."""
    a, b = f32(a), f32(b)
    ax = a * widen(x)
    by = b * widen(y) if b != 0.0 else torch.zeros_like(ax)
    return ax + by, 3 * U * (ax.abs() + by.abs())


# ---------------------------------------------------------------------------------------------- softmax cross entropy
XENT_OLD_BARS = {"narrow": (1e-5, 1e-4, 1e-7), "wide": (2e-5, 1e-4, 1e-6)}      # loss rel, gradient rtol / atol of the older tests


def xent_route(classes, ld, ld_out=None, logits_offset_bytes=0, has_grad=True):
    wide = classes >= 4096 and ld % 4 == 0 and logits_offset_bytes % 16 == 0
    if has_grad:
        wide = wide and (ld_out if ld_out is not None else classes) % 4 == 0
    return "wide" if wide else "narrow"


def xent_input(rows, classes, seed, ignore_index=-100, ignored="some"):
    """N(0, 2) logits; the first rows carry a +60 logit late in the row (never the target: the target's gradient would otherwise
    be the cancellation 1 - p of two numbers one fp32 step apart) and shifts of +80 / -80; targets in [0, classes)."""
    g = gen(seed)
    x = torch.randn(rows, classes, generator=g) * 2.0
    t = torch.randint(0, classes, (rows,), generator=g)
    x[0, classes - 1] = 60.0
    t[0] = 0
    if rows > 2:
        x[1] += 80.0
        x[2] -= 80.0
    if ignored == "some" and rows > 3:
        drop = torch.rand(rows, generator=g) < 0.3
        drop[:3] = False                     # the +60 row and the two shifted rows stay valid in every case
        t[drop] = ignore_index
        t[3] = ignore_index
    elif ignored == "all":
        t[:] = ignore_index
    return x.float(), t


def _exp_rel(d):
    return (2.25 * d + C_EXP) * U


def ref_softmax_xent(logits, target, smoothing, ignore_index, grad_scale, grad_dtype, route, ld_out=None, mutant=None):
    """-> dict(loss, loss_bar, grad, grad_bar) for logits fp32 [rows, classes] (the statement above softmax_xent_kernel):
        loss_row = (1 - s) (lse - x[t]) + s (lse - mean x), loss = sum over valid rows / n_valid,
        grad     = (softmax - (1 - s) onehot(t) - s / classes) grad_scale / n_valid, 0 in ignored rows and padded columns.
    sum of exponentials se = sum e_i, e_i = exp(x_i - max), all terms positive:
      narrow (wave per row): each lane adds L = ceil(classes / 64) terms serially, then a 6-level butterfly:
          |d se| <= sum e_i E(d_i) + (L + 5) u se
      wide (workgroup per row): a thread meets T = ceil(ceil(classes / 4) / 256) groups of 4; every group costs a rescale
          se *= exp(m - m') (E(m' - m) + u; the distances telescope to d_i = max - x_i, the constants add up T times) and 4 adds;
          then the wave rescale, the butterfly (6), the 4-wave rescale and fold (4):
          |d se| <= sum e_i (2.25 d_i + (T + 3) C_EXP) u + (5 T + 12) u se
    lse = max + ln se: |d lse| <= |d se| / se + (C_LOG + 1.25) u ln se + u |lse|.
    sum of logits sx: the same chains without exponentials, (L + 5) u sum|x| resp. (4 T + 10) u sum|x|; / classes: u.
    row loss: u |nll| + s [d(sx) / classes + u |mean x| + u |smooth|] + 3 u (|(1 - s) nll| + |s smooth|) next to d lse (s = 0: the
    products by 1 and 0 are exact, the bound stays).  loss: one atomic add per valid row in ARBITRARY order, every partial sum is
    at most sum|loss_row|: (n_valid - 1) u sum|loss_row|, then the division (u).  At 256 rows that worst case (1.5e-5) is above
    the older tests' relative bar, which therefore stays as a ceiling: loss_bar = min(derived, XENT_OLD_BARS[route][0] |loss|).
    gradient: p = e_i / se carries E(d_i) + |d se| / se + 2 u (reciprocal, product); 1 - s, s / classes and grad_scale / n_valid one
    u each; two subtractions and the final product:
      |d g| <= [p rel(p) + u (1 - s) onehot + u s / classes + u |p - oh| + u |p - oh - sm|] |gs| + 2 u |g| + 2^-126 (1 + |gs|),
      + ulp16 / 2 when stored in 16 bits (2^-126: an exponential below the smallest normal fp32 has an absolute error).
    mutant: 'no_smoothing_term' (gradient without s / classes), 'rows_norm' (loss divided by rows)."""
    x = widen(logits)
    rows, classes = x.shape
    s = f32(smoothing)
    valid = target != ignore_index
    nv = max(int(valid.sum()), 1)
    mx = x.max(1, keepdim=True).values
    d = mx - x
    e = torch.exp(-d)
    se = e.sum(1, keepdim=True)
    if route == "narrow":
        L = -(-classes // 64)
        dse = (e * _exp_rel(d)).sum(1, keepdim=True) + (L + 5) * U * se
        dsx = (L + 5) * U * x.abs().sum(1)
    else:
        T = -(-(-(-classes // 4)) // 256)
        dse = (e * (2.25 * d + (T + 3) * C_EXP) * U).sum(1, keepdim=True) + (5 * T + 12) * U * se
        dsx = (4 * T + 10) * U * x.abs().sum(1)
    lse = (mx + torch.log(se)).squeeze(1)
    dlse = (dse / se).squeeze(1) + (C_LOG + 1.25) * U * torch.log(se).squeeze(1) + U * lse.abs()
    tt = torch.where(valid, target, torch.zeros_like(target))
    nll = lse - x.gather(1, tt.view(-1, 1)).squeeze(1)
    meanx = x.sum(1) / classes
    smooth = lse - meanx
    row = (1 - s) * nll + s * smooth
    drow = dlse + U * nll.abs() + s * (dsx / classes + U * meanx.abs() + U * smooth.abs()) + 3 * U * (((1 - s) * nll).abs() + (s * smooth).abs())
    row, drow = row * valid, drow * valid
    loss = row.sum() / (rows if mutant == "rows_norm" else nv)
    n_add = max(int(valid.sum()) - 1, 0)
    loss_bar = (drow.sum() + n_add * U * row.abs().sum()) / nv + U * loss.abs()
    loss_bar = torch.minimum(loss_bar, XENT_OLD_BARS[route][0] * loss.abs())
    out = {"loss": loss.view(1), "loss_bar": loss_bar.view(1), "grad": None, "grad_bar": None, "n_valid": int(valid.sum())}
    if grad_dtype is None:
        return out
    scale = 1.0 if grad_scale is None else f32(grad_scale)
    gs = (valid.to(F64) * scale / nv).view(-1, 1)
    p = e / se
    relp = _exp_rel(d) + dse / se + 2 * U
    oh = torch.zeros_like(x)
    oh[torch.arange(rows), tt] = 1.0
    oh = oh * (1 - s)
    sm = s / classes
    core = p - oh - (0.0 if mutant == "no_smoothing_term" else sm)
    g = core * gs
    dg = (p * relp + U * oh + U * sm + U * (p - oh).abs() + U * core.abs()) * gs.abs() + 2 * U * g.abs() + TINY * (1 + gs.abs()) * (gs != 0)
    ldo = ld_out or classes
    ref, bar = torch.zeros(rows, ldo, dtype=F64), torch.zeros(rows, ldo, dtype=F64)
    ref[:, :classes], bar[:, :classes] = g, stored(g, dg, grad_dtype)
    bar[~valid] = 0          # ignored rows: exactly zero
    share = torch.zeros(rows, ldo, dtype=F64)      # the exponential's part of the fp32 bar: where it is large, C_EXP is what is measured
    share[:, :classes] = p * _exp_rel(d) * gs.abs() / dg.clamp_min(1e-300)
    out["grad"], out["grad_bar"], out["grad_exp_share"] = ref, bar, share
    return out


def f32_softmax_xent(logits, target, smoothing, ignore_index, grad_scale, route):
    """The kernels' statement evaluated in fp32 in their order (torch.exp / torch.log in fp32 stand for __expf / __logf) ->
    (loss fp32 [1], grad fp32 [rows, classes])."""
    x = logits.float()
    rows, classes = x.shape
    s = np.float32(smoothing)
    valid = target != ignore_index
    nv = np.float32(max(int(valid.sum()), 1))
    if route == "narrow":
        L = -(-classes // 64)
        xp = torch.full((rows, L * 64), -float("inf"))
        xp[:, :classes] = x
        xp = xp.view(rows, L, 64)
        mx = xp.max(1).values.max(1, keepdim=True).values
        se, sx = torch.zeros(rows, 64), torch.zeros(rows, 64)
        for i in range(L):
            ok = torch.isfinite(xp[:, i]) | (xp[:, i] > 0)
            se = se + torch.where(ok, torch.exp(xp[:, i] - mx), torch.zeros(()))
            sx = sx + torch.where(ok, xp[:, i], torch.zeros(()))
        for o in (32, 16, 8, 4, 2, 1):
            se, sx = se[:, :o] + se[:, o:2 * o], sx[:, :o] + sx[:, o:2 * o]
        tot, totx = se, sx
    else:
        n4 = -(-classes // 4)
        T = -(-n4 // 256)
        xp = torch.full((rows, T * 1024), -float("inf"))
        xp[:, :classes] = x
        xp = xp.view(rows, T, 256, 4)
        m = torch.full((rows, 256), -float("inf"))
        se, sx = torch.zeros(rows, 256), torch.zeros(rows, 256)
        for i in range(T):
            v = xp[:, i]
            has = torch.isfinite(v[..., 0])
            m2 = torch.maximum(m, v.max(2).values)
            se2 = se * torch.where(torch.isfinite(m), torch.exp(m - m2), torch.zeros(()))
            sx2 = sx
            for k in range(4):
                se2 = se2 + torch.exp(v[..., k] - m2)
                sx2 = sx2 + torch.where(torch.isfinite(v[..., k]), v[..., k], torch.zeros(()))
            m, se, sx = torch.where(has, m2, m), torch.where(has, se2, se), torch.where(has, sx2, sx)
        m, se, sx = m.view(rows, 4, 64), se.view(rows, 4, 64), sx.view(rows, 4, 64)
        wm = m.max(2, keepdim=True).values
        se = se * torch.exp(m - wm)
        for o in (32, 16, 8, 4, 2, 1):
            se, sx = se[..., :o] + se[..., o:2 * o], sx[..., :o] + sx[..., o:2 * o]
        mx = wm.max(1).values
        tot, totx = torch.zeros(rows, 1), torch.zeros(rows, 1)
        for q in range(4):
            tot = tot + se[:, q] * torch.exp(wm[:, q] - mx)
            totx = totx + sx[:, q]
    lse = (mx + torch.log(tot)).squeeze(1)
    tt = torch.where(valid, target, torch.zeros_like(target))
    nll = lse - x.gather(1, tt.view(-1, 1)).squeeze(1)
    smooth = lse - totx.squeeze(1) / np.float32(classes)
    row = (np.float32(1) - s) * nll + s * smooth
    loss = torch.zeros(())
    for r in range(rows):
        if bool(valid[r]):
            loss = loss + row[r]
    loss = loss / nv
    scale = np.float32(1.0 if grad_scale is None else grad_scale)
    gs = (valid.float() * float(scale / nv)).view(-1, 1)
    oh = torch.zeros_like(x)
    oh[torch.arange(rows), tt] = float(np.float32(1) - s)
    g = (torch.exp(x - mx) * (1.0 / tot) - oh - float(s / np.float32(classes))) * gs
    return loss.view(1), g


# ---------------------------------------------------------------------------------------------- BCE with logits
BCE_EDGE_X = [0.0, 8.0, -8.0, 20.0, -20.0, 88.0, -88.0]


def bce_input(n, dtype, seed):
    """N(0, 3) logits with the edge values in front (each against labels 0, 1 and 0.3); labels 0 / 1 / soft 0.3 in thirds"""
    g = gen(seed)
    x = torch.randn(n, generator=g) * 3.0
    y = torch.randint(0, 3, (n,), generator=g).float() * 0.5
    y = torch.where(y == 0.5, torch.full_like(y, 0.3), y)
    ex = torch.tensor([v for v in BCE_EDGE_X for _ in range(3)])
    ey = torch.tensor([0.0, 1.0, 0.3] * len(BCE_EDGE_X))
    m = min(n, ex.numel())
    x[:m], y[:m] = ex[:m], ey[:m]
    return x.to(dtype), y.float()


def bce_grid(n):
    return max(1, min(2048, -(-n // 1024)))


def ref_bce(logits, target, grad_scale, mutant=None):
    """loss = mean(max(x, 0) - x y + log1p(exp(-|x|))), grad = (sigmoid(x) - y) grad_scale / n (stored in the logits' type).
    e = __expf(-|x|): E(|x|).  log1pf(e): the library's, 2 ulp (4 u) next to e E / (1 + e).  x y: u; the two additions: u each:
      |d l_i| <= e E / (1 + e) + 4 u log1p(e) + u |x y| + u |max(x, 0) - x y| + u |l_i|
    sum: a thread adds its T = ceil(n / (256 grid)) terms serially, the butterfly (6), the 4-wave fold (4), the division by n (u),
    one atomic per workgroup in ARBITRARY order (grid - 1 roundings of partial sums below the total, the terms being >= 0):
      loss_bar = sum|d l_i| / n + (T + 11 + grid) u loss         -- holds for any order.
    gradient, written (1 - y) S - y Cc with S, Cc the two quotients 1 / (1 + e), e / (1 + e) chosen by the sign of x: each carries
    E + 2 u (the sum 1 + e and the division); 1 - y: u; two products, the difference, grad_scale / n (u) and the last product:
      |d g| <= [(|1 - y| S + |y| Cc) (E + 4 u) + u |(1 - y) S - y Cc|] gs + 2 u |g| + 2^-126 (1 + gs), + ulp16 / 2 in 16 bits
    (2^-126: at |x| = 88 e is below the smallest normal fp32, where an error is absolute -- rounded at the subnormal spacing or flushed).
    mutant 'naive_minus_one': 1 / (1 + e) - 1 evaluated in fp32 for y = 1, x >= 0 (what the kernel's comment warns of)."""
    x, y = widen(logits), widen(target)
    n = x.numel()
    ax = x.abs()
    e = torch.exp(-ax)
    E = _exp_rel(ax)
    l1p = torch.log1p(e)
    li = x.clamp_min(0) - x * y + l1p
    dli = e * E / (1 + e) + 4 * U * l1p + U * (x * y).abs() + U * (x.clamp_min(0) - x * y).abs() + U * li.abs()
    loss = li.sum() / n
    grid = bce_grid(n)
    T = -(-n // (256 * grid))
    loss_bar = dli.sum() / n + (T + 11 + grid) * U * loss.abs()
    gs = (1.0 if grad_scale is None else f32(grad_scale)) / n
    p, q = 1 / (1 + e), e / (1 + e)
    S, Cc = torch.where(x >= 0, p, q), torch.where(x >= 0, q, p)
    core = (1 - y) * S - y * Cc
    if mutant == "naive_minus_one":
        naive = ((1.0 / (1.0 + e.float())) - 1.0).double()
        core = torch.where((y == 1) & (x >= 0), naive, core)
    g = core * gs
    dg = (((1 - y).abs() * S + y.abs() * Cc) * (E + 4 * U) + U * core.abs()) * gs + 2 * U * g.abs() + TINY * (1 + gs)
    return {"loss": loss.view(1), "loss_bar": loss_bar.view(1), "grad": g, "grad_bar": stored(g, dg, logits.dtype)}


def f32_bce(logits, target, grad_scale):
    x, y = logits.float(), target.float()
    n = x.numel()
    e = torch.exp(-x.abs())
    li = torch.clamp_min(x, 0) - x * y + torch.log1p(e)
    grid = bce_grid(n)
    per = 256 * grid
    T = -(-n // per)
    lp = torch.zeros(T * per)
    lp[:n] = li
    acc = torch.zeros(per)
    for i in range(T):
        acc = acc + lp[i * per:(i + 1) * per]
    acc = acc.view(grid, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :o] + acc[..., o:2 * o]
    blk = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    blk = (blk / np.float32(n)).view(-1)
    loss = torch.zeros(())
    for v in blk:
        loss = loss + v
    gs = float(np.float32(1.0 if grad_scale is None else grad_scale) / np.float32(n))
    p, q = 1.0 / (1.0 + e), e / (1.0 + e)
    S, Cc = torch.where(x >= 0, p, q), torch.where(x >= 0, q, p)
    return loss.view(1), (((1.0 - y) * S - y * Cc) * gs).to(logits.dtype)


# ---------------------------------------------------------------------------------------------- activation backward
def act_input(n, dtype, seed, act):
    """gelu: pre-activations over [-12, 12] with 0, +-1e-4 (fast_tanh cancels there) and +-12; tanh: outputs in [-1, 1] with +-1, 0"""
    g = gen(seed)
    grad = torch.randn(n, generator=g).to(dtype)
    if act == "gelu":
        src = (torch.rand(n, generator=g) * 24 - 12)
        src[:8] = torch.tensor([0.0, 1e-4, -1e-4, 12.0, -12.0, 1.0, -1.0, -0.0])
    else:
        src = torch.tanh(torch.randn(n, generator=g) * 2)
        src[:8] = torch.tensor([1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.999, -0.999])
    return grad, src.to(dtype)


def fast_tanh_delta(t, dt):
    """absolute error of fast_tanh(t) = 1 - 2 rcp(exp2(t * 2 log2 e) + 1) for an argument already off by dt:
    e = exp(2 t): relative 2 dt + (2.5 |t| + C_EXP) u (the product's rounding and the constant move the exponent, as in E());
    e + 1: u; rcp: C_RCP u; the doubling is exact; 1 - ...: u |tanh|:
      delta = 2 / (e + 1) [e rel(e) / (e + 1) + (1 + C_RCP) u] + u |tanh t|."""
    e = torch.exp(2 * t)
    rel = 2 * dt + (2.5 * t.abs() + C_EXP) * U
    w = 2 / (e + 1)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (e + 1))
    return w * (frac * rel + (1 + C_RCP) * U) + U * torch.tanh(t).abs()


def ref_act_bwd(g, src, act, mutant=None, parts=False):
    """out = g act'(src), bar = ulp16 / 2 + |g| dd + u |g d| (the fp32 product, then the 16-bit store).
    tanh (src = the output y): d = 1 - y^2, dd = u y^2 + u |d|.
    gelu (src = the pre-activation y): t = k0 (y + k1 y^3) from 5 roundings and two constants (dt = 7 u |t| at most, no
      cancellation: both terms have y's sign), th = fast_tanh(t) within delta (fast_tanh_delta), and
      d = 0.5 (1 + th) + 0.5 y (1 - th^2) k0 (1 + 3 k1 y^2) =: A + B;  dA = delta / 2 + u |A|;
      1 - th^2: 2 |th| delta + u th^2 + u |1 - th^2|; the other factors of B: 7 roundings;
      dd = dA + 7 u |B| + |0.5 y k0 (1 + 3 k1 y^2)| (2 |th| delta + u th^2 + u |1 - th^2|) + u |d|.
    mutant 'no_second_term': the GELU derivative without B."""
    gd, y = widen(g), widen(src)
    if act == "tanh":
        d = 1 - y * y
        dd = U * y * y + U * d.abs()
    else:
        t = GELU_K0 * (y + GELU_K1 * y ** 3)
        th = torch.tanh(t)
        delta = fast_tanh_delta(t, 7 * U * t.abs())
        A = torch.sigmoid(2 * t)                     # 0.5 (1 + tanh t) without the cancellation at t << 0
        rest = 0.5 * y * GELU_K0 * (1 + 3 * GELU_K1 * y * y)
        om = 1 / torch.cosh(t) ** 2                  # 1 - tanh^2 t without the cancellation at |t| >> 0
        B = rest * om
        d = A + (0.0 if mutant == "no_second_term" else B)
        dd = delta / 2 + U * A.abs() + 7 * U * B.abs() + rest.abs() * (2 * th.abs() * delta + U * th * th + U * om.abs()) + U * d.abs()
    ref = gd * d
    e32 = gd.abs() * dd + U * ref.abs()
    if parts:                # (ref, the fp32 part of the bar, the bar): the part the exp2 / rcp constants enter, apart from the store's half ulp
        return ref, e32, stored(ref, e32, g.dtype)
    return ref, stored(ref, e32, g.dtype)


def f32_act_bwd(g, src, act):
    gf, y = g.float(), src.float()
    if act == "tanh":
        d = 1.0 - y * y
    else:
        e = torch.exp2((np.float32(GELU_K0) * (y + np.float32(GELU_K1) * y * y * y)) * np.float32(2.885390081777927))
        th = 1.0 - 2.0 * (1.0 / (e + 1.0))
        d = 0.5 * (1.0 + th) + 0.5 * y * (1.0 - th * th) * np.float32(GELU_K0) * (1.0 + 3.0 * np.float32(GELU_K1) * y * y)
    return (gf * d).to(g.dtype)


# ---------------------------------------------------------------------------------------------- GradScaler bookkeeping
def ref_amp_update(scale, tracker, found_inf, growth, backoff, interval, clear):
    """torch._amp_update_scale_ restated on fp32 scalars -> (scale, inv_scale, tracker, found_inf)"""
    s, growth, backoff = np.float32(scale), np.float32(growth), np.float32(backoff)
    with np.errstate(over="ignore"):
        if found_inf > 0:
            s, tracker = np.float32(s * backoff), 0
        else:
            tracker += 1
            if tracker == interval:
                ns = np.float32(s * growth)
                if np.isfinite(ns):
                    s = ns
                tracker = 0
    return float(s), float(np.float32(1.0) / s), int(tracker), (0.0 if clear else float(found_inf))


AMP_CASES = [   # scale, tracker, found_inf, growth, backoff, interval, clear
    (65536.0, 5, 1.0, 2.0, 0.5, 2000, True),            # back-off, found_inf cleared
    (65536.0, 5, 1.0, 2.0, 0.5, 2000, False),           # back-off, found_inf kept
    (65536.0, 1998, 0.0, 2.0, 0.5, 2000, True),         # growth exactly at the interval
    (65536.0, 1997, 0.0, 2.0, 0.5, 2000, True),         # one short of it
    (2.0 ** 127, 0, 0.0, 2.0, 0.5, 1, True),            # growth would overflow: the scale stays, the tracker restarts
    (2.0 ** 127, 7, 3.0, 2.0, 0.5, 1, False),           # found_inf wins over growth
    (3.0, 0, 0.0, 2.0, 0.5, 1, True),                   # 6: inv_scale = fp32(1 / 6), not a power of two
    (1000.0, 9, 1.0, 2.0, 0.3, 10, True),               # fp32(0.3) back-off
]


# ---------------------------------------------------------------------------------------------- non-finite flag
def nonfinite_positions(n, dtype):
    """first, last and every position of the tail the kernel handles apart (n % 8 for 16-bit, n % 4 for fp32)"""
    tail = n % (4 if dtype == F32 else 8)
    return sorted({0, n - 1} | set(range(n - tail, n)))


def finite_max(dtype):
    return torch.finfo(dtype).max


# ---------------------------------------------------------------------------------------------- the cases both test files use
MAXPOOL_CASES = [   # N, H, W, C, k, s, p, backward route
    (2, 8, 10, 8, 3, 2, 1, "patch"), (3, 2, 2, 24, 3, 2, 1, "patch"),
    (2, 13, 11, 24, 3, 2, 1, "k3s2"), (3, 1, 5, 8, 3, 2, 1, "k3s2"), (2, 7, 8, 64, 3, 2, 1, "k3s2"),
    (2, 6, 8, 8, 2, 2, 0, "generic"), (2, 5, 7, 24, 3, 1, 1, "generic"), (2, 9, 9, 64, 3, 2, 0, "generic"), (2, 11, 6, 8, 5, 3, 2, "generic"),
]
MAXPOOL_BIG = (5, 460, 460, 64, 3, 2, 1, "patch")     # 5 * 230 * 230 * 8 = 2 116 000 items > 8192 * 256: the second grid-stride trip
AVGPOOL_CASES = [(5, 49, 2048), (3, 1, 8), (2, 49, 24), (2049, 1, 2048)]      # the last: N C / 8 = 524 544 > 2048 * 256
AVGPOOL_BWD_BIG = (42, 49, 2048)                                              # N HW C / 8 = 526 848 > 2048 * 256
LAYOUT_CASES = [   # N, C, H, W, Cp
    (2, 3, 5, 7, 4), (3, 3, 17, 19, 4), (2, 3, 5, 7, 8), (2, 3, 17, 19, 8), (1, 10, 3, 3, 16), (2, 10, 13, 23, 16), (1, 80, 9, 1, 80),
    (2, 80, 37, 5, 80),
]
XENT_CASES = [   # id, rows, classes, ld, offset (floats), ld_out, smoothing, ignore_index, ignored, grad_scale, grad dtype
    ("c2_ld2", 37, 2, 2, 0, None, 0.0, -100, "some", None, F32),
    ("c2_ld8", 256, 2, 8, 0, 8, 0.1, -1, "some", 128.0, F16),
    ("c1000", 37, 1000, 1000, 0, None, 0.1, -100, "some", None, F32),
    ("c1000_row1", 1, 1000, 1008, 0, 1008, 0.0, -100, "none", 128.0, BF16),
    ("c1000_f16", 37, 1000, 1000, 0, None, 0.0, -1, "some", None, F16),
    ("c1000_lossonly", 37, 1000, 1000, 0, None, 0.1, -100, "some", None, None),
    ("c1000_allignored", 37, 1000, 1000, 0, None, 0.1, -100, "all", 128.0, F32),
    ("c4095", 256, 4095, 4095, 0, None, 0.1, -1, "some", None, F32),
    ("c4097_ld4097", 37, 4097, 4097, 0, None, 0.0, -100, "some", None, F32),
    ("w4096", 37, 4096, 4096, 0, None, 0.0, -100, "some", None, F32),
    ("w4096_smooth_f16", 256, 4096, 4096, 0, None, 0.1, -1, "some", 128.0, F16),
    ("w4097_bf16", 37, 4097, 4100, 0, 4100, 0.1, -100, "some", None, BF16),
    ("w4098_row1", 1, 4098, 4104, 0, 4104, 0.0, -100, "none", None, F32),
    ("w4096_ldout", 37, 4096, 4096, 0, 4104, 0.1, -100, "some", 128.0, F32),
    ("w4096_lossonly", 37, 4096, 4096, 0, None, 0.1, -100, "some", None, None),
    ("w4096_allignored", 37, 4096, 4096, 0, None, 0.0, -1, "all", None, F32),
    ("b4096_oddld", 37, 4096, 4097, 0, None, 0.1, -100, "some", None, F32),          # router boundary: narrow
    ("b4096_offset", 37, 4096, 4096, 1, None, 0.1, -100, "some", None, F32),         # router boundary: narrow
    ("b4096_ldout4097", 37, 4096, 4096, 0, 4097, 0.1, -100, "some", None, F32),      # router boundary: narrow
]
XENT_BOUNDARY_TWIN = "w4096_twin"     # the wide result the three boundary cases must agree with: same inputs, aligned


def xent_case_route(case):
    _, rows, classes, ld, off, ld_out, s, ign, ignored, scale, gdt = case
    return xent_route(classes, ld, ld_out, off * 4, gdt is not None)


def xent_case_input(case):
    cid, rows, classes = case[:3]
    seed = 4096 if cid.startswith("b4096") or cid == XENT_BOUNDARY_TWIN else sum(map(ord, cid))
    return xent_input(rows, classes, seed, case[7], case[8])


CAST_PAIRS = [(a, b) for a in (F32, F16, BF16) for b in (F32, F16, BF16)]
CAST_FLAT_N = [1, 2, 3, 5, 1027, 2100003]             # the last: n / 4 = 525 000 > 2048 * 256
TRANSPOSE_CASES = [(1, 1, 1, 1), (64, 64, 64, 64), (65, 63, 72, 80), (130, 70, 77, 136)]      # rows, cols, ld_x, ld_y
BCE_N = [1, 1000, 4099, 2100001]                      # the last: above 2048 * 1024
NONFINITE_N = [1, 7, 8, 9, 4099]
AXPBY_N = [1, 3, 4, 4099]
ACT_N = [8, 8 * 1031]
