"""float64 statements, derived per-element bars, input builders, case tables and a faulty float32 model for the 24 entry points of
csrc/waveglow.hip: the training step (wg_taps*, wg_gate_*, wg_invconv_*, wg_logdet_inv*, wg_coupling_*, wg_loss, wg_dz_init,
wg_weight_norm_* with their table-driven forms, wg_upsample_weight*) and the reverse flow (wg_flow_inv, wg_flow_inv_first).
tests/ only: no GPU and no ctypes in here.  The helpers (U, TINY, ulp, stored, ratio, worst, bits, same_cast, gen, f32, C_EXP, C_RCP)
are those of tests/_smallops_reference.py, the sigmoid and the tanhf figure those of tests/_tacotron2_reference.py.

Shape of the module.  For every kernel K:
    K_inputs(case, dtype) -> dict of CPU tensors, exactly as the kernel sees them;
    K_model(inp, fault)   -> dict of outputs: the kernel's arithmetic in float32 on the CPU (a correctly rounded exp, torch's
                             summation order); `fault` plants one error (FAULTS); an element a faulty kernel would not write holds
                             NaN, what the GPU test's guard pattern holds there;
    K_check(inp, got)     -> {output name: (largest |got - ref| / bar, flat index)} over EVERY element of every output; outputs
                             that are copies, gathers, permutations, zero padding or 16-bit roundings of a returned fp32 value have
                             no bar: they are compared bit for bit and report 0 or inf.
kernel_model(kernel, inp, fault=None) and check(kernel, inp, got) dispatch on the kernel's name.  The pass condition is ratio <= 1.

Bars.  u = 2^-24 is one fp32 rounding (half an ulp, relative, at worst).  A sum of n terms in an order the test does not assume:
(n - 1) u sum|term|; a tree of depth D over rounded products: D u sum|term| with the product's rounding counted as one level
(a contraction to FMA spends less).  A 16-bit store: half a ulp at the far end of the fp32 bar (stored()).  c is the number of
active channels of the [M, 8] flow state, off = 8 - c, nh = c / 2.  The build (deeplearningexamples_amd/build.py FLAGS) carries
neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt, so `/` and sqrtf are IEEE: u each (ieee_div_sqrt() reads the
flags; were they loosened, C_SQRT and C_DIV would become measured constants starting at 2 u).
  __expf(a): relative E(|a|) = (2.25 |a| + C_EXP) u (derived in _smallops_reference); below 2^-126 the error is absolute.
  sigmoid 1 / (1 + __expf(-x)): _tacotron2_reference.sigmoid_ref.     tanhf (library): 4 u relative + 2^-126.
  taps            a gather of 16-byte groups: bit for bit, all-zero bits outside [0, T) of the row's own sample.
  taps_bwd        acc = addend (exact), then += the n_live <= ntaps exact 16-bit terms: n = n_live + [addend] operands,
                  stored((n - 1) u sum|term|), n counted per element.
  gate_fwd        out = th sg: d_th sg + |th| d_sg + u |out| + 2^-126, stored.
  gate_bwd        om = 1 - th^2 evaluated as 1 - fl(th th): |d om| <= 2 |th| d_th + u th^2 + u |om|.  At saturation om -> 0 while the
                  error stays (2 . 4 + 1) u: ABSOLUTE in th, so the reference is 1 / cosh^2 and the bar is not relative to it.
                  da = g sg om: |g| (d_sg |om| + sg d_om) + 2 u |da|;   1 - sg: d_sg + u |1 - sg| (reference sigmoid(-x));
                  db = g th sg (1 - sg): |g| [d_th sg (1 - sg) + |th| d_sg (1 - sg) + |th| sg d_(1 - sg)] + 3 u |db|; + 2^-126, stored.
  invconv_fwd     y[:, off + j] = sum_i W[j, i] x[:, off + i] as an 8-term product with the identity rows: 8 u sum|w x| in any order;
                  y[:, :off] bit for bit x (1 x + zeros is exact); a0 = r16(y_got[:, off:off + nh]) | +0, bit for bit.
  invconv_bwd     g = dy + da0 on the first nh active channels: u |g| there, exact elsewhere.  dx[:, off + i] = sum_j W[j, i] g[j]:
                  8 u sum|w g| + sum|w| d_g; dx[:, :off] bit for bit dy.
                  dW[j, i] = sum_m g[m, off + j] x[m, off + i] - sc coef WinvT[j, i].  Depth of the tree, not M: a thread makes
                  T = ceil(M / (256 G)) trips (a product and an add each: T + 1 levels), the wave sum 6, the sum across the 4 waves
                  3, the finishing kernel G - 1 (G = min(128, ceil(M / 256)) partials):  D = T + 9 + G levels,
                  D u sum|g x| + sum d_g |x|;  sc coef WinvT: two products, 2 u |.|;  the subtraction: u |dW|.
  logdet_inv      Gauss-Jordan with partial pivoting in fp64 on one lane, one fp32 rounding of each result.  With eps = 2^-53 and
                  kappa = ||W|| ||W^-1|| (2-norm) the elimination's backward error is a modest multiple of c eps ||W||, which moves
                  log|det| by at most c kappa times that relative amount and W^-1 by kappa times it:
                      logdet: u |ld| + 8 c^2 kappa eps + 2^-126       W^-T[i, j]: u |v| + 8 c kappa eps max|W^-1| + 2^-126
                  (the fp64 terms are 1e-11 at kappa = 1e3, against u |v| = 6e-8 |v|: they matter where ld is near 0).  sign: +-1 exact.
                  Batched: slot f = 64 floats, the floats past c^2 and every other flow's slot keep their bits.
  coupling_fwd    z1 = __expf(ls) y1 + b: (E(|ls|) + u) |e^ls y1| + u |z1| + 2^-126; z[:, :off + nh] bit for bit y.
                  logs_partial[g] = the sum of log_s over the rows workgroup g owns ((m / 256) % G == g, G = wg_coupling_partials(M) =
                  min(4096, ceil(M / 256))): a thread adds T nh terms serially, block_sum 6 + 3: D = T nh + 9, D u sum|ls| per slot
                  and for the fp64 sum of the slots; exactly G floats are written.
  coupling_bwd    es = __expf(ls); dy1 = gz es: (E + u) |.|; dy[:, :off + nh] bit for bit dz; d_b = r16(gz) bit for bit;
                  d_ls = gz y1 es - lsg, lsg = sc coef (u): (E + 2 u) |gz y1 es| + u |lsg| + u |d_ls|, stored; +0 above 2 nh.
  loss            A = sum z^2: a thread's trip is 4 products, 3 adds and the add into its sum (5 levels), T = ceil(2 M / (256 G))
                  trips, block_sum 9; the finishing kernel adds ceil(G / 256) partials per thread, block_sum 9:
                      D_A = 5 T + ceil(G / 256) + 18;  B = sum logs_partial: D_B = ceil(n_logs / 256) + 9;  Dd likewise over n_flows.
                  As the C ABI forms them: inv_two_sigma2 = 1.0f / (2 sigma sigma): 2 u (one product, one division; x 2 exact);
                  rows = (float) M: exact below 2^24, else u (the reference takes the fp32 value); inv_count = 1.0f / (rows 8): u.
                  loss = (A i2s - B - rows Dd) inv_count: per term its sum's bar, the constants' roundings and the product, two
                  subtractions and the last product:
                      [D_A u A i2s + 3 u A i2s + D_B u sum|lp| + (Dd u + u) rows sum|ld| + 2 u (A i2s + |B| + rows |Dd|)] inv_count + 2 u |loss|
  dz_init         dz = z (sc coef): two roundings, 2 u |dz|.
  weight_norm_fwd s = sum v^2 over n = Ci Kt: a lane adds L = ceil(n / 64) rounded squares, the wave sum 6: relative (L + 7) u (all
                  terms >= 0); sqrtf: half of it + C_SQRT u; g / .: C_DIV u; v f: u:  stored(|w| ((L + 7) / 2 + C_SQRT + C_DIV + 1) u).
                  Columns ci >= Ci: +0 bits.  g == NULL: r16(v) re-laid out, bit for bit.
  weight_norm_bwd d = sum dw v: (L + 7) u sum|dw v|;  inv = 1 / sqrtf(s): r = ((L + 7) / 2 + C_SQRT + C_DIV) u;  dg = d inv: d_d inv +
                  (r + u) |dg|;  t = v d inv inv: |v| inv^2 d_d + (2 r + 3 u) |t|;  dv = (g inv) (dw - t): |g inv| (d_t + u |dw - t|) +
                  (r + 2 u) |dv|.   g == NULL: dv = dw re-laid out, bit for bit.
  upsample_weight a permutation and one cast; its backward a permutation: bit for bit.
  flow_inv_first  sigma noise: ONE IEEE product, so the CPU's fp32 product is the answer bit for bit; the other columns +0.
  flow_inv        x1' = (x1 - b) expf(-ls): (2 + C_EXPF) u |x1'|;  out[:, off + j] = sum_i W^-1[j, i] x'_i: 8 u sum|w x'| + sum|w| d_x';
                  columns [off - early, off) = sigma noise[:, z_col ..]: one IEEE product, bit for bit; below off - early bit for bit
                  the state; a0 = r16(out_got[:, 8 - next_c : 8 - next_c / 2]) | +0 bit for bit.

Exactly summable cases ("exact" in a case id): small integers or dyadic values, every partial sum below 2^24, so the reduction is
exact in any order and its bar is 0 -- a dropped or repeated row cannot hide (taps_bwd, invconv dW, logs_partial, the loss's sum of
squares -- checked through fl(fl(A / 2) fl(1 / (8 M))) with sigma = 1 and no other term --, the weight-norm sums with n = 64 rows of
+-1: s = 64, sqrt = 8, g a multiple of 8).

Measured constant.  C_EXPF, the library expf of wg_flow_inv, is the only number introduced here that is not derived (no accuracy
statement for it was found in the ROCm installation's documentation on the build machine); it starts at 2 u under the rule of
_smallops_reference.  The rule's element class -- elements whose bar is at least half made of the constant -- is EMPTY for flow_inv:
the exponential's C_EXPF u |w x'| sits next to the product's 8 u sum|w x'| >= 8 u |w x'|, four times it, in every element.  The
check therefore records the figure on the elements where the constant's share is largest ("out, largest C_EXPF share": at least
0.9 of the largest share found, which is at most 2 / 12 = 0.17 of the bar).  The first MI355X run of tests/test_gpu_waveglow_reference.py, with
C_EXPF = 2 u, recorded 0.315 (fp16 and bf16 alike: the state is fp32) on that class, against 0.313 for the float32 model with a
correctly rounded exp, and 0.430 over all elements of `out`: at or below 0.5, so the constant stays at 2 u (before = after = 2 u).
No sqrtf / division constant was needed: the build flags keep both IEEE.
"""
import numpy as np
import torch

from tests import _smallops_reference as S
from tests import _tacotron2_reference as T2

F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16
I16, I64 = torch.int16, torch.int64
U, TINY, C_EXP, C_RCP = S.U, S.TINY, S.C_EXP, S.C_RCP
ulp, stored, ratio, worst, bits, same_cast, gen, widen, name, f32 = (S.ulp, S.stored, S.ratio, S.worst, S.bits, S.same_cast, S.gen,
                                                                     S.widen, S.name, S.f32)
sigmoid_ref, exp_rel, r16, untouched = T2.sigmoid_ref, T2.exp_rel, T2.r16, T2.untouched
_bitcmp, _worse = T2._bitcmp, T2._worse
INF = float("inf")
EPS64 = 2.0 ** -53
WG_BLOCK, WG_CAP, INVCONV_BWD_CAP = 256, 4096, 128
ONE_TRIP = WG_BLOCK * WG_CAP          # items a streaming kernel covers before its grid-stride loop takes a second trip
C_EXPF = 2.0                          # library expf, in u (module docstring: measured constant)


def ieee_div_sqrt(flags=None):
    """True when the library is built with correctly rounded fp32 `/` and sqrtf (hipcc's default), read from the build flags"""
    if flags is None:
        from deeplearningexamples_amd import build
        flags = build.FLAGS
    loose = ("-ffast-math", "-Ofast", "-funsafe-math-optimizations", "-freciprocal-math", "-fapprox-func",
             "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffp-model=fast", "-ffp-model=aggressive", "-cl-fast-relaxed-math")
    return not any(f in loose for f in flags)


C_SQRT = C_DIV = 1.0 if ieee_div_sqrt() else 2.0

FAULTS = ("taps_ignore_boundary", "left_ignored", "gate_halves_swapped", "one_minus_sg_dropped", "w_transposed", "embed_off_by_one",
          "a0_second_half", "da0_dropped", "logdet_term_dropped", "logdet_scale_dropped", "logs_from_b", "lsg_sign", "rows_dropped",
          "norm_over_padded_row", "layout_swapped", "table_row_off_by_one", "phase_tap_swapped", "wrong_noise_column",
          "second_trip_skipped", "winv_not_transposed")


def grid(items, per=WG_BLOCK, cap=WG_CAP):
    """wg_grid of the launcher"""
    return max(1, min(cap, -(-items // per)))


def _seed(cid):
    return 9000 + sum(map(ord, str(cid)))


def _reach(items, fault, cap=ONE_TRIP):
    """bool [items]: what a kernel that takes one grid-stride trip only reaches; None when the fault has no place here"""
    if fault != "second_trip_skipped" or items <= cap:
        return None
    return torch.arange(items) < cap


def _rows(mask, t, other):
    """t where the row mask holds, `other` elsewhere"""
    return t if mask is None else torch.where(mask.view(-1, *([1] * (t.dim() - 1))), t, other)


def _pad16(cols, dtype):
    """[M, k] fp32 -> the zero-padded 16-bit [M, 8] operand"""
    out = torch.zeros(cols.shape[0], 8, dtype=dtype)
    out[:, :cols.shape[1]] = r16(cols, dtype)
    return out


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ================================================================================================ wg_taps / wg_taps_bwd
TAPS_CASES = [   # id, B, T, C, ntaps, dilation, left, ld_x
    ("k3_d1", 2, 7, 8, 3, 1, 1, 8),
    ("k3_d4_T5", 3, 5, 16, 3, 4, 1, 16),                  # only the middle tap of most rows is inside the sample
    ("k3_d8_T5", 2, 5, 8, 3, 8, 1, 8),                    # dilation > T: the outer taps are all-zero everywhere
    ("k2_left0", 1, 6, 8, 2, 1, 0, 8),
    ("slice_2C", 2, 9, 16, 3, 2, 1, 32),                  # x = a column slice of a matrix twice as wide
    ("slice_C8", 2, 9, 16, 3, 2, 1, 24),
    ("upsample_neg", 2, 11, 80, 4, -1, 0, 80),            # the upsampling GEMM's operand: dilation -1, left 0
    ("m257", 1, 257, 8, 3, 1, 1, 8),
    ("second_trip", 2, 2735, 512, 3, 1, 1, 512),          # 1 050 240 items of 16 bytes
]


def taps_items(case):
    _, b, t, c, nt = case[:5]
    return b * t * nt * (c // 8)


def taps_inputs(case, dtype):
    """N(0, 1) with NaN, +-inf, -0 and the largest finite value planted (a gather keeps every bit)"""
    cid, b, t, c = case[:4]
    x = torch.randn(b * t, c, generator=gen(_seed(cid))).to(dtype)
    sp = torch.tensor([float("nan"), INF, -INF, -0.0, torch.finfo(dtype).max, 2.0 ** -24], dtype=F32).to(dtype)
    x.view(-1)[:6] = sp
    x[b * t - 1, c - 1] = -0.0
    return {"case": case, "dtype": dtype, "x": x}


def _tap_src(case, k, fault, sign):
    """(source row, valid) of tap k for every output row r = b T + t; sign +1: the gather, -1: its transpose"""
    _, b, t, c, nt, dil, left = case[:7]
    r = torch.arange(b * t)
    tt = r % t
    sh = sign * (k - (0 if fault == "left_ignored" else left)) * dil
    if fault == "taps_ignore_boundary":
        return r + sh, (r + sh >= 0) & (r + sh < b * t)
    return r + sh, (tt + sh >= 0) & (tt + sh < t)


def taps_model(inp, fault=None):
    case, dt = inp["case"], inp["dtype"]
    _, b, t, c, nt = case[:5]
    xb = bits(inp["x"])
    col = torch.zeros(b * t, nt, c, dtype=I16)
    for k in range(nt):
        src, ok = _tap_src(case, k, fault, +1)
        col[:, k] = torch.where(ok.view(-1, 1), xb[src.clamp(0, b * t - 1)], torch.zeros((), dtype=I16))
    col = col.view(b * t, nt * c).view(dt)
    reach = _reach(taps_items(case), fault)
    if reach is not None:
        col = torch.where(reach.repeat_interleave(8).view(b * t, nt * c), col, untouched((), dt))
    return {"col": col}


def taps_check(inp, got):
    return {"col": _bitcmp(got["col"], taps_model(inp)["col"])}


TAPS_BWD_CASES = [   # id, B, T, C, ntaps, dilation, left, addend (None | separate | alias), ld_dx, ld_add
    ("noadd", 2, 7, 8, 3, 1, 1, None, 8, 0),
    ("separate", 2, 9, 16, 3, 2, 1, "separate", 24, 40),             # ld_add != ld_dx, both wider than C
    ("alias", 3, 5, 16, 3, 4, 1, "alias", 32, 32),                   # dx IS the addend
    ("alias_d8_T5", 2, 5, 8, 3, 8, 1, "alias", 8, 8),                # one live term: the addend passes through its 16-bit store
    ("upsample_neg", 2, 11, 80, 4, -1, 0, None, 88, 0),
    ("m257", 1, 257, 8, 3, 1, 1, "separate", 8, 16),
    ("exact", 2, 13, 8, 3, 2, 1, "separate", 16, 8),                 # integers in [-8, 8]: bar 0
    ("second_trip", 2, 8200, 512, 3, 1, 1, "separate", 512, 520),    # 1 049 600 items
]


def taps_bwd_inputs(case, dtype):
    cid, b, t, c, nt, dil, left, add = case[:8]
    g = gen(_seed(cid))
    if cid == "exact":
        dcol, addend = _ints((b * t, nt * c), -8, 8, g), _ints((b * t, c), -8, 8, g)
    else:
        dcol, addend = torch.randn(b * t, nt * c, generator=g), torch.randn(b * t, c, generator=g)
    return {"case": case, "dtype": dtype, "dcol": dcol.to(dtype), "addend": addend.to(dtype) if add else None}


def taps_bwd_model(inp, fault=None):
    case, dt = inp["case"], inp["dtype"]
    _, b, t, c, nt = case[:5]
    d = inp["dcol"].float().view(b * t, nt, c)
    acc = inp["addend"].float().clone() if inp["addend"] is not None else torch.zeros(b * t, c)
    for k in range(nt):
        src, ok = _tap_src(case, k, fault, -1)
        acc = acc + torch.where(ok.view(-1, 1), d[src.clamp(0, b * t - 1), k], torch.zeros(()))
    dx = r16(acc, dt)
    reach = _reach(b * t * (c // 8), fault)
    if reach is not None:
        dx = torch.where(reach.repeat_interleave(8).view(b * t, c), dx, inp["addend"] if case[7] == "alias" else untouched((), dt))
    return {"dx": dx}


def taps_bwd_check(inp, got):
    case, dt = inp["case"], inp["dtype"]
    _, b, t, c, nt = case[:5]
    d = widen(inp["dcol"]).view(b * t, nt, c)
    has = inp["addend"] is not None
    ref = widen(inp["addend"]).clone() if has else torch.zeros(b * t, c, dtype=F64)
    mag, n = ref.abs(), torch.full((b * t, 1), 1.0 if has else 0.0, dtype=F64)
    for k in range(nt):
        src, ok = _tap_src(case, k, None, -1)
        term = torch.where(ok.view(-1, 1), d[src.clamp(0, b * t - 1), k], torch.zeros((), dtype=F64))
        ref, mag, n = ref + term, mag + term.abs(), n + ok.view(-1, 1).double()
    bar = stored(ref, (n - 1).clamp_min(0) * U * mag, dt)
    if case[0] == "exact":
        bar = torch.zeros_like(bar)
    return {"dx": worst(got["dx"], ref, bar)}


# ================================================================================================ wg_gate_fwd / bwd
GATE_CASES = [   # id, M, nc, ld_s, ld_ds
    ("m1", 1, 8, 16, 24),
    ("m255", 255, 8, 24, 16),
    ("m257_nc24", 257, 24, 56, 48),
    ("m1000", 1000, 64, 136, 128),
    ("second_trip", 16400, 512, 1032, 1024),             # 1 049 600 items of 8 channels
]


def gate_plants(dtype):
    sub = 2.0 ** -24 if dtype == F16 else 2.0 ** -133
    mx = float(torch.finfo(dtype).max)
    return torch.tensor([0.0, sub, -sub, 8.0, -8.0, 20.0, -20.0, 88.0, -88.0, mx, -mx], dtype=F64)


def gate_inputs(case, dtype):
    """s = (a | b) N(0, 2); the first elements carry pairs of the planted values 0, +-the smallest subnormal, +-8, +-20, +-88, +-the
    largest finite value (every value meets every other one where 121 elements fit, the diagonal first); dacts N(0, 1)"""
    cid, m, nc = case[:3]
    g = gen(_seed(cid))
    s = torch.randn(m, 2 * nc, generator=g, dtype=F64) * 2
    p = gate_plants(dtype)
    k = min(m * nc, p.numel() ** 2)
    i = torch.arange(k)
    rows, cols = i // nc, i % nc
    s[rows, cols] = p[i % 11]
    s[rows, nc + cols] = p[(i % 11 + i // 11) % 11]
    return {"case": case, "dtype": dtype, "s": s.to(dtype), "dacts": torch.randn(m, nc, generator=g).to(dtype)}


def _gate_halves(inp, work, fault=None):
    nc = inp["case"][2]
    s = inp["s"].to(work)
    a, b = s[:, :nc], s[:, nc:]
    return (b, a) if fault == "gate_halves_swapped" else (a, b)


def gate_fwd_model(inp, fault=None):
    m, nc = inp["case"][1:3]
    a, b = _gate_halves(inp, F32, fault)
    out = r16(torch.tanh(a) * (1.0 / (1.0 + torch.exp(-b))), inp["dtype"])
    reach = _reach(m * (nc // 8), fault)
    if reach is not None:
        out = torch.where(reach.repeat_interleave(8).view(m, nc), out, untouched((), inp["dtype"]))
    return {"acts": out}


def _gate_parts(inp):
    a, b = _gate_halves(inp, F64)
    th = torch.tanh(a)
    sg, dsg = sigmoid_ref(b)
    return a, b, th, 4 * U * th.abs() + TINY, sg, dsg


def gate_fwd_check(inp, got):
    a, b, th, dth, sg, dsg = _gate_parts(inp)
    out = th * sg
    return {"acts": worst(got["acts"], out, stored(out, dth * sg + th.abs() * dsg + U * out.abs() + TINY, inp["dtype"]))}


def gate_bwd_model(inp, fault=None):
    m, nc = inp["case"][1:3]
    a, b = _gate_halves(inp, F32, fault)
    g = inp["dacts"].float()
    th, sg = torch.tanh(a), 1.0 / (1.0 + torch.exp(-b))
    da = g * sg * (1.0 - th * th)
    db = g * th * sg * (1.0 if fault == "one_minus_sg_dropped" else (1.0 - sg))
    ds = r16(torch.cat([da, db], 1), inp["dtype"])
    reach = _reach(m * (nc // 8), fault)
    if reach is not None:
        ds = torch.where(reach.repeat_interleave(8).view(m, nc).repeat(1, 2), ds, untouched((), inp["dtype"]))
    return {"ds": ds}


def gate_bwd_check(inp, got):
    a, b, th, dth, sg, dsg = _gate_parts(inp)
    g = widen(inp["dacts"])
    om = 1 / torch.cosh(a) ** 2
    d_om = 2 * th.abs() * dth + U * th * th + U * om
    da = g * sg * om
    e_da = g.abs() * (dsg * om + sg * d_om) + 2 * U * da.abs() + TINY
    omsg = torch.sigmoid(-b)
    d_omsg = dsg + U * omsg
    db = g * th * sg * omsg
    e_db = g.abs() * (dth * sg * omsg + th.abs() * dsg * omsg + th.abs() * sg * d_omsg) + 3 * U * db.abs() + TINY
    ref, err = torch.cat([da, db], 1), torch.cat([e_da, e_db], 1)
    return {"ds": worst(got["ds"], ref, stored(ref, err, inp["dtype"]))}


# ================================================================================================ wg_invconv_fwd / bwd
ROW_M = [1, 255, 257, 1000]
ROW_BIG = 1048833                                 # one thread per row of [M, 8]: 4096 x 256 + 257 rows
INVCONV_CASES = [("m%d_c%d" % (m, c), m, c) for m, c in zip(ROW_M, (2, 4, 6, 8))] + [("m257_c2", 257, 2), ("m1000_c4", 1000, 4),
                                                                                      ("exact_m1000_c6", 1000, 6), ("second_trip_c4", ROW_BIG, 4)]
INVCONV_BWD_CASES = [   # id, M, c, da0 given, scale given, logdet_coef
    ("m1_c2", 1, 2, True, False, 0.125), ("m255_c4", 255, 4, True, True, 0.125), ("m257_c6", 257, 6, False, True, 0.125),
    ("m1000_c8", 1000, 8, True, True, 0.125), ("m1000_c4", 1000, 4, True, False, 0.37), ("exact_m1000_c6", 1000, 6, True, False, 0.0),
    ("second_trip_c8", 33025, 8, True, True, 0.125),       # G = 128 workgroups: 32 768 rows per trip
]


def _mix_matrix(c, g, exact=False):
    if exact:
        return _ints((c, c), -2, 2, g) + 3 * torch.eye(c)
    q, _ = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=F64))
    return (q + 0.05 * torch.randn(c, c, generator=g, dtype=F64)).float().contiguous()       # (qr hands back a column-major q)


def invconv_inputs(case, dtype):
    cid, m, c = case
    g = gen(_seed(cid))
    ex = cid.startswith("exact")
    return {"case": case, "dtype": dtype, "c": c, "x": _ints((m, 8), -8, 8, g) if ex else torch.randn(m, 8, generator=g), "W": _mix_matrix(c, g, ex)}


def _embed(W, c, fault=None):
    """diag(I_off, W) as the kernels' 8 x 8 matrix"""
    off = 8 - c
    if fault == "embed_off_by_one" and off > 0:
        off -= 1
    w8 = torch.eye(8, dtype=W.dtype)
    w8[off:off + c, off:off + c] = W.t() if fault == "w_transposed" else W
    return w8


def invconv_fwd_model(inp, fault=None):
    c, x, dt = inp["c"], inp["x"], inp["dtype"]
    off, nh = 8 - c, c // 2
    y = x @ _embed(inp["W"], c, fault).t()
    if fault != "embed_off_by_one":
        y[:, :off] = x[:, :off]
    lo = off + nh if fault == "a0_second_half" else off
    a0 = _pad16(y[:, lo:lo + nh], dt)
    reach = _reach(x.shape[0], fault)
    return {"y": _rows(reach, y, untouched((), F32)), "a0": _rows(reach, a0, untouched((), dt))}


def invconv_fwd_check(inp, got):
    c, dt = inp["c"], inp["dtype"]
    off, nh = 8 - c, c // 2
    x, W = widen(inp["x"]), widen(inp["W"])
    ref, mag = x[:, off:] @ W.t(), x[:, off:].abs() @ W.abs().t()
    bar = torch.zeros_like(mag) if inp["case"][0].startswith("exact") else 8 * U * mag
    res = {"y": worst(got["y"][:, off:], ref, bar), "a0": _bitcmp(got["a0"], _pad16(got["y"][:, off:off + nh], dt))}
    res["y pass-through"] = _bitcmp(got["y"][:, :off], inp["x"][:, :off])
    return res


def invconv_bwd_inputs(case, dtype):
    cid, m, c, has_da0, has_scale, coef = case
    g = gen(_seed(cid))
    ex = cid.startswith("exact")
    W = _mix_matrix(c, g, ex)
    rnd = (lambda: _ints((m, 8), -4, 4, g)) if ex else (lambda: torch.randn(m, 8, generator=g))
    return {"case": case, "dtype": dtype, "c": c, "dy": rnd(), "x": rnd(), "da0": rnd() if has_da0 else None, "W": W,
            "winv_t": torch.linalg.inv(W.double()).t().contiguous().float(), "scale": torch.tensor([3.0]) if has_scale else None, "coef": coef}


def invconv_bwd_partials(m):
    return grid(m, cap=INVCONV_BWD_CAP)


def _g_of(inp, work, fault=None):
    c = inp["c"]
    off, nh = 8 - c, c // 2
    g = inp["dy"].to(work).clone()
    if inp["da0"] is not None and fault != "da0_dropped":
        g[:, off:off + nh] += inp["da0"].to(work)[:, :nh]
    return g


def invconv_bwd_model(inp, fault=None):
    c, m = inp["c"], inp["dy"].shape[0]
    off = 8 - c
    g = _g_of(inp, F32, fault)
    dx = g @ _embed(inp["W"], c, fault)
    if fault != "embed_off_by_one":
        dx[:, :off] = g[:, :off]
    reach = _reach(m, fault, invconv_bwd_partials(m) * WG_BLOCK)
    gs, xs = (g, inp["x"]) if reach is None else (g[reach], inp["x"][reach])
    s = gs[:, off:].t() @ xs[:, off:]
    sc = np.float32(1.0 if inp["scale"] is None or fault == "logdet_scale_dropped" else float(inp["scale"]))
    dW = s if fault == "logdet_term_dropped" else s - float(sc * np.float32(inp["coef"])) * inp["winv_t"]
    return {"dx": _rows(reach, dx, untouched((), F32)), "dW": dW.contiguous()}


def invconv_bwd_check(inp, got):
    c, m = inp["c"], inp["dy"].shape[0]
    off, nh = 8 - c, c // 2
    ex = inp["case"][0].startswith("exact")
    g, x, W = _g_of(inp, F64), widen(inp["x"]), widen(inp["W"])
    d_g = torch.zeros_like(g)
    if inp["da0"] is not None and not ex:
        d_g[:, off:off + nh] = U * g[:, off:off + nh].abs()
    ref, bar = g[:, off:] @ W, 8 * U * (g[:, off:].abs() @ W.abs()) + d_g[:, off:] @ W.abs()
    res = {"dx": worst(got["dx"][:, off:], ref, torch.zeros_like(bar) if ex else bar),
           "dx pass-through": _bitcmp(got["dx"][:, :off], inp["dy"][:, :off])}
    G = invconv_bwd_partials(m)
    D = -(-m // (WG_BLOCK * G)) + 9 + G
    s, mag = g[:, off:].t() @ x[:, off:], g[:, off:].abs().t() @ x[:, off:].abs()
    sc = 1.0 if inp["scale"] is None else float(inp["scale"])
    term = sc * f32(inp["coef"]) * widen(inp["winv_t"])
    dW = s - term
    e = D * U * mag + d_g[:, off:].t() @ x[:, off:].abs() + 2 * U * term.abs() + U * dW.abs()
    res["dW"] = worst(got["dW"].view(c, c), dW, torch.zeros_like(e) if ex else e)
    return res


# ================================================================================================ wg_logdet_inv (+ batched)
LOGDET_KINDS = ("well", "pivot", "negdet")
LOGDET_CASES = [(kind, c) for c in range(1, 9) for kind in LOGDET_KINDS]
LOGDET_TABLES = {"five_flows": [(8, 8), (96, 8), (200, 6), (264, 4), (320, 2)], "one_flow": [(16, 3)], "odd_c": [(0, 1), (8, 5), (40, 7)]}


def logdet_matrix(kind, c, seed=0):
    """well: orthogonal + 0.05 N(0, 1) (kappa <= 1e3, asserted by the host test); pivot: the same with W[0, 0] = 0 (c = 1: a small
    pivot 2^-10); negdet: row 0 negated when the determinant is positive"""
    g = gen(_seed("%s%d" % (kind, c)) + seed)
    W = _mix_matrix(c, g).double() * 1.5
    if kind == "pivot":
        W[0, 0] = 0.0 if c > 1 else 2.0 ** -10
    s = torch.linalg.slogdet(W)[0]
    if (kind == "negdet") != (float(s) < 0):
        W[0] = -W[0]
    return W.float().contiguous()


def logdet_inputs(case, dtype=None):
    kind, c = case
    return {"case": case, "dtype": dtype, "c": c, "W": logdet_matrix(kind, c)}


def logdet_model(inp, fault=None):
    W = inp["W"].double()
    sign, ld = torch.linalg.slogdet(W)
    wi = torch.linalg.inv(W)
    return {"logdet": ld.float().view(1), "sign": sign.float().view(1), "winv_t": (wi if fault == "winv_not_transposed" else wi.t()).contiguous().float()}


def _logdet_one(W, got_ld, got_sign, got_wt):
    c = W.shape[0]
    Wd = W.double()
    sign, ld = torch.linalg.slogdet(Wd)
    wi = torch.linalg.inv(Wd)
    kappa = float(torch.linalg.matrix_norm(Wd, 2) * torch.linalg.matrix_norm(wi, 2))
    r_ld = worst(got_ld.view(1), ld.view(1), (U * ld.abs() + 8 * c * c * kappa * EPS64 + TINY).view(1))
    ref = wi.t().contiguous()
    r_wt = worst(got_wt.reshape(c, c), ref, U * ref.abs() + 8 * c * kappa * EPS64 * float(wi.abs().max()) + TINY)
    return r_ld, _bitcmp(got_sign.view(1), sign.float().view(1)), r_wt


def logdet_check(inp, got):
    r_ld, r_s, r_wt = _logdet_one(inp["W"], got["logdet"], got["sign"], got["winv_t"])
    return {"logdet": r_ld, "sign": r_s, "winv_t": r_wt}


def logdet_batched_inputs(case, dtype=None):
    """a flat parameter buffer of N(0, 1) junk with the flows' matrices at their offsets (kinds in rotation)"""
    tab = LOGDET_TABLES[case]
    flat = torch.randn(max(o + c * c for o, c in tab) + 8, generator=gen(_seed(case)))
    for f, (o, c) in enumerate(tab):
        flat[o:o + c * c] = logdet_matrix(LOGDET_KINDS[f % 3], c, seed=f).reshape(-1)
    return {"case": case, "dtype": dtype, "table": tab, "flat": flat}


def logdet_batched_model(inp, fault=None):
    n = len(inp["table"])
    out = {"logdets": torch.zeros(n), "signs": torch.zeros(n), "winv_t_all": untouched((n, 64), F32)}
    for f, (o, c) in enumerate(inp["table"]):
        one = logdet_model({"W": inp["flat"][o:o + c * c].view(c, c)}, fault)
        out["logdets"][f], out["signs"][f], out["winv_t_all"][f, :c * c] = one["logdet"][0], one["sign"][0], one["winv_t"].reshape(-1)
    return out


def logdet_batched_check(inp, got):
    res = {"logdets": (0.0, -1), "signs": (0.0, -1), "winv_t_all": (0.0, -1), "winv_t_all untouched": (0.0, -1)}
    for f, (o, c) in enumerate(inp["table"]):
        r_ld, r_s, r_wt = _logdet_one(inp["flat"][o:o + c * c].view(c, c), got["logdets"][f], got["signs"][f], got["winv_t_all"][f, :c * c])
        res["logdets"], res["signs"], res["winv_t_all"] = _worse(res["logdets"], r_ld), _worse(res["signs"], r_s), _worse(res["winv_t_all"], r_wt)
        res["winv_t_all untouched"] = _worse(res["winv_t_all untouched"], _bitcmp(got["winv_t_all"][f, c * c:], untouched((64 - c * c,), F32)))
    return res


# ================================================================================================ wg_coupling_fwd / bwd
COUPLING_CASES = [   # id, M, c, scale given (backward)
    ("m1_c2", 1, 2, False), ("m255_c4", 255, 4, True), ("m257_c6", 257, 6, False), ("m1000_c8", 1000, 8, True),
    ("exact_m1000_c4", 1000, 4, False), ("second_trip_c8", ROW_BIG, 8, True),
]


def coupling_inputs(case, dtype):
    """o = (b | log_s | junk): log_s N(0, 0.5) with +-10, 0 planted (exact case: multiples of 1 / 8 in [-2, 2]); the columns of o past
    c hold N(0, 1) junk the kernels must not read into anything"""
    cid, m, c, has_scale = case
    nh = c // 2
    g = gen(_seed(cid))
    y, o, dz = (torch.randn(m, 8, generator=g) for _ in range(3))
    ls = _ints((m, nh), -16, 16, g) / 8 if cid.startswith("exact") else torch.randn(m, nh, generator=g) * 0.5
    sp = torch.tensor([10.0, -10.0, 0.0])
    k = min(3, m * nh)
    ls.view(-1)[:k] = sp[:k]
    if m > 300:
        ls[m - 1, nh - 1], ls[299, 0] = -10.0, 10.0
    o[:, nh:c] = ls
    return {"case": case, "dtype": dtype, "c": c, "y": y, "o": o, "dz": dz, "scale": torch.tensor([64.0]) if has_scale else None,
            "logs_coef": 1.0 / (m * 8)}


def _block_of(m, G):
    return (torch.arange(m) // WG_BLOCK) % G


def coupling_fwd_model(inp, fault=None):
    c, y, o = inp["c"], inp["y"], inp["o"]
    m, off, nh = y.shape[0], 8 - c, c // 2
    ls = o[:, :nh] if fault == "logs_from_b" else o[:, nh:c]
    z = y.clone()
    z[:, off + nh:] = torch.exp(ls) * y[:, off + nh:] + o[:, :nh]
    G = grid(m)
    reach = _reach(m, fault)
    rows = ls.sum(1) if reach is None else torch.where(reach, ls.sum(1), torch.zeros(()))
    return {"z": _rows(reach, z, untouched((), F32)), "logs_partial": torch.zeros(G).index_add_(0, _block_of(m, G), rows)}


def coupling_fwd_check(inp, got):
    c, y, o = inp["c"], widen(inp["y"]), widen(inp["o"])
    m, off, nh = y.shape[0], 8 - c, c // 2
    ls, b, y1 = o[:, nh:c], o[:, :nh], y[:, off + nh:]
    p = torch.exp(ls) * y1
    z1 = p + b
    res = {"z": worst(got["z"][:, off + nh:], z1, (exp_rel(ls.abs()) + U) * p.abs() + U * z1.abs() + TINY),
           "z pass-through": _bitcmp(got["z"][:, :off + nh], inp["y"][:, :off + nh])}
    G = grid(m)
    if got["logs_partial"].numel() != G:
        res["logs_partial"] = (INF, 0)
        return res
    D = -(-m // (WG_BLOCK * G)) * nh + 9
    blk = _block_of(m, G)
    ref, mag = torch.zeros(G, dtype=F64).index_add_(0, blk, ls.sum(1)), torch.zeros(G, dtype=F64).index_add_(0, blk, ls.abs().sum(1))
    zero = inp["case"][0].startswith("exact")
    res["logs_partial"] = worst(got["logs_partial"], ref, torch.zeros_like(mag) if zero else D * U * mag)
    res["logs sum"] = worst(widen(got["logs_partial"]).sum().view(1), ls.sum().view(1), (0.0 if zero else D * U) * mag.sum().view(1))
    return res


def coupling_bwd_model(inp, fault=None):
    c, dz, y, o, dt = inp["c"], inp["dz"], inp["y"], inp["o"], inp["dtype"]
    m, off, nh = y.shape[0], 8 - c, c // 2
    ls = o[:, :nh] if fault == "logs_from_b" else o[:, nh:c]
    es, gz = torch.exp(ls), dz[:, off + nh:]
    lsg = float(np.float32(1.0 if inp["scale"] is None else float(inp["scale"])) * np.float32(inp["logs_coef"]))
    dy = dz.clone()
    dy[:, off + nh:] = gz * es
    dls = gz * y[:, off + nh:] * es
    d_o = torch.zeros(m, 8, dtype=dt)
    d_o[:, :nh], d_o[:, nh:c] = r16(gz, dt), r16(dls + lsg if fault == "lsg_sign" else dls - lsg, dt)
    reach = _reach(m, fault)
    return {"dy": _rows(reach, dy, untouched((), F32)), "d_o": _rows(reach, d_o, untouched((), dt))}


def coupling_bwd_check(inp, got):
    c, dt = inp["c"], inp["dtype"]
    dz, y, o = widen(inp["dz"]), widen(inp["y"]), widen(inp["o"])
    m, off, nh = y.shape[0], 8 - c, c // 2
    ls, gz, y1 = o[:, nh:c], dz[:, off + nh:], y[:, off + nh:]
    E = exp_rel(ls.abs())
    dy1 = gz * torch.exp(ls)
    lsg = (1.0 if inp["scale"] is None else float(inp["scale"])) * f32(inp["logs_coef"])
    p = gz * y1 * torch.exp(ls)
    dls = p - lsg
    want = torch.zeros(m, 8, dtype=dt)
    want[:, :nh] = r16(inp["dz"][:, off + nh:], dt)
    fixed = torch.ones(m, 8, dtype=torch.bool)
    fixed[:, nh:c] = False
    return {"dy": worst(got["dy"][:, off + nh:], dy1, (E + U) * dy1.abs() + TINY), "dy pass-through": _bitcmp(got["dy"][:, :off + nh], inp["dz"][:, :off + nh]),
            "d_o log_s": worst(got["d_o"][:, nh:c], dls, stored(dls, (E + 2 * U) * p.abs() + U * abs(lsg) + U * dls.abs() + TINY, dt)),
            "d_o b, padding": _bitcmp(got["d_o"], want, fixed)}


# ================================================================================================ wg_loss / wg_dz_init
LOSS_BIG = 524417                                  # a float4 per lane: 2 M = 1 048 834 items
LOSS_CASES = [   # id, M, n_logs, n_flows, sigma
    ("m1", 1, 1, 12, 1.0), ("m255", 255, 12, 12, 0.7), ("m257_nologs", 257, 0, 12, 1.0), ("m1000_noflows", 1000, 12, 0, 1.3),
    ("m1000_logs48k", 1000, 12 * 4096, 12, 1.0), ("exact_m1000", 1000, 0, 0, 1.0), ("exact_second_trip", LOSS_BIG, 0, 0, 1.0),
    ("second_trip", LOSS_BIG, 12 * 4096, 12, 1.0),
]
DZ_CASES = [("m1", 1, False), ("m255", 255, True), ("m257", 257, False), ("m1000", 1000, True), ("second_trip", LOSS_BIG, True)]


def loss_inputs(case, dtype=None):
    """z N(0, 1) (exact cases: -1 / 0 / 1, every partial sum of squares below 2^24); logs_partial N(0, 30); logdets N(0, 0.5); the
    buffers hold one NaN past n_logs / n_flows that the kernel must not read"""
    cid, m, n_logs, n_flows, sigma = case
    g = gen(_seed(cid))
    z = _ints((m, 8), -1, 1, g) if cid.startswith("exact") else torch.randn(m, 8, generator=g)
    lp, ld = torch.randn(n_logs + 1, generator=g) * 30, torch.randn(n_flows + 1, generator=g) * 0.5
    lp[n_logs], ld[n_flows] = float("nan"), float("nan")
    return {"case": case, "dtype": dtype, "z": z, "logs_partial": lp, "n_logs": n_logs, "logdets": ld, "n_flows": n_flows, "sigma": sigma}


def _loss_consts(inp):
    m = inp["z"].shape[0]
    sg = np.float32(inp["sigma"])
    i2s = np.float32(1.0) / (np.float32(2.0) * sg * sg)
    rows = np.float32(m)
    return i2s, rows, np.float32(1.0) / (rows * np.float32(8.0))


def loss_model(inp, fault=None):
    z = inp["z"]
    reach = _reach(2 * z.shape[0], fault)
    zz = z.reshape(-1, 4) if reach is None else z.reshape(-1, 4)[reach]
    i2s, rows, inv = _loss_consts(inp)
    a = np.float32((zz * zz).sum())
    b, d = np.float32(inp["logs_partial"][:inp["n_logs"]].sum()), np.float32(inp["logdets"][:inp["n_flows"]].sum())
    t = d if fault == "rows_dropped" else rows * d
    return {"loss": torch.tensor([float(np.float32(np.float32(np.float32(a * i2s) - b) - t) * inv)], dtype=F32)}


def loss_check(inp, got):
    z = widen(inp["z"])
    m = z.shape[0]
    i2s, rows, inv = _loss_consts(inp)
    A = (z * z).sum()
    if inp["case"][0].startswith("exact"):
        want = torch.tensor([float(np.float32(np.float32(float(A)) * i2s) * inv)], dtype=F32)
        return {"loss": _bitcmp(got["loss"].view(1), want)}
    G = grid(2 * m)
    Tt = -(-2 * m // (WG_BLOCK * G))
    lp, ld = widen(inp["logs_partial"][:inp["n_logs"]]), widen(inp["logdets"][:inp["n_flows"]])
    D_A, D_B, D_D = 5 * Tt + -(-G // 256) + 18, -(-inp["n_logs"] // 256) + 9, -(-inp["n_flows"] // 256) + 9
    sig = f32(inp["sigma"])
    i2, rw = 1.0 / (2.0 * sig * sig), float(rows)
    ic = 1.0 / (rw * 8.0)
    t1, t2, t3 = A * i2, lp.sum(), rw * ld.sum()
    loss = (t1 - t2 - t3) * ic
    e = ((D_A + 3) * U * t1 + D_B * U * lp.abs().sum() + (D_D + 1) * U * rw * ld.abs().sum() + 2 * U * (t1 + t2.abs() + t3.abs())) * ic + 2 * U * loss.abs()
    return {"loss": worst(got["loss"].view(1), loss.view(1), e.view(1))}


def dz_inputs(case, dtype=None):
    cid, m, has_scale = case
    return {"case": case, "dtype": dtype, "z": torch.randn(m, 8, generator=gen(_seed(cid))), "scale": torch.tensor([1024.0 / 3]) if has_scale else None,
            "coef": 1.0 / (0.7 * 0.7 * m * 8)}


def dz_model(inp, fault=None):
    fac = np.float32(1.0 if inp["scale"] is None else float(inp["scale"])) * np.float32(inp["coef"])
    dz = inp["z"] * float(fac)
    reach = _reach(2 * dz.shape[0], fault)
    if reach is not None:
        dz = torch.where(reach.repeat_interleave(4).view(-1, 8), dz, untouched((), F32))
    return {"dz": dz}


def dz_check(inp, got):
    ref = widen(inp["z"]) * ((1.0 if inp["scale"] is None else float(inp["scale"])) * f32(inp["coef"]))
    return {"dz": worst(got["dz"], ref, 2 * U * ref.abs() + TINY)}


# ================================================================================================ wg_weight_norm_fwd / bwd (+ batched)
WN_CASES = [   # id, Co, Ci, Kt, Cip
    ("n3", 5, 1, 3, 8), ("n63", 3, 21, 3, 24), ("n64", 4, 64, 1, 64), ("n65", 3, 13, 5, 16), ("n1920", 2, 640, 3, 640),
    ("exact_n64", 5, 16, 4, 24),
    ("t_128x64x3", 128, 64, 3, 64), ("t_64x4x1", 64, 4, 1, 8), ("t_64x3x1", 64, 3, 1, 8), ("t_128x640x1", 128, 640, 1, 640), ("t_16x80x8", 16, 80, 8, 80),
    ("t_1024x512x3", 1024, 512, 3, 512),
]
WN_TABLES = {   # entries: (Co, Ci, Kt, Cip, gain given)
    "single": [(7, 13, 5, 16, True)],
    "co1": [(3, 4, 1, 8, True), (1, 21, 3, 24, True), (5, 16, 4, 16, True)],
    "five": [(64, 4, 1, 8, True), (8, 64, 1, 64, False), (1, 64, 3, 64, True), (33, 80, 8, 80, True), (6, 64, 1, 64, False)],
}


def wn_case(cid):
    return next(c for c in WN_CASES if c[0] == cid)


def wn_inputs(case, dtype, gain=True, seed=0):
    """v N(0, 0.1), g 1 + N(0, 0.1), dw N(0, 1) in the GEMM layout [Co, Kt Cip] with N(0, 1) junk in the padding columns (which
    no gradient may read).  exact_n64: v = +-1, g = 8 (co + 1), dw integers in [-4, 4]."""
    cid, co, ci, kt, cip = case
    g = gen(_seed(cid) + seed)
    if str(cid).startswith("exact"):
        v = _ints((co, ci, kt), 0, 1, g) * 2 - 1
        gg, dw = 8.0 * torch.arange(1, co + 1).float(), _ints((co, kt * cip), -4, 4, g)
    else:
        v, gg, dw = torch.randn(co, ci, kt, generator=g) * 0.1, 1 + 0.1 * torch.randn(co, generator=g), torch.randn(co, kt * cip, generator=g)
    return {"case": case, "dtype": dtype, "v": v, "g": gg if gain else None, "dw": dw}


def _wn_layout(t, case, fault=None):
    """[Co, Ci, Kt] -> the GEMM layout [Co, Kt, Cip], zero padded"""
    _, co, ci, kt, cip = case
    out = torch.zeros(co, kt, cip, dtype=t.dtype)
    out[:, :, :ci] = t.reshape(co, kt, ci) if fault == "layout_swapped" else t.permute(0, 2, 1)
    return out.view(co, kt * cip)


def _wn_sumsq(inp, fault, work=F32):
    _, co, ci, kt, cip = inp["case"]
    v = inp["v"].to(work)
    if fault == "norm_over_padded_row":          # Kt Cip elements from the row's start: past its end into the next row (0 after the last)
        flat = torch.cat([v.reshape(-1), torch.zeros(kt * cip, dtype=work)])
        idx = torch.arange(co).view(-1, 1) * ci * kt + torch.arange(kt * cip).view(1, -1)
        return (flat[idx] ** 2).sum(1)
    return (v * v).sum((1, 2))


def wn_fwd_model(inp, fault=None):
    v, dt = inp["v"], inp["dtype"]
    f = inp["g"] / torch.sqrt(_wn_sumsq(inp, fault)) if inp["g"] is not None else torch.ones(v.shape[0])
    return {"w16": r16(_wn_layout(v * f.view(-1, 1, 1), inp["case"], fault), dt)}


def _wn_rel(n):
    return -(-n // 64) + 7


def wn_fwd_check(inp, got):
    _, co, ci, kt, cip = inp["case"]
    dt = inp["dtype"]
    if inp["g"] is None:
        return {"w16": _bitcmp(got["w16"], r16(_wn_layout(inp["v"], inp["case"]), dt))}
    v = widen(inp["v"])
    w = _wn_layout(v * (widen(inp["g"]) / v.flatten(1).norm(dim=1)).view(-1, 1, 1), inp["case"])
    real = _wn_layout(torch.ones(co, ci, kt), inp["case"]) > 0
    bar = stored(w, w.abs() * (_wn_rel(ci * kt) / 2 + C_SQRT + C_DIV + 1) * U, dt)
    if str(inp["case"][0]).startswith("exact"):
        bar = torch.zeros_like(bar)
    bar = torch.where(real, bar, torch.zeros(()))
    return {"w16": _worse(worst(got["w16"], w, bar), _bitcmp(got["w16"], torch.zeros(co, kt * cip, dtype=dt), ~real))}


def _wn_unlayout(dw, case, fault=None):
    """the GEMM layout [Co, Kt Cip] -> [Co, Ci, Kt]"""
    _, co, ci, kt, cip = case
    d = dw.view(co, kt, cip)[:, :, :ci]
    return d.reshape(co, ci, kt) if fault == "layout_swapped" else d.permute(0, 2, 1).contiguous()


def wn_bwd_model(inp, fault=None):
    v = inp["v"]
    dr = _wn_unlayout(inp["dw"], inp["case"], fault)
    if inp["g"] is None:
        return {"dv": dr.clone(), "dg": None}
    d = (dr * v).sum((1, 2))
    inv = 1.0 / torch.sqrt(_wn_sumsq(inp, fault))
    dv = (inp["g"] * inv).view(-1, 1, 1) * (dr - v * (d * inv * inv).view(-1, 1, 1))
    return {"dv": dv, "dg": d * inv}


def wn_bwd_check(inp, got):
    _, co, ci, kt, cip = inp["case"]
    dr = _wn_unlayout(inp["dw"], inp["case"])
    if inp["g"] is None:
        return {"dv": _bitcmp(got["dv"], dr)}
    v, dr, g = widen(inp["v"]), dr.double(), widen(inp["g"])
    L = _wn_rel(ci * kt)
    d, e_d = (dr * v).sum((1, 2)), L * U * (dr * v).abs().sum((1, 2))
    inv = 1 / v.flatten(1).norm(dim=1)
    r = (L / 2 + C_SQRT + C_DIV) * U
    dg = d * inv
    e_dg = e_d * inv + (r + U) * dg.abs()
    col = lambda t: t.view(-1, 1, 1)
    t = v * col(d * inv * inv)
    e_t = v.abs() * col(inv * inv * e_d) + (2 * r + 3 * U) * t.abs()
    dv = col(g * inv) * (dr - t)
    e_dv = col((g * inv).abs()) * (e_t + U * (dr - t).abs()) + (r + 2 * U) * dv.abs()
    if str(inp["case"][0]).startswith("exact"):
        e_dg, e_dv = torch.zeros_like(e_dg), torch.zeros_like(e_dv)
    return {"dv": worst(got["dv"], dv, e_dv), "dg": worst(got["dg"].reshape(-1), dg, e_dg)}


def wn_table_inputs(tid, dtype):
    ents = [wn_inputs(("%s%d" % (tid, k), co, ci, kt, cip), dtype, gain, seed=k) for k, (co, ci, kt, cip, gain) in enumerate(WN_TABLES[tid])]
    return {"case": tid, "dtype": dtype, "entries": ents}


def _wn_table(inp, fn, fault):
    """per-entry results; table_row_off_by_one: the binary search takes `<` for `<=`, so the first row of every entry but the first
    is handed to the entry before it as a row past its end and is never written"""
    outs = []
    for k, e in enumerate(inp["entries"]):
        o = fn(e, None if fault == "table_row_off_by_one" else fault)
        if fault == "table_row_off_by_one" and k > 0:
            for key in o:
                if o[key] is not None:
                    o[key] = o[key].clone()
                    o[key][0] = float("nan")
        outs.append(o)
    return outs


def wn_fwd_batched_model(inp, fault=None):
    return {"entries": _wn_table(inp, wn_fwd_model, fault)}


def wn_bwd_batched_model(inp, fault=None):
    return {"entries": _wn_table(inp, wn_bwd_model, fault)}


def _wn_table_check(inp, got, chk):
    """every entry against the per-tensor statement; the first and the last row of every entry once more by name (the binary
    search's edges)"""
    res = {}
    for e, o in zip(inp["entries"], got["entries"]):
        for key, r in chk(e, o).items():
            res[key] = _worse(res.get(key, (0.0, -1)), r)
        co = e["case"][1]
        for nm, row in (("first rows", 0), ("last rows", co - 1)):
            sub = dict(e, case=(e["case"][0], 1) + tuple(e["case"][2:]), v=e["v"][row:row + 1], dw=e["dw"][row:row + 1],
                       g=None if e["g"] is None else e["g"][row:row + 1])
            one = {k: (None if t is None else t.reshape(co, -1)[row:row + 1].reshape((1,) + tuple(t.shape[1:]))) for k, t in o.items()}
            for key, r in chk(sub, one).items():
                res["%s, %s" % (key, nm)] = _worse(res.get("%s, %s" % (key, nm), (0.0, -1)), r)
    return res


def wn_fwd_batched_check(inp, got):
    return _wn_table_check(inp, got, wn_fwd_check)


def wn_bwd_batched_check(inp, got):
    return _wn_table_check(inp, got, wn_bwd_check)


# ================================================================================================ wg_upsample_weight / bwd
UPSAMPLE_CASES = [(3, 6, 6), (8, 16, 4), (80, 1024, 256)]      # Cm, ksize, stride; the last: 6 553 600 elements, 7 trips


def upsample_inputs(case, dtype):
    cm, ks, st = case
    g = gen(_seed(case))
    w = torch.randn(cm, cm, ks, generator=g) * 0.01
    w.view(-1)[:4] = torch.tensor([INF, -0.0, 65520.0, 2.0 ** -25])
    return {"case": case, "dtype": dtype, "w": w, "bias": torch.randn(cm, generator=g), "db": torch.randn(st * cm, (ks // st) * cm, generator=g)}


def _up_perm(case, fault=None):
    """index [r, co, j, ci] -> flat index of w[ci, co, r + stride j]"""
    cm, ks, st = case
    nt = ks // st
    r, co, j, ci = torch.meshgrid(torch.arange(st), torch.arange(cm), torch.arange(nt), torch.arange(cm), indexing="ij")
    k = r * nt + j if fault == "phase_tap_swapped" else r + st * j
    return ((ci * cm + co) * ks + k).reshape(-1)


def upsample_model(inp, fault=None):
    cm, ks, st = inp["case"]
    idx = _up_perm(inp["case"], fault)
    b16 = r16(inp["w"].reshape(-1)[idx], inp["dtype"])
    reach = _reach(idx.numel(), fault)
    if reach is not None:
        b16 = torch.where(reach, b16, untouched((), inp["dtype"]))
    return {"b16": b16.view(st * cm, (ks // st) * cm), "bias_rep": inp["bias"].repeat(st)}


def upsample_check(inp, got):
    want = upsample_model(inp)
    return {"b16": _bitcmp(got["b16"], want["b16"]), "bias_rep": _bitcmp(got["bias_rep"], want["bias_rep"])}


def upsample_bwd_model(inp, fault=None):
    cm, ks, st = inp["case"]
    idx = _up_perm(inp["case"], fault)
    dw = torch.zeros(cm * cm * ks)
    dw[idx] = inp["db"].reshape(-1)
    reach = _reach(idx.numel(), fault)
    if reach is not None:
        dw = torch.where(reach, dw, untouched((), F32))
    return {"dw": dw.view(cm, cm, ks)}


def upsample_bwd_check(inp, got):
    return {"dw": _bitcmp(got["dw"], upsample_bwd_model(inp)["dw"])}


# ================================================================================================ wg_flow_inv / wg_flow_inv_first
FLOW_CASES = [   # id, M, c, early, z_col, next_c (0: no a0), out aliases state
    ("m1_c8", 1, 8, 0, 0, 8, False), ("m255_c6_e2_z0", 255, 6, 2, 0, 8, True), ("m257_c4_e2_z2", 257, 4, 2, 2, 6, False),
    ("m1000_c2_e2_z6", 1000, 2, 2, 6, 4, True), ("m1000_c4_same", 1000, 4, 0, 0, 4, False), ("m257_c6_noa0", 257, 6, 0, 0, 0, True),
    ("m255_c2_plus2", 255, 2, 0, 0, 4, False), ("second_trip_c6_e2", ROW_BIG, 6, 2, 2, 8, True),
]
FLOW_FIRST_CASES = [("m1_c2", 1, 2, True), ("m255_c4", 255, 4, True), ("m257_c6", 257, 6, False), ("m1000_c8", 1000, 8, True),
                    ("second_trip_c4", ROW_BIG, 4, True)]
FLOW_SIGMA = 0.6


def flow_inputs(case, dtype):
    """state N(0, 1); o = (b | log_s N(0, 0.5) with +-4 planted | junk); W^-T of a well conditioned matrix; noise N(0, 1)"""
    cid, m, c, early, z_col, next_c, alias = case
    nh = c // 2
    g = gen(_seed(cid))
    state, o, noise = (torch.randn(m, 8, generator=g) for _ in range(3))
    o[:, nh:c] *= 0.5
    o[0, nh], o[m - 1, c - 1] = 4.0, -4.0
    W = _mix_matrix(c, g)
    return {"case": case, "dtype": dtype, "c": c, "state": state, "o": o, "noise": noise, "sigma": FLOW_SIGMA,
            "winv_t": torch.linalg.inv(W.double()).t().contiguous().float()}


def _sig_noise(inp, cols):
    """sigma noise as ONE fp32 product"""
    return inp["noise"][:, cols] * float(np.float32(inp["sigma"]))


def _next_a0(out, next_c, dt):
    return _pad16(out[:, 8 - next_c:8 - next_c + next_c // 2], dt)


def flow_model(inp, fault=None):
    cid, m, c, early, z_col, next_c, alias = inp["case"]
    off, nh, dt = 8 - c, c // 2, inp["dtype"]
    x, o = inp["state"].clone(), inp["o"]
    x[:, off + nh:] = (x[:, off + nh:] - o[:, :nh]) * torch.exp(-o[:, nh:c])
    wi = inp["winv_t"] if fault == "winv_not_transposed" else inp["winv_t"].t()
    out = x.clone()
    out[:, off:] = x[:, off:] @ wi.t()
    if early:
        zc = 0 if fault == "wrong_noise_column" else z_col
        out[:, off - early:off] = _sig_noise(inp, slice(zc, zc + early))
    reach = _reach(m, fault)
    res = {"out": _rows(reach, out, inp["state"] if alias else untouched((), F32)), "a0": None}
    if next_c:
        res["a0"] = _rows(reach, _next_a0(out, next_c, dt), untouched((), dt))
    return res


def flow_check(inp, got, _share=False):
    cid, m, c, early, z_col, next_c, alias = inp["case"]
    off, nh, dt = 8 - c, c // 2, inp["dtype"]
    x, o, wi = widen(inp["state"]), widen(inp["o"]), widen(inp["winv_t"]).t()
    x1 = (x[:, off + nh:] - o[:, :nh]) * torch.exp(-o[:, nh:c])
    xa, d_x = torch.cat([x[:, off:off + nh], x1], 1), torch.cat([torch.zeros(m, nh, dtype=F64), (2 + C_EXPF) * U * x1.abs()], 1)
    ref = xa @ wi.t()
    bar = 8 * U * (xa.abs() @ wi.abs().t()) + d_x @ wi.abs().t() + TINY
    res = {"out": worst(got["out"][:, off:], ref, bar), "out pass-through": _bitcmp(got["out"][:, :off - early], inp["state"][:, :off - early])}
    share = (C_EXPF * U * torch.cat([torch.zeros(m, nh, dtype=F64), x1.abs()], 1) @ wi.abs().t()) / bar
    rr = ratio(got["out"][:, off:], ref, bar)
    top = share >= 0.9 * share.max()
    res["out, largest C_EXPF share"] = (float(rr[top].max()), int(torch.nonzero(top.reshape(-1))[0]))
    if _share:
        return float(share.max())
    if early:
        res["out early"] = _bitcmp(got["out"][:, off - early:off], _sig_noise(inp, slice(z_col, z_col + early)))
    if next_c:
        res["a0"] = _bitcmp(got["a0"], _next_a0(got["out"], next_c, dt))
    return res


def flow_first_inputs(case, dtype):
    cid, m, c, has_a0 = case
    return {"case": case, "dtype": dtype, "c": c, "noise": torch.randn(m, 8, generator=gen(_seed(cid))), "sigma": FLOW_SIGMA}


def flow_first_model(inp, fault=None):
    cid, m, c, has_a0 = inp["case"]
    out = torch.zeros(m, 8)
    out[:, 8 - c:] = _sig_noise(inp, slice(1, c + 1) if fault == "wrong_noise_column" and c < 8 else slice(0, c))
    reach = _reach(m, fault)
    return {"out": _rows(reach, out, untouched((), F32)), "a0": _rows(reach, _next_a0(out, c, inp["dtype"]), untouched((), inp["dtype"])) if has_a0 else None}


def flow_first_check(inp, got):
    want = flow_first_model(inp)
    res = {"out": _bitcmp(got["out"], want["out"])}
    if inp["case"][3]:
        res["a0"] = _bitcmp(got["a0"], _next_a0(got["out"], inp["c"], inp["dtype"]))
    return res


# ================================================================================================ dispatch
KERNELS = {
    "taps": (taps_model, taps_check), "taps_bwd": (taps_bwd_model, taps_bwd_check),
    "gate_fwd": (gate_fwd_model, gate_fwd_check), "gate_bwd": (gate_bwd_model, gate_bwd_check),
    "invconv_fwd": (invconv_fwd_model, invconv_fwd_check), "invconv_bwd": (invconv_bwd_model, invconv_bwd_check),
    "logdet_inv": (logdet_model, logdet_check), "logdet_inv_batched": (logdet_batched_model, logdet_batched_check),
    "coupling_fwd": (coupling_fwd_model, coupling_fwd_check), "coupling_bwd": (coupling_bwd_model, coupling_bwd_check),
    "loss": (loss_model, loss_check), "dz_init": (dz_model, dz_check),
    "weight_norm_fwd": (wn_fwd_model, wn_fwd_check), "weight_norm_bwd": (wn_bwd_model, wn_bwd_check),
    "weight_norm_fwd_batched": (wn_fwd_batched_model, wn_fwd_batched_check), "weight_norm_bwd_batched": (wn_bwd_batched_model, wn_bwd_batched_check),
    "upsample_weight": (upsample_model, upsample_check), "upsample_weight_bwd": (upsample_bwd_model, upsample_bwd_check),
    "flow_inv": (flow_model, flow_check), "flow_inv_first": (flow_first_model, flow_first_check),
}


def kernel_model(kernel, inp, fault=None):
    """The kernel's arithmetic in float32 on the CPU; fault: one of FAULTS, planted where the kernel has the corresponding code; a
    fault the kernel has no place for changes nothing."""
    assert fault is None or fault in FAULTS
    return KERNELS[kernel][0](inp, fault)


def check(kernel, inp, got):
    """-> {output: (largest ratio, flat index)}; every element of every output takes part"""
    return KERNELS[kernel][1](inp, got)
