"""float64 statements, derived per-element bars, input builders, case tables and a faulty float32 model for the twelve training
kernels of csrc/tacotron2.hip (the decoder-step launches -- its inference section and the cell fused into the gates product,
dle_t2_lstm_gemm_fwd -- have theirs in tests/_tacotron2_step_reference.py, on this module's helpers): t2_tanh, t2_lstm_{fwd,bwd}<DT, VEC = true | false>,
t2_attention_{fwd,bwd} without and with the fused location term (wloc / wlocT), t2_location_bwd, t2_mel_loss (+ t2_sum), t2_mask_rows,
t2_sum_steps.  tests/ only: no GPU and no ctypes in here.  The helpers (U, ulp, stored, ratio, worst, bits, same_cast, gen, C_EXP,
C_RCP) are those of tests/_smallops_reference.py.

Shape of the module.  For every kernel K:
    K_inputs(case, dtype) -> dict of CPU tensors, exactly as the kernel sees them (16-bit, fp32, u8, int64) + the base values of
                             every accumulated output;
    K_model(inp, fault)   -> dict of outputs: the kernel's arithmetic in float32 on the CPU in a plausible order, a correctly rounded
                             exp and an exact reciprocal where the hardware approximates; `fault` plants one error (FAULTS);
    K_check(inp, got)     -> {output name: (largest |got - ref| / bar, flat index)} over EVERY element of every output; outputs
                             without a bar (copies, zeros, flags, casts, 16-bit roundings of a returned fp32 value) are compared bit
                             for bit and report 0 or inf.
kernel_model(kernel, inp, fault=None) and check(kernel, inp, got) dispatch on the kernel's name.  The pass condition is ratio <= 1.

Bars.  u = 2^-24 is one fp32 rounding.  A sum of n terms in an order the test does not assume: (n - 1) u sum|term|, and u |term| for
each term that is itself a rounded product.  A 16-bit store: half a ulp at the far end of the fp32 bar (stored()).  An MFMA
accumulation over K: K u sum|a_i b_i| (16-bit products are exact in fp32).  1.0f / x is an IEEE division (u).
  __expf(a) = exp2(a log2 e): relative E(|a|) = (2.25 |a| + C_EXP) u (derived in _smallops_reference); below 2^-126 the error is absolute.
  t2_sigmoid(x) = 1 / (1 + __expf(-x)) = s:  |ds| <= s [ (1 - s) E(|x|) + 2 u ] + 2^-126            (the sum 1 + e and the division)
  fast_tanh(x) = 1 - 2 rcp(exp2(2 x log2 e) + 1): S.fast_tanh_delta(x, dx), for an argument already off by dx (absolute):
      2 / (e + 1) [ e / (e + 1) (2 dx + (2.5 |x| + C_EXP) u) + (1 + C_RCP) u ] + u |tanh x|
    Near 0 the result is the CANCELLATION 1 - (1 - x): the error there is ABSOLUTE, (C_EXP / 2 + 1 + C_RCP) u = 5 u with the measured
    constants, however small tanh x is -- a relative bar would be wrong by any factor.  At saturation it is u.
    (C_RCP was 2 u until the first GPU run of this module's test: the LSTM cell state's elements whose bar is at least half made of
    the two constants stood at 0.505 / 0.493 (fp16 / bf16); 3 u brought them to 0.410 / 0.400.  lstm_*_check record that figure.)
  t2_tanh uses the library's tanhf: 2 ulp = 4 u relative, and 2^-126 absolute (an fp32 subnormal may be flushed).

Staged statements.  Where a kernel rounds an intermediate to 16 bits and goes on from the rounded value, the downstream reference
is computed from the GOT intermediate (a tie broken the other way moves the result by far more than the fp32 bar):
  attention fwd   tanh_out against fp64 from the inputs (with the fused location term when wloc is given); aw_out against the fp64
                  masked softmax of v . tanh_out_got; awc_next BIT FOR BIT = (r16(aw_got), r16(fp32(prev_cum) + aw_got), 0 x 6) in fp32
                  on the CPU; the contexts against sum_t aw_got[t] memory[t]; every destination the same bits; aw_out exactly 0 at
                  t >= len.
  attention bwd   from the inputs; with wlocT, d_prev and the d_cum addend from the returned 16-bit d_pl; dq16 = r16(dq_got) when dq is
                  returned; dctx16 = r16 of the fp32 sum of the pieces; dv_acc, d_pm_acc, d_memory, d_cum as got - base against the
                  ADDEND with the addend's bar + u |base + addend| (the final add).
  lstm fwd        activations in place against fp64; c_out and h from the UNROUNDED activations (as the kernel uses them), so their
                  bars carry the activations' fp32 errors, not the 16-bit store's.
Detailed derivations sit in each check's docstring.

A text length of 0 makes the softmax 0 / 0 (NaN weights), here as in the reference model (masked_fill(-inf) + softmax); no caller
passes it (the collate function sorts by length >= 1) and no case uses it.
"""
import numpy as np
import torch

from tests import _smallops_reference as S

F64, F32, F16, BF16, U8 = S.F64, S.F32, S.F16, S.BF16, S.U8
U, TINY, C_EXP, C_RCP = S.U, S.TINY, S.C_EXP, S.C_RCP
ulp, stored, ratio, worst, bits, same_cast, gen, widen, name, f32 = (S.ulp, S.stored, S.ratio, S.worst, S.bits, S.same_cast, S.gen,
                                                                     S.widen, S.name, S.f32)
INF = float("inf")
T2_BLOCK, T2_CAP, LSTM_BLOCK, LSTM_CAP, T2A_BLOCK = 256, 1024, 128, 2048, 1024
LOG2E2 = float(np.float32(2.885390081777927))

FAULTS = ("cum_without_w", "mask_off_by_one", "inactive_lanes_counted", "energy_from_unrounded_tanh", "loc_pad_shift",
          "loc_rows_past_ti_live", "keep_bit_reversed", "keep_index_dropped", "live_ignored", "dv_overwritten", "dcum_overwritten",
          "second_trip_skipped", "tail_steps_skipped")


def r16(x, dtype):
    """fp32 -> 16-bit, round to nearest even (the kernels' Elem<DT>::from_f32)"""
    return x.float().to(dtype)


def pow2_ge(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def inv_keep(p):
    """tacotron2/ops.py inv_keep, as the C `float` parameter carries it"""
    thr = min(max(int(p * 65536.0 + 0.5), 0), 65535)
    return f32(65536.0 / (65536 - thr))


def exp_rel(d):
    return (2.25 * d + C_EXP) * U


def sigmoid_ref(x):
    """-> (s, |ds|) of t2_sigmoid in fp32 (docstring above)"""
    s = torch.sigmoid(x)
    return s, s * ((1 - s) * exp_rel(x.abs()) + 2 * U) + TINY


def tanh_ref(x, dx):
    return torch.tanh(x), S.fast_tanh_delta(x, dx)


def _bitcmp(got, want, mask=None):
    """(0 | inf, first differing flat index): bit equality, over the rows of `mask` when given"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return INF, 0
    a, b = bits(got.contiguous()), bits(want.contiguous())
    d = a != b
    if mask is not None:
        d = d & mask.expand_as(d)
    if bool(d.any()):
        return INF, int(torch.nonzero(d.reshape(-1))[0])
    return 0.0, -1


def _no_const(fn):
    """fn() with the measured constants C_EXP, C_RCP at 0: the part of a bar that is derived from roundings alone"""
    global C_EXP, C_RCP
    kept = (S.C_EXP, S.C_RCP, C_EXP, C_RCP)
    S.C_EXP = S.C_RCP = C_EXP = C_RCP = 0.0
    try:
        return fn()
    finally:
        S.C_EXP, S.C_RCP, C_EXP, C_RCP = kept


def _const_dominated(got, raw, raw0):
    """largest ratio over the elements whose bar is at least half made of C_EXP / C_RCP: the figure the rule `measured constants
    leave what they dominate at or below 0.5` applies to (a second record; the full comparison leaves no element out)"""
    (ref, bar), (_, bar0) = raw, raw0
    r = ratio(got, ref, bar)
    r = torch.where(bar0.expand_as(r) <= 0.5 * bar.expand_as(r), r, torch.zeros_like(r)).reshape(-1)
    i = int(torch.argmax(r))
    return float(r[i]), i


def _worse(a, b):
    return a if a[0] >= b[0] else b


def _f32model_tanh(x):
    e = torch.exp2(x * np.float32(LOG2E2))
    return 1.0 - 2.0 * (1.0 / (e + 1.0))


def _f32model_sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def untouched(shape, dtype):
    """what an output buffer holds before the launch (the GPU test's guard pattern): NaN"""
    return torch.full(shape, float("nan"), dtype=dtype)


# ================================================================================================ t2_tanh
def tanh_inputs(case, dtype):
    """a grid of exponents from the smallest subnormal of `dtype` to saturation (three mantissas, both signs), +-0, +-inf, NaN"""
    lo = -24 if dtype == F16 else -133
    k = torch.arange(lo, 5, dtype=F64)
    v = torch.cat([torch.pow(2.0, k) * m for m in (1.0, 1.25, 1.984375)])
    v = torch.cat([v, -v, torch.tensor([0.0, -0.0, INF, -INF, float("nan"), 9.0, -9.0, 0.5493, 65504.0, -65504.0], dtype=F64)])
    return {"x": v.to(dtype), "dtype": dtype}


def tanh_model(inp, fault=None):
    return {"y": r16(torch.tanh(inp["x"].float()), inp["dtype"])}


def tanh_check(inp, got):
    """y = r16(tanhf(x)): bar = ulp16 / 2 + 4 u |tanh x| + 2^-126 (the library's 2 ulp; a subnormal fp32 result may be flushed);
    tanh(+-inf) = +-1 and NaN -> NaN by class (ratio()); path: one block, no grid-stride trip."""
    x = widen(inp["x"])
    ref = torch.tanh(x)
    fin = torch.isfinite(x)
    bar = torch.where(fin, stored(torch.nan_to_num(ref), 4 * U * torch.nan_to_num(ref).abs() + TINY, inp["dtype"]), torch.zeros_like(ref))
    return {"y": worst(got["y"], ref, bar)}


# ================================================================================================ t2_lstm_fwd / bwd
LSTM_CASES = [   # id, B, H, dropout p, live, keep_index, gates offset (elements), route, extra dh pieces, dgates aliases act
    ("scalar_h20", 3, 20, 0.1, False, 0, 0, "scalar", 0, True),
    ("scalar_keepindex4", 5, 32, 0.1, True, 4, 0, "scalar", 1, False),
    ("scalar_unaligned", 4, 64, None, True, 0, 2, "scalar", 2, True),
    ("vec_h8", 3, 8, 0.1, True, 0, 0, "vec", 0, False),
    ("vec_strided_h96", 7, 96, 0.1, True, 8 * 5, 0, "vec", 2, True),
    ("vec_second_trip", 2064, 1024, 0.1, False, 0, 0, "vec", 1, False),
]


def lstm_route(h, keep_index, offset):
    """the launcher's choice: vector kernel only for H % 8 == 0, keep_index % 8 == 0 and 16-byte aligned views"""
    return "vec" if h % 8 == 0 and keep_index % 8 == 0 and offset % 8 == 0 else "scalar"


def lstm_items(case):
    _, b, h, p, live, kidx, off, route = case[:8]
    return b * (h // 8 if route == "vec" else h)


def lstm_inputs(case, dtype):
    """gates N(0, 1.5) with +-20, +-1e-3, 0 planted; c_prev N(0, 1) with +-6; keep bits random at p with whole bytes of 0x00 and
    0xFF; live random with at least one row of each kind; h_prev, dh pieces, dc_next N(0, 1)."""
    cid, b, h, p, live, kidx, off, route, nextra, alias = case
    assert lstm_route(h, kidx, off) == route
    g = gen(1000 + b * 7 + h)
    gates = torch.randn(b, 4 * h, generator=g) * 1.5
    sp = torch.tensor([20.0, -20.0, 1e-3, -1e-3, 0.0, 9.0, -9.0, 3e-5])
    m = min(sp.numel(), h)
    for q in range(4):
        gates[0, q * h:q * h + m] = sp[:m].roll(q)
    c_prev = torch.randn(b, h, generator=g)
    c_prev[b - 1, :min(h, 4)] = torch.tensor([6.0, -6.0, 0.0, 1e-4])[:min(h, 4)]
    inp = {"case": case, "dtype": dtype, "B": b, "H": h, "gates": gates.to(dtype), "c_prev": c_prev, "keep": None, "keep_index": kidx,
           "inv_keep": 1.0, "live": None, "h_prev": None, "alias": alias}
    if p is not None:
        nbytes = (kidx + b * h + 7) // 8 + 3
        kb = (torch.rand(nbytes * 8, generator=g) >= 0.3).view(-1, 8)     # (dropped more often than p: 60 bits at 0.1 can all be kept)
        kb[(kidx // 8 + 1) % nbytes] = False          # a whole byte 0x00
        kb[(kidx // 8 + 2) % nbytes] = True           # and one 0xFF
        w = (1 << torch.arange(8, dtype=torch.int32))
        inp["keep"] = (kb.to(torch.int32) * w).sum(1).to(U8)
        inp["inv_keep"] = inv_keep(p)
    if live:
        lv = (torch.rand(b, generator=g) > 0.4).float()
        lv[0], lv[b - 1] = 1.0, 0.0
        inp["live"] = lv
        inp["h_prev"] = torch.randn(b, h, generator=g).to(dtype)
    inp["dh"] = [torch.randn(b, h, generator=g) for _ in range(1 + nextra)]
    inp["dc_next"] = torch.randn(b, h, generator=g)
    return inp


def _keep_mask(inp, fault=None):
    """[B, H] bool from the packed bits: bit e of the mask <-> element keep_index + b H + j"""
    b, h = inp["B"], inp["H"]
    if inp["keep"] is None:
        return None
    e = (0 if fault == "keep_index_dropped" else inp["keep_index"]) + torch.arange(b * h)
    sh = e & 7
    if fault == "keep_bit_reversed":
        sh = 7 - sh
    return (((inp["keep"][e >> 3].to(torch.int32) >> sh.to(torch.int32)) & 1) == 1).view(b, h)


def _trip_mask(items_per_row, rows, width, cap_items, fault):
    """elements [rows, items_per_row * width] a one-trip-only kernel would reach (fault second_trip_skipped), else None"""
    if fault != "second_trip_skipped" or rows * items_per_row <= cap_items:
        return None
    reach = torch.arange(rows * items_per_row) < cap_items
    return reach.view(rows, items_per_row, 1).expand(rows, items_per_row, width).reshape(rows, items_per_row * width)


def lstm_fwd_model(inp, fault=None):
    dt, b, h = inp["dtype"], inp["B"], inp["H"]
    gx = inp["gates"].float()
    gi, gf, go = (_f32model_sigmoid(gx[:, q * h:(q + 1) * h]) for q in (0, 1, 3))
    gg = _f32model_tanh(gx[:, 2 * h:3 * h])
    c = gf * inp["c_prev"] + gi * gg
    hh = go * _f32model_tanh(c)
    km = _keep_mask(inp, fault)
    if km is not None:
        hh = torch.where(km, hh * np.float32(inp["inv_keep"]), torch.zeros(()))
    out = {"act": r16(torch.cat([gi, gf, gg, go], 1), dt), "out_dst": None}
    if inp["live"] is not None:
        dead = (inp["live"] == 0).view(b, 1)
        out["out_dst"] = r16(torch.where(dead, torch.zeros(()), hh), dt)
        if fault != "live_ignored":
            c = torch.where(dead, inp["c_prev"], c)
            out["c_out"], out["h"] = c, torch.where(dead, inp["h_prev"], r16(hh, dt))
    if "h" not in out:
        out["c_out"], out["h"] = c, r16(hh, dt)
    w = 8 if inp["case"][7] == "vec" else 1
    reach = _trip_mask(h // w, b, w, LSTM_CAP * LSTM_BLOCK, fault)
    if reach is not None:
        out["act"] = torch.where(reach.repeat(1, 4), out["act"], inp["gates"])
        out["c_out"] = torch.where(reach, out["c_out"], untouched((b, h), F32))
        out["h"] = torch.where(reach, out["h"], untouched((b, h), dt))
    out["h_dsts"] = [out["h"], out["h"].clone()]
    return out


def lstm_fwd_check(inp, got, _raw=False):
    """got: act [B, 4H] (the gates buffer after the call), c_out fp32, h_dsts (list of [B, H]), out_dst or None.
    i, f, o = t2_sigmoid, g = fast_tanh of the exact 16-bit gates (bars above, stored()).  From the UNROUNDED activations:
      c = f c_prev + i g:  |dc| <= df |c_prev| + di |g| + dg |i| + 2 u (|f c_prev| + |i g|)      (two products, the sum; an fma has less)
      h = o fast_tanh(c):  |dh| <= do |tanh c| + |o| delta(c, dc) + u |h|;  kept: x inv_keep, + u |h inv_keep|;  dropped: exactly 0.
    c_out fp32: bar dc.  h destinations: stored(h, dh), all destinations the same bits.  live == 0 rows: c_out bit-equal to c_prev,
    the destinations bit-equal to h_prev, out_dst exactly +0; out_dst of a live row bit-equal to h."""
    dt, b, h = inp["dtype"], inp["B"], inp["H"]
    gx = widen(inp["gates"])
    (i, di), (f, df), (o, do) = (sigmoid_ref(gx[:, q * h:(q + 1) * h]) for q in (0, 1, 3))
    g, dg = tanh_ref(gx[:, 2 * h:3 * h], torch.zeros(()))
    cp = widen(inp["c_prev"])
    c = f * cp + i * g
    dc = df * cp.abs() + di * g.abs() + dg * i.abs() + 2 * U * ((f * cp).abs() + (i * g).abs())
    tc, dtc = tanh_ref(c, dc)
    hh = o * tc
    dh = do * tc.abs() + o.abs() * dtc + U * hh.abs()
    km = _keep_mask(inp)
    if km is not None:
        ik = inp["inv_keep"]
        hh, dh = torch.where(km, hh * ik, torch.zeros(())), torch.where(km, dh * ik + U * (hh * ik).abs(), torch.zeros(()))
    act = torch.cat([i, f, g, o], 1)
    res = {"act": worst(got["act"], act, stored(act, torch.cat([di, df, dg, do], 1), dt))}
    hbar, cbar = stored(hh, dh, dt), dc
    live = torch.ones(b, 1, dtype=torch.bool)
    if inp["live"] is not None:
        live = (inp["live"] != 0).view(b, 1)
        cbar = torch.where(live, cbar, torch.zeros(()))
        c = torch.where(live, c, cp)
        hbar = torch.where(live, hbar, torch.zeros(()))
        hh = torch.where(live, hh, widen(inp["h_prev"]))
    if _raw:
        return c, cbar
    res["c_out"] = _worse(worst(got["c_out"], c, cbar), _bitcmp(got["c_out"], inp["c_prev"], ~live))
    res["c_out, constants >= half the bar"] = _const_dominated(got["c_out"], (c, cbar), _no_const(lambda: lstm_fwd_check(inp, got, True)))
    rh = worst(got["h_dsts"][0], hh, hbar)
    if inp["live"] is not None:
        rh = _worse(rh, _bitcmp(got["h_dsts"][0], inp["h_prev"], ~live))
        ro = _bitcmp(got["out_dst"], got["h_dsts"][0], live)
        res["out_dst"] = _worse(ro, _bitcmp(got["out_dst"], torch.zeros(b, h, dtype=dt), ~live))
    for d in got["h_dsts"][1:]:
        rh = _worse(rh, _bitcmp(d, got["h_dsts"][0]))
    res["h"] = rh
    return res


def lstm_bwd_inputs(case, dtype):
    """the forward model's saved activations + dh pieces, dc_next"""
    inp = lstm_inputs(case, dtype)
    inp["act"] = lstm_fwd_model(inp)["act"]
    return inp


def _sum32(pieces):
    s = pieces[0].float()
    for p in pieces[1:]:
        s = s + p.float()
    return s


def lstm_bwd_model(inp, fault=None):
    dt, b, h = inp["dtype"], inp["B"], inp["H"]
    a = inp["act"].float()
    gi, gf, gg, go = (a[:, q * h:(q + 1) * h] for q in range(4))
    dhv = _sum32(inp["dh"])
    g = dhv
    km = _keep_mask(inp, fault)
    if km is not None:
        g = torch.where(km, g * np.float32(inp["inv_keep"]), torch.zeros(()))
    cp, dcn = inp["c_prev"], inp["dc_next"]
    tc = _f32model_tanh(gf * cp + gi * gg)
    d_o = g * tc
    dc = dcn + g * go * (1.0 - tc * tc)
    di, df = dc * gg * gi * (1.0 - gi), dc * cp * gf * (1.0 - gf)
    dg, dog = dc * gi * (1.0 - gg * gg), d_o * go * (1.0 - go)
    dcp = dc * gf
    out = {"dh_prev": None}
    if inp["live"] is not None:
        dead = (inp["live"] == 0).view(b, 1)
        if fault != "live_ignored":
            z = torch.zeros(())
            di, df, dg, dog = (torch.where(dead, z, t) for t in (di, df, dg, dog))
            dcp = torch.where(dead, dcn, dcp)
        out["dh_prev"] = torch.where(dead, dhv, torch.zeros(()))
    out["dgates"], out["dc_prev"] = r16(torch.cat([di, df, dg, dog], 1), dt), dcp
    w = 8 if inp["case"][7] == "vec" else 1
    reach = _trip_mask(h // w, b, w, LSTM_CAP * LSTM_BLOCK, fault)
    if reach is not None:
        out["dgates"] = torch.where(reach.repeat(1, 4), out["dgates"], inp["act"] if inp["alias"] else untouched((b, 4 * h), dt))
        out["dc_prev"] = torch.where(reach, dcp, untouched((b, h), F32))
    return out


def lstm_bwd_check(inp, got, _raw=False):
    """From the saved 16-bit activations (exact in fp32), dhv = (dh + dh1) + dh2 summed on load: e_dhv = (pieces - 1) u sum|piece|.
      g = dhv inv_keep (kept; + u |g|) or exactly 0;  c = f c_prev + i gg: 2 u (|f c_prev| + |i gg|);  tc = fast_tanh(c): delta(c, dc)
      d_o = g tc: e_g |tc| + |g| delta + u |d_o|
      om = 1 - tc^2: e_om = 2 |tc| delta + u tc^2 + u |om|;  T = g o om: e_T = e_g |o om| + |g o| e_om + 2 u |T|
      dc = dc_next + T: e_dc = e_T + u (|dc_next| + |T|)
      di = dc gg i (1 - i): e_dc |gg i (1 - i)| + 4 u |di|      df = dc c_prev f (1 - f): likewise
      dg = dc i (1 - gg^2): e_dc |i (1 - gg^2)| + |dc i| (u gg^2 + u |1 - gg^2|) + 2 u |dg|
      do = d_o o (1 - o): e_do |o (1 - o)| + 3 u |do|           dc_prev = dc f: e_dc |f| + u |dc_prev| (fp32)
    live == 0 rows: the four gate gradients exactly 0, dc_prev bit-equal to dc_next, dh_prev bit-equal to the fp32 sum of the pieces;
    live rows: dh_prev exactly +0.  Without `live` dh_prev is not written."""
    dt, b, h = inp["dtype"], inp["B"], inp["H"]
    a = widen(inp["act"])
    gi, gf, gg, go = (a[:, q * h:(q + 1) * h] for q in range(4))
    pcs = [widen(p) for p in inp["dh"]]
    dhv = sum(pcs)
    e_g = (len(pcs) - 1) * U * sum(p.abs() for p in pcs)
    g = dhv
    km = _keep_mask(inp)
    if km is not None:
        ik = inp["inv_keep"]
        g = torch.where(km, dhv * ik, torch.zeros(()))
        e_g = torch.where(km, e_g * ik + U * g.abs(), torch.zeros(()))
    cp, dcn = widen(inp["c_prev"]), widen(inp["dc_next"])
    c = gf * cp + gi * gg
    tc, dl = tanh_ref(c, 2 * U * ((gf * cp).abs() + (gi * gg).abs()))
    d_o = g * tc
    e_do = e_g * tc.abs() + g.abs() * dl + U * d_o.abs()
    om = 1 / torch.cosh(c) ** 2
    e_om = 2 * tc.abs() * dl + U * tc * tc + U * om
    T = g * go * om
    e_dc = e_g * (go * om).abs() + (g * go).abs() * e_om + 2 * U * T.abs() + U * (dcn.abs() + T.abs())
    dc = dcn + T
    di, df = dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf)
    e_di, e_df = e_dc * (gg * gi * (1 - gi)).abs() + 4 * U * di.abs(), e_dc * (cp * gf * (1 - gf)).abs() + 4 * U * df.abs()
    dg = dc * gi * (1 - gg * gg)
    e_dg = e_dc * (gi * (1 - gg * gg)).abs() + (dc * gi).abs() * (U * gg * gg + U * (1 - gg * gg).abs()) + 2 * U * dg.abs()
    dog = d_o * go * (1 - go)
    e_dog = e_do * (go * (1 - go)).abs() + 3 * U * dog.abs()
    dcp = dc * gf
    e_dcp = e_dc * gf.abs() + U * dcp.abs()
    ref, err = torch.cat([di, df, dg, dog], 1), torch.cat([e_di, e_df, e_dg, e_dog], 1)
    bar = stored(ref, err, dt)
    res = {}
    if inp["live"] is not None:
        live = (inp["live"] != 0).view(b, 1)
        ref, bar = torch.where(live, ref, torch.zeros(())), torch.where(live, bar, torch.zeros(()))
        dcp, e_dcp = torch.where(live, dcp, dcn), torch.where(live, e_dcp, torch.zeros(()))
        want = torch.where(live, torch.zeros(()), _sum32(inp["dh"]))
        res["dh_prev"] = _bitcmp(got["dh_prev"], want)
        res["dc_prev"] = _bitcmp(got["dc_prev"], inp["dc_next"], ~live)
        res["dgates"] = _bitcmp(got["dgates"], torch.zeros(b, 4 * h, dtype=dt), ~live)
    if _raw:
        return dcp, e_dcp
    res["dc_prev, constants >= half the bar"] = _const_dominated(got["dc_prev"], (dcp, e_dcp), _no_const(lambda: lstm_bwd_check(inp, got, True)))
    res["dgates"] = _worse(worst(got["dgates"], ref, bar), res.get("dgates", (0.0, -1)))
    res["dc_prev"] = _worse(worst(got["dc_prev"], dcp, e_dcp), res.get("dc_prev", (0.0, -1)))
    return res


# ================================================================================================ t2_attention_fwd / bwd
ATT_CASES = [   # id, B, Ti, A, E, lengths, awc_prev given, KL, KK (0: no fused location term), context destinations
    ("odd_groups", 3, 23, 24, 40, [23, 1, 12], True, 0, 0, 3),          # A / 8 = 3, E / 8 = 5: lpa = 4, lpe = 8 with clamped lanes
    ("one_group_first_step", 2, 37, 40, 8, [37, 5], False, 0, 0, 1),     # lpe = 1, awc_prev == NULL
    ("limits_512", 2, 70, 512, 512, [70, 33], True, 0, 0, 2),            # lpa = lpe = 64: the row folds run no iteration
    ("second_trip", 2, 1100, 32, 64, [1100, 1030], True, 0, 0, 1),       # Ti > 1024: per-thread loops over t take two trips
    ("len_above_ti", 2, 9, 128, 512, [14, 9], True, 0, 0, 1),            # clamped to Ti: bit-equal to [9, 9]
    ("default", 4, 150, 128, 512, [150, 97, 3, 149], True, 0, 0, 2),
    ("loc_ti32", 2, 23, 32, 64, [23, 17], True, 31, 64, 1),              # Ti32 = 32 != Ti
    ("loc_k5", 2, 40, 64, 128, [40, 31], True, 5, 32, 2),
    ("loc_ti_below_pad", 1, 2, 32, 8, [2], True, 5, 32, 1),              # Ti < KL / 2 + 1
    ("loc_default", 2, 160, 128, 512, [160, 101], True, 31, 64, 1),
]
ATT_TWIN = {"len_above_ti": [9, 9]}
# backward variants per case: (context pieces, weight-gradient pieces, d_memory, dq, d_pm_acc given, dq16, dctx16)
ATT_BWD_VARIANTS = {
    "odd_groups": (3, 2, True, True, True, True, True), "one_group_first_step": (1, 1, False, True, False, False, False),
    "limits_512": (2, 1, True, False, True, True, True), "second_trip": (1, 2, False, True, True, False, True),
    "len_above_ti": (2, 2, True, True, False, True, False), "default": (3, 2, False, False, False, True, True),
    "loc_ti32": (2, 2, True, True, True, True, False), "loc_k5": (1, 1, False, True, False, True, True),
    "loc_ti_below_pad": (3, 2, True, True, True, False, False), "loc_default": (2, 2, False, False, False, True, True),
}


def att_case(cid):
    return next(c for c in ATT_CASES if c[0] == cid)


def att_inputs(case, dtype, lengths=None):
    """v N(0, 1) 4 sqrt(32 / A) (sum|v| ~ 18 sqrt(A) >= 88).  pl = r16(target - q) with q N(0, 1) and the pre-activation `target`:
      sample 0 (Ti > 2), row 0: +8 sign(v), row 1: -8 sign(v) -- saturated tanh, energies +-sum|v|, more than 104 apart: __expf underflows to
      exactly 0; its other rows N(0, 1.5) (weights down to 1e-30 and below);
      other samples N(0, 0.07) (energies N(0, ~1.5): softmax sums of many comparable terms);
      last sample: row 2 = row 0 (equal energies up to the order of the sums: a few fp32 ulps), row 1 = row 0 except the element
      of the smallest |v|, one 16-bit step away (the closest two different rows can be).
    memory N(0, 1); awc_prev: columns 0 / 1 a softmax-like previous weight and a cumulative one, columns 2..7 junk the kernel must not
    read into anything; wloc [A, KK] N(0, 0.3) in its first 2 KL columns, zero beyond."""
    cid, b, ti, a, e, lens, has_prev, kl, kk, ndst = case
    g = gen(2000 + sum(map(ord, cid)))
    v = (torch.randn(a, generator=g) * 4.0 * (32.0 / a) ** 0.5).float()
    q = torch.randn(b, a, generator=g)
    target = torch.randn(b, ti, a, generator=g) * 0.07
    target[0] = torch.randn(ti, a, generator=g) * 1.5
    sgn = torch.where(v >= 0, torch.ones(()), -torch.ones(()))
    if ti > 2:
        target[0, 0], target[0, 1] = 8.0 * sgn, -8.0 * sgn
    pl = (target - q.view(b, 1, a)).to(dtype)
    if ti > 1:
        pl[b - 1, 1] = pl[b - 1, 0]
        k = int(v.abs().argmin())
        x = pl[b - 1, 1, k].float()
        pl[b - 1, 1, k] = (x + ulp(x.double(), dtype).float()).to(dtype)
    if ti > 2:
        pl[b - 1, 2] = pl[b - 1, 0]
    inp = {"case": case, "dtype": dtype, "B": b, "Ti": ti, "A": a, "E": e, "q": q, "pl": pl.view(b * ti, a), "v": v,
           "memory": torch.randn(b * ti, e, generator=g).to(dtype), "lengths": torch.tensor(lengths or lens, dtype=torch.int64),
           "awc_prev": None, "wloc": None, "KL": kl, "KK": kk, "ndst": ndst}
    if has_prev:
        pw = torch.softmax(torch.randn(b, ti, generator=g) * 2, 1)
        awc = torch.randn(b, ti, 8, generator=g)
        awc[..., 0], awc[..., 1] = pw, pw * 3 + torch.rand(b, ti, generator=g) * 0.2
        inp["awc_prev"] = awc.view(b * ti, 8).to(dtype)
    if kk:
        w = torch.zeros(a, kk)
        w[:, :2 * kl] = torch.randn(a, 2 * kl, generator=g) * 0.3
        inp["wloc"] = w.to(dtype)
    return inp


def _loc_cols(inp, work, shift=0):
    """the im2col operand of the fused location term: cols[b, t, 2 j + c] = awc_prev[b, t + j - KL / 2 (+ shift), c], 0 outside
    [0, Ti) -> [B, Ti, KK] (all KK / 2 taps, as the kernel multiplies them; wloc is zero past 2 KL)"""
    b, ti, kk, pad = inp["B"], inp["Ti"], inp["KK"], inp["KL"] // 2
    nt = kk // 2
    P = torch.zeros(b, ti + nt + pad + 2, 2, dtype=work)
    if inp["awc_prev"] is not None:
        P[:, pad:pad + ti] = inp["awc_prev"].view(b, ti, 8)[..., :2].to(work)
    P = P[:, shift:]
    return P.unfold(1, nt, 1)[:, :ti].permute(0, 1, 3, 2).reshape(b, ti, kk)


def att_fwd_model(inp, fault=None):
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]
    x = inp["pl"].float().view(b, ti, a)
    if inp["wloc"] is not None:
        x = x + _loc_cols(inp, F32, 1 if fault == "loc_pad_shift" else 0) @ inp["wloc"].float().t()
    th32 = _f32model_tanh(inp["q"].view(b, 1, a) + x)
    th = r16(th32, dt)
    v = inp["v"]
    src = th32 if fault == "energy_from_unrounded_tanh" else th.float()
    en = (src * v).sum(2)
    if fault == "inactive_lanes_counted":
        en = en + (pow2_ge(a // 8) - a // 8) * (src[..., :8] * v[:8]).sum(2)
    ln = inp["lengths"].clamp(max=ti)
    if fault == "mask_off_by_one":
        ln = (ln + 1).clamp(max=ti)
    valid = torch.arange(ti).view(1, ti) < ln.view(b, 1)
    mx = torch.where(valid, en, torch.full((), -3.0e38)).max(1, keepdim=True).values
    ex = torch.where(valid, torch.exp(en - mx), torch.zeros(()))
    w = ex * (1.0 / ex.sum(1, keepdim=True))
    prev_cum = inp["awc_prev"].view(b, ti, 8)[..., 1].float() if inp["awc_prev"] is not None else torch.zeros(b, ti)
    nxt = torch.zeros(b, ti, 8, dtype=dt)
    nxt[..., 0], nxt[..., 1] = r16(w, dt), r16(prev_cum if fault == "cum_without_w" else prev_cum + w, dt)
    ctx = r16((w.view(b, ti, 1) * inp["memory"].float().view(b, ti, e)).sum(1), dt)
    return {"tanh_out": th.view(b * ti, a), "aw_out": w, "awc_next": nxt.view(b * ti, 8), "ctx": [ctx.clone() for _ in range(inp["ndst"])]}


def att_fwd_check(inp, got):
    """got: tanh_out [B Ti, A], aw_out fp32 [B, Ti], awc_next [B Ti, 8], ctx: list of [B, E].
    1. x = q + pl (+ loc): loc[t, a] = sum_k wloc[a, k] cols[t, k] on the matrix cores: KK u sum|w cols|; pl + loc: u; q + .: u
         dx = KK u sum|w cols| + u |pl + loc| + u |x|   (no wloc: u |x|);   tanh_out = r16(fast_tanh(x)): stored(tanh, delta(x, dx))
    2. from tanh_out_got: en[t] = sum_a v[a] th[t, a], A rounded products in an order not assumed: d_en = A u sum|v th| (the clamped
       lanes of a non-power-of-two A / 8 add exact zeros).  w = exp(en - max) / sum over t < len.  A common shift of `max` cancels in
       the quotient, so per weight: rel(e_t) = d_en[t] + E(max - en[t]); the sum: a thread adds ceil(Ti / 1024) terms, block_sum is a
       6-level butterfly and a 16-term fold: (trips + 22) u; the division and the product: 2 u
         |dw| <= w [ rel(e_t) + sum_s e_s rel(e_s) / sum + (trips + 24) u ] + 2^-126        (an underflowed e_t is exactly 0)
       aw_out is exactly 0 at t >= len (len clamped to Ti).
    3. awc_next bit for bit from aw_got: (r16(w), r16(fp32(prev_cum) + w), 0, 0, 0, 0, 0, 0).
    4. ctx[c] = sum_{t < len} aw_got[t] memory[t, c]: len rounded products in an order not assumed: stored(ctx, len u sum|w m|); every
       destination the same bits."""
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]
    q, pl = widen(inp["q"]).view(b, 1, a), widen(inp["pl"]).view(b, ti, a)
    if inp["wloc"] is not None:
        cols, w64 = _loc_cols(inp, F64), widen(inp["wloc"])
        loc, mag = cols @ w64.t(), cols.abs() @ w64.abs().t()
        x = q + pl + loc
        dx = inp["KK"] * U * mag + U * (pl + loc).abs() + U * x.abs()
    else:
        x = q + pl
        dx = U * x.abs()
    th, dth = tanh_ref(x, dx)
    res = {"tanh_out": worst(got["tanh_out"].view(b, ti, a), th, stored(th, dth, dt))}
    thg, v = widen(got["tanh_out"]).view(b, ti, a), widen(inp["v"])
    en = (thg * v).sum(2)
    d_en = a * U * (thg * v).abs().sum(2)
    ln = inp["lengths"].clamp(max=ti)
    valid = torch.arange(ti).view(1, ti) < ln.view(b, 1)
    mx = torch.where(valid, en, torch.full((), -INF, dtype=F64)).max(1, keepdim=True).values
    d = (mx - en).clamp_min(0)
    ex = torch.where(valid, torch.exp(-d), torch.zeros((), dtype=F64))
    rel = d_en + exp_rel(d)
    s = ex.sum(1, keepdim=True)
    trips = -(-ti // T2A_BLOCK)
    w = ex / s
    dw = torch.where(valid, w * (rel + (ex * rel).sum(1, keepdim=True) / s + (trips + 24) * U) + TINY, torch.zeros((), dtype=F64))
    res["aw_out"] = worst(got["aw_out"], w, dw)
    wg = got["aw_out"].float()
    prev_cum = inp["awc_prev"].view(b, ti, 8)[..., 1].float() if inp["awc_prev"] is not None else torch.zeros(b, ti)
    nxt = torch.zeros(b, ti, 8, dtype=dt)
    nxt[..., 0], nxt[..., 1] = r16(wg, dt), r16(prev_cum + wg, dt)
    res["awc_next"] = _bitcmp(got["awc_next"], nxt.view(b * ti, 8))
    terms = torch.where(valid, wg.double(), torch.zeros((), dtype=F64)).view(b, ti, 1) * widen(inp["memory"]).view(b, ti, e)
    ctx = terms.sum(1)
    cbar = stored(ctx, ln.view(b, 1).double() * U * terms.abs().sum(1), dt)
    r = worst(got["ctx"][0], ctx, cbar)
    for other in got["ctx"][1:]:
        r = _worse(r, _bitcmp(other, got["ctx"][0]))
    res["ctx"] = r
    return res


def att_bwd_inputs(case, dtype):
    """from the forward model's saved tensors (tanh_out, weights); gradient pieces N(0, 1) (context) and N(0, 1) (weights);
    accumulation bases N(0, 1): of order 1, so that a lost addend of order 1e-3 shows only against the addend's bar"""
    inp = att_inputs(case, dtype)
    cid, b, ti, a, e = case[:5]
    fw = att_fwd_model(inp)
    npc, naw, has_dm, has_dq, has_pm, has_dq16, has_dctx16 = ATT_BWD_VARIANTS[cid]
    g = gen(3000 + sum(map(ord, cid)))
    inp.update(tanh_out=fw["tanh_out"], aw=fw["aw_out"], dc=[torch.randn(b, e, generator=g) for _ in range(npc)],
               daw=[torch.randn(b, ti, generator=g) for _ in range(naw)],
               d_memory=torch.randn(b * ti, e, generator=g) if has_dm else None, has_dq=has_dq, has_dq16=has_dq16 or not has_dq,
               has_dctx16=has_dctx16, d_pm_acc=torch.randn(b * ti, a, generator=g) if has_pm else None,
               dv_acc=torch.randn(b, a, generator=g), d_cum=torch.randn(b, ti, generator=g) if inp["KK"] else None,
               wloc_t=inp["wloc"].t().contiguous() if inp["KK"] else None)
    return inp


def _loc_fold(dcol, ti, kl, shift=0):
    """d weights[s][c] = sum_j dcol[s - j + KL / 2 (- shift)][2 j + c] over 0 <= t < Ti -> ([B, Ti, 2] sums, [B, Ti, 2] sums of |terms|)"""
    b, pad = dcol.shape[0], kl // 2
    D = torch.zeros(b, ti + 2 * kl + 2, dcol.shape[2], dtype=dcol.dtype)
    D[:, kl + 1:kl + 1 + ti] = dcol
    acc, mag = torch.zeros(b, ti, 2, dtype=dcol.dtype), torch.zeros(b, ti, 2, dtype=dcol.dtype)
    for j in range(kl):
        o = kl + 1 + pad - j - shift
        acc += D[:, o:o + ti, 2 * j:2 * j + 2]
        mag += D[:, o:o + ti, 2 * j:2 * j + 2].abs()
    return acc, mag


def att_bwd_model(inp, fault=None):
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]
    dcv = _sum32(inp["dc"])
    mem, aw, th, v = inp["memory"].float().view(b, ti, e), inp["aw"], inp["tanh_out"].float().view(b, ti, a), inp["v"]
    dot = (mem * dcv.view(b, 1, e)).sum(2)
    if fault == "inactive_lanes_counted":
        dot = dot + (pow2_ge(e // 8) - e // 8) * (mem[..., :8] * dcv.view(b, 1, e)[..., :8]).sum(2)
    de = dot + inp["daw"][0]
    if len(inp["daw"]) > 1:
        de = de + inp["daw"][1]
    s = (aw * de).sum(1, keepdim=True)
    de = aw * (de - s)
    dpre = de.view(b, ti, 1) * v * (1.0 - th * th)
    dq, dv = dpre.sum(1), (de.view(b, ti, 1) * th).sum(1)
    if fault == "inactive_lanes_counted":
        extra = pow2_ge(a // 8) - a // 8
        dq[:, :8] += extra * dq[:, :8]
        dv[:, :8] += extra * dv[:, :8]
    out = {"d_pl": r16(dpre, dt).view(b * ti, a), "dq": dq if inp["has_dq"] else None, "dq16": r16(dq, dt) if inp["has_dq16"] else None,
           "dctx16": r16(dcv, dt) if inp["has_dctx16"] else None, "dv_acc": dv if fault == "dv_overwritten" else inp["dv_acc"] + dv,
           "d_memory": None, "d_pm_acc": None, "d_prev": None, "d_cum": None}
    if inp["d_memory"] is not None:
        out["d_memory"] = inp["d_memory"] + (aw.view(b, ti, 1) * dcv.view(b, 1, e)).view(b * ti, e)
    if inp["d_pm_acc"] is not None:
        out["d_pm_acc"] = inp["d_pm_acc"] + dpre.view(b * ti, a)
    if inp["wloc_t"] is not None:
        # (loc_rows_past_ti_live: operand rows Ti..Ti32 hold stale values; their products land in rows of dcol the fold never reads)
        dcol = out["d_pl"].float().view(b, ti, a) @ inp["wloc_t"].float().t()
        acc, _ = _loc_fold(dcol, ti, inp["KL"], 1 if fault == "loc_pad_shift" else 0)
        out["d_prev"] = acc[..., 0].contiguous()
        out["d_cum"] = acc[..., 1].contiguous() if fault == "dcum_overwritten" else inp["d_cum"] + acc[..., 1]
    return out


def _acc(got, base, add, e_add):
    """an accumulated output: got - base against the addend, the addend's bar + one rounding of the final add"""
    return worst(widen(got) - widen(base), add, e_add + U * (widen(base) + add).abs())


def att_bwd_check(inp, got):
    """dcv = (dc0 + dc1) + dc2 on load: e_dcv = (pieces - 1) u sum|piece|; dctx16 = r16 of that fp32 sum, bit for bit.
      de_raw[t] = sum_c m[t, c] dcv[c] + daw0 + daw1: E u sum|m dcv| + sum|m| e_dcv + 2 u (|dot| + |daw0| + |daw1|)
      s = sum_t aw de_raw: sum aw e_de + (trips + 23) u sum|aw de_raw|      (one product, per-thread trips, butterfly 6, fold 16)
      de[t] = aw (de_raw - s): aw (e_de + e_s + u |de_raw - s|) + u |de|
      d_memory[t, c] += aw[t] dcv[c]: aw e_dcv + u |aw dcv|
      dpre[t, a] = de v (1 - th^2): e_de |v (1 - th^2)| + |de v| (u th^2 + u |1 - th^2|) + 2 u |dpre|;  d_pl = r16(dpre);  d_pm_acc += dpre
      dq[a] = sum_t dpre: sum e_dpre + (Ti - 1) u sum|dpre|;   dq16 = r16(dq_got) bit for bit (dq NULL: stored(dq, e_dq))
      dv_acc[a] += sum_t de th: sum (e_de |th| + u |de th|) + (Ti - 1) u sum|de th|
    wlocT (staged on the returned 16-bit d_pl): dcol[t, k] = sum_a d_pl[t, a] W[a, k] on the matrix cores: A u sum|d_pl W|;
      d_prev[s] = sum_j dcol[s - j + pad][2 j] over 0 <= t < Ti: sum e_dcol + (KL - 1) u sum|dcol|; d_cum[s] += the channel-1 sum.
    Every position s is checked, the first and last KL / 2 included."""
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]
    pcs = [widen(p) for p in inp["dc"]]
    dcv = sum(pcs).view(b, 1, e)
    e_dcv = ((len(pcs) - 1) * U * sum(p.abs() for p in pcs)).view(b, 1, e)
    mem, aw, th, v = widen(inp["memory"]).view(b, ti, e), widen(inp["aw"]), widen(inp["tanh_out"]).view(b, ti, a), widen(inp["v"])
    daw = [widen(t) for t in inp["daw"]]
    dot = (mem * dcv).sum(2)
    de_raw = dot + sum(daw)
    e_de = e * U * (mem * dcv).abs().sum(2) + (mem.abs() * e_dcv).sum(2) + 2 * U * (dot.abs() + sum(t.abs() for t in daw))
    trips = -(-ti // T2A_BLOCK)
    s = (aw * de_raw).sum(1, keepdim=True)
    e_s = (aw * e_de).sum(1, keepdim=True) + (trips + 23) * U * (aw * de_raw).abs().sum(1, keepdim=True)
    de = aw * (de_raw - s)
    e_de = aw * (e_de + e_s + U * (de_raw - s).abs()) + U * de.abs()
    res = {}
    if inp["has_dctx16"]:
        res["dctx16"] = _bitcmp(got["dctx16"], r16(_sum32(inp["dc"]), dt))
    if inp["d_memory"] is not None:
        add = (aw.view(b, ti, 1) * dcv).view(b * ti, e)
        e_add = (aw.view(b, ti, 1) * e_dcv).view(b * ti, e) + U * add.abs()
        res["d_memory"] = _acc(got["d_memory"], inp["d_memory"], add, e_add)
    om = 1 - th * th
    dev, e_dev = de.view(b, ti, 1), e_de.view(b, ti, 1)
    dpre = dev * v * om
    e_dpre = e_dev * (v * om).abs() + (dev * v).abs() * (U * th * th + U * om.abs()) + 2 * U * dpre.abs()
    res["d_pl"] = worst(got["d_pl"].view(b, ti, a), dpre, stored(dpre, e_dpre, dt))
    if inp["d_pm_acc"] is not None:
        res["d_pm_acc"] = _acc(got["d_pm_acc"], inp["d_pm_acc"], dpre.view(b * ti, a), e_dpre.view(b * ti, a))
    dq = dpre.sum(1)
    e_dq = e_dpre.sum(1) + (ti - 1) * U * dpre.abs().sum(1)
    if inp["has_dq"]:
        res["dq"] = worst(got["dq"], dq, e_dq)
        if inp["has_dq16"]:
            res["dq16"] = _bitcmp(got["dq16"], r16(got["dq"], dt))
    else:
        res["dq16"] = worst(got["dq16"], dq, stored(dq, e_dq, dt))
    dvt = dev * th
    res["dv_acc"] = _acc(got["dv_acc"], inp["dv_acc"], dvt.sum(1), (e_dev * th.abs() + U * dvt.abs()).sum(1) + (ti - 1) * U * dvt.abs().sum(1))
    if inp["wloc_t"] is not None:
        dplg, w64, kl = widen(got["d_pl"]).view(b, ti, a), widen(inp["wloc_t"]), inp["KL"]
        dcol = dplg @ w64.t()
        e_dcol = a * U * (dplg.abs() @ w64.abs().t())
        acc, mag = _loc_fold(dcol, ti, kl)
        eacc, _ = _loc_fold(e_dcol, ti, kl)
        bar = eacc + (kl - 1) * U * mag
        res["d_prev"] = worst(got["d_prev"], acc[..., 0], bar[..., 0])
        res["d_cum"] = _acc(got["d_cum"], inp["d_cum"], acc[..., 1], bar[..., 1])
    return res


# ================================================================================================ t2_location_bwd
LOC_CASES = [(3, 23, 31), (2, 9, 5), (1, 2, 5), (70, 3800, 3)]      # B, Ti, KL; the last: 266 000 items > 1024 x 256


def loc_inputs(case, dtype):
    b, ti, kl = case
    g = gen(4000 + ti + kl)
    return {"case": case, "dtype": dtype, "dcol": torch.randn(b * ti, kl * 8, generator=g).to(dtype), "d_cum": torch.randn(b, ti, generator=g)}


def loc_model(inp, fault=None):
    b, ti, kl = inp["case"]
    d = inp["dcol"].float().view(b, ti, kl, 8)[..., :2].reshape(b, ti, kl * 2)
    acc, _ = _loc_fold(d, ti, kl, 1 if fault == "loc_pad_shift" else 0)
    d_prev, d_cum = acc[..., 0].contiguous(), (acc[..., 1] if fault == "dcum_overwritten" else inp["d_cum"] + acc[..., 1])
    if fault == "second_trip_skipped" and b * ti > T2_CAP * T2_BLOCK:
        reach = (torch.arange(b * ti) < T2_CAP * T2_BLOCK).view(b, ti)
        d_prev, d_cum = torch.where(reach, d_prev, untouched((b, ti), F32)), torch.where(reach, d_cum, inp["d_cum"])
    return {"d_prev": d_prev, "d_cum": d_cum}


def loc_check(inp, got):
    """d_prev[b, s] = sum_j dcol[b, s - j + KL / 2, 8 j] over 0 <= t < Ti (written), d_cum[b, s] += the same of column 8 j + 1: serial
    fp32 sums of at most KL exact 16-bit terms from 0: (KL - 1) u sum|term|; d_cum: + u |base + addend|.  Columns 8 j + 2 .. 8 j + 7
    are not read.  Every position, the first and last KL / 2 included."""
    b, ti, kl = inp["case"]
    d = widen(inp["dcol"]).view(b, ti, kl, 8)[..., :2].reshape(b, ti, kl * 2)
    acc, mag = _loc_fold(d, ti, kl)
    bar = (kl - 1) * U * mag
    return {"d_prev": worst(got["d_prev"], acc[..., 0], bar[..., 0]), "d_cum": _acc(got["d_cum"], inp["d_cum"], acc[..., 1], bar[..., 1])}


# ================================================================================================ t2_mel_loss
MEL_CASES = [(1, 7, 10, 12), (1, 80, 83, 88), (3300, 80, 83, 85)]      # R, n_mel, ld_out, ld_dout; the last: 264 000 > 1024 x 256
MEL_SCALES = [None, 2.0 ** -3]


def mel_inputs(case, dtype, scale):
    r, nm, ldo, ldd = case
    g = gen(5000 + r + nm)
    return {"case": case, "dtype": dtype, "scale": scale, "out_all": torch.randn(r, ldo, generator=g)[:, :nm], "post": (torch.randn(r * nm, generator=g) * 0.5).to(dtype),
            "target": torch.randn(r * nm, generator=g) - 1.0}


def mel_model(inp, fault=None):
    r, nm, _, _ = inp["case"]
    dt, n = inp["dtype"], r * nm
    mo, tg = inp["out_all"].reshape(-1), inp["target"]
    mp = mo + inp["post"].float()
    e1, e2 = mo - tg, mp - tg
    invn, sc = np.float32(1.0) / np.float32(n), np.float32(1.0 if inp["scale"] is None else inp["scale"])
    term = e1 * e1 + e2 * e2
    g2 = 2.0 * e2 * invn * sc
    d_post, d_out = r16(g2, dt), r16(2.0 * e1 * invn * sc + g2, dt)
    if fault == "second_trip_skipped" and n > T2_CAP * T2_BLOCK:
        reach = torch.arange(n) < T2_CAP * T2_BLOCK
        term = torch.where(reach, term, torch.zeros(()))
        d_post, d_out = torch.where(reach, d_post, untouched((n,), dt)), torch.where(reach, d_out, untouched((n,), dt))
    return {"loss": (term.sum() * invn).view(1), "d_post": d_post, "d_out": d_out.view(r, nm)}


def mel_check(inp, got):
    """loss = [sum (mo - tg)^2 + (mo + post - tg)^2] / n,  d_post = r16(2 e2 sc / n),  d_out = r16(2 e1 sc / n + d_post's fp32 value).
      mp = mo + post: u |mp|;  e1 = mo - tg: u |e1|;  e2 = mp - tg: u |mp| + u |e2| =: d2
      term: 3 u e1^2 + 2 |e2| d2 + u e2^2 + u term.  The sum (all terms >= 0, so every partial sum is below the total): a thread adds
      T = ceil(n / (256 G)) terms, block_sum 6 + 4, x fp32(1 / n) (2 u), then t2_sum: ceil(G / 256) serial, 6 + 4:
         loss_bar = sum d_term / n + (T + ceil(G / 256) + 22) u loss
      g2 = 2 e2 invn sc: 2 d2 sc / n + 3 u |g2|  (invn, two products; x 2 is exact);  g1 likewise with u |e1|: 4 u |g1|;  the sum: u |d_out|.
    sc = *scale or 1; strided out_all and d_out (the bytes between the rows are the frame's to check)."""
    r, nm, _, _ = inp["case"]
    dt, n = inp["dtype"], r * nm
    mo, tg, po = widen(inp["out_all"]).reshape(-1), widen(inp["target"]), widen(inp["post"])
    sc = 1.0 if inp["scale"] is None else f32(inp["scale"])
    mp = mo + po
    e1, e2 = mo - tg, mp - tg
    d2 = U * mp.abs() + U * e2.abs()
    term = e1 * e1 + e2 * e2
    d_term = 3 * U * e1 * e1 + 2 * e2.abs() * d2 + U * e2 * e2 + U * term
    loss = term.sum() / n
    G = max(1, min(T2_CAP, -(-n // T2_BLOCK)))
    T = -(-n // (T2_BLOCK * G))
    loss_bar = d_term.sum() / n + (T + -(-G // 256) + 22) * U * loss
    g2, g1 = 2 * e2 * sc / n, 2 * e1 * sc / n
    e_g2 = 2 * d2 * sc / n + 3 * U * g2.abs()
    d_out = g1 + g2
    e_out = e_g2 + 4 * U * g1.abs() + U * d_out.abs()
    return {"loss": worst(got["loss"], loss.view(1), loss_bar.view(1)), "d_post": worst(got["d_post"], g2, stored(g2, e_g2, dt)),
            "d_out": worst(got["d_out"].reshape(-1), d_out, stored(d_out, e_out, dt))}


# ================================================================================================ t2_sum_steps
SUM_STEPS_N = [1, 3, 4, 7, 9]         # tail only, tail only, one unrolled body, body + tail of 3, two bodies + tail of 1
SUM_STEPS_R = [8, 4104]               # one item; 513 items of 8: three workgroups, the last one partly idle


def sum_steps_inputs(case, dtype):
    n, r = case
    g = gen(6000 + n + r)
    return {"case": case, "dtype": dtype, "x": torch.randn(n, r, generator=g).to(dtype), "out": torch.randn(r, generator=g)}


def sum_steps_model(inp, fault=None):
    n, r = inp["case"]
    x = inp["x"].float()
    acc = torch.zeros(r)
    for s in range(n - n % 4 if fault == "tail_steps_skipped" else n):
        acc = acc + x[s]
    return {"out": inp["out"] + acc}


def sum_steps_check(inp, got):
    """out[r] += sum_s x[s][r]: a serial fp32 sum of n exact terms from 0 (the 4-way unrolled body and the n % 4 tail add in step order):
    (n - 1) u sum|x|, + u |base + sum| for the final add; checked as got - base against the sum."""
    n, r = inp["case"]
    x = widen(inp["x"])
    return {"out": _acc(got["out"], inp["out"], x.sum(0), (n - 1) * U * x.abs().sum(0))}


# ================================================================================================ t2_mask_rows
MASK_CASES = [   # B, To, cols, ld, lengths, fill
    (4, 5, 3, 7, [0, 5, 9, 2], 0.0), (4, 5, 3, 7, [0, 5, 9, 2], 1e3), (2, 3, 8, 8, [1, 3], 1e3),
    (3, 1100, 80, 88, [0, 1100, 500], 1e3),          # R cols = 264 000 > 1024 x 256
]


def mask_inputs(case, dtype):
    b, to, cols, ld, lens, fill = case
    return {"case": case, "dtype": dtype, "x": torch.randn(b * to, ld, generator=gen(7000 + to + cols)).to(dtype), "lengths": torch.tensor(lens, dtype=torch.int64)}


def mask_model(inp, fault=None):
    b, to, cols, ld, lens, fill = inp["case"]
    x = inp["x"].clone()
    t = torch.arange(b * to) % to
    row = t >= inp["lengths"].repeat_interleave(to)
    if fault == "mask_off_by_one":
        row = t > inp["lengths"].repeat_interleave(to)
    m = row.view(-1, 1) & (torch.arange(ld) < cols).view(1, -1)
    if fault == "second_trip_skipped":
        m[:, :cols] &= (torch.arange(b * to * cols) < T2_CAP * T2_BLOCK).view(b * to, cols)
    x[m] = torch.tensor(fill, dtype=F32).to(inp["dtype"])
    return {"x": x}


def mask_check(inp, got):
    """exact: rows (b, t) with t >= lengths[b] hold fill (fp32: the float itself; 16-bit: r16(fill), 1e3 is exact in both) in columns
    [0, cols), every other element -- columns cols..ld, rows below the length, lengths of 0, To and above To -- keeps its bits"""
    return {"x": _bitcmp(got["x"], mask_model(inp)["x"])}


# ================================================================================================ dispatch
KERNELS = {
    "tanh_fwd": (tanh_model, tanh_check), "lstm_fwd": (lstm_fwd_model, lstm_fwd_check), "lstm_bwd": (lstm_bwd_model, lstm_bwd_check),
    "attention_fwd": (att_fwd_model, att_fwd_check), "attention_bwd": (att_bwd_model, att_bwd_check),
    "location_bwd": (loc_model, loc_check), "mel_loss": (mel_model, mel_check), "sum_steps": (sum_steps_model, sum_steps_check),
    "mask_rows": (mask_model, mask_check),
}


def kernel_model(kernel, inp, fault=None):
    """The kernel's arithmetic in float32 on the CPU (a correctly rounded exp, an exact reciprocal, torch's summation order);
    fault: one of FAULTS, planted where the kernel has the corresponding code; a fault the kernel has no place for changes nothing."""
    assert fault is None or fault in FAULTS
    return KERNELS[kernel][0](inp, fault)


def check(kernel, inp, got):
    """-> {output: (largest ratio, flat index)}; every element of every output takes part"""
    return KERNELS[kernel][1](inp, got)
