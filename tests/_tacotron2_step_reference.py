"""float64 statements, derived per-element bars, input builders, case tables and a faulty float32 model for the three launches of the
Tacotron2 decoder step: dle_t2_lstm_gemm_fwd (csrc/gemm_smallm.hip, the LSTM = true instantiation of the few-row GEMM: the whole
LSTMCell, the dropout and up to three strided hidden-state stores in its epilogue) and dle_t2_prenet_infer / dle_t2_frame_infer
(csrc/tacotron2.hip, its inference section).  A sibling of tests/_tacotron2_reference.py (the twelve training kernels), in the same
shape and on its helpers: K_inputs(case, dtype, ...), K_model(inp, fault), K_check(inp, got), dispatched by kernel_model / check;
ratio = |got - ref| / bar <= 1 on EVERY element, outputs without a bar bit for bit (0 or inf).  tests/ only: no GPU, no ctypes.

Each kernel has two tiers.  Tier A: exactly summable inputs (tests/_exact_grid.py), every output that is a sum compared bit for
bit, the preconditions asserted on the float64 side in the builders.  Tier B: realistic inputs against bars derived from the
roundings (u = 2^-24).  The only measured constants are the project's: C_EXP, C_RCP (through lstm_fwd_check) and the library-expf
constant C_EXPF of tests/_waveglow_reference.py (the gate's sigmoid; it enters no bar, only the condition on the inputs below).
The dropout masks come from oracle/philox_oracle.keep_mask.

lstm_gemm_fwd.  z = x w^T (+ bias) (+ addend), rounded to 16 bits as the unfused dle_gemm output is, then exactly t2_lstm_fwd.
  A  x, w, addend = k / 4, bias a multiple of 1/16: z is a multiple of 1/16 and exact in fp32 in any order while sum|x w| + |bias|
     + |addend| < B_MFMA (asserted), so gates = r16(z) is deterministic and lstm_fwd_check(gates = r16(z)) is the whole statement:
     act in the gates buffer, c_out and h from the unrounded activations, every destination the same bits, dropped elements exactly
     +0.  The density of w keeps at least half of all |z| below 4 (a wrong tap or row moves a visible activation) and a planted
     +-14 puts some |z| > 8 into each gate block (both asserted).
  B  x N(0, 1/4), w N(0, 1/K), bias N(0, 0.01), addend N(0, 1/4), rounded to storage.  The pre-activation cannot be observed from
     the fused launch, so the statement is staged on pre16, the 16-bit output of the unfused dle_gemm on the same operands (the CPU
     model forms it itself): pre16 against stored(z, (K + 2) u (sum|x w| + |bias| + |addend|)) on every element, then the fused
     launch against lstm_fwd_check(gates = pre16): a fused pre-activation that rounds differently from the unfused one fails.
  keep_index: include/dle_mi355x.h states the entry point as "exactly dle_t2_lstm_fwd" behind the product and restricts H, K, the
     pitches and the bases, not keep_index; the epilogue reads byte (keep_index + idx) >> 3 and bit (keep_index + idx) & 7 per
     element, so ANY keep_index is allowed.  The cases run 0, 8 * 5 and 3.
  A workgroup of the last row tile computes 64 rows whatever B is; rows m >= B are clamped on load and must not be stored.  The GPU
  test sees such a store as a changed byte outside a Framed view; the model reports it as the output "outside" (0: none).

prenet_infer.  relu(x W0^T) -> dropout -> relu(. W1^T) -> dropout, p = 0.5 (inv_keep = 2 exactly), step t from a device word.
  A  frame, w0, w1 = k / 4 (the frame up to 63.75, so that layer-1 sums pass 128 and the hidden 16-bit rounding is visible in fp16
     too).  All terms of both layers are multiples of 2^-7 with sum of magnitudes x 2^7 < 2^24 (asserted): both fp32 sums are
     exact, h1 = 2 r16(relu(.)) is deterministic and dst = r16(2 r16(relu(exact))) bit for bit, +0 where dropped.
  B  frame 2 N(0, 1) in fp32, weights N(0, 1 / fan_in).  The hidden layer's rounding is not observable, so the bar carries it:
     for hidden unit j the admissible values are the 16-bit roundings of relu(v), v within e1 = (NM + 1) u sum|w0 x| of the fp64
     z_j; r16 o relu is monotone, so they lie between r16(relu(z_j - e1)) and r16(relu(z_j + e1)) and delta_j is the larger distance
     of the two from r16(relu(z_j)).  Output: stored(ref, (P + 1) u sum|w1 h| + sum_j |w1_ij| delta_j inv_keep) (x 2 for the kept
     elements: exact), no element left out.  pre_check leaves the share of hidden units with delta_j > 0 in inp["info"].
  Both mask outputs equal keep_mask(B P, 0.5, seed, 1 + 2 t + l) bit for bit, at every step; t = 2^31 carries into the offset's
  high word.  The go frame (frame = None) gives all zeros.

frame_infer.  [mel | gate logit] = hc w^T + bias in fp32, the stop bookkeeping of model.py:578-582 and the step words.
  A  hc, w = k / 4, bias a multiple of 1/16: mel_out, gate_out, frame_next bit for bit the fp64 value.
  B  hc N(0, 1), w N(0, 1 / K): (K + 1) u (sum|w h| + |bias|) per element.
  not_finished, mel_lengths and the four state words follow from the fp64 logits and must match exactly after every step.  That
  needs every decision to be defined: a logit whose fp64 sigmoid lies within s (1 - s) (e_v + C_EXPF u) + 2 u s of the threshold
  (e_v: its own bar) is undecided; fr_inputs moves the gate bias until there is none and asserts the count is zero -- a condition on
  the inputs, never a skip.  Steps beyond out_steps or max_steps are counted but not stored: their rows keep the NaN fill, and
  frame_next is still written.  The fused form's pre_dst is held to pre_check of step t + 1 on the frame the launch itself
  returned (frame_next, checked above; in tier A it IS the exact value): a staged statement, as in _tacotron2_reference.

Faults (kernel_model's `fault`), each caught at a named (output, case) by tests/test_tacotron2_step_reference_host.py.
"""
import numpy as np
import torch

from oracle import philox_oracle as PO
from tests import _exact_grid as G
from tests import _smallops_reference as S
from tests import _tacotron2_reference as R
from tests import _waveglow_reference as WG

F64, F32, F16, BF16, U8 = S.F64, S.F32, S.F16, S.BF16, S.U8
U, INF = S.U, float("inf")
stored, worst, widen, gen, name, f32 = S.stored, S.worst, S.widen, S.gen, S.name, S.f32
r16, inv_keep, untouched, lstm_fwd_check, lstm_fwd_model = R.r16, R.inv_keep, R.untouched, R.lstm_fwd_check, R.lstm_fwd_model
_keep_mask, _bitcmp, _worse = R._keep_mask, R._bitcmp, R._worse
C_EXPF = WG.C_EXPF
TIERS = ("A", "B")
SM_TS, SM_BKE, T2I_MAXB, TRIP = 64, 128, 8, 512
Q = 2.0 ** -7                       # the grid every term of a tier-A prenet / frame sum lies on

FAULTS = ("tile_map_transposed", "last_k_chunk_dropped", "clamped_rows_written", "keep_index_dropped", "bias_from_gate0",
          "masks_swapped", "offset_truncated", "second_k_trip_skipped", "hidden_fp32",
          "step_at_out_steps_stored", "lengths_before_not_finished", "wrong_parity_advanced")


def _exact(terms_mag, value, q, bound, what):
    """tier-A precondition: `value` lies on the grid q and its sum of magnitudes / q stays below `bound`: every partial sum, in any
    order, has at most log2(bound) significant bits, so the fp32 sum is exact"""
    assert torch.equal(value / q, torch.round(value / q)), "%s: off the 2^%d grid" % (what, int(np.log2(q)))
    assert float(terms_mag.max()) / q < bound, "%s: sum of magnitudes %g, fp32 sums would not be exact" % (what, float(terms_mag.max()))


# ================================================================================================ lstm_gemm_fwd
LG_CASES = [   # id, B, H, K, bias, addend, dropout p, keep indices, destinations given (d0, d1, d2)
    ("one_tile_k8", 1, 8, 8, True, True, 0.1, (0, 40), (1, 1, 0)),              # one tile, one chunk of 8, 63 clamped rows
    ("b8_second_chunk8", 8, 16, 136, True, False, None, (0,), (0, 1, 0)),       # second chunk 8 wide; d0 = NULL, d1 set
    ("b3_h96", 3, 96, 160, True, True, 0.1, (0, 40), (1, 1, 1)),                # the existing small case; all three destinations
    ("b63", 63, 8, 264, False, True, 0.1, (3,), (1, 1, 0)),                     # row-tile edge, nk = 3 = NST - 1 (four stages)
    ("b64", 64, 8, 264, True, False, None, (0,), (1, 1, 0)),
    ("b65", 65, 8, 264, True, True, 0.1, (0, 40), (1, 1, 0)),
    ("b129_wrap", 129, 8, 648, True, True, 0.1, (40,), (1, 1, 1)),              # three row tiles, the last with one row; the ring wraps
    ("nst3_short", 65, 1032, 136, True, True, 0.1, (40,), (1, 1, 0)),           # 258 tiles: three stages, nk = 2 = NST - 1
    ("nst3_wrap", 65, 1032, 392, True, False, 0.1, (0,), (0, 1, 0)),            # three stages with a wrap
    ("infer_attention", 8, 1024, 1792, True, False, None, (0,), (1, 1, 0)),     # the two cells of the inference step
    ("infer_decoder", 8, 1024, 2560, True, False, None, (0,), (1, 1, 0)),
    ("train", 128, 1024, 1536, False, True, 0.1, (0, 40), (1, 1, 0)),           # the trainer's shape: addend and keep
]


def lg_case(cid):
    return next(c for c in LG_CASES if c[0] == cid)


def lg_stages(b, h):
    """the launcher's ring depth: four stages up to 256 tiles, else three"""
    return 4 if -(-b // SM_TS) * (h // 8) <= 256 else 3


def lg_inputs(case, dtype, tier):
    """-> the operands as the kernel sees them, z (fp64) and its sum of magnitudes; keep bits as R.lstm_inputs draws them (whole
    bytes of 0x00 and 0xFF); keep_index = the case's first (lg_at moves it)"""
    cid, b, h, k, has_bias, has_add, p, kidxs, dsts = case
    g = gen(8000 + 3 * b + 5 * h + k)
    if tier == "A":
        x = G.grid((b, k), 8100 + b + k, dtype, "cpu", 4)
        w = G.grid((4 * h, k), 8200 + h + k, dtype, "cpu", 4, min(1.0, 64.0 / k))
        bias = torch.randint(-32, 33, (4 * h,), generator=g).float() / 16 if has_bias else None
        add = G.grid((b, 4 * h), 8300 + b + h, dtype, "cpu", 8) if has_add else None
        for q in range(4):                        # some |z| > 8 in every gate block
            col, sgn = q * h + q % h, 1.0 if q % 2 == 0 else -1.0
            if has_bias:
                bias[col] += 14.0 * sgn
            else:
                add[:, col] = 14.0 * sgn
    else:
        x = (torch.randn(b, k, generator=g) * 0.5).to(dtype)
        w = (torch.randn(4 * h, k, generator=g) / k ** 0.5).to(dtype)
        bias = torch.randn(4 * h, generator=g) * 0.1 if has_bias else None
        add = (torch.randn(b, 4 * h, generator=g) * 0.5).to(dtype) if has_add else None
    z, mag = widen(x) @ widen(w).t(), widen(x).abs() @ widen(w).abs().t()
    for t in (bias, add):
        if t is not None:
            z, mag = z + widen(t), mag + widen(t).abs()
    if tier == "A":
        _exact(mag, z, 1.0 / 16, G.B_MFMA, "lstm_gemm %s" % cid)
        assert float((z.abs() < 4).double().mean()) >= 0.5, "%s: fewer than half of the pre-activations are unsaturated" % cid
        assert all(float(z[:, q * h:(q + 1) * h].abs().max()) > 8 for q in range(4)), "%s: a gate block without |z| > 8" % cid
    inp = {"case": (cid, b, h, p, False, kidxs[0], 0, "vec"), "lg_case": case, "tier": tier, "dtype": dtype, "B": b, "H": h, "K": k, "x": x,
           "w": w, "bias": bias, "addend": add, "c_prev": torch.randn(b, h, generator=g), "keep": None, "keep_index": kidxs[0],
           "inv_keep": 1.0, "live": None, "h_prev": None, "dsts": dsts, "z": z, "mag": mag, "p": p}
    if p is not None:
        nbytes = (max(kidxs) + b * h + 7) // 8 + 3
        kb = (torch.rand(nbytes * 8, generator=g) >= 0.3).view(-1, 8)
        kb[1 % nbytes], kb[2 % nbytes] = False, True
        inp["keep"] = (kb.to(torch.int32) * (1 << torch.arange(8, dtype=torch.int32))).sum(1).to(U8)
        inp["inv_keep"] = inv_keep(p)
    return inp


def lg_at(inp, keep_index):
    return dict(inp, keep_index=keep_index, case=inp["case"][:5] + (keep_index,) + inp["case"][6:])


def _transposed_rows(h):
    """weight row a tile would load for (gate, unit) under row r <-> gate r & 3, unit r >> 2 (right: gate r >> 3, unit r & 7)"""
    gq, tn, un = torch.arange(4).view(4, 1, 1), torch.arange(h // 8).view(1, -1, 1), torch.arange(8).view(1, 1, 8)
    r = 8 * gq + un
    return ((r & 3) * h + 8 * tn + (r >> 2)).reshape(-1)


def lg_model(inp, fault=None):
    """fp32: the product in torch's order, + bias, + addend (the kernel's order), r16, then R.lstm_fwd_model.  pre16 stands for the
    UNFUSED product's output (tier B's staging): no fault is planted in it"""
    dt, b, h, k = inp["dtype"], inp["B"], inp["H"], inp["K"]

    def pre(fault):
        x, w, bias = inp["x"].float(), inp["w"].float(), inp["bias"]
        if fault == "tile_map_transposed":
            w = w[_transposed_rows(h)]
        if fault == "last_k_chunk_dropped":
            x = x.clone()
            x[:, (k - 1) // SM_BKE * SM_BKE:] = 0
        z = x @ w.t()
        if bias is not None:
            z = z + (bias[:h].repeat(4) if fault == "bias_from_gate0" else bias)
        if inp["addend"] is not None:
            z = z + inp["addend"].float()
        return r16(z, dt)
    out = lstm_fwd_model(dict(inp, gates=pre(fault)), fault if fault == "keep_index_dropped" else None)
    rows = -(-b // SM_TS) * SM_TS - b
    return {"pre16": pre(None), "act": out["act"], "c_out": out["c_out"], "h_dsts": [out["h"].clone() for d in inp["dsts"] if d],
            "outside": rows * h if fault == "clamped_rows_written" else 0}


def lg_check(inp, got):
    """module docstring; got: act [B, 4H], c_out, h_dsts (the given destinations), outside (count of changed elements outside the
    views), and in tier B pre16, the unfused product's 16-bit output"""
    dt, res = inp["dtype"], {}
    if inp["tier"] == "A":
        gates = r16(inp["z"], dt)               # (z is exact in fp32: one rounding)
    else:
        gates = got["pre16"]
        res["pre16"] = worst(gates, inp["z"], stored(inp["z"], (inp["K"] + 2) * U * inp["mag"], dt))
    res.update(lstm_fwd_check(dict(inp, gates=gates), got))
    res["outside"] = (INF if got.get("outside") else 0.0, -1)
    return res


# ================================================================================================ prenet_infer
PRE_CASES = [   # B, NM, P, ld_dst - P
    (1, 8, 8, 0),             # smallest shape
    (3, 80, 32, 40),          # strided destination
    (8, 80, 256, 40),         # the network's own shape
    (2, 80, 520, 8),          # second k += 512 trip with one live lane; second trip of the first-layer loop at 256 threads
    (8, 16, 1032, 0),         # grid capped at 64, the column stride wraps
]
PRE_STEPS = [(0, True), (0, False), (1, False), (6, False), (1999, False), (2 ** 31, False)]     # (t, go frame)


def pre_weights(nm, p, dtype, tier, seed):
    if tier == "A":
        return G.grid((p, nm), seed, dtype, "cpu", 4), G.grid((p, p), seed + 1, dtype, "cpu", 4, min(1.0, 16.0 / p))
    g = gen(seed)
    return (torch.randn(p, nm, generator=g) / nm ** 0.5).to(dtype), (torch.randn(p, p, generator=g) / p ** 0.5).to(dtype)


def pack_bits(keep):
    """bool [n] -> uint8 [n / 8], element 8 i + j in bit j of byte i"""
    return (keep.view(-1, 8).to(torch.int32) * (1 << torch.arange(8, dtype=torch.int32))).sum(1).to(U8)


def pre_keep(b, p, seed, t, layer):
    return torch.from_numpy(PO.keep_mask(b * p, 0.5, seed, 1 + 2 * t + layer)).view(b, p)


def _r16_up(v, dtype, up):
    """r16 of an fp64 value through fp32 rounded AWAY from the reference side (up / down), so that the two roundings in a row cannot
    fall short of the one the statement means (r16 is monotone)"""
    f = v.float()
    f = torch.where(f.double() < v, torch.nextafter(f, torch.full_like(f, INF)), f) if up else \
        torch.where(f.double() > v, torch.nextafter(f, torch.full_like(f, -INF)), f)
    return widen(f.to(dtype))


def pre_inputs(case, dtype, tier, t=1, go=False, frame=None, weights=None, seed=None):
    """frame / weights given: the fused frame launch's prenet (frame = what the launch left in frame_next)"""
    b, nm, p, pad = case
    seed = 4321 + b + p if seed is None else seed
    w0, w1 = weights if weights is not None else pre_weights(nm, p, dtype, tier, 9000 + nm + p)
    if frame is None and not go:
        frame = G.grid((b, nm), 9100 + b + nm, F32, "cpu", 255) if tier == "A" else torch.randn(b, nm, generator=gen(9100 + b + nm)) * 2.0
    inp = {"case": case, "dtype": dtype, "tier": tier, "B": b, "NM": nm, "P": p, "pad": pad, "t": t, "seed": seed, "w0": w0, "w1": w1,
           "frame": None if go else frame, "info": {}}
    if tier == "A":
        _pre_exact(inp)                         # asserts the preconditions
    return inp


def _pre_exact(inp):
    """tier A: -> the expected dst, from exact sums (asserted)"""
    dt, b, nm, p = inp["dtype"], inp["B"], inp["NM"], inp["P"]
    xs = widen(r16(inp["frame"], dt)) if inp["frame"] is not None else torch.zeros(b, nm, dtype=F64)
    w0, w1 = widen(inp["w0"]), widen(inp["w1"])
    k0, k1 = pre_keep(b, p, inp["seed"], inp["t"], 0), pre_keep(b, p, inp["seed"], inp["t"], 1)
    z1 = xs @ w0.t()
    _exact(xs.abs() @ w0.abs().t(), z1, Q, 2.0 ** 24, "prenet layer 1")
    h1 = torch.where(k0, 2 * widen(r16(torch.relu(z1), dt)), torch.zeros((), dtype=F64))
    z2 = h1 @ w1.t()
    _exact(h1.abs() @ w1.abs().t(), z2, Q, 2.0 ** 24, "prenet layer 2")
    dst = torch.where(k1, r16(2 * r16(torch.relu(z2), dt).float(), dt), torch.zeros((), dtype=dt))
    assert bool(torch.isfinite(dst.float()).all()) and bool(torch.isfinite(h1).all()), "prenet tier A overflows the 16-bit range"
    return dst, z1


def pre_model(inp, fault=None):
    dt, b, nm, p, t = inp["dtype"], inp["B"], inp["NM"], inp["P"], inp["t"]
    xs = r16(inp["frame"], dt).float() if inp["frame"] is not None else torch.zeros(b, nm)

    def keep(layer):
        if fault == "masks_swapped":
            layer = 1 - layer
        off = 1 + 2 * t + layer
        if fault == "offset_truncated":
            off &= 0xFFFFFFFF
        return torch.from_numpy(PO.keep_mask(b * p, 0.5, inp["seed"], off)).view(b, p)
    k0, k1 = keep(0), keep(1)
    v = torch.relu(xs @ inp["w0"].float().t())
    if fault != "hidden_fp32":
        v = r16(v, dt).float()
    h1 = torch.where(k0, v * 2.0, torch.zeros(()))
    if fault != "hidden_fp32":
        h1 = r16(h1, dt).float()
    w1 = inp["w1"].float()
    if fault == "second_k_trip_skipped":
        w1 = w1.clone()
        w1[:, TRIP:] = 0
    v2 = r16(torch.relu(h1 @ w1.t()), dt).float()
    return {"dst": r16(torch.where(k1, v2 * 2.0, torch.zeros(())), dt), "mask0": pack_bits(k0), "mask1": pack_bits(k1)}


def pre_check(inp, got):
    """module docstring; got: dst [B, P], and mask0 / mask1 (uint8 [B P / 8]) where the launch returns them"""
    dt, b, nm, p, tier = inp["dtype"], inp["B"], inp["NM"], inp["P"], inp["tier"]
    k0, k1 = pre_keep(b, p, inp["seed"], inp["t"], 0), pre_keep(b, p, inp["seed"], inp["t"], 1)
    res = {}
    for key, k in (("mask0", k0), ("mask1", k1)):
        if got.get(key) is not None:
            res[key] = _bitcmp(got[key], pack_bits(k))
    if inp["frame"] is None:
        res["dst"] = _bitcmp(got["dst"], torch.zeros(b, p, dtype=dt))
    elif tier == "A":
        res["dst"] = _bitcmp(got["dst"], _pre_exact(inp)[0])
    else:
        xs, w0, w1 = widen(r16(inp["frame"], dt)), widen(inp["w0"]), widen(inp["w1"])
        z1 = xs @ w0.t()
        e1 = (nm + 1) * U * (xs.abs() @ w0.abs().t())
        mid = widen(r16(torch.relu(z1), dt))        # (fp64 -> fp32 -> 16 bit: a double rounding can differ from r16 by one step only
        hi, lo = _r16_up(torch.relu(z1 + e1), dt, True), _r16_up(torch.relu(z1 - e1), dt, False)      # inside [lo, hi])
        delta = torch.maximum(hi - mid, mid - lo).clamp_min(0)
        inp["info"]["delta_share"] = float((delta > 0).double().mean())
        zero = torch.zeros((), dtype=F64)
        h1, dh = torch.where(k0, 2 * mid, zero), torch.where(k0, 2 * delta, zero)
        z2 = h1 @ w1.t()
        e2 = (p + 1) * U * ((h1.abs() + dh) @ w1.abs().t()) + dh @ w1.abs().t()
        ref = torch.where(k1, 2 * torch.relu(z2), zero)
        bar = torch.where(k1, 2 * stored(torch.relu(z2), e2, dt), zero)
        res["dst"] = worst(got["dst"], ref, bar)
    return res


# ================================================================================================ frame_infer
FR_CASES = [   # B, NM, K, ld_hc - K, ldw - K
    (1, 8, 8, 0, 0),          # one lane live, 3 workgroups
    (3, 80, 160, 8, 16),      # strided operands
    (2, 80, 520, 0, 8),       # second k += 512 trip
    (8, 80, 1536, 0, 0),      # the network's own shape
]
FR_P = [None, 8, 48, 256, 1032]                # None: the unfused launch
FR_LIMITS = [(4, 6), (6, 4)]                   # (out_steps, max_steps); six steps run: two beyond the smaller of the two
FR_STEPS = 6


def _inteq(got, want):
    """(0 | inf, first differing index) of two integer tensors"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return INF, 0
    d = got != want
    return (INF, int(torch.nonzero(d.reshape(-1))[0])) if bool(d.any()) else (0.0, -1)


def fr_lds(b, nm, k, p):
    """the launcher's LDS request"""
    n = (b * k + 1) // 2 * 4
    return n if p is None else n + b * nm * 4 + (b * nm + b * p) * 4 + 2 * b * p // 8


def _sig_undecided(v, e_v, thr):
    """logits whose decision sigmoid(v) <= thr the roundings could turn"""
    s = torch.sigmoid(v)
    return (s - f32(thr)).abs() <= s * (1 - s) * (e_v + C_EXPF * U) + 2 * U * s


def fr_inputs(case, dtype, tier, p, limits, thr=0.5):
    b, nm, k, pad_h, pad_w = case
    out_steps, max_steps = limits
    assert fr_lds(b, nm, k, p) <= 64 * 1024
    g = gen(9500 + b + nm + k)
    if tier == "A":
        hc = G.grid((FR_STEPS, b, k), 9600 + b + k, dtype, "cpu", 4)
        w = G.grid((nm + 1, k), 9700 + nm + k, dtype, "cpu", 4, min(1.0, 32.0 / k))
        bias = torch.randint(-32, 33, (nm + 1,), generator=g).float() / 16
    else:
        hc = torch.randn(FR_STEPS, b, k, generator=g).to(dtype)
        w = (torch.randn(nm + 1, k, generator=g) / k ** 0.5).to(dtype)
        bias = torch.randn(nm + 1, generator=g) * 0.1
    raw = widen(hc) @ widen(w[nm])                                   # [steps, B] gate logits without the bias
    # a quarter of the logits above the threshold: samples finish at different steps, some never
    bias[nm] = float(np.log(thr / (1 - thr))) - float(torch.round(torch.quantile(raw.reshape(-1), 0.75) * 16) / 16)
    if tier == "A":
        bias[nm] = torch.round(bias[nm] * 16) / 16
    inp = {"case": case, "dtype": dtype, "tier": tier, "B": b, "NM": nm, "K": k, "P": p, "hc": hc, "w": w, "bias": bias, "thr": thr,
           "out_steps": out_steps, "max_steps": max_steps, "seed": 77 + b, "w0": None, "w1": None, "info": {}}
    for _ in range(64):
        if int(_fr_undecided(inp).sum()) == 0:
            break
        inp["bias"][nm] -= 1.0 / 16
    _fr_preconditions(inp)
    if p is not None:
        inp["w0"], inp["w1"] = pre_weights(nm, p, dtype, tier, 9000 + nm + p)
    return inp


def fr_scripted(dtype, thr, fused):
    """gate logits scripted a whole 16-bit step either side of the threshold's logit (weight row = e_0, hc[:, 0] = the logit, bias 0:
    exact), three samples that stop at different steps; mel weights k / 4"""
    b, nm, k = 3, 8, 16
    l0 = torch.tensor(float(np.log(thr / (1 - thr)))).to(dtype)
    step = float(S.ulp(widen(l0), dtype))
    lo, hi = float(l0) - step, float(l0) + step                      # lo: goes on; hi: stops
    rows = [[lo, lo, lo], [lo, hi, lo], [lo, lo, lo], [hi, lo, lo], [hi, hi, hi], [lo, lo, lo]]
    hc = G.grid((FR_STEPS, b, k), 9800, dtype, "cpu", 4)
    hc[:, :, 0] = torch.tensor(rows).to(dtype)
    assert torch.equal(hc[:, :, 0].double(), torch.tensor(rows, dtype=F64)), "the scripted logits are not 16-bit values"
    w = G.grid((nm + 1, k), 9801, dtype, "cpu", 4)
    w[nm], w[:, 0] = 0, 0
    w[nm, 0] = 1.0
    inp = {"case": (b, nm, k, 0, 0), "dtype": dtype, "tier": "A", "B": b, "NM": nm, "K": k, "P": 8 if fused else None, "hc": hc, "w": w,
           "bias": torch.zeros(nm + 1), "thr": thr, "out_steps": 8, "max_steps": 8, "seed": 5, "w0": None, "w1": None, "info": {}, "scripted": True}
    _fr_preconditions(inp)
    if fused:
        inp["w0"], inp["w1"] = pre_weights(nm, 8, dtype, "A", 9000 + nm + 8)
    return inp


def _fr_ref(inp):
    """-> out64 [steps, B, NM + 1], its sum of magnitudes, its fp32 bar"""
    hc, w, bias = widen(inp["hc"]), widen(inp["w"]), widen(inp["bias"])
    out, mag = hc @ w.t() + bias, hc.abs() @ w.abs().t() + bias.abs()
    return out, mag, (torch.zeros_like(mag) if inp["tier"] == "A" else (inp["K"] + 1) * U * mag)


def _fr_undecided(inp):
    out, _, bar = _fr_ref(inp)
    return _sig_undecided(out[..., inp["NM"]], bar[..., inp["NM"]], inp["thr"])


def _fr_preconditions(inp):
    out, mag, _ = _fr_ref(inp)
    assert int(_fr_undecided(inp).sum()) == 0, "a gate logit's decision is undefined within its bar"
    if inp["tier"] == "A":              # (scripted: the gate column is one term, the logit itself)
        nm = inp["NM"] if inp.get("scripted") else inp["NM"] + 1
        _exact(mag[..., :nm], out[..., :nm], Q, 2.0 ** 24, "frame")


def fr_book(inp, logits, fault=None):
    """model.py:578-582 + the step words, from logits [steps, B] (fp64 or fp32) -> per step (valid, not_finished, mel_lengths, state)"""
    b = inp["B"]
    nf, ml, state = torch.ones(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    thr = torch.tensor(inp["thr"], dtype=F32).to(logits.dtype)
    steps = []
    for t in range(logits.shape[0]):
        par = t & 1
        tt = int(state[par])
        valid = tt < inp["max_steps"] and (tt <= inp["out_steps"] if fault == "step_at_out_steps_stored" else tt < inp["out_steps"])
        if valid:
            dec = (torch.sigmoid(logits[t]) <= thr).to(torch.int32)
            if fault == "lengths_before_not_finished":
                ml = ml + nf
            nf = nf * dec
            if fault != "lengths_before_not_finished":
                ml = ml + nf
            if int(state[3]) == 0:
                state[2] = tt + 1
                if int(nf.sum()) == 0:
                    state[3] = 1
        state[par if fault == "wrong_parity_advanced" else 1 - par] = tt + 1
        steps.append((valid, tt, nf.clone(), ml.clone(), state.clone()))
    return steps


def fr_model(inp, fault=None):
    dt, b, nm, k = inp["dtype"], inp["B"], inp["NM"], inp["K"]
    w = inp["w"].float()
    if fault == "second_k_trip_skipped":
        w = w.clone()
        w[:, TRIP:] = 0
    out = inp["hc"].float() @ w.t() + inp["bias"]
    book = fr_book(inp, out[..., nm], fault)
    got = {"mel_out": untouched((b, inp["out_steps"], nm), F32), "gate_out": untouched((b, inp["out_steps"]), F32), "frame_next": [],
           "not_finished": [], "mel_lengths": [], "state": [], "pre_dst": [] if inp["P"] is not None else None, "outside": 0}
    for t, (valid, tt, nf, ml, state) in enumerate(book):
        if valid and tt < inp["out_steps"]:
            got["mel_out"][:, tt], got["gate_out"][:, tt] = out[t, :, :nm], out[t, :, nm]
        elif valid:
            got["outside"] += b * (nm + 1)                         # (step_at_out_steps_stored: a row past the end of both buffers)
        got["frame_next"].append(out[t, :, :nm].contiguous())
        got["not_finished"].append(nf)
        got["mel_lengths"].append(ml)
        got["state"].append(state)
        if inp["P"] is not None:
            sub = pre_inputs((b, nm, inp["P"], 0), dt, inp["tier"], tt + 1, frame=got["frame_next"][-1], weights=(inp["w0"], inp["w1"]),
                             seed=inp["seed"])
            got["pre_dst"].append(pre_model(sub, fault if fault in ("second_k_trip_skipped", "hidden_fp32") else None)["dst"])
    return got


def fr_check(inp, got):
    """module docstring; got: mel_out [B, out_steps, NM] and gate_out [B, out_steps] after the last step (NaN before the first),
    and per step lists frame_next, not_finished, mel_lengths, state, pre_dst (fused)"""
    dt, b, nm, tier = inp["dtype"], inp["B"], inp["NM"], inp["tier"]
    out, _, bar = _fr_ref(inp)
    book = fr_book(inp, out[..., nm])
    mel_ref, mel_bar = widen(untouched((b, inp["out_steps"], nm), F32)), torch.zeros(b, inp["out_steps"], nm, dtype=F64)
    gate_ref, gate_bar = widen(untouched((b, inp["out_steps"]), F32)), torch.zeros(b, inp["out_steps"], dtype=F64)
    res = {k: (0.0, -1) for k in ("frame_next", "not_finished", "mel_lengths", "state")}
    if inp["P"] is not None:
        res["pre_dst"] = (0.0, -1)
    shares = []
    for t, (valid, tt, nf, ml, state) in enumerate(book):
        if valid:
            mel_ref[:, tt], mel_bar[:, tt], gate_ref[:, tt], gate_bar[:, tt] = out[t, :, :nm], bar[t, :, :nm], out[t, :, nm], bar[t, :, nm]
        res["frame_next"] = _worse(res["frame_next"], worst(got["frame_next"][t], out[t, :, :nm], bar[t, :, :nm]))
        for key, want in (("not_finished", nf), ("mel_lengths", ml), ("state", state)):
            res[key] = _worse(res[key], _inteq(got[key][t], want))
        if inp["P"] is not None:
            sub = pre_inputs((b, nm, inp["P"], 0), dt, tier, tt + 1, frame=got["frame_next"][t], weights=(inp["w0"], inp["w1"]),
                             seed=inp["seed"])
            res["pre_dst"] = _worse(res["pre_dst"], pre_check(sub, {"dst": got["pre_dst"][t]})["dst"])
            shares.append(sub["info"].get("delta_share", 0.0))
    if shares:
        inp["info"]["delta_share"] = max(shares)
    # (a bar of 0 demands equality: tier A is bit for bit up to the sign of a zero, which no sum of these inputs has; NaN rows: class)
    res["mel_out"], res["gate_out"] = worst(got["mel_out"], mel_ref, mel_bar), worst(got["gate_out"], gate_ref, gate_bar)
    res["outside"] = (INF if got.get("outside") else 0.0, -1)
    return res


# ================================================================================================ dispatch
KERNELS = {"lstm_gemm_fwd": (lg_model, lg_check), "prenet_infer": (pre_model, pre_check), "frame_infer": (fr_model, fr_check)}


def kernel_model(kernel, inp, fault=None):
    """The launch's arithmetic in float32 on the CPU (torch's summation order, a correctly rounded exp); fault: one of FAULTS, planted
    where the launch has the corresponding code; a fault the launch has no place for changes nothing."""
    assert fault is None or fault in FAULTS
    return KERNELS[kernel][0](inp, fault)


def check(kernel, inp, got):
    """-> {output: (largest ratio, flat index)}; every element of every output takes part"""
    return KERNELS[kernel][1](inp, got)
