"""The three launches of the Tacotron2 decoder step -- dle_t2_lstm_gemm_fwd (csrc/gemm_smallm.hip, LSTM = true), dle_t2_prenet_infer
and dle_t2_frame_infer (csrc/tacotron2.hip) -- against the float64 statements and derived per-element bars of
tests/_tacotron2_step_reference.py: |got - ref| / bar <= 1 on EVERY element; exact sums, masks, copies, zeros and the stop
bookkeeping bit for bit (reported as 0 / inf).  Tier A: exactly summable inputs; tier B: realistic ones (the module's docstring).
Every output is a view an odd multiple of 8 elements into a NaN-filled buffer whose other bytes must keep their bits (Framed),
every call runs twice from fresh buffers and must give the same bits.

Largest |error| / bar, GPU (MI355X) | the float32 model on the CPU (tests/test_tacotron2_step_reference_host.py); a record, the pass
condition is <= 1 (test_zz_report_ratios prints the GPU column with -s).  Outputs compared bit for bit are 0 in both columns and
left out: the masks, not_finished, mel_lengths, state, "outside", and in tier A prenet dst and every frame output, pre_dst included.
    output                              GPU fp16  bf16 | CPU fp16  bf16
    lstm_gemm_fwd A act                    0.997 0.998 | 0.997 0.998
    lstm_gemm_fwd A c_out                  0.688 0.688 | 0.688 0.688     on the elements whose bar is at least half C_EXP / C_RCP: 0.341 0.341 | 0.341 0.341
    lstm_gemm_fwd A h                      0.999 1.000 | 0.999 1.000
    lstm_gemm_fwd B pre16 (dle_gemm)       0.964 0.999 | 0.964 0.999
    lstm_gemm_fwd B act                    1.000 1.000 | 1.000 1.000
    lstm_gemm_fwd B c_out                  0.520 0.536 | 0.520 0.505     constant-dominated elements: 0.401 0.420 | 0.374 0.367
    lstm_gemm_fwd B h                      0.998 1.000 | 0.998 1.000
    prenet_infer B dst                     0.984 0.986 | 0.984 0.986
    frame_infer B mel_out                  0.112 0.075 | 0.169 0.075
    frame_infer B gate_out                 0.053 0.001 | 0.040 0.002
    frame_infer B frame_next               0.124 0.075 | 0.169 0.075
    frame_infer B pre_dst                  0.989 0.997 | 0.989 0.997
Nothing left its bar and every exact comparison held on the first run: no kernel arithmetic changed.  One launcher change came out
of the argument checks: dle_t2_lstm_gemm_fwd accepted row pitches below the row (ldx < K, ld_g < 4 H, a destination pitch < H:
overlapping rows, the stores of two samples racing); it now refuses them (csrc/gemm_smallm.hip).  Measured constants: the largest
figure on the elements of c_out dominated by C_EXP / C_RCP is 0.420, at or below 0.5, so both stay as they are; C_EXPF enters no
bar.  The 16-bit figures at 1 are the half ulp of the store.
Share of hidden units whose bar carries an admissible-set term (delta_j > 0; printed per case with -s), largest over the cases:
prenet_infer 0.135 (fp16) / 0.023 (bf16); the fused frame launch 0.292 / 0.083 at P = 8, B = 3 (7 and 2 of 24 units), 0.14 /
0.03 - 0.04 at P >= 256 -- the layer-1 bar (NM + 1) u sum|w0 x| of about 3e-5 against an fp16 spacing of 5e-4 at 0.5 .. 1.

Launch paths reached: each test's docstring.
"""
import pytest
import torch

from tests import _tacotron2_step_reference as T
from tests.test_gpu_smallops_reference import Framed

pytestmark = pytest.mark.gpu

F64, F32, F16, BF16, U8 = T.F64, T.F32, T.F16, T.BF16, T.U8
DTYPES = [F16, BF16]
SKIP = 72                       # 9 x 8 elements: 16-byte aligned for every element size used here
RATIOS = {}
WHERE = {}


def _ops():
    from deeplearningexamples_amd.tacotron2 import ops
    return ops


def _judge(kernel, inp, got, where):
    """record and assert every output's largest ratio (the figures are printed before the assertion decides)"""
    res = T.check(kernel, inp, got)
    bad = []
    for out, (r, i) in sorted(res.items()):
        key = "%s %s %s %s" % (kernel, inp["tier"], out, T.name(inp["dtype"]))
        if r >= RATIOS.get(key, 0.0):
            WHERE[key] = where
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print("    %-44s %-34s %.3f" % (key, where, r))
        if not r <= 1.0:
            bad.append("%s %s: |error| / bar = %.3f at flat index %d" % (key, where, r, i))
    if "delta_share" in inp.get("info", {}):
        print("    %-44s %-34s share of hidden units with an admissible-set term: %.4f" % (kernel, where, inp["info"]["delta_share"]))
    assert not bad, "; ".join(bad)
    return res


def _flat(got):
    for k in sorted(got):
        v = got[k]
        for t in (v if isinstance(v, list) else [v]):
            if isinstance(t, torch.Tensor):
                yield k, t


def _same_bits(u, v):
    return u.dtype == v.dtype and u.shape == v.shape and bool(torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)))


def _twice(fn):
    """determinism: the same call from fresh buffers twice gives the same bits in every output"""
    a, b = fn(), fn()
    for (k, u), (_, v) in zip(_flat(a), _flat(b)):
        assert _same_bits(u, v), "two identical calls differ in %s" % k
    return a


def _dev(t, cuda):
    return None if t is None else t.to(cuda)


def _strided(t, ld, cuda, off=0):
    """a [rows, cols] device copy of `t` with row stride ld, `off` elements into its rows"""
    base = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=cuda)
    base[:, off:off + t.shape[1]] = t.to(cuda)
    return base[:, off:off + t.shape[1]]


# ------------------------------------------------------------------------------------------------ lstm_gemm_fwd
def _lg_run(cuda, inp):
    ops = _ops()
    dt, b, h, k = inp["dtype"], inp["B"], inp["H"], inp["K"]
    x = _strided(inp["x"], k + 16, cuda, 8)                    # a column slice 8 elements into a wider buffer
    gates = Framed(b, 4 * h, 4 * h + 8, dt, cuda, skip=SKIP)
    add = _strided(inp["addend"], 4 * h + 8, cuda) if inp["addend"] is not None else None
    c_out = Framed(b, h, h, F32, cuda, skip=SKIP)
    dsts = [Framed(b, h, ld, dt, cuda, skip=SKIP) if given else None for given, ld in zip(inp["dsts"], (h + 8, 2 * h, 3 * h + 16))]
    ops.lstm_gemm_fwd(x, inp["w"].to(cuda), _dev(inp["bias"], cuda), add, inp["c_prev"].to(cuda), c_out.t, gates.t,
                      [d.t if d is not None else None for d in dsts], keep=_dev(inp["keep"], cuda), keep_index=inp["keep_index"],
                      p=inp["p"] or 0.0)
    torch.cuda.synchronize()
    return {"act": gates.check("lstm_gemm_fwd gates").cpu(), "c_out": c_out.check("lstm_gemm_fwd c_out").cpu(),
            "h_dsts": [d.check("lstm_gemm_fwd destination").cpu() for d in dsts if d is not None], "outside": 0}


def _lg_unfused_pre16(cuda, inp):
    """the 16-bit output of the unfused product on the same operands (tier B's staging)"""
    from deeplearningexamples_amd import functional as F, _cabi as C
    dt, b, h, k = inp["dtype"], inp["B"], inp["H"], inp["K"]
    pre = Framed(b, 4 * h, 4 * h, dt, cuda, skip=SKIP)
    add = _dev(inp["addend"], cuda)
    F.gemm(_strided(inp["x"], k + 16, cuda, 8), inp["w"].to(cuda), b, 4 * h, k, True, True, out=pre.t, bias=_dev(inp["bias"], cuda),
           act=C.ACT_ADD if add is not None else C.ACT_NONE, mask_src=add)
    torch.cuda.synchronize()
    return pre.check("dle_gemm").cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("case", T.LG_CASES, ids=lambda c: c[0])
def test_lstm_gemm_fwd(cuda, case, tier, dtype):
    """One tile with one chunk of 8 and 63 clamped rows (1 x 8 x 8); a second chunk 8 wide (K = 136); the row-tile edge 63 / 64 / 65
    with nk = 3 = NST - 1 of the four-stage form; three row tiles, the last with one row, and a ring that wraps (129 x 8 x 648); the
    three-stage form (258 tiles) with nk = 2 = NST - 1 and with a wrap; the two cells of the inference step (B = 8, bias only, no
    keep) and the trainer's (B = 128, addend and keep).  x a column slice 8 elements into a wider buffer, ld_g = 4 H + 8, the
    destinations at pitches H + 8, 2 H, 3 H + 16, d0 = NULL with d1 set in two cases, all three in two; keep_index 0, 40 and 3."""
    inp = T.lg_inputs(case, dtype, tier)
    pre16 = _lg_unfused_pre16(cuda, inp) if tier == "B" else None
    for kidx in case[7]:
        at = T.lg_at(inp, kidx)
        got = _twice(lambda: _lg_run(cuda, at))
        got["pre16"] = pre16
        _judge("lstm_gemm_fwd", at, got, "%s keep_index %d" % (case[0], kidx))


# ------------------------------------------------------------------------------------------------ prenet_infer
def _pre_run(cuda, inp, parity):
    b, nm, p, pad = inp["case"]
    dt, t = inp["dtype"], inp["t"]
    dst = Framed(b, p, p + pad, dt, cuda, skip=SKIP)
    m0, m1 = Framed(1, b * p // 8, b * p // 8, U8, cuda, skip=SKIP), Framed(1, b * p // 8, b * p // 8, U8, cuda, skip=SKIP)
    state = torch.tensor([t, t + 100, 0, 0] if parity == 0 else [t + 100, t, 0, 0], dtype=torch.int64, device=cuda)
    _ops().prenet_infer(_dev(inp["frame"], cuda), inp["w0"].to(cuda), inp["w1"].to(cuda), dst.t, inp["seed"], state[parity:],
                        m0.t.view(-1), m1.t.view(-1))
    torch.cuda.synchronize()
    return {"dst": dst.check("prenet_infer dst").cpu(), "mask0": m0.check("prenet_infer mask0").cpu().view(-1),
            "mask1": m1.check("prenet_infer mask1").cpu().view(-1)}


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("case", T.PRE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_prenet_infer(cuda, case, tier, dtype):
    """The smallest shape (1 x 8 x 8); a strided destination whose columns beyond P keep their bits; the network's own shape;
    P = 520: the second k += 512 trip with one live lane and the second trip of the first-layer loop at 256 threads; P = 1032: the
    grid capped at 64 workgroups, the column stride wraps.  Steps 0 (the go frame, and a frame), 1, 6, 1999 and 2^31 (the call
    offset 1 + 2 t + l carries into its high word), read from the even and the odd state word in turn."""
    for i, (t, go) in enumerate(T.PRE_STEPS):
        inp = T.pre_inputs(case, dtype, tier, t, go)
        _judge("prenet_infer", inp, _twice(lambda: _pre_run(cuda, inp, i & 1)), "%s t %d%s" % ("x".join(map(str, case)), t, " go" if go else ""))


# ------------------------------------------------------------------------------------------------ frame_infer
def _fr_run(cuda, inp):
    ops = _ops()
    b, nm, k, pad_h, pad_w = inp["case"]
    dt, p, out_steps = inp["dtype"], inp["P"], inp["out_steps"]
    mel, gate = Framed(b, out_steps * nm, out_steps * nm, F32, cuda, skip=SKIP), Framed(b, out_steps, out_steps, F32, cuda, skip=SKIP)
    frame = Framed(b, nm, nm, F32, cuda, skip=SKIP)
    nf, ml = Framed(1, b, b, torch.int32, cuda, skip=SKIP), Framed(1, b, b, torch.int32, cuda, skip=SKIP)
    nf.t.fill_(1)
    ml.t.fill_(0)
    words = torch.full((12,), -7, dtype=torch.int64, device=cuda)
    state = words[4:8]
    state.zero_()
    w, bias = _strided(inp["w"], k + pad_w, cuda), inp["bias"].to(cuda)
    pre = Framed(b, p, p + 8, dt, cuda, skip=SKIP) if p is not None else None
    prenet = (inp["w0"].to(cuda), inp["w1"].to(cuda), pre.t) if p is not None else None
    got = {"frame_next": [], "not_finished": [], "mel_lengths": [], "state": [], "pre_dst": [] if p is not None else None, "outside": 0}
    for t in range(inp["hc"].shape[0]):
        frame.t.fill_(float("nan"))                            # (written at every step, stored or not)
        if pre is not None:
            pre.t.fill_(float("nan"))
        ops.frame_infer(_strided(inp["hc"][t], k + pad_h, cuda), w, bias, mel.t.view(b, out_steps, nm), gate.t, frame.t, nf.t.view(-1),
                        ml.t.view(-1), state, t & 1, inp["thr"], inp["max_steps"], prenet=prenet, seed=inp["seed"])
        torch.cuda.synchronize()
        got["frame_next"].append(frame.check("frame_infer frame_next").cpu().clone())
        got["not_finished"].append(nf.check("frame_infer not_finished").cpu().view(-1).clone())
        got["mel_lengths"].append(ml.check("frame_infer mel_lengths").cpu().view(-1).clone())
        got["state"].append(state.cpu().clone())
        if pre is not None:
            got["pre_dst"].append(pre.check("frame_infer pre_dst").cpu().clone())
    assert words[:4].tolist() == [-7] * 4 and words[8:].tolist() == [-7] * 4, "frame_infer wrote next to its state words"
    got["mel_out"] = mel.check("frame_infer mel_out").cpu().view(b, out_steps, nm)
    got["gate_out"] = gate.check("frame_infer gate_out").cpu()
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("p", T.FR_P, ids=lambda p: "unfused" if p is None else "P%d" % p)
@pytest.mark.parametrize("case", T.FR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_frame_infer(cuda, case, p, tier, dtype):
    """One live lane in 3 workgroups (1 x 8 x 8); strided hc and w; K = 520: the second k += 512 trip; the network's own shape.
    Unfused (256 threads per workgroup, one column per wavefront) and fused with P = 8, 48, 256 and 1032 (one workgroup of 1024
    threads; P = 1032 takes the second trip of the first-layer loop at 1024 threads and fits the 64 KiB check with K = 1536).  Six
    steps against out_steps = 4 < max_steps = 6 and max_steps = 4 < out_steps = 6: two steps beyond the limit are counted, not
    stored (NaN rows stay), frame_next and the fused pre_dst are still written.  The bookkeeping from the float64 logits, after every
    step; no logit is undecided (asserted by the builder)."""
    for limits in T.FR_LIMITS:
        inp = T.fr_inputs(case, dtype, tier, p, limits)
        _judge("frame_infer", inp, _twice(lambda: _fr_run(cuda, inp)), "%s %s out %d max %d" % (
            "x".join(map(str, case)), "unfused" if p is None else "P %d" % p, limits[0], limits[1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_frame_infer_threshold_other_than_half(cuda, fused, dtype):
    """gate_threshold = 0.3 with logits scripted one whole 16-bit step either side of ln(0.3 / 0.7): the samples stop at steps 3, 1
    and 4, the all-finished word is set at step 4 and n_steps stays 5"""
    inp = T.fr_scripted(dtype, 0.3, fused)
    got = _twice(lambda: _fr_run(cuda, inp))
    _judge("frame_infer", inp, got, "scripted thr 0.3")
    assert got["mel_lengths"][-1].tolist() == [3, 1, 4] and got["state"][-1].tolist() == [6, 5, 5, 1]


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_without_a_launch(cuda):
    """B = 9 for both inference entry points, K % 8 != 0, parity = 2, a row pitch below K / P / H, the fused form without w1,
    B = 8 with K = 4104 (LDS above 64 KiB), lstm_gemm with H = 12, a misaligned x and fp32 operands: ValueError, nothing launched
    (the row pitches of dle_t2_lstm_gemm_fwd were unchecked before this test; its launcher now refuses a pitch below the row)."""
    from deeplearningexamples_amd import _cabi as C
    ops = _ops()
    z = lambda *s, dt=F16: torch.zeros(*s, dtype=dt, device=cuda)
    zi = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=cuda)

    def prenet(b=2, nm=8, p=8, dst=None):
        ops.prenet_infer(z(b, nm, dt=F32), z(p, nm), z(p, p), dst if dst is not None else z(b, p), 1, zi(4, torch.int64))

    def frame(b=2, nm=8, k=16, parity=0, hc=None, prenet=None):
        ops.frame_infer(hc if hc is not None else z(b, k), z(nm + 1, k), z(nm + 1, dt=F32), z(b, 4, nm, dt=F32), z(b, 4, dt=F32),
                        z(b, nm, dt=F32), zi(b), zi(b), zi(4, torch.int64), parity, 0.5, 4, prenet=prenet)

    def lstm(b=2, h=8, k=16, x=None, dt=F16, dst=None, gates=None):
        ops.lstm_gemm_fwd(x if x is not None else z(b, k, dt=dt), z(4 * h, k, dt=dt), None, None, z(b, h, dt=F32), z(b, h, dt=F32),
                          gates if gates is not None else z(b, 4 * h, dt=dt), [dst if dst is not None else z(b, h, dt=dt)])
    narrow = lambda rows, cols: torch.as_strided(z(rows * cols), (rows, cols), (8, 1))          # overlapping rows: pitch 8 < cols
    bad = [lambda: prenet(b=9), lambda: frame(b=9), lambda: frame(k=12), lambda: lstm(k=12), lambda: prenet(nm=12), lambda: frame(parity=2),
           lambda: prenet(p=16, dst=narrow(2, 16)), lambda: frame(hc=narrow(2, 16)),
           lambda: frame(prenet=(z(16, 8), z(16, 16), narrow(2, 16))), lambda: frame(b=8, k=4104), lambda: lstm(h=12),
           lambda: lstm(x=z(2, 24)[:, 4:20]), lambda: lstm(dt=F32), lambda: lstm(x=narrow(2, 16)), lambda: lstm(dst=narrow(2, 16), h=16),
           lambda: lstm(gates=narrow(2, 32))]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("argument check %d let the call through" % i)
    # the fused form without w1 (the wrapper itself insists on both weights: straight to the entry point)
    hc, w, bias, mel, gate, fr = z(2, 16), z(9, 16), z(9, dt=F32), z(2, 4, 8, dt=F32), z(2, 4, dt=F32), z(2, 8, dt=F32)
    nf, ml, st, w0, dst = zi(2), zi(2), zi(4, torch.int64), z(8, 8), z(2, 8)
    with pytest.raises(ValueError):
        C.call("dle_t2_frame_infer", C.ptr(hc), 16, C.ptr(w), 16, C.ptr(bias), C.ptr(mel), C.ptr(gate), C.ptr(fr), C.ptr(nf), C.ptr(ml),
               C.ptr(st), 0, 0.5, 4, 4, C.ptr(w0), 0, C.ptr(dst), 8, 0, 2, 8, 16, 8, C.dt(hc), C.stream())
    torch.cuda.synchronize()
    assert float(mel.abs().max()) == 0 and st.tolist() == [0, 0, 0, 0]


def test_zz_report_ratios():
    print()
    for k in sorted(RATIOS):
        print("    %-44s %.3f   %s" % (k, RATIOS[k], WHERE.get(k, "")))
