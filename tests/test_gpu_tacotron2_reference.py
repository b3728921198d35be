"""The twelve training kernels of csrc/tacotron2.hip (t2_tanh, t2_lstm_{fwd,bwd} in both template forms, t2_attention_{fwd,bwd}
without and with the fused location term, t2_location_bwd, t2_mel_loss + t2_sum, t2_mask_rows, t2_sum_steps) against the float64
statements and derived per-element bars of tests/_tacotron2_reference.py: |got - ref| / bar <= 1 on EVERY element; copies, zeros,
flags and 16-bit roundings of a returned fp32 value bit for bit (reported as 0 / inf).  Every output is a view inside a NaN-filled
buffer whose other bytes must keep their bits (Framed), every call runs twice from fresh buffers and must give the same bits.

Largest |error| / bar, GPU (MI355X) | the float32 model on the CPU (tests/test_tacotron2_reference_host.py); a record, the pass
condition is <= 1 (test_zz_report_ratios prints the GPU column with -s):
    output                     GPU fp16  bf16 | CPU fp16  bf16
    lstm_fwd act                  1.000 1.000 | 1.000 1.000
    lstm_fwd c_out                0.600 0.557 | 0.654 0.596     on the elements whose bar is at least half C_EXP / C_RCP: 0.410 0.400 | 0.388 0.382
    lstm_fwd h                    0.999 1.000 | 0.999 1.000     out_dst: bit for bit
    lstm_bwd dgates               1.000 1.000 | 1.000 1.000     dh_prev: bit for bit
    lstm_bwd dc_prev              0.869 0.892 | 0.869 0.892     constant-dominated elements: 0.357 0.371 | 0.344 0.329
    attention_fwd tanh_out        1.000 1.000 | 1.000 1.000     awc_next: bit for bit
    attention_fwd aw_out          0.649 0.636 | 0.029 0.029
    attention_fwd ctx             0.997 0.999 | 0.997 0.999
    attention_bwd d_pl            0.997 0.999 | 0.997 0.999     dctx16: bit for bit
    attention_bwd dq              0.047 0.025 | 0.047 0.025     dq16 (dq NULL, else bit for bit): 0.011 0.110 | 0.011 0.110
    attention_bwd dv_acc          0.114 0.123 | 0.122 0.123
    attention_bwd d_memory        0.982 0.985 | 0.982 0.985
    attention_bwd d_pm_acc        0.962 0.981 | 0.962 0.981
    attention_bwd d_prev          0.014 0.018 | 0.023 0.018     d_cum: 0.145 0.085 | 0.145 0.085
    location_bwd d_prev           0.500 0.450 | 0.500 0.450     d_cum: 0.752 0.752 | 0.752 0.752
    mel_loss loss                 0.023 0.028 | 0.077 0.037     d_out, d_post: 1.000
    sum_steps out                 0.999 1.000 | 0.999 1.000
    tanh_fwd y                    0.923 0.992 | 0.923 0.992     mask_rows: exact
Nothing left its bar: no kernel or wrapper change came out of this test.  The fp32 outputs near 1 (d_memory, d_pm_acc, sum_steps at
n = 1) are single roundings measured against u |value|, i.e. against their own half ulp.
aw_out, GPU 0.649 against 0.029 on the CPU: the largest ratios sit at weights far below the maximum (max - en of several tens),
where the bar is the derived 2.25 (max - en) u of __expf's argument product and of the fp32 constant log2 e, which the CPU model
(a correctly rounded exp) does not spend.  C_EXP is nowhere more than 2 of the at least 27 u of an aw_out bar, so the rule for the
measured constants does not bear on it.
Measured constants.  The first run of this test, with C_EXP = C_RCP = 2 u, recorded 0.505 (fp16) and 0.493 (bf16) on the elements
of c_out whose bar is at least half made of the two constants (fast_tanh of a gate near 0, absolute (C_EXP / 2 + 1 + C_RCP) u, the
reciprocal holding the largest share) and 0.392 / 0.408 on those of dc_prev.  Above 0.5, so by the rule of _smallops_reference the
dominating constant was raised to the smallest integer that brings the figure to 0.5 or below: C_RCP = 3 u gives 0.410 / 0.400 and
0.357 / 0.371 (the table above; C_EXP = 3 u instead would have given 0.450 / 0.439).  The smallops tests pass with it; the one figure
of theirs that C_RCP enters, act_bwd gelu's fp32 part, moved from 0.297 to 0.234.
The 16-bit figures at 1 are the half ulp of the store.

Launch paths reached: each test's docstring.  A text length of 0 is 0 / 0 in the softmax, here as in the reference model; no
caller passes it and no case does.
"""
import pytest
import torch

from tests import _tacotron2_reference as R
from tests.test_gpu_smallops_reference import Framed

pytestmark = pytest.mark.gpu

F64, F32, F16, BF16, U8 = R.F64, R.F32, R.F16, R.BF16, R.U8
DTYPES = [F16, BF16]
RATIOS = {}
WHERE = {}


def _ops():
    from deeplearningexamples_amd.tacotron2 import ops
    return ops


def _judge(kernel, inp, got, where):
    """record and assert every output's largest ratio (the figures are printed before the assertion decides)"""
    res = R.check(kernel, inp, got)
    bad = []
    for out, (r, i) in sorted(res.items()):
        key = "%s %s %s" % (kernel, out, R.name(inp["dtype"]))
        if r >= RATIOS.get(key, 0.0):
            WHERE[key] = where
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print("    %-36s %-28s %.3f" % (key, where, r))
        if not r <= 1.0:
            bad.append("%s %s: |error| / bar = %.3f at flat index %d" % (key, where, r, i))
    assert not bad, "; ".join(bad)
    return res


def _flat(got):
    for k in sorted(got):
        v = got[k]
        for t in (v if isinstance(v, list) else [v]):
            if t is not None:
                yield k, t


def _twice(fn):
    """determinism: the same call from fresh buffers twice gives the same bits in every output"""
    a, b = fn(), fn()
    for (k, u), (_, v) in zip(_flat(a), _flat(b)):
        assert torch.equal(R.bits(u), R.bits(v)), "two identical calls differ in %s" % k
    return a


def _dev(t, cuda):
    return None if t is None else t.to(cuda)


def _strided(t, ld, cuda):
    """a [rows, cols] device copy of `t` with row stride ld"""
    base = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=cuda)
    base[:, :t.shape[1]] = t.to(cuda)
    return base[:, :t.shape[1]]


# ------------------------------------------------------------------------------------------------ LSTM cell
def _lstm_fwd(cuda, inp):
    ops = _ops()
    cid, b, h, p, live, kidx, off = inp["case"][:7]
    dt = inp["dtype"]
    gates = Framed(b, 4 * h, 4 * h + 8, dt, cuda, skip=64 + off, fill=inp["gates"].to(cuda))
    c_out = Framed(b, h, h, F32, cuda)
    d0, d1 = Framed(b, h, h + 8, dt, cuda), Framed(b, h, 2 * h, dt, cuda)
    out_dst = Framed(b, h, 3 * h, dt, cuda) if live else None
    ops.lstm_fwd(gates.t, inp["c_prev"].to(cuda), c_out.t, [d0.t, d1.t], keep=_dev(inp["keep"], cuda), keep_index=kidx, p=p or 0.0,
                 live=_dev(inp["live"], cuda), h_prev=_dev(inp["h_prev"], cuda), out_dst=out_dst.t if live else None)
    torch.cuda.synchronize()
    return {"act": gates.check("lstm_fwd gates").cpu(), "c_out": c_out.check("lstm_fwd c_out").cpu(),
            "h_dsts": [d0.check("lstm_fwd d0").cpu(), d1.check("lstm_fwd d1").cpu()],
            "out_dst": out_dst.check("lstm_fwd out_dst").cpu() if live else None}


def _lstm_bwd(cuda, inp):
    ops = _ops()
    cid, b, h, p, live, kidx, off = inp["case"][:7]
    dt = inp["dtype"]
    act = Framed(b, 4 * h, 4 * h + 8, dt, cuda, skip=64 + off, fill=inp["act"].to(cuda))
    dgates = act if inp["alias"] else Framed(b, 4 * h, 4 * h + 16, dt, cuda, skip=64 + off)
    dc_prev = Framed(b, h, h, F32, cuda)
    dh_prev = Framed(b, h, h, F32, cuda) if live else None
    dh = [_strided(t, h + 4 * k, cuda) for k, t in enumerate(inp["dh"])]
    ops.lstm_bwd(dh[0], inp["dc_next"].to(cuda), act.t, inp["c_prev"].to(cuda), dgates.t, dc_prev.t, keep=_dev(inp["keep"], cuda),
                 keep_index=kidx, p=p or 0.0, live=_dev(inp["live"], cuda), dh_prev=dh_prev.t if live else None, dh_add=tuple(dh[1:]))
    torch.cuda.synchronize()
    if not inp["alias"]:
        assert torch.equal(R.bits(act.check("lstm_bwd act").cpu()), R.bits(inp["act"])), "lstm_bwd changed the saved activations"
    return {"dgates": dgates.check("lstm_bwd dgates").cpu(), "dc_prev": dc_prev.check("lstm_bwd dc_prev").cpu(),
            "dh_prev": dh_prev.check("lstm_bwd dh_prev").cpu() if live else None}


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.LSTM_CASES, ids=lambda c: c[0])
def test_lstm_cell(cuda, case, dtype):
    """t2_lstm_fwd / t2_lstm_bwd.  Scalar form (VEC = false), reached three ways: H % 8 != 0 (3 x 20), keep_index % 8 != 0 (5 x 32 at
    4: the (keep[e >> 3] >> (e & 7)) & 1 addressing), a gates / activations view 2 elements into its buffer (4 x 64, no dropout).
    Vector form: one group per row (3 x 8), a strided slice with keep_index = 40 (7 x 96), and 2064 x 1024 = 264 192 items, one
    grid-stride trip beyond the launcher's 2048 x 128.  live rows (state carried, out_dst zero) in four of the six, keep masks with
    whole bytes of 0x00 and 0xFF; the backward with zero, one and two extra dh pieces (row-strided) and dgates aliasing act in three."""
    assert R.lstm_items(case) > R.LSTM_CAP * R.LSTM_BLOCK or case[0] != "vec_second_trip"
    inp = R.lstm_inputs(case, dtype)
    _judge("lstm_fwd", inp, _twice(lambda: _lstm_fwd(cuda, inp)), case[0])
    inp = R.lstm_bwd_inputs(case, dtype)
    _judge("lstm_bwd", inp, _twice(lambda: _lstm_bwd(cuda, inp)), case[0])


# ------------------------------------------------------------------------------------------------ attention step
def _att_fwd(cuda, inp):
    ops = _ops()
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]
    tanh_out, aw_out, nxt = Framed(b * ti, a, a, dt, cuda), Framed(b, ti, ti, F32, cuda), Framed(b * ti, 8, 8, dt, cuda)
    dsts = [Framed(b, e, e + 8 * k, dt, cuda) for k in range(inp["ndst"])]
    ops.attention_fwd(inp["q"].to(cuda), inp["pl"].to(cuda), inp["v"].to(cuda), inp["memory"].to(cuda), inp["lengths"].to(cuda),
                      _dev(inp["awc_prev"], cuda), tanh_out.t, aw_out.t, nxt.t, [d.t for d in dsts], wloc=_dev(inp["wloc"], cuda), kl=inp["KL"])
    torch.cuda.synchronize()
    return {"tanh_out": tanh_out.check("attention_fwd tanh_out").cpu(), "aw_out": aw_out.check("attention_fwd aw_out").cpu(),
            "awc_next": nxt.check("attention_fwd awc_next").cpu(), "ctx": [d.check("attention_fwd ctx").cpu() for d in dsts]}


def _att_bwd(cuda, inp):
    ops = _ops()
    dt, b, ti, a, e = inp["dtype"], inp["B"], inp["Ti"], inp["A"], inp["E"]

    def acc(t, rows, cols):
        return None if t is None else Framed(rows, cols, cols, F32, cuda, fill=t.to(cuda))
    fr = {"d_memory": acc(inp["d_memory"], b * ti, e), "d_pl": Framed(b * ti, a, a, dt, cuda),
          "dq": Framed(b, a, a, F32, cuda) if inp["has_dq"] else None, "dq16": Framed(b, a, a, dt, cuda) if inp["has_dq16"] else None,
          "dctx16": Framed(b, e, e, dt, cuda) if inp["has_dctx16"] else None, "dv_acc": acc(inp["dv_acc"], b, a),
          "d_pm_acc": acc(inp["d_pm_acc"], b * ti, a), "d_prev": Framed(b, ti, ti, F32, cuda) if inp["KK"] else None,
          "d_cum": acc(inp["d_cum"], b, ti)}
    v = {k: (f.t if f is not None else None) for k, f in fr.items()}
    dc = [_strided(t, e + 4 * (k + 1), cuda) for k, t in enumerate(inp["dc"])]
    daw = [t.to(cuda) for t in inp["daw"]]
    ops.attention_bwd(dc[0], daw[0], inp["aw"].to(cuda), inp["tanh_out"].to(cuda), inp["v"].to(cuda), inp["memory"].to(cuda),
                      v["d_memory"], v["d_pl"], v["dq"], v["dv_acc"], v["d_pm_acc"], d_ctx_add=tuple(dc[1:]),
                      d_aw_add=daw[1] if len(daw) > 1 else None, dq16=v["dq16"], dctx16=v["dctx16"], wloc_t=_dev(inp["wloc_t"], cuda),
                      kl=inp["KL"], d_prev=v["d_prev"], d_cum=v["d_cum"])
    torch.cuda.synchronize()
    return {k: (f.check("attention_bwd " + k).cpu() if f is not None else None) for k, f in fr.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.ATT_CASES, ids=lambda c: c[0])
def test_attention_step(cuda, case, dtype):
    """t2_attention_fwd / t2_attention_bwd, staged as the reference module states.  Without the location term: A / 8 = 3 and E / 8 = 5
    (lpa = 4, lpe = 8: clamped lanes that must add nothing), lengths 23 / 1 / 12 with Ti = 23 = 5 passes of 4 rows + a partly clamped
    one; E of one group with awc_prev == NULL; A = E = 512 (lpa = lpe = 64: the row folds after the loops run no iteration); Ti =
    1100 (two trips of the per-thread loops over t, of the max and of the sum); lengths above Ti (clamped); the default widths.  With
    wloc / wlocT: Ti32 = 32 != 23 with KL = 31, KK = 64; KL = 5, KK = 32; Ti = 2 < KL / 2 + 1; the default widths at Ti = 160.
    Energies from saturated tanh more than 104 apart (exp underflows to exactly 0 inside the length), equal rows and rows one
    16-bit step apart.  Backward from the float32 model's saved tensors: one, two and three row-strided context pieces, one and two
    weight-gradient pieces, d_memory / dq / d_pm_acc given and NULL, dq16 and dctx16; accumulation bases of order 1."""
    inp = R.att_inputs(case, dtype)
    got = _twice(lambda: _att_fwd(cuda, inp))
    _judge("attention_fwd", inp, got, case[0])
    if case[0] in R.ATT_TWIN:
        twin = _att_fwd(cuda, R.att_inputs(case, dtype, lengths=R.ATT_TWIN[case[0]]))
        for (k, u), (_, w) in zip(_flat(got), _flat(twin)):
            assert torch.equal(R.bits(u), R.bits(w)), "lengths above Ti are not clamped to Ti: %s differs" % k
    inp = R.att_bwd_inputs(case, dtype)
    _judge("attention_bwd", inp, _twice(lambda: _att_bwd(cuda, inp)), case[0])


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
def test_tanh_fwd(cuda, dtype):
    """t2_tanh over a grid of exponents from the smallest subnormal to saturation, +-0, +-inf, NaN (one workgroup)"""
    from deeplearningexamples_amd import _cabi as C
    inp = R.tanh_inputs(None, dtype)
    n = inp["x"].numel()
    xd = inp["x"].to(cuda)

    def run():
        y = Framed(1, n, n, dtype, cuda)
        C.call("dle_t2_tanh_fwd", C.ptr(xd), C.ptr(y.t), n, C.dt(dtype), C.stream())
        torch.cuda.synchronize()
        return {"y": y.check("tanh_fwd").cpu().view(-1)}
    _judge("tanh_fwd", inp, _twice(run), "grid")
    y = _ops().tanh_fwd(xd).cpu()
    assert R.same_cast(y, run()["y"]), "the wrapper's own output differs"


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.LOC_CASES, ids=lambda c: "x".join(map(str, c)))
def test_location_bwd(cuda, case, dtype):
    """t2_location_bwd: KL = 31 > Ti = 23, KL = 5, Ti = 2 < KL / 2 + 1, and 70 x 3800 = 266 000 items > 1024 x 256 (second trip);
    d_prev written, d_cum accumulated onto a base of order 1, every position checked"""
    inp = R.loc_inputs(case, dtype)
    b, ti, kl = case

    def run():
        d_prev, d_cum = Framed(b, ti, ti, F32, cuda), Framed(b, ti, ti, F32, cuda, fill=inp["d_cum"].to(cuda))
        _ops().location_bwd(inp["dcol"].to(cuda), d_prev.t, d_cum.t, b, ti, kl)
        torch.cuda.synchronize()
        return {"d_prev": d_prev.check("location_bwd d_prev").cpu(), "d_cum": d_cum.check("location_bwd d_cum").cpu()}
    _judge("location_bwd", inp, _twice(run), str(case))


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("scale", R.MEL_SCALES, ids=["noscale", "scale"])
@pytest.mark.parametrize("case", R.MEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mel_loss(cuda, case, scale, dtype):
    """t2_mel_loss + t2_sum at R n_mel = 7, 80 (one workgroup, partly idle) and 264 000 (> 1024 x 256: second trip, 1024 partials);
    out_all and d_out row-strided wider than n_mel, scale NULL and 2^-3"""
    inp = R.mel_inputs(case, dtype, scale)
    r, nm, ldo, ldd = case

    def run():
        d_out, d_post = Framed(r, nm, ldd, dtype, cuda), Framed(1, r * nm, r * nm, dtype, cuda)
        sc = None if scale is None else torch.tensor([scale], dtype=F32, device=cuda)
        loss = _ops().mel_loss(_strided(inp["out_all"], ldo, cuda), inp["post"].to(cuda), inp["target"].to(cuda), nm, sc, d_out.t, d_post.t.view(-1))
        torch.cuda.synchronize()
        return {"loss": loss.cpu(), "d_out": d_out.check("mel_loss d_out").cpu(), "d_post": d_post.check("mel_loss d_post").cpu().view(-1)}
    _judge("mel_loss", inp, _twice(run), "%s %s" % (case, scale))


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("r", R.SUM_STEPS_R)
@pytest.mark.parametrize("n", R.SUM_STEPS_N)
def test_sum_steps(cuda, n, r, dtype):
    """t2_sum_steps: n = 1, 3 (tail only), 4 (one unrolled body), 7, 9 (bodies + tails of 3 and 1); R = 8 (one item) and 4104 (513
    items: three workgroups, the last partly idle); accumulated onto a base of order 1"""
    inp = R.sum_steps_inputs((n, r), dtype)

    def run():
        out = Framed(1, r, r, F32, cuda, fill=inp["out"].to(cuda))
        _ops().sum_steps(inp["x"].to(cuda), out.t.view(-1))
        torch.cuda.synchronize()
        return {"out": out.check("sum_steps").cpu().view(-1)}
    _judge("sum_steps", inp, _twice(run), "n=%d R=%d" % (n, r))


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=R.name)
@pytest.mark.parametrize("case", R.MASK_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "_%g" % c[5])
def test_mask_rows(cuda, case, dtype):
    """t2_mask_rows, exact: lengths 0, To and above To, ld > cols (the columns between keep their bits), fill 0 and 1e3, fp32 and
    16-bit; 3 x 1100 x 80 = 264 000 > 262 144 items (second trip)"""
    inp = R.mask_inputs(case, dtype)
    b, to, cols, ld, lens, fill = case

    def run():
        x = Framed(b * to, ld, ld, dtype, cuda, fill=inp["x"].to(cuda))
        _ops().mask_rows(x.t, cols, inp["lengths"].to(cuda), b, to, fill)
        torch.cuda.synchronize()
        return {"x": x.check("mask_rows").cpu()}
    _judge("mask_rows", inp, _twice(run), str(case[:4]))


def test_zz_report_ratios():
    print()
    for k in sorted(RATIOS):
        print("    %-36s %.3f   %s" % (k, RATIOS[k], WHERE.get(k, "")))
