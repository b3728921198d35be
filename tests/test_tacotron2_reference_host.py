"""CPU-only checks of tests/_tacotron2_reference.py (the float64 statements and bars tests/test_gpu_tacotron2_reference.py holds the
Tacotron2 training kernels to).

1. For every case and both 16-bit dtypes, kernel_model (the kernels' arithmetic in float32, no fault) stays inside the bars on every
   element of every output: largest ratio <= 1, recorded per output (test_zz_report with -s prints the table; the figures are copied
   into the GPU test's docstring).  The staged references (weights from tanh_out, awc_next and contexts from the weights, d_prev /
   d_cum from d_pl, dq16 from dq) are formed from the MODEL's own intermediates, as the GPU test forms them from the GPU's.
   Largest ratios, fp16 / bf16 (with C_RCP = 3 u; outputs compared bit for bit are 0):
       lstm_fwd: act 1.000 / 1.000  c_out 0.654 / 0.596 (constant-dominated elements 0.388 / 0.382)  h 0.999 / 1.000
       lstm_bwd: dgates 1.000 / 1.000  dc_prev 0.869 / 0.892 (constant-dominated elements 0.344 / 0.329)
       attention_fwd: tanh_out 1.000 / 1.000  aw_out 0.029 / 0.029  ctx 0.997 / 0.999
       attention_bwd: d_pl 0.997 / 0.999  dq 0.047 / 0.025  dq16 0.011 / 0.110  dv_acc 0.122 / 0.123  d_memory 0.982 / 0.985
                      d_pm_acc 0.962 / 0.981  d_prev 0.023 / 0.018  d_cum 0.145 / 0.085
       location_bwd: d_prev 0.500 / 0.450  d_cum 0.752 / 0.752      mel_loss: loss 0.077 / 0.037  d_out, d_post 1.000
       sum_steps 0.999 / 1.000      tanh_fwd 0.923 / 0.992      mask_rows exact
   (the 16-bit figures at 1 are the half ulp of the store; the fp32 ones near 1 are single roundings against u |value|.)
2. Every fault of FAULTS pushes a named output of a named case above ratio 1 (an output compared bit for bit reports inf); the pair
   (output, case) is asserted, for both dtypes.  One fault has no place to show: loc_rows_past_ti_live.  The fused backward's operand
   rows Ti..Ti32 only feed rows Ti..Ti32 of dcol (a matrix product keeps rows apart), and the anti-diagonal fold reads rows
   0 <= t < Ti only, so whatever those rows hold, no output changes; the kernel's zeroing is defensive.  The test states that: the
   model with the fault returns the same bits, and no case or bar could make it otherwise.
3. The independent pieces of the statements agree with torch's own float64 autograd: the LSTM cell and the attention step (with the
   location convolution as conv1d).
"""
import pytest
import torch
import torch.nn.functional as TF

from tests import _tacotron2_reference as R

F64, F32, F16, BF16 = R.F64, R.F32, R.F16, R.BF16
DTYPES = [F16, BF16]
RATIOS = {}


def _run(kernel, inp, key, fault=None):
    got = R.kernel_model(kernel, inp, fault)
    res = R.check(kernel, inp, got)
    if fault is None:
        for out, (r, i) in res.items():
            k = "%s %s %s" % (kernel, out, R.name(inp["dtype"]))
            RATIOS[k] = max(RATIOS.get(k, 0.0), r)
            assert r <= 1.0, "%s, %s: |fp32 model - ref| / bar = %.3f at flat index %d" % (k, key, r, i)
    return res


def _lstm(cid):
    return next(c for c in R.LSTM_CASES if c[0] == cid)


# ------------------------------------------------------------------------------------------------ 1. the model stays inside
@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.LSTM_CASES, ids=lambda c: c[0])
def test_lstm_model_within_bars(case, dtype):
    """both template forms of both cell kernels (route asserted from the launcher's conditions in lstm_inputs)"""
    _run("lstm_fwd", R.lstm_inputs(case, dtype), case[0])
    _run("lstm_bwd", R.lstm_bwd_inputs(case, dtype), case[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("case", R.ATT_CASES, ids=lambda c: c[0])
def test_attention_model_within_bars(case, dtype):
    """attention forward and backward, without and with the fused location term"""
    inp = R.att_inputs(case, dtype)
    res = _run("attention_fwd", inp, case[0])
    assert set(res) == {"tanh_out", "aw_out", "awc_next", "ctx"}
    _run("attention_bwd", R.att_bwd_inputs(case, dtype), case[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
def test_attention_inputs_reach_the_edges(dtype):
    """the drawn energies do reach an exp underflow to exactly 0 inside the length, saturated tanh, and a pair a few ulps apart"""
    inp = R.att_inputs(R.att_case("odd_groups"), dtype)
    got = R.kernel_model("attention_fwd", inp)
    b, ti, a = inp["B"], inp["Ti"], inp["A"]
    th, aw = got["tanh_out"].float().view(b, ti, a), got["aw_out"]
    assert bool((th[0, 0].abs() == 1).all()) and bool((th[0, 1].abs() == 1).all())
    assert float(aw[0, 1]) == 0.0 and float(aw[0, 0]) > 0.99 and int(inp["lengths"][0]) > 1
    en = (th * inp["v"]).sum(2)
    assert abs(float(en[b - 1, 0] - en[b - 1, 2])) <= 64 * R.U * float((th[b - 1, 0] * inp["v"]).abs().sum())
    assert 0 < abs(float(en[b - 1, 0] - en[b - 1, 1])) < 2e-2 and int(inp["lengths"][b - 1]) > 2


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
def test_length_above_ti_is_clamped(dtype):
    case = R.att_case("len_above_ti")
    a = R.kernel_model("attention_fwd", R.att_inputs(case, dtype))
    b = R.kernel_model("attention_fwd", R.att_inputs(case, dtype, lengths=R.ATT_TWIN["len_above_ti"]))
    for k in ("tanh_out", "aw_out", "awc_next"):
        assert torch.equal(R.bits(a[k]), R.bits(b[k]))
    assert torch.equal(R.bits(a["ctx"][0]), R.bits(b["ctx"][0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
def test_small_kernel_models_within_bars(dtype):
    _run("tanh_fwd", R.tanh_inputs(None, dtype), "grid")
    for case in R.LOC_CASES:
        _run("location_bwd", R.loc_inputs(case, dtype), str(case))
    for case in R.MEL_CASES:
        for sc in R.MEL_SCALES:
            _run("mel_loss", R.mel_inputs(case, dtype, sc), "%s scale %s" % (case, sc))
    for n in R.SUM_STEPS_N:
        for r in R.SUM_STEPS_R:
            _run("sum_steps", R.sum_steps_inputs((n, r), dtype), "n=%d R=%d" % (n, r))
    for case in R.MASK_CASES:
        for dt in (dtype, F32):
            _run("mask_rows", R.mask_inputs(case, dt), str(case))


# ------------------------------------------------------------------------------------------------ 2. every fault is caught
def _att_f(cid):
    return lambda dt: R.att_inputs(R.att_case(cid), dt)


def _att_b(cid):
    return lambda dt: R.att_bwd_inputs(R.att_case(cid), dt)


CAUGHT = [   # fault, kernel, case, input builder, outputs that must leave the bar
    ("cum_without_w", "attention_fwd", "odd_groups", _att_f("odd_groups"), ["awc_next"]),
    ("mask_off_by_one", "attention_fwd", "odd_groups", _att_f("odd_groups"), ["aw_out"]),
    ("mask_off_by_one", "mask_rows", "4x5 lengths 0,5,9,2", lambda dt: R.mask_inputs(R.MASK_CASES[0], dt), ["x"]),
    ("inactive_lanes_counted", "attention_fwd", "odd_groups", _att_f("odd_groups"), ["aw_out"]),
    ("inactive_lanes_counted", "attention_bwd", "odd_groups", _att_b("odd_groups"), ["dq", "dv_acc", "d_pl"]),
    ("energy_from_unrounded_tanh", "attention_fwd", "default", _att_f("default"), ["aw_out"]),
    ("energy_from_unrounded_tanh", "attention_fwd", "odd_groups", _att_f("odd_groups"), ["aw_out"]),
    ("loc_pad_shift", "attention_fwd", "loc_ti32", _att_f("loc_ti32"), ["tanh_out"]),
    ("loc_pad_shift", "attention_fwd", "loc_ti_below_pad", _att_f("loc_ti_below_pad"), ["tanh_out"]),
    ("loc_pad_shift", "attention_bwd", "loc_ti32", _att_b("loc_ti32"), ["d_prev", "d_cum"]),
    ("loc_pad_shift", "attention_bwd", "loc_k5", _att_b("loc_k5"), ["d_prev", "d_cum"]),
    ("loc_pad_shift", "location_bwd", "3x23x31", lambda dt: R.loc_inputs(R.LOC_CASES[0], dt), ["d_prev", "d_cum"]),
    ("keep_bit_reversed", "lstm_fwd", "scalar_keepindex4", lambda dt: R.lstm_inputs(_lstm("scalar_keepindex4"), dt), ["h"]),
    ("keep_bit_reversed", "lstm_fwd", "vec_strided_h96", lambda dt: R.lstm_inputs(_lstm("vec_strided_h96"), dt), ["h"]),
    ("keep_bit_reversed", "lstm_bwd", "scalar_h20", lambda dt: R.lstm_bwd_inputs(_lstm("scalar_h20"), dt), ["dgates"]),
    ("keep_index_dropped", "lstm_fwd", "scalar_keepindex4", lambda dt: R.lstm_inputs(_lstm("scalar_keepindex4"), dt), ["h"]),
    ("keep_index_dropped", "lstm_bwd", "vec_strided_h96", lambda dt: R.lstm_bwd_inputs(_lstm("vec_strided_h96"), dt), ["dgates"]),
    ("live_ignored", "lstm_fwd", "scalar_unaligned", lambda dt: R.lstm_inputs(_lstm("scalar_unaligned"), dt), ["c_out", "h"]),
    ("live_ignored", "lstm_bwd", "vec_h8", lambda dt: R.lstm_bwd_inputs(_lstm("vec_h8"), dt), ["dgates", "dc_prev"]),
    ("dv_overwritten", "attention_bwd", "odd_groups", _att_b("odd_groups"), ["dv_acc"]),
    ("dcum_overwritten", "attention_bwd", "loc_ti32", _att_b("loc_ti32"), ["d_cum"]),
    ("dcum_overwritten", "location_bwd", "2x9x5", lambda dt: R.loc_inputs(R.LOC_CASES[1], dt), ["d_cum"]),
    ("second_trip_skipped", "lstm_fwd", "vec_second_trip", lambda dt: R.lstm_inputs(_lstm("vec_second_trip"), dt), ["act", "c_out", "h"]),
    ("second_trip_skipped", "lstm_bwd", "vec_second_trip", lambda dt: R.lstm_bwd_inputs(_lstm("vec_second_trip"), dt), ["dgates", "dc_prev"]),
    ("second_trip_skipped", "mel_loss", "3300x80", lambda dt: R.mel_inputs(R.MEL_CASES[2], dt, None), ["loss", "d_post", "d_out"]),
    ("second_trip_skipped", "location_bwd", "70x3800x3", lambda dt: R.loc_inputs(R.LOC_CASES[3], dt), ["d_prev", "d_cum"]),
    ("second_trip_skipped", "mask_rows", "3x1100x80", lambda dt: R.mask_inputs(R.MASK_CASES[3], dt), ["x"]),
    ("tail_steps_skipped", "sum_steps", "n=7 R=8", lambda dt: R.sum_steps_inputs((7, 8), dt), ["out"]),
    ("tail_steps_skipped", "sum_steps", "n=1 R=4104", lambda dt: R.sum_steps_inputs((1, 4104), dt), ["out"]),
]
SEEN = set()


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("entry", CAUGHT, ids=lambda e: "%s-%s-%s" % (e[0], e[1], e[2].replace(" ", "_")))
def test_fault_is_caught(entry, dtype):
    fault, kernel, cid, build, outputs = entry
    res = _run(kernel, build(dtype), cid, fault)
    for out in outputs:
        assert res[out][0] > 1.0, "the bar does not catch %s on %s of %s, case %s (largest ratio %.3f)" % (fault, out, kernel, cid, res[out][0])
    SEEN.add(fault)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
def test_fault_without_a_place_to_show(dtype):
    """loc_rows_past_ti_live (module docstring, 2.): same bits with and without"""
    inp = R.att_bwd_inputs(R.att_case("loc_ti32"), dtype)
    a, b = R.kernel_model("attention_bwd", inp), R.kernel_model("attention_bwd", inp, "loc_rows_past_ti_live")
    for k in a:
        if a[k] is not None:
            assert torch.equal(R.bits(a[k]), R.bits(b[k])), k


def test_every_fault_is_listed():
    assert {e[0] for e in CAUGHT} | {"loc_rows_past_ti_live"} == set(R.FAULTS)


# ------------------------------------------------------------------------------------------------ 3. the statements are the model's
def test_lstm_statement_is_the_cell():
    """a model output equal to float64 torch (sigmoid / tanh cell, autograd backward) has ratio ~ 0 against the statements"""
    case = _lstm("scalar_keepindex4")
    inp = R.lstm_bwd_inputs(case, F16)
    b, h = inp["B"], inp["H"]
    gx = inp["gates"].double().requires_grad_()
    cp = inp["c_prev"].double().requires_grad_()
    i, f, g, o = (torch.sigmoid(gx[:, :h]), torch.sigmoid(gx[:, h:2 * h]), torch.tanh(gx[:, 2 * h:3 * h]), torch.sigmoid(gx[:, 3 * h:]))
    c = f * cp + i * g
    km = R._keep_mask(inp).double()
    hh = o * torch.tanh(c) * km * inp["inv_keep"]
    live = (inp["live"] != 0).view(b, 1)
    got = {"act": torch.cat([i, f, g, o], 1).detach().to(F16), "c_out": torch.where(live, c.detach(), cp.detach()).float(),
           "h_dsts": [torch.where(live, hh.detach(), inp["h_prev"].double()).to(F16)]}
    got["out_dst"] = torch.where(live, got["h_dsts"][0], torch.zeros((), dtype=F16))
    res = R.check("lstm_fwd", inp, got)
    assert all(r <= 1.0 for r, _ in res.values()), res
    # backward: autograd through the SAVED (rounded) activations' formulas is what the statement restates
    a = inp["act"].double()
    gi, gf, gg, go = (a[:, q * h:(q + 1) * h] for q in range(4))
    dhv = sum(p.double() for p in inp["dh"])
    gk = dhv * km * inp["inv_keep"]
    tc = torch.tanh(gf * inp["c_prev"].double() + gi * gg)
    dc = inp["dc_next"].double() + gk * go * (1 - tc * tc)
    want = torch.cat([dc * gg * gi * (1 - gi), dc * inp["c_prev"].double() * gf * (1 - gf), dc * gi * (1 - gg * gg), gk * tc * go * (1 - go)], 1)
    want = torch.where(live, want, torch.zeros((), dtype=F64))
    gotb = {"dgates": want.to(F16), "dc_prev": torch.where(live, dc * gf, inp["dc_next"].double()).float(),
            "dh_prev": torch.where(live, torch.zeros(()), R._sum32(inp["dh"]))}
    res = R.check("lstm_bwd", inp, gotb)
    assert all(r <= 1.0 for r, _ in res.values()), res


@pytest.mark.parametrize("cid", ["loc_ti32", "loc_k5", "loc_ti_below_pad"])
def test_location_term_is_the_convolution(cid):
    """_loc_cols x wloc = conv1d(2 -> A, k = KL, padding = KL / 2) of the (previous, cumulative) weights; _loc_fold is its transpose"""
    inp = R.att_inputs(R.att_case(cid), BF16)
    b, ti, a, kl = inp["B"], inp["Ti"], inp["A"], inp["KL"]
    w = inp["wloc"].double()
    loc = R._loc_cols(inp, F64) @ w.t()
    x = inp["awc_prev"].double().view(b, ti, 8)[..., :2].permute(0, 2, 1).contiguous().requires_grad_()      # [B, 2, Ti]
    wc = w[:, :2 * kl].view(a, kl, 2).permute(0, 2, 1).contiguous()                                            # [A, 2, KL]
    y = TF.conv1d(x, wc, padding=kl // 2)                                                                      # [B, A, Ti]
    assert torch.allclose(loc, y.detach().permute(0, 2, 1), rtol=1e-12, atol=1e-14)
    dy = torch.randn(b, ti, a, generator=R.gen(1), dtype=F64)
    y.backward(dy.permute(0, 2, 1))
    acc, _ = R._loc_fold(dy @ w, ti, kl)
    assert torch.allclose(acc, x.grad.permute(0, 2, 1), rtol=1e-12, atol=1e-14)


def test_attention_statement_is_the_step():
    """the float64 attention step under autograd (energies from the saved 16-bit tanh, as the kernel defines its backward)"""
    case = R.att_case("odd_groups")
    inp = R.att_bwd_inputs(case, F16)
    b, ti, a, e = inp["B"], inp["Ti"], inp["A"], inp["E"]
    th = inp["tanh_out"].double().view(b, ti, a)
    pre = torch.atanh(th.clamp(-1 + 1e-12, 1 - 1e-12)).requires_grad_()
    v = inp["v"].double().requires_grad_()
    mem = inp["memory"].double().view(b, ti, e).requires_grad_()
    valid = torch.arange(ti).view(1, ti) < inp["lengths"].clamp(max=ti).view(b, 1)
    en = (torch.tanh(pre) * v).sum(2).masked_fill(~valid, -float("inf"))
    w = torch.softmax(en, 1)
    ctx = (w.view(b, ti, 1) * mem).sum(1)
    dctx = sum(p.double() for p in inp["dc"])
    daw = sum(p.double() for p in inp["daw"])
    aw = inp["aw"].double()
    # the kernel's backward takes the SAVED fp32 weights; autograd at the float64 weights differs by their fp32 error only
    ((ctx * dctx).sum() + (w * daw).sum()).backward()
    got = R.kernel_model("attention_bwd", inp)
    sat = th.abs() == 1
    d_pl = got["d_pl"].double().view(b, ti, a)
    assert torch.allclose(d_pl[~sat], pre.grad[~sat], rtol=4e-3, atol=1e-4)
    assert torch.allclose(got["dv_acc"].double() - inp["dv_acc"].double(), _dv(inp, pre, v, mem, valid, dctx, daw), rtol=2e-3, atol=2e-3)
    assert torch.allclose(got["d_memory"].double() - inp["d_memory"].double(), mem.grad.view(b * ti, e), rtol=1e-4, atol=1e-6)


def _dv(inp, pre, v, mem, valid, dctx, daw):
    """per-sample gradient of v (the kernel keeps one row of partials per sample)"""
    b, ti = valid.shape
    rows = []
    for s in range(b):
        vv = v.detach().clone().requires_grad_()
        en = (torch.tanh(pre[s].detach()) * vv).sum(1).masked_fill(~valid[s], -float("inf"))
        w = torch.softmax(en, 0)
        (((w.view(ti, 1) * mem[s].detach()).sum(0) * dctx[s]).sum() + (w * daw[s]).sum()).backward()
        rows.append(vv.grad)
    return torch.stack(rows)


def test_zz_report():
    print()
    for k in sorted(RATIOS):
        print("    %-36s %.3f" % (k, RATIOS[k]))
