"""CPU-only checks of tests/_waveglow_reference.py (the float64 statements and bars tests/test_gpu_waveglow_reference.py holds the
WaveGlow kernels to).

1. For every case and both 16-bit dtypes, kernel_model (the kernels' arithmetic in float32, no fault) stays inside the bars on every
   element of every output: largest ratio <= 1, recorded per output (test_zz_report with -s prints the table; the figures are copied
   into the GPU test's docstring).  Staged references (a0 from the returned y / out) are formed from the MODEL's own fp32 output, as
   the GPU test forms them from the GPU's.  Largest ratios (fp16 = bf16 unless two figures are given; bit-compared outputs are 0):
       taps_bwd 1.000  gate_fwd 1.000  gate_bwd 1.000  invconv_fwd y 0.408  invconv_bwd dx 0.504, dW 0.117
       logdet_inv logdet 0.762, winv_t 0.955 (batched 0.529, 0.936)  coupling_fwd z 0.985, logs_partial 0.106  coupling_bwd dy 0.647,
       d_o 1.000  loss 0.051  dz_init 0.749  weight_norm_fwd 0.999 / 1.000  weight_norm_bwd dv 0.347, dg 0.171  flow_inv out 0.430
   (the 16-bit figures at 1 are the half ulp of the store.)
2. Every fault of FAULTS pushes a named output of a named case above ratio 1 (an output compared bit for bit reports inf); the
   pair (output, case) is asserted, for both dtypes.  second_trip_skipped has no place in the weight-norm kernels (one wavefront
   per row, no grid-stride loop) nor in logdet_inv (one lane per matrix): kernel_model returns the same bits there with and without
   it, which test_fault_without_a_place_to_show states; every other fault shows in at least one output.
3. The statements agree with torch's own float64 results where an independent formulation exists: taps + a matrix product against
   conv1d, its transpose against autograd; the upsampling weight + taps(dilation -1) against conv_transpose1d; weight norm against
   torch._weight_norm and autograd; logdet_inv against det and W W^-1 = I; the gate, the coupling and the invertible convolution
   (with its log-determinant term) against autograd.
"""
import functools

import pytest
import torch
import torch.nn.functional as TF

from tests import _waveglow_reference as R

F64, F32, F16, BF16 = R.F64, R.F32, R.F16, R.BF16
DTYPES = [F16, BF16]
RATIOS = {}

BUILDERS = {
    "taps": (R.taps_inputs, R.TAPS_CASES), "taps_bwd": (R.taps_bwd_inputs, R.TAPS_BWD_CASES),
    "gate_fwd": (R.gate_inputs, R.GATE_CASES), "gate_bwd": (R.gate_inputs, R.GATE_CASES),
    "invconv_fwd": (R.invconv_inputs, R.INVCONV_CASES), "invconv_bwd": (R.invconv_bwd_inputs, R.INVCONV_BWD_CASES),
    "logdet_inv": (R.logdet_inputs, R.LOGDET_CASES), "logdet_inv_batched": (R.logdet_batched_inputs, list(R.LOGDET_TABLES)),
    "coupling_fwd": (R.coupling_inputs, R.COUPLING_CASES), "coupling_bwd": (R.coupling_inputs, R.COUPLING_CASES),
    "loss": (R.loss_inputs, R.LOSS_CASES), "dz_init": (R.dz_inputs, R.DZ_CASES),
    "weight_norm_fwd": (R.wn_inputs, R.WN_CASES), "weight_norm_bwd": (R.wn_inputs, R.WN_CASES),
    "weight_norm_fwd_batched": (R.wn_table_inputs, list(R.WN_TABLES)), "weight_norm_bwd_batched": (R.wn_table_inputs, list(R.WN_TABLES)),
    "upsample_weight": (R.upsample_inputs, R.UPSAMPLE_CASES), "upsample_weight_bwd": (R.upsample_inputs, R.UPSAMPLE_CASES),
    "flow_inv": (R.flow_inputs, R.FLOW_CASES), "flow_inv_first": (R.flow_first_inputs, R.FLOW_FIRST_CASES),
}


def _cid(case):
    if isinstance(case, str):
        return case
    if len(case) == 2 and isinstance(case[0], str):
        return "%s%d" % case
    return case[0] if isinstance(case[0], str) else "x".join(map(str, case))


def _find(kernel, cid):
    return next(c for c in BUILDERS[kernel][1] if _cid(c) == cid)


@functools.lru_cache(maxsize=4)
def _inputs(kernel, cid, dtype):
    return BUILDERS[kernel][0](_find(kernel, cid), dtype)


def _run(kernel, inp, key, fault=None):
    got = R.kernel_model(kernel, inp, fault)
    res = R.check(kernel, inp, got)
    if fault is None:
        for out, (r, i) in res.items():
            k = "%s %s %s" % (kernel, out, R.name(inp["dtype"]) if inp["dtype"] is not None else "fp32")
            RATIOS[k] = max(RATIOS.get(k, 0.0), r)
            assert r <= 1.0, "%s, %s: |fp32 model - ref| / bar = %.3f at flat index %d" % (k, key, r, i)
    return res


# ------------------------------------------------------------------------------------------------ 1. the model stays inside
@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("kernel", sorted(BUILDERS))
def test_model_within_bars(kernel, dtype):
    build, cases = BUILDERS[kernel]
    for case in cases:
        inp = build(case, dtype)
        _run(kernel, inp, _cid(case))
        if kernel.startswith("weight_norm") and not kernel.endswith("batched"):
            _run(kernel, R.wn_inputs(case, dtype, gain=False), _cid(case) + " plain")


def test_case_tables_reach_the_paths():
    """the second-trip cases are the sizes the issue names and do exceed one trip; every c and every small M appears"""
    assert R.taps_items(R.TAPS_CASES[-1]) == 1050240 > R.ONE_TRIP
    c = R.TAPS_BWD_CASES[-1]
    assert c[1] * c[2] * c[3] // 8 == 1049600 > R.ONE_TRIP
    assert R.GATE_CASES[-1][1] * R.GATE_CASES[-1][2] // 8 == 1049600
    assert R.ROW_BIG == 1048833 > R.ONE_TRIP and 2 * R.LOSS_BIG > R.ONE_TRIP and R.LOSS_BIG == 524417
    assert R.INVCONV_BWD_CASES[-1][1] == 33025 > R.INVCONV_BWD_CAP * R.WG_BLOCK
    for table in (R.INVCONV_CASES, R.INVCONV_BWD_CASES, R.COUPLING_CASES):
        assert {c[1] for c in table} >= {1, 255, 257, 1000} and {c[2] for c in table} == {2, 4, 6, 8}
    assert {c[2] for c in R.FLOW_CASES} == {2, 4, 6, 8} and {c[3] for c in R.FLOW_CASES} == {0, 2} and {c[4] for c in R.FLOW_CASES} == {0, 2, 6}
    assert {c[2] * c[3] for c in R.WN_CASES} >= {3, 63, 64, 65, 1920}
    assert {(c[2], c[3]) for c in R.LOSS_CASES} >= {(0, 12), (12, 0), (12 * 4096, 12), (1, 12)}


def test_logdet_matrices_are_what_they_claim():
    for kind, c in R.LOGDET_CASES:
        W = R.logdet_matrix(kind, c).double()
        assert float(torch.linalg.cond(W)) <= 1e3, (kind, c)
        if kind == "pivot" and c > 1:
            assert float(W[0, 0]) == 0.0
        if kind == "negdet":
            assert float(torch.det(W)) < 0
        else:
            assert float(torch.det(W)) > 0


def test_build_flags_keep_ieee_division_and_sqrt():
    assert R.ieee_div_sqrt() and R.C_SQRT == R.C_DIV == 1.0
    assert not R.ieee_div_sqrt(["-O3", "-ffast-math"]) and not R.ieee_div_sqrt(["-fno-hip-fp32-correctly-rounded-divide-sqrt"])


# ------------------------------------------------------------------------------------------------ 2. every fault is caught
ST = "second_trip_skipped"
CAUGHT = [   # fault, kernel, case, outputs that must leave the bar
    ("taps_ignore_boundary", "taps", "k3_d1", ["col"]), ("taps_ignore_boundary", "taps_bwd", "noadd", ["dx"]),
    ("left_ignored", "taps", "k3_d1", ["col"]), ("left_ignored", "taps_bwd", "separate", ["dx"]),
    ("gate_halves_swapped", "gate_fwd", "m255", ["acts"]), ("gate_halves_swapped", "gate_bwd", "m255", ["ds"]),
    ("one_minus_sg_dropped", "gate_bwd", "m255", ["ds"]), ("one_minus_sg_dropped", "gate_bwd", "m1", ["ds"]),
    ("w_transposed", "invconv_fwd", "m255_c4", ["y"]), ("w_transposed", "invconv_bwd", "m255_c4", ["dx"]),
    ("embed_off_by_one", "invconv_fwd", "m255_c4", ["y", "y pass-through"]), ("embed_off_by_one", "invconv_bwd", "m255_c4", ["dx", "dx pass-through"]),
    ("a0_second_half", "invconv_fwd", "m255_c4", ["a0"]), ("a0_second_half", "invconv_fwd", "m1_c2", ["a0"]),
    ("da0_dropped", "invconv_bwd", "m255_c4", ["dx", "dW"]), ("da0_dropped", "invconv_bwd", "exact_m1000_c6", ["dx", "dW"]),
    ("logdet_term_dropped", "invconv_bwd", "m255_c4", ["dW"]), ("logdet_scale_dropped", "invconv_bwd", "m255_c4", ["dW"]),
    ("logs_from_b", "coupling_fwd", "m255_c4", ["z", "logs_partial", "logs sum"]), ("logs_from_b", "coupling_bwd", "m255_c4", ["dy", "d_o log_s"]),
    ("lsg_sign", "coupling_bwd", "m255_c4", ["d_o log_s"]), ("lsg_sign", "coupling_bwd", "m1000_c8", ["d_o log_s"]),
    ("rows_dropped", "loss", "m255", ["loss"]), ("rows_dropped", "loss", "second_trip", ["loss"]),
    ("norm_over_padded_row", "weight_norm_fwd", "n3", ["w16"]), ("norm_over_padded_row", "weight_norm_bwd", "n3", ["dv", "dg"]),
    ("layout_swapped", "weight_norm_fwd", "n63", ["w16"]), ("layout_swapped", "weight_norm_bwd", "n63", ["dv", "dg"]),
    ("table_row_off_by_one", "weight_norm_fwd_batched", "five", ["w16, first rows"]),
    ("table_row_off_by_one", "weight_norm_bwd_batched", "five", ["dv, first rows"]),
    ("table_row_off_by_one", "weight_norm_fwd_batched", "co1", ["w16, first rows", "w16, last rows"]),
    ("phase_tap_swapped", "upsample_weight", "8x16x4", ["b16"]), ("phase_tap_swapped", "upsample_weight_bwd", "8x16x4", ["dw"]),
    ("wrong_noise_column", "flow_inv", "m257_c4_e2_z2", ["out early"]), ("wrong_noise_column", "flow_inv_first", "m255_c4", ["out"]),
    ("winv_not_transposed", "logdet_inv", "well4", ["winv_t"]), ("winv_not_transposed", "flow_inv", "m1000_c4_same", ["out"]),
    (ST, "taps", "second_trip", ["col"]), (ST, "taps_bwd", "second_trip", ["dx"]), (ST, "gate_fwd", "second_trip", ["acts"]),
    (ST, "gate_bwd", "second_trip", ["ds"]), (ST, "invconv_fwd", "second_trip_c4", ["y", "a0"]), (ST, "invconv_bwd", "second_trip_c8", ["dx", "dW"]),
    (ST, "coupling_fwd", "second_trip_c8", ["z", "logs_partial", "logs sum"]), (ST, "coupling_bwd", "second_trip_c8", ["dy", "d_o log_s"]),
    (ST, "loss", "second_trip", ["loss"]), (ST, "loss", "exact_second_trip", ["loss"]), (ST, "dz_init", "second_trip", ["dz"]),
    (ST, "upsample_weight", "80x1024x256", ["b16"]), (ST, "upsample_weight_bwd", "80x1024x256", ["dw"]),
    (ST, "flow_inv", "second_trip_c6_e2", ["out", "a0"]), (ST, "flow_inv_first", "second_trip_c4", ["out"]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=R.name)
@pytest.mark.parametrize("entry", CAUGHT, ids=lambda e: "%s-%s-%s" % e[:3])
def test_fault_is_caught(entry, dtype):
    fault, kernel, cid, outputs = entry
    res = _run(kernel, _inputs(kernel, cid, dtype), cid, fault)
    for out in outputs:
        assert res[out][0] > 1.0, "the bar does not catch %s on %s of %s, case %s (largest ratio %.3f)" % (fault, out, kernel, cid, res[out][0])


@pytest.mark.parametrize("kernel,cid", [("weight_norm_fwd", "n1920"), ("weight_norm_bwd", "t_1024x512x3"), ("logdet_inv", "well8")])
def test_fault_without_a_place_to_show(kernel, cid):
    """second_trip_skipped in a kernel without a grid-stride loop (module docstring, 2.): same bits with and without"""
    inp = _inputs(kernel, cid, F16)
    a, b = R.kernel_model(kernel, inp), R.kernel_model(kernel, inp, ST)
    for k in a:
        if a[k] is not None:
            assert torch.equal(R.bits(a[k]), R.bits(b[k])), k


def test_every_fault_is_listed():
    assert {e[0] for e in CAUGHT} == set(R.FAULTS)


# ------------------------------------------------------------------------------------------------ 3. the statements are torch's
@pytest.mark.parametrize("cid", ["k3_d1", "k3_d4_T5", "slice_2C"])
def test_taps_and_a_product_are_conv1d(cid):
    """taps(x) @ w = conv1d(dilation, padding = left dilation) channels-last; taps_bwd is its transpose (autograd)"""
    case = _find("taps", cid)
    _, b, t, c, nt, dil, left, _ = case
    inp = R.taps_inputs(case, BF16)
    x = torch.nan_to_num(inp["x"].double(), nan=0.5, posinf=2.0, neginf=-2.0)
    inp["x"] = x.to(BF16)
    x = inp["x"].double()
    col = R.taps_model(inp)["col"].double()
    w = torch.randn(5, c, nt, generator=R.gen(3), dtype=F64)                      # conv1d weight [out, in, k]
    xc = x.view(b, t, c).permute(0, 2, 1).contiguous().requires_grad_()
    y = TF.conv1d(xc, w, dilation=dil, padding=left * dil)[:, :, :t]
    assert torch.allclose(col @ w.permute(2, 1, 0).reshape(nt * c, 5), y.permute(0, 2, 1).reshape(b * t, 5), rtol=1e-12, atol=1e-12)
    dcol = torch.randn(b * t, nt * c, generator=R.gen(4)).to(BF16)
    gx, = torch.autograd.grad((TF.conv1d(xc, torch.eye(nt * c, dtype=F64).view(nt * c, nt, c).permute(0, 2, 1).contiguous(), dilation=dil, padding=left * dil)[:, :, :t]
                               * dcol.double().view(b, t, nt * c).permute(0, 2, 1)).sum(), xc)
    bcase = ("x", b, t, c, nt, dil, left, None, c, 0)
    res = R.taps_bwd_check({"case": bcase, "dtype": BF16, "dcol": dcol, "addend": None}, {"dx": gx.permute(0, 2, 1).reshape(b * t, c).to(BF16)})
    assert res["dx"][0] <= 1.0, res


def test_upsampling_weight_and_taps_are_conv_transpose1d():
    cm, ks, st = 8, 16, 4
    inp = R.upsample_inputs((cm, ks, st), BF16)
    inp["w"] = torch.randn(cm, cm, ks, generator=R.gen(1)) * 0.1
    got = R.upsample_model(inp)
    b, fq, nt = 2, 7, ks // st
    mel = torch.randn(b, cm, fq, generator=R.gen(2)).to(BF16)
    rows = mel.permute(0, 2, 1).reshape(b * fq, cm).contiguous()
    col = R.taps_model({"case": ("up", b, fq, cm, nt, -1, 0, cm), "dtype": BF16, "x": rows})["col"]
    up = col.double() @ got["b16"].double().t() + got["bias_rep"].double()
    ref = TF.conv_transpose1d(mel.double(), inp["w"].to(BF16).double(), inp["bias"].double(), stride=st)[:, :, :fq * st]
    assert torch.allclose(up.view(b, fq * st, cm), ref.permute(0, 2, 1), rtol=1e-12, atol=1e-12)
    # the backward permutation is the forward's inverse
    back = R.upsample_bwd_model(dict(inp, db=got["b16"].float()))["dw"]
    assert torch.equal(back, inp["w"].to(BF16).float())


@pytest.mark.parametrize("cid", ["n63", "n65", "t_16x80x8"])
def test_weight_norm_statement_is_torch_weight_norm(cid):
    inp = R.wn_inputs(R.wn_case(cid), F16)
    _, co, ci, kt, cip = inp["case"]
    v, g = inp["v"].double().requires_grad_(), inp["g"].double().view(co, 1, 1).requires_grad_()
    w = torch._weight_norm(v, g, 0)
    got = {"w16": R._wn_layout(w.detach(), inp["case"]).to(F16)}
    assert R.wn_fwd_check(inp, got)["w16"][0] <= 1.0
    (w * R._wn_unlayout(inp["dw"], inp["case"]).double()).sum().backward()
    res = R.wn_bwd_check(inp, {"dv": v.grad.float(), "dg": g.grad.float().view(-1)})
    assert all(r <= 1.0 for r, _ in res.values()), res


def test_logdet_statement_is_det_and_inverse():
    for kind, c in R.LOGDET_CASES:
        inp = R.logdet_inputs((kind, c))
        W = inp["W"].double()
        out = R.logdet_model(inp)
        assert torch.allclose(out["logdet"].double(), torch.log(torch.det(W).abs()).view(1), rtol=1e-6, atol=1e-7)
        assert float(out["sign"]) == (1.0 if float(torch.det(W)) > 0 else -1.0)
        assert torch.allclose(W @ out["winv_t"].double().t(), torch.eye(c, dtype=F64), atol=1e-4)


def test_gate_statement_is_autograd():
    inp = R.gate_inputs(R.GATE_CASES[2], BF16)
    nc = inp["case"][2]
    s = inp["s"].double().clamp(-30, 30).requires_grad_()
    inp["s"] = s.detach().to(BF16)
    s = inp["s"].double().requires_grad_()
    out = torch.tanh(s[:, :nc]) * torch.sigmoid(s[:, nc:])
    assert R.gate_fwd_check(inp, {"acts": out.detach().to(BF16)})["acts"][0] <= 1.0
    (out * inp["dacts"].double()).sum().backward()
    assert R.gate_bwd_check(inp, {"ds": s.grad.to(BF16)})["ds"][0] <= 1.0


def test_invconv_and_coupling_statements_are_autograd():
    inp = R.invconv_bwd_inputs(R.INVCONV_BWD_CASES[1], F16)           # m255_c4, da0 and scale given
    c, m = inp["c"], inp["dy"].shape[0]
    off, nh = 8 - c, c // 2
    x, W = inp["x"].double().requires_grad_(), inp["W"].double().requires_grad_()
    y = torch.cat([x[:, :off], x[:, off:] @ W.t()], 1)
    fw = R.invconv_fwd_check({"case": ("m255_c4", m, c), "dtype": F16, "c": c, "x": inp["x"], "W": inp["W"]},
                             {"y": y.detach().float(), "a0": R._pad16(y.detach().float()[:, off:off + nh], F16)})
    assert all(r <= 1.0 for r, _ in fw.values()), fw
    g = inp["dy"].double().clone()
    g[:, off:off + nh] += inp["da0"].double()[:, :nh]
    ((y * g).sum() - float(inp["scale"]) * R.f32(inp["coef"]) * torch.linalg.slogdet(W)[1]).backward()
    res = R.invconv_bwd_check(inp, {"dx": torch.cat([inp["dy"][:, :off], x.grad[:, off:].float()], 1), "dW": W.grad.float()})
    assert all(r <= 1.0 for r, _ in res.values()), res
    inp = R.coupling_inputs(R.COUPLING_CASES[1], F16)                  # m255_c4, scale given
    c, m = inp["c"], inp["y"].shape[0]
    off, nh = 8 - c, c // 2
    y, o = inp["y"].double().requires_grad_(), inp["o"].double().requires_grad_()
    z1 = torch.exp(o[:, nh:c]) * y[:, off + nh:] + o[:, :nh]
    lsg = float(inp["scale"]) * R.f32(inp["logs_coef"])
    ((z1 * inp["dz"].double()[:, off + nh:]).sum() - lsg * o[:, nh:c].sum()).backward()
    d_o = torch.zeros(m, 8, dtype=F16)
    d_o[:, :c] = o.grad[:, :c].to(F16)
    d_o[:, :nh] = inp["dz"][:, off + nh:].to(F16)
    res = R.coupling_bwd_check(inp, {"dy": torch.cat([inp["dz"][:, :off + nh], y.grad[:, off + nh:].float()], 1), "d_o": d_o})
    assert all(r <= 1.0 for r, _ in res.values()), res


def test_flow_inv_undoes_the_forward_flow():
    """flow_inv(coupling_fwd(invconv_fwd(x))) = x in float64 (the statement of the reverse flow is the inverse of the training step's)"""
    c, m = 6, 50
    off, nh = 8 - c, c // 2
    g = R.gen(11)
    x, o = torch.randn(m, 8, generator=g, dtype=F64), torch.randn(m, 8, generator=g, dtype=F64) * 0.5
    W = R._mix_matrix(c, g).double()
    y = torch.cat([x[:, :off], x[:, off:] @ W.t()], 1)
    z = y.clone()
    z[:, off + nh:] = torch.exp(o[:, nh:c]) * y[:, off + nh:] + o[:, :nh]
    inp = {"case": ("inv", m, c, 0, 0, 0, False), "dtype": F16, "c": c, "state": z.float(), "o": o.float(), "noise": None, "sigma": 1.0,
           "winv_t": torch.linalg.inv(W).t().contiguous().float()}
    res = R.flow_check(inp, {"out": x.float(), "a0": None})
    assert res["out"][0] <= 4.0, res          # x, z and o were rounded to fp32 on the way: a few u more than the bar of exact inputs


def test_zz_report():
    print()
    for k in sorted(RATIOS):
        print("    %-50s %.3f" % (k, RATIOS[k]))
