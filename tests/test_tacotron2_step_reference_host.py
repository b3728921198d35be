"""CPU-only checks of tests/_tacotron2_step_reference.py (the float64 statements and bars tests/test_gpu_tacotron2_step_reference.py
holds dle_t2_lstm_gemm_fwd, dle_t2_prenet_infer and dle_t2_frame_infer to).

1. For every case, both tiers and both 16-bit dtypes, kernel_model (the launch's arithmetic in float32, no fault) stays inside the
   bars on every element of every output: largest ratio <= 1, recorded per output (test_zz_report with -s prints the table; the
   figures are copied into the GPU test's docstring).  The builders assert the tier-A preconditions (exact sums, the unsaturated
   share, no undecided gate logit) while they run.  For tier B of lstm_gemm the staged pre16 is the model's own.
2. Every fault of FAULTS pushes a named output of a named case above ratio 1 (an output compared bit for bit reports inf); the pair
   (output, case) is asserted, for both dtypes.
3. The float64 statements agree with torch's own float64 LSTMCell and linear + relu.
"""
import pytest
import torch
import torch.nn.functional as TF

from tests import _tacotron2_step_reference as T

F64, F32, F16, BF16 = T.F64, T.F32, T.F16, T.BF16
DTYPES = [F16, BF16]
RATIOS = {}


def _run(kernel, inp, key, fault=None):
    got = T.kernel_model(kernel, inp, fault)
    res = T.check(kernel, inp, got)
    if fault is None:
        for out, (r, i) in res.items():
            k = "%s %s %s %s" % (kernel, inp["tier"], out, T.name(inp["dtype"]))
            RATIOS[k] = max(RATIOS.get(k, 0.0), r)
            assert r <= 1.0, "%s, %s: |fp32 model - ref| / bar = %.3f at flat index %d" % (k, key, r, i)
    return res


# ------------------------------------------------------------------------------------------------ 1. the model stays inside
@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("case", T.LG_CASES, ids=lambda c: c[0])
def test_lstm_gemm_model_within_bars(case, tier, dtype):
    inp = T.lg_inputs(case, dtype, tier)
    assert T.lg_stages(case[1], case[2]) == (3 if case[0].startswith("nst3") else 4)
    for kidx in case[7]:
        res = _run("lstm_gemm_fwd", T.lg_at(inp, kidx), "%s keep_index %d" % (case[0], kidx))
        assert ("pre16" in res) == (tier == "B")


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("case", T.PRE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_prenet_model_within_bars(case, tier, dtype):
    for t, go in T.PRE_STEPS:
        res = _run("prenet_infer", T.pre_inputs(case, dtype, tier, t, go), "%s t %d" % (case, t))
        assert set(res) == {"dst", "mask0", "mask1"}


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("tier", T.TIERS)
@pytest.mark.parametrize("p", T.FR_P, ids=lambda p: "unfused" if p is None else "P%d" % p)
@pytest.mark.parametrize("case", T.FR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_frame_model_within_bars(case, p, tier, dtype):
    for limits in T.FR_LIMITS:
        inp = T.fr_inputs(case, dtype, tier, p, limits)
        res = _run("frame_infer", inp, "%s P %s limits %s" % (case, p, limits))
        assert ("pre_dst" in res) == (p is not None)


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("fused", [False, True])
def test_frame_scripted_threshold(fused, dtype):
    """thr = 0.3, logits one 16-bit step either side: the three samples stop at steps 3, 1 and 4, all finished after step 4"""
    inp = T.fr_scripted(dtype, 0.3, fused)
    _run("frame_infer", inp, "scripted")
    book = T.fr_book(inp, (T.widen(inp["hc"]) @ T.widen(inp["w"]).t())[..., inp["NM"]])
    assert book[-1][3].tolist() == [3, 1, 4] and book[-1][4].tolist() == [6, 5, 5, 1]


def test_frame_inputs_reach_the_bookkeeping():
    """the drawn logits do stop samples at different steps inside the limits, and leave one unfinished at the limit, somewhere"""
    seen_stop, seen_alive = False, False
    for case in T.FR_CASES:
        for tier in T.TIERS:
            inp = T.fr_inputs(case, F16, tier, None, (4, 6))
            book = T.fr_book(inp, T._fr_ref(inp)[0][..., inp["NM"]])
            nf = book[3][2]
            seen_stop |= int(nf.sum()) < inp["B"]
            seen_alive |= int(nf.sum()) > 0
    assert seen_stop and seen_alive


def test_fused_shapes_fit_the_lds_check():
    assert T.fr_lds(8, 80, 1536, 256) <= 64 * 1024 and T.fr_lds(8, 80, 1536, 1032) <= 64 * 1024 < T.fr_lds(8, 8, 4104, None)


# ------------------------------------------------------------------------------------------------ 2. every fault is caught
def _lg(cid, tier, kidx=None):
    def build(dt):
        inp = T.lg_inputs(T.lg_case(cid), dt, tier)
        return inp if kidx is None else T.lg_at(inp, kidx)
    return build


def _pre(i, tier, t):
    return lambda dt: T.pre_inputs(T.PRE_CASES[i], dt, tier, t)


def _fr(i, tier, p, limits):
    return lambda dt: T.fr_inputs(T.FR_CASES[i], dt, tier, p, limits)


CAUGHT = [   # fault, kernel, case, input builder, outputs that must leave the bar
    ("tile_map_transposed", "lstm_gemm_fwd", "b8_second_chunk8 A", _lg("b8_second_chunk8", "A"), ["act"]),
    ("tile_map_transposed", "lstm_gemm_fwd", "infer_attention A", _lg("infer_attention", "A"), ["act"]),
    ("tile_map_transposed", "lstm_gemm_fwd", "b3_h96 B", _lg("b3_h96", "B"), ["act"]),
    ("last_k_chunk_dropped", "lstm_gemm_fwd", "b8_second_chunk8 A", _lg("b8_second_chunk8", "A"), ["act"]),
    ("last_k_chunk_dropped", "lstm_gemm_fwd", "one_tile_k8 A", _lg("one_tile_k8", "A"), ["act"]),
    ("last_k_chunk_dropped", "lstm_gemm_fwd", "nst3_short A", _lg("nst3_short", "A"), ["act"]),
    ("clamped_rows_written", "lstm_gemm_fwd", "one_tile_k8 A", _lg("one_tile_k8", "A"), ["outside"]),
    ("clamped_rows_written", "lstm_gemm_fwd", "b129_wrap B", _lg("b129_wrap", "B"), ["outside"]),
    ("keep_index_dropped", "lstm_gemm_fwd", "b63 A keep_index 3", _lg("b63", "A", 3), ["h"]),
    ("keep_index_dropped", "lstm_gemm_fwd", "train B keep_index 40", _lg("train", "B", 40), ["h"]),
    ("bias_from_gate0", "lstm_gemm_fwd", "b64 A", _lg("b64", "A"), ["act"]),
    ("bias_from_gate0", "lstm_gemm_fwd", "infer_decoder B", _lg("infer_decoder", "B"), ["act"]),
    ("masks_swapped", "prenet_infer", "3x80x32 A t 1", _pre(1, "A", 1), ["dst", "mask0", "mask1"]),
    ("masks_swapped", "prenet_infer", "8x80x256 B t 6", _pre(2, "B", 6), ["dst", "mask0", "mask1"]),
    ("offset_truncated", "prenet_infer", "1x8x8 A t 2^31", _pre(0, "A", 2 ** 31), ["mask0", "mask1"]),
    ("offset_truncated", "prenet_infer", "8x80x256 B t 2^31", _pre(2, "B", 2 ** 31), ["dst", "mask0", "mask1"]),
    ("second_k_trip_skipped", "prenet_infer", "2x80x520 A t 1", _pre(3, "A", 1), ["dst"]),
    ("second_k_trip_skipped", "prenet_infer", "8x16x1032 B t 1", _pre(4, "B", 1), ["dst"]),
    ("hidden_fp32", "prenet_infer", "8x80x256 A t 1", _pre(2, "A", 1), ["dst"]),
    ("second_k_trip_skipped", "frame_infer", "2x80x520 A", _fr(2, "A", None, (4, 6)), ["mel_out", "frame_next"]),
    ("second_k_trip_skipped", "frame_infer", "8x80x1536 B", _fr(3, "B", None, (6, 4)), ["mel_out", "gate_out", "frame_next"]),
    ("second_k_trip_skipped", "frame_infer", "8x80x1536 A fused P 1032", _fr(3, "A", 1032, (4, 6)), ["pre_dst"]),
    ("step_at_out_steps_stored", "frame_infer", "8x80x1536 A out 4 max 6", _fr(3, "A", None, (4, 6)), ["state", "outside"]),
    ("lengths_before_not_finished", "frame_infer", "8x80x1536 B", _fr(3, "B", None, (4, 6)), ["mel_lengths"]),
    ("lengths_before_not_finished", "frame_infer", "3x80x160 A", _fr(1, "A", 48, (6, 4)), ["mel_lengths"]),
    ("wrong_parity_advanced", "frame_infer", "1x8x8 A", _fr(0, "A", None, (4, 6)), ["state"]),
    ("wrong_parity_advanced", "frame_infer", "3x80x160 B fused", _fr(1, "B", 48, (6, 4)), ["state"]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=T.name)
@pytest.mark.parametrize("entry", CAUGHT, ids=lambda e: "%s-%s-%s" % (e[0], e[1], e[2].replace(" ", "_")))
def test_fault_is_caught(entry, dtype):
    fault, kernel, cid, build, outputs = entry
    res = _run(kernel, build(dtype), cid, fault)
    for out in outputs:
        assert res[out][0] > 1.0, "the bar does not catch %s on %s of %s, case %s (largest ratio %.3f)" % (fault, out, kernel, cid, res[out][0])


def test_every_fault_is_listed():
    assert {e[0] for e in CAUGHT} == set(T.FAULTS)


# ------------------------------------------------------------------------------------------------ 3. the statements are the model's
@pytest.mark.parametrize("tier", T.TIERS)
def test_lstm_gemm_statement_is_the_cell(tier):
    """torch.nn.LSTMCell in float64 on the same operands (h = 0, weight_hh = 0; the 16-bit rounding of the pre-activation applied
    where the kernel applies it) + dropout from the packed bits lands inside the bars"""
    inp = T.lg_at(T.lg_inputs(T.lg_case("b3_h96"), F16, tier), 40)
    b, h, k = inp["B"], inp["H"], inp["K"]
    z = TF.linear(inp["x"].double(), inp["w"].double(), inp["bias"].double()) + inp["addend"].double()
    assert torch.allclose(z, inp["z"], rtol=1e-13, atol=1e-13)
    pre16 = z.to(F16)
    cell = torch.nn.LSTMCell(4 * h, h, bias=False, dtype=F64)
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(4 * h, dtype=F64))
        cell.weight_hh.zero_()
        hh, c = cell(pre16.double(), (torch.zeros(b, h, dtype=F64), inp["c_prev"].double()))
    km = T._keep_mask(inp).double()
    g = pre16.double()
    act = torch.cat([torch.sigmoid(g[:, :h]), torch.sigmoid(g[:, h:2 * h]), torch.tanh(g[:, 2 * h:3 * h]), torch.sigmoid(g[:, 3 * h:])], 1)
    hd = (hh * km * inp["inv_keep"]).to(F16)
    got = {"pre16": pre16, "act": act.to(F16), "c_out": c.float(), "h_dsts": [hd, hd.clone(), hd.clone()], "outside": 0}
    res = T.check("lstm_gemm_fwd", inp, got)
    assert all(r <= 1.0 for r, _ in res.values()), res


@pytest.mark.parametrize("tier", T.TIERS)
def test_prenet_and_frame_statements_are_linear_relu(tier):
    """F.linear + relu + the mask x 2 in float64, rounded where the kernel rounds; F.linear for the frame"""
    inp = T.pre_inputs(T.PRE_CASES[1], BF16, tier, 6)
    b, p = inp["B"], inp["P"]
    x = inp["frame"].to(BF16).double()
    h1 = (torch.relu(TF.linear(x, inp["w0"].double())).to(BF16).double() * T.pre_keep(b, p, inp["seed"], 6, 0) * 2).to(BF16).double()
    y = (torch.relu(TF.linear(h1, inp["w1"].double())).to(BF16).double() * T.pre_keep(b, p, inp["seed"], 6, 1) * 2).to(BF16)
    res = T.check("prenet_infer", inp, {"dst": y})
    assert res["dst"][0] <= 1.0, res
    fi = T.fr_inputs(T.FR_CASES[1], BF16, tier, None, (6, 4))
    out = TF.linear(fi["hc"].double(), fi["w"].double(), fi["bias"].double())
    got = T.kernel_model("frame_infer", fi)
    got["frame_next"] = [out[t, :, :fi["NM"]].float() for t in range(T.FR_STEPS)]
    for t in range(4):
        got["mel_out"][:, t], got["gate_out"][:, t] = out[t, :, :fi["NM"]].float(), out[t, :, fi["NM"]].float()
    res = T.check("frame_infer", fi, got)
    assert all(r <= 1.0 for r, _ in res.values()), res


def test_zz_report():
    print()
    for k in sorted(RATIOS):
        print("    %-44s %.3f" % (k, RATIOS[k]))
