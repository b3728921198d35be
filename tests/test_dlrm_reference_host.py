"""CPU checks of tests/_dlrm_reference.py, before a GPU is involved: the float64 statements agree with independent ones
(oracle/dlrm_oracle.py, the fixtures tests/golden/dlrm_dot_interact.npz and dlrm_embedding.npz, torch.autograd in float64), the
exactness preconditions hold on EVERY grid input tests/test_gpu_dlrm_reference.py uses (_exact_grid.check_exact: no GPU needed to
know that the bit-exact bars are sound), and a float32 evaluation on the CPU stays inside the derived bars."""
import os

import numpy as np
import pytest
import torch

from oracle import dlrm_oracle as O
from tests import _dlrm_reference as D
from tests._exact_grid import bits

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16


def _np(t):
    return t.to(F32).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ dot interaction
@pytest.mark.parametrize("shape", [(5, 27, 128), (6, 1, 32), (6, 2, 32), (4, 13, 20), (3, 33, 128)], ids=str)
def test_dot_statements_match_the_oracle(shape):
    b, r, c = shape
    case = D.dot_case(shape, "gauss", F16)
    assert D.out_width(r, c) == O.interact_out_width(r, c) and case["y"].shape == (b, O.interact_out_width(r, c))
    ri, ci = D.tril_pairs(r)
    ori, oci = O.tril_pairs(r)
    assert np.array_equal(ri.numpy(), ori) and np.array_equal(ci.numpy(), oci)
    # the oracle accumulates in fp32: it has to sit inside the derived fp32 bar around the float64 statement
    y32 = _t(O.dot_interact_fwd(_np(case["x"]), np.float32))
    assert D.worst_ratio(y32, case["y"], D.bar(case["y"], case["ymag"], c + 2, F32)) <= 1.0
    g32, m32 = O.dot_interact_bwd(_np(case["x"]), _np(case["ug"]), np.float32)
    assert D.worst_ratio(_t(g32), case["grad"], D.bar(case["grad"], case["gmag"], r + 3, F32)) <= 1.0
    assert torch.equal(_t(m32).to(F64), case["head"])
    fg, fm = D.fused(case)
    tot = g32.copy()
    tot[:, 0, :] += m32
    assert D.worst_ratio(_t(tot), fg, D.bar(fg, fm, r + 3, F32)) <= 1.0
    g2, none, m2 = D.dot_interact_bwd(case["x"].to(F64), case["ug"].to(F64), True)
    assert none is None and torch.equal(g2, fg) and torch.equal(m2, fm)


def test_dot_statements_match_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "dlrm_dot_interact.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in z.files if k.endswith("_x")})
    assert keys
    for k in keys:
        x, ug = _t(z[k + "_x"]).to(F64), _t(z[k + "_ug"]).to(F64)
        r, c = x.shape[1:]
        y, ymag = D.dot_interact_fwd(x)
        assert D.worst_ratio(_t(z[k + "_y"]), y, D.bar(y, ymag, c + 2, F32)) <= 1.0, k
        g, none, gmag = D.dot_interact_bwd(x, ug, True)
        assert D.worst_ratio(_t(z[k + "_gx_total"]), g, D.bar(g, gmag, r + 3, F32)) <= 1.0, k


def test_dot_gradient_is_the_autograd_gradient():
    """float64 autograd of the forward statement: both pieces of the gradient land on the same leaf (the fused form)"""
    case = D.dot_case((4, 13, 20), "gauss", F16)
    x = case["x"].to(F64).requires_grad_()
    y, _ = D.dot_interact_fwd(x)
    y.backward(case["ug"].to(F64))
    fg, fm = D.fused(case)
    assert bool(((x.grad - fg).abs() <= 1e-13 * fm + 1e-300).all())
    g, head, _ = D.dot_interact_bwd(case["x"].to(F64), case["ug"].to(F64), False)
    assert torch.equal(g, case["grad"]) and torch.equal(head, case["ug"][:, :20].to(F64))


@pytest.mark.parametrize("shape", D.DOT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dot_grid_inputs_are_exactly_summable(shape):
    case = D.dot_case(shape, "grid", F16)
    D.dot_check_exact(case)
    for dt in (F16, BF16):                                    # the grid is exact in every type: one reference serves all
        assert torch.equal(case["x"].to(dt).to(F32), case["x"]) and torch.equal(case["ug"].to(dt).to(F32), case["ug"])
    for v in (case["y"], case["grad"], D.fused(case)[0]):
        D.round_once(v, F16)                                  # (asserts that the value is exact in fp32)
    # round-to-nearest-even is exercised: forward sums that need more than 8 (bf16) / 11 (fp16, at C = 256 only: a sum of C terms
    # below 1 on the 1/16 grid has at most log2(16 C) bits) significant bits and land on a tie
    y = case["y"]
    for dt, wide_enough in ((BF16, shape[1] >= 9 and shape[2] >= 32), (F16, shape[1] >= 9 and shape[2] >= 256)):
        r = D.round_once(y, dt).to(F64)
        tie = ((r - y).abs() == 0.5 * D.ulp16(y, dt)) & (y != 0)
        assert bool(tie.any()) or not wide_enough, "no rounding tie at %s in %s" % (shape, dt)


@pytest.mark.parametrize("shape", D.DOT_GAUSS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=D.name)
def test_dot_float32_evaluation_is_inside_the_bar(shape, dtype):
    if shape[0] > 1000:
        shape = (64,) + tuple(shape[1:])                      # (the bar does not depend on the batch: a slice is enough here)
    b, r, c = shape
    case = D.dot_case(shape, "gauss", dtype)
    y = _t(O.dot_interact_fwd(_np(case["x"]), np.float32)).to(dtype)
    assert D.worst_ratio(y, case["y"], D.bar(case["y"], case["ymag"], c + 2, dtype)) <= 1.0
    g, _ = O.dot_interact_bwd(_np(case["x"]), _np(case["ug"]), np.float32)
    assert D.worst_ratio(_t(g).to(dtype), case["grad"], D.bar(case["grad"], case["gmag"], r + 3, dtype)) <= 1.0


# ------------------------------------------------------------------------------------------------ embeddings
def test_hash_and_offsets_are_floor_mod():
    sizes = [7, 1, 1000, 2]
    off = D.table_offsets(sizes)
    assert np.array_equal(off.numpy(), O.table_offsets(sizes))
    idx = torch.tensor([[-22, -1, -3000, -1], [-7, 5, 2999, 3], [0, 0, 0, 0], [6, -9, -1, -2]], dtype=torch.int64)
    rows = D.hash_offset(idx, off, torch.tensor(sizes))
    for b in range(idx.shape[0]):
        for t, s in enumerate(sizes):
            assert int(rows[b, t]) == int(idx[b, t]) % s + int(off[t])          # python's % is the floor-mod
    assert np.array_equal(rows.numpy(), O.offset_indices(O.hash_indices(idx.numpy(), sizes), off.numpy()))
    assert torch.equal(D.hash_offset(idx), idx)


def test_embedding_statements_match_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "dlrm_embedding.npz"))
    idx, off, sizes, w0 = _t(z["idx_in"]), _t(z["offsets"]), _t(z["sizes"]), _t(z["w0"])
    rows = D.hash_offset(idx, off, sizes)
    assert np.array_equal(rows.numpy(), O.offset_indices(z["idx_hashed"], z["offsets"]))
    assert torch.equal(bits(D.gather(w0, rows, F32)), bits(_t(z["out"])))
    ug = _t(z["ug"])
    ref, mag, dup = D.sparse_sgd(w0.to(F64), rows, ug.to(F64), float(z["lr"]))
    assert D.worst_ratio(_t(z["w1"]), ref, D.bar(ref, mag, dup[:, None] + 2, F32)) <= 1.0
    assert int(dup.sum()) == rows.numel() and np.allclose(ref.numpy(), O.sparse_sgd(z["w0"], rows.numpy(), z["ug"], float(z["lr"])),
                                                         rtol=1e-6, atol=1e-7)


def test_gather_with_a_batch_stride():
    case = D.gather_case(12, batch=9)
    rows = D.hash_offset(case["wild"], case["off"], case["sizes"])
    b, t = rows.shape
    d = 12
    stride = (t + 1) * d
    flat = torch.full((b * stride + 5,), -7.0, dtype=BF16)
    out = D.gather_strided(case["w"], rows, flat, d, stride)
    want = flat.clone()
    for i in range(b):
        for j in range(t):
            want[d + i * stride + j * d: d + i * stride + (j + 1) * d] = case["w"][rows[i, j]].to(BF16)
    assert torch.equal(bits(out), bits(want))
    assert bool((out[:b * stride].view(b, t + 1, d)[:, 0, :] == -7.0).all()) and bool((out[b * stride:] == -7.0).all())
    assert torch.equal(bits(flat), bits(torch.full_like(flat, -7.0)))            # the input buffer is left alone


@pytest.mark.parametrize("dim", D.GATHER_DIMS)
def test_gather_inputs(dim):
    case = D.gather_case(dim)
    assert torch.equal(case["w"] * 4, torch.round(case["w"] * 4)) and float(case["w"].abs().max()) <= 4.0
    for dt in (F16, BF16):
        assert torch.equal(case["w"].to(dt).to(F32), case["w"])      # exact in 16 bits too: the rounding is the identity here ...
    assert bool((case["wild"] < 0).any()) and bool((case["wild"] >= case["sizes"][None, :]).any())


@pytest.mark.parametrize("p", D.sgd_params(), ids=D.sgd_id)
def test_sgd_grid_inputs_are_exactly_summable(p):
    cfg, dim, gdtype, batch = p
    case = D.sgd_case(cfg, dim, gdtype, batch, "grid")
    D.sgd_check_exact(case)
    D.round_once(case["ref"], F32)
    assert bool((case["dup"] == 0).any()) and int(case["dup"].sum()) == batch * case["tables"]
    assert bool(torch.isnan(case["g"][:, 0, :].float()).all()) and case["g"].dtype == gdtype
    # a serial fp32 evaluation (torch's index_add_) gives the same bits: the sums are exact in fp32 in this order at least
    w = case["w"].clone()
    w.index_add_(0, case["rows"].reshape(-1), case["g"][:, 1:, :].to(F32).reshape(-1, dim), alpha=-D.SGD_LR * D.SGD_SCALE)
    assert torch.equal(bits(w), bits(D.round_once(case["ref"], F32)))


def test_sgd_configurations_reach_the_paths_they_name():
    """the dispatcher's size rules, restated: which tables of each configuration are small / tiny / mid / listed"""
    def classes(sizes, dim, sixteen_bit):
        out, n_small = [], 0
        for r in sizes:
            if r * dim * 4 <= 64 * 1024 and n_small < 64:
                n_small += 1
                out.append("tiny" if sixteen_bit and r <= 128 and dim <= 128 else "lds")
            elif sixteen_bit and r <= 4096 and dim <= 128 and len(sizes) <= 128:
                out.append("mid")
            else:
                out.append("list")
        return out
    c = D.SGD_CONFIGS
    assert classes(c["a"]["sizes"], 128, True) == ["tiny", "tiny", "tiny", "tiny", "mid", "mid", "list", "mid"]
    assert classes(c["b"]["sizes"], 64, True) == ["tiny"] * 6 + ["lds", "lds", "mid", "list"]
    assert classes(c["b"]["sizes"], 32, True) == ["tiny"] * 6 + ["lds", "lds", "lds", "list"]
    assert classes(c["c"]["sizes"], 256, True) == ["lds", "lds", "list", "list"]
    assert classes(c["d"]["sizes"], 128, False) == ["lds", "lds", "lds", "list", "list"]
    assert classes(c["d"]["sizes"], 64, False) == ["lds", "lds", "lds", "list", "list"]
    assert classes(c["e"]["sizes"], 128, True) == ["tiny"] * 64 + ["mid"] * 6 + ["list"]
    f = classes(c["f"]["sizes"], 16, True)
    assert len(f) == 130 and f[:3] == ["tiny", "lds", "list"] and f[96:99] == ["list", "list", "list"] and "mid" not in f


# ------------------------------------------------------------------------------------------------ BCE with logits
@pytest.mark.parametrize("n", D.BCE_SIZES)
def test_bce_statement_matches_torch_in_float64(n):
    x, y = D.bce_case(n, F32)
    x64 = x.to(F64).requires_grad_()
    want = torch.nn.functional.binary_cross_entropy_with_logits(x64, y.to(F64))
    (want * 3.0).backward()
    loss, mag, grad = D.bce_with_logits(x.to(F64), y.to(F64), 3.0)
    assert abs(float(loss) - float(want.detach())) <= 1e-14 * float(mag)
    assert bool(((grad - x64.grad).abs() <= 1e-15 * 3.0 / n).all())


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=D.name)
def test_bce_edge_values(dtype):
    x, y = D.bce_edge(dtype)
    assert bool(torch.isfinite(x.float()).all()) and x.numel() == 18
    loss, mag, grad = D.bce_with_logits(x.to(F64), y.to(F64))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    # where float64's own sigmoid(x) - y cancels (x = 20, y = 1: 2e-9 left of 1), the statement keeps full precision
    i = 9 + 3
    assert float(x[i]) == 20.0 and float(y[i]) == 1.0
    assert abs(float(grad[i]) * 18 + np.exp(-20.0) / (1 + np.exp(-20.0))) <= 1e-24
    big = x.float().abs() > 1000
    x64, y64 = x.to(F64), y.to(F64)
    for j in torch.nonzero(big).flatten().tolist():
        l1, _, g1 = D.bce_with_logits(x64[j:j + 1], y64[j:j + 1])
        assert float(l1) == float(x64[j].clamp_min(0) - x64[j] * y64[j]) and float(g1) in (0.0, 1.0, -1.0)


def test_bce_float32_evaluation_is_inside_the_bars():
    """the kernel's formula in torch float32 on the CPU: loss within gamma(N + 8) sum|terms|, gradient within 8 u |ref| + half an
    ulp -- which the textbook sigmoid(x) - y misses wherever sigmoid(x) rounds towards y (asserted too: the bar has teeth)"""
    n = 4099
    x, y = D.bce_case(n, F32)
    y = (x > 0).to(F32)
    loss, mag, grad = D.bce_with_logits(x.to(F64), y.to(F64), 1024.0)
    e = torch.exp(-x.abs())
    l32 = (x.clamp_min(0) - x * y + torch.log1p(e)).sum() / n
    assert abs(float(l32) - float(loss)) <= float(D.gamma(n + 8) * mag)
    p, q = 1.0 / (1.0 + e), e / (1.0 + e)
    s, c = torch.where(x >= 0, p, q), torch.where(x >= 0, q, p)
    gs = torch.tensor(1024.0) / n
    bar = 9 * D.U * grad.abs()
    assert D.worst_ratio(((1.0 - y) * s - y * c) * gs, grad, bar) <= 1.0
    assert D.worst_ratio((s - y) * gs, grad, bar) > 1.0
