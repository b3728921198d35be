"""The DLRM sparse-side kernels (csrc/dot_interact.hip, embedding.hip, emb_onehot.hip, the BCE loss of elementwise.hip) against the
float64 statements of tests/_dlrm_reference.py.

(a) exactly summable inputs (k / 4): the output bits equal the float64 value rounded once, on every route of every launcher --
    MFMA, persistent walks, generic, misaligned pointers, every path of the sparse-SGD dispatcher; every output is the head of an
    over-long NaN buffer whose tail keeps its bits.
(b) gaussian inputs: every element within half an output ulp + gamma(n) sum|terms| (derived in _dlrm_reference.py).
(c) BCE with logits: loss within gamma(N + 8) sum|terms|, gradient within half an output ulp + 8 u |ref|, edge values included.

Largest |error| / bar on the GPU (MI355X) -- a record, the pass condition is <= 1 (printed by test_zz_report_ratios with -s):
    dot forward          fp16 0.993   bf16 0.997   fp32 0.101      (MFMA and generic routes give the same figures)
    dot backward         fp16 0.996   bf16 0.999   fp32 0.196      (fused and unfused alike)
    sparse SGD, atomic   fp16 0.489   bf16 0.353   fp32 0.507
    sparse SGD, dedup    a 0.333   b 0.333   d (fp32 gradients) 0.425
    BCE N(0, 4)          loss fp32 0.099, fp16 0.041, bf16 0.050   gradient fp32 0.780, fp16 0.999, bf16 0.999
    BCE edge values      loss 0.506 (all types)                    gradient fp32 0.543, fp16 0.927, bf16 0.911
The 16-bit figures near 1 are the half ulp of the store (an output a hair from a tie); the fp32 ones show the room in gamma(n).
Before the BCE gradient was written as (1 - y) sigmoid(x) - y sigmoid(-x), its fp32 ratio was 42.9 on N(0, 4) and 1.9e6 at
x = 80, y = 1 (sigmoid(x) - 1 in fp32 is 0 there), and the bf16 edge ratio 503.
"""
import pytest
import torch

from tests import _dlrm_reference as D
from tests._exact_grid import Out, assert_same, bits, ulp16

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
RATIOS = {}


def _F():
    from deeplearningexamples_amd import functional as F
    return F


def _C():
    from deeplearningexamples_amd import _cabi as C
    return C


def _note(key, r, where):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, "%s: |error| / bar = %.3f at %s" % (key, r, where)


def _same(got, want, what):
    assert_same(bits(got.cpu()), bits(want), what)


# ------------------------------------------------------------------------------------------------ dot interaction
class _Buf:
    """A tensor of `shape` at `skip` elements into an Out buffer (skip = 0: aligned; 8 bytes' worth: the pointer the launchers
    answer with their generic kernels); head and tail must keep their NaN bits."""

    def __init__(self, shape, dtype, dev, skip=0, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.o = Out((skip + n,), dtype, dev)
        self.skip = skip
        self.t = self.o.t[skip:].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        self.o.check(what)
        assert bool(torch.isnan(self.o.t[:self.skip].float()).all()), "%s wrote in front of its output" % what
        return self.t


def _dot_run(case, dtype, force, dev, skip=0):
    """forward, backward and fused backward through the C ABI -> (y, grad, mlp_grad, fused grad) on the CPU"""
    C = _C()
    b, r, c = case["x"].shape
    ow = D.out_width(r, c)
    assert _F().dot_interact_out_width(r, c) == ow
    x = _Buf((b, r, c), dtype, dev, skip, case["x"].to(dtype)).t
    ug = _Buf((b, ow), dtype, dev, skip, case["ug"].to(dtype)).t
    assert x.data_ptr() % 16 == (8 if skip else 0) and ug.data_ptr() % 16 == (8 if skip else 0)
    y, g, m, gf = (_Buf(s, dtype, dev, skip) for s in ((b, ow), (b, r, c), (b, c), (b, r, c)))
    C.call("dle_dot_interact_fwd", C.ptr(x), C.ptr(y.t), b, r, c, C.dt(dtype), int(force), C.stream())
    C.call("dle_dot_interact_bwd", C.ptr(x), C.ptr(ug), C.ptr(g.t), C.ptr(m.t), b, r, c, C.dt(dtype), int(force), C.stream())
    C.call("dle_dot_interact_bwd", C.ptr(x), C.ptr(ug), C.ptr(gf.t), 0, b, r, c, C.dt(dtype), int(force), C.stream())
    torch.cuda.synchronize()
    return tuple(o.check(what).cpu() for o, what in ((y, "forward"), (g, "backward"), (m, "backward (mlp_grad)"), (gf, "fused backward")))


def _dot_layout_facts(case, dtype, y, m):
    b, r, c = case["x"].shape
    _same(y[:, :c], case["x"][:, 0, :].to(dtype), "y[:, :C] == x[:, 0, :]")
    assert bool((bits(y[:, c + r * (r - 1) // 2:]) == 0).all()), "pad columns"
    _same(m, case["ug"][:, :c].to(dtype), "mlp_grad == upstream[:, :C]")


@pytest.mark.parametrize("route", D.DOT_ROUTES, ids=[r[0] for r in D.DOT_ROUTES])
@pytest.mark.parametrize("shape", D.DOT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dot_interact_exact(cuda, shape, route):
    _, dtype, force = route
    case = D.dot_case(shape, "grid", dtype)
    y, g, m, gf = _dot_run(case, dtype, force, cuda)
    where = "%s %s" % (shape, route[0])
    _same(y, D.round_once(case["y"], dtype), "forward " + where)
    _same(g, D.round_once(case["grad"], dtype), "backward " + where)
    _same(gf, D.round_once(D.fused(case)[0], dtype), "fused backward " + where)
    _dot_layout_facts(case, dtype, y, m)


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=D.name)
def test_dot_interact_misaligned_pointers(cuda, dtype):
    """x, the upstream gradient and every output 8 bytes into their buffers: the launchers' generic kernels, the same bits"""
    case = D.dot_case((5, 27, 128), "grid", dtype)
    a = _dot_run(case, dtype, False, cuda)
    b = _dot_run(case, dtype, False, cuda, skip=8 // torch.empty(0, dtype=dtype).element_size())
    for u, v, what in zip(a, b, ("forward", "backward", "mlp_grad", "fused backward")):
        _same(v, u, what + ": misaligned vs aligned")
    _same(b[0], D.round_once(case["y"], dtype), "forward, misaligned")
    _same(b[3], D.round_once(D.fused(case)[0], dtype), "fused backward, misaligned")


@pytest.mark.parametrize("route", D.DOT_ROUTES, ids=[r[0] for r in D.DOT_ROUTES])
@pytest.mark.parametrize("shape", D.DOT_GAUSS, ids=lambda s: "x".join(map(str, s)))
def test_dot_interact_gaussian(cuda, shape, route):
    tag, dtype, force = route
    case = D.dot_case(shape, "gauss", dtype)
    b, r, c = shape
    y, g, m, gf = _dot_run(case, dtype, force, cuda)
    where = "%s %s" % (shape, tag)
    fg, fm = D.fused(case)
    _note("dot_fwd." + tag, D.worst_ratio(y, case["y"], D.bar(case["y"], case["ymag"], c + 2, dtype)), where)
    _note("dot_bwd." + tag, D.worst_ratio(g, case["grad"], D.bar(case["grad"], case["gmag"], r + 1 + 2, dtype)), where)
    _note("dot_bwd_fused." + tag, D.worst_ratio(gf, fg, D.bar(fg, fm, r + 1 + 2, dtype)), where)
    _dot_layout_facts(case, dtype, y, m)


# ------------------------------------------------------------------------------------------------ gather
def _gather_checks(case, dim, out_dtype, dev):
    F = _F()
    w, off, sizes = case["w"].to(dev), case["off"].to(dev), case["sizes"].to(dev)
    b, t = case["idx"].shape
    for what, idx, hs in (("plain", case["idx"], None), ("hashed", case["wild"], sizes)):
        rows = D.hash_offset(idx, case["off"], None if hs is None else case["sizes"])
        assert int(rows.min()) >= 0 and bool((rows < case["off"][1:][None, :]).all()) and bool((rows >= case["off"][:-1][None, :]).all())
        want = D.gather(case["w"], rows, out_dtype)
        o = Out((b, t, dim), out_dtype, dev)
        F.emb_gather_fwd(w, idx.to(dev), off, hs, out_dtype, out=o.t)           # (out_batch_stride 0: the dense [B, T, dim])
        torch.cuda.synchronize()
        _same(o.check("gather").cpu(), want, "gather with offsets, %s, dim %d" % (what, dim))
        ro = Out((b, 2 * t), torch.int32, dev)               # (int64 rows: Out compares 4-byte words)
        C = _C()
        idx_d = idx.to(dev)
        C.call("dle_emb_offset_indices", C.ptr(idx_d), C.ptr(off), C.ptr(hs), C.ptr(ro.t), b, t, C.stream())
        torch.cuda.synchronize()
        assert torch.equal(ro.check("offset_indices").view(torch.int64).cpu(), rows), "emb_offset_indices, " + what
        assert torch.equal(F.emb_offset_indices(idx_d, off, hs).cpu(), rows)
        # the joint table with pre-offset rows (no offsets), into slots 1.. of a [B, T + 1, dim] buffer of sentinels
        stride = (t + 1) * dim
        so = Out((b, t + 1, dim), out_dtype, dev, fill=torch.full((b, t + 1, dim), -7.0, dtype=out_dtype))
        before = so.t.cpu().clone().reshape(-1)
        F.emb_gather_fwd(w, rows.to(dev), None, None, out_dtype, out=so.t[:, 1:, :], out_batch_stride=stride)
        torch.cuda.synchronize()
        got = so.check("strided gather").cpu()
        _same(got.reshape(-1), D.gather_strided(case["w"], rows, before, dim, stride), "strided gather, %s, dim %d" % (what, dim))
        _same(got[:, 0, :], torch.full((b, dim), -7.0, dtype=out_dtype), "slot 0 of every sample")


@pytest.mark.parametrize("out_dtype", [F32, F16, BF16], ids=D.name)
@pytest.mark.parametrize("dim", D.GATHER_DIMS)
def test_gather_exact(cuda, dim, out_dtype):
    _gather_checks(D.gather_case(dim), dim, out_dtype, cuda)


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=D.name)
def test_gather_second_grid_lap(cuda, out_dtype):
    dim, t, batch = D.GATHER_LAP
    assert batch * t > 2048 * 32                              # the grid cap x rows per workgroup and trip at dim 128
    _gather_checks(D.gather_case(dim, batch), dim, out_dtype, cuda)


# ------------------------------------------------------------------------------------------------ sparse SGD
def _sgd_runs(case, dim, dev, lr_dev):
    """-> (W' of the atomic kernel, W' of the duplicate-free dispatcher, twice) on the CPU; checks the workspace invariant"""
    F = _F()
    t = case["tables"]
    rows, g = case["rows"].to(dev), case["g"].to(dev)
    scale = torch.tensor([D.SGD_SCALE], device=dev)
    lr = torch.tensor([D.SGD_LR], device=dev) if lr_dev else D.SGD_LR
    stride = (t + 1) * dim
    outs = []
    o = Out(tuple(case["w"].shape), F32, dev, fill=case["w"])
    F.emb_sparse_sgd_(o.t, rows, g[:, 1:, :], lr, scale=scale)
    torch.cuda.synchronize()
    outs.append(o.check("emb_sparse_sgd").cpu())
    for _ in range(2):
        o = Out(tuple(case["w"].shape), F32, dev, fill=case["w"])
        ws = F.EmbUpdateWorkspace(case["off"].numpy(), dim, dev)
        F.emb_sgd_dedup_(o.t, rows, g[:, 1:, :], ws, lr, scale=scale, grad_batch_stride=stride)
        torch.cuda.synchronize()
        assert int((ws.head != -1).sum()) == 0, "ws.head is not all -1 after the update"
        outs.append(o.check("emb_sgd_dedup").cpu())
    return outs


@pytest.mark.parametrize("p", D.sgd_params(), ids=D.sgd_id)
def test_sparse_sgd_exact(cuda, p):
    cfg, dim, gdtype, batch = p
    F = _F()
    case = D.sgd_case(cfg, dim, gdtype, batch, "grid")
    want = D.round_once(case["ref"], F32)
    untouched = case["dup"] == 0
    assert bool(untouched.any()) and torch.equal(bits(want[untouched]), bits(case["w"][untouched]))
    for lr_dev in (False, True):
        atomic, a, b = _sgd_runs(case, dim, cuda, lr_dev)
        where = "%s, %s lr" % (D.sgd_id(p), "device" if lr_dev else "host")
        _same(atomic, want, "emb_sparse_sgd_ " + where)
        _same(a, want, "emb_sgd_dedup_ " + where)
        _same(b, a, "emb_sgd_dedup_, second run " + where)
    # the skip flag: no bit moves, in either kernel
    rows, g = case["rows"].to(cuda), case["g"].to(cuda)
    skip = torch.ones(1, device=cuda)
    o = Out(tuple(case["w"].shape), F32, cuda, fill=case["w"])
    ws = F.EmbUpdateWorkspace(case["off"].numpy(), dim, cuda)
    F.emb_sgd_dedup_(o.t, rows, g[:, 1:, :], ws, D.SGD_LR, scale=torch.tensor([D.SGD_SCALE], device=cuda), skip_flag=skip,
                     grad_batch_stride=(case["tables"] + 1) * dim)
    F.emb_sparse_sgd_(o.t, rows, g[:, 1:, :], D.SGD_LR, skip_flag=skip)
    torch.cuda.synchronize()
    _same(o.check("skipped update").cpu(), case["w"], "skip flag " + D.sgd_id(p))
    assert int((ws.head != -1).sum()) == 0


@pytest.mark.parametrize("p", D.sgd_params(D.SGD_GAUSS, [4099]), ids=D.sgd_id)
def test_sparse_sgd_gaussian(cuda, p):
    cfg, dim, gdtype, batch = p
    case = D.sgd_case(cfg, dim, gdtype, batch, "gauss")
    b = D.bar(case["ref"], case["mag"], case["dup"][:, None] + 2, F32)
    atomic, a, _ = _sgd_runs(case, dim, cuda, True)
    _note("sgd_atomic." + D.name(gdtype), D.worst_ratio(atomic, case["ref"], b), D.sgd_id(p))
    _note("sgd_dedup.%s.%s" % (cfg, D.name(gdtype)), D.worst_ratio(a, case["ref"], b), D.sgd_id(p))
    untouched = case["dup"] == 0
    assert torch.equal(bits(a[untouched]), bits(case["w"][untouched])) and torch.equal(bits(atomic[untouched]), bits(case["w"][untouched]))


# ------------------------------------------------------------------------------------------------ BCE with logits
def _bce_check(x, y, dtype, dev, key, where):
    """every variant on one (logits, labels): ld_logits 1 / 8, grad_scale absent / 1024, want_grad False"""
    F = _F()
    n = x.numel()
    x64, y64 = x.to(D.F64), y.to(D.F64)
    wide = torch.full((n, 8), float("nan"), dtype=dtype)
    wide[:, 3] = x
    wide = wide.to(dev)
    yd = y.to(dev)
    first = None
    for scale in (None, 1024.0):
        loss_ref, loss_mag, grad_ref = D.bce_with_logits(x64, y64, 1.0 if scale is None else scale)
        loss_bar = D.gamma(n + 8) * loss_mag
        # (fp32 gradients have no separate storage rounding in the issue's bar; half an fp32 ulp is below u |ref|)
        grad_bar = 8 * D.U * grad_ref.abs() + 0.5 * (ulp16(grad_ref, dtype) if dtype != F32 else grad_ref.abs() * 2.0 ** -23)
        sd = None if scale is None else torch.tensor([scale], device=dev)
        for ld, logits in ((1, x.to(dev)), (8, wide[:, 3])):
            loss, dl = F.bce_with_logits(logits, yd, grad_scale=sd, ld_logits=ld)
            loss0, none = F.bce_with_logits(logits, yd, grad_scale=sd, want_grad=False, ld_logits=ld)
            torch.cuda.synchronize()
            assert none is None and dl.dtype == dtype and dl.shape == (n,)
            assert bool(torch.isfinite(loss).all()) and not bool(torch.isnan(dl.float()).any()), where
            for v in (loss, loss0):
                _note(key + ".loss", D.worst_ratio(v, loss_ref.reshape(1), loss_bar.reshape(1)), where)
            _note(key + ".grad", D.worst_ratio(dl, grad_ref, grad_bar), where)
            if n <= 1024:                                    # one workgroup (256 threads x 4): one order of addition, the same
                # loss bits.  (Past it the workgroups' partial sums meet in an fp32 atomic, in the order they finish: both losses
                # are held to the bar above.)
                assert torch.equal(bits(loss.cpu()), bits(loss0.cpu())), "want_grad changes the loss"
                first = loss.cpu() if first is None else first
                assert torch.equal(bits(loss.cpu()), bits(first)), "ld_logits / grad_scale change the loss"
    return first


@pytest.mark.parametrize("n", D.BCE_SIZES)
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=D.name)
def test_bce_with_logits_gaussian(cuda, dtype, n):
    x, y = D.bce_case(n, dtype)
    _bce_check(x, y, dtype, cuda, "bce." + D.name(dtype), "N(0,4), n = %d" % n)
    # labels that sigmoid(x) rounds to: the gradient is the small side of the sigmoid, never NaN (checked inside)
    _bce_check(x, (x > 0).to(F32), dtype, cuda, "bce." + D.name(dtype), "y = round(sigmoid(x)), n = %d" % n)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=D.name)
def test_bce_with_logits_edge_values(cuda, dtype):
    x, y = D.bce_edge(dtype)
    _bce_check(x, y, dtype, cuda, "bce_edge." + D.name(dtype), "edge vector")
    for i in range(x.numel()):                               # and one value at a time: the bar is that term's own
        xi, yi = x[i:i + 1], y[i:i + 1]
        loss = _bce_check(xi, yi, dtype, cuda, "bce_edge." + D.name(dtype), "x = %g, y = %g" % (float(xi), float(yi)))
        if abs(float(xi)) > 1000:                            # exp(-|x|) is 0: the loss IS max(x, 0) - x y
            want = (xi.double().clamp_min(0) - xi.double() * yi.double()).to(F32)
            assert bool(torch.isfinite(loss).all()) and torch.equal(bits(loss), bits(want)), "loss at x = %g" % float(xi)


def test_zz_report_ratios():
    """(runs last in this file) the record quoted in the module docstring; -s shows it"""
    for k in sorted(RATIOS):
        print("GPU ratio %-32s %.3f" % (k, RATIOS[k]))
    assert all(r <= 1.0 for r in RATIOS.values())
