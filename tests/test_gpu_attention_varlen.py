"""Packed forward attention (dle_attention_fwd_varlen, csrc/attention.hip) and dle_embed_sum_packed on the MI355X.

* Bit identity: the valid rows of a padded batch under a 0 / -10000 mask through dle_attention_fwd(p = 0) equal the packed kernel's
  rows under torch.equal.  It follows from the code: a fully masked key block leaves the running max unchanged, adds exp(~-10000) = 0
  to the sum and 0 * V to the context; the one-pass softmax of the S = 128 kernel sums in the order of pass 1 over a single block.
* float64: the same cases against tests/_attention_reference (reference, bars, check_generic with ik = 1, no keep mask) at the
  valid rows; the bars are that module's.
* Nothing else is written: canary rows around ctx and past a sequence's length keep their bytes; a sequence's rows do not depend
  on its neighbours.
* The envelope and the 32-bit size limit are refused with an error text before anything is launched.
"""
import pytest
import torch

from tests import _attention_reference as A
from tests import _exact_grid as G
from tests import _varlen_cases as V

pytestmark = pytest.mark.gpu


def _F():
    from deeplearningexamples_amd import functional as F
    return F


def _C():
    from deeplearningexamples_amd import _cabi as C
    return C


def _varlen(cuda, qkv_packed, cu, max_seqlen, nh, canary=64):
    """attention_fwd_varlen into a view with `canary` rows of 0xFF bytes before and after; the canaries are checked. -> CPU ctx."""
    F = _F()
    t, h = qkv_packed.shape[0], nh * A.D
    buf = torch.full(((t + 2 * canary) * h,), -1, dtype=torch.int16, device=cuda)
    view = buf.view(qkv_packed.dtype).view(t + 2 * canary, h)[canary:canary + t]
    before = F.attention_varlen_launch_count()
    out = F.attention_fwd_varlen(qkv_packed.to(cuda), cu.to(cuda), max_seqlen, nh, V.SCALE, out=view)
    torch.cuda.synchronize()
    assert F.attention_varlen_launch_count() == before + 1
    rows = buf.view(t + 2 * canary, h)
    assert bool((rows[:canary] == -1).all()) and bool((rows[canary + t:] == -1).all()), "rows outside ctx were written"
    return out.cpu()


def _padded(cuda, case, nh):
    F = _F()
    ctx, _, _ = F.attention_fwd(case["qkv_pad"].to(cuda), case["mask_add"].to(cuda), case["b"], case["s"], nh, V.SCALE, p=0.0)
    return ctx.cpu()


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_bits_of_the_padded_kernel_and_fp64_bars(cuda, case, dtype):
    lengths, nh = case
    c = V.build(lengths, nh, dtype)
    got = _varlen(cuda, c["qkv_packed"], c["cu"], max(lengths), nh)
    assert not bool(torch.isnan(got.float()).any()), "a valid row was not written"
    want = _padded(cuda, c, nh)[c["rows"]]
    assert torch.equal(G.bits(got), G.bits(want)), "packed rows differ from the padded kernel's: %d elements" % int(
        (G.bits(got) != G.bits(want)).sum())
    # max_seqlen only sizes the grid: the padded S gives the same bits
    again = _varlen(cuda, c["qkv_packed"], c["cu"], c["s"], nh)
    assert torch.equal(G.bits(again), G.bits(got))
    full = torch.zeros(c["b"] * c["s"], nh * A.D, dtype=dtype)
    full[c["rows"]] = got
    V.check_valid_rows(A.heads(full, c["b"], c["s"], nh), c, lengths, nh, dtype, "varlen %s" % V.case_id(case))


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_rows_past_the_length_keep_their_bytes(cuda, dtype):
    """B = 1, len = 33, ctx a view of 128 canary rows: rows 33 .. 127 stay as they were (the 32-row slab store is guarded per row)."""
    F = _F()
    nh, h = 2, 2 * A.D
    c = V.build([33], nh, dtype)
    buf = torch.full((128 * h,), -1, dtype=torch.int16, device=cuda)
    view = buf.view(dtype).view(128, h)[:33]
    F.attention_fwd_varlen(c["qkv_packed"].to(cuda), c["cu"].to(cuda), 33, nh, V.SCALE, out=view)
    torch.cuda.synchronize()
    rows = buf.view(128, h)
    assert bool((rows[33:] == -1).all()), "rows at or past the length were written"
    assert torch.equal(G.bits(view.cpu()), G.bits(_padded(cuda, c, nh)[:33]))


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("lengths", [[33, 95], [95, 33]], ids=["33-95", "95-33"])
def test_each_sequence_equals_its_single_run(cuda, lengths, dtype):
    nh = 2
    c = V.build(lengths, nh, dtype)
    both = _varlen(cuda, c["qkv_packed"], c["cu"], max(lengths), nh)
    o = 0
    for n in lengths:
        one = _varlen(cuda, c["qkv_packed"][o:o + n].contiguous(), V.cu_seqlens([n]), n, nh)
        assert torch.equal(G.bits(both[o:o + n]), G.bits(one)), "sequence of length %d" % n
        o += n


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_a_sequence_does_not_depend_on_its_neighbour(cuda, dtype):
    lengths, nh = [100, 60, 200], 2
    c = V.build(lengths, nh, dtype)
    a = _varlen(cuda, c["qkv_packed"], c["cu"], 200, nh)
    other = c["qkv_packed"].clone()
    g = torch.Generator().manual_seed(3)
    other[100:160] = (torch.randn(60, other.shape[1], generator=g) * 2.0).to(dtype)
    b = _varlen(cuda, other, c["cu"], 200, nh)
    assert torch.equal(G.bits(a[:100]), G.bits(b[:100])) and torch.equal(G.bits(a[160:]), G.bits(b[160:]))
    assert not torch.equal(G.bits(a[100:160]), G.bits(b[100:160]))
    # not on Inf / NaN there either: the neighbour's rows inside a sequence's last 128-row tile are read as zero
    bad = c["qkv_packed"].clone()
    bad[100:160:2], bad[101:160:2] = float("inf"), float("nan")
    n = _varlen(cuda, bad, c["cu"], 200, nh)
    assert torch.equal(G.bits(a[:100]), G.bits(n[:100])) and torch.equal(G.bits(a[160:]), G.bits(n[160:]))


def test_envelope_is_refused_before_launch(cuda):
    C, F = _C(), _F()
    lib = C.lib()
    assert lib.dle_attention_varlen_supported(1024, 64) == 1 and lib.dle_attention_varlen_supported(1, 64) == 1
    assert lib.dle_attention_varlen_supported(128, 32) == 0 and lib.dle_attention_varlen_supported(1025, 64) == 0
    assert lib.dle_attention_varlen_supported(0, 64) == 0
    assert F.attention_varlen_supported(200, 64) and not F.attention_varlen_supported(200, 32)
    qkv = torch.zeros(5, 3 * 128, dtype=torch.float16, device=cuda)
    ctx = torch.zeros(5, 128, dtype=torch.float16, device=cuda)
    cu = torch.tensor([0, 5], dtype=torch.int32, device=cuda)
    before = F.attention_varlen_launch_count()
    for max_seqlen, heads, head_dim, total in ((128, 4, 32, 5), (1025, 2, 64, 5),
                                               # the smallest row count whose [T, 3 * 128] 16-bit tensor reaches 2^32 bytes
                                               (128, 2, 64, (2 ** 32 + 3 * 128 * 2 - 1) // (3 * 128 * 2))):
        rc = lib.dle_attention_fwd_varlen(C.ptr(qkv), C.ptr(cu), C.ptr(ctx), 1, max_seqlen, total, heads, head_dim, 0.125,
                                          C.dt(qkv), C.stream())
        assert rc != 0
        msg = lib.dle_last_error().decode()
        assert "attention_fwd_varlen" in msg, msg
        if total != 5:
            assert "4 GiB" in msg, msg
    torch.cuda.synchronize()
    assert F.attention_varlen_launch_count() == before
    assert not bool(ctx.any())


@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
def test_embed_sum_packed(cuda, dtype):
    F = _F()
    g = torch.Generator().manual_seed(9)
    vocab, h, s, lengths = 97, 128, 40, [40, 1, 17, 33]
    b = len(lengths)
    word, pos, typ = (torch.randn(n, h, generator=g).to(cuda) for n in (vocab, 64, 2))
    ids = torch.randint(0, vocab, (b * s,), generator=g).to(cuda)
    tt = torch.randint(0, 2, (b * s,), generator=g).to(cuda)
    want = F.embed_sum(word, pos, typ, ids, tt, s, dtype)
    pid = (torch.arange(b * s, dtype=torch.int32) % s).to(cuda)
    assert torch.equal(G.bits(F.embed_sum_packed(word, pos, typ, ids, tt, pid, dtype).cpu()), G.bits(want.cpu()))
    rows = V.valid_rows(lengths, s).to(cuda)
    got = F.embed_sum_packed(word, pos, typ, ids[rows].contiguous(), tt[rows].contiguous(), pid[rows].contiguous(), dtype)
    assert torch.equal(G.bits(got.cpu()), G.bits(want[rows].cpu()))
