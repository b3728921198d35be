"""The three ResNet-50 kernels that fold BatchNorm into a neighbouring 1x1 convolution -- csrc/conv_bnload.hip
(dle_conv1x1_bnload_fwd / _fwd2), csrc/conv_bnbwd.hip (dle_conv1x1_bnbwd_dgrad / _dgrad_wgrad) and csrc/gemm_expand.hip
(dle_gemm_expand_masked_bnred + dle_bn_bwd_finish) -- against a float64 statement of their operations.  GPU only.

The older files (test_gpu_conv_bnload.py, test_gpu_conv_bnbwd.py, test_gpu_conv_bnbwd_wgrad.py, test_gpu_gemm_bnred.py) compare each
fused kernel with the two launches it replaces: the library against itself, under hand-picked bars.  A fault that both sides share
(a coefficient, the bit order of a mask, a row past M entering a reduction) passes them.  This file ties the kernels to the
operation, as test_gpu_bn_reference.py does for the stand-alone passes.  The reference, the inputs, the derivation of every bar and
the comparisons live in tests/_bnconv_reference.py (read its docstring first); tests/test_bnconv_reference_host.py proves them on the
CPU against an fp32 model with planted faults.  Every tolerance is "bits" or a formula in u = 2^-24, the magnitudes of the terms and
a chain length counted here from the kernels' structure:

    statistics of bnload:   ceil(row tiles / groups) trips + 4 (16 lanes) + wavefronts + 1, S1 one more (the square)
    bnred sums:             the same, + 3 for dgamma2 (the roundings of g (t2 - mean2) rstd2); the folds over groups run in fp64
    gw:                     ceil(row tiles / groups) x 64 rows through the matrix unit + ceil(groups / 16) + 16 (wgrad1x1_fold)

How the kernels are called.  Through the C ABI, with every output, partial buffer and workspace a view at the head of a NaN-filled
(0xFF for bytes) over-long buffer (tests/_exact_grid.Out): the return code must be 1, the tail must keep its bits, a NaN left inside
an output fails its comparison.  The Python wrapper must return the same bits, and so must a second launch into fresh buffers (the
fold orders are fixed).  Rows past M of every input allocation hold a large finite poison with all keep bits set.

Shapes.  M = 4096 (a power of two: exact backward coefficients), 4096 + 37, and (groups + 1) x rows-per-tile + 37, where some
workgroups take a second tile and the last tile is partial; groups and rows per tile come from dle_conv1x1_bnload_groups,
dle_conv1x1_bnbwd_groups, dle_conv1x1_bnbwd_wgrad_workspace and dle_gemm_expand_groups (rows per tile = 4096 / groups(4096), the cap
= groups at a very large M).  Every case runs the exact kind and the Gaussian kind, in bf16 and fp16.

Worst |error| / bar measured on the MI355X over the whole file, both dtypes (a record; the pass condition is <= 1):
    16-bit outputs (one rounding: a tie reaches ulp16 / 2, the first term of the bar)
        y 1.000, out 0.999, dt 1.000 (the stand-alone bn_bwd too), dx 0.991 (both forms), dx of the bnred GEMM 0.998
    gw of the weight-gradient form 0.846 (its bar carries whole 16-bit steps of the dt near a rounding boundary)
    fp32 sums: S0 0.013, S1 0.054, dbeta2 0.007, dgamma2 0.014
    mean 0.083, rstd 0.137, running_mean 0.348, running_var 0.289; exact kind: rstd 0.500 ulp, running stats 0.45 of 4 u

A bug this file found.  The keep bits were taken from the fp32 value (v > 0) while y is that value rounded: an fp32 value in
(0, 2^-25] rounds to an fp16 zero (below 2^-134: to a bf16 zero) and kept its bit set (test_bnload[k256-n64-res0-wrap-fp16], one
element of 12.6 million).  conv_bnload_kernel, bn_apply_pf_kernel, bn_apply2_pf_kernel and bn_relu_maxpool_k3s2_kernel now take
the bit from the stored value; test_keep_bit_of_a_value_that_rounds_to_zero holds all four to it in both types.  An fp16 training
run changes its bits where such elements occur (their gradient is now masked); bf16 runs do not reach 2^-134 in practice.
"""
import ctypes
import functools
import types
import zlib

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests import _bnconv_reference as R
from tests._exact_grid import Out, bits as _bits

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DT_IDS = {BF: "bf16", HF: "fp16"}
F32 = torch.float32
_VP, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
BIG_M = 1 << 22
MKINDS = ["pow2", "ragged", "wrap"]


@functools.lru_cache(maxsize=None)
def _proto(name, res, *args):
    """A private prototype of one library symbol (the shared handle's argtypes are left alone)."""
    return ctypes.CFUNCTYPE(res, *args)((name, C.lib()))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFF


def _rows_of(mkind, tm, cap):
    return {"pow2": 4096, "ragged": 4096 + 37, "wrap": (cap + 1) * tm + 37}[mkind]


def _tile_rows(groups_at_4096):
    assert groups_at_4096 in (32, 64), "4096 rows are 64 tiles of 64 rows or 32 of 128"
    return 4096 // groups_at_4096


def _same_bits(a, b, what):
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), "%s: not the same bits" % what


def _untouched(*outs):
    for o in outs:
        t = o.check("a declined launch")
        assert bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == 0xFF).all()), "a declined launch wrote an output"


# ================================================================ bnload
def _bnload_groups(m, n, k):
    return int(C.lib().dle_conv1x1_bnload_groups(m, n, k))


def _bnload_call(s, w, t=None, m=None, n=None, k=None):
    """One launch into fresh guarded buffers -> (rc, outs).  t / m / n / k override the case's (the declines)."""
    t = s.t if t is None else t
    m, n, k = m or s.m, n or s.n, k or s.k
    dev = t.device
    groups = max(_bnload_groups(m, n, k), 8)
    o = types.SimpleNamespace(y=Out((m, k), s.dtype, dev), bits=Out((m * k // 8,), torch.uint8, dev), out=Out((m, n), s.dtype, dev),
                              part=Out((groups * 2 * n,), F32, dev), groups=groups)
    head = (C.ptr(t), C.ptr(s.res), C.ptr(w), C.ptr(o.out.t), C.ptr(o.y.t), C.ptr(o.bits.t)) + tuple(C.ptr(v) for v in s.bn)
    tail = (C.ptr(o.part.t), o.part.t.numel() * 4, m, n, k, C.dt(t), C.stream())
    if s.resmode == 2:
        fn = _proto("dle_conv1x1_bnload_fwd2", _I, *([_VP] * 15 + [_LL, _I, _I, _I, _I, _VP]))
        rc = fn(*(head + tuple(C.ptr(v) for v in s.bnr) + tail))
    else:
        fn = _proto("dle_conv1x1_bnload_fwd", _I, *([_VP] * 11 + [_LL, _I, _I, _I, _I, _VP]))
        rc = fn(*(head + tail))
    return rc, o


def _bnload_run(s, w, what, stats=True):
    rc, o = _bnload_call(s, w)
    assert rc == 1, "%s: return code %d" % (what, rc)
    got = types.SimpleNamespace(y=o.y.check(what + " y"), bits=o.bits.check(what + " bits"), out=o.out.check(what + " out"))
    part = o.part.check(what + " partial rows")
    if stats:
        dev = s.t.device
        mean, rstd = Out((s.n,), F32, dev), Out((s.n,), F32, dev)
        got.rm, got.rv = s.rm0.clone(), s.rv0.clone()
        ws = Out((32 * 2 * s.n,), F32, dev)
        C.call("dle_bn_stats_from_partials", C.ptr(part), o.groups, s.m, s.n, R.EPS, R.MOM, C.ptr(mean.t), C.ptr(rstd.t), C.ptr(got.rm),
               C.ptr(got.rv), C.ptr(ws.t), ws.t.numel() * 4, C.stream())
        got.mean, got.rstd = mean.check(what + " mean"), rstd.check(what + " rstd")
        ws.check(what + " fold workspace")
        got.S = part.view(o.groups, 2, s.n).double().sum(0)
    return got


def _bnload_case(cuda, dtype, k, n, resmode, mkind):
    tm = _tile_rows(_bnload_groups(4096, n, k))
    cap = _bnload_groups(BIG_M, n, k)
    m = _rows_of(mkind, tm, cap)
    groups = _bnload_groups(m, n, k)
    assert groups > 0, "inside the envelope"
    trips = -(-(-(-m // tm)) // groups)
    assert trips == (2 if mkind == "wrap" else 1)
    chain = trips + 4 + tm // 16 + 1
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnload_inputs(kind, dtype, cuda, m, k, n, resmode, _seed("bnload", kind, k, n, resmode, mkind))
        what = "bnload %s M=%d N=%d K=%d res%d %s" % (kind, m, n, k, resmode, DT_IDS[dtype])
        got = _bnload_run(s, s.w, what)
        R.bnload_check(s, got, chain, what, worst)
        again = _bnload_run(s, s.w, what + " (second launch)")
        for name in ("y", "bits", "out", "mean", "rstd", "rm", "rv"):
            _same_bits(getattr(again, name), getattr(got, name), what + " second launch " + name)
        rm, rv = s.rm0.clone(), s.rv0.clone()
        wrapped = F.conv1x1_bnload_fwd(s.t, s.res, s.w.view(n, 1, 1, k), *s.bn, running_mean=rm, running_var=rv, eps=R.EPS,
                                       momentum=R.MOM, res_bn=s.bnr)
        assert wrapped is not None, what + ": the wrapper declined"
        for a, b, name in zip(wrapped + (rm, rv), (got.out, got.y, got.bits, got.mean, got.rstd, got.rm, got.rv),
                              ("out", "y", "bits", "mean", "rstd", "running_mean", "running_var")):
            _same_bits(a, b, what + " wrapper " + name)
        if kind == "exact":
            R.bnload_check(s, _bnload_run(s, s.w_dense, what + " dense w", stats=False), chain, what, worst, dense=True)
    print("bnload M=%d N=%d K=%d res%d %s: worst |error| / bar: %s" % (m, n, k, resmode, DT_IDS[dtype], worst))


BNLOAD_KN = [(64, 64), (64, 256), (128, 128), (128, 256), (256, 64), (256, 128), (256, 256)]
BNLOAD_CASES = [(k, n, r, mk, dt) for k, n in BNLOAD_KN for r in (0, 1, 2) for mk in MKINDS for dt in (BF, HF)]


@pytest.mark.parametrize("k, n, resmode, mkind, dtype", BNLOAD_CASES,
                         ids=["k%d-n%d-res%d-%s-%s" % (k, n, r, mk, DT_IDS[dt]) for k, n, r, mk, dt in BNLOAD_CASES])
def test_bnload(cuda, k, n, resmode, mkind, dtype):
    """Both tile widths (N = 64: 64 columns, else 128), 4 and 8 wavefronts (K = 256 with 128-column tiles), one and two column
    tiles, the three residual modes."""
    _bnload_case(cuda, dtype, k, n, resmode, mkind)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mkind", MKINDS)
def test_bnload_k512(cuda, mkind, dtype, monkeypatch):
    """K = 512 x N = 128 with the residual tensor: the opt-in instantiation (one 8-wave workgroup per CU)."""
    assert _bnload_groups(4096, 128, 512) == 0, "off by default"
    monkeypatch.setenv("DLE_CONV_BNLOAD_K512", "1")
    _bnload_case(cuda, dtype, 512, 128, 1, mkind)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_keep_bit_of_a_value_that_rounds_to_zero(cuda, dtype):
    """The keep bits are those of the STORED y.  t = the smallest positive 16-bit value (fp16 2^-24, bf16 2^-133) with sc = 1/4
    gives an fp32 value > 0 a quarter of that, which rounds to a 16-bit zero: the bit must be 0, as a backward pass that reads
    y > 0 from the stored activation would have it.  (Found in fp16 by test_bnload[k256-n64-res0-wrap-fp16]: one element of 12.6
    million with 0 < fp32 value <= 2^-25 had y = 0 and its bit set; the fused kernel and the three stand-alone apply kernels took the
    bit from the fp32 value.)"""
    m, k, n = 4096, 64, 64
    tiny = torch.rand((m, k), generator=R.gen(cuda, 1), device=cuda) < 0.5
    least = torch.ones((), dtype=torch.int16, device=cuda).view(dtype)            # bit pattern 0x0001
    assert float(least) == (2.0 ** -24 if dtype == HF else 2.0 ** -133)
    t = torch.where(tiny, least, torch.ones((), dtype=dtype, device=cuda))
    zero, one = torch.zeros(k, device=cuda), torch.ones(k, device=cuda)
    bn = (zero, one * 0.25, one, zero)
    want_y = torch.where(tiny, torch.zeros((), device=cuda), torch.full((), 0.25, device=cuda)).to(dtype)
    want_bits = R.pack_bits(~tiny)
    s = types.SimpleNamespace(t=t, res=None, bn=bn, bnr=None, resmode=0, dtype=dtype, m=m, n=n, k=k)
    rc, o = _bnload_call(s, torch.zeros((n, k), dtype=dtype, device=cuda))
    assert rc == 1
    assert torch.equal(o.y.check("y"), want_y) and torch.equal(o.bits.check("bits"), want_bits), "conv_bnload_kernel"
    y, bits = F.bn_fwd_apply(t, *bn, relu=True, want_mask=True)
    assert torch.equal(y, want_y) and torch.equal(bits, want_bits), "bn_apply_pf_kernel"
    y, bits = F.bn_fwd_apply(t, *bn, residual=torch.zeros_like(t), relu=True, want_mask=True, residual_bn=(zero, one, one, zero))
    assert torch.equal(y, want_y) and torch.equal(bits, want_bits), "bn_apply2_pf_kernel"
    _, _, bits = F.bn_relu_maxpool_fwd(t.view(4, 32, 32, k), *bn)
    assert torch.equal(bits, want_bits), "bn_relu_maxpool_k3s2_kernel"


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_bnload_declines(cuda, dtype):
    """Outside the envelope: return code 0 / None, nothing written."""
    s = R.bnload_inputs("gauss", dtype, cuda, 4096, 256, 1024, 0, 5)
    v = torch.ones(256, device=cuda)
    for what, m, n in (("N = 192", 4096, 192), ("N = 1024 at K = 256", 4096, 1024), ("M = 4095", 4095, 256)):
        assert _bnload_groups(m, n, 256) == 0, what
        rc, o = _bnload_call(s, s.w, m=m, n=n)
        assert rc == 0, "%s: return code %d" % (what, rc)
        _untouched(o.y, o.bits, o.out, o.part)
        assert F.conv1x1_bnload_fwd(s.t[:m], None, s.w[:n].view(n, 1, 1, 256), v, v, v, v) is None, what
    shifted = torch.zeros(4096 * 256 + 8, dtype=dtype, device=cuda)[4:4 + 4096 * 256].view(4096, 256)          # 8 bytes off the 16-byte grid
    assert shifted.data_ptr() % 16 == 8
    rc, o = _bnload_call(s, s.w, t=shifted, n=256)
    assert rc == 0, "misaligned t: return code %d" % rc
    _untouched(o.y, o.bits, o.out, o.part)
    assert F.conv1x1_bnload_fwd(shifted, None, s.w[:256].view(256, 1, 1, 256), v, v, v, v) is None


# ================================================================ bnbwd
def _bnbwd_call(s, wg, m=None, k=R.BK, short=0):
    """One launch of the plain (dt written) or weight-gradient form into fresh guarded buffers -> (rc, outs)."""
    m = m or s.m
    dev = s.t.device
    lib = C.lib()
    g768 = int(lib.dle_conv1x1_bnbwd_groups(m))
    o = types.SimpleNamespace(dx=Out((m, R.BN), s.dtype, dev), part=Out((g768 * 2 * R.BN,), F32, dev), groups=g768, dt=None, gw=None, ws=None)
    red = (C.ptr(s.t2), C.ptr(s.bits2), C.ptr(s.mean2), C.ptr(s.rstd2), C.ptr(o.part.t) if s.bred else 0,
           o.part.t.numel() * 4 if s.bred else 0)
    coef = tuple(C.ptr(v) for v in (s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta))
    tail = (m, R.BN, k, C.dt(s.t), C.stream())
    if wg:
        nbytes = int(lib.dle_conv1x1_bnbwd_wgrad_workspace(m, int(s.bred)))
        o.gw, o.ws = Out((R.BK, R.BN), F32, dev), Out((nbytes // 4,), F32, dev)
        fn = _proto("dle_conv1x1_bnbwd_dgrad_wgrad", _I, *([_VP] * 15 + [_LL, _VP, _VP, _VP, _LL, _I, _I, _I, _I, _VP]))
        rc = fn(C.ptr(s.dy), C.ptr(s.t), C.ptr(s.bits), C.ptr(s.w), C.ptr(o.dx.t), *(coef + red + (C.ptr(s.x), C.ptr(o.gw.t),
                C.ptr(o.ws.t), nbytes - short) + tail))
    else:
        o.dt = Out((m, R.BK), s.dtype, dev)
        fn = _proto("dle_conv1x1_bnbwd_dgrad", _I, *([_VP] * 16 + [_LL, _I, _I, _I, _I, _VP]))
        rc = fn(C.ptr(s.dy), C.ptr(s.t), C.ptr(s.bits), C.ptr(s.w), C.ptr(o.dt.t), C.ptr(o.dx.t), *(coef + red + tail))
    return rc, o


def _bnbwd_run(s, wg, what):
    rc, o = _bnbwd_call(s, wg)
    assert rc == 1, "%s: return code %d" % (what, rc)
    got = types.SimpleNamespace(dx=o.dx.check(what + " dx"), dt=None, gw=None)
    part = o.part.check(what + " partial rows")
    if wg:
        got.gw = o.gw.check(what + " gw")
        o.ws.check(what + " workspace")
    else:
        got.dt = o.dt.check(what + " dt")
    if s.bred:
        dg2, db2 = Out((R.BN,), F32, s.t.device), Out((R.BN,), F32, s.t.device)
        C.call("dle_bn_bwd_finish", C.ptr(part), o.groups, R.BN, C.ptr(dg2.t), C.ptr(db2.t), 0, C.stream())
        got.dg2, got.db2 = dg2.check(what + " dgamma2"), db2.check(what + " dbeta2")
    else:
        assert bool(torch.isnan(part).all()), what + ": partial rows written without bnred"
    return got


BNBWD_CASES = [(mk, masked, bred, wg, dt) for mk in MKINDS for masked in (True, False) for bred in (True, False) for wg in (False, True)
               for dt in (BF, HF)]


@pytest.mark.parametrize("mkind, masked, bred, wg, dtype", BNBWD_CASES,
                         ids=["%s-%s-%s-%s-%s" % (mk, "mask" if ma else "nomask", "bnred" if br else "nobnred", "wgrad" if wg else "plain",
                                                  DT_IDS[dt]) for mk, ma, br, wg, dt in BNBWD_CASES])
def test_bnbwd(cuda, mkind, masked, bred, wg, dtype):
    """K = 256, N = 64: mask on / off, bnred on / off, dt written (plain) or the weight gradient formed in the kernel (dt never
    written).  The plain form runs 768 groups, the weight-gradient form 512 (its bnred chain fold still runs over 768)."""
    lib = C.lib()
    tm = _tile_rows(int(lib.dle_conv1x1_bnbwd_groups(4096)))
    cap768 = int(lib.dle_conv1x1_bnbwd_groups(BIG_M))
    cap512 = int(lib.dle_conv1x1_bnbwd_wgrad_workspace(BIG_M, 0)) // (R.BK * R.BN * 4)
    assert (tm, cap768, cap512) == (64, 768, 512)
    m = _rows_of(mkind, tm, cap512 if wg else cap768)
    tiles = -(-m // tm)
    g768 = int(lib.dle_conv1x1_bnbwd_groups(m))
    g512 = int(lib.dle_conv1x1_bnbwd_wgrad_workspace(m, 0)) // (R.BK * R.BN * 4)
    assert -(-tiles // (g512 if wg else g768)) == (2 if mkind == "wrap" else 1)
    chains = {"bnred": -(-tiles // g768) + 4 + tm // 16 + 1, "gw": -(-tiles // g512) * tm + -(-g512 // 16) + 16}
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnbwd_inputs(kind, dtype, cuda, m, masked, bred, _seed("bnbwd", kind, mkind, masked, bred))
        what = "bnbwd %s M=%d %s%s%s %s" % (kind, m, "mask " if masked else "", "bnred " if bred else "", "wgrad" if wg else "plain",
                                           DT_IDS[dtype])
        got = _bnbwd_run(s, wg, what)
        R.bnbwd_check(s, got, chains, what, worst)
        again = _bnbwd_run(s, wg, what + " (second launch)")
        names = ["dx", "gw" if wg else "dt"] + (["dg2", "db2"] if bred else [])
        for name in names:
            _same_bits(getattr(again, name), getattr(got, name), what + " second launch " + name)
        dg2, db2 = torch.full((R.BN,), 9.0, device=cuda), torch.full((R.BN,), 9.0, device=cuda)
        bn2 = (s.t2, s.bits2, s.mean2, s.rstd2, dg2, db2) if bred else None
        if wg:
            gw = torch.full((R.BK, R.BN), 7.0, device=cuda)
            wrapped = F.bn_bwd_conv1x1_dgrad_wgrad(s.dy, s.t, s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta, s.w, s.x, gw, relu_mask=s.bits,
                                                   reduce_done=True, bnred=bn2)
            assert wrapped is not None and wrapped[1] == bred, what + ": the wrapper"
            pairs = [(wrapped[0], got.dx, "dx"), (gw, got.gw, "gw")]
        else:
            wrapped = F.bn_bwd_conv1x1_dgrad(s.dy, s.t, s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta, s.w, relu_mask=s.bits,
                                             reduce_done=True, bnred=bn2)
            assert wrapped is not None and wrapped[2] == bred, what + ": the wrapper"
            pairs = [(wrapped[0], got.dt, "dt"), (wrapped[1], got.dx, "dx")]
        if bred:
            pairs += [(dg2, got.dg2, "dgamma2"), (db2, got.db2, "dbeta2")]
        for a, b, name in pairs:
            _same_bits(a, b, what + " wrapper " + name)
    print("bnbwd M=%d mask%d bnred%d %s %s: worst |error| / bar: %s" % (m, masked, bred, "wgrad" if wg else "plain", DT_IDS[dtype], worst))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_bnbwd_declines(cuda, dtype):
    s = R.bnbwd_inputs("gauss", dtype, cuda, 4096, True, True, 9)
    for wg in (False, True):
        for what, kw in (("M = 4095", dict(m=4095)), ("K = 128", dict(k=128))):
            rc, o = _bnbwd_call(s, wg, **kw)
            assert rc == 0, "%s: return code %d" % (what, rc)
            _untouched(*[b for b in (o.dx, o.dt, o.gw, o.ws, o.part) if b is not None])
    rc, o = _bnbwd_call(s, True, short=1)
    assert rc == 0, "a workspace one byte short: return code %d" % rc
    _untouched(o.dx, o.gw, o.ws, o.part)
    gw = torch.empty((R.BK, R.BN), device=cuda)
    assert F.bn_bwd_conv1x1_dgrad(s.dy[:4095], s.t[:4095], s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta, s.w) is None
    assert F.bn_bwd_conv1x1_dgrad_wgrad(s.dy[:4095], s.t[:4095], s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta, s.w, s.x[:4095], gw) is None
    half = slice(0, 128)
    assert F.bn_bwd_conv1x1_dgrad(s.dy[:, half].contiguous(), s.t[:, half].contiguous(), s.mean[half], s.rstd[half], s.gamma[half],
                                  s.dgamma[half], s.dbeta[half], s.w[half].contiguous()) is None


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_standalone_bn_bwd_per_element(cuda, masked, dtype):
    """F.bn_bwd's apply pass (bn_bwd_apply_pf_kernel), which the fused kernel claims to equal bit for bit, under the SAME per-element
    dt bar, at a ragged (M, C) = (4096 + 37, 72): the global 1.5-step bar of test_gpu_bn_reference.py lets an element a thousand
    times smaller than the largest be wrong in every bit."""
    m, c = 4096 + 37, 72
    g = R.gen(cuda, 21 + masked)
    s = types.SimpleNamespace(kind="gauss", dtype=dtype, m=m, masked=masked, keep=None)
    s.t = (torch.randn((m, c), generator=g, device=cuda) * 1.5 + 0.3).to(dtype)
    s.dy = (torch.randn((m, c), generator=g, device=cuda) * 0.01).to(dtype)
    mask = None
    if masked:
        s.keep = torch.rand((m, c), generator=g, device=cuda) < 0.6
        mask = R.pack_bits(s.keep)
    s.gamma = torch.rand(c, generator=g, device=cuda) + 0.5
    td = s.t.double()
    s.mean, s.rstd = td.mean(0).float(), (1.0 / torch.sqrt(td.var(0, unbiased=False) + R.EPS64)).float()
    gd = s.dy.double() * (s.keep if masked else 1.0)
    s.dbeta, s.dgamma = gd.sum(0).float(), (gd * (td - s.mean.double()) * s.rstd.double()).sum(0).float()
    s.exact_ch = torch.zeros(c, dtype=torch.bool, device=cuda)
    dx = Out((m, c), dtype, cuda)
    F.bn_bwd(s.dy, None, s.t, s.mean, s.rstd, s.gamma, s.dgamma, s.dbeta, dx_out=dx.t, relu_mask=mask, reduce_done=True)
    worst = R.Worst()
    R.check_dt(s, dx.check("bn_bwd dx"), "bn_bwd M=%d C=%d" % (m, c), worst, name="dt (bn_bwd)")
    print("bn_bwd M=%d C=%d %s: worst |error| / bar: %s" % (m, c, DT_IDS[dtype], worst))


# ================================================================ bnred GEMM
def _bnred_groups(m, n, k):
    return int(C.lib().dle_gemm_expand_groups(m, n, k))


def _bnred_call(s, n=None):
    n = n or s.n
    dev = s.a.device
    groups = _bnred_groups(s.m, n, s.k)
    o = types.SimpleNamespace(dx=Out((s.m, n), s.dtype, dev), part=Out((groups * 2 * n,), F32, dev), groups=groups)
    fn = _proto("dle_gemm_expand_masked_bnred", _I, *([_VP] * 10 + [_LL, _I, _I, _I, _LL, _LL, _LL, _I, _I, _VP]))
    rc = fn(C.ptr(s.a), C.ptr(s.w), C.ptr(o.dx.t), C.ptr(s.addend), C.ptr(s.bits1), C.ptr(s.t2), C.ptr(s.bits2), C.ptr(s.mean2),
            C.ptr(s.rstd2), C.ptr(o.part.t), o.part.t.numel() * 4, s.m, n, s.k, s.k, s.w.stride(0), n, 0, C.dt(s.a), C.stream())
    return rc, o


def _bnred_run(s, what):
    rc, o = _bnred_call(s)
    assert rc == 1, "%s: return code %d" % (what, rc)
    got = types.SimpleNamespace(dx=o.dx.check(what + " dx"))
    part = o.part.check(what + " partial rows")
    dg2, db2 = Out((s.n,), F32, s.a.device), Out((s.n,), F32, s.a.device)
    C.call("dle_bn_bwd_finish", C.ptr(part), o.groups, s.n, C.ptr(dg2.t), C.ptr(db2.t), 0, C.stream())
    got.dg2, got.db2 = dg2.check(what + " dgamma2"), db2.check(what + " dbeta2")
    return got


BNRED_KN = [(64, 128), (64, 256), (128, 256), (128, 512), (256, 512)]
BNRED_CASES = [(k, n, mk, dt) for k, n in BNRED_KN for mk in MKINDS for dt in (BF, HF)]


@pytest.mark.parametrize("k, n, mkind, dtype", BNRED_CASES, ids=["k%d-n%d-%s-%s" % (k, n, mk, DT_IDS[dt]) for k, n, mk, dt in BNRED_CASES])
def test_bnred_gemm(cuda, k, n, mkind, dtype, monkeypatch):
    """dx = a W + addend under keep bits (ACT_ADD_MASKED as tests/test_gpu_gemm_reference.py states it) with the next BatchNorm's
    backward reduction in the epilogue.  K = 256 is the opt-in 8-wave instantiation."""
    if k == 256:
        monkeypatch.setenv("DLE_GEMM_BNRED_K256", "1")
    tm = _tile_rows(_bnred_groups(4096, n, k))
    m = _rows_of(mkind, tm, _bnred_groups(BIG_M, n, k))
    trips = -(-(-(-m // tm)) // _bnred_groups(m, n, k))
    assert trips == (2 if mkind == "wrap" else 1)
    chain = trips + 4 + tm // 16 + 1
    worst = R.Worst()
    for kind in ("exact", "gauss"):
        s = R.bnred_inputs(kind, dtype, cuda, m, k, n, _seed("bnred", kind, k, n, mkind))
        what = "bnred %s M=%d N=%d K=%d %s" % (kind, m, n, k, DT_IDS[dtype])
        got = _bnred_run(s, what)
        R.bnred_check(s, got, chain, what, worst)
        again = _bnred_run(s, what + " (second launch)")
        dg2, db2 = torch.full((n,), 5.0, device=cuda), torch.full((n,), 5.0, device=cuda)
        dx = F.gemm_masked_add_bnred(s.a, s.w, m, n, k, s.addend, s.bits1, s.t2, s.bits2, s.mean2, s.rstd2, dg2, db2)
        assert dx is not None, what + ": the wrapper declined"
        for name, w_ in (("dx", dx), ("dg2", dg2), ("db2", db2)):
            _same_bits(getattr(again, name), getattr(got, name), what + " second launch " + name)
            _same_bits(w_, getattr(got, name), what + " wrapper " + name)
    print("bnred M=%d N=%d K=%d %s: worst |error| / bar: %s" % (m, n, k, DT_IDS[dtype], worst))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_bnred_gemm_declines(cuda, dtype):
    """N < 2 K: return code 0 / None, nothing written; K = 256 without its switch likewise."""
    s = R.bnred_inputs("gauss", dtype, cuda, 4096, 128, 256, 3)
    rc, o = _bnred_call(s, n=128)
    assert rc == 0, "N < 2 K: return code %d" % rc
    _untouched(o.dx, o.part)
    v = torch.zeros(128, device=cuda)
    assert F.gemm_masked_add_bnred(s.a, s.w[:, :128].contiguous(), 4096, 128, 128, s.addend[:, :128].contiguous(), s.bits1[:4096 * 16],
                                   s.t2[:, :128].contiguous(), s.bits2[:4096 * 16], v, v + 1, v.clone(), v.clone()) is None
    s = R.bnred_inputs("gauss", dtype, cuda, 4096, 256, 512, 4)
    rc, o = _bnred_call(s)
    assert rc == 0, "K = 256 is opt-in: return code %d" % rc
    _untouched(o.dx, o.part)
