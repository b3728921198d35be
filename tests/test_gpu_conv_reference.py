"""The ResNet-50 convolution kernels (forward, data gradient, weight gradient) against a float64 restatement of the convolution, at
the batch-256 sizes the step runs, over the WHOLE output tensor.  GPU only.

Reference.  torch float64 on the GPU, written as a sum of per-tap matrix products over padded, strided slices of the activation
(no torch.nn.functional.conv2d, nothing of this library):

    y[n, p, q, :]          = sum_(r, s)  xpad[n, p stride + r, q stride + s, :] @ w[:, r, s, :]^T
    dxpad[n, p stride + r, q stride + s, :] += dy[n, p, q, :] @ w[:, r, s, :]          (the gather of dx written as its scatter)
    dw[:, r, s, :]         = sum_(n, p, q)  dy[n, p, q, :]^T xpad[n, p stride + r, q stride + s, :]

Exactly summable inputs.  Activations, gradients and weights are k / 4 with small integer k (tests/_exact_grid.py): exact in fp16
and bf16, every product a multiple of 1/16.  When the sum of the magnitudes of the terms of an output stays below B, every partial
sum of that output, in any order and any grouping, is a multiple of 1/16 below B: exact in fp32.  That covers MFMA chains, split-K
slabs, per-workgroup partial blocks and their folds alike.  B = 2^18 (not the 2^20 of the plain fp32 additions of the BatchNorm
tests): headroom for a matrix unit that aligns a group of products to the largest exponent before it adds them.  The bound is
asserted from the data before any comparison:
* forward and data gradient: K max|a| max|b| (+ max|addend|) with K = R S C (forward) or R S Ko (data gradient) <= 4608 and
  |k| <= 4: at most 4608 + 1, far below B;
* weight gradients sum over N P Q pixels (802,816 at 56 x 56, 3.2 M for the stem): |k| <= 2, and about half zeros for the stem's
  dy; the bound is the float64 reference of |dy| and |x| (plus |dw0| when accumulating), checked element by element.
So:
* fp32 outputs (weight gradients, accumulate=True included, on top of a prior dw0 on the 1/16 grid) equal the float64 reference
  BIT FOR BIT;
* 16-bit outputs (forward, data gradients, + addend) are the exact fp32 sum rounded once to 16 bits by the RNE hardware convert:
  they equal ref64.float().to(dtype) BIT FOR BIT (float64 -> float32 is exact here, torch's float32 -> 16-bit is RNE).
A dropped or repeated tile, channel chunk, tap, K slice, parity class, partial block or pixel then fails at once.

Which kernel ran.  The halo-tile kernels and the streaming 1x1 weight gradient have `_try` entry points that return 1 when they took
the launch and 0 when the shape is outside their envelope.  The tests call them through the C ABI, assert the return code, and
then assert that the public wrapper gives the same bits.  Each such case runs again with the kernel pinned off
(dle_conv3x3_mode(0), dle_conv3x3_wgrad_mode(0), dle_wgrad1x1_mode(0), restored in `finally`): the tile / split-K fallbacks must
be exact at the same batch-256 sizes.  The DLE_* environment switches are read once per process; the mode calls are not.

Envelopes (from the LDS checks of the `_try` functions):
* halo forward / data gradient (csrc/conv3x3.hip): LDS = 1 KiB x ceil((256 + 2 (W + 2) + 2) / 8) patch pieces + 2 NT x 64 x 2
  bytes of weights <= 80 KiB, NT = 128 when the output channels (Ko forward, C data gradient) are a multiple of 128, else 64:
  W <= 61 for NT = 128 and W <= 125 for NT = 64 (W = 62 / 126 decline).  The forward also declines H W < 100 (7 x 7);
* halo weight gradient (csrc/conv3x3_wgrad.hip): at most 32 patch pieces of (128 + 2 (W + 2) + 2) slots: W <= 61 (62 declines);
* wgrad1x1 (csrc/wgrad1x1.hip): seven (Ko, C) configurations, M >= 8192 (8191 declines).
Ragged cases use a prime N with odd H and W, so that the last 256-slot (halo) or 128-slot (halo weight gradient) pixel tile is
partial, H = 1, and for wgrad1x1 M = 8192 (fewer tiles than workgroups) and M = 200,704 + 37 (a partial last row tile).

Every case runs in bf16 and in fp16.

No stray writes.  Outputs are views at the head of over-long buffers filled with NaN; the tail must keep its bits, and a NaN left
inside the output fails the comparison.

Realistic inputs (test_gaussian): x ~ N(0, 1), w ~ N(0, 1 / K), dy ~ N(0, 1 / 4), rounded to the 16-bit type; the reference
runs on the rounded values.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham), an fp32 sum of products along chains of at most
n additions errs by at most gamma_n sum |a b| (the float64 reference of |a| and |b|):
* 16-bit outputs: |got - ref| <= ulp16(max(|got|, |ref|)) / 2 + gamma_K sum |a b|, K = R S C or R S Ko (one rounding of a sum
  whose chains are at most K terms long);
* fp32 weight gradients: |got - ref| <= gamma_n sum |a b|, where n counts the longest chain the kernel's structure implies
  (each MFMA step counted as one addition per product):
    wgrad1x1:      ceil(ceil(M / TG) / WG) TG / PH rows per wave + PH - 1 (pixel-half meeting) + WG + 16 (fold of WG partial blocks:
                   a chain over the group slices, then 16 slices);
    halo wgrad:    ceil(tiles / (256 / nsub)) x 64 slots per pixel half + 1 (meeting) + 256 / nsub + 16 (fold);
    split-K GEMM:  ceil(K tiles / splitk) x 64 + splitk + 16 (the slab fold);
    stem wgrad:    ceil(N P / 512) x 128 dy slots + 512 + 8 (fold of 512 partials in four chains, then 4).
"""
import contextlib
import ctypes
import functools
import zlib

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd import functional as F
from tests._exact_grid import B_MFMA, Out as _Out, assert_same as _assert_same, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DT_IDS = {BF: "bf16", HF: "fp16"}
U = 2.0 ** -24
F64 = torch.float64


# ---------------------------------------------------------------- float64 reference
def _out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def _win(t, i, j, stride, p, q):
    """[N, P, Q, C] view of the padded tensor t read by tap (i, j)."""
    return t[:, i:i + stride * (p - 1) + 1:stride, j:j + stride * (q - 1) + 1:stride, :]


def ref_fwd(x, w, stride, pad):
    """y [N, P, Q, Ko] of x [N, H, W, C], w [Ko, R, S, C], float64."""
    x, w = x.to(F64), w.to(F64)
    n, h, wd, c = x.shape
    ko, r, s, _ = w.shape
    p, q = _out_hw(h, wd, r, s, stride, pad)
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros((n * p * q, ko), dtype=F64, device=x.device)
    for i in range(r):
        for j in range(s):
            y.addmm_(_win(xp, i, j, stride, p, q).reshape(-1, c), w[:, i, j, :].t())
    return y.view(n, p, q, ko)


def ref_dgrad(dy, w, hw, stride, pad):
    """dx [N, H, W, C] of dy [N, P, Q, Ko], w [Ko, R, S, C], float64."""
    dy, w = dy.to(F64), w.to(F64)
    n, p, q, ko = dy.shape
    _, r, s, c = w.shape
    h, wd = hw
    dxp = torch.zeros((n, h + 2 * pad, wd + 2 * pad, c), dtype=F64, device=dy.device)
    d2 = dy.reshape(-1, ko)
    for i in range(r):
        for j in range(s):
            _win(dxp, i, j, stride, p, q).add_((d2 @ w[:, i, j, :]).view(n, p, q, c))
    return dxp[:, pad:pad + h, pad:pad + wd, :]


def _tn(a, b, chunk=8192):
    """a [M, A]^T b [M, B] in float64, as a batch of row chunks (a long contraction with a small output)."""
    a, b = a.to(F64), b.to(F64)
    extra = -a.shape[0] % chunk
    if extra:
        a = torch.nn.functional.pad(a, (0, 0, 0, extra))
        b = torch.nn.functional.pad(b, (0, 0, 0, extra))
    k = a.shape[0] // chunk
    return torch.bmm(a.reshape(k, chunk, -1).transpose(1, 2), b.reshape(k, chunk, -1)).sum(0)


def ref_wgrad(dy, x, r, s, stride, pad):
    """dw [Ko, R, S, C] of dy [N, P, Q, Ko], x [N, H, W, C], float64."""
    dy, x = dy.to(F64), x.to(F64)
    n, p, q, ko = dy.shape
    c = x.shape[3]
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    d2 = dy.reshape(-1, ko)
    dw = torch.empty((ko, r, s, c), dtype=F64, device=x.device)
    for i in range(r):
        for j in range(s):
            dw[:, i, j, :] = _tn(d2, _win(xp, i, j, stride, p, q).reshape(-1, c))
    return dw


def _stuffed(compact, hw):
    """[N, H, W, C] with compact [N, H/2, W/2, C] at the even pixels, zero elsewhere."""
    n, p, q, c = compact.shape
    out = torch.zeros((n, hw[0], hw[1], c), dtype=compact.dtype, device=compact.device)
    out[:, ::2, ::2, :] = compact
    return out


# ---------------------------------------------------------------- preconditions and comparisons
def _on_grid(*ts):
    for t in ts:
        t4 = t.to(F64) * 4
        assert torch.equal(t4, torch.round(t4)), "input off the 1/4 grid"


def _summable_16(k, a, b, addend=None):
    """Forward / data gradient: each output sums k products |a b| <= max|a| max|b| (+ one addend)."""
    _on_grid(a, b)
    bound = k * float(a.abs().max()) * float(b.abs().max())
    if addend is not None:
        _on_grid(addend)
        bound += float(addend.abs().max())
    assert bound < B_MFMA, "sum of magnitudes up to %g: fp32 sums would not be exact" % bound


def _summable_32(absref, *inputs, dw0=None):
    """Weight gradients: the float64 sum of |dy| |x| of every element (+ |dw0|) is below B_MFMA."""
    _on_grid(*inputs)
    worst = absref if dw0 is None else absref + dw0.to(F64).abs()
    worst = float(worst.max())
    assert worst < B_MFMA, "sum of magnitudes up to %g: fp32 sums would not be exact" % worst
    if dw0 is not None:
        _on_grid(dw0)


# ---------------------------------------------------------------- C ABI entry points that may decline
_VP, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


@functools.lru_cache(maxsize=None)
def _proto(name, res, *args):
    """A private prototype of one library symbol (the shared handle's argtypes are left alone)."""
    return ctypes.CFUNCTYPE(res, *args)((name, C.lib()))


def _conv3x3_try(x, w, y, n, h, wd, c, ko, dgrad):
    fn = _proto("dle_conv3x3_try", _I, _VP, _VP, _VP, _VP, _LL, _I, _I, _I, _I, _I, _I, _I, _VP)
    return fn(C.ptr(x), C.ptr(w), C.ptr(y), None, 0, n, h, wd, c, ko, dgrad, C.dt(x), C.stream())


def _conv3x3_wgrad_try(dy, x, dw, accumulate):
    n, h, wd, c = x.shape
    ko = dy.shape[3]
    ws = F.splitk_workspace(x.device, int(C.lib().dle_conv3x3_wgrad_workspace()))
    fn = _proto("dle_conv3x3_wgrad_try", _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _I, _VP, _LL, _VP)
    return fn(C.ptr(dy), C.ptr(x), C.ptr(dw), n, h, wd, c, ko, C.dt(x), int(accumulate), C.ptr(ws), ws.numel() * 4, C.stream())


def _wgrad1x1_try(dy2d, x2d, dw, accumulate):
    m, ko = dy2d.shape
    c = x2d.shape[1]
    need = int(C.lib().dle_wgrad1x1_workspace_for(m, ko, c))
    ws = F.splitk_workspace(dy2d.device, need) if need else None
    fn = _proto("dle_wgrad1x1_try", _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _LL, _VP)
    return fn(C.ptr(dy2d), C.ptr(x2d), C.ptr(dw), m, ko, c, C.dt(dy2d), int(accumulate), C.ptr(ws),
              ws.numel() * 4 if ws is not None else 0, C.stream())


@contextlib.contextmanager
def _pinned_off(mode_fn):
    setter = _proto(mode_fn, _I, _I)
    old = setter(0)
    try:
        yield
    finally:
        setter(old)


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def _ids(cases, fmt):
    return [fmt(*c) for c in cases]


# ================================================================ forward
# halo-tile kernel: (x [N, H, W, C], Ko)
HALO_FWD = [((256, 56, 56, 64), 64), ((256, 28, 28, 128), 128), ((256, 14, 14, 256), 256)]
HALO_DGRAD = [((256, 56, 56, 64), 64), ((256, 28, 28, 128), 128), ((256, 14, 14, 256), 256), ((256, 7, 7, 512), 512)]
# envelope edges: prime N with odd H, W (partial last 256-slot tile), H = 1, the widest W and one past it
HALO_EDGES = [("fwd", (13, 27, 29, 64), 128, 1), ("fwd", (211, 1, 121, 64), 64, 1), ("fwd", (7, 9, 61, 64), 128, 1),
              ("fwd", (7, 9, 62, 64), 128, 0), ("fwd", (5, 3, 125, 128), 64, 1), ("fwd", (5, 3, 126, 128), 64, 0),
              ("fwd", (256, 7, 7, 512), 512, 0),                    # H W < 100: the forward leaves 7 x 7 to the im2col tile kernel
              ("dgrad", (13, 27, 29, 128), 64, 1), ("dgrad", (211, 1, 121, 64), 128, 1), ("dgrad", (7, 9, 61, 128), 64, 1),
              ("dgrad", (7, 9, 62, 128), 64, 0), ("dgrad", (5, 3, 125, 64), 128, 1), ("dgrad", (5, 3, 126, 64), 128, 0)]
HALO_CASES = [c + (dt,) for c in [("fwd", xs, ko, 1) for xs, ko in HALO_FWD] + [("dgrad", xs, ko, 1) for xs, ko in HALO_DGRAD] +
              HALO_EDGES for dt in (BF, HF)]


@pytest.mark.parametrize("direction, xs, ko, rc, dtype", HALO_CASES,
                         ids=_ids(HALO_CASES, lambda d, xs, ko, rc, dt: "%s-%s-k%d-%s" % (d, "x".join(map(str, xs)), ko, DT_IDS[dt])))
def test_halo_3x3(cuda, direction, xs, ko, rc, dtype):
    """3 x 3 / stride 1 / pad 1 forward and data gradient: the halo-tile kernel (rc == 1) or its decline (rc == 0), the wrapper,
    and the im2col tile kernel with the halo kernel pinned off."""
    n, h, wd, c = xs
    dgrad = direction == "dgrad"
    w = grid((ko, 3, 3, c), _seed("w", xs, ko), dtype, cuda)
    if dgrad:
        src = grid((n, h, wd, ko), _seed("dy", xs, ko), dtype, cuda)
        _summable_16(9 * ko, src, w)
        want = ref_dgrad(src, w, (h, wd), 1, 1).float().to(dtype)
        run = lambda out: F.conv2d_dgrad(src, w, (h, wd), 1, 1, out=out)
    else:
        src = grid(xs, _seed("x", xs, ko), dtype, cuda)
        _summable_16(9 * c, src, w)
        want = ref_fwd(src, w, 1, 1).float().to(dtype)
        run = lambda out: F.conv2d_fwd(src, w, 1, 1, out=out)
    what = "%s %s k%d" % (direction, xs, ko)
    o1 = _Out(want.shape, dtype, cuda)
    assert _conv3x3_try(src, w, o1.t, n, h, wd, c, ko, int(dgrad)) == rc, "%s: dle_conv3x3_try" % what
    if rc == 1:
        _assert_same(o1.check("conv3x3 " + what), want, "halo " + what)
    o2 = _Out(want.shape, dtype, cuda)
    run(o2.t)
    _assert_same(o2.check(what), want, "wrapper " + what)
    with _pinned_off("dle_conv3x3_mode"):
        assert _conv3x3_try(src, w, o1.t, n, h, wd, c, ko, int(dgrad)) == 0, "%s: mode 0 must decline" % what
        o3 = _Out(want.shape, dtype, cuda)
        run(o3.t)
        _assert_same(o3.check(what), want, "tile kernel (halo pinned off) " + what)


# im2col tile kernel of gemm_dma.hip: (x [N, H, W, C], Ko, R, stride, pad)
TILE_FWD = [((256, 56, 56, 128), 128, 3, 2, 1), ((256, 28, 28, 256), 256, 3, 2, 1), ((256, 14, 14, 512), 512, 3, 2, 1),
            ((256, 56, 56, 256), 512, 1, 2, 0), ((256, 28, 28, 512), 1024, 1, 2, 0), ((256, 14, 14, 1024), 2048, 1, 2, 0)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("xs, ko, r, stride, pad", TILE_FWD,
                         ids=_ids(TILE_FWD, lambda xs, ko, r, st, pd: "%s-k%d-%dx%d-s%d" % ("x".join(map(str, xs)), ko, r, r, st)))
def test_fwd_tile(cuda, xs, ko, r, stride, pad, dtype):
    """The stride-2 3 x 3 and 1 x 1 forward convolutions (the 7 x 7 3 x 3 layer is a case of test_halo_3x3)."""
    x = grid(xs, _seed("x", xs, ko, r), dtype, cuda)
    w = grid((ko, r, r, xs[3]), _seed("w", xs, ko, r), dtype, cuda)
    _summable_16(r * r * xs[3], x, w)
    want = ref_fwd(x, w, stride, pad).float().to(dtype)
    o = _Out(want.shape, dtype, cuda)
    F.conv2d_fwd(x, w, stride, pad, out=o.t)
    _assert_same(o.check("conv2d_fwd"), want, "fwd %s k%d %dx%d s%d" % (xs, ko, r, r, stride))


# the producers of test_gpu_bn_reference.test_conv_producer_stats, with DENSE weights: every output sums R S C products
PRODUCERS = [
    ("halo56", (256, 56, 56, 64), 64, 3, 1, 1), ("halo28", (256, 28, 28, 128), 128, 3, 1, 1),
    ("halo14", (256, 14, 14, 256), 256, 3, 1, 1), ("tile7", (256, 7, 7, 512), 512, 3, 1, 1),
    ("tile3s2", (256, 56, 56, 128), 128, 3, 2, 1), ("tile1x1", (256, 56, 56, 256), 64, 1, 1, 0),
    ("gemm8", (256, 14, 14, 256), 1024, 1, 1, 0), ("expand", (256, 56, 56, 64), 256, 1, 1, 0)]
PRODUCER_CASES = [p + (dt,) for p in PRODUCERS for dt in (BF, HF)]


@pytest.mark.parametrize("pid, xs, ko, r, stride, pad, dtype", PRODUCER_CASES,
                         ids=_ids(PRODUCER_CASES, lambda pid, *rest: "%s-%s" % (pid, DT_IDS[rest[-1]])))
def test_fwd_bnstats_dense(cuda, pid, xs, ko, r, stride, pad, dtype):
    """conv2d_fwd_bnstats: the convolution output of every statistics producer, dense weights (the statistics themselves are
    test_gpu_bn_reference's)."""
    x = grid(xs, _seed("x", pid), dtype, cuda)
    w = grid((ko, r, r, xs[3]), _seed("w", pid), dtype, cuda)
    _summable_16(r * r * xs[3], x, w)
    want = ref_fwd(x, w, stride, pad).float().to(dtype)
    y, _, _ = F.conv2d_fwd_bnstats(x, w, stride, pad)
    _assert_same(y, want, "%s y" % pid)


def _stem_inputs(dtype, dev, seed, kmax=4):
    """x4 [256, 224, 224, 4] (channel 3 zero, as the model feeds it), fp32 channels_last master [64, 3, 7, 7] on the grid."""
    x4 = grid((256, 224, 224, 4), seed, dtype, dev, kmax=kmax)
    x4[..., 3] = 0
    wm = grid((64, 7, 7, 3), seed + 1, torch.float32, dev).permute(0, 3, 1, 2)      # memory order [64][7][7][3]
    return x4, wm


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_stem_fwd(cuda, dtype):
    """stem_conv7_fwd: 7 x 7 / 2 / pad 3, 256 x 224 x 224 x 3 -> 112 x 112 x 64, with and without the statistics epilogue."""
    x4, wm = _stem_inputs(dtype, cuda, 21)
    w_krsc = wm.permute(0, 2, 3, 1)
    _summable_16(147, x4, w_krsc.to(dtype))
    want = ref_fwd(x4[..., :3], w_krsc, 2, 3).float().to(dtype)
    w2 = F.stem_pack_weight(wm, dtype)
    o = _Out(want.shape, dtype, cuda)
    C.call("dle_stem_conv7_fwd", C.ptr(x4), C.ptr(w2), C.ptr(o.t), None, 0, 256, 224, 224, C.dt(x4), C.stream())
    _assert_same(o.check("stem_conv7_fwd"), want, "stem fwd")
    y, _ = F.stem_conv_fwd(x4, w2, want_stats=True)
    _assert_same(y, want, "stem fwd + statistics")


# ================================================================ data gradient
S2_3X3 = [((256, 56, 56, 128), 128), ((256, 28, 28, 256), 256), ((256, 14, 14, 512), 512)]
S2_CASES = [(xs, ko, dt) for xs, ko in S2_3X3 for dt in (BF, HF)]


@pytest.mark.parametrize("xs, ko, dtype", S2_CASES,
                         ids=_ids(S2_CASES, lambda xs, ko, dt: "%s-k%d-%s" % ("x".join(map(str, xs)), ko, DT_IDS[dt])))
def test_dgrad_s2_3x3(cuda, xs, ko, dtype):
    """3 x 3 / stride 2 data gradient: the four parity-class GEMMs of dle_conv2d_dgrad_s2 (the wrapper's path), and the gather
    form dle_conv2d_dgrad called directly."""
    n, h, wd, c = xs
    dy = grid((n, h // 2, wd // 2, ko), _seed("dy", xs), dtype, cuda)
    w = grid((ko, 3, 3, c), _seed("w", xs), dtype, cuda)
    _summable_16(9 * ko, dy, w)
    want = ref_dgrad(dy, w, (h, wd), 2, 1).float().to(dtype)
    o = _Out(want.shape, dtype, cuda)
    F.conv2d_dgrad(dy, w, (h, wd), 2, 1, out=o.t)
    _assert_same(o.check("dgrad_s2"), want, "parity classes %s" % (xs,))
    o2 = _Out(want.shape, dtype, cuda)
    C.call("dle_conv2d_dgrad", C.ptr(dy), C.ptr(w), C.ptr(o2.t), None, n, h, wd, c, ko, 3, 3, 2, 1, C.dt(dy), C.stream())
    _assert_same(o2.check("conv2d_dgrad"), want, "gather form %s" % (xs,))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_dgrad_3x3_addend(cuda, dtype):
    """dx + addend of a 3 x 3 / stride 1 layer: the halo kernel declines an addend, the gather form's ACT_ADD epilogue takes it."""
    n, h, wd, c, ko = 256, 28, 28, 128, 128
    dy = grid((n, h, wd, ko), 31, dtype, cuda)
    w = grid((ko, 3, 3, c), 32, dtype, cuda)
    add = grid((n, h, wd, c), 33, dtype, cuda)
    _summable_16(9 * ko, dy, w, addend=add)
    want = (ref_dgrad(dy, w, (h, wd), 1, 1) + add.to(F64)).float().to(dtype)
    o = _Out(want.shape, dtype, cuda)
    F.conv2d_dgrad(dy, w, (h, wd), 1, 1, addend=add, out=o.t)
    _assert_same(o.check("conv2d_dgrad + addend"), want, "dgrad + addend")


# 1 x 1 / stride 2 downsample layers: (x [N, H, W, C], Ko, Kc1 = Ko of the block's conv1, whose data gradient takes the branch's)
S2_1X1 = [((256, 56, 56, 256), 512, 128), ((256, 28, 28, 512), 1024, 256), ((256, 14, 14, 1024), 2048, 512)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("xs, ko, k1", S2_1X1, ids=_ids(S2_1X1, lambda xs, ko, k1: "%s-k%d" % ("x".join(map(str, xs)), ko)))
def test_dgrad_1x1_s2(cuda, xs, ko, k1, dtype):
    """The downsample branch's data gradient: conv1x1_s2_dgrad_compact on the P x Q grid, dle_upsample_zero, conv2d_dgrad (GEMM +
    zero stuffing), and gemm_add_upsampled2 (conv1's data gradient + the stuffed branch, never materialised) where K = Kc1 fits
    its envelope (64 / 128 / 256): it declines the 14 x 14 layer (K = 512)."""
    n, h, wd, c = xs
    p, q = h // 2, wd // 2
    dy = grid((n, p, q, ko), _seed("dy", xs), dtype, cuda)
    w = grid((ko, 1, 1, c), _seed("w", xs), dtype, cuda)
    _summable_16(ko, dy, w)
    ref_c = (dy.reshape(-1, ko).to(F64) @ w.view(ko, c).to(F64)).view(n, p, q, c)
    want_c = ref_c.float().to(dtype)
    compact = F.conv1x1_s2_dgrad_compact(dy, w)
    _assert_same(compact, want_c, "compact %s" % (xs,))
    o = _Out((n, h, wd, c), dtype, cuda)
    C.call("dle_upsample_zero", C.ptr(compact), C.ptr(o.t), n, p, q, h, wd, c, 2, C.dt(compact), C.stream())
    want = _stuffed(want_c, (h, wd))
    _assert_same(o.check("upsample_zero"), want, "upsample_zero %s" % (xs,))
    _assert_same(want, ref_dgrad(dy, w, (h, wd), 2, 0).float().to(dtype), "reference consistency")
    o2 = _Out((n, h, wd, c), dtype, cuda)
    F.conv2d_dgrad(dy, w, (h, wd), 2, 0, out=o2.t)
    _assert_same(o2.check("conv2d_dgrad 1x1 s2"), want, "conv2d_dgrad %s" % (xs,))
    # conv1 of the block: a = its dy [N H W, Kc1], b = its weight [Kc1, C]; compact on the grid of its own
    a = grid((n * h * wd, k1), _seed("a", xs), dtype, cuda)
    b = grid((k1, c), _seed("b", xs), dtype, cuda)
    cg = grid((n, p, q, c), _seed("c", xs), dtype, cuda)
    out = F.gemm_add_upsampled2(a, b, cg, (h, wd))
    if k1 > 256:
        assert out is None, "gemm_add_upsampled2 must decline K = %d" % k1
        return
    assert out is not None, "gemm_add_upsampled2 declined K = %d" % k1
    _summable_16(k1, a, b, addend=cg)
    want2 = (a.to(F64) @ b.to(F64) + _stuffed(cg, (h, wd)).reshape(-1, c).to(F64)).float().to(dtype)
    _assert_same(out, want2, "gemm_add_upsampled2 %s" % (xs,))


# ================================================================ weight gradient
# wgrad1x1's seven (Ko, C) configurations at their ResNet-50 M; (256, 128) has no ResNet-50 layer: M = 200,704
W1 = [(256, 64, 802816), (64, 256, 802816), (64, 64, 802816), (128, 256, 802816), (256, 128, 200704), (512, 128, 200704),
      (128, 512, 200704)]
W1_EDGES = [(64, 64, 8192, 1), (256, 64, 8192, 1), (64, 64, 8191, 0), (512, 128, 200741, 1), (64, 64, 200741, 1)]
W1_CASES = [(ko, c, m, rc, dt) for ko, c, m, rc in [w + (1,) for w in W1] + W1_EDGES for dt in (BF, HF)]


@pytest.mark.parametrize("ko, c, m, rc, dtype", W1_CASES,
                         ids=_ids(W1_CASES, lambda ko, c, m, rc, dt: "%dx%d-m%d-%s" % (ko, c, m, DT_IDS[dt])))
def test_wgrad1x1(cuda, ko, c, m, rc, dtype):
    """dw [Ko, C] = dy^T x over M rows: the streaming kernel (rc == 1) or its decline, the wrapper, accumulate=True, and the split-K
    tile GEMM resnet.py falls back to, with the streaming kernel pinned off."""
    dy = grid((m, ko), _seed("dy", ko, c, m), dtype, cuda, kmax=2)
    x = grid((m, c), _seed("x", ko, c, m), dtype, cuda, kmax=2)
    ref = _tn(dy, x)
    dw0 = grid((ko, c), _seed("dw0", ko, c, m), torch.float32, cuda)
    _summable_32(_tn(dy.abs(), x.abs()), dy, x, dw0=dw0)
    want, want_acc = ref.float(), (ref + dw0.to(F64)).float()
    what = "wgrad1x1 %dx%d M=%d" % (ko, c, m)
    o = _Out((ko, c), torch.float32, cuda)
    assert _wgrad1x1_try(dy, x, o.t, False) == rc, "%s: dle_wgrad1x1_try" % what
    if rc == 1:
        _assert_same(o.check(what), want, what)
        o2 = _Out((ko, c), torch.float32, cuda)
        assert F.wgrad1x1(dy, x, o2.t)
        _assert_same(o2.check(what), want, "wrapper " + what)
        o3 = _Out((ko, c), torch.float32, cuda, fill=dw0)
        assert F.wgrad1x1(dy, x, o3.t, accumulate=True)
        _assert_same(o3.check(what), want_acc, "accumulate " + what)
    else:
        assert int(C.lib().dle_wgrad1x1_workspace_for(m, ko, c)) == 0 and not F.wgrad1x1(dy, x, o.t)
    with _pinned_off("dle_wgrad1x1_mode"):
        assert _wgrad1x1_try(dy, x, o.t, False) == 0 and not F.wgrad1x1(dy, x, o.t)
        o4 = _Out((ko, c), torch.float32, cuda)
        F.gemm(dy, x, ko, c, m, False, False, out=o4.t, splitk=F.pick_splitk(ko, c, m, target_blocks=1024))
        _assert_same(o4.check(what), want, "split-K GEMM (wgrad1x1 pinned off) " + what)


# 1 x 1 weight gradients outside wgrad1x1's configurations: F.gemm with pick_splitk, as resnet.py calls it
SPLITK_1X1 = [(256, 512, 200704), (1024, 256, 50176), (256, 1024, 50176), (512, 1024, 50176), (2048, 512, 12544),
              (512, 2048, 12544)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ko, c, m", SPLITK_1X1, ids=_ids(SPLITK_1X1, lambda ko, c, m: "%dx%d-m%d" % (ko, c, m)))
def test_wgrad1x1_splitk_gemm(cuda, ko, c, m, dtype):
    dy = grid((m, ko), _seed("dy", ko, c, m), dtype, cuda, kmax=2)
    x = grid((m, c), _seed("x", ko, c, m), dtype, cuda, kmax=2)
    assert int(C.lib().dle_wgrad1x1_workspace_for(m, ko, c)) == 0
    sk = F.pick_splitk(ko, c, m, target_blocks=1024)
    assert sk > 1
    ref = _tn(dy, x)
    dw0 = grid((ko, c), _seed("dw0", ko, c), torch.float32, cuda)
    _summable_32(_tn(dy.abs(), x.abs()), dy, x, dw0=dw0)
    o = _Out((ko, c), torch.float32, cuda)
    F.gemm(dy, x, ko, c, m, False, False, out=o.t, splitk=sk)
    _assert_same(o.check("gemm"), ref.float(), "split-K %d GEMM %dx%d M=%d" % (sk, ko, c, m))
    o2 = _Out((ko, c), torch.float32, cuda, fill=dw0)
    F.gemm(dy, x, ko, c, m, False, False, out=o2.t, splitk=sk, accumulate=True)
    _assert_same(o2.check("gemm"), (ref + dw0.to(F64)).float(), "split-K GEMM accumulate %dx%d" % (ko, c))


# halo-tile weight gradient: (x [N, H, W, C], Ko, rc); nsub = Ko C / 64^2 = 1, 4, 16, 64 at the ResNet-50 layers
HALO_W = [((256, 56, 56, 64), 64), ((256, 28, 28, 128), 128), ((256, 14, 14, 256), 256), ((256, 7, 7, 512), 512)]
HALO_W_EDGES = [((13, 27, 29, 64), 128, 1), ((997, 1, 59, 64), 64, 1), ((7, 9, 61, 64), 64, 1), ((7, 9, 62, 64), 64, 0)]
HALO_W_CASES = [c + (dt,) for c in [(xs, ko, 1) for xs, ko in HALO_W] + HALO_W_EDGES for dt in (BF, HF)]


@pytest.mark.parametrize("xs, ko, rc, dtype", HALO_W_CASES,
                         ids=_ids(HALO_W_CASES, lambda xs, ko, rc, dt: "%s-k%d-%s" % ("x".join(map(str, xs)), ko, DT_IDS[dt])))
def test_wgrad_halo_3x3(cuda, xs, ko, rc, dtype):
    """3 x 3 / stride 1 weight gradient: the halo-tile kernel (rc == 1) or its decline, conv2d_wgrad with and without accumulate,
    and the split-K implicit GEMM with the halo kernel pinned off."""
    n, h, wd, c = xs
    dy = grid((n, h, wd, ko), _seed("dy", xs, ko), dtype, cuda, kmax=2)
    x = grid(xs, _seed("x", xs, ko), dtype, cuda, kmax=2)
    ref = ref_wgrad(dy, x, 3, 3, 1, 1)
    dw0 = grid((ko, 3, 3, c), _seed("dw0", xs, ko), torch.float32, cuda)
    _summable_32(ref_wgrad(dy.abs(), x.abs(), 3, 3, 1, 1), dy, x, dw0=dw0)
    want, want_acc = ref.float(), (ref + dw0.to(F64)).float()
    what = "halo wgrad %s k%d" % (xs, ko)
    o = _Out(want.shape, torch.float32, cuda)
    assert _conv3x3_wgrad_try(dy, x, o.t, False) == rc, "%s: dle_conv3x3_wgrad_try" % what
    if rc == 1:
        _assert_same(o.check(what), want, what)
    o2 = _Out(want.shape, torch.float32, cuda)
    F.conv2d_wgrad(dy, x, (3, 3), 1, 1, out=o2.t)
    _assert_same(o2.check(what), want, "conv2d_wgrad " + what)
    o3 = _Out(want.shape, torch.float32, cuda, fill=dw0)
    F.conv2d_wgrad(dy, x, (3, 3), 1, 1, out=o3.t, accumulate=True)
    _assert_same(o3.check(what), want_acc, "conv2d_wgrad accumulate " + what)
    with _pinned_off("dle_conv3x3_wgrad_mode"):
        assert _conv3x3_wgrad_try(dy, x, o.t, False) == 0
        o4 = _Out(want.shape, torch.float32, cuda)
        F.conv2d_wgrad(dy, x, (3, 3), 1, 1, out=o4.t)
        _assert_same(o4.check(what), want, "split-K implicit GEMM (halo pinned off) " + what)


# split-K implicit GEMM (dle_conv2d_wgrad): the stride-2 layers, (x [N, H, W, C], Ko, R, pad)
IMPLICIT_W = [((256, 56, 56, 128), 128, 3, 1), ((256, 28, 28, 256), 256, 3, 1), ((256, 14, 14, 512), 512, 3, 1),
              ((256, 56, 56, 256), 512, 1, 0), ((256, 28, 28, 512), 1024, 1, 0), ((256, 14, 14, 1024), 2048, 1, 0)]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("xs, ko, r, pad", IMPLICIT_W,
                         ids=_ids(IMPLICIT_W, lambda xs, ko, r, pd: "%s-k%d-%dx%d" % ("x".join(map(str, xs)), ko, r, r)))
def test_wgrad_implicit_s2(cuda, xs, ko, r, pad, dtype):
    n, h, wd, c = xs
    p, q = _out_hw(h, wd, r, r, 2, pad)
    dy = grid((n, p, q, ko), _seed("dy", xs, ko), dtype, cuda, kmax=2)
    x = grid(xs, _seed("x", xs, ko), dtype, cuda, kmax=2)
    sk = F.pick_splitk(ko, r * r * c, n * p * q, target_blocks=1024)
    assert sk > 1
    ref = ref_wgrad(dy, x, r, r, 2, pad)
    dw0 = grid((ko, r, r, c), _seed("dw0", xs, ko), torch.float32, cuda)
    _summable_32(ref_wgrad(dy.abs(), x.abs(), r, r, 2, pad), dy, x, dw0=dw0)
    what = "implicit wgrad %s k%d %dx%d (split-K %d)" % (xs, ko, r, r, sk)
    o = _Out(ref.shape, torch.float32, cuda)
    F.conv2d_wgrad(dy, x, (r, r), 2, pad, out=o.t)
    _assert_same(o.check(what), ref.float(), what)
    o2 = _Out(ref.shape, torch.float32, cuda, fill=dw0)
    F.conv2d_wgrad(dy, x, (r, r), 2, pad, out=o2.t, accumulate=True)
    _assert_same(o2.check(what), (ref + dw0.to(F64)).float(), "accumulate " + what)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_stem_wgrad(cuda, dtype):
    """stem_conv7_wgrad over 3.2 M output pixels: |k| <= 2 and half of dy zero keep every sum of magnitudes below 2^18."""
    x4, _ = _stem_inputs(dtype, cuda, 41, kmax=2)
    dy = grid((256, 112, 112, 64), 43, dtype, cuda, kmax=2, density=0.5)
    ref = ref_wgrad(dy, x4[..., :3], 7, 7, 2, 3)
    dw0 = grid((64, 7, 7, 3), 44, torch.float32, cuda)
    _summable_32(ref_wgrad(dy.abs(), x4[..., :3].abs(), 7, 7, 2, 3), dy, x4, dw0=dw0)
    o = _Out((64 * 147,), torch.float32, cuda)
    F.stem_conv_wgrad(dy, x4, o.t)
    _assert_same(o.check("stem wgrad").view(64, 7, 7, 3), ref.float(), "stem wgrad")
    o2 = _Out((64 * 147,), torch.float32, cuda, fill=dw0.reshape(-1))
    F.stem_conv_wgrad(dy, x4, o2.t, accumulate=True)
    _assert_same(o2.check("stem wgrad").view(64, 7, 7, 3), (ref + dw0.to(F64)).float(), "stem wgrad accumulate")


# ================================================================ realistic inputs
def _gamma(n):
    return n * U / (1 - n * U)


def _assert_close16(got, ref, absref, k, what):
    """One rounding to 16 bits of an fp32 sum of chains of at most k additions."""
    g = got.to(F64)
    bar = 0.5 * ulp16(torch.maximum(g.abs(), ref.abs()), got.dtype) + _gamma(k) * absref
    d = (g - ref).abs()
    assert bool((d <= bar).all()), "%s: worst %g of the bar at %s" % (what, float((d / bar).max()), torch.nonzero(d > bar)[:4].tolist())


def _assert_close32(got, ref, absref, n, what):
    d = (got.to(F64) - ref).abs()
    bar = _gamma(n) * absref
    assert bool((d <= bar).all()), "%s: worst %g of the bar (n = %d)" % (what, float((d / bar).max()), n)


def _gauss(shape, seed, dtype, dev, scale=1.0):
    return (torch.randn(shape, generator=gen(dev, seed), device=dev) * scale).to(dtype)


def _chain_wgrad1x1(ko, c, m):
    tg, wg, ph = {(256, 64): (64, 512, 1), (64, 256): (64, 512, 1), (64, 64): (128, 512, 2), (128, 256): (64, 256, 1),
                  (256, 128): (64, 256, 1), (512, 128): (32, 256, 1), (128, 512): (32, 256, 1)}[(ko, c)]
    tiles = -(-m // tg)
    wg = min(wg, tiles)
    return -(-tiles // wg) * tg // ph + ph - 1 + wg + 16


def _chain_halo_wgrad(n, h, wd, c, ko):
    tiles = -(-(n * (h + 1) * (wd + 2)) // 128)
    npg = 256 // ((ko // 64) * (c // 64))
    return -(-tiles // npg) * 64 + 1 + npg + 16


def _chain_splitk(k, sk):
    ktiles = -(-k // 64)
    return -(-ktiles // sk) * 64 + sk + 16


GAUSS = ["fwd_halo", "fwd_tile", "fwd_stem", "dgrad_halo", "dgrad_s2", "wgrad1x1", "wgrad_halo", "wgrad_implicit", "wgrad_stem"]
GAUSS_CASES = [(k, dt) for k in GAUSS for dt in (BF, HF)]


@pytest.mark.parametrize("family, dtype", GAUSS_CASES, ids=_ids(GAUSS_CASES, lambda k, dt: "%s-%s" % (k, DT_IDS[dt])))
def test_gaussian(cuda, family, dtype):
    """One batch-256 layer per direction and kernel family on Gaussian data: the error-analysis bars of the module docstring."""
    s = _seed("gauss", family, DT_IDS[dtype])
    if family in ("fwd_halo", "fwd_tile", "dgrad_halo", "dgrad_s2", "wgrad_halo", "wgrad_implicit"):
        xs, ko, stride = {"fwd_halo": ((256, 56, 56, 64), 64, 1), "fwd_tile": ((256, 28, 28, 256), 256, 2),
                          "dgrad_halo": ((256, 28, 28, 128), 128, 1), "dgrad_s2": ((256, 28, 28, 256), 256, 2),
                          "wgrad_halo": ((256, 56, 56, 64), 64, 1), "wgrad_implicit": ((256, 28, 28, 256), 256, 2)}[family]
        n, h, wd, c = xs
        p, q = _out_hw(h, wd, 3, 3, stride, 1)
        x = _gauss(xs, s, dtype, cuda)
        w = _gauss((ko, 3, 3, c), s + 1, dtype, cuda, (9.0 * c) ** -0.5)
        dy = _gauss((n, p, q, ko), s + 2, dtype, cuda, 0.5)
        if family.startswith("fwd"):
            y = F.conv2d_fwd(x, w, stride, 1)
            _assert_close16(y, ref_fwd(x, w, stride, 1), ref_fwd(x.abs(), w.abs(), stride, 1), 9 * c, family)
        elif family.startswith("dgrad"):
            dx = F.conv2d_dgrad(dy, w, (h, wd), stride, 1)
            _assert_close16(dx, ref_dgrad(dy, w, (h, wd), stride, 1), ref_dgrad(dy.abs(), w.abs(), (h, wd), stride, 1), 9 * ko,
                            family)
        else:
            dw = F.conv2d_wgrad(dy, x, (3, 3), stride, 1)
            if stride == 1:
                chain = _chain_halo_wgrad(n, h, wd, c, ko)
            else:
                chain = _chain_splitk(n * p * q, F.pick_splitk(ko, 9 * c, n * p * q, target_blocks=1024))
            _assert_close32(dw, ref_wgrad(dy, x, 3, 3, stride, 1), ref_wgrad(dy.abs(), x.abs(), 3, 3, stride, 1), chain, family)
    elif family == "wgrad1x1":
        ko, c, m = 256, 64, 802816
        dy = _gauss((m, ko), s, dtype, cuda, 0.5)
        x = _gauss((m, c), s + 1, dtype, cuda)
        dw = torch.empty((ko, c), dtype=torch.float32, device=cuda)
        assert F.wgrad1x1(dy, x, dw)
        _assert_close32(dw, _tn(dy, x), _tn(dy.abs(), x.abs()), _chain_wgrad1x1(ko, c, m), family)
    else:
        x4 = _gauss((256, 224, 224, 4), s, dtype, cuda)
        x4[..., 3] = 0
        wm = _gauss((64, 7, 7, 3), s + 1, torch.float32, cuda, 147 ** -0.5).permute(0, 3, 1, 2)
        w2 = F.stem_pack_weight(wm, dtype)
        w16 = wm.permute(0, 2, 3, 1).to(dtype)                   # the packed operand holds the master rounded to 16 bits
        x3 = x4[..., :3]
        if family == "fwd_stem":
            y, _ = F.stem_conv_fwd(x4, w2, want_stats=False)
            _assert_close16(y, ref_fwd(x3, w16, 2, 3), ref_fwd(x3.abs(), w16.abs(), 2, 3), 147, family)
        else:
            dy = _gauss((256, 112, 112, 64), s + 2, dtype, cuda, 0.5)
            dw = torch.empty(64 * 147, dtype=torch.float32, device=cuda)
            F.stem_conv_wgrad(dy, x4, dw)
            chain = -(-(256 * 112) // 512) * 128 + 512 + 8
            _assert_close32(dw.view(64, 7, 7, 3), ref_wgrad(dy, x3, 7, 7, 2, 3), ref_wgrad(dy.abs(), x3.abs(), 7, 7, 2, 3), chain,
                            family)
