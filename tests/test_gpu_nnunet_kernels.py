"""The nnU-Net kernels (csrc/nnunet.hip) against tests/_nnunet_ref.py: dle_conv3d_in_fwd bit for bit on exactly summable inputs and
under the derived per-element bar on random ones, the padding-behind-the-norm rule, channel slices, the statistic partials,
reproducibility and the argument checks; dle_instnorm_fold, dle_upsample3d_x2_fwd and dle_nnunet_head_blend_fwd likewise.

Shapes: (1,1,1) and (2,2,2) are less than one 128-voxel tile, (3,5,7) and (5,6,17) have odd extents (stride 2 then reads past the
last voxel on one side only) and 105 / 510 voxels: one partial tile, and three full tiles plus a partial one; (4,4,4) and (8,8,8) are
the fixture's levels, 8^3 = 512 voxels = exactly four tiles.  C = 8 is the stem's path (a tap per 16-byte piece, K = 216 padded to
256), C = 64 one K chunk per tap, C = 192 three.  Ko = 128 gives two channel tiles."""
import itertools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from tests import _exact_grid as G
from tests import _nnunet_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (4, 4, 4), (8, 8, 8), (5, 6, 17)]
CASES = [pytest.param(s, st, c, ko, id="%dx%dx%d-s%d-c%d-k%d" % (s + (st, c, ko)))
         for s, st, c, ko in itertools.product(SHAPES, (1, 2), (8, 64, 192), (64, 128))]
RELUS = [(False, False), (False, True), (True, False), (True, True)]


def out_dims(shape, stride):
    return tuple((e - 1) // stride + 1 for e in shape)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def random_case(shape, C, Ko, N, dtype, seed):
    g = gen(seed)
    x = torch.randn((N,) + shape + (C,), generator=g).to(dtype)
    w = (torch.randn(Ko, 3, 3, 3, C, generator=g) * (2.0 / (27 * C)) ** 0.5).to(dtype)
    # 11 significant bits: scale * x + shift is exact in float64, so the host reproduces the fma bit for bit; different per sample
    scale = (1.0 + 0.25 * torch.randn(N, C, generator=g)).half().float()
    shift = (0.5 * torch.randn(N, C, generator=g)).half().float()
    return x, w, scale, shift


def run_conv(x, w, scale, shift, stride, relu_in, relu_out, with_part=True):
    N, D, H, W, C = x.shape
    Ko = w.shape[0]
    y = G.Out((N,) + out_dims((D, H, W), stride) + (Ko,), x.dtype, DEV)
    part = None
    if with_part:
        part = G.Out((N, F.conv3d_in_bands(D, H, W, stride), Ko, 3), torch.float32, DEV)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    F.conv3d_in_fwd(dev(x), dev(w), y.t, scale=dev(scale), shift=dev(shift), stride=stride, relu_in=relu_in, relu_out=relu_out,
                    part=None if part is None else part.t)
    torch.cuda.synchronize()
    return y.check("conv3d_in_fwd").cpu(), (None if part is None else part.check("conv3d_in_fwd partials").cpu())


def check_partials(part, y, what):
    """The partials, merged in float64, against two-pass float64 statistics of the kernel's own stored output."""
    n, s, m2 = R.chan_merge64(part)
    n0, s0, m20 = R.stats64(y)
    sum_bar, m2_bar = R.stats_bars(y)
    assert torch.equal(n, n0), what
    assert bool((part[..., 0] > 0).all()) and bool((part[..., 2] >= 0).all()), what
    r_sum, r_m2 = float(((s - s0).abs() / sum_bar).max()), float(((m2 - m20).abs() / m2_bar).max())
    assert r_sum <= 1.0 and r_m2 <= 1.0, "%s: partial sums at %.3g / %.3g of their bars" % (what, r_sum, r_m2)


# ---------------------------------------------------------------------------------------------- dle_conv3d_in_fwd
@pytest.mark.parametrize("shape, stride, C, Ko", CASES)
def test_conv_bit_for_bit_on_exact_grid(shape, stride, C, Ko):
    """x = k / 4, scale a power of two, shift = k / 4, w = k / 4 (sparse): every product is a multiple of 1 / 32 and every partial
    sum is exact in fp32 in any order, so the stored output is the correctly rounded exact sum."""
    idx = SHAPES.index(shape) + (C // 64) + Ko // 64
    dtype, N = (HF, BF)[idx % 2], 1 + (idx // 2) % 2
    relu_in, relu_out = RELUS[idx % 4]
    x = G.grid((N,) + shape + (C,), 11 + idx, dtype, "cpu")
    w = G.grid((Ko, 3, 3, 3, C), 12 + idx, dtype, "cpu", kmax=2, density=0.25)
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (N, C), generator=gen(13 + idx))]
    shift = G.grid((N, C), 14 + idx, torch.float32, "cpu")
    a = R.conv_operand(x, scale, shift, relu_in, dtype)
    an, wn = a.permute(0, 4, 1, 2, 3), w.double().permute(0, 4, 1, 2, 3)
    mag = torch.nn.functional.conv3d(an.abs(), wn.abs(), stride=stride, padding=1)
    assert torch.equal(a * 8, torch.round(a * 8)) and float(mag.max()) < G.B_MFMA
    want, _ = R.conv3d_in(x, w, scale, shift, stride, relu_in, relu_out, dtype)
    y, part = run_conv(x, w, scale, shift, stride, relu_in, relu_out)
    G.assert_same(G.bits(y), G.bits(want.float().to(dtype)), "conv3d_in %s" % (shape,))
    check_partials(part, y, "exact grid")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape, stride, C, Ko", CASES)
def test_conv_under_bar_on_random_inputs(shape, stride, C, Ko, dtype):
    idx = SHAPES.index(shape) + (C // 64) + Ko // 64 + stride
    N = 1 + idx % 2
    relu_in, relu_out = RELUS[(idx // 2) % 4]
    x, w, scale, shift = random_case(shape, C, Ko, N, dtype, 100 + idx)
    want, bar = R.conv3d_in(x, w, scale, shift, stride, relu_in, relu_out, dtype)
    y, part = run_conv(x, w, scale, shift, stride, relu_in, relu_out)
    worst = float(((y.double() - want).abs() / bar).max())
    assert worst <= 1.0, "conv3d_in at %.3g of its bar" % worst
    check_partials(part, y, "random")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu_in, relu_out", RELUS)
@pytest.mark.parametrize("with_scale", [True, False])
def test_conv_flags_and_null_scale(relu_in, relu_out, with_scale, dtype):
    x, w, scale, shift = random_case((3, 5, 7), 64, 64, 2, dtype, 7)
    if not with_scale:
        scale = shift = None
    want, bar = R.conv3d_in(x, w, scale, shift, 1, relu_in, relu_out, dtype)
    y, part = run_conv(x, w, scale, shift, 1, relu_in, relu_out, with_part=False)
    assert part is None
    assert float(((y.double() - want).abs() / bar).max()) <= 1.0
    if not relu_out:
        assert bool((y < 0).any())
    if not with_scale and not relu_in:
        # scale == NULL passes the bits through: the same as scale 1, shift 0
        one, zero = torch.ones(2, 64), torch.zeros(2, 64)
        y1, _ = run_conv(x, w, one, zero, 1, False, relu_out, with_part=False)
        G.assert_same(G.bits(y), G.bits(y1), "scale NULL against scale 1")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_padding_sits_behind_the_norm(stride, dtype):
    """x = 0, shift = 96 on every channel, w = 1/64 on channel 0 of every tap: an output counts its taps inside the volume times
    1.5.  A kernel that padded in front of the norm would give 27 * 1.5 everywhere."""
    D, H, W = 4, 5, 6
    x = torch.zeros(1, D, H, W, 64, dtype=dtype)
    w = torch.zeros(64, 3, 3, 3, 64, dtype=dtype)
    w[:, :, :, :, 0] = 1.0 / 64
    scale, shift = torch.ones(1, 64), torch.full((1, 64), 96.0)
    y, _ = run_conv(x, w, scale, shift, stride, False, False, with_part=False)
    ones = torch.ones(1, 1, D, H, W, dtype=torch.float64)
    taps = torch.nn.functional.conv3d(ones, torch.ones(1, 1, 3, 3, 3, dtype=torch.float64), stride=stride, padding=1)[0, 0]
    want = (1.5 * taps)[..., None].expand(-1, -1, -1, 64)
    G.assert_same(y[0].double(), want.contiguous(), "taps inside the volume")
    if stride == 1:
        assert float(y[0, 1, 1, 1, 0]) == 27 * 1.5 and float(y[0, 0, 0, 0, 0]) == 8 * 1.5 and float(y[0, 0, 2, 2, 0]) == 18 * 1.5


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_channel_slices_leave_the_rest_untouched(dtype):
    """ldx > C, ldy > Ko, both offsets non-zero; the other channels of y hold a pattern that must survive; stride 2."""
    N, shape, C, Ko, ldx, ldy, x_off, y_off = 2, (5, 6, 7), 64, 64, 192, 136, 128, 64
    x, w, scale, shift = random_case(shape, C, Ko, N, dtype, 21)
    wide = torch.randn((N,) + shape + (ldx,), generator=gen(22)).to(dtype)
    wide[..., x_off:x_off + C] = x
    out = out_dims(shape, 2)
    pattern = (torch.arange(N * out[0] * out[1] * out[2] * ldy) % 251).reshape((N,) + out + (ldy,)).to(dtype)
    y = G.Out((N,) + out + (ldy,), dtype, DEV, fill=pattern)
    part = G.Out((N, F.conv3d_in_bands(*shape, 2), Ko, 3), torch.float32, DEV)
    F.conv3d_in_fwd(wide.to(DEV), w.to(DEV), y.t, C_in=C, x_off=x_off, y_off=y_off, scale=scale.to(DEV), shift=shift.to(DEV), stride=2,
                    relu_in=False, relu_out=True, part=part.t)
    torch.cuda.synchronize()
    got = y.check("sliced conv3d_in_fwd").cpu()
    want, bar = R.conv3d_in(x, w, scale, shift, 2, False, True, dtype)
    assert float(((got[..., y_off:y_off + Ko].double() - want).abs() / bar).max()) <= 1.0
    keep = torch.ones(ldy, dtype=torch.bool)
    keep[y_off:y_off + Ko] = False
    G.assert_same(G.bits(got[..., keep]), G.bits(pattern[..., keep]), "channels outside the slice")
    check_partials(part.check("partials").cpu(), got[..., y_off:y_off + Ko], "sliced")
    # the same convolution from a dense tensor gives the same bits
    dense, _ = run_conv(x, w, scale, shift, 2, False, True, with_part=False)
    G.assert_same(G.bits(got[..., y_off:y_off + Ko].contiguous()), G.bits(dense), "slice against dense")


def test_conv_two_calls_are_bit_identical():
    x, w, scale, shift = random_case((5, 6, 17), 192, 128, 2, HF, 31)
    y1, p1 = run_conv(x, w, scale, shift, 1, True, True)
    y2, p2 = run_conv(x, w, scale, shift, 1, True, True)
    G.assert_same(G.bits(y1), G.bits(y2), "output")
    G.assert_same(G.bits(p1), G.bits(p2), "partials")


def test_conv_more_than_one_band():
    """A volume of more than 512 tiles: bands of two tiles, the last band partial (24 x 24 x 115 = 66240 voxels = 517.5 tiles)."""
    shape = (24, 24, 115)
    assert F.conv3d_in_bands(*shape, 1) == 259
    x, w, _, _ = random_case(shape, 8, 64, 1, HF, 41)
    want, bar = R.conv3d_in(x, w, None, None, 1, False, True, HF)
    y, part = run_conv(x, w, None, None, 1, False, True)
    assert float(((y.double() - want).abs() / bar).max()) <= 1.0
    assert part.shape[1] == 259 and float(part[0, :-1, 0, 0].min()) == 256.0 and float(part[0, -1, 0, 0]) == 66240 - 258 * 256
    check_partials(part, y, "bands of two tiles")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_partials_at_an_offset_mean(dtype):
    """The epilogue's own Welford / Chan path where a sum(x^2) - n mean^2 formula loses the variance: x = 4 + noise, positive weights
    on the centre tap only (so border voxels see the same sum), no scale, no ReLU: every output channel has mean >= 16 sd over the
    510 voxels (four tiles, the last partial) of each sample."""
    g = gen(45)
    x = (4.0 + 0.05 * torch.randn(2, 5, 6, 17, 64, generator=g)).to(dtype)
    w = torch.zeros(64, 3, 3, 3, 64)
    w[:, 1, 1, 1, :] = (0.5 + torch.rand(64, 64, generator=g)) / 64
    w = w.to(dtype)
    y, part = run_conv(x, w, None, None, 1, False, False)
    n, s_, m2 = R.stats64(y)
    assert float(((s_ / n).abs() / torch.sqrt(m2 / n)).min()) >= 16.0
    check_partials(part, y, "offset mean")
    want, bar = R.conv3d_in(x, w, None, None, 1, False, False, dtype)
    assert float(((y.double() - want).abs() / bar).max()) <= 1.0


def test_conv_argument_errors_launch_nothing():
    x = torch.zeros(1, 2, 2, 2, 64, dtype=HF, device=DEV)
    w = torch.zeros(64, 3, 3, 3, 64, dtype=HF, device=DEV)
    y = G.Out((1, 2, 2, 2, 64), HF, DEV, fill=torch.full((1, 2, 2, 2, 64), 3.0))
    before = y.t.clone()
    one = torch.ones(1, 64, device=DEV)
    bad = [
        dict(x=x, weight=torch.zeros(32, 3, 3, 3, 64, dtype=HF, device=DEV), y=torch.zeros(1, 2, 2, 2, 32, dtype=HF, device=DEV)),   # Ko % 64
        dict(x=torch.zeros(1, 2, 2, 2, 16, dtype=HF, device=DEV), weight=torch.zeros(64, 3, 3, 3, 16, dtype=HF, device=DEV), y=y.t),  # C = 16
        dict(x=x, weight=w, y=y.t, x_off=8),                                     # slice past the line
        dict(x=x, weight=w, y=y.t, y_off=4),
        dict(x=x, weight=w, y=y.t, stride=3),
        dict(x=x, weight=w, y=y.t, scale=one),                                   # scale without shift
        dict(x=x, weight=w.to(BF), y=y.t),
        dict(x=x, weight=w, y=torch.zeros(1, 1, 1, 1, 64, dtype=HF, device=DEV)),  # stride-1 output of the wrong size
        dict(x=x.float(), weight=w, y=y.t),
        dict(x=x, weight=w, y=y.t, part=torch.zeros(1, 2, 64, 3, device=DEV)),   # wrong band count
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            F.conv3d_in_fwd(**kw)
    # straight at the C ABI: a misaligned pointer, a wrong dtype code
    from deeplearningexamples_amd import _cabi as C
    for args in ((x.data_ptr() + 2, 64, 0), (x.data_ptr(), 64, 0)):
        dtype_code = C.F16 if args[0] != x.data_ptr() else C.F32
        rc = C.lib().dle_conv3d_in_fwd(args[0], args[1], args[2], 0, 0, w.data_ptr(), y.t.data_ptr(), 64, 0, 0, 1, 2, 2, 2, 64, 64, 1, 0, 0,
                                       dtype_code, C.stream())
        assert rc == -1 and len(C.lib().dle_last_error()) > 0
    assert F.conv3d_in_bands(128, 128, 128, 1) == 512 and F.conv3d_in_bands(1, 1, 1, 2) == 1
    with pytest.raises(ValueError):
        F.conv3d_in_bands(0, 1, 1, 1)
    torch.cuda.synchronize()
    G.assert_same(G.bits(y.check("rejected calls")), G.bits(before), "output after rejected calls")


# ---------------------------------------------------------------------------------------------- dle_instnorm_fold
def fold_case(N, G_, C, n_per_band, offset, seed):
    """Partials of G_ bands of a channel population with mean = offset * sd, as exact float64 statistics rounded to fp32."""
    y = torch.randn(N, G_ * n_per_band, C, generator=gen(seed), dtype=torch.float64) * 0.75 + offset * 0.9
    y = y.float().double()
    part = torch.stack([torch.stack(R.stats64(y[:, g * n_per_band:(g + 1) * n_per_band]), -1) for g in range(G_)], 1).float()
    gamma = (1.0 + 0.25 * torch.randn(C, generator=gen(seed + 1))).float()
    beta = (0.1 * torch.randn(C, generator=gen(seed + 2))).float()
    return y, part, gamma, beta


@pytest.mark.parametrize("G_, offset", [(1, 0.0), (1, 16.0), (5, 16.0), (8, 40.0)])
def test_fold_against_float64(G_, offset):
    N, C = 2, 72
    y, part, gamma, beta = fold_case(N, G_, C, 300, offset, 50 + G_)
    if offset:
        n, s, m2 = R.stats64(y)
        assert float(((s / n).abs() / torch.sqrt(m2 / n)).min()) >= 16.0
    scale = G.Out((N, C), torch.float32, DEV)
    shift = G.Out((N, C), torch.float32, DEV)
    F.instnorm_fold(part.to(DEV), gamma.to(DEV), beta.to(DEV), R.EPS, scale.t, shift.t)
    torch.cuda.synchronize()
    # the reference folds the fp32 partials the kernel was given, merged in float64: the bars carry the merge and the evaluation
    n, s, m2 = R.chan_merge64(part)
    want_scale, want_shift = R.fold64(n, s, m2, gamma, beta)
    # the kernel's G_ merges in fp32: each rounds the running mean (u |mean|) and takes the difference d of two means with an error of
    # 2 u |mean|, which M2 feels as 2 |d| n_b 2 u |mean| per band; sum_b |d_b| n_b <= sqrt(n M2)
    mean = (s / n).abs()
    scale_bar, shift_bar = R.fold_bars(n, s, m2, gamma, beta, G_ * R.U * s.abs(), 2 * G_ * R.U * m2 + 4 * R.U * mean * torch.sqrt(n * m2))
    r1 = float(((scale.check("fold").cpu().double() - want_scale).abs() / scale_bar).max())
    r2 = float(((shift.check("fold").cpu().double() - want_shift).abs() / shift_bar).max())
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    # and the population's own float64 statistics, with the rounding of the partials to fp32 as their bar
    n0, s0, m20 = R.stats64(y)
    sb, mb = (G_ + 2) * R.U * s0.abs(), (2 * G_ + 2) * R.U * m20 + 8 * R.U * (s0 / n0).abs() * torch.sqrt(m20 * n0)
    w_scale, w_shift = R.fold64(n0, s0, m20, gamma, beta)
    b_scale, b_shift = R.fold_bars(n0, s0, m20, gamma, beta, sb, mb)
    assert float(((scale.t.cpu().double() - w_scale).abs() / b_scale).max()) <= 1.0
    assert float(((shift.t.cpu().double() - w_shift).abs() / b_shift).max()) <= 1.0


def test_fold_slice_form():
    """Two producers fold into one table: columns [0, 40) and [40, 104) of a [N, 104] pair; the other columns keep their bits."""
    N = 2
    _, pa, ga, ba = fold_case(N, 3, 40, 100, 2.0, 60)
    _, pb, gb, bb = fold_case(N, 1, 64, 50, 16.0, 70)
    gamma, beta = torch.cat((ga, gb)).to(DEV), torch.cat((ba, bb)).to(DEV)
    scale = G.Out((N, 112), torch.float32, DEV, fill=torch.full((N, 112), 7.0))
    shift = G.Out((N, 112), torch.float32, DEV, fill=torch.full((N, 112), -7.0))
    F.instnorm_fold(pa.to(DEV), gamma[:40], beta[:40], R.EPS, scale.t, shift.t, out_off=0)
    F.instnorm_fold(pb.to(DEV), gamma[40:], beta[40:], R.EPS, scale.t, shift.t, out_off=40)
    torch.cuda.synchronize()
    sc, sh = scale.check("fold").cpu(), shift.check("fold").cpu()
    assert bool((sc[:, 104:] == 7.0).all()) and bool((sh[:, 104:] == -7.0).all())
    for part, g, b, lo in ((pa, ga, ba, 0), (pb, gb, bb, 40)):
        dense_s, dense_h = torch.empty(N, part.shape[2], device=DEV), torch.empty(N, part.shape[2], device=DEV)
        F.instnorm_fold(part.to(DEV), g.to(DEV), b.to(DEV), R.EPS, dense_s, dense_h)
        G.assert_same(G.bits(sc[:, lo:lo + part.shape[2]].contiguous()), G.bits(dense_s.cpu()), "scale slice")
        G.assert_same(G.bits(sh[:, lo:lo + part.shape[2]].contiguous()), G.bits(dense_h.cpu()), "shift slice")
    with pytest.raises(ValueError):
        F.instnorm_fold(pb.to(DEV), gamma[40:], beta[40:], R.EPS, scale.t, shift.t, out_off=64)       # 64 + 64 > 112


# ---------------------------------------------------------------------------------------------- dle_upsample3d_x2_fwd
def run_upsample(x, C=None, x_off=0, ldy=None, y_off=0, fill=None):
    N, D, H, W, ldx = x.shape
    C = ldx if C is None else C
    ldy = C if ldy is None else ldy
    y = G.Out((N, 2 * D, 2 * H, 2 * W, ldy), x.dtype, DEV, fill=fill)
    part = G.Out((N, F.upsample3d_x2_bands(D, H, W), C, 3), torch.float32, DEV)
    F.upsample3d_x2_fwd(x.to(DEV), y.t, channels=C, x_off=x_off, y_off=y_off, part=part.t)
    torch.cuda.synchronize()
    return y.check("upsample").cpu(), part.check("upsample partials").cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 2), (2, 2, 2), (3, 5, 4), (4, 4, 4), (9, 10, 11)])
def test_upsample_under_bar_and_partials(shape, dtype):
    N, C = 2, 24 if shape != (4, 4, 4) else 768                  # 768: 96 channel groups, two voxel lanes and 64 idle threads
    x = torch.randn((N,) + shape + (C,), generator=gen(80)).to(dtype)
    y, part = run_upsample(x)
    want = R.upsample64(x)
    worst = float(((y.double() - want).abs() / R.upsample_bar(x, want, dtype)).max())
    assert worst <= 1.0, worst
    check_partials(part, y, "upsample")
    if shape == (1, 1, 1):
        G.assert_same(G.bits(y), G.bits(x.expand(N, 2, 2, 2, C).contiguous()), "extent 1 copies")
    if shape == (9, 10, 11):
        assert part.shape[1] > 1                                  # 7920 output voxels: bands of 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample_exact_where_representable(dtype):
    """Constant along every interpolated axis -> the value itself; extent 2 along one axis with values 0 and 3 -> i / 3 * 3 = i
    (lambda = i / 3 rounded, times 3: fma(lambda, 3, 0) rounds back to the integer, exactly representable)."""
    C = 16
    per_channel = G.grid((1, 1, 1, 1, C), 90, dtype, "cpu", kmax=40)
    x = per_channel.expand(2, 3, 4, 5, C).contiguous()
    y, _ = run_upsample(x)
    G.assert_same(G.bits(y), G.bits(per_channel.expand(2, 6, 8, 10, C).contiguous()), "constant volume")
    x = torch.zeros(1, 1, 1, 2, 8, dtype=dtype)
    x[0, 0, 0, 1] = 3.0
    y, _ = run_upsample(x)
    want = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)[None, None, None, :, None].expand(1, 2, 2, 4, 8)
    G.assert_same(y.double(), want.contiguous(), "ramp of thirds")
    # varies along d only, extents 1 along h and w: a pure copy along those axes
    x = G.grid((1, 2, 1, 1, 8), 91, dtype, "cpu")
    y, _ = run_upsample(x)
    assert torch.equal(y[:, :, 0, 0], y[:, :, 1, 1]) and torch.equal(y[0, 0, 0, 0], x[0, 0, 0, 0]) and torch.equal(y[0, 3, 0, 0], x[0, 1, 0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample_partials_at_an_offset_mean(dtype):
    x = (8.0 + 0.05 * torch.randn(2, 9, 10, 11, 24, generator=gen(96))).to(dtype)
    y, part = run_upsample(x)
    n, s_, m2 = R.stats64(y)
    assert float(((s_ / n).abs() / torch.sqrt(m2 / n)).min()) >= 16.0 and part.shape[1] > 1
    check_partials(part, y, "upsample, offset mean")


def test_upsample_slice_write():
    dtype, N, shape, C, ldx, x_off, ldy, y_off = HF, 2, (2, 3, 4), 16, 40, 24, 48, 8
    wide = torch.randn((N,) + shape + (ldx,), generator=gen(95)).to(dtype)
    pattern = (torch.arange(N * 4 * 6 * 8 * ldy) % 199).reshape(N, 4, 6, 8, ldy).to(dtype)
    y, part = run_upsample(wide, C=C, x_off=x_off, ldy=ldy, y_off=y_off, fill=pattern)
    dense, dense_part = run_upsample(wide[..., x_off:x_off + C].contiguous())
    G.assert_same(G.bits(y[..., y_off:y_off + C].contiguous()), G.bits(dense), "slice against dense")
    G.assert_same(G.bits(part), G.bits(dense_part), "partials")
    keep = torch.ones(ldy, dtype=torch.bool)
    keep[y_off:y_off + C] = False
    G.assert_same(G.bits(y[..., keep]), G.bits(pattern[..., keep]), "channels outside the slice")
    with pytest.raises(ValueError):
        F.upsample3d_x2_fwd(wide.to(DEV), torch.zeros(N, 4, 6, 8, 48, dtype=dtype, device=DEV), channels=12)        # C % 8
    with pytest.raises(ValueError):
        F.upsample3d_x2_fwd(wide.to(DEV), torch.zeros(N, 4, 6, 7, 48, dtype=dtype, device=DEV), channels=16)


# ---------------------------------------------------------------------------------------------- dle_nnunet_head_blend_fwd
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_blend_two_overlapping_windows(dtype):
    K, C, patch, vol = 3, 64, (3, 4, 5), (5, 6, 9)
    g = gen(99)
    w = (torch.randn(K, C, generator=g) * 0.2).to(dtype)
    b = torch.randn(K, generator=g)
    imp = torch.rand(patch, generator=g) + 0.1
    wins = [torch.randn(patch + (C,), generator=g).to(dtype) for _ in range(2)]
    origins = [(0, 1, 2), (2, 2, 4)]                               # they share d = 2, h = 2..4, w = 4..6
    start = torch.randn((K,) + vol, generator=g)
    out = G.Out((K,) + vol, torch.float32, DEV, fill=start)
    want, bar = start.double().clone(), torch.zeros((K,) + vol, dtype=torch.float64)
    for x, (d0, h0, w0) in zip(wins, origins):
        F.nnunet_head_blend_fwd(x.to(DEV), w.to(DEV), b.to(DEV), imp.to(DEV), out.t, (d0, h0, w0))
        sl = (slice(None), slice(d0, d0 + patch[0]), slice(h0, h0 + patch[1]), slice(w0, w0 + patch[2]))
        logits = torch.einsum("dhwc,kc->kdhw", x.double(), w.double()) + b.double()[:, None, None, None]
        mag = torch.einsum("dhwc,kc->kdhw", x.double().abs(), w.double().abs()) + b.double().abs()[:, None, None, None]
        want[sl] += imp.double() * logits
        bar[sl] += (C + 4) * R.U * imp.double() * mag + R.U * want[sl].abs() + 2.0 ** -140
    torch.cuda.synchronize()
    got = out.check("head_blend").cpu()
    touched = bar > 0
    assert int(touched[0].sum()) == 2 * 60 - 9                     # 3 x 4 x 5 voxels each, 1 x 3 x 3 shared
    assert float(((got.double() - want).abs()[touched] / bar[touched]).max()) <= 1.0
    G.assert_same(G.bits(got[~touched]), G.bits(start[~touched]), "voxels outside the windows")
    both = torch.zeros(vol, dtype=torch.bool)
    both[2, 2:5, 4:7] = True
    assert bool(touched[0][both].all())
    for origin in ((3, 0, 0), (0, 3, 0), (0, 0, 5), (-1, 0, 0)):
        with pytest.raises(ValueError):
            F.nnunet_head_blend_fwd(wins[0].to(DEV), w.to(DEV), b.to(DEV), imp.to(DEV), out.t, origin)
    with pytest.raises(ValueError):
        F.nnunet_head_blend_fwd(wins[0].to(DEV), torch.zeros(9, C, dtype=dtype, device=DEV), torch.zeros(9, device=DEV), imp.to(DEV),
                                torch.zeros((9,) + vol, device=DEV), (0, 0, 0))
    torch.cuda.synchronize()
    G.assert_same(G.bits(out.check("rejected calls").cpu()), G.bits(got), "output after rejected calls")
