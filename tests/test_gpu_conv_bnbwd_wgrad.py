"""csrc/conv_bnbwd.hip, weight-gradient form (dle_conv1x1_bnbwd_dgrad_wgrad): the conv3 / bn3 unit's BatchNorm backward, data
gradient AND weight gradient in one kernel, dt never written.  Against dle_conv1x1_bnbwd_dgrad on the same inputs: dx and the
folded bn2 sums bit-identical; gw against a float64 product (host) of x and the 16-bit dt that call writes, with at most twice
the error of the parent's weight-gradient launch on that dt, and bit-identical to the streaming weight-gradient kernel where
that is the parent's launch (the same accumulation order); rows beyond M poisoned; two runs bit-identical.  And which path one ResNet-50 backward takes.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K, N = 256, 64
POISON = 3.0e4                     # large, finite in fp16 and bf16


def _pack(keep):
    """[M, C] bool -> bit-packed keep bits (bit i of a byte = element 8 b + i), little endian like numpy.packbits(bitorder="little")"""
    wts = (2 ** torch.arange(8, device=keep.device)).to(torch.int32)
    return (keep.view(-1, 8).to(torch.int32) * wts).sum(-1).to(torch.uint8)


def _rows(m, c, dtype, gen, cuda, scale=1.0, shift=0.0, tail=64):
    """[m, c] as the head of an allocation of m + tail rows whose tail holds POISON"""
    big = torch.full((m + tail, c), POISON, dtype=dtype, device=cuda)
    big[:m] = (torch.randn(m, c, generator=gen, device=cuda) * scale + shift).to(dtype)
    return big[:m]


def _bits(m, c, p, gen, cuda, tail=64):
    keep = torch.ones(m + tail, c, dtype=torch.bool, device=cuda)      # the tail keeps everything: a leaked row is not masked away
    keep[:m] = torch.rand(m, c, generator=gen, device=cuda) < p
    return _pack(keep)[:m * c // 8]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("bred", [True, False])
@pytest.mark.parametrize("m", [802816, 4096, 4096 + 37])
def test_weight_gradient_in_the_fused_kernel(cuda, m, bred, masked, dtype):
    from deeplearningexamples_amd import functional as F
    gen = torch.Generator(device=cuda).manual_seed(m + 2 * int(bred) + int(masked))
    t = _rows(m, K, dtype, gen, cuda)
    dy = _rows(m, K, dtype, gen, cuda, scale=0.01)
    x = _rows(m, N, dtype, gen, cuda, shift=0.3).clamp_(min=0)           # the unit's input sits behind a ReLU
    w = (torch.randn(K, N, generator=gen, device=cuda) / 16).to(dtype)
    gamma = torch.rand(K, generator=gen, device=cuda) + 0.5
    mean, rstd = t.float().mean(0), 1.0 / torch.sqrt(t.float().var(0, unbiased=False) + 1e-5)
    bits = _bits(m, K, 0.6, gen, cuda) if masked else None
    b2 = lambda: None
    if bred:
        t2 = _rows(m, N, dtype, gen, cuda, shift=0.2)
        bits2 = _bits(m, N, 0.5, gen, cuda)
        mean2, rstd2 = t2.float().mean(0), 1.0 / torch.sqrt(t2.float().var(0, unbiased=False) + 1e-5)
        b2 = lambda: (t2, bits2, mean2, rstd2, torch.full((N,), 9.0, device=cuda), torch.full((N,), 9.0, device=cuda))
    # the parent: fused BatchNorm backward + data gradient (dt written), then the weight-gradient launch on that dt
    dg_p, db_p = torch.empty(K, device=cuda), torch.empty(K, device=cuda)
    bp = b2()
    dt, dx_p, taken_p = F.bn_bwd_conv1x1_dgrad(dy, t, mean, rstd, gamma, dg_p, db_p, w, relu_mask=bits, bnred=bp)
    gw_p = torch.empty(K, N, device=cuda)
    streamed = F.wgrad1x1(dt, x, gw_p)
    if not streamed:
        F.gemm(dt, x, K, N, m, False, False, out=gw_p, splitk=F.pick_splitk(K, N, m, target_blocks=1024))
    # the new path, twice
    runs = []
    for _ in range(2):
        dg, db = torch.empty(K, device=cuda), torch.empty(K, device=cuda)
        gw = torch.full((K, N), 7.0, device=cuda)
        bn = b2()
        out = F.bn_bwd_conv1x1_dgrad_wgrad(dy, t, mean, rstd, gamma, dg, db, w, x, gw, relu_mask=bits, bnred=bn)
        assert out is not None
        runs.append((out[0], out[1], gw, dg, db, bn))
    dx, taken, gw, dg, db, bn = runs[0]
    assert taken == taken_p == bred
    assert torch.equal(dg, dg_p) and torch.equal(db, db_p)
    assert torch.equal(dx, dx_p)
    if bred:
        assert torch.equal(bn[4], bp[4]) and torch.equal(bn[5], bp[5])
        assert not torch.any(bn[4] == 9.0)
    assert torch.equal(runs[1][2], gw) and torch.equal(runs[1][0], dx)
    # float64 on the host, from the 16-bit dt the parent wrote
    ref = dt.cpu().double().t() @ x.cpu().double()
    err_new = (gw.cpu().double() - ref).abs().max().item()
    err_parent = (gw_p.cpu().double() - ref).abs().max().item()
    print("M=%d %s masked=%d bred=%d: max |gw - fp64| new %.4e parent %.4e (max |ref| %.4e)"
          % (m, str(dtype).split(".")[-1], masked, bred, err_new, err_parent, ref.abs().max().item()))
    assert err_new <= 2.0 * err_parent
    if streamed:                   # same accumulation order as the streaming weight-gradient kernel: a training run stays its bits
        assert torch.equal(gw, gw_p)


def test_outside_the_envelope_nothing_is_launched(cuda):
    from deeplearningexamples_amd import functional as F
    t = torch.randn(8192, 128, device=cuda).half()
    out = F.bn_bwd_conv1x1_dgrad_wgrad(t, t, torch.zeros(128, device=cuda), torch.ones(128, device=cuda), torch.ones(128, device=cuda),
                                       torch.empty(128, device=cuda), torch.empty(128, device=cuda),
                                       torch.randn(128, 32, device=cuda).half(), torch.randn(8192, 32, device=cuda).half(),
                                       torch.empty(128, 32, device=cuda))
    assert out is None


@pytest.mark.parametrize("switch", ["1", "0"])
def test_rn50_backward_takes_the_path_the_switch_says(cuda, switch, monkeypatch):
    """One ResNet-50 forward + backward at batch 256: with DLE_RN50_FUSE_BNBWD_WGRAD on, the new entry point is launched 4 times
    (the three conv3 units of layer1 and its downsample unit) and the streaming weight gradient for [256, 64] never; off: 0 and 4."""
    from deeplearningexamples_amd import _cabi as C
    from deeplearningexamples_amd.convnets.resnet import ResNet50
    from deeplearningexamples_amd.convnets.engine import ResNetTrainer
    monkeypatch.setenv("DLE_RN50_FUSE_BNBWD_WGRAD", switch)
    torch.manual_seed(3)
    model = ResNet50(device=cuda)
    tr = ResNetTrainer(model, lr=0.01, compute_dtype=torch.bfloat16, static_loss_scale=128.0)
    x = torch.randn(256, 3, 224, 224, device=cuda)
    y = torch.randint(0, 1000, (256,), device=cuda)
    tm = C.KernelTimer()
    old = C.set_timer(tm)
    try:
        loss = tr.train_step(x, y)
        torch.cuda.synchronize()
    finally:
        C.set_timer(old)
    assert torch.isfinite(loss).all()
    fused = sum(1 for name, _, _, _ in tm.records if name == "dle_conv1x1_bnbwd_dgrad_wgrad")
    plain = sum(1 for name, _, _, _ in tm.records if name == "dle_conv1x1_bnbwd_dgrad")
    wg = sum(1 for name, _, _, meta in tm.records if name == "dle_gemm" and meta and meta.get("tag") == "256x64x802816")
    assert (fused, plain, wg) == ((4, 0, 0) if switch == "1" else (0, 4, 4)), (fused, plain, wg)
