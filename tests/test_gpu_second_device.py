"""Every launcher that opts in to more dynamic LDS than the default (DLE_LAUNCH_LDS, csrc/common.h) on a second device of the
same process: the same seeded inputs on cuda:0, then on cuda:1, give bitwise the same outputs.  The opt-in and the cached device
limits are kept per device; device 0 runs first, so any state kept for the whole process would be set there.  GPU only; skipped
with fewer than two devices."""
import numpy as np
import pytest
import torch

from oracle import dlrm_oracle as O
from test_gpu_conv_bnload import _bn_vectors
from test_gpu_gemm import _F, _mk
from test_gpu_gemm8 import _operands

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _attention_bwd(s):
    def run(dev):
        F, _ = _F()
        b, nh, d = 2, 4, 64
        g = torch.Generator().manual_seed(s)
        qkv = _mk((b * s, 3 * nh * d), BF16, g, 0.8).to(dev)
        dctx = _mk((b * s, nh * d), BF16, g, 0.5).to(dev)
        mask_add = torch.zeros(b, s, device=dev)
        mask_add[1, s // 2:] = -10000.0
        _, stats, _ = F.attention_fwd(qkv, mask_add, b, s, nh, 0.125, 0.1, 1234, 7)
        return [F.attention_bwd(qkv, dctx, mask_add, stats, b, s, nh, 0.125, 0.1, 1234, 7)]
    return run


def _conv3x3(dev):
    F, _ = _F()
    g = torch.Generator().manual_seed(3)
    x, dy = _mk((2, 14, 14, 64), BF16, g, 0.5).to(dev), _mk((2, 14, 14, 128), BF16, g, 0.5).to(dev)
    w = _mk((128, 3, 3, 64), BF16, g, 1.0 / 24).to(dev)
    return [F.conv2d_fwd(x, w, 1, 1), F.conv2d_dgrad(dy, w, (14, 14), 1, 1)]


def _conv3x3_wgrad(dev):
    F, C = _F()
    g = torch.Generator().manual_seed(4)
    x, dy = _mk((3, 14, 14, 128), BF16, g).to(dev), _mk((3, 14, 14, 64), BF16, g).to(dev)
    out = torch.empty((64, 3, 3, 128), device=dev)
    old = C.lib().dle_conv3x3_wgrad_mode(1)
    try:
        F.conv2d_wgrad(dy, x, (3, 3), 1, 1, out=out)
        return [out]
    finally:
        C.lib().dle_conv3x3_wgrad_mode(old)


def _wgrad1x1(dev):
    F, _ = _F()
    g = torch.Generator().manual_seed(5)
    dy, x = _mk((8192, 256), BF16, g).to(dev), _mk((8192, 64), BF16, g).to(dev)
    out = torch.empty((256, 64), device=dev)
    assert F.wgrad1x1(dy, x, out)
    return [out]


def _conv_bnbwd(dev):
    F, _ = _F()
    m, k, n = 5000, 256, 64
    g = torch.Generator().manual_seed(6)
    t, dy, w = _mk((m, k), BF16, g).to(dev), _mk((m, k), BF16, g, 0.01).to(dev), _mk((k, n), BF16, g, 1.0 / 16).to(dev)
    mean, rstd, gamma, _ = _bn_vectors(g, k, dev)
    bits = torch.randint(0, 256, (m * k // 8,), generator=g, dtype=torch.uint8).to(dev)
    dg, db = torch.empty(k, device=dev), torch.empty(k, device=dev)
    out = F.bn_bwd_conv1x1_dgrad(dy, t, mean, rstd, gamma, dg, db, w, relu_mask=bits)
    assert out is not None
    return [out[0], out[1], dg, db]


def _conv_bnload(dev):
    F, _ = _F()
    g = torch.Generator().manual_seed(7)
    t, res = _mk((2, 56, 56, 256), BF16, g).to(dev), _mk((2, 56, 56, 256), BF16, g).to(dev)
    w = _mk((128, 1, 1, 256), BF16, g, 0.1).to(dev)
    out = F.conv1x1_bnload_fwd(t, res, w, *_bn_vectors(g, 256, dev))
    assert out is not None
    return list(out)


def _gemm_expand(epi, b_kc, mnk):
    def run(dev):
        F, C = _F()
        act = {"none": C.ACT_NONE, "masked": C.ACT_ADD_MASKED}[epi]
        m, n, k = mnk
        g = torch.Generator().manual_seed(m + n + k)
        a, w = _mk((m, k), BF16, g, 0.5).to(dev), _mk((n, k) if b_kc else (k, n), BF16, g, 0.1).to(dev)
        src = _mk((m, n), BF16, g).to(dev) if act != C.ACT_NONE else None
        bits = torch.randint(0, 256, (m * n // 8,), generator=g, dtype=torch.uint8).to(dev) if act == C.ACT_ADD_MASKED else None
        return [F.gemm(a, w, m, n, k, True, b_kc, act=act, mask_src=src, aux=bits)]
    return run


def _gemm_expand_bnred(dev):
    F, _ = _F()
    m, n, k = 12544, 512, 128
    g = torch.Generator().manual_seed(8)
    g2, w, addend, t2 = (_mk((m, k), BF16, g, 0.05).to(dev), _mk((k, n), BF16, g, k ** -0.5).to(dev),
                         _mk((m, n), BF16, g, 0.05).to(dev), _mk((m, n), BF16, g, 1.5).to(dev))
    bits1, bits2 = (torch.randint(0, 256, (m * n // 8,), generator=g, dtype=torch.uint8).to(dev) for _ in range(2))
    mean2, rstd2, _, _ = _bn_vectors(g, n, dev)
    dg, db = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dx = F.gemm_masked_add_bnred(g2, w, m, n, k, addend, bits1, t2, bits2, mean2, rstd2, dg, db)
    assert dx is not None
    return [dx, dg, db]


def _gemm_smallm(dev):
    F, _ = _F()
    m, n, k = 128, 4096, 1536
    g = torch.Generator().manual_seed(9)
    a, b = _mk((m, k), BF16, g).to(dev), _mk((n, k), BF16, g).to(dev)
    return [F.gemm(a, b, m, n, k, True, True), F.gemm(a, b, m, n, k, True, True, out_dtype=torch.float32)]


def _gemm_big_tile(dev):
    F, C = _F()
    m, n, k = 4096, 2560, 256
    g = torch.Generator().manual_seed(10)
    a, b = _mk((m, k), BF16, g).to(dev), _mk((n, k), BF16, g).to(dev)
    bias = torch.randn(n, generator=g).to(dev)
    old = C.lib().dle_gemm8_mode(0)
    try:
        return [F.gemm(a, b, m, n, k, True, True, bias=bias, act=C.ACT_RELU),
                F.gemm(a, b.T.contiguous(), m, n, k, True, False, out_dtype=torch.float32)]
    finally:
        C.lib().dle_gemm8_mode(old)


def _gemm8(dev):
    F, C = _F()
    m, n, k = 2048, 1280, 128
    g = torch.Generator().manual_seed(11)
    a, b, a_kc, b_kc, _ = _operands("nt", m, n, k, BF16, dev, g, scale=0.5)
    bias = torch.randn(n, generator=g).to(dev)
    lib = C.lib()
    prev_items, prev_mode = lib.dle_gemm8_min_items(1), lib.dle_gemm8_mode(1)
    try:
        before = lib.dle_gemm8_launch_count()
        out = F.gemm(a, b, m, n, k, a_kc, b_kc, bias=bias, act=C.ACT_RELU)
        assert lib.dle_gemm8_launch_count() == before + 1
        return [out]
    finally:
        lib.dle_gemm8_min_items(prev_items)
        lib.dle_gemm8_mode(prev_mode)


def _emb_onehot(dev):
    F, _ = _F()
    sizes, dim, batch = [4, 128, 1, 97, 11, 63, 104, 35], 128, 4099
    rng = np.random.default_rng(12)
    off = O.table_offsets(sizes)
    w = torch.from_numpy(rng.standard_normal((int(off[-1]), dim)).astype(np.float32)).to(dev)
    idx = np.stack([rng.integers(0, s, batch) for s in sizes], 1).astype(np.int64)
    rows = torch.from_numpy(O.offset_indices(idx, off)).to(dev)
    grad = torch.from_numpy(rng.standard_normal((batch, len(sizes), dim)).astype(np.float32) * 0.05).to(BF16).to(dev)
    ws = F.EmbUpdateWorkspace(off, dim, dev)
    assert ws.n_onehot == len(sizes)
    F.emb_sgd_dedup_(w, rows, grad, ws, 0.5, scale=torch.tensor([0.25], device=dev))
    return [w]


LAUNCHERS = {
    "attention_bwd_s512": _attention_bwd(512),
    "attention_bwd_s128": _attention_bwd(128),
    "conv3x3_fwd_dgrad": _conv3x3,
    "conv3x3_wgrad": _conv3x3_wgrad,
    "wgrad1x1": _wgrad1x1,
    "conv_bnbwd": _conv_bnbwd,
    "conv_bnload": _conv_bnload,
    "gemm_expand_plain": _gemm_expand("none", True, (4097, 512, 128)),
    "gemm_expand_masked": _gemm_expand("masked", False, (4101, 256, 64)),
    "gemm_expand_bnred": _gemm_expand_bnred,
    "gemm_smallm": _gemm_smallm,
    "gemm_dma_big_tile": _gemm_big_tile,
    "gemm8": _gemm8,
    "emb_onehot": _emb_onehot,
}


@pytest.mark.parametrize("name", list(LAUNCHERS))
def test_second_device_matches_the_first(name):
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    outs = []
    for i in (0, 1):
        dev = torch.device("cuda", i)
        with torch.cuda.device(dev):
            got = LAUNCHERS[name](dev)
            torch.cuda.synchronize()
        assert all(t.device == dev for t in got)
        outs.append([t.cpu() for t in got])
    for j, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), "%s: output %d differs between cuda:0 and cuda:1" % (name, j)
