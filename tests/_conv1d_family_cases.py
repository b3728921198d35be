"""The cases of tests/test_gpu_conv1d_family_bits.py and tools/make_conv1d_family_bits.py: every entry point of the conv1d family
(csrc/hifigan.hip, fastpitch.hip, quartznet.hip, jasper.hip) at the smallest shapes at which each piece they share through
csrc/conv1d_family.h can go wrong.  Inputs are seeded on the CPU (one torch.Generator per case) and moved to the device; a case
returns {output name: tensor} and `digest` is the sha256 of a tensor's bytes.

  hfg_ko{24,40,136}     conv1d_lrelu_fwd, B 2, T 70 (a ragged time tile), C 72 (a chunk tail beyond C), ksize 7, dilation 3, slope 0.1,
                        alpha 0.5, add1 and add2 = out; Ko 24 / 40 / 136: one, two, four wavefronts across the channels, all ragged
  fp_k3, fp_k5, fp_clamp  conv1d_packed_fwd, lengths (70, 0, 33), max_len 128, C 72, Ko 136, slope 0, add1 = out; ksize 3 holds all
                        taps in registers, ksize 5 loads one tap ahead; fp_clamp: the table gives the last sequence 50 rows, 17 past
                        `total`
  qn_{s1d1,s2,d2}_pf{0,1}  tcs_conv1d_packed_fwd, lengths (130, 0, 65), C 128, Ko 320 (a second, ragged channel block), ksize 33,
                        residual + ReLU, d_out, both forms of the chunk loop
  js_{s1d1,s2,d2}       conv1d_bn_packed_fwd, lengths (130, 0, 65), C 128, Ko 192, ksize 11, residual + ReLU
  qn_b65_pf{0,1}, js_b65  65 sequences of 3 rows, one of them empty: the tile search takes its second 64-sequence step and carries
                        the running count
  normalize             qn_normalize_pack and qn_normalize_pack_lead (lead 16), B 3, F 64
"""
import hashlib

import torch

from deeplearningexamples_amd import functional as F

DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
LENS = (130, 0, 65)
LENS65 = (3,) * 7 + (0,) + (3,) * 57


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _rand(g, shape, dtype, std=1.0):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * std).to(dtype).to(DEV)


def _cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def _hfg(ko, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        b, t, c, ks, dil = 2, 70, 72, 7, 3
        x = _rand(g, (b, t, c), dtype)
        w = _rand(g, (ko, ks, c), dtype, (ks * c) ** -0.5)
        bias = _rand(g, (ko,), torch.float32)
        add1, out = _rand(g, (b, t, ko), dtype), _rand(g, (b, t, ko), dtype)
        return {"y": F.conv1d_lrelu_fwd(x, w, bias, dilation=dil, slope=0.1, alpha=0.5, add1=add1, add2=out, out=out)}
    return case


def _fp(ks, seed, past_total=0):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        lens, c, ko = (70, 0, 33), 72, 136
        total = sum(lens)
        x = _rand(g, (total, c), dtype)
        w = _rand(g, (ko, ks, c), dtype, (ks * c) ** -0.5)
        bias = _rand(g, (ko,), torch.float32)
        out = _rand(g, (total, ko), dtype)
        cu = _cu(lens[:-1] + (lens[-1] + past_total,))
        return {"y": F.conv1d_packed_fwd(x, w, bias, cu, 128, slope=0.0, add1=out, out=out)}
    return case


def _packed_operands(g, lens, stride, c, ko, dtype):
    ol = [(n - 1) // stride + 1 if n > 0 else 0 for n in lens]
    x = _rand(g, (sum(lens), c), dtype)
    scale = _rand(g, (ko,), torch.float32)
    shift = _rand(g, (ko,), torch.float32)
    res = _rand(g, (sum(ol), ko), dtype)
    return x, scale, shift, res, _cu(lens), (_cu(ol) if stride != 1 else None), (sum(ol) if stride != 1 else None)


def _qn(lens, stride, dil, pf, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        c, ko, ks = 128, 320, 33
        dw = _rand(g, (ks, c), dtype, ks ** -0.5)
        pw = _rand(g, (ko, c), dtype, c ** -0.5)
        x, scale, shift, res, cu_in, cu_out, total_out = _packed_operands(g, lens, stride, c, ko, dtype)
        d = torch.zeros((res.shape[0], c), dtype=dtype, device=DEV)
        old = F.tcs_prefetch_mode(pf)
        try:
            y = F.tcs_conv1d_packed_fwd(x, dw, pw, scale, shift, cu_in, cu_out, total_out, stride=stride, dilation=dil, residual=res,
                                        relu=True, d_out=d)
        finally:
            F.tcs_prefetch_mode(old)
        return {"y": y, "d": d}
    return case


def _js(lens, stride, dil, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        c, ko, ks = 128, 192, 11
        w = _rand(g, (ko, ks, c), dtype, (ks * c) ** -0.5)
        x, scale, shift, res, cu_in, cu_out, total_out = _packed_operands(g, lens, stride, c, ko, dtype)
        return {"y": F.conv1d_bn_packed_fwd(x, w, scale, shift, cu_in, cu_out, total_out, stride=stride, dilation=dil, residual=res,
                                            relu=True)}
    return case


def _normalize(dtype):
    g = torch.Generator().manual_seed(70)
    lens, f, t_pad, lead = (70, 2, 33), 64, 72, 16
    x = (torch.randn((len(lens), f, t_pad), generator=g) * 3 + 1).to(DEV)
    return {"plain": F.qn_normalize_pack(x, _cu(lens), sum(lens), dtype),
            "lead": F.qn_normalize_pack_lead(x, _cu([n + lead for n in lens]), sum(lens) + lead * len(lens), dtype, lead)}


CASES = {"hfg_ko40": _hfg(40, 10), "hfg_ko24": _hfg(24, 11), "hfg_ko136": _hfg(136, 12),
         "fp_k3": _fp(3, 20), "fp_k5": _fp(5, 21), "fp_clamp": _fp(3, 22, past_total=17)}
for _i, (_v, _s, _d) in enumerate((("s1d1", 1, 1), ("s2", 2, 1), ("d2", 1, 2))):
    for _pf in (0, 1):
        CASES["qn_%s_pf%d" % (_v, _pf)] = _qn(LENS, _s, _d, _pf, 30 + _i)
    CASES["js_%s" % _v] = _js(LENS, _s, _d, 40 + _i)
for _pf in (0, 1):
    CASES["qn_b65_pf%d" % _pf] = _qn(LENS65, 1, 1, _pf, 50)
CASES["js_b65"] = _js(LENS65, 1, 1, 60)
CASES["normalize"] = _normalize


def digests(name, dtype):
    out = CASES[name](dtype)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in out.items()}
