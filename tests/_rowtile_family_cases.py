"""The cases of tests/test_gpu_rowtile_family_bits.py and tools/make_rowtile_family_bits.py: the entry points of the row-tile family
(tft.hip, ncf.hip, moflow.hip) and of transformer_xl.hip, dot_interact.hip and attention.hip, which take the index map rt_feat from
csrc/mfma32_rows.h, at the smallest shapes at which the shared pieces can go wrong.  The other files that store an accumulator
through rt_feat (conv3x3_wgrad.hip, wgrad1x1.hip, conv_bnbwd.hip, stem.hip, emb_onehot.hip, nnunet.hip) have no case here: only
an integer index is involved, and a wrong one fails their own float64 suites grossly.  Inputs are seeded on the CPU (one
torch.Generator per case) and moved to the device; a case returns {output name: tensor} and `digest` is the sha256 of a tensor's
bytes.  Each case is one or two launches.

  grn_ctx, grn_gate, grn_index_q, grn_row1   tft_grn_fwd: 33 rows (a second, ragged tile) in the full form with a context row per 3
                        rows; the gate form with the residual addressed per (batch element, step); the full form over a row index
                        list with the quantile tail (3 quantiles) and no 16-bit output; one row
  vsn_f1, vsn_f8        tft_vsn_fwd, 33 rows: one variable (no LayerNorm over the variables); 8 variables in three groups with a
                        context and the selection weights
  lstm                  tft_lstm_fwd, batch 33, 3 steps, h0 and c0 not zero
  tft_attn              tft_attention_fwd, 2 x 33 steps, encoder length 20, with the probabilities
  ncf_b100_wg2, ncf_b33 ncf_score_fwd, 37 users, 23 items, labels and probabilities; 100 samples on two workgroups (one walks two
                        tiles, one walks one) and 33 on the device's own grid; one index outside its table in each (a NaN logit,
                        digested as it is).  The loss partials behind the first workgroup of ncf_b33 are as many as the device has
                        compute units: the case returns the first and the sum of the rest (zero)
  couple_s{0,1}_h{0,1}, couple_b129   mf_couple_fwd, 33 samples, 4 positions of 8 + 8 channels, K 48, both mask orders with the image
                        on either half; 129 samples: a second workgroup in y with one live wavefront
  atom_wg1, atom_wg0    mf_atom_reverse_fwd, 33 samples, 9 nodes of 5 types, hidden 64 / 96, 40 (40 pads to 64), 3 flows, row stride
                        1: one workgroup that walks both tiles, and the device's own grid
  txl                   txl_rel_attention_fwd, 2 sequences of 33 queries over 16 memory rows, 2 heads, the ring started at row 5
  dot_fwd, dot_bwd      dot_interact_fwd / _bwd at [5, 27, 128], the smallest shape of the DLRM suite
  attn_varlen, attn_s256  the only user of the masked score block (attention_fwd_varlen; lengths 130 and 33: a full and a partial key
                        block) and, for the walk it shares, attention_fwd at 256 keys, the shortest long sequence; one head each
"""
import hashlib

import torch

from deeplearningexamples_amd import functional as F

DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
H = 128


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _rand(g, shape, dtype, std=1.0, mean=0.0):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * std + mean).to(dtype).to(DEV)


def _grn_params(g, dtype, full, ctx):
    p = {"wg": _rand(g, (2 * H, H), dtype, H ** -0.5), "bg": _rand(g, (2 * H,), torch.float32, 0.3),
         "gamma": _rand(g, (H,), torch.float32, 0.3, 1.0), "beta": _rand(g, (H,), torch.float32, 0.3)}
    if full:
        p.update(wa=_rand(g, (H, H), dtype, H ** -0.5), ba=_rand(g, (H,), torch.float32, 0.3),
                 wi=_rand(g, (H, H), dtype, H ** -0.5), bi=_rand(g, (H,), torch.float32, 0.3))
        if ctx:
            p["wc"] = _rand(g, (H, H), dtype, H ** -0.5)
    return p


def _grn_ctx(dtype):
    g = torch.Generator().manual_seed(100)
    p = _grn_params(g, dtype, True, True)
    return {"y": F.tft_grn_fwd(_rand(g, (33, H), dtype), p, ctx=_rand(g, (11, H), dtype), rows_per_ctx=3)}


def _grn_gate(dtype):
    g = torch.Generator().manual_seed(101)
    p = _grn_params(g, dtype, False, False)
    return {"y": F.tft_grn_fwd(_rand(g, (33, H), dtype), p, res=_rand(g, (11, 5, H), dtype), res_rows_per_batch=3)}


def _grn_index_q(dtype):
    g = torch.Generator().manual_seed(102)
    p = _grn_params(g, dtype, True, False)
    x = _rand(g, (40, H), dtype)
    idx = torch.randperm(40, generator=g)[:33].to(torch.int32).to(DEV)
    wq, bq = _rand(g, (3, H), torch.float32, H ** -0.5), _rand(g, (3,), torch.float32)
    return {"q": F.tft_grn_fwd(x, p, x_index=idx, wq=wq, bq=bq, want_out=False)}


def _grn_row1(dtype):
    g = torch.Generator().manual_seed(103)
    p = _grn_params(g, dtype, True, False)
    return {"y": F.tft_grn_fwd(_rand(g, (1, H), dtype), p)}


def _vsn(nvars, groups, ctx, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        b, t = 11, 3
        p = {"w16": _rand(g, (2 * H * H + 32 * H + nvars * 3 * H * H,), dtype, H ** -0.5),
             "p32": _rand(g, (nvars * H + 2 * H + 32 + nvars * 8 + 24 + nvars * 9 * H,), torch.float32, 0.3), "F": nvars, "has_ctx": ctx}
        xs = [_rand(g, (b, t, n), torch.float32) for n in groups]
        c = _rand(g, (b, H), dtype) if ctx else None
        if ctx:
            y, w = F.tft_vsn_fwd(xs, p, dtype, t, ctx=c, want_weights=True)
            return {"y": y, "w": w}
        return {"y": F.tft_vsn_fwd(xs, p, dtype, t)}
    return case


def _lstm(dtype):
    g = torch.Generator().manual_seed(120)
    b, t = 33, 3
    out, hn, cn = F.tft_lstm_fwd(_rand(g, (b, t, 4 * H), torch.float32), _rand(g, (4 * H, H), dtype, H ** -0.5), _rand(g, (b, H), dtype, 0.5),
                                 _rand(g, (b, H), torch.float32, 0.5))
    return {"out": out, "hn": hn, "cn": cn}


def _tft_attn(dtype):
    g = torch.Generator().manual_seed(130)
    b, t = 2, 33
    out, probs = F.tft_attention_fwd(_rand(g, (b * t, 288), dtype), _rand(g, (H, 32), dtype, 32 ** -0.5), b, t, 20, want_probs=True)
    return {"out": out, "probs": probs}


def _ncf(batch, max_wg, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        nu, ni = 37, 23
        tables = [_rand(g, s, dtype, 0.5) for s in ((nu, 64), (ni, 64), (nu, 128), (ni, 128))]
        weights = [_rand(g, (o, i), dtype, i ** -0.5) for o, i in ((256, 256), (128, 256), (64, 128))]
        biases = [_rand(g, (o,), torch.float32, 0.3) for o in (256, 128, 64)]
        wf, bf = _rand(g, (128,), torch.float32, 0.2), _rand(g, (1,), torch.float32)
        user = torch.randint(0, nu, (batch,), generator=g)
        item = torch.randint(0, ni, (batch,), generator=g)
        user[7], item[batch - 2] = nu, -1
        label = torch.randint(0, 2, (batch,), generator=g).float().to(DEV)
        logit, prob, part = F.ncf_score_fwd(*tables, weights, biases, wf, bf, user.to(DEV), item.to(DEV), label=label, want_prob=True,
                                            max_workgroups=max_wg)
        if max_wg:
            return {"logit": logit, "prob": prob, "loss": part}
        return {"logit": logit, "prob": prob, "loss": part[:1], "loss_behind": part[1:].abs().sum().reshape(1)}
    return case


def _couple(batch, swap, half, seed):
    def case(dtype):
        g = torch.Generator().manual_seed(seed)
        p, ch, k = 4, 8, 48
        m = p * ch
        state, img = F.mf_couple_fwd(_rand(g, (batch, k), dtype), _rand(g, (2 * m, k), dtype, k ** -0.5), _rand(g, (2 * m,), torch.float32, 0.3),
                                     _rand(g, (2 * ch,), torch.float32, 0.1, 1.0), _rand(g, (2 * ch,), torch.float32, 0.3),
                                     _rand(g, (batch, p, 2 * ch), torch.float32), p, swap, img_half=half)
        return {"state": state, "img": img}
    return case


def _atom(max_wg):
    def case(dtype):
        g = torch.Generator().manual_seed(150)
        b, n, t, gnn, lin, flows = 33, 9, 5, (64,), (96, 40), 3
        kg, d1, d2, d3 = 32, 64, 96, 64
        w16 = _rand(g, (flows, d1 * kg + d2 * d1 + d3 * d2 + 32 * d3), dtype, 0.1)
        p32 = _rand(g, (flows, 276), torch.float32, 0.1)
        p32[:, d1 + d2 + d3 + 32:d1 + d2 + d3 + 32 + n] += 1.0             # ActNorm's scale: a divisor
        z = _rand(g, (b, n * t), torch.float32)
        mask = torch.randint(0, 16, (b, n, n), generator=g).to(torch.uint8).to(DEV)
        return {"x": F.mf_atom_reverse_fwd(z, mask, w16, p32, n, t, gnn, lin, 1, True, max_workgroups=max_wg)}
    return case


def _txl(dtype):
    g = torch.Generator().manual_seed(160)
    b, heads, qlen, mlen, cap = 2, 2, 33, 16, 64
    h = heads * 64
    return {"ctx": F.txl_rel_attention_fwd(_rand(g, (b * qlen, h), dtype), _rand(g, (heads, 64), dtype, 0.3), _rand(g, (heads, 64), dtype, 0.3),
                                           _rand(g, (b, cap, 2 * h), dtype), _rand(g, (qlen + mlen, h), dtype), heads, qlen, mlen, 5,
                                           qlen + mlen, 0.125)}


def _dot_fwd(dtype):
    g = torch.Generator().manual_seed(170)
    return {"y": F.dot_interact_fwd(_rand(g, (5, 27, 128), dtype))}


def _dot_bwd(dtype):
    g = torch.Generator().manual_seed(171)
    x = _rand(g, (5, 27, 128), dtype)
    grad, mlp_grad = F.dot_interact_bwd(x, _rand(g, (5, F.dot_interact_out_width(27, 128)), dtype))
    return {"grad": grad, "mlp_grad": mlp_grad}


def _attn_varlen(dtype):
    g = torch.Generator().manual_seed(180)
    lens = (130, 33)
    cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=DEV)
    return {"ctx": F.attention_fwd_varlen(_rand(g, (sum(lens), 192), dtype, 0.7), cu, max(lens), 1, 0.125)}


def _attn_s256(dtype):
    g = torch.Generator().manual_seed(181)
    mask_add = torch.zeros(1, 256, device=DEV)
    mask_add[0, 200:] = -10000.0
    ctx, stats, _ = F.attention_fwd(_rand(g, (256, 192), dtype, 0.7), mask_add, 1, 256, 1, 0.125)
    return {"ctx": ctx, "stats": stats[..., :2]}


CASES = {"grn_ctx": _grn_ctx, "grn_gate": _grn_gate, "grn_index_q": _grn_index_q, "grn_row1": _grn_row1,
         "vsn_f1": _vsn(1, (1,), False, 110), "vsn_f8": _vsn(8, (3, 3, 2), True, 111), "lstm": _lstm, "tft_attn": _tft_attn,
         "ncf_b100_wg2": _ncf(100, 2, 140), "ncf_b33": _ncf(33, 0, 141), "couple_b129": _couple(129, 0, 1, 149),
         "atom_wg1": _atom(1), "atom_wg0": _atom(0), "txl": _txl, "dot_fwd": _dot_fwd, "dot_bwd": _dot_bwd,
         "attn_varlen": _attn_varlen, "attn_s256": _attn_s256}
for _s in (0, 1):
    for _h in (0, 1):
        CASES["couple_s%d_h%d" % (_s, _h)] = _couple(33, _s, _h, 145 + 2 * _s + _h)


def digests(name, dtype):
    out = CASES[name](dtype)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in out.items()}
