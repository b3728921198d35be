"""float64 statements, error bars, input generators and tensor-list layouts for the multi-tensor optimizer kernels
(deeplearningexamples_amd/csrc/multi_tensor.hip).  tests/ only: no GPU and no ctypes in here.

STATEMENTS.  One function per kernel, elementwise on flat tensors (a caller hands over the concatenation of a tensor list and,
where a kernel reads a per-tensor scalar, the tensor index of every element).  Inputs are the exact stored values: 16-bit
gradients and fp32 state widened to float64, host scalars as the fp32 the C ABI's `float` parameters carry (f32()).  Sources, as
multi_tensor.hip cites them: multi_tensor_l2norm_kernel.cu, multi_tensor_lamb.cu:43-368, torch.optim.SGD / Adam, apex FusedAdam,
models/common.py:191-212 (EMA, whose contract is bit-identity with the two torch ops, so its reference IS those two ops).

BARS.  Every value travels as an R = (float64 value, bound on |fp32 evaluation - value|): a running-error analysis of the kernel's
own statement.  rn() is one fp32 rounding: it adds 2^-24 (|value| + incoming error); products, quotients and square roots carry
the incoming errors through with their exact (not first-order) bounds.  Unrolled, the bar of an output is k 2^-24 sum|terms| of
the expression that produces it, k = the roundings on the longest path, counted in a comment where each output is formed.  fp32
`/` and sqrtf are correctly rounded (no fast-math); contraction to FMA only removes roundings; multiplying or dividing by exactly
1 and adding exactly 0 are exact and take none.  An output stored in 16 bits adds half an ulp of that format at |value| + bar.

NORMS.  All terms are non-negative, so the bar is relative: depth 2^-24 on the sum of squares, halved by the square root, plus
the root's own rounding.  depth = the longest chain of fp32 roundings one element's square can pass through (norm_depth()).
None of these numbers comes from a GPU run.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}
MT_BLOCK = 512                      # workgroup size of every multi-tensor kernel


def f32(x):
    """A host scalar as the kernel receives it through a C `float` parameter."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------- running error
class R:
    """value (float64) and a bound on the distance of an fp32 evaluation from it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64)


def _r(x):
    return x if isinstance(x, R) else R(x)


def _const(x, c):
    if c == 0.0:
        return bool((x.v == 0).all()) and bool((x.e == 0).all())
    return x.v.numel() == 1 and float(x.e) == 0.0 and float(x.v) == c


def rn(x):
    """one fp32 rounding of x (normal range)"""
    return R(x.v, x.e + U * (x.v.abs() + x.e))


def mul(a, b):
    a, b = _r(a), _r(b)
    if _const(a, 1.0):
        return b
    if _const(b, 1.0):
        return a
    if _const(a, 0.0) or _const(b, 0.0):
        return R(torch.zeros(torch.broadcast_shapes(a.v.shape, b.v.shape), dtype=F64))
    return rn(R(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e))


def add(a, b, sign=1.0):
    a, b = _r(a), _r(b)
    if _const(b, 0.0):
        return a
    if _const(a, 0.0) and sign == 1.0:
        return b
    return rn(R(a.v + sign * b.v, a.e + b.e))


def sub(a, b):
    return add(a, b, -1.0)


def div(a, b):
    a, b = _r(a), _r(b)
    if _const(b, 1.0):
        return a
    lo = b.v.abs() - b.e
    assert bool((lo > 0).all()), "a denominator's bar reaches zero"
    q = a.v / b.v
    return rn(R(q, (a.e + q.abs() * b.e) / lo))


def sqrt(a):
    a = _r(a)
    assert bool((a.v - a.e >= 0).all()), "a radicand's bar reaches below zero"
    s = torch.sqrt(a.v)
    lo = torch.sqrt(a.v - a.e)
    return rn(R(s, torch.where(a.e > 0, a.e / (s + lo).clamp_min(1e-300), torch.zeros_like(s))))


def one_minus_pow(beta, step):
    """(float)(1.0 - pow((double)beta, (double)step)): evaluated in double, rounded once (2^-48: the double pow's own error)."""
    v = 1.0 - f32(beta) ** int(step)
    return R(v, (U + 2.0 ** -48) * abs(v))


def ulp(v, dtype):
    """Spacing of `dtype` at |v| (float64), the subnormal spacing at and near 0."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(EMIN[dtype]).double() - MANT[dtype])


def stored(x, dtype):
    """(value, bar) of R `x` once it is stored in `dtype`: fp32 adds nothing (the last rn() was the store), 16 bits add half an
    ulp of the format at the far end of the bar."""
    if dtype == torch.float32:
        return x.v, x.e
    return x.v, x.e + 0.5 * ulp(x.v.abs() + x.e, dtype)


def subnormal(v, dtype):
    """elements of the float64 reference `v` that are non-zero and below the smallest normal of `dtype`"""
    return (v != 0) & (v.abs() < 2.0 ** EMIN[dtype])


def widen(t):
    return t.detach().cpu().to(F64)


# ---------------------------------------------------------------------------------------------- L2 norm
def norm_depth(chunk, nchunks):
    """Longest chain of fp32 roundings between one element's square and the sum the square root is taken of.
    mt_l2norm_partial / mt_lamb_stage1<NORMS>, one workgroup of 512 lanes per chunk:
      4   the 4-element group of mt_sumsq4: v0*v0 is rounded, then three fused multiply-adds round once each;
      T   `s + t`, once per trip of the lane's loop: T = ceil(chunk / (4 * 512)) trips, the first group rides through all of them;
      1   the ragged tail (len4 .. len, at most 3 elements, one per lane): `s += v * v` after the trips (its own element takes
          2, product and sum, fewer than the chain it closes);
      6   wave_sum: the xor-shuffle tree over 64 lanes;
      8   block_sum: the serial fold `t += red[i]` over the 512 / 64 = 8 waves (red[0] rides through all 8);
    mt_l2norm_finish / mt_lamb_norms_finish, one workgroup per output:
      F   `s += partial[i]`, stride 512: F = ceil(nchunks / 512) (at least 1);
      6 + 8  wave_sum and block_sum again.
    """
    trips = -(-int(chunk) // (4 * MT_BLOCK))
    fold = max(1, -(-int(nchunks) // MT_BLOCK))
    return 4 + trips + 1 + 6 + 8 + fold + 6 + 8


def norm_rel_bar(chunk, nchunks):
    """Relative bar of sqrtf(sum): sum (1 + d), |d| <= depth u (1 + depth u) covers the second order; the root halves it
    (sqrt(1 + d) <= 1 + d / 2) and rounds once."""
    d = norm_depth(chunk, nchunks) * U
    return 0.5 * d * (1.0 + d) + U * (1.0 + d)


def ref_l2norm(tensors, chunk):
    """-> total, total_bar, per[n], per_bar[n]  (float64; multi_tensor_l2norm_kernel.cu: sqrt of the sum of squares, globally and
    per tensor).  `tensors`: the stored tensors (any float dtype, any device)."""
    ss = torch.tensor([float((widen(t) ** 2).sum()) for t in tensors], dtype=F64)
    nch = [-(-t.numel() // chunk) for t in tensors]
    per = torch.sqrt(ss)
    per_bar = per * torch.tensor([norm_rel_bar(chunk, c) for c in nch], dtype=F64)
    total = math.sqrt(float(ss.sum()))
    return total, total * norm_rel_bar(chunk, sum(nch)), per, per_bar


# ---------------------------------------------------------------------------------------------- LAMB
def ref_lamb_stage1(g, p, m, v, gdtype, *, beta1, beta2, beta3, step, bias_correction, eps, mode, decay, ggn, mgn, inv_scale):
    """multi_tensor_lamb.cu:43-245.  g (stored in gdtype), p, m, v: flat float64.  ggn, mgn, inv_scale: the device words' values.
    -> {"g": (update, bar), "m": ..., "v": ...}"""
    b1, b2, b3, eps, decay = f32(beta1), f32(beta2), f32(beta3), f32(eps), f32(decay)
    b1c, b2c = (one_minus_pow(b1, step), one_minus_pow(b2, step)) if bias_correction == 1 else (R(1.0), R(1.0))
    clip = div(ggn, mgn) if ggn > mgn else R(1.0)                   # :79, 1 rounding when active
    omb2 = sub(1.0, b2)                                             # 1.f - beta2
    sg = div(mul(g, inv_scale), clip)                               # 2 (+1 clip)
    dp = mul(decay, p)                                              # 1; exactly 0 without decay (p is not even read)
    if mode == 0:
        sg = add(sg, dp)                                            # L2 mode: 1 more on the gradient
    m2 = add(mul(m, b1), mul(b3, sg))                               # m: 2 + path(sg) <= 2 + 5 = 7
    v2 = add(mul(v, b2), mul(mul(omb2, sg), sg))                    # v: 1 (omb2) + 3 + 2 path(sg) <= 4 + 10 = 14
    mh, vh = div(m2, b1c), div(v2, b2c)                             # +1 (b1c) +1, +1 (b2c) +1
    upd = div(mh, add(sqrt(vh), eps))                               # numerator 9, denominator 16 / 2 + 2: <= 20 in all
    if mode != 0:
        upd = add(upd, dp)                                          # AdamW mode: +1
    return {"g": stored(upd, gdtype), "m": (m2.v, m2.e), "v": (v2.v, v2.e)}


def ref_lamb_stage2(u, p, tid, pn, un, *, lr, decay, use_nvlamb):
    """multi_tensor_lamb.cu:251-368.  u: the STORED update (widened), p: flat float64, tid: tensor index per element (int64), pn /
    un: the per-tensor norm words' values [n] (float64), lr: the device word's value.  -> {"p": (value, bar)}"""
    n = pn.numel()
    ratio = R(torch.full((n,), float(lr), dtype=F64))
    if use_nvlamb or f32(decay) != 0.0:                             # :277-282
        ok = (un != 0) & (pn != 0)
        q = mul(lr, div(pn, torch.where(ok, un, torch.ones_like(un))))      # 2 roundings
        ratio = R(torch.where(ok, q.v, ratio.v), torch.where(ok, q.e, ratio.e))
    r = R(ratio.v[tid], ratio.e[tid])
    p2 = sub(p, mul(r, u))                                          # p: 2 + 2 = 4
    return {"p": (p2.v, p2.e)}


# ---------------------------------------------------------------------------------------------- SGD
def ref_sgd(g, p, buf, *, lr, momentum, dampening, wd, nesterov, first_step, inv_scale, has_momentum):
    """torch.optim.SGD: d = g * inv_scale + wd * p; buf = first ? d : mom * buf + (1 - damp) * d; d = nesterov ? d + mom * buf :
    buf; p -= lr * d.  lr / inv_scale: the fp32 values the kernel reads (device word or host float).  -> {"p", "buf"}"""
    mom, damp, wd = f32(momentum), f32(dampening), f32(wd)
    d = add(mul(g, inv_scale), mul(wd, p))                          # 3
    out = {}
    if has_momentum:
        b = d if first_step else add(mul(mom, buf), mul(sub(1.0, damp), d))     # buf: 3 + (1 + 1 + 1) = 6
        d = add(d, mul(mom, b)) if nesterov else b                  # +2
        out["buf"] = (b.v, b.e)
    p2 = sub(p, mul(lr, d))                                         # p: 8 + 2 = 10 at most
    out["p"] = (p2.v, p2.e)
    return out


# ---------------------------------------------------------------------------------------------- Adam
def ref_adam(g, p, m, v, *, lr, beta1, beta2, eps, wd, step, inv_scale, gnorm, max_norm):
    """GradScaler.unscale_ + clip_grad_norm_ + torch.optim.Adam.step as mt_adam states them.  gnorm None / max_norm <= 0: no
    clip.  -> {"p", "m", "v"}"""
    b1, b2, eps, wd, mx = f32(beta1), f32(beta2), f32(eps), f32(wd), f32(max_norm)
    gs = R(float(inv_scale))
    if gnorm is not None and mx > 0.0:
        coef = div(mx, add(mul(gnorm, inv_scale), f32(1e-6)))       # 3
        assert abs(float(coef.v) - 1.0) > 1e-3, "the clip decision must not hang on a rounding"
        if float(coef.v) < 1.0:
            gs = mul(inv_scale, coef)                               # 4
    gr = add(mul(g, gs), mul(wd, p))                                # 4 + 2 = 6
    m2 = add(mul(b1, m), mul(sub(1.0, b1), gr))                     # m: 6 + 3 = 9
    v2 = add(mul(b2, v), mul(mul(sub(1.0, b2), gr), gr))            # v: 12 + 4 = 16
    bc1, bc2 = one_minus_pow(b1, step), one_minus_pow(b2, step)
    step_size = div(lr, bc1)                                        # 2
    rsq = div(1.0, sqrt(bc2))                                       # 3
    den = add(mul(sqrt(v2), rsq), eps)                              # 16 / 2 + 1 + 3 + 1 + 1 = 14
    p2 = sub(p, div(mul(step_size, m2), den))                       # p: 9 + 2 + 1 + 14 + 1 + 1 = 28 at most
    return {"p": (p2.v, p2.e), "m": (m2.v, m2.e), "v": (v2.v, v2.e)}


def ref_adam_copy(g, p, m, v, tid, *, lr, beta1, beta2, eps, step, inv_scale, tensor_mul):
    """apex FusedAdam (bias_correction, weight_decay 0): m = b1 m + (1 - b1) grad; v = b2 v + (1 - b2) grad^2;
    p -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps), grad = g * inv_scale * tensor_mul[tensor].  -> {"p", "m", "v"}"""
    b1, b2, eps = f32(beta1), f32(beta2), f32(eps)
    if tensor_mul is None:
        gs = R(float(inv_scale))
    else:
        s = mul(float(inv_scale), tensor_mul)                       # 1
        gs = R(s.v[tid], s.e[tid])
    gr = mul(g, gs)                                                 # 2
    m2 = add(mul(b1, m), mul(sub(1.0, b1), gr))                     # m: 2 + 3 = 5
    v2 = add(mul(b2, v), mul(mul(sub(1.0, b2), gr), gr))            # v: 4 + 4 = 8
    bc1, bc2 = one_minus_pow(b1, step), one_minus_pow(b2, step)
    den = add(sqrt(div(v2, bc2)), eps)                              # (8 + 2) / 2 + 2 = 7
    p2 = sub(p, mul(lr, div(div(m2, bc1), den)))                    # p: 5 + 2 + 7 + 1 + 1 + 1 = 17 at most
    return {"p": (p2.v, p2.e), "m": (m2.v, m2.e), "v": (v2.v, v2.e)}


# ---------------------------------------------------------------------------------------------- EMA
def ref_ema(x, e, mu, one_minus_mu=None):
    """models/common.py:191-212 on fp32 CPU tensors: `e.mul_(mu); e.add_((1 - mu) * x)`, 1 - mu taken in double.  -> e' (fp32)"""
    omm = 1.0 - float(mu) if one_minus_mu is None else float(one_minus_mu)
    out = e.detach().cpu().clone()
    out.mul_(float(mu))
    out.add_(omm * x.detach().cpu())
    return out


# ---------------------------------------------------------------------------------------------- length sets
def RAGGED(chunk):
    """all four tail lengths, exact / under-full / over-full chunks, a multi-chunk tensor with a ragged last chunk, an empty tensor
    in the middle"""
    return [1, 2, 3, 5, 7, 8, chunk - 1, chunk, chunk + 1, chunk + 3, 2 * chunk + 2, 0, 4, 6]


def _many():
    n = np.random.default_rng(419).integers(0, 5001, 419).tolist()
    n[0] = n[-1] = 0
    n[200] = n[201] = n[202] = 0
    return [int(x) for x in n]


MANY = _many()                       # 419 tensors (odd, no power of two), empties first, last and three in a row
DEGENERATE = {"n1": [5], "n2": [0, 7], "n3": [3, 0, 2050]}


def tensor_index(lengths):
    return torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- inputs
def gaussian(seed, n, scale=1.0, dtype=torch.float32, floor=None):
    """N(0, scale^2) with both signs, stored in `dtype`; floor: |N| + floor instead (second moments: non-negative, away from 0)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=F64) * scale
    if floor is not None:
        x = x.abs() + floor
    return x.to(torch.float32).to(dtype)


SEED = {"l2norm": 11, "lamb_stage1": 12, "lamb_stage2": 13, "sgd": 14, "adam": 15, "adam_copy": 16, "ema": 17}
V_FLOOR = 2e-2                       # second moments stay above every eps in use (1e-2 the largest)


def make_inputs(kernel, n, gdtype=torch.float32):
    """The flat stored inputs of `kernel` for a table of n elements in all (one fixed seed per kernel and list)."""
    s = SEED[kernel] * 100
    if kernel == "l2norm":
        return {"x": gaussian(s, n, 1.0, gdtype)}
    if kernel == "lamb_stage1":      # gradients as under a loss scale of 128
        return {"g": gaussian(s, n, 12.8, gdtype), "p": gaussian(s + 1, n), "m": gaussian(s + 2, n, 0.05),
                "v": gaussian(s + 3, n, 0.01, floor=V_FLOOR)}
    if kernel == "lamb_stage2":
        return {"u": gaussian(s, n, 1.0, gdtype), "p": gaussian(s + 1, n)}
    if kernel == "sgd":
        return {"g": gaussian(s, n, 1.0, gdtype), "p": gaussian(s + 1, n), "buf": gaussian(s + 2, n, 0.5)}
    if kernel in ("adam", "adam_copy"):
        return {"g": gaussian(s, n, 64.0), "p": gaussian(s + 1, n), "m": gaussian(s + 2, n, 0.05),
                "v": gaussian(s + 3, n, 0.01, floor=V_FLOOR)}
    if kernel == "ema":
        return {"x": gaussian(s, n, 2.0), "e": gaussian(s + 1, n, 2.0)}
    raise KeyError(kernel)


def stage1_cfg(**over):
    """clip active: ||g|| = 300 against a limit of 128 (both in loss-scaled units); inactive: ggn=30."""
    c = dict(beta1=0.9, beta2=0.999, beta3=0.1, step=4, bias_correction=1, eps=1e-6, mode=1, decay=0.01, ggn=300.0, mgn=128.0,
             inv_scale=1.0 / 128.0)
    c.update(over)
    return c


def sgd_cfg(**over):
    c = dict(lr=0.1, momentum=0.875, dampening=0.0, wd=3.0517578125e-05, nesterov=False, first_step=False, inv_scale=0.25,
             has_momentum=True)
    c.update(over)
    return c


def adam_cfg(**over):
    """clip active: ||g|| = 2000 * 128 scaled against max_norm 1000 -> coef ~ 0.5; inactive: gnorm=12800 (coef ~ 10)."""
    c = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, wd=1e-6, step=3, inv_scale=1.0 / 128.0, gnorm=256000.0, max_norm=1000.0)
    c.update(over)
    return c


def adam_copy_cfg(**over):
    c = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3, inv_scale=1.0 / 128.0, tensor_mul=None)
    c.update(over)
    return c


# ---------------------------------------------------------------------------------------------- layouts
GUARD = 64                           # guard elements before the first and after every tensor: a multiple of 16 bytes in every dtype
SENTINEL = {4: 0x5A5AA5A5, 2: 0x5A5A}
_INT = {4: torch.int32, 2: torch.int16}
LAYOUTS = ("aligned", "packed", "grad_packed", "state_packed", "copy_half")


def _offsets(lengths, present, esize, mode):
    """element offsets of the tensors inside one arena (whose base is 16-byte aligned) and the arena's length"""
    per16 = 16 // esize
    offs, at, rank = [], GUARD, 0
    for n, has in zip(lengths, present):
        if not has:
            offs.append(None)
            continue
        if mode == "aligned":
            at = -(-at // per16) * per16
        elif mode == "half":            # 16-bit copies: every other non-empty one at 8 mod 16 (vector-legal for the copy), the rest
            assert esize == 2           # at 2 mod 8 (the whole chunk goes element by element)
            want = 4 if rank % 2 == 0 else 1
            rank += 1 if n else 0
            at = -(-at // per16) * per16 + want
        offs.append(at)
        at += n
        if mode != "packed":
            at += GUARD
    return offs, at + GUARD


class Layout:
    """Tensor lists cut out of one sentinel-filled arena per list.  lists[l][t]: the view (None for an absent optional entry)."""

    def __init__(self, name, lengths, values, device, absent=None, copy_list=None):
        """values[l]: the flat concatenation of list l (its dtype is the list's dtype; absent tensors' elements are skipped over,
        so every list's flat tensor has sum(lengths) elements).  absent: tensor indices without an entry in `copy_list`."""
        assert name in LAYOUTS
        self.name, self.lengths, self.copy_list = name, list(lengths), copy_list
        absent = set(absent or ())
        self.arenas, self.masks, self.lists, self.spans = [], [], [], []
        starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        for l, flat in enumerate(values):
            assert flat.numel() == int(starts[-1])
            esize = flat.element_size()
            present = [not (l == copy_list and t in absent) for t in range(len(lengths))]
            packed = {"aligned": False, "packed": True, "grad_packed": l == 0, "state_packed": l != 0, "copy_half": False}[name]
            mode = "packed" if packed else ("half" if name == "copy_half" and l == copy_list else "aligned")
            offs, total = _offsets(lengths, present, esize, mode)
            host = torch.full((total,), SENTINEL[esize], dtype=_INT[esize])
            guard = torch.ones(total, dtype=torch.bool)
            src = flat.contiguous().view(_INT[esize])
            for t, (o, n) in enumerate(zip(offs, lengths)):
                if o is not None:
                    host[o:o + n] = src[starts[t]:starts[t] + n]
                    guard[o:o + n] = False
            arena = host.to(device).view(flat.dtype)
            assert arena.data_ptr() % 16 == 0, "an arena's base is not 16-byte aligned"
            self.arenas.append(arena)
            self.masks.append(guard.to(device))
            self.lists.append([None if o is None else arena[o:o + n] for o, n in zip(offs, lengths)])
            self.spans.append([(None if o is None else (o, o + n)) for o, n in zip(offs, lengths)])
        self.check_residues()

    def residues(self, l, mod=16):
        return [t.data_ptr() % mod for t in self.lists[l] if t is not None and t.numel()]

    def check_residues(self):
        """the misalignments a layout promises are really there (from data_ptr(), whatever the allocator did)"""
        many = sum(1 for n in self.lengths if n) >= 8           # the degenerate tables cannot hold every residue
        for l, arena in enumerate(self.arenas):
            res, esize = self.residues(l), arena.element_size()
            packed = {"aligned": False, "packed": True, "grad_packed": l == 0, "state_packed": l != 0, "copy_half": False}[self.name]
            if self.name == "copy_half" and l == self.copy_list:
                assert all((a == 8) if rank % 2 == 0 else (a % 8 == 2) for rank, a in enumerate(res)), res
                assert len(res) >= 2 or not many
            elif not packed:
                assert all(r == 0 for r in res), (self.name, l, res)
            elif many:
                if esize == 4:
                    assert {4, 8, 12} <= set(res), (self.name, l, sorted(set(res)))
                else:       # (2, 4, ..., 14 all occur in MANY; RAGGED's fourteen lengths reach six of the seven)
                    odd = {r for r in res if r % 4 == 2}
                    assert len(set(res) - {0}) >= (7 if len(res) >= 64 else 5) and odd, (self.name, l, sorted(set(res)))

    def guards_intact(self):
        for arena, mask in zip(self.arenas, self.masks):
            esize = arena.element_size()
            if not bool((arena.view(_INT[esize])[mask] == SENTINEL[esize]).all()):
                return False
        return True

    def flat(self, l):
        """list l read back as one flat CPU tensor (absent entries contribute nothing)"""
        vs = [v for v in self.lists[l] if v is not None]
        return torch.cat(vs).cpu() if vs else self.arenas[l][:0].cpu()


def bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over every element (0 / 0 = 0: an exact value meets a zero bar); inf when a value is not finite"""
    got = widen(got)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    return float(ratio.max())
