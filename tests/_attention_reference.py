"""Float64 statement of fused self-attention (BertSelfAttention.forward, modeling.py:340-384, and its backward in closed form),
exactly computable inputs, derived per-element bars and a CPU model of the kernels' arithmetic (tests/ only; helpers, no tests).

Shared by tests/test_attention_reference_host.py (CPU) and tests/test_gpu_attention_reference.py (MI355X); the derivation of the
bars is in the docstring of the GPU file.  Everything here runs on the CPU; heads are 64 wide (the kernels' envelope)."""
import functools
import math

import numpy as np
import torch

from tests import _exact_grid as G

U = 2.0 ** -24
D = 64
BLK = 128
NEG = -10000.0
GAP = 104.0                 # exp(-104) = 6.8e-46 < 2^-150: an fp32 exp of a difference of -104 or less is exactly 0
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
# (S, B, heads): the smallest shapes that walk the dispatch (1, 2, 3, 5 and 8 key blocks; 1, 2, 3 heads; B = 1)
SHAPES = [(128, 1, 1), (128, 3, 3), (256, 2, 3), (384, 2, 2), (640, 1, 3), (1024, 1, 2)]
BIG = (1024, 2, 16)         # selector only: chunk index (bh S + q)(S / 8) up to 2^22, byte offsets up to 12.6 MB
# valid keys per sequence for the uniform cases (0: the whole sequence is -10000); n_valid = S only where S is a power of two
PLANS = {(128, 1, 1): [[32], [1]], (128, 3, 3): [[1, 64, 0]], (256, 2, 3): [[256, 32], [0, 64]], (384, 2, 2): [[32, 64], [1, 128]],
         (640, 1, 3): [[64], [1]], (1024, 1, 2): [[1024], [32], [0]]}


def name(x):
    return {F16: "fp16", BF16: "bf16"}.get(x, str(x))


def shape_id(c):
    return "S%d-B%d-h%d" % c


def r16(x, dtype):
    """One rounding to the 16-bit type, returned in x's dtype."""
    return x.to(dtype).to(x.dtype)


def inv_keep(p):
    from oracle import philox_oracle as P
    return float(P.inv_keep(p)) if p > 0 else 1.0


@functools.lru_cache(maxsize=2)
def oracle_keep(b, nh, s, p, seed, off):
    """bool [b, nh, s, s]: the keep mask of the Philox oracle on the chunk index of the never-stored probability tensor."""
    from oracle import philox_oracle as P
    return torch.from_numpy(P.keep_mask(b * nh * s * s, p, seed, off)).view(b, nh, s, s)


def pack_keep(keep):
    """bool keep mask -> the kernels' bit-packed bytes (bit k of byte i <-> flat element 8 i + k)."""
    return torch.from_numpy(np.packbits(keep.numpy().reshape(-1), bitorder="little"))


def unpack_keep(mbytes, shape):
    return torch.from_numpy(np.unpackbits(mbytes.cpu().numpy(), bitorder="little")).view(shape).bool()


def heads(x, b, s, nh):
    """[T, nh * 64] -> [b, nh, s, 64] (a view)."""
    return x.view(b, s, nh, D).permute(0, 2, 1, 3)


def merge(x):
    """[b, nh, s, 64] -> [T, nh * 64]."""
    b, nh, s, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * s, nh * D)


def split(qkv, b, s, nh):
    h = nh * D
    return [heads(qkv[:, i * h:(i + 1) * h], b, s, nh) for i in range(3)]


# ---------------------------------------------------------------------------------------------------- the float64 statement
def reference(qkv, dctx, mask_add, keep, b, s, nh, scale, ik):
    """Closed-form float64 forward and backward of the 16-bit inputs, any additive [b, s] mask, any bool keep mask [b, nh, s, s] (or
    None).  Every tensor is [b, nh, s, ...]; M_* are the magnitude products of the bars."""
    q, k, v = [x.double() for x in split(qkv, b, s, nh)]
    do = heads(dctx, b, s, nh).double()
    sc = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask_add is not None:
        sc = sc + mask_add.double()[:, None, None, :]
    mx = sc.amax(-1)
    e = torch.exp(sc - mx[..., None])
    inv = 1.0 / e.sum(-1)
    P = e * inv[..., None]
    zero = torch.zeros((), dtype=torch.float64)
    Pd = P if keep is None else torch.where(keep, P * ik, zero)
    ctx = torch.matmul(Pd, v)
    dPd = torch.matmul(do, v.transpose(-1, -2))
    dP = dPd if keep is None else torch.where(keep, dPd * ik, zero)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None]) * scale
    r = dict(sc=sc, mx=mx, inv=inv, P=P, Pd=Pd, dP=dP, delta=delta, dS=dS, ctx=ctx, dq=torch.matmul(dS, k),
             dk=torch.matmul(dS.transpose(-1, -2), q), dv=torch.matmul(Pd.transpose(-1, -2), do), scale=scale, ik=ik, q=q, k=k, v=v, do=do)
    r["M_ctx"] = torch.matmul(Pd.abs(), v.abs())
    r["M_dq"] = torch.matmul(dS.abs(), k.abs())
    r["M_dk"] = torch.matmul(dS.abs().transpose(-1, -2), q.abs())
    r["M_dv"] = torch.matmul(Pd.abs().transpose(-1, -2), do.abs())
    return r


def bars(r, dtype, literal=False, mask_add=None):
    """Per-element bars of ctx, dq, dk, dv (derivation: tests/test_gpu_attention_reference.py) and of the row statistics.
    literal=True: the shorter formula without the three derived terms marked (+) below (recorded beside the bar, never asserted)."""
    s = r["sc"].shape[-1]
    nblk = s // BLK
    half = 2.0 ** -(G.MANT[dtype] + 1)
    sub = 0.0 if literal else 2.0 ** (G.EMIN[dtype] - G.MANT[dtype] - 1)     # (+) half the SUBNORMAL spacing: fp16 2^-25
    n = s + math.ceil(math.log2(s))
    steps = D // 16 + 1                                                       # matrix-instruction accumulations of a 64-deep sum
    eP = (3.0 * (r["sc"].abs() + r["mx"].abs()[..., None]) + 20.0) * U
    q, k, v, do = r["q"].abs(), r["k"].abs(), r["v"].abs(), r["do"].abs()
    P, dP, sc = r["P"], r["dP"].abs(), abs(r["scale"])
    cancel = U * (dP + r["delta"].abs()[..., None])
    if not literal:
        # (+) dP is itself an fp32 sum (D / 16 accumulations, one product with inv_keep) and delta an fp32 chain of S / 2 + 1 terms
        # P dP whose P carry e_P: both errors pass through (dP - delta) like the rounding of the difference does
        err_dP = steps * U * r["ik"] * torch.matmul(do, v.transpose(-1, -2))
        err_delta = (P * (eP * dP + err_dP)).sum(-1) + (s / 2 + 2) * U * (P * dP).sum(-1)
        cancel = cancel + err_dP + err_delta[..., None]
    cancel = cancel * P * sc

    def op(x):                        # the error of ONE rounding of an operand to the 16-bit type
        return torch.where(x == 0, torch.zeros_like(x), torch.clamp_min(half * x.abs(), sub))

    def fin(R, M, MeP, x, extra=0.0):
        return R + n * U * M + MeP + G.ulp16(x.to(dtype).double(), dtype) + 2 * U * x.abs() + extra

    PdE, dSE, PdR, dSR = r["Pd"].abs() * eP, r["dS"].abs() * eP, op(r["Pd"]), op(r["dS"])
    out = dict(ctx=fin(torch.matmul(PdR, v), r["M_ctx"], torch.matmul(PdE, v), r["ctx"]),
               dv=fin(torch.matmul(PdR.transpose(-1, -2), do), r["M_dv"], torch.matmul(PdE.transpose(-1, -2), do), r["dv"]),
               dq=fin(torch.matmul(dSR, k), r["M_dq"], torch.matmul(dSE, k), r["dq"], torch.matmul(cancel, k)),
               dk=fin(torch.matmul(dSR.transpose(-1, -2), q), r["M_dk"], torch.matmul(dSE.transpose(-1, -2), q), r["dk"],
                      torch.matmul(cancel.transpose(-1, -2), q)))
    out["mx"] = 2 * U * (1.0 + r["mx"].abs())
    if not literal:
        # (+) a score is D / 16 accumulations, a product with the scale and a sum with the mask: (D / 16 + 2) u of its magnitude
        # sum |q| |k| scale + |mask|, at the keys within 1 of the maximum (no other key's computed score can become the maximum)
        msc = torch.matmul(q, k.transpose(-1, -2)) * sc + (r["sc"] - torch.matmul(r["q"], r["k"].transpose(-1, -2)) * r["scale"]).abs()
        near = r["sc"] >= r["mx"][..., None] - 1.0
        out["mx"] = (steps + 1) * U * torch.where(near, msc, torch.zeros_like(msc)).amax(-1)
    # 1 / sum: every term exp(v - max) carries e_P; the sum is a chain of 64 + 1 shuffle per key block, the online update adds a
    # product and a sum per block and a factor exp(m_old - m_new) whose exponent is below 2 A (A: largest |score| of a key that
    # contributes more than 2^-60 of the sum; a block whose keys are all below that changes the sum by less than 2^-50 of it)
    contrib = (r["sc"] - r["mx"][..., None]) > -60 * math.log(2.0)
    A = torch.where(contrib, r["sc"].abs(), torch.zeros((), dtype=torch.float64)).amax(-1)
    out["inv_rel"] = (eP * r["P"]).sum(-1) + (70.0 * nblk + (nblk - 1) * (6.0 * A + 20.0)) * U + 2.0 ** -40
    return out


def ratio(got, ref, bar):
    """Largest |got - ref| / bar and where (flat index)."""
    rt = ((got.double() - ref).abs() / bar).reshape(-1)
    i = int(torch.argmax(rt))
    return float(rt[i]), i


def block_l2(got, ref):
    """Relative L2 error per (sequence, head, 128-row block) of [b, nh, s, 64] tensors; 0 / 0 counts as 0, x / 0 as inf."""
    b, nh, s, _ = ref.shape
    en = (got.double() - ref).reshape(b, nh, s // BLK, -1).norm(dim=-1)
    rn = ref.reshape(b, nh, s // BLK, -1).norm(dim=-1)
    return torch.where(en == 0, torch.zeros_like(en), en / rn)


def block_bar(what, dtype):
    return (1.0 if what == "ctx" else 2.0) * 2.0 ** -(G.MANT[dtype] + 1)


def check_generic(out, r, dtype, what="", sink=None):
    """Every bar of part 3 on `out` (dict of [b, nh, s, 64] ctx / dq / dk / dv and [b, nh, s] mx / inv, any float dtype).  Returns
    the worst error / bar ratio of every check (also merged into `sink`, a dict of running maxima, BEFORE anything is asserted, so
    a failing run still leaves its figures); raises when one is above 1."""
    bs = bars(r, dtype)
    ratios, notes = {}, []
    for nm in ("ctx", "dq", "dk", "dv"):
        if nm not in out:
            continue
        assert bool(torch.isfinite(out[nm].double()).all()), "%s %s: non-finite" % (what, nm)
        ratios[nm], i = ratio(out[nm], r[nm], bs[nm])
        notes.append("%s: |error| / bar = %.3f at flat index %d (got %r, fp64 %r, bar %r)" % (
            nm, ratios[nm], i, float(out[nm].reshape(-1)[i]), float(r[nm].reshape(-1)[i]), float(bs[nm].reshape(-1)[i])))
        l2 = block_l2(out[nm], r[nm])
        ratios[nm + "_l2"] = float(l2.max()) / block_bar(nm, dtype)
        notes.append("%s: relative L2 of (sequence, head, block) %s is %.3g, bar %.3g" % (
            nm, tuple(torch.nonzero(l2 == l2.max())[0].tolist()), float(l2.max()), block_bar(nm, dtype)))
    if "mx" in out:
        ratios["mx"], i = ratio(out["mx"], r["mx"], bs["mx"])
        notes.append("row max: |error| / bar = %.3f at %d" % (ratios["mx"], i))
        ratios["inv"], i = ratio(out["inv"], r["inv"], bs["inv_rel"] * r["inv"])
        notes.append("1 / row sum: |error| / bar = %.3f at %d" % (ratios["inv"], i))
    lit = bars(r, dtype, literal=True)
    for nm in ("ctx", "dq", "dk", "dv", "mx"):
        if nm in out:
            ratios["lit_" + nm] = ratio(out[nm], r[nm], lit[nm])[0]
    if sink is not None:
        for k, v in ratios.items():
            sink[k] = max(sink.get(k, 0.0), v)
    bad = [n for n, k in zip(notes, ratios) if not ratios[k] <= 1.0]               # (zip stops before the lit_ entries)
    assert not bad, "%s leaves its bars: %s" % (what, "; ".join(bad))
    return ratios


# ---------------------------------------------------------------------------------------------------- exactness preconditions
def gran_log2(t):
    """Largest e with every element of t (float64) a multiple of 2^e."""
    nz = t[t != 0]
    if nz.numel() == 0:
        return 0
    m, ex = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    return int((ex.to(torch.int64) - 53 + torch.log2((mi & -mi).double()).to(torch.int64)).min())


def check_contraction(a, bm, what):
    """Precondition of a bit-exact contraction a @ bm through the matrix units: every product is a multiple of g (a power of two)
    and every sum of magnitudes is below B_MFMA in units of 16 g (check_exact's bound for its 1/16 grid): every partial sum, in any
    order, has at most 22 significant bits -- exact in fp32 with the headroom B_MFMA leaves for the matrix units' alignment."""
    g = 2.0 ** (gran_log2(a) + gran_log2(bm))
    worst = float(torch.matmul(a.abs(), bm.abs()).max())
    assert worst < G.B_MFMA * 16.0 * g, "%s: magnitude sum %g on a grid of %g: fp32 sums would not be exact" % (what, worst, g)


def check_colsum(x16, what):
    """Precondition of the exact column sums: the stored [rows, cols] values (float64) are multiples of g and every 128-row sum of
    magnitudes is below 2^20 in units of 16 g (check_exact)."""
    g = 2.0 ** gran_log2(x16)
    worst = float(x16.abs().view(-1, BLK, x16.shape[-1]).sum(1).max())
    assert worst < 2.0 ** 24 * g, "%s: column magnitude sum %g on a grid of %g" % (what, worst, g)


def colsum_ref(dqkv16):
    """float64 column sums of the stored [T, 3H] gradient per (sequence, 128-row block)."""
    return dqkv16.double().view(-1, BLK, dqkv16.shape[-1]).sum(1)


# ---------------------------------------------------------------------------------------------------- selector
class Selector:
    """Every query q has exactly one key pi(q) whose scaled score beats every other key's by at least GAP: P is exactly 0 / 1,
    inv = 1, mx = the winner's score, ctx[q] = inv_keep keep V[pi(q)], dq = dk = 0, dv[k] = the sum of inv_keep dO[q] over the kept
    q with pi(q) = k.  Rows of Q and K are two-hot codes C (e_a + e_b): scores are C^2 times the number of shared dimensions."""
    C = 32.0
    scale = 0.125

    def __init__(self, s, b, nh, dtype, seed=1, with_mask=True):
        self.s, self.b, self.nh, self.dtype = s, b, nh, dtype
        g = torch.Generator().manual_seed(seed)
        nblk = s // BLK
        pairs = torch.combinations(torch.arange(D), 2)                                   # 2016 distinct two-hot codes
        assert s <= pairs.shape[0]
        j = torch.arange(s) // 2                                                         # queries 2 j, 2 j + 1 choose the same key
        blks = torch.tensor([0, nblk // 2, nblk - 1])[j % 3]                             # first / middle / last key block
        Q, K = torch.zeros(b, nh, s, D), torch.zeros(b, nh, s, D)
        self.pi = torch.zeros(b, nh, s, dtype=torch.long)
        rows = torch.arange(s)[:, None]
        for bi in range(b):
            for h in range(nh):
                bh = bi * nh + h
                self.pi[bi, h] = blks * BLK + (37 * j + 9 * bh) % BLK
                code = pairs[torch.randperm(pairs.shape[0], generator=g)[:s]]            # [s, 2]: key k's pair
                K[bi, h][rows, code] = self.C
                Q[bi, h][rows, code[self.pi[bi, h]]] = self.C
        V = heads(G.grid((b * s, nh * D), seed + 1, torch.float32, "cpu"), b, s, nh)
        self.dctx = G.grid((b * s, nh * D), seed + 2, dtype, "cpu")
        self.qkv = torch.cat([merge(Q), merge(K), merge(V)], 1).to(dtype).contiguous()
        self.mask_add = None
        if with_mask:                                                                    # -10000 on every third key no head chose
            self.mask_add = torch.zeros(b, s)
            for bi in range(b):
                free = torch.ones(s, dtype=torch.bool)
                free[self.pi[bi].reshape(-1)] = False
                self.mask_add[bi, torch.nonzero(free).reshape(-1)[::3]] = NEG
        self.mx = 2 * self.C * self.C * self.scale
        self._check(nblk)

    def _check(self, nblk):
        s, b, nh = self.s, self.b, self.nh
        q, k, v = split(self.qkv.float(), b, s, nh)
        assert torch.equal(self.qkv.float().double() * 4, torch.round(self.qkv.float().double() * 4)), "off the k / 4 grid"
        for bi in range(b):
            for h in range(nh):
                sc = torch.matmul(q[bi, h], k[bi, h].t()) * self.scale                   # exact: multiples of 128 up to 256
                if self.mask_add is not None:
                    sc = sc + self.mask_add[bi][None, :]
                win = sc.gather(1, self.pi[bi, h][:, None])
                assert bool((win == self.mx).all()), "the chosen key's score is not the known maximum"
                rest = sc.scatter(1, self.pi[bi, h][:, None], float("-inf")).amax(1)
                assert float((win[:, 0] - rest).min()) >= GAP, "score gap below %g: P would not be exactly 0 / 1" % GAP
        pi = self.pi
        assert int(pi[0, 0].unique().numel()) < s, "pi is injective"
        qb, kb = (torch.arange(s) // BLK).expand_as(pi), pi // BLK
        if nblk > 1:
            assert bool(((qb == 0) & (kb == nblk - 1)).any()) and bool(((qb == nblk - 1) & (kb == 0)).any()), "no block crossing"
        for i in range(nblk):                                                            # every workgroup: first, middle, last block
            assert set(kb[0, 0][qb[0, 0] == i].tolist()) == {0, nblk // 2, nblk - 1}
        assert set((pi[0, 0] % 8).tolist()) == set(range(8)), "a chunk position (lane half) is never chosen"
        fan = torch.zeros(b * nh * s).index_add_(0, (pi + (torch.arange(b * nh) * s).view(b, nh, 1)).reshape(-1), torch.ones(b * nh * s))
        assert float(fan.min()) == 0, "every key is chosen"
        # sums through the matrix units: scores <= 2 C^2, dO . V <= 64 terms of 1/16 .. 1, dv <= fan-in x 2 x |dO|
        assert 2 * self.C * self.C < G.B_MFMA and 64.0 < G.B_MFMA and float(fan.max()) * 2.0 < G.B_MFMA

    def expected(self, keep, ik):
        """float64 [b, nh, s, 64] ctx, dq, dk, dv for a bool keep mask [b, nh, s, s] (or None)."""
        b, s, nh = self.b, self.s, self.nh
        v = split(self.qkv.double(), b, s, nh)[2]
        do = heads(self.dctx.double(), b, s, nh)
        kq = torch.ones(b, nh, s, dtype=torch.float64) if keep is None else keep.gather(-1, self.pi[..., None])[..., 0].double() * ik
        idx = self.pi[..., None].expand(b, nh, s, D)
        ctx = kq[..., None] * v.gather(2, idx)
        dv = torch.zeros(b, nh, s, D, dtype=torch.float64).scatter_add_(2, idx, kq[..., None] * do)
        z = torch.zeros_like(ctx)
        return dict(ctx=ctx, dq=z, dk=z, dv=dv)


# ---------------------------------------------------------------------------------------------------- uniform
def odd_n(dtype, ik):
    """The smallest n, not a power of two, at which rounding P = 1 / n to 16 bits BEFORE the dropout scale changes the stored
    dropout(P) (the planted-error case of the host test; asserted there)."""
    ik32 = torch.tensor(ik, dtype=torch.float32)
    for n in (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15):
        p32 = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
        if float((p32 * ik32).to(dtype)) != float((p32.to(dtype).float() * ik32).to(dtype)):
            return n
    raise AssertionError("no n separates the two roundings")


class Uniform:
    """Q = 0 (mirror: K = 0), the other an arbitrary k / 4 grid: every score is 0, so with mask_add = -10000 on all but n_valid
    scattered keys P = 1 / n_valid on the valid keys and exactly 0 elsewhere (a sequence that is entirely -10000: mx = -10000,
    P = 1 / S).  In every (sequence, head) dO lives on 32 of the 64 dimensions and V, on those 32, sums to 0 over the valid keys
    (each valid key paired with its negation), so delta = dO . ctx = 0 while ctx itself (the other 32 dimensions) does not vanish;
    |dP| <= 32 / 4 / 4 x ... < 16 leaves dS = P dP scale with at most 8 significant bits."""
    scale = 1.0               # scores are 0 whatever the scale; 1 keeps dS = dP / n at or above 2^-14, normal in fp16

    def __init__(self, s, b, nh, dtype, plan, mirror=False, seed=3, pair=True):
        self.s, self.b, self.nh, self.dtype, self.plan = s, b, nh, dtype, plan
        g = torch.Generator().manual_seed(seed + s + 7 * sum(plan))
        T, H = b * s, nh * D
        arb = G.grid((T, H), seed, torch.float32, "cpu")
        V = G.grid((T, H), seed + 1, torch.float32, "cpu", kmax=2)
        dO = G.grid((T, H), seed + 2, torch.float32, "cpu", kmax=2)
        self.mask_add = torch.full((b, s), NEG)
        self.valid = []
        for bi, n in enumerate(plan):
            idx = torch.sort(torch.randperm(s, generator=g)[:n if n else s]).values
            if n:
                self.mask_add[bi, idx] = 0.0
            self.valid.append(idx)
            rows = bi * s + idx
            for h in range(nh):
                dims = torch.randperm(D, generator=g)
                on, off = h * D + dims[:32], h * D + dims[32:]
                dO[bi * s:(bi + 1) * s, off] = 0.0
                if not pair:
                    continue
                if idx.numel() == 1:
                    V[rows[:, None], on[None, :]] = 0.0
                else:
                    assert idx.numel() % 2 == 0
                    V[rows[1::2, None], on[None, :]] = -V[rows[0::2, None], on[None, :]]
        zero = torch.zeros(T, H)
        self.qkv = torch.cat([arb if mirror else zero, zero if mirror else arb, V], 1).to(dtype).contiguous()
        self.dctx = dO.to(dtype)
        self.n = torch.tensor([float(n if n else s) for n in plan])
        self.mx = torch.tensor([0.0 if n else NEG for n in plan])

    def pd16(self, keep, ik):
        """dropout(P) as stored (float64 of the 16-bit values): fp32 1 / n, fp32 product with inv_keep, one rounding."""
        b, s, nh = self.b, self.s, self.nh
        inv32 = torch.tensor(1.0, dtype=torch.float32) / self.n.float()
        P = torch.zeros(b, nh, s, s, dtype=torch.float32)
        for bi in range(b):
            P[bi][:, :, self.valid[bi]] = inv32[bi]
        Pd = P if keep is None else torch.where(keep, P * torch.tensor(ik, dtype=torch.float32), torch.zeros((), dtype=torch.float32))
        return Pd.to(self.dtype).double(), inv32

    def expected_fwd(self, keep, ik):
        """Exact forward: float64 ctx [b, nh, s, 64] (before its one rounding), fp32 mx and inv [b]."""
        Pd, inv32 = self.pd16(keep, ik)
        v = split(self.qkv.double(), self.b, self.s, self.nh)[2]
        check_contraction(Pd, v, "uniform ctx")
        return dict(ctx=torch.matmul(Pd, v), mx=self.mx, inv=inv32)

    def expected_bwd(self):
        """Exact backward for p = 0 and n_valid a power of two, with its preconditions: float64 dq, dk, dv [b, nh, s, 64]."""
        b, s, nh = self.b, self.s, self.nh
        r = reference(self.qkv, self.dctx, self.mask_add, None, b, s, nh, self.scale, 1.0)
        assert all(math.log2(float(n)).is_integer() for n in self.n), "n_valid is not a power of two"
        assert float(r["delta"].abs().max()) == 0.0, "delta is not exactly 0"
        assert float(r["dP"].abs().max()) < 16.0, "|dP| reaches 16"
        assert torch.equal(r["dS"].to(BF16).double(), r["dS"]) and torch.equal(r["dS"].to(F16).double(), r["dS"]), \
            "dS has more than 8 significant bits (or is subnormal in fp16)"
        assert torch.equal(r["P"].to(self.dtype).double(), r["P"])
        check_contraction(r["do"], r["v"].transpose(-1, -2), "uniform dP")
        check_contraction(r["P"], r["dP"].transpose(-1, -2), "uniform delta")
        check_contraction(r["dS"], r["k"], "uniform dq")
        check_contraction(r["dS"].transpose(-1, -2), r["q"], "uniform dk")
        check_contraction(r["P"].transpose(-1, -2), r["do"], "uniform dv")
        for bi, n in enumerate(self.plan):                         # rows of dk / dv at padded keys: exactly 0
            if n:
                pad = torch.ones(s, dtype=torch.bool)
                pad[self.valid[bi]] = False
                assert float(r["dk"][bi][:, pad].abs().max() if pad.any() else 0.0) == 0.0
                assert float(r["dv"][bi][:, pad].abs().max() if pad.any() else 0.0) == 0.0
        return r


def same(got, want, dtype, what):
    """Bit-exact bar: the stored values equal the float64 expectation rounded once (as values: +0 and -0 are equal)."""
    G.assert_same(got.double(), want.to(dtype).double(), what)


def check_selector(out, case, keep, ik, what):
    """`out`: [b, nh, s, 64] ctx / dq / dk / dv (those present) and [b, nh, s] mx / inv, from the kernels or the CPU model."""
    exp = case.expected(keep, ik)
    for nm in ("ctx", "dq", "dk", "dv"):
        if nm in out:
            same(out[nm], exp[nm], case.dtype, "%s %s" % (what, nm))
    G.assert_same(out["mx"].double(), torch.full_like(out["mx"].double(), case.mx), what + " row max")
    G.assert_same(out["inv"].double(), torch.ones_like(out["inv"].double()), what + " 1 / row sum")


def check_uniform_fwd(out, case, keep, ik, what):
    exp = case.expected_fwd(keep, ik)
    same(out["ctx"], exp["ctx"], case.dtype, what + " ctx")
    G.assert_same(out["mx"].double(), exp["mx"].double()[:, None, None].expand_as(out["mx"]).contiguous(), what + " row max")
    G.assert_same(out["inv"].double(), exp["inv"].double()[:, None, None].expand_as(out["inv"]).contiguous(), what + " 1 / row sum")


def check_uniform_bwd(out, case, what):
    """p = 0, n_valid powers of two: dq, dk, dv bit for bit (the rows of dk / dv at padded keys are exactly 0)."""
    r = case.expected_bwd()
    for nm in ("dq", "dk", "dv"):
        same(out[nm], r[nm], case.dtype, "%s %s" % (what, nm))
    return r


# ---------------------------------------------------------------------------------------------------- generic inputs
def scattered_mask(b, s, seed):
    """[b, s] additive mask: sequence 0 unmasked, the others with a quarter / a half of their keys (scattered) at -10000."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(b, s)
    for bi in range(1, b):
        m[bi, torch.randperm(s, generator=g)[:(s // 4) * min(bi, 2)]] = NEG
    if b == 1:
        m[0, torch.randperm(s, generator=g)[:s // 8]] = NEG
    return m


def generic_inputs(s, b, nh, dtype, sigma, seed=5):
    g = torch.Generator().manual_seed(seed + s + b)
    qkv = (torch.randn(b * s, 3 * nh * D, generator=g) * sigma).to(dtype)
    dctx = (torch.randn(b * s, nh * D, generator=g) * 0.5).to(dtype)
    return qkv, dctx, scattered_mask(b, s, seed + 1)


# ---------------------------------------------------------------------------------------------------- CPU model of the kernels
FAULTS = ("swap_keys", "skip_block", "mask_halves", "chunk_row", "round_before", "stale_max")


def _mm(a, bm, order):
    """fp32 contraction the way a 16-deep matrix instruction accumulates: the 16 products of a slice of the contraction index enter
    exactly, the accumulator is rounded to fp32 once per slice; slices from the first to the last (order 0) or back (order 1)."""
    acc = torch.zeros(a.shape[:-1] + bm.shape[-1:], dtype=torch.float32)
    cs = range(0, a.shape[-1], 16)
    for c in (cs if order == 0 else reversed(cs)):
        acc = (acc.double() + torch.matmul(a[..., c:c + 16].double(), bm[..., c:c + 16, :].double())).float()
    return acc


def _exp(x):
    e = torch.exp(x)
    return torch.where(e < 2.0 ** -126, torch.zeros((), dtype=torch.float32), e)      # v_exp_f32 flushes subnormal results


def kernel_model(qkv, dctx, mask_add, keep, b, s, nh, scale, ik, order=0, fault=None):
    """The kernels' arithmetic on the CPU: an fp32 softmax (one pass at S = 128, blocked online max / sum over 128-key blocks above)
    whose dropout(P) and dS are rounded once to the 16-bit type, fp32 sums in one of two orders.  `fault` plants one error.
    -> float32 [b, nh, s, 64] ctx, dq, dk, dv (the stored 16-bit values) and [b, nh, s] mx, inv."""
    dtype = qkv.dtype
    q, k, v = [x.float() for x in split(qkv, b, s, nh)]
    do = heads(dctx, b, s, nh).float()
    sc32, ik32 = torch.tensor(scale, dtype=torch.float32), torch.tensor(ik, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    x = _mm(q, k.transpose(-1, -2), order) * sc32
    if mask_add is not None:
        m = mask_add.float()
        if fault == "mask_halves":
            m = m[:, torch.arange(s) ^ 4]
        x = x + m[:, None, None, :]
    if s == BLK:
        mx = x.amax(-1)
        e = _exp(x - mx[..., None])
        l = e.sum(-1) if order == 0 else e.flip(-1).sum(-1)
    else:
        mx = torch.full(x.shape[:-1], float("-inf"))
        l = torch.zeros(x.shape[:-1])
        for j in range(s // BLK):
            xb = x[..., j * BLK:(j + 1) * BLK]
            m_new = torch.maximum(mx, xb.amax(-1))
            e = _exp(xb - m_new[..., None])
            sm = e.sum(-1) if order == 0 else e.flip(-1).sum(-1)
            f = torch.ones_like(l) if fault == "stale_max" else _exp(mx - m_new)
            l = l * f + sm
            mx = m_new
    inv = 1.0 / l
    P = _exp(x - mx[..., None]) * inv[..., None]
    if keep is not None and fault == "chunk_row":
        keep = torch.roll(keep, -1, 2)
    if keep is None:
        Pd32 = P
    elif fault == "round_before":
        Pd32 = torch.where(keep, r16(P, dtype) * ik32, zero)
    else:
        Pd32 = torch.where(keep, P * ik32, zero)
    Pd = r16(Pd32, dtype)
    Pf = Pd
    if fault == "swap_keys":                                       # keys 1 and 2 of every 8-key chunk exchanged for the P V product
        kk = torch.arange(s)
        kk = torch.where(kk % 8 == 1, kk + 1, torch.where(kk % 8 == 2, kk - 1, kk))
        Pf = Pd[..., kk]
    if fault == "skip_block" and s > BLK:
        Pf = Pd.clone()
        Pf[..., BLK:2 * BLK] = 0.0
    out = dict(mx=mx, inv=inv, ctx=r16(_mm(Pf, v, order), dtype))
    dPd = _mm(do, v.transpose(-1, -2), order)
    dP = dPd if keep is None else torch.where(keep, dPd * ik32, zero)
    pdp = P * dP
    delta = pdp.sum(-1) if order == 0 else pdp.flip(-1).sum(-1)
    dS = r16(P * (dP - delta[..., None]) * sc32, dtype)
    out["dq"] = r16(_mm(dS, k, order), dtype)
    out["dk"] = r16(_mm(dS.transpose(-1, -2), q, order), dtype)
    out["dv"] = r16(_mm(Pd.transpose(-1, -2), do, order), dtype)
    return out
