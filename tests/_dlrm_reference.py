"""float64 statements, error bars, inputs and case tables for the DLRM sparse-side kernels (csrc/dot_interact.hip, embedding.hip,
emb_onehot.hip and the BCE loss of elementwise.hip).  tests/ only: no GPU and no ctypes in here.

STATEMENTS.  Plain restatements of each operation on the exact stored inputs (16-bit values widened to float64), nothing rounded
before the end.  Sources as the kernels cite them: dlrm/nn/interactions.py:50-82 and dot_based_interact_fp32_bwd.cu:93-169 (the
interaction and its gradient), dlrm/nn/embeddings.py:123-137 (floor-mod hashing, offsets, the gather), gather_gpu.cu:53-75 (the
sparse SGD: duplicates of a row add), torch.nn.BCEWithLogitsLoss(mean) and its derivative.

BARS.  Two kinds, neither taken from a kernel's output.
  * exact: inputs k / 4 (tests/_exact_grid.py).  Every product is a multiple of 1/16 and every sum of magnitudes stays far below
    2^18, so an fp32 accumulation is exact in any order and the output is the float64 value rounded ONCE (round_once()).
  * derived: |error| <= half an ulp of a 16-bit output at the reference value + gamma(n) sum|terms|, gamma(n) = n u / (1 - n u),
    u = 2^-24, n = the additions into the element + 2 (the standard bound of an fp32 sum of n terms in ANY order).
"""
import functools

import torch

from tests._exact_grid import B_MFMA, check_exact, gen, grid, ulp16

F64 = torch.float64
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U = 2.0 ** -24


def name(dt):
    return str(dt).split(".")[1]


def widen(t):
    return t.detach().cpu().to(F64)


def round_once(v, dtype):
    """The float64 value rounded once to `dtype`.  (torch casts float64 to a 16-bit type through float32: one rounding only when
    that first step is exact, which is asserted -- every exact-grid result has far fewer than 24 significant bits.)"""
    f = v.to(F32)
    assert torch.equal(f.to(F64), v), "the value is not exact in fp32: two roundings"
    return f.to(dtype)


def gamma(n):
    n = torch.as_tensor(n, dtype=F64)
    return n * U / (1.0 - n * U)


def bar(ref, mag, n, dtype):
    """half an output ulp (16-bit outputs only) + gamma(n) sum|terms|"""
    b = gamma(n) * mag
    return b + 0.5 * ulp16(ref, dtype) if dtype in (F16, BF16) else b


def worst_ratio(got, ref, b):
    """largest |got - ref| / bar over EVERY element; an element off a zero bar counts as inf, a non-finite output as inf"""
    err = (widen(got) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def check_grid_sums(inputs, mags, bound):
    """Precondition of the bit-exact bars: the inputs are k / 4 (so every product of two is a multiple of 1/16) and each sum of
    magnitudes `mags` is a multiple of 1/16 below `bound` (_exact_grid.check_exact, one sum per column)."""
    for t in inputs:
        assert torch.equal(t * 4, torch.round(t * 4)), "input off the 1/4 grid"
    check_exact(*[m.reshape(1, -1) for m in mags], bound=bound)


# ---------------------------------------------------------------------------------------------- dot interaction
def out_width(r, c):
    raw = r * (r - 1) // 2 + c
    return ((raw - 1) // 8 + 1) * 8


def tril_pairs(r):
    """strict lower triangle, row-major: (1,0), (2,0), (2,1), ..."""
    ij = torch.tril_indices(r, r, -1)
    return ij[0], ij[1]


def dot_interact_fwd(x):
    """x [B, R, C] float64 -> (y [B, OW], sum of the magnitudes of the terms of every y): [x[:, 0, :] | (X X^T)[i, j], i > j |
    zeros up to a multiple of 8]"""
    b, r, c = x.shape
    ri, ci = tril_pairs(r)
    pad = torch.zeros(b, out_width(r, c) - c - ri.numel(), dtype=F64)
    a = x.abs()
    y = torch.cat([x[:, 0, :], torch.bmm(x, x.transpose(1, 2))[:, ri, ci], pad], 1)
    mag = torch.cat([a[:, 0, :], torch.bmm(a, a.transpose(1, 2))[:, ri, ci], pad], 1)
    return y + 0.0, mag                                      # (+ 0.0: a sum that starts at +0 is never -0)


def dot_interact_bwd(x, ug, fuse_mlp_grad):
    """-> (grad [B, R, C], mlp_grad [B, C] or None, sum of magnitudes per grad element).  grad = U_sym X with U_sym[i][j] =
    U_sym[j][i] = ug[:, C + pair(i, j)] and a zero diagonal; fused: ug[:, :C] is one more addend of row 0 and no mlp_grad is
    returned (the kernel adds it in the same fp32 accumulator and rounds once)."""
    b, r, c = x.shape
    ri, ci = tril_pairs(r)
    u = torch.zeros(b, r, r, dtype=F64)
    u[:, ri, ci] = ug[:, c:c + ri.numel()]
    u = u + u.transpose(1, 2)
    g = torch.bmm(u, x)
    mag = torch.bmm(u.abs(), x.abs())
    head = ug[:, :c].clone()
    if fuse_mlp_grad:
        g[:, 0, :] += head
        mag[:, 0, :] += head.abs()
        return g + 0.0, None, mag
    return g + 0.0, head, mag


# (B, R, C) of the bit-exact tests.  Routes of the launchers (dle_dot_interact_fwd / _bwd_checked), 16-bit types, aligned pointers:
#   forward  MFMA when R <= 32 and C % 16 == 0 (the persistent walk when C in {64, 128} and B >= 4096), else generic;
#   backward MFMA when R <= 32 and C in {32, 64, 128, 256} (NB = C / 32), else generic.  fp32 and force_generic: generic.
DOT_SHAPES = [
    (5, 27, 128),        # the Criteo width
    (7, 32, 128),        # 496 pairs: tv[] of the backward nearly full (8 x 64 slots)
    (3, 33, 128),        # generic by row count
    (6, 1, 32),          # no pairs (OW == C: the pairwise part of the upstream row is empty)
    (6, 2, 32),          # two rows
    (9, 27, 32),         # NB = 1
    (9, 27, 64),         # NB = 2
    (9, 27, 256),        # NB = 8: 79,872 bytes of LDS
    (9, 32, 256),
    (5, 27, 16),         # forward MFMA, backward generic
    (5, 27, 48),
    (4, 13, 20),         # generic, C no multiple of 8
    (2051, 27, 128),     # backward walk (2048 wavefronts a lap): a second trip for three wavefronts
    (4099, 27, 128),     # forward walk
    (4099, 20, 64),
    (4097, 27, 128),     # a wavefront whose prefetch target is past B
]
DOT_GAUSS = [(5, 27, 128), (9, 27, 256), (4099, 27, 128), (4, 13, 20)]
# (id, dtype, force_generic)
DOT_ROUTES = [("f16", F16, False), ("f16_generic", F16, True), ("bf16", BF16, False), ("bf16_generic", BF16, True),
              ("f32", F32, False)]


def _dot_seed(shape):
    b, r, c = shape
    return b * 1000 + r * 10 + c


@functools.lru_cache(maxsize=2)
def _dot_case(shape, kind, dtype):
    b, r, c = shape
    ow = out_width(r, c)
    if kind == "grid":                       # the same values in every type: k / 4 is exact in all three
        x = grid(shape, _dot_seed(shape), F32, "cpu")
        ug = grid((b, ow), _dot_seed(shape) + 1, F32, "cpu")
        if r >= 9:
            # Random signs keep |sum| near 0.4 sqrt(C): 8 significant bits or fewer, hardly a rounding at all.  Rows 1 .. 8 of the first
            # four samples are 3/4 or 1 throughout: each of their 28 pairs sums to about 0.77 C in multiples of 1/16 -- 9 bits at
            # C = 32, 12 at C = 256: bf16 ties from C = 32 on, fp16 ties at C = 256 (spacing 1/8 above 128).
            k = torch.randint(3, 5, (min(b, 4), 8, c), generator=gen("cpu", _dot_seed(shape) + 3))
            x[:4, 1:9, :] = k.to(F32) * 0.25
    else:
        g = gen("cpu", _dot_seed(shape) + 2)
        x = torch.randn(shape, generator=g).to(dtype).to(F32)
        ug = torch.randn((b, ow), generator=g).to(dtype).to(F32)
    x64, u64 = x.to(F64), ug.to(F64)
    y, ymag = dot_interact_fwd(x64)
    gr, head, gmag = dot_interact_bwd(x64, u64, False)
    return dict(x=x, ug=ug, y=y, ymag=ymag, grad=gr, gmag=gmag, head=head)


def dot_case(shape, kind, dtype):
    """inputs (fp32 tensors holding values of `dtype`) and float64 references of one shape, computed once and shared.  The fused
    gradient differs from the unfused one in row 0 only: fused() builds it."""
    return _dot_case(tuple(shape), kind, None if kind == "grid" else dtype)


def fused(case):
    g, m = case["grad"].clone(), case["gmag"].clone()
    g[:, 0, :] += case["head"]
    m[:, 0, :] += case["head"].abs()
    return g + 0.0, m


def dot_check_exact(case):
    x64, u64 = case["x"].to(F64), case["ug"].to(F64)
    _, fm = fused(case)
    check_grid_sums([x64, u64], [case["ymag"], case["gmag"], fm], B_MFMA)
    assert float(case["ymag"].max()) <= x64.shape[2] and float(fm.max()) <= x64.shape[1] + 1


# ---------------------------------------------------------------------------------------------- embeddings
def table_offsets(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def hash_offset(idx, offsets=None, hash_sizes=None):
    """rows[b, t] = (idx[b, t] mod size_t, the floor-mod of python: in [0, size_t) for a negative index too) + offsets[t]"""
    rows = idx.clone()
    if hash_sizes is not None:
        rows = torch.remainder(rows, hash_sizes[None, :])
    if offsets is not None:
        rows = rows + offsets[None, :rows.shape[1]]
    return rows


def gather(w, rows, out_dtype):
    """out[b, t, :] = W[rows[b, t], :]: a copy, rounded once when the output is a 16-bit type"""
    return w[rows].to(out_dtype)


def gather_strided(w, rows, flat, first, batch_stride):
    """the same rows written into a copy of the flat buffer `flat`: element (b, t, d) at first + b * batch_stride + t * dim + d;
    everything else keeps its bits"""
    out = flat.clone()
    b, t = rows.shape
    d = w.shape[1]
    out.as_strided((b, t, d), (batch_stride, d, 1), first).copy_(w[rows].to(flat.dtype))
    return out


def sparse_sgd(w, rows, g, lr, scale=1.0):
    """W[rows[i]] -= lr * scale * g[i], duplicates of a row summed -> (W', sum of the magnitudes of the terms of every element,
    lookups per row).  w [N, D], rows [...], g [..., D]: float64 / int64."""
    d = w.shape[1]
    r = rows.reshape(-1)
    acc = torch.zeros_like(w).index_add_(0, r, g.reshape(-1, d))
    mag = torch.zeros_like(w).index_add_(0, r, g.reshape(-1, d).abs())
    dup = torch.zeros(w.shape[0], dtype=F64).index_add_(0, r, torch.ones(r.numel(), dtype=F64))
    return w - (lr * scale) * acc, w.abs() + (lr * scale) * mag, dup


GATHER_DIMS = [4, 12, 20, 64, 128, 136, 200, 256]      # D4 = 1, 3, 5 (no power of two), 16, 32, 34, 50, 64 (a second column trip)
GATHER_SIZES = [7, 1, 1000, 33, 5000, 2, 129]
GATHER_BATCH = 777
GATHER_LAP = (128, 7, 10001)                            # dim, tables, batch: 70,007 rows, past the 65,536 of one grid lap


def gather_case(dim, batch=GATHER_BATCH):
    """fp32 grid table (|w| <= 4), plain indices, indices for hashing in [-3 size, 3 size)"""
    sizes = GATHER_SIZES
    off = table_offsets(sizes)
    g = gen("cpu", 1000 + dim + batch)
    w = grid((int(off[-1]), dim), 2000 + dim, F32, "cpu", kmax=16)
    idx = torch.stack([torch.randint(0, s, (batch,), generator=g) for s in sizes], 1)
    wild = torch.stack([torch.randint(-3 * s, 3 * s, (batch,), generator=g) for s in sizes], 1)
    return dict(w=w, off=off, sizes=torch.tensor(sizes, dtype=torch.int64), idx=idx, wild=wild)


# The sparse SGD configurations: (dim, gradient types, table sizes, batches).  Which kernels dle_emb_sgd_dedup_ws picks follows from
# its rules.  A table is "small" when rows * dim * 4 <= 64 KB (the first 64 of them only); a small table is "tiny" when it has
# <= 128 rows, dim <= 128 and 16-bit gradients.  Tiny tables run as the one-hot MFMA sum at dim 128 (the workspace is given) and as
# the register form emb_sgd_tiny at other dims (no one-hot scratch is planned there); the other small ones take the LDS form
# emb_sgd_small.  Every table that is not small is linked into lists; of those, tables of <= 4096 rows at dim <= 128 with 16-bit
# gradients and tables <= 128 (at most 16 of them) get eight lists per row and the fold pass.
SGD_CONFIGS = {
    # small: rows <= 128.  one-hot: 4, 128, 1, 97.  eight lists + fold: 300, 2209, 129.  one list per row: 5000.
    "a": dict(dim=[128], gdtypes=[F16, BF16], sizes=[4, 128, 1, 97, 300, 2209, 5000, 129], batches=[37, 1000, 4099]),
    # dim 64 (small: rows <= 256).  emb_sgd_tiny: 1, 32 (one row group), 33, 64 (two), 65, 128 (four).  emb_sgd_small: 129, 256.
    #   eight lists + fold: 300.  one list: 5000.
    # dim 32 (small: rows <= 512).  emb_sgd_tiny as above.  emb_sgd_small: 129, 256, 300.  one list: 5000 (> 4096 rows, no fold).
    "b": dict(dim=[64, 32], gdtypes=[F16, BF16], sizes=[1, 32, 33, 64, 65, 128, 129, 256, 300, 5000], batches=[37, 1000, 4099]),
    # dim 256 (small: rows <= 64; never tiny: dim > 128).  emb_sgd_small with D4 = 64 (its tail loop only): 8, 64.
    #   one list per row, the columns past 128 on the second walk of the chain: 65, 3000 (no fold: dim > 128).
    "c": dict(dim=[256], gdtypes=[F16, BF16], sizes=[8, 64, 65, 3000], batches=[37, 1000, 4099]),
    # fp32 gradients: never tiny, no workspace plan (no one-hot, no fold).  dim 128: emb_sgd_small 4, 100, 128; lists 300, 5000.
    #   dim 64: emb_sgd_small 4, 100, 128; lists 300 (> 256 rows), 5000.
    "d": dict(dim=[128, 64], gdtypes=[F32], sizes=[4, 100, 128, 300, 5000], batches=[37, 1000, 4099]),
    # 71 tables: the first 64 four-row tables are small and tiny (one-hot); the other six are not small (the cap of 64): eight lists
    #   + fold; 5000: one list per row.
    "e": dict(dim=[128], gdtypes=[F16, BF16], sizes=[4] * 70 + [5000], batches=[37, 1000, 4099]),
    # 130 tables at dim 16 (small: rows <= 1024): more than 128 tables, so the lookup map is off (map.nl == 0: every lookup is
    #   walked, the small tables' skipped through is_small[]) and there is no fold.  The first 64 of the 3- and 200-row tables
    #   (table indices 0 .. 95) are small: emb_sgd_tiny for 3 rows, emb_sgd_small for 200; from index 96 on they are linked, as
    #   every 5000-row table is.
    "f": dict(dim=[16], gdtypes=[F16, BF16], sizes=[[3, 200, 5000][i % 3] for i in range(130)], batches=[1000]),
}
SGD_GAUSS = ["a", "b", "d"]                       # at batch 4099
SGD_LR, SGD_SCALE = 0.5, 0.25                      # powers of two: lr * scale * g is exact


def sgd_params(names=None, batches=None):
    """(config, dim, gradient type, batch) of every case"""
    out = []
    for k in names or SGD_CONFIGS:
        c = SGD_CONFIGS[k]
        for dim in c["dim"]:
            for dt in c["gdtypes"]:
                for b in batches or c["batches"]:
                    out.append((k, dim, dt, b))
    return out


def sgd_id(p):
    return "%s-dim%d-%s-b%d" % (p[0], p[1], name(p[2]), p[3])


@functools.lru_cache(maxsize=2)
def sgd_case(cfg, dim, gdtype, batch, kind):
    """w fp32 [rows, dim]; rows int64 [B, T] (the LAST row of a table of more than one row is never looked up); g [B, T + 1, dim] of
    the gradient type as the train step lays it out: slot 0 belongs to the bottom MLP (NaN here: nobody may read it), slot 1 + t
    is table t's gradient.  -> inputs + float64 reference, magnitudes and lookups per row."""
    sizes = SGD_CONFIGS[cfg]["sizes"]
    t = len(sizes)
    off = table_offsets(sizes)
    seed = 31 * dim + batch + len(cfg) + ord(cfg[0])
    g = gen("cpu", seed)
    idx = torch.stack([torch.randint(0, max(s - 1, 1), (batch,), generator=g) for s in sizes], 1)
    rows = hash_offset(idx, off)
    if kind == "grid":
        w = grid((int(off[-1]), dim), seed + 1, F32, "cpu", kmax=16)
        gr = grid((batch, t + 1, dim), seed + 2, gdtype, "cpu")
    else:
        w = torch.randn((int(off[-1]), dim), generator=g)
        gr = torch.randn((batch, t + 1, dim), generator=g).to(gdtype)
    gr[:, 0, :] = float("nan")
    ref, mag, dup = sparse_sgd(w.to(F64), rows, gr[:, 1:, :].to(F64), SGD_LR, SGD_SCALE)
    return dict(w=w, rows=rows, g=gr, off=off, ref=ref, mag=mag, dup=dup, tables=t)


def sgd_check_exact(case):
    """W' / (lr scale) = W / (lr scale) - sum g: with lr scale a power of two the kernel's sums are these, scaled exactly"""
    k = SGD_LR * SGD_SCALE
    w64, g64 = case["w"].to(F64), case["g"][:, 1:, :].to(F64)
    check_grid_sums([w64, g64], [case["mag"] / k], 2.0 ** 18)
    assert float(case["mag"].max()) <= 4 + k * case["g"].shape[0]


# ---------------------------------------------------------------------------------------------- BCE with logits
def bce_with_logits(x, y, scale=1.0):
    """x, y float64 [N], y in {0, 1} (click labels) -> (mean loss, sum of the magnitudes of the loss terms / N, gradient).
    loss_i = max(x, 0) - x y + log1p(exp(-|x|)); gradient = (sigmoid(x) - y) scale / N, with sigmoid(x) - y written as
    (1 - y) sigmoid(x) - y sigmoid(-x) so that float64 does not cancel where sigmoid(x) rounds to y."""
    n = x.numel()
    e = torch.exp(-x.abs())
    terms = x.clamp_min(0) - x * y + torch.log1p(e)
    p, q = 1.0 / (1.0 + e), e / (1.0 + e)
    s = torch.where(x >= 0, p, q)
    c = torch.where(x >= 0, q, p)
    return terms.sum() / n, terms.abs().sum() / n, ((1.0 - y) * s - y * c) * scale / n


BCE_SIZES = [1, 37, 1000, 4099]


def bce_edge(dtype):
    """the fixed edge vector, each value with the label 0 and the label 1"""
    big = 60000.0 if dtype == F16 else 1e30
    v = [0.0, 1e-4, -1e-4, 20.0, -20.0, 80.0, -80.0, big, -big]
    x = torch.tensor(v + v, dtype=F32).to(dtype)
    y = torch.cat([torch.zeros(len(v)), torch.ones(len(v))])
    return x, y


def bce_case(n, dtype, seed=0):
    """logits N(0, 4) rounded to `dtype`, labels Bernoulli(1/2)"""
    g = gen("cpu", 77 + n + seed)
    x = (torch.randn(n, generator=g) * 2.0).to(dtype)
    y = (torch.rand(n, generator=g) < 0.5).to(F32)
    return x, y
