"""Float64 statement of the NCF kernels (csrc/ncf.hip) and front end, their per-element error bars, the rank rule in integers and
the emulation of the reference's model.half().  No GPU, no product kernel.  The bars are built as tests/_tft_ref.py builds its
own (its V / Mode / linear / r16 are used as they stand):

  exact   float64, nothing rounded: the function dle_ncf_score_fwd approximates, on the 16-bit tables and weights it is given;
  emul    float64 arithmetic with the kernel's rounding contract: the outputs of layers 1 and 2 rounded to the 16-bit type once,
          nothing else (the GMF product, the third layer, the final dot product, the bias stay unrounded);
  bar     the exact values with a per-element bar e + 8 sigma.  Each rounded intermediate contributes one unit roundoff of the
          16-bit type, rnd(|x| + bar) with rnd(y) = 2^-(m+1) y (m = 10 / 7), as a variance rnd^2 / 3 that a following layer carries
          as W^2 sigma^2 (tests/_tft_ref.py says why not |W| rnd: three layers of row sums ~ 10 would put the bar 100 times above
          any real error, and no planted fault could leave it); ReLU is 1-Lipschitz and passes e and sigma on; every fp32
          accumulation of K products adds e = (K + 2) u (|W||x| + |b|), u = 2^-24.  The GMF product of two 16-bit values is exact
          in fp32 (22 / 16 significant bits); its 64-term dot product and the sum of the three parts are fp32 accumulations.

Loss and probability are functions of the kernel's own fp32 logit x, so their bars hold fp32 evaluation errors only:
  prob    p = 1 / (1 + expf(-x)): expf, the sum and the division within 6 u p, plus the smallest subnormal;
  loss    per element -(y lp + (1 - y) lq), lp = max(min(x, 0) - log1pf(expf(-|x|)), -100): each of expf, log1pf, the difference and
          the two products within an ulp or two of values bounded by |x| + 1: 8 u (|x| + 1); the sum of n terms in fp32, in any
          order, then float64: (n + 8) u sum |l|.
"""
import math

import torch

from tests import _tft_ref as T

U = T.U
FACTORS, LAYERS = 64, (256, 256, 128, 64)
NAMES = ("mf_user_embed.weight", "mf_item_embed.weight", "mlp_user_embed.weight", "mlp_item_embed.weight")


# ---- the forward ------------------------------------------------------------------------------------------------------------------
def relu(M, a):
    return T.V(torch.relu(a.v), a.e, a.s) if M.track else T.V(torch.relu(a.v))


def forward(M, sd, user, item, faults=()):
    """NeuMF.forward on the state `sd` (reference names; float64 is taken of whatever precision the tensors hold) in mode M ->
    T.V of logits [B].  faults (the bar's self-test): 'round_h3' and 'round_product' round what the contract leaves in fp32,
    to M.dtype; 'drop_b2' leaves a bias out."""
    d = lambda n: sd[n].double()
    user, item = user.long(), item.long()
    n_mlp = len([k for k in sd if k.startswith("mlp.") and k.endswith(".weight")])
    prod = d(NAMES[0])[user] * d(NAMES[1])[item]
    if "round_product" in faults:
        prod = T.to16(prod, M.dtype)
    x = T.V(torch.cat((d(NAMES[2])[user], d(NAMES[3])[item]), dim=1))
    for i in range(n_mlp):
        b = None if ("drop_b2" in faults and i == 1) else d("mlp.%d.bias" % i)
        x = relu(M, T.linear(M, x, d("mlp.%d.weight" % i), b))
        if i < n_mlp - 1:
            x = T.r16(M, x)
        elif "round_h3" in faults:
            x = T.V(T.to16(x.v, M.dtype))
    wf, bf = d("final.weight").reshape(-1), d("final.bias").reshape(())
    F = prod.shape[1]
    v = prod @ wf[:F] + x.v @ wf[F:] + bf
    if not M.track:
        return T.V(v)
    mag = prod.abs() @ wf[:F].abs() + x.v.abs() @ wf[F:].abs() + bf.abs()
    e = x.e @ wf[F:].abs() + (F + x.v.shape[1] + 4) * U * mag
    return T.V(v, e, x.s @ (wf[F:] ** 2))


def half_forward(sd, user, item, dtype):
    """The reference's model.half() forward (inference.py:73-90), emulated in float64: every parameter, the GMF product, every
    layer's output and the logit rounded to `dtype`; sums accumulate unrounded (the library's GEMMs accumulate in fp32)."""
    r = lambda t: T.to16(t, dtype)
    p = lambda n: r(sd[n].double())
    user, item = user.long(), item.long()
    n_mlp = len([k for k in sd if k.startswith("mlp.") and k.endswith(".weight")])
    xmf = r(p(NAMES[0])[user] * p(NAMES[1])[item])
    x = torch.cat((p(NAMES[2])[user], p(NAMES[3])[item]), dim=1)
    for i in range(n_mlp):
        x = torch.relu(r(x @ p("mlp.%d.weight" % i).T + p("mlp.%d.bias" % i)))
    return r(torch.cat((xmf, x), dim=1) @ p("final.weight").reshape(-1) + p("final.bias").reshape(()))


def sigmoid64(x):
    return torch.sigmoid(x.double())


def bce64(x, y):
    """Per-element binary cross-entropy of p = sigmoid(x) with torch's clamp of the logarithms at -100, from the logit."""
    x, y = x.double(), y.double()
    lp = torch.clamp(torch.nn.functional.logsigmoid(x), min=-100.0)
    lq = torch.clamp(torch.nn.functional.logsigmoid(-x), min=-100.0)
    return -(y * lp + (1 - y) * lq)


def prob_bar(x):
    return 6 * U * sigmoid64(x) + 2.0 ** -149


def loss_sum_bar(x, y):
    l = bce64(x, y)
    return float((8 * U * (x.double().abs() + 1)).sum() + (x.numel() + 8) * U * l.abs().sum())


# ---- the rank rule, in integers -----------------------------------------------------------------------------------------------------
def rank_rule(rating, label, ignore, S, k):
    """-> (hits int64 [n_series], dcg float64 [n_series]).  r_j = -1 where ignored; rank_j = #{i: r_i > r_j or (r_i == r_j and
    i < j)}, NaN below everything and among themselves by index; label-1 elements with rank_j < k count."""
    rating = rating.double().reshape(-1, S).clone()
    label = label.reshape(-1, S)
    if ignore is not None:
        rating[ignore.reshape(-1, S).bool()] = -1.0
    nan = torch.isnan(rating)
    key = torch.where(nan, torch.full_like(rating, -math.inf), rating)          # no rating is -inf: a probability or -1
    ri, rj = key[:, :, None], key[:, None, :]                                    # [n, i, j]
    idx = torch.arange(S)
    earlier = idx[:, None] < idx[None, :]
    both_nan = nan[:, :, None] & nan[:, None, :]
    one_nan_j = ~nan[:, :, None] & nan[:, None, :]
    plain = ~nan[:, :, None] & ~nan[:, None, :]
    above = (plain & ((ri > rj) | ((ri == rj) & earlier))) | one_nan_j | (both_nan & earlier)
    rank = above.sum(1)                                                          # [n, j]
    counted = (label == 1) & (rank < k)
    hits = counted.sum(1)
    dcg = torch.where(counted, math.log(2.0) / torch.log(rank.double() + 2.0), torch.zeros(rank.shape, dtype=torch.float64)).sum(1)
    return hits, dcg


def boundary_clear(logit64, label, ignore, S, k, margin):
    """Series in which every label-1 logit is further than `margin` from the k-th best OTHER (not ignored, not itself) logit: an
    error below margin / 2 on every logit cannot change its hit decision."""
    x = logit64.double().reshape(-1, S)
    lab = label.reshape(-1, S) == 1
    ign = ignore.reshape(-1, S).bool() if ignore is not None else torch.zeros_like(lab)
    clear = torch.ones(x.shape[0], dtype=torch.bool)
    for s in range(x.shape[0]):
        for j in torch.nonzero(lab[s] & ~ign[s]).flatten().tolist():
            others = x[s][~ign[s] & (torch.arange(S) != j)]
            if others.numel() >= k:
                kth = torch.sort(others, descending=True)[0][k - 1]
                clear[s] &= bool((x[s, j] - kth).abs() > margin)
    return clear


# ---- seeded models and inputs -----------------------------------------------------------------------------------------------------
def seeded_state(n_users, n_items, seed, dtype=None, factors=FACTORS, layers=LAYERS):
    """Reference names; tables ~ N(0, 1), MLP glorot uniform, final lecun uniform, biases ~ U(-0.1, 0.1).  dtype: tables and
    W1..W3 are made representable in it (what the kernel is handed), biases and the final layer stay fp32."""
    g = torch.Generator().manual_seed(seed)
    q = (lambda t: t.to(dtype).float()) if dtype is not None else (lambda t: t)
    uni = lambda shape, lim: (torch.rand(shape, generator=g) * 2 - 1) * lim
    sd = {NAMES[0]: q(torch.randn(n_users, factors, generator=g)), NAMES[1]: q(torch.randn(n_items, factors, generator=g)),
          NAMES[2]: q(torch.randn(n_users, layers[0] // 2, generator=g)), NAMES[3]: q(torch.randn(n_items, layers[0] // 2, generator=g))}
    for i in range(1, len(layers)):
        sd["mlp.%d.weight" % (i - 1)] = q(uni((layers[i], layers[i - 1]), math.sqrt(6.0 / (layers[i] + layers[i - 1]))))
        sd["mlp.%d.bias" % (i - 1)] = uni((layers[i],), 0.1)
    sd["final.weight"] = uni((1, layers[-1] + factors), math.sqrt(3.0 / (layers[-1] + factors)))
    sd["final.bias"] = uni((1,), 0.1)
    return sd


def seeded_pairs(n_users, n_items, B, seed):
    """B (user, item) pairs that include the first and the last row of each table when B allows."""
    g = torch.Generator().manual_seed(seed)
    u, i = torch.randint(0, n_users, (B,), generator=g), torch.randint(0, n_items, (B,), generator=g)
    if B >= 2:
        u[0], i[0], u[-1], i[-1] = 0, n_items - 1, n_users - 1, 0
    return u, i
