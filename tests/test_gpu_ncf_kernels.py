"""dle_ncf_score_fwd and dle_ncf_rank_fwd (csrc/ncf.hip) against tests/_ncf_ref.py: bit for bit on exactly summable inputs, under the
propagated per-element bar on random ones, the index rule, reproducibility, the argument checks, and the rank rule in integers.

Sizes: U = 37, I = 23 (the first and the last row of each table are always among the pairs); B in {1, 31, 32, 33, 100, 257} covers
one partial tile, a half tile and its neighbours, two tiles and five; max_workgroups 0 / 1 / 2 gives one trip per workgroup, five
trips on one workgroup, and the uneven 3 + 2 split."""
import functools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from tests import _exact_grid as G
from tests import _ncf_ref as R
from tests import _tft_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
ITYPES = [pytest.param(torch.int64, id="i64"), pytest.param(torch.int32, id="i32")]
NU, NI = 37, 23
BATCHES = (1, 31, 32, 33, 100, 257)
WORKGROUPS = (0, 1, 2)


def on_dev(sd, dtype):
    """The kernel's operands from a state dict whose tables and W1..W3 are representable in dtype."""
    t = lambda n: sd[n].to(DEV, dtype).contiguous()
    f = lambda n: sd[n].to(DEV, torch.float32).contiguous()
    return dict(tables=tuple(t(n) for n in R.NAMES), weights=tuple(t("mlp.%d.weight" % i) for i in range(3)),
                biases=tuple(f("mlp.%d.bias" % i) for i in range(3)), wf=f("final.weight").reshape(-1), bf=f("final.bias").reshape(1))


def score(ops, u, i, itype, label=None, want_prob=False, mwg=0):
    return F.ncf_score_fwd(*ops["tables"], ops["weights"], ops["biases"], ops["wf"], ops["bf"], u.to(DEV, itype), i.to(DEV, itype),
                           label=None if label is None else label.to(DEV), want_prob=want_prob, max_workgroups=mwg)


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_state():
    """Tables k / 4; W1 = identity + a sparse grid, W2 / W3 = selectors (+1 of one input, -1/2 of its neighbour) + a sparse grid;
    biases and the final layer k / 4.  Every product chain stays on the 1/1024 grid with small magnitude sums."""
    g = lambda shape, seed, kmax=4, density=1.0: G.grid(shape, seed, torch.float32, "cpu", kmax, density)
    sd = {R.NAMES[0]: g((NU, 64), 1), R.NAMES[1]: g((NI, 64), 2), R.NAMES[2]: g((NU, 128), 3), R.NAMES[3]: g((NI, 128), 4)}
    w1 = torch.eye(256) + g((256, 256), 5, 2, 0.04)
    w2, w3 = g((128, 256), 6, 2, 0.04), g((64, 128), 7, 2, 0.06)
    for n in range(128):
        w2[n, 2 * n], w2[n, 2 * n + 1] = 1.0, -0.5
    for n in range(64):
        w3[n, 2 * n], w3[n, 2 * n + 1] = 1.0, -0.5
    sd.update({"mlp.0.weight": w1, "mlp.1.weight": w2, "mlp.2.weight": w3, "mlp.0.bias": g((256,), 8), "mlp.1.bias": g((128,), 9),
               "mlp.2.bias": g((64,), 10), "final.weight": g((1, 128), 11, 2), "final.bias": torch.tensor([0.25])})
    return sd


def check_exactly_summable(sd, u, i, dtype):
    """Every fp32 sum of the kernel is exact: its terms lie on a grid 2^-g and their magnitudes sum to less than 2^(22 - g) (two
    bits of headroom under fp32's 24 for the matrix units' alignment of a group of products)."""
    d = lambda n: sd[n].double()
    x = torch.cat((d(R.NAMES[2])[u], d(R.NAMES[3])[i]), 1)
    grid = 4                                                         # x W1: multiples of 2^-4
    for l in range(3):
        w, b = d("mlp.%d.weight" % l), d("mlp.%d.bias" % l)
        assert float((x.abs() @ w.abs().T + b.abs()).max()) < 2.0 ** (22 - grid), "layer %d" % (l + 1)
        x = torch.relu(x @ w.T + b)
        assert torch.equal(x * 2 ** grid, torch.round(x * 2 ** grid))
        if l < 2:
            x = T.to16(x, dtype)                                     # rounding keeps a value on its grid
        grid += 2
    prod = d(R.NAMES[0])[u] * d(R.NAMES[1])[i]
    wf = d("final.weight").reshape(-1)
    assert float((prod.abs() @ wf[:64].abs() + x.abs() @ wf[64:].abs()).max() + 1) < 2.0 ** (22 - grid)


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_bit_for_bit(dtype, itype):
    sd = exact_state()
    ops = on_dev(sd, dtype)
    for B in BATCHES:
        u, i = R.seeded_pairs(NU, NI, B, 100 + B)
        check_exactly_summable(sd, u, i, dtype)
        want = R.forward(T.Mode("emul", dtype), sd, u, i).v
        assert float(want.abs().max()) > 1.0 or B == 1
        for mwg in WORKGROUPS:
            logit, prob, part = score(ops, u, i, itype, mwg=mwg)
            assert prob is None and part is None and logit.dtype == torch.float32
            G.assert_same(logit.double().cpu(), want, "logit B=%d max_workgroups=%d" % (B, mwg))


# ---- random inputs against the bar --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_random_against_the_bar(dtype):
    sd = R.seeded_state(NU, NI, 5, dtype)
    ops = on_dev(sd, dtype)
    worst = 0.0
    for B in BATCHES:
        u, i = R.seeded_pairs(NU, NI, B, 200 + B)
        y = (torch.rand(B, generator=torch.Generator().manual_seed(B)) < 0.3).float()
        ref = R.forward(T.Mode("bar", dtype), sd, u, i)
        for mwg in WORKGROUPS:
            logit, prob, part = score(ops, u, i, torch.int64, label=y, want_prob=True, mwg=mwg)
            x = logit.double().cpu()
            ratio = float(((x - ref.v).abs() / ref.bar()).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, "B=%d max_workgroups=%d: error / bar = %.3f" % (B, mwg, ratio)
            # the probability and the loss are functions of the kernel's own fp32 logit
            assert bool(((prob.double().cpu() - R.sigmoid64(x)).abs() <= R.prob_bar(x)).all())
            want_loss = float(R.bce64(x, y).sum())
            got_loss = float(part.sum(dtype=torch.float64))
            assert abs(got_loss - want_loss) <= R.loss_sum_bar(x, y), (B, mwg, got_loss, want_loss)
            n = part.numel()
            used = min((B + 63) // 64, n)
            assert n == (mwg or torch.cuda.get_device_properties(0).multi_processor_count)
            assert float(part[used:].abs().sum()) == 0.0             # the slots behind the grid are zeroed
    print("%s: worst error / bar %.3f" % (dtype, worst))
    assert worst > 0.0


def test_loss_clamp_and_saturation():
    """Logits far out (|x| up to ~50 through a large final bias): the probability saturates to exactly 0 / 1 without NaN, and the
    loss is the linear tail, nowhere near the -100 clamp's inf."""
    sd = dict(R.seeded_state(NU, NI, 5, HF))
    u, i = R.seeded_pairs(NU, NI, 64, 7)
    for bias in (-50.0, 50.0):
        sd["final.bias"] = torch.tensor([bias])
        logit, prob, part = score(on_dev(sd, HF), u, i, torch.int64, label=torch.ones(64) if bias < 0 else torch.zeros(64), want_prob=True)
        x = logit.double().cpu()
        assert bool(torch.isfinite(prob).all()) and bool(torch.isfinite(part).all())
        assert abs(float(part.sum(dtype=torch.float64)) - float(R.bce64(x, torch.ones(64) if bias < 0 else torch.zeros(64)).sum())) <= \
            R.loss_sum_bar(x, torch.ones(64))
        assert float(part.sum()) > 64 * 30


# ---- the index rule, reproducibility, argument checks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("itype", ITYPES)
def test_out_of_range_indices_give_nan_and_touch_nothing_else(itype):
    sd = R.seeded_state(NU, NI, 5, BF)
    ops = on_dev(sd, BF)
    u, i = R.seeded_pairs(NU, NI, 100, 9)
    y = torch.ones(100)
    clean = score(ops, u, i, itype, label=y, want_prob=True, mwg=1)
    ub, ib = u.clone(), i.clone()
    ub[40], ub[45], ib[70] = -1, NU, NI + 1000                       # in the middle of the first and of the second tile
    bad = torch.zeros(100, dtype=torch.bool)
    bad[[40, 45, 70]] = True
    logit, prob, part = score(ops, ub, ib, itype, label=y, want_prob=True, mwg=1)
    assert bool(torch.isnan(logit.cpu()[bad]).all()) and bool(torch.isnan(prob.cpu()[bad]).all())
    assert torch.equal(G.bits(logit.cpu()[~bad]), G.bits(clean[0].cpu()[~bad]))
    assert torch.equal(G.bits(prob.cpu()[~bad]), G.bits(clean[1].cpu()[~bad]))
    x = clean[0].double().cpu()
    want = float(R.bce64(x[~bad], y[~bad]).sum())                    # the bad rows add nothing
    assert abs(float(part.sum(dtype=torch.float64)) - want) <= R.loss_sum_bar(x[~bad], y[~bad])
    assert bool(torch.isfinite(part).all())


def test_two_calls_give_identical_bits():
    sd = R.seeded_state(NU, NI, 5, HF)
    ops = on_dev(sd, HF)
    u, i = R.seeded_pairs(NU, NI, 257, 3)
    y = (torch.arange(257) % 3 == 0).float()
    a = score(ops, u, i, torch.int64, label=y, want_prob=True)
    b = score(ops, u, i, torch.int64, label=y, want_prob=True)
    for s, t in zip(a, b):
        assert torch.equal(G.bits(s), G.bits(t))
    # and a sample's score does not depend on the batch around it or on the trip that computes it
    c = score(ops, u[100:101], i[100:101], torch.int32, mwg=1)
    assert torch.equal(G.bits(c[0]), G.bits(a[0][100:101]))


def test_argument_checks_fire():
    sd = R.seeded_state(NU, NI, 5, HF)
    ops = on_dev(sd, HF)
    u, i = R.seeded_pairs(NU, NI, 8, 3)
    call = lambda o, **kw: score(o, u, i, torch.int64, **kw)
    # a table that is not 16-byte aligned
    buf = torch.zeros(NU * 64 + 8, dtype=HF, device=DEV)
    mis = dict(ops, tables=(buf[1:1 + NU * 64].view(NU, 64),) + ops["tables"][1:])
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(mis)
    # outside the envelope: 32 factors
    small = dict(ops, tables=(ops["tables"][0][:, :32].contiguous(), ops["tables"][1][:, :32].contiguous()) + ops["tables"][2:],
                 wf=ops["wf"][:96].contiguous())
    with pytest.raises(ValueError, match="built for --factors 64 --layers 256 256 128 64"):
        call(small)
    with pytest.raises(ValueError, match="16-bit"):
        call(dict(ops, tables=tuple(t.float() for t in ops["tables"]), weights=tuple(w.float() for w in ops["weights"])))
    with pytest.raises(ValueError, match="max_workgroups"):
        call(ops, mwg=-1)
    with pytest.raises(ValueError, match="int32 or int64"):
        F.ncf_score_fwd(*ops["tables"], ops["weights"], ops["biases"], ops["wf"], ops["bf"], u.to(DEV).float(), i.to(DEV).float())
    with pytest.raises(ValueError, match="label"):
        call(ops, label=torch.ones(7))
    r = torch.rand(200, device=DEV)
    with pytest.raises(ValueError, match="k <= samples per series"):
        F.ncf_rank_fwd(r, r, None, 100, 101)
    with pytest.raises(ValueError, match="k <= samples per series"):
        F.ncf_rank_fwd(r, r, None, 100, 0)
    with pytest.raises(ValueError, match="<= 4096"):
        F.ncf_rank_fwd(torch.rand(5000, device=DEV), torch.rand(5000, device=DEV), None, 5000, 10)
    with pytest.raises(ValueError, match="whole series"):
        F.ncf_rank_fwd(r, r, None, 99, 10)
    # an empty batch is no launch and no error
    e = torch.zeros(0, dtype=torch.int64)
    logit, _, part = score(ops, e, e, torch.int64, label=torch.zeros(0))
    assert logit.numel() == 0 and float(part.abs().sum()) == 0.0


# ---- the rank kernel ------------------------------------------------------------------------------------------------------------------
def check_rank(rating, label, ignore, S, k):
    hits, dcg = F.ncf_rank_fwd(rating.to(DEV), label.to(DEV), None if ignore is None else ignore.to(DEV), S, k)
    want_h, want_d = R.rank_rule(rating, label, ignore, S, k)
    assert hits.dtype == torch.int32 and dcg.dtype == torch.float32
    G.assert_same(hits.cpu().long(), want_h, "hits S=%d k=%d" % (S, k))
    assert bool(((dcg.double().cpu() - want_d).abs() <= 1e-6 * want_d.abs()).all()), "dcg S=%d k=%d" % (S, k)
    return want_h


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 100, 257])
def test_rank_against_the_integer_statement(S):
    g = torch.Generator().manual_seed(S)
    for n in (1, 1000):
        # few rating levels: ties everywhere, across the k boundary and between positives; ~10 % positives, ~20 % ignored, some NaN
        rating = torch.randint(0, 6, (n * S,), generator=g).float() / 8
        rating[torch.rand(n * S, generator=g) < 0.02] = float("nan")
        label = (torch.rand(n * S, generator=g) < 0.1).float()
        ignore = torch.rand(n * S, generator=g) < 0.2
        total = 0
        for k in sorted({1, min(10, S), S}):
            total += int(check_rank(rating, label, ignore, S, k).sum())
            check_rank(rating, label, None, S, k)
        assert total > 0 or n == 1
    # distinct ratings, one positive per series: the evaluation's own shape
    rating = torch.rand(50 * S, generator=g)
    label = torch.zeros(50, S)
    label[torch.arange(50), torch.randint(0, S, (50,), generator=g)] = 1
    check_rank(rating, label.reshape(-1), None, S, min(10, S))


def test_rank_constructed_cases():
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    m = lambda *v: torch.tensor(v, dtype=torch.bool)
    nan = float("nan")
    cases = [
        (f(0.5, 0.5, 0.1, 0.0), f(0, 1, 0, 0), None, 1, [0]),                   # a tie across the k boundary: the earlier index wins
        (f(0.5, 0.5, 0.1, 0.0), f(1, 0, 0, 0), None, 1, [1]),
        (f(0.5, 0.5, 0.1, 0.0), f(1, 1, 0, 0), None, 1, [1]),                   # a tie between two label-1 elements
        (f(0.5, 0.5, 0.1, 0.0), f(1, 1, 0, 0), None, 2, [2]),
        (f(0.9, 0.2, 0.1, 0.0), f(1, 0, 0, 0), m(1, 0, 0, 0), 3, [0]),     # an ignored label-1 element ranks as -1: last
        (f(0.9, 0.2, 0.1, 0.0), f(1, 0, 0, 0), m(1, 0, 0, 0), 4, [1]),
        (f(0.9, 0.2, 0.1, 0.0), f(0, 0, 1, 0), m(1, 1, 1, 1), 3, [1]),     # all ignored: all -1, by index
        (f(0.9, 0.2, 0.1, 0.0), f(0, 0, 0, 1), m(1, 1, 1, 1), 3, [0]),
        (f(nan, 0.2, 0.1, 0.0), f(1, 0, 0, 0), None, 3, [0]),                   # NaN ranks below everything
        (f(nan, 0.2, nan, 0.0), f(0, 0, 1, 0), None, 4, [1]),
        (f(nan, 0.2, nan, 0.0), f(1, 0, 1, 0), None, 3, [1]),                   # NaNs among themselves by index
        (f(0.2, nan, 0.1, 0.0), f(1, 0, 0, 0), m(0, 1, 0, 0), 1, [1]),     # an ignored NaN is -1
        (f(0.1, 0.9, 0.8, 0.7), f(1, 0, 1, 1), None, 3, [2]),                   # several positives
    ]
    for rating, label, ignore, k, want in cases:
        got = check_rank(rating, label, ignore, 4, k)
        assert got.tolist() == want, (rating, label, ignore, k)
    # bool and uint8 masks are the same mask
    r, l, ig = torch.rand(300), (torch.rand(300) < 0.2).float(), torch.rand(300) < 0.3
    a = F.ncf_rank_fwd(r.to(DEV), l.to(DEV), ig.to(DEV), 100, 10)
    b = F.ncf_rank_fwd(r.to(DEV), l.to(DEV), ig.to(DEV).to(torch.uint8), 100, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(G.bits(a[1]), G.bits(b[1]))
