"""The kernels of csrc/moflow.hip against the float64 statements of tests/_moflow_ref.py: bit for bit on exactly summable inputs,
under the propagated bars on random ones, plus the properties of the contract (pass-through half, 16-bit image, an overflow stays in
its sample, batch independence, determinism, argument errors launch nothing)."""
import functools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from deeplearningexamples_amd.moflow import model as MM
from tests import _exact_grid as G
from tests import _moflow_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
BATCHES = [1, 15, 16, 17, 33, 100]


def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def quarter(shape, g, kmax=4):
    return torch.randint(-kmax, kmax + 1, shape, generator=g).float() / 4


def pow2(shape, g, choices=(0.5, 1.0, 2.0, 4.0)):
    return torch.tensor(choices)[torch.randint(0, len(choices), shape, generator=g)]


# ---- dle_mf_couple_fwd ---------------------------------------------------------------------------------------------------------------
def couple_case(B, P, ch, hid, swap, dtype, seed, exact):
    g = cpu_gen(seed)
    m, k = P * ch, P * hid
    if exact:                                           # s columns zero: the factor is exactly 2; everything a multiple of 1/16
        w3 = torch.cat([torch.zeros(m, k), quarter((m, k), g, 2) * (torch.rand(m, k, generator=g) < 0.25)])
        f = {"w3": w3, "b3": torch.cat([torch.zeros(m), quarter((m,), g)]), "scale": pow2((2 * ch,), g), "loc": quarter((2 * ch,), g),
             "swap": swap}
        h2, state = quarter((B, k), g, 2).abs(), quarter((B, P, 2 * ch), g, 8)
    else:
        f = {"w3": (torch.randn(2 * m, k, generator=g) / k ** 0.5).to(dtype).float(), "b3": torch.randn(2 * m, generator=g) * 0.1,
             "scale": torch.rand(2 * ch, generator=g) + 0.75, "loc": torch.randn(2 * ch, generator=g) * 0.1, "swap": swap}
        h2, state = torch.randn(B, k, generator=g).abs().to(dtype).float(), torch.randn(B, P, 2 * ch, generator=g)
    return f, h2, state


def run_couple(f, h2, state, P, dtype, img_half=0, **kw):
    d = lambda t: t.to(DEV)
    return F.mf_couple_fwd(d(h2).to(dtype), d(f["w3"]).to(dtype), d(f["b3"]), d(f["scale"]), d(f["loc"]), d(state), P, f["swap"],
                           img_half=img_half, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("swap", [False, True], ids=["plain", "swap"])
def test_couple_exact(swap, dtype):
    """Every batch size x position count in one test (the suite pays per test, and each case is a millisecond of GPU work)."""
    for B in BATCHES:
        for P in (1, 4, 9):
            case = "B %d, P %d: " % (B, P)
            f, h2, state = couple_case(B, P, 32, 32, swap, dtype, 100 * B + P, exact=True)
            img_half = (B + P) % 2
            out, img = run_couple(f, h2, state, P, dtype, img_half)
            want = R.couple(R.Mode("exact"), R.V(h2), f, R.V(state), P).v
            assert torch.equal(want.float().double(), want), case
            G.assert_same(G.bits(out.cpu()), G.bits(want.float()), case + "state")
            ch, a0 = 32, (32 if swap else 0)
            passed = state[..., a0:a0 + ch] / f["scale"][a0:a0 + ch] - f["loc"][a0:a0 + ch]  # fp32, as the contract states it
            G.assert_same(G.bits(out.cpu()[..., a0:a0 + ch]), G.bits(passed), case + "pass-through half")
            G.assert_same(G.bits(img.cpu()), G.bits(out.cpu()[..., img_half * ch:(img_half + 1) * ch].to(dtype)), case + "16-bit image")


@pytest.mark.parametrize("dtype", DTYPES)
def test_couple_exact_at_the_real_widths(dtype):
    f, h2, state = couple_case(17, 4, 800, 512, True, dtype, 7, exact=True)
    out, img = run_couple(f, h2, state, 4, dtype, 0)
    want = R.couple(R.Mode("exact"), R.V(h2), f, R.V(state), 4).v
    G.assert_same(G.bits(out.cpu()), G.bits(want.float()), "state")
    G.assert_same(G.bits(img.cpu()), G.bits(out.cpu()[..., :800].to(dtype)), "16-bit image")


@pytest.mark.parametrize("dtype", DTYPES)
def test_couple_random_under_the_bar(dtype):
    for B in BATCHES:
        for P in (1, 4, 9):
            case = "B %d, P %d: " % (B, P)
            swap = bool((B + P) % 2)
            f, h2, state = couple_case(B, P, 32, 32, swap, dtype, 200 * B + P, exact=False)
            out, img = run_couple(f, h2, state, P, dtype, 1)
            bar = R.couple(R.Mode("bar", dtype), R.V(h2), f, R.V(state), P)
            err = (out.cpu().double() - bar.v).abs()
            assert float(bar.bar().max()) < 0.02, case           # fp32 accumulation terms only: far below a 16-bit rounding of these values
            assert bool((err <= bar.bar()).all()), case + "%.3f" % float((err / bar.bar()).max())
            a0 = 32 if swap else 0
            passed = state[..., a0:a0 + 32] / f["scale"][a0:a0 + 32] - f["loc"][a0:a0 + 32]
            G.assert_same(G.bits(out.cpu()[..., a0:a0 + 32]), G.bits(passed), case + "pass-through half")
            G.assert_same(G.bits(img.cpu()), G.bits(out.cpu()[..., 32:].to(dtype)), case + "16-bit image")
            out2, img2 = run_couple(f, h2, state, P, dtype, 1)
            assert torch.equal(G.bits(out2), G.bits(out)) and torch.equal(G.bits(img2), G.bits(img)), case


def test_couple_overflow_stays_in_its_sample():
    f, h2, state = couple_case(33, 4, 32, 32, False, HF, 5, exact=False)
    f["w3"][:128] = -f["w3"][:128].abs()
    ref, _ = run_couple(f, h2, state, 4, HF)
    h2[17] = 60000.0                                    # s = -(a huge sum): exp(-s) overflows
    out, _ = run_couple(f, h2, state, 4, HF)
    out, ref = out.cpu(), ref.cpu()
    assert not bool(torch.isfinite(out[17, :, 32:]).all()) and bool(torch.isfinite(out[17, :, :32]).all())
    keep = torch.arange(33) != 17
    assert torch.equal(G.bits(out[keep]), G.bits(ref[keep]))


def test_couple_argument_errors_launch_nothing():
    f, h2, state = couple_case(4, 4, 32, 32, False, HF, 6, exact=False)
    sentinel = torch.full((4, 4, 64), 7.0, device=DEV)
    with pytest.raises(ValueError, match="16-bit operands"):
        F.mf_couple_fwd(h2.to(DEV), f["w3"].to(DEV), f["b3"].to(DEV), f["scale"].to(DEV), f["loc"].to(DEV), state.to(DEV), 4, False,
                        state_out=sentinel)
    with pytest.raises(ValueError, match="positions"):
        run_couple(f, h2, state, 3, HF, state_out=sentinel)
    bad = dict(f, scale=f["scale"][:-1])
    with pytest.raises(ValueError, match="scale"):
        run_couple(bad, h2, state, 4, HF, state_out=sentinel)
    # C/2 = 6: outside the kernel's envelope, rejected by the library
    f6 = {"w3": torch.zeros(12, 32), "b3": torch.zeros(12), "scale": torch.ones(12), "loc": torch.zeros(12), "swap": False}
    sentinel6 = torch.full((4, 1, 12), 7.0, device=DEV)
    with pytest.raises(ValueError, match="built for"):
        F.mf_couple_fwd(torch.zeros(4, 32, device=DEV, dtype=HF), f6["w3"].to(DEV, HF), f6["b3"].to(DEV), f6["scale"].to(DEV),
                        f6["loc"].to(DEV), torch.zeros(4, 1, 12, device=DEV), 1, False, state_out=sentinel6)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()) and bool((sentinel6 == 7.0).all())


# ---- dle_mf_squeeze_fwd / dle_mf_bond_decide_fwd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fold", [(4, 2), (8, 4), (40, 20)])
def test_squeeze_is_the_index_map(n, fold):
    g = cpu_gen(n)
    z = torch.randn(5, 3 + 4 * n * n, generator=g)      # a column slice of a wider latent vector
    for half in (0, 1):
        state, img = F.mf_squeeze_fwd(z.to(DEV)[:, 3:], n, fold, half, BF)
        want = R.to_state(z[:, 3:].reshape(5, 4, n, n), fold)
        ch = want.shape[2] // 2
        assert torch.equal(state.cpu(), want) and torch.equal(G.bits(img.cpu()), G.bits(want[..., half * ch:(half + 1) * ch].to(BF)))


@pytest.mark.parametrize("unshift", [False, True], ids=["noise", "noise0"])
@pytest.mark.parametrize("n,fold", [(4, 2), (8, 4), (40, 20)])
def test_bond_decide_against_the_rule(n, fold, unshift):
    g = cpu_gen(10 * n + unshift)
    b = 5
    h = quarter((b, 4, n, n), g, 2)                     # five levels: two-way and four-way ties are common; not symmetric
    h[0] = 0.25                                         # every position a four-way tie
    state = R.to_state(h, fold).contiguous()
    mask, code, adj, hadj = F.mf_bond_decide_fwd(state.to(DEV), n, fold, unshift, want_adj=True, want_h=True)
    wm, wc, wa = R.decide(h, unshift)
    pop = sum(((wm >> e) & 1).long() for e in range(4))
    assert int((pop == 2).sum()) > 0 and int((pop == 4).sum()) >= n * n and int((pop == 1).sum()) > 0
    assert not torch.equal(h, h.transpose(2, 3))
    assert torch.equal(mask.cpu(), wm) and torch.equal(code.cpu(), wc)
    assert torch.equal(mask, mask.transpose(1, 2)) and torch.equal(code, code.transpose(1, 2))
    assert torch.equal(adj.cpu().double(), wa) and torch.equal(hadj.cpu(), h)
    m2, c2, a2, h2 = F.mf_bond_decide_fwd(state.to(DEV), n, fold, unshift)
    assert a2 is None and h2 is None and torch.equal(m2, mask) and torch.equal(c2, code)


def test_bond_decide_unshift_changes_nothing_but_follows_the_order_of_operations():
    """(h + 0.5) * 2 is monotone: the same decisions; values near the fp32 spacing may tie after it, which the statement shares."""
    g = cpu_gen(3)
    h = torch.randn(3, 4, 8, 8, generator=g)
    state = R.to_state(h, 4).contiguous().to(DEV)
    for unshift in (False, True):
        v = h
        if unshift:
            v = (v + 0.5) * 2
        v = (v + v.transpose(2, 3)) / 2                 # fp32, the kernel's order
        want = (v == v.max(dim=1, keepdim=True).values)
        mask = F.mf_bond_decide_fwd(state, 8, 4, unshift)[0].cpu()
        assert torch.equal(R.bits_to_adj(mask).bool(), want)


def test_bond_decide_argument_errors():
    with pytest.raises(ValueError, match="multiple of the fold"):
        F.mf_bond_decide_fwd(torch.zeros(2, 4, 64, device=DEV), 8, 3, False)
    with pytest.raises(ValueError, match="whole"):
        F.mf_bond_decide_fwd(torch.zeros(2, 4, 60, device=DEV), 8, 4, False)


# ---- dle_mf_atom_reverse_fwd ----------------------------------------------------------------------------------------------------------
FIX_W, ZINC_W = (16, (32, 8)), (256, (512, 64))


@functools.lru_cache(maxsize=None)
def atom_flows(n, t, widths, n_flow, dtype, seed, exact=False):
    torch.manual_seed(seed)
    net = R.seed_model(MM.GlowOnGraph(n, t, [widths[0]], list(widths[1]), n_flow, 1, [1], [1]), seed + 1).eval()
    flows = R.representable(MM.fold_atom_model(net, t), dtype, ("wg", "w1", "w2", "w3"))
    if exact:                                           # the last linear's weights zero, s = 0: the factor is exactly 2
        g = cpu_gen(seed + 2)
        for i, f in enumerate(flows):
            f["w3"] = torch.zeros_like(f["w3"])
            f["b3"] = torch.cat([torch.zeros(t), quarter((t,), g)])
            f["scale"] = torch.ones(n)
            f["scale"][f["row"]] = 2.0                  # undoes the factor on the coupled row: the chain keeps 24 bits
            if i % 5 == 0:
                f["scale"][(f["row"] + 1) % n] = 0.5
            if i % 7 == 0:
                f["scale"][(f["row"] + 2) % n] = 2.0
            f["loc"] = quarter((n,), g)
    return flows


def adjacency(kind, b, n, seed):
    g = cpu_gen(seed)
    if kind == "empty":
        m = torch.zeros(b, n, n, dtype=torch.uint8)
    elif kind == "full":
        m = torch.full((b, n, n), 15, dtype=torch.uint8)
    elif kind == "tied":
        m = torch.tensor([3, 5, 10, 15, 1, 8], dtype=torch.uint8)[torch.randint(0, 6, (b, n, n), generator=g)]
    else:
        m = (1 << torch.randint(0, 4, (b, n, n), generator=g)).to(torch.uint8)
    return torch.maximum(m, m.transpose(1, 2)) if kind == "random" else m


def run_atom(flows, mask, zx, widths, dtype, **kw):
    n, t = zx.shape[1:]
    w16, p32 = MM.pack_folded_atom_flows(flows, dtype)
    return F.mf_atom_reverse_fwd(zx.reshape(zx.shape[0], -1).to(DEV), mask.to(DEV), w16.to(DEV), p32.to(DEV), n, t, [widths[0]],
                                 list(widths[1]), 1, kw.pop("unshift", False), **kw)


ATOM_SHAPES = [(4, 4), (8, 4), (40, 10)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dflow", [None, -2, 0, 2], ids=["one", "N-2", "N", "N+2"])
@pytest.mark.parametrize("n,t", ATOM_SHAPES)
def test_atom_exact_chain(n, t, dflow, dtype):
    n_flow = 1 if dflow is None else n + dflow
    flows = atom_flows(n, t, FIX_W, n_flow, dtype, 11 * n + n_flow, exact=True)
    for b, kind in ((1, "random"), (33, "tied")):
        zx, mask = quarter((b, n, t), cpu_gen(b), 8), adjacency(kind, b, n, b)
        want = R.atom_reverse(R.Mode("exact"), flows, R.bits_to_adj(mask), zx, False).v
        assert torch.equal(want.float().double(), want)
        G.assert_same(G.bits(run_atom(flows, mask, zx, FIX_W, dtype).cpu()), G.bits(want.float()), "x")


@pytest.mark.parametrize("dtype", DTYPES)
def test_atom_exact_chain_zinc_widths(dtype):
    flows = atom_flows(40, 10, ZINC_W, 42, dtype, 77, exact=True)
    zx, mask = quarter((17, 40, 10), cpu_gen(1), 8), adjacency("random", 17, 40, 2)
    want = R.atom_reverse(R.Mode("exact"), flows, R.bits_to_adj(mask), zx, True).v
    G.assert_same(G.bits(run_atom(flows, mask, zx, ZINC_W, dtype, unshift=True).cpu()), G.bits(want.float()), "x")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,t,widths,n_flow,b", [(4, 4, FIX_W, 6, 15), (8, 4, FIX_W, 10, 33), (8, 4, FIX_W, 1, 16), (40, 10, FIX_W, 38, 17),
                                                 (40, 10, ZINC_W, 42, 100), (8, 10, ZINC_W, 6, 1)])
def test_atom_random_under_the_bar(n, t, widths, n_flow, b, dtype):
    flows = atom_flows(n, t, widths, n_flow, dtype, 5 * n + n_flow)
    for kind in ("empty", "full", "tied", "random"):
        zx, mask = torch.randn(b, n, t, generator=cpu_gen(b)) * 0.6, adjacency(kind, b, n, b + 1)
        got = run_atom(flows, mask, zx, widths, dtype).cpu().double()
        bar = R.atom_reverse(R.Mode("bar", dtype), flows, R.bits_to_adj(mask), zx, False)
        err = (got - bar.v).abs()
        print("%s: max error %.3e, max bar %.3e, max error / bar %.3f" % (kind, float(err.max()), float(bar.bar().max()),
                                                                          float((err / bar.bar()).max())))
        assert bool((err <= bar.bar()).all()), kind
        assert float(bar.bar().max()) < 0.25 * float(bar.v.abs().max()), kind


@pytest.mark.parametrize("dtype", DTYPES)
def test_atom_workgroup_caps_batch_independence_and_determinism(dtype):
    flows = atom_flows(8, 4, FIX_W, 10, dtype, 31)
    zx, mask = torch.randn(100, 8, 4, generator=cpu_gen(9)), adjacency("random", 100, 8, 10)
    ref = run_atom(flows, mask, zx, FIX_W, dtype)
    for cap in (0, 1, 2):
        assert torch.equal(G.bits(run_atom(flows, mask, zx, FIX_W, dtype, max_workgroups=cap)), G.bits(ref)), cap
    for i in (0, 31, 32, 99):                           # a sample alone is the same sample in the batch
        assert torch.equal(G.bits(run_atom(flows, mask[i:i + 1], zx[i:i + 1], FIX_W, dtype)), G.bits(ref[i:i + 1])), i
    assert torch.equal(G.bits(run_atom(flows, mask[:17], zx[:17], FIX_W, dtype)), G.bits(ref[:17]))


def test_atom_envelope_and_argument_checks():
    assert F.mf_atom_supported(40, 10, [256], [512, 64], 38) and F.mf_atom_supported(8, 4, [16], [32, 8], 10)
    for bad in (dict(hidden_gnn=[16, 16]), dict(hidden_lin=[32]), dict(mask_row_size=2), dict(n_block=2), dict(n_node=65), dict(n_type=17),
                dict(hidden_lin=[1024, 8])):
        kw = dict(n_node=8, n_type=4, hidden_gnn=[16], hidden_lin=[32, 8], n_flow=10)
        kw.update(bad)
        assert not F.mf_atom_supported(**kw), bad
    flows = atom_flows(8, 4, FIX_W, 10, HF, 31)
    zx, mask = torch.randn(4, 8, 4, generator=cpu_gen(9)), adjacency("random", 4, 8, 10)
    sentinel = torch.full((4, 8, 4), 7.0, device=DEV)
    with pytest.raises(ValueError, match="tiles of 32"):
        run_atom(flows, mask, zx, FIX_W, HF, tile=64, out=sentinel)
    with pytest.raises(ValueError, match="max_workgroups"):
        run_atom(flows, mask, zx, FIX_W, HF, max_workgroups=-1, out=sentinel)
    with pytest.raises(ValueError, match="mask"):
        run_atom(flows, mask[:3], zx, FIX_W, HF, out=sentinel)
    with pytest.raises(ValueError, match="needs"):     # the weights of other widths: the pitch is too small
        run_atom(flows, mask, zx, ZINC_W, HF, out=sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
