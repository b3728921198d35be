"""CPU checks of tests/_mt_reference.py, before a GPU is involved: the float64 statements agree with independent ones
(oracle/lamb_oracle.py, torch.optim.SGD and torch.optim.Adam in float64, the apex FusedAdam formula), a float32 evaluation of
every statement stays inside the derived bar on every length set and seed tests/test_gpu_multi_tensor_reference.py uses (no element
excluded), and the layout builder delivers the pointer residues and guard regions it promises.

Largest |float32 evaluation - float64 value| / bar per output over those runs.  The bars are tight: an output's last rounding
alone is worth up to 2^-24 |value| of a bar that is seldom more than a few times that, so an element just above a power of two
comes close to 1; a count of roundings one too low shows as a ratio above 1 (and did, while this file was written).
    l2norm (numpy pairwise sum)   per tensor 0.117   total 0.105   (the bar is for the kernel's longer chain)
    lamb_stage1   update fp32 0.814, fp16 0.999, bf16 1.000 (ties of the 16-bit store: exactly half an ulp)   m 0.966   v 0.998
    lamb_stage2   p 0.999
    sgd           p 0.997   momentum 0.968
    adam          p 0.998   m 0.946   v 0.988
    adam_copy     p 0.999   m 0.941   v 0.992
"""
import numpy as np
import pytest
import torch

from oracle import lamb_oracle as L
from tests import _mt_reference as M

F64 = torch.float64
SETS = {"ragged2048": M.RAGGED(2048), "many": M.MANY, "ragged65536": M.RAGGED(65536)}
GDTYPES = [torch.float32, torch.float16, torch.bfloat16]
RATIOS = {}


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, "%s: a float32 evaluation leaves the bar (ratio %.3f): the count of roundings is wrong" % (key, r)


def _np(t):
    return t.float().numpy()


def _cast(dtype):
    return lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype).float().numpy()


# ------------------------------------------------------------------------------------ float32 evaluations stay inside the bars
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("dtype", GDTYPES, ids=str)
def test_l2norm_float32_sum_is_inside_the_bar(name, dtype):
    lengths = SETS[name]
    chunk = {"ragged2048": 2048, "many": 4096, "ragged65536": 65536}[name]
    xs = list(torch.split(M.make_inputs("l2norm", sum(lengths), dtype)["x"], lengths))
    tot, tot_bar, per, per_bar = M.ref_l2norm(xs, chunk)
    t32, p32 = L.l2norm([_np(x) for x in xs])
    sq = np.float32(0)
    for x in xs:                                           # a serial fp32 chain over the tensors for the total
        sq = np.float32(sq + np.sum(np.square(_np(x)), dtype=np.float32))
    _note("l2norm.per", M.worst_ratio(torch.from_numpy(p32), per, per_bar))
    _note("l2norm.total", abs(float(np.sqrt(sq)) - tot) / tot_bar)
    empty = [i for i, n in enumerate(lengths) if n == 0]
    assert empty and all(float(per[i]) == 0.0 and float(per_bar[i]) == 0.0 for i in empty)


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("dtype", GDTYPES, ids=str)
@pytest.mark.parametrize("mode,decay,bc,clip,step", [(1, 0.01, 1, True, 4), (0, 0.01, 1, False, 1), (1, 0.0, 0, True, 4),
                                                     (0, 0.0, 0, False, 4)])
def test_lamb_oracle_is_inside_the_bars(name, dtype, mode, decay, bc, clip, step):
    """oracle.lamb_oracle.lamb_step (fp32 numpy, the .cu restated line by line) against ref_lamb_stage1 and ref_lamb_stage2."""
    n = sum(SETS[name])
    # (the oracle takes its betas as Python doubles and beta3 as 1 - beta1: hand it what the kernel's float parameters hold)
    cfg = M.stage1_cfg(mode=mode, decay=decay, bias_correction=bc, step=step, ggn=300.0 if clip else 30.0, beta1=M.f32(0.9),
                       beta2=M.f32(0.999), beta3=1.0 - M.f32(0.9))
    x = M.make_inputs("lamb_stage1", n, dtype)
    ref = M.ref_lamb_stage1(M.widen(x["g"]), M.widen(x["p"]), M.widen(x["m"]), M.widen(x["v"]), dtype, **cfg)
    assert not bool(M.subnormal(ref["m"][0], torch.float32).any()) and not bool(M.subnormal(ref["v"][0], torch.float32).any())
    upd, p2, m2, v2, _ = L.lamb_step([_np(x["g"])], [_np(x["p"])], [_np(x["m"])], [_np(x["v"])], 6e-3, cfg["beta1"], cfg["beta2"],
                                     cfg["eps"], step, bool(bc), decay, True, mode, np.float32(cfg["ggn"]), np.float32(cfg["mgn"]),
                                     inv_scale=cfg["inv_scale"], round_update=None if dtype == torch.float32 else _cast(dtype))
    tag = "stage1.%s." % str(dtype).split(".")[1]
    _note(tag + "g", M.worst_ratio(torch.from_numpy(upd[0]), *ref["g"]))
    _note("stage1.m", M.worst_ratio(torch.from_numpy(m2[0]), *ref["m"]))
    _note("stage1.v", M.worst_ratio(torch.from_numpy(v2[0]), *ref["v"]))
    # stage 2 of the same oracle step: its own stored update and its own norms are the inputs
    u = torch.from_numpy(upd[0])
    pn = torch.tensor([float(np.sqrt(np.sum(np.square(_np(x["p"])), dtype=np.float32)))], dtype=F64)
    un = torch.tensor([float(np.sqrt(np.sum(np.square(upd[0]), dtype=np.float32)))], dtype=F64)
    r2 = M.ref_lamb_stage2(M.widen(u), M.widen(x["p"]), torch.zeros(n, dtype=torch.int64), pn, un, lr=M.f32(6e-3), decay=decay,
                           use_nvlamb=False)
    _note("stage2.p", M.worst_ratio(torch.from_numpy(p2[0]), *r2["p"]))


@pytest.mark.parametrize("nvlamb,decay", [(0, 0.0), (1, 0.0), (0, 0.01), (1, 0.01)])
@pytest.mark.parametrize("dtype", GDTYPES, ids=str)
def test_lamb_stage2_float32_is_inside_the_bar(dtype, nvlamb, decay):
    lengths = M.RAGGED(2048)
    x = M.make_inputs("lamb_stage2", sum(lengths), dtype)
    tid = M.tensor_index(lengths)
    u, p = x["u"].float().clone(), x["p"].clone()
    u[tid == 3] = 0
    p[tid == 4] = 0
    f = np.float32
    pn = torch.tensor([np.sqrt(np.sum(np.square(_np(t)), dtype=f)) for t in torch.split(p, lengths)])
    un = torch.tensor([np.sqrt(np.sum(np.square(_np(t)), dtype=f)) for t in torch.split(u, lengths)])
    ref = M.ref_lamb_stage2(M.widen(u), M.widen(p), tid, M.widen(pn), M.widen(un), lr=M.f32(6e-3), decay=decay, use_nvlamb=nvlamb)
    lr = torch.tensor(6e-3)
    ratio = lr.expand(len(lengths)).clone()
    if nvlamb or decay != 0:
        ok = (pn != 0) & (un != 0)
        ratio = torch.where(ok, lr * (pn / torch.where(ok, un, torch.ones_like(un))), lr)
        assert float(ratio[3]) == float(lr) and float(ratio[4]) == float(lr) and float(ratio[6]) != float(lr)
    _note("stage2.p", M.worst_ratio(p - ratio[tid] * u, *ref["p"]))


SGD_CASES = [dict(has_momentum=False, wd=0.0, inv_scale=1.0), dict(has_momentum=False), dict(first_step=True),
             dict(nesterov=True), dict(dampening=0.1), dict(dampening=0.1, nesterov=True, first_step=True),
             dict(dampening=0.1, nesterov=True)]


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("dtype", GDTYPES, ids=str)
def test_sgd_oracle_is_inside_the_bars(name, dtype):
    n = sum(SETS[name])
    x = M.make_inputs("sgd", n, dtype)
    for over in SGD_CASES:
        cfg = M.sgd_cfg(**over)
        ref = M.ref_sgd(M.widen(x["g"]), M.widen(x["p"]), M.widen(x["buf"]), **dict(cfg, lr=M.f32(cfg["lr"]),
                                                                                     inv_scale=M.f32(cfg["inv_scale"])))
        p2, b2 = L.sgd_step(_np(x["g"]), _np(x["p"]), _np(x["buf"]), cfg["lr"], cfg["momentum"] if cfg["has_momentum"] else 0.0,
                            cfg["dampening"], cfg["wd"], cfg["nesterov"], first=cfg["first_step"], inv_scale=cfg["inv_scale"])
        _note("sgd.p", M.worst_ratio(torch.from_numpy(p2), *ref["p"]))
        if cfg["has_momentum"]:
            _note("sgd.buf", M.worst_ratio(torch.from_numpy(np.asarray(b2)), *ref["buf"]))


def _adam32(x, cfg):
    """mt_adam's statement in torch float32 ops (one rounding each, no contraction)"""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    g, p, m, v = x["g"], x["p"], x["m"], x["v"]
    b1, b2, eps, wd, isc = t(cfg["beta1"]), t(cfg["beta2"]), t(cfg["eps"]), t(cfg["wd"]), t(cfg["inv_scale"])
    gs = isc
    if cfg["gnorm"] is not None and cfg["max_norm"] > 0:
        coef = t(cfg["max_norm"]) / (t(cfg["gnorm"]) * isc + t(1e-6))
        if coef < 1:
            gs = isc * coef
    gr = g * gs + wd * p
    m2 = b1 * m + (1 - b1) * gr
    v2 = b2 * v + (1 - b2) * gr * gr
    bc1 = t(1.0 - float(b1) ** cfg["step"])
    bc2 = t(1.0 - float(b2) ** cfg["step"])
    p2 = p - (t(cfg["lr"]) / bc1) * m2 / (torch.sqrt(v2) * (1 / torch.sqrt(bc2)) + eps)
    return p2, m2, v2


def _adam_copy32(x, cfg, tid):
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    g, p, m, v = x["g"], x["p"], x["m"], x["v"]
    b1, b2, eps = t(cfg["beta1"]), t(cfg["beta2"]), t(cfg["eps"])
    gs = t(cfg["inv_scale"]) * (cfg["tensor_mul"][tid] if cfg["tensor_mul"] is not None else t(1.0))
    gr = g * gs
    m2 = b1 * m + (1 - b1) * gr
    v2 = b2 * v + (1 - b2) * gr * gr
    bc1 = t(1.0 - float(b1) ** cfg["step"])
    bc2 = t(1.0 - float(b2) ** cfg["step"])
    p2 = p - t(cfg["lr"]) * ((m2 / bc1) / (torch.sqrt(v2 / bc2) + eps))
    return p2, m2, v2


@pytest.mark.parametrize("name", list(SETS))
def test_adam_float32_is_inside_the_bars(name):
    n = sum(SETS[name])
    x = M.make_inputs("adam", n)
    for over in [dict(), dict(gnorm=12800.0), dict(gnorm=None), dict(wd=0.0), dict(step=1, wd=0.0, gnorm=None)]:
        cfg = M.adam_cfg(**over)
        ref = M.ref_adam(*(M.widen(x[k]) for k in "gpmv"), **dict(cfg, lr=M.f32(cfg["lr"]), inv_scale=M.f32(cfg["inv_scale"]),
                                                                 gnorm=None if cfg["gnorm"] is None else M.f32(cfg["gnorm"])))
        for k, got in zip("pmv", _adam32(x, cfg)):
            _note("adam." + k, M.worst_ratio(got, *ref[k]))


@pytest.mark.parametrize("name", list(SETS))
def test_adam_copy_float32_is_inside_the_bars(name):
    lengths = SETS[name]
    n, tid = sum(lengths), M.tensor_index(lengths)
    x = M.make_inputs("adam_copy", n)
    tm = M.gaussian(5, len(lengths), 0.0, floor=0.125) + torch.arange(len(lengths)) % 3 * 0.4375
    for over in [dict(), dict(tensor_mul=tm), dict(eps=1e-2), dict(eps=1e-2, tensor_mul=tm, step=1)]:
        cfg = M.adam_copy_cfg(**over)
        ref = M.ref_adam_copy(*(M.widen(x[k]) for k in "gpmv"), tid,
                              **dict(cfg, lr=M.f32(cfg["lr"]), inv_scale=M.f32(cfg["inv_scale"]),
                                     tensor_mul=None if cfg["tensor_mul"] is None else M.widen(cfg["tensor_mul"])))
        for k, got in zip("pmv", _adam_copy32(x, cfg, tid)):
            _note("adam_copy." + k, M.worst_ratio(got, *ref[k]))


def test_zz_report_ratios():
    """(runs last in this file) the record quoted in the module docstring; -s shows it"""
    for k in sorted(RATIOS):
        print("%-22s %.3f" % (k, RATIOS[k]))
    assert all(0.0 < r <= 1.0 for r in RATIOS.values()) or not RATIOS


# ------------------------------------------------------------------------------------ independent float64 statements
def _f(x):
    return M.f32(x)


@pytest.mark.parametrize("nesterov,dampening", [(False, 0.0), (True, 0.0), (False, 0.1)])
@pytest.mark.parametrize("wd", [0.0, 3.0517578125e-05])
def test_sgd_statement_is_torch_sgd_in_float64(nesterov, dampening, wd):
    x = M.make_inputs("sgd", 1000)
    p = torch.nn.Parameter(M.widen(x["p"]).clone())
    opt = torch.optim.SGD([p], lr=_f(0.1), momentum=_f(0.875), dampening=_f(dampening), weight_decay=_f(wd), nesterov=nesterov)
    mine_p, mine_b = M.widen(x["p"]), torch.zeros(1000, dtype=F64)
    for it in range(3):
        g = M.widen(M.gaussian(900 + it, 1000))
        p.grad = g * _f(0.25)
        opt.step()
        out = M.ref_sgd(g, mine_p, mine_b, lr=_f(0.1), momentum=0.875, dampening=dampening, wd=wd, nesterov=nesterov,
                        first_step=(it == 0), inv_scale=_f(0.25), has_momentum=True)
        mine_p, mine_b = out["p"][0], out["buf"][0]
        torch.testing.assert_close(mine_p, p.detach(), rtol=1e-13, atol=1e-14)
        torch.testing.assert_close(mine_b, opt.state[p]["momentum_buffer"], rtol=1e-13, atol=1e-14)
    plain = M.ref_sgd(g, mine_p, None, lr=_f(0.1), momentum=0.0, dampening=0.0, wd=wd, nesterov=False, first_step=False,
                      inv_scale=1.0, has_momentum=False)
    torch.testing.assert_close(plain["p"][0], mine_p - _f(0.1) * (g + _f(wd) * mine_p), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("wd", [0.0, 1e-6])
def test_adam_statement_is_torch_adam_in_float64(wd):
    x = M.make_inputs("adam", 1000)
    p = torch.nn.Parameter(M.widen(x["p"]).clone())
    opt = torch.optim.Adam([p], lr=_f(1e-3), betas=(_f(0.9), _f(0.999)), eps=_f(1e-6), weight_decay=_f(wd))
    mp, mm, mv = M.widen(x["p"]), torch.zeros(1000, dtype=F64), torch.zeros(1000, dtype=F64)
    for it in range(3):
        g = M.widen(M.gaussian(700 + it, 1000))
        p.grad = g.clone()
        opt.step()
        out = M.ref_adam(g, mp, mm, mv, lr=_f(1e-3), beta1=0.9, beta2=0.999, eps=1e-6, wd=wd, step=it + 1, inv_scale=1.0,
                         gnorm=None, max_norm=0.0)
        mp, mm, mv = out["p"][0], out["m"][0], out["v"][0]
        torch.testing.assert_close(mp, p.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(mm, opt.state[p]["exp_avg"], rtol=1e-12, atol=1e-16)
        torch.testing.assert_close(mv, opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=1e-16)
    # unscale and clip: grad = g * inv_scale * min(1, max_norm / (||g|| inv_scale + 1e-6))  (clip_grad_norm_)
    g = M.widen(x["g"][:1000])
    gn, isc = _f(256000.0), _f(1.0 / 128.0)
    coef = _f(1000.0) / (gn * isc + _f(1e-6))
    a = M.ref_adam(g, mp, mm, mv, lr=_f(1e-3), beta1=0.9, beta2=0.999, eps=1e-6, wd=wd, step=4, inv_scale=isc, gnorm=gn, max_norm=1000.0)
    b = M.ref_adam(g * isc * coef, mp, mm, mv, lr=_f(1e-3), beta1=0.9, beta2=0.999, eps=1e-6, wd=wd, step=4, inv_scale=1.0, gnorm=None,
                   max_norm=0.0)
    assert coef < 1
    for k in "pmv":
        torch.testing.assert_close(a[k][0], b[k][0], rtol=1e-12, atol=1e-16)


def test_adam_copy_statement_is_the_fused_adam_formula():
    """apex FusedAdam, ADAM_MODE_0 without decay: p -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)"""
    lengths = [300, 0, 700]
    x = M.make_inputs("adam_copy", 1000)
    tid = M.tensor_index(lengths)
    tm = torch.tensor([0.5, 2.0, 0.25], dtype=F64)
    g, p, m, v = (M.widen(x[k]) for k in "gpmv")
    b1, b2, eps, lr, isc, t = _f(0.9), _f(0.999), _f(1e-8), _f(1e-3), _f(1 / 128.0), 5
    grad = g * isc * tm[tid]
    m2 = b1 * m + (1 - b1) * grad
    v2 = b2 * v + (1 - b2) * grad * grad
    p2 = p - lr * (m2 / (1 - b1 ** t)) / ((v2 / (1 - b2 ** t)).sqrt() + eps)
    out = M.ref_adam_copy(g, p, m, v, tid, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, step=t, inv_scale=isc, tensor_mul=tm)
    for k, want in zip("pmv", (p2, m2, v2)):
        torch.testing.assert_close(out[k][0], want, rtol=1e-12, atol=1e-16)


def test_lamb_statement_matches_a_float64_closed_form():
    x = M.make_inputs("lamb_stage1", 500, torch.float32)
    g, p, m, v = (M.widen(x[k]) for k in "gpmv")
    cfg = M.stage1_cfg()
    b1, b2, b3 = _f(0.9), _f(0.999), _f(0.1)
    sg = g * cfg["inv_scale"] / (300.0 / 128.0)
    for mode in (0, 1):
        s = sg + _f(0.01) * p if mode == 0 else sg
        m2, v2 = b1 * m + b3 * s, b2 * v + (1 - b2) * s * s
        u = (m2 / (1 - b1 ** 4)) / ((v2 / (1 - b2 ** 4)).sqrt() + _f(1e-6)) + (0 if mode == 0 else _f(0.01) * p)
        out = M.ref_lamb_stage1(g, p, m, v, torch.float32, **dict(cfg, mode=mode))
        for k, want in zip("gmv", (u, m2, v2)):
            torch.testing.assert_close(out[k][0], want, rtol=1e-12, atol=1e-16)
            assert bool((out[k][1] > 0).all()) and float((out[k][1] / want.abs().clamp_min(1e-3)).max()) < 1e-4
    noclip = M.ref_lamb_stage1(g, p, m, v, torch.float32, **dict(cfg, ggn=30.0, bias_correction=0))
    torch.testing.assert_close(noclip["m"][0], b1 * m + b3 * g * cfg["inv_scale"], rtol=1e-12, atol=1e-16)


def test_ema_statement_is_the_two_tensor_ops():
    from tests.test_ema_reference import ema_three_roundings
    x = M.make_inputs("ema", 4099)
    for mu in (0.9, 0.9999):
        got = M.ref_ema(x["x"], x["e"], mu)
        want = torch.from_numpy(ema_three_roundings(x["e"].numpy(), x["x"].numpy(), mu))
        assert torch.equal(M.bits(got), M.bits(want))


def test_norm_depth_and_bar():
    assert M.norm_depth(2048, 1) == 4 + 1 + 1 + 14 + 1 + 14
    assert M.norm_depth(65536, 1) == 4 + 32 + 1 + 14 + 1 + 14
    assert M.norm_depth(4096, 513) == M.norm_depth(4096, 512) + 1
    assert 17 * M.U < M.norm_rel_bar(2048, 1) < 19 * M.U        # (35 / 2 + 1) u: far inside the 2e-5 the older test allows


# ------------------------------------------------------------------------------------ the layout builder
@pytest.mark.parametrize("name", M.LAYOUTS)
@pytest.mark.parametrize("lengths", [M.RAGGED(2048), M.MANY, M.DEGENERATE["n3"]], ids=["ragged", "many", "n3"])
def test_layouts_on_cpu(name, lengths):
    n = sum(lengths)
    dts = [torch.float16, torch.float32, torch.float32, torch.bfloat16]
    vals = [M.gaussian(40 + i, n, 1.0, d) for i, d in enumerate(dts)]
    absent = {1, 5} if len(lengths) > 5 else {0}
    lay = M.Layout(name, lengths, vals, torch.device("cpu"), absent=absent, copy_list=3)     # (asserts the residues itself)
    assert lay.guards_intact()
    for l, d in enumerate(dts):
        views = lay.lists[l]
        assert [v is None for v in views] == [(l == 3 and t in absent) for t in range(len(lengths))]
        keep = torch.cat([torch.ones(k, dtype=torch.bool) if views[t] is not None else torch.zeros(k, dtype=torch.bool)
                          for t, k in enumerate(lengths)])
        assert torch.equal(M.bits(lay.flat(l)), M.bits(vals[l][keep]))
        # guard regions are disjoint from every view, and a guard sits directly before and after every tensor or run of tensors
        mask = lay.masks[l]
        spans = [s for s in lay.spans[l] if s is not None]
        assert all(not bool(mask[a:b].any()) for a, b in spans)
        assert int((~mask).sum()) == sum(b - a for a, b in spans)
        assert bool(mask[:M.GUARD].all()) and bool(mask[-M.GUARD:].all())
        first, last = min(a for a, _ in spans), max(b for _, b in spans)
        assert first >= M.GUARD and bool(mask[first - M.GUARD:first].all()) and bool(mask[last:last + M.GUARD].all())
        packed = {"aligned": False, "packed": True, "grad_packed": l == 0, "state_packed": l != 0, "copy_half": False}[name]
        if not packed:
            assert all(bool(mask[b:b + M.GUARD].all()) for _, b in spans)
    if name == "aligned":                      # a write one element past a tensor is seen
        t = next(i for i, k in enumerate(lengths) if k)
        lay.arenas[1][lay.spans[1][t][1]] = 1.0
        assert not lay.guards_intact()


def test_length_sets():
    assert len(M.MANY) == 419 and M.MANY[0] == 0 and M.MANY[-1] == 0 and M.MANY[200:203] == [0, 0, 0]
    assert max(M.MANY) <= 5000 and sum(1 for n in M.MANY if n == 0) >= 5
    r = M.RAGGED(2048)
    assert {n % 4 for n in r if n} == {0, 1, 2, 3} and 0 in r[1:-1] and 2 * 2048 + 2 in r
    assert [len(v) for v in M.DEGENERATE.values()] == [1, 2, 3]
