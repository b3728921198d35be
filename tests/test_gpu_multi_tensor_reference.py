"""The multi-tensor optimizer kernels (csrc/multi_tensor.hip: l2norm, LAMB stage 1 / stage 1 with the norms / stage 2, SGD, Adam,
Adam with the 16-bit copy, EMA) against the float64 statements and derived bars of tests/_mt_reference.py, in tensor-list layouts
that reach the element-by-element branch of ld4 / st4 (views at unpadded offsets of one flat buffer, as the BERT and ResNet-50
engines cut their gradients), at the small chunks streaming_chunk() hands out, over tables of 1 to 419 tensors with empty ones.

Every case checks (a) each output element within its bar (no element excluded; ratio = |error| / bar <= 1), (b) outputs
bit-identical across layouts (and, for the elementwise kernels, across chunk sizes): alignment only changes the width of a load,
chunking only which workgroup owns a 4-group, (c) guard regions, read-only lists and tensors without a copy entry untouched.

Largest ratio per output on the GPU (MI355X), beside the float32-on-CPU ratios of tests/test_mt_reference_host.py -- a record, the
pass condition is <= 1:
    l2norm        per tensor 0.101   total 0.029   (CPU 0.117 / 0.105)
    lamb_stage1   update fp32 0.564, fp16 0.999, bf16 1.000 (a tie of the 16-bit store)   m 0.966   v 0.990
                  (CPU 0.814, 0.999, 1.000; 0.966; 0.998)
    lamb_stage1_norms   param_norm 0.058   update_norm 0.073
    lamb_stage2   p 0.998 (CPU 0.999)
    sgd           p 0.992   momentum 0.971   (CPU 0.997 / 0.968)
    adam          p 0.998   m 0.485   v 0.975   (CPU 0.998 / 0.946 / 0.988)
    adam_copy     p 0.999   m 0.912   v 0.498   (CPU 0.999 / 0.941 / 0.992)
No GPU ratio is above the float32-on-CPU one by more than the third decimal: fused multiply-adds only remove roundings.
"""
import itertools

import pytest
import torch

from tests import _mt_reference as M

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GDTYPES = [F32, F16, BF16]
RATIOS = {}
# (id, lengths, chunk, layouts): the aligned layout leads, it is the baseline of (b)
SWEEPS = {"ragged2048": (M.RAGGED(2048), 2048, M.LAYOUTS), "many": (M.MANY, 4096, ("aligned", "packed")),
          "ragged65536": (M.RAGGED(65536), 65536, ("aligned", "grad_packed"))}
LISTS = {"l2norm": ["x"], "lamb_stage1": ["g", "p", "m", "v"], "lamb_stage2": ["u", "p"], "sgd": ["g", "p", "buf"],
         "adam": ["g", "p", "m", "v"], "adam_copy": ["g", "p", "m", "v"], "ema": ["x", "e"]}
READ_ONLY = {"l2norm": ["x"], "lamb_stage1": ["p"], "lamb_stage2": ["u"], "sgd": ["g"], "adam": ["g"], "adam_copy": ["g"], "ema": ["x"]}


def _mt():
    from deeplearningexamples_amd import multi_tensor as mt
    return mt


def _name(dt):
    return "none" if dt is None else str(dt).split(".")[1]


def _word(x, dev, dtype=F32):
    return torch.tensor([x], dtype=dtype, device=dev)


def _note(key, r, where):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, "%s: |error| / bar = %.3f at %s" % (key, r, where)


def _names(kernel, cfg):
    names = list(LISTS[kernel])
    if kernel == "sgd" and not cfg["has_momentum"]:
        names.remove("buf")
    if cfg.get("cdtype") is not None:
        names.append("c")
    return names


def _values(kernel, lengths, cfg):
    n = sum(lengths)
    x = M.make_inputs(kernel, n, cfg.get("gdtype", F32))
    if kernel == "lamb_stage2" and len(lengths) > 5:          # one tensor whose update is all zero, one whose parameters are
        tid = M.tensor_index(lengths)
        x["u"][tid == 3] = 0
        x["p"][tid == 4] = 0
    if cfg.get("cdtype") is not None:
        x["c"] = torch.full((n,), 7.0, dtype=cfg["cdtype"])
    vals = {k: x[k] for k in _names(kernel, cfg)}
    assert all(bool(torch.isfinite(v.float()).all()) for v in vals.values())
    return vals


def _launch(kernel, lay, names, chunk, cfg, dev):
    """one call of the kernel over the layout's lists; -> extra outputs (norms) and the device words the reference has to read"""
    mt = _mt()
    table = mt.TensorTable(lay.lists, chunk)
    extra = {}
    if kernel == "l2norm":
        noop = torch.zeros(1, dtype=torch.int32, device=dev)
        tot, per = mt.l2norm(table, noop, per_tensor=True)
        tot_only, none = mt.l2norm(table, noop, per_tensor=False)
        assert none.numel() == 0 and int(noop) == 0
        extra = {"total": tot.cpu(), "per": per.cpu(), "total_only": tot_only.cpu()}
    elif kernel in ("lamb_stage1", "lamb_stage1_norms"):
        noop = torch.zeros(1, dtype=torch.int32, device=dev)
        fn = mt.lamb_stage1 if kernel == "lamb_stage1" else mt.lamb_stage1_norms
        r = fn(table, noop, cfg["beta1"], cfg["beta2"], cfg["beta3"], _word(cfg["step"], dev, torch.int32), cfg["bias_correction"],
               cfg["eps"], cfg["mode"], cfg["decay"], _word(cfg["ggn"], dev), _word(cfg["mgn"], dev), _word(cfg["inv_scale"], dev))
        if r is not None:
            extra = {"pn": r[0].cpu(), "un": r[1].cpu()}
        assert int(noop) == 0
    elif kernel == "lamb_stage2":
        noop = torch.zeros(1, dtype=torch.int32, device=dev)
        if "pn_un" in cfg:
            pn, un = cfg["pn_un"]
        else:                                           # the host sequence's two sweeps: the reference reads the words they stored
            _, pn = mt.l2norm(mt.TensorTable([lay.lists[1]], chunk), noop, per_tensor=True)
            _, un = mt.l2norm(mt.TensorTable([lay.lists[0]], chunk), noop, per_tensor=True)
        mt.lamb_stage2(table, noop, pn, un, _word(cfg["lr"], dev), cfg["decay"], cfg["use_nvlamb"])
        extra = {"pn": pn.cpu(), "un": un.cpu()}
    elif kernel == "sgd":
        lr = _word(cfg["lr"], dev) if cfg.get("lr_dev", True) else cfg["lr"]
        mt.sgd(table, lr, cfg["momentum"], cfg["dampening"], cfg["wd"], cfg["nesterov"], cfg["first_step"],
               skip_flag=_word(cfg["skip"], dev) if "skip" in cfg else None,
               inv_scale=None if cfg["inv_scale"] is None else _word(cfg["inv_scale"], dev), has_momentum=cfg["has_momentum"],
               model_copy=cfg.get("cdtype") is not None)
    elif kernel == "adam":
        mt.adam(table, _word(cfg["lr"], dev), cfg["beta1"], cfg["beta2"], cfg["eps"], cfg["wd"], _word(cfg["step"], dev, torch.int32),
                skip_flag=_word(cfg["skip"], dev) if "skip" in cfg else None, inv_scale=_word(cfg["inv_scale"], dev),
                grad_norm=None if cfg["gnorm"] is None else _word(cfg["gnorm"], dev), max_grad_norm=cfg["max_norm"])
    elif kernel == "adam_copy":
        tm = cfg["tensor_mul"]
        mt.adam_copy(table, cfg["lr"], _word(cfg["step"], dev, torch.int32), cfg["beta1"], cfg["beta2"], cfg["eps"],
                     skip_flag=_word(cfg["skip"], dev) if "skip" in cfg else None, inv_scale=_word(cfg["inv_scale"], dev),
                     tensor_mul=None if tm is None else tm.to(dev), model_copy=cfg.get("cdtype") is not None)
    elif kernel == "ema":
        if cfg.get("coef_dev"):
            coef = torch.tensor([cfg["mu"], 1.0 - cfg["mu"]], dtype=torch.float64).to(F32).to(dev)
            mt.ema(table, -1.0, one_minus_mu=-1.0, coef=coef)
        else:
            mt.ema(table, cfg["mu"])
    torch.cuda.synchronize()
    return extra


def _reference(kernel, vals, lengths, chunk, cfg, extra):
    """name -> (float64 value, bar) for every fp32 / gradient-dtype output; the EMA's is the torch result with a zero bar"""
    w = {k: M.widen(v) for k, v in vals.items()}
    tid = M.tensor_index(lengths)
    f = M.f32
    if kernel == "lamb_stage1":
        num = {k: cfg[k] for k in ("beta1", "beta2", "beta3", "step", "bias_correction", "eps", "mode", "decay")}
        return M.ref_lamb_stage1(w["g"], w["p"], w["m"], w["v"], cfg["gdtype"], ggn=f(cfg["ggn"]), mgn=f(cfg["mgn"]),
                                 inv_scale=f(cfg["inv_scale"]), **num)
    if kernel == "lamb_stage2":
        return M.ref_lamb_stage2(w["u"], w["p"], tid, M.widen(extra["pn"]), M.widen(extra["un"]), lr=f(cfg["lr"]), decay=cfg["decay"],
                                 use_nvlamb=cfg["use_nvlamb"])
    if kernel == "sgd":
        num = {k: cfg[k] for k in ("momentum", "dampening", "wd", "nesterov", "first_step", "has_momentum")}
        return M.ref_sgd(w["g"], w["p"], w.get("buf"), lr=f(cfg["lr"]), inv_scale=1.0 if cfg["inv_scale"] is None else f(cfg["inv_scale"]),
                         **num)
    if kernel == "adam":
        num = {k: cfg[k] for k in ("beta1", "beta2", "eps", "wd", "step", "max_norm")}
        return M.ref_adam(w["g"], w["p"], w["m"], w["v"], lr=f(cfg["lr"]), inv_scale=f(cfg["inv_scale"]),
                          gnorm=None if cfg["gnorm"] is None else f(cfg["gnorm"]), **num)
    if kernel == "adam_copy":
        num = {k: cfg[k] for k in ("beta1", "beta2", "eps", "step")}
        tm = cfg["tensor_mul"]
        return M.ref_adam_copy(w["g"], w["p"], w["m"], w["v"], tid, lr=f(cfg["lr"]), inv_scale=f(cfg["inv_scale"]),
                               tensor_mul=None if tm is None else M.widen(tm), **num)
    raise KeyError(kernel)


def _keep_mask(lengths, absent):
    tid = M.tensor_index(lengths)
    keep = torch.ones(len(lengths), dtype=torch.bool)
    keep[list(absent)] = False
    return keep[tid]


def _run(kernel, lengths, chunk, layout, cfg, dev, vals=None):
    """-> (outputs: name -> flat CPU tensor (+ norms), inputs).  Checks (c) on the way."""
    base = "lamb_stage1" if kernel == "lamb_stage1_norms" else kernel
    vals = _values(base, lengths, cfg) if vals is None else vals
    names = list(vals)
    absent = cfg.get("absent", ())
    lay = M.Layout(layout, lengths, [vals[k] for k in names], dev, absent=absent,
                   copy_list=names.index("c") if "c" in names else None)
    extra = _launch(kernel, lay, names, chunk, cfg, dev)
    out = {k: lay.flat(i) for i, k in enumerate(names)}
    assert lay.guards_intact(), "%s %s: a guard region was written" % (kernel, layout)
    for k in READ_ONLY[base]:
        assert torch.equal(M.bits(out[k]), M.bits(vals[k])), "%s %s: the read-only list %s was written" % (kernel, layout, k)
    if "c" in out:                     # the copy: torch's cast of the stored fp32 parameter, for exactly the tensors that have one
        keep = _keep_mask(lengths, absent)
        assert out["c"].numel() == int(keep.sum())
        if not cfg.get("skip"):
            assert torch.equal(M.bits(out["c"]), M.bits(out["p"][keep].to(cfg["cdtype"]))), "%s %s: copy != cast(p)" % (kernel, layout)
    out.update(extra)
    return out, vals


def _conditioned(kernel, lengths, chunk, cfg):
    """The inputs, with the precondition of the bars met: no reference value subnormal in its storage type.  Only the fp16 update of
    LAMB stage 1 can miss it (|m / sqrt(v) + decay p| < 2^-14 for a few elements in a million): their gradient is moved by 16."""
    vals = _values(kernel, lengths, cfg)
    if kernel == "lamb_stage1" and cfg["gdtype"] == F16:
        for _ in range(4):
            bad = M.subnormal(_reference(kernel, vals, lengths, chunk, cfg, {})["g"][0], F16)
            if not bool(bad.any()):
                break
            vals["g"][bad] += 16.0
    return vals


def _sweep(kernel, lengths, chunk, layouts, cfg, dev, tag):
    """(a) + (b) + (c) of one configuration over `layouts` (aligned first)"""
    first = None
    vals0 = _conditioned(kernel, lengths, chunk, cfg)
    for layout in layouts:
        if layout == "copy_half" and cfg.get("cdtype") not in (F16, BF16):
            continue                                  # (no 16-bit copy list: the layout would be `aligned` again)
        out, vals = _run(kernel, lengths, chunk, layout, cfg, dev, vals={k: v.clone() for k, v in vals0.items()})
        where = "%s/%s/chunk %d" % (tag, layout, chunk)
        if kernel == "ema":
            want = M.ref_ema(vals["x"], vals["e"], cfg["mu"])
            assert torch.equal(M.bits(out["e"]), M.bits(want)), where
        else:
            ref = _reference(kernel, vals, lengths, chunk, cfg, out)
            for k, (v, bar) in ref.items():
                dt = vals[k].dtype
                assert not bool(M.subnormal(v, dt).any()), "%s: a reference value of %s is subnormal in %s" % (where, k, dt)
                _note("%s.%s%s" % (kernel, k, "." + _name(dt) if dt != F32 else ""), M.worst_ratio(out[k], v, bar), where)
        if first is None:
            first = out
        for k in out:
            assert torch.equal(M.bits(out[k]), M.bits(first[k])), "%s: output %s differs from the aligned layout's bits" % (where, k)
    return first


def _absent(lengths):
    return tuple(range(1, len(lengths), 2))


# ------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("dtype", GDTYPES, ids=_name)
def test_l2norm(cuda, dtype, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    first = None
    for layout in [l for l in layouts if l in ("aligned", "packed", "grad_packed")]:
        out, vals = _run("l2norm", lengths, chunk, layout, dict(gdtype=dtype), cuda)
        tot, tot_bar, per, per_bar = M.ref_l2norm(list(torch.split(vals["x"], lengths)), chunk)
        where = "%s/%s" % (sweep, layout)
        _note("l2norm.per", M.worst_ratio(out["per"], per, per_bar), where)
        _note("l2norm.total", abs(float(out["total"]) - tot) / tot_bar, where)
        assert torch.equal(out["total"], out["total_only"]), "per_tensor changes the total"
        assert all(float(out["per"][i]) == 0.0 for i, n in enumerate(lengths) if n == 0)
        first = first or out
        for k in ("per", "total"):
            assert torch.equal(M.bits(out[k]), M.bits(first[k])), "%s: %s differs from the aligned layout's bits" % (where, k)


@pytest.mark.parametrize("dtype", GDTYPES, ids=_name)
def test_l2norm_inf_in_a_scalar_path_tail_raises_the_flag(cuda, dtype):
    mt = _mt()
    lengths = M.RAGGED(2048)
    vals = _values("l2norm", lengths, dict(gdtype=dtype))
    t = 4                                                  # 7 elements: the last one is in the ragged tail
    vals["x"][sum(lengths[:t + 1]) - 1] = float("inf")
    lay = M.Layout("grad_packed", lengths, [vals["x"]], cuda)
    assert lay.lists[0][t].data_ptr() % 16 != 0 and lengths[t] % 4 != 0
    noop = torch.zeros(1, dtype=torch.int32, device=cuda)
    tot, per = mt.l2norm(mt.TensorTable(lay.lists, 2048), noop, per_tensor=True)
    assert int(noop) == 1 and float(tot) == 0.0 and float(per.abs().sum()) == 0.0 and per.numel() == len(lengths)
    assert lay.guards_intact()


# ------------------------------------------------------------------------------------------------ LAMB stage 1
@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_lamb_stage1(cuda, gdtype, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    _sweep("lamb_stage1", lengths, chunk, layouts, M.stage1_cfg(gdtype=gdtype), cuda, sweep)


@pytest.mark.parametrize("mode,decay", [(0, 0.0), (0, 0.01), (1, 0.0), (1, 0.01)])
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_lamb_stage1_switches(cuda, gdtype, mode, decay):
    lengths = M.RAGGED(2048)
    for bc, ggn, step in itertools.product((0, 1), (300.0, 30.0), (1, 4)):       # bias correction, clip active / inactive, step
        cfg = M.stage1_cfg(gdtype=gdtype, mode=mode, decay=decay, bias_correction=bc, ggn=ggn, step=step)
        _sweep("lamb_stage1", lengths, 2048, ("aligned", "grad_packed"), cfg, cuda, "bc%d,ggn%g,step%d" % (bc, ggn, step))


@pytest.mark.parametrize("layout", ["aligned", "packed"])
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_lamb_stage1_norms(cuda, gdtype, layout):
    lengths, chunk = M.RAGGED(2048), 2048
    mt = _mt()
    cfg = M.stage1_cfg(gdtype=gdtype)
    a, vals = _run("lamb_stage1", lengths, chunk, layout, cfg, cuda)
    b, _ = _run("lamb_stage1_norms", lengths, chunk, layout, cfg, cuda)
    for k in "gmv":
        assert torch.equal(M.bits(a[k]), M.bits(b[k])), "stage 1 with the norms: %s differs from stage 1" % k
    # the two sweeps of the host sequence, over the same layout: p before the step, the stored update after it
    noop = torch.zeros(1, dtype=torch.int32, device=cuda)
    lp = M.Layout(layout, lengths, [vals["p"]], cuda)
    lu = M.Layout(layout, lengths, [a["g"]], cuda)
    _, pn = mt.l2norm(mt.TensorTable(lp.lists, chunk), noop, per_tensor=True)
    _, un = mt.l2norm(mt.TensorTable(lu.lists, chunk), noop, per_tensor=True)
    whole = torch.tensor([n % 4 == 0 for n in lengths])
    assert torch.equal(b["pn"][whole], pn.cpu()[whole]) and torch.equal(b["un"][whole], un.cpu()[whole])
    _, _, rp, rp_bar = M.ref_l2norm(list(torch.split(vals["p"], lengths)), chunk)
    _, _, ru, ru_bar = M.ref_l2norm(list(torch.split(a["g"], lengths)), chunk)
    for got, ref, bar, key in ((b["pn"], rp, rp_bar, "param_norm"), (b["un"], ru, ru_bar, "update_norm"), (pn, rp, rp_bar, "l2norm.per"),
                               (un, ru, ru_bar, "l2norm.per")):
        _note(key if "." in key else "lamb_stage1_norms." + key, M.worst_ratio(got, ref, bar), layout)


# ------------------------------------------------------------------------------------------------ LAMB stage 2
STAGE2 = dict(lr=6e-3, decay=0.01, use_nvlamb=0)


@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("cdtype", [None, F32, F16, BF16], ids=_name)
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_lamb_stage2(cuda, gdtype, cdtype, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    out = _sweep("lamb_stage2", lengths, chunk, layouts, dict(STAGE2, gdtype=gdtype, cdtype=cdtype), cuda, sweep)
    if len(lengths) > 5:
        assert float(out["un"][3]) == 0.0 and float(out["pn"][4]) == 0.0 and float(out["un"][4]) != 0.0


@pytest.mark.parametrize("cdtype", [None, F32, F16, BF16], ids=_name)
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_lamb_stage2_switches(cuda, gdtype, cdtype):
    for nv, decay in itertools.product((0, 1), (0.0, 0.01)):
        cfg = dict(STAGE2, gdtype=gdtype, cdtype=cdtype, use_nvlamb=nv, decay=decay)
        _sweep("lamb_stage2", M.RAGGED(2048), 2048, ("aligned", "grad_packed"), cfg, cuda, "nvlamb%d,decay%g" % (nv, decay))


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("cdtype", [None, F16, BF16], ids=_name)
@pytest.mark.parametrize("mom", [False, True], ids=["plain", "momentum"])
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_sgd(cuda, gdtype, mom, cdtype, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    cfg = M.sgd_cfg(gdtype=gdtype, has_momentum=mom, cdtype=cdtype, absent=_absent(lengths) if cdtype is not None else ())
    _sweep("sgd", lengths, chunk, layouts, cfg, cuda, sweep)


@pytest.mark.parametrize("cdtype", [None, F16, BF16], ids=_name)
@pytest.mark.parametrize("mom", [False, True], ids=["plain", "momentum"])
@pytest.mark.parametrize("gdtype", GDTYPES, ids=_name)
def test_sgd_switches(cuda, gdtype, mom, cdtype):
    lengths = M.RAGGED(2048)
    base = dict(gdtype=gdtype, has_momentum=mom, cdtype=cdtype, absent=_absent(lengths) if cdtype is not None else ())
    grid = itertools.product((False, True), (False, True), (0.0, 0.1)) if mom else [(False, False, 0.0)]
    for i, (first, nesterov, damp) in enumerate(grid):
        for wd, inv, lr_dev in ((3.0517578125e-05, 0.25, True), (0.0, None, False)):
            cfg = M.sgd_cfg(first_step=first, nesterov=nesterov, dampening=damp, wd=wd, inv_scale=inv, lr_dev=lr_dev, **base)
            _sweep("sgd", lengths, 2048, ("aligned", "grad_packed"), cfg, cuda, "first%d,nest%d,damp%g,wd%g" % (first, nesterov, damp, wd))
    out, vals = _run("sgd", lengths, 2048, "grad_packed", M.sgd_cfg(skip=1.0, **base), cuda)
    assert all(torch.equal(M.bits(out[k]), M.bits(vals[k])) for k in vals if k != "c"), "the skip flag did not skip"
    if cdtype is not None:
        assert bool((out["c"] == 7.0).all())


def test_sgd_is_chunk_invariant(cuda):
    lengths = M.RAGGED(2048)
    cfg = M.sgd_cfg(gdtype=F16, cdtype=BF16, absent=_absent(lengths))
    outs = [_run("sgd", lengths, c, "packed", cfg, cuda)[0] for c in (2048, 4096, 65536)]
    assert all(torch.equal(M.bits(o[k]), M.bits(outs[0][k])) for o in outs for k in o)


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("sweep", list(SWEEPS))
def test_adam(cuda, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    _sweep("adam", lengths, chunk, layouts, M.adam_cfg(), cuda, sweep)


def test_adam_switches_skip_and_two_steps(cuda):
    lengths = M.RAGGED(2048)
    for gnorm, wd in itertools.product((256000.0, 12800.0, None), (0.0, 1e-6)):      # clip active, inactive, absent
        _sweep("adam", lengths, 2048, ("aligned", "grad_packed"), M.adam_cfg(gnorm=gnorm, wd=wd), cuda, "gnorm%s,wd%g" % (gnorm, wd))
    out, vals = _run("adam", lengths, 2048, "grad_packed", M.adam_cfg(skip=1.0), cuda)
    assert all(torch.equal(M.bits(out[k]), M.bits(vals[k])) for k in vals), "the skip flag did not skip"
    # two consecutive steps: the second starts from the first one's stored state, with a fresh gradient
    one, _ = _run("adam", lengths, 2048, "grad_packed", M.adam_cfg(step=1), cuda)
    nxt = dict(g=M.gaussian(77, sum(lengths), 64.0), p=one["p"], m=one["m"], v=one["v"])
    cfg = M.adam_cfg(step=2)
    two, _ = _run("adam", lengths, 2048, "grad_packed", cfg, cuda, vals=nxt)
    for k, (v, bar) in _reference("adam", nxt, lengths, 2048, cfg, two).items():
        _note("adam." + k, M.worst_ratio(two[k], v, bar), "second step")
    outs = [_run("adam", lengths, c, "packed", M.adam_cfg(), cuda)[0] for c in (2048, 4096, 65536)]
    assert all(torch.equal(M.bits(o[k]), M.bits(outs[0][k])) for o in outs for k in o), "chunk size changes a bit"


@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("cdtype", [None, F16, BF16], ids=_name)
def test_adam_copy(cuda, cdtype, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    cfg = M.adam_copy_cfg(cdtype=cdtype, absent=_absent(lengths) if cdtype is not None else ())
    _sweep("adam_copy", lengths, chunk, layouts, cfg, cuda, sweep)


@pytest.mark.parametrize("cdtype", [None, F16, BF16], ids=_name)
def test_adam_copy_switches(cuda, cdtype):
    lengths = M.RAGGED(2048)
    base = dict(cdtype=cdtype, absent=_absent(lengths) if cdtype is not None else ())
    tm = (0.125 + (torch.arange(len(lengths)) % 3) * 0.4375).to(F32)
    for mul, eps in itertools.product((None, tm), (1e-8, 1e-2)):
        cfg = M.adam_copy_cfg(tensor_mul=mul, eps=eps, **base)
        _sweep("adam_copy", lengths, 2048, ("aligned", "grad_packed"), cfg, cuda, "mul%d,eps%g" % (mul is not None, eps))
    out, vals = _run("adam_copy", lengths, 2048, "grad_packed", M.adam_copy_cfg(skip=1.0, **base), cuda)
    assert all(torch.equal(M.bits(out[k]), M.bits(vals[k])) for k in vals if k != "c"), "the skip flag did not skip"
    outs = [_run("adam_copy", lengths, c, "packed", M.adam_copy_cfg(**base), cuda)[0] for c in (2048, 4096, 65536)]
    assert all(torch.equal(M.bits(o[k]), M.bits(outs[0][k])) for o in outs for k in o), "chunk size changes a bit"


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("coef_dev", [False, True], ids=["host_coef", "device_coef"])
@pytest.mark.parametrize("mu", [0.9, 0.9999])
def test_ema(cuda, mu, coef_dev, sweep):
    lengths, chunk, layouts = SWEEPS[sweep]
    _sweep("ema", lengths, chunk, layouts, dict(mu=mu, coef_dev=coef_dev), cuda, sweep)


# ------------------------------------------------------------------------------------------------ chunk invariance, tables
@pytest.mark.parametrize("kernel,cfg", [("lamb_stage1", M.stage1_cfg(gdtype=BF16)),
                                        ("lamb_stage2", dict(STAGE2, gdtype=F16, cdtype=F16, decay=0.0)), ("ema", dict(mu=0.9999))],
                         ids=["stage1", "stage2", "ema"])
def test_elementwise_outputs_do_not_depend_on_the_chunk(cuda, kernel, cfg):
    """(stage 2 without decay: ratio = lr.  With decay its ratio comes from the l2norm sweeps, whose sums do depend on the chunk.)"""
    lengths = M.RAGGED(2048)
    outs = [_run(kernel, lengths, c, "packed", cfg, cuda)[0] for c in (2048, 4096, 65536)]
    keys = [k for k in outs[0] if k not in ("pn", "un")]
    assert all(torch.equal(M.bits(o[k]), M.bits(outs[0][k])) for o in outs for k in keys)


CASES = {"l2norm": dict(gdtype=F16), "lamb_stage1": M.stage1_cfg(gdtype=F16), "lamb_stage1_norms": M.stage1_cfg(gdtype=F16),
         "lamb_stage2": dict(STAGE2, gdtype=F16, cdtype=F16), "sgd": M.sgd_cfg(gdtype=F16, cdtype=F16),
         "adam": M.adam_cfg(), "adam_copy": M.adam_copy_cfg(cdtype=BF16), "ema": dict(mu=0.9)}


@pytest.mark.parametrize("table", list(M.DEGENERATE))
@pytest.mark.parametrize("kernel", [k for k in CASES if k != "lamb_stage1_norms"])
def test_tables_of_one_two_and_three_tensors(cuda, kernel, table):
    lengths = M.DEGENERATE[table]
    if kernel == "l2norm":
        out, vals = _run(kernel, lengths, 2048, "packed", CASES[kernel], cuda)
        tot, tot_bar, per, per_bar = M.ref_l2norm(list(torch.split(vals["x"], lengths)), 2048)
        _note("l2norm.per", M.worst_ratio(out["per"], per, per_bar), table)
        _note("l2norm.total", abs(float(out["total"]) - tot) / tot_bar, table)
    else:
        _sweep(kernel, lengths, 2048, ("aligned", "packed"), CASES[kernel], cuda, table)


@pytest.mark.parametrize("lengths", [[], [0, 0, 0]], ids=["n0", "all_empty"])
@pytest.mark.parametrize("kernel", list(CASES))
def test_empty_tables(cuda, kernel, lengths):
    if kernel == "l2norm" and lengths:                # whatever torch.empty hands l2norm next: not zeros
        poison = [torch.full((len(lengths),), float("nan"), device=cuda) for _ in range(8)]
        del poison
    cfg = CASES[kernel] if lengths else {k: v for k, v in CASES[kernel].items() if k != "cdtype"}    # (no tensor, no copy dtype)
    out, vals = _run(kernel, lengths, 2048, "aligned", cfg, cuda)
    assert all(v.numel() == 0 for k, v in out.items() if k in vals)
    if kernel == "l2norm":
        assert float(out["total"]) == 0.0 and out["per"].numel() == len(lengths) and bool((M.bits(out["per"]) == 0).all())
    if kernel == "lamb_stage1_norms":
        assert out["pn"].numel() == len(lengths) and bool((M.bits(out["pn"]) == 0).all()) and bool((M.bits(out["un"]) == 0).all())


@pytest.mark.parametrize("bad", [dict(chunk=0), dict(chunk=-4), dict(chunk=6), dict(total_chunks=-1)],
                         ids=["chunk0", "chunk-4", "chunk6", "chunks-1"])
@pytest.mark.parametrize("kernel", list(CASES))
def test_bad_chunk_is_an_argument_error_and_launches_nothing(cuda, kernel, bad):
    """every entry point answers the library's argument error (-1 -> ValueError with the message of dle_last_error()) to a chunk that
    is not a positive multiple of 4 and to a chunk count that is no grid size; the lists keep their bits"""
    mt = _mt()
    lengths = [5, 2050]
    cfg = dict(CASES[kernel], pn_un=(torch.ones(2, device=cuda), torch.ones(2, device=cuda)))
    base = "lamb_stage1" if kernel == "lamb_stage1_norms" else kernel
    vals = _values(base, lengths, cfg)
    names = list(vals)
    lay = M.Layout("aligned", lengths, [vals[k] for k in names], cuda)
    real = mt.TensorTable

    class Table(real):                                 # a well-formed table that then claims the bad chunk / chunk count
        def __init__(self, lists, chunk=2048):
            real.__init__(self, lists, 2048)
            for k, v in bad.items():
                setattr(self, k, v)

    mt.TensorTable = Table
    try:
        with pytest.raises(ValueError, match="chunk"):
            _launch(kernel, lay, names, 2048, cfg, cuda)
    finally:
        mt.TensorTable = real
    torch.cuda.synchronize()
    assert lay.guards_intact()
    for i, k in enumerate(names):
        assert torch.equal(M.bits(lay.flat(i)), M.bits(vals[k])), "%s ran with %r" % (kernel, bad)


def test_a_chunk_count_past_int_max_is_an_argument_error(cuda):
    from deeplearningexamples_amd import _cabi as C
    x, e = torch.zeros(8, device=cuda), torch.ones(8, device=cuda)
    table = _mt().TensorTable([[x], [e]], 2048)
    with pytest.raises(ValueError, match="total_chunks"):
        C.call("dle_mt_ema", C.ptr(table.table), 1, 2 ** 31, 2048, 0, 0.5, 0.5, C.stream())
    torch.cuda.synchronize()
    assert float(e.sum()) == 8.0


def test_zz_report_ratios():
    """(runs last in this file) the record quoted in the module docstring; -s shows it"""
    for k in sorted(RATIOS):
        print("GPU ratio %-32s %.3f" % (k, RATIOS[k]))
    assert all(r <= 1.0 for r in RATIOS.values())
