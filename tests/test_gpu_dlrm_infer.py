"""DLRM inference: the fused gather + interaction launch (dle_dlrm_gather_interact_try), DlrmPredictor and --mode
inference_benchmark.  GPU only.

The fused kernel's contract is the bits of dle_dot_interact_fwd over cat(mlp_out, table16[rows]); against float64 it is checked on
exactly summable inputs (tests/_exact_grid.py), where the fp32 accumulation is exact in any order and the output is the float64
value rounded once.  The predictor's contract is the bits of DistributedDlrm.forward on the same weights."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import dlrm_step_oracle as SO
from tests import _dlrm_reference as D
from tests._exact_grid import B_MFMA, Out, assert_same, bits, grid

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# the launch rule of the persistent walk (csrc/dot_interact.hip): at most 2 workgroups on each of 256 CUs, 4 wavefronts (samples)
# per workgroup and lap.  The ids run two laps ahead of the products, so the lap case walks a third lap for five wavefronts.
LAP = 256 * 2 * 4
BATCHES = [1, 3, 4, 5, 64, 257, 2 * LAP + 5]
SHAPES = [(26, 128), (1, 16), (31, 128), (26, 64)]
SIZES = [7, 1, 1000, 33, 129, 2, 500]


def _F():
    from deeplearningexamples_amd import functional as F
    return F


def _sizes(tables):
    return [SIZES[t % len(SIZES)] for t in range(tables)]


def _case(tables, dim, dtype, batch, mode, dev, seed=0):
    """-> table16, indices (as handed to the kernel), offsets, hash_sizes, mlp_out, joint rows (the float64-side statement of the
    index arithmetic, D.hash_offset).  mode: "joint" (ids address the joint table), "offsets", "hash" (offsets + floor-mod hashing
    with ids above the table size and negative ones)."""
    g = torch.Generator().manual_seed(1000 * tables + dim + 7 * batch + seed)
    sizes = torch.tensor(_sizes(tables), dtype=torch.int64)
    off = D.table_offsets(sizes.tolist())
    total = int(off[-1])
    table = torch.randn((total, dim), generator=g).to(dtype)
    mlp = torch.randn((batch, dim), generator=g).to(dtype)
    idx = torch.cat([torch.randint(0, int(s), (batch, 1), generator=g) for s in sizes], 1)
    if batch > 1:
        idx[1, :] = 0                               # one id for every slot of the sample
    idx[0, 0] = 0                                   # first row of the first table
    last = (0, tables - 1) if tables > 1 else (batch - 1, 0)
    if tables > 1 or batch > 1:
        idx[last] = sizes[-1] - 1                   # last row of the last table
    if mode == "joint":
        ids = idx + off[None, :tables]
        if batch > 2:
            ids[2, :] = ids[2, 0]                   # the SAME joint row in every slot
        rows, offsets, hs = ids.clone(), None, None
    elif mode == "offsets":
        ids, offsets, hs = idx, off[:tables].clone(), None
        rows = D.hash_offset(ids, offsets, None)
    else:
        wrap = torch.randint(-3, 4, idx.shape, generator=g)
        ids, offsets, hs = idx + wrap * sizes[None, :], off[:tables].clone(), sizes
        rows = D.hash_offset(ids, offsets, hs)
        assert bool((ids >= sizes[None, :]).any()) or batch < 3
    assert int(rows.min()) >= 0 and int(rows.max()) < total
    assert int(rows[0, 0]) == 0 and (int(rows[last]) == total - 1 or (tables == 1 and batch == 1))
    mv = lambda t: None if t is None else t.to(dev)
    return mv(table), mv(ids), mv(offsets), mv(hs), mv(mlp), mv(rows)


def _unfused(table, rows, mlp):
    return _F().dot_interact_fwd(torch.cat([mlp[:, None, :], table[rows]], 1))


def _fused_checked(table, ids, offsets, hs, mlp, what):
    F = _F()
    b, t, d = ids.shape[0], ids.shape[1], table.shape[1]
    o = Out((b, F.dot_interact_out_width(t + 1, d)), table.dtype, table.device)
    got = F.gather_interact(table, ids, offsets, hs, mlp, out=o.t)
    torch.cuda.synchronize()
    assert got is not None, "%s: the kernel declined a shape inside its envelope" % what
    return o.check(what)


# ------------------------------------------------------------------------------------------------ 1. fused == unfused
@pytest.mark.parametrize("dtype", [F16, BF16], ids=D.name)
@pytest.mark.parametrize("shape", SHAPES + [(3, 48)], ids=lambda s: "%dx%d" % s)        # (3, 48): the one-shot form
def test_fused_equals_unfused_bit_for_bit(cuda, shape, dtype):
    tables, dim = shape
    assert BATCHES[-1] > 2 * LAP
    for batch in BATCHES:
        for mode in ("joint", "offsets", "hash"):
            table, ids, offsets, hs, mlp, rows = _case(tables, dim, dtype, batch, mode, cuda)
            what = "gather_interact %dx%d %s batch %d %s" % (tables, dim, D.name(dtype), batch, mode)
            got = _fused_checked(table, ids, offsets, hs, mlp, what)
            assert_same(bits(got), bits(_unfused(table, rows, mlp)), what)


# ------------------------------------------------------------------------------------------------ 2. exact against float64
@pytest.mark.parametrize("dtype", [F16, BF16], ids=D.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fused_exact_against_float64(cuda, shape, dtype):
    tables, dim = shape
    batch = 2 * LAP + 5
    sizes = _sizes(tables)
    off = D.table_offsets(sizes)
    total = int(off[-1])
    table = grid((total, dim), 11 * tables + dim, dtype, "cpu")
    mlp = grid((batch, dim), 13 * tables + dim, dtype, "cpu")
    g = torch.Generator().manual_seed(5)
    idx = torch.cat([torch.randint(0, s, (batch, 1), generator=g) for s in sizes], 1)
    if total >= 8 and tables >= 8:
        # rows of 3/4 and 1 throughout: their pairs sum to ~0.77 dim in multiples of 1/16 -- enough significant bits for bf16 (and,
        # from dim 128 on, fp16) to ROUND, ties included (tests/_dlrm_reference.py _dot_case)
        table[:8] = (torch.randint(3, 5, (8, dim), generator=g).float() * 0.25).to(dtype)
        idx[:4, :8] = torch.arange(8)[None, :] - off[None, :8]           # joint rows 0..7 (negative ids: offsets bring them back)
    rows = idx + off[None, :tables]
    x64 = torch.cat([mlp[:, None, :], table[rows]], 1).to(D.F64)
    y, mag = D.dot_interact_fwd(x64)
    D.check_grid_sums([x64], [mag], B_MFMA)
    want = D.round_once(y, dtype)
    got = _fused_checked(table.to(cuda), idx.to(cuda), off[:tables].to(cuda), None, mlp.to(cuda), "exact %dx%d" % shape).cpu()
    assert_same(bits(got), bits(want), "gather_interact vs float64 %dx%d %s" % (tables, dim, D.name(dtype)))
    ntril = (tables + 1) * tables // 2
    assert torch.equal(bits(got[:, :dim]), bits(mlp)), "the first dim columns are mlp_out unchanged"
    assert int((bits(got[:, dim + ntril:]) != 0).sum()) == 0, "pad columns are exactly zero"


# ------------------------------------------------------------------------------------------------ 3. 64-bit addressing
def test_fused_addresses_past_2_31_elements(cuda):
    dim, tables, batch = 128, 26, 8
    n_rows = 2 ** 24 + 8
    table = torch.empty((n_rows, dim), dtype=F16, device=cuda)
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, n_rows, (batch, tables), generator=g)
    rows[:, ::2] = torch.randint(2 ** 24, n_rows, (batch, (tables + 1) // 2), generator=g)    # element offset >= 2^31
    rows[0, 0], rows[0, -1] = 0, n_rows - 1
    assert int(rows.max()) * dim >= 2 ** 31
    uniq = torch.unique(rows)
    table[uniq.to(cuda)] = torch.randn((uniq.numel(), dim), generator=g).to(F16).to(cuda)
    mlp = torch.randn((batch, dim), generator=g).to(F16).to(cuda)
    rows = rows.to(cuda)
    got = _fused_checked(table, rows, None, None, mlp, "2^31")
    assert_same(bits(got), bits(_unfused(table, rows, mlp)), "gather_interact past 2^31 elements")


# ------------------------------------------------------------------------------------------------ 4. envelope
def _shifted(t):
    """the same values at an address 2 bytes further (a contiguous view of a longer buffer)"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


def test_envelope_declines_and_writes_nothing(cuda):
    F = _F()
    from deeplearningexamples_amd import _cabi as C

    def declined(table, ids, offsets, mlp, out=None, what=""):
        b, t, d = ids.shape[0], ids.shape[1], table.shape[1]
        if out is None:
            out = torch.empty((b, F.dot_interact_out_width(t + 1, d)), dtype=table.dtype, device=cuda)
        out.fill_(-7.0)
        rc = C.lib().dle_dlrm_gather_interact_try(C.ptr(table), C.ptr(ids), C.ptr(offsets), 0, C.ptr(mlp), C.ptr(out), b, t, d,
                                                  C.dt(table), C.stream())
        assert rc == 0, "%s: rc %d" % (what, rc)
        assert F.gather_interact(table, ids, offsets, None, mlp, out=out) is None, what
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), "%s: a declined call wrote to out" % what

    table, ids, offsets, _, mlp, _ = _case(32, 128, F16, 5, "offsets", cuda)
    declined(table, ids, offsets, mlp, what="33 rows")
    table, ids, offsets, _, mlp, _ = _case(3, 24, F16, 5, "offsets", cuda)
    declined(table, ids, offsets, mlp, what="dim 24")
    table, ids, offsets, _, mlp, _ = _case(26, 128, F16, 5, "offsets", cuda)
    declined(table.float(), ids, offsets, mlp.float(), what="fp32")
    declined(_shifted(table), ids, offsets, mlp, what="table16 + 2 bytes")
    declined(table, ids, offsets, _shifted(mlp), what="mlp_out + 2 bytes")
    ow = F.dot_interact_out_width(27, 128)
    declined(table, ids, offsets, mlp, out=_shifted(torch.empty((5, ow), dtype=F16, device=cuda)), what="out + 2 bytes")


def test_predictor_outside_the_envelope_gives_the_unfused_answer(cuda):
    """embedding_dim 24 (no multiple of 16): the fused launch declines, the predictor answers with the pair."""
    from deeplearningexamples_amd.dlrm.infer import DlrmPredictor
    cfg = dict(sizes=[11, 4, 968], dim=24, bottom=[64, 24], top=[64, 32, 1], num=13, seed=21)
    model = _model(cfg, cuda, F16)
    num, cat, _ = _batch(cfg, 37, cuda)
    want = model(num, cat).view(-1)
    for fused in (True, False):
        got = DlrmPredictor(model, fused=fused).predict(num, cat)
        assert_same(bits(got), bits(want), "predictor at dim 24, fused=%s" % fused)


# ------------------------------------------------------------------------------------------------ 5. predictor == model.forward
def _model(cfg, dev, dtype):
    from deeplearningexamples_amd.dlrm.model import DistributedDlrm
    model = DistributedDlrm(num_numerical_features=cfg["num"], categorical_feature_sizes=cfg["sizes"],
                            bottom_mlp_sizes=cfg["bottom"], top_mlp_sizes=cfg["top"], embedding_dim=cfg["dim"],
                            device=dev, compute_dtype=dtype)
    state = SO.seeded_dlrm_state(cfg["sizes"], cfg["dim"], cfg["bottom"], cfg["top"], cfg["num"], cfg["seed"])
    SO.load_into_hip_model(model, state)
    return model


def _batch(cfg, batch, dev, seed=1000):
    num, cat, click = SO.seeded_dlrm_batch(cfg["sizes"], cfg["num"], batch, cfg["seed"] + seed)
    return num.to(dev), cat.to(dev), click.to(dev)


def _cfg(name, cap=None):
    cfg = dict(SO.DLRM_STEP_CONFIGS[name])
    if cap:
        cfg["sizes"] = [min(s, cap) for s in cfg["sizes"]]
    return cfg


@pytest.mark.parametrize("dtype", [F16, BF16], ids=D.name)
@pytest.mark.parametrize("name", ["tiny", "criteo_shape"])
def test_predictor_equals_training_forward(cuda, name, dtype):
    from deeplearningexamples_amd.dlrm.infer import DlrmPredictor
    cfg = _cfg(name, cap=1000)
    model = _model(cfg, cuda, dtype)
    fused, unfused = DlrmPredictor(model, fused=True), DlrmPredictor(model, fused=False)
    graphed = DlrmPredictor(model, fused=True, graphs=True)
    wants = {}
    for batch in (1, 64, 256):
        for k, seed in enumerate((1000, 2000)):          # a first and a second batch of different contents
            num, cat, _ = _batch(cfg, batch, cuda, seed)
            want = wants[(batch, k)] = model(num, cat).view(-1).clone()
            what = "%s %s batch %d #%d" % (name, D.name(dtype), batch, k)
            assert_same(bits(fused.predict(num, cat)), bits(want), "fused predictor, " + what)
            assert_same(bits(unfused.predict(num, cat)), bits(want), "unfused predictor, " + what)
            assert_same(bits(graphed.predict(num, cat)), bits(want), "graphed predictor, " + what)
        for p in (fused, graphed):                       # a batch size already seen: no allocation survives the call
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            y = p.predict(num, cat)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == before and y.numel() == batch
    # the fp32 table storage released: both routes from the 16-bit copy alone
    for fz in (True, False):
        model = _model(cfg, cuda, dtype)
        p = DlrmPredictor(model, fused=fz, release_fp32=True)
        assert model.bottom_model.embeddings.weight.numel() == 0
        num, cat, _ = _batch(cfg, 64, cuda, 2000)
        assert_same(bits(p.predict(num, cat)), bits(wants[(64, 1)]), "release_fp32, fused=%s" % fz)


# ------------------------------------------------------------------------------------------------ 6. the reference fixture
STEP_LOSS_RTOL = 1e-3            # the tolerance tests/test_gpu_dlrm_step.py applies to these fixtures (BASELINE.json north_star)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=D.name)
@pytest.mark.parametrize("name", ["tiny", "criteo_shape"])
def test_predictor_loss_matches_reference_fixture(cuda, golden_dir, name, dtype):
    from deeplearningexamples_amd.dlrm.infer import DlrmPredictor
    cfg = _cfg(name)
    gold = np.load(os.path.join(golden_dir, "dlrm_step_%s.npz" % name))
    model = _model(cfg, cuda, dtype)
    num, cat, click = _batch(cfg, cfg["batch"], cuda)
    x = DlrmPredictor(model).predict(num, cat).double().cpu()
    y = click.double().cpu().view(-1)
    loss = float((x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean())
    ref = float(gold["losses"][0])
    rel = abs(loss - ref) / ref
    print(name, dtype, "loss", loss, "reference", ref, "rel / 1e-3", rel / 1e-3)
    assert rel <= STEP_LOSS_RTOL, (loss, ref)


# ------------------------------------------------------------------------------------------------ 7. command line
def _records(path):
    return [json.loads(line[5:]) for line in open(path) if line.startswith("DLLL ")]


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "cuda_graphs"])
def test_inference_benchmark_command_line(cuda, tmp_path, graphs, capsys):
    from deeplearningexamples_amd.dlrm import main as dl
    log = str(tmp_path / "infer.json")
    argv = ["--mode", "inference_benchmark", "--dataset_type", "synthetic_gpu", "--synthetic_dataset_table_sizes",
            "1000,1000,30,1000,7,1000", "--inference_benchmark_batch_sizes", "1,64", "--inference_benchmark_steps", "14", "--amp",
            "--embedding_dim", "32", "--bottom_mlp_sizes", "64,32", "--top_mlp_sizes", "64,32,1", "--log_path", log]
    dl.main(argv + (["--cuda_graphs"] if graphs else []))
    data = [r["data"] for r in _records(log) if r.get("type") == "LOG" and r.get("step") == []][-1]
    for bs in (1, 64):
        lat, thr = data["mean_inference_latency_batch_%d" % bs], data["mean_inference_throughput_batch_%d" % bs]
        assert np.isfinite(lat) and lat > 0 and np.isfinite(thr) and thr > 0
        assert abs(thr - bs / lat) <= 1e-9 * thr
    assert len([k for k in data if k.startswith("mean_inference_")]) == 4
    assert capsys.readouterr().out.count("auc: ") == 2


def test_inference_benchmark_is_single_gpu(cuda, tmp_path, monkeypatch):
    from deeplearningexamples_amd.dlrm import main as dl
    monkeypatch.setattr(dl, "init_from_env", lambda: (0, 2, 0))
    with pytest.raises(ValueError, match="Inference benchmark only supports singleGPU mode."):
        dl.main(["--mode", "inference_benchmark", "--dataset_type", "synthetic_gpu", "--amp", "--log_path", str(tmp_path / "l.json")])
