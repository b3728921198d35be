"""DLRM with Adam: the duplicate-free sparse Adam kernel (csrc/emb_adam.hip), FusedAdam with the 16-bit copy refresh
(dle_mt_adam_copy) and the train step with --Adam_embedding_optimizer / --Adam_MLP_optimizer.  GPU only.

Kernel tolerance (test_sparse_adam_matches_float64).  The gradients are multiples of 1/16 in [-8, 8]: exact in fp16, bf16 and
fp32, and every sum of up to 2^20 of them is exact in fp32 in any order, so the kernel's row sums equal the float64 coalesce
bit for bit and the comparison sees the Adam epilogue alone.  Per element and step that is g = s * grad_mul (1 rounding),
m and v (2 roundings each, on top of the previous step's), sqrt, +eps, one division, one product with the step size and the add
into w: <= ~12 fp32 roundings, i.e. a relative error of the update <= 12 * 2^-24 ~ 7e-7 per step, compounding over 3 steps
through m and v to < 3e-6 of the update.  The update is at most lr * (1 - b1) / sqrt(1 - b2) ~ 3.2 lr per step (t = 1, the
largest ratio), so |w - w64| <= 3 steps * 3e-6 * 3.2 lr + one ulp of w per step ~ 3e-5 lr + 3 ulp.  The bar used: 1e-4 * lr +
4 ulp(|w|) (3x margin); m and v: 4e-6 relative + 1e-6 of the largest |m| / |v| (a moment that nearly cancels, 0.9 m + 0.1 g ~ 0,
keeps the absolute error of its terms).  A kernel with the other eps placement (Adam's sqrt(v / bc2) + eps) is off by up to ~1 % of the update
at eps = 1e-2, t = 1..3, far outside; a lost or doubled duplicate changes g by a whole gradient.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dlrm_step_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1, B2 = 0.9, 0.999
SIZES = [1, 4, 11, 97, 128, 129, 200, 300, 4096, 4097, 5000, 20000]


def _np_sparse_adam(w, m, v, rows, g, t, lr, eps, gmul):
    """float64 restatement of torch.optim._functional.sparse_adam: coalesce (duplicates summed), then the touched rows only."""
    uniq, inv = np.unique(rows, return_inverse=True)
    s = np.zeros((uniq.size, w.shape[1]))
    np.add.at(s, inv, g)
    s *= gmul
    mo, vo = m[uniq], v[uniq]
    mn = mo + (s - mo) * (1 - B1)
    vn = vo + (s * s - vo) * (1 - B2)
    step = lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    m[uniq], v[uniq] = mn, vn
    w[uniq] = w[uniq] - step * mn / (np.sqrt(vn) + eps)
    return uniq


def _batch(sizes, batch, seed):
    rng = np.random.default_rng(seed)
    # heavily skewed ids: many duplicates on the first rows of every table
    cat = np.stack([np.minimum((s * rng.random(batch) ** 3).astype(np.int64), s - 1) for s in sizes], axis=1)
    return cat


@pytest.mark.parametrize("eps", [1e-8, 1e-2])
@pytest.mark.parametrize("gdt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dim", [128, 64, 256])
def test_sparse_adam_matches_float64(cuda, dim, gdt, eps):
    from deeplearningexamples_amd import functional as F
    T, batch, lr, inv_scale = len(SIZES), 4096, 1e-2, 0.375
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    rng = np.random.default_rng(dim + 7 * int(eps > 1e-4))
    w64 = rng.uniform(-0.05, 0.05, (int(off[-1]), dim))
    m64, v64 = np.zeros_like(w64), np.zeros_like(w64)
    w = torch.tensor(w64, dtype=torch.float32, device=cuda)
    w64 = w.double().cpu().numpy()
    m = torch.zeros_like(w)
    v = torch.zeros_like(w)
    ws = F.EmbUpdateWorkspace(off, dim, cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    gmul = torch.tensor([inv_scale], dtype=torch.float32, device=cuda)
    w_sp = torch.nn.Parameter(torch.tensor(w64))                         # torch's own SparseAdam, float64, on the CPU
    opt = torch.optim.SparseAdam([w_sp], lr=lr, betas=(B1, B2), eps=eps)
    for t in (1, 2, 3):
        cat = _batch(SIZES, batch, 100 * t + dim)
        rows_np = cat + off[:-1]
        gq = rng.integers(-128, 129, (batch, T, dim)) / 16.0
        # two lookups of one row carry +g and -g (from step 2; +g twice at step 1): the row's sum is exactly 0 and it must still
        # be updated (its m decays).  One such row in table 7 (200 rows: LDS / mid / large path by dim) and one in table 4 (128
        # rows: the one-hot tiny path at dim 128 with 16-bit gradients, the LDS path at 64, the lists at 256)
        zrows = []
        for tz, r0 in ((7, 5), (4, 120)):
            zr = int(off[tz]) + r0
            rows_np[0, tz] = rows_np[1, tz] = zr
            rows_np[:, tz][2:][rows_np[2:, tz] == zr] = zr + 1
            gq[1, tz] = gq[0, tz] if t == 1 else -gq[0, tz]
            zrows.append(zr)
        full = torch.zeros((batch, T + 1, dim), dtype=gdt)                # a strided view: slot 0 stands for the bottom MLP
        full[:, 1:, :] = torch.tensor(gq, dtype=gdt)
        full = full.to(cuda)
        rows = torch.from_numpy(rows_np).to(cuda)
        step.fill_(t)
        prev = [x.clone() for x in (w, m, v)]
        F.emb_adam_dedup_(w, m, v, rows, full[:, 1:, :], ws, lr, step, grad_mul=gmul, eps=eps, grad_batch_stride=(T + 1) * dim)
        touched = _np_sparse_adam(w64, m64, v64, rows_np.reshape(-1), gq.reshape(-1, dim), t, lr, eps, inv_scale)
        ri = torch.from_numpy(rows_np.reshape(-1))
        opt.zero_grad()
        w_sp.grad = torch.sparse_coo_tensor(ri.unsqueeze(0), torch.tensor(gq.reshape(-1, dim) * inv_scale), w_sp.shape)
        opt.step()
        np.testing.assert_allclose(w_sp.detach().numpy(), w64, rtol=0, atol=1e-12)
        wg, mg, vg = (x.double().cpu().numpy() for x in (w, m, v))
        ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(wg - w64) <= 1e-4 * lr + 4 * ulp), (t, np.abs(wg - w64).max())
        np.testing.assert_allclose(mg, m64, rtol=4e-6, atol=1e-6 * np.abs(m64).max())
        np.testing.assert_allclose(vg, v64, rtol=4e-6, atol=1e-6 * np.abs(v64).max())
        # rows this call did not look up: w, m, v bit-identical to before the call
        untouched = np.ones(w64.shape[0], bool)
        untouched[touched] = False
        assert untouched.sum() > 0
        ut = torch.from_numpy(untouched).to(cuda)
        for a, b in zip((w, m, v), prev):
            assert torch.equal(a[ut], b[ut])
        if t > 1:
            for zr in zrows:
                assert prev[1][zr].abs().sum().item() > 0
                assert not torch.equal(m[zr], prev[1][zr]), "a looked-up row with a zero sum was not updated"
        assert int((ws.head != -1).sum().item()) == 0


def test_sparse_adam_skip_flag_writes_nothing(cuda):
    from deeplearningexamples_amd import functional as F
    dim, batch = 128, 2048
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    w = torch.randn(int(off[-1]), dim, device=cuda)
    m, v = torch.rand_like(w), torch.rand_like(w)
    ws = F.EmbUpdateWorkspace(off, dim, cuda)
    rows = torch.from_numpy(_batch(SIZES, batch, 3) + off[:-1]).to(cuda)
    g = torch.randn(batch, len(SIZES), dim, device=cuda).half()
    before = [x.clone() for x in (w, m, v)]
    step = torch.ones(1, dtype=torch.int32, device=cuda)
    F.emb_adam_dedup_(w, m, v, rows, g, ws, 1e-2, step, skip_flag=torch.ones(1, device=cuda))
    for a, b in zip((w, m, v), before):
        assert torch.equal(a, b)
    assert int((ws.head != -1).sum().item()) == 0
    F.emb_adam_dedup_(w, m, v, rows, g, ws, 1e-2, step, skip_flag=torch.zeros(1, device=cuda))
    assert not torch.equal(w, before[0])


# ------------------------------------------------------------------------------------------------ FusedAdam with copies
@pytest.mark.parametrize("eps", [1e-8, 1e-2])
@pytest.mark.parametrize("cdt", [torch.float16, torch.bfloat16])
def test_mt_adam_copy_matches_torch_adam(cuda, eps, cdt):
    """Against torch.optim.Adam in float64 (apex FusedAdam at weight_decay 0): 3 steps; the copy equals the cast of the master;
    the per-tensor multiplier scales one tensor's gradient; the skip flag leaves every list bit-identical."""
    from deeplearningexamples_amd import multi_tensor as mt
    torch.manual_seed(0)
    shapes = [(256, 96), (256,), (33, 7), (5,), (1000, 3)]
    ps = [torch.randn(s, device=cuda) * 0.1 for s in shapes]
    gs = [torch.zeros_like(p) for p in ps]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    cs = [p.to(cdt) if p.dim() == 2 else None for p in ps]
    table = mt.TensorTable([gs, ps, ms, vs, cs], mt.streaming_chunk([gs]))
    mul = torch.tensor([1.0, 1.0, 0.5, 0.5, 0.25], device=cuda)
    inv = torch.tensor([1.0 / 1024], device=cuda)
    p64 = [torch.nn.Parameter(p.double().cpu()) for p in ps]
    opt = torch.optim.Adam(p64, lr=1e-3, betas=(B1, B2), eps=eps)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    lr = torch.tensor([1e-3], device=cuda)
    for t in range(3):
        for g in gs:
            g.copy_(torch.randn_like(g) * 1024 * (10.0 ** -t))
        step += 1
        mt.adam_copy(table, lr, step, eps=eps, inv_scale=inv, tensor_mul=mul)
        for q, g, f in zip(p64, gs, mul.tolist()):
            q.grad = g.double().cpu() / 1024 * f
        opt.step()
        for q, p, c in zip(p64, ps, cs):
            ref = q.detach()
            # one fp32 rounding of p per step plus ~1e-6 of the <= lr update
            assert (p.double().cpu() - ref).abs().max() <= (t + 1) * (2 * np.spacing(np.float32(ref.abs().max())) + 1e-9)
            if c is not None:
                assert torch.equal(c, p.to(cdt))
    before = [x.clone() for x in ps + ms + vs + [c for c in cs if c is not None]]
    step += 1
    mt.adam_copy(table, lr, step, eps=eps, inv_scale=inv, tensor_mul=mul, skip_flag=torch.ones(1, device=cuda))
    for a, b in zip(ps + ms + vs + [c for c in cs if c is not None], before):
        assert torch.equal(a, b)


def test_mt_adam_copy_eps_placement(cuda):
    """FusedAdam's eps sits outside sqrt(v / bc2); the sparse form's inside the bias correction: at eps = 1e-2 and t = 1 the two
    differ by ~3 % -- this kernel follows torch.optim.Adam."""
    from deeplearningexamples_amd import multi_tensor as mt
    p = torch.zeros(64, device=cuda)
    g = torch.full_like(p, 1e-2)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    table = mt.TensorTable([[g], [p], [m], [v]])
    mt.adam_copy(table, 1.0, torch.ones(1, dtype=torch.int32, device=cuda), eps=1e-2, model_copy=False)
    adam = -1.0 * 1e-3 / (np.sqrt(1e-7 / 1e-3) + 1e-2) / 0.1        # -lr * m/bc1 / (sqrt(v/bc2) + eps)
    sparse = -1.0 * np.sqrt(1e-3) / 0.1 * 1e-3 / (np.sqrt(1e-7) + 1e-2)
    assert abs(adam - sparse) > 0.02 * abs(adam)
    np.testing.assert_allclose(p.cpu().numpy(), adam, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ the train step
class AdamOracle(SO.DlrmOracle):
    """The reference's step with Adam: the embedding gradient as the sparse COO tensor its embedding backward produces (one entry
    per lookup) into torch.optim.SparseAdam, the MLPs into torch.optim.Adam (apex FusedAdam at weight_decay 0, CPU-less)."""

    def __init__(self, state, sizes, lr, adam_emb, adam_mlp, sgd_lr=1.0, storage_dtype=None):
        super().__init__(state, sizes, lr, storage_dtype)
        self.adam_emb, self.adam_mlp, self.sgd_lr = adam_emb, adam_mlp, sgd_lr
        self.emb = self.p.pop("embedding").detach().requires_grad_(False)
        self.emb_param = torch.nn.Parameter(self.emb)
        mlp = list(self.p.values())
        self.mlp_opt = torch.optim.Adam(mlp, lr=lr, betas=(B1, B2), eps=1e-8) if adam_mlp else None
        self.emb_opt = torch.optim.SparseAdam([self.emb_param], lr=lr, betas=(B1, B2), eps=1e-8) if adam_emb else None

    def forward(self, num, cat):
        rows = cat + self.offsets[:-1]
        self._rows = rows
        self._leaf = self.emb_param.detach()[rows].requires_grad_(True)
        self.p["embedding"] = _Gathered(self._leaf, rows)
        try:
            return super().forward(num, cat)
        finally:
            del self.p["embedding"]

    def step(self, num, cat, click, lr=None):
        for v in self.p.values():
            v.grad = None
        loss = torch.nn.functional.binary_cross_entropy_with_logits(self.forward(num, cat), click, reduction="mean")
        loss.backward()
        with torch.no_grad():
            if self.adam_mlp:
                self.mlp_opt.step()
            else:
                for v in self.p.values():
                    v -= self.sgd_lr * v.grad
            d = self.emb.shape[1]
            idx = self._rows.reshape(1, -1)
            vals = self._leaf.grad.reshape(-1, d)
            if self.adam_emb:
                self.emb_param.grad = torch.sparse_coo_tensor(idx, vals, self.emb.shape)
                self.emb_opt.step()
            else:
                self.emb_param.index_add_(0, idx[0], vals, alpha=-self.sgd_lr)
        return float(loss.detach())


class _Gathered:
    """p["embedding"][rows] inside DlrmOracle.forward returns the leaf gathered beforehand."""

    def __init__(self, leaf, rows):
        self.leaf, self.rows = leaf, rows

    def __getitem__(self, rows):
        assert rows is self.rows or torch.equal(rows, self.rows)
        return self.leaf


def _build(cfg, device, dtype, adam_emb, adam_mlp, lr):
    from deeplearningexamples_amd.dlrm.model import DistributedDlrm
    from deeplearningexamples_amd.dlrm.engine import DlrmTrainer
    model = DistributedDlrm(num_numerical_features=cfg["num"], categorical_feature_sizes=cfg["sizes"],
                            bottom_mlp_sizes=cfg["bottom"], top_mlp_sizes=cfg["top"], embedding_dim=cfg["dim"],
                            device=device, compute_dtype=dtype)
    state = SO.seeded_dlrm_state(cfg["sizes"], cfg["dim"], cfg["bottom"], cfg["top"], cfg["num"], cfg["seed"])
    SO.load_into_hip_model(model, state)
    trainer = DlrmTrainer(model, lr=lr, batch_sizes_per_gpu=[cfg["batch"]], amp=True, adam_embeddings=adam_emb,
                          adam_mlps=adam_mlp)
    return model, trainer, state


CASES = {"emb": (True, False), "mlp": (False, True), "both": (True, True)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["tiny", "mixed_paths", "criteo_shape"])
def test_adam_step_matches_live_reference(cuda, name, dtype, case):
    """Per-step loss within the bare 1e-3 relative of the north star, 4 steps, against the CPU reference with SparseAdam / Adam
    (one --lr for both optimizers, as in the reference: the SGD part of a mixed case steps with it too).  On mixed_paths the embedding updates of
    every probed table (one-hot, eight-list and one-list paths) are compared as final - initial: Adam's first steps are
    sign-like (|update| ~ lr per element whatever |g|), so an element whose 16-bit gradient sum is near 0 may move the other
    way; the bar is the WaveGlow / Tacotron2 Adam tests' ||hip - ref|| <= 0.15 ||ref|| per table, while a lost or doubled
    duplicate or an unupdated zero-sum row moves whole rows by ~lr."""
    adam_emb, adam_mlp = CASES[case]
    cfg = SO.DLRM_STEP_CONFIGS[name]
    lr = 1e-3
    steps = 4
    model, trainer, state = _build(cfg, cuda, dtype, adam_emb, adam_mlp, lr)
    orc = AdamOracle(state, cfg["sizes"], lr, adam_emb, adam_mlp, sgd_lr=lr)
    num, cat, click = SO.seeded_dlrm_batch(cfg["sizes"], cfg["num"], cfg["batch"], cfg["seed"] + 2000)
    dn, dc, dk = num.to(cuda), cat.to(cuda), click.to(cuda)
    for i in range(steps):
        lo = orc.step(num, cat, click)
        lh = float(trainer.train_step(dn, dc, dk).item())
        assert abs(lh - lo) <= 1e-3 * abs(lo), (i, lh, lo)
    assert trainer.scaler.found_inf.item() == 0 or dtype == torch.bfloat16
    if adam_emb:
        assert int(trainer.emb_step.item()) == steps
    if adam_mlp:
        assert int(trainer.mlp_step.item()) == steps
    emb = model.bottom_model.embeddings
    assert int((emb.workspace().head != -1).sum().item()) == 0
    if name == "mixed_paths" and adam_emb:
        rows = SO.probe_rows(cfg, cat)
        init = state["embedding"].numpy()[rows]
        d_ref = orc.emb.numpy()[rows] - init
        d_hip = emb.weight.detach()[torch.from_numpy(rows).to(cuda)].cpu().numpy() - init
        off = np.concatenate([[0], np.cumsum(cfg["sizes"])])
        for t in SO.MIXED_PATHS_PROBE_TABLES:
            msk = (rows >= off[t]) & (rows < off[t + 1])
            moved = np.linalg.norm(d_ref[msk])
            dist = np.linalg.norm(d_hip[msk] - d_ref[msk])
            print("table", t, "rows", cfg["sizes"][t], "moved", moved, "dist", dist)
            assert moved > 0 and dist <= 0.15 * moved, (t, dist, moved)


def test_adam_overflow_step_changes_nothing(cuda):
    """A forced absurd loss scale: w, m, v, both step counters and all MLP state stay bit-identical and the scale halves; the next
    normal step then runs with t = 1 and matches the reference's first step."""
    cfg = SO.DLRM_STEP_CONFIGS["tiny"]
    model, trainer, state = _build(cfg, cuda, torch.float16, True, True, 1e-3)
    num, cat, click = SO.seeded_dlrm_batch(cfg["sizes"], cfg["num"], cfg["batch"], 77)
    dn, dc, dk = num.to(cuda), cat.to(cuda), click.to(cuda)
    sc = trainer.scaler
    sc.scale.fill_(3e38)
    sc.inv_scale.fill_(1.0 / 3e38)
    emb = model.bottom_model.embeddings
    snap = lambda: [x.clone() for x in [emb.weight.data, *emb.adam_state(), trainer.emb_step, trainer.mlp_step]
                    + list(model.parameters()) + trainer.mlp_adam_state[0] + trainer.mlp_adam_state[1]]
    before = snap()
    trainer.train_step(dn, dc, dk)
    for a, b in zip(snap(), before):
        assert torch.equal(a, b)
    assert sc.scale.item() == pytest.approx(1.5e38)
    sc.scale.fill_(1024.0)
    sc.inv_scale.fill_(1.0 / 1024)
    orc = AdamOracle(state, cfg["sizes"], 1e-3, True, True)
    lo = orc.step(num, cat, click)
    lh = float(trainer.train_step(dn, dc, dk).item())
    assert int(trainer.emb_step.item()) == 1 and int(trainer.mlp_step.item()) == 1
    assert abs(lh - lo) <= 1e-3 * abs(lo)
    lo = orc.step(num, cat, click)
    lh = float(trainer.train_step(dn, dc, dk).item())
    assert abs(lh - lo) <= 1e-3 * abs(lo)


def test_adam_step_under_graph_capture(cuda):
    """GraphedStep around an Adam train_step (its warm-up steps run eagerly, then capture + replays) vs N eager steps."""
    from deeplearningexamples_amd.utils.graph import GraphedStep
    cfg = SO.DLRM_STEP_CONFIGS["tiny"]
    num, cat, click = SO.seeded_dlrm_batch(cfg["sizes"], cfg["num"], cfg["batch"], 5)
    dn, dc, dk = num.to(cuda), cat.to(cuda), click.to(cuda)
    n = 7
    out = []
    for graphed in (False, True):
        model, trainer, _ = _build(cfg, cuda, torch.float16, True, True, 1e-3)
        fn = GraphedStep(trainer.train_step, enabled=graphed, warmup_steps=3)
        losses = [float(fn(dn, dc, dk).item()) for _ in range(n)]
        torch.cuda.synchronize()
        assert int(trainer.emb_step.item()) == n and int(trainer.mlp_step.item()) == n
        out.append((losses, model.bottom_model.embeddings.weight.detach().clone(),
                    model.top_model.out.weight.detach().clone()))
    (l0, e0, o0), (l1, e1, o1) = out
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    assert (e1 - e0).abs().max().item() <= 1e-5
    assert (o1 - o0).abs().max().item() <= 1e-5


@pytest.mark.parametrize("graphs", [False, True])
def test_entry_point_trains_with_adam(cuda, graphs, tmp_path):
    import json
    log = str(tmp_path / "log.json")
    cmd = [sys.executable, "-m", "deeplearningexamples_amd.dlrm.main", "--mode", "train", "--dataset_type", "synthetic_gpu",
           "--Adam_embedding_optimizer", "--Adam_MLP_optimizer", "--lr", "0.001", "--amp",
           "--synthetic_dataset_table_sizes", "100,3000,50000,7", "--synthetic_dataset_num_entries", "65536",
           "--batch_size", "8192", "--epochs", "1", "--max_steps", "6", "--test_freq", "100000", "--print_freq", "1",
           "--embedding_dim", "128", "--bottom_mlp_sizes", "256,128", "--top_mlp_sizes", "256,128,1",
           "--log_path", log, "--cuda_graphs=%s" % graphs]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = []
    for line in open(log):
        rec = json.loads(line[line.index("{"):]) if "{" in line else {}
        if "loss" in rec.get("data", {}):
            losses.append(rec["data"]["loss"])
    assert len(losses) >= 5 and np.all(np.isfinite(losses)), losses


@pytest.mark.parametrize("adam_emb,adam_mlp", [(False, False), (True, False), (False, True), (True, True)])
def test_trainer_rates_follow_the_plan(cuda, adam_emb, adam_mlp):
    """The device learning rates the trainer steps with are optimizer_plan's (the reference's rules), and they follow
    set_lr_factor.  (World 2 is checked by the two-rank test.)"""
    from deeplearningexamples_amd.dlrm.engine import optimizer_plan
    cfg = SO.DLRM_STEP_CONFIGS["tiny"]
    model, trainer, _ = _build(cfg, cuda, torch.float16, adam_emb, adam_mlp, 0.5)
    plan = optimizer_plan(0.5, 1, adam_emb, adam_mlp)
    assert trainer.lr_emb.item() == plan["embeddings"][0]
    if adam_emb:
        assert trainer.emb_div == plan["embeddings"][1]
    if adam_mlp:
        assert trainer.lr_mlp.item() == plan["top_mlp"][0] == plan["bottom_mlp"][0]
    trainer.set_lr_factor(0.25)
    assert trainer.lr_emb.item() == plan["embeddings"][0] * 0.25
    if adam_mlp:
        assert trainer.lr_mlp.item() == plan["top_mlp"][0] * 0.25


def test_frozen_parts_allocate_no_adam_state(cuda):
    cfg = SO.DLRM_STEP_CONFIGS["tiny"]
    from deeplearningexamples_amd.dlrm.model import DistributedDlrm
    from deeplearningexamples_amd.dlrm.engine import DlrmTrainer
    model = DistributedDlrm(num_numerical_features=cfg["num"], categorical_feature_sizes=cfg["sizes"],
                            bottom_mlp_sizes=cfg["bottom"], top_mlp_sizes=cfg["top"], embedding_dim=cfg["dim"], device=cuda)
    tr = DlrmTrainer(model, lr=1e-3, batch_sizes_per_gpu=[cfg["batch"]], adam_embeddings=True, adam_mlps=True,
                     freeze_embeddings=True, freeze_mlps=True)
    assert getattr(model.bottom_model.embeddings, "_adam_m", None) is None
    assert not hasattr(tr, "mlp_adam_state")
    num, cat, click = SO.seeded_dlrm_batch(cfg["sizes"], cfg["num"], cfg["batch"], 1)
    tr.train_step(num.to(cuda), cat.to(cuda), click.to(cuda))
    assert int(tr.emb_step.item()) == 0 and int(tr.mlp_step.item()) == 0


def test_two_ranks_adam_match_one_rank(cuda, tmp_path):
    """Table-wise placement at world 2 with both optimizers Adam (tests/_dlrm_adam_worker.py, the launcher of
    tests/test_gpu_multirank.py: gloo staged on one GPU, 2 ranks) against ONE rank holding every table, same weights and batch.
    What differs at world 2 is what is checked: the embeddings and the bottom MLP keep the full rate and divide their gradients
    by 2 (the top MLP's all-reduce mean is not divided again).  eps is set near the gradients' size, so Adam is not blind to a
    wrong divisor.  Bars: the losses at 3e-4 and the data-parallel weights as in the SGD two-rank test; the movement (final -
    initial) of looked-up embedding rows of every table within 5 % of the table's largest movement (the 16-bit gradients of
    the two runs are summed in different orders; a halved rate or a doubled gradient moves them by tens of percent)."""
    import json
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    out = str(tmp_path / "dlrm_adam.json")
    port = 29900 + os.getpid() % 90
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(here, "_dlrm_adam_worker.py"), "dlrm_adam", backend, out]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "2-rank run failed (%s):\n%s\n%s" % (backend, r.stdout[-3000:], r.stderr[-6000:])
    two = json.load(open(out))
    sys.path.insert(0, here)
    import _dlrm_adam_worker as AW
    one = AW.run_dlrm_adam(0, 1, cuda, 3)
    print("2-rank", two[0]["losses"], "1-rank", one["losses"])
    # the rules in force on each rank
    for rk in two:
        rt = rk["rates"]
        assert rt["lr_mlp"] == pytest.approx(AW.ADAM_LR, rel=1e-7)
        if rt["lr_emb"] is not None:
            assert rt["lr_emb"] == pytest.approx(AW.ADAM_LR, rel=1e-7) and rt["emb_div"] == 2
        n_top = rt["n_top_tensors"]
        assert rt["mlp_gmul"][:n_top] == [1.0] * n_top
        assert rt["mlp_gmul"][n_top:] == ([0.5] * (len(rt["mlp_gmul"]) - n_top) if rt["has_bottom"] else [])
        assert rk["steps"] == [3, 3]
    assert any(rk["rates"]["has_bottom"] for rk in two)
    np.testing.assert_allclose(two[0]["losses"], one["losses"], rtol=3e-4)
    assert two[0]["probe"] == two[1]["probe"], "data-parallel replicas diverged"
    ref = np.asarray(one["probe"])
    np.testing.assert_allclose(np.asarray(two[0]["probe"]), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).max())
    got = {}
    for rk in two:
        got.update(rk["emb_rows"])
    assert sorted(got) == sorted(one["emb_rows"])
    for t, want in one["emb_rows"].items():
        want, have = np.asarray(want), np.asarray(got[t])
        assert np.abs(want).max() > 0
        assert np.abs(have - want).max() <= 5e-2 * np.abs(want).max(), (t, np.abs(have - want).max(), np.abs(want).max())
