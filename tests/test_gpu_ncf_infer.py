"""NeuMFScorer and ncf.evaluate against the reference's recorded float64 results (tests/golden/ncf_eval.npz), both routes, graph
replay, the launch list of an evaluation, and the two command lines.

Yardstick of the scorer, as for the other front ends: E_new <= 1.5 E_emulated, E the largest absolute logit error against the
reference's float64 forward, E_emulated that of the reference's own model.half() arithmetic emulated in float64
(tests/_ncf_ref.half_forward); the test computes both.  End to end, a series is boundary-clear when its positive's float64 logit is
further than 8 E_emulated from the k-th best other logit: there the hit decision must be the float64 one; at most 10 % of the
series may be unclear."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.ncf import data as D
from deeplearningexamples_amd.ncf import model as NM
from deeplearningexamples_amd.ncf.evaluate import evaluate
from deeplearningexamples_amd.ncf.infer import NeuMFScorer
from tests import _exact_grid as G
from tests import _ncf_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
ROUTES = [pytest.param(True, id="fused"), pytest.param(False, id="unfused")]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "ncf_eval.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


@functools.lru_cache(maxsize=None)
def state():
    fx = fixture()
    return R.seeded_state(fx["n_users"], fx["n_items"], fx["seed"])


@functools.lru_cache(maxsize=None)
def e_emulated(dtype):
    fx = fixture()
    return float((R.half_forward(state(), fx["sorted_users"], fx["sorted_items"], dtype) - fx["sorted_logit64"]).abs().max())


@functools.lru_cache(maxsize=None)
def scorer(dtype, fused=True, graphs=False):
    return NeuMFScorer(NM.model_from_state(state()), dtype=dtype, fused=fused, graphs=graphs)


def loader():
    fx = fixture()
    spec = D.FeatureSpec({"user": {"cardinality": fx["n_users"]}, "item": {"cardinality": fx["n_items"]}, "label": {}}, {"test": []},
                         {D.USER_CHANNEL: ["user"], D.ITEM_CHANNEL: ["item"], D.LABEL_CHANNEL: ["label"]},
                         {D.TEST_SAMPLES_PER_SERIES: fx["samples_in_series"]}, "")
    feats = {"user": fx["users"].view(-1, 1), "item": fx["items"].view(-1, 1), "label": fx["labels"].view(-1, 1)}
    return D.TestLoader(spec, feats, fx["valid_batch_size"]).to(DEV)


@pytest.mark.parametrize("fused", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scorer_against_float64(dtype, fused):
    fx = fixture()
    sc = scorer(dtype, fused)
    assert sc.fused == fused and sc.in_envelope
    u, i = fx["sorted_users"].to(DEV), fx["sorted_items"].to(DEV)
    logit = sc.logits(u, i)
    assert logit.dtype == torch.float32 and logit.is_cuda
    e_new, e_emu = float((logit.double().cpu() - fx["sorted_logit64"]).abs().max()), e_emulated(dtype)
    print("%s %s: E_new %.4e  E_emulated %.4e  ratio %.3f" % (dtype, "fused" if fused else "unfused", e_new, e_emu, e_new / e_emu))
    assert e_new <= 1.5 * e_emu
    prob = sc.predict(u.int(), i.int())
    assert bool(((prob.double().cpu() - R.sigmoid64(logit.cpu())).abs() <= 4 * R.prob_bar(logit.cpu())).all())
    # an index outside its table: NaN on both routes, the rest untouched
    ub = u[:200].clone()
    ub[77] = fx["n_users"]
    lb = sc.logits(ub, i[:200]).cpu()
    assert bool(torch.isnan(lb[77])) and torch.equal(lb[:77], logit[:77].cpu()) and torch.equal(lb[78:], logit[78:200].cpu())


@pytest.mark.parametrize("fused", ROUTES)
def test_graph_replay_equals_eager(fused):
    fx = fixture()
    eager, graphed = scorer(HF, fused), scorer(HF, fused, True)
    y = fx["sorted_labels"].to(DEV)
    for n, seed in ((300, 0), (64, 1), (300, 2), (300, 3), (300, 4)):         # warm-up calls, the capture, replays with new inputs
        g = torch.Generator().manual_seed(seed)
        sel = torch.randperm(fx["sorted_users"].numel(), generator=g)[:n]
        u, i, lab = fx["sorted_users"][sel].to(DEV), fx["sorted_items"][sel].to(DEV), y[sel.to(DEV)]
        assert torch.equal(G.bits(graphed.logits(u, i)), G.bits(eager.logits(u, i))), (n, seed)
        assert torch.equal(G.bits(graphed.predict(u, i)), G.bits(eager.predict(u, i))), (n, seed)
        pg, lg = graphed.score_with_loss(u, i, lab)
        pe, le = eager.score_with_loss(u, i, lab)
        assert torch.equal(G.bits(pg), G.bits(pe)) and torch.equal(lg, le), (n, seed)
    assert graphed._graphs[("logits", 300, torch.int64)].graph is not None


def test_launch_list_and_one_host_read(monkeypatch):
    fx = fixture()
    sc, ld = scorer(BF), loader()
    evaluate(sc, ld, fx["k"])                                           # warm
    names, copies = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (copies.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: copies.append("synchronize"))
    evaluate(sc, ld, fx["k"])
    monkeypatch.undo()
    assert copies == ["cpu"], copies
    assert len(ld.batches) == fx["n_batches"] >= 4
    assert names == ["dle_ncf_score_fwd", "dle_ncf_rank_fwd"] * len(ld.batches), names


@pytest.mark.parametrize("fused", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluate_composition_and_end_to_end(dtype, fused):
    """evaluate's hr is the integer rank statement on the scorer's own read-back ratings, exactly; its ndcg is that statement's to
    the rank kernel's 1e-6 (the kernel's dcg is fp32); its loss is the float64 fold of those ratings to 1e-6.  Then, on the
    boundary-clear series, the hit decisions are the recorded float64 ones."""
    fx = fixture()
    S, k = fx["samples_in_series"], fx["k"]
    sc, ld = scorer(dtype, fused), loader()
    hr, ndcg, loss = evaluate(sc, ld, k)
    rating = torch.cat([sc.predict(u, i).clone() for u, i, _ in ld.batches]).cpu()
    hits, dcg = R.rank_rule(rating, fx["sorted_labels"], fx["mask"], S, k)
    n = rating.numel() // S
    assert hr == int(hits.sum()) / n
    assert abs(ndcg - float(dcg.sum()) / n) <= 1e-6 * float(dcg.sum()) / n
    p, y = rating.double(), fx["sorted_labels"].double()
    per = -(y * torch.log(p).clamp_min(-100) + (1 - y) * torch.log1p(-p).clamp_min(-100))
    want = float(torch.stack([c.mean() for c in per.split(fx["valid_batch_size"])]).mean())
    print("%s %s: hr %.6f (float64 %.6f)  ndcg %.6f (%.6f)  loss %.8f (fold %.8f, float64 %.8f)" %
          (dtype, fused, hr, fx["hr"], ndcg, fx["ndcg"], loss, want, fx["loss"]))
    assert abs(loss - want) <= 1e-6 * want
    # end to end
    clear = R.boundary_clear(fx["sorted_logit64"], fx["sorted_labels"], fx["mask"], S, k, 8 * e_emulated(dtype))
    skipped = 1.0 - float(clear.double().mean())
    assert skipped <= 0.10, "%.1f %% of the series are unclear" % (100 * skipped)
    hits64, _ = R.rank_rule(torch.sigmoid(fx["sorted_logit64"]), fx["sorted_labels"], fx["mask"], S, k)
    assert int(hits64.sum()) / n == fx["hr"]
    assert torch.equal(hits[clear], hits64[clear]), "hit decisions differ on boundary-clear series %s" % \
        torch.nonzero(clear & (hits != hits64)).flatten().tolist()


def _records(path):
    out = {}
    for line in open(path):
        rec = json.loads(line[len("DLLL "):])
        if rec["type"] == "LOG" and rec["step"] == []:
            out.update(rec["data"])
    return out


def test_command_line_inference(tmp_path):
    log = str(tmp_path / "log.json")
    argv = [sys.executable, "-m", "deeplearningexamples_amd.ncf.inference", "--fp16", "--n_users", "61", "--n_items", "211",
            "--load_checkpoint_path", os.path.join(GOLDEN, "ncf_checkpoint.pt"), "--batch_sizes", "1,100", "--num_batches", "14",
            "--log_path", log]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = _records(log)
    for b in (1, 100):
        for key in ("mean_throughput", "mean_latency", "p90_latency", "p95_latency", "p99_latency"):
            assert rec["batch_%d_%s" % (b, key)] > 0, (b, key)
        assert abs(rec["batch_%d_mean_throughput" % b] * rec["batch_%d_mean_latency" % b] - b) <= 1e-6 * b


def test_command_line_test_mode(tmp_path):
    fx = fixture()
    torch.save(torch.stack((fx["users"], fx["items"]), dim=1), str(tmp_path / "test_0.pt"))
    torch.save(fx["labels"].view(-1, 1), str(tmp_path / "test_1.pt"))
    with open(str(tmp_path / "feature_spec.yaml"), "w") as f:
        f.write("channel_spec:\n  item_ch: [item]\n  label_ch: [label]\n  user_ch: [user]\n"
                "feature_spec:\n  item: {cardinality: 211, dtype: torch.int64}\n  label: {dtype: torch.float32}\n"
                "  user: {cardinality: 61, dtype: torch.int64}\n"
                "metadata: {test_samples_per_series: 100}\n"
                "source_spec:\n  test:\n  - features: [user, item]\n    files: [test_0.pt]\n    type: torch_tensor\n"
                "  - features: [label]\n    files: [test_1.pt]\n    type: torch_tensor\n  train: []\n")
    log = str(tmp_path / "log.json")
    argv = [sys.executable, "-m", "deeplearningexamples_amd.ncf.test", "--data", str(tmp_path), "--mode", "test", "--amp", "--amp-dtype", "bf16",
            "--load_checkpoint_path", os.path.join(GOLDEN, "ncf_checkpoint.pt"), "--valid_batch_size", str(fx["valid_batch_size"]),
            "--log_path", log]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = _records(log)
    hr, ndcg, loss = evaluate(scorer(BF), loader(), fx["k"])          # the same evaluation in this process: the same bits
    assert rec["hr@10"] == hr and rec["validation_loss"] == loss and rec["best_eval_throughput"] > 0
