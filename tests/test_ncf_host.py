"""The host side of the NCF family against what tools/make_ncf_fixture.py recorded from the reference (tests/golden/ncf_*), and the
self-test of the error bars of tests/_ncf_ref.py.  No GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.ncf import data as D
from deeplearningexamples_amd.ncf import inference as INF
from deeplearningexamples_amd.ncf import model as NM
from deeplearningexamples_amd.ncf import test as TST
from deeplearningexamples_amd.ncf.evaluate import evaluate
from tests import _ncf_ref as R
from tests import _tft_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "ncf_eval.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


@functools.lru_cache(maxsize=None)
def state():
    fx = fixture()
    return R.seeded_state(fx["n_users"], fx["n_items"], fx["seed"])


def spec_of(fx):
    return D.FeatureSpec({"user": {"cardinality": fx["n_users"]}, "item": {"cardinality": fx["n_items"]}, "label": {}}, {"test": []},
                         {D.USER_CHANNEL: ["user"], D.ITEM_CHANNEL: ["item"], D.LABEL_CHANNEL: ["label"]},
                         {D.TEST_SAMPLES_PER_SERIES: fx["samples_in_series"]}, "")


def loader_of(fx):
    feats = {"user": fx["users"].view(-1, 1), "item": fx["items"].view(-1, 1), "label": fx["labels"].view(-1, 1)}
    return D.TestLoader(spec_of(fx), feats, fx["valid_batch_size"])


def test_restated_forward_reproduces_the_reference():
    fx, sd = fixture(), state()
    m = NM.model_from_state(sd).double()
    with torch.no_grad():
        got = m(fx["users"], fx["items"]).view(-1)
    assert float((got - fx["logit64"]).abs().max()) <= 1e-12
    ref = R.forward(T.Mode("exact"), sd, fx["users"], fx["items"]).v
    assert float((ref - fx["logit64"]).abs().max()) <= 1e-12
    # the logits spread over several units: there is something to rank
    assert float(fx["logit64"].std()) > 0.5


def test_restated_loader_reproduces_the_reference():
    fx = fixture()
    ld = loader_of(fx)
    assert torch.equal(ld.users, fx["sorted_users"]) and torch.equal(ld.items, fx["sorted_items"])
    assert torch.equal(ld.labels, fx["sorted_labels"]) and torch.equal(ld.mask, fx["mask"])
    assert len(ld.batches) == fx["n_batches"] and ld.raw_length == fx["users"].numel()
    assert [b[0].numel() for b in ld.batches] == [t.numel() for t in fx["users"].split(fx["valid_batch_size"])]
    # the mask never hides a label-1 element, and some positives do have a hidden duplicate
    assert not bool((ld.mask & (ld.labels == 1)).any())
    S = fx["samples_in_series"]
    items, lab, mask = ld.items.view(-1, S), ld.labels.view(-1, S), ld.mask.view(-1, S)
    pos_item = (items * (lab == 1)).sum(1, keepdim=True)
    assert int(((items == pos_item) & mask).any(1).sum()) >= fx["users"].numel() // S // 4


def test_rank_rule_and_loss_reproduce_val_epoch():
    fx = fixture()
    S, k = fx["samples_in_series"], fx["k"]
    rating = torch.sigmoid(fx["sorted_logit64"])
    hits, dcg = R.rank_rule(rating, fx["sorted_labels"], fx["mask"], S, k)
    n = rating.numel() // S
    assert abs(int(hits.sum()) / n - fx["hr"]) <= 1e-12
    assert abs(float(dcg.sum()) / n - fx["ndcg"]) <= 1e-12
    per = R.bce64(fx["sorted_logit64"], fx["sorted_labels"])
    loss = float(torch.stack([c.mean() for c in per.split(fx["valid_batch_size"])]).mean())
    assert abs(loss - fx["loss"]) <= 1e-12


def test_fixture_is_tie_free_and_boundary_clear():
    fx, sd = fixture(), state()
    S, k = fx["samples_in_series"], fx["k"]
    r = torch.sigmoid(fx["sorted_logit64"]).view(-1, S).clone()
    r[fx["mask"].view(-1, S)] = -1
    lab = fx["sorted_labels"].view(-1, S) == 1
    assert int(lab.sum()) == r.shape[0]
    for s in range(r.shape[0]):
        for j in torch.nonzero(lab[s]).flatten().tolist():
            assert int((r[s] == r[s, j]).sum()) == 1
    for dtype in (torch.float16, torch.bfloat16):
        e_emul = float((R.half_forward(sd, fx["sorted_users"], fx["sorted_items"], dtype) - fx["sorted_logit64"]).abs().max())
        clear = R.boundary_clear(fx["sorted_logit64"], fx["sorted_labels"], fx["mask"], S, k, 8 * e_emul)
        assert float(clear.double().mean()) >= 0.9, (dtype, e_emul)


def test_state_dict_names_and_shapes():
    want = json.load(open(os.path.join(GOLDEN, "ncf_state_dict.json")))
    for tag, (nu, ni) in (("ml-20m", (138493, 26744)), ("fixture", (61, 211))):
        got = NM.state_shapes(nu, ni)
        assert list(got) == list(want[tag]) and [list(v) for v in got.values()] == list(want[tag].values()), tag


def test_checkpoint_with_module_prefix_loads():
    ck = torch.load(os.path.join(GOLDEN, "ncf_checkpoint.pt"), map_location="cpu")
    assert all(k.startswith("module.") for k in ck)
    m = NM.load_checkpoint(os.path.join(GOLDEN, "ncf_checkpoint.pt"))
    assert (m.nb_users, m.nb_items, m.mf_dim, m.mlp_layer_sizes) == (61, 211, 64, (256, 256, 128, 64))
    sd = state()
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    fresh = NM.NeuMFModel(61, 211)
    fresh.load_state_dict(ck)
    assert torch.equal(fresh.final.weight, sd["final.weight"])


def test_initialisation_is_the_references():
    torch.manual_seed(0)
    m = NM.NeuMFModel(2000, 1000)
    for emb in (m.mf_user_embed, m.mf_item_embed, m.mlp_user_embed, m.mlp_item_embed):
        w = emb.weight.detach()
        assert abs(float(w.std()) - 0.01) < 5e-4 and abs(float(w.mean())) < 1e-4
    for lin in m.mlp:
        lim = (6.0 / (lin.in_features + lin.out_features)) ** 0.5
        assert 0.97 * lim < float(lin.weight.detach().abs().max()) <= lim
    lim = (3.0 / 128) ** 0.5
    assert 0.9 * lim < float(m.final.weight.detach().abs().max()) <= lim


@pytest.mark.parametrize("which,parser", [("inference", INF.get_parser), ("ncf", TST.get_parser)])
def test_every_reference_flag_and_default_parses(which, parser):
    flags = json.load(open(os.path.join(GOLDEN, "ncf_cli_flags.json")))[which]
    assert len(flags) >= 10
    p = parser()
    defaults = vars(p.parse_args([]))
    for f in flags:
        long = [x for x in f["flags"] if x.startswith("--")][0]
        dest = long[2:].replace("-", "_")
        assert dest in defaults, long
        assert defaults[dest] == f["default"], (long, defaults[dest], f["default"])
        for name in f["flags"]:                                     # every spelling, with a value of its kind
            if f["action"] == "store_true":
                argv = [name]
            elif f["choices"]:
                argv = [name, f["choices"][-1]]
            elif f["nargs"] == "+":
                argv = [name, "8", "4"]
            else:
                argv = [name, {"int": "3", "float": "0.5", "str": "x"}[f["type"]]]
            got = vars(p.parse_args(argv))[dest]
            assert got != f["default"] or f["default"] in ("x", 3, 0.5), (name, got)


def test_one_line_rejections(monkeypatch):
    with pytest.raises(SystemExit, match="--mode train is not built.*evaluation"):
        TST.main(["--data", "nowhere"])
    with pytest.raises(SystemExit, match="--mode train is not built"):
        TST.main(["--data", "nowhere", "--mode", "train", "--amp"])
    with pytest.raises(SystemExit, match="16 bits"):
        TST.main(["--data", "nowhere", "--mode", "test"])
    with pytest.raises(SystemExit, match="16 bits"):
        INF.main([])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="distributed evaluation is not built"):
        TST.main(["--data", "nowhere", "--mode", "test", "--amp"])
    monkeypatch.undo()
    fx = fixture()
    with pytest.raises(SystemExit, match="distributed evaluation is not built"):
        D.TestLoader(spec_of(fx), {}, 2048, world_size=2)
    with pytest.raises(SystemExit, match="--topk 101 does not fit a series of 100"):
        evaluate(None, loader_of(fx), 101)
    with pytest.raises(SystemExit, match="--topk 0"):
        evaluate(None, loader_of(fx), 0)


def test_score_supported_envelope():
    import __graft_entry__ as ge
    ge.build_product()
    from deeplearningexamples_amd import functional as F
    assert F.ncf_score_supported(64, [256, 256, 128, 64])
    assert not F.ncf_score_supported(32, [256, 256, 128, 64])
    assert not F.ncf_score_supported(64, [128, 128, 64, 32])
    assert not F.ncf_score_supported(64, [256, 256, 128, 32])
    assert not F.ncf_score_supported(64, [256, 128, 64])
    from deeplearningexamples_amd import _cabi
    assert _cabi.lib().dle_ncf_score_supported(64, 256, 256, 128, 64) == 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_bar_self_test(dtype):
    """The stated contract stays inside the bar; a model that drops a bias leaves it; so does, in fp16, one that also rounds the
    third layer's output and the GMF product to bf16 (eight times the contract's unit roundoff)."""
    sd = R.seeded_state(37, 23, 5, dtype)
    u, i = R.seeded_pairs(37, 23, 512, 6)
    bar = R.forward(T.Mode("bar", dtype), sd, u, i)
    emul = R.forward(T.Mode("emul", dtype), sd, u, i).v
    exact = R.forward(T.Mode("exact"), sd, u, i).v
    assert torch.equal(bar.v, exact)
    ratio = ((emul - exact).abs() / bar.bar()).max()
    print("contract / bar: %.3f   (max bar %.3e, max error %.3e)" % (float(ratio), float(bar.bar().max()), float((emul - exact).abs().max())))
    assert float(ratio) < 1.0
    assert float((emul - exact).abs().max()) > 0.0                  # the contract does round something
    dropped = R.forward(T.Mode("emul", dtype), sd, u, i, faults=("drop_b2",)).v
    assert float(((dropped - exact).abs() / bar.bar()).max()) > 1.0
    if dtype == torch.float16:
        only = _only_the_two_faults(sd, u, i)
        print("faults alone / bar: %.3f" % float(((only - exact).abs() / bar.bar()).max()))
        assert float(((only - exact).abs() / bar.bar()).max()) > 1.0


def _only_the_two_faults(sd, u, i):
    """fp16 contract roundings of layers 1 and 2, plus the third layer's output and the GMF product rounded to bf16."""
    M = T.Mode("emul", torch.float16)
    d = lambda n: sd[n].double()
    prod = T.to16(d(R.NAMES[0])[u] * d(R.NAMES[1])[i], torch.bfloat16)
    x = T.V(torch.cat((d(R.NAMES[2])[u], d(R.NAMES[3])[i]), dim=1))
    for l in range(3):
        x = R.relu(M, T.linear(M, x, d("mlp.%d.weight" % l), d("mlp.%d.bias" % l)))
        x = T.r16(M, x) if l < 2 else T.V(T.to16(x.v, torch.bfloat16))
    wf = d("final.weight").reshape(-1)
    return prod @ wf[:64] + x.v @ wf[64:] + d("final.bias").reshape(())


def test_rank_rule_statement():
    """Hand-checked cases of the rule itself."""
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    # ties across the k boundary: the earlier index wins
    hits, dcg = R.rank_rule(f(0.5, 0.5, 0.1), f(0, 1, 0), None, 3, 1)
    assert hits.tolist() == [0]
    hits, dcg = R.rank_rule(f(0.5, 0.5, 0.1), f(1, 0, 0), None, 3, 1)
    assert hits.tolist() == [1] and abs(float(dcg) - 1.0) < 1e-15
    # an ignored positive ranks with -1; NaN below everything, also below -1
    hits, _ = R.rank_rule(f(0.9, 0.2, float("nan")), f(1, 0, 0), torch.tensor([1, 0, 0]), 3, 2)
    assert hits.tolist() == [1]
    hits, _ = R.rank_rule(f(float("nan"), 0.2, 0.1), f(1, 0, 0), None, 3, 2)
    assert hits.tolist() == [0]
    hits, dcg = R.rank_rule(f(0.1, 0.9, 0.8, 0.7), f(1, 0, 1, 0), None, 4, 4)
    assert hits.tolist() == [2] and abs(float(dcg) - (np.log(2) / np.log(3) + np.log(2) / np.log(5))) < 1e-15
