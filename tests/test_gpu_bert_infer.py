"""BertPredictor (bert/infer.py) on the MI355X: the packed path against the fp32 CPU oracle at the padded path's own error, routing,
encode, checkpoint forms and the extract_features command line.  Tiny model: 2 layers, hidden 128, 2 heads of 64.

Accuracy bar.  Both paths round the same quantities the same number of times and differ only in how the GEMMs are routed by row
count, so the packed path's error against BertOracle(storage_dtype=None) may be as large as the padded path's on the same inputs
times a margin, in max-abs and in rms.  The margin is measured here, from the padded path and the oracle alone: the largest
seed-to-seed ratio (max / min) of the padded path's error over five input seeds on the first batch shape.

Measured on the MI355X (fp16; error of the MLM logits against the oracle, batch [1, 17, 128, 77] at S = 128; a record, the
assertion uses what the run itself measures):
    padded path, seeds 1 .. 5 (max-abs, rms): (7.50e-4, 1.74e-4) (6.71e-4, 1.70e-4) (8.75e-4, 1.88e-4) (7.94e-4, 1.71e-4)
    (1.06e-3, 2.00e-4): margin 1.579 (max-abs; rms alone gives 1.174)
    packed / padded error: 1.000 / 1.000 (max-abs / rms) for the MLM and NSP logits, layers and pooled output at S = 128 and
    S = 384 -- the same bits; at S = 200, where the padded baseline runs the batched-GEMM attention: MLM 1.000 / 0.996, NSP
    0.725 / 0.797, layers 1.000 / 1.002, pooled 1.062 / 1.027
"""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as TF

from oracle import bert_oracle as BO

pytestmark = pytest.mark.gpu

CFG = dict(hidden=128, heads=2, layers=2, intermediate=512, vocab=1024, real_vocab=1000, max_pos=512, type_vocab=2, seq=128)
BATCHES = [([1, 17, 128, 77], 128), ([384, 130, 2], 384), ([200, 9, 64], 200)]
DTYPE = torch.float16
SEEDS = (1, 2, 3, 4, 5)


def _F():
    from deeplearningexamples_amd import functional as F
    return F


def _batch(lengths, s, seed):
    """ids, token types, prefix mask, labels (-1 but at 3 valid positions per sequence: first, last, one between)."""
    g = torch.Generator().manual_seed(seed)
    b = len(lengths)
    lens = torch.tensor(lengths)
    ids = torch.randint(0, CFG["real_vocab"], (b, s), generator=g)
    mask = (torch.arange(s)[None, :] < lens[:, None]).to(torch.int64)
    tt = ((torch.arange(s)[None, :] >= (lens[:, None] + 1) // 2) & (mask == 1)).to(torch.int64)
    labels = -torch.ones((b, s), dtype=torch.int64)
    for i, n in enumerate(lengths):
        for p in {0, n - 1, n // 2}:
            labels[i, p] = int(ids[i, p])
    return ids, tt, mask, labels


@pytest.fixture(scope="module")
def state():
    return BO.seeded_state(CFG, 21)


@pytest.fixture(scope="module")
def predictor(cuda, state):
    from deeplearningexamples_amd.bert.infer import BertPredictor
    return BertPredictor(state, CFG, compute_dtype=DTYPE, device=cuda)


@pytest.fixture(scope="module")
def oracle(state):
    return BO.BertOracle(CFG, state, storage_dtype=None)


def _oracle_all(orc, ids, tt, mask, labels):
    """BertOracle.forward's fp32 statement with the hidden states of every layer and the pooled output kept (the oracle returns
    only the head outputs); its final logits are checked against orc.forward itself."""
    with torch.no_grad():
        p, c = orc.p, orc.cfg
        b, s = ids.shape
        h, nh = c["hidden"], c["heads"]
        d = h // nh
        e = (p["bert.embeddings.word_embeddings.weight"][ids] + p["bert.embeddings.position_embeddings.weight"][:s][None]
             + p["bert.embeddings.token_type_embeddings.weight"][tt])
        x = TF.layer_norm(e, (h,), p["bert.embeddings.LayerNorm.weight"], p["bert.embeddings.LayerNorm.bias"], 1e-12)
        ext = (1.0 - mask.float())[:, None, None, :] * -10000.0
        hidden = []
        for l in range(c["layers"]):
            pre = "bert.encoder.layer.%d." % l
            lin = lambda t, n: TF.linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"])
            q, k, v = (lin(x, "attention.self." + n).view(b, s, nh, d).transpose(1, 2) for n in ("query", "key", "value"))
            probs = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d) + ext, -1)
            ctx = torch.matmul(probs, v).transpose(1, 2).reshape(b, s, h)
            a = TF.layer_norm(lin(ctx, "attention.output.dense") + x, (h,), p[pre + "attention.output.LayerNorm.weight"],
                              p[pre + "attention.output.LayerNorm.bias"], 1e-12)
            it = BO.gelu(lin(a, "intermediate.dense_act"))
            x = TF.layer_norm(lin(it, "output.dense") + a, (h,), p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], 1e-12)
            hidden.append(x)
        pooled = torch.tanh(TF.linear(x[:, 0], p["bert.pooler.dense_act.weight"], p["bert.pooler.dense_act.bias"]))
        scores, nsp, sel = orc.forward(ids, tt, mask, labels)
        nsp_here = TF.linear(pooled, p["cls.seq_relationship.weight"], p["cls.seq_relationship.bias"])
        assert torch.allclose(nsp_here, nsp, rtol=0, atol=1e-6), "the test's restatement left the oracle"
        return dict(hidden=hidden, pooled=pooled, scores=scores.detach(), nsp=nsp.detach(), sel=sel)


def _err(got, ref):
    d = (got.detach().float().cpu() - ref.float()).double()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


_REF = {}


def _ref(oracle, lengths, s, seed=SEEDS[0]):
    key = (tuple(lengths), s, seed)
    if key not in _REF:
        batch = _batch(lengths, s, seed)
        _REF[key] = (batch, _oracle_all(oracle, *batch))
    return _REF[key]


@pytest.fixture(scope="module")
def margin(predictor, oracle):
    """Largest seed-to-seed ratio of the PADDED path's error against the oracle (max-abs and rms taken separately, the larger)."""
    lengths, s = BATCHES[0]
    errs = []
    for seed in SEEDS:
        (ids, tt, mask, labels), o = _ref(oracle, lengths, s, seed)
        logits, _ = predictor.pretraining_logits(ids, tt, mask, o["sel"], packed=False)
        errs.append(_err(logits, o["scores"]))
    m = max(max(e[i] for e in errs) / min(e[i] for e in errs) for i in (0, 1))
    print("\npadded-path error against the oracle over seeds %s (max-abs, rms): %s; margin %.3f" % (
        SEEDS, "  ".join("(%.3e, %.3e)" % e for e in errs), m))
    assert m >= 1.0
    return m


def _check(name, got_packed, got_padded, ref, margin):
    ep, eb = _err(got_packed, ref), _err(got_padded, ref)
    print("%s: packed (max-abs %.3e, rms %.3e)  padded (%.3e, %.3e)  ratios %.3f %.3f  margin %.3f" % (
        name, ep[0], ep[1], eb[0], eb[1], ep[0] / eb[0], ep[1] / eb[1], margin))
    assert ep[0] <= margin * eb[0] and ep[1] <= margin * eb[1], name


@pytest.mark.parametrize("lengths,s", BATCHES, ids=["S128", "S384", "S200"])
def test_packed_logits_at_the_padded_paths_error(predictor, oracle, margin, lengths, s):
    F = _F()
    (ids, tt, mask, labels), o = _ref(oracle, lengths, s)
    before = F.attention_varlen_launch_count()
    logits, nsp = predictor.pretraining_logits(ids, tt, mask, o["sel"], packed=None)
    assert predictor.last_route == "packed"
    assert F.attention_varlen_launch_count() == before + CFG["layers"]
    assert logits.shape == (o["sel"].numel(), CFG["vocab"]) and logits.dtype == torch.float32 and nsp.shape == (len(lengths), 2)
    base_logits, base_nsp = predictor.pretraining_logits(ids, tt, mask, o["sel"], packed=False)
    assert predictor.last_route == "padded" and F.attention_varlen_launch_count() == before + CFG["layers"]
    _check("MLM logits %s" % (lengths,), logits, base_logits, o["scores"], margin)
    _check("NSP logits %s" % (lengths,), nsp, base_nsp, o["nsp"], margin)


def test_routing(predictor, oracle):
    F = _F()
    lengths, s = [128, 128, 128], 128
    ids, tt, mask, labels = _batch(lengths, s, 9)
    before = F.attention_varlen_launch_count()
    full, pooled = predictor.encode(ids, tt, mask)
    assert predictor.last_route == "padded" and F.attention_varlen_launch_count() == before
    # a hole in the middle of a sequence: not prefix-form
    ids, tt, mask, labels = _batch([1, 17, 128, 77], 128, 9)
    hole = mask.clone()
    hole[3, 40] = 0
    got, gp = predictor.encode(ids, tt, hole)
    assert predictor.last_route == "padded" and F.attention_varlen_launch_count() == before
    want, wp = predictor.encode(ids, tt, hole, packed=False)
    assert torch.equal(got[0], want[0]) and torch.equal(gp, wp)
    assert not bool(got[0][3, 40].any()) and bool(got[0][3, 41].any())
    with pytest.raises(ValueError):
        predictor.encode(ids, tt, hole, packed=True)
    # forced packed on a full batch runs the packed kernel
    predictor.encode(*_batch(lengths, s, 9)[:3], packed=True)
    assert predictor.last_route == "packed" and F.attention_varlen_launch_count() == before + CFG["layers"]


def test_full_batch_outside_the_padded_paths_reach_goes_packed(cuda, state):
    """S = 600 is no multiple of 128 and past the softmax kernel's 512 keys: the padded path cannot run, so the router sends a
    full batch to the packed kernel; a mask that is not prefix-form has no path there and says so."""
    from deeplearningexamples_amd.bert.infer import BertPredictor
    F = _F()
    cfg = dict(CFG, max_pos=640)
    g = torch.Generator().manual_seed(5)
    sd = {k: v.clone() for k, v in state.items()}
    sd["bert.embeddings.position_embeddings.weight"] = torch.randn(640, CFG["hidden"], generator=g) * 0.02
    p = BertPredictor(sd, cfg, compute_dtype=DTYPE, device=cuda)
    ids, tt, mask, _ = _batch([600, 600], 600, 6)
    before = F.attention_varlen_launch_count()
    layers, pooled = p.encode(ids, tt, mask)
    assert p.last_route == "packed" and F.attention_varlen_launch_count() == before + CFG["layers"]
    assert layers[0].shape == (2, 600, CFG["hidden"]) and bool(torch.isfinite(layers[0].float()).all())
    # the same rows as two sequences of a longer, partly filled batch (row-wise kernels, per-sequence attention)
    ids2, tt2, mask2 = (torch.cat([x, torch.zeros(2, 40, dtype=x.dtype)], 1) for x in (ids, tt, mask))
    longer, _ = p.encode(ids2, tt2, mask2)
    assert torch.equal(longer[0][:, :600], layers[0]) and not bool(longer[0][:, 600:].any())
    hole = mask.clone()
    hole[1, 300] = 0
    with pytest.raises(ValueError):
        p.encode(ids, tt, hole)


def test_positions_are_checked_in_the_one_synchronisation(predictor):
    ids, tt, mask, labels = _batch([1, 17, 128, 77], 128, 4)
    for packed in (None, False):
        for bad in (128 + 17, 4 * 128, -1):                         # a padding token, past the batch, negative
            with pytest.raises(ValueError):
                predictor.pretraining_logits(ids, tt, mask, torch.tensor([0, bad]), packed=packed)


@pytest.mark.parametrize("lengths,s", BATCHES, ids=["S128", "S384", "S200"])
def test_encode_layers_padding_and_pooled(predictor, oracle, margin, lengths, s):
    (ids, tt, mask, labels), o = _ref(oracle, lengths, s)
    layers, pooled = predictor.encode(ids, tt, mask, layers=(-1, -2, 0))
    assert predictor.last_route == "packed"
    base, base_pooled = predictor.encode(ids, tt, mask, layers=(-1, -2, 0), packed=False)
    valid = mask.bool()
    for got, bs, li in zip(layers, base, (1, 0, 0)):
        assert got.shape == (len(lengths), s, CFG["hidden"]) and got.dtype == DTYPE
        assert not bool(got.cpu()[~valid].any()) and not bool(bs.cpu()[~valid].any()), "padding rows must be zero"
        ref = o["hidden"][li]
        _check("layer %d %s" % (li, lengths), got.cpu()[valid], bs.cpu()[valid], ref[valid], margin)
    assert torch.equal(layers[1], layers[2])
    _check("pooled %s" % (lengths,), pooled, base_pooled, o["pooled"], margin)
    # the pooled output is a function of row 0 of each sequence alone
    from deeplearningexamples_amd import _cabi as C
    F = _F()
    first = layers[0][:, 0].contiguous()
    again = F.gemm(first, predictor.pool, len(lengths), CFG["hidden"], CFG["hidden"], True, True, bias=predictor.pool_b,
                   act=C.ACT_TANH)
    assert torch.equal(again, pooled)


def test_loading_forms_give_identical_bits(cuda, state, predictor):
    from deeplearningexamples_amd.bert.infer import BertPredictor
    from deeplearningexamples_amd.bert.model import BertForPreTraining
    ids, tt, mask, labels = _batch([1, 17, 128, 77], 128, 4)
    pos = torch.nonzero(labels.reshape(-1) != -1).squeeze(1)
    want_layers, want_pooled = predictor.encode(ids, tt, mask)
    want_logits, want_nsp = predictor.pretraining_logits(ids, tt, mask, pos)
    module = BertForPreTraining(CFG, device=cuda)
    module.load_state_dict({k: v.clone() for k, v in state.items()}, strict=False)
    full_sd = module.state_dict()
    assert "cls.predictions.decoder.weight" in full_sd
    forms = {"module": (module, None), "state dict with the tied decoder": (full_sd, CFG), "ckpt dictionary": ({"model": state}, CFG),
             "module. prefix": ({"module." + k: v for k, v in state.items()}, CFG)}
    for name, (src, cfg) in forms.items():
        p = BertPredictor(src, cfg, compute_dtype=DTYPE, device=cuda)
        layers, pooled = p.encode(ids, tt, mask)
        logits, nsp = p.pretraining_logits(ids, tt, mask, pos)
        assert torch.equal(layers[0], want_layers[0]) and torch.equal(pooled, want_pooled), name
        assert torch.equal(logits, want_logits) and torch.equal(nsp, want_nsp), name
    enc = BertPredictor({k: v for k, v in state.items() if not k.startswith("cls.")}, CFG, compute_dtype=DTYPE, device=cuda)
    assert not enc.has_heads
    layers, pooled = enc.encode(ids, tt, mask)
    assert torch.equal(layers[0], want_layers[0]) and torch.equal(pooled, want_pooled)
    with pytest.raises(ValueError):
        enc.pretraining_logits(ids, tt, mask, pos)


def test_extract_features_cli(cuda, golden_dir, tmp_path, predictor, state):
    from deeplearningexamples_amd.bert import extract_features as X
    from deeplearningexamples_amd.bert import tokenization as T
    fx = json.load(open(os.path.join(golden_dir, "bert_tokenizer.json"), encoding="utf-8"))
    vocab_file, cfg_file, ckpt, inp, out = (str(tmp_path / n) for n in ("vocab.txt", "config.json", "ckpt_10.pt", "in.txt", "out.jsonl"))
    open(vocab_file, "w", encoding="utf-8").write("\n".join(fx["vocab"]) + "\n")
    json.dump(dict(vocab_size=CFG["real_vocab"], hidden_size=CFG["hidden"], num_attention_heads=CFG["heads"],
                   num_hidden_layers=CFG["layers"], intermediate_size=CFG["intermediate"], max_position_embeddings=CFG["max_pos"],
                   type_vocab_size=CFG["type_vocab"]), open(cfg_file, "w"))
    torch.save({"model": state, "epoch": 0}, ckpt)
    lines = ["The quick brown fox jumps over the lazy dog.", "hello world ||| the dog runs", "unaffable café 中文!"]
    open(inp, "w", encoding="utf-8").write("\n".join(lines) + "\n")
    X.main(["--input_file", inp, "--output_file", out, "--vocab_file", vocab_file, "--config_file", cfg_file, "--init_checkpoint", ckpt,
            "--do_lower_case", "--layers=-1,0", "--max_seq_length", "24", "--batch_size", "2"])
    recs = [json.loads(l) for l in open(out, encoding="utf-8")]
    assert [r["linex_index"] for r in recs] == [0, 1, 2]
    tk = T.BertTokenizer(vocab_file, do_lower_case=True)
    built = [T.build_input(tk, *T.parse_line(l), 24) for l in lines]
    for start in (0, 2):                                                       # the batches the tool formed
        chunk = built[start:start + 2]
        ids, mask, types = (torch.tensor([c[k] for c in chunk]) for k in (1, 2, 3))
        layers, _ = predictor.encode(ids, types, mask, layers=(-1, 0))
        for i, c in enumerate(chunk):
            rec = recs[start + i]
            assert [f["token"] for f in rec["features"]] == c[0]
            assert c[0][0] == "[CLS]" and c[0][-1] == "[SEP]"
            for t, f in enumerate(rec["features"]):
                assert [l["index"] for l in f["layers"]] == [-1, 0]
                for j in range(2):
                    vals = f["layers"][j]["values"]
                    assert len(vals) == CFG["hidden"]
                    assert vals == [round(x, 6) for x in layers[j][i, t].float().cpu().tolist()]
    assert recs[1]["features"][3]["token"] == "[SEP]" and recs[2]["features"][-2]["token"] == "!"
