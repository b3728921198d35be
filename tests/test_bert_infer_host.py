"""Host side of BERT inference (no GPU): the WordPiece tokenizer against a fixture recorded from the reference's tokenizer, the
packed-layout bookkeeping and routing rule of bert/infer.py, the extract_features command line and JSON writer, and the CPU model
of the attention kernels at the packed-attention length sets."""
import io
import json
import os

import pytest
import torch

from deeplearningexamples_amd.bert import extract_features as X
from deeplearningexamples_amd.bert import infer as I
from deeplearningexamples_amd.bert import tokenization as T
from tests import _attention_reference as A
from tests import _varlen_cases as V


@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    fx = json.load(open(os.path.join(golden_dir, "bert_tokenizer.json"), encoding="utf-8"))
    assert "reference's own tokenizer" in fx["_header"]
    vf = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    vf.write_text("\n".join(fx["vocab"]) + "\n", encoding="utf-8")
    fx["vocab_file"] = str(vf)
    return fx


# ------------------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_matches_the_recorded_reference(fixture):
    tks = {lower: T.BertTokenizer(fixture["vocab_file"], do_lower_case=lower) for lower in (True, False)}
    assert len(fixture["cases"]) >= 30
    for c in fixture["cases"]:
        tk = tks[c["do_lower_case"]]
        toks = tk.tokenize(c["text"])
        assert toks == c["tokens"], (c["text"], c["do_lower_case"], toks, c["tokens"])
        assert tk.convert_tokens_to_ids(toks) == c["ids"]
        assert tk.convert_ids_to_tokens(c["ids"]) == c["tokens"]
    seen = [t for c in fixture["cases"] for t in c["tokens"]]
    assert "[UNK]" in seen and "中" in seen and any(t.startswith("##") for t in seen)


def test_pairs_and_truncation_match_the_recorded_reference(fixture):
    tk = T.BertTokenizer(fixture["vocab_file"], do_lower_case=True)
    assert {f["seq_length"] for f in fixture["features"]} == {8, 16}
    for f in fixture["features"]:
        tokens, ids, mask, types = T.build_input(tk, *T.parse_line(f["line"] + "\n"), f["seq_length"])
        assert tokens == f["tokens"], (f["line"], f["seq_length"])
        assert ids == f["input_ids"] and mask == f["input_mask"] and types == f["input_type_ids"]
        assert len(ids) == len(mask) == len(types) == f["seq_length"]


# ------------------------------------------------------------------------------------------------ lengths, layout, routing
def _mask(lengths, s):
    return (torch.arange(s)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64)


def test_lengths_prefix_and_cu_seqlens():
    m = _mask([1, 17, 128, 77], 128)
    assert I.lengths_and_prefix(m) == ([1, 17, 128, 77], True)
    assert I.lengths_and_prefix(_mask([0, 5], 8)) == ([0, 5], True)
    hole = m.clone()
    hole[1, 5] = 0
    assert I.lengths_and_prefix(hole) == ([1, 16, 128, 77], False)
    shifted = torch.tensor([[0, 1, 1, 0]])
    assert I.lengths_and_prefix(shifted) == ([2], False)
    # positions ride on the same synchronisation: in range and at ones of the mask
    m8 = _mask([3, 8], 8)
    assert I.inspect_batch(m8) == ([3, 8], True, True)
    assert I.inspect_batch(m8, torch.tensor([0, 2, 8, 15])) == ([3, 8], True, True)
    assert I.inspect_batch(m8, torch.tensor([], dtype=torch.int64)) == ([3, 8], True, True)
    for bad in ([3], [0, 16], [-1]):                                 # a padding token, past the batch, negative
        assert I.inspect_batch(m8, torch.tensor(bad)) == ([3, 8], True, False)
    cu = I.cu_seqlens([1, 17, 128, 77])
    assert cu.dtype == torch.int32 and cu.tolist() == [0, 1, 18, 146, 223]
    assert I.cu_seqlens([]).tolist() == [0]


def test_routing_predicate():
    ch = I.choose_packed
    assert ch([1, 17, 128, 77], True, 128, True) is True
    assert ch([128, 128], True, 128, True) is False                 # nothing to save: T == B * S
    assert ch([1, 17], False, 128, True) is False                   # not prefix-form
    assert ch([0, 17], True, 128, True) is False                    # an empty sequence
    assert ch([1, 17], True, 128, False) is False                   # head size / length outside the kernel
    assert ch([1, 17], True, 128, True, packed=False) is False
    assert ch([128, 128], True, 128, True, packed=True) is True     # forced: allowed even when it saves nothing
    for lengths, prefix, sup in (([1, 17], False, True), ([0, 17], True, True), ([1, 17], True, False)):
        with pytest.raises(ValueError):
            ch(lengths, prefix, 128, sup, packed=True)
    assert ch([64, 64], True, 128, True, max_fill=0.4) is False and ch([64, 64], True, 128, True, max_fill=0.5) is True
    # where the padded path cannot run (S = 600: no multiple of 128, keys past the softmax kernel) a full batch goes packed
    assert I.padded_supported(128, 64, True) and I.padded_supported(200, 64, False) and I.padded_supported(512, 64, False)
    assert not I.padded_supported(600, 64, False) and I.padded_supported(640, 64, True)
    assert ch([600, 600], True, 600, True, padded_ok=False) is True
    assert ch([600, 600], True, 600, True, packed=False, padded_ok=False) is False
    assert ch([600, 30], False, 600, True, padded_ok=False) is False
    assert ch([600, 600], True, 600, True, max_fill=0.4, padded_ok=False) is True
    assert I.resolve_layers((-1, -2, 0), 2) == [1, 0, 0]
    with pytest.raises(ValueError):
        I.resolve_layers((2,), 2)


def test_state_dict_forms():
    sd = {"bert.pooler.dense_act.bias": torch.zeros(2), "cls.predictions.decoder.weight": torch.zeros(1)}
    want = ["bert.pooler.dense_act.bias"]
    assert list(I.clean_state_dict(sd)) == want
    assert list(I.clean_state_dict({"model": sd, "optimizer": {}})) == want
    assert list(I.clean_state_dict({"module." + k: v for k, v in sd.items()})) == want


# ------------------------------------------------------------------------------------------------ command line and writer
BASE = ["--input_file", "in.txt", "--output_file", "out.jsonl", "--vocab_file", "v.txt", "--config_file", "c.json",
        "--init_checkpoint", "ckpt.pt"]


def test_cli_flags():
    a = X.parse_args(BASE)
    assert a.layer_indexes == [-1, -2, -3, -4] and a.max_seq_length == 128 and a.batch_size == 32
    assert not a.do_lower_case and a.local_rank == -1 and a.amp_dtype == "fp16"
    a = X.parse_args(BASE + ["--do_lower_case", "--layers=-1,0", "--max_seq_length", "200", "--batch_size", "8",
                             "--local_rank", "0", "--amp-dtype", "bf16"])
    assert a.do_lower_case and a.layer_indexes == [-1, 0] and a.max_seq_length == 200 and a.batch_size == 8 and a.amp_dtype == "bf16"
    with pytest.raises(SystemExit) as e:
        X.parse_args(BASE + ["--no_cuda"])
    assert "MI355X" in str(e.value)
    with pytest.raises(SystemExit):
        X.parse_args(BASE + ["--layers", "last"])
    with pytest.raises(SystemExit):
        X.parse_args(BASE[2:])


def test_json_writer_on_cpu_tensors():
    tokens = ["[CLS]", "hello", "[SEP]"]
    l0 = torch.tensor([[0.1234567, -1.0], [2.00000049, 3.5], [1e-7, -1e-7], [9.0, 9.0]])       # row 3: padding, not written
    l1 = l0 * 2
    fh = io.StringIO()
    X.write_features(fh, 7, tokens, [-1, 0], [l0, l1])
    line = fh.getvalue()
    assert line.endswith("\n") and line.count("\n") == 1
    rec = json.loads(line)
    assert list(rec) == ["linex_index", "features"] and rec["linex_index"] == 7
    assert [f["token"] for f in rec["features"]] == tokens
    for i, f in enumerate(rec["features"]):
        assert [l["index"] for l in f["layers"]] == [-1, 0]
        assert f["layers"][0]["values"] == [round(float(x), 6) for x in l0[i]]
        assert f["layers"][1]["values"] == [round(float(x), 6) for x in l1[i]]
    assert rec["features"][0]["layers"][0]["values"][0] == 0.123457


# ------------------------------------------------------------------------------------------------ the kernels' CPU model
@pytest.mark.parametrize("dtype", A.DTYPES, ids=A.name)
@pytest.mark.parametrize("lengths", V.LENGTH_SETS, ids=lambda ls: "-".join(str(x) for x in ls))
def test_kernel_model_stays_inside_the_bars_at_the_valid_rows(lengths, dtype):
    """The arithmetic the attention kernels perform (tests/_attention_reference.kernel_model: blocked online max / sum, P rounded
    once), on the padded batch under the length mask, holds the float64 bars at the valid rows of every packed length set."""
    nh = 2
    c = V.build(lengths, nh, dtype)
    dctx = torch.zeros(c["b"] * c["s"], nh * A.D, dtype=dtype)
    out = A.kernel_model(c["qkv_pad"], dctx, c["mask_add"], None, c["b"], c["s"], nh, V.SCALE, 1.0)
    ratios = V.check_valid_rows(out["ctx"], c, lengths, nh, dtype, "kernel model")
    assert ratios["ctx"] <= 1.0 and ratios["ctx_l2"] <= 1.0
