"""TransformerXLEvaluator (deeplearningexamples_amd/transformer_xl/infer.py) against the float64 forward of tests/_txl_ref.py, its
state, its launch list, the absence of host reads, the checkpoint form and the command line.  GPU only.

Cases: those of tests/test_txl_host.py (div_val 1 / 2, same_length, clamp_len 12 / -1; 2 layers, 2 heads, d_model 128; batch 3,
five segments of tgt_len 8 and a last one of 3, mem_len 20), fp16 and bf16.

Reference.  _txl_ref.RefModel.forward: the reference's own formulation in float64 (pinned to the reference's recorded output by
the host test).  Yardstick, the project's established one: forward_kv with every value rounded to the 16-bit type where the
evaluator rounds (weights, embeddings, every GEMM output, a and b, the probabilities, both LayerNorms; fp32 logits).  With E the
RMS error of the per-token nll against the unrounded forward over all WARM tokens (the segments behind the first ceil(mem_len /
tgt_len) = 3, as LMOrderedIterator counts them): E_new <= 1.5 E_emulated; the factor and its justification are those of
tests/test_gpu_resnext_infer.py (the evaluator's fp32 accumulations are not the emulation's float64 ones, so the two sets of
roundings fall differently: equal in distribution, not in value).  Both values are printed.
On the MI355X (a record): E_new / E_emulated 0.94 - 1.02 in fp16 (E_emulated 1.1e-3 - 1.2e-3), 0.91 - 1.01 in bf16 (7.7e-3 - 9.4e-3).
"""
import functools
import math
import os
import shutil

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.transformer_xl import eval as E
from deeplearningexamples_amd.transformer_xl import model as M
from deeplearningexamples_amd.transformer_xl.infer import TransformerXLEvaluator
from tests import _txl_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
SEED, TOKEN_SEED, WARM_FROM = 3, 5, 3
CASE_IDS = [c[0] for c in R.CASES]


@functools.lru_cache(maxsize=None)
def case(name):
    _, dv, same, clamp = next(c for c in R.CASES if c[0] == name)
    cfg = R.small_config(dv, same, clamp)
    state = R.fill_state(cfg, SEED)
    toks = R.make_tokens(cfg, TOKEN_SEED, R.BATCH * (sum(R.SEGMENTS) + 1))
    return cfg, state, R.stream_batches(toks, R.BATCH, R.SEGMENTS)


@functools.lru_cache(maxsize=None)
def references(name, dtype):
    cfg, state, batches = case(name)
    ref = R.RefModel(cfg, state)
    return ref.run(batches, "forward")[0], ref.run(batches, "kv", dtype)[0]


@functools.lru_cache(maxsize=None)
def evaluator(name, dtype, bsz=R.BATCH):
    cfg, state, _ = case(name)
    return TransformerXLEvaluator(M.TransformerXLModel(cfg).load_state_dict(state), bsz, dtype=dtype)


def run_stream(ev, batches):
    ev.reset()
    return [ev.segment(d.contiguous(), t.contiguous()) for d, t in batches]


def rms(a, b):
    return float((torch.cat([x.reshape(-1) for x in a]) - torch.cat([x.reshape(-1) for x in b])).pow(2).mean().sqrt())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CASE_IDS)
def test_nll_against_float64(name, dtype):
    cfg, state, batches = case(name)
    exact, emu = references(name, dtype)
    got = [g.cpu().double() for g in run_stream(evaluator(name, dtype), batches)]
    assert [tuple(g.shape) for g in got] == [(q, R.BATCH) for q in R.SEGMENTS]
    assert all(bool(torch.isfinite(g).all()) for g in got)
    e_new, e_emu = rms(got[WARM_FROM:], exact[WARM_FROM:]), rms(emu[WARM_FROM:], exact[WARM_FROM:])
    print("%s %s: warm tokens E_new %.4e, E_emulated %.4e, ratio %.3f; all tokens E_new %.4e, E_emulated %.4e" % (
        name, dtype, e_new, e_emu, e_new / e_emu, rms(got, exact), rms(emu, exact)))
    assert e_new <= 1.5 * e_emu, "RMS error %.4e against %.4e of the emulated roundings" % (e_new, e_emu)


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_reset_and_batch_independence(dtype):
    name = "dv2_same_clamp"
    cfg, state, batches = case(name)
    ev = evaluator(name, dtype)
    ev.reset()
    seen, outs = [], []
    for d, t in batches:
        seen.append((ev.mlen, ev.start))
        outs.append(ev.segment(d.contiguous(), t.contiguous()))
    cap = ev.cap
    assert cap == 28 and [m for m, _ in seen] == [0, 8, 16, 20, 20, 20]
    assert [s for _, s in seen] == [0, 0, 0, 4, 12, 20]
    # segments 4 and 5 write rows (start + mlen + t) % cap that wrap: 24..31 -> 24..27, 0..3 and 32..39 -> 4..11
    assert (seen[3][1] + seen[3][0] + 7) >= cap and (seen[4][1] + seen[4][0]) >= cap
    assert (ev.mlen, ev.start) == (20, (20 + 20 + 3 - 20) % cap)
    again = run_stream(ev, batches)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "reset() followed by the same stream gave other bits"
    ev1 = evaluator(name, dtype, 1)
    for b in range(R.BATCH):
        alone = run_stream(ev1, [(d[:, b:b + 1], t[:, b:b + 1]) for d, t in batches])
        for s, (x, y) in enumerate(zip(alone, outs)):
            assert torch.equal(x[:, 0], y[:, b]), "stream %d alone and in the batch differ in segment %d" % (b, s)


def test_launches_and_no_host_reads(monkeypatch):
    name = "dv2"
    cfg, state, batches = case(name)
    ev = evaluator(name, BF)
    run_stream(ev, batches)                                                     # warm: nothing lazily built is counted below
    ev.reset()
    from deeplearningexamples_amd import functional as F
    names, copies = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (copies.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "numpy", (lambda real_np: lambda self, *a, **k: (copies.append("numpy") if self.is_cuda else None,
                                                                                           real_np(self, *a, **k))[1])(torch.Tensor.numpy))
    per_segment = []
    before = F.txl_attention_launch_count()
    for d, t in batches:
        del names[:]
        ev.segment(d.contiguous(), t.contiguous())
        per_segment.append(list(names))
    monkeypatch.undo()
    assert copies == [], copies
    L = cfg["n_layer"]
    assert F.txl_attention_launch_count() == before + L * len(batches)
    for (d, t), nm in zip(batches, per_segment):
        assert nm.count("dle_txl_rel_attention_fwd") == L and nm.count("dle_txl_kv_append") == L and nm.count("dle_layernorm_fwd") == 2 * L
        assert not [n for n in nm if "attention" in n and n != "dle_txl_rel_attention_fwd"] and "dle_softmax" not in " ".join(nm)
        ends = [0] + cfg["cutoffs"] + [cfg["n_token"]]
        emb = sum(1 for lo, hi in zip(ends, ends[1:]) if bool(((d >= lo) & (d < hi)).any()))
        tails = sum(1 for lo, hi in zip(ends[1:], ends[2:]) if bool(((t >= lo) & (t < hi)).any()))
        # div_val 2: every bucket has a projection.  gathers: 2 per embedding bucket, 1 per tail; nll: the head and each tail
        assert nm.count("dle_rows_gather_scale") == 2 * emb + tails and nm.count("dle_row_nll") == 1 + tails
        assert nm.count("dle_gemm") == emb + 4 * L + 2 * (1 + tails)
        assert set(nm) == {"dle_rows_gather_scale", "dle_gemm", "dle_txl_kv_append", "dle_txl_rel_attention_fwd", "dle_layernorm_fwd",
                           "dle_row_nll"}
    first = [n for n in per_segment[0] if n in ("dle_gemm", "dle_txl_kv_append", "dle_txl_rel_attention_fwd", "dle_layernorm_fwd")]
    layer = ["dle_gemm", "dle_txl_kv_append", "dle_txl_rel_attention_fwd", "dle_gemm", "dle_layernorm_fwd", "dle_gemm", "dle_gemm",
             "dle_layernorm_fwd"]
    i = first.index("dle_txl_kv_append") - 1
    assert first[i:i + 8 * L] == layer * L


@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_round_trip(dtype, tmp_path):
    import argparse
    name = "dv1_same"
    cfg, state, batches = case(name)
    model = M.TransformerXLModel(cfg).load_state_dict(state)
    vocab = M.Vocab.from_symbols(["<unk>"] + ["w%d" % i for i in range(cfg["n_token"] - 2)])
    assert len(vocab) == cfg["n_token"]
    path = str(tmp_path / "checkpoint_best.pt")
    M.save_checkpoint(path, model, vocab, argparse.Namespace(vocab="word", dataset="wt103"))
    ev = TransformerXLEvaluator.from_checkpoint(path, R.BATCH, cfg["tgt_len"], cfg["mem_len"], clamp_len=cfg["clamp_len"],
                                                same_length=cfg["same_length"], dtype=dtype)
    assert ev.vocab.idx2sym == vocab.idx2sym and ev.args.vocab == "word"
    # (the file holds fp32 weights; both evaluators round the same fp32 values to the 16-bit type)
    direct = TransformerXLEvaluator(M.TransformerXLModel(cfg).load_state_dict({k: v.float() for k, v in state.items()}), R.BATCH, dtype=dtype)
    a, b = run_stream(ev, batches), run_stream(direct, batches)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_command_line_on_a_text_file(amp, tmp_path, capsys):
    shutil.copy(os.path.join(GOLDEN, "txl_text.txt"), str(tmp_path / "test.txt"))
    ckpt = os.path.join(GOLDEN, "txl_checkpoint.pt")
    argv = ["--cuda", "--model", ckpt, "--data", str(tmp_path), "--split", "test", "--batch_size", "2", "--tgt_len", "4", "--mem_len", "6",
            "--log_interval", "2", "--work_dir", str(tmp_path), "--save_data"] + (["--fp16"] if amp == "fp16" else ["--amp-dtype", "bf16"])
    loss = E.main(argv)
    out = capsys.readouterr().out
    line = E.format_log(loss, "test", E.get_parser().parse_args(["--fp16"]))
    assert line in out and "| step" in out and "ms/batch" in out and "Throughput Avg" in out
    # the evaluator's own mean over the warm tokens of the same iterator
    dtype = HF if amp == "fp16" else BF
    ev = TransformerXLEvaluator.from_checkpoint(ckpt, 2, 4, 6, dtype=dtype)
    tensor = ev.vocab.encode_file(str(tmp_path / "test.txt"))
    total, n = 0.0, 0
    for data, target, seq_len, warm in E.LMOrderedIterator(tensor, bsz=2, bptt=4, mem_len=6, ext_len=0):
        m = float(ev.segment(data.contiguous(), target.contiguous()).mean())
        if warm:
            total, n = total + seq_len * m, n + seq_len
    assert n > 0 and abs(loss - total / n) <= 1e-6 * abs(loss)
    assert ("ppl %9.3f" % math.exp(total / n)) in out
    assert os.path.exists(str(tmp_path / ("eval_data_2_%s_pytorch" % amp)))
    # the exit status follows the targets
    with pytest.raises(SystemExit) as e:
        E.main(argv + ["--target_perplexity", "1.5"])
    assert e.value.code == 1
    capsys.readouterr()
