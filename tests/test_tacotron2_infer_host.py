"""Tacotron2 inference on the CPU: the plain-torch statement of Tacotron2.infer (tests/_tacotron2_infer_doubles.py) against the
fixture the REFERENCE's own Tacotron2.infer produced under the prenet-mask contract (tests/golden/tacotron2_infer.npz,
tools/make_tacotron2_infer_golden.py), the host sequencing of Tacotron2Synthesizer with the C-ABI calls replaced by doubles
(chunking, truncation after the stop, max_decoder_steps), the mask contract, the command line and the new symbols.  The kernels
are checked on the GPU (tests/test_gpu_tacotron2_infer.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _tacotron2_infer_doubles as DI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("dle_t2_prenet_infer", "dle_t2_frame_infer")


def _case():
    from oracle import tacotron2_oracle as TO
    gold = np.load(os.path.join(HERE, "golden", "tacotron2_infer.npz"))
    cfg = TO.TACOTRON2_SMALL
    p = DI.full_state(cfg, int(gold["model_seed"][0]), int(gold["gate_seed"][0]), float(gold["gate_scale"][0]), float(gold["gate_bias"][0]))
    return cfg, p, gold, torch.from_numpy(gold["text"]), torch.from_numpy(gold["text_lengths"]), int(gold["seed"][0])


def _max_steps(gold, tag):
    return 2000 if tag == "a" else int(gold["b_max_decoder_steps"][0])


def test_fixture_has_the_cases_and_the_margin_the_issue_asks_for():
    cfg, p, gold, text, lengths, seed = _case()
    ml = gold["a_mel_lengths"].tolist()
    assert len(set(ml)) == 3 and gold["a_mel_post"].shape[2] == max(ml) + 1 < 40          # three different stops, the last below 40
    assert len(set(gold["text_lengths"].tolist())) == 3
    cut = int(gold["b_max_decoder_steps"][0])
    assert cut < min(ml) and gold["b_mel_post"].shape[2] == cut and gold["b_mel_lengths"].tolist() == [cut] * 3
    assert float(gold["margin"][0]) >= 10.0 * float(gold["bf16_deviation"][0])
    # the margin, re-derived here from the reference's gate logits: every (step, sample) up to the sample's stop
    g = gold["a_gate"]
    live = np.arange(g.shape[1])[None, :] <= np.asarray(ml)[:, None]
    assert abs(np.abs(g[live]).min() - float(gold["margin"][0])) <= 1e-5
    # and the deviation of a run with the operands rounded to bf16 at the engine's storage points (CPU)
    got = DI.infer(p, cfg, text, lengths, seed, store=torch.bfloat16)
    assert got[1].tolist() == ml
    dev = float(np.abs(got[3].numpy() - g)[live].max())
    print("gate margin %.4f, bf16 gate deviation %.5f (fixture %.5f)" % (float(gold["margin"][0]), dev, float(gold["bf16_deviation"][0])))
    assert 10.0 * dev <= float(gold["margin"][0])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_statement_reproduces_the_reference_fixture_at_fp32(tag, capsys):
    cfg, p, gold, text, lengths, seed = _case()
    post, ml, al, gate = DI.infer(p, cfg, text, lengths, seed, max_decoder_steps=_max_steps(gold, tag))
    assert post.shape == gold[tag + "_mel_post"].shape and ml.dtype == torch.int32
    assert ml.tolist() == gold[tag + "_mel_lengths"].tolist()
    for got, name in ((post, "_mel_post"), (al, "_alignments"), (gate, "_gate")):
        print("statement fp32 vs reference %s%s: max abs %.3e" % (tag, name, float(np.abs(got.numpy() - gold[tag + name]).max())))
        np.testing.assert_allclose(got.numpy(), gold[tag + name], rtol=1e-5, atol=1e-5)


def _synth(monkeypatch, cfg, p, **kw):
    from deeplearningexamples_amd.tacotron2.infer import Tacotron2Synthesizer
    from deeplearningexamples_amd.tacotron2.model import Tacotron2
    DI.install(monkeypatch)
    model = Tacotron2(**cfg)
    model.load_reference_state(p)
    return Tacotron2Synthesizer(model, compute_dtype=torch.float32, graph=False, **kw)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_synthesizer_sequence_reproduces_the_fixture_for_every_chunk_size(monkeypatch, tag, fused, capsys):
    """Tacotron2Synthesizer's own host code (operands, alternating buffers, step words, staging, truncation) over fp32 doubles."""
    cfg, p, gold, text, lengths, seed = _case()
    outs = {}
    for chunk in (2, 8):
        s = _synth(monkeypatch, cfg, p, seed=seed, chunk=chunk, max_decoder_steps=_max_steps(gold, tag), fused_tail=fused)
        post, ml, al = s.infer(text, lengths)
        outs[chunk] = (post, ml, al, s.gate_outputs)
        assert post.dtype == torch.float32 and ml.dtype == torch.int32 and len(s._buffers) == 1
        assert post.shape == gold[tag + "_mel_post"].shape and ml.tolist() == gold[tag + "_mel_lengths"].tolist()
        for got, name in ((post, "_mel_post"), (al, "_alignments"), (s.gate_outputs, "_gate")):
            np.testing.assert_allclose(got.numpy(), gold[tag + name], rtol=1e-5, atol=1e-5)
        again = s.infer(text, lengths)                          # the buffers of the shape are reused and fully reset
        assert torch.equal(again[0], post) and torch.equal(again[1], ml) and torch.equal(again[2], al)
    for a, b in zip(outs[2], outs[8]):
        assert torch.equal(a, b)                                # the result does not depend on the chunk size
    if tag == "b":
        assert "Warning! Reached max decoder steps" in capsys.readouterr().out
    else:
        assert "Reached max" not in capsys.readouterr().out
    stat = DI.infer(p, cfg, text, lengths, seed, max_decoder_steps=_max_steps(gold, tag))
    np.testing.assert_allclose(outs[8][0].numpy(), stat[0].numpy(), rtol=1e-5, atol=1e-5)


def test_synthesizer_seed_selects_the_stream_and_no_early_stopping_runs_to_the_limit(monkeypatch):
    cfg, p, gold, text, lengths, seed = _case()
    a = _synth(monkeypatch, cfg, p, seed=seed, max_decoder_steps=16, early_stopping=False).infer(text, lengths)
    b = _synth(monkeypatch, cfg, p, seed=seed + 1, max_decoder_steps=16, early_stopping=False).infer(text, lengths)
    assert a[0].shape == b[0].shape == (3, 80, 16) and not torch.equal(a[0], b[0])
    assert a[1].tolist() == gold["a_mel_lengths"].tolist()      # the bookkeeping goes on after everything has stopped
    stat = DI.infer(p, cfg, text, lengths, seed, max_decoder_steps=16, early_stopping=False)
    np.testing.assert_allclose(a[0].numpy(), stat[0].numpy(), rtol=1e-5, atol=1e-5)
    assert stat[1].tolist() == a[1].tolist()
    with pytest.raises(ValueError):
        _synth(monkeypatch, cfg, p, chunk=3)
    with pytest.raises(ValueError):
        _synth(monkeypatch, cfg, p).infer(torch.zeros(9, 4, dtype=torch.int64), torch.full((9,), 4))


def test_mask_contract_against_the_philox_oracle():
    """Step t, layer l over the row-major [B, P] block = keep_mask(B * P, 0.5, seed, 1 + 2 t + l); kept values x inv_keep(0.5) = 2."""
    from oracle import philox_oracle as PO
    from tests import _tacotron2_doubles as D
    assert float(PO.inv_keep(0.5)) == 2.0 and D.inv_keep(0.5) == 2.0
    b, p, nm, seed = 3, 48, 80, 99
    g = torch.Generator().manual_seed(0)
    w0, w1 = torch.randn(p, nm, generator=g), torch.randn(p, p, generator=g)
    frame = torch.randn(b, nm, generator=g)
    seen = []
    for t in (0, 1, 7):
        m0, m1 = torch.zeros(b * p // 8, dtype=torch.uint8), torch.zeros(b * p // 8, dtype=torch.uint8)
        dst = torch.zeros(b, p)
        DI.prenet_infer(frame, w0, w1, dst, seed, torch.tensor([t, 0]), m0, m1)
        for layer, m in enumerate((m0, m1)):
            want = PO.keep_mask(b * p, 0.5, seed, 1 + 2 * t + layer)
            assert np.array_equal(D.unpack_dropout_mask(m, (b * p,)).numpy(), want)
            seen.append(want.tobytes())
        k0 = torch.from_numpy(PO.keep_mask(b * p, 0.5, seed, 1 + 2 * t)).view(b, p)
        k1 = torch.from_numpy(PO.keep_mask(b * p, 0.5, seed, 2 + 2 * t)).view(b, p)
        want = torch.relu((torch.relu(frame @ w0.t()) * k0 * 2.0) @ w1.t()) * k1 * 2.0
        np.testing.assert_allclose(dst.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert len(set(seen)) == 6                                  # every (step, layer) draws its own mask
    assert not np.array_equal(PO.keep_mask(b * p, 0.5, seed + 1, 1), PO.keep_mask(b * p, 0.5, seed, 1))


def test_frame_double_bookkeeping_follows_the_reference_loop():
    """not_finished / mel_lengths / n_steps over a scripted logit sequence, against the loop of model.py:578-585."""
    b, nm, k, steps = 3, 8, 16, 12
    logits = torch.tensor([[-1.0, -1.0, 0.0, 2.0, -3.0, -3.0], [-1.0, 0.5, -2.0, -2.0, -2.0, -2.0], [-2.0, -2.0, -2.0, -2.0, 0.0, 1e-3]]).t()
    w = torch.zeros(nm + 1, k)
    hc = torch.zeros(b, k)
    mel, gate, frame = torch.zeros(b, steps, nm), torch.zeros(b, steps), torch.zeros(b, nm)
    nf, ml, state = torch.ones(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    ref_nf, ref_ml, ref_n = torch.ones(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), None
    for t in range(logits.shape[0]):
        bias = torch.zeros(nm + 1)
        for i in range(b):                                     # one bias per launch cannot script per-sample logits: use hc
            hc[i, 0] = logits[t, i]
        w[nm, 0] = 1.0
        DI.frame_infer(hc, w, bias, mel, gate, frame, nf, ml, state, t & 1, 0.5, steps)
        dec = (torch.sigmoid(logits[t]) <= 0.5).to(torch.int32)
        ref_nf = ref_nf * dec
        ref_ml = ref_ml + ref_nf
        if ref_n is None and int(ref_nf.sum()) == 0:
            ref_n = t + 1
        assert nf.tolist() == ref_nf.tolist() and ml.tolist() == ref_ml.tolist() and int(state[1 - (t & 1)]) == t + 1
    assert ref_n == 6 and int(state[2]) == 6 and int(state[3]) == 1 and ml.tolist() == [3, 1, 5]
    assert torch.equal(gate[:, :6], logits.t())


def test_command_line_parses_the_reference_flags():
    from deeplearningexamples_amd.tacotron2 import inference as I
    a = I.parse_args(["-i", "p.txt", "-o", "out", "--suffix", "_x", "--tacotron2", "t.pt", "--waveglow", "w.pt", "-s", "0.8", "-d", "0.05",
                      "-sr", "16000", "--fp16", "--log-file", "l.json", "--include-warmup", "--stft-hop-length", "256",
                      "--amp-dtype", "fp16", "--seed", "5"])
    assert (a.input, a.output, a.suffix, a.tacotron2, a.waveglow, a.sigma_infer, a.denoising_strength, a.sampling_rate, a.fp16,
            a.log_file, a.include_warmup, a.stft_hop_length, a.amp_dtype, a.seed) == (
                "p.txt", "out", "_x", "t.pt", "w.pt", 0.8, 0.05, 16000, True, "l.json", True, 256, "fp16", 5)
    I.check_args(a)
    d = I.parse_args(["-i", "p.txt", "-o", "out", "--tacotron2", "t.pt"])
    assert (d.sigma_infer, d.denoising_strength, d.sampling_rate, d.log_file, d.waveglow, d.seed) == (0.9, 0.01, 22050, "nvlog.json", None, 1234)
    I.check_args(d)                                             # no --waveglow: the mel tensors are saved
    for bad, word in ((["--cpu"], "MI355X"), (["--fp16", "--amp-dtype", "bf16"], "contradict"), (["--stft-hop-length", "128"], "256")):
        with pytest.raises(SystemExit) as e:
            I.check_args(I.parse_args(["-i", "p.txt", "-o", "out", "--tacotron2", "t.pt"] + bad))
        assert word in str(e.value)
    with pytest.raises(SystemExit):
        I.check_args(I.parse_args(["-i", "p.txt", "-o", "out"]))
    with pytest.raises(SystemExit):
        I.parse_args(["-o", "out", "--tacotron2", "t.pt"])     # -i is required, as in the reference
    # the reference's own flag names (tests/golden/reference_interfaces.json holds its inference.py parser when recorded)
    src = open(os.path.join(ROOT, "deeplearningexamples_amd", "tacotron2", "inference.py")).read()
    for flag in ("-i", "--input", "-o", "--output", "--suffix", "--tacotron2", "--waveglow", "-s", "--sigma-infer", "-d",
                 "--denoising-strength", "-sr", "--sampling-rate", "--fp16", "--cpu", "--log-file", "--include-warmup",
                 "--stft-hop-length"):
        assert '"%s"' % flag in src, flag


def test_input_sequences_are_sorted_and_padded_like_the_reference(tmp_path):
    from deeplearningexamples_amd.tacotron2 import inference as I
    from deeplearningexamples_amd.tacotron2.text import text_to_sequence
    f = tmp_path / "phrases.txt"
    f.write_text("Hello there.\nThe quick brown fox jumps over the lazy dog.\n\nYes.\n")
    texts = I.read_phrases(str(f))
    assert len(texts) == 3
    text, lengths = I.prepare_input_sequence(texts)
    seqs = sorted((text_to_sequence(t, ["english_cleaners"]) for t in texts), key=len, reverse=True)
    assert lengths.tolist() == [len(s) for s in seqs] and text.shape == (3, len(seqs[0])) and text.dtype == torch.int64
    for row, s in zip(text, seqs):
        assert row[:len(s)].tolist() == s and int(row[len(s):].abs().sum()) == 0


def test_waveglow_entry_point_still_rejects_text_input():
    from deeplearningexamples_amd.waveglow import inference as WI
    with pytest.raises(SystemExit) as e:
        WI._reject_unbuilt(WI.parse_args(["--waveglow", "c", "--synth-data", "-o", "out", "-i", "p.txt"]))
    assert "Tacotron2" in str(e.value) and "tacotron2.inference" in str(e.value)


def test_new_symbols_in_header_library_and_ctypes_table():
    import __graft_entry__ as ge
    ge.build()
    from deeplearningexamples_amd import _cabi
    src = open(os.path.join(ROOT, "include", "dle_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(h, name), "library does not export %s" % name
        assert name in _cabi.declared_symbols()
    assert _cabi.lib().dle_abi_version() == 1
