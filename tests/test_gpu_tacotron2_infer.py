"""Tacotron2 inference on the MI355X: dle_t2_prenet_infer / dle_t2_frame_infer against their plain-torch statements
(tests/_tacotron2_infer_doubles.py) and the mask contract, Tacotron2Synthesizer against the fixture the REFERENCE's own
Tacotron2.infer produced (tests/golden/tacotron2_infer.npz), graph replay against eager launches, chunk sizes, seeds, the
default-width network, memory, and the text-to-speech command line.

Bars of the whole-network checks follow tests/test_gpu_waveglow_infer.py: the FLOOR is what 16-bit storage alone costs, measured
here (and printed) with the CPU statement rounding at the engine's storage points against the fp32 reference; the engine gets
MARGIN = 4 x that floor, separately for fp16 and bf16 -- its result is another realisation of the same roundings (fp32
accumulation order, other tanh / exp), and the free-running recurrence feeds every such difference back.  The stop steps are
exact: that is what the fixture's gate margin is for.  Nothing here is taken from the kernels' own output.
"""
import os
import wave

import numpy as np
import pytest
import torch

from oracle import philox_oracle as PO
from tests import _tacotron2_doubles as D
from tests import _tacotron2_infer_doubles as DI

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.float16, torch.bfloat16]
MARGIN = 4.0


def _tol(dtype):                                          # the 16-bit tolerances of tests/test_gpu_tacotron2.py
    return dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=1.6e-2, atol=1.6e-2)


def _close(got, ref, **kw):
    np.testing.assert_allclose(got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy(), **kw)


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [32, 256])
@pytest.mark.parametrize("b", [1, 3, 8])
def test_prenet_infer_masks_and_values(cuda, b, p, dtype):
    from deeplearningexamples_amd.tacotron2 import ops
    nm, seed = 80, 4321 + b
    g = torch.Generator().manual_seed(b * 1000 + p)
    w0 = (torch.randn(p, nm, generator=g) / nm ** 0.5).to(dtype)
    w1 = (torch.randn(p, p, generator=g) / p ** 0.5).to(dtype)
    frame = torch.randn(b, nm, generator=g) * 2.0
    for t in (0, 1, 6, 1999):
        state = torch.tensor([t, t + 100, 0, 0], dtype=torch.int64)
        buf = torch.full((b, p + 40), 7.0, dtype=dtype, device=cuda)                        # row-strided destination, as x_a is
        m0 = torch.zeros(b * p // 8, dtype=torch.uint8, device=cuda)
        m1 = torch.zeros_like(m0)
        ops.prenet_infer(None if t == 0 else frame.to(cuda), w0.to(cuda), w1.to(cuda), buf[:, :p], seed, state.to(cuda), m0, m1)
        for layer, m in enumerate((m0, m1)):
            want = PO.keep_mask(b * p, 0.5, seed, 1 + 2 * t + layer)
            assert np.array_equal(D.unpack_dropout_mask(m.cpu(), (b * p,)).numpy(), want), (t, layer)
        ref = torch.zeros(b, p, dtype=dtype)
        DI.prenet_infer(None if t == 0 else frame, w0, w1, ref, seed, state)
        _close(buf[:, :p], ref, **_tol(dtype))
        assert float((buf[:, p:].float() - 7.0).abs().max()) == 0                           # nothing outside the prenet columns
        if t == 0:
            assert float(buf[:, :p].float().abs().max()) == 0                               # the go frame: relu(0 W) = 0
    # the odd step word is the one an odd step reads
    state = torch.tensor([5, 9, 0, 0], dtype=torch.int64, device=cuda)
    m0 = torch.zeros(b * p // 8, dtype=torch.uint8, device=cuda)
    out = torch.zeros(b, p, dtype=dtype, device=cuda)
    ops.prenet_infer(frame.to(cuda), w0.to(cuda), w1.to(cuda), out, seed, state[1:], m0)
    assert np.array_equal(D.unpack_dropout_mask(m0.cpu(), (b * p,)).numpy(), PO.keep_mask(b * p, 0.5, seed, 1 + 2 * 9))


def _frame_buffers(cuda, b, nm, steps):
    return dict(mel=torch.zeros(b, steps, nm, device=cuda), gate=torch.zeros(b, steps, device=cuda), frame=torch.zeros(b, nm, device=cuda),
                nf=torch.ones(b, dtype=torch.int32, device=cuda), ml=torch.zeros(b, dtype=torch.int32, device=cuda),
                state=torch.zeros(4, dtype=torch.int64, device=cuda))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("b,k", [(1, 160), (3, 160), (8, 1536)])
def test_frame_infer_values(cuda, b, k, fused, dtype):
    from deeplearningexamples_amd.tacotron2 import ops
    nm, steps, p, seed = 80, 6, 48, 77
    g = torch.Generator().manual_seed(b + k)
    hc = torch.randn(b, k, generator=g).to(dtype)
    w = (torch.randn(88, k, generator=g) / k ** 0.5).to(dtype)
    bias = torch.randn(88, generator=g) * 0.1
    w0 = (torch.randn(p, nm, generator=g) / nm ** 0.5).to(dtype)
    w1 = (torch.randn(p, p, generator=g) / p ** 0.5).to(dtype)
    dev, ref = _frame_buffers(cuda, b, nm, steps), _frame_buffers("cpu", b, nm, steps)
    dst_d, dst_r = torch.zeros(b, p, dtype=dtype, device=cuda), torch.zeros(b, p, dtype=dtype)
    for t in range(steps + 2):                                                              # two steps past the limit: counted, not stored
        par = t & 1
        for bufs, to, dst in ((dev, lambda x: x.to(cuda), dst_d), (ref, lambda x: x, dst_r)):
            fn = ops.frame_infer if bufs is dev else DI.frame_infer
            fn(to(hc), to(w), to(bias), bufs["mel"], bufs["gate"], bufs["frame"], bufs["nf"], bufs["ml"], bufs["state"], par, 0.5, steps,
               prenet=(to(w0), to(w1), dst) if fused else None, seed=seed)
        assert dev["state"].cpu().tolist() == ref["state"].tolist()
        if fused:
            _close(dst_d, dst_r, **_tol(dtype))
    # fp32 outputs of 16-bit operands: the accumulation order is the only difference
    _close(dev["mel"], ref["mel"], rtol=1e-4, atol=1e-4)
    _close(dev["gate"], ref["gate"], rtol=1e-4, atol=1e-4)
    _close(dev["frame"], ref["frame"], rtol=1e-4, atol=1e-4)
    assert dev["nf"].cpu().tolist() == ref["nf"].tolist() and dev["ml"].cpu().tolist() == ref["ml"].tolist()


@pytest.mark.parametrize("fused", [False, True])
def test_frame_infer_stop_bookkeeping_is_exact(cuda, fused):
    """Scripted gate logits (weight row = e_0, hc[:, 0] = the logit, exactly representable in fp16), with logits exactly at the
    threshold (sigmoid(0) = 0.5 <= 0.5: not a stop) and the all-finished-at-step-1 case."""
    from deeplearningexamples_amd.tacotron2 import ops
    nm, k, steps, p = 8, 16, 16, 8
    scripts = {"mixed": [[-1.0, -1.0, 0.0], [-1.0, 0.5, -2.0], [0.0, -2.0, -2.0], [2.0, -2.0, -2.0], [-3.0, -2.0, 0.0], [-3.0, -2.0, 0.25],
                         [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]],
               "all_at_step_1": [[1.0, 0.5, 3.0], [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0], [-1.0, -1.0, -1.0]],
               "never": [[0.0, -1.0, -0.5]] * 6}
    w = torch.zeros(nm + 1, k, dtype=torch.float16)
    w[nm, 0] = 1.0
    w0, w1 = torch.zeros(p, nm, dtype=torch.float16, device=cuda), torch.zeros(p, p, dtype=torch.float16, device=cuda)
    for name, logits in scripts.items():
        b = 3
        bufs = _frame_buffers(cuda, b, nm, steps)
        dst = torch.zeros(b, p, dtype=torch.float16, device=cuda)
        ref_nf, ref_ml, ref_n = torch.ones(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), None
        for t, row in enumerate(logits):
            hc = torch.zeros(b, k, dtype=torch.float16)
            hc[:, 0] = torch.tensor(row)
            ops.frame_infer(hc.to(cuda), w.to(cuda), torch.zeros(nm + 1, device=cuda), bufs["mel"], bufs["gate"], bufs["frame"], bufs["nf"],
                            bufs["ml"], bufs["state"], t & 1, 0.5, steps, prenet=(w0, w1, dst) if fused else None)
            dec = (torch.sigmoid(torch.tensor(row)) <= 0.5).to(torch.int32)                 # model.py:578-582
            ref_nf = ref_nf * dec
            ref_ml = ref_ml + ref_nf
            if ref_n is None and int(ref_nf.sum()) == 0:
                ref_n = t + 1
            st = bufs["state"].cpu().tolist()
            assert bufs["nf"].cpu().tolist() == ref_nf.tolist() and bufs["ml"].cpu().tolist() == ref_ml.tolist(), (name, t)
            assert st[1 - (t & 1)] == t + 1 and st[2] == (ref_n if ref_n is not None else t + 1) and st[3] == int(ref_n is not None)
        assert torch.equal(bufs["gate"][:, :len(logits)].cpu(), torch.tensor(logits).t())
        assert {"mixed": 6, "all_at_step_1": 1, "never": None}[name] == ref_n


# ------------------------------------------------------------------------------------------------- the network
def _case():
    from oracle import tacotron2_oracle as TO
    gold = np.load(os.path.join(HERE, "golden", "tacotron2_infer.npz"))
    cfg = TO.TACOTRON2_SMALL
    p = DI.full_state(cfg, int(gold["model_seed"][0]), int(gold["gate_seed"][0]), float(gold["gate_scale"][0]), float(gold["gate_bias"][0]))
    return cfg, p, gold, torch.from_numpy(gold["text"]), torch.from_numpy(gold["text_lengths"]), int(gold["seed"][0])


def _synth(cuda, cfg, state, dtype, **kw):
    from deeplearningexamples_amd.tacotron2.infer import Tacotron2Synthesizer
    from deeplearningexamples_amd.tacotron2.model import Tacotron2
    model = Tacotron2(**cfg, device=cuda)
    model.load_reference_state(state)
    return Tacotron2Synthesizer(model, compute_dtype=dtype, **kw)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_infer_vs_reference_fixture(cuda, dtype, tag):
    cfg, p, gold, text, lengths, seed = _case()
    max_steps = 2000 if tag == "a" else int(gold["b_max_decoder_steps"][0])
    floor = DI.infer(p, cfg, text, lengths, seed, max_decoder_steps=max_steps, store=dtype)
    assert floor[1].tolist() == gold[tag + "_mel_lengths"].tolist()
    s = _synth(cuda, cfg, p, dtype, seed=seed, max_decoder_steps=max_steps)
    post, ml, al = s.infer(text.to(cuda), lengths.to(cuda))
    assert post.dtype == torch.float32 and ml.dtype == torch.int32 and bool(torch.isfinite(post).all())
    assert ml.cpu().tolist() == gold[tag + "_mel_lengths"].tolist() and post.shape == gold[tag + "_mel_post"].shape      # exact
    assert al.shape == gold[tag + "_alignments"].shape and s.gate_outputs.shape == gold[tag + "_gate"].shape
    for got, fl, name in ((post, floor[0], "_mel_post"), (al, floor[2], "_alignments")):
        f, err = _rel(fl, gold[tag + name]), _rel(got, gold[tag + name])
        print("infer %s case %s %s: rel L2 %.3e, 16-bit storage floor %.3e, bar %.3e" % (dtype, tag, name, err, f, MARGIN * f))
        assert err <= MARGIN * f, (name, err, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_eager_chunk_and_seed(cuda, dtype):
    """Graph replay against eager launches, chunk 2 against the default, one launch against two for the tail: the same bits.  Two
    calls with one seed: the same bits; another seed: another spectrogram."""
    cfg, p, gold, text, lengths, seed = _case()
    text, lengths = text.to(cuda), lengths.to(cuda)

    def run(**kw):
        s = _synth(cuda, cfg, p, dtype, seed=kw.pop("seed", seed), **kw)
        out = s.infer(text, lengths)
        return s, out + (s.gate_outputs,)
    s0, base = run()
    for kw in (dict(graph=False), dict(chunk=2), dict(chunk=2, graph=False), dict(fused_tail=True), dict(fused_tail=True, graph=False)):
        _, other = run(**kw)
        for a, b in zip(base, other):
            assert torch.equal(a, b), kw
    again = s0.infer(text, lengths)                                                         # replays the captured graph again
    assert all(torch.equal(a, b) for a, b in zip(base[:3], again)) and len(s0._buffers) == 1
    _, other = run(seed=seed + 1, max_decoder_steps=12, early_stopping=False)
    _, same = run(max_decoder_steps=12, early_stopping=False)
    assert other[0].shape == same[0].shape and not torch.equal(other[0], same[0])


def _default_case(b):
    from oracle import tacotron2_oracle as TO
    cfg = TO.TACOTRON2_DEFAULT
    rng = np.random.default_rng(300 + b)
    lens = sorted(rng.integers(96, 129, b).tolist(), reverse=True)
    lens[0] = 128
    text = np.zeros((b, 128), np.int64)
    for i, n in enumerate(lens):
        text[i, :n] = rng.integers(1, cfg["n_symbols"], n)
    return cfg, DI.full_state(cfg, 23), torch.from_numpy(text), torch.tensor(lens, dtype=torch.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b", [1, 8])
def test_default_widths_vs_statement(cuda, b, dtype):
    """Default widths, 128 symbols, 64 forced steps: the synthesizer against the fp32 statement under the same masks; the floor
    is the statement with 16-bit storage against the same fp32 run."""
    cfg, p, text, lengths = _default_case(b)
    want = DI.infer(p, cfg, text, lengths, 5, max_decoder_steps=64, early_stopping=False)
    floor = DI.infer(p, cfg, text, lengths, 5, max_decoder_steps=64, early_stopping=False, store=dtype)
    s = _synth(cuda, cfg, p, dtype, seed=5, max_decoder_steps=64, early_stopping=False)
    post, ml, al = s.infer(text.to(cuda), lengths.to(cuda))
    assert post.shape == (b, 80, 64) and al.shape == (b, 64, 128) and bool(torch.isfinite(post).all())
    for got, fl, ref, name in ((post, floor[0], want[0], "mel"), (al, floor[2], want[2], "alignments")):
        f, err = _rel(fl, ref), _rel(got, ref)
        print("default widths b %d %s %s: rel L2 %.3e, 16-bit storage floor %.3e, bar %.3e" % (b, dtype, name, err, f, MARGIN * f))
        assert err <= MARGIN * f, (name, err, f)


def _memory_of_first_call(cuda, steps):
    cfg, p, text, lengths = _default_case(1)
    s = _synth(cuda, cfg, p, torch.float16, max_decoder_steps=steps, early_stopping=False)
    text, lengths = text.to(cuda), lengths.to(cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = s.infer(text, lengths)
    torch.cuda.synchronize()
    assert out[0].shape == (1, 80, steps)
    del out
    held = torch.cuda.memory_allocated() - base
    peak = torch.cuda.max_memory_allocated() - base
    s.gate_outputs = None
    before = torch.cuda.memory_allocated()
    s.infer(text, lengths)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before + 4 * steps + 1024, "the second call at the same shape kept more memory"
    return held, peak


def test_memory_grows_only_with_the_outputs(cuda):
    """64 against 512 steps: what the synthesizer holds differs by its output buffers (mel, gate logits, alignments: fp32 rows of
    n_mel + 1 + Ti values per step) and nothing else; the transient peak above that is the postnet over T frames."""
    (h64, p64), (h512, p512) = _memory_of_first_call(cuda, 64), _memory_of_first_call(cuda, 512)
    outputs = (512 - 64) * (80 + 1 + 128) * 4
    print("held bytes: 64 steps %d, 512 steps %d (outputs differ by %d); peaks %d / %d" % (h64, h512, outputs, p64, p512))
    assert abs((h512 - h64) - outputs) <= 64 * 1024, (h64, h512, outputs)
    # postnet transients per frame: 5-tap rows of 512 channels + four 512-channel activations, 16-bit, + the fp32 copies
    assert (p512 - h512) - (p64 - h64) <= (512 - 64) * 12 * 1024, (p64, p512)


def test_command_line_text_to_speech(cuda, tmp_path):
    """Seeded checkpoints as the train entry points write them -> phrases -> wav files of mel_lengths * 256 samples."""
    from oracle import waveglow_oracle as WO
    from deeplearningexamples_amd.tacotron2 import inference as I
    from deeplearningexamples_amd.tacotron2.engine import Tacotron2Trainer
    from deeplearningexamples_amd.tacotron2.model import Tacotron2
    from deeplearningexamples_amd.waveglow import train as WT
    from deeplearningexamples_amd.waveglow.engine import WaveGlowTrainer
    from deeplearningexamples_amd.waveglow.model import WaveGlow
    cfg, p, gold, _, _, _ = _case()
    t2 = Tacotron2(**cfg, device=cuda)
    t2.load_reference_state(p)
    t2_cfg = dict(cfg, mask_padding=False, max_decoder_steps=24, gate_threshold=0.5, decoder_no_early_stopping=False)
    from deeplearningexamples_amd.tacotron2.train import parameter_order
    t2_ckpt = WT.save_checkpoint(Tacotron2Trainer(t2), 0, t2_cfg, str(tmp_path), "Tacotron2", 0, 1, parameter_order(cfg))
    wg = WaveGlow(**WO.WAVEGLOW_SMALL, device=cuda)
    wg.load_reference_state(WO.seeded_state(WO.WAVEGLOW_SMALL, 7))
    wg_ckpt = WT.save_checkpoint(WaveGlowTrainer(wg, compute_dtype=torch.float16), 0, WO.WAVEGLOW_SMALL, str(tmp_path), "WaveGlow", 0, 1)
    phrases = tmp_path / "phrases.txt"
    phrases.write_text("Hello there.\nThe quick brown fox jumps over the lazy dog.\nYes indeed.\n")
    out = str(tmp_path / "audio")
    mel, ml, audio = I.main(["-i", str(phrases), "--tacotron2", t2_ckpt, "--waveglow", wg_ckpt, "-o", out, "--fp16", "-sr", "16000"])
    assert mel.shape[0] == 3 and mel.shape[1] == 80 and 1 <= mel.shape[2] <= 24 and audio.shape == (3, mel.shape[2] * 256)
    assert bool(torch.isfinite(audio).all())
    for i, n in enumerate(ml.cpu().tolist()):
        with wave.open(os.path.join(out, "audio_%d.wav" % i), "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, n * 256)
    log = open(os.path.join(out, "nvlog.json")).read()
    for key in ("tacotron2_items_per_sec", "tacotron2_latency", "waveglow_items_per_sec", "waveglow_latency", "denoiser_latency", "latency"):
        assert key in log, key
    # without a vocoder the mel tensors are saved, trimmed to their lengths; the same seed gives the same spectrogram
    out2 = str(tmp_path / "mels")
    mel2, ml2, none = I.main(["-i", str(phrases), "--tacotron2", t2_ckpt, "-o", out2, "--suffix", "_m"])
    assert none is None and torch.equal(mel2, mel) and torch.equal(ml2, ml)
    for i, n in enumerate(ml2.cpu().tolist()):
        assert torch.load(os.path.join(out2, "mel_%d_m.pt" % i)).shape == (80, n)
