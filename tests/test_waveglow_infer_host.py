"""WaveGlow inference on the CPU: the plain-torch statement of infer (tests/_waveglow_infer_doubles.py) against the fixture the
REFERENCE's own WaveGlow.infer and Denoiser produced (tests/golden/waveglow_infer.npz, tools/make_waveglow_infer_golden.py),
the round trip through the oracle's forward flow, the host sequencing of WaveGlowVocoder with the C-ABI calls replaced by the
doubles, the Denoiser restatement and the command line.  The kernels are checked on the GPU (tests/test_gpu_waveglow_infer.py).
"""
import os

import numpy as np
import pytest
import torch

from tests import _waveglow_infer_doubles as DI

HERE = os.path.dirname(os.path.abspath(__file__))


def _case():
    from oracle import waveglow_oracle as WO
    gold = np.load(os.path.join(HERE, "golden", "waveglow_infer.npz"))
    cfg = WO.WAVEGLOW_SMALL
    return WO, cfg, WO.seeded_state(cfg, 7), gold, torch.from_numpy(gold["mel"]), torch.from_numpy(gold["z"])


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("tag,sigma", [("s09", 0.9), ("s0", 0.0)])
def test_double_reproduces_the_reference_fixture_at_fp32(tag, sigma):
    WO, cfg, p, gold, mel, z = _case()
    want = torch.from_numpy(gold["audio_" + tag])
    got = DI.infer(p, cfg, mel, z, sigma, work=torch.float32)
    assert got.shape == want.shape == (2, 8 * 256)        # `frames` row blocks of the upsampling = the reference after its trim
    print("double fp32 vs reference, sigma %s: rel L2 %.3e, max abs %.3e" % (sigma, _rel(got, want), float((got - want).abs().max())))
    # measured: rel L2 3.5e-7 (both sigmas), max abs 4.8e-6 at |audio| <= 10 (sigma 0.9), 3.3e-7 at |audio| <= 0.63 (sigma 0):
    # fp32 summation order and (a - b) * exp(-s) for (a - b) / exp(s); the bar is the 1e-5 class of fp32 with that headroom
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert _rel(got, want) <= 5e-6


def _oracle_forward_z(WO, p, cfg, mel, audio):
    """WaveGlow.forward's flow (model.py:196-232) on the oracle's WN: -> z in the forward's channel order."""
    import torch.nn.functional as TF
    ng, wn = cfg["n_group"], cfg["WN_config"]
    spect = TF.conv_transpose1d(mel, p["upsample.weight"], p["upsample.bias"], stride=256)[:, :, :audio.size(1)]
    spect = spect.unfold(2, ng, ng).permute(0, 2, 1, 3)
    spect = spect.contiguous().view(spect.size(0), spect.size(1), -1).permute(0, 2, 1)
    a, outs = audio.unfold(1, ng, ng).permute(0, 2, 1), []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            outs.append(a[:, :cfg["n_early_size"]])
            a = a[:, cfg["n_early_size"]:]
        a = TF.conv1d(a, p["convinv.%d.conv.weight" % k])
        nh = a.size(1) // 2
        o = WO.wn_forward(p, "WN.%d." % k, a[:, :nh], spect, wn["n_layers"], wn["n_channels"], wn["kernel_size"])
        a = torch.cat([a[:, :nh], torch.exp(o[:, nh:]) * a[:, nh:] + o[:, :nh]], 1)
    outs.append(a)
    return torch.cat(outs, 1)


def test_infer_then_the_oracles_forward_flow_returns_z():
    WO, cfg, p, gold, mel, z = _case()
    audio = DI.infer(p, cfg, mel, z, 0.9, work=torch.float32)
    back = _oracle_forward_z(WO, p, cfg, mel, audio)
    want = DI.noise_in_forward_order(z, cfg, 0.9)
    print("round trip fp32: rel L2 %.3e" % _rel(back, want))
    assert _rel(back, want) <= 1e-5                       # measured 3.7e-7: two fp32 passes through 4 couplings
    # and the doubles' own forward statement is that flow
    assert _rel(DI.forward_z(p, cfg, mel, audio, work=torch.float32), back) <= 1e-5


def _install(monkeypatch):
    """The doubles for every C-ABI call WaveGlowVocoder makes (the train step's + the three inference wrappers)."""
    from tests import _waveglow_doubles as D
    from deeplearningexamples_amd.waveglow import ops
    D.install(monkeypatch)

    def flow_inv_first(noise, c, sigma, out, a0):
        s, a = DI.flow_inv_first(noise, c, sigma, a0.dtype)
        out.copy_(s)
        a0.copy_(a)
        return out, a0

    def flow_inv(state, o, winv_t, c, out=None, a0=None, next_c=0, early=0, noise=None, z_col=0, sigma=1.0):
        s, a = DI.flow_inv(state, o, winv_t, c, next_c if a0 is not None else 0, early, noise, z_col, sigma,
                           a0.dtype if a0 is not None else torch.float16)
        out.copy_(s)
        if a0 is not None:
            a0.copy_(a)
        return out, a0

    def mel_rows(mel, out):
        out.copy_(mel.permute(0, 2, 1).reshape(out.shape))
        return out
    for name, fn in (("flow_inv_first", flow_inv_first), ("flow_inv", flow_inv), ("mel_rows", mel_rows)):
        monkeypatch.setattr(ops, name, fn)


@pytest.mark.parametrize("tag,sigma", [("s09", 0.9), ("s0", 0.0)])
def test_vocoder_sequence_reproduces_the_reference_fixture(monkeypatch, tag, sigma):
    """WaveGlowVocoder's own host code (weight tables, per-flow cond slices, buffers, noise columns) over fp32 doubles."""
    from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
    from deeplearningexamples_amd.waveglow.model import WaveGlow
    WO, cfg, p, gold, mel, z = _case()
    _install(monkeypatch)
    model = WaveGlow(**cfg)
    model.load_reference_state(p)
    voc = WaveGlowVocoder(model, compute_dtype=torch.float32)
    want = torch.from_numpy(gold["audio_" + tag])
    got = voc.infer(mel, sigma=sigma, z=z)
    assert got.shape == want.shape and got.dtype == torch.float32
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    again = voc.infer(mel, sigma=sigma, z=z)              # the cached buffers of the shape are reused and fully rewritten
    assert again.data_ptr() == got.data_ptr() and len(voc._buffers) == 1
    np.testing.assert_allclose(again.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)


def test_vocoder_refresh_follows_new_weights(monkeypatch):
    from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
    from deeplearningexamples_amd.waveglow.model import WaveGlow
    WO, cfg, p, gold, mel, z = _case()
    _install(monkeypatch)
    torch.manual_seed(1)
    model = WaveGlow(**cfg)                               # fresh: end = 0, every coupling is the identity
    voc = WaveGlowVocoder(model, compute_dtype=torch.float32)
    model.load_reference_state(p)
    voc.refresh()
    np.testing.assert_allclose(voc.infer(mel, sigma=0.9, z=z).numpy(), gold["audio_s09"], rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        voc.infer(mel, sigma=0.9, z=z[:, :, :-1])


def test_twelve_flow_noise_columns_follow_infer_onnx():
    """Default network: 4 initial channels, then the draw used at k = 8, then the one used at k = 4."""
    from deeplearningexamples_amd.waveglow.model import DEFAULT_CONFIG, flow_channels
    assert DI.n_remaining(DEFAULT_CONFIG) == flow_channels(DEFAULT_CONFIG)[-1][0] == 4
    z = torch.arange(8.0).view(1, 8, 1)
    assert DI.noise_in_forward_order(z, DEFAULT_CONFIG, 1.0).flatten().tolist() == [6, 7, 4, 5, 0, 1, 2, 3]


def test_denoiser_restatement_matches_the_reference_fixture():
    from deeplearningexamples_amd.waveglow.infer import Denoiser
    WO, cfg, p, gold, mel, z = _case()

    class Vocoder:
        dev = "cpu"

        def infer(self, m, sigma=1.0):
            return DI.infer(p, cfg, m, torch.zeros(m.shape[0], 8, m.shape[2] * 32), sigma, work=torch.float32)
    d = Denoiser(Vocoder())
    assert _rel(d.bias_spec, torch.from_numpy(gold["denoiser_bias_spec"])) <= 1e-5          # measured 5.6e-7
    audio = torch.from_numpy(gold["audio_s09"])
    got = d(audio, strength=float(gold["denoiser_strength"][0]))
    want = torch.from_numpy(gold["denoised_s09"])
    assert got.shape == want.shape == (2, 1, 2048)
    print("denoiser vs reference: rel L2 %.3e, max abs %.3e" % (_rel(got, want), float((got - want).abs().max())))
    # measured: rel L2 4.3e-7, max abs 3.8e-6 at |audio| <= 10 (the pseudo-inverse basis and the window envelope are formed in
    # fp64 by another library); the denoising itself moves the audio by 1.3e-2 rel L2, far above the bar
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert _rel(audio[:, None], want) > 1e-3


def test_command_line_parses_every_flag_and_rejects_the_tacotron2_ones():
    from deeplearningexamples_amd.waveglow import inference as I
    a = I.parse_args(["--waveglow", "ckpt.pt", "--mel", "m.pt", "-o", "out", "--sigma-infer", "0.8", "--denoising-strength", "0.05",
                      "--fp16", "-sr", "16000", "--suffix", "_x", "--log-file", "l.json", "--include-warmup",
                      "--stft-hop-length", "256", "--amp-dtype", "fp16", "--seed", "5"])
    assert (a.waveglow, a.mel, a.output, a.sigma_infer, a.denoising_strength, a.fp16, a.sampling_rate, a.suffix, a.log_file,
            a.include_warmup, a.amp_dtype, a.seed) == ("ckpt.pt", "m.pt", "out", 0.8, 0.05, True, 16000, "_x", "l.json", True,
                                                       "fp16", 5)
    I._reject_unbuilt(a)
    d = I.parse_args(["--waveglow", "c", "--synth-data", "-o", "out"])
    assert (d.sigma_infer, d.denoising_strength, d.sampling_rate, d.synth_frames, d.batch_size) == (0.9, 0.01, 22050, 895, 1)
    I._reject_unbuilt(d)
    s = I.parse_args(["--waveglow", "c", "--synth-data", "-o", "out", "-s", "0.7", "-d", "0.2", "--amp-dtype", "bf16"])
    assert (s.sigma_infer, s.denoising_strength, s.amp_dtype) == (0.7, 0.2, "bf16")
    for bad, word in ((["-i", "phrases.txt"], "Tacotron2"), (["--tacotron2", "t.pt"], "Tacotron2"), (["--cpu"], "MI355X"),
                      (["--fp16", "--amp-dtype", "bf16"], "contradict")):
        with pytest.raises(SystemExit) as e:
            I._reject_unbuilt(I.parse_args(["--waveglow", "c", "--synth-data", "-o", "out"] + bad))
        assert word in str(e.value)
    with pytest.raises(SystemExit):
        I._reject_unbuilt(I.parse_args(["-o", "out", "--synth-data"]))                      # no checkpoint
    with pytest.raises(SystemExit):
        I._reject_unbuilt(I.parse_args(["-o", "out", "--waveglow", "c"]))                   # no spectrogram
    with pytest.raises(SystemExit):
        I.parse_args(["--waveglow", "c", "--synth-data", "--mel", "m.pt", "-o", "out"])     # one source only


def test_wav_writer_and_synthetic_mel(tmp_path):
    import wave
    from deeplearningexamples_amd.waveglow import inference as I
    x = np.sin(np.arange(1000) / 10.0)
    path = str(tmp_path / "a.wav")
    I.write_wav(path, x, 22050)
    with wave.open(path, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, 1000)
        pcm = np.frombuffer(f.readframes(1000), dtype="<i2")
    assert np.array_equal(pcm, np.rint(x * 32767).astype(np.int16))
    m = I.synth_mel(2, 80, 500, 3)
    assert m.shape == (2, 80, 500) and abs(float(m.mean()) + 5.62) < 0.05 and abs(float(m.std()) - 1.98) < 0.05
    assert torch.equal(m, I.synth_mel(2, 80, 500, 3))


def test_flow_inv_double_inverts_the_forward_kernel_doubles():
    """flow_inv undoes invconv_fwd + coupling_fwd of tests/_waveglow_doubles.py on the same (b | log_s): the column convention."""
    from tests import _waveglow_doubles as D
    g = torch.Generator().manual_seed(3)
    for c in (8, 6, 4):
        m = 257
        q, _ = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=torch.float64))
        w = (q + 0.05 * torch.randn(c, c, generator=g, dtype=torch.float64)).float()
        x = torch.randn(m, 8, generator=g)
        o = torch.randn(m, 8, generator=g) * 0.5
        y, _ = D.invconv_fwd(x, w, c, torch.float16)
        zz = D.coupling_fwd(y, o, c, torch.zeros(4))
        winv_t = D.logdet_inv(w, c, torch.zeros(1), torch.zeros(1))
        back, a0 = DI.flow_inv(zz, o, winv_t, c, next_c=c)
        assert torch.allclose(back, x, rtol=1e-4, atol=1e-4)
        assert torch.equal(back[:, :8 - c], x[:, :8 - c])
        assert torch.equal(a0[:, :c // 2], back[:, 8 - c:8 - c + c // 2].half()) and float(a0[:, c // 2:].abs().max()) == 0
