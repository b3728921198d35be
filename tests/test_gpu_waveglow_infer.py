"""WaveGlow inference on the MI355X: dle_wg_flow_inv(_first) against their plain-torch statements, WaveGlowVocoder.infer against
the fixture the REFERENCE's own WaveGlow.infer produced (tests/golden/waveglow_infer.npz), the round trip through the train
step's forward, memory that does not grow with n_flows, the command line and one call of the reference-size network.

Bars of the whole-network checks follow tests/test_gpu_waveglow.py: the FLOOR is what 16-bit storage alone costs, measured here
(and printed) with the fp64-accumulating statement of tests/_waveglow_infer_doubles.py rounding at the engine's storage points;
the kernels get MARGIN x that floor.  MARGIN = 4: the engine's result is another realisation of the same roundings (fp32
accumulation, other tanh / exp) -- each rounding that falls the other way moves the audio as much as the storage error itself, so
its distance from the reference is a second draw of the floor's size, and the inverse couplings multiply whatever an earlier flow
left (exp(-log_s), W^-1), which spreads two draws by a small factor.  Nothing here is taken from the kernels' own output.
"""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import _waveglow_doubles as D
from tests import _waveglow_infer_doubles as DI

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTYPES = [torch.float16, torch.bfloat16]
MARGIN = 4.0


def _tol16(dtype):                                        # the 16-bit operand tolerances of tests/test_gpu_waveglow.py
    return dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=1.6e-2, atol=1.6e-2)


def _close(got, ref, **kw):
    np.testing.assert_allclose(got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy(), **kw)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _rot(c, g, noise=0.05):
    q, _ = torch.linalg.qr(torch.randn(c, c, generator=g))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return (q + noise * torch.randn(c, c, generator=g)).contiguous()


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [512, 1000, 70001])
@pytest.mark.parametrize("early", [0, 2])
@pytest.mark.parametrize("c", [8, 6, 4])
def test_flow_inv_vs_double(cuda, c, early, m, dtype):
    from deeplearningexamples_amd.waveglow import ops
    g = torch.Generator().manual_seed(c * 100 + early * 10 + m)
    state = torch.randn(m, 8, generator=g)
    o = torch.randn(m, 8, generator=g) * 0.5
    noise = torch.randn(m, 8, generator=g)
    winv_t = D.logdet_inv(_rot(c, g), c, torch.zeros(1), torch.zeros(1)).reshape(-1)
    if early > 8 - c:
        # a flow that still owns all 8 columns has no column to fill with an early output: the entry point says so
        with pytest.raises(ValueError, match="early"):
            ops.flow_inv(state.to(cuda), o.to(cuda), winv_t.to(cuda), c, early=early, noise=noise.to(cuda), z_col=4, sigma=0.9)
        return
    next_c, z_col, sigma = c + early, 4 if early else 0, 0.9
    ref, a0r = DI.flow_inv(state, o, winv_t, c, next_c, early, noise, z_col, sigma, dtype)
    a0 = torch.full((m, 8), 7.0, dtype=dtype, device=cuda)
    out, _ = ops.flow_inv(state.to(cuda), o.to(cuda), winv_t.to(cuda), c, a0=a0, next_c=next_c, early=early, noise=noise.to(cuda),
                          z_col=z_col, sigma=sigma)
    # fp32 outputs: the class tests/test_gpu_waveglow.py holds for the same 8 x 8 row product; exp(-log_s) is expf (1 ulp) on
    # |log_s| <~ 2, its error stays inside that bar
    _close(out, ref, rtol=1e-5, atol=1e-5)
    _close(a0, a0r, **_tol16(dtype))
    assert float(a0[:, next_c // 2:].abs().max()) == 0                                       # zero padded to 8 columns
    off = 8 - c
    assert torch.equal(out[:, :off - early].cpu(), state[:, :off - early])                 # channels below pass through
    if early:
        assert torch.equal(out[:, off - early:off].cpu(), sigma * noise[:, z_col:z_col + early])
    # in place (how the vocoder runs it), and without an operand
    st = state.to(cuda)
    same, none = ops.flow_inv(st, o.to(cuda), winv_t.to(cuda), c, out=st, early=early, noise=noise.to(cuda), z_col=z_col, sigma=sigma)
    assert same.data_ptr() == st.data_ptr() and none is None and torch.equal(st, out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [8, 6, 4])
def test_flow_inv_first_vs_double(cuda, c, dtype):
    from deeplearningexamples_amd.waveglow import ops
    m = 1000
    noise = torch.randn(m, 8, generator=torch.Generator().manual_seed(c))
    out = torch.full((m, 8), 3.0, device=cuda)
    a0 = torch.full((m, 8), 3.0, dtype=dtype, device=cuda)
    ops.flow_inv_first(noise.to(cuda), c, 0.7, out, a0)
    ref, a0r = DI.flow_inv_first(noise, c, 0.7, dtype)
    assert torch.equal(out.cpu(), ref) and torch.equal(a0.cpu(), a0r)


def test_flow_inv_argument_checks(cuda):
    from deeplearningexamples_amd.waveglow import ops
    st = torch.zeros(64, 8, device=cuda)
    w = torch.eye(8, device=cuda).reshape(-1)
    with pytest.raises(ValueError):
        ops.flow_inv(st, st, w, 5)                                                          # odd c
    with pytest.raises(ValueError):
        ops.flow_inv(st, st, w, 6, a0=torch.zeros(64, 8, dtype=torch.float16, device=cuda), next_c=4)   # next flow cannot have fewer
    with pytest.raises(ValueError):
        ops.flow_inv(st, st[:32], w, 6)
    with pytest.raises(Exception):
        ops.flow_inv(st.cpu(), st, w, 6)                                                    # no CPU path


# ------------------------------------------------------------------------------------------------- the network
def _case():
    from oracle import waveglow_oracle as WO
    gold = np.load(os.path.join(HERE, "golden", "waveglow_infer.npz"))
    cfg = WO.WAVEGLOW_SMALL
    return WO, cfg, WO.seeded_state(cfg, 7), gold, torch.from_numpy(gold["mel"]), torch.from_numpy(gold["z"])


def _vocoder(cuda, cfg, state, dtype):
    from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
    from deeplearningexamples_amd.waveglow.model import WaveGlow
    model = WaveGlow(**cfg, device=cuda)
    model.load_reference_state(state)
    return model, WaveGlowVocoder(model, compute_dtype=dtype)


@pytest.mark.parametrize("tag,sigma", [("s09", 0.9), ("s0", 0.0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_infer_vs_reference_fixture(cuda, dtype, tag, sigma):
    """sigma 0.9 with the recorded noise, and sigma 0 -- exactly what the denoiser runs, deterministic."""
    WO, cfg, p, gold, mel, z = _case()
    want = torch.from_numpy(gold["audio_" + tag])
    floor = _rel(DI.infer(p, cfg, mel, z, sigma, store=dtype, work=torch.float64), want)
    model, voc = _vocoder(cuda, cfg, p, dtype)
    got = voc.infer(mel.to(cuda), sigma=sigma, z=z.to(cuda))
    assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    err = _rel(got, want)
    print("infer %s sigma %s: rel L2 %.3e, 16-bit storage floor %.3e, bar %.3e" % (dtype, sigma, err, floor, MARGIN * floor))
    assert err <= MARGIN * floor, (err, floor)
    if sigma == 0.0:                                      # the noise does not matter at sigma 0
        again = voc.infer(mel.to(cuda), sigma=0.0).clone()
        assert torch.equal(again, voc.infer(mel.to(cuda), sigma=0.0, z=z.to(cuda)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_through_the_train_forward(cuda, dtype):
    """vocoder(z) -> audio -> WaveGlowTrainer.forward with the same weights -> z again.
    Floor: the 16-bit-storage forward flow applied to the reference's EXACT audio of this z.  (The doubles' own infer -> forward
    chain is no floor: both of its passes round a0 identically, so it returns z to 2e-5 / 9e-8 by bit-identical arithmetic,
    which two GEMM passes with different summation orders do not share; one a0 rounding that falls the other way between the
    passes is an error of the storage class, which is what this floor measures.)"""
    from deeplearningexamples_amd.waveglow.engine import WaveGlowTrainer
    WO, cfg, p, gold, mel, z = _case()
    sigma = 0.9
    want = DI.noise_in_forward_order(z, cfg, sigma)                                         # [B, 8, T/8], the forward's channel order
    floor = _rel(DI.forward_z(p, cfg, mel, torch.from_numpy(gold["audio_s09"]), store=dtype, work=torch.float64), want)
    chain = _rel(DI.forward_z(p, cfg, mel, DI.infer(p, cfg, mel, z, sigma, store=dtype).float(), store=dtype), want)
    model, voc = _vocoder(cuda, cfg, p, dtype)
    audio = voc.infer(mel.to(cuda), sigma=sigma, z=z.to(cuda)).clone()
    tr = WaveGlowTrainer(model, compute_dtype=dtype, sigma=sigma)
    tr.forward(mel.to(cuda), audio)
    got = tr.z.view(z.shape[0], -1, 8).permute(0, 2, 1)                                     # the last state IS z: rows (b, t)
    err = _rel(got, want)
    print("round trip %s: rel L2 %.3e, floor %.3e (the doubles' own chain: %.3e), bar %.3e" % (dtype, err, floor, chain, MARGIN * floor))
    assert err <= MARGIN * floor, (err, floor)


def _peak_of_first_call(cuda, n_flows):
    from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
    from deeplearningexamples_amd.waveglow.model import WaveGlow
    cfg = dict(n_mel_channels=80, n_flows=n_flows, n_group=8, n_early_every=4, n_early_size=2,
               WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
    torch.manual_seed(n_flows)
    voc = WaveGlowVocoder(WaveGlow(**cfg, device=cuda), compute_dtype=torch.float16)
    mel = (torch.randn(1, 80, 256) * 1.98 - 5.62).to(cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    audio = voc.infer(mel, sigma=0.9)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base       # the weights were there before: work buffers + transients of the call
    assert audio.shape == (1, 256 * 256) and bool(torch.isfinite(audio).all())
    held = torch.cuda.memory_allocated()
    voc.infer(mel, sigma=0.9)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held, "the second call at the same shape allocated"
    assert len(voc._buffers) == 1
    return peak


def test_memory_does_not_scale_with_the_number_of_flows(cuda):
    p12, p4 = _peak_of_first_call(cuda, 12), _peak_of_first_call(cuda, 4)
    print("peak bytes of one [1, 80, 256] call: 12 flows %d, 4 flows %d" % (p12, p4))
    assert p12 > 0 and abs(p12 - p4) <= 0.05 * max(p12, p4), (p12, p4)


def test_command_line_writes_audio(cuda, tmp_path):
    """A checkpoint as waveglow/train.py writes it -> --synth-data -> .wav files; --denoising-strength 0 is infer, bit for bit."""
    from deeplearningexamples_amd.waveglow import inference as I
    from deeplearningexamples_amd.waveglow import train as T
    from deeplearningexamples_amd.waveglow.engine import WaveGlowTrainer
    WO, cfg, p, gold, mel, z = _case()
    model, voc = _vocoder(cuda, cfg, p, torch.float16)
    ckpt = T.save_checkpoint(WaveGlowTrainer(model, compute_dtype=torch.float16), 0, cfg, str(tmp_path), "WaveGlow", 0, 1)
    frames, out = 12, str(tmp_path / "audio")
    common = ["--waveglow", ckpt, "--synth-data", "--synth-frames", str(frames), "-bs", "2", "-o", out, "--fp16", "-sr", "16000",
              "--seed", "11"]
    plain = I.main(common + ["--denoising-strength", "0", "--suffix", "_raw"]).clone()
    torch.manual_seed(11)
    direct = voc.infer(I.synth_mel(2, 80, frames, 11).to(cuda), sigma=0.9)
    assert torch.equal(plain, direct)
    den = I.main(common + ["--denoising-strength", "0.1"])
    assert den.shape == plain.shape and bool(torch.isfinite(den).all()) and not torch.equal(den, plain)
    assert _rel(den, plain) < 0.2                         # the bias removal is a correction, not another signal
    for name, ref in (("audio_0_raw.wav", plain[0]), ("audio_1_raw.wav", plain[1]), ("audio_0.wav", den[0]), ("audio_1.wav", den[1])):
        with wave.open(os.path.join(out, name), "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, frames * 256)
            pcm = np.frombuffer(f.readframes(frames * 256), dtype="<i2").astype(np.float64) / 32767.0
        a = ref.double().cpu().numpy()
        assert np.abs(pcm - a / np.abs(a).max()).max() <= 1.0 / 32767.0
    log = open(os.path.join(out, "nvlog.json")).read()
    assert "waveglow_latency" in log and "waveglow_items_per_sec" in log and "denoiser_latency" in log


_FULL_SIZE = """
import sys, torch
sys.path.insert(0, %r)
from deeplearningexamples_amd.waveglow.infer import WaveGlowVocoder
from deeplearningexamples_amd.waveglow.model import DEFAULT_CONFIG, WaveGlow
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = WaveGlow(**DEFAULT_CONFIG, device=dev)
with torch.no_grad():
    for k in range(12):                                   # a fresh `end` is zero: give the couplings something to undo
        model.store["WN.%%d.end.weight" %% k].normal_(0.0, 0.01)
        model.store["WN.%%d.end.bias" %% k].normal_(0.0, 0.05)
voc = WaveGlowVocoder(model)
mel = (torch.randn(1, 80, 895) * 1.98 - 5.62).to(dev)
audio = voc.infer(mel, sigma=0.9)
torch.cuda.synchronize()
print("FULL", tuple(audio.shape), bool(torch.isfinite(audio).all()), float(audio.abs().max()), float(audio.std()))
"""


def test_reference_size_network_one_utterance(cuda, tmp_path):
    """n_channels 512, 12 flows, [1, 80, 895] (the reference's inference_perf input): 229,120 finite samples; its own time limit."""
    script = tmp_path / "full_size.py"
    script.write_text(_FULL_SIZE % ROOT)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FULL")][-1]
    print(line)
    assert "(1, 229120) True" in line
