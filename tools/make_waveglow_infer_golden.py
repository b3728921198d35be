"""Writes tests/golden/waveglow_infer.npz from the REFERENCE's own WaveGlow.infer and Denoiser (CPU, fp32).  Needs the reference
tree (oracle/_ref_import.py, DLE_REFERENCE); run once where it is mounted:

    python tools/make_waveglow_infer_golden.py

Case: oracle.waveglow_oracle.WAVEGLOW_SMALL with seeded_state(.., 7) (a fresh model has end = 0, which makes every flow an
identity), batch 2 x 8 mel frames, one recorded noise tensor z [2, 8, 256] in infer_onnx's layout, sigma 0.9 and 0.0.  The
reference's infer draws its noise with torch.randn; the draws are replaced by the recorded z for the duration of the call, and
infer_onnx (explicit z; it leaves the early draws unscaled, so they are passed pre-multiplied by sigma) must agree.  The
Denoiser (bias from the same model, strength 0.1) is applied to the sigma 0.9 audio.  librosa is not installed here: the three
helpers tacotron2_common imports from it are supplied as small numpy functions of the documented behaviour.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_import as R                                      # noqa: E402
from oracle import waveglow_oracle as WO                                 # noqa: E402

SEED, BATCH, FRAMES, STRENGTH = 7, 2, 8, 0.1


def case_inputs(cfg):
    rng = np.random.default_rng(SEED + 100)
    mel = (rng.standard_normal((BATCH, cfg["n_mel_channels"], FRAMES)) * 2.0 - 5.0).astype(np.float32)
    z = rng.standard_normal((BATCH, cfg["n_group"], FRAMES * 256 // cfg["n_group"])).astype(np.float32)
    return torch.from_numpy(mel), torch.from_numpy(z)


def _librosa_stubs():
    def pad_center(data, size):
        lo = (size - len(data)) // 2
        return np.pad(data, (lo, size - len(data) - lo))

    def tiny(x):
        return np.finfo(np.asarray(x).dtype if np.issubdtype(np.asarray(x).dtype, np.floating) else np.float32).tiny

    def normalize(s, norm=None):
        assert norm is None
        return s
    util = types.ModuleType("librosa.util")
    util.pad_center, util.tiny, util.normalize = pad_center, tiny, normalize
    filt = types.ModuleType("librosa.filters")
    filt.mel = None
    top = types.ModuleType("librosa")
    top.util, top.filters = util, filt
    sys.modules.update({"librosa": top, "librosa.util": util, "librosa.filters": filt})


class _Feed:
    """Stands in for torch.randn inside WaveGlow.infer: hands out the recorded noise in the order it is asked for."""

    def __init__(self, chunks):
        self.chunks = list(chunks)

    def __call__(self, *shape, **kw):
        t = self.chunks.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.clone()


def reference_infer(model, cfg, mel, z, sigma):
    n_rem, es = model.n_remaining_channels, cfg["n_early_size"]
    chunks = [z[:, :n_rem]] + [z[:, c:c + es] for c in range(n_rem, cfg["n_group"], es)]
    real = torch.randn
    torch.randn = _Feed(chunks)
    try:
        with torch.no_grad():
            audio = model.infer(mel, sigma=sigma)
    finally:
        torch.randn = real
    with torch.no_grad():
        onnx = model.infer_onnx(mel, torch.cat([z[:, :n_rem], sigma * z[:, n_rem:]], 1), sigma=sigma)
    assert torch.equal(audio, onnx), float((audio - onnx).abs().max())
    return audio


def main():
    if not R.have_reference():
        raise SystemExit("the reference tree is not mounted (DLE_REFERENCE)")
    ref = R.import_waveglow()
    cfg = WO.WAVEGLOW_SMALL
    model = ref.model.WaveGlow(**cfg)
    model.load_state_dict(WO.seeded_state(cfg, SEED))
    model.eval()
    mel, z = case_inputs(cfg)
    arrs = {"mel": mel.numpy(), "z": z.numpy()}
    for tag, sigma in (("s09", 0.9), ("s0", 0.0)):
        arrs["audio_" + tag] = reference_infer(model, cfg, mel, z, sigma).numpy()
    assert arrs["audio_s09"].shape == (BATCH, FRAMES * 256)
    # the reference Denoiser: tacotron2_common.{layers, stft, audio_processing} by their package name
    _librosa_stubs()
    root = os.path.join(R.REF, "PyTorch", "SpeechSynthesis", "Tacotron2")
    sys.path.insert(0, root)
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ref_waveglow_denoiser", os.path.join(root, "waveglow", "denoiser.py"))
    den = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(den)
    d = den.Denoiser(model)
    with torch.no_grad():
        out = d(torch.from_numpy(arrs["audio_s09"]), strength=STRENGTH)
    arrs["denoised_s09"] = out.numpy()
    arrs["denoiser_strength"] = np.asarray([STRENGTH], np.float64)
    arrs["denoiser_bias_spec"] = d.bias_spec.numpy()
    path = os.path.join(ROOT, "tests", "golden", "waveglow_infer.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, {k: v.shape for k, v in arrs.items()}, "%d bytes" % os.path.getsize(path))
    # what the plain-torch statement of tests/_waveglow_infer_doubles.py gives on the same case (the bars of the host tests)
    from tests import _waveglow_infer_doubles as D
    p = WO.seeded_state(cfg, SEED)
    for tag, sigma in (("s09", 0.9), ("s0", 0.0)):
        want = torch.from_numpy(arrs["audio_" + tag]).double()
        for work in (torch.float32, torch.float64):
            got = D.infer(p, cfg, mel, z, sigma, work=work).double()
            print("double vs reference, sigma %s, %s: max abs %.3e, rel L2 %.3e (max |audio| %.3f)" % (
                sigma, work, float((got - want).abs().max()), float((got - want).norm() / want.norm()), float(want.abs().max())))


if __name__ == "__main__":
    main()
