"""Write the HiFi-GAN fixtures from the reference's own Generator (SpeechSynthesis/HiFiGAN/hifigan/models.py:140-232), built on
the CPU:

  tests/golden/hifigan_state_dict.json   state-dict names and shapes (nothing else), in state_dict() order, for the V1 and the small
                                         configuration;
  tests/golden/hifigan_infer.npz         small configuration: the spectrogram [2, 80, 9], the configuration (JSON) and the float64
                                         output of the reference module after .double() and remove_weight_norm().

No weights are stored: every state tensor comes from tests/_hifigan_ref.fill_state, which the tests repeat.

    python tools/make_hifigan_fixture.py        (needs the reference tree: DLE_REFERENCE)
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference_models():
    """hifigan.models of the reference.  `librosa` (common/stft.py, common/audio_processing.py: window and filter-bank helpers the
    generator never touches) and `soundfile` are absent here: stubbed, as oracle/_ref_import.py stubs librosa for Tacotron2."""
    from oracle._ref_import import REF
    root = os.path.join(REF, "PyTorch", "SpeechSynthesis", "HiFiGAN")
    if root not in sys.path:
        sys.path.insert(0, root)
    util = _stub("librosa.util", pad_center=None, tiny=None, normalize=None)
    filt = _stub("librosa.filters", mel=None)
    _stub("librosa", util=util, filters=filt)
    _stub("soundfile")
    import importlib
    return importlib.import_module("hifigan.models")


def reference_generator(models, config, state=None):
    g = models.Generator(dict(config))
    if state is not None:
        g.load_state_dict(state)
    return g


def main():
    from deeplearningexamples_amd.hifigan.model import V1_CONFIG
    from tests._hifigan_ref import SMALL_CONFIG, fill_state, make_mel
    models = import_reference_models()
    golden = os.path.join(ROOT, "tests", "golden")
    shapes = {}
    for name, cfg in (("v1", V1_CONFIG), ("small", SMALL_CONFIG)):
        shapes[name] = {k: list(v.shape) for k, v in reference_generator(models, cfg).state_dict().items()}
    path = os.path.join(golden, "hifigan_state_dict.json")
    with open(path, "w") as f:
        json.dump(shapes, f, indent=0)                    # (keys in the order of the reference's state_dict())
        f.write("\n")
    print("wrote", path)

    g = reference_generator(models, SMALL_CONFIG, fill_state(SMALL_CONFIG)).double().eval()
    with contextlib.redirect_stdout(io.StringIO()):
        g.remove_weight_norm()
    mel = make_mel((2, 80, 9))
    with torch.no_grad():
        audio = g(mel.double())[:, 0]
    path = os.path.join(golden, "hifigan_infer.npz")
    np.savez_compressed(path, mel=mel.numpy(), config=np.array(json.dumps(SMALL_CONFIG, sort_keys=True)), audio=audio.numpy())
    print("wrote", path, "audio", tuple(audio.shape), "rms %.4f" % float(audio.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
