"""Write the Jasper fixtures from the reference's own modules (SpeechRecognition/Jasper/jasper/model.py, common/features.py,
inference.py), built on the CPU:

  tests/golden/jasper_state_dict.json   state-dict names and shapes (nothing else), in state_dict() order, for the 10x5dr YAML
                                        (configs/jasper10x5dr_speedp-online_speca.yaml) and the small configuration;
  tests/golden/jasper_cli_flags.json    the option strings of the reference parser (inference.py:45-98), with the number of values
                                        each takes;
  tests/golden/jasper_infer.npz         small configuration (tests/_jasper_ref.small_config, weights fill_state(cfg, SEED, True)):
                                        the float64 log-probs of the reference's Jasper.double().eval() for EACH UTTERANCE RUN ALONE
                                        with 16 leading zero frames (features seeded_features((150, 41, 2), 7)); the reference
                                        FilterbankFeatures output (fp32, dither 0, normalised and masked) for three seeded synthetic
                                        waveforms, each run alone, and `feat_fp32_vs_fp64`: the largest difference between that
                                        output and the same arithmetic restated in float64.

No weights are stored: every state tensor comes from tests/_jasper_ref.fill_state, which the tests repeat.  librosa is not
installed: `librosa.filters.mel` is bound to this project's bank (tacotron2.audio.mel_filter_bank), so the feature fixture pins the
pipeline AROUND the bank, not the bank's parity with librosa.  soundfile and sox (file helpers) are stubbed.

    python tools/make_jasper_fixture.py            (needs the reference tree: DLE_REFERENCE)
"""
import ast
import copy
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

WAVE_SAMPLES = (16000, 7777, 2400)
SEED, LEAD = 1, 16                   # tests/test_gpu_jasper_infer.py: the small case's weights, --pad_leading


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def reference_root():
    from oracle._ref_import import REF
    return os.path.join(REF, "PyTorch", "SpeechRecognition", "Jasper")


def import_reference():
    """(jasper.model, common.features) of the reference.  Other recipes of the reference have packages of the same names
    (`common`), so whatever this process holds under those names is set aside for the import and put back afterwards."""
    from deeplearningexamples_amd.tacotron2.audio import mel_filter_bank
    import importlib
    root = reference_root()
    mine = lambda k: k.split(".")[0] in ("common", "jasper", "librosa", "soundfile", "sox")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if mine(k)}
    sys.path.insert(0, root)
    try:
        filt = _stub("librosa.filters", mel=lambda sr, n_fft, n_mels, fmin, fmax: mel_filter_bank(sr, n_fft, n_mels, fmin, fmax))
        _stub("librosa", filters=filt)
        _stub("soundfile")
        _stub("sox")
        return importlib.import_module("jasper.model"), importlib.import_module("common.features")
    finally:
        sys.path.remove(root)
        for k in [k for k in sys.modules if mine(k)]:
            del sys.modules[k]
        sys.modules.update(saved)


def reference_module(ref_model, cfg):
    """Jasper(encoder_kw, decoder_kw) as inference.py:270-274 builds it through jasper/config.py (a deep copy: the YAML's anchors
    share block dicts, and JasperEncoder pops `residual_dense` from them)."""
    enc = copy.deepcopy(cfg["jasper"]["encoder"])
    dec = dict(cfg["jasper"]["decoder"], n_classes=len(cfg["labels"]) + 1)
    return ref_model.Jasper(encoder_kw=enc, decoder_kw=dec)


def parser_flags():
    """get_parser of the reference's inference.py, compiled ALONE (the module imports DALI, tqdm and the NeMo converter)."""
    path = os.path.join(reference_root(), "inference.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_parser"]
    import argparse
    ns = {"argparse": argparse, "os": os}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    out = []
    for a in ns["get_parser"]()._actions:
        if a.option_strings and a.dest != "help":
            nvals = 0 if a.nargs == 0 else ("+" if a.nargs == "+" else 1)
            out.append(dict(flags=list(a.option_strings), values=nvals, required=bool(a.required), choices=list(a.choices or [])))
    return out


def synthetic_waves():
    g = torch.Generator().manual_seed(11)
    waves = []
    for i, n in enumerate(WAVE_SAMPLES):
        t = torch.arange(n, dtype=torch.float64) / 16000
        w = 0.3 * torch.sin(2 * np.pi * (220 + 130 * i) * t) + 0.1 * torch.sin(2 * np.pi * (1800 + 900 * i) * t * (1 + 0.3 * t))
        w = w + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
        waves.append(w.to(torch.float32))
    return waves


def features64(wave, fb, window, n_fft, hop, win):
    """calculate_features (features.py:259-302), dither 0, restated in float64 for one utterance."""
    x = wave.double().reshape(1, -1)
    n = int(np.ceil(x.shape[1] / hop))
    x = torch.cat((x[:, 0].unsqueeze(1), x[:, 1:] - 0.97 * x[:, :-1]), dim=1)
    spec = torch.view_as_real(torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=win, window=window.double(), return_complex=True))
    mel = torch.log(torch.matmul(fb.double(), spec.pow(2).sum(-1)) + 1e-20)
    m = mel[0, :, :n].mean(1, keepdim=True)
    s = mel[0, :, :n].std(1, keepdim=True) + 1e-5
    out = (mel[0] - m) / s
    out[:, n:] = 0
    return out, n


def main():
    import yaml
    from tests import _jasper_ref as R
    ref_model, ref_feat = import_reference()
    golden = os.path.join(ROOT, "tests", "golden")
    # (the YAML's anchors make blocks share one dict; jasper/config.py:22-32 reloads to separate them, as the JSON round trip does)
    big = json.loads(json.dumps(yaml.safe_load(open(os.path.join(reference_root(), "configs", "jasper10x5dr_speedp-online_speca.yaml")))))
    small = R.small_config()
    shapes = {}
    for name, cfg in (("10x5dr", big), ("small", small)):
        shapes[name] = {k: list(v.shape) for k, v in reference_module(ref_model, cfg).state_dict().items()}
    path = os.path.join(golden, "jasper_state_dict.json")
    with open(path, "w") as f:
        json.dump(shapes, f, indent=0)
        f.write("\n")
    print("wrote", path)

    path = os.path.join(golden, "jasper_cli_flags.json")
    with open(path, "w") as f:
        json.dump(parser_flags(), f, indent=0)
        f.write("\n")
    print("wrote", path)

    arrays = {}
    state = R.fill_state(small, SEED, True)
    m = reference_module(ref_model, small)
    m.load_state_dict(state, strict=True)
    m = m.double().eval()
    feats = R.seeded_features((150, 41, 2), 7)
    with torch.no_grad():
        for u, f in enumerate(feats):
            # (the reference is handed normalised features: per-feature normalisation restated in float64, as forward64 does)
            x = f.double()
            x = (x - x.mean(1, keepdim=True)) / (x.std(1, keepdim=True) + 1e-5)
            x = torch.nn.functional.pad(x, (LEAD, 0))                     # inference.py:332-333
            logp, lens = m(x[None], torch.tensor([f.shape[1] + LEAD]))
            arrays["logp%d" % u] = logp[0, :int(lens[0])].numpy()
            print("utterance %d: %d + %d frames -> %d rows" % (u, LEAD, f.shape[1], int(lens[0])))
    fp = ref_feat.FilterbankFeatures(**dict(big["input_val"]["filterbank_features"], dither=0.0))
    worst = 0.0
    with torch.no_grad():
        for u, w in enumerate(synthetic_waves()):
            out, n = fp.calculate_features(w.clone()[None], torch.tensor([w.numel()]))
            o64, n64 = features64(w, fp.fb[0], fp.window, fp.n_fft, fp.hop_length, fp.win_length)
            assert int(n[0]) == n64
            worst = max(worst, float((out[0].double() - o64).abs().max()))
            arrays["feat%d" % u] = out[0].numpy()
            arrays["feat%d_len" % u] = np.asarray(int(n[0]))
    arrays["feat_fp32_vs_fp64"] = np.asarray(worst)
    print("front end: fp32 against float64, largest difference %.3e" % worst)
    path = os.path.join(golden, "jasper_infer.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path)


if __name__ == "__main__":
    main()
