"""Write the FastPitch fixtures from the reference's own module (SpeechSynthesis/FastPitch/fastpitch/model.py), built on the CPU:

  tests/golden/fastpitch_state_dict.json   state-dict names and shapes (nothing else), in state_dict() order, for the default and
                                           the small configuration;
  tests/golden/fastpitch_infer.npz         small configuration, texts of 9, 5 and 1 symbols: the float64 outputs of the reference's
                                           FastPitch.double().eval().infer for EACH TEXT RUN ALONE (batch 1) -- once with the
                                           defaults, once with pace = 0.8 and a dur_tgt -- and the configuration (JSON).

No weights are stored: every state tensor comes from tests/_fastpitch_ref.fill_state, which the tests repeat.

    python tools/make_fastpitch_fixture.py            (needs the reference tree: DLE_REFERENCE)
    python tools/make_fastpitch_fixture.py --search   (no reference needed: prints DUR_SEED values under which the duration
                                                       conditions of tests/_fastpitch_ref.py hold)
"""
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


def import_reference_model():
    """fastpitch.model of the reference.  Absent here and never touched by infer(): numba (fastpitch/alignment.py: the training-only
    monotonic alignment search; `jit` becomes the identity), librosa and soundfile (common/: audio file helpers)."""
    from oracle._ref_import import REF
    root = os.path.join(REF, "PyTorch", "SpeechSynthesis", "FastPitch")
    if root not in sys.path:
        sys.path.insert(0, root)

    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f
    _stub("numba", jit=jit, prange=range)
    util = _stub("librosa.util", pad_center=None, tiny=None, normalize=None)
    filt = _stub("librosa.filters", mel=None)
    _stub("librosa", util=util, filters=filt)
    _stub("soundfile")
    import importlib
    return importlib.import_module("fastpitch.model")


def reference_module(ref, config, state=None):
    from deeplearningexamples_amd.fastpitch.model import check_config
    cfg = check_config(config)
    m = ref.FastPitch(**cfg)
    if state is not None:
        status = m.load_state_dict(state, strict=False)
        assert not status.unexpected_keys, status.unexpected_keys
        assert all(k.startswith("attention.") or k.endswith(".inv_freq") for k in status.missing_keys), status.missing_keys
    return m


def dur_targets(lens):
    """The dur_tgt of the second call: 0, 1, 3, 4 or 5 by position (zeros at the start, in the middle and at the end of the
    9-symbol text; never 2, whose quotient 2.5 at pace 0.8 is a rounding boundary): every quotient lies 0.25 from a boundary at least."""
    val = lambda i, n: 5 if (3 * i + n) % 5 == 2 else (3 * i + n) % 5
    return [torch.tensor([val(i, n) if 0 < i < n - 1 else 0 for i in range(n)], dtype=torch.float64) if n > 1
            else torch.tensor([3.0], dtype=torch.float64) for n in lens]


def conditions(model, texts, paces=(1.0,)):
    """The duration conditions of tests/_fastpitch_ref.py's docstring -> (ok, description)."""
    from tests._fastpitch_ref import duration_margin, forward64
    base, _ = forward64(model, texts, None, False, stop_after_durations=True)
    durs = torch.cat([o["dur_pred"] for o in base])
    if not (bool((durs == 0).any()) and bool((durs > 3).any())):
        return False, "no zero or no duration above 3"
    for dtype in (None, torch.float16, torch.bfloat16):
        for emulate in ((False,) if dtype is None else (False, True)):
            got, _ = forward64(model, texts, dtype, emulate, stop_after_durations=True)
            if not emulate and min(duration_margin(o["dur_pred"], p) for o in got for p in paces) < 0.1:
                return False, "margin below 0.1 (%s)" % dtype
            if any(not torch.equal(a["reps"], b["reps"]) for a, b in zip(got, base)):
                return False, "repetitions differ (%s, emulate %s)" % (dtype, emulate)
    return True, "durations %s" % [[round(float(v), 2) for v in o["dur_pred"]] for o in base]


def search():
    from deeplearningexamples_amd.fastpitch.model import DEFAULT_CONFIG
    from tests._fastpitch_ref import SMALL_CONFIG, TEXT_LENS, make_model, make_texts
    for name, cfg, lens in (("small", SMALL_CONFIG, TEXT_LENS["small"]), ("default", DEFAULT_CONFIG, TEXT_LENS["default"]),
                            ("small, 3 speakers", dict(SMALL_CONFIG, n_speakers=3), TEXT_LENS["small"])):
        texts = make_texts(lens)
        for ds in range(2000):
            ok, what = conditions(make_model(cfg, dur_seed=ds), texts)
            if ok:
                print("%s: DUR_SEED %d; %s" % (name, ds, what))
                break
        else:
            print("%s: nothing found" % name)


def main():
    if "--search" in sys.argv[1:]:
        return search()
    from deeplearningexamples_amd.fastpitch.model import DEFAULT_CONFIG, check_config
    from tests._fastpitch_ref import SMALL_CONFIG, TEXT_LENS, fill_state, make_texts
    ref = import_reference_model()
    golden = os.path.join(ROOT, "tests", "golden")
    shapes = {}
    for name, cfg in (("default", DEFAULT_CONFIG), ("small", SMALL_CONFIG)):
        shapes[name] = {k: list(v.shape) for k, v in reference_module(ref, cfg).state_dict().items()}
    path = os.path.join(golden, "fastpitch_state_dict.json")
    with open(path, "w") as f:
        json.dump(shapes, f, indent=0)                    # (keys in the order of the reference's state_dict())
        f.write("\n")
    print("wrote", path)

    m = reference_module(ref, SMALL_CONFIG, fill_state(SMALL_CONFIG)).double().eval()
    texts = make_texts(TEXT_LENS["small"])
    tgt = dur_targets(TEXT_LENS["small"])
    arrays = dict(config=np.array(json.dumps(check_config(SMALL_CONFIG), sort_keys=True)))
    with torch.no_grad():
        for u, ids in enumerate(texts):
            for call, kw in (("a", {}), ("b", dict(pace=0.8, dur_tgt=tgt[u][None]))):
                mel, mel_lens, dur_pred, pitch_pred, energy_pred = m.infer(ids[None], **kw)
                arrays["text%d" % u] = ids.numpy()
                arrays["%s%d_mel" % (call, u)] = mel[0].numpy()
                arrays["%s%d_mel_len" % (call, u)] = mel_lens.numpy()
                arrays["%s%d_dur_pred" % (call, u)] = dur_pred[0].numpy()
                arrays["%s%d_pitch_pred" % (call, u)] = pitch_pred[0, 0].numpy()
                arrays["%s%d_energy_pred" % (call, u)] = energy_pred[0].numpy()
            arrays["b%d_dur_tgt" % u] = tgt[u].numpy()
            print("text %d: %d symbols -> %d / %d frames, mel rms %.3f" % (u, ids.numel(), int(arrays["a%d_mel_len" % u][0]),
                                                                        int(arrays["b%d_mel_len" % u][0]),
                                                                        float(np.sqrt((arrays["a%d_mel" % u] ** 2).mean()))))
    path = os.path.join(golden, "fastpitch_infer.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path)


if __name__ == "__main__":
    main()
