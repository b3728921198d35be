"""Writes the TFT fixtures under tests/golden/ from a checkout of the reference recipe (CPU only; needs pandas and scikit-learn,
which the reference's data_utils imports).  Recorded data only: results of the reference's programs, never their text.

    python tools/make_tft_fixture.py --reference /path/to/DeepLearningExamples/PyTorch/Forecasting/TFT

  tft_forecasts.npz     float64 forecasts of the reference model for the small cases of tests/_tft_ref.py (weights and inputs are
                        regenerated from seeds there, so only results are stored)
  tft_state_dict.json   parameter / buffer names and shapes of the electricity and traffic models
  tft_cli_flags.json    the flags and defaults of the reference's inference.py parser
  tft_small.csv         a small preprocessed split, and tft_dataset.npz: what the reference's TFTDataset yields for it
  tft_metrics.npz       qrisk and both un-scalings on recorded arrays (the scalers are StandardScaler(mean, scale) pairs, recorded)
  tft_checkpoint.pt     a hidden_size 8 electricity model in the reference's {'config', 'model'} form, its config pickled as the
                        reference's class (for the host load path only)
"""
import argparse
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FORECAST_CASES = [("elec", 12, 8), ("elec", 40, 33), ("obs", 12, 8), ("obs", 40, 33)]
SEED_STATE, SEED_BATCH, BATCH = 11, 12, 5


def reference_modules(ref):
    os.environ["TFT_SCRIPTING"] = "1"                      # modeling.py: skip torch.jit.script
    import torch
    torch.cuda.synchronize = lambda *a, **k: None          # TFTBack.forward calls it
    sys.path.insert(0, ref)
    import pandas as pd
    getitem = pd.DataFrame.__getitem__                     # TFTDataset indexes a frame with a set, which pandas 2 refuses
    pd.DataFrame.__getitem__ = lambda self, key: getitem(self, sorted(key) if isinstance(key, set) else key)
    import configuration
    import criterions
    import data_utils
    import modeling
    return torch, configuration, data_utils, modeling, criterions


def functions_of(path, names, namespace):
    """Definitions `names` of a reference file that cannot be imported here (it imports its logger and plotting stack)."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), namespace)
    return [namespace[n] for n in names]


def parser_flags(path):
    """(flag, default, action, type) of every add_argument call of the reference's command line, read from its syntax tree."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            lit = lambda k: ast.literal_eval(kw[k]) if k in kw else None
            action = lit("action")
            out.append({"flag": ast.literal_eval(node.args[0]), "default": False if action == "store_true" else lit("default"),
                        "action": action, "type": getattr(kw.get("type"), "id", None)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    torch, configuration, data_utils, modeling, criterions = reference_modules(args.reference)
    from tests import _tft_ref as R
    os.makedirs(GOLDEN, exist_ok=True)

    # 1. forecasts of the small cases, float64
    out = {}
    for kind, T, enc in FORECAST_CASES:
        cfg = R.small_config(kind, T, enc)
        sd = R.seeded_state(cfg, SEED_STATE)
        batch = R.seeded_batch(cfg, BATCH, SEED_BATCH)
        ref_cfg = types.SimpleNamespace(**{k: getattr(cfg, k) for k in dir(cfg) if not k.startswith("_") and not callable(getattr(cfg, k))})
        model = modeling.TemporalFusionTransformer(ref_cfg).double()
        model.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.no_grad():
            y = model.eval()({k: (v.double() if v.is_floating_point() else v) for k, v in batch.items() if v is not None})
        out["%s_T%d_enc%d" % (kind, T, enc)] = y.numpy()
    np.savez_compressed(os.path.join(GOLDEN, "tft_forecasts.npz"), **out)

    # 2. names and shapes of the two published models (one forward materialises the lazy embedding parameters)
    shapes = {}
    for name, cls in configuration.CONFIGS.items():
        cfg = cls()
        model = modeling.TemporalFusionTransformer(cfg)
        T = cfg.example_length
        dummy = {"s_cat": torch.zeros(1, T, 1, dtype=torch.long), "k_cont": torch.zeros(1, T, cfg.temporal_known_continuous_inp_size),
                 "target": torch.zeros(1, T, 1)}
        with torch.no_grad():
            model.eval()(dummy)
        shapes[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
    json.dump(shapes, open(os.path.join(GOLDEN, "tft_state_dict.json"), "w"), indent=0, sort_keys=True)

    # 3. the command line's flags
    json.dump(parser_flags(os.path.join(args.reference, "inference.py")), open(os.path.join(GOLDEN, "tft_cli_flags.json"), "w"), indent=1)

    # 4. a small split and what TFTDataset yields for it: 3 series of 9, 7 and 4 rows (the last one too short), rows shuffled
    cfg = configuration.ElectricityConfig()
    cfg.example_length, cfg.encoder_length = 5, 3
    rng = np.random.RandomState(5)
    rows = []
    for sid, n in ((2, 9), (0, 7), (1, 4)):
        for t in range(n):
            rows.append({"id": sid, "hours_from_start": float(t + 10 * sid), "power_usage": rng.randn(), "hour": rng.randn(),
                         "day_of_week": rng.randn(), "categorical_id": sid, "days_from_start": t // 2, "extra": rng.randn()})
    order = rng.permutation(len(rows))
    csv_path = os.path.join(GOLDEN, "tft_small.csv")
    cols = list(rows[0])
    with open(csv_path, "w") as f:
        f.write("," + ",".join(cols) + "\n")
        for i, j in enumerate(order):
            f.write("%d," % i + ",".join(repr(rows[j][c]) for c in cols) + "\n")
    ds = data_utils.TFTDataset(csv_path, cfg)
    items = {"len": np.asarray(len(ds))}
    for i in range(len(ds)):
        for k, v in ds[i].items():
            items["%d_%s" % (i, k)] = v.numpy()
    np.savez_compressed(os.path.join(GOLDEN, "tft_dataset.npz"), **items)

    # 5. qrisk and the un-scalings
    import pandas as pd
    import sklearn.preprocessing
    unscale_per_id, unscale = functions_of(os.path.join(args.reference, "inference.py"), ["_unscale_per_id", "_unscale"], {"pd": pd, "np": np})
    pred, tgt = rng.randn(12, 4, 3), rng.randn(12, 4, 1)
    ids = np.repeat(np.arange(3), 4)
    means, scales = rng.randn(3), 0.5 + rng.rand(3)
    scalers = {}
    for i in range(3):
        s = sklearn.preprocessing.StandardScaler()
        s.mean_, s.scale_, s.var_, s.n_features_in_ = np.array([means[i]]), np.array([scales[i]]), np.array([scales[i] ** 2]), 1
        scalers[i] = s
    ucfg = types.SimpleNamespace(example_length=7, encoder_length=3)
    np.savez_compressed(os.path.join(GOLDEN, "tft_metrics.npz"), pred=pred, tgt=tgt, ids=ids, means=means, scales=scales,
                        quantiles=np.array([0.1, 0.5, 0.9]), qrisk=criterions.qrisk(pred, tgt, np.array([0.1, 0.5, 0.9])),
                        per_id=unscale_per_id(ucfg, pred[:, :, 1], ids, scalers), one=unscale(ucfg, pred[:, :, 1], scalers[0]))

    # 6. a tiny checkpoint in the reference's form
    cfg = configuration.ElectricityConfig()
    cfg.hidden_size, cfg.example_length, cfg.encoder_length = 8, 6, 4
    model = modeling.TemporalFusionTransformer(cfg)
    dummy = {"s_cat": torch.zeros(1, 6, 1, dtype=torch.long), "k_cont": torch.zeros(1, 6, 3), "target": torch.zeros(1, 6, 1)}
    with torch.no_grad():
        model.eval()(dummy)
        probe = {"s_cat": torch.full((2, 6, 1), 7, dtype=torch.long), "k_cont": torch.linspace(-1, 1, 36).reshape(2, 6, 3),
                 "target": torch.linspace(1, -1, 12).reshape(2, 6, 1)}
        y = model(probe)
    torch.save({"config": cfg, "model": model.state_dict(), "probe_forecast": y}, os.path.join(GOLDEN, "tft_checkpoint.pt"))
    print("fixtures written to", GOLDEN)


if __name__ == "__main__":
    main()
