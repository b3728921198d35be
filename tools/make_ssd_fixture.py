"""Write the SSD300 fixtures from the reference's own modules (Detection/SSD/ssd/model.py, ssd/utils.py, main.py), on the CPU:

  tests/golden/ssd_state_dict.json   names and shapes of the reference SSD300's state dict, in state_dict() order;
  tests/golden/ssd_cli_flags.json    the option strings of the reference parser (main.py:53-127) with the number of values each takes;
  tests/golden/ssd_decode.npz        the reference's dboxes300_coco() in both orders; its DefaultBoxes on the tiny pyramid
                                     (tests/_ssd_ref.TINY) in both orders; the outputs of the reference's own Encoder.decode_batch
                                     (fp32, CPU) for the seeded inputs tests/_ssd_ref.case_inputs rebuilds -- the full SSD300
                                     geometry (81 labels) and the tiny pyramid (5 labels), N = 2 each, at criteria 0.45 and 0.5
                                     with max_output 200 and 20: per image the boxes, labels and scores in the reference's
                                     (ascending-score) order.  The inputs are not stored.

torchvision is not installed: `torchvision`, `torchvision.transforms` and `torchvision.models.resnet` are stubbed, the last with the
small torchvision-shaped ResNet-50 of tests/_ssd_ref.py.  So the BACKBONE inside the recorded reference model is this project's
stand-in (its key spelling follows from model.py:42-48 and torchvision's published module names); the heads, the additional layers,
bbox_view, the default boxes and the decode are the reference's.

    python tools/make_ssd_fixture.py            (needs the reference tree: DLE_REFERENCE)
"""
import ast
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

CASES = [(0.45, 200), (0.5, 200), (0.45, 20), (0.5, 20)]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def reference_root():
    from oracle._ref_import import REF
    return os.path.join(REF, "PyTorch", "Detection", "SSD")


def import_reference():
    """(ssd.utils, ssd.model) of the reference, with the torchvision stubs in place for the import only."""
    from tests import _ssd_ref as R
    root = reference_root()
    mine = lambda k: k.split(".")[0] in ("ssd", "torchvision")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if mine(k)}
    sys.path.insert(0, root)
    try:
        tr = _stub("torchvision.transforms")
        rn = _stub("torchvision.models.resnet", **{n: R.resnet50 for n in ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")})
        _stub("torchvision", transforms=tr, models=_stub("torchvision.models", resnet=rn))
        return importlib.import_module("ssd.utils"), importlib.import_module("ssd.model")
    finally:
        sys.path.remove(root)
        for k in [k for k in sys.modules if mine(k)]:
            del sys.modules[k]
        sys.modules.update(saved)


def parser_flags():
    """make_parser of the reference's main.py, compiled ALONE (the module imports DALI, dllogger and the training loops)."""
    path = os.path.join(reference_root(), "main.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "make_parser"]
    import argparse
    ns = {"ArgumentParser": argparse.ArgumentParser, "os": os}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    out = []
    for a in ns["make_parser"]()._actions:
        if a.option_strings and a.dest != "help":
            nvals = 0 if a.nargs == 0 else ("*" if a.nargs == "*" else 1)
            out.append(dict(flags=list(a.option_strings), values=nvals, required=bool(a.required), choices=list(a.choices or [])))
    return out


def record(arrays, prefix, utils, dboxes, ploc, plabel):
    enc = utils.Encoder(dboxes)
    for criteria, max_output in CASES:
        with torch.no_grad():
            res = enc.decode_batch(torch.from_numpy(ploc).clone(), torch.from_numpy(plabel).clone(), criteria, max_output)
        for i, (bb, ll, ss) in enumerate(res):
            key = "%s_c%d_m%d_i%d" % (prefix, round(criteria * 100), max_output, i)
            arrays[key + "_boxes"] = bb.numpy().astype(np.float32).reshape(-1, 4)
            arrays[key + "_labels"] = ll.numpy().astype(np.int64)
            arrays[key + "_scores"] = ss.numpy().astype(np.float32)
            print("%s: %d detections" % (key, len(ll)))


def main():
    from tests import _ssd_ref as R
    utils, model = import_reference()
    golden = os.path.join(ROOT, "tests", "golden")
    torch.manual_seed(0)
    shapes = {k: list(v.shape) for k, v in model.SSD300().state_dict().items()}
    path = os.path.join(golden, "ssd_state_dict.json")
    with open(path, "w") as f:
        json.dump(shapes, f, indent=0)
        f.write("\n")
    print("wrote", path)

    path = os.path.join(golden, "ssd_cli_flags.json")
    with open(path, "w") as f:
        json.dump(parser_flags(), f, indent=0)
        f.write("\n")
    print("wrote", path)

    arrays = {}
    full = utils.dboxes300_coco()
    tiny = utils.DefaultBoxes(R.TINY["fig_size"], R.TINY["feat_size"], R.TINY["steps"], R.TINY["scales"], R.TINY["aspect_ratios"])
    for name, d in (("full", full), ("tiny", tiny)):
        arrays[name + "_dboxes_ltrb"] = d(order="ltrb").numpy()
        arrays[name + "_dboxes_xywh"] = d(order="xywh").numpy()
    arrays["scale_xy_wh"] = np.asarray([full.scale_xy, full.scale_wh], dtype=np.float64)
    record(arrays, "full", utils, full, *R.case_inputs(arrays["full_dboxes_xywh"], 2, 81, R.FULL_SEED, big_class=True))
    record(arrays, "tiny", utils, tiny, *R.case_inputs(arrays["tiny_dboxes_xywh"], 2, R.TINY_LABELS, R.TINY_SEED, big_class=False))
    path = os.path.join(golden, "ssd_decode.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
