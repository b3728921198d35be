"""Write tests/golden/resnext_state_dict.json: the state-dict names and shapes (nothing else) of the reference's own
resnext101-32x4d and se-resnext101-32x4d model classes (Classification/ConvNets/image_classification/models/resnet.py:412-458),
built on the CPU through the reference import helper.  tests/test_resnext_host.py compares convnets/resnext.py against it.

    python tools/make_resnext_state_dict_fixture.py        (needs the reference tree: DLE_REFERENCE)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARCHS = ("resnext101-32x4d", "se-resnext101-32x4d")


def reference_names_and_shapes():
    """{arch: {state-dict name: shape}} from the reference's model classes."""
    from oracle import _ref_import as R
    models = R.import_convnets().models
    out = {}
    for arch in ARCHS:
        entry = getattr(models, arch.replace("-", "_"))
        model = entry(pretrained=False)
        out[arch] = {k: list(v.shape) for k, v in model.state_dict().items()}
    return out


def main():
    path = os.path.join(ROOT, "tests", "golden", "resnext_state_dict.json")
    with open(path, "w") as f:
        json.dump(reference_names_and_shapes(), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
