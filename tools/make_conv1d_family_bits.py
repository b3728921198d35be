"""Record tests/golden/conv1d_family_bits.json: the sha256 of every output of the cases in tests/_conv1d_family_cases.py (the four
conv1d-family entry points and the two normalise-and-pack entries, fp16 and bf16), computed by the library as it is built now.

Run it on the GPU with the library whose bits are the reference -- the commit BEFORE a change to csrc/conv1d_family.h or to one of
the kernels that use it -- and commit the file; tests/test_gpu_conv1d_family_bits.py then holds every later build to those bits.

    python tools/make_conv1d_family_bits.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv1d_family_bits.json"))
    args = ap.parse_args()
    from tests import _conv1d_family_cases as K
    rec = {dn: {name: K.digests(name, dt) for name in K.CASES} for dn, dt in K.DTYPES.items()}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d digests" % (args.out, sum(len(v) for d in rec.values() for v in d.values())))


if __name__ == "__main__":
    main()
