"""Record tests/golden/rowtile_family_bits.json: the sha256 of every output of the cases in tests/_rowtile_family_cases.py (the TFT,
NCF and MoFlow entry points and the four kernels that only take the index map from csrc/mfma32_rows.h, fp16 and bf16), computed by
the library as it is built now.  Every case is computed twice and must give the same bytes both times.

Run it on the GPU with the library whose bits are the reference -- the commit BEFORE a change to csrc/mfma32_rows.h or to one of
the kernels that use it -- and commit the file; tests/test_gpu_rowtile_family_bits.py then holds every later build to those bits.

    python tools/make_rowtile_family_bits.py [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rowtile_family_bits.json"))
    args = ap.parse_args()
    from tests import _rowtile_family_cases as K
    rec = {dn: {name: K.digests(name, dt) for name in K.CASES} for dn, dt in K.DTYPES.items()}
    again = {dn: {name: K.digests(name, dt) for name in K.CASES} for dn, dt in K.DTYPES.items()}
    moved = sorted("%s/%s" % (dn, name) for dn in rec for name in rec[dn] if rec[dn][name] != again[dn][name])
    if moved:
        sys.exit("not reproducible run to run, nothing written: %s" % ", ".join(moved))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d digests, each computed twice" % (args.out, sum(len(v) for d in rec.values() for v in d.values())))


if __name__ == "__main__":
    main()
