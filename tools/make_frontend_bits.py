"""Records tests/golden/frontend_bits.json: the SHA-256 of what every inference front end returns on the cases of
tests/_frontend_cases.py, on the GPU.  Run it from the commit whose behaviour is to be pinned, BEFORE the front ends are changed:

    python tools/make_frontend_bits.py [--out tests/golden/frontend_bits.json]

Every run (eager, and captured where the class has a `graphs` option) is made twice on freshly built front ends; a case whose
digests differ between the two, or between eager and captured, is reported and left out of the file, and the exit status is 1.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frontend_bits.json"))
    args = ap.parse_args(argv)
    from tests import _frontend_cases as FC
    out, bad = {}, []
    for name, (fn, has_graphs) in FC.CASES.items():
        got = [FC.digest(fn(g)) for g in ((False, True) if has_graphs else (False,)) for _ in range(2)]
        print(name, got, flush=True)
        if len(set(got)) == 1:
            out[name] = got[0]
        else:
            bad.append(name)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)%s" % (args.out, len(out), "; NOT reproducible: %s" % ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
