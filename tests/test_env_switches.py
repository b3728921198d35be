"""The environment switches of csrc/ and the table of DESIGN.md (section 0.0) list the same names (no compute, CPU ok)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeplearningexamples_amd", "csrc")


def _read_by_source():
    """Every name handed to dle_env_int (common.h; the per-call reader dle_gemm_expand_enabled of gemm_family.h goes through it
    too), and no other way into the environment: getenv appears once, inside dle_env_int (rccl_comm.hip aside)."""
    names, getenv_sites = set(), []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(CSRC, f)).read()
        names.update(re.findall(r'dle_env_int\("([A-Z0-9_]+)"', src))
        code = re.sub(r"//[^\n]*", "", src)
        if f != "rccl_comm.hip":
            getenv_sites += [f] * len(re.findall(r"\bgetenv\s*\(", code))
        # a call with anything but a literal name would escape the scan
        assert len(re.findall(r"\bdle_env_int\s*\(", code)) == len(re.findall(r'\bdle_env_int\s*\(\s*"', code)) + (f == "common.h"), f
    return names, getenv_sites


def _listed_in_design():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = doc.index("### 0.0 Environment switches of the library")
    sec = doc[start:doc.index("\n### ", start + 1)]
    return set(re.findall(r"^\| `(DLE_[A-Z0-9_]+)` \|", sec, re.M))


def test_env_switches_match_design_table():
    names, getenv_sites = _read_by_source()
    assert getenv_sites == ["common.h"], getenv_sites
    assert "DLE_GEMM_EXPAND" in names and len(names) >= 10
    assert all(n.startswith("DLE_") for n in names), sorted(names)
    listed = _listed_in_design()
    assert names - listed == set(), "read by csrc/ but missing from DESIGN.md's table: %s" % sorted(names - listed)
    assert listed - names == set(), "listed in DESIGN.md but read nowhere in csrc/: %s" % sorted(listed - names)
