"""The dynamic-LDS opt-in and the device-limit queries live in csrc/common.h only (DLE_LAUNCH_LDS, dle_device_limits): no launcher
keeps a guard or a device cache of its own (no GPU needed)."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deeplearningexamples_amd", "csrc")


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert any(p.endswith("common.h") for p in paths)
    return {os.path.basename(p): open(p).read() for p in paths}


def test_attribute_calls_only_in_common_h():
    for name, src in _sources().items():
        if name == "common.h":
            continue
        for api in ("hipFuncSetAttribute", "hipDeviceGetAttribute"):
            assert api not in src, "%s calls %s: use DLE_LAUNCH_LDS / dle_device_limits (common.h)" % (name, api)


def test_no_per_site_guards_left():
    for name, src in _sources().items():
        assert not re.search(r"\battr_set\b", src), "%s keeps an attr_set guard" % name
