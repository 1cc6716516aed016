#!/usr/bin/env python3
"""Records what the built library answers to the host-only calls of tests/unet_host_cases.py (argument checks of every lnh_unet_*
entry point and every *_workspace_size function; no GPU needed) into tests/golden/unet_host.json.

    python tests/golden/make_unet_host.py <commit the library was built from>

The record is a statement about THAT commit: tests/test_unet_cpu.py holds later libraries to it, so it is regenerated only when a
change means to alter these answers, from a build of the commit before that change (LNH_LIB_PATH names such a library).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lidar-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import unet_host_cases as cases  # noqa: E402
from lidarnerf import _hip  # noqa: E402

if __name__ == "__main__":
    lib = _hip.lib()
    rec = {"recorded_from": {"commit": sys.argv[1], "lnh_version": lib.lnh_version()},
           "refusals": cases.refusal_answers(lib), "sizes": cases.size_answers(lib)}
    passed = [name for name, a in rec["refusals"].items() if a["rc"] != cases.INVALID_ARG]
    assert not passed, f"calls that were not refused (they must never be made on a machine with a GPU): {passed}"
    out = os.path.join(HERE, "unet_host.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rec['refusals'])} refused calls, {len(rec['sizes'])} size answers")
