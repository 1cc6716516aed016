#!/usr/bin/env python3
"""Records what the built library answers to the host-only calls of tests/grid_host_cases.py (workspace plan functions and
argument checks of the bucketed grid backward; no GPU needed) into tests/golden/grid_host.json.

    python tests/golden/make_grid_host.py <commit the library was built from>

The record is a statement about THAT commit: tests/test_host_cpu.py holds later libraries to it, so it is regenerated only
when a change means to alter these answers, from a build of the commit before that change.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lidar-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import grid_host_cases as cases  # noqa: E402
from lidarnerf import _hip  # noqa: E402

if __name__ == "__main__":
    lib = _hip.lib()
    rec = {"recorded_from": {"commit": sys.argv[1], "lnh_version": lib.lnh_version()},
           "plan": cases.plan_answers(lib), "ws": cases.ws_answers(lib)}
    out = os.path.join(HERE, "grid_host.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rec['plan'])} plan cases, {len(rec['ws'])} calls")
