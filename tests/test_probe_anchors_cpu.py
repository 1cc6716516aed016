"""tools/probe_variants.py patches the product sources by text anchor: every anchor of every variant must occur exactly once
in the file the variant names, or the variant cannot be built (no compile here: the sources are only read)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-nerf_amd", "csrc")


def _probe_variants():
    spec = importlib.util.spec_from_file_location("probe_variants", os.path.join(ROOT, "tools", "probe_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SETS = _probe_variants().SETS


@pytest.mark.parametrize("set_name", sorted(SETS))
def test_probe_anchors_occur_once(set_name):
    assert SETS[set_name], f"set {set_name} has no variant"
    for name, (fname, subs) in SETS[set_name].items():
        path = os.path.join(CSRC, fname)
        assert os.path.isfile(path), f"{set_name}/{name}: no such file csrc/{fname}"
        text = open(path).read()
        for old, new in subs:
            # (build_variant applies the substitutions in order: an anchor must still be there after the earlier ones)
            assert text.count(old) == 1, f"{set_name}/{name}: anchor found {text.count(old)} times in {fname}:\n{old[:160]}"
            text = text.replace(old, new)
