"""Host-side behaviour of the grid encoder's bucketed backward that needs no device: the workspace plan functions and the
argument checks of the five lnh_grid_encode_backward_ws* entry points.  One table of calls, used twice: by
tests/golden/make_grid_host.py, which records what a library answers into tests/golden/grid_host.json, and by
tests/test_host_cpu.py, which compares the library under test with that record.  Every call here returns before the first
HIP call (B == 0, an argument the entry point rejects, or a workspace too small for the batch), so the pointers are never
dereferenced."""
import ctypes

import numpy as np

F32, F16 = 0, 1
PTR = 1  # any non-null address


def offsets(log2_hashmap_size=19, gridtype=0, align=0, levels=16):
    from lidarnerf.gridencoder.grid import level_offsets
    pls = np.exp2(np.log2(32768 / 16) / 15)
    off = level_offsets(3, levels, pls, 16, log2_hashmap_size, bool(align), "tcnn" if gridtype == 2 else "hash")
    return off, float(np.float32(np.log2(pls)))


# name -> (log2_hashmap_size, gridtype, align_corners)
CONFIGS = {"hash": (19, 0, 0), "tcnn": (19, 2, 0), "tiled": (19, 1, 0), "align": (19, 0, 1), "hash_log2_20": (20, 0, 0)}
BATCHES = (1024, 4096 * 832, 16384 * 832, 5_000_000)  # the last two are walked in chunks


def _set_error_sentinel(lib):
    """A call that succeeds must leave lnh_last_error() alone: give it a known text to leave."""
    assert lib.lnh_sh_encode_forward(1, 1, 4, 3, 9, None, None) != 0
    return lib.lnh_last_error().decode()


def _plan_answers(lib, off, geo, dtype):
    """geo = (B, D, C, L, S, H, gridtype, align): what the four plan functions say about it."""
    p = off.ctypes.data if off is not None else None
    full = int(lib.lnh_grid_backward_workspace_size(p, *geo, dtype))
    least = int(lib.lnh_grid_backward_workspace_size_min(p, *geo, dtype))
    out = {"size": full, "size_min": least, "clear_bytes": {}, "plan_info": {}}
    for interp in (0, 1):
        for what, nbytes in (("full", full), ("min", least), ("below_min", max(least, 1) - 1)):
            out["clear_bytes"][f"interp{interp}_{what}"] = int(
                lib.lnh_grid_backward_workspace_clear_bytes(p, *geo, interp, dtype, nbytes))
    for level in (0, 5, 15):
        out4 = (ctypes.c_uint32 * 4)(0xdead, 0xdead, 0xdead, 0xdead)
        _set_error_sentinel(lib)
        rc = lib.lnh_grid_backward_plan_info(p, *geo, dtype, level, ctypes.cast(out4, ctypes.c_void_p))
        out["plan_info"][str(level)] = {"rc": rc, "out4": list(out4), "error": lib.lnh_last_error().decode()}
    return out


def plan_answers(lib):
    """{case name: answers} for the table of configurations, and for the arguments each function answers with 0."""
    res = {}
    for name, (log2h, gridtype, align) in CONFIGS.items():
        off, S = offsets(log2h, gridtype, align)
        for dtype in (F32, F16):
            for B in BATCHES:
                res[f"{name}/dtype{dtype}/B{B}"] = _plan_answers(lib, off, (B, 3, 2, 16, S, 16, gridtype, align), dtype)
    off, S = offsets()
    odd = {"B0": (0, 3, 2, 16, S, 16, 0, 0), "D2": (4096, 2, 2, 16, S, 16, 0, 0), "C4": (4096, 3, 4, 16, S, 16, 0, 0),
           "L0": (4096, 3, 2, 0, S, 16, 0, 0), "L33": (4096, 3, 2, 33, S, 16, 0, 0),
           "gridtype3": (4096, 3, 2, 16, S, 16, 3, 0), "tcnn_align": (4096, 3, 2, 16, S, 16, 2, 1)}
    for name, geo in odd.items():
        res[f"odd/{name}"] = _plan_answers(lib, off, geo, F16)
    res["odd/dtype7"] = _plan_answers(lib, off, (4096, 3, 2, 16, S, 16, 0, 0), 7)
    res["odd/null_offsets"] = _plan_answers(lib, None, (4096, 3, 2, 16, S, 16, 0, 0), F16)
    return res


ENTRY_POINTS = ("lnh_grid_encode_backward_ws", "lnh_grid_encode_backward_ws_levels", "lnh_grid_encode_backward_ws_begin",
                "lnh_grid_encode_backward_ws_finish", "lnh_grid_encode_backward_ws_ex")


def ws_calls():
    """[(case name, entry point, argument dict)].  The defaults are a valid call with B == 0."""
    base = dict(grad=PTR, inputs=PTR, ge=PTR, B=0, D=3, C=2, L=16, gridtype=0, align=0, interp=0, dtype=F16, lb=0, le=16,
                split=0, flags=0, ws=PTR, ws_bytes=1 << 20)
    wrong = {
        "B0": {},
        "null_grad": dict(grad=None),
        "null_grad_embeddings": dict(ge=None),
        "null_inputs": dict(inputs=None),
        "D2": dict(D=2),
        "C4": dict(C=4),
        "L0": dict(L=0, le=0),
        "L33": dict(L=33, le=33),
        "bad_dtype": dict(dtype=7),
        "gridtype3": dict(gridtype=3, B=4096),          # build_meta's refusals come after the B == 0 return
        "gridtype3_B0": dict(gridtype=3),
        "tcnn_align": dict(gridtype=2, align=1, B=4096),
        "begin_gt_end": dict(lb=9, le=8),
        "end_L_plus_1": dict(le=17),
        "empty_window": dict(lb=5, le=5, B=4096),       # nothing to do: returns before the plan
        "workspace_too_small": dict(B=4096),            # 1 MiB: refused by host arithmetic alone
        "null_workspace": dict(B=4096, ws=None, ws_bytes=1 << 40),
        # wrong in two ways: which check speaks first
        "null_grad+D2": dict(grad=None, D=2),
        "D2+end_L_plus_1": dict(D=2, le=17),
        "gridtype3+begin_gt_end": dict(gridtype=3, B=4096, lb=9, le=8),
        "L33+null_grad": dict(L=33, le=33, grad=None),
    }
    ex_only = {
        "split3": dict(split=3),
        "flags4": dict(flags=4),
        "split1_B0": dict(split=1, flags=3),
        "split2_B0": dict(split=2, lb=8, le=12),
        "split1_begin_gt_end": dict(split=1, lb=9, le=8),  # the window is validated before split 1 overrides it
        "split3+null_grad": dict(split=3, grad=None),
        "flags4+L0": dict(flags=4, L=0, le=0),
    }
    calls = []
    for fn in ENTRY_POINTS:
        for name, delta in list(wrong.items()) + (list(ex_only.items()) if fn.endswith("_ex") else []):
            calls.append((f"{fn}/{name}", fn, dict(base, **delta)))
    return calls


def ws_answers(lib):
    off, S = offsets()
    res = {}
    for name, fn, a in ws_calls():
        args = [a["grad"], a["inputs"], off.ctypes.data, a["ge"], a["B"], a["D"], a["C"], a["L"], S, 16, a["gridtype"],
                a["align"], a["interp"], a["dtype"], a["ws"], a["ws_bytes"]]
        if fn.endswith(("_levels", "_finish", "_ex")):
            args += [a["lb"], a["le"]]
        if fn.endswith("_ex"):
            args += [a["split"], a["flags"]]
        _set_error_sentinel(lib)
        rc = getattr(lib, fn)(*args, None)
        res[name] = {"rc": rc, "error": lib.lnh_last_error().decode()}
    return res
