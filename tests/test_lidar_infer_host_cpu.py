"""Host side of the alive-ray LiDAR evaluation (csrc/lidar_infer.hip), no GPU needed: the three entry points are declared,
exported and bound with matching signatures; bad arguments are refused before any launch; the round schedule is the
documented one and bounds the loop."""
import ctypes as C
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lnh_lidar_march_rays", "lnh_lidar_composite_rays", "lnh_alive_compact")


def _prototypes():
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return dict(re.findall(r"LNH_API\s+int\s+(lnh_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S))


def test_entry_points_are_declared_exported_and_bound():
    from lidarnerf import _hip
    protos = _prototypes()
    lib = C.CDLL(_hip.lib_path())
    kinds = {"uint32_t": C.c_uint32, "int32_t": C.c_int, "int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64,
             "lnh_stream_t": C.c_void_p}
    for name in NAMES:
        assert name in protos, f"{name} is not declared in include/lidarnerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _hip._SIGS and name in _hip.EXPORTS
        want = []
        for arg in protos[name].split(","):
            a = " ".join(arg.split())
            want.append(C.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0].replace("const ", "").strip()])
        assert want[-1] is C.c_void_p and "lnh_stream_t" in protos[name].split(",")[-1]
        assert want == list(_hip._SIGS[name]) + [C.c_void_p], name
    # no bf16 twins: nothing in these three touches MLP element types (the header says so)
    assert not any(n + "_bf16" in protos or n + "_bf16" in _hip._SIGS for n in NAMES)
    header = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    assert "no _bf16" in header and "+inf" in header


def test_argument_errors_are_reported_without_a_gpu():
    from lidarnerf import _hip
    L = _hip.lib()
    p = 64  # any non-null value: validation never dereferences
    march = lambda **kw: L.lnh_lidar_march_rays(
        kw.get("n_alive", 4), kw.get("n_step", 8), kw.get("N", 4), p, p, kw.get("rays_t", p), kw.get("rays_steps", p), p, p, p,
        1.0, 0.0, kw.get("max_steps", 1024), kw.get("C", 1), 128, p, p, p, p, None, None)
    assert march(n_step=0) == -1 and b"n_step must be at least 1" in L.lnh_last_error()
    assert march(rays_t=None) == -1 and b"null ray state" in L.lnh_last_error()
    assert march(rays_steps=None) == -1 and b"null ray state" in L.lnh_last_error()
    assert march(C=0) == -1 and b"cascade" in L.lnh_last_error()
    assert march(n_alive=5) == -1 and b"n_alive_max must not exceed N" in L.lnh_last_error()
    assert march(N=0, n_alive=0) == 0                                        # nothing to do is not an error
    comp = lambda **kw: L.lnh_lidar_composite_rays(
        kw.get("n_alive", 4), kw.get("n_step", 8), 4, kw.get("K", 2), 1e-4, p, p, p, p, p, p, p, p, p, p, kw.get("ws", p),
        kw.get("depth", p), kw.get("image", p), kw.get("T", p), None)
    assert comp(n_step=0) == -1 and b"n_step must be at least 1" in L.lnh_last_error()
    assert comp(K=4) == -2 and b"K must be 1, 2 or 3 (got 4)" in L.lnh_last_error()
    assert comp(K=0) == -2
    for which in ("ws", "depth", "image", "T"):
        assert comp(**{which: None}) == -1 and b"null ray state" in L.lnh_last_error(), which
    assert comp(n_alive=0) == 0
    assert L.lnh_alive_compact(4, p, p, None, p, None) == -1 and b"null pointer" in L.lnh_last_error()
    assert L.lnh_alive_compact(4, p, p, p, None, None) == -1
    assert L.lnh_alive_compact(4, p, p + 64, p + 64, p + 128, None) == -1 and b"OTHER half" in L.lnh_last_error()


def test_round_schedule_and_its_bound():
    """n_step = n_step0 * (N // n_alive), between n_step0 = 32 and 128: the rows of a round never exceed the N * n_step0 the
    call allocated, n_step never falls below n_step0, and ceil(max_steps / n_step0) rounds are the worst case."""
    from lidarnerf import raymarching as rm
    assert (rm.ALIVE_N_STEP0, rm.ALIVE_N_STEP_MAX) == (32, 128)
    table = {4096: 32, 4095: 32, 2049: 32, 2048: 64, 1366: 64, 1365: 96, 1025: 96, 1024: 128, 600: 128, 100: 128, 1: 128}
    for n_alive, want in table.items():
        assert rm.alive_n_step(n_alive, 4096) == want, (n_alive, rm.alive_n_step(n_alive, 4096), want)
    assert rm.alive_n_step(0, 4096) == 32 and rm.alive_n_step(10, 0) == 32
    assert rm.alive_n_step(1, 4096, n_step0=8, n_step_max=32) == 32 and rm.alive_n_step(4096, 4096, 8, 32) == 8
    for N in (1, 7, 452, 4096, 460800):
        for n_alive in sorted({1, 2, 3, N // 3 + 1, N // 2, N // 2 + 1, N - 1, N} - {0}):
            if n_alive > N:
                continue
            s = rm.alive_n_step(n_alive, N)
            assert 32 <= s <= 128 and n_alive * s <= N * 32, (N, n_alive, s)
    assert rm.alive_max_rounds(1024) == 32 == math.ceil(1024 / 32)
    assert rm.alive_max_rounds(1000, 16) == 63 and rm.alive_max_rounds(40, 8) == 5
    # the loop of a ray that takes the smallest round every time and holds max_steps samples ends in exactly that many rounds
    steps, rounds = 0, 0
    while steps < 1024:
        steps += min(rm.alive_n_step(4096, 4096), 1024 - steps)
        rounds += 1
    assert rounds == rm.alive_max_rounds(1024)


def test_switch_defaults_to_the_existing_path():
    from lidarnerf.nerf.renderer import NeRFRenderer
    r = NeRFRenderer(cuda_ray=True)
    assert r.alive_march is False and r.alive_stats is None and hasattr(r, "run_cuda_alive")
    import inspect
    assert inspect.signature(r.run_cuda).parameters["alive_march"].default is None
