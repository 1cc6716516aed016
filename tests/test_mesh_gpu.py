"""Mesh export on the device (csrc/mesh.hip, lidarnerf/nerf/mesh.py, LidarTrainer.save_mesh) against the NumPy restatement of
its output contract (tests/marching_cubes_ref.py).

Counts, triangles and vertices are compared BIT FOR BIT: the only rounded operations are iso - va, vb - va, their quotient
and float(i) + t, each one IEEE fp32 operation on both sides (hipcc's fp32 division is correctly rounded at the library's
flags, nothing is contracted: -ffp-contract=off).  No tolerance is used anywhere in this file."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import marching_cubes_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5ca1ab1e
# csrc/mesh.hip: one workgroup holds kMcThreads = 256 lattice points, and k_mc_scan scans the workgroup totals in tiles of
# kScanTile (csrc/scan.h) = 1024 threads x 4 = 4096 totals: a volume of more than 4096 * 256 = 1 048 576 samples needs a second tile.
MC_THREADS = 256


def _scan_tile():
    text = open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "scan.h")).read()
    m = re.search(r"kScanThreads = (\d+), kScanPerThread = (\d+), kScanTile = kScanThreads \* kScanPerThread;", text)
    return int(m.group(1)) * int(m.group(2))


MC_SCAN_TILE = _scan_tile()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _raw(vol, iso, max_v=None, max_t=None):
    """count + emit through the C ABI with guard words behind both outputs; capacities default to the counts."""
    from lidarnerf import _hip
    L = _hip.lib()
    d = torch.tensor(np.asarray(vol, np.float32)).cuda()
    nx, ny, nz = d.shape
    need = int(L.lnh_marching_cubes_workspace_size(nx, ny, nz))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    _hip.call("lnh_marching_cubes_count", d.data_ptr(), nx, ny, nz, float(iso), ws.data_ptr(), need, counts.data_ptr())
    V, T, bad, zero = counts.tolist()
    cap_v, cap_t = (V if max_v is None else max_v), (T if max_t is None else max_t)
    guard = 16
    vbuf = torch.full((cap_v * 3 + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    tbuf = torch.full((cap_t * 3 + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    if cap_v and cap_t:
        _hip.call("lnh_marching_cubes_emit", d.data_ptr(), nx, ny, nz, float(iso), ws.data_ptr(), need, vbuf.data_ptr(), cap_v,
                  tbuf.data_ptr(), cap_t)
    torch.cuda.synchronize()
    vbuf, tbuf = vbuf.cpu().numpy(), tbuf.cpu().numpy()
    assert (vbuf[cap_v * 3:] == SENTINEL).all() and (tbuf[cap_t * 3:] == SENTINEL).all(), "guard words overwritten"
    return (V, T, bad, zero), vbuf[:cap_v * 3].view(np.float32).reshape(-1, 3), tbuf[:cap_t * 3].reshape(-1, 3)


def _random(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32), np.float32(0.1)


def _quarters(shape=(9, 10, 11), seed=3):
    """Multiples of 0.25 with iso = 0.25: many samples EQUAL iso (not below), and quotients such as 1/3 that must round."""
    vol = np.random.default_rng(seed).integers(-4, 6, size=shape).astype(np.float32) * np.float32(0.25)
    assert (vol == 0.25).sum() > 50
    return vol, np.float32(0.25)


def _past_one_scan_tile():
    shape = (130, 101, 101)
    groups = -(-shape[0] * shape[1] * shape[2] // MC_THREADS)
    assert groups > MC_SCAN_TILE + 1000
    # a sphere across the lattice points 4096 * 256 (x = 102.8): surface on both sides of the tile boundary
    return ref.sphere_volume(shape, 20.3, centre=(104.2, 50.1, 49.7))


VOLUMES = {
    "cases_64x64x4": ref.case_volume,
    "2x2x2": lambda: _random((2, 2, 2), 1),
    "2x2x9": lambda: _random((2, 2, 9), 2),
    "5x7x9": lambda: _random((5, 7, 9), 3),
    "13x11x19": lambda: _random((13, 11, 19), 4),  # 2717 points: 11 workgroups, the last one partial
    "iso_equals_samples": _quarters,
    "past_one_scan_tile": _past_one_scan_tile,
}


@functools.lru_cache(maxsize=None)
def _volume_and_reference(name):
    vol, iso = VOLUMES[name]()
    v, t, counts = ref.marching_cubes(vol, iso)
    for a in (vol, v, t):
        a.setflags(write=False)
    return vol, iso, v, t, counts


@pytest.mark.parametrize("name", list(VOLUMES))
def test_counts_triangles_and_vertices_match_the_restatement_bit_for_bit(name):
    vol, iso, want_v, want_t, want_counts = _volume_and_reference(name)
    assert want_counts[0] > 0 and want_counts[1] > 0, "the volume must hold a surface"
    counts, v, t = _raw(vol, iso)
    assert counts == want_counts
    assert np.array_equal(t, want_t)
    diff = _bits(v) != _bits(want_v)
    print(f"{name}: V {counts[0]}, T {counts[1]}; vertex words that differ from the restatement: {int(diff.sum())}")
    assert not diff.any(), (name, np.argwhere(diff)[:5])
    if name == "past_one_scan_tile":
        first_late = np.searchsorted(np.ravel_multi_index(np.floor(want_v).astype(np.int64).T, vol.shape),
                                     MC_SCAN_TILE * MC_THREADS)
        assert 0 < first_late < len(want_v)  # vertices on both sides of the scan's tile boundary
        assert ref.open_edges(t) == [] and ref.euler_characteristic(len(v), t) == 2
    # the Python function: exact allocation, the same arrays
    from lidarnerf.nerf import mesh
    pv, pt = mesh.marching_cubes(torch.tensor(vol).cuda(), float(iso))
    assert pv.is_cuda and pv.dtype == torch.float32 and pt.dtype == torch.int32
    assert pv.shape == (want_counts[0], 3) and pt.shape == (want_counts[1], 3)
    assert np.array_equal(_bits(pv.cpu().numpy()), _bits(want_v)) and np.array_equal(pt.cpu().numpy(), want_t)


def test_no_surface_gives_an_empty_mesh():
    from lidarnerf.nerf import mesh
    for fill, iso in ((0.0, 1.0), (2.0, 1.0), (1.0, 1.0)):  # all below, all not below, all EQUAL to iso (not below)
        vol = np.full((7, 6, 5), fill, np.float32)
        counts, v, t = _raw(vol, iso)
        assert counts == (0, 0, 0, 0)
        pv, pt = mesh.marching_cubes(torch.tensor(vol).cuda(), iso)
        assert pv.shape == (0, 3) and pt.shape == (0, 3) and pv.is_cuda and pt.dtype == torch.int32


def test_a_planted_nan_is_counted_and_refused():
    from lidarnerf.nerf import mesh
    vol, iso, *_ = _volume_and_reference("5x7x9")
    vol = vol.copy()
    vol[2, 3, 4] = np.nan
    want = ref.marching_cubes(vol, iso)
    counts, v, t = _raw(vol, iso)
    assert counts[2] == 1 and counts == want[2]
    assert np.array_equal(t, want[1])  # (a NaN is not below: the mesh is still defined, its NaN-edge vertices are NaN)
    vol[0, 0, 0] = np.inf
    assert _raw(vol, iso)[0][2] == 2
    with pytest.raises(RuntimeError, match="not finite"):
        mesh.marching_cubes(torch.tensor(vol).cuda(), float(iso))


def test_two_calls_are_bit_identical():
    from lidarnerf.nerf import mesh
    for name in ("13x11x19", "past_one_scan_tile"):
        vol, iso, *_ = _volume_and_reference(name)
        d = torch.tensor(vol).cuda()
        a, b = mesh.marching_cubes(d, float(iso)), mesh.marching_cubes(d, float(iso))
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_capacities_one_short_leave_the_guard_words_alone():
    vol, iso, want_v, want_t, (V, T, _, _) = _volume_and_reference("13x11x19")
    counts, v, t = _raw(vol, iso, max_v=V - 1, max_t=T - 1)  # (_raw asserts the guard words)
    assert counts[:2] == (V, T)
    assert np.array_equal(_bits(v), _bits(want_v[:V - 1])) and np.array_equal(t, want_t[:T - 1])
    counts, v, t = _raw(vol, iso, max_v=1, max_t=1)
    assert np.array_equal(_bits(v), _bits(want_v[:1])) and np.array_equal(t, want_t[:1])


# ------------------------------------------------------------------------------------------------- the density volume
SCALE = 0.010784853507573345


@functools.lru_cache(maxsize=None)
def _small_model():
    """The small occupancy-free NeRFNetwork of the other GPU tests (tests/test_sampler_gpu.py), its table spread out."""
    from lidarnerf.nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(encoding="hashgrid", desired_resolution=2048, bound=1, min_near=SCALE, min_near_lidar=SCALE)
    with torch.no_grad():
        net.encoder.embeddings.uniform_(-0.5, 0.5)
    return net.cuda().eval()


def _lattice(model, R):
    lo_hi = model.aabb_infer.cpu().tolist()
    axes = [torch.linspace(lo_hi[a], lo_hi[3 + a], R) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).cuda()


def test_density_volume_equals_model_density_on_the_lattice():
    from lidarnerf.nerf import mesh
    model, R = _small_model(), 20
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want = model.density(_lattice(model, R))["sigma"].float().reshape(R, R, R)
    chunked = mesh.density_volume(model, R, S=8)  # chunks of 8 + 8 + 4 per axis
    whole = mesh.density_volume(model, R, S=20)
    assert chunked.is_cuda and chunked.dtype == torch.float32 and chunked.shape == (R, R, R) and not chunked.requires_grad
    assert torch.equal(chunked.view(torch.int32), want.view(torch.int32))
    assert torch.equal(chunked.view(torch.int32), whole.view(torch.int32))
    assert torch.equal(mesh.density_volume(model, R).view(torch.int32), whole.view(torch.int32))  # S = 128: one chunk
    assert float(chunked.std()) > 0 and bool(torch.isfinite(chunked).all())
    fp32 = mesh.density_volume(model, R, S=8, fp16=False)
    with torch.no_grad():
        want32 = model.density(_lattice(model, R))["sigma"].reshape(R, R, R)
    assert torch.equal(fp32.view(torch.int32), want32.view(torch.int32)) and not torch.equal(fp32, chunked)


def test_extract_geometry_equals_the_restatement_on_the_same_volume():
    from lidarnerf.nerf import mesh
    model, R = _small_model(), 20

    def query_func(pts):
        assert pts.is_cuda and pts.shape[1] == 3
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return model.density(pts)["sigma"]

    b_min, b_max = model.aabb_infer[:3], model.aabb_infer[3:]
    u = mesh.extract_fields(b_min, b_max, R, query_func)
    assert isinstance(u, np.ndarray) and u.dtype == np.float32 and u.shape == (R, R, R)
    assert np.array_equal(_bits(u), _bits(mesh.density_volume(model, R).cpu().numpy()))
    threshold = float(np.median(u))
    vertices, triangles = mesh.extract_geometry(b_min, b_max, R, threshold, query_func)
    want_v, want_t, counts = ref.marching_cubes(u, threshold)
    assert counts[0] > 100
    lo, hi = b_min.cpu().numpy(), b_max.cpu().numpy()
    want_world = want_v.astype(np.float64) / (R - 1.0) * (hi - lo)[None, :] + lo[None, :]
    assert isinstance(vertices, np.ndarray) and vertices.dtype == np.float64 and triangles.dtype == np.int32
    assert np.array_equal(vertices, want_world) and np.array_equal(triangles, want_t)
    assert vertices.min() >= -1 and vertices.max() <= 1


# ----------------------------------------------------------------------------------------------------------- the trainer
RENDER = dict(num_steps=768, upsample_steps=64)
MESH_R = 24


def _trainer(graph=False, rays=1024, **kw):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph, render_kwargs=RENDER, **kw)
    assert tr.table is not None and tr.graph == graph
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, rays, 0, dev, (1, 1), "analytic") for s in range(8)]
    return tr, model, batches


def _median_threshold(tr, ema=False):
    """A threshold from the volume's own median, so that the surface is not empty."""
    import contextlib
    from lidarnerf.nerf import mesh
    with (tr.ema_weights() if ema else contextlib.nullcontext()):
        u = mesh.density_volume(tr.model, MESH_R, fp16=tr.fp16)
    return float(u.median()), u


def _world(tr, v):
    box = tr.model.aabb_infer.cpu().numpy()
    return (v.astype(np.float64) / (MESH_R - 1.0) * (box[3:] - box[:3])[None, :] + box[:3][None, :]).astype(np.float32)


def test_save_mesh_writes_the_mesh_of_the_volume(tmp_path):
    from lidarnerf.nerf import mesh
    tr, model, batches = _trainer()
    torch.manual_seed(11)
    for s in range(4):
        tr.step(*batches[s])
    threshold, u = _median_threshold(tr)
    path = os.path.join(tmp_path, "meshes", "deep", "scene.ply")  # the directories do not exist yet
    was_training = model.training
    n_v, n_t = tr.save_mesh(path, resolution=MESH_R, threshold=threshold)
    assert model.training == was_training and n_v > 0 and n_t > 0
    v, t = mesh.marching_cubes(u, threshold)
    assert (n_v, n_t) == (v.shape[0], t.shape[0])
    got_v, got_t = ref.read_ply(path)
    assert np.array_equal(_bits(got_v), _bits(_world(tr, v.cpu().numpy()))) and np.array_equal(got_t, t.cpu().numpy())
    assert tr.save_mesh(os.path.join(tmp_path, "empty.ply"), resolution=MESH_R, threshold=float(u.max()) * 2 + 1) == (0, 0)
    assert ref.read_ply(os.path.join(tmp_path, "empty.ply"))[0].shape == (0, 3)


def _train(graph, with_mesh, tmp_path):
    tr, model, batches = _trainer(graph=graph)
    torch.manual_seed(11)
    losses = []
    for s in range(20):
        losses.append(tr.step(*batches[s % 8]).detach().clone())
        if with_mesh and s + 1 == 10:
            captured = (len(tr.capture_ms), len(tr._graphs)) if graph else None
            ptrs = (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
            threshold, _ = _median_threshold(tr)
            assert tr.save_mesh(os.path.join(tmp_path, f"mid_{graph}.ply"), resolution=MESH_R, threshold=threshold)[0] > 0
            assert ptrs == (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
    torch.cuda.synchronize()
    if graph:
        assert tr.graph and tr.graph_error is None
        if with_mesh:
            assert captured == (len(tr.capture_ms), len(tr._graphs))  # nothing was captured again after the mesh
    state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
    return state + [p.detach().clone() for p in tr.small] + [torch.stack(losses)]


@pytest.mark.parametrize("graph", [False, True])
def test_training_does_not_notice_a_save_mesh(graph, tmp_path):
    """Twenty steps from one seed with a save_mesh after the tenth against twenty without: table, fp16 copy, Adam moments,
    optimizer scalars, every MLP matrix and all losses bit for bit — launch by launch and as a captured step."""
    a = _train(graph, False, tmp_path)
    b = _train(graph, True, tmp_path)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i
    assert torch.isfinite(a[-1]).all()


def test_save_mesh_with_an_ema_meshes_the_averaged_weights(tmp_path):
    from lidarnerf.nerf import mesh
    tr, model, batches = _trainer(ema_decay=0.95, ema_interval=2)
    torch.manual_seed(11)
    for s in range(6):
        tr.step(*batches[s])
    assert tr.ema.num_updates == 3
    live = [p.detach().clone() for p in model.parameters()]
    threshold, u_ema = _median_threshold(tr, ema=True)
    _, u_live = _median_threshold(tr, ema=False)
    assert not torch.equal(u_ema, u_live)
    averaged, own = os.path.join(tmp_path, "ema.ply"), os.path.join(tmp_path, "live.ply")
    n_ema = tr.save_mesh(averaged, resolution=MESH_R, threshold=threshold)  # ema=True is the default
    n_live = tr.save_mesh(own, resolution=MESH_R, threshold=threshold, ema=False)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), live)) and not hasattr(tr.table, "_lnh_ema_weights")
    for path, u, n in ((averaged, u_ema, n_ema), (own, u_live, n_live)):
        v, t = mesh.marching_cubes(u, threshold)
        got_v, got_t = ref.read_ply(path)
        assert n == (v.shape[0], t.shape[0]) and n[0] > 0
        assert np.array_equal(_bits(got_v), _bits(_world(tr, v.cpu().numpy()))) and np.array_equal(got_t, t.cpu().numpy())
    assert open(averaged, "rb").read() != open(own, "rb").read()
