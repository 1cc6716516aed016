"""Device-side batch sampler, the part that needs no GPU: the NumPy restatement against the published Philox known answer
and against rays.patch_indices' arithmetic, every argument refusal of the two C entry points (validation happens before any
launch), LidarBatchSampler's refusals, and the API surface."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import sampler_ref as ref


def test_philox_known_answer():
    """Random123's kat_vectors, philox4x32 10 rounds: counter 0 / key 0; and its two other published vectors."""
    got = ref.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert tuple(int(v) for v in got) == ref.KAT_ZERO == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    ones = 0xFFFFFFFF
    got = ref.philox4x32_10((ones, ones, ones, ones), (ones, ones))
    assert tuple(int(v) for v in got) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    got = ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert tuple(int(v) for v in got) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # vectorised over the first counter word = one call per value
    many = ref.philox4x32_10((np.arange(5), 7, 1, 3), (11, 13))
    for i in range(5):
        one = ref.philox4x32_10((i, 7, 1, 3), (11, 13))
        assert [int(w[i]) for w in many] == [int(w) for w in one]


def test_range_mapping():
    assert int(ref.to_range(0, 77)) == 0 and int(ref.to_range(0xFFFFFFFF, 77)) == 76
    assert int(ref.to_range(0x80000000, 7)) == 3 and int(ref.to_range(0xFFFFFFFF, 1 << 24)) == (1 << 24) - 1


@pytest.mark.parametrize("N,H,W,px,py,n", [(16, 8, 12, 1, 1, 16), (70, 8, 12, 2, 4, 64), (200, 8, 12, 1, 1, 96),
                                          (200, 8, 12, 2, 4, 96), (4096, 66, 1030, 2, 8, 4096), (4100, 66, 1030, 3, 5, 4095)])
def test_indices_follow_patch_indices_arithmetic(N, H, W, px, py, n):
    """The restated indices = the index arithmetic of rays.patch_indices (meshgrid of in-patch offsets, row-major) applied to
    the same top-left corners; corners stay inside [0, H-px) x [0, W-py)."""
    rows, cols = ref.corners(N, H, W, px, py, seed=5, draw=3, stream_id=1)
    assert ref.batch_rows(N, H, W, px, py) == n == rows.size * px * py
    assert rows.min() >= 0 and rows.max() < H - px and cols.min() >= 0 and cols.max() < W - py
    rows_t, cols_t = torch.from_numpy(rows), torch.from_numpy(cols)
    dr, dc = torch.meshgrid(torch.arange(px), torch.arange(py), indexing="ij")  # rays.py:21-24
    r = (rows_t[:, None] + dr.reshape(1, -1)).reshape(-1)
    c = (cols_t[:, None] + dc.reshape(1, -1)).reshape(-1)
    np.testing.assert_array_equal(ref.batch_indices(N, H, W, px, py, 5, 3, 1), (r * W + c).numpy())


def test_independent_pixels_and_streams():
    a = ref.batch_indices(200, 8, 12, 0, 0, seed=9, draw=0, stream_id=0)
    assert a.size == 96 and a.min() >= 0 and a.max() < 96
    assert not np.array_equal(a, ref.batch_indices(200, 8, 12, 0, 0, 9, 1, 0))      # another draw
    assert not np.array_equal(a, ref.batch_indices(200, 8, 12, 0, 0, 9, 0, 1))      # another stream
    assert not np.array_equal(a, ref.batch_indices(200, 8, 12, 0, 0, 10, 0, 0))     # another seed
    assert not np.array_equal(a, ref.batch_indices(200, 8, 12, 0, 0, 9 + (1 << 32), 0, 0))  # the seed's high word counts
    np.testing.assert_array_equal(a, ref.batch_indices(200, 8, 12, 0, 0, 9, 0, 0))


def uniformity_counts(draws=256, N=4096, H=8, W=12, seed=0):
    counts = np.zeros((H - 1) * (W - 1), dtype=np.int64)
    for d in range(draws):
        inds = ref.batch_indices(N, H, W, 1, 1, seed, d, 0)
        counts += np.bincount((inds // W) * (W - 1) + inds % W, minlength=counts.size)
    return counts


def check_uniform(counts, total, cells=77):
    p = 1.0 / cells
    sigma = np.sqrt(total * p * (1 - p))
    assert counts.size == cells and counts.sum() == total
    assert np.abs(counts - total * p).max() <= 5 * sigma, (counts.min(), counts.max(), total * p, sigma)


def test_restatement_is_uniform_for_seed_0():
    """1 x 1 patches on 8 x 12, seed 0, 256 draws of min(4096, 96) = 96 rays: the GPU test asserts the same bound on the
    kernel's draws; the run is deterministic, so the restatement must satisfy it first."""
    counts = uniformity_counts()
    check_uniform(counts, 256 * 96)


# ------------------------------------------------------------------------------------------ the C ABI's refusals
def _sample_args(**kw):
    a = dict(poses=1, images=1, dtype=0, F=3, H=8, W=12, fov_up=2.0, fov=26.9, perm=1, cursor=1, seed_lo=0, seed_hi=0,
             stream_id=0, n_rays=16, px=1, py=1, frame=-1, rays_o=1, rays_d=1, gt=1, inds=1)
    a.update(kw)
    return [a[k] for k in ("poses", "images", "dtype", "F", "H", "W", "fov_up", "fov", "perm", "cursor", "seed_lo", "seed_hi",
                           "stream_id", "n_rays", "px", "py", "frame", "rays_o", "rays_d", "gt", "inds")] + [None]


@pytest.mark.parametrize("kw,rc,names", [
    (dict(px=8), -1, b"px"), (dict(px=9), -1, b"px"), (dict(py=12), -1, b"py"), (dict(px=2, py=0), -1, b"py"),
    (dict(px=2, py=-1), -1, b"py"), (dict(n_rays=0), -1, b"n_rays"), (dict(n_rays=-5), -1, b"n_rays"),
    (dict(H=4097, W=4096), -2, b"H * W"), (dict(F=0), -1, b"F"), (dict(F=-1), -1, b"F"), (dict(frame=3), -1, b"frame"),
    (dict(frame=-2), -1, b"frame"), (dict(rays_o=None), -1, b"rays_o"), (dict(rays_d=None), -1, b"rays_d"),
    (dict(gt=None), -1, b"gt"), (dict(inds=None), -1, b"inds"), (dict(poses=None), -1, b"poses"),
    (dict(images=None), -1, b"images"), (dict(cursor=None), -1, b"cursor"), (dict(perm=None), -1, b"perm"),
    (dict(dtype=2), -2, b"image_dtype"), (dict(stream_id=-1), -1, b"stream_id")])
def test_sample_batch_refuses_by_name(kw, rc, names):
    """Pointers are the dummy address 1: every check runs on the host before any launch, and each refusal returns first."""
    from lidarnerf import _hip
    L = _hip.lib()
    got = L.lnh_lidar_sample_batch(*_sample_args(**kw))
    msg = L.lnh_last_error()
    assert got == rc and msg.startswith(b"lidar_sample_batch: ") and names in msg, (got, msg)


@pytest.mark.parametrize("kw,rc,names", [
    (dict(F=0), -1, b"F"), (dict(frame=3), -1, b"frame"), (dict(frame=-1), -1, b"frame"), (dict(H=4097, W=4096), -2, b"H * W"),
    (dict(rays_o=None), -1, b"rays_o"), (dict(rays_d=None), -1, b"rays_d"), (dict(poses=None), -1, b"poses")])
def test_frame_rays_refuses_by_name(kw, rc, names):
    from lidarnerf import _hip
    L = _hip.lib()
    a = dict(poses=1, F=3, frame=0, H=8, W=12, fov_up=2.0, fov=26.9, rays_o=1, rays_d=1)
    a.update(kw)
    got = L.lnh_lidar_frame_rays(*[a[k] for k in ("poses", "F", "frame", "H", "W", "fov_up", "fov", "rays_o", "rays_d")], None)
    msg = L.lnh_last_error()
    assert got == rc and msg.startswith(b"lidar_frame_rays: ") and names in msg, (got, msg)


# ------------------------------------------------------------------------------------------ the Python object
def _sequence(device="cpu", channels=3, F=3, H=8, W=12):
    g = torch.Generator().manual_seed(0)
    return {"poses_lidar": torch.eye(4).repeat(F, 1, 1).to(device), "H_lidar": H, "W_lidar": W,
            "images_lidar": torch.rand(F, H, W, channels, generator=g).to(device)}


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box without a GPU")
def test_sampler_refuses_cpu_tensors():
    from lidarnerf.dataset.sampler import LidarBatchSampler
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        LidarBatchSampler(_sequence(), (2.0, 26.9), num_rays=16)


def test_sampler_refuses_other_channel_counts():
    from lidarnerf.dataset.sampler import LidarBatchSampler
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    for ch in (1, 2, 4):
        with pytest.raises(ValueError, match=r"\[F, H, W, 3\]"):
            LidarBatchSampler(_sequence(dev, channels=ch), (2.0, 26.9), num_rays=16)


def test_api_surface():
    from lidarnerf import _hip
    from lidarnerf.dataset import sampler
    from lidarnerf.nerf.train_step import LidarTrainer
    assert list(inspect.signature(sampler.LidarBatchSampler.__init__).parameters) == \
        ["self", "sequence", "intrinsics", "num_rays", "patch_size", "seed", "stream_id"]
    d = {k: v.default for k, v in inspect.signature(sampler.LidarBatchSampler.__init__).parameters.items()}
    assert (d["num_rays"], d["patch_size"], d["seed"], d["stream_id"]) == (4096, 1, 0, 0)
    for name in ("new_epoch", "draw", "frame", "frames", "state_dict", "load_state_dict", "set_patch"):
        assert callable(getattr(sampler.LidarBatchSampler, name)), name
    assert list(inspect.signature(LidarTrainer.step_sampled).parameters) == ["self", "sampler"]
    assert list(inspect.signature(LidarTrainer.train_epoch).parameters) == ["self", "sampler", "steps"]
    assert list(inspect.signature(LidarTrainer.step).parameters) == ["self", "rays_o", "rays_d", "images_lidar", "patch"]
    assert {"lnh_lidar_sample_batch", "lnh_lidar_frame_rays"} <= set(_hip.EXPORTS)
    L = C.CDLL(_hip.lib_path())
    assert hasattr(L, "lnh_lidar_sample_batch") and hasattr(L, "lnh_lidar_frame_rays")
    # the three forms of patch_size, as get_lidar_rays takes them
    assert sampler.patch_shape(2) == (2, 2) and sampler.patch_shape([3]) == (3, 3) and sampler.patch_shape([2, 8]) == (2, 8)
    assert sampler.batch_rows(70, 8, 12, 2, 4) == 64 and sampler.batch_rows(200, 8, 12, 0, 0) == 96
