"""with `lidar-nerf_amd/` in front of a lidar-nerf checkout on PYTHONPATH, the import chain of
main_lidarnerf.py (main_lidarnerf.py:6-13, 27-34, 289-324) resolves the hot-path modules from THIS package and the
host glue (Trainer, datasets) from the checkout.  The checkout is a stand-in written into a temporary directory: the
upstream layout (a `lidarnerf/__init__.py`, `nerf/` and `dataset/` without one), its host-glue modules with the
cross-module imports they make (nerf/utils.py:26-28, kitti360_dataset.py:10, nerfmvl_dataset.py:10), and decoys of
every module this package provides, which fail if imported.  Runs in a subprocess (the package's __path__ is fixed at
first import)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# module path -> source, relative to the stand-in checkout's root
UPSTREAM_GLUE = {
    "main_lidarnerf.py": "from lidarnerf.nerf.utils import Trainer, seed_everything\n",
    "lidarnerf/__init__.py": "",
    "lidarnerf/loss.py": "",
    "lidarnerf/nerf/utils.py": ("from lidarnerf.dataset.base_dataset import custom_meshgrid\n"
                                "from lidarnerf.convert import pano_to_lidar\n"
                                "def seed_everything(seed):\n    pass\n"
                                "class Trainer:\n    pass\n"),
    "lidarnerf/dataset/base_dataset.py": ("def get_lidar_rays(*args, **kwargs):\n    pass\n"
                                          "def custom_meshgrid(*args):\n    pass\n"
                                          "class BaseDataset:\n    pass\n"),
    "lidarnerf/dataset/kitti360_dataset.py": ("from lidarnerf.dataset.base_dataset import get_lidar_rays, BaseDataset\n"
                                              "class KITTI360Dataset(BaseDataset):\n    pass\n"),
    "lidarnerf/dataset/nerfmvl_dataset.py": ("from lidarnerf.dataset.base_dataset import get_lidar_rays, BaseDataset\n"
                                             "class NeRFMVLDataset(BaseDataset):\n    pass\n"),
}
# modules of the upstream tree that this package shadows
SHADOWED = ["lidarnerf/activation.py", "lidarnerf/convert.py", "lidarnerf/encoding.py", "lidarnerf/nerf/network.py",
            "lidarnerf/nerf/network_tcnn.py", "lidarnerf/nerf/renderer.py", "lidarnerf/gridencoder/__init__.py",
            "lidarnerf/raymarching/__init__.py", "lidarnerf/freqencoder/__init__.py", "lidarnerf/shencoder/__init__.py",
            "lidarnerf/ffmlp/__init__.py"]

SCRIPT = r'''
import sys
import main_lidarnerf                                    # main_lidarnerf.py:1-13
from lidarnerf.nerf.utils import Trainer                 # the upstream host glue
from lidarnerf.nerf.network import NeRFNetwork           # main_lidarnerf.py:309
from lidarnerf.nerf.network_tcnn import NeRFNetwork as TcnnNetwork   # main_lidarnerf.py:292 (-L)
from lidarnerf.dataset.kitti360_dataset import KITTI360Dataset      # main_lidarnerf.py:27
from lidarnerf.dataset.nerfmvl_dataset import NeRFMVLDataset
import lidarnerf, lidarnerf.nerf.renderer, lidarnerf.encoding, lidarnerf.gridencoder, lidarnerf.raymarching
upstream = sys.argv[1]
for mod in (Trainer, KITTI360Dataset, NeRFMVLDataset, main_lidarnerf):
    f = sys.modules[mod.__module__].__file__ if hasattr(mod, "__module__") else mod.__file__
    assert f.startswith(upstream + "/"), f
for mod in (NeRFNetwork, TcnnNetwork, lidarnerf.nerf.renderer, lidarnerf.encoding, lidarnerf.gridencoder,
            lidarnerf.raymarching, lidarnerf.convert):
    f = sys.modules[mod.__module__].__file__ if isinstance(mod, type) else mod.__file__
    assert "/lidar-nerf_amd/lidarnerf/" in f, f
# the model main() would build (main_lidarnerf.py:309-323) constructs from this package, with the reference's kwargs
model = NeRFNetwork(encoding="hashgrid", desired_resolution=2048, log2_hashmap_size=19, num_layers=2, hidden_dim=64,
                    geo_feat_dim=15, bound=1, density_scale=1, min_near=0.01, density_thresh=10, bg_radius=-1)
assert type(model).__module__ == "lidarnerf.nerf.network" and hasattr(model, "render")
assert [g["lr"] for g in model.get_params(1e-2)]         # Trainer's optimizer factory: main_lidarnerf.py:389-391
print("DROPIN_OK")
'''


def test_main_lidarnerf_import_chain(tmp_path):
    upstream = tmp_path / "lidar-nerf"
    files = dict(UPSTREAM_GLUE)
    files.update({p: f"raise ImportError('upstream {p} imported: lidar-nerf_amd should shadow it')\n" for p in SHADOWED})
    for rel, src in files.items():
        path = upstream / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(src)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "lidar-nerf_amd"), str(upstream)]))
    r = subprocess.run([sys.executable, "-c", SCRIPT, str(upstream)], env=env, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0 and "DROPIN_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
