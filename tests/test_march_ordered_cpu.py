"""Host side of the ray-ordered marcher: the library exports lnh_march_rays_train_ordered, the header declares it with
lnh_march_rays_train's argument list, its argument checks answer before any launch (so without a GPU), and the Python
surface — march_rays_train(ordered=), NeRFRenderer / both NeRFNetworks (ordered_march=), run_cuda(ordered_march=) — takes
the new keyword with the default off."""
import ctypes
import inspect
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lnh_march_rays_train_ordered"


def test_library_exports_the_entry_point():
    from lidarnerf import _hip
    assert hasattr(ctypes.CDLL(_hip.lib_path()), NAME)
    assert NAME in _hip.EXPORTS and _hip._SIGS[NAME] == _hip._SIGS["lnh_march_rays_train"]
    _hip.require_symbols([NAME], "ordered marching")


def test_header_declares_it_with_the_arguments_of_the_arrival_order_marcher():
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    protos = dict(re.findall(r"LNH_API\s+int\s+(lnh_march_rays_train\w*)\s*\(([^;]*?)\)\s*;", text, flags=re.S))
    assert set(protos) == {"lnh_march_rays_train", NAME}
    norm = lambda args: [" ".join(a.split()) for a in args.split(",")]
    assert norm(protos[NAME]) == norm(protos["lnh_march_rays_train"])
    comment = text[:text.index("LNH_API int " + NAME)].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("Adds") and "ray" in comment and "offset + count > M" in comment


def test_argument_checks_answer_without_a_gpu():
    from lidarnerf import _hip
    L = _hip.lib()
    ok = [8] * 11  # (never dereferenced: every call below is refused, or returns, before a launch)

    def rc(n=16, C=1, H=128, max_steps=1024, null=None):
        p = [None if i == null else v for i, v in enumerate(ok)]
        return getattr(L, NAME)(p[0], p[1], p[2], 1.0, 0.0, max_steps, n, C, H, 64, *p[3:], None)

    for kw in [dict(null=i) for i in range(11)] + [dict(C=0), dict(C=9), dict(H=0), dict(H=1025), dict(max_steps=0)]:
        assert rc(**kw) == -1 and b"march_rays_train_ordered" in L.lnh_last_error(), kw
    assert rc(null=0, n=0) == -1  # (the refusals come first, as in lnh_march_rays_train)
    assert rc(n=0) == 0


def test_python_surface_takes_the_keyword_and_defaults_to_off():
    from lidarnerf import raymarching
    from lidarnerf.nerf import network, network_tcnn
    from lidarnerf.nerf.renderer import NeRFRenderer
    assert inspect.signature(raymarching.march_rays_train).parameters["ordered"].default is False
    assert inspect.signature(NeRFRenderer.__init__).parameters["ordered_march"].default is False
    assert inspect.signature(NeRFRenderer.run_cuda).parameters["ordered_march"].default is None
    assert inspect.signature(NeRFRenderer.update_extra_state).parameters["ordered_march"].default is None
    assert "ordered_march" not in inspect.signature(NeRFRenderer.run_cuda_alive).parameters
    for cls in (network.NeRFNetwork, network_tcnn.NeRFNetwork):
        kw = dict(desired_resolution=512, log2_hashmap_size=12, bound=1, cuda_ray=True)
        assert cls(**kw).ordered_march is False
        assert cls(ordered_march=True, **kw).ordered_march is True
        assert cls(desired_resolution=512, log2_hashmap_size=12, bound=1).ordered_march is False  # (dense: nothing to order)
    with torch.no_grad():
        net = network.NeRFNetwork(ordered_march=True, **kw)
    assert "ordered_march" not in net.state_dict()  # an attribute, not a buffer: checkpoints keep their layout
