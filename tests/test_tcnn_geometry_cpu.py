"""tiny-cuda-nn level geometry of the hash grid (GridEncoder gridtype "tcnn", tcnn_compat geometry="tcnn"): row counts,
the flat `params` vector's length, native loading of tiny-cuda-nn-sized vectors and refusal of torch-ngp-sized ones.
The tiny-cuda-nn side is tcnn_compat's restatement of its published GridEncoding (parity with a real build unpinned)."""
import numpy as np
import pytest
import torch

from lidarnerf import tcnn_compat as T
from lidarnerf.gridencoder import grid

CFG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "per_level_scale": 1.4472692012786865}  # network_tcnn.py:40-57 with desired_resolution 2048 * bound


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("desired", [2048, 8192, 32768])
def test_tcnn_offsets_equal_tiny_cuda_nn_row_counts(desired, D):
    pls = T.per_level_scale(desired, 1)
    for log2 in range(15, 23):
        cfg = dict(CFG, per_level_scale=pls, log2_hashmap_size=log2)
        want = [rows for _, rows, _ in T._tcnn_levels(cfg, D)]
        off = grid.level_offsets(D, 16, pls, 16, log2, False, gridtype="tcnn")
        assert np.diff(off).tolist() == want, (desired, log2, D)
        enc = grid.GridEncoder(input_dim=D, num_levels=16, per_level_scale=pls, base_resolution=16, log2_hashmap_size=log2,
                               gridtype="tcnn")
        assert enc.gridtype_id == 2 and enc.embeddings.shape[0] == sum(want)


def test_tcnn_gridtype_has_no_align_corners():
    with pytest.raises(ValueError, match="align_corners"):
        grid.GridEncoder(gridtype="tcnn", align_corners=True)


def test_tcnn_geometry_params_load_natively_and_save_tcnn_sized(monkeypatch):
    monkeypatch.delenv("LNH_TCNN_CONVERT", raising=False)
    monkeypatch.delenv("LNH_TCNN_GEOMETRY", raising=False)
    e = T.Encoding(3, CFG, geometry="tcnn")
    n = T._tcnn_hashgrid_param_count(CFG, 3)
    assert e.geometry == "tcnn" and e.impl.gridtype_id == 2
    assert e.params.numel() == n
    assert list(e.state_dict()) == ["params"] and e.state_dict()["params"].numel() == n
    v = torch.randn(n, generator=torch.Generator().manual_seed(0))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no conversion, no warning
        e.load_state_dict({"params": v})
    assert torch.equal(e.impl.params.detach(), v)
    # a vector of this package's default (torch-ngp) geometry is refused by name, naming the switch
    ngp = T.Encoding(3, CFG).impl.params.numel()
    assert ngp != n
    with pytest.raises(RuntimeError, match="torch-ngp"):
        e.load_state_dict({"params": torch.zeros(ngp)})
    with pytest.raises(RuntimeError, match="another encoding config"):
        e.load_state_dict({"params": torch.zeros(1000)})


def test_geometry_from_environment(monkeypatch):
    monkeypatch.setenv("LNH_TCNN_GEOMETRY", "tcnn")
    assert T.Encoding(3, CFG).impl.gridtype_id == 2
    monkeypatch.setenv("LNH_TCNN_GEOMETRY", "torch-ngp")
    assert T.Encoding(3, CFG).impl.gridtype_id == 0
    assert T.Encoding(3, CFG, geometry="tcnn").impl.gridtype_id == 2  # the argument wins
    monkeypatch.setenv("LNH_TCNN_GEOMETRY", "instant-ngp")
    with pytest.raises(ValueError, match="geometry"):
        T.Encoding(3, CFG)
    monkeypatch.delenv("LNH_TCNN_GEOMETRY")
    with pytest.raises(ValueError, match="geometry"):
        T.Encoding(3, CFG, geometry="dense")
    assert T.Encoding(3, CFG).geometry == "torch-ngp"  # default unchanged


def test_default_geometry_refusal_names_the_switch(monkeypatch):
    monkeypatch.delenv("LNH_TCNN_CONVERT", raising=False)
    e = T.Encoding(3, CFG, geometry="torch-ngp")
    with pytest.raises(RuntimeError, match="LNH_TCNN_GEOMETRY=tcnn"):
        e.load_state_dict({"params": torch.zeros(T._tcnn_hashgrid_param_count(CFG, 3))})


def test_config_the_converter_refuses_loads_natively(monkeypatch):
    """desired_resolution 8192 / log2_hashmap_size 21: a level is dense in tiny-cuda-nn and hashed in torch-ngp geometry,
    so convert_tcnn_hashgrid_params refuses it; tiny-cuda-nn geometry needs no conversion."""
    monkeypatch.delenv("LNH_TCNN_CONVERT", raising=False)
    cfg = dict(CFG, per_level_scale=T.per_level_scale(8192, 1), log2_hashmap_size=21)
    n = T._tcnn_hashgrid_param_count(cfg, 3)
    with pytest.raises(RuntimeError, match="dense in tiny-cuda-nn and hashed"):
        T.convert_tcnn_hashgrid_params(torch.zeros(n), cfg, 3)
    e = T.Encoding(3, cfg, geometry="tcnn")
    assert e.params.numel() == n
    v = torch.rand(n, generator=torch.Generator().manual_seed(1))
    e.load_state_dict({"params": v})
    assert torch.equal(e.impl.params.detach(), v)


def test_network_tcnn_state_dict_has_tcnn_sized_encoder_params(monkeypatch):
    from lidarnerf.nerf.network_tcnn import NeRFNetwork
    monkeypatch.delenv("LNH_TCNN_GEOMETRY", raising=False)
    net = NeRFNetwork(desired_resolution=2048, log2_hashmap_size=19, bound=1, tcnn_geometry="tcnn")
    sd = net.state_dict()
    assert sd["encoder.params"].numel() == T._tcnn_hashgrid_param_count(net.encoder.encoding_config, 3)
    dflt = NeRFNetwork(desired_resolution=2048, log2_hashmap_size=19, bound=1)
    assert dflt.encoder.geometry == "torch-ngp" and dflt.state_dict()["encoder.params"].numel() != sd["encoder.params"].numel()
    fresh = NeRFNetwork(desired_resolution=2048, log2_hashmap_size=19, bound=1, tcnn_geometry="tcnn")
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.encoder.params.detach(), net.encoder.params.detach())


def test_dense_levels_take_the_paired_backward_plan():
    """The bucketed backward deals the rows of a dense tcnn-geometry level to 128-row groups over up to 64 buckets (the
    paired scatter class, like a dense level of the default lattice), not to 8192-row buckets of the generic class."""
    import ctypes
    from lidarnerf import _hip
    pls = T.per_level_scale(32768, 1)
    off = torch.from_numpy(grid.level_offsets(3, 16, pls, 16, 19, False, gridtype="tcnn"))
    levels = T._tcnn_levels(dict(CFG, per_level_scale=pls), 3)
    out = (ctypes.c_uint32 * 4)()
    for l, (res, rows, hashed) in enumerate(levels):
        rc = _hip.lib().lnh_grid_backward_plan_info(off.data_ptr(), 1 << 20, 3, 2, 16, float(np.log2(pls)), 16, 2, 0,
                                                    _hip.LNH_F16, l, ctypes.addressof(out))
        assert rc == 0
        want = -(-rows // 8192) if hashed else min(-(-rows // 128), 64)
        assert out[0] == want, (l, res, rows, hashed, out[0])
