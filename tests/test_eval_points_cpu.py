"""The fused points meter without a GPU: the argument checks of the lnh_eval_points_* entry points, which happen before any
launch; the LNH_PTS_* enum of the header against the names bound in _hip.py; and the Python surface —
metrics.FramePointsEvaluator, nerf.evaluate.evaluate(fused_points=) and LidarTrainer(fused_points=) — with its refusal of CPU tensors."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
SCALE, K = 0.0107848535, (2.0, 26.9)


def test_entry_points_check_arguments_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    H, W = 16, 130
    need = L.lnh_eval_points_workspace_bytes(H, W)
    assert need > 0 and L.lnh_eval_points_workspace_bytes(66, 1030) > need
    for h, w in ((0, 130), (16, 0), (1 << 13, 1 << 12)):
        assert L.lnh_eval_points_workspace_bytes(h, w) == 0
    buf = (C.c_double * (need // 8 + 2))()
    ws = (C.addressof(buf) + 15) & ~15
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced

    def project(pred=x, gt=x, h=H, w=W, scale=SCALE, wsp=ws, wsb=need, c0=x, c1=x, counts=x):
        return L.lnh_eval_points_project(pred, gt, h, w, K[0], K[1], scale, 0, wsp, wsb, c0, c1, counts, None)

    for kw, word in ((dict(pred=None), "pred_depth"), (dict(gt=None), "gt"), (dict(c0=None), "cloud"), (dict(c1=None), "cloud"),
                     (dict(counts=None), "counts"), (dict(c0=24), "aligned"), (dict(counts=18), "aligned"),
                     (dict(h=0), "H * W"), (dict(w=0), "H * W"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"),
                     (dict(wsp=None), "workspace"), (dict(wsb=need - 8), "workspace"), (dict(wsp=ws + 8), "workspace")):
        assert project(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert project(h=1 << 13, w=1 << 12) == UNSUPPORTED and "2^24" in err()

    def nn(c0=x, c1=x, counts=x, cap=H * W, wsp=ws, wsb=need, d0=x, i0=x, d1=x, i1=x):
        return L.lnh_eval_points_nn(c0, c1, counts, cap, wsp, wsb, d0, i0, d1, i1, None)

    for kw, word in ((dict(c0=None), "cloud"), (dict(c1=None), "cloud"), (dict(counts=None), "counts"), (dict(d0=None), "dist_pred"),
                     (dict(i0=None), "idx_pred"), (dict(d1=None), "dist_gt"), (dict(i1=None), "idx_gt"), (dict(c1=8), "aligned"),
                     (dict(cap=0), "H * W"), (dict(wsp=None), "workspace"), (dict(wsb=need - 8), "workspace"),
                     (dict(cap=H * W + 4096), "workspace")):  # (a larger capacity needs a larger workspace)
        assert nn(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert nn(cap=(1 << 24) + 1) == UNSUPPORTED and "2^24" in err()

    def finalize(d0=x, d1=x, counts=x, cap=H * W, th=0.05, acc=x, hist=x, frames=4):
        return L.lnh_eval_points_finalize(d0, d1, counts, cap, th, acc, hist, frames, None)

    for kw, word in ((dict(d0=None), "dist"), (dict(d1=None), "dist"), (dict(counts=None), "counts"), (dict(acc=None), "accumulator"),
                     (dict(hist=None), "history"), (dict(acc=12), "aligned"), (dict(hist=20), "aligned"), (dict(cap=0), "H * W"),
                     (dict(th=0.0), "threshold"), (dict(th=-0.05), "threshold")):
        assert finalize(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert finalize(cap=(1 << 24) + 1) == UNSUPPORTED and "2^24" in err()
    assert L.lnh_version() == 102 and _hip.EVAL_SLOTS == 20  # (the new entry points are detected by symbol)


def test_header_slot_layout_matches_the_binding():
    from lidarnerf import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lidarnerf_hip.h")).read()
    slots = dict((n.lower(), int(v)) for n, v in re.findall(r"LNH_PTS_(\w+) = (\d+)", text))
    assert slots.pop("slots") == _hip.PTS_SLOTS == 10
    assert [k for k, _ in sorted(slots.items(), key=lambda kv: kv[1])] == list(_hip.PTS_SLOT_NAMES)
    import eval_points_ref
    assert eval_points_ref.SLOTS == _hip.PTS_SLOT_NAMES
    for name in ("lnh_eval_points_project", "lnh_eval_points_nn", "lnh_eval_points_finalize"):
        assert name in _hip._SIGS and name in _hip.EXPORTS and hasattr(_hip.lib(), name)
        assert re.search(r"LNH_API int " + name + r"\(", text)
    assert "lnh_eval_points_workspace_bytes" in _hip.EXPORTS


def test_python_surface_and_no_cpu_fallback():
    from lidarnerf import metrics
    from lidarnerf.nerf import evaluate
    from lidarnerf.nerf.train_step import LidarTrainer
    sig = inspect.signature(metrics.FramePointsEvaluator.__init__)
    assert list(sig.parameters)[1:] == ["H", "W", "scale", "intrinsics", "threshold", "nerf_mvl", "max_frames"]
    assert sig.parameters["threshold"].default == 0.05 and sig.parameters["nerf_mvl"].default is False
    assert sig.parameters["max_frames"].default == 1024
    assert list(inspect.signature(metrics.FramePointsEvaluator.update).parameters)[1:] == ["pred_depth", "images_lidar"]
    for name in ("measure", "clear", "report", "cloud"):
        assert callable(getattr(metrics.FramePointsEvaluator, name))
    p = inspect.signature(evaluate.evaluate).parameters["fused_points"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    # LidarTrainer.evaluate's parameter list is pinned (tests/test_g14_eval_cpu.py): the trainer carries the switch
    assert inspect.signature(LidarTrainer.__init__).parameters["fused_points"].default is False

    H, W = 16, 130
    ev = metrics.FramePointsEvaluator(H, W, SCALE, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(torch.zeros(H, W), torch.zeros(H, W, 3))
    with pytest.raises(RuntimeError, match="no frame"):
        ev.measure()
    with pytest.raises(RuntimeError, match="no frame"):
        ev.cloud()
    ev.clear()  # (nothing to clear yet: not an error)
    for bad in (dict(H=0), dict(scale=0.0), dict(threshold=0.0), dict(max_frames=-1)):
        kw = dict(H=H, W=W, scale=SCALE, intrinsics=K)
        kw.update(bad)
        with pytest.raises(ValueError):
            metrics.FramePointsEvaluator(**kw)

    class _Field(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))

        def get_params(self, lr):
            return [{"params": [self.w], "lr": lr}]

    assert LidarTrainer(_Field(), fp16=False, scale=SCALE).fused_points is False
    tr = LidarTrainer(_Field(), fp16=False, scale=SCALE, fused_points=True)
    assert tr.fused_points is True
    data = {"rays_o_lidar": torch.zeros(1, H * W, 3), "rays_d_lidar": torch.zeros(1, H * W, 3),
            "images_lidar": torch.zeros(1, H, W, 3), "H_lidar": H, "W_lidar": W}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.evaluate([data], points_intrinsics=K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.evaluate(tr, [data], points_intrinsics=K, fused_points=True)
    assert tr.model.training and tr.stats["results"] == []
