"""The training forward tail (lnh_lidar_color_composite_forward_train, csrc/lidar_color.hip): the forward tail of a ray, the
default loss's gradient of that ray and its compositing adjoint in one launch.

Everything is compared with torch.equal against the three-call chain it replaces, on the same inputs:
lnh_lidar_color_composite_forward -> lnh_lidar_loss -> lnh_lidar_composite_backward.  The kernels share the per-ray loss
(csrc/lidar_loss_ray.h) and the two passes of the adjoint (csrc/composite_adjoint.h) as device functions, and the tail hands
the adjoint the alpha_i and T_i its own forward walk formed, so there is no tolerance to state.  T in {1, 63, 65, 449}: one
sample; a partial and a just-started second 64-sample span; one sample past the seven rounds a wave requests at once
(7 x 64 = 448).  N in {1, 5}: 5 is no multiple of the four waves of a workgroup.  sigma_m and rgb stay in LDS in training:
the entry point takes no buffer for either, so there is nothing of them to compare or to guard.

The stand-alone lnh_lidar_composite_backward is held to what the build BEFORE its body moved into composite_adjoint.h
answered to the inputs of tests/golden/composite_backward_parent.npz (recorded by tests/golden/make_composite_backward.py).

One step end to end: LidarTrainer at 64 rays x (48 + 16) samples, 3 steps, launch by launch and captured, LNH_TRAIN_TAIL=0
against =1: every parameter, the table gradient and the three losses carry the same bits.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TS = (1, 63, 65, 449)
NS = (1, 5)
MASK = 1e-4  # renderer.py:249: the colour head runs where weights > 1e-4
ALPHAS = (1000.0, 1.0, 10.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_backward_parent.npz")
# what a ray is there for (the ray of an N = 1 case takes the kind KIND_OF_T[T]; an N = 5 case holds all five, in order)
ALL_BELOW, BOTH_SIDES, DROPPED, SIGN_ZERO, PLAIN = range(5)
KIND_OF_T = {1: SIGN_ZERO, 63: ALL_BELOW, 65: BOTH_SIDES, 449: DROPPED}


def make_case(T, N, seed=0):
    """Host inputs of the forward tail (numpy, float32 / int32; h16 and w16 as float32 still to be narrowed) and the kind of
    every ray.  Densities are laid out in MERGED order first and scattered through the permutation."""
    r = np.random.default_rng(1000 * T + 10 * N + seed)
    kinds = [KIND_OF_T[T]] if N == 1 else [ALL_BELOW, BOTH_SIDES, DROPPED, SIGN_ZERO, PLAIN]
    z = np.sort(r.uniform(0.01, 0.81, (N, T)).astype(np.float32), axis=1)
    perm = np.stack([r.permutation(T) for _ in range(N)]).astype(np.int32)
    sigma_m = r.uniform(0.0, 3.0, (N, T)).astype(np.float32)
    for n, k in enumerate(kinds):
        if k == ALL_BELOW:
            sigma_m[n] = 0.0  # no weight at all
        elif k == BOTH_SIDES:
            # opaque within the first span: every later span sees a transmittance of ~0
            sigma_m[n] = 0.0
            sigma_m[n, :min(T, 8)] = 40.0 * T
    sigma_pt = np.zeros_like(sigma_m)
    np.put_along_axis(sigma_pt, perm.astype(np.int64), sigma_m, axis=1)
    gt = np.stack([np.ones(N), r.uniform(0, 1, N), r.uniform(0.05, 0.8, N)], -1).astype(np.float32)
    for n, k in enumerate(kinds):
        if k == DROPPED:
            gt[n, 0] = 0.0
    return dict(T=T, N=N, kinds=kinds, z=z, perm=perm, sigma_pt=sigma_pt, sd=np.full(N, 0.8 / T, np.float32), gt=gt,
                h16=(r.standard_normal((N * T, 16)) * 0.5).astype(np.float32), cdir=r.standard_normal((N, 64)).astype(np.float32),
                w16=(r.standard_normal(64 * 16 + 64 * 64 + 16 * 64) * 0.2).astype(np.float32))


def _outs(N, T):
    """(sigma_m, weights, rgb, weights_sum, depth, image), NaN-filled: a word nobody wrote fails torch.equal."""
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    return nan(N, T), nan(N, T), nan(N, T, 2), nan(N), nan(N), nan(N, 2)


class Chain:
    """A case on the device and the answers of the three-call chain.  The ground-truth depth of the SIGN_ZERO ray is the
    depth the forward tail predicts for it, so its depth difference is an exact 0."""

    def __init__(self, T, N, sfx):
        from gpu_util import call
        c = make_case(T, N)
        mdt = torch.bfloat16 if sfx == "_bf16" else torch.half
        dev = lambda a: torch.from_numpy(a).cuda()
        self.T, self.N, self.sfx, self.kinds = T, N, sfx, c["kinds"]
        self.fwd_in = (dev(c["z"]), dev(c["sigma_pt"]), dev(c["perm"]), dev(c["sd"]), dev(c["h16"]).to(mdt), dev(c["cdir"]),
                       dev(c["w16"]).to(mdt))
        self.fwd = _outs(N, T)
        call("lnh_lidar_color_composite_forward" + sfx, *self.fwd_in, N, T, 1.0, *self.fwd)
        self.gt = dev(c["gt"])
        for n, k in enumerate(self.kinds):
            if k == SIGN_ZERO:
                self.gt[n, 2] = self.fwd[4][n]
        torch.cuda.synchronize()

    def backward(self, grad_scale):
        """(loss, g_depth, g_image, g_sigma) of lnh_lidar_loss -> lnh_lidar_composite_backward on the forward's outputs."""
        from gpu_util import call
        N, T = self.N, self.T
        sigma_m, _w, rgb, _ws, depth, image = self.fwd
        loss, g_depth, g_image = torch.full((), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda"), \
            torch.full((N, 2), float("nan"), device="cuda")
        call("lnh_lidar_loss", depth, image, self.gt, N, *ALPHAS, grad_scale, loss, g_depth, g_image)
        g_sigma = torch.full((N, T), float("nan"), device="cuda")
        call("lnh_lidar_composite_backward", None, g_depth, g_image, self.fwd_in[0], sigma_m, rgb, self.fwd_in[3], N, T, 2, 1.0,
             g_sigma, None)
        return loss, g_depth, g_image, g_sigma

    def present(self):
        """Which of the cases the issue lists this input holds, read off the DATA (the chain's own outputs)."""
        w, depth = self.fwd[1].cpu().numpy(), self.fwd[4].cpu().numpy()
        gt = self.gt.cpu().numpy()
        T = self.T
        spans = [(w[:, s:s + 64] > MASK).any(axis=1) for s in range(0, T, 64)]  # [span][ray]: holds a sample above the threshold
        above = np.stack(spans, 1)
        dd = depth * gt[:, 0] - gt[:, 2] * gt[:, 0]
        return {"all_below": bool((~above.any(1)).any()), "both_sides": bool((above.any(1) & ~above.all(1)).any()),
                "dropped": bool((gt[:, 0] == 0).any()), "sign_zero": bool(((dd == 0) & (gt[:, 0] != 0)).any()),
                "above": bool(above.any())}


_CHAINS = {}


def chain(T, N, sfx):
    key = (T, N, sfx)
    if key not in _CHAINS:
        _CHAINS[key] = Chain(T, N, sfx)
    return _CHAINS[key]


def test_inputs_hold_every_case():
    """Every N = 5 input holds a ray with all spans below the mask threshold, one with ray-drop 0, one with depth difference
    0 at ray-drop 1 and spans above the threshold; with more than one span (T > 64) also a ray with spans on both sides.  The
    N = 1 inputs hold one of them each."""
    for T in TS:
        p = chain(T, 5, "").present()
        assert p["all_below"] and p["dropped"] and p["sign_zero"] and p["above"], (T, p)
        assert p["both_sides"] == (T > 64), (T, p)
    one = [chain(T, 1, "").present() for T in TS]
    for k in ("all_below", "both_sides", "dropped", "sign_zero"):
        assert any(p[k] for p in one), k


@pytest.mark.parametrize("scale_log2", [None, 16])
@pytest.mark.parametrize("sfx", ["", "_bf16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_train_tail_equals_the_three_call_chain(T, N, sfx, scale_log2):
    from gpu_util import call
    ch = chain(T, N, sfx)
    grad_scale = None if scale_log2 is None else torch.tensor(float(2 ** scale_log2), device="cuda")
    loss, g_depth, g_image, g_sigma = ch.backward(grad_scale)
    _sm, w_t, _rgb, ws_t, dp_t, im_t = _outs(N, T)
    gs_t, gi_t = torch.full((N, T), float("nan"), device="cuda"), torch.full((N, 2), float("nan"), device="cuda")
    call("lnh_lidar_color_composite_forward_train" + sfx, *ch.fwd_in, N, T, 1.0, ch.gt, *ALPHAS, grad_scale, w_t, ws_t, dp_t, im_t,
         gs_t, gi_t)
    torch.cuda.synchronize()
    want = (ch.fwd[1], ch.fwd[3], ch.fwd[4], ch.fwd[5], g_sigma, g_image)
    for name, a, b in zip(("weights", "weights_sum", "depth", "image", "g_sigma", "g_image"), want, (w_t, ws_t, dp_t, im_t, gs_t, gi_t)):
        assert torch.equal(a, b), f"T={T} N={N}{sfx} scale={scale_log2}: {name} differs from the three-call chain"
    assert torch.isfinite(g_sigma).all()
    for n, k in enumerate(ch.kinds):
        if k == SIGN_ZERO:
            assert float(g_depth[n]) == 0.0  # sign(0) = 0: the depth term hands nothing back
    if scale_log2 is not None:  # the scale arrives: a power of two multiplies the image gradient exactly
        assert torch.equal(ch.backward(None)[2] * 2.0 ** scale_log2, gi_t)
    # the loss VALUE of a step on this path: the same kernel with null gradient outputs, the same bits
    loss_v = torch.full((), float("nan"), device="cuda")
    call("lnh_lidar_loss", ch.fwd[4], ch.fwd[5], ch.gt, N, *ALPHAS, grad_scale, loss_v, None, None)
    assert torch.equal(loss_v, loss)


def test_train_tail_at_the_largest_ray():
    """T = 2048, the most the entry point takes: 128 KiB of LDS per workgroup, above the 64 KiB a launch gets unasked."""
    from gpu_util import call
    T, N = 2048, 5
    ch = chain(T, N, "")
    grad_scale = torch.tensor(65536.0, device="cuda")
    _loss, _gd, g_image, g_sigma = ch.backward(grad_scale)
    _sm, w_t, _rgb, ws_t, dp_t, im_t = _outs(N, T)
    gs_t, gi_t = torch.full((N, T), float("nan"), device="cuda"), torch.full((N, 2), float("nan"), device="cuda")
    call("lnh_lidar_color_composite_forward_train", *ch.fwd_in, N, T, 1.0, ch.gt, *ALPHAS, grad_scale, w_t, ws_t, dp_t, im_t, gs_t, gi_t)
    torch.cuda.synchronize()
    for name, a, b in zip(("weights", "weights_sum", "depth", "image", "g_sigma", "g_image"),
                          (ch.fwd[1], ch.fwd[3], ch.fwd[4], ch.fwd[5], g_sigma, g_image), (w_t, ws_t, dp_t, im_t, gs_t, gi_t)):
        assert torch.equal(a, b), f"T={T}: {name} differs from the three-call chain"


def test_train_tail_refuses_null_pointers():
    from gpu_util import call
    ch = chain(63, 5, "")
    _sm, w, _rgb, ws, dp, im = _outs(5, 63)
    g = torch.empty(5, 63, device="cuda")
    with pytest.raises(RuntimeError, match="null pointer"):
        call("lnh_lidar_color_composite_forward_train", *ch.fwd_in, 5, 63, 1.0, None, *ALPHAS, None, w, ws, dp, im, g, g)
    with pytest.raises(RuntimeError, match="null pointer"):
        call("lnh_lidar_color_composite_forward_train", *ch.fwd_in, 5, 63, 1.0, ch.gt, *ALPHAS, None, w, ws, dp, im, None, g)
    with pytest.raises(RuntimeError, match="LDS"):
        call("lnh_lidar_color_composite_forward_train", *ch.fwd_in, 1, 2049, 1.0, ch.gt, *ALPHAS, None, w, ws, dp, im, g, g)


def test_composite_backward_answers_as_before_the_refactor():
    """lnh_lidar_composite_backward on the recorded inputs: the bits the build before composite_adjoint.h existed wrote."""
    from gpu_util import call
    rec = np.load(GOLDEN)
    n_cases = int(rec["n_cases"])
    assert n_cases == 2 * len(TS)
    for i in range(n_cases):
        dev = lambda k: torch.from_numpy(rec[f"{i}_{k}"]).cuda()
        z, sigma, rgb, sd, g_depth, g_image = (dev(k) for k in ("z", "sigma", "rgb", "sd", "g_depth", "g_image"))
        N, T = z.shape
        full = bool(rec[f"{i}_full"])  # with grad_weights_sum and grad_rgb, or as the training step calls it (both null)
        gs, gc = torch.full((N, T), float("nan"), device="cuda"), torch.full((N, T, 2), float("nan"), device="cuda")
        call("lnh_lidar_composite_backward", dev("g_ws") if full else None, g_depth, g_image, z, sigma, rgb, sd, N, T, 2, 1.0, gs,
             gc if full else None)
        assert torch.equal(gs, dev("out_g_sigma")), f"case {i} (T={T}, full={full}): g_sigma"
        if full:
            assert torch.equal(gc, dev("out_g_rgb")), f"case {i} (T={T}): g_rgb"


def _steps(graph, tail, monkeypatch):
    import bench
    from lidarnerf import _hip
    from lidarnerf.nerf.train_step import LidarTrainer
    monkeypatch.setenv("LNH_TRAIN_TAIL", "1" if tail else "0")
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph,
                      render_kwargs=dict(num_steps=48, upsample_steps=16))
    poses = bench.synthetic_frames(3, dev)
    batches = [bench.make_batch(poses, s, 64, 0, dev, (1, 1), "analytic") for s in range(3)]
    torch.manual_seed(11)
    losses = [tr.step(*b).detach().clone() for b in batches]
    torch.cuda.synchronize()
    assert bool(tr.graph) == graph and (not graph or len(tr._graphs) == 1), tr.graph_error
    state = [p.detach().clone() for p in model.parameters()] + [tr.table_grad().clone(), torch.stack(losses)]
    return state, tuple(names)  # (a copy: the wrapper of this run stays underneath the next run's)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_one_step_end_to_end(graph, monkeypatch):
    old, old_names = _steps(graph, False, monkeypatch)
    new, new_names = _steps(graph, True, monkeypatch)
    # each run took the path it was asked for
    assert "lnh_lidar_composite_backward" in old_names and "lnh_lidar_color_composite_forward_train" not in old_names
    assert "lnh_lidar_color_composite_forward_train" in new_names and "lnh_lidar_composite_backward" not in new_names
    assert old_names.count("lnh_lidar_loss") == new_names.count("lnh_lidar_loss") > 0
    assert len(old) == len(new)
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), f"tensor {i} of {len(old)} (parameters..., table gradient, losses) differs"
    assert torch.isfinite(new[-1]).all() and float(new[-2].abs().sum()) > 0
