"""Occupancy-grid training with the ray-ordered marcher (NeRFRenderer.ordered_march / run_cuda(ordered_march=)): two runs
of a seed are the same bits at 256 rays per batch — 16 workgroups of the marcher, where the arrival-order marcher's runs
differ in the last bits (tests/test_sampler_gpu.py stays at 16 rays for that reason) —, step_sampled = step on the same
draws through the captured steps' capacity ladder, update_extra_state with duplicated cells, and an evaluation render that
equals the arrival-order one per ray."""
import numpy as np
import pytest
import torch

from test_sampler_gpu import SCALE, _sampler, _sequence

pytestmark = pytest.mark.gpu
RAYS = 256  # 16 workgroups of the training marcher (csrc/raymarch.hip, kMarchRaysPerGroup = 16); frames of 16 x 32 pixels


def _net(ordered=True, fused=True):
    """The occupancy model of tests/test_sampler_gpu.py::_trainer."""
    from lidarnerf.nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(encoding="hashgrid", desired_resolution=2048, bound=1, min_near=SCALE, min_near_lidar=SCALE,
                      density_thresh=10, cuda_ray=True, ordered_march=ordered, fused_lidar=fused)
    with torch.no_grad():
        net.encoder.embeddings.uniform_(-0.5, 0.5)
    return net.cuda()


def _trainer(graph, fused=True, how="kwargs"):
    """how: the flag through LidarTrainer(render_kwargs=) on a model built without it, or as the module attribute."""
    from lidarnerf.nerf.train_step import LidarTrainer
    net = _net(ordered=how == "attribute", fused=fused).train()
    tr = LidarTrainer(net, lr=1e-2, iters=30000, fp16=True, scale=SCALE, graph=graph,
                      render_kwargs={"ordered_march": True} if how == "kwargs" else {})
    assert tr.occupancy and tr.graph == graph and (tr.table is not None) == fused
    return tr


def _state(tr, losses):
    torch.cuda.synchronize()
    net = tr.model
    out = {"losses": torch.stack(losses), "density_grid": net.density_grid.clone(),
           "density_bitfield": net.density_bitfield.clone(), "step_counter": net.step_counter.clone()}
    for name, p in net.named_parameters():
        out["param " + name] = p.detach().clone()  # the table and every MLP matrix
    if tr.table is not None:
        out.update(table16=tr.table._lnh_table16.clone(), t_m=tr.t_m.clone(), t_v=tr.t_v.clone(),
                   opt_state=tr.opt_state.clone(), small_m=tr.small_m.clone(), small_v=tr.small_v.clone())
    else:
        for i, p in enumerate(tr.params):
            for k, v in tr.optimizer.state[p].items():
                out[f"adam {i} {k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))
        out["loss_scale"] = torch.tensor(tr.scaler.get_scale())
    return out


def _run(graph, steps, sampled, fused=True, how="kwargs"):
    s = _sampler(_sequence(F=3, H=16, W=32, seed=4), num_rays=RAYS, patch_size=1, seed=17)
    s.new_epoch()
    tr = _trainer(graph, fused, how)
    torch.manual_seed(11)
    losses = []
    for _ in range(steps):
        loss = tr.step_sampled(s) if sampled else tr.step(*s.draw(), s.patch)
        losses.append(loss.detach().float().clone())
    assert s.n == RAYS and s.cursor.tolist() == [steps, steps] and tr.global_step == steps
    return tr, _state(tr, losses)


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 6. two trainers, one seed
@pytest.mark.parametrize("graph,fused,how", [(False, True, "kwargs"), (True, True, "kwargs"), (True, True, "attribute"),
                                             (False, False, "kwargs")])
def test_two_trainers_of_one_seed_are_bit_identical(graph, fused, how):
    """20 steps (grid refreshes in front of steps 0 and 16; with graph=True steps 17 .. 19 are captured): losses, table, fp16
    copy, Adam moments, optimizer scalars, every MLP matrix, density_grid, density_bitfield and the marcher's counters."""
    tr, a = _run(graph, 20, sampled=True, fused=fused, how=how)
    _, b = _run(graph, 20, sampled=True, fused=fused, how=how)
    _assert_same(a, b)
    assert torch.isfinite(a["losses"]).all() and int(a["step_counter"][:, 0].min()) > 0  # (16 marches, samples on each)
    assert int(a["step_counter"][:, 1].min()) == RAYS == int(a["step_counter"][:, 1].max())
    if graph:
        assert tr.graph and tr.graph_error is None and len(tr._graphs) >= 1


# ------------------------------------------------------------------------------------------------ 7. step_sampled = step
def test_step_sampled_equals_step_through_the_capacity_ladder():
    tr, a = _run(True, 40, sampled=True)
    _, b = _run(True, 40, sampled=False)
    assert tr.graph and tr.graph_error is None and len(tr._graphs) >= 1
    _assert_same(a, b)


def test_a_replay_never_marches_the_other_way():
    """The module attribute is part of the captured steps' key: flipping it between steps captures a new step, flipping it
    back replays the first one."""
    flag = lambda key: key[key.index("ordered_march") + 1]
    s = _sampler(_sequence(F=3, H=16, W=32, seed=4), num_rays=RAYS, patch_size=1, seed=17)
    assert s.n == RAYS
    s.new_epoch()
    tr = _trainer(True, how="attribute")
    torch.manual_seed(11)
    for _ in range(18):  # 16 launch by launch, then captured
        tr.step_sampled(s)
    n = len(tr._graphs)
    assert tr.graph_error is None and n >= 1 and all(flag(k) is True for k in tr._graphs)
    tr.model.ordered_march = False
    tr.step_sampled(s)
    assert tr.graph_error is None and len(tr._graphs) == n + 1 and sum(flag(k) is False for k in tr._graphs) == 1
    tr.model.ordered_march = True
    tr.step_sampled(s)
    assert tr.graph_error is None and len(tr._graphs) == n + 1


# ------------------------------------------------------------------------------------------------ 8. update_extra_state
def _updates(n, snapshot_at=None):
    net = _net().train()
    torch.manual_seed(23)
    snap = None
    with torch.autocast("cuda", dtype=torch.float16):
        for i in range(n):
            if i == snapshot_at:
                snap = (net.density_grid.clone(), torch.cuda.get_rng_state())
            net.update_extra_state()
            if i == snapshot_at:
                snap += (net.density_grid.clone(),)
    return net, snap


def test_update_extra_state_takes_the_maximum_of_duplicated_cells():
    """18 updates (16 full sweeps, two partial ones that draw cells with repetition) on two models of one seed: the same
    grid; and update 17 against a host restatement — the same draws, every cell the maximum of its candidates."""
    from lidarnerf import raymarching
    a, (grid16, rng, grid17) = _updates(18, snapshot_at=16)
    b, _ = _updates(18)
    assert a.iter_density == 18 and torch.equal(a.density_grid, b.density_grid)
    assert torch.equal(a.density_bitfield, b.density_bitfield)
    # update 17 again, by hand: the draws of update_extra_state's partial branch from the saved generator state
    G, n, decay = a.grid_size, a.grid_size ** 3 // 4, 0.95
    torch.cuda.set_rng_state(rng)
    tmp = np.full(tuple(grid16.shape), -1.0, np.float32)
    duplicated = differing = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for cas in range(a.cascade):
            coords = torch.randint(0, G, (n, 3), dtype=torch.int32, device="cuda")
            indices = raymarching.morton3D(coords).long()
            occ = torch.nonzero(grid16[cas] > 0).squeeze(-1)
            assert occ.numel() > 0
            occ = occ[torch.randint(0, occ.shape[0], (n,), device="cuda")]
            coords = torch.cat([coords, raymarching.morton3D_invert(occ.int())], 0).contiguous()
            indices = torch.cat([indices, occ], 0)
            bound = min(2 ** cas, a.bound)
            half = bound / G
            xyzs = (2 * coords.float() / (G - 1) - 1) * (bound - half)
            xyzs = xyzs + (torch.rand_like(xyzs) * 2 - 1) * half
            sig = (a.density(xyzs)["sigma"].reshape(-1).detach().float() * a.density_scale).cpu().numpy()
            idx = indices.cpu().numpy()
            np.maximum.at(tmp[cas], idx, sig)
            order = np.argsort(idx, kind="stable")
            si, ss = idx[order], sig[order]
            same = si[1:] == si[:-1]
            duplicated += int(same.sum())
            differing += int((same & (ss[1:] != ss[:-1])).sum())
    assert duplicated > 1000 and differing > 0  # (cells whose winner an indexed assignment would leave open)
    g16, t = grid16.cpu(), torch.from_numpy(tmp)
    want = torch.where((g16 >= 0) & (t >= 0), torch.maximum(g16 * decay, t), g16)
    assert torch.equal(grid17.cpu(), want)


# ------------------------------------------------------------------------------------------------ 9. same render
def test_eval_render_is_the_arrival_order_render_per_ray():
    """One 66 x 1030 frame in eval mode through the modular chain (fused_lidar=False: density() and color() sample by sample,
    no fused node; each ray's compositing reads only its own rows), under the fp16 autocast the trainer evaluates with: the
    keyword on against off.  (Under autocast every kernel between the marcher and the compositor is this library's and computes
    a row from that row alone.  In fp32 the MLPs of the modular chain are the BLAS library's GEMMs, whose result for a row
    depends on where the row sits in the matrix: there the two layouts agree to rounding only.)"""
    net = _net(ordered=False, fused=False).train()
    torch.manual_seed(5)
    with torch.autocast("cuda", dtype=torch.float16):
        for _ in range(2):
            net.update_extra_state()
    net.eval()
    data = _sampler(_sequence(F=3, H=66, W=1030, seed=4), num_rays=16).frame(0)
    o, d = data["rays_o_lidar"], data["rays_d_lidar"]
    assert o.shape == (1, 66 * 1030, 3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        off = net.render(o, d, cal_lidar_color=True, staged=False, perturb=False)
        on = net.render(o, d, cal_lidar_color=True, staged=False, perturb=False, ordered_march=True)
    for k in ("depth_lidar", "image_lidar", "weights_sum_lidar"):
        differ = int((on[k].reshape(66 * 1030, -1) != off[k].reshape(66 * 1030, -1)).any(-1).sum())
        print(f"[eval render, ordered against arrival order] {k}: {differ} of {66 * 1030} rays differ, "
              f"max |diff| {float((on[k].float() - off[k].float()).abs().max()):.3e}")
        assert torch.equal(on[k], off[k]), k
    assert float(on["weights_sum_lidar"].max()) > 0 and float(on["depth_lidar"].max()) > 0
