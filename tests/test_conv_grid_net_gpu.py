"""Whole-network level of test_conv_grid_gpu.py: reserving CUs (stabnet_conv_reserve_cus) moves tiles between the workgroups of the
persistent conv grids and nothing else.

  1. The inference regressor in operand modes 0 and 4 at two sizes.  The row-run stem (conv_ring_f32_kernel<2, B, 1, 0>) is reached by
     no operator, so its two tile-count classes are asserted here, from the T and G of its Profiler record at 37 and at CUs / 8 usable
     CUs: (1, 96, 160) gives 60 M tiles in two K slices, T = 120 (G < T < 2G for G = 111, 96, 74, 64); (1, 200, 344) gives 269 M
     tiles (the last of 48 rows), T = 538 (T >= 3G + 1, T % G != 0).  At the larger size block 1's 256-channel 1x1 convs walk
     several tiles per workgroup too.  theta with 37 and CUs / 8 usable CUs equals theta without a reservation bit for bit, and
     the Profiler's ordered kernel names are identical (the reservation moves no launch to another kernel).  The workspace is NaN
     before every forward.  The float64 bar of theta stays where it is, at the shapes of test_operand_routes_gpu.py.
  2. One training step (the fixture of test_train_gpu.py at batch 4) with the reservation set through the API: loss, theta and every
     gradient bit-identical to the unreserved step, and at least one ring launch of the step with more tiles than workgroups."""
import re

import numpy as np
import pytest
import torch

from _grid import U_ODD, cdiv, check_tile_classes, reservation  # noqa: F401  (reservation: a fixture)

pytestmark = pytest.mark.gpu

RING = re.compile(r"conv_ring_f32_kernel<(\d), (\d), (\d), (\d)>")


def ring_launches(prof, usable):
    """[(name, MODE, T, G, workgroups per CU)] of the ring launches in the Profiler's records: T tiles on G = min(T, workgroups per CU x usable CUs)
    workgroups (conv.hip launch_ring_route; 3 per CU, 2 of the packed kernel, 1 with K groups, whose K slices are no tiles)."""
    out = []
    for rec in prof.records_with_shapes():
        m = RING.match(rec[0])
        if not m:
            continue
        mode, operand, kg, _ = (int(v) for v in m.groups())
        M, Cout, _, splitk = rec[-1]
        T = cdiv(M, 64) * cdiv(Cout, 64) * (1 if kg > 1 else splitk)
        per_cu = 1 if kg > 1 else 2 if operand == 4 else 3
        out.append((rec[0], mode, T, min(T, per_cu * usable), per_cu))
    return out


@pytest.mark.parametrize("H,W,cls", [(96, 160, "a"), (200, 344, "b")])
@pytest.mark.parametrize("mode", [0, 4])
def test_regressor_forward_does_not_depend_on_the_grid(cuda, reservation, mode, H, W, cls):
    from stabnet_amd import _lib, synthetic
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import Profiler
    from stabnet_amd.regressor import Regressor
    L = _lib.lib()
    cus, grids = reservation
    N = 1
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    x = torch.from_numpy(np.random.default_rng(11).uniform(-0.5, 0.5, (N, H, W, cfg.in_ch)).astype(np.float32)).to(cuda)
    reg = Regressor(P, N, H, W, cfg, device=cuda, operand_mode=mode)
    prof = Profiler(max_records=4096, device=cuda)
    thetas, names, launches = {}, {}, {}
    try:
        for U, reserved in grids:
            L.stabnet_conv_reserve_cus(reserved)
            reg.workspace.view(torch.float32).fill_(float("nan"))        # no region may be read before this forward writes it
            theta = torch.full((N, cfg.n_theta), float("nan"), dtype=torch.float32, device=cuda)
            prof.reset()
            _lib.call("stabnet_backbone_fwd_infer", reg.plan.handle, ptr(reg.params), ptr(reg.fold), ptr(x), ptr(theta), ptr(reg.workspace),
                      reg.workspace.numel(), stream_ptr(cuda), prof.handle, device=cuda)
            torch.cuda.synchronize()
            thetas[U] = theta.cpu().numpy()
            names[U] = [r[0] for r in prof.records(raw=True)]
            launches[U] = ring_launches(prof, U)
    finally:
        L.stabnet_conv_reserve_cus(0)
    assert "?" not in names[cus] and names[cus]
    several = sorted({(n, T, G) for n, _, T, G, _ in launches[U_ODD] if T > G})
    print("mode %d, %d x %d, %d usable CUs: ring launches with more tiles than workgroups (kernel, T, G): %s" % (mode, H, W, U_ODD, several))
    # the row-run stem (MODE 2) in this size's tile class, at both reduced grids, from the T and G of its own launch
    stem = [(n, T, per_cu) for n, m, T, _, per_cu in launches[U_ODD] if m == 2]
    assert len(stem) == 1 and stem[0][0] == "conv_ring_f32_kernel<2, %d, 1, 0>" % mode, stem
    table = check_tile_classes(cls, stem[0][1], stem[0][2], [u for u, _ in grids[1:]], stem[0][0])
    assert [g for n, m, T, g, _ in launches[U_ODD] if m == 2] == [table[0][2]] and [g for n, m, T, g, _ in launches[cus // 8] if m == 2] == [table[1][2]]
    print("%s: (U, T, G) = %s" % (stem[0][0], table))
    if cls == "b":         # block 1's 256-channel 1x1 convs walk several tiles per workgroup on a grid that is no multiple of 8
        assert [1 for n, m, T, G, _ in launches[U_ODD] if m == 0 and T >= 240 and T > G and G & 7], launches[U_ODD]
    for U, _ in grids:
        assert np.isfinite(thetas[U]).all()
        assert names[U] == names[cus], "U=%d: the reservation moved a launch to another kernel" % U
        assert np.array_equal(thetas[U].view(np.uint32), thetas[cus].view(np.uint32)), (U, np.abs(thetas[U] - thetas[cus]).max())


def test_training_step_does_not_depend_on_the_grid(cuda, reservation):
    from stabnet_amd import _lib, synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import Profiler
    from stabnet_amd.train import Trainer
    L = _lib.lib()
    cus, grids = reservation
    N, H, W = 4, 64, 96                  # test_train_gpu.py's fixture with the batch enlarged until a ring launch has T > G
    cfg = Config(height=H, width=W, batch_size=N, max_matches=48)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    b = synthetic.make_train_batch(cfg, N, H, W, 5)
    b["flow"] = (b["flow"] + np.random.default_rng(1).normal(0, 0.02, b["flow"].shape)).astype(np.float32)
    dev_b = {k: torch.from_numpy(v).to(cuda) for k, v in b.items()}
    gates = {"use_theta_loss": 1, "use_temp_loss": 1, "use_black_loss": 1, "use_theta_only": 0}
    got = {}
    try:
        for U, reserved in grids:
            tr = Trainer(P, N, H, W, cfg, device=cuda)
            tr.prof = Profiler(max_records=16384, device=cuda)
            L.stabnet_conv_reserve_cus(reserved)
            tr.forward_backward(dev_b, gates, apply_update=False)
            torch.cuda.synchronize()
            got[U] = (tr.grad_flat().cpu().numpy().copy(), np.stack([t.cpu().numpy() for t in tr.theta]), tr.losses(),
                      ring_launches(tr.prof, U), [r[0] for r in tr.prof.records(raw=True)])
            L.stabnet_conv_reserve_cus(0)
            del tr
    finally:
        L.stabnet_conv_reserve_cus(0)
    g0, th0, lo0, _, names0 = got[cus]
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    for U, (g, th, lo, rings, names) in got.items():
        if U != cus:
            several = sorted({(n, T, G) for n, _, T, G, _ in rings if T > G})
            print("%d usable CUs: ring launches of the step with more tiles than workgroups (kernel, T, G): %s" % (U, several))
            assert several, "no ring launch of the step has T > G: enlarge the batch"
        assert names == names0, "U=%d: the reservation moved a launch to another kernel" % U
        assert np.array_equal(th.view(np.uint32), th0.view(np.uint32)), U
        assert np.array_equal(g.view(np.uint32), g0.view(np.uint32)), (U, int((g.view(np.uint32) != g0.view(np.uint32)).sum()))
        assert lo == lo0, (U, lo, lo0)
