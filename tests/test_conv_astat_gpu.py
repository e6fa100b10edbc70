"""GPU: the A-stationary packed kernel (conv_astat_f32_kernel<BM>, csrc/conv_astat_kernel.h) computes what the packed ring kernel
computes, bit for bit, and conv_route() sends it only the launches its rule names.  The conv switches are read once per process, so
every arm is a fresh child (tests/conv_astat_child.py); the forced arms run with STABNET_CONV_ASTAT_MIN_M=1 and no K split
(STABNET_CONV_TILE=2 makes STABNET_CONV_SPLITK=1 effective: the 64x64 tile is the built-in choice anyway), and -- so that EVERY case
reaches the new kernel when the route is on and the packed ring kernel when it is off -- with STABNET_CONV_ASTAT_MIN_COUT=1 (the
rule's Cout >= 256 would keep the 64- and 96-channel cases on the ring kernel in both arms) and STABNET_CONV_LOWK_IGEMM=0 (the dense
K = 64 case would run the exact-f32 register-staged kernel in both arms).  Which kernel a case ran is conv_route()'s own answer
(stabnet_conv2d_packed_kind), asserted per case.
  1. bitwise equality of ops.conv2d_packed under STABNET_CONV_ASTAT=1 (each tile height that ships) and =0, on the smallest shapes
     at which the kernel can go wrong (conv_astat_child.CASES);
  2. the bars of tests/test_conv_packed_gpu.py on the same outputs: 2e-5 of the output scale against oracle.conv2d (4e-5 with an
     output BN), 4e-6 against ops.conv2d;
  3. a regressor forward at (1, 96, 160) with the route forced on names the kernel, keeps stabnet_net_num_launches equal to the
     record count, gives the theta of the STABNET_CONV_ASTAT=0 child bit for bit, within 2e-6 of the float64 evaluation;
  4. with default switches no launch at (1, 96, 160) takes the new kernel (M <= 1224 there: below the smallest M of the rule), at
     (1, 360, 640) at least one does (block 2: M = 3600);
  5. one deploy step at 360 x 640 with default switches: theta, maps and output image equal bit for bit with and without the route;
  6. the N-group count follows the usable CUs (stabnet_conv_reserve_cus; conv.hip launch_astat): conv_astat_child.GRID_CASE with all,
     37 and CUs / 8 usable CUs runs the most, two (the second shorter) and one group, every time the bits of the ring kernel."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conv_astat_child import CASES, GRID_CASE, case_data, forward_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "conv_astat_f32_kernel<"
BMS = (32,)                                                # every tile height the library ships
FORCED = {"STABNET_CONV_ASTAT_MIN_M": "1", "STABNET_CONV_ASTAT_MIN_COUT": "1", "STABNET_CONV_LOWK_IGEMM": "0",
          "STABNET_CONV_TILE": "2", "STABNET_CONV_SPLITK": "1"}
RING = "conv_ring_f32_kernel<0, 4, 1, 0>"                  # what every case runs with the route off
ARMS = {
    "on32": (dict(FORCED, STABNET_CONV_ASTAT="1"), ("ops", "forward", "grid:37")),
    "off": (dict(FORCED, STABNET_CONV_ASTAT="0"), ("ops", "forward", "grid:37")),
    "default": ({}, ("routes", "deploy")),
    "default_off": ({"STABNET_CONV_ASTAT": "0"}, ("deploy",)),
}
F32_BAR = 2e-6                                             # theta against float64 (tests/test_operand_routes_gpu.py)


@functools.lru_cache(maxsize=None)
def _child(arm, tmp):
    env_add, parts = ARMS[arm]
    out = os.path.join(tmp, "astat_%s.npz" % arm)
    env = {k: v for k, v in os.environ.items() if not k.startswith("STABNET_CONV_")}
    env.update(env_add, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_astat_child.py"), out] + list(parts), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@functools.lru_cache(maxsize=None)
def _oracle(i):
    """oracle.conv2d (+ residual, output BN, ReLU) of case i, evaluated once."""
    from oracle import stabnet_oracle as O
    d, case = case_data(i), CASES[i]
    want = O.conv2d(d["x"], d["w"], 1, ((0, 0), (0, 0)), d["b"])
    if case[6] == 1:
        want = want + d["r"]
    elif case[6] == 2:
        want = want + d["r"][:, ::2, ::2, :]
    if case[7]:
        want = (want * d["osc"] + d["osh"]).astype(np.float32)
    if case[8]:
        want = np.maximum(want, 0)
    return want


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%dx%dx%d-%d" % c[:5] for c in CASES])
def test_bitwise_equal_to_the_ring_kernel(cuda, tmp_path_factory, i, bm):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("on%d" % bm, tmp), _child("off", tmp)
    assert str(on["kernel_%d" % i]) == KERNEL + "%d>" % bm, str(on["kernel_%d" % i])
    assert str(off["kernel_%d" % i]) == RING, str(off["kernel_%d" % i])
    assert on["got_%d" % i].shape == off["got_%d" % i].shape
    assert np.array_equal(on["got_%d" % i], off["got_%d" % i])


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%dx%dx%d-%d" % c[:5] for c in CASES])
def test_keeps_the_bars_of_the_packed_kernels(cuda, tmp_path_factory, i, bm):
    d = _child("on%d" % bm, str(tmp_path_factory.getbasetemp()))
    assert str(d["kernel_%d" % i]) == KERNEL + "%d>" % bm, str(d["kernel_%d" % i])
    got, f32, want = d["got_%d" % i], d["f32_%d" % i], _oracle(i)
    assert got.shape == want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= (4e-5 if CASES[i][7] else 2e-5) * scale, "max err vs oracle %g (scale %g)" % (err, scale)
    diff = np.abs(got - f32).max()
    assert diff <= 4e-6 * scale, "max difference to the exact-f32-MFMA kernels %g (scale %g)" % (diff, scale)


@functools.lru_cache(maxsize=None)
def _theta64():
    """theta of the float64 evaluation (oracle/torch_ref.py) of the child's float32 parameters and input at (1, 96, 160)."""
    import torch
    from oracle import stabnet_oracle as O
    from oracle import torch_ref as T
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    H, W = 96, 160
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    with torch.no_grad():
        theta, _, _ = T.get_resnet(T.t(forward_input(H, W, cfg.in_ch)), {k: T.t(v) for k, v in P.items()}, O.Config(height=H, width=W), False)
    return theta.numpy()


@pytest.mark.parametrize("bm", BMS)
def test_forward_runs_the_new_kernel(cuda, tmp_path_factory, bm):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("on%d" % bm, tmp), _child("off", tmp)
    names = [str(n) for n in on["names"]]
    assert any(n.startswith(KERNEL) for n in names), sorted(set(names))
    assert not any(str(n).startswith(KERNEL) for n in off["names"])
    assert "?" not in names
    # one record per plan step; the GAP step's record covers two kernels (tests/test_operand_routes_gpu.py)
    assert int(on["launches"]) == len(names) + sum(n == "gap_bn_relu_partial_kernel" for n in names)
    assert int(on["launches"]) == int(off["launches"])
    assert np.array_equal(on["theta"], off["theta"])
    err = float(np.abs(on["theta"].astype(np.float64) - _theta64()).max())
    print("theta max error vs float64: %.3e" % err)
    assert err < F32_BAR


def _groups(usable, mtiles, nblk):
    """conv.hip launch_astat: (N groups, 32-column blocks per group) of a launch with `usable` CUs."""
    cdiv = lambda a, b: -(-a // b)
    groups = min(cdiv(nblk, 4), max(1, 2 * usable // mtiles))
    per = 4 * cdiv(cdiv(nblk, groups), 4)
    return cdiv(nblk, per), per


@pytest.mark.parametrize("bm", BMS)
def test_n_groups_follow_the_usable_cus(cuda, tmp_path_factory, bm):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("on%d" % bm, tmp), _child("off", tmp)
    assert str(on["grid_kernel"]) == KERNEL + "%d>" % bm and str(off["grid_kernel"]) == RING
    N, H, W, Cin, Cout = GRID_CASE[:5]
    mtiles, nblk = -(-N * H * W // bm), 2 * -(-Cout // 64)
    usable = [int(u) for u in on["grid_usable"]]
    assert usable == [int(on["cus"]), 37, int(on["cus"]) // 8] and (N * H * W) % bm != 0 and Cout % 64 != 0
    counts = [_groups(u, mtiles, nblk) for u in usable]
    print("conv_astat_f32_kernel<%d>: M tiles %d, column blocks %d, (usable CUs, N groups, blocks per group) = %s" % (
        bm, mtiles, nblk, [(u,) + c for u, c in zip(usable, counts)]))
    assert len({g for g, _ in counts}) == 3 and counts[0][0] == -(-nblk // 4) and counts[2][0] == 1
    assert 1 < counts[1][0] < counts[0][0] and nblk % counts[1][1] != 0        # strictly between, its last group shorter than the others
    # the bars of the packed kernels, then bit for bit: every group count, and the ring kernel at the same usable CUs
    from oracle import stabnet_oracle as O
    d = case_data(-1)
    want = np.maximum(O.conv2d(d["x"], d["w"], 1, ((0, 0), (0, 0)), d["b"]) + d["r"], 0)
    scale = np.abs(want).max()
    for u in usable:
        got = on["grid_%d" % u]
        assert np.abs(got - want).max() <= 2e-5 * scale, u
        assert np.array_equal(got.view(np.uint32), on["grid_%d" % usable[0]].view(np.uint32)), u
        assert np.array_equal(got.view(np.uint32), off["grid_%d" % u].view(np.uint32)), u


def test_default_routing_leaves_small_shapes_alone(cuda, tmp_path_factory):
    d = _child("default", str(tmp_path_factory.getbasetemp()))
    assert not [str(n) for n in d["names_small"] if KERNEL in str(n)]
    assert [str(n) for n in d["names_large"] if KERNEL in str(n)]


def test_deploy_step_is_bitwise_unchanged(cuda, tmp_path_factory):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("default", tmp), _child("default_off", tmp)
    for k in ("deploy_theta", "deploy_x_map", "deploy_y_map", "deploy_output"):
        assert on[k].shape == off[k].shape and np.array_equal(on[k], off[k]), k
