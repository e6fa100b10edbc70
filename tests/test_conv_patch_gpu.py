"""GPU: the patch-stationary packed kernel (conv_patch_f32_kernel<PH, PW, WR, NS>, csrc/conv_patch_kernel.h) computes what the packed ring
kernel computes, bit for bit, and conv_route() sends it only the launches its rule names.  The conv switches are read once per
process, so every arm is a fresh child (tests/conv_patch_child.py); the forced arms run with STABNET_CONV_PATCH_MIN_M=1, one arm per
form the library ships (STABNET_CONV_PATCH_CFG: the rule picks between them); the K split is the call's own argument (1, or 2
for the two-K-half cases; STABNET_CONV_TILE=2 / STABNET_CONV_SPLITK=1 keep the plan's own choice out of it).  Which kernel a case ran is conv_route()'s own answer
(stabnet_conv2d_packed_kind), asserted per case.
  1. bitwise equality of the packed convolution with the route on (each form) and STABNET_CONV_PATCH=0, on the smallest shapes at which
     the kernel can go wrong (conv_patch_child.CASES), NaN around and beside the input, canaries around the output;
     and the same for the launches the ring kernel runs as two K halves inside the workgroup (splitk = 2, conv_patch_child.KG2);
  2. the bars of tests/test_conv_packed_gpu.py on the same outputs: 2e-5 of the output scale against oracle.conv2d (4e-5 with an
     output BN), 4e-6 against ops.conv2d;
  3. with default switches no launch of a forward at (1, 96, 160) takes the new kernel (M <= 1224 there), at (1, 360, 640) at least one
     does (block 1's conv2: M = 14400); the Profiler's record count is stabnet_net_num_launches in both;
  4. one deploy step at 360 x 640 with default switches: theta, maps and output image equal bit for bit with and without the route;
  5. the same input twice gives equal bits, and so does the replay of a captured graph;
  6. the N-group count follows the usable CUs (stabnet_conv_reserve_cus; conv.hip launch_patch_one): conv_patch_child.GRID_CASE with
     all, 37 and CUs / 8 usable CUs runs the most, two (the second shorter) and one group, every time the bits of the ring kernel."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conv_patch_child import CASES, GRID_CASE, KG2, case_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "conv_patch_f32_kernel<"
# STABNET_CONV_PATCH_CFG -> <PH, PW, WR, NS>: every form the library ships
FORMS = {1: (8, 8, 1, 3), 2: (8, 8, 2, 3)}
FORCED = {"STABNET_CONV_PATCH_MIN_M": "1", "STABNET_CONV_TILE": "2", "STABNET_CONV_SPLITK": "1"}
RING = {"": "conv_ring_f32_kernel<1, 4, 1, 0>", "2": "conv_ring_f32_kernel<1, 4, 2, 0>"}     # what a case runs with the route off
# (test id, case, "" / "2": no K split / two K halves)
RUNS = ([("%dx%dx%dx%d-%d+%d" % CASES[i][:6], i, "") for i in range(len(CASES))] +
        [("%dx%dx%dx%d-%d+%d-halves" % CASES[i][:6], i, "2") for i in KG2])
ARMS = {
    "on1": (dict(FORCED, STABNET_CONV_PATCH="1", STABNET_CONV_PATCH_CFG="1"), ("ops", "ops2", "twice", "grid:37")),
    "on2": (dict(FORCED, STABNET_CONV_PATCH="1", STABNET_CONV_PATCH_CFG="2"), ("ops", "ops2", "twice", "grid:37")),
    "off": (dict(FORCED, STABNET_CONV_PATCH="0"), ("ops", "ops2", "grid:37")),
    "default": ({}, ("routes", "deploy")),
    "default_off": ({"STABNET_CONV_PATCH": "0"}, ("deploy",)),
}


def _kernel(cfg, i, t):
    """The kernel case i runs under form cfg: the form if its halo patch fits the 160 KiB of LDS (conv_patch_kernel.h), else the ring kernel."""
    ph, pw, wr, ns = FORMS[cfg]
    pixel = 6 * CASES[i][3] + 16
    row = (((pw + 2) * pixel + 127) & ~255) + 128
    return KERNEL + "%d, %d, %d, %d>" % FORMS[cfg] if (ph + 2) * row + 4 * 4096 <= 160 * 1024 else RING[t]


@functools.lru_cache(maxsize=None)
def _child(arm, tmp):
    env_add, parts = ARMS[arm]
    out = os.path.join(tmp, "patch_%s.npz" % arm)
    env = {k: v for k, v in os.environ.items() if not k.startswith("STABNET_CONV_")}
    env.update(env_add, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_patch_child.py"), out] + list(parts), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@functools.lru_cache(maxsize=None)
def _oracle(i):
    """oracle.conv2d (+ output BN, ReLU) of case i, evaluated once."""
    from oracle import stabnet_oracle as O
    d, case = case_data(i), CASES[i]
    want = O.conv2d(d["x"], d["w"], 1, ((1, 1), (1, 1)), d["b"])
    if case[7]:
        want = (want * d["osc"] + d["osh"]).astype(np.float32)
    if case[8]:
        want = np.maximum(want, 0)
    return want


@pytest.mark.parametrize("cfg", sorted(FORMS))
@pytest.mark.parametrize("i,t", [r[1:] for r in RUNS], ids=[r[0] for r in RUNS])
def test_bitwise_equal_to_the_ring_kernel(cuda, tmp_path_factory, i, t, cfg):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("on%d" % cfg, tmp), _child("off", tmp)
    k = "%s_%d" % (t, i)
    assert str(on["kernel" + k]) == _kernel(cfg, i, t), str(on["kernel" + k])
    assert str(off["kernel" + k]) == RING[t], str(off["kernel" + k])
    assert int(on["guards" + k]) == 1 and int(off["guards" + k]) == 1, "write outside y"
    assert on["got" + k].shape == off["got" + k].shape
    assert np.isfinite(on["got" + k]).all(), "a read outside the input tensor (NaN) or an element never stored (canary)"
    assert np.array_equal(on["got" + k], off["got" + k])


@pytest.mark.parametrize("cfg", sorted(FORMS))
@pytest.mark.parametrize("i,t", [r[1:] for r in RUNS], ids=[r[0] for r in RUNS])
def test_keeps_the_bars_of_the_packed_kernels(cuda, tmp_path_factory, i, t, cfg):
    d = _child("on%d" % cfg, str(tmp_path_factory.getbasetemp()))
    k = "%s_%d" % (t, i)
    assert str(d["kernel" + k]) == _kernel(cfg, i, t), str(d["kernel" + k])
    got, f32, want = d["got" + k], d["f32" + k], _oracle(i)
    assert got.shape == want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("max err vs oracle %g, vs the exact-f32 kernels %g (scale %g)" % (err, np.abs(got - f32).max(), scale))
    assert err <= (4e-5 if CASES[i][7] else 2e-5) * scale, "max err vs oracle %g (scale %g)" % (err, scale)
    diff = np.abs(got - f32).max()
    assert diff <= 4e-6 * scale, "max difference to the exact-f32-MFMA kernels %g (scale %g)" % (diff, scale)


def _lds_bytes(cfg, Cin):
    """conv_patch_kernel.h sn_patch_lds_bytes of form cfg (as _kernel above)."""
    ph, pw, wr, ns = FORMS[cfg]
    return (ph + 2) * ((((pw + 2) * (6 * Cin + 16) + 127) & ~255) + 128) + 4 * 4096


def _groups(cfg, usable, mtiles, nblk, Cin):
    """conv.hip launch_patch_one: (N groups, 32-column blocks per group) of a launch of form cfg with `usable` CUs."""
    cdiv = lambda a, b: -(-a // b)
    ph, pw, wr, ns = FORMS[cfg]
    cs = 4 // ((ph // 4) * (pw // 8) // wr)
    slots = min(1 if wr >= 4 else 2, 160 * 1024 // _lds_bytes(cfg, Cin)) * usable
    groups = min(cdiv(nblk, cs), max(1, slots // mtiles))
    per = cs * cdiv(cdiv(nblk, groups), cs)
    return cdiv(nblk, per), per


@pytest.mark.parametrize("cfg", sorted(FORMS))
def test_n_groups_follow_the_usable_cus(cuda, tmp_path_factory, cfg):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("on%d" % cfg, tmp), _child("off", tmp)
    assert str(on["grid_kernel"]) == KERNEL + "%d, %d, %d, %d>" % FORMS[cfg] and str(off["grid_kernel"]) == RING[""]
    N, H, W, Cin, Cout = GRID_CASE[:5]
    ph, pw = FORMS[cfg][:2]
    mtiles, nblk = N * -(-H // ph) * -(-W // pw), 2 * -(-Cout // 64)
    usable = [int(u) for u in on["grid_usable"]]
    assert usable == [int(on["cus"]), 37, int(on["cus"]) // 8] and H % ph != 0 and W % pw != 0 and Cout % 64 != 0
    counts = [_groups(cfg, u, mtiles, nblk, Cin) for u in usable]
    print("conv_patch_f32_kernel<%d, %d, %d, %d>: patches %d, column blocks %d, (usable CUs, N groups, blocks per group) = %s" % (
        FORMS[cfg] + (mtiles, nblk, [(u,) + c for u, c in zip(usable, counts)])))
    cs = 4 // ((ph // 4) * (pw // 8) // FORMS[cfg][2])
    assert len({g for g, _ in counts}) == 3 and counts[0][0] == -(-nblk // cs) and counts[2][0] == 1
    assert 1 < counts[1][0] < counts[0][0] and nblk % counts[1][1] != 0        # strictly between, its last group shorter than the others
    from oracle import stabnet_oracle as O
    d = case_data(-1)
    want = np.maximum(O.conv2d(d["x"], d["w"], 1, ((1, 1), (1, 1)), d["b"]), 0)
    scale = np.abs(want).max()
    for u in usable:
        got = on["grid_%d" % u]
        assert np.abs(got - want).max() <= 2e-5 * scale, u
        assert np.array_equal(got.view(np.uint32), on["grid_%d" % usable[0]].view(np.uint32)), u
        assert np.array_equal(got.view(np.uint32), off["grid_%d" % u].view(np.uint32)), u


def test_default_routing_leaves_small_shapes_alone(cuda, tmp_path_factory):
    d = _child("default", str(tmp_path_factory.getbasetemp()))
    small, large = [str(n) for n in d["names_small"]], [str(n) for n in d["names_large"]]
    assert not [n for n in small if KERNEL in n]
    assert [n for n in large if KERNEL in n]
    for names, launches in ((small, d["launches_small"]), (large, d["launches_large"])):
        assert "?" not in names
        # one record per plan step; the GAP step's record covers two kernels (tests/test_operand_routes_gpu.py)
        assert int(launches) == len(names) + sum(n == "gap_bn_relu_partial_kernel" for n in names)


def test_deploy_step_is_bitwise_unchanged(cuda, tmp_path_factory):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("default", tmp), _child("default_off", tmp)
    for k in ("deploy_theta", "deploy_x_map", "deploy_y_map", "deploy_output"):
        assert on[k].shape == off[k].shape and np.array_equal(on[k], off[k]), k


@pytest.mark.parametrize("cfg", sorted(FORMS))
def test_repeat_and_graph_replay_give_equal_bits(cuda, tmp_path_factory, cfg):
    d = _child("on%d" % cfg, str(tmp_path_factory.getbasetemp()))
    assert np.isfinite(d["first"]).all()
    assert np.array_equal(d["first"], d["again"])
    assert int(d["replay_guards"]) == 1
    assert np.array_equal(d["first"], d["replay"])
