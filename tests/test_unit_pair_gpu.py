"""GPU: conv_unit_pair_f32_kernel<F32A, BM> (csrc/conv_pair_kernel.h) -- a unit's conv3 and the next unit's conv1 as one launch --
computes what the two launches it replaces compute, bit for bit: the raw conv3 output and the conv1 output.  The conv switches are read
once per process, so every arm is a fresh child (tests/unit_pair_child.py).
  1. operator level (default switches): every case of unit_pair_child.CASES -- K1 64 (f32 form) and 128 (packed form), N1 256 and 512
     (two and four 128-channel passes), N2 64 and 128 (both tile heights), M = 99 (ragged last tile) and 2 x 99 (two images), a residual
     read with a pixel stride > N1 -- `==` against ops.conv2d_packed of the two convolutions, every output pre-filled with NaN; which
     kernels the three launches ran is asserted per case;
  2. a regressor forward at (1, 96, 160) in operand mode 4 on a NaN-filled workspace, with the M floor lowered and no K split (so that
     block 1's two pairs and block 2's three are eligible), asked to fuse and refused (STABNET_CONV_PAIR=0): theta, every activation
     tap and the whole workspace `==`; the Profiler's record count is stabnet_net_num_launches, the new kernel is named once per pair;
  3. the same for one deploy step (StabNetStream asks for the fusion itself): theta, maps and output `==`, the record count against
     stabnet_deploy_frame_launches."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from unit_pair_child import CASES, TAPS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "conv_unit_pair_f32_kernel<"
PLAN = {"STABNET_CONV_PAIR_MIN_M": "1", "STABNET_CONV_TILE": "2", "STABNET_CONV_SPLITK": "1"}
ARMS = {
    "ops": ({}, ("ops",)),
    "fused": (PLAN, ("forward", "deploy")),
    "plain": (dict(PLAN, STABNET_CONV_PAIR="0"), ("forward", "deploy")),
}
PAIRS = 5                                                  # block 1: two identity units, block 2: three
FORM = {64: "64", 128: "32"}                               # conv1's channels -> the kernel's BM


@functools.lru_cache(maxsize=None)
def _child(arm, tmp):
    env_add, parts = ARMS[arm]
    out = os.path.join(tmp, "unit_pair_%s.npz" % arm)
    env = {k: v for k, v in os.environ.items() if not k.startswith("STABNET_CONV_")}
    env.update(env_add, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unit_pair_child.py"), out] + list(parts), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _launches(names):
    """one record per plan step; the GAP step's record covers two kernels (tests/test_operand_routes_gpu.py)"""
    return len(names) + sum(n == "gap_bn_relu_partial_kernel" for n in names)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx99-k%d-n%d-n%d-r%d" % c[:5] for c in CASES])
def test_bitwise_equal_to_the_two_launches(cuda, tmp_path_factory, i):
    d = _child("ops", str(tmp_path_factory.getbasetemp()))
    N, K1, N1, N2, Cr, _ = CASES[i]
    k3, k1, kf = (str(k) for k in d["kernels_%d" % i])
    # the two launches are the kernels whose arithmetic the fused kernel repeats
    assert k3 == ("conv_igemm_f32_kernel<64, 64, 32, 32, 32, 0, 2, 0>" if K1 == 64 else "conv_ring_f32_kernel<0, 4, 1, 0>"), k3
    assert k1 == "conv_ring_f32_kernel<0, 4, 1, 1>", k1
    assert kf == KERNEL + "%d, %s>" % (1 if K1 == 64 else 0, FORM[N2]), kf
    for what in ("3", "1"):
        got, ref = d["got" + what + "_%d" % i], d["ref" + what + "_%d" % i]
        assert got.shape == ref.shape
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, "conv%s: %d elements differ, first at %s" % (what, len(bad), bad[0])
        assert np.array_equal(_bits(got), _bits(ref))


def test_forward_is_bitwise_unchanged_and_names_the_kernel(cuda, tmp_path_factory):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("fused", tmp), _child("plain", tmp)
    names, plain = [str(n) for n in on["names"]], [str(n) for n in off["names"]]
    assert "?" not in names
    assert sum(n.startswith(KERNEL) for n in names) == PAIRS, sorted(set(names))
    assert sum(n == KERNEL + "1, %s>" % FORM[64] for n in names) == 2 and sum(n == KERNEL + "0, %s>" % FORM[128] for n in names) == 3
    assert not any(n.startswith(KERNEL) for n in plain)
    assert int(on["launches"]) == _launches(names) and int(off["launches"]) == _launches(plain)
    assert int(on["launches"]) == int(off["launches"]) - PAIRS and int(on["steps"]) == int(off["steps"]) - PAIRS
    assert np.array_equal(_bits(on["theta"]), _bits(off["theta"])) and np.isfinite(on["theta"]).all()
    for tap in TAPS:
        k = "tap_" + tap.replace("/", "_")
        assert on[k].shape == off[k].shape and len(on[k]) > 0 and np.array_equal(on[k], off[k]), tap
    assert np.array_equal(on["workspace"], off["workspace"])


def test_deploy_step_is_bitwise_unchanged(cuda, tmp_path_factory):
    tmp = str(tmp_path_factory.getbasetemp())
    on, off = _child("fused", tmp), _child("plain", tmp)
    for k in ("deploy_theta", "deploy_x_map", "deploy_y_map", "deploy_output"):
        assert on[k].shape == off[k].shape and np.array_equal(_bits(on[k]), _bits(off[k])), k
    names, plain = [str(n) for n in on["deploy_names"]], [str(n) for n in off["deploy_names"]]
    assert sum(n.startswith(KERNEL) for n in names) == PAIRS and not any(n.startswith(KERNEL) for n in plain)
    assert int(on["deploy_launches"]) == _launches(names) and int(off["deploy_launches"]) == _launches(plain)
    assert int(on["deploy_launches"]) == int(off["deploy_launches"]) - PAIRS
    assert int(on["deploy_net_launches"]) == int(off["deploy_net_launches"]) - PAIRS
