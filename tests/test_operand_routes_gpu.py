"""GPU: every reachable conv route of the inference plan keeps the arithmetic of its operand mode (include/stabnet_hip.h,
stabnet_net_set_bf16_operands).  The plan switches are read once per process, so each (mode, switch set) runs in a fresh child
(tests/operand_route_child.py) at the shapes (1, 96, 160) and (2, 72, 136) -- ragged tiles -- and one deploy step.  Per route:
  a. precision class: theta against a FLOAT64 evaluation of the same float32 parameters and input (oracle/torch_ref.py) within
     the f32 bar in modes 0, 2, 3, 4; mode 1 (bf16 operands) measurably off it, within its own 3e-3, and at least 5x the f32 bar
     away from it (the bar cannot drift into bf16 territory);
  b. kernel class: every conv record of the Profiler names an instantiation of the mode (BF16 template argument = the mode;
     mode 4 also runs the exact-f32 kernels wherever no packed kernel takes a launch);
  c. launch accounting: the records of one forward / one deploy step equal stabnet_net_num_launches /
     stabnet_deploy_frame_launches (counted from the routes the launcher takes: the steps bound to placeholders);
  d. the same bits every time;
  e. guard bands: `fold` and the workspace carry 64 KiB canary tails beyond their queried sizes, `fold` is NaN before
     stabnet_net_fold_bn and the workspace NaN before every forward -- theta stays finite and within (a);
  f. the same kernels: the ordered Profiler names of the forward at both shapes and of the deploy step equal
     tests/golden/conv_routes.json, recorded (twice, with equal results) with this child before conv_route() became the single routing
     decision of conv.hip.  A change that moves a launch to another kernel has to say so by recording the fixture again.
One more comparison across routes: in mode 1 the B2B plan runs its fused steps as their two plain convolutions, through the code of any
conv step -- the launches and arguments of the default plan, so theta and the Profiler names are the default plan's, `==`."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 96, 160), (2, 72, 136)]

# theta error against float64: mode 0 measures 1.1e-7 at both shapes; bf16 operands must sit >= 5x above (test_mode1_is_off_the_f32_bar)
F32_BAR = 2e-6
BF16_BAR = 3e-3

SWITCHES = {
    "default": {},
    "b2b": {"STABNET_CONV_B2B_PLAN": "1"},
    "no_packed_kg2": {"STABNET_CONV_PACKED_KG2": "0"},
    "no_packed_pro": {"STABNET_CONV_PACKED_PRO": "0"},
    "no_packed_kg3": {"STABNET_CONV_PACKED_KG3": "0"},
    "no_kgroups": {"STABNET_CONV_KGROUPS": "0", "STABNET_CONV_KGROUPS_PRO": "0"},
    "no_ring": {"STABNET_CONV_RING": "0"},
    "no_tuning_table": {"STABNET_CONV_TUNING_TABLE": "0"},
}
ROUTES = [(m, k) for m in (0, 4) for k in SWITCHES] + [(m, k) for m in (1, 2, 3) for k in ("default", "b2b")]


def _ring(mode, bf16, kg=1, pro=0):
    return "conv_ring_f32_kernel<%d, %d, %d, %d>" % (mode, bf16, kg, pro)


def _ring_family(b):
    """The conv_ring_f32_kernel<MODE, BF16, KG, PRO> instantiations the launcher runs with operand argument b (conv.hip): the ring
    launch (MODE 0 / 1 / 2 = 1x1 / padded / row-run), three K groups (MODE 0 / 1), the fragment prologue (one / two K groups)."""
    return {_ring(m, b) for m in (0, 1, 2)} | {_ring(0, b, 3), _ring(1, b, 3), _ring(0, b, 1, 1), _ring(0, b, 2, 1)}


# the packed split kernel (PK_KERNEL_CONV_PACKED, conv.hip conv_prof_kind_name): <MODE, 4, KG, PRO>
PACKED = {_ring(m, 4) for m in (0, 1, 2)} | {_ring(0, 4, 1, 1), _ring(0, 4, 2, 0), _ring(1, 4, 2, 0), _ring(0, 4, 2, 1)}
B2B = {"conv_b2b_f32_kernel<2>", "conv_b2b_f32_kernel<4>"}
IGEMM = re.compile(r"conv_igemm_f32_kernel<\d+, \d+, \d+, \d+, \d+, \d, \d, (\d)>$")
# mode -> (allowed ring / fused names, allowed BF16 arguments of the register-staged kernel)
ALLOWED = {
    0: (_ring_family(0) | B2B, {0}),
    1: ({_ring(m, 1) for m in (0, 1, 2)}, {1}),          # (no K groups and no PRO form on bf16 operands: conv.hip conv_route)
    2: (_ring_family(2), {2}),
    3: (_ring_family(3), {3}),
    4: (_ring_family(0) | B2B | PACKED, {0}),
}
NON_CONV = {"pad_channels_kernel", "max_pool_kernel", "gap_bn_relu_partial_kernel", "fc_kernel", "theta_mesh_kernel",
            "mesh_homography_kernel", "conv_splitk_reduce_kernel", "stack_assemble_bordered_kernel", "warp_sample_kernel",
            "ring_push_kernel"}


def _bad_names(names, mode):
    allowed, igemm_bf16 = ALLOWED[mode]
    bad = []
    for n in names:
        if n in NON_CONV or n in allowed:
            continue
        m = IGEMM.match(n)
        if m and int(m.group(1)) in igemm_bf16:
            continue
        bad.append(n)
    return bad


def _launches(names):
    """Kernel launches behind the Profiler records of a forward: one record per plan step, and the GAP step is two kernels (the
    partial sums, then gap_finalize_kernel or -- the shortened head -- fc_1 reading the partials; net.hip run_forward)."""
    return len(names) + sum(n == "gap_bn_relu_partial_kernel" for n in names)


def _mode_is_on(names, mode, switches):
    """At least one conv launch carries the mode's own operand argument (mode 0: nothing to show; mode 4 without the ring kernel:
    no packed kernel takes a launch, every conv runs exact f32)."""
    if mode == 0 or (mode == 4 and switches == "no_ring"):
        return True
    if mode == 4:
        return any(n in PACKED for n in names)
    return any(n.startswith("conv_ring_f32_kernel<") and n.split(", ")[1] == str(mode) or
               (IGEMM.match(n) and IGEMM.match(n).group(1) == str(mode)) for n in names)


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """theta of the float64 evaluation (oracle/torch_ref.py, moving-average BN) of the child's float32 params and input."""
    import torch
    from oracle import stabnet_oracle as O
    from oracle import torch_ref as T
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    N, H, W = shape
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    x = np.random.default_rng(11).uniform(-0.5, 0.5, (N, H, W, cfg.in_ch)).astype(np.float32)
    with torch.no_grad():
        theta, _, _ = T.get_resnet(T.t(x), {k: T.t(v) for k, v in P.items()}, O.Config(height=H, width=W), False)
    return x, theta.numpy()


@functools.lru_cache(maxsize=None)
def _child(mode, switches, tmp):
    out = os.path.join(tmp, "route_%d_%s.npz" % (mode, switches))
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_CONV_B2B_MIN_TILES="1", **SWITCHES[switches])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "operand_route_child.py"), out, str(mode)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@functools.lru_cache(maxsize=None)
def _recorded_routes():
    """route id -> the three recorded name sequences (forward at SHAPES[0], at SHAPES[1], deploy step) of tests/golden/conv_routes.json:
    one table of distinct kernel names, and per route three lists of indices into it."""
    with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as fh:
        rec = json.load(fh)
    return {rid: [[rec["names"][i] for i in seq] for seq in seqs] for rid, seqs in rec["routes"].items()}


def _errors(d):
    errs = []
    for si, shape in enumerate(SHAPES):
        x, want = _reference(shape)
        assert np.array_equal(d["x_%d" % si], x)
        errs.append(float(np.abs(d["theta_%d" % si].astype(np.float64) - want).max()))
    return errs


@pytest.mark.parametrize("mode,switches", ROUTES, ids=["mode%d-%s" % r for r in ROUTES])
def test_route_keeps_its_operand_mode(cuda, tmp_path_factory, mode, switches):
    d = _child(mode, switches, str(tmp_path_factory.getbasetemp()))
    errs = _errors(d)
    print("mode %d %s: theta max error vs float64 %s; launches %s" % (
        mode, switches, ["%.3e" % e for e in errs], [int(d["launches_%d" % si]) for si in range(len(SHAPES))]))
    problems = []
    for si, shape in enumerate(SHAPES):
        theta, names = d["theta_%d" % si], [str(n) for n in d["names_%d" % si]]
        # a. precision class
        if not np.isfinite(theta).all():
            problems.append("%s: non-finite theta" % (shape,))
        elif mode == 1:
            if not (1e-6 < errs[si] <= BF16_BAR):
                problems.append("%s: bf16-operand theta error %.3e outside (1e-6, %g]" % (shape, errs[si], BF16_BAR))
        elif errs[si] >= F32_BAR:
            problems.append("%s: theta error %.3e >= the f32 bar %g" % (shape, errs[si], F32_BAR))
        # b. kernel class
        bad = _bad_names(names, mode)
        if bad:
            problems.append("%s: kernels outside mode %d: %s" % (shape, mode, sorted(set(bad))))
        if "?" in names:
            problems.append("%s: unnamed Profiler kind" % (shape,))
        if not _mode_is_on(names, mode, switches):
            problems.append("%s: no conv launch in mode %d" % (shape, mode))
        # c. launch accounting (kernel launches; the GAP step's record covers two)
        n_rec = _launches(names)
        # (counted before the forward, after it, and -- first shape -- after a forward in another operand mode on the same thread: the
        # model must not depend on the mode the thread's last conv launch left)
        keys = ("launches_before_%d" % si, "launches_%d" % si) + (("launches_cross_0",) if si == 0 else ())
        for key in keys:
            if int(d[key]) != n_rec:
                problems.append("%s: %s = %d, the forward ran %d launches" % (shape, key, int(d[key]), n_rec))
        # d. repeatability (the workspace NaN before each forward; the third forward under the Profiler)
        if not (np.array_equal(theta, d["theta2_%d" % si]) and np.array_equal(theta, d["theta3_%d" % si])):
            problems.append("%s: theta differs between forwards" % (shape,))
        # e. guard bands
        for key in ("fold_tail_bad_%d" % si, "ws_tail_bad_%d" % si):
            if int(d[key]):
                problems.append("%s: %d words of the canary tail behind %s overwritten" % (shape, int(d[key]), key))
    dep = [str(n) for n in d["deploy_names"]]
    if _launches(dep) != int(d["deploy_launches"]):
        problems.append("deploy step: stabnet_deploy_frame_launches = %d, ran %d" % (int(d["deploy_launches"]), _launches(dep)))
    bad = _bad_names(dep, mode)
    if bad:
        problems.append("deploy step: kernels outside mode %d: %s" % (mode, sorted(set(bad))))
    # f. the recorded kernel sequence
    ran = [[str(n) for n in d["names_%d" % si]] for si in range(len(SHAPES))] + [dep]
    for what, got, want in zip(["%s" % (s,) for s in SHAPES] + ["deploy step"], ran, _recorded_routes()["mode%d-%s" % (mode, switches)]):
        if got != want:
            first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
            problems.append("%s: %d launches recorded, %d ran; first difference at launch %d: recorded %s, ran %s" % (
                what, len(want), len(got), first, want[first:first + 1], got[first:first + 1]))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("switches", ["default", "b2b"])
def test_mode1_is_off_the_f32_bar(cuda, tmp_path_factory, switches):
    """The f32 bar sits at least 5x below the bf16-operand error at the same shapes: a route that falls back to bf16 operands
    cannot pass (a) by luck."""
    errs = _errors(_child(1, switches, str(tmp_path_factory.getbasetemp())))
    print("mode 1 %s: theta max error vs float64 %s (f32 bar %g)" % (switches, ["%.3e" % e for e in errs], F32_BAR))
    assert min(errs) >= 5 * F32_BAR, errs


def test_mode1_b2b_plan_is_the_default_plan(cuda, tmp_path_factory):
    """STABNET_CONV_B2B_PLAN=1 (MIN_TILES=1: all seven units of blocks 1 and 2) in operand mode 1: every fused step runs as conv2 then conv3,
    the same launches with the same arguments as the default plan makes -- equal theta bits and equal Profiler name lists, forward (both
    shapes) and deploy step."""
    tmp = str(tmp_path_factory.getbasetemp())
    b2b, plain = _child(1, "b2b", tmp), _child(1, "default", tmp)
    for si, shape in enumerate(SHAPES):
        assert np.array_equal(b2b["x_%d" % si], plain["x_%d" % si])
        assert np.array_equal(b2b["theta_%d" % si], plain["theta_%d" % si]), shape
        assert [str(n) for n in b2b["names_%d" % si]] == [str(n) for n in plain["names_%d" % si]], shape
        assert int(b2b["launches_%d" % si]) == int(plain["launches_%d" % si])
    assert [str(n) for n in b2b["deploy_names"]] == [str(n) for n in plain["deploy_names"]]
