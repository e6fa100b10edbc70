"""CPU: the 32-bit range of the conv kernels ("Conv extents") is enforced where plans and strided operands are made.

The kernels address their operands with 32-bit offsets; tests/_extents.py restates, operand by operand and family by family, the largest
extent for which that arithmetic is exact.  Here:
  * per frame size, operand mode and fusion, the largest batch stabnet_net_create() accepts is found by bisection; every conv step of the
    accepted plan (and of the plan at half that batch) is inside its limits by _extents.py, the next batch is refused with a message that
    names the layer and the operand, and the boundary equals tests/golden/conv_extents.json (tools/conv_extents.py rewrites it);
  * _route_census.check_invariants, which had only seen batches up to 8, holds over the accepted boundary plans;
  * training plans: at the accepted batch the launch-time requirement of the weight gradient (conv_bwd.hip) cannot fire;
  * the three operator entries that take a pixel stride refuse one step past the limit and pass the shape check one step inside it, before
    any pointer is looked at (all pointers null: nothing can be launched);
  * Regressor and StabNetStream raise StabnetError before any device allocation.
Plans are host objects: no GPU."""
import ctypes as C
import json

import numpy as np
import pytest

import _extents as ex
import _extents_search as es
import _route_census as rc

LIMIT = 1 << 30
INFER = [(name, mode, pairs) for name, mode, pairs, b2b in es.CONFIGS if not b2b]


@pytest.fixture(scope="module")
def golden():
    with open(es.GOLDEN) as fh:
        return json.load(fh)


def _check_plan(p, fused_of=None):
    """Every conv step of plan `p` inside its limits; returns (rows [steps][fields], workspace bytes) of its conv steps."""
    rows = []
    for step in range(p.num_steps):
        info = p.info(step)
        if info["kind"] not in (ex.S_CONV, ex.S_CONV_PAIR):
            continue
        fused = "pair" if info["kind"] == ex.S_CONV_PAIR else None
        bad = ex.violations(info, fused)
        assert not bad, "N=%d %dx%d mode %d step %d outside the kernels' range: %s" % (p.N, p.H, p.W, p.mode, step, bad)
        rows.append([info[n] for n in rc.fields()])
    return np.array(rows, np.int64)


@pytest.mark.parametrize("H,W", es.SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,mode,pairs", INFER, ids=[c[0] for c in INFER])
def test_boundary_batch_of_an_inference_plan(golden, name, mode, pairs, H, W):
    N = es.boundary(mode, H, W, pairs)
    print("%s %dx%d: largest accepted batch %d" % (name, H, W, N))
    for n in sorted({N, max(1, N // 2)}):
        p, msg = es.make_plan(mode, n, H, W, pairs)
        assert p is not None, msg
        rows = _check_plan(p)
        if pairs and n == N:
            assert (rows[:, rc.col("kind")] == ex.S_CONV_PAIR).any(), "no fused unit pair in the boundary plan: the pair kernel's limits went unchecked"
        # the census' own invariants, so far only ever run at batches <= 8 (kind-6 rows describe the conv3 half as its own launch; the
        # grid fields are the fused launch's, which the census checks on S_CONV rows only)
        conv = rows[rows[:, rc.col("kind")] == ex.S_CONV]
        rc.check_invariants(conv, np.full(len(conv), p.workspace_bytes, np.int64))
        p.close()
    p, msg = es.make_plan(mode, N + 1, H, W, pairs)
    assert p is None, "N + 1 = %d accepted" % (N + 1)
    assert es.is_extent_refusal(msg), msg
    # the arithmetic of the issue: the merged shortcut | conv1 buffer of block 1, [N][H/4][W/4][320], read by conv2 with x_ld = 320
    h4, w4 = -(-H // 4), -(-W // 4)
    assert N * h4 * w4 * 320 < LIMIT <= (N + 1) * h4 * w4 * 320
    assert N == golden["inference"]["%dx%d" % (H, W)][name], "the boundary moved: run tools/conv_extents.py"


def test_expected_boundaries(golden):
    g = golden["inference"]
    assert {k: set(v.values()) for k, v in g.items()} == {"288x512": {364}, "720x1280": {58}, "1080x1920": {25}, "1079x1919": {25}, "2160x3840": {6}}
    assert golden["limit_floats"] == LIMIT and sorted(g) == sorted("%dx%d" % s for s in es.SIZES)
    assert all(sorted(v) == sorted(c[0] for c in es.CONFIGS) for v in g.values())


@pytest.mark.parametrize("mode", [0, 4])
def test_boundary_batch_with_back_to_back_units(golden, mode):
    """STABNET_CONV_B2B_PLAN=1 is read once per process: a child finds the boundaries and lists the step kinds; the rows of a kind-5 step's
    two halves come from the plan made here (without the switch: the plain plan is the same), judged by the back-to-back kernel's limits."""
    name = "mode%d_b2b" % mode
    res = es.run_b2b_child(mode)
    for H, W in es.SIZES:
        r = res["%dx%d" % (H, W)]
        N = r["N"]
        for n_str, kinds in r["kinds"].items():
            assert ex.S_CONV_B2B in kinds, "no back-to-back unit at %dx%d N=%s" % (H, W, n_str)
            p, msg = es.make_plan(mode, int(n_str), H, W)
            assert p is not None, msg
            plain = 0                                       # index of the fused plan's step in the plan made here
            for k in kinds:
                if k == ex.S_CONV_B2B:
                    for half in (plain, plain + 1):
                        info = p.info(half)
                        assert info["kind"] == ex.S_CONV
                        bad = ex.violations(info, "b2b")
                        assert not bad, "N=%s %dx%d step %d outside the back-to-back kernel's range: %s" % (n_str, H, W, half, bad)
                    plain += 2
                else:
                    assert p.info(plain)["kind"] == k
                    plain += 1
            assert plain == p.num_steps
            p.close()
        assert r["refusal"] and es.is_extent_refusal(r["refusal"]), "N + 1 = %d accepted" % (N + 1)
        assert N == golden["inference"]["%dx%d" % (H, W)][name], "the boundary moved: run tools/conv_extents.py"


@pytest.mark.parametrize("H,W", es.TRAIN_SIZES, ids=lambda v: str(v))
def test_boundary_batch_of_a_training_plan(golden, H, W):
    N = es.bisect_boundary(lambda n: es.accepts_training(n, H, W)[0])
    print("training %dx%d: largest accepted batch %d" % (H, W, N))
    assert N == golden["training"]["%dx%d" % (H, W)], "the boundary moved: run tools/conv_extents.py"
    ok, msg = es.accepts_training(N + 1, H, W)
    assert not ok
    if N < es.N_MAX:
        assert es.is_extent_refusal(msg), msg
    # The layers of the training plan are the inference plan's convolutions (the merged shortcut | conv1 launch of the inference plan is the
    # two layers side by side: Cout = depth + dbn bounds both; the stem is tried with its 13 channels and padded to 16).  wgrad_launch_g
    # (conv_bwd.hip:506) requires M * Cout < 2^31 and (N * (H + 2 pad) + 1) * (W + 2 pad) * Cin < 2^31 per tower, at launch time.
    n_inf = min(N, golden["inference"].get("%dx%d" % (H, W), {}).get("mode0", N))
    geo, _ = es.make_plan(0, n_inf, H, W)
    layers = 0
    for step in range(geo.num_steps):
        i = geo.info(step)
        if i["kind"] != ex.S_CONV:
            continue
        for cin in {i["cin"], -(-i["cin"] // 16) * 16}:
            assert ex.wgrad_requirement_holds(N, i["h"], i["w"], cin, i["cout"], i["kh"], i["stride"], i["pad"]), (N, i)
            # ... and the guard's own form of it, so the statement does not lean on the merged layer being an upper bound
            assert N * i["ho"] * i["wo"] * i["cout"] < 2 * LIMIT and N * i["h"] * i["w"] * cin < 2 * LIMIT
        layers += 1
    assert layers >= 49                                     # the stem + 16 units of 3 (the 4 projection units' shortcut rides with conv1)
    geo.close()


# ---- the operator entries: all pointers null, so the only thing that can happen is a refusal -------------------------------------------------
def _err():
    return rc._lib().stabnet_last_error().decode()


def _packed(x_ld, N=1, H=64, W=64, Cin=64, Cout=64, k=1, stride=1, pad=0, res_H=0, res_W=0, res_stride=1):
    L = rc._lib()
    return L.stabnet_conv2d_fwd_packed_ld(None, x_ld, None, None, None, None, None, None, res_H, res_W, res_stride, None, None, None, N, H, W, Cin,
                                          Cout, k, k, stride, pad, 0, 0, None, 0, None)


def _largest_ld(pixels):
    ld = (LIMIT - 1) // pixels // 4 * 4
    assert pixels * ld < LIMIT <= pixels * (ld + 4)
    return ld


@pytest.mark.parametrize("N,H,W,k,stride,pad", [(1, 64, 64, 1, 1, 0), (2, 40, 40, 3, 1, 1), (2, 41, 41, 3, 2, 1)])
def test_packed_entry_counts_x_ld(N, H, W, k, stride, pad):
    ld = _largest_ld(N * (H + 2 * pad) * (W + 2 * pad))
    assert _packed(ld + 4, N, H, W, 64, 64, k, stride, pad) != 0
    assert "input spans" in _err() and "2^30" in _err(), _err()
    assert _packed(ld, N, H, W, 64, 64, k, stride, pad) != 0
    assert "null pointer" in _err(), _err()                # inside the range: the shape check passed, the (null) pointers are looked at next


def _unit_pair(res_ld, N=1, H=9, W=11, K1=64, N1=256, N2=64):
    L = rc._lib()
    return L.stabnet_conv_unit_pair_fwd(None, None, None, None, None, res_ld, None, None, None, None, None, None, None, None, N, H, W, K1, N1, N2, 0, None)


@pytest.mark.parametrize("N", [1, 2])
def test_unit_pair_entry_counts_res_ld(N):
    ld = _largest_ld(N * 99)
    assert _unit_pair(ld + 4, N) != 0
    assert "residual spans" in _err() and "2^30" in _err(), _err()
    assert _unit_pair(ld, N) != 0
    assert "null pointer" in _err(), _err()


def _b2b(x_ld, res_ld, N=1, H=9, W=11, Cc=64, Cout=256, stride=1, res_stride=1):
    L = rc._lib()
    return L.stabnet_conv3x3_conv1x1_fwd(None, x_ld, None, None, None, None, None, None, H * res_stride if stride == 1 else H, W * res_stride if stride == 1 else W,
                                         res_stride, res_ld, None, None, None, N, H, W, Cc, Cout, stride, 0, None)


@pytest.mark.parametrize("N,res_stride", [(1, 1), (2, 1), (1, 2)])
def test_back_to_back_entry_counts_res_ld_and_x_ld(N, res_stride):
    ld = _largest_ld(N * 9 * res_stride * 11 * res_stride)
    assert _b2b(0, ld + 4, N, res_stride=res_stride) != 0
    assert "residual spans" in _err() and "2^30" in _err(), _err()
    assert _b2b(0, ld, N, res_stride=res_stride) != 0
    assert "null pointer" in _err(), _err()
    xld = _largest_ld(N * 11 * 13)
    assert _b2b(xld + 4, 0, N) != 0
    assert "input spans" in _err(), _err()
    assert _b2b(xld, 0, N) != 0
    assert "null pointer" in _err(), _err()


def test_a_strided_residual_is_counted_by_its_own_frame():
    """[N][res_H][res_W][Cout] read at (2 oy, 2 ox) is four times the output: the shapes of conv_extents_child.py's Dres cases"""
    assert 2 * 1024 * 2047 * 256 < LIMIT == 2 * 1024 * 2048 * 256
    assert _packed(0, 2, 512, 1024, 32, 256, res_H=1024, res_W=2048, res_stride=2) != 0
    assert "residual spans" in _err() and "2^30" in _err(), _err()
    assert _packed(0, 2, 512, 1024, 32, 256, res_H=1024, res_W=2047, res_stride=2) != 0
    assert "null pointer" in _err(), _err()


def test_dense_tensors_keep_their_bound():
    assert _packed(0, 1, 1 << 13, 1 << 13, 16, 16) != 0 and "2^30" in _err(), _err()                  # exactly 2^30 input floats
    assert _packed(0, 1, 1 << 13, (1 << 13) - 1, 16, 16) != 0 and "null pointer" in _err(), _err()
    assert _packed(0, 1, 4, 4, 1 << 15, 1 << 15) != 0 and "2^30" in _err(), _err()                      # exactly 2^30 weights
    assert _packed(0, 1, 4, 4, 1 << 15, (1 << 15) - 16) != 0 and "null pointer" in _err(), _err()


# ---- the Python mirror: the refusal arrives as StabnetError before anything is allocated on a device ------------------------------------
def test_regressor_and_stream_refuse_before_any_allocation(monkeypatch):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd.deploy import StabNetStream
    from stabnet_amd.regressor import Regressor

    def no_alloc(*a, **k):
        raise AssertionError("a tensor was allocated before the plan was refused")
    monkeypatch.setattr(torch, "empty", no_alloc)
    monkeypatch.setattr(torch, "zeros", no_alloc)
    monkeypatch.setattr(torch, "from_numpy", no_alloc)
    flat = np.zeros(4, np.float32)
    with pytest.raises(_lib.StabnetError, match="resnet_v2_50/.*floats"):
        Regressor(flat, 26, 1080, 1920, operand_mode=4, fuse_unit_pairs=True)
    with pytest.raises(_lib.StabnetError, match="resnet_v2_50/.*floats"):
        Regressor(flat, 456, 288, 512, keep_activations=True)
    with pytest.raises(_lib.StabnetError, match="resnet_v2_50/.*floats"):
        StabNetStream(flat, 720, 1280, streams=59, operand_mode=4)
