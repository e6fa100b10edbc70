"""stabnet_net_fuse_unit_pairs on the host: which plan steps it replaces, and that it touches nothing else.

Plans are host objects and stabnet_net_step_info() reads no device."""
import numpy as np
import pytest

import _route_census as RC

S_CONV, S_CONV_PAIR = 1, 6
# frame -> fused pairs of the mode-4 plan: block 1 (M = H/4 * W/4, two identity units) and block 2 (M = H/8 * W/8, three) where M >= 12288
SIZES = [((64, 96), 0), ((360, 640), 2), ((720, 1280), 5)]


def _fuse(plan, on=1):
    L = RC._lib()
    assert L.stabnet_net_fuse_unit_pairs(plan.h, on) == 0
    plan.num_steps = L.stabnet_net_num_steps(plan.h)


def _eligible(info):
    """Indices i of the plain plan whose steps (i, i + 1) are a [conv3, conv1] pair the issue's rule takes."""
    f = lambda r, name: int(r[RC.col(name)])                                    # noqa: E731
    out = []
    for i in range(len(info) - 1):
        a, b = info[i], info[i + 1]
        if f(a, "kind") != S_CONV or f(b, "kind") != S_CONV:
            continue
        one = all(f(r, "kh") == 1 and f(r, "kw") == 1 and f(r, "stride") == 1 and f(r, "pad") == 0 and f(r, "splitk") == 1 for r in (a, b))
        if (one and f(a, "out_bn_off") < 0 and f(a, "res_off") >= 0 and f(a, "res_stride") == 1 and f(a, "k") <= 256 and f(a, "prologue") == 0 and
                f(b, "in_off") == f(a, "out_off") and f(b, "prologue") == 1 and f(b, "cout") <= 128 and f(a, "m") >= 12288):
            out.append(i)
    return out


@pytest.mark.parametrize("size,pairs", SIZES, ids=["%dx%d" % s for s, _ in SIZES])
def test_fusion_replaces_exactly_the_eligible_pairs(size, pairs):
    L = RC._lib()
    H, W = size
    plain, fused = RC.Plan(4, 1, H, W), RC.Plan(4, 1, H, W)
    info0 = plain.infos()
    n0 = L.stabnet_net_num_launches(plain.h)
    _fuse(fused)
    info1 = fused.infos()
    want = _eligible(info0)
    assert len(want) == pairs
    assert fused.num_steps == plain.num_steps - pairs
    assert L.stabnet_net_num_launches(fused.h) == n0 - pairs
    assert fused.workspace_bytes == L.stabnet_net_workspace_bytes(fused.h) == plain.workspace_bytes
    assert L.stabnet_net_fold_floats(fused.h) == L.stabnet_net_fold_floats(plain.h)
    # walk both plans: a fused step stands where an eligible pair stood, every other step's info is identical
    i = j = 0
    seen = 0
    keep = [RC.col(n) for n in RC.fields() if n not in ("kind", "prof_kind", "tiles", "wgs", "gx", "gy", "gz", "lds_bytes", "lds_limit")]
    while i < len(info0):
        if i in want:
            row = info1[j]
            assert row[RC.col("kind")] == S_CONV_PAIR
            assert np.array_equal(row[keep], info0[i][keep])                    # the conv3 half, offsets and all
            name = RC.kind_name(row[RC.col("prof_kind")])
            bm = 64 if info0[i + 1][RC.col("cout")] == 64 else 32
            assert name == "conv_unit_pair_f32_kernel<%d, %d>" % (1 if info0[i][RC.col("k")] == 64 else 0, bm)
            assert row[RC.col("gx")] == -(-int(row[RC.col("m")]) // bm) and row[RC.col("wgs")] == row[RC.col("gx")]
            assert 0 < row[RC.col("lds_bytes")] <= row[RC.col("lds_limit")]
            seen += 1
            i += 2
        else:
            assert np.array_equal(info1[j], info0[i]), (i, j)
            i += 1
        j += 1
    assert j == len(info1) and seen == pairs
    # asking again changes nothing; on = 0 and a later mode change both give the plan as built back
    _fuse(fused)
    assert np.array_equal(fused.infos(), info1)
    _fuse(fused, 0)
    assert np.array_equal(fused.infos(), info0) and L.stabnet_net_num_launches(fused.h) == n0
    _fuse(fused)
    assert L.stabnet_net_set_bf16_operands(fused.h, 4) == 0
    fused.num_steps = L.stabnet_net_num_steps(fused.h)
    assert np.array_equal(fused.infos(), info0)


@pytest.mark.parametrize("size", [s for s, _ in SIZES], ids=["%dx%d" % s for s, _ in SIZES])
def test_mode_0_plan_is_left_alone(size):
    L = RC._lib()
    H, W = size
    plain, asked = RC.Plan(0, 1, H, W), RC.Plan(0, 1, H, W)
    _fuse(asked)
    assert asked.num_steps == plain.num_steps
    assert np.array_equal(asked.infos(), plain.infos())
    assert L.stabnet_net_num_launches(asked.h) == L.stabnet_net_num_launches(plain.h)
