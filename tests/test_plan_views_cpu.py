"""The plan a caller sees is the plan the recorded commit made: tests/golden/plan_views.json holds, for six frame sizes, operand modes
0-4 and the plan variants default / unit pairs asked / B2B plan / both (tests/_plan_views.py), num_steps, num_launches,
deploy_frame_launches, workspace_bytes, fold_floats and every field of every step's stabnet_net_step_info.  It was recorded at the
commit named inside it, BEFORE the fusions became passes over the plain plan; everything is recomputed here and compared with `==`
(fold_floats of the B2B plans included: the fused units' convolutions still get no weight images).

Plans are host objects and stabnet_net_step_info() reads no device."""
import json

import numpy as np
import pytest

import _plan_views as PV
import _route_census as RC

S_CONV, S_CONV_B2B, S_CONV_PAIR = 1, 5, 6


@pytest.fixture(scope="module")
def golden():
    with open(PV.GOLDEN) as f:
        g = json.load(f)
    assert g["fields"] == list(RC.fields()) and g["cus"] == RC.CUS and len(g["commit"]) == 40
    return PV.unpack(g)


@pytest.fixture(scope="module")
def b2b_views():
    return PV.child_views()


def _compare(got, want):
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        for f in want[k]:
            if f != "info":
                assert got[k][f] == want[k][f], (k, f, got[k][f], want[k][f])
        a, b = np.array(got[k]["info"], np.int64), np.array(want[k]["info"], np.int64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (k, [(int(i), RC.fields()[j], int(a[i, j]), int(b[i, j])) for i, j in bad[:8]])


def test_default_and_pair_plans_equal_the_record(golden):
    got = PV.views(False)
    assert len(got) == len(PV.SIZES) * 7
    _compare(got, {k: v for k, v in golden.items() if k.split("/")[-1] in ("default", "pairs", "train")})


def test_b2b_plans_equal_the_record(golden, b2b_views):
    assert len(b2b_views) == len(PV.SIZES) * 6
    _compare(b2b_views, {k: v for k, v in golden.items() if k.split("/")[-1] in ("b2b", "b2b+pairs")})


def test_no_pair_from_a_conv3_that_b2b_took(golden, b2b_views):
    """Unit pairs are formed over what B2B left as S_CONV.  With STABNET_CONV_B2B_MIN_TILES=1 B2B takes conv2 -> conv3 of all seven
    units of block 1 and block 2, which holds every conv3 a pair starts at: asking for pairs then changes no step kind."""
    col = RC.col("kind")
    for size in PV.SIZES:
        plain = np.array(golden[PV.key(size, 4, "pairs")]["info"])[:, col]
        assert (size[1] < 360) == (S_CONV_PAIR not in plain)                   # the sizes at which pairs exist without B2B
        a = np.array(b2b_views[PV.key(size, 4, "b2b")]["info"])[:, col]
        b = np.array(b2b_views[PV.key(size, 4, "b2b+pairs")]["info"])[:, col]
        assert (a == S_CONV_B2B).sum() == 7                                    # block 1 and block 2: every conv3 a pair could start at
        assert np.array_equal(a, b) and S_CONV_PAIR not in b


def test_a_mode_change_forgets_the_pair_request():
    L = RC._lib()
    plan = RC.Plan(4, 1, 720, 1280)
    n0, info0 = plan.num_steps, plan.infos()
    assert L.stabnet_net_fuse_unit_pairs(plan.h, 1) == 0
    assert L.stabnet_net_num_steps(plan.h) == n0 - 5
    assert L.stabnet_net_set_bf16_operands(plan.h, 4) == 0                     # the same mode again: still a mode change
    assert L.stabnet_net_num_steps(plan.h) == n0
    assert np.array_equal(plan.infos(), info0)
    for mode in (0, 4):                                                        # and nothing is remembered across a round trip
        assert L.stabnet_net_set_bf16_operands(plan.h, mode) == 0
        assert L.stabnet_net_num_steps(plan.h) == n0
