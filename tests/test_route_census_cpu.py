"""CPU: the census of conv routes (tests/_route_census.py) against the committed tests/golden/route_census.json, both ways, and the
properties every conv step of the sweep must have.  A routing change -- a threshold of conv_route(), a tuning-table row, the grid
rule, the plan -- that adds a signature, drops one or moves an exemplar fails here until `python tools/route_census.py` rewrites the
file; test_route_census_gpu.py then runs the new exemplars.  Plans are host objects: no GPU."""
import ctypes as C

import pytest

import _route_census as rc


@pytest.fixture(scope="module")
def census():
    return rc.census()                 # also runs check_invariants() over every conv step of the sweep


def _by_signature(doc):
    out = {}
    for e in doc["signatures"]:
        key = (e["kernel"],) + tuple(e["signature"][n] for n in doc["signature_fields"] if n != "kind")
        assert key not in out, "signature listed twice: %s" % (key,)
        out[key] = e
    return out


def test_census_equals_the_committed_file(census):
    gold = rc.load_golden()
    assert gold["sweep"] == census["sweep"], "the sweep changed: run tools/route_census.py"
    assert gold["signature_fields"] == census["signature_fields"]
    got, want = _by_signature(census), _by_signature(gold)
    new = sorted(set(got) - set(want))
    gone = sorted(set(want) - set(got))
    assert not new, "%d conv signatures the committed census does not know (no test runs them), e.g. %s at %s" % (
        len(new), new[0], got[new[0]]["exemplar"])
    assert not gone, "%d signatures of the committed census no longer occur, e.g. %s" % (len(gone), gone[0])
    moved = [(k, want[k]["exemplar"], got[k]["exemplar"]) for k in sorted(want) if want[k]["exemplar"] != got[k]["exemplar"]]
    assert not moved, "%d exemplars moved, e.g. %s" % (len(moved), moved[0])
    counts = [(k, want[k]["launches"], got[k]["launches"]) for k in sorted(want) if want[k]["launches"] != got[k]["launches"]]
    assert not counts, "%d launch counts changed, e.g. %s" % (len(counts), counts[0])
    assert (gold["plans"], gold["conv_launches"]) == (census["plans"], census["conv_launches"])


def test_sweep_definition(census):
    sw = census["sweep"]
    assert sw["modes"] == [0, 4] and sw["step"] in (8, 16) and sw["H"] == [32, 1088] and sw["W"] == [32, 1920]
    sizes = set(rc.sweep_sizes())
    for s in [(1, 45, 77), (1, 90, 130), (1, 270, 480), (1, 1079, 1919), (1, 1080, 1920), (1, 32, 32), (1, 1088, 1920), (8, 288, 512),
              (2, 32, 32), (4, 45, 77)]:
        assert s in sizes, s
    assert (2, 296, 512) not in sizes and (2, 288, 520) not in sizes
    assert census["plans"] == len(sizes) * len(sw["modes"])
    assert census["conv_launches"] == sum(e["launches"] for e in census["signatures"])


def test_every_kernel_family_of_the_plan_is_in_the_census(census):
    kernels = {e["kernel"] for e in census["signatures"]}
    for name in ("conv_igemm_f32_kernel<64, 64, 32, 32, 32, 0, 2, 0>", "conv_igemm_f32_kernel<64, 64, 32, 32, 32, 0, 1, 0>",
                 "conv_ring_f32_kernel<0, 0, 1, 0>", "conv_ring_f32_kernel<1, 0, 1, 0>", "conv_ring_f32_kernel<2, 0, 1, 0>",
                 "conv_ring_f32_kernel<1, 0, 3, 0>", "conv_ring_f32_kernel<0, 0, 2, 1>", "conv_ring_f32_kernel<0, 4, 1, 0>",
                 "conv_ring_f32_kernel<1, 4, 1, 0>", "conv_ring_f32_kernel<2, 4, 1, 0>", "conv_ring_f32_kernel<0, 4, 1, 1>",
                 "conv_ring_f32_kernel<0, 4, 2, 0>", "conv_ring_f32_kernel<1, 4, 2, 0>", "conv_ring_f32_kernel<0, 4, 2, 1>",
                 "conv_astat_f32_kernel<32>", "conv_patch_f32_kernel<8, 8, 1, 3>", "conv_patch_f32_kernel<8, 8, 2, 3>"):
        assert name in kernels, name
    assert any(e["signature"]["reduce"] for e in census["signatures"])
    # the launch conv.hip names as never tried on the A-stationary kernel's rule: 1080p, 8160 x 512 x 128 stays on the packed ring kernel
    p = rc.Plan(4, 1, 1080, 1920)
    hit = [i for i in (p.info(s) for s in range(p.num_steps)) if i["kind"] == rc.S_CONV and (i["m"], i["cout"], i["k"]) == (8160, 512, 128)]
    assert hit and all(rc.kind_name(i["prof_kind"]) == "conv_ring_f32_kernel<0, 4, 1, 0>" for i in hit)


def test_exemplars_recompute_to_their_signature_and_divide_exactly():
    gold = rc.load_golden()
    for e in gold["signatures"]:
        x = e["exemplar"]
        p = rc.Plan(x["mode"], x["N"], x["H"], x["W"])
        info = p.info(x["step"])
        p.close()
        assert info["kind"] == rc.S_CONV, x
        kernel, sig = rc.signature_of(info)
        assert (kernel, sig) == (e["kernel"], e["signature"]), (x, kernel, sig)
        rc.check_fastdiv(info)


def test_k_step_classes_separate_fill_ring_and_tail():
    assert [int(v) for v in rc.k_step_class(list(range(1, 13)))] == [1, 2, 3, 4, 5, 6, 7, 8, 6, 7, 8, 6]


def test_grid_scales_with_the_cu_count_given_not_with_a_device():
    p = rc.Plan(0, 1, 200, 344)
    a, b = p.info(1, cus=256), p.info(1, cus=32)
    assert a["tiles"] == b["tiles"] and a["wgs"] == min(a["tiles"], 3 * 256) and b["wgs"] == min(b["tiles"], 3 * 32)


def test_step_entries_refuse_what_they_cannot_do():
    from stabnet_amd import _lib
    L = _lib.lib()
    nf = L.stabnet_net_step_info_fields()
    info = (C.c_long * nf)()
    inf, trn = C.c_void_p(), C.c_void_p()
    assert L.stabnet_net_create(C.byref(inf), 1, 64, 96, 13, 50, 0) == 0
    assert L.stabnet_net_create(C.byref(trn), 1, 64, 96, 13, 50, 1) == 0
    try:
        n = L.stabnet_net_num_steps(inf)
        assert n > 50 and L.stabnet_net_num_steps(None) == -1
        assert L.stabnet_net_step_info(inf, 1, 256, info, nf) == 0 and info[0] == rc.S_CONV
        assert L.stabnet_net_step_info(inf, 0, 256, info, nf) == 0 and info[0] == 0 and not any(info[1:nf])
        assert L.stabnet_net_step_info(inf, n, 256, info, nf) == -1 and b"outside" in L.stabnet_last_error()
        assert L.stabnet_net_step_info(inf, -1, 256, info, nf) == -1
        assert L.stabnet_net_step_info(inf, 1, 0, info, nf) == -1
        assert L.stabnet_net_step_info(inf, 1, 256, info, nf - 1) == -1
        assert L.stabnet_net_step_info(inf, 1, 256, None, nf) == -1
        assert L.stabnet_net_step_info(trn, 1, 256, info, nf) == -1 and b"inference" in L.stabnet_last_error()
        # run_steps: nothing is launched (and no device is touched) for a training plan, a bad range, a small workspace
        fake = 4096
        big = L.stabnet_net_workspace_bytes(inf)
        assert L.stabnet_net_run_steps(trn, fake, fake, fake, fake, fake, 1 << 40, 1, 1, None) == -1 and b"inference" in L.stabnet_last_error()
        assert L.stabnet_net_run_steps(inf, fake, fake, fake, fake, fake, big, 2, 1, None) == -1
        assert L.stabnet_net_run_steps(inf, fake, fake, fake, fake, fake, big, -1, 1, None) == -1
        assert L.stabnet_net_run_steps(inf, fake, fake, fake, fake, fake, big, 1, n, None) == -1 and b"outside" in L.stabnet_last_error()
        assert L.stabnet_net_run_steps(inf, fake, fake, fake, fake, fake, big - 1, 1, 1, None) == -3
        assert L.stabnet_net_run_steps(inf, fake, fake, None, fake, fake, big, 0, 1, None) == -1 and b"x_tensor" in L.stabnet_last_error()
        assert L.stabnet_net_run_steps(inf, fake, fake, fake, None, fake, big, n - 1, n - 1, None) == -1 and b"theta" in L.stabnet_last_error()
        assert L.stabnet_net_run_steps(inf, None, fake, fake, fake, fake, big, 1, 1, None) == -1
    finally:
        L.stabnet_net_destroy(inf)
        L.stabnet_net_destroy(trn)
