"""GPU: every structurally distinct conv launch of the inference plan (tests/golden/route_census.json, one exemplar per signature)
runs ALONE, as the plan binds it (stabnet_net_run_steps), on random inputs into a NaN-poisoned workspace, against a float64
evaluation of that one step (tests/_route_census.py reference_step: prologue, convolution, bias, residual read with its stride and
res_ld, output BN, floor or ReLU; float32 parameters and inputs; the stem from the OHWI weights, not the row-run copy).

Per exemplar:
  (a) error against float64 <= 2e-5 of the output's largest magnitude, 4e-5 with an output BN (the bars of test_conv_gpu.py);
  (b) mode-4 exemplars: the same step of a mode-0 plan of the same size on the same inputs differs by <= 4e-6 of that magnitude
      (the bar of test_conv_packed_gpu.py);
  (c) no NaN in the output;
  (d) every workspace word outside the output range and the reported scratch range keeps its poison or its input bits;
  (e) the launch's own route (stabnet_conv_last_launch_kind) is the kernel of the signature;
  (f) a second run gives the same bits.
out_floor, res_ld != Cout and the row-run stem reading the fold buffer are reachable through a plan only; the whole-network tests
see them through theta, behind the global pool."""
import ctypes as C

import numpy as np
import pytest
import torch

import _route_census as rc

pytestmark = pytest.mark.gpu

GOLD = rc.load_golden()
BN_EPS = 1e-5
# (a): error against float64 as a fraction of the output's largest magnitude, without / with an output BN (or the merged launch's
# vectors); the same for every family and operand mode.  test_conv_extents_gpu.py holds its launches to these too.
BAR_PLAIN, BAR_OUT_BN = 2e-5, 4e-5


@pytest.fixture(scope="module")
def world(cuda):
    """The parameters every plan of the sweep shares (the layout does not depend on the frame size), on the host and on the GPU."""
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import NetPlan
    cfg = Config(height=64, width=96)
    assert (cfg.in_ch, cfg.n_theta, cfg.bn_eps) == (rc.IN_CH, rc.N_THETA, BN_EPS)
    flat = NetPlan(1, 64, 96, cfg).pack(synthetic.make_params(cfg, seed=0, theta_scale=0.3))
    return {"params": flat, "params_dev": torch.from_numpy(flat).to(cuda), "fold": {}}


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _fold(world, plan, cuda):
    """stabnet_net_fold_bn of this plan (the fold kernels have bit-exact tests of their own) -> (fold on the GPU, scales, shifts as
    numpy).  The fold buffer's layout depends on nothing but the network: one per process."""
    from stabnet_amd import _lib
    L = _lib.lib()
    n = L.stabnet_net_fold_floats(plan.h)
    assert L.stabnet_net_param_floats(plan.h) == len(world["params"])
    if n not in world["fold"]:
        fold = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda)
        _lib.call("stabnet_net_fold_bn", plan.h, world["params_dev"].data_ptr(), fold.data_ptr(), BN_EPS, _stream(cuda), device=cuda)
        G = L.stabnet_net_bn_channels(plan.h)
        bn = fold[:2 * G].cpu().numpy()
        assert np.isfinite(bn).all()
        world["fold"][n] = (fold, bn[:G], bn[G:])
    return world["fold"][n]


def _run(plan, world, fold, ws, first, last, cuda, x=None):
    from stabnet_amd import _lib
    _lib.call("stabnet_net_run_steps", plan.h, world["params_dev"].data_ptr(), fold.data_ptr(), 0 if x is None else x.data_ptr(), 0,
              ws.data_ptr(), ws.numel() * 4, first, last, _stream(cuda), device=cuda)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _workspace(plan, cuda):
    assert plan.workspace_bytes % 4 == 0
    return torch.full((plan.workspace_bytes // 4,), float("nan"), dtype=torch.float32, device=cuda)


def test_the_census_was_made_for_this_chip(cuda):
    """The tile classes of the signatures hold for the CU count the census was made with."""
    assert torch.cuda.get_device_properties(cuda).multi_processor_count == GOLD["sweep"]["cus"] == rc.CUS


@pytest.mark.parametrize("entry", GOLD["signatures"], ids=rc.exemplar_id)
def test_exemplar_alone_against_float64(cuda, world, entry):
    from stabnet_amd import _lib
    L = _lib.lib()
    x = entry["exemplar"]
    mode, N, H, W, step = x["mode"], x["N"], x["H"], x["W"], x["step"]
    plan = rc.Plan(mode, N, H, W)
    info = plan.info(step)
    assert rc.signature_of(info) == (entry["kernel"], entry["signature"]), "the committed census is stale: run tools/route_census.py"
    fold, scale, shift = _fold(world, plan, cuda)
    gen = torch.Generator(device=cuda)
    gen.manual_seed(1000 + step)
    rnd = lambda n: torch.rand(n, generator=gen, device=cuda, dtype=torch.float32) * 2 - 1     # noqa: E731

    # ---- the step's inputs in a poisoned workspace
    ws = _workspace(plan, cuda)
    frame = None
    if info["rowrun"]:
        assert step == 1, "the row-run stem follows the pad step"
        frame = rnd(N * H * W * rc.IN_CH).view(N, H, W, rc.IN_CH)
        _run(plan, world, fold, ws, 0, 0, cuda, x=frame)                       # embeds the frame in its zero border (+ the slack row)
    else:
        ws[info["in_base"]:info["in_base"] + info["in_floats"]] = rnd(info["in_floats"])
    if info["res_off"] >= 0:
        ws[info["res_off"]:info["res_off"] + info["res_floats"]] = rnd(info["res_floats"])
    before = ws.clone()
    o0, o1 = info["out_off"], info["out_off"] + info["out_floats"]
    s0, s1 = info["scratch_off"], info["scratch_off"] + info["scratch_floats"]
    assert 0 <= o0 < o1 <= s0 <= s1 <= ws.numel()

    # ---- the one conv step (with its reduce launch)
    _run(plan, world, fold, ws, step, step, cuda)
    torch.cuda.synchronize()
    kind = L.stabnet_conv_last_launch_kind()
    assert rc.kind_name(kind) == entry["kernel"], "(e) the launch took %s" % rc.kind_name(kind)
    y_dev = ws[o0:o1].clone()
    got = y_dev.cpu().numpy().reshape(N, info["ho"], info["wo"], info["cout"])
    unwritten = int(np.isnan(got).sum())
    assert unwritten == 0, "(c) %d of %d outputs are NaN, rows %s ..." % (
        unwritten, got.size, np.unique(np.argwhere(np.isnan(got.reshape(-1, info["cout"])))[:, 0])[:8])
    for a, b, what in ((0, o0, "in front of the output"), (o1, s0, "between the output and the scratch"), (s1, ws.numel(), "behind the scratch")):
        assert _same_bits(ws[a:b], before[a:b]), "(d) the step wrote %s" % what

    # ---- float64 reference of the step
    merged = None
    if info["merged_off"] >= 0:
        merged = fold[info["merged_off"]:info["merged_off"] + 4 * info["cout"]].cpu().numpy().reshape(4, info["cout"])
    x_buf = None if info["rowrun"] else before[info["in_base"]:info["in_base"] + info["in_floats"]].cpu().numpy()
    res_buf = before[info["res_off"]:info["res_off"] + info["res_floats"]].cpu().numpy() if info["res_off"] >= 0 else None
    want = rc.reference_step(info, world["params"], scale, shift, merged, x_buf=x_buf, res_buf=res_buf,
                             frame=None if frame is None else frame.cpu().numpy())
    mag = np.abs(want).max()
    err = np.abs(got - want).max()
    bar = BAR_OUT_BN if (info["out_bn_off"] >= 0 or merged is not None) else BAR_PLAIN
    print("%s %s: err %.3g of %.3g (%.2g of the bar)" % (rc.exemplar_id(entry), entry["kernel"], err, mag, err / (bar * mag)))
    assert mag > 0 and err <= bar * mag, "(a) max err %g against float64, output magnitude %g, bar %g" % (err, mag, bar * mag)

    # ---- (f) the same bits again, from the same poisoned state
    ws.copy_(before)
    _run(plan, world, fold, ws, step, step, cuda)
    torch.cuda.synchronize()
    assert _same_bits(ws[o0:o1], y_dev), "(f) a second run gave other bits"

    # ---- (b) the same step of the mode-0 plan of this size, on the same inputs
    if mode == 4:
        plan0 = rc.Plan(0, N, H, W)
        info0 = plan0.info(step)
        same = ("n", "h", "w", "cin", "ho", "wo", "cout", "kh", "kw", "stride", "pad", "x_ld", "res_ld", "in_off", "in_base", "in_floats",
                "out_off", "res_off", "res_floats", "w_off", "bias_off", "pro_bn_off", "out_bn_off", "merged_off")
        assert [info0[k] for k in same] == [info[k] for k in same]
        assert info0["operand"] == 0
        fold0 = _fold(world, plan0, cuda)[0]
        ws0 = _workspace(plan0, cuda)
        for a, n in ((info["in_base"], info["in_floats"]), (info["res_off"], info["res_floats"])):
            if a >= 0:
                ws0[a:a + n] = before[a:a + n]
        _run(plan0, world, fold0, ws0, step, step, cuda)
        torch.cuda.synchronize()
        got0 = ws0[o0:o1].cpu().numpy().reshape(got.shape)
        assert np.isfinite(got0).all()
        d = np.abs(got - got0).max()
        assert d <= 4e-6 * mag, "(b) max difference to the exact-f32 plan's step %g (magnitude %g)" % (d, mag)
        assert np.abs(got0 - want).max() <= bar * mag
        plan0.close()
    plan.close()
