"""Child of tests/test_conv_astat_gpu.py (not a test module): the conv switches are read once per process, so every arm of that
test is one run of this script under its own STABNET_CONV_* environment.  `python conv_astat_child.py <out.npz> <part> ...`:
  ops      every case of CASES through ops.conv2d_packed (splitk = 1) and ops.conv2d: got_<i>, f32_<i>, and the kernel the packed
           call runs (stabnet_conv2d_packed_kind, conv_route()'s own answer): kernel_<i>;
           -- every packed output a freshly poisoned caller-owned buffer (_poison.py);
  grid:U   GRID_CASE through ops.conv2d_packed (splitk = 1) with all, U and CUs / 8 usable CUs (stabnet_conv_reserve_cus, the
           reservation argument): grid_<usable>, grid_usable (the three counts), grid_kernel, cus;
  forward  one regressor forward at (1, 96, 160) in operand mode 4 under the Profiler: theta, names, launches;
  routes   the Profiler names of one forward at (1, 96, 160) and at (1, 360, 640): names_small, names_large;
  deploy   one deploy step at 360 x 640: theta, x_map, y_map, output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# N, H, W, Cin, Cout, bias, residual (0 none, 1 same, 2 strided), out BN, relu
CASES = [
    (1, 17, 23, 32, 64, False, 0, False, False),      # one K step, ragged M for both tile heights
    (1, 17, 23, 64, 320, True, 0, True, True),        # five N tiles, bias + out BN + ReLU
    (2, 9, 13, 128, 512, False, 1, False, False),     # batch 2, residual
    (1, 17, 23, 256, 96, True, 0, False, False),      # 8 K steps, ragged Cout, bias
    (1, 17, 23, 256, 1024, False, 1, True, False),    # several N groups, residual + out BN
    (1, 18, 32, 96, 256, False, 0, False, False),     # K = 96, three steps
    (1, 9, 13, 128, 256, True, 2, False, True),       # residual read with res_stride = 2
]
# the N-group sweep: 36 M tiles of 32 rows (the last of 30) and 12 column blocks (the last tile ragged), so that 2 x usable CUs / M tiles
# gives three, two (of 8 and 4 blocks) and one N group at 256, 37 and 32 usable CUs
GRID_CASE = (1, 25, 46, 128, 372, True, 1, False, True)


def case_data(i):
    """The float32 inputs of case i, -1: of GRID_CASE (shared with the test, which evaluates the oracle on them)."""
    N, H, W, Cin, Cout, bias, res, out_bn, relu = CASES[i] if i >= 0 else GRID_CASE
    rng = np.random.default_rng(100 + i)
    d = {"x": rng.standard_normal((N, H, W, Cin)).astype(np.float32),
         "w": (rng.standard_normal((1, 1, Cin, Cout)) * np.sqrt(2.0 / Cin)).astype(np.float32)}
    d["b"] = rng.standard_normal(Cout).astype(np.float32) if bias else None
    d["r"] = None
    if res == 1:
        d["r"] = rng.standard_normal((N, H, W, Cout)).astype(np.float32)
    elif res == 2:
        d["r"] = rng.standard_normal((N, 2 * H - 1, 2 * W, Cout)).astype(np.float32)
    d["osc"] = rng.uniform(0.5, 1.5, Cout).astype(np.float32) if out_bn else None
    d["osh"] = (rng.standard_normal(Cout) * 0.3).astype(np.float32) if out_bn else None
    return d


def forward_input(H, W, in_ch):
    return np.random.default_rng(11).uniform(-0.5, 0.5, (1, H, W, in_ch)).astype(np.float32)


def grid_sweep(res, dev, u_odd, case, d, k, pad):
    """case = (N, H, W, Cin, Cout, ...), d its data: the packed convolution at every usable CU count, each into freshly poisoned
    buffers; the reservation is put back whatever happens."""
    import _poison
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    N, H, W, Cin, Cout = case[:5]
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    args = (t(d["x"]), t(ops.pack_conv_weight(d["w"])), t(d["b"]), None, None, t(d.get("r")), 1, 1, pad, bool(case[-1]))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus // 8 < u_odd < cus
    ws = ops.conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, k, k, 1, pad, 1)
    prev = L.stabnet_conv_reserve_cus(0)
    try:
        for usable, reserved in ((cus, 0), (u_odd, cus - u_odd), (cus // 8, cus)):
            L.stabnet_conv_reserve_cus(reserved)
            res["grid_%d" % usable] = _poison.run(dev, ops.conv2d_packed, (N, H, W, Cout), ws, *args, out_scale=t(d["osc"]),
                                                  out_shift=t(d["osh"]), splitk=1, what="usable %d" % usable)
    finally:
        L.stabnet_conv_reserve_cus(prev)
    res["grid_usable"] = np.array([cus, u_odd, cus // 8])
    res["cus"] = np.int64(cus)
    kind = int(L.stabnet_conv2d_packed_kind(N, H, W, Cin, Cout, k, k, 1, pad, 0, 1))
    assert kind > 0, kind
    res["grid_kernel"] = np.array(L.stabnet_prof_kind_name(kind).decode())


def _ops(res, dev):
    import _poison
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    for i, case in enumerate(CASES):
        d = case_data(i)
        args = (t(d["x"]), t(ops.pack_conv_weight(d["w"])), t(d["b"]), None, None, t(d["r"]), 2 if case[6] == 2 else 1, 1, 0, case[8])
        N, H, W, Cin, Cout = case[:5]
        res["got_%d" % i] = _poison.run(dev, ops.conv2d_packed, (N, H, W, Cout), ops.conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, 1, 1, 1, 0, 1),
                                        *args, out_scale=t(d["osc"]), out_shift=t(d["osh"]), splitk=1, what="case %d" % i)
        res["f32_%d" % i] = ops.conv2d(*args, out_scale=t(d["osc"]), out_shift=t(d["osh"])).cpu().numpy()
        kind = int(L.stabnet_conv2d_packed_kind(N, H, W, Cin, Cout, 1, 1, 1, 0, 0, 1))
        assert kind > 0, kind
        res["kernel_%d" % i] = np.array(L.stabnet_prof_kind_name(kind).decode())


def _forward(dev, H, W, prof):
    """theta, Profiler names and stabnet_net_num_launches of one mode-4 forward at (1, H, W)."""
    from stabnet_amd import _lib, synthetic
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import Regressor
    L = _lib.lib()
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    reg = Regressor(P, 1, H, W, cfg, device=dev, operand_mode=4)
    h = reg.plan.handle
    fold = torch.empty(int(L.stabnet_net_fold_floats(h)), dtype=torch.float32, device=dev)
    ws_n = int(L.stabnet_net_workspace_bytes(h))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    _lib.call("stabnet_net_fold_bn", h, ptr(reg.params), ptr(fold), cfg.bn_eps, stream_ptr(dev), device=dev)
    xt = torch.from_numpy(forward_input(H, W, cfg.in_ch)).to(dev)
    theta = torch.empty((1, cfg.n_theta), dtype=torch.float32, device=dev)
    prof.reset()
    _lib.call("stabnet_backbone_fwd_infer", h, ptr(reg.params), ptr(fold), ptr(xt), ptr(theta), ptr(ws), ws_n, stream_ptr(dev),
              prof.handle, device=dev)
    torch.cuda.synchronize()
    return theta.cpu().numpy(), np.array([r[0] for r in prof.records(raw=True)]), np.int64(L.stabnet_net_num_launches(h))


def _deploy(res, dev):
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    H, W = 360, 640
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    clip = synthetic.make_clip(H, W, 2, seed=5, margin=32)
    s = StabNetStream(P, H, W, cfg, streams=1, device=dev, operand_mode=4)
    s.start(torch.from_numpy(clip[0:1]).to(dev))
    got = s.step(torch.from_numpy(clip[1:2]).to(dev))
    torch.cuda.synchronize()
    for k in ("theta", "x_map", "y_map", "output"):
        res["deploy_" + k] = got[k].cpu().numpy()


def main(out, parts):
    from stabnet_amd.deploy import Profiler
    dev = torch.device("cuda:0")
    res = {}
    prof = Profiler(max_records=4096, device=dev)
    if "ops" in parts:
        _ops(res, dev)
    for part in parts:
        if part.startswith("grid:"):
            grid_sweep(res, dev, int(part[5:]), GRID_CASE, case_data(-1), 1, 0)
    if "forward" in parts:
        res["theta"], res["names"], res["launches"] = _forward(dev, 96, 160, prof)
    if "routes" in parts:
        _, res["names_small"], _ = _forward(dev, 96, 160, prof)
        _, res["names_large"], _ = _forward(dev, 360, 640, prof)
    if "deploy" in parts:
        _deploy(res, dev)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
