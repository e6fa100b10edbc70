"""Child of tests/test_unit_pair_gpu.py (not a test module): the conv switches are read once per process, so every arm of that test
is one run of this script under its own STABNET_CONV_* environment.  `python unit_pair_child.py <out.npz> <part> ...`:
  ops      every case of CASES as two launches (ops.conv2d_packed, splitk = 1: conv3 + bias + residual, then conv1 with the prologue)
           and as one (ops.conv_unit_pair), every output a freshly poisoned caller-owned buffer (_poison.py): ref3_<i>, ref1_<i>,
           got3_<i>, got1_<i>, and the kernels the three launches ran (stabnet_conv_last_launch_kind): kernels_<i>;
  forward  one regressor forward at (1, 96, 160) in operand mode 4, asked to fuse, on a NaN-filled workspace under the Profiler:
           theta, names, launches, the whole workspace (bits) and every activation tap;
  deploy   two deploy steps at 96 x 160 (StabNetStream asks for the fusion itself), the second under the Profiler: theta, maps,
           output, names, stabnet_deploy_frame_launches."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# N (images of 9 x 11 pixels: M = 99 has a ragged last tile for both tile heights, 198 spans two images), K1, N1, N2, channels of the
# residual buffer (> N1: read with a pixel stride), bias.  K1 = 64 is the f32 form, 128 the packed one; N2 = 64 the 64-row tile, 128 the
# 32-row tile; N1 = 256 / 512 are two / four 128-channel passes
CASES = [
    (1, 64, 256, 64, 256, True),
    (2, 64, 512, 128, 576, True),
    (1, 128, 512, 128, 640, True),
    (2, 128, 256, 64, 256, False),
    (1, 128, 256, 128, 320, False),
    (2, 64, 256, 64, 320, False),
    (2, 128, 512, 128, 512, True),
    (1, 64, 512, 64, 512, True),
]
H, W = 9, 11
TAPS = ["conv1", "pool1"] + ["block%d/unit_%d" % (b + 1, u + 1) for b, n in enumerate((3, 4, 6, 3)) for u in range(n)] + ["global_pool"]


def case_data(i):
    N, K1, N1, N2, Cr, bias = CASES[i]
    rng = np.random.default_rng(700 + i)
    return {
        "x": np.maximum(rng.standard_normal((N, H, W, K1)), 0).astype(np.float32),          # conv3 reads an activated tensor
        "w3": (rng.standard_normal((N1, 1, 1, K1)) * np.sqrt(2.0 / K1)).astype(np.float32),
        "b3": rng.standard_normal(N1).astype(np.float32) if bias else None,
        "r": rng.standard_normal((N, H, W, Cr)).astype(np.float32),
        "ps": rng.uniform(0.5, 1.5, N1).astype(np.float32), "pb": (rng.standard_normal(N1) * 0.3).astype(np.float32),
        "w1": (rng.standard_normal((N2, 1, 1, N1)) * np.sqrt(2.0 / N1)).astype(np.float32),
        "os": rng.uniform(0.5, 1.5, N2).astype(np.float32), "ob": (rng.standard_normal(N2) * 0.3).astype(np.float32),
    }


def forward_input(h, w, in_ch):
    return np.random.default_rng(11).uniform(-0.5, 0.5, (1, h, w, in_ch)).astype(np.float32)


def _ops(res, dev):
    import _poison
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    name = lambda: L.stabnet_prof_kind_name(int(L.stabnet_conv_last_launch_kind())).decode()
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    for i, (N, K1, N1, N2, Cr, _) in enumerate(CASES):
        d = {k: t(v) for k, v in case_data(i).items()}
        # one buffer, the shifts behind the scales: what the packed prologue kernel asks of its two vectors (conv.hip ring_pro_vectors_ok)
        pv = t(np.stack([case_data(i)["ps"], case_data(i)["pb"]]))
        d["ps"], d["pb"] = pv[0], pv[1]
        dense = d["r"][..., :N1].contiguous()                 # the two-launch operator takes a dense residual: the same values
        p3 = _poison.Poisoned(dev, (N, H, W, N1), ops.conv2d_packed_workspace_bytes(N, H, W, K1, N1, 1, 1, 1, 0, 1))
        ops.conv2d_packed(d["x"], d["w3"], d["b3"], None, None, dense, 1, 1, 0, False, splitk=1, out=p3.out, workspace=p3.workspace)
        k3 = name()
        res["ref3_%d" % i] = p3.result("case %d conv3" % i)
        p1 = _poison.Poisoned(dev, (N, H, W, N2), ops.conv2d_packed_workspace_bytes(N, H, W, N1, N2, 1, 1, 1, 0, 1))
        ops.conv2d_packed(p3.out, d["w1"], None, d["ps"], d["pb"], None, 1, 1, 0, True, out_scale=d["os"], out_shift=d["ob"], splitk=1,
                          out=p1.out, workspace=p1.workspace)
        k1 = name()
        res["ref1_%d" % i] = p1.result("case %d conv1" % i)
        q3, q1 = _poison.Poisoned(dev, (N, H, W, N1)), _poison.Poisoned(dev, (N, H, W, N2))
        ops.conv_unit_pair(d["x"], d["w3"], d["b3"], d["r"], d["ps"], d["pb"], d["w1"], d["os"], d["ob"], True, out3=q3.out, out=q1.out)
        res["kernels_%d" % i] = np.array([k3, k1, name()])
        res["got3_%d" % i] = q3.result("case %d fused conv3" % i)
        res["got1_%d" % i] = q1.result("case %d fused conv1" % i)


def _forward(res, dev, prof):
    from stabnet_amd import _lib, synthetic
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import Regressor
    import ctypes
    L = _lib.lib()
    h, w = 96, 160
    cfg = Config(height=h, width=w)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    reg = Regressor(P, 1, h, w, cfg, device=dev, operand_mode=4, fuse_unit_pairs=True)
    hd = reg.plan.handle
    ws_n = int(L.stabnet_net_workspace_bytes(hd))
    ws = torch.empty((ws_n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    ws.view(torch.float32).fill_(float("nan"))               # no region may be read before the forward writes it
    xt = torch.from_numpy(forward_input(h, w, cfg.in_ch)).to(dev)
    theta = torch.empty((1, cfg.n_theta), dtype=torch.float32, device=dev)
    prof.reset()
    _lib.call("stabnet_backbone_fwd_infer", hd, ptr(reg.params), ptr(reg.fold), ptr(xt), ptr(theta), ptr(ws), ws_n, stream_ptr(dev),
              prof.handle, device=dev)
    torch.cuda.synchronize()
    res["theta"] = theta.cpu().numpy()
    res["names"] = np.array([r[0] for r in prof.records(raw=True)])
    res["launches"] = np.int64(L.stabnet_net_num_launches(hd))
    res["steps"] = np.int64(L.stabnet_net_num_steps(hd))
    bits = ws.view(torch.int32).cpu().numpy()
    res["workspace"] = bits
    off, dims = ctypes.c_long(), (ctypes.c_int * 4)()
    for tap in TAPS:
        _lib.call("stabnet_net_activation_info", hd, tap.encode(), ctypes.byref(off), dims)
        res["tap_" + tap.replace("/", "_")] = bits[off.value:off.value + int(np.prod(list(dims)))].copy()


def _deploy(res, dev, prof):
    from stabnet_amd import _lib, synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    L = _lib.lib()
    h, w = 96, 160
    cfg = Config(height=h, width=w)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    clip = synthetic.make_clip(h, w, 3, seed=5, margin=32)
    s = StabNetStream(P, h, w, cfg, streams=1, device=dev, operand_mode=4)
    s.reg.workspace[:s.reg.workspace.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    s.start(torch.from_numpy(clip[0:1]).to(dev))
    s.step(torch.from_numpy(clip[1:2]).to(dev))
    prof.reset()
    got = s.step(torch.from_numpy(clip[2:3]).to(dev), prof=prof)
    torch.cuda.synchronize()
    for k in ("theta", "x_map", "y_map", "output"):
        res["deploy_" + k] = got[k].cpu().numpy()
    res["deploy_names"] = np.array([r[0] for r in prof.records(raw=True)])
    res["deploy_launches"] = np.int64(L.stabnet_deploy_frame_launches(s.reg.plan.handle, cfg.grid_h, cfg.grid_w))
    res["deploy_net_launches"] = np.int64(L.stabnet_net_num_launches(s.reg.plan.handle))


def main(out, parts):
    from stabnet_amd.deploy import Profiler
    dev = torch.device("cuda:0")
    res = {}
    prof = Profiler(max_records=4096, device=dev)
    if "ops" in parts:
        _ops(res, dev)
    if "forward" in parts:
        _forward(res, dev, prof)
    if "deploy" in parts:
        _deploy(res, dev, prof)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
