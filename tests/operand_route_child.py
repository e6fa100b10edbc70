"""Child of tests/test_operand_routes_gpu.py (not a test module): the inference regressor in one conv operand mode with the plan
switches of the environment (read once per process), at both shapes of the route matrix and one deploy step; dumps to <out>.npz:
theta twice, the input, the Profiler names of one forward, stabnet_net_num_launches (before the first forward, after the last,
and -- first shape -- after a forward in another operand mode), the canary tails of `fold` and the workspace, and the deploy step's Profiler names next to stabnet_deploy_frame_launches."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 96, 160), (2, 72, 136)]
TAIL_BYTES = 64 * 1024
CANARY = 0x5CA1AB1E                                   # a finite float32 bit pattern no kernel writes by accident


def _guarded(nbytes, device):
    """A uint8 buffer of nbytes + TAIL_BYTES whose tail holds the canary pattern."""
    buf = torch.empty(nbytes + TAIL_BYTES, dtype=torch.uint8, device=device)
    buf[nbytes:].view(torch.int32).fill_(CANARY)
    return buf


def _tail_bad(buf, nbytes):
    return int((buf[nbytes:].view(torch.int32).cpu().numpy().view(np.uint32) != CANARY).sum())


def main(out, mode):
    from stabnet_amd import _lib, synthetic
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import Profiler, StabNetStream
    from stabnet_amd.regressor import Regressor
    L = _lib.lib()
    dev = torch.device("cuda:0")
    res = {}
    prof = Profiler(max_records=4096, device=dev)
    for si, (N, H, W) in enumerate(SHAPES):
        cfg = Config(height=H, width=W)
        P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
        rng = np.random.default_rng(11)
        x = rng.uniform(-0.5, 0.5, (N, H, W, cfg.in_ch)).astype(np.float32)
        reg = Regressor(P, N, H, W, cfg, device=dev, operand_mode=mode)
        h = reg.plan.handle
        # first shape: no conv has run in this process yet; second shape: after the first shape's forwards and deploy step
        launches_before = int(L.stabnet_net_num_launches(h))
        fold_n = int(L.stabnet_net_fold_floats(h)) * 4
        ws_n = int(L.stabnet_net_workspace_bytes(h))
        assert ws_n % 4 == 0
        fold = _guarded(fold_n, dev)
        ws = _guarded(ws_n, dev)
        fold[:fold_n].view(torch.float32).fill_(float("nan"))     # whatever fold_bn leaves unwritten is NaN
        _lib.call("stabnet_net_fold_bn", h, ptr(reg.params), ptr(fold), cfg.bn_eps, stream_ptr(dev), device=dev)
        xt = torch.from_numpy(x).to(dev)
        thetas = []
        for rep in range(3):                                     # twice plain, once under the Profiler
            ws[:ws_n].view(torch.float32).fill_(float("nan"))    # no region may be read before the forward writes it
            theta = torch.empty((N, cfg.n_theta), dtype=torch.float32, device=dev)
            if rep == 2:
                prof.reset()
            _lib.call("stabnet_backbone_fwd_infer", h, ptr(reg.params), ptr(fold), ptr(xt), ptr(theta), ptr(ws), ws_n,
                      stream_ptr(dev), prof.handle if rep == 2 else 0, device=dev)
            torch.cuda.synchronize()
            thetas.append(theta.cpu().numpy())
        names = [r[0] for r in prof.records(raw=True)]
        res["theta_%d" % si], res["theta2_%d" % si], res["theta3_%d" % si] = thetas
        res["x_%d" % si] = x
        res["names_%d" % si] = np.array(names)
        res["launches_before_%d" % si] = np.int64(launches_before)
        res["launches_%d" % si] = np.int64(L.stabnet_net_num_launches(h))
        res["fold_tail_bad_%d" % si] = np.int64(_tail_bad(fold, fold_n))
        res["ws_tail_bad_%d" % si] = np.int64(_tail_bad(ws, ws_n))
        if si == 0:                                              # one deploy step (stabnet_deploy_frame) at the first shape
            clip = synthetic.make_clip(H, W, 3, seed=5, margin=32)
            s = StabNetStream(P, H, W, cfg, streams=1, device=dev, operand_mode=mode)
            s.start(torch.from_numpy(clip[0:1]).to(dev))
            s.step(torch.from_numpy(clip[1:2]).to(dev))
            prof.reset()
            s.step(torch.from_numpy(clip[2:3]).to(dev), prof=prof)
            res["deploy_launches"] = np.int64(L.stabnet_deploy_frame_launches(s.reg.plan.handle, cfg.grid_h, cfg.grid_w))
            res["deploy_names"] = np.array([r[0] for r in prof.records(raw=True)])
            del s
            reg0 = reg
        del reg
    # the first plan's count once more, after a forward in another operand mode on this thread (the model must not follow it)
    N, H, W = SHAPES[0]
    cfg = Config(height=H, width=W)
    other = Regressor(synthetic.make_params(cfg, seed=0, theta_scale=0.3), N, H, W, cfg, device=dev, operand_mode=1 if mode != 1 else 0)
    other(torch.from_numpy(res["x_0"]).to(dev))
    torch.cuda.synchronize()
    res["launches_cross_0"] = np.int64(L.stabnet_net_num_launches(reg0.plan.handle))
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
