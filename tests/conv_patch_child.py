"""Child of tests/test_conv_patch_gpu.py (not a test module): the conv switches are read once per process, so every arm of that
test is one run of this script under its own STABNET_CONV_* environment.  `python conv_patch_child.py <out.npz> <part> ...`:
  ops      every case of CASES through the packed C ABI (stabnet_conv2d_fwd_packed_ld, splitk = 1: what ops.conv2d_packed calls, plus
           the input's pixel pitch) with guard bands -- x lies in a NaN-filled buffer (NaN in the columns beside it where x_ld > Cin,
           NaN in front and behind), y between canaries -- and through ops.conv2d on a dense copy: got_<i>, f32_<i>, guards_<i> (1:
           canaries intact), and the kernel the packed call runs (stabnet_conv2d_packed_kind, conv_route()'s own answer): kernel_<i>;
  ops2     the cases of KG2 (Cin = 64: an even number of K steps) with splitk = 2, the two equal K halves the ring kernel runs inside
           the workgroup: got2_<i>, f322_<i>, guards2_<i>, kernel2_<i>;
  grid:U   GRID_CASE through ops.conv2d_packed (splitk = 1, freshly poisoned caller-owned buffers: _poison.py) with all, U and CUs / 8
           usable CUs (stabnet_conv_reserve_cus, the reservation argument): grid_<usable>, grid_usable, grid_kernel, cus;
  twice    case REPLAY a second time, and once more as the replay of a captured graph: again, replay;
  routes   the Profiler names and stabnet_net_num_launches of one mode-4 forward at (1, 96, 160) and at (1, 360, 640);
  deploy   one deploy step at 360 x 640: theta, x_map, y_map, output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# N, H, W, Cin, Cout, columns of the input buffer beside x (x_ld - Cin; x starts a quarter of them in), bias, out BN, relu
CASES = [
    (1, 1, 1, 32, 32, 0, False, False, False),        # one pixel: every tap but the centre is halo; one step per tap; one column block
    (1, 3, 5, 64, 64, 0, True, False, False),         # smaller than a patch in both directions; two steps per tap; bias
    (1, 5, 7, 96, 72, 0, True, True, True),           # odd steps per tap; ragged last column block; bias + out BN + ReLU
    (1, 9, 17, 64, 160, 0, False, False, False),      # ragged in both directions, several patches; more column blocks than one group
    (1, 12, 40, 32, 64, 0, False, True, True),        # five patches a row, two patch rows; out BN + ReLU without bias
    (2, 9, 17, 96, 160, 0, True, False, False),       # batch 2: a patch never crosses into the next image
    (2, 5, 7, 64, 72, 64, False, False, False),       # batch 2, the input as a column slice of a wider buffer
    (1, 12, 40, 96, 32, 32, True, True, True),        # x_ld > Cin over several patches
    (1, 9, 17, 32, 72, 0, True, False, False),
]
# the N-group sweep: 6 x 6 patches (the last of 5 x 5 pixels) and 10 column blocks (the last tile ragged), so that 2 x usable CUs /
# patches gives the most (five / three), two (the second shorter) and one N group at 256, 37 and 32 usable CUs
GRID_CASE = (1, 45, 45, 32, 308, 0, True, False, True)
KG2 = [i for i, c in enumerate(CASES) if c[3] == 64]
REPLAY = 5
GUARD = 4096
CANARY = 0x7FC0BEEF                                        # a NaN pattern no kernel computes


def case_data(i):
    """The float32 inputs of case i, -1: of GRID_CASE (shared with the test, which evaluates the oracle on them)."""
    N, H, W, Cin, Cout, extra, bias, out_bn, relu = CASES[i] if i >= 0 else GRID_CASE
    rng = np.random.default_rng(300 + i)
    d = {"x": rng.standard_normal((N, H, W, Cin)).astype(np.float32),
         "w": (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)}
    d["b"] = rng.standard_normal(Cout).astype(np.float32) if bias else None
    d["osc"] = rng.uniform(0.5, 1.5, Cout).astype(np.float32) if out_bn else None
    d["osh"] = (rng.standard_normal(Cout) * 0.3).astype(np.float32) if out_bn else None
    return d


class _Call:
    """Case i's buffers on the device; launch() enqueues the packed convolution on the current stream and nothing else."""

    def __init__(self, i, dev, splitk=1):
        from stabnet_amd import _lib, ops
        self.L, self.dev = _lib.lib(), dev
        self.case, self.splitk = CASES[i], splitk
        N, H, W, Cin, Cout, extra = self.case[:6]
        d = case_data(i)
        t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
        self.ld, c0 = Cin + extra, (extra // 4) // 4 * 4
        xb = np.full((N, H, W, self.ld), np.nan, np.float32)
        xb[..., c0:c0 + Cin] = d["x"]
        self.xb = torch.full((xb.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.xb[GUARD:GUARD + xb.size] = t(xb.reshape(-1))
        self.xp = self.xb[GUARD + c0:].data_ptr()
        self.ny = N * H * W * Cout
        self.yb = torch.full((self.ny + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
        self.w = t(ops.pack_conv_weight(d["w"]))
        self.img = torch.empty(int(self.L.stabnet_conv_weight_image_floats(Cout, 3, 3, Cin)), dtype=torch.float32, device=dev)
        self.b, self.osc, self.osh = t(d["b"]), t(d["osc"]), t(d["osh"])
        self.ws_bytes = max(int(self.L.stabnet_conv2d_workspace_bytes(N, H, W, Cin, Cout, 3, 3, 1, 1)), splitk * self.ny * 4)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.dense = t(d["x"])
        from stabnet_amd._tensor import stream_ptr
        _lib.call("stabnet_conv_weight_split_image", self.w.data_ptr(), Cout, 3, 3, Cin, self.img.data_ptr(), stream_ptr(dev), device=dev)

    def launch(self):
        from stabnet_amd import _lib
        from stabnet_amd._tensor import ptr, stream_ptr
        N, H, W, Cin, Cout = self.case[:5]
        _lib.call("stabnet_conv2d_fwd_packed_ld", self.xp, self.ld, self.w.data_ptr(), self.img.data_ptr(), ptr(self.b), 0, 0, 0, 0, 0, 1,
                  ptr(self.osc), ptr(self.osh), self.yb[GUARD:].data_ptr(), N, H, W, Cin, Cout, 3, 3, 1, 1, int(self.case[8]), self.splitk,
                  self.ws.data_ptr(), self.ws_bytes, stream_ptr(self.dev), device=self.dev)

    def result(self):
        """(y, guards intact) of the last launch; y's buffer is filled with canaries again."""
        torch.cuda.synchronize()
        N, H, W, Cin, Cout = self.case[:5]
        yh = self.yb.cpu().numpy().view(np.uint32)
        ok = (yh[:GUARD] == CANARY).all() and (yh[GUARD + self.ny:] == CANARY).all()
        ok = ok and not (yh[GUARD:GUARD + self.ny] == CANARY).any()            # every element of y was written
        self.yb.fill_(CANARY)
        return yh[GUARD:GUARD + self.ny].view(np.float32).reshape(N, H, W, Cout).copy(), np.int64(ok)

    def f32(self):
        from stabnet_amd import ops
        return ops.conv2d(self.dense, self.w, self.b, None, None, None, 1, 1, 1, self.case[8], out_scale=self.osc, out_shift=self.osh).cpu().numpy()


def _kernel(L, case, splitk):
    N, H, W, Cin, Cout = case[:5]
    kind = int(L.stabnet_conv2d_packed_kind(N, H, W, Cin, Cout, 3, 3, 1, 1, 0, splitk))
    assert kind > 0, kind
    return np.array(L.stabnet_prof_kind_name(kind).decode())


def _ops(res, dev, cases, splitk, tag):
    for i in cases:
        c = _Call(i, dev, splitk)
        c.launch()
        res["got%s_%d" % (tag, i)], res["guards%s_%d" % (tag, i)] = c.result()
        res["f32%s_%d" % (tag, i)] = c.f32()
        res["kernel%s_%d" % (tag, i)] = _kernel(c.L, CASES[i], splitk)


def _twice(res, dev):
    c = _Call(REPLAY, dev)
    c.launch()
    res["first"], _ = c.result()
    c.launch()
    res["again"], _ = c.result()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.launch()
    c.result()                                             # (capture runs nothing; the buffer holds canaries again either way)
    g.replay()
    res["replay"], res["replay_guards"] = c.result()


def main(out, parts):
    from conv_astat_child import _deploy, _forward, grid_sweep
    from stabnet_amd.deploy import Profiler
    dev = torch.device("cuda:0")
    res = {}
    if "ops" in parts:
        _ops(res, dev, range(len(CASES)), 1, "")
    if "ops2" in parts:
        _ops(res, dev, KG2, 2, "2")
    if "twice" in parts:
        _twice(res, dev)
    for part in parts:
        if part.startswith("grid:"):
            grid_sweep(res, dev, int(part[5:]), GRID_CASE, case_data(-1), 3, 1)
    if "routes" in parts:
        prof = Profiler(max_records=4096, device=dev)
        _, res["names_small"], res["launches_small"] = _forward(dev, 96, 160, prof)
        _, res["names_large"], res["launches_large"] = _forward(dev, 360, 640, prof)
    if "deploy" in parts:
        _deploy(res, dev)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
