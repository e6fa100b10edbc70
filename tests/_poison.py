"""Caller-owned, poisoned outputs for the convolution operators (ops.conv2d, conv2d_packed, conv3x3_conv1x1, conv2d_dgrad,
conv2d_dgrad_split take them as out= / workspace=): the guard-band idea of test_operand_routes_gpu.py (e) at operator level.

The operators allocate `y` with torch.empty; a test that copies it to the host hands the block back to the caching allocator and the
next identical call gets it again -- still holding the previous call's correct values.  A tile that a kernel never writes is then
invisible to every `got == got_b` or grid-A-versus-grid-B comparison.  Here `y` and the workspace each sit in a buffer of their own
that is NaN all over, with a 64 KiB tail behind them that holds a canary bit pattern: after the call every element of `y` must be
finite and both tails untouched.  (A split-K slab that is never written is NaN in the workspace; behind a ReLU epilogue the reduce
launch turns it into 0, which the finite check cannot see: the oracle bars and the bitwise comparisons of the callers do.)"""
import numpy as np
import torch

TAIL_BYTES = 64 * 1024
CANARY = 0x5CA1AB1E                                   # a finite float32 bit pattern no kernel writes by accident


class Poisoned:
    """out= (float32, `shape`) and workspace= (uint8, `ws_bytes`) for ONE operator call."""

    def __init__(self, device, shape, ws_bytes=0):
        self.shape = tuple(int(v) for v in shape)
        self.n = int(np.prod(self.shape))
        self.ws_words = (int(ws_bytes) + 3) // 4
        tail = TAIL_BYTES // 4
        self._y = torch.full((self.n + tail,), float("nan"), dtype=torch.float32, device=device)
        self._y[self.n:].view(torch.int32).fill_(CANARY)
        self._ws = torch.full((max(self.ws_words, 1) + tail,), float("nan"), dtype=torch.float32, device=device)
        self._ws[max(self.ws_words, 1):].view(torch.int32).fill_(CANARY)
        self.out = self._y[:self.n].view(self.shape)
        # (a call without scratch still gets a pointer: one NaN word in front of the tail)
        self.workspace = self._ws[:max(self.ws_words, 1)].view(torch.uint8)

    def result(self, what="y"):
        """y as numpy, after the checks: every element written (finite), both canary tails intact."""
        torch.cuda.synchronize()
        y = self._y.cpu().numpy()
        ws_tail = self._ws[max(self.ws_words, 1):].cpu().numpy()
        got = y[:self.n].reshape(self.shape).copy()
        unwritten = int(np.isnan(got).sum())
        assert unwritten == 0, "%s: %d of %d elements still NaN (rows %s ...): a tile was never written" % (
            what, unwritten, self.n, np.unique(np.argwhere(np.isnan(got.reshape(-1, self.shape[-1])))[:, 0])[:8])
        assert np.isfinite(got).all(), what + ": non-finite values"
        assert (y[self.n:].view(np.uint32) == CANARY).all(), what + ": write behind y"
        assert (ws_tail.view(np.uint32) == CANARY).all(), what + ": write behind the workspace"
        return got


def run(device, op, shape, ws_bytes, *args, what="y", **kw):
    """op(*args, out=, workspace=, **kw) into freshly poisoned buffers -> y (numpy), checked.  ws_bytes None: the operator takes no
    workspace argument."""
    buf = Poisoned(device, shape, ws_bytes or 0)
    if ws_bytes is None:
        ret = op(*args, out=buf.out, **kw)
    else:
        ret = op(*args, out=buf.out, workspace=buf.workspace, **kw)
    y = ret[0] if isinstance(ret, tuple) else ret
    assert y.data_ptr() == buf.out.data_ptr(), "the operator did not write the caller's tensor"
    return buf.result(what)


def conv_out_shape(x_shape, w_shape, stride=1, pad=0):
    N, H, W, _ = x_shape
    Cout, KH, KW, _ = w_shape
    return (N, (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1, Cout)
