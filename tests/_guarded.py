"""Canary-banded device buffers and bit comparisons shared by the operator tests (test_train_layers_gpu.py,
test_infer_layers_gpu.py)."""
import numpy as np
import torch

GUARD = 4096                                               # canary words on each side of a buffer
CANARY = 0x5CA1AB1E


class Guarded:
    """n elements between two canary bands.  init: None = NaN (float) / 0xEE (bytes), "canary" = the canary word, or values."""

    def __init__(self, dev, n, init=None, dtype=torch.float32):
        self.n = int(n)
        self.words = self.n if dtype == torch.float32 else (self.n + 3) // 4
        self.buf = torch.full((self.words + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
        inner = self.buf[GUARD:GUARD + self.words]
        self.t = inner.view(dtype)[:self.n]
        if isinstance(init, str):
            assert init == "canary"
        elif init is None:
            self.t.fill_(float("nan") if dtype == torch.float32 else 0xEE)
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dev))

    def check(self, what):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.words:]
        assert bool((lo == CANARY).all()) and bool((hi == CANARY).all()), "write outside " + what

    def np(self):
        return self.t.cpu().numpy().copy()

    def untouched(self):
        return bool((self.buf == CANARY).all())


def _check_all(named):
    torch.cuda.synchronize()
    for what, b in named.items():
        if b is not None:
            b.check(what)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))
