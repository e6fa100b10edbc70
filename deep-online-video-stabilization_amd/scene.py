"""Scene cuts of the online loop (csrc/scene.hip): a 4 x 4 x 32 integer tile histogram of the incoming grey frame compared with the
previous frame's on the device, a flag in device memory.  deploy.StabNetStream.enable_scene_cut puts the two launches and the
predicated ring reseed (stabnet_ring_reseed_if) in front of every frame; nothing is read back."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import StabnetError
from ._tensor import dev_f32, ptr, stream_ptr

STATE_WORDS = 1026          # {seen, since, prev[16][32], cur[16][32]} (stabnet_scene_state_words)


def check_params(threshold, min_gap):
    """-> (threshold, min_gap); StabnetError unless 0 < threshold <= 1 (a NaN fails both comparisons) and min_gap is an integer >= 0."""
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise StabnetError("scene cut: threshold must be a number in (0, 1], got %r" % (threshold,))
    if not 0.0 < threshold <= 1.0:
        raise StabnetError("scene cut: threshold must be in (0, 1], got %r" % (threshold,))
    if isinstance(min_gap, bool) or not isinstance(min_gap, int) or min_gap < 0 or min_gap > 0x7fffffff:
        raise StabnetError("scene cut: min_gap must be an integer >= 0, got %r" % (min_gap,))
    return threshold, min_gap


class SceneCut:
    """The detector's state for `streams` streams of H x W frames.  update(grey) = stabnet_scene_update on the current torch stream:
    afterwards flag (int32 [S], 1 where the frame starts a new scene) and dist (uint32 [S], D = sum |hist - hist_prev|; the distance
    is D / (2*H*W)) hold the frame's values, on the device.  flag and dist are the two halves of one buffer (`out`, int32 [2*S])."""

    def __init__(self, streams: int, H: int, W: int, threshold: float = 0.35, min_gap: int = 8, device="cuda:0"):
        self.threshold, self.min_gap = check_params(threshold, min_gap)
        if int(streams) < 1 or not (4 <= int(H) <= 32767 and 4 <= int(W) <= 32767):
            raise StabnetError("scene cut: %d stream(s) of %dx%d: needs one stream or more and sides in 4..32767" % (streams, H, W))
        self.S, self.H, self.W = int(streams), int(H), int(W)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise StabnetError("scene cut: the detector runs on the GPU (there is no CPU fallback), got device %s" % (self.device,))
        self.thr_num = int(math.floor(self.threshold * 2.0 * self.H * self.W))
        assert _lib.lib().stabnet_scene_state_words() == STATE_WORDS
        self.state = torch.zeros((self.S, STATE_WORDS), dtype=torch.int32, device=self.device)
        self.out = torch.zeros(2 * self.S, dtype=torch.int32, device=self.device)
        self.flag = self.out[:self.S]
        self.dist = self.out[self.S:].view(torch.uint32)

    def reset(self):
        """A fresh stream: the next frame has nothing to differ from."""
        self.state.zero_()
        self.out.zero_()

    def enqueue(self, grey_ptr: int):
        """The two launches on the current stream, reading float32 [S,H,W] at grey_ptr (fixed arguments: capturable)."""
        _lib.call("stabnet_scene_update", grey_ptr, self.S, self.H, self.W, self.thr_num, self.min_gap, ptr(self.state), ptr(self.flag),
                  ptr(self.dist), stream_ptr(self.device), device=self.device)

    def update(self, grey: torch.Tensor):
        g = dev_f32(grey, "grey")
        if g.numel() != self.S * self.H * self.W or g.device != self.device:
            raise StabnetError("scene cut: expected %d x %d x %d values on %s, got %s on %s"
                               % (self.S, self.H, self.W, self.device, list(g.shape), g.device))
        self.enqueue(ptr(g))
        return self.flag

    def distance(self):
        """d = D / (2*H*W) per stream as a host list (synchronises)."""
        return [int(v) / (2.0 * self.H * self.W) for v in self.dist.cpu().numpy()]
