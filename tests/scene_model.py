"""NumPy model of the scene-cut statistic and rule (csrc/scene.hip, include/stabnet_hip.h "scene cuts"): the float32 quantisation, the
4 x 4 x 32 tile histograms, D, and the rule with its state over a sequence of frames.  The yardstick of every bit-for-bit comparison
in test_scene_*."""
import math

import numpy as np

TILES, BINS = 16, 32
HIST = TILES * BINS
WORDS = 2 + 2 * HIST                                        # {seen, since, prev[16][32], cur[16][32]}
U32_MAX = 0xFFFFFFFF


def bins(g):
    """float32 [...] -> int64 bin 0..31: t = floor((g + 0.5) * 255 + 0.5), one float32 rounding per operation; clamped to 0..255 by
    fmax / fmin (a NaN lands in 0); q >> 3."""
    g = np.asarray(g, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((g + np.float32(0.5)) * np.float32(255.0) + np.float32(0.5))
        t = np.fmin(np.fmax(t, np.float32(0.0)), np.float32(255.0))
    assert t.dtype == np.float32
    return t.astype(np.int64) >> 3


def tiles(H, W):
    """int64 [H,W]: tile = (4*y // H) * 4 + (4*x // W)."""
    ty = (4 * np.arange(H, dtype=np.int64)) // H
    tx = (4 * np.arange(W, dtype=np.int64)) // W
    return ty[:, None] * 4 + tx[None, :]


def hist(g):
    """float32 [N,H,W] -> uint32 [N,16,32]."""
    g = np.asarray(g, np.float32)
    N, H, W = g.shape
    idx = tiles(H, W)[None] * BINS + bins(g)
    out = np.zeros((N, HIST), np.uint32)
    for n in range(N):
        out[n] = np.bincount(idx[n].reshape(-1), minlength=HIST).astype(np.uint32)
    return out.reshape(N, TILES, BINS)


def distance(h_cur, h_prev):
    """uint32 [N,16,32] x 2 -> D uint32 [N] = sum |cur - prev|."""
    d = np.abs(h_cur.astype(np.int64) - h_prev.astype(np.int64)).reshape(len(h_cur), -1).sum(axis=1)
    assert d.max(initial=0) <= U32_MAX
    return d.astype(np.uint32)


def thr_num(threshold, H, W):
    return int(math.floor(float(threshold) * 2.0 * H * W))


class SceneModel:
    """The state of N streams, laid out as the device keeps it: state uint32 [N,1026]; after update() cur is zero again and prev is
    the histogram of the frame that was given."""

    def __init__(self, N, H, W, threshold=0.35, min_gap=8):
        self.N, self.H, self.W = N, H, W
        self.thr_num, self.min_gap = thr_num(threshold, H, W), int(min_gap)
        self.state = np.zeros((N, WORDS), np.uint32)

    def reset(self):
        self.state[:] = 0

    def update(self, g):
        """g float32 [N,H,W] -> (flag int32 [N], D uint32 [N], hist uint32 [N,16,32])."""
        h = hist(np.asarray(g, np.float32).reshape(self.N, self.H, self.W))
        prev = self.state[:, 2:2 + HIST].reshape(self.N, TILES, BINS)
        D = distance(h, prev)
        flag = np.zeros(self.N, np.int32)
        for n in range(self.N):
            seen, since = int(self.state[n, 0]), int(self.state[n, 1])
            if seen == 0:
                D[n] = 0
            else:
                flag[n] = int(since >= self.min_gap and int(D[n]) > self.thr_num)
            self.state[n, 1] = 0 if flag[n] else min(since + 1, U32_MAX)
            self.state[n, 0] = min(seen + 1, U32_MAX)
        self.state[:, 2:2 + HIST] = h.reshape(self.N, HIST)
        self.state[:, 2 + HIST:] = 0
        return flag, D, h


def run(frames, threshold=0.35, min_gap=8):
    """frames float32 [T,H,W], one stream -> (flags int32 [T], D uint32 [T], d float64 [T] = D / (2*H*W))."""
    frames = np.asarray(frames, np.float32)
    T, H, W = frames.shape
    m = SceneModel(1, H, W, threshold, min_gap)
    flags, Ds = np.zeros(T, np.int32), np.zeros(T, np.uint32)
    for t in range(T):
        f, D, _ = m.update(frames[t:t + 1])
        flags[t], Ds[t] = f[0], D[0]
    return flags, Ds, Ds.astype(np.float64) / (2.0 * H * W)


def cut_clip(H, W, Ta, Tb):
    """The clips of the tests: A = make_clip(seed 1) followed by B = 0.4 * make_clip(seed 2) - 0.25.  -> (A, B) float32."""
    from stabnet_amd import synthetic
    A = synthetic.make_clip(H, W, Ta, seed=1, margin=32)
    B = (np.float32(0.4) * synthetic.make_clip(H, W, Tb, seed=2, margin=32) - np.float32(0.25)).astype(np.float32)
    return A.astype(np.float32), B


def to_u8(frames):
    """Train-normalised float32 -> uint8 grey, (v + 0.5) * 255 rounded: the clips the driver tests write to disk."""
    return np.clip(np.rint((np.asarray(frames, np.float64) + 0.5) * 255.0), 0, 255).astype(np.uint8)


def multi_stream_clip(N, H, W, T=6):
    """float32 [T,N,H,W]: stream n shows scene A and, from frame 2 + n on, scene B, so that the streams' flags differ."""
    A, B = cut_clip(H, W, T, T)
    out = np.empty((T, N, H, W), np.float32)
    for n in range(N):
        c = 2 + n
        out[:c, n], out[c:, n] = A[:c], B[:T - c]
    return out
