"""Inputs for the full-frame tests (tests/mosaic_model.py, csrc/mosaic.hip).

border_clip: why the guard exists.  One smooth texture (tvl1_model.texture) seen through a smooth INTEGER pan, so the true motion
between two frames is an exact translation; around it a black border whose four widths jitter by up to +-18 px about 19 px, as the
border of a stabilised frame does.  black is 1 in the border, 0 on content.

compose_case: random inputs of one compose launch with every edge case the kernel tests need."""
import functools

import numpy as np

import tvl1_model as TM

F = np.float32
GH, GW, GT = 144, 256, 10            # the guard experiment's clip
BASE, JIT = 19, 18                   # border width 19 +- 18 px
MARGIN = 32


@functools.lru_cache(maxsize=None)
def border_clip(seed=7):
    """-> frames float32 [T,H,W] on the 0..255 scale, black float32 [T,H,W], pan int [T,2] (x, y): frame t shows the texture's pixel
    (x + pan_x[t], y + pan_y[t]) at (x, y)."""
    tex = (TM.texture(GH + 2 * MARGIN, GW + 2 * MARGIN, seed) * 255.0).astype(F)
    t = np.arange(GT)
    pan = np.stack([np.rint(10.0 * (1.0 - np.cos(np.pi * t / (GT - 1)))), np.rint(0.4 * t)], axis=1).astype(int)     # 0..20 px, 0..4 px
    rng = np.random.default_rng(seed + 1)
    # left, right, top, bottom: the difference of two uniform draws, so large jumps are rarer than small ones (with uniform draws
    # the tracker itself, unguarded or not, loses too many corners for a model on some pairs)
    widths = BASE + np.rint((rng.random((GT, 4)) - rng.random((GT, 4))) * JIT).astype(int)
    frames, black = np.zeros((GT, GH, GW), F), np.ones((GT, GH, GW), F)
    for k in range(GT):
        l, r, tp, bt = widths[k]
        view = tex[MARGIN + pan[k, 1]:MARGIN + pan[k, 1] + GH, MARGIN + pan[k, 0]:MARGIN + pan[k, 0] + GW]
        frames[k, tp:GH - bt, l:GW - r] = view[tp:GH - bt, l:GW - r]
        black[k, tp:GH - bt, l:GW - r] = 0
    for a in (frames, black, pan):
        a.setflags(write=False)
    return frames, black, pan


def planted_homography(pan, t):
    """Hm [9] float64 of frame t -> frame t - 1 in the normalised frame: a point of the scene at x in frame t lies at
    x + pan[t] - pan[t - 1] in frame t - 1."""
    dx, dy = pan[t] - pan[t - 1]
    return np.array([1, 0, 2.0 * dx / GW, 0, 1, 2.0 * dy / GH, 0, 0, 1], np.float64)


def corner_error_px(Hm, truth, H, W):
    """The largest distance in pixels between the images of the four image corners under Hm and under truth."""
    c = np.array([[-1, -1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], np.float64).T
    a, b = np.asarray(Hm, np.float64).reshape(3, 3) @ c, np.asarray(truth, np.float64).reshape(3, 3) @ c
    a, b = a[:2] / a[2], b[:2] / b[2]
    return float(np.hypot((a[0] - b[0]) * W / 2, (a[1] - b[1]) * H / 2).max())


# ---- one compose launch ------------------------------------------------------------------------------------------------------------

def normalised_shift(dx, dy, SH, SW):
    """Hm of a shift by (dx, dy) CANVAS pixels: canvas pixel j of frame t shows what pixel j + dx of frame t - 1 showed."""
    return np.array([1, 0, 2.0 * dx / SW, 0, 1, 2.0 * dy / SH, 0, 0, 1], F)


def homographies(SH, SW):
    """name -> Hm float32 [9]: identity, integer shift, sub-pixel shift, mild perspective, one whose w falls below w_min inside the frame."""
    return {"identity": normalised_shift(0, 0, SH, SW), "integer": normalised_shift(3, -2, SH, SW),
            "subpixel": normalised_shift(1.37, 0.61, SH, SW),
            "perspective": np.array([1.01, 0.02, 0.03, -0.015, 0.99, -0.02, 0.04, -0.03, 1], F),
            "w_crosses": np.array([1, 0, 0, 0, 1, 0, 1.6, 0.4, 1], F)}


def compose_case(N, SH, SW, seed):
    """-> dict of the arrays of one launch: warped, px, py, canvas_prev, age_prev.  The coordinates are a shifted, slightly scaled
    identity, so that a band of every side is uncovered; planted among them: NaN, values far outside, and coordinates exactly on
    qx = 0 and qx = 32 (SW - 1); the ages hold holes (255) and 0 and 254."""
    r = np.random.default_rng(seed)
    I, J = np.meshgrid(np.arange(SH, dtype=np.float64), np.arange(SW, dtype=np.float64), indexing="ij")
    px, py = np.zeros((N, SH, SW), F), np.zeros((N, SH, SW), F)
    for n in range(N):
        s, ox, oy = 1.0 + r.uniform(0.15, 0.3), r.uniform(-3, 3), r.uniform(-3, 3)
        px[n] = ((J - SW / 2) * s + SW / 2 + ox + r.normal(0, 0.2, (SH, SW))).astype(F)
        py[n] = ((I - SH / 2) * s + SH / 2 + oy + r.normal(0, 0.2, (SH, SW))).astype(F)
    k = r.integers(0, SH * SW * N, 24)
    px.ravel()[k[0:3]] = np.nan
    py.ravel()[k[3:6]] = np.nan
    px.ravel()[k[6:9]] = (1e30, -1e30, np.inf)
    py.ravel()[k[9:12]] = (-3e9, 4e12, -np.inf)
    px.ravel()[k[12:15]] = 0.0                                             # qx = 0 exactly: covered when y is
    px.ravel()[k[15:18]] = SW - 1                                           # qx = 32 (SW - 1) exactly
    py.ravel()[k[12:18]] = SH / 2.0
    px.ravel()[k[18:21]] = (-1.0 / 64 - 1e-4, SW - 1 + 1.0 / 64 + 1e-4, SW - 1 + 1.0 / 64)     # just outside; a tie that rounds to even
    py.ravel()[k[18:21]] = SH / 2.0
    age = r.integers(0, 90, (N, SH, SW)).astype(np.uint8)                    # most of them younger than the default max_age
    age[r.random((N, SH, SW)) < 0.25] = 0
    age[r.random((N, SH, SW)) < 0.1] = 254
    hole = r.random((N, SH, SW)) < 0.03
    hole[:, SH // 3:SH // 3 + 5, SW // 2:SW // 2 + 7] = True
    age[hole] = 255
    canvas = r.integers(0, 256, (N, SH, SW, 3)).astype(np.uint8)
    canvas[hole] = 0
    return dict(warped=r.integers(0, 256, (N, SH, SW, 3)).astype(np.uint8), px=px, py=py, canvas_prev=canvas, age_prev=age)
