"""Inputs of the homography tests, shared by the CPU file (the model against planted truth) and the GPU file (the kernel against the
model): rows planted under a known homography with uniform outliers, and the degenerate sets.  Coordinates are the normalised
frame's, 2x/W - 1 and 2y/H - 1."""
import numpy as np

F = np.float32

# pixel-frame homographies: a translation, a similarity (1.03 x, 2 degrees, shifted), a mild perspective
_c, _s = 1.03 * np.cos(np.deg2rad(2.0)), 1.03 * np.sin(np.deg2rad(2.0))
MODELS = {
    "translation": np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1]], np.float64),
    "similarity": np.array([[_c, -_s, 4.0], [_s, _c, -6.0], [0, 0, 1]], np.float64),
    "perspective": np.array([[1.01, 0.004, 2.0], [-0.003, 0.99, 1.5], [2e-5, -1e-5, 1]], np.float64),
}


def normalised(Hpx, H, W):
    """The pixel-frame homography in the normalised frame, with [2,2] = 1."""
    N = np.array([[2.0 / W, 0, -1], [0, 2.0 / H, -1], [0, 0, 1]], np.float64)
    Hn = N @ Hpx @ np.linalg.inv(N)
    return Hn / Hn[2, 2]


def apply_px(Hpx, p):
    q = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ Hpx.T
    return q[:, :2] / q[:, 2:3]


def outlier_count(n, share):
    """A model through four rows always has four inliers, so a planted set can only be told from a chance one when it has five rows
    or more: the outliers are floor(share * n), but never more than n - 5 (none for n = 4 and 5)."""
    return max(0, min(int(share * n), n - 5))


def planted(model, n, share, noise_px, H, W, seed, M=None):
    """-> (rows [M,4] float32 with NaN from row n on, inlier [n] bool, truth [9] float64 in the normalised frame).  Source points are
    uniform in the frame; an inlier's target is the model's, moved by up to noise_px per axis (uniform); an outlier's target is
    uniform in the frame and at least 4 px from the model's."""
    rng = np.random.default_rng(seed)
    Hpx = MODELS[model]
    M = n if M is None else M
    src = rng.uniform([0, 0], [W - 1, H - 1], (n, 2))
    dst = apply_px(Hpx, src) + rng.uniform(-noise_px, noise_px, (n, 2))
    inl = np.ones(n, bool)
    inl[rng.permutation(n)[:outlier_count(n, share)]] = False
    for i in np.flatnonzero(~inl):
        while True:
            q = rng.uniform([0, 0], [W - 1, H - 1])
            if np.hypot(*(q - apply_px(Hpx, src[i:i + 1])[0])) >= 4.0:
                break
        dst[i] = q
    rows = np.full((M, 4), np.nan, F)
    rows[:n, 0], rows[:n, 1] = 2 * src[:, 0] / W - 1, 2 * src[:, 1] / H - 1
    rows[:n, 2], rows[:n, 3] = 2 * dst[:, 0] / W - 1, 2 * dst[:, 1] / H - 1
    return rows, inl, normalised(Hpx, H, W).reshape(9)


def transfer_error_px(Hm, truth, rows, H, W):
    """The largest distance in pixels between where the two normalised-frame homographies send the rows' source points.  (Over the
    rows and not the frame's corners: four or five rows say little about a corner far from them.)"""
    p = np.concatenate([np.asarray(rows, np.float64)[:, :2], np.ones((len(rows), 1))], axis=1)
    a, b = p @ np.asarray(Hm, np.float64).reshape(3, 3).T, p @ np.asarray(truth, np.float64).reshape(3, 3).T
    d = (a[:, :2] / a[:, 2:3] - b[:, :2] / b[:, 2:3]) * np.array([W / 2.0, H / 2.0])
    return float(np.hypot(d[:, 0], d[:, 1]).max())


def identical(n, M=None):
    rows = np.full((M or n, 4), np.nan, F)
    rows[:n] = (0.25, -0.5, 0.3125, -0.4375)
    return rows


def collinear(n, M=None):
    """Points on the line y = x/2 + 1/4, moved by (1/32, 1/64): every coordinate is a small multiple of 2^-10, so each product and
    difference of the four-point model is exact, the adjugates' weights are exactly 0 and every hypothesis divides 0 by 0."""
    rows = np.full((M or n, 4), np.nan, F)
    x = (np.arange(n) * 37 % 512 - 256) / 512.0
    rows[:n, 0], rows[:n, 1] = x, x / 2 + 0.25
    rows[:n, 2], rows[:n, 3] = x + 1 / 32.0, x / 2 + 0.25 + 1 / 64.0
    return rows
