"""Clips for the scoring tests: every frame is one texture (tvl1_model.texture: smooth noise at cell sizes of 4 and 12 pixels, coarse
enough to be tracked through a 1.25-fold zoom) moved by a known affine map q = A (p - centre) + centre + t, on the 0..255 scale.  stable: a smooth path, half a cycle of a cosine along x and a quarter of that along y.  unstable: the same path plus a
per-frame jitter of up to 3 px.  zoomed: the unstable clip magnified 1.25 times about the frame's centre."""
import functools

import numpy as np

import tvl1_model as M

F = np.float32
T, H, W = 16, 72, 96


MARGIN = 24


@functools.lru_cache(maxsize=None)
def _texture(seed):
    return M.texture(H + 2 * MARGIN, W + 2 * MARGIN, seed) * 255.0


def _frame(aff, seed):
    """The texture's point p is seen at q = A (p - centre) + centre + t: bilinear, float64, rounded once to float32."""
    tex = _texture(seed)
    a, b, c, d, tx, ty = aff
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cy, cx = (H - 1) / 2, (W - 1) / 2
    Ai = np.linalg.inv(np.array([[a, b], [c, d]], np.float64))
    qx, qy = X - cx - tx, Y - cy - ty
    x = np.clip(Ai[0, 0] * qx + Ai[0, 1] * qy + cx + MARGIN, 0, tex.shape[1] - 1.001)
    y = np.clip(Ai[1, 0] * qx + Ai[1, 1] * qy + cy + MARGIN, 0, tex.shape[0] - 1.001)
    x0, y0 = x.astype(int), y.astype(int)
    fx, fy = x - x0, y - y0
    return ((tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy).astype(F)


def _frames(affs, seed=21):
    out = np.stack([_frame(a, seed) for a in affs])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def paths():
    t = np.arange(T)
    sx = 4.0 * (1.0 - np.cos(np.pi * t / (T - 1)))
    sy = 0.25 * sx
    j = np.random.default_rng(8).uniform(-3.0, 3.0, (T, 2))
    return sx, sy, j


@functools.lru_cache(maxsize=None)
def stable():
    sx, sy, _ = paths()
    return _frames([(1, 0, 0, 1, sx[i], sy[i]) for i in range(T)])


@functools.lru_cache(maxsize=None)
def unstable():
    sx, sy, j = paths()
    return _frames([(1, 0, 0, 1, sx[i] + j[i, 0], sy[i] + j[i, 1]) for i in range(T)])


@functools.lru_cache(maxsize=None)
def zoomed(z=1.25):
    sx, sy, j = paths()
    return _frames([(z, 0, 0, z, z * (sx[i] + j[i, 0]), z * (sy[i] + j[i, 1])) for i in range(T)])


def model_homographies(i0, i1):
    """klt_model.matches -> homfit_model.fit for every pair (i0[t], i1[t]), the pair's index in the batch being t."""
    import homfit_model as HM
    import klt_model as K
    ny, nx = K.cells(H, W)
    rows, n = zip(*[K.matches(a, b, ny * nx + 1) for a, b in zip(i0, i1)])
    return HM.fit_batch(np.stack(rows), np.array(n, np.int32), H, W)


def model_score(u, s):
    """The CPU models chained: (metrics dict, H_us, status_us, H_ss, status_ss)."""
    import homfit_model as HM
    H_us, _, _, st_us, _ = model_homographies(u, s)
    H_ss, _, _, st_ss, _ = model_homographies(s[:-1], s[1:])
    return HM.metrics(H_us, st_us, H_ss, st_ss, H, W), H_us, st_us, H_ss, st_ss
