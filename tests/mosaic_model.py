"""NumPy model of csrc/mosaic.hip, the executable statement of include/stabnet_hip.h's full-frame section: the coverage guard over a
match list (stabnet_mosaic_guard_matches) and the per-pixel composite of the current warped frame with the previous canvas
(stabnet_mosaic_compose).  float32 and float64 operations are single operations with one rounding each, in the order written here;
everything else is integer arithmetic.  The kernels perform the same operations in the same order: the comparison is bit for bit."""
import numpy as np

F = np.float32
D = np.float64
EMPTY = 255                      # the age of a canvas pixel that holds nothing
FRESH, BLENDED, HISTORY, NONE = 0, 1, 2, 3          # the order of counts [4]

DEFAULTS = dict(feather_log2=3, max_age=64, guard=8, w_min=1e-6)


# ---- the guard -----------------------------------------------------------------------------------------------------------------

def end_safe(xn, yn, black, guard):
    """xn, yn float32 [n]: one end of every row in the frame 2x/W - 1; black float32 [H,W] -> bool [n]: the (2 guard + 1)^2 box
    about the rounded pixel lies inside the image and every black in it is < 0.5.  A NaN coordinate is unsafe."""
    black = np.asarray(black, F)
    H, W = black.shape
    xn, yn = np.asarray(xn, F), np.asarray(yn, F)
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((xn + F(1)) * F(W)) * F(0.5)
        Y = ((yn + F(1)) * F(H)) * F(0.5)
        xr, yr = np.rint(X), np.rint(Y)
        assert xr.dtype == F
        g = F(guard)
        inside = (xr - g >= F(0)) & (xr + g <= F(W - 1)) & (yr - g >= F(0)) & (yr + g <= F(H - 1))        # (false for NaN)
    bad = (black >= F(0.5)) | np.isnan(black)                      # "every black is < 0.5": a NaN is not
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = bad.cumsum(0).cumsum(1)
    out = np.zeros(len(xn), bool)
    xi, yi = xr[inside].astype(np.int64), yr[inside].astype(np.int64)
    x0, x1, y0, y1 = xi - guard, xi + guard + 1, yi - guard, yi + guard + 1
    out[inside] = (S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]) == 0
    return out


def guard_matches(rows, n, black0, black1, guard=8):
    """rows float32 [M,4] = (x0, y0, x1, y1), only the first n are read; black0, black1 [H,W]: the coverage of the frame each end
    lives in -> (out [M,4]: the rows whose two ends are safe, in their order, zeros after them; their number)."""
    rows = np.asarray(rows, F)
    M = len(rows)
    n = min(max(int(n), 0), M)
    r = rows[:n]
    keep = end_safe(r[:, 0], r[:, 1], black0, guard) & end_safe(r[:, 2], r[:, 3], black1, guard)
    out = np.zeros((M, 4), F)
    k = int(keep.sum())
    out[:k] = r[keep]
    return out, k


def guard_batch(rows, n, black0, black1, guard=8):
    out = [guard_matches(rows[b], n[b], black0[b], black1[b], guard) for b in range(len(rows))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


# ---- the composite -------------------------------------------------------------------------------------------------------------

def quant32(p):
    """float32 coordinate -> int64 in 1/32 px: * 32, clamped to +-2e9, rounded half to even; NaN -> -2e9 (the remap's rule)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.asarray(p, F) * F(32), F(-2.0e9), F(2.0e9))
    assert q.dtype == F
    return np.rint(np.nan_to_num(q, nan=-2.0e9)).astype(np.int64)


def quant64(p):
    """The same rule on a float64 coordinate (the history sample's)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.asarray(p, D) * 32.0, -2.0e9, 2.0e9)
    return np.rint(np.nan_to_num(q, nan=-2.0e9)).astype(np.int64)


def depth(px, py, SH, SW):
    """d int64 [SH,SW] in 1/32 px: how far the rounded coordinate lies inside the source frame; covered = d >= 0."""
    qx, qy = quant32(px), quant32(py)
    return np.minimum(np.minimum(qx, 32 * (SW - 1) - qx), np.minimum(qy, 32 * (SH - 1) - qy))


def constants(SH, SW, H, W):
    """Eight float64 constants of the pixel <-> normalised change of coordinates, each expression as the host evaluates it.
    x_n = ax j + cx (cv2's half-pixel convention between SW and W pixels, then 2u/W - 1); j = sx x_n + tx is its inverse."""
    ax, cx = 2.0 / SW, (1.0 / SW - 1.0 / W) - 1.0
    ay, cy = 2.0 / SH, (1.0 / SH - 1.0 / H) - 1.0
    sx, tx = 0.5 * SW, (0.5 * SW + (0.5 * SW) / W) - 0.5
    sy, ty = 0.5 * SH, (0.5 * SH + (0.5 * SH) / H) - 0.5
    return ax, cx, ay, cy, sx, tx, sy, ty


def pixel_homography(Hm, SH, SW, H, W):
    """G [9] float64 = B (Hm A): canvas pixel (j, i, 1) of frame t -> canvas pixel of frame t - 1, up to scale."""
    h = np.asarray(Hm, F).astype(D).reshape(9)
    ax, cx, ay, cy, sx, tx, sy, ty = constants(SH, SW, H, W)
    with np.errstate(all="ignore"):
        m = [None] * 9
        for r in range(3):
            m[3 * r + 0] = h[3 * r + 0] * ax
            m[3 * r + 1] = h[3 * r + 1] * ay
            m[3 * r + 2] = (h[3 * r + 0] * cx + h[3 * r + 1] * cy) + h[3 * r + 2]
        g = [sx * m[c] + tx * m[6 + c] for c in range(3)] + [sy * m[3 + c] + ty * m[6 + c] for c in range(3)] + m[6:9]
    return np.array(g, D)


def history(canvas_prev, age_prev, Hm, status, H, W, max_age=64, w_min=1e-6):
    """The history sample of every pixel -> (hist uint8 [SH,SW,3], hist_age int64 [SH,SW], available bool [SH,SW])."""
    canvas_prev, age_prev = np.asarray(canvas_prev, np.uint8), np.asarray(age_prev, np.uint8)
    SH, SW = age_prev.shape
    hist, hage, avail = np.zeros((SH, SW, 3), np.uint8), np.zeros((SH, SW), np.int64), np.zeros((SH, SW), bool)
    if int(status) not in (1, 2):
        return hist, hage, avail
    G = pixel_homography(Hm, SH, SW, H, W)
    I, J = np.meshgrid(np.arange(SH, dtype=D), np.arange(SW, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        u = (G[0] * J + G[1] * I) + G[2]
        v = (G[3] * J + G[4] * I) + G[5]
        w = (G[6] * J + G[7] * I) + G[8]
        ok = w > D(F(w_min))
        qx, qy = quant64(u / w), quant64(v / w)
    ix, iy, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
    ok &= (ix >= 0) & (ix + (fx != 0) <= SW - 1) & (iy >= 0) & (iy + (fy != 0) <= SH - 1)     # every tap with weight lies inside
    ix, iy, fx, fy = ix[ok], iy[ok], fx[ok], fy[ok]
    acc, amax, full = np.zeros((len(ix), 3), np.int64), np.zeros(len(ix), np.int64), np.ones(len(ix), bool)
    for dy, dx, wt in ((0, 0, (32 - fy) * (32 - fx)), (0, 1, (32 - fy) * fx), (1, 0, fy * (32 - fx)), (1, 1, fy * fx)):
        y, x = np.minimum(iy + dy, SH - 1), np.minimum(ix + dx, SW - 1)     # (a clamped tap has weight 0)
        a = age_prev[y, x].astype(np.int64)
        on = wt != 0
        full &= ~on | (a < EMPTY)
        amax = np.where(on, np.maximum(amax, a), amax)
        acc += canvas_prev[y, x].astype(np.int64) * wt[:, None]
    good = full & (amax + 1 <= max_age)
    sel = np.flatnonzero(ok.ravel())[good]
    hist.reshape(-1, 3)[sel] = ((acc[good] + 512) >> 10).astype(np.uint8)
    hage.ravel()[sel] = amax[good] + 1
    avail.ravel()[sel] = True
    return hist, hage, avail


def compose(warped, px, py, canvas_prev, age_prev, Hm, status, H, W, feather_log2=3, max_age=64, w_min=1e-6, classes=False):
    """One stream: warped uint8 [SH,SW,3], px, py float32 [SH,SW] as the source-size remap wrote them, the previous canvas and ages,
    Hm [9] float32 and status as the fit wrote them (frame t -> frame t - 1, normalised) -> (canvas uint8 [SH,SW,3], age uint8
    [SH,SW], counts int32 [4] = fresh, blended, history, empty) (and the class of every pixel with classes=True)."""
    warped = np.asarray(warped, np.uint8)
    SH, SW = warped.shape[:2]
    Fq = 32 << feather_log2
    d = depth(px, py, SH, SW)
    a = np.clip(d, 0, Fq)
    covered = d >= 0
    hist, hage, avail = history(canvas_prev, age_prev, Hm, status, H, W, max_age, w_min)
    avail &= d < Fq                                                         # deeper than the feather band nothing looks at history
    cls = np.where(covered, np.where(avail, BLENDED, FRESH), np.where(avail, HISTORY, NONE))
    blend = (warped.astype(np.int64) * a[..., None] + hist.astype(np.int64) * (Fq - a)[..., None] + Fq // 2) >> (5 + feather_log2)
    out = np.zeros_like(warped)
    age = np.full((SH, SW), EMPTY, np.uint8)
    m = cls == FRESH
    out[m], age[m] = warped[m], 0
    m = cls == BLENDED
    out[m] = blend[m].astype(np.uint8)
    age[m] = np.where(2 * a[m] >= Fq, 0, hage[m]).astype(np.uint8)
    m = cls == HISTORY
    out[m], age[m] = hist[m], hage[m].astype(np.uint8)
    counts = np.bincount(cls.ravel(), minlength=4).astype(np.int32)
    return (out, age, counts, cls) if classes else (out, age, counts)


def compose_batch(warped, px, py, canvas_prev, age_prev, Hm, status, H, W, **kw):
    out = [compose(warped[n], px[n], py[n], canvas_prev[n], age_prev[n], Hm[n], status[n], H, W, **kw) for n in range(len(warped))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
