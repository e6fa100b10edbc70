"""NumPy float32 model of csrc/klt.hip, stage by stage: the yardstick of the corner-tracking tests, as tvl1_model.py is for the flow.
Shi-Tomasi corners, one per grid cell; pyramidal Lucas-Kanade with a fixed number of iterations; a forward-backward check.  Every
operation is one float32 operation with one rounding, in the order written here, the window sums included (a lane of a 64-lane
wave adds its samples in order, then six butterfly steps): the kernels perform the same operations in the same order, so the
comparison is bit for bit.  Pyramid, gradient and bilinear sampling are tvl1_model's.  Images are single [H,W] arrays."""
import numpy as np

from tvl1_model import bilinear, gradient, level_sizes, pyramid_down

F = np.float32
LANES = 64

DEFAULTS = dict(levels=4, min_side=16, r=2, border=8, cell=16, floor=1.0, quality=0.01, R=7, iters=10, min_eig=1e-3, fb=0.5)


def cells(H, W, cell=16):
    """(rows, columns) of the grid: partial cells at the right and bottom edges count."""
    return (H + cell - 1) // cell, (W + cell - 1) // cell


def pyramid(I, levels=4, min_side=16):
    p = [np.asarray(I, F)]
    for _ in level_sizes(*p[0].shape, scales=levels, min_side=min_side)[1:]:
        p.append(pyramid_down(p[-1]))
    return p


def _min_eig(a, b, c):
    d = a - c
    return F(0.5) * ((a + c) - np.sqrt(d * d + F(4) * (b * b)))


def response(I, r=2, border=8):
    """The smaller eigenvalue of the structure tensor summed over a (2r+1)^2 box: along x left to right, then along y top to
    bottom; 0 for pixels closer than `border` (> r) to an image edge, so that no box leaves the image."""
    I = np.asarray(I, F)
    H, W = I.shape
    assert border >= r + 1 and H >= 2 * border + 1 and W >= 2 * border + 1
    gx, gy = gradient(I)
    out = np.zeros((H, W), F)
    sums = []
    for prod in (gx * gx, gx * gy, gy * gy):
        t = prod[:, 0:W - 2 * r]
        for k in range(1, 2 * r + 1):
            t = t + prod[:, k:k + W - 2 * r]                      # t[y, x - r] = the row sum centred on x
        s = t[0:H - 2 * r]
        for k in range(1, 2 * r + 1):
            s = s + t[k:k + H - 2 * r]
        sums.append(s)                                           # s[y - r, x - r]
    resp = _min_eig(*sums)
    assert resp.dtype == F
    out[border:H - border, border:W - border] = resp[border - r:H - border - r, border - r:W - border - r]
    return out


def detect(resp, cell=16, floor=1.0, quality=0.01):
    """-> [cells, 4] float32 in row-major cell order: x, y, response, detected (1 / 0).  The candidate of a cell is its largest
    response, ties to the smallest (y, x); detected: resp > 0, resp >= floor, resp >= quality * (the largest response)."""
    H, W = resp.shape
    ny, nx = cells(H, W, cell)
    out = np.zeros((ny * nx, 4), F)
    for cy in range(ny):
        for cx in range(nx):
            blk = resp[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell]
            k = int(np.argmax(blk))                              # the first of equal maxima in row-major order
            y, x = divmod(k, blk.shape[1])
            out[cy * nx + cx, :3] = (cx * cell + x, cy * cell + y, blk[y, x])
    top = out[:, 2].max()
    v = out[:, 2]
    out[:, 3] = (v > 0) & (v >= F(floor)) & (v >= F(quality) * top)
    return out


def _wsum(t, valid):
    """t [N,4,64]: lane l adds its samples l, l+64, l+128, l+192 (the valid ones) in order, from 0; then the butterfly."""
    acc = np.zeros((t.shape[0], LANES), F)
    for k in range(4):
        acc = np.where(valid[k], acc + t[:, k, :], acc)
    lanes = np.arange(LANES)
    for dist in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ dist]
    assert acc.dtype == F
    assert (acc.view(np.uint32) == acc[:, :1].view(np.uint32)).all() or np.isnan(acc).any()
    return acc[:, 0]


def _sample(I, y, x):
    """bilinear() with the device's treatment of a NaN coordinate (fmaxf(NaN, 0) = 0): only lost points have any."""
    return bilinear(I, np.where(np.isnan(y), F(0), y), np.where(np.isnan(x), F(0), x))


def track_one_way(pa, pb, pts, R=7, iters=10, min_eig=1e-3):
    """pa, pb: pyramids (finest first) of the image the points lie in and of the other one; pts [N,2] float32 (x, y).
    -> q [N,2], lost [N] bool.  Nothing here depends on whether a point is already lost: its arithmetic goes on."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    N = len(pts)
    side = 2 * R + 1
    n = side * side
    assert n <= 4 * LANES
    s = np.arange(4)[:, None] * LANES + np.arange(LANES)[None, :]          # [4,64]
    valid = s < n
    oy, ox = (s // side - R).astype(F), (s % side - R).astype(F)
    lost = np.zeros(N, bool)
    dx, dy = np.zeros(N, F), np.zeros(N, F)
    q = np.zeros((N, 2), F)
    with np.errstate(all="ignore"):
        for l in range(len(pa) - 1, -1, -1):
            A, B = pa[l], pb[l]
            h, w = A.shape
            Ax, Ay = gradient(A)
            sc = F(2.0 ** -l)
            px, py = pts[:, 0] * sc, pts[:, 1] * sc
            x, y = px[:, None, None] + ox[None], py[:, None, None] + oy[None]
            T, Tx, Ty = _sample(A, y, x), _sample(Ax, y, x), _sample(Ay, y, x)
            a, b, c = _wsum(Tx * Tx, valid), _wsum(Tx * Ty, valid), _wsum(Ty * Ty, valid)
            det = a * c - b * b
            lost |= (_min_eig(a, b, c) / F(n) < F(min_eig)) | (det == 0)
            for _ in range(iters):
                e = T - _sample(B, y + dy[:, None, None], x + dx[:, None, None])
                bx, by = _wsum(e * Tx, valid), _wsum(e * Ty, valid)
                dx = dx + (c * bx - b * by) / det
                dy = dy + (a * by - b * bx) / det
            q = np.stack([px + dx, py + dy], axis=-1)
            lost |= ~((q[:, 0] >= 0) & (q[:, 0] <= F(w - 1)) & (q[:, 1] >= 0) & (q[:, 1] <= F(h - 1)))
            if l:
                dx, dy = F(2) * dx, F(2) * dy
    assert q.dtype == F and dx.dtype == F
    return q, lost


def track(p0, p1, pts, R=7, iters=10, min_eig=1e-3):
    """Forward from i0 to i1 and back.  -> [N,4] float32: qx, qy, lost (1 / 0), forward-backward distance squared; a lost
    point's row is (0, 0, 1, 0)."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    q, lf = track_one_way(p0, p1, pts, R, iters, min_eig)
    back, lb = track_one_way(p1, p0, q, R, iters, min_eig)
    with np.errstate(all="ignore"):
        ex, ey = back[:, 0] - pts[:, 0], back[:, 1] - pts[:, 1]
        fb2 = ex * ex + ey * ey
    lost = lf | lb
    out = np.stack([q[:, 0], q[:, 1], lost.astype(F), fb2], axis=-1).astype(F)
    out[lost] = (0, 0, 1, 0)
    return out


def rows(cand, trk, H, W, max_matches, fb=0.5):
    """-> matches [max_matches,4], n: the valid matches in cell order, at most max_matches - 1 of them, zeros from row n on."""
    valid = (cand[:, 3] != 0) & (trk[:, 2] == 0) & (trk[:, 3] <= F(fb) * F(fb))
    out = np.zeros((max_matches, 4), F)
    k = np.flatnonzero(valid)[:max_matches - 1]
    out[:len(k), 0] = (F(2) * cand[k, 0]) / F(W) - F(1)
    out[:len(k), 1] = (F(2) * cand[k, 1]) / F(H) - F(1)
    out[:len(k), 2] = (F(2) * trk[k, 0]) / F(W) - F(1)
    out[:len(k), 3] = (F(2) * trk[k, 1]) / F(H) - F(1)
    return out, len(k)


def matches(I0, I1, max_matches, levels=4, min_side=16, r=2, border=8, cell=16, floor=1.0, quality=0.01, R=7, iters=10,
            min_eig=1e-3, fb=0.5, stages=False):
    """The whole solve of one pair -> (matches [max_matches,4], n) (and the candidates and tracks with stages=True)."""
    p0, p1 = pyramid(I0, levels, min_side), pyramid(I1, levels, min_side)
    cand = detect(response(p0[0], r, border), cell, floor, quality)
    trk = track(p0, p1, cand[:, :2], R, iters, min_eig)
    m, n = rows(cand, trk, p0[0].shape[0], p0[0].shape[1], max_matches, fb)
    return (m, n, cand, trk) if stages else (m, n)
