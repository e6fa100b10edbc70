"""NumPy float32 model of csrc/tvl1.hip, stage by stage: the yardstick of the TV-L1 tests, as tf_image_model.py is for get_img.
Zach / Pock / Bischof TV-L1 in the IPOL formulation (Sanchez, Meinhardt-Llopis, Facciolo), cut down to deterministic float32
stencils: a fixed number of inner iterations (no epsilon stop), no median filter, bilinear warps, a pyramid factor of exactly 2.
Every operation is one float32 operation with one rounding, in the order written here; the kernels perform the same operations in
the same order, so the comparison is bit for bit.  Written for exactness, not speed; images are single [H,W] arrays."""
import numpy as np

F = np.float32

DEFAULTS = dict(tau=0.25, lam=0.15, theta=0.3, scales=5, warps=5, iters=30, min_side=16)


def level_sizes(H, W, scales=5, min_side=16):
    """[(h, w)] from the finest level: one more while there are fewer than `scales` and min(h, w) // 2 >= min_side."""
    s = [(int(H), int(W))]
    while len(s) < scales and min(s[-1]) // 2 >= min_side:
        s.append(((s[-1][0] + 1) // 2, (s[-1][1] + 1) // 2))
    return s


def pyramid_down(I):
    """[1,4,6,4,1]/16 along x, then along y, replicated borders, summed left to right; then the pixels at even (y, x)."""
    I = np.asarray(I, F)
    k = [F(1) / F(16), F(4) / F(16), F(6) / F(16), F(4) / F(16), F(1) / F(16)]
    H, W = I.shape
    P = np.pad(I, ((0, 0), (2, 2)), mode="edge")
    t = k[0] * P[:, 0:W]
    for i in range(1, 5):
        t = t + k[i] * P[:, i:i + W]
    P = np.pad(t, ((2, 2), (0, 0)), mode="edge")
    t = k[0] * P[0:H, :]
    for i in range(1, 5):
        t = t + k[i] * P[i:i + H, :]
    assert t.dtype == F
    return np.ascontiguousarray(t[::2, ::2])


def gradient(I):
    """Centred differences 0.5 * (next - prev) on replicated borders -> (Ix, Iy)."""
    P = np.pad(np.asarray(I, F), 1, mode="edge")
    return F(0.5) * (P[1:-1, 2:] - P[1:-1, :-2]), F(0.5) * (P[2:, 1:-1] - P[:-2, 1:-1])


def bilinear(I, y, x):
    """I at float32 coordinates (y, x): clamped to [0, n-1], upper neighbour clamped to n-1;
    top = a + fx*(b-a), bot = c + fx*(d-c), top + fy*(bot-top)."""
    H, W = I.shape
    x = np.minimum(np.maximum(np.asarray(x, F), F(0)), F(W - 1))
    y = np.minimum(np.maximum(np.asarray(y, F), F(0)), F(H - 1))
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int32), yf.astype(np.int32)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - xf, y - yf
    a, b, c, d = I[y0, x0], I[y0, x1], I[y1, x0], I[y1, x1]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    out = top + fy * (bot - top)
    assert out.dtype == F
    return out


def upsample(u, H, W):
    """Half-pixel-centred bilinear to exactly (H, W): source coordinate (i + 0.5) * 0.5 - 0.5, clamped; times 2."""
    yy = (np.arange(H, dtype=F) + F(0.5)) * F(0.5) - F(0.5)
    xx = (np.arange(W, dtype=F) + F(0.5)) * F(0.5) - F(0.5)
    Y, X = np.meshgrid(yy, xx, indexing="ij")
    return F(2) * bilinear(np.asarray(u, F), Y, X)


def warp_constants(I0, I1, I1x, I1y, u1, u2):
    """-> Ix, Iy, rc, g: I1 and its gradient sampled at (x + u1, y + u2), g = Ix*Ix + Iy*Iy, rc = ((Iw - Ix*u1) - Iy*u2) - I0."""
    H, W = I0.shape
    Y, X = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    xs, ys = X + u1, Y + u2
    Iw, Ix, Iy = bilinear(I1, ys, xs), bilinear(I1x, ys, xs), bilinear(I1y, ys, xs)
    g = Ix * Ix + Iy * Iy
    rc = ((Iw - Ix * u1) - Iy * u2) - np.asarray(I0, F)
    assert g.dtype == F and rc.dtype == F
    return Ix, Iy, rc, g


def _div(px, py):
    dx = px.copy()
    dx[:, 1:-1] = px[:, 1:-1] - px[:, :-2]
    dx[:, -1] = -px[:, -2]
    dy = py.copy()
    dy[1:-1, :] = py[1:-1, :] - py[:-2, :]
    dy[-1, :] = -py[-2, :]
    return dx + dy


def _fwd(u):
    gx = np.zeros_like(u)
    gx[:, :-1] = u[:, 1:] - u[:, :-1]
    gy = np.zeros_like(u)
    gy[:-1, :] = u[1:, :] - u[:-1, :]
    return gx, gy


def iterate(state, consts, n, tau=0.25, lam=0.15, theta=0.3):
    """n inner iterations.  state: (u1, u2, p11, p12, p21, p22); consts: (Ix, Iy, rc, g) -> the new state (inputs untouched)."""
    u1, u2, p11, p12, p21, p22 = [np.array(a, F) for a in state]
    Ix, Iy, rc, g = [np.asarray(a, F) for a in consts]
    lt, taut, th = F(lam) * F(theta), F(tau) / F(theta), F(theta)
    for _ in range(int(n)):
        rho = (rc + Ix * u1) + Iy * u2
        lg = lt * g
        c1, c2 = rho < -lg, rho > lg
        c3 = ~c1 & ~c2 & (g > F(1e-10))
        with np.errstate(all="ignore"):
            f = np.where(c1, lt, np.where(c2, -lt, np.where(c3, -rho / g, F(0)))).astype(F)
        u1 = (u1 + f * Ix) + th * _div(p11, p12)
        u2 = (u2 + f * Iy) + th * _div(p21, p22)
        a, b = _fwd(u1)
        nrm = F(1) + taut * np.sqrt(a * a + b * b)
        p11, p12 = (p11 + taut * a) / nrm, (p12 + taut * b) / nrm
        a, b = _fwd(u2)
        nrm = F(1) + taut * np.sqrt(a * a + b * b)
        p21, p22 = (p21 + taut * a) / nrm, (p22 + taut * b) / nrm
        assert u1.dtype == F and p11.dtype == F and nrm.dtype == F
    return u1, u2, p11, p12, p21, p22


def flow_to_map(u1, u2):
    """[H,W,2] in the convention interpolate() reads (xp = (x+1)*W/2): 2*(j + u1)/W - 1, 2*(i + u2)/H - 1."""
    H, W = u1.shape
    Y, X = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    return np.stack([(F(2) * (X + u1)) / F(W) - F(1), (F(2) * (Y + u2)) / F(H) - F(1)], axis=-1)


def solve(I0, I1, tau=0.25, lam=0.15, theta=0.3, scales=5, warps=5, iters=30, min_side=16):
    """The whole solve of one pair -> (u1, u2) with I1(x + u1, y + u2) ~ I0(x, y)."""
    p0, p1 = [np.asarray(I0, F)], [np.asarray(I1, F)]
    for _ in level_sizes(*p0[0].shape, scales=scales, min_side=min_side)[1:]:
        p0.append(pyramid_down(p0[-1]))
        p1.append(pyramid_down(p1[-1]))
    u1 = u2 = None
    for A, B in zip(p0[::-1], p1[::-1]):
        H, W = A.shape
        if u1 is None:
            u1, u2 = np.zeros((H, W), F), np.zeros((H, W), F)
        else:
            u1, u2 = upsample(u1, H, W), upsample(u2, H, W)
        p = [np.zeros((H, W), F) for _ in range(4)]
        Bx, By = gradient(B)
        for _ in range(warps):
            consts = warp_constants(A, B, Bx, By, u1, u2)
            u1, u2, *p = iterate((u1, u2, *p), consts, iters, tau, lam, theta)
    return u1, u2


# ---- synthetic pairs with a known motion (the CPU tests) ----------------------------------------------------------------------------

def _smooth(a, H, W):
    yy, xx = np.linspace(0, a.shape[0] - 1.001, H), np.linspace(0, a.shape[1] - 1.001, W)
    Y, X = np.meshgrid(yy, xx, indexing="ij")
    y0, x0 = Y.astype(int), X.astype(int)
    fy, fx = Y - y0, X - x0
    return (a[y0, x0] * (1 - fx) + a[y0, x0 + 1] * fx) * (1 - fy) + (a[y0 + 1, x0] * (1 - fx) + a[y0 + 1, x0 + 1] * fx) * fy


def texture(H, W, seed):
    """Smooth random texture in 0..1: bilinearly upsampled uniform noise at cell sizes 4 and 12, weights 0.6 / 0.4."""
    r = np.random.default_rng(seed)
    big = r.random((H // 4 + 8, W // 4 + 8))
    return _smooth(big, H, W) * 0.6 + _smooth(r.random((H // 12 + 4, W // 12 + 4)), H, W) * 0.4


def make_pair(H, W, seed, aff):
    """aff = (a, b, c, d, tx, ty): q = M (p - centre) + centre + t.  -> I0, I1 (float32, 0..255), and the true flow ux, uy
    (float64).  Both images are sampled from one 4x supersampled texture."""
    S = 4
    T = texture(H * S, W * S, seed)

    def samp(y, x):
        y, x = np.clip(y * S, 0, T.shape[0] - 1.001), np.clip(x * S, 0, T.shape[1] - 1.001)
        y0, x0 = y.astype(int), x.astype(int)
        fy, fx = y - y0, x - x0
        return (T[y0, x0] * (1 - fx) + T[y0, x0 + 1] * fx) * (1 - fy) + (T[y0 + 1, x0] * (1 - fx) + T[y0 + 1, x0 + 1] * fx) * fy

    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b, c, d, tx, ty = aff
    cy, cx = (H - 1) / 2, (W - 1) / 2
    Mi = np.linalg.inv(np.array([[a, b], [c, d]]))
    qx, qy = X - cx - tx, Y - cy - ty
    I1 = samp(Mi[1, 0] * qx + Mi[1, 1] * qy + cy, Mi[0, 0] * qx + Mi[0, 1] * qy + cx)
    ux = a * (X - cx) + b * (Y - cy) + cx + tx - X
    uy = c * (X - cx) + d * (Y - cy) + cy + ty - Y
    return (samp(Y, X) * 255).astype(F), (I1 * 255).astype(F), ux, uy
