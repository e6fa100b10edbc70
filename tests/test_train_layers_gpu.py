"""GPU: the non-convolution training layers (csrc/train_layers.hip), one operator at a time against float64 on the CPU.

Batch-statistics BN forward, BN+ReLU backward, bias gradient, max-pool forward / argmax / backward, global-pool backward and FC
backward are otherwise reached only through whole training steps at one small shape.  Here each runs through its own C entry
point at the row / channel counts of the 8 x 288 x 512 step and at ragged edge shapes, every output and workspace between canary
bands, workspaces pre-filled with NaN.  References are NumPy / torch float64 written in this file; a bar that is not derived from
the number format is 4 x the error of a float32 NumPy restatement of the same arithmetic, measured in the test at the same inputs
(the figures measured when the test was written are in the comments marked MEASURED).  The L2 regulariser (stabnet_weight_decay)
and the host mirror's elementwise helpers (stabnet_axpb, stabnet_interleave2) follow at the end, through their own entry points."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

from _guarded import Guarded, _check_all, _same_bits

pytestmark = pytest.mark.gpu

EPS, DECAY = 1e-5, 0.997                                   # slim resnet_arg_scope (config.Config.bn_eps / bn_decay)
EPS32 = float(np.float32(EPS))
OMD = 1.0 - float(np.float32(DECAY))                       # 1 - decay as the kernel forms it in float32 (exact: Sterbenz)
U23, U24 = 2.0 ** -23, 2.0 ** -24

# per-tower (rows, channels) of the BN / bias sites of the 8 x 288 x 512 step, and shapes that are no multiple of the 64-column
# block, the 16-channel finalize block or the 64-row trip
PRODUCTION = [(294912, 64), (73728, 64), (73728, 256), (18432, 128), (18432, 512), (4608, 256), (4608, 1024), (1152, 512), (1152, 2048)]
EDGES = [(M, C) for M in (1, 12, 63, 64, 65, 1000) for C in (4, 16, 68, 132)]
SHAPES = PRODUCTION + EDGES
R_BUCKETS = (0, 1, 3, 8, 16, 32, 100)                      # |mean| / std of a channel


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


# ---- a. batch-statistics BN forward -----------------------------------------------------------------------------------------
def _bn_input(rng, M, C, buckets=R_BUCKETS):
    """x [M, C] float32 with |mean| / std of channel c = buckets[(c + M) % len] and unequal std 2^-6 .. 2^6; -> x, bucket index."""
    idx = (np.arange(C) + M) % len(buckets)
    r = np.array(buckets, np.float64)[idx]
    std = 2.0 ** rng.integers(-6, 7, C)
    sign = rng.choice([-1.0, 1.0], C)
    x = (rng.standard_normal((M, C)) * std + sign * r * std).astype(np.float32)
    return x, idx


def _affine(rng, C):
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    return gamma, beta


def _bn_fwd(cuda, xs, gamma, beta, mov=None, decay=DECAY, partial_floats=None):
    """stabnet_bn_stats_train on the device tensors xs (one per group).  -> ([stats [4, C] per group], mov_mean, mov_var)."""
    from stabnet_amd import train_ops
    M, C = xs[0].shape
    stats = [Guarded(cuda, 4 * C) for _ in xs]
    partial = Guarded(cuda, train_ops.col_reduce_workspace_floats(M, C, len(xs)))
    mm = Guarded(cuda, C, mov[0]) if mov is not None else None
    mv = Guarded(cuda, C, mov[1]) if mov is not None else None
    train_ops.bn_stats_train(xs, gamma, beta, EPS, decay, [s.t for s in stats], mm.t if mm else None, mv.t if mv else None, partial.t)
    _check_all({"stats0": stats[0], "stats1": stats[-1], "partial": partial, "mov_mean": mm, "mov_var": mv})
    out = [s.np().reshape(4, C) for s in stats]
    assert all(np.isfinite(o).all() for o in out), "non-finite statistics (an unwritten workspace word was read?)"
    # (the statistics keep float64 partials; the whole workspace of the size query is theirs)
    assert bool(torch.isfinite(partial.t.view(torch.float64)).all()), "workspace words the size query counts were never written"
    if mov is None:
        return out, None, None
    return out, mm.np(), mv.np()


def _bn_ref64(x, gamma, beta):
    x64 = x.astype(np.float64)
    mean, var = x64.mean(0), x64.var(0)
    inv = 1.0 / np.sqrt(var + EPS32)
    scale = inv * gamma
    return mean, var, inv, scale, beta - mean * scale


def _bn_ref32(x, gamma, beta):
    """tf.nn.moments + tf.nn.batch_normalization restated in float32 NumPy (two passes: mean, then mean of squared differences)."""
    mean = x.mean(0, dtype=np.float32)
    var = np.square(x - mean).mean(0, dtype=np.float32)
    inv = (np.float32(1.0) / np.sqrt(var + np.float32(EPS))).astype(np.float32)
    scale = inv * gamma
    return mean, var, inv, scale, beta - mean * scale


def _moving64(old, value):
    return old.astype(np.float64) - (old.astype(np.float64) - value) * OMD


def _moving32(old, value):
    return old - (old - value.astype(np.float32)) * (np.float32(1.0) - np.float32(DECAY))


@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_stats_against_float64(cuda, M, C):
    """Variance within the conditioning bound of E[x^2] - mean^2, (1 + r^2) 2^-23 with r = |mean| / std, per channel, for r up to
    100; invstd / scale within what follows from it plus their own float32 roundings; mean, shift and the moving averages within
    4 x the error of the float32 two-pass restatement.
    MEASURED on an MI355X, worst over all shapes (the test prints the figures of each shape):
      relative variance error at r = 0 / 1 / 3 / 8 / 16 / 32 / 100
        kernel (float64 sums)             5.8e-8 / 5.9e-8 / 5.9e-8 / 6.0e-8 / 5.9e-8 / 5.9e-8 / 5.9e-8   (2^-24 = 6.0e-8)
        float32 two-pass (NumPy)          9.3e-5 / 1.0e-4 / 1.0e-4 / 9.1e-5 / 9.4e-5 / 9.3e-5 / 8.3e-5   (294 912 rows, summed in order)
        bound (1 + r^2) 2^-23, smallest   1.2e-7 / 1.7e-7 / 6.4e-7 / 4.2e-6 / 1.7e-5 / 7.6e-5 / 8.0e-4
        the kernels before the float64 sums: 2.0e-7 / 7.4e-7 / 1.4e-5 / 8.5e-5 / 1.3e-4 / 5.6e-4 / 4.5e-3 (53 cases of this file failed)
      mean 5.8e-8, shift 2.2e-7, mov_mean 5.6e-8, mov_var 4.2e-8 of the channel's magnitude, each at most 1.00 x the float32
      restatement's error at the same shape (which ranges from 1e-8 at a few rows to 5.7e-5 at 294 912)."""
    rng = np.random.default_rng(1000 * C + M)
    x, idx = _bn_input(rng, M, C)
    gamma, beta = _affine(rng, C)
    mean64, var64, inv64, scale64, shift64 = _bn_ref64(x, gamma, beta)
    mean32, var32, inv32, scale32, shift32 = _bn_ref32(x, gamma, beta)
    xd, gd, bd = _dev(x, cuda), _dev(gamma, cuda), _dev(beta, cuda)

    # decay = 0 on zero-seeded moving averages hands out the kernel's float32 mean and variance themselves:
    # mov -= (mov - value) * (1 - 0)  ->  0 - (0 - value) = value
    zero = np.zeros(C, np.float32)
    (st,), meanf, varf = _bn_fwd(cuda, [xd], gd, bd, mov=(zero, zero), decay=0.0)
    bound = (var64 + mean64 ** 2) * U23                                # = var * (1 + r^2) * 2^-23
    e_var = np.abs(varf.astype(np.float64) - var64)
    e_var32 = np.abs(var32.astype(np.float64) - var64)
    if M > 1:
        print("M=%d C=%d relative variance error per r bucket: GPU | float32 two-pass | bound (1 + r^2) 2^-23" % (M, C))
        for b, r in enumerate(R_BUCKETS):
            sel = idx == b
            if sel.any():
                print("  MEASURED r=%-3d  %.2e | %.2e | %.2e" % (r, (e_var[sel] / var64[sel]).max(), (e_var32[sel] / var64[sel]).max(),
                                                               (bound[sel] / var64[sel]).min()))
    worst = int(np.argmax(e_var / bound))
    assert (e_var <= bound).all(), ("variance of channel %d (r = %g): error %.3e of var, bound %.3e" % (
        worst, R_BUCKETS[idx[worst]], e_var[worst] / var64[worst], bound[worst] / var64[worst]))
    assert np.array_equal(st[2], meanf)                                  # save_mean is that mean
    # invstd = 1 / sqrtf(varf + eps): half the relative error of (var + eps), plus three float32 roundings -- the sum (2^-24 of the
    # radicand = 2^-25 of the root), the root and the quotient (2^-24 each, both correctly rounded) = 2.5 * 2^-24 (+1% for the
    # second order); scale = invstd * gamma: one more rounding
    rel_var = bound / (var64 + EPS32)
    bar_inv = 1.01 * (0.5 * rel_var + 2.5 * U24)
    e_inv = np.abs(st[3] / inv64 - 1.0)
    assert (e_inv <= bar_inv).all(), float((e_inv / bar_inv).max())
    e_scale = np.abs(st[0] / scale64 - 1.0)
    assert (e_scale <= bar_inv + 1.01 * U24).all(), float((e_scale / (bar_inv + 1.01 * U24)).max())

    # the step's own call: decay 0.997, moving averages seeded with random old values
    old_m = (mean64 + np.sqrt(var64 + 1e-3) * rng.standard_normal(C)).astype(np.float32)
    old_v = (var64 * rng.uniform(0.5, 2.0, C) + 1e-3).astype(np.float32)
    (st2,), mm, mv = _bn_fwd(cuda, [xd], gd, bd, mov=(old_m, old_v))
    assert _same_bits(st2, st)                                          # the statistics do not depend on the moving averages
    std64 = np.sqrt(var64)
    tiny = np.finfo(np.float64).tiny
    checks = {   # name: (GPU, float32 restatement, float64, per-channel magnitude the error is read against)
        "mean": (st2[2], mean32, mean64, np.abs(mean64) + std64 + tiny),
        "shift": (st2[1], shift32, shift64, np.abs(beta) + np.abs(mean64 * scale64) + tiny),
        "mov_mean": (mm, _moving32(old_m, mean32), _moving64(old_m, mean64), np.abs(old_m) + np.abs(mean64) + tiny),
        "mov_var": (mv, _moving32(old_v, var32), _moving64(old_v, var64), np.abs(old_v) + var64 + tiny),
    }
    for name, (got, f32, f64, mag) in checks.items():
        e_gpu = (np.abs(got.astype(np.float64) - f64) / mag).max()
        e_f32 = (np.abs(f32.astype(np.float64) - f64) / mag).max()
        print("  MEASURED %-8s GPU %.2e | float32 two-pass %.2e (bar: 4 x)" % (name, e_gpu, e_f32))
        assert e_gpu <= 4.0 * e_f32, (name, e_gpu, e_f32)


@pytest.mark.parametrize("M,C", [(73728, 64), (1152, 2048), (65, 68), (12, 4), (1000, 132)])
def test_bn_stats_groups_moving_null_and_determinism(cuda, M, C):
    rng = np.random.default_rng(7 * C + M)
    x1, _ = _bn_input(rng, M, C)
    x2, _ = _bn_input(rng, M, C)
    gamma, beta = _affine(rng, C)
    xd1, xd2, gd, bd = _dev(x1, cuda), _dev(x2, cuda), _dev(gamma, cuda), _dev(beta, cuda)
    old = (rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32))
    (a1,), m1, v1 = _bn_fwd(cuda, [xd1], gd, bd, mov=old)
    (a2,), m2, v2 = _bn_fwd(cuda, [xd2], gd, bd, mov=(m1, v1))           # tower 1's update, then tower 2's
    (p1, p2), mp, vp = _bn_fwd(cuda, [xd1, xd2], gd, bd, mov=old)
    assert _same_bits(p1, a1) and _same_bits(p2, a2) and _same_bits(mp, m2) and _same_bits(vp, v2)
    (q1, q2), mq, vq = _bn_fwd(cuda, [xd1, xd2], gd, bd, mov=old)       # the same call twice: the same bits
    assert _same_bits(q1, p1) and _same_bits(q2, p2) and _same_bits(mq, mp) and _same_bits(vq, vp)
    # no moving averages given: same statistics, and the arrays that were not passed keep their values
    keep = Guarded(cuda, 2 * C, np.concatenate(old))
    (n1, n2), _, _ = _bn_fwd(cuda, [xd1, xd2], gd, bd, mov=None)
    torch.cuda.synchronize()
    assert _same_bits(n1, p1) and _same_bits(n2, p2) and _same_bits(keep.np(), np.concatenate(old))


# ---- b. BN + ReLU backward --------------------------------------------------------------------------------------------------
def _upsample(addend, s, H, W):
    """[N, ceil(H/s), ceil(W/s), C] -> [N, H, W, C] with the values at (y % s == 0, x % s == 0) and zeros elsewhere."""
    N, Hs, Ws, C = addend.shape
    full = np.zeros((N, H, W, C), addend.dtype)
    full[:, ::s, ::s] = addend
    return full


def _bn_bwd_gpu(cuda, xs, gs, stats, gamma, seeds, addends=None, add_stride=1, H=0, W=0, alias=False):
    """-> ([d_x per group], d_gamma, d_beta); stats: device [4, C] tensors of the forward."""
    from stabnet_amd import train_ops
    M, C = xs[0].shape
    d_gamma, d_beta = Guarded(cuda, C, seeds[0]), Guarded(cuda, C, seeds[1])
    partial = Guarded(cuda, train_ops.col_reduce_workspace_floats(M, C, len(xs)))
    coefs = [Guarded(cuda, 3 * C) for _ in xs]
    if alias:                                   # d_x written over g
        dxs = [Guarded(cuda, M * C, "canary") for _ in xs]
        for d, g in zip(dxs, gs):
            d.t.copy_(g.reshape(-1))
        g_in = [d.t.view(M, C) for d in dxs]
    else:
        dxs = [Guarded(cuda, M * C) for _ in xs]
        g_in = gs
    train_ops.bn_relu_bwd(xs, g_in, stats, gamma, d_gamma.t, d_beta.t, [d.t for d in dxs], [c.t for c in coefs],
                          addends=addends, add_stride=add_stride, H=H, W=W, partial=partial.t)
    _check_all({"d_gamma": d_gamma, "d_beta": d_beta, "partial": partial, "coef0": coefs[0], "coef1": coefs[-1], "d_x0": dxs[0],
                "d_x1": dxs[-1]})
    # (float32 partials: the first half of the workspace, which is sized for the float64 ones of the statistics)
    assert bool(torch.isfinite(partial.t[:partial.n // 2]).all()) and all(bool(torch.isfinite(c.t).all()) for c in coefs)
    out = [d.np().reshape(M, C) for d in dxs]
    assert all(np.isfinite(o).all() for o in out)
    return out, d_gamma.np(), d_beta.np()


def _bn_bwd_ref64(x, g, gamma, beta, mask):
    """float64 autograd of sum(g * relu(batch_norm_batch(x))) with the ReLU decision forced to `mask`."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gm = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    mean = xt.mean(0)
    var = xt.var(0, unbiased=False)
    y = (xt - mean) / torch.sqrt(var + EPS32) * gm + bt
    (y * torch.tensor(g.astype(np.float64) * mask)).sum().backward()
    return xt.grad.numpy(), gm.grad.numpy(), bt.grad.numpy()


def _bn_bwd_ref32(x, g, gamma, beta, mask):
    """The kernels' formula, d_x = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)), in float32 NumPy on the two-pass statistics."""
    mean, var, inv, _, _ = _bn_ref32(x, gamma, beta)
    dz = g * mask.astype(np.float32)
    xhat = (x - mean) * inv
    c1 = dz.mean(0, dtype=np.float32)
    c2 = (dz * xhat).mean(0, dtype=np.float32)
    return (gamma * inv) * (dz - c1 - xhat * c2)


B_BUCKETS = (0, 1, 3, 8)


def _bn_bwd_case(cuda, M, C, seed, add_stride=0, NHW=None, alias=False, seeded=True):
    rng = np.random.default_rng(seed)
    x, _ = _bn_input(rng, M, C, B_BUCKETS)
    gamma, beta = _affine(rng, C)
    _, var64, inv64, scale64, _ = _bn_ref64(x, gamma, beta)
    g = (rng.standard_normal((M, C)) + 0.25).astype(np.float32)
    xd, gd, gmd, btd = _dev(x, cuda), _dev(g, cuda), _dev(gamma, cuda), _dev(beta, cuda)
    (st,), _, _ = _bn_fwd(cuda, [xd], gmd, btd)
    std = _dev(st, cuda)
    # the forward's own ReLU decision: the sign of fma(x, scale, shift) is the sign of the exact x * scale + shift
    mask = (x.astype(np.float64) * st[0].astype(np.float64) + st[1].astype(np.float64)) > 0
    assert M * C < 4096 or 0.2 < mask.mean() < 0.8
    want_dx, want_dg, want_db = _bn_bwd_ref64(x, g, gamma, beta, mask)
    f32_dx = _bn_bwd_ref32(x, g, gamma, beta, mask)
    addend = add_full = None
    if add_stride:
        N, H, W = NHW
        assert N * H * W == M
        Hs, Ws = -(-H // add_stride), -(-W // add_stride)
        # of the size of d_x itself, so that a skipped, doubled or misplaced addend is an error of order 1
        addend = (rng.standard_normal((N, Hs, Ws, C)) * np.abs(scale64)).astype(np.float32)
        add_full = _upsample(addend, add_stride, H, W).reshape(M, C)
        want_dx = want_dx + add_full
        f32_dx = f32_dx + add_full
    seeds = (rng.standard_normal(C).astype(np.float32) * np.abs(want_dg).max(), rng.standard_normal(C).astype(np.float32) * np.abs(want_db).max())
    if not seeded:
        seeds = (np.zeros(C, np.float32), np.zeros(C, np.float32))
    H, W = (NHW[1], NHW[2]) if NHW else (0, 0)
    run = lambda: _bn_bwd_gpu(cuda, [xd], [gd], [std], gmd, seeds, addends=[_dev(addend, cuda)] if add_stride else None,
                              add_stride=max(add_stride, 1), H=H, W=W, alias=alias)
    (dx,), dgam, dbet = run()
    (dx_b,), dgam_b, dbet_b = run()
    assert _same_bits(dx, dx_b) and _same_bits(dgam, dgam_b) and _same_bits(dbet, dbet_b)       # twice: the same bits
    # d_gamma / d_beta: column sums of M terms, the bar of the project's bias sums (test_conv_bwd_gpu.py)
    bar = 2e-5 * np.sqrt(M / 64 + 1)
    got_dg, got_db = dgam.astype(np.float64) - seeds[0], dbet.astype(np.float64) - seeds[1]
    # (a seeded sum also carries the rounding of the final float32 add: half an ulp of the result)
    ulp_g, ulp_b = np.spacing(np.abs(dgam)).max() * seeded, np.spacing(np.abs(dbet)).max() * seeded
    e_dg, e_db = np.abs(got_dg - want_dg).max(), np.abs(got_db - want_db).max()
    colmax = np.abs(want_dx).max(0) + np.finfo(np.float64).tiny
    e_gpu = (np.abs(dx.astype(np.float64) - want_dx) / colmax).max()
    e_f32 = (np.abs(f32_dx.astype(np.float64) - want_dx) / colmax).max()
    print("  MEASURED M=%d C=%d stride=%d: d_x GPU %.2e | float32 restatement %.2e (bar: 4 x); d_gamma %.2e d_beta %.2e of scale (bar %.2e)" % (
        M, C, add_stride, e_gpu, e_f32, e_dg / (np.abs(want_dg).max() + 1e-300), e_db / (np.abs(want_db).max() + 1e-300), bar))
    assert e_dg <= bar * np.abs(want_dg).max() + ulp_g and e_db <= bar * np.abs(want_db).max() + ulp_b
    assert e_gpu <= 4.0 * e_f32, (e_gpu, e_f32)
    assert e_gpu < 2e-4           # orders below the 2e-2 of the whole-step test
    return dx


@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_relu_bwd_against_float64_autograd(cuda, M, C):
    """MEASURED on an MI355X, worst over all shapes and variants of this file: d_x 6.9e-7 of the channel's largest gradient, at
    most 0.84 x the float32 restatement's error at the same shape (bar 4 x; the whole-step test allows 2e-2); d_gamma 1.1e-6 and
    d_beta 2.4e-7 of the largest sum, at most 3.4 % of the bar 2e-5 sqrt(M/64 + 1)."""
    _bn_bwd_case(cuda, M, C, seed=31 * C + M)


@pytest.mark.parametrize("N,H,W,C,stride", [(2, 9, 13, 68, 2), (3, 8, 8, 64, 2), (2, 9, 13, 16, 1), (2, 36, 64, 256, 2), (1, 1, 1, 4, 2),
                                            (2, 5, 7, 132, 3)])
def test_bn_relu_bwd_addend(cuda, N, H, W, C, stride):
    """The identity-shortcut gradient: added everywhere (stride 1) or at the even pixels, from a [ceil(H/s)][ceil(W/s)] tensor."""
    _bn_bwd_case(cuda, N * H * W, C, seed=H * W + C + stride, add_stride=stride, NHW=(N, H, W))


@pytest.mark.parametrize("M,C", [(4608, 256), (65, 68), (1, 4)])
def test_bn_relu_bwd_in_place_and_unseeded(cuda, M, C):
    a = _bn_bwd_case(cuda, M, C, seed=5 * C + M, alias=True)
    b = _bn_bwd_case(cuda, M, C, seed=5 * C + M, alias=False)
    assert _same_bits(a, b)                                             # d_x over g: the same result
    _bn_bwd_case(cuda, M, C, seed=5 * C + M, seeded=False)


@pytest.mark.parametrize("N,H,W,C,stride", [(8, 24, 24, 256, 0), (2, 9, 13, 68, 2), (1, 3, 4, 4, 1)])
def test_bn_relu_bwd_groups_equal_two_calls(cuda, N, H, W, C, stride):
    M = N * H * W
    rng = np.random.default_rng(M + C)
    gamma, beta = _affine(rng, C)
    gmd, btd = _dev(gamma, cuda), _dev(beta, cuda)
    xs = [_dev(_bn_input(rng, M, C, B_BUCKETS)[0], cuda) for _ in range(2)]
    gs = [_dev(rng.standard_normal((M, C)), cuda) for _ in range(2)]
    ads = [_dev(rng.standard_normal((N, -(-H // stride), -(-W // stride), C)), cuda) for _ in range(2)] if stride else None
    stats, _, _ = _bn_fwd(cuda, xs, gmd, btd)
    sd = [_dev(s, cuda) for s in stats]
    seeds = (rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32))
    kw = dict(add_stride=max(stride, 1), H=H, W=W)
    (d1,), dg1, db1 = _bn_bwd_gpu(cuda, xs[:1], gs[:1], sd[:1], gmd, seeds, addends=ads[:1] if ads else None, **kw)
    (d2,), dg2, db2 = _bn_bwd_gpu(cuda, xs[1:], gs[1:], sd[1:], gmd, (dg1, db1), addends=ads[1:] if ads else None, **kw)
    (p1, p2), dgp, dbp = _bn_bwd_gpu(cuda, xs, gs, sd, gmd, seeds, addends=ads, **kw)
    assert _same_bits(p1, d1) and _same_bits(p2, d2) and _same_bits(dgp, dg2) and _same_bits(dbp, db2)


# ---- c. bias gradient -------------------------------------------------------------------------------------------------------
def _bias_grad_gpu(cuda, gs, seed1, seed2):
    from stabnet_amd import train_ops
    M, C = gs[0].shape
    b1 = Guarded(cuda, C, seed1)
    b2 = Guarded(cuda, C, seed2) if seed2 is not None else None
    partial = Guarded(cuda, train_ops.col_reduce_workspace_floats(M, C, len(gs)))
    train_ops.bias_grad(gs, b1.t, b2.t if b2 else None, partial.t)
    _check_all({"d_bias": b1, "d_bias2": b2, "partial": partial})
    # (the second half of each chunk's partial pair belongs to the two-sum modes and is written too)
    assert bool(torch.isfinite(b1.t).all()) and bool(torch.isfinite(partial.t[:partial.n // 2]).all())
    return b1.np(), (b2.np() if b2 else None)


@pytest.mark.parametrize("M,C", SHAPES)
def test_bias_grad_against_float64(cuda, M, C):
    """MEASURED on an MI355X, worst over all shapes: 3.5e-7 of the largest sum, 1.2 % of the bar 2e-5 sqrt(M/64 + 1)."""
    rng = np.random.default_rng(17 * C + M)
    g = [(rng.standard_normal((M, C)) * 2.0 ** rng.integers(-6, 7, C) + 0.1).astype(np.float32) for _ in range(2)]
    gd = [_dev(v, cuda) for v in g]
    want = [v.astype(np.float64).sum(0) for v in g]
    scale = np.abs(want[0]).max()
    zero = np.zeros(C, np.float32)
    s1, s2 = (rng.standard_normal(C) * scale).astype(np.float32), (rng.standard_normal(C) * scale).astype(np.float32)
    inc, inc2 = _bias_grad_gpu(cuda, gd[:1], zero, zero)                 # zero-seeded: the increment itself
    assert _same_bits(inc, inc2)
    e = np.abs(inc.astype(np.float64) - want[0]).max()
    print("  MEASURED M=%d C=%d bias sums: %.2e of scale (bar %.2e)" % (M, C, e / scale, 2e-5 * np.sqrt(M / 64 + 1)))
    assert e <= 2e-5 * scale * np.sqrt(M / 64 + 1)
    # both destinations seeded: each receives that same increment (one float32 add), bit for bit -- and twice the same bits
    for _ in range(2):
        b1, b2 = _bias_grad_gpu(cuda, gd[:1], s1, s2)
        assert _same_bits(b1, s1 + inc) and _same_bits(b2, s2 + inc)
    b1, none = _bias_grad_gpu(cuda, gd[:1], s1, None)                    # no second bias
    assert none is None and _same_bits(b1, s1 + inc)
    # both towers in one launch = tower 1's call, then tower 2's
    t1, u1 = _bias_grad_gpu(cuda, gd[:1], s1, s2)
    t2, u2 = _bias_grad_gpu(cuda, gd[1:], t1, u1)
    p1, p2 = _bias_grad_gpu(cuda, gd, s1, s2)
    assert _same_bits(p1, t2) and _same_bits(p2, u2)
    both = np.abs(p1.astype(np.float64) - s1 - (want[0] + want[1])).max()
    assert both <= 2e-5 * np.abs(want[0] + want[1]).max() * np.sqrt(2 * M / 64 + 1) + np.spacing(np.maximum(np.abs(p1), np.abs(t1))).max()


# ---- d. max-pool forward + argmax + backward --------------------------------------------------------------------------------
def _same_pads(n, k=3, s=2):
    """TF 'SAME': (output size, leading pad)."""
    o = -(-n // s)
    return o, max((o - 1) * s + k - n, 0) // 2


def _pool_ref(x, k, s, pt, pl, Ho, Wo):
    """Literal scan of the window, rows then columns; the first maximum wins (strict >).  -> (y, argmax tap dy*k + dx)."""
    N, H, W, C = x.shape
    xp = np.full((N, (Ho - 1) * s + k, (Wo - 1) * s + k, C), -np.inf, np.float32)
    xp[:, pt:pt + H, pl:pl + W] = x
    m = np.full((N, Ho, Wo, C), -np.inf, np.float32)
    a = np.zeros((N, Ho, Wo, C), np.uint8)
    for dy in range(k):
        for dx in range(k):
            v = xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s]
            better = v > m
            m = np.where(better, v, m)
            a = np.where(better, np.uint8(dy * k + dx), a)
    return m, a


def _pool_bwd_ref(a, dy, H, W, k, s, pt, pl):
    """Literal scatter by argmax: every window's gradient goes to the pixel its argmax names."""
    N, Ho, Wo, C = dy.shape
    dxp = np.zeros((N, (Ho - 1) * s + k, (Wo - 1) * s + k, C), np.float32)
    for ty in range(k):
        for tx in range(k):
            dxp[:, ty:ty + (Ho - 1) * s + 1:s, tx:tx + (Wo - 1) * s + 1:s] += np.where(a == ty * k + tx, dy, np.float32(0))
    assert not dxp[:, :pt].any() and not dxp[:, :, :pl].any() and not dxp[:, pt + H:].any() and not dxp[:, :, pl + W:].any()
    return dxp[:, pt:pt + H, pl:pl + W]


def _pool_gpu(cuda, x, dy, k, s, pt, pl, Ho, Wo):
    from stabnet_amd import train_ops
    N, H, W, C = x.shape
    n_out = N * Ho * Wo * C
    y, am, dx = Guarded(cuda, n_out), Guarded(cuda, n_out, dtype=torch.uint8), Guarded(cuda, x.size)
    xd = _dev(x, cuda)
    train_ops.max_pool_train_fwd(xd, y.t.view(N, Ho, Wo, C), am.t.view(N, Ho, Wo, C), k, s, pt, pl)
    train_ops.max_pool_bwd(am.t.view(N, Ho, Wo, C), _dev(dy, cuda), dx.t.view(N, H, W, C), k, s, pt, pl)
    _check_all({"y": y, "argmax": am, "dx": dx})
    return y.np().reshape(N, Ho, Wo, C), am.np().reshape(N, Ho, Wo, C), dx.np().reshape(N, H, W, C)


@pytest.mark.parametrize("N,H,W,C", [(8, 144, 256, 64), (2, 45, 77, 64), (2, 45, 77, 4), (3, 8, 9, 64), (3, 8, 9, 4), (2, 2, 2, 64),
                                     (1, 2, 2, 4), (2, 144, 256, 4), (1, 1, 1, 4), (2, 3, 1, 4)])
@pytest.mark.parametrize("kind", ["ties", "continuous"])
def test_max_pool_forward_argmax_backward(cuda, N, H, W, C, kind):
    k, s = 3, 2
    (Ho, pt), (Wo, pl) = _same_pads(H), _same_pads(W)
    rng = np.random.default_rng(H * W + C + N)
    if kind == "ties":                        # a few levels, both zeros among them: ties are the rule
        x = np.array([-1.0, -0.0, 0.0, 1.0], np.float32)[rng.integers(0, 4, (N, H, W, C))]
    else:
        x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    dy = rng.integers(-8, 9, (N, Ho, Wo, C)).astype(np.float32)          # integers: every sum of the backward is exact
    want_y, want_a = _pool_ref(x, k, s, pt, pl, Ho, Wo)
    want_dx = _pool_bwd_ref(want_a, dy, H, W, k, s, pt, pl)
    for _ in range(2):                                                      # twice: the same bits
        y, a, dx = _pool_gpu(cuda, x, dy, k, s, pt, pl, Ho, Wo)
        assert _same_bits(y, want_y)                                        # (the sign of a zero included)
        assert np.array_equal(a, want_a), "argmax: %d of %d differ" % (int((a != want_a).sum()), a.size)
        assert _same_bits(dx, want_dx)
        assert dx.astype(np.float64).sum() == dy.astype(np.float64).sum()
    if kind == "continuous":                  # an independent reference: torch float64 max_pool2d on the -inf padded input
        Hp, Wp = (Ho - 1) * s + k, (Wo - 1) * s + k
        xp = torch.full((N, C, Hp, Wp), -float("inf"), dtype=torch.float64)
        xp[:, :, pt:pt + H, pl:pl + W] = torch.from_numpy(x).permute(0, 3, 1, 2).double()
        ty, ti = Fnn.max_pool2d(xp, k, s, return_indices=True)
        iy, ix = (ti // Wp).numpy(), (ti % Wp).numpy()
        oy, ox = np.arange(Ho).reshape(1, 1, Ho, 1), np.arange(Wo).reshape(1, 1, 1, Wo)
        tap = ((iy - oy * s) * k + (ix - ox * s)).transpose(0, 2, 3, 1)
        assert np.array_equal(ty.permute(0, 2, 3, 1).numpy(), y.astype(np.float64)) and np.array_equal(tap, a)


# ---- e. global-pool backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 3])
@pytest.mark.parametrize("HW", [1, 6, 144])
@pytest.mark.parametrize("C", [2048, 257, 50, 1])
def test_gap_bwd_bit_exact(cuda, N, HW, C):
    from stabnet_amd import train_ops
    rng = np.random.default_rng(N * HW + C)
    dg = (rng.standard_normal((N, C)) * 10.0 ** rng.integers(-6, 3, (N, C))).astype(np.float32)
    want = np.broadcast_to((dg / np.float32(HW))[:, None, :], (N, HW, C))
    assert want.dtype == np.float32
    for _ in range(2):
        da = Guarded(cuda, N * HW * C)
        train_ops.gap_bwd(_dev(dg, cuda), da.t.view(N, HW, C))
        _check_all({"da": da})
        assert _same_bits(da.np().reshape(N, HW, C), want)


# ---- f. FC backward ---------------------------------------------------------------------------------------------------------
def _fc_inputs(rng, M, K, Nout, relu):
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
    dy = rng.standard_normal((M, Nout)).astype(np.float32)
    y = None
    if relu:                                   # the mask is y > 0: exact zeros of both signs and negative entries are planted
        y = rng.standard_normal((M, Nout)).astype(np.float32)
        u = rng.random((M, Nout))
        y[u < 0.15] = 0.0
        y[u < 0.08] = -0.0
        y[(u >= 0.15) & (u < 0.25)] = -np.abs(y[(u >= 0.15) & (u < 0.25)]) - np.float32(1e-30)
        if y.size >= 4:                        # whatever the draw: one of each kind (a one-element y cannot hold them all; its
            y.reshape(-1)[-4:] = [1.0, -1.0, -0.0, 0.0]     # four values are the cases of test_fc_bwd_mask_is_strictly_positive)
    return x, w, y, dy


def _fc_gpu(cuda, x, w, y, dy, seed_w, seed_b, want_dx=True, scratch_delta=0, scratch_init=None):
    from stabnet_amd import train_ops
    M, K = x.shape
    Nout = w.shape[0]
    dW, db = Guarded(cuda, Nout * K, seed_w), Guarded(cuda, Nout, seed_b)
    dx = Guarded(cuda, M * K) if want_dx else None
    scratch = Guarded(cuda, train_ops.fc_bwd_scratch_floats(M, K, Nout) + scratch_delta, scratch_init)
    yd = _dev(y, cuda) if y is not None else None
    train_ops.fc_bwd(_dev(x, cuda), _dev(w, cuda).view(Nout, K), yd, _dev(dy, cuda), dW.t, db.t, dx.t if dx else None, scratch.t)
    _check_all({"dW": dW, "db": db, "dx": dx, "scratch": scratch})
    return dW, db, dx, scratch


HEAD = [(16, 2048, 2048, 1), (16, 2048, 1024, 1), (16, 1024, 512, 1), (8, 512, 50, 0)]
RAGGED = [(M, K, Nout, relu) for M, K, Nout, relu in [
    (1, 4, 1, 1), (3, 68, 50, 1), (17, 1028, 257, 1), (33, 68, 300, 1), (17, 4, 300, 0), (33, 1028, 50, 1), (1, 1028, 257, 0),
    (3, 1028, 300, 1), (33, 4, 1, 1), (17, 68, 257, 0), (3, 4, 257, 1), (1, 68, 300, 1), (16, 2048, 300, 1), (9, 1028, 1, 0)]]


@pytest.mark.parametrize("M,K,Nout,relu", HEAD + RAGGED)
def test_fc_bwd_against_float64(cuda, M, K, Nout, relu):
    """MEASURED on an MI355X, worst over all cases, error relative to the largest element of the increment (GPU | its ratio to
    the float32 NumPy error of the same case; bar 4 x): dW 2.5e-7 | 1.60, db 2.2e-7 | 1.00, dx 2.0e-7 | 2.56."""
    rng = np.random.default_rng(M * 7 + K + Nout)
    x, w, y, dy = _fc_inputs(rng, M, K, Nout, relu)
    dyr64 = dy.astype(np.float64) * ((y > 0) if relu else 1.0)
    dyr32 = (dy * (y > 0)).astype(np.float32) if relu else dy
    if relu and y.size >= 4:
        assert (y == 0).any() and np.signbit(y[y == 0]).any() and (~np.signbit(y[y == 0])).any() and (y < 0).any() and (y > 0).any()
    inc64 = {"dW": dyr64.T @ x.astype(np.float64), "db": dyr64.sum(0), "dx": dyr64 @ w.astype(np.float64)}
    seed_w = (rng.standard_normal((Nout, K)) * np.abs(inc64["dW"]).max()).astype(np.float32)
    seed_b = (rng.standard_normal(Nout) * np.abs(inc64["db"]).max()).astype(np.float32)
    want = {"dW": seed_w + inc64["dW"], "db": seed_b + inc64["db"], "dx": inc64["dx"]}
    f32 = {"dW": seed_w + dyr32.T @ x, "db": seed_b + dyr32.sum(0, dtype=np.float32), "dx": dyr32 @ w}
    got = None
    for _ in range(2):                                                     # twice: the same bits
        dW, db, dx, scratch = _fc_gpu(cuda, x, w, y, dy, seed_w, seed_b)
        assert bool(torch.isfinite(scratch.t).all()), "scratch words the size query counts were never written"
        now = {"dW": dW.np().reshape(Nout, K), "db": db.np(), "dx": dx.np().reshape(M, K)}
        assert got is None or all(_same_bits(now[n], got[n]) for n in now)
        got = now
    for name in ("dW", "db", "dx"):
        assert f32[name].dtype == np.float32 and np.isfinite(got[name]).all()
        scale = np.abs(inc64[name]).max() + np.finfo(np.float64).tiny
        e_gpu = np.abs(got[name].astype(np.float64) - want[name]).max() / scale
        e_f32 = np.abs(f32[name].astype(np.float64) - want[name]).max() / scale
        print("  MEASURED M=%d K=%d Nout=%d %s: GPU %.2e | float32 NumPy %.2e (bar: 4 x)" % (M, K, Nout, name, e_gpu, e_f32))
        assert e_gpu <= 4.0 * e_f32, (name, e_gpu, e_f32)
    # dx not wanted: dW / db as before, the scratch is not touched
    dW2, db2, _, scratch2 = _fc_gpu(cuda, x, w, y, dy, seed_w, seed_b, want_dx=False, scratch_init="canary")
    assert _same_bits(dW2.np().reshape(Nout, K), got["dW"]) and _same_bits(db2.np(), got["db"]) and scratch2.untouched()


def test_fc_bwd_mask_is_strictly_positive(cuda):
    """One sample, one output: y = +0, -0, a small negative, a small positive number: only the positive ones pass the gradient."""
    for yv, passes in ((0.0, False), (-0.0, False), (-2e-38, False), (2e-38, True), (2.0, True)):
        x = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
        w = np.array([[0.5, -1.0, 2.0, 4.0]], np.float32)
        dW, db, dx, _ = _fc_gpu(cuda, x, w, np.array([[yv]], np.float32), np.array([[3.0]], np.float32), np.zeros(4, np.float32),
                                np.zeros(1, np.float32))
        k = 3.0 if passes else 0.0
        assert np.array_equal(dW.np(), k * x[0]) and np.array_equal(db.np(), [k]) and np.array_equal(dx.np(), k * w[0]), yv


def test_fc_bwd_refuses_a_short_scratch_before_launching(cuda):
    from stabnet_amd import _lib
    rng = np.random.default_rng(3)
    M, K, Nout = 16, 1024, 512
    x, w, y, dy = _fc_inputs(rng, M, K, Nout, 1)
    seed_w, seed_b = rng.standard_normal((Nout, K)).astype(np.float32), rng.standard_normal(Nout).astype(np.float32)
    with pytest.raises(_lib.StabnetError, match="scratch"):
        _fc_gpu(cuda, x, w, y, dy, seed_w, seed_b, scratch_delta=-1)
    # the same call through the raw ABI, to look at the buffers afterwards
    from stabnet_amd import train_ops
    from stabnet_amd._tensor import stream_ptr
    need = train_ops.fc_bwd_scratch_floats(M, K, Nout)
    dW, db, dx, scratch = Guarded(cuda, Nout * K, seed_w), Guarded(cuda, Nout, seed_b), Guarded(cuda, M * K, "canary"), Guarded(cuda, need - 1, "canary")
    t = [_dev(v, cuda) for v in (x, w, y, dy)]
    rc = _lib.lib().stabnet_fc_bwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), M, K, Nout, 1, dW.t.data_ptr(),
                                   db.t.data_ptr(), dx.t.data_ptr(), scratch.t.data_ptr(), need - 1, stream_ptr(cuda))
    torch.cuda.synchronize()
    assert rc == -1 and b"scratch" in _lib.lib().stabnet_last_error()
    assert _same_bits(dW.np(), seed_w.reshape(-1)) and _same_bits(db.np(), seed_b) and dx.untouched() and scratch.untouched()


# ---- h. argument errors (nothing is launched) -------------------------------------------------------------------------------
def test_argument_errors(cuda):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    L = _lib.lib()
    st = stream_ptr(cuda)
    buf = Guarded(cuda, 1 << 16, "canary")
    d = buf.t.data_ptr()
    host = np.zeros(1 << 12, np.float32)
    h = host.ctypes.data

    def refused(rc, word):
        msg = L.stabnet_last_error()
        assert rc == -1 and msg and word.encode() in msg, (rc, msg)

    # C % 4 != 0
    refused(L.stabnet_bn_stats_train(1, d, 0, 8, 6, d, d, EPS, DECAY, d, 0, 0, 0, d, st), "C % 4")
    refused(L.stabnet_bn_relu_bwd(1, d, 0, d, 0, d, 0, d, 8, 6, 0, 0, 1, 0, 0, d, d, d, 0, d, d, 0, st), "C % 4")
    refused(L.stabnet_bias_grad(1, d, 0, 8, 6, d, 0, d, st), "C % 4")
    refused(L.stabnet_max_pool_train_fwd(d, d, d, 1, 4, 4, 6, 2, 2, 3, 2, 0, 0, st), "C % 4")
    refused(L.stabnet_max_pool_bwd(d, d, d, 1, 4, 4, 6, 2, 2, 3, 2, 0, 0, st), "C % 4")
    # groups = 3
    refused(L.stabnet_bn_stats_train(3, d, d, 8, 8, d, d, EPS, DECAY, d, d, 0, 0, d, st), "groups")
    refused(L.stabnet_bn_relu_bwd(3, d, d, d, d, d, d, d, 8, 8, 0, 0, 1, 0, 0, d, d, d, d, d, d, d, st), "groups")
    refused(L.stabnet_bias_grad(3, d, d, 8, 8, d, 0, d, st), "groups")
    assert L.stabnet_col_reduce_workspace_floats(8, 8, 3) == 0 and L.stabnet_col_reduce_workspace_floats(8, 8, 2) > 0
    # K % 4 != 0
    refused(L.stabnet_fc_bwd(d, d, 0, d, 2, 6, 3, 0, d, d, 0, 0, 0, st), "K % 4")
    # null pointers (the second group's when groups = 2, a lone moving average, a missing y under relu)
    refused(L.stabnet_bn_stats_train(1, 0, 0, 8, 8, d, d, EPS, DECAY, d, 0, 0, 0, d, st), "null")
    refused(L.stabnet_bn_stats_train(2, d, 0, 8, 8, d, d, EPS, DECAY, d, d, 0, 0, d, st), "null")
    refused(L.stabnet_bn_stats_train(1, d, 0, 8, 8, d, d, EPS, DECAY, d, 0, d, 0, d, st), "both or neither")
    refused(L.stabnet_bn_relu_bwd(1, d, 0, d, 0, d, 0, d, 8, 8, 0, 0, 1, 0, 0, d, d, d, 0, d, 0, 0, st), "null")
    refused(L.stabnet_bn_relu_bwd(2, d, d, d, d, d, d, d, 8, 8, 0, 0, 1, 0, 0, d, d, d, 0, d, d, d, st), "null")
    refused(L.stabnet_bn_relu_bwd(1, d, 0, d, 0, d, 0, d, 8, 8, d, 0, 2, 3, 3, d, d, d, 0, d, d, 0, st), "strided addend")
    refused(L.stabnet_bias_grad(1, 0, 0, 8, 8, d, 0, d, st), "null")
    refused(L.stabnet_max_pool_train_fwd(d, d, 0, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, st), "null")
    refused(L.stabnet_max_pool_bwd(0, d, d, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, st), "null")
    refused(L.stabnet_max_pool_train_fwd(d, d, d, 1, 4, 4, 8, 9, 2, 3, 2, 0, 0, st), "geometry")
    refused(L.stabnet_gap_bwd(d, 2, 4, 8, 0, st), "null")
    refused(L.stabnet_gap_bwd(d, 2, 0, 8, d, st), "HW")
    refused(L.stabnet_fc_bwd(d, d, 0, d, 2, 8, 3, 1, d, d, 0, 0, 0, st), "relu")
    refused(L.stabnet_fc_bwd(d, 0, 0, d, 2, 8, 3, 0, d, d, 0, 0, 0, st), "null")
    refused(L.stabnet_fc_bwd(d, d, 0, d, 2, 8, 3, 0, d, d, d, 0, 0, st), "scratch")
    # host pointers
    refused(L.stabnet_bn_stats_train(1, h, 0, 8, 8, d, d, EPS, DECAY, d, 0, 0, 0, d, st), "bn_stats_train")
    refused(L.stabnet_bn_relu_bwd(1, d, 0, d, 0, d, 0, d, 8, 8, 0, 0, 1, 0, 0, d, d, h, 0, d, d, 0, st), "bn_relu_bwd")
    refused(L.stabnet_bias_grad(1, d, 0, 8, 8, h, 0, d, st), "bias_grad")
    refused(L.stabnet_max_pool_train_fwd(h, d, d, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, st), "max_pool_train_fwd")
    refused(L.stabnet_max_pool_bwd(d, d, h, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, st), "max_pool_bwd")
    refused(L.stabnet_gap_bwd(h, 2, 4, 8, d, st), "gap_bwd")
    refused(L.stabnet_fc_bwd(d, h, 0, d, 2, 8, 3, 0, d, d, 0, 0, 0, st), "fc_bwd")
    torch.cuda.synchronize()
    assert buf.untouched() and not host.any()                             # none of the refused calls launched anything


# ---- i. L2 regulariser (stabnet_weight_decay) -------------------------------------------------------------------------------
WD_N = 4096                                                # floats of the flat parameter / gradient buffer
WD_LENS = (1, 2, 3, 4, 5, 7, 8, 9)
WD_COEFS = (1e-4, 2e-4, 0.0)                               # slim conv weights, fc_weights / fc_bias, and a segment that is switched off


def _wd_table(k):
    """Segment table k: a 1 027-float segment whose offset & 3 == k, then lengths 1..9 at every offset & 3.  Placed greedily, so a
    segment whose wanted alignment is the cursor's is ADJACENT to its predecessor and every other one leaves a gap of 1..3 floats
    (and 5 floats lead the table) that no call may touch.  -> offsets, lengths (int64), coefficients (float32)."""
    items = [(k, 1027)] + [(a, n) for n in WD_LENS for a in (0, 1, 2, 3)]
    off, cur = [], 5
    for a, n in items:
        o = cur + ((a - cur) & 3)
        off.append(o)
        cur = o + n
    assert cur <= WD_N
    lens = np.array([n for _, n in items], np.int64)
    coef = np.array([WD_COEFS[i % 3] for i in range(len(items))], np.float32)
    return np.array(off, np.int64), lens, coef


def _wd_model(params, off, lens, coef, loss0):
    """The kernels' own summation tree, op for op (weight_decay_kernel + weight_decay_finalize_kernel, grid (64, nseg) x 256):
    thread t of a segment squares its head / tail element and its float4s ((x2 + y2) + (z2 + w2), stride 64 * 256), the 64 lanes
    of a wave add in an xor butterfly 32..1, the four waves as (0 + 1) + (2 + 3), the block partial is (0.5 * coef) * that -- all
    float32; the finalize sums the 64 * nseg partials in double (thread i takes i, i + 1024, ..; butterfly; 16 waves in order)
    and adds the float32 rounding of that onto *loss_out.  -> the float32 value the call must leave in *loss_out, and the block
    partials [nseg, 64] it must leave in the workspace."""
    f = np.float32
    lane = np.arange(64)
    parts = np.zeros((len(off), 64), f)
    for g, (o, n, c) in enumerate(zip(off, lens, coef)):
        head = min(int(n), (4 - (int(o) & 3)) & 3)
        body, tail = (int(n) - head) >> 2, (int(n) - head) & 3
        s = np.zeros(64 * 256, f)
        t = np.arange(head + tail)
        w = params[o + np.where(t < head, t, head + 4 * body + (t - head))]
        s[:head + tail] = w * w
        for start in range(0, body, 64 * 256):
            m = min(64 * 256, body - start)
            w4 = params[o + head + 4 * start:o + head + 4 * (start + m)].reshape(m, 4)
            q = w4 * w4
            s[:m] = s[:m] + ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))
        s = s.reshape(64, 4, 64)
        for x in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ x]
        red = s[:, :, 0]
        parts[g] = (f(0.5) * f(c)) * ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]))
    flat = parts.reshape(-1).astype(np.float64)
    d = np.zeros(1024 * ((flat.size + 1023) // 1024))
    d[:flat.size] = flat
    acc = np.zeros(1024)
    for row in d.reshape(-1, 1024):                         # thread i: partial[i], then partial[i + 1024], ...
        acc = acc + row
    acc = acc.reshape(16, 64)
    for x in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ x]
    tot = acc[0, 0]
    for wv in range(1, 16):
        tot = tot + acc[wv, 0]
    return f(f(loss0) + f(tot)), parts


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_weight_decay_matches_float64(cuda, k):
    """stabnet_weight_decay through its own entry point: every offset & 3 crossed with lengths 1, 2, 3, 4, 5, 7, 8, 9 and 1 027
    (scalar head, float4 body, scalar tail; segments shorter than their head; adjacent segments; gaps), coefficients 1e-4 / 2e-4 /
    0, with and without a gradient, with and without the value, gscale 0 (the theta-only step) and 2 * regu_mul.

    Gradient: grads + gscale * coef * w formed in float64 and rounded once, within 1 ulp.  (The kernel rounds gscale * coef, its
    product with w and the sum: the first two are 2^-23 of a term that is <= 2.4e-6 * 2 / 0.1 of the gradient it is added to --
    the gradients here are 0.1 <= |g| < 2 so that the sum does not cancel -- so the result is the correctly rounded one or its
    neighbour.)

    Value: *loss_out starts at L0 != 0 and must end at L0 + S, S = sum coef * 0.5 * sum w^2 in float64.  Bound from the summation
    tree (see _wd_model): no segment has more than 256 float4s, so a thread adds at most ONE float4 to at most one head / tail
    square: 1 rounding for a square, 2 for the float4's tree, 1 for the thread's add, 6 butterfly levels, 2 for the waves, 1 for
    the product with 0.5 * coef (0.5 * coef itself is exact) = 13 roundings on any path, all terms >= 0, so every block partial is
    within (1 + u)^13 - 1 of exact, u = 2^-24; the double sum of 64 * nseg partials adds < 2^-40; its float32 rounding u; the
    final float32 add u * (L0 + S) / S.  With L0 = S / 4 (rounded): (13 + 1 + 1.25) u = 9.1e-7 of S < the 1e-6 of S asserted.
    Beyond that bound the value AND the 64 * nseg float32 block partials in the workspace must equal the model of that tree BIT FOR
    BIT: an element that moves to another thread (a wrong head length whose float4 accesses stay inside the segment) changes no
    gradient and moves the value by roundings only -- the double sum hides them in the final float32, the partials show them."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    from stabnet_amd.config import Config
    L, st = _lib.lib(), stream_ptr(cuda)
    rng = np.random.default_rng(100 + k)
    off, lens, coef = _wd_table(k)
    nseg = len(off)
    ends = off + lens
    assert (off[1:] >= ends[:-1]).all() and (off[1:] == ends[:-1]).any() and (off[1:] > ends[:-1]).any()   # disjoint; adjacent ones; gaps
    assert {(int(o) & 3, int(n)) for o, n in zip(off, lens)} >= {(a, n) for a in range(4) for n in WD_LENS} | {(k, 1027)}
    assert any(n < ((4 - (o & 3)) & 3) for o, n in zip(off, lens))                                         # shorter than its head
    inside = np.zeros(WD_N, bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    w = rng.standard_normal(WD_N).astype(np.float32)
    g0 = (rng.uniform(0.1, 2.0, WD_N) * rng.choice([-1.0, 1.0], WD_N)).astype(np.float32)
    S = float(sum(np.float64(c) * 0.5 * (w[o:o + n].astype(np.float64) ** 2).sum() for o, n, c in zip(off, lens, coef)))
    L0 = np.float32(0.25 * S)
    u = 2.0 ** -24
    bound = (((1 + u) ** 13 - 1) + 2.0 ** -40 + u) * S + u * (float(L0) + S)
    assert S > 0 and bound < 1e-6 * S, (S, bound)                                                         # (input condition)
    d_off, d_len = torch.from_numpy(off).to(cuda), torch.from_numpy(lens).to(cuda)
    d_coef = torch.from_numpy(coef).to(cuda)
    gs_live = 2.0 * Config().regu_mul                       # (the entry point takes it as a float: the reference below rounds it too)

    def run(gscale, with_grads, with_loss):
        P, G = Guarded(cuda, WD_N, w), Guarded(cuda, WD_N, g0)
        loss, part = Guarded(cuda, 1, np.array([L0], np.float32)), Guarded(cuda, 64 * nseg)
        rc = L.stabnet_weight_decay(P.t.data_ptr(), G.t.data_ptr() if with_grads else 0, d_off.data_ptr(), d_len.data_ptr(),
                                    d_coef.data_ptr(), nseg, gscale, loss.t.data_ptr() if with_loss else 0,
                                    part.t.data_ptr() if with_loss else 0, st)
        assert rc == 0, L.stabnet_last_error()
        _check_all({"params": P, "grads": G, "loss_out": loss, "partials": part})
        assert _same_bits(P.np(), w)
        if not with_loss:
            assert _same_bits(loss.np(), [L0]) and bool(torch.isnan(part.t).all())
        return G.np(), float(loss.np()[0]), part.np()

    for gscale in (gs_live, 0.0):
        g, val, parts = run(gscale, True, True)
        g_again, val_again, parts_again = run(gscale, True, True)
        assert _same_bits(g, g_again) and val == val_again and _same_bits(parts, parts_again)                      # two calls, equal bits
        assert _same_bits(g[~inside], g0[~inside]), "a gap between segments was written"
        want = g0.astype(np.float64)
        for o, n, c in zip(off, lens, coef):
            want[o:o + n] += float(np.float32(gscale)) * np.float64(c) * w[o:o + n].astype(np.float64)
        want32 = want.astype(np.float32)
        if gscale == 0.0:
            assert _same_bits(g, g0), "gscale 0 (theta-only step) changed gradient bits"
        else:
            assert (np.abs(g.astype(np.float64) - want32) <= np.spacing(np.abs(want32))).all()
            on = np.zeros(WD_N, bool)
            for o, n, c in zip(off, lens, coef):
                on[o:o + n] = c != 0
            assert not _same_bits(g[on], g0[on]) and _same_bits(g[inside & ~on], g0[inside & ~on])   # coef 0: untouched values
        print("weight_decay table %d gscale %g: value %.9g float64 %.9g rel err %.2e (bound %.2e)"
              % (k, gscale, val, float(L0) + S, abs(val - (float(L0) + S)) / S, bound / S))
        assert abs(val - (float(L0) + S)) <= 1e-6 * S
        model_val, model_parts = _wd_model(w, off, lens, coef, L0)
        assert np.float32(val) == model_val, "value differs from the kernels' own summation order"
        assert _same_bits(parts, model_parts.reshape(-1)), "block partials differ from the kernel's thread <-> element map"
    # grads = NULL: the value alone, the same bits; loss_out = NULL: the gradient alone, the same bits
    _, val_only, _ = run(gs_live, False, True)
    assert val_only == val
    g_only, _, _ = run(gs_live, True, False)
    g_live, _, _ = run(gs_live, True, True)
    assert _same_bits(g_only, g_live)


def test_weight_decay_argument_errors(cuda):
    """The refusals of stabnet_weight_decay (and of stabnet_axpb / stabnet_interleave2) return before any launch."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    L, st = _lib.lib(), stream_ptr(cuda)
    buf = Guarded(cuda, 1 << 12, "canary")
    d = buf.t.data_ptr()
    off, lens, coef = _wd_table(0)
    d_off, d_len, d_coef = torch.from_numpy(off).to(cuda), torch.from_numpy(lens).to(cuda), torch.from_numpy(coef).to(cuda)
    so, sl, sc = d_off.data_ptr(), d_len.data_ptr(), d_coef.data_ptr()

    def refused(rc, word):
        msg = L.stabnet_last_error()
        assert rc == -1 and msg and word.encode() in msg, (rc, msg)

    refused(L.stabnet_weight_decay(0, d, so, sl, sc, len(off), 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, 0, sl, sc, len(off), 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, so, 0, sc, len(off), 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, so, sl, 0, len(off), 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, so, sl, sc, 0, 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, so, sl, sc, 65536, 1.0, d, d, st), "bad arguments")
    refused(L.stabnet_weight_decay(d, d, so, sl, sc, len(off), 1.0, d, 0, st), "workspace")
    refused(L.stabnet_axpb(0, 1.0, 0.0, 4, d, st), "axpb")
    refused(L.stabnet_axpb(d, 1.0, 0.0, 0, d, st), "axpb")
    refused(L.stabnet_interleave2(d, 0, 4, d, st), "interleave2")
    refused(L.stabnet_interleave2(d, d, 0, d, st), "interleave2")
    torch.cuda.synchronize()
    assert buf.untouched()


# ---- j. the host mirror's elementwise helpers -------------------------------------------------------------------------------
ELEMWISE_N = (1, 255, 256, 257, 1027)                      # one thread; one block less / exactly / plus one; five blocks, ragged


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_axpb_bit_exact(cuda, n):
    """stabnet_axpb: y = a * x + b, two roundings (no contraction), bit for bit against NumPy float32."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    L, st = _lib.lib(), stream_ptr(cuda)
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    for a, b in ((-1.0, 1.0), (0.3, -0.7), (0.0, 2.5)):      # (-1, 1) is the step's 1 - black_pix
        X, Y = Guarded(cuda, n, x), Guarded(cuda, n)
        assert L.stabnet_axpb(X.t.data_ptr(), a, b, n, Y.t.data_ptr(), st) == 0, L.stabnet_last_error()
        _check_all({"x": X, "y": Y})
        assert _same_bits(Y.np(), np.float32(a) * x + np.float32(b)) and _same_bits(X.np(), x)


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_interleave2_bit_exact(cuda, n):
    """stabnet_interleave2: out [n][2] = (a, b), written as float2 -- also into a view that starts 8 bytes into its allocation
    (float2's natural alignment, not 16 bytes)."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    L, st = _lib.lib(), stream_ptr(cuda)
    rng = np.random.default_rng(1000 + n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    want = np.stack([a, b], axis=1).reshape(-1)
    for shift in (0, 2):                                     # floats: the inner buffer starts 16-byte aligned
        A, B, O = Guarded(cuda, n, a), Guarded(cuda, n, b), Guarded(cuda, 2 * n + 4)
        out = O.t[shift:shift + 2 * n]
        assert O.t.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 * shift
        assert L.stabnet_interleave2(A.t.data_ptr(), B.t.data_ptr(), n, out.data_ptr(), st) == 0, L.stabnet_last_error()
        _check_all({"a": A, "b": B, "out": O})
        got = O.np()
        assert _same_bits(got[shift:shift + 2 * n], want)
        assert np.isnan(got[:shift]).all() and np.isnan(got[shift + 2 * n:]).all(), "write outside the [n][2] view"
        assert _same_bits(A.np(), a) and _same_bits(B.np(), b)
