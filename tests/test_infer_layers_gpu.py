"""GPU: the non-convolution inference layers (csrc/layers.hip) and the shortened head (csrc/head.hip), one operator at a time
against float64 on the CPU.

pad_channels, stem_repack, merge_vectors, bn_fold, max_pool (+ fused BN + ReLU), gap_bn_relu, fc, the head's gap + fc_1 and its
output layer + mesh are otherwise reached only through whole forward passes at batch 1 or 2.  Here each runs through its own C
entry point (the launcher the plan calls) at the shapes where its code takes another path: every chunk count of the two
poolings, the three FC kernels and their 128 KiB boundary, every rows-per-wave count of the output layer, unbalanced grids.
Every output and scratch buffer sits between canary bands and is pre-filled with NaN, inputs are compared with their values
after the call, every arithmetic case runs twice for equal bits.  References are float64 NumPy or the oracle; the bounds are
derived from the kernels' summation chains in units of u = 2^-24 (the figures measured when the test was written are in the
docstrings marked MEASURED)."""
import numpy as np
import pytest
import torch

from _guarded import Guarded, _check_all, _same_bits
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS32 = float(np.float32(1e-5))                            # slim resnet_arg_scope batch_norm_epsilon as the kernel receives it


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
class Bufs:
    """The buffers of one call: inputs (values, checked unchanged afterwards), outputs and scratch (NaN), all between canaries."""

    def __init__(self, cuda):
        self.cuda, self.ins, self.outs = cuda, {}, {}

    def inp(self, name, a):
        a = np.ascontiguousarray(a)
        g = Guarded(self.cuda, a.size, a)
        self.ins[name] = (g, a.copy())
        return g.t.view(a.shape)

    def out(self, name, n):
        g = Guarded(self.cuda, n)
        self.outs[name] = g
        return g.t

    def done(self):
        named = dict(self.outs)
        named.update({k: g for k, (g, _) in self.ins.items()})
        _check_all(named)
        for name, (g, a) in self.ins.items():
            assert np.array_equal(g.np().view(np.uint32), a.reshape(-1).view(np.uint32)), "input %s was written" % name

    def get(self, name, shape=None):
        a = self.outs[name].np()
        return a if shape is None else a.reshape(shape)


def _twice(run):
    """run() -> tuple of arrays; twice, equal bits; -> the first."""
    a, b = run(), run()
    assert all(_same_bits(x, y) for x, y in zip(a, b)), "the same call gave other bits"
    return a


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- exact operators --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 255, 257])
@pytest.mark.parametrize("C,Cp", [(13, 16), (1, 4), (5, 8), (16, 16)])
def test_pad_channels_bit_exact(cuda, C, Cp, npix):
    from stabnet_amd import ops
    rng = np.random.default_rng(C * 1000 + npix)
    x = _f32(rng.standard_normal((npix, C)))
    want = np.zeros((npix, Cp), np.float32)
    want[:, :C] = x
    B = Bufs(cuda)
    ops.pad_channels(B.inp("x", x), B.out("y", npix * Cp).view(npix, Cp))
    B.done()
    assert _same_bits(B.get("y", (npix, Cp)), want)


@pytest.mark.parametrize("Cin,CinPad", [(13, 16), (5, 8)])
@pytest.mark.parametrize("k", [7, 3])
@pytest.mark.parametrize("Cout", [64, 3])
def test_stem_repack_bit_exact(cuda, Cout, k, Cin, CinPad):
    from stabnet_amd import ops
    rng = np.random.default_rng(Cout + k + Cin)
    w = _f32(rng.standard_normal((Cout, k, k, CinPad)))                 # (pad channels non-zero: they must not be copied)
    Rp = (k * Cin + 31) // 32 * 32
    want = np.zeros((Cout, k, Rp), np.float32)
    want[:, :, :k * Cin] = w[..., :Cin].reshape(Cout, k, k * Cin)
    B = Bufs(cuda)
    ops.stem_repack(B.inp("w", w), B.out("out", want.size), Cin)
    B.done()
    assert _same_bits(B.get("out", want.shape), want)


@pytest.mark.parametrize("depth,dbn", [(256, 64), (1, 1), (255, 257), (2048, 512)])
def test_merge_vectors_bit_exact(cuda, depth, dbn):
    from stabnet_amd import ops
    rng = np.random.default_rng(depth + dbn)
    b_sc, s1, h1 = (_f32(rng.standard_normal(n)) for n in (depth, dbn, dbn))
    want = np.stack([np.concatenate([b_sc, np.zeros(dbn, np.float32)]), np.concatenate([np.ones(depth, np.float32), s1]),
                     np.concatenate([np.zeros(depth, np.float32), h1]),
                     np.concatenate([np.full(depth, -np.inf, np.float32), np.zeros(dbn, np.float32)])])
    B = Bufs(cuda)
    ops.merge_vectors(B.inp("b_sc", b_sc), B.inp("scale1", s1), B.inp("shift1", h1), B.out("out", want.size))
    B.done()
    assert _same_bits(B.get("out", want.shape), want)                   # (the -inf floors and the sign of the zeros included)


# ---- bn_fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 255, 256, 257, 4100])
def test_bn_fold_against_float64(cuda, G):
    """scale within 4u of the float64 value (the add, sqrt, divide and multiply, each correctly rounded); shift within
    u (|beta| + 2 |mean scale|) + |mean| 4u |scale|.
    MEASURED on an MI355X, worst over the five sizes: scale 2.43u relative (bound 4u), shift 0.92 of its bound.  Both are the
    figures of a float32 NumPy restatement at the same inputs (1.97u / 0.92 at G = 255 ... 2.43u / 0.90 at G = 4100): every operation
    of the kernel is correctly rounded.  The 0.92 is a channel with shift = -0.51615 from beta = -0.51588: the closing subtraction
    rounds by half an ulp of a result just above 0.5, which is u |beta| nearly in full; the bound is tight there by construction."""
    from stabnet_amd import ops
    rng = np.random.default_rng(G)
    var = _f32(10.0 ** rng.uniform(-6, 3, G))
    gamma = _f32(rng.uniform(0.25, 2.0, G) * rng.choice([-1.0, 1.0], G))
    beta, mean = _f32(rng.standard_normal(G)), _f32(rng.standard_normal(G) * 10.0 ** rng.uniform(-2, 2, G))
    var[0], gamma[-1] = 1e-6, -gamma[-1]
    scale64 = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + EPS32)
    shift64 = beta.astype(np.float64) - mean.astype(np.float64) * scale64

    def run():
        B = Bufs(cuda)
        ops.bn_fold(B.inp("gamma", gamma), B.inp("beta", beta), B.inp("mean", mean), B.inp("var", var), 1e-5, B.out("scale", G),
                    B.out("shift", G))
        B.done()
        return B.get("scale"), B.get("shift")
    scale, shift = _twice(run)
    e_scale = np.abs(scale / scale64 - 1.0)
    bar_shift = U * (np.abs(beta) + 2 * np.abs(mean * scale64)) + np.abs(mean) * 4 * U * np.abs(scale64)
    e_shift = np.abs(shift - shift64)
    print("  MEASURED G=%d: scale %.2fu relative (bound 4u); shift %.2f of its bound" % (G, e_scale.max() / U, (e_shift / bar_shift).max()))
    assert (e_scale <= 4 * U).all(), "scale: %.3fu" % (e_scale.max() / U)
    assert (e_shift <= bar_shift).all(), float((e_shift / bar_shift).max())


# ---- max_pool ---------------------------------------------------------------------------------------------------------------
def _same_pads(n, k=3, s=2):
    o = -(-n // s)
    return o, max((o - 1) * s + k - n, 0) // 2


# workgroups (256 channel quads each): 1, 1, 1, 6, 57 (= 1 mod 8), 1, 8 (= 0), 15 (= 7), 9 (= 1)
POOL_SHAPES = [(1, 1, 1, 4), (1, 2, 2, 4), (2, 9, 7, 8), (1, 16, 24, 64), (1, 45, 77, 64), (3, 8, 8, 4), (1, 16, 32, 64),
               (1, 30, 32, 64), (1, 18, 32, 64)]


def test_pool_shapes_cover_the_unbalanced_grids():
    wgs = [-(-(N * _same_pads(H)[0] * _same_pads(W)[0] * (C // 4)) // 256) for N, H, W, C in POOL_SHAPES]
    assert any(w < 8 for w in wgs) and {0, 1, 7} <= {w % 8 for w in wgs if w >= 8}, wgs


@pytest.mark.parametrize("kind", ["normal", "negative", "ties"])
@pytest.mark.parametrize("N,H,W,C", POOL_SHAPES)
def test_max_pool_against_oracle(cuda, N, H, W, C, kind):
    """Without scale / shift: the bits of the oracle's -inf padded pool (an all-negative input separates it from a zero pad).  With:
    relu(m scale + shift) within one fma rounding, u |want| + 2^-52 (|m scale| + |shift|), and the same sign decisions.
    MEASURED on an MI355X, worst over all cases: 1.00 of the bound, which a correctly rounded fma reaches by construction: half
    an ulp of a result just above a power of two is u |want|.  Before the kernel kept the later tap at ties (fmaxf: +0 beats -0
    wherever it stands) the ties input differed from the oracle in the sign of 402 of 9216 zeros at (1, 16, 24, 64), and in 7 of
    the 9 shapes."""
    from stabnet_amd import ops
    rng = np.random.default_rng(H * W + C + N)
    if kind == "ties":
        x = np.array([-1.0, -0.0, 0.0, 1.0], np.float32)[rng.integers(0, 4, (N, H, W, C))]
    else:
        x = _f32(rng.standard_normal((N, H, W, C)))
        if kind == "negative":
            x = -np.abs(x) - np.float32(0.01)
    (Ho, pt), (Wo, pl) = _same_pads(H), _same_pads(W)
    m = O.max_pool_3x3_s2_same(x)
    assert m.shape == (N, Ho, Wo, C) and m.dtype == np.float32
    sc = _f32(rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C))
    sc[0], sc[-1] = -abs(sc[0]), abs(sc[-1])                                # negative scales among them, whatever the draw
    sh = _f32(rng.standard_normal(C) * 0.5)

    def run(bn):
        B = Bufs(cuda)
        ops.max_pool_fwd(B.inp("x", x), B.out("y", m.size).view(m.shape), 3, 2, pt, pl, B.inp("scale", sc) if bn else None,
                         B.inp("shift", sh) if bn else None)
        B.done()
        return (B.get("y", m.shape),)
    (y,) = _twice(lambda: run(False))
    assert _same_bits(y, m), "%d of %d pooled values differ" % (int((y.view(np.uint32) != m.view(np.uint32)).sum()), m.size)
    (z,) = _twice(lambda: run(True))
    pre = m.astype(np.float64) * sc + sh
    want = np.maximum(pre, 0.0)
    bar = U * want + 2.0 ** -52 * (np.abs(m.astype(np.float64) * sc) + np.abs(sh))
    err = np.abs(z - want)
    print("  MEASURED pool %s %s: %.2f of the bound" % ((N, H, W, C), kind, (err / np.maximum(bar, 1e-300)).max()))
    assert (err <= bar).all() and np.array_equal(z > 0, pre > 0)


# ---- gap_bn_relu and the head's partial sums + gap_out ----------------------------------------------------------------------
def gap_chunks(HW):
    return max(1, min(32, HW // 32))


def head_gap_chunks(N, HW):
    return max(1, min(max(1, 8 // N), HW // 16))


def _gap_case(rng, N, HW, C):
    """x, scale, shift, the float64 mean of relu(x scale + shift) and where it is 0; every 7th channel has no positive term."""
    x = _f32(rng.standard_normal((N, HW, C)))
    sc = _f32(rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C))
    sh = _f32(rng.standard_normal(C) * 0.5)
    dead = np.arange(C) % 7 == 3
    sh[dead] = -100.0
    want = np.maximum(x.astype(np.float64) * sc + sh, 0.0).mean(1)
    assert not want[:, dead].any()
    return x, sc, sh, want, want == 0


def _gap_bound(HW, chunks):
    """Additions on the longest chain: rows r, r + 16, ... of a chunk, the 16 row lanes, the chunks; + the fma and the division."""
    rpc = -(-HW // chunks)
    return (-(-rpc // 16) + 15 + chunks + 2) * U


GAP_CASES = [(1, 4, 1), (3, 4, 15), (1, 64, 16), (3, 68, 17), (1, 68, 33), (3, 64, 127), (1, 2048, 129), (3, 68, 144), (1, 64, 1023),
             (3, 68, 1025), (1, 2048, 1025), (3, 2048, 16), (1, 4, 1025)]


@pytest.mark.parametrize("N,C,HW", GAP_CASES)
def test_gap_bn_relu_against_float64(cuda, N, C, HW):
    """MEASURED on an MI355X, worst over all cases: 0.21 of the bound (ceil(ceil(HW / chunks) / 16) + 15 + chunks + 2) u."""
    from stabnet_amd import ops
    x, sc, sh, want, zero = _gap_case(np.random.default_rng(N + C + HW), N, HW, C)
    chunks = gap_chunks(HW)
    n_part = ops.gap_partial_floats(N, HW, C)
    assert n_part == N * chunks * C

    def run():
        B = Bufs(cuda)
        ops.gap_bn_relu(B.inp("x", x), B.inp("scale", sc), B.inp("shift", sh), B.out("out", N * C), B.out("partial", n_part))
        B.done()
        assert np.isfinite(B.get("partial")).all(), "partial words the size query counts were never written"
        return (B.get("out", (N, C)),)
    (out,) = _twice(run)
    assert not out[zero].any()                                             # no positive term: exactly 0
    rel = np.abs(out[~zero] / want[~zero] - 1.0) if (~zero).any() else np.zeros(1)
    print("  MEASURED gap N=%d C=%d HW=%d chunks=%d: %.2f of the bound" % (N, C, HW, chunks, rel.max() / _gap_bound(HW, chunks)))
    assert (rel <= _gap_bound(HW, chunks)).all()


def _fc_bound(x, w, b, K):
    """(4 ceil(K / 256) + 9) u (sum |x w| + |b|), per element."""
    mag = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + (np.abs(b) if b is not None else 0.0)
    return (4 * -(-K // 256) + 9) * U * mag


def _fc_ref(x, w, b, relu):
    y = x.astype(np.float64) @ w.astype(np.float64).T + (b if b is not None else 0.0)
    return np.maximum(y, 0.0) if relu else y


def _fc_run(cuda, x, w, b, relu):
    from stabnet_amd import ops
    M, Nout = x.shape[0], w.shape[0]
    B = Bufs(cuda)
    ops.fc_fwd(B.inp("x", x), B.inp("w", w), B.inp("b", b) if b is not None else None, B.out("y", M * Nout).view(M, Nout), relu)
    B.done()
    return B.get("y", (M, Nout))


HEAD_GAP_CASES = [(1, 64, 1), (2, 64, 15), (3, 64, 16), (4, 2048, 17), (5, 64, 40), (8, 2048, 144), (1, 2048, 920), (2, 2048, 144),
                  (3, 2048, 920), (4, 64, 144), (5, 2048, 16), (8, 64, 920), (1, 64, 40), (8, 2048, 1)]


def test_gap_cases_cover_every_chunk_count():
    assert {1, 4, 32} <= {gap_chunks(HW) for _, _, HW in GAP_CASES}
    assert {1, 2, 4, 8} <= {head_gap_chunks(N, HW) for N, _, HW in HEAD_GAP_CASES}
    # (the eighth row of a trip of the partial kernel is reached from 113 rows per chunk on)
    assert any(-(-HW // head_gap_chunks(N, HW)) > 112 for N, _, HW in HEAD_GAP_CASES)


@pytest.mark.parametrize("N,C,HW", HEAD_GAP_CASES)
def test_head_gap_fc1_against_float64(cuda, N, C, HW):
    """gap_out within the pooling bound at the head's chunk count; fc_1's output with the bits of fc_fwd(gap_out, relu = 1) --
    fc_gap_kernel against fc_kernel -- and within the FC bound of the float64 product.
    MEASURED on an MI355X, worst over all cases: gap_out 0.18 of its bound, fc_1 0.07 of its bound."""
    from stabnet_amd import ops
    rng = np.random.default_rng(10 * N + C + HW)
    x, sc, sh, want, zero = _gap_case(rng, N, HW, C)
    Nout = 37
    w, b = _f32(rng.standard_normal((Nout, C)) / np.sqrt(C)), _f32(rng.standard_normal(Nout) * 0.1)
    chunks = head_gap_chunks(N, HW)
    n_part = ops.head_gap_partial_floats(N, HW, C)
    assert n_part == N * chunks * C

    def run(tap=True):
        B = Bufs(cuda)
        ops.head_gap_fc1(B.inp("x", x), B.inp("scale", sc), B.inp("shift", sh), B.inp("w", w), B.inp("b", b),
                         B.out("y", N * Nout).view(N, Nout), B.out("gap_out", N * C).view(N, C) if tap else None, B.out("partial", n_part))
        B.done()
        assert np.isfinite(B.get("partial")).all(), "partial words the size query counts were never written"
        return (B.get("y", (N, Nout)), B.get("gap_out", (N, C))) if tap else (B.get("y", (N, Nout)),)
    y, gap = _twice(run)
    assert not gap[zero].any()
    rel = np.abs(gap[~zero] / want[~zero] - 1.0) if (~zero).any() else np.zeros(1)
    e_fc = np.abs(y - _fc_ref(gap, w, b, 1)) / _fc_bound(gap, w, b, C)
    print("  MEASURED head gap N=%d C=%d HW=%d chunks=%d: gap_out %.2f of the bound, fc_1 %.2f of the bound" % (
        N, C, HW, chunks, rel.max() / _gap_bound(HW, chunks), e_fc.max()))
    assert (rel <= _gap_bound(HW, chunks)).all()
    assert (e_fc <= 1.0).all() and (y > 0).any()
    assert _same_bits(y, _fc_run(cuda, gap, w, b, 1)), "fc_gap_kernel and fc_kernel disagree"
    assert _same_bits(run(tap=False)[0], y)                                 # without the tap: the same fc_1


def test_head_fused_supported():
    from stabnet_amd import ops
    dims = [2048, 2048, 1024, 512, 50]
    assert ops.head_fused_supported(1, 2048, dims) and ops.head_fused_supported(8, 2048, dims)
    assert ops.head_fused_supported(3, 64, [64, 2048, 1024, 512, 64])
    assert not ops.head_fused_supported(9, 2048, dims) and not ops.head_fused_supported(0, 2048, dims)
    assert not ops.head_fused_supported(1, 2080, [2080] + dims[1:]) and not ops.head_fused_supported(1, 4096, [4096] + dims[1:])
    assert not ops.head_fused_supported(1, 2048, [2048, 2048, 1024, 256, 50])
    assert not ops.head_fused_supported(1, 2048, [2048, 2048, 1024, 512, 65])
    assert not ops.head_fused_supported(1, 2048, [1024] + dims[1:])


# ---- fc_fwd -----------------------------------------------------------------------------------------------------------------
# fc_lds_kernel: 9 <= M <= 16 and M K 4 <= 128 KiB; else fc_kernel<16> per 16 rows while more than 8 are left, then fc_kernel<8>
FC_CASES = [(1, 4, 1), (3, 68, 3), (8, 1028, 5), (9, 2048, 50), (16, 2048, 257), (16, 2052, 50), (9, 3640, 5), (12, 68, 1030),
            (17, 68, 50), (24, 1028, 3), (25, 4, 257), (33, 2048, 5), (1, 4100, 50), (3, 2052, 257), (8, 4100, 1030), (9, 4, 1),
            (16, 68, 1030), (17, 4100, 3), (24, 2048, 1), (25, 2052, 5), (33, 68, 257), (1, 2048, 1030), (8, 2048, 50), (16, 1028, 5),
            (9, 1028, 257), (16, 4, 3), (33, 4100, 50), (3, 4, 1030), (24, 68, 5), (17, 1028, 1030)]


def _fc_inputs(rng, M, K, Nout):
    x = _f32(rng.standard_normal((M, K)))
    w = _f32(rng.standard_normal((Nout, K)) / np.sqrt(K))
    b = _f32(rng.standard_normal(Nout) * 0.5)
    return x, w, b


@pytest.mark.parametrize("M,K,Nout", FC_CASES)
def test_fc_fwd_against_float64(cuda, M, K, Nout):
    """With bias, with bias + ReLU, and with b = NULL: every element within (4 ceil(K / 256) + 9) u (sum |x w| + |b|).
    MEASURED on an MI355X, worst over all cases and variants: 0.19 of the bound."""
    x, w, b = _fc_inputs(np.random.default_rng(M * 7 + K + Nout), M, K, Nout)
    worst = 0.0
    for bias, relu in ((b, 0), (b, 1), (None, 0)):
        (y,) = _twice(lambda: (_fc_run(cuda, x, w, bias, relu),))
        e = np.abs(y - _fc_ref(x, w, bias, relu)) / _fc_bound(x, w, bias, K)
        worst = max(worst, float(e.max()))
        assert (e <= 1.0).all(), (relu, bias is None, float(e.max()))
        assert not relu or ((y >= 0).all() and (M * Nout < 32 or (y == 0).any()))
    print("  MEASURED fc M=%d K=%d Nout=%d: %.3f of the bound" % (M, K, Nout, worst))


@pytest.mark.parametrize("K,Nout", [(2048, 257), (68, 1030), (1028, 5), (2052, 50)])
def test_fc_rows_do_not_depend_on_the_kernel(cuda, K, Nout):
    """Rows 0..7 of an M = 16 call (fc_lds_kernel; fc_kernel<16> past 128 KiB) have the bits of the M = 8 call (fc_kernel<8>)."""
    x, w, b = _fc_inputs(np.random.default_rng(K + Nout), 16, K, Nout)
    for relu in (0, 1):
        assert _same_bits(_fc_run(cuda, x, w, b, relu)[:8], _fc_run(cuda, x[:8], w, b, relu))


# ---- head_theta_mesh --------------------------------------------------------------------------------------------------------
CROP = 0.8                                                  # config.Config.do_crop_rate: vertices are clipped to +-1 / 0.8


def _theta_inputs(rng, N, n_theta, gain=1.0):
    x = _f32(np.abs(rng.standard_normal((N, 512))))                        # (fc_3's output is behind a ReLU)
    w = _f32(rng.standard_normal((n_theta, 512)) * (0.2 * gain / np.sqrt(512)))
    b = _f32(rng.standard_normal(n_theta) * 0.05)
    return x, w, b


def _theta_run(cuda, x, w, b, grid=None, adv=None, frame=None, frame_hw=(0, 0), frame_offset=0):
    """-> (theta, Hs or None, head after the call or None); grid = (gh, gw) asks for Hs; adv = (start, depth)."""
    from stabnet_amd import ops
    N, n_theta = x.shape[0], w.shape[0]
    B = Bufs(cuda)
    theta = B.out("theta", N * n_theta).view(N, n_theta)
    Hs = B.out("Hs", N * grid[0] * grid[1] * 9) if grid else None
    head = Guarded(cuda, 1, np.array([adv[0]], np.int32), dtype=torch.int32) if adv else None
    pf = B.inp("frame", frame) if frame is not None else None
    ops.head_theta_mesh(B.inp("x", x), B.inp("w", w), B.inp("b", b), theta, grid[0] if grid else 1, grid[1] if grid else 1, CROP, Hs,
                        head.t if adv else None, adv[1] if adv else 1, prefetch_hw=frame_hw,
                        prefetch_ptr=(pf.data_ptr() + frame_offset) if pf is not None else None)
    B.done()
    if head is not None:
        head.check("head_adv")
    return (B.get("theta", (N, n_theta)), B.get("Hs", (N, grid[0], grid[1], 9)) if grid else None,
            int(head.t.cpu()[0]) if head is not None else None)


def _theta_check(cuda, x, w, b, theta, Hs, grid):
    e = np.abs(theta - _fc_ref(x, w, b, 0)) / _fc_bound(x, w, b, 512)
    assert (e <= 1.0).all(), float(e.max())
    if grid:
        from stabnet_amd import warp
        from stabnet_amd.config import Config
        _, _, want = warp.get_4_pts(torch.from_numpy(theta).to(cuda), cfg=Config(grid_h=grid[0], grid_w=grid[1], do_crop_rate=CROP),
                                    with_Hs=True)
        assert _same_bits(Hs, want.cpu().numpy()), "Hs differs from get_4_pts on the same theta"
    return float(e.max())


@pytest.mark.parametrize("N,gh,gw,gain", [(1, 4, 4, 1), (3, 4, 4, 1), (8, 4, 4, 1), (2, 2, 3, 1), (1, 1, 1, 1), (2, 5, 4, 1), (1, 3, 4, 1),
                                          (3, 4, 4, 6)])
def test_head_theta_mesh_against_float64(cuda, N, gh, gw, gain):
    """theta within the FC bound at K = 512; Hs with the bits of get_4_pts on that theta (gain 6: vertices clip at +-1.25).
    MEASURED on an MI355X, worst over all cases: theta 0.024 of the bound."""
    n_theta = 2 * (gh + 1) * (gw + 1)
    x, w, b = _theta_inputs(np.random.default_rng(N + 10 * gh + gw), N, n_theta, gain)
    theta, Hs = _twice(lambda: _theta_run(cuda, x, w, b, (gh, gw))[:2])
    if gain > 1:                                        # most vertices leave the +-lim box
        vx = theta.reshape(N, gh + 1, gw + 1, 2)[..., 0] + np.linspace(-1, 1, gw + 1)
        assert (np.abs(vx) > 1 / CROP).mean() > 0.25
    assert gain > 1 or np.isfinite(Hs).all()
    worst = _theta_check(cuda, x, w, b, theta, Hs, (gh, gw))
    print("  MEASURED theta N=%d %dx%d: %.3f of the bound" % (N, gh, gw, worst))
    assert _same_bits(_theta_run(cuda, x, w, b)[0], theta)                  # without Hs: the same theta


@pytest.mark.parametrize("n_theta", [1, 63, 64])
def test_head_theta_without_mesh(cuda, n_theta):
    """The rows-per-wave limit: 64 rows are 16 on each wave.  MEASURED on an MI355X: 0.019 of the bound."""
    x, w, b = _theta_inputs(np.random.default_rng(n_theta), 2, n_theta)
    (theta,) = _twice(lambda: _theta_run(cuda, x, w, b)[:1])
    print("  MEASURED theta n_theta=%d: %.3f of the bound" % (n_theta, _theta_check(cuda, x, w, b, theta, None, None)))


@pytest.mark.parametrize("N,grid,start,depth,want", [(1, (4, 4), 6, 7, 0), (8, (4, 4), 2, 5, 3), (8, None, 2, 5, 3), (3, (2, 3), 0, 1, 0)])
def test_head_adv_advances_once_per_launch(cuda, N, grid, start, depth, want):
    n_theta = 2 * (grid[0] + 1) * (grid[1] + 1) if grid else 50
    x, w, b = _theta_inputs(np.random.default_rng(N + depth), N, n_theta)
    theta, Hs, head = _theta_run(cuda, x, w, b, grid, adv=(start, depth))
    assert head == want
    plain = _theta_run(cuda, x, w, b, grid)
    assert _same_bits(theta, plain[0]) and (grid is None or _same_bits(Hs, plain[1]))


@pytest.mark.parametrize("H,W", [(8, 4), (9, 12), (45, 76), (288, 512)])
def test_head_prefetch_only_reads(cuda, H, W):
    """The prefetching workgroups read the frame and nothing else: the outputs of the call without them, whatever the frame holds."""
    N, grid = 2, (4, 4)
    rng = np.random.default_rng(H + W)
    x, w, b = _theta_inputs(rng, N, 50)
    theta, Hs, _ = _theta_run(cuda, x, w, b, grid)
    frame = _f32(rng.standard_normal((N, H, W)))
    for f in (frame, np.full((N, H, W), np.nan, np.float32)):
        t2, H2, head = _theta_run(cuda, x, w, b, grid, adv=(1, 3), frame=f, frame_hw=(H, W))
        assert _same_bits(t2, theta) and _same_bits(H2, Hs) and head == 2


@pytest.mark.parametrize("H,W,offset", [(9, 10, 0), (7, 8, 0), (9, 12, 4)])
def test_head_prefetch_switches_itself_off(cuda, H, W, offset):
    """W % 4 != 0, H < 8 or a frame that is not 16-byte aligned: no prefetch, no error, the same outputs."""
    N, grid = 2, (4, 4)
    rng = np.random.default_rng(H * W + offset)
    x, w, b = _theta_inputs(rng, N, 50)
    theta, Hs, _ = _theta_run(cuda, x, w, b, grid)
    frame = _f32(rng.standard_normal(N * H * W + 4))
    t2, H2, _ = _theta_run(cuda, x, w, b, grid, frame=frame, frame_hw=(H, W), frame_offset=offset)
    assert _same_bits(t2, theta) and _same_bits(H2, Hs)


# ---- argument errors (nothing is launched) ----------------------------------------------------------------------------------
def test_argument_errors(cuda):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    L = _lib.lib()
    st = stream_ptr(cuda)
    buf = Guarded(cuda, 1 << 16, "canary")
    d = buf.t.data_ptr()
    assert d % 16 == 0
    m = d + 4                                                               # a device pointer that is not 16-byte aligned
    host = np.zeros(1 << 12, np.float32)
    h = host.ctypes.data
    assert h % 16 == 0
    big = 1 << 20

    def refused(rc, word):
        msg = L.stabnet_last_error()
        assert rc == -1 and msg and word.encode() in msg, (rc, msg, word)

    # shapes the kernels cannot do
    refused(L.stabnet_pad_channels(d, d, 8, 5, 6, st), "multiple of 4")
    refused(L.stabnet_pad_channels(d, d, 8, 9, 8, st), "multiple of 4")
    refused(L.stabnet_stem_repack(d, d, 4, 3, 3, 4, 5, st), "CinPad >= Cin")
    refused(L.stabnet_merge_vectors(d, d, d, 0, 4, d, st), "depth")
    refused(L.stabnet_bn_fold(d, d, d, d, 1e-5, 0, d, d, st), "G =")
    refused(L.stabnet_max_pool_fwd(d, d, 1, 4, 4, 6, 2, 2, 3, 2, 0, 0, 0, 0, st), "C % 4")
    refused(L.stabnet_max_pool_fwd(d, d, big, 128, 128, 4, 64, 64, 3, 2, 0, 0, 0, 0, st), "2^32 channel quads")
    refused(L.stabnet_max_pool_fwd(d, d, 1, 4, 4, 8, 9, 2, 3, 2, 0, 0, 0, 0, st), "geometry")
    refused(L.stabnet_max_pool_fwd(d, d, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, d, 0, st), "both or neither")
    refused(L.stabnet_gap_bn_relu(d, d, d, 1, 4, 6, d, d, 64, st), "C % 4")
    refused(L.stabnet_gap_bn_relu(d, d, d, 65536, 4, 8, d, d, 1 << 30, st), "N =")
    refused(L.stabnet_gap_bn_relu(d, d, d, 2, 64, 8, d, d, 2 * 2 * 8 - 1, st), "partial")
    assert L.stabnet_gap_partial_floats(1, 4, 6) == 0 and L.stabnet_gap_partial_floats(2, 64, 8) == 32
    refused(L.stabnet_fc_fwd(d, d, d, d, 2, 6, 3, 0, st), "K % 4")
    refused(L.stabnet_head_gap_fc1(d, d, d, 9, 4, 64, d, 1 << 30, d, d, d, d, 4, st), "N = 9")
    refused(L.stabnet_head_gap_fc1(d, d, d, 1, 4, 2112, d, 1 << 30, d, d, d, d, 4, st), "C > 2048")
    refused(L.stabnet_head_gap_fc1(d, d, d, 1, 4, 96, d, 1 << 30, d, d, d, d, 4, st), "C % 64")
    refused(L.stabnet_head_gap_fc1(d, d, d, 2, 64, 64, d, 2 * 4 * 64 - 1, d, d, d, d, 4, st), "partial")
    assert L.stabnet_head_gap_partial_floats(9, 4, 64) == 0 and L.stabnet_head_gap_partial_floats(2, 64, 64) == 2 * 4 * 64
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 65, d, 1, 1, 0.8, 0, 0, 1, 0, 0, 0, st), "n_theta = 65")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 50, d, 9, 8, 0.8, 0, 0, 1, 0, 0, 0, st), "gh*gw")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 256, 50, d, 4, 4, 0.8, 0, 0, 1, 0, 0, 0, st), "K = 256")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 48, d, 4, 4, 0.8, d, 0, 1, 0, 0, 0, st), "needs n_theta = 50")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 50, d, 4, 4, 0.8, 0, d, 0, 0, 0, 0, st), "depth")
    # pointers the kernels read as float4
    refused(L.stabnet_pad_channels(d, m, 8, 5, 8, st), "aligned")
    refused(L.stabnet_max_pool_fwd(m, d, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, 0, 0, st), "aligned")
    refused(L.stabnet_max_pool_fwd(d, d, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, d, m, st), "aligned")
    refused(L.stabnet_gap_bn_relu(d, m, d, 1, 4, 8, d, d, 64, st), "aligned")
    refused(L.stabnet_gap_bn_relu(d, d, d, 1, 4, 8, d, m, 64, st), "aligned")
    refused(L.stabnet_fc_fwd(d, m, d, d, 2, 8, 3, 0, st), "aligned")
    refused(L.stabnet_head_gap_fc1(d, d, d, 1, 4, 64, d, 64, m, d, d, d, 4, st), "aligned")
    refused(L.stabnet_head_theta_mesh(m, d, d, 1, 512, 50, d, 4, 4, 0.8, 0, 0, 1, 0, 0, 0, st), "aligned")
    # null pointers
    refused(L.stabnet_pad_channels(0, d, 8, 5, 8, st), "null")
    refused(L.stabnet_stem_repack(d, 0, 4, 3, 3, 8, 5, st), "null")
    refused(L.stabnet_merge_vectors(d, 0, d, 4, 4, d, st), "null")
    refused(L.stabnet_bn_fold(d, d, d, d, 1e-5, 8, d, 0, st), "null")
    refused(L.stabnet_max_pool_fwd(d, 0, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, 0, 0, st), "null")
    refused(L.stabnet_gap_bn_relu(d, d, d, 1, 4, 8, d, 0, 64, st), "null")
    refused(L.stabnet_fc_fwd(d, d, d, 0, 2, 8, 3, 0, st), "null")
    refused(L.stabnet_head_gap_fc1(d, d, d, 1, 4, 64, d, 64, 0, d, 0, d, 4, st), "null")        # (fc_1 always has its bias)
    refused(L.stabnet_head_theta_mesh(d, d, 0, 1, 512, 50, d, 4, 4, 0.8, 0, 0, 1, 0, 0, 0, st), "null")
    assert L.stabnet_head_fused_supported(1, 2048, 0) == 0
    # host pointers
    refused(L.stabnet_pad_channels(h, d, 8, 5, 8, st), "pad_channels")
    refused(L.stabnet_stem_repack(h, d, 4, 3, 3, 8, 5, st), "stem_repack")
    refused(L.stabnet_merge_vectors(d, d, d, 4, 4, h, st), "merge_vectors")
    refused(L.stabnet_bn_fold(d, d, h, d, 1e-5, 8, d, d, st), "bn_fold")
    refused(L.stabnet_max_pool_fwd(d, h, 1, 4, 4, 8, 2, 2, 3, 2, 0, 0, 0, 0, st), "max_pool_fwd")
    refused(L.stabnet_gap_bn_relu(d, d, d, 1, 4, 8, h, d, 64, st), "gap_bn_relu")
    refused(L.stabnet_fc_fwd(d, d, h, d, 2, 8, 3, 0, st), "fc_fwd")
    refused(L.stabnet_head_gap_fc1(d, d, d, 1, 4, 64, d, 64, 0, h, d, d, 4, st), "head_gap_fc1")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 50, d, 4, 4, 0.8, 0, 0, 1, h, 8, 8, st), "head_theta_mesh")
    refused(L.stabnet_head_theta_mesh(d, d, d, 1, 512, 50, h, 4, 4, 0.8, 0, 0, 1, 0, 0, 0, st), "head_theta_mesh")
    torch.cuda.synchronize()
    assert buf.untouched() and not host.any()                               # none of the refused calls launched anything
