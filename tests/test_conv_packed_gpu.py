"""GPU parity of the packed split convolution kernels (conv_ring_f32_kernel<MODE, 4, KG, PRO>, through stabnet_conv2d_fwd_packed):
float32 operands as exact sums of three bf16 terms, six bf16 x bf16 partial products per f32 product, f32 accumulation on
v_mfma_f32_32x32x16_bf16.  Same bar as the exact-f32-MFMA kernels (2e-5 of the output scale against the oracle's im2col + sgemm
convolution, different summation order) and a tighter one against those kernels themselves: this is not a reduced-precision mode."""
import numpy as np
import pytest
import torch

from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu

# N,H,W,Cin,Cout,k,stride,pad, prologue, bias, residual(0 none,1 same,2 strided), relu, splitk (0 = planned)
CASES = [
    (1, 17, 23, 32, 64, 1, 1, 0, False, False, 0, False, 0),    # 1 K-step, ragged M
    (1, 17, 23, 96, 96, 1, 1, 0, False, True, 0, True, 0),      # 3 K-steps, ragged Cout tile
    (1, 17, 23, 128, 64, 1, 1, 0, False, False, 1, False, 0),   # 4 K-steps + residual
    (1, 17, 23, 160, 64, 1, 1, 0, False, False, 0, False, 0),   # 5 K-steps
    (1, 17, 23, 256, 64, 1, 1, 0, False, False, 0, False, 0),   # 8 K-steps: the mid-tile fast steps
    (2, 36, 64, 64, 64, 3, 1, 1, False, False, 0, False, 0),    # 3x3 SAME, zero page taps
    (1, 37, 63, 128, 128, 3, 2, 1, False, True, 0, True, 0),    # 3x3 stride 2, odd sizes
    (1, 36, 64, 64, 64, 3, 1, 2, False, False, 0, False, 0),    # pad 2
    (1, 9, 16, 512, 512, 3, 1, 1, False, False, 0, True, 0),    # planned split-K: slabs + reduce
    (1, 18, 32, 128, 512, 1, 2, 0, False, True, 2, False, 0),   # strided 1x1 + strided residual read
    (1, 180, 320, 64, 64, 3, 1, 1, False, True, 1, True, 0),    # 900 tiles > 512 resident workgroups: the ring across tile boundaries
    (1, 180, 320, 32, 256, 1, 1, 0, False, False, 1, False, 0), # 3600 one-step tiles
    (1, 60, 60, 256, 256, 3, 1, 1, False, True, 1, False, 3),   # the block-3 conv2 shape of a 720p frame, three slabs + reduce
    (1, 60, 60, 256, 256, 3, 1, 1, False, True, 1, True, 2),    # ... two K groups inside the workgroup
    (1, 30, 30, 64, 64, 3, 1, 1, False, False, 0, False, 2),    # 3x3, 18 steps, two groups, single ragged round
    (1, 17, 23, 192, 96, 1, 1, 0, False, True, 1, True, 2),     # 1x1, 6 steps, two groups, ragged M and Cout
    (1, 150, 160, 128, 64, 1, 1, 0, False, False, 0, False, 2), # 375 tiles > 256 CUs: several tiles per 8-wave workgroup
    # BN + ReLU prologue on the A fragments (the inference conv1 layers)
    (1, 36, 64, 64, 64, 1, 1, 0, True, False, 0, False, 0),
    (1, 36, 64, 256, 64, 1, 1, 0, True, True, 1, True, 0),
    (1, 90, 160, 512, 128, 1, 1, 0, True, False, 0, True, 0),   # block-2 conv1 of a 720p frame
    (1, 60, 60, 1024, 256, 1, 1, 0, True, False, 0, True, 2),   # block-3 conv1: prologue + two K groups inside the workgroup
    (1, 23, 40, 2048, 512, 1, 1, 0, True, False, 0, True, 4),   # block-4 conv1: prologue + slabs
    (1, 17, 23, 128, 96, 1, 1, 0, True, True, 0, False, 2),     # prologue, two groups, ragged tiles
    # geometries the packed kernels do not take: the same call runs the exact-f32 kernels on w_ohwi
    (1, 20, 24, 16, 64, 7, 2, 3, False, True, 0, False, 0),     # Cin = 16 (no weight image exists)
    (1, 37, 63, 128, 128, 3, 2, 1, True, False, 0, False, 0),   # 3x3 with a prologue (register-staged kernel)
]


@pytest.mark.parametrize("out_bn", [False, True])
@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad,prologue,bias,res,relu,splitk", CASES)
def test_conv2d_packed_matches_oracle_and_f32_kernels(cuda, N, H, W, Cin, Cout, k, stride, pad, prologue, bias, res, relu, splitk, out_bn):
    from stabnet_amd import ops
    rng = np.random.default_rng(Cin * 7 + Cout + k + splitk)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32) if bias else None
    sc = rng.uniform(0.5, 1.5, Cin).astype(np.float32) if prologue else None
    sh = (rng.standard_normal(Cin) * 0.3).astype(np.float32) if prologue else None
    a = x if not prologue else np.maximum(x * sc + sh, 0).astype(np.float32)
    want = O.conv2d(a, w, stride, ((pad, pad), (pad, pad)), b)
    Ho, Wo = want.shape[1:3]
    r = None
    if res == 1:
        r = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
        want = want + r
    elif res == 2:
        r = rng.standard_normal((N, 2 * Ho - 1, 2 * Wo, Cout)).astype(np.float32)
        want = want + r[:, ::2, ::2, :]
    osc = osh = None
    if out_bn:
        osc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
        osh = (rng.standard_normal(Cout) * 0.3).astype(np.float32)
        want = (want * osc + osh).astype(np.float32)
    if relu:
        want = np.maximum(want, 0)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(cuda)
    # scales and shifts as two slices of one buffer (the prologue kernels address the shifts relative to the scales)
    ss = t(np.concatenate([sc, sh])) if prologue else None
    tsc, tsh = (ss[:Cin], ss[Cin:]) if prologue else (None, None)
    args = (t(x), t(ops.pack_conv_weight(w)), t(b), tsc, tsh, t(r), 2 if res == 2 else 1, stride, pad, relu)
    got = ops.conv2d_packed(*args, out_scale=t(osc), out_shift=t(osh), splitk=splitk).cpu().numpy()
    f32 = ops.conv2d(*args, out_scale=t(osc), out_shift=t(osh)).cpu().numpy()
    assert got.shape == want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= (4e-5 if out_bn else 2e-5) * scale, "max err vs oracle %g (scale %g)" % (err, scale)
    d = np.abs(got - f32).max()
    assert d <= 4e-6 * scale, "max difference to the exact-f32-MFMA kernels %g (scale %g)" % (d, scale)


def test_weight_image_is_an_exact_three_term_split(cuda):
    """Every weight equals h + m + l of its image entry, bit for bit (float32 sum of the three bf16 terms, small terms first)."""
    from stabnet_amd import _lib, ops
    from stabnet_amd._tensor import ptr, stream_ptr
    rng = np.random.default_rng(5)
    Cout, K = 96, 64
    w = (rng.standard_normal((Cout, 1, 1, K)) * np.exp(rng.uniform(-8, 8, (Cout, 1, 1, K)))).astype(np.float32)
    wt = torch.from_numpy(w).to(cuda)
    n = int(_lib.lib().stabnet_conv_weight_image_floats(Cout, 1, 1, K))
    assert n == 2 * 2 * 3072
    img = torch.zeros(n, dtype=torch.float32, device=cuda)
    _lib.call("stabnet_conv_weight_split_image", ptr(wt), Cout, 1, 1, K, ptr(img), stream_ptr(cuda), device=cuda)
    raw = img.cpu().numpy().view(np.uint16).reshape(2, 2, 2, 3, 2, 64, 8)          # [N tile][K step][wn][plane][j][lane][e]
    f = (raw.astype(np.uint32) << 16).view(np.float32)
    for n_ in range(Cout):
        nt, wn, ln = n_ // 64, (n_ % 64) // 32, n_ % 32
        for k in range(K):
            ks, kk = k // 32, k % 32
            j, rem = kk // 16, kk % 16
            e_hi, rem2 = rem // 8, rem % 8
            g, e_lo = rem2 // 4, rem2 % 4
            h, m, l = (f[nt, ks, wn, p, j, ln + 32 * g, 4 * e_hi + e_lo] for p in range(3))
            assert np.float32(np.float32(l + m) + h) == w[n_, 0, 0, k], (n_, k)
    # rows of the ragged second tile beyond Cout are zero
    assert not raw[1, :, 1].any()


def _image_planes(img, Cout, K):
    """h, m, l (float32, [Cout][K]) of every weight from a fragment-major image: [N tile][K step][wn][plane][j][lane][e]."""
    raw = img.cpu().numpy().view(np.uint16).reshape((Cout + 63) // 64, K // 32, 2, 3, 2, 64, 8)
    f = (raw.astype(np.uint32) << 16).view(np.float32)
    n, k = np.meshgrid(np.arange(Cout), np.arange(K), indexing="ij")
    kk = k % 32
    j, rem = kk // 16, kk % 16
    lane = n % 32 + 32 * ((rem % 8) // 4)
    e = 4 * (rem // 8) + rem % 4
    return [f[n // 64, k // 32, (n % 64) // 32, p, j, lane, e] for p in range(3)]


def test_weight_image_split_over_the_whole_float32_range(cuda):
    """The weight image (fold time) over every float32 class: finite |w| >= 2^-110 is h + m + l bit for bit -- up to FLT_MAX: a
    finite |w| >= 2^127 (2 - 2^-8) takes the largest finite bf16 as its head instead of rounding to infinity (FLT_MAX = (2^128 -
    2^120) + 2^120 - 2^104); below 2^-110 the last term is a bf16 subnormal and the split is exact to 2^-133; +-inf and NaN stay
    non-finite (include/stabnet_hip.h, operand mode 4)."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    rng = np.random.default_rng(17)
    Cout, K = 64, 64
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x003FFFFF, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,   # +-0, subnormals, 2^-126
            0x7F7F8000, 0xFF7F8000, 0x7F7F8001, 0x7F7FC000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F0000,                # the top of the range
            0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001]                                                                  # +-inf, NaN
    n_small = 256                                          # exponents -149 .. -100: around and below 2^-110
    small = (rng.integers(0, 2, n_small) << 31) | (rng.integers(0, 27, n_small) << 23) | rng.integers(0, 1 << 23, n_small)
    n_rest = Cout * K - len(bits) - n_small                 # random exponents -126 .. 127, random mantissas and signs
    rest = (rng.integers(0, 2, n_rest) << 31) | (rng.integers(1, 255, n_rest) << 23) | rng.integers(0, 1 << 23, n_rest)
    allbits = np.concatenate([np.array(bits, np.int64), small, rest]).astype(np.uint32)
    w = rng.permutation(allbits).view(np.float32).reshape(Cout, 1, 1, K)
    wt = torch.from_numpy(w).to(cuda)
    img = torch.full((int(_lib.lib().stabnet_conv_weight_image_floats(Cout, 1, 1, K)),), float("nan"), device=cuda)
    _lib.call("stabnet_conv_weight_split_image", ptr(wt), Cout, 1, 1, K, ptr(img), stream_ptr(cuda), device=cuda)
    h, m, l = _image_planes(img, Cout, K)
    w2 = w.reshape(Cout, K)
    fin = np.isfinite(w2)
    big = fin & (np.abs(w2) >= 2.0 ** -110)
    with np.errstate(over="ignore", invalid="ignore"):
        s32 = (l + m) + h                                   # float32, small terms first
        s64 = l.astype(np.float64) + m.astype(np.float64) + h.astype(np.float64)
    assert np.isfinite(h[fin]).all() and np.isfinite(m[fin]).all() and np.isfinite(l[fin]).all()
    assert np.array_equal(s32[big].view(np.uint32), w2[big].view(np.uint32)), np.argwhere(s32 != w2)[:5]
    tiny_err = np.abs(s64[fin & ~big] - w2[fin & ~big].astype(np.float64)).max()
    print("split error below 2^-110: max %.3e = 2^%.1f" % (tiny_err, np.log2(tiny_err) if tiny_err > 0 else -np.inf))
    assert tiny_err <= 2.0 ** -133
    assert not np.isfinite(s64[~fin]).any()
    top = np.abs(w2) == np.float32(np.finfo(np.float32).max)
    assert top.any() and (np.abs(h[top]).view(np.uint32) == 0x7F7F0000).all()   # the saturated head


@pytest.mark.parametrize("k,Cin,Cout", [(1, 512, 128), (3, 128, 64), (1, 2048, 64)])
def test_packed_error_against_float64_is_the_f32_mfma_error(cuda, k, Cin, Cout):
    """Not a reduced-precision mode: against a FLOAT64 convolution of the same float32 inputs, the packed split kernel's error is
    the exact-f32-MFMA kernel's error (both are float32 accumulations of exact -- resp. 2^-23-accurate -- products; the bf16-operand
    mode on the same data is three orders of magnitude further away)."""
    from stabnet_amd import ops
    rng = np.random.default_rng(k * 1000 + Cin)
    N, H, W = 1, 24, 32
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    pad = k // 2
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    cols = np.concatenate([xp[:, i:i + H, j:j + W, :] for i in range(k) for j in range(k)], axis=-1)      # [N,H,W,k*k*Cin] (kh, kw, c)
    want = cols.reshape(-1, k * k * Cin) @ w.astype(np.float64).reshape(k * k * Cin, Cout)
    want = want.reshape(N, H, W, Cout)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(cuda)
    wt = t(ops.pack_conv_weight(w))
    got_p = ops.conv2d_packed(t(x), wt, pad=pad).cpu().numpy().astype(np.float64)
    got_f = ops.conv2d(t(x), wt, pad=pad).cpu().numpy().astype(np.float64)
    scale = np.abs(want).max()
    e_p, e_f = np.abs(got_p - want).max() / scale, np.abs(got_f - want).max() / scale
    r_p, r_f = np.sqrt(np.mean((got_p - want) ** 2)) / scale, np.sqrt(np.mean((got_f - want) ** 2)) / scale
    print("k=%d K=%d: max / rms error vs float64, relative to the output scale: packed split %.2e / %.2e, f32 MFMA %.2e / %.2e" % (
        k, k * k * Cin, e_p, r_p, e_f, r_f))
    assert e_p <= 2.0 * e_f + 1e-7 and r_p <= 1.5 * r_f + 2e-8
    assert e_p < 3e-6


# ---- activations: the run-time split of the A fragments (operand range, non-finite inputs, guard bands) -------------------------
GUARD_FLOATS = 16 * 1024                                   # 64 KiB of NaN / canary on each side of a buffer
CANARY = 0x5CA1AB1E


def _conv64(a, w, stride=1, pad=0):
    """float64 convolution of the float32 values (HWIO weights, NHWC input)."""
    k, C = w.shape[0], a.shape[3]
    N, H, W = a.shape[:3]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ap = np.pad(a.astype(np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    cols = np.concatenate([ap[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride, :]
                           for i in range(k) for j in range(k)], axis=-1)
    return (cols.reshape(-1, k * k * C) @ w.astype(np.float64).reshape(k * k * C, -1)).reshape(N, Ho, Wo, -1)


def _conv_guarded(cuda, packed, x, w, stride=1, pad=0, relu=False, splitk=0, sc=None, sh=None):
    """One convolution through the C ABI -- stabnet_conv2d_fwd_packed (packed=True) or stabnet_conv2d_fwd_ex -- with guard bands:
    x sits inside a NaN-filled buffer, y inside a canary-filled one, and the workspace is NaN with a canary tail beyond the size
    asked for.  Asserts the canaries intact; returns y (numpy)."""
    from stabnet_amd import _lib, ops
    from stabnet_amd._tensor import stream_ptr
    L = _lib.lib()
    N, H, W, Cin = x.shape
    k, Cout = w.shape[0], w.shape[3]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = GUARD_FLOATS
    xb = torch.full((x.size + 2 * g,), float("nan"), dtype=torch.float32, device=cuda)
    xb[g:g + x.size] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1)).to(cuda)
    ny = N * Ho * Wo * Cout
    yb = torch.full((ny + 2 * g,), CANARY, dtype=torch.int32, device=cuda)
    ws_bytes = int(L.stabnet_conv2d_workspace_bytes(N, H, W, Cin, Cout, k, k, stride, pad))
    if packed:
        ws_bytes = max(ws_bytes, max(splitk, 0) * ny * 4)
    n4 = (ws_bytes + 3) // 4
    wsb = torch.full((n4 + g,), CANARY, dtype=torch.int32, device=cuda)
    wsb[:n4].view(torch.float32).fill_(float("nan"))
    wt = torch.from_numpy(np.ascontiguousarray(ops.pack_conv_weight(w), dtype=np.float32)).to(cuda)
    ss = torch.from_numpy(np.concatenate([sc, sh]).astype(np.float32)).to(cuda) if sc is not None else None
    p_sc, p_sh = (ss[:Cin].data_ptr(), ss[Cin:].data_ptr()) if ss is not None else (0, 0)
    xp, yp, wsp = xb[g:].data_ptr(), yb[g:].data_ptr(), wsb.data_ptr()
    st = stream_ptr(cuda)
    if packed:
        n_img = int(L.stabnet_conv_weight_image_floats(Cout, k, k, Cin))
        img = torch.empty(max(n_img, 1), dtype=torch.float32, device=cuda)
        if n_img:
            _lib.call("stabnet_conv_weight_split_image", wt.data_ptr(), Cout, k, k, Cin, img.data_ptr(), st, device=cuda)
        _lib.call("stabnet_conv2d_fwd_packed", xp, wt.data_ptr(), img.data_ptr(), 0, p_sc, p_sh, 0, 0, 0, 1, 0, 0, yp, N, H, W, Cin,
                  Cout, k, k, stride, pad, int(relu), int(splitk), wsp, ws_bytes, st, device=cuda)
    else:
        _lib.call("stabnet_conv2d_fwd_ex", xp, wt.data_ptr(), 0, p_sc, p_sh, 0, 0, 0, 1, 0, 0, yp, N, H, W, Cin, Cout, k, k, stride,
                  pad, int(relu), wsp, ws_bytes, st, device=cuda)
    torch.cuda.synchronize()
    yh, wsh = yb.cpu().numpy().view(np.uint32), wsb.cpu().numpy().view(np.uint32)
    assert (yh[:g] == CANARY).all() and (yh[g + ny:] == CANARY).all(), "write outside y"
    assert (wsh[n4:] == CANARY).all(), "write beyond the workspace size asked for"
    return yh[g:g + ny].view(np.float32).reshape(N, Ho, Wo, Cout).copy()


@pytest.mark.parametrize("s", [-100, -60, 60])
@pytest.mark.parametrize("k,Cin,Cout,splitk", [(1, 512, 128, 0), (3, 128, 64, 0), (3, 64, 64, 2)])
def test_packed_error_is_the_f32_error_across_the_activation_range(cuda, k, Cin, Cout, splitk, s):
    """Inputs scaled by 2^s and weights by 2^-s: the run-time split of the activations stays exact (|x| >= 2^-110), so the packed
    kernel's error against a float64 convolution is the f32 kernel's at every scale (the bar of the unscaled test above)."""
    rng = np.random.default_rng(1000 * k + Cin + s)
    N, H, W = 1, 24, 32
    x = (rng.standard_normal((N, H, W, Cin)) * 2.0 ** s).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin)) * 2.0 ** -s).astype(np.float32)
    pad = k // 2
    want = _conv64(x, w, 1, pad)
    got_p = _conv_guarded(cuda, True, x, w, pad=pad, splitk=splitk).astype(np.float64)
    got_f = _conv_guarded(cuda, False, x, w, pad=pad).astype(np.float64)
    scale = np.abs(want).max()
    e_p, e_f = np.abs(got_p - want).max() / scale, np.abs(got_f - want).max() / scale
    print("s=%d k=%d K=%d splitk=%d: max error vs float64 / output scale: packed %.2e, f32 %.2e" % (s, k, k * k * Cin, splitk, e_p, e_f))
    assert np.isfinite(got_p).all() and np.isfinite(got_f).all()
    assert e_p <= 2.0 * e_f + 1e-7 and e_p < 3e-6


# N,H,W,Cin,Cout,k,stride,pad, prologue, splitk (0 = planned)
NONFINITE_CASES = [
    (1, 17, 23, 96, 64, 1, 1, 0, False, 0),      # 1x1, ragged last M tile
    (1, 17, 23, 64, 64, 3, 1, 1, False, 0),      # 3x3 SAME, zero-padded border
    (1, 9, 16, 512, 512, 3, 1, 1, False, 0),     # planned split-K: slabs + reduce
    (1, 30, 30, 64, 64, 3, 1, 1, False, 2),      # two K groups inside the workgroup
    (1, 36, 64, 256, 64, 1, 1, 0, True, 0),      # BN + ReLU prologue on the A fragments (fmaxf: NaN -> 0, -inf -> 0)
]


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad,prologue,splitk", NONFINITE_CASES)
def test_nonfinite_inputs_poison_exactly_their_receptive_fields(cuda, N, H, W, Cin, Cout, k, stride, pad, prologue, splitk):
    """+-inf and NaN at chosen input positions -- the last pixel (ragged last tile, last K slice), a mid-K channel of an inner pixel,
    a pixel of the top row (next to the zero padding).  Without a ReLU epilogue the non-finite outputs of the packed kernel, of the
    f32 kernel and the receptive fields of the non-finite (post-prologue, np.fmax semantics) inputs are the same set; the packed
    kernel gives NaN there (the split of an infinity is inf + NaN + NaN) where the f32 kernel may give +-inf.  Every other output
    keeps the bars of test_conv2d_packed_matches_oracle_and_f32_kernels."""
    rng = np.random.default_rng(Cin + 7 * Cout + k + splitk)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, Cin).astype(np.float32) if prologue else None
    sh = (rng.standard_normal(Cin) * 0.3).astype(np.float32) if prologue else None
    vals = [np.inf, -np.inf, np.nan]
    for i, (pix, c) in enumerate([((N - 1, H - 1, W - 1), Cin - 1), ((0, H // 2, W // 2), Cin // 2 + 3), ((0, 0, W // 3), 1)]):
        x[pix + (c,)] = vals[(i + k + splitk) % 3]
    with np.errstate(invalid="ignore"):
        a = x if not prologue else np.fmax(x * sc + sh, np.float32(0)).astype(np.float32)
    bad = ~np.isfinite(a).all(axis=-1)
    expect = _conv64(bad[..., None].astype(np.float64), np.ones((k, k, 1, 1)), stride, pad)[..., 0] > 0
    expect = np.broadcast_to(expect[..., None], expect.shape + (Cout,))
    got_p = _conv_guarded(cuda, True, x, w, stride, pad, splitk=splitk, sc=sc, sh=sh)
    got_f = _conv_guarded(cuda, False, x, w, stride, pad, sc=sc, sh=sh)
    assert expect.any()
    assert np.array_equal(~np.isfinite(got_f), expect)
    assert np.array_equal(~np.isfinite(got_p), expect)
    assert np.isnan(got_p[expect]).all()
    want = _conv64(np.where(np.isfinite(a), a, 0), w, stride, pad)
    fin = ~expect
    scale = np.abs(want[fin]).max()
    assert np.abs(got_p[fin] - want[fin]).max() <= 2e-5 * scale
    assert np.abs(got_p[fin] - got_f[fin]).max() <= 4e-6 * scale


def test_relu_epilogue_turns_the_packed_nan_of_an_infinite_input_into_zero(cuda):
    """Pinned, not wanted: an output that is +inf on the f32 kernel is NaN before the ReLU epilogue on the packed kernel, and
    fmaxf(NaN, 0) = 0 -- a silent finite result.  -inf outputs are 0 on both (include/stabnet_hip.h, operand mode 4)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 17, 23, 128)).astype(np.float32)      # (Cin = 64 1x1 layers take the f32 register-staged kernel)
    w = (rng.standard_normal((1, 1, 128, 64)) * 0.125).astype(np.float32)
    x[0, 5, 7, 10] = np.inf
    got_p = _conv_guarded(cuda, True, x, w, relu=True)
    got_f = _conv_guarded(cuda, False, x, w, relu=True)
    pos = w[0, 0, 10, :] > 0
    assert pos.any() and (~pos).any()
    assert (got_f[0, 5, 7, pos] == np.inf).all() and (got_f[0, 5, 7, ~pos] == 0).all()
    assert (got_p[0, 5, 7, :] == 0).all()
    other = np.ones(got_p.shape[:3], bool)
    other[0, 5, 7] = False
    assert np.isfinite(got_p[other]).all() and np.abs(got_p[other] - got_f[other]).max() <= 4e-6 * np.abs(got_f[other]).max()


def test_finite_activations_beyond_the_bf16_range_are_out_of_contract(cuda):
    """Pinned, out of contract: the run-time split of x does not saturate (no VALU added to the K loop), so a finite |x| >=
    2^127 (2 - 2^-8) rounds its head to a bf16 infinity and the packed output is NaN where the f32 kernel's is finite.  The largest
    float32 below that bound still splits."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 17, 23, 128)).astype(np.float32)
    w = (rng.standard_normal((1, 1, 128, 64)) * 2.0 ** -20).astype(np.float32)
    big = [((0, 3, 4), 9, 0x7F7F8000), ((0, 10, 11), 20, 0x7F7FFFFF), ((0, 16, 22), 63, 0xFF7FFFFF)]
    for pix, c, b in big:
        x[pix + (c,)] = np.array([b], np.uint32).view(np.float32)[0]
    x[0, 8, 8, 30] = np.array([0x7F7F7FFF], np.uint32).view(np.float32)[0]
    got_p = _conv_guarded(cuda, True, x, w)
    got_f = _conv_guarded(cuda, False, x, w)
    assert np.isfinite(got_f).all()
    mask = np.zeros(got_p.shape[:3], bool)
    for pix, _, _ in big:
        mask[pix] = True
    assert np.isnan(got_p[mask]).all()
    assert np.isfinite(got_p[~mask]).all()
    d = np.abs(got_p[~mask].astype(np.float64) - got_f[~mask])
    assert (d <= 4e-6 * np.abs(got_f[~mask]).max(axis=-1, keepdims=True)).all()
