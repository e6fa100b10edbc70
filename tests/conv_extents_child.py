"""Child of tests/test_conv_extents_gpu.py (not a test module): ONE case per process -- every case allocates a buffer of about 4 GiB, and
the conv switches a case needs (STABNET_CONV_PATCH_MIN_M) are read once per process.  `python conv_extents_child.py <case>`; exits
non-zero on the first failed assertion and prints one MEASURED line per launch.  The cases and what they assert are described in the
parent's docstring."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _extents as ex                                        # noqa: E402
import _extents_search as es                                 # noqa: E402
import _poison                                               # noqa: E402
from _guarded import CANARY, GUARD                           # noqa: E402

LIMIT = 1 << 30                                              # floats (the guard: an operand's extent stays BELOW it)
BAR_PLAIN = BAR_OUT_BN = None                                # test_route_census_gpu's own, set by bars() in main(): no number is written here
DEV = torch.device("cuda:0")


def bars():
    """The bars of tests/test_route_census_gpu.py, read from the module itself (importing it needs pytest only)."""
    global BAR_PLAIN, BAR_OUT_BN
    import test_route_census_gpu as census
    BAR_PLAIN, BAR_OUT_BN = census.BAR_PLAIN, census.BAR_OUT_BN


def largest_ld(pixels):
    ld = (LIMIT - 1) // pixels // 4 * 4
    assert pixels * ld < LIMIT <= pixels * (ld + 4)
    return ld


class Big:
    """n floats of NaN between two canary bands, allocated once per child."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=torch.float32, device=DEV)
        self.buf[:GUARD].view(torch.int32).fill_(CANARY)
        self.buf[GUARD + self.n:].view(torch.int32).fill_(CANARY)
        self.t = self.buf[GUARD:GUARD + self.n]
        self.poison()

    def poison(self):
        self.t.fill_(float("nan"))

    def check_bands(self, what):
        lo, hi = self.buf[:GUARD].view(torch.int32), self.buf[GUARD + self.n:].view(torch.int32)
        assert bool((lo == CANARY).all()) and bool((hi == CANARY).all()), "write outside " + what

    def count_not_nan(self):
        total, step = 0, 1 << 28
        for a in range(0, self.n, step):
            total += int((~torch.isnan(self.t[a:a + step])).sum())
        return total


def kind_name():
    from stabnet_amd import _lib
    L = _lib.lib()
    return L.stabnet_prof_kind_name(int(L.stabnet_conv_last_launch_kind())).decode()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def conv64(x, w, stride, pad):
    """float64 convolution of float32 inputs: x [N,H,W,C], w [O,KH,KW,C] -> [N,Ho,Wo,O]"""
    y = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(0, 3, 1, 2))),
                                   torch.from_numpy(np.ascontiguousarray(w.astype(np.float64).transpose(0, 3, 1, 2))), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).numpy()


def held(what, got, want, bar):
    mag, err = float(np.abs(want).max()), float(np.abs(got.astype(np.float64) - want).max())
    print("MEASURED %s: err %.3g of magnitude %.3g (%.2g of the bar)" % (what, err, mag, err / (bar * mag)))
    assert mag > 0 and err <= bar * mag, "%s: max err %g against float64, magnitude %g, bar %g" % (what, err, mag, bar * mag)


def edge_rows(M, row_floats, seed):
    """Rows of an [M][row_floats] operand: the first and the last 64-row tile, the rows on both sides of byte offsets 2^31 and 3 * 2^30,
    64 rows drawn with a fixed seed."""
    rows = set(range(min(64, M))) | set(range(max(0, M - 64), M))
    for off in (1 << 31, 3 << 30):
        m = off // (4 * row_floats)
        rows |= {r for r in (m - 1, m, m + 1) if 0 <= r < M}
    rows |= {int(r) for r in np.random.default_rng(seed).integers(0, M, 64)}
    return np.array(sorted(rows), np.int64)


# ---- A, B, C: the input's pixel stride at the limit (stabnet_conv2d_fwd_packed_ld) ------------------------------------------------------
def strided_input(N, H, W, Cin, Cout, k, stride, pad, expect):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    L = _lib.lib()
    rng = np.random.default_rng(1000 * k + 10 * stride + Cin)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ld_big = largest_ld(N * (H + 2 * pad) * (W + 2 * pad))      # the entry counts the zero-padded frame
    ld_small = Cin + 4                                         # a multiple of 4 that is not Cin: the same route, offsets near the base
    pixels = N * H * W
    big = Big(pixels * ld_big)
    xd, wd, bd = dev(x), dev(w), dev(b)
    img = torch.empty(int(L.stabnet_conv_weight_image_floats(Cout, k, k, Cin)), dtype=torch.float32, device=DEV)
    _lib.call("stabnet_conv_weight_split_image", ptr(wd), Cout, k, k, Cin, ptr(img), stream_ptr(DEV), device=DEV)
    got = {}
    for ld in (ld_big, ld_small):
        big.poison()
        view = big.t[:pixels * ld].view(N, H, W, ld)
        view[..., :Cin] = xd                                   # only the columns the launch reads
        out = _poison.Poisoned(DEV, (N, Ho, Wo, Cout), 0)
        _lib.call("stabnet_conv2d_fwd_packed_ld", ptr(view), ld, ptr(wd), ptr(img), ptr(bd), 0, 0, 0, 0, 0, 1, 0, 0, ptr(out.out), N, H, W, Cin, Cout,
                  k, k, stride, pad, 0, 1, ptr(out.workspace), 0, stream_ptr(DEV), device=DEV)
        y = out.result("x_ld=%d" % ld)
        name = kind_name()
        print("x_ld=%d (%.2f GB): %s" % (ld, 4e-9 * pixels * ld, name))
        assert expect in name, "the launch took %s, not a %s kernel" % (name, expect)
        big.check_bands("the input buffer")
        assert big.count_not_nan() == pixels * Cin, "the input buffer was written"
        assert same_bits(view[..., :Cin].cpu().numpy(), x)
        got[ld] = (y, name)
    assert got[ld_big][1] == got[ld_small][1]
    assert same_bits(got[ld_big][0], got[ld_small][0]), "the launch at x_ld=%d and the same launch at x_ld=%d differ: %d elements" % (
        ld_big, ld_small, int((got[ld_big][0].view(np.uint32) != got[ld_small][0].view(np.uint32)).sum()))
    held("x_ld=%d %s" % (ld_big, got[ld_big][1]), got[ld_big][0], conv64(x, w, stride, pad) + b.astype(np.float64), BAR_PLAIN)


# ---- D: the residual's pixel stride at the limit ---------------------------------------------------------------------------------------
def pair_residual(case):
    """stabnet_conv_unit_pair_fwd, shapes of unit_pair_child.CASES"""
    from stabnet_amd import ops
    import unit_pair_child as upc
    N, K1, N1, N2, _, bias = upc.CASES[case]
    H, W = upc.H, upc.W
    d = upc.case_data(case)
    pixels = N * H * W
    ld_big, ld_small = largest_ld(pixels), N1 + 4
    r = d["r"][..., :N1]
    big = Big(pixels * ld_big)
    t = {k: dev(v) for k, v in d.items() if k != "r"}
    pv = dev(np.stack([d["ps"], d["pb"]]))                     # one buffer, the shifts behind the scales (conv.hip ring_pro_vectors_ok)
    rd = dev(r)
    got = {}
    for ld in (ld_big, ld_small):
        big.poison()
        view = big.t[:pixels * ld].view(N, H, W, ld)
        view[..., :N1] = rd
        q3, q1 = _poison.Poisoned(DEV, (N, H, W, N1)), _poison.Poisoned(DEV, (N, H, W, N2))
        ops.conv_unit_pair(t["x"], t["w3"], t["b3"], view, pv[0], pv[1], t["w1"], t["os"], t["ob"], True, out3=q3.out, out=q1.out)
        name = kind_name()
        y3, y1 = q3.result("conv3, res_ld=%d" % ld), q1.result("conv1, res_ld=%d" % ld)
        print("res_ld=%d (%.2f GB): %s" % (ld, 4e-9 * pixels * ld, name))
        assert "conv_unit_pair" in name, name
        big.check_bands("the residual buffer")
        assert big.count_not_nan() == pixels * N1 and same_bits(view[..., :N1].cpu().numpy(), r)
        got[ld] = (y3, y1, name)
    assert got[ld_big][2] == got[ld_small][2]
    assert same_bits(got[ld_big][0], got[ld_small][0]) and same_bits(got[ld_big][1], got[ld_small][1]), "res_ld=%d against res_ld=%d" % (ld_big, ld_small)
    f = lambda v: v.astype(np.float64)                         # noqa: E731
    y3 = f(d["x"]).reshape(-1, K1) @ f(d["w3"]).reshape(N1, K1).T + (f(d["b3"]) if bias else 0.0) + f(r).reshape(-1, N1)
    a = np.maximum(y3 * f(d["ps"]) + f(d["pb"]), 0.0)
    y1 = np.maximum((a @ f(d["w1"]).reshape(N2, N1).T) * f(d["os"]) + f(d["ob"]), 0.0)
    held("unit pair conv3, res_ld=%d" % ld_big, got[ld_big][0].reshape(-1, N1), y3, BAR_PLAIN)
    held("unit pair conv1, res_ld=%d" % ld_big, got[ld_big][1].reshape(-1, N2), y1, BAR_OUT_BN)


def b2b_residual(N, stride):
    """stabnet_conv3x3_conv1x1_fwd: the plain residual (stride 1) and the strided one (conv stride 2 reading the unit's input at (2 oy, 2 ox))"""
    from stabnet_amd import ops
    H, W, Cc, Cout = 9, 11, 64, 256
    rng = np.random.default_rng(40 + 2 * N + stride)
    x = np.maximum(rng.standard_normal((N, H, W, Cc)), 0).astype(np.float32)
    w2 = (rng.standard_normal((Cc, 3, 3, Cc)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
    ms, mb = rng.uniform(0.5, 1.5, Cc).astype(np.float32), (rng.standard_normal(Cc) * 0.3).astype(np.float32)
    w3 = (rng.standard_normal((Cout, 1, 1, Cc)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b3 = rng.standard_normal(Cout).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rH, rW = (H, W) if stride == 2 else (Ho, Wo)               # res_stride = stride: slim's subsample() shortcut
    r = rng.standard_normal((N, rH, rW, Cout)).astype(np.float32)
    pixels = N * rH * rW
    ld_big, ld_small = largest_ld(pixels), Cout + 4
    big = Big(pixels * ld_big)
    xd, w2d, msd, mbd, w3d, b3d, rd = (dev(v) for v in (x, w2, ms, mb, w3, b3, r))
    got = {}
    for ld in (ld_big, ld_small):
        big.poison()
        view = big.t[:pixels * ld].view(N, rH, rW, ld)
        view[..., :Cout] = rd
        out = _poison.Poisoned(DEV, (N, Ho, Wo, Cout))
        ops.conv3x3_conv1x1(xd, w2d, msd, mbd, w3d, b3d, residual=view, res_stride=stride, stride=stride, out=out.out)
        name = kind_name()
        y = out.result("res_ld=%d" % ld)
        print("res_ld=%d (%.2f GB): %s" % (ld, 4e-9 * pixels * ld, name))
        assert "b2b" in name, name
        big.check_bands("the residual buffer")
        assert big.count_not_nan() == pixels * Cout and same_bits(view[..., :Cout].cpu().numpy(), r)
        got[ld] = (y, name)
    assert got[ld_big][1] == got[ld_small][1]
    assert same_bits(got[ld_big][0], got[ld_small][0]), "res_ld=%d against res_ld=%d" % (ld_big, ld_small)
    mid = np.maximum(conv64(x, w2, stride, 1) * ms.astype(np.float64) + mb.astype(np.float64), 0.0)
    want = mid.reshape(-1, Cc) @ w3.astype(np.float64).reshape(Cout, Cc).T + b3.astype(np.float64)
    want = want.reshape(N, Ho, Wo, Cout) + r.astype(np.float64)[:, ::stride, ::stride][:, :Ho, :Wo]
    held("back-to-back, res_ld=%d" % ld_big, got[ld_big][0], want, BAR_PLAIN)


def strided_residual(N, H, W, Cin, Cout, k, packed, expect):
    """The residual's own size at the limit, through the epilogues that no entry gives a res_ld: a stride-1 convolution (1x1, or 3x3 / pad 1)
    + bias + a residual [N][2H][2W - 1][Cout] of 2^30 - 2^19 floats read at (2 oy, 2 ox) -- the strided form of the epilogues' m * res_ld
    (conv_kernel.h:96, conv_patch_kernel.h:76) -- beside an output a quarter of its size.  packed: stabnet_conv2d_fwd_packed (the parent sets
    STABNET_CONV_PATCH_MIN_M=1 for the patch kernel), else stabnet_conv2d_fwd_ex.  The twin launch reads the same values from a dense
    [N][H][W][Cout] residual with res_stride 1 (the plain form, :91 / :71): all output bits must agree."""
    from stabnet_amd import ops
    pad, rH, rW, M = k // 2, 2 * H, 2 * W - 1, N * H * W
    rn = N * rH * rW * Cout
    assert LIMIT - LIMIT // 1024 < rn < LIMIT, rn
    rng = np.random.default_rng(77 + Cin + k)
    w = (rng.standard_normal((Cout, k, k, Cin)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    x = torch.empty((N, H, W, Cin), dtype=torch.float32, device=DEV).uniform_(-1.0, 1.0, generator=gen)
    rb = Big(rn)
    rb.t.uniform_(-1.0, 1.0, generator=gen)
    r = rb.t.view(N, rH, rW, Cout)
    finger = rb.t.view(torch.int32)[::4097].clone()
    wd, bd = dev(w), dev(b)

    def launch(res, res_stride, out):
        if packed:
            ws = _poison.Poisoned(DEV, (1,), ops.conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, k, k, 1, pad, 1))
            ops.conv2d_packed(x, wd, bd, None, None, res, res_stride, 1, pad, False, splitk=1, out=out, workspace=ws.workspace)
        else:
            ws = _poison.Poisoned(DEV, (1,), ops.conv2d_workspace_bytes(N, H, W, Cin, Cout, k, k, 1, pad))
            ops.conv2d(x, wd, bd, None, None, res, res_stride, 1, pad, False, out=out, workspace=ws.workspace)
        torch.cuda.synchronize()
        return kind_name()

    yb = Big(M * Cout)
    y = yb.t.view(N, H, W, Cout)
    name = launch(r, 2, y)
    print("residual %d floats (%.2f GB) read with res_stride 2, M=%d: %s" % (rn, 4e-9 * rn, M, name))
    assert expect in name, "the launch took %s, not a %s kernel" % (name, expect)
    yb.check_bands("the output")
    assert yb.count_not_nan() == M * Cout, "%d outputs were never written" % (M * Cout - yb.count_not_nan())
    rb.check_bands("the residual")
    assert bool((rb.t.view(torch.int32)[::4097] == finger).all()), "the residual was written"
    # rows: the first and the last tile, the output rows whose residual pixel lies on both sides of byte offsets 2^31 and 3 * 2^30 of the
    # residual, 64 rows drawn with a fixed seed
    rows = set(range(64)) | set(range(M - 64, M)) | {int(v) for v in np.random.default_rng(5).integers(0, M, 64)}
    for off in (1 << 31, 3 << 30):
        pix = off // (4 * Cout)
        img, ry, rx = pix // (rH * rW), pix % (rH * rW) // rW, pix % rW
        m = (img * H + ry // 2) * W + min(rx // 2, W - 1)
        rows |= {v for v in range(m - 2, m + 3) if 0 <= v < M}
    rows = np.array(sorted(rows), np.int64)
    img, oy, ox = rows // (H * W), rows % (H * W) // W, rows % W
    ti = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    want = b.astype(np.float64) + r[ti(img), ti(2 * oy), ti(2 * ox)].cpu().numpy().astype(np.float64)
    below, above = False, False
    for off in (1 << 31, 3 << 30):
        byte = (((img * rH + 2 * oy) * rW + 2 * ox) * Cout) * 4
        below, above = below or bool((byte < off).any()), above or bool((byte >= off).any())
    assert below and above
    for kh in range(k):
        for kw in range(k):
            iy, ix = oy + kh - pad, ox + kw - pad
            ok = ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).astype(np.float64)[:, None]
            xt = x[ti(img), ti(np.clip(iy, 0, H - 1)), ti(np.clip(ix, 0, W - 1))].cpu().numpy().astype(np.float64) * ok
            want += xt @ w[:, kh, kw, :].astype(np.float64).T
    held("strided residual at the limit, %d rows, %s" % (len(rows), name), y.view(M, Cout)[ti(rows)].cpu().numpy(), want, BAR_PLAIN)
    # the twin: the same values from a dense residual
    r2 = r[:, ::2, ::2][:, :H, :W].contiguous()
    del r, rb
    torch.cuda.empty_cache()
    y2 = torch.full((N, H, W, Cout), float("nan"), dtype=torch.float32, device=DEV)
    name2 = launch(r2, 1, y2)
    assert name2 == name, (name, name2)
    differ = int((y.view(torch.int32) != y2.view(torch.int32)).sum())
    assert differ == 0, "the launch on the residual at the limit and its dense twin differ in %d elements" % differ


# ---- E, F: dense tensors at the limit (stabnet_conv2d_fwd_ex) ------------------------------------------------------------------------------
def dense(N, H, W, Cin, Cout, expect, big_is):
    """1x1: E (big_is = "input") M * Cin just inside the limit, F ("output") M * Cout just inside it"""
    from stabnet_amd import ops
    M = N * H * W
    assert LIMIT - max(Cin, Cout) <= M * (Cin if big_is == "input" else Cout) < LIMIT
    rng = np.random.default_rng(Cin * 1000 + Cout)
    w = (rng.standard_normal((Cout, 1, 1, Cin)) * np.sqrt(2.0 / Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    if big_is == "input":
        xb = Big(M * Cin)
        xb.t.uniform_(-1.0, 1.0, generator=gen)
        yb = Big(M * Cout)
        xs = xb.t.view(torch.int32)[::4097].clone()            # a fingerprint of the input: the launch must not write it
    else:
        xb = None
        xt = torch.empty(M * Cin, dtype=torch.float32, device=DEV).uniform_(-1.0, 1.0, generator=gen)
        yb = Big(M * Cout)
    x = (xb.t if xb is not None else xt).view(N, H, W, Cin)
    ws_bytes = ops.conv2d_workspace_bytes(N, H, W, Cin, Cout, 1, 1)
    ws = _poison.Poisoned(DEV, (1,), ws_bytes)
    t0 = time.time()
    ops.conv2d(x, dev(w), dev(b), out=yb.t.view(N, H, W, Cout), workspace=ws.workspace)
    torch.cuda.synchronize()
    name = kind_name()
    print("%s at the limit, M=%d Cin=%d Cout=%d: %s (%.2f s)" % (big_is, M, Cin, Cout, name, time.time() - t0))
    assert expect in name, "the launch took %s, not a %s kernel" % (name, expect)
    yb.check_bands("the output")
    assert yb.count_not_nan() == M * Cout, "%d outputs were never written" % (M * Cout - yb.count_not_nan())
    if xb is not None:
        xb.check_bands("the input")
        assert bool((xb.t.view(torch.int32)[::4097] == xs).all()), "the input was written"
    rows = edge_rows(M, Cin if big_is == "input" else Cout, 5)
    idx = torch.from_numpy(rows).to(DEV)
    xr = x.view(M, Cin)[idx].cpu().numpy().astype(np.float64)
    got = yb.t.view(M, Cout)[idx].cpu().numpy()
    held("%s at the limit, %d rows, %s" % (big_is, len(rows), name), got, xr @ w.astype(np.float64).reshape(Cout, Cin).T + b.astype(np.float64), BAR_PLAIN)


# ---- G: one accepted plan end to end ----------------------------------------------------------------------------------------------------
def plan_end_to_end():
    import json
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import Regressor
    H, W = 1080, 1920
    with open(es.GOLDEN) as fh:
        N = json.load(fh)["inference"]["%dx%d" % (H, W)]["mode4_pairs"]
    cfg = Config(height=H, width=W)
    # what this case is relied on for, asserted from the plan's own step info (host only) before anything runs
    buf = N * (H // 4) * (W // 4) * 320                      # block 1's merged shortcut | conv1 buffer
    assert 0.96 * LIMIT < buf < LIMIT
    for mode, pairs in ((0, 0), (4, 1)):
        p, msg = es.make_plan(mode, N, H, W, pairs)
        assert p is not None, msg
        rows = [p.info(i) for i in range(p.num_steps)]
        rows = [r for r in rows if r["kind"] in (ex.S_CONV, ex.S_CONV_PAIR)]
        at_x = sorted({r["family"] for r in rows if r["x_ld"] == 320 and r["in_base"] + r["in_floats"] - r["in_off"] == buf - 256})
        at_r = sorted({r["family"] for r in rows if r["res_off"] >= 0 and r["res_ld"] == 320 and r["res_floats"] == buf})
        stem = [r for r in rows if r["rowrun"]]
        print("mode %d: families reading x_ld = 320 at %.3f of the limit %s, res_ld = 320 %s; fused pairs %d" % (
            mode, buf / LIMIT, at_x, at_r, sum(r["kind"] == ex.S_CONV_PAIR for r in rows)))
        assert len(stem) == 1 and stem[0]["family"] in ex.RING_LIKE and stem[0]["mode"] == 2
        if mode == 0:
            assert at_x == [ex.FAMILY_RING], at_x            # the exact-f32 ring kernel (MODE 1) on a strided input at the limit
            assert at_r == [ex.FAMILY_IGEMM], at_r           # the register-staged epilogue's plain m * res_ld at the limit
        else:
            assert at_x and set(at_x) <= {ex.FAMILY_PACKED, ex.FAMILY_PACKED_KG2, ex.FAMILY_PATCH}, at_x
            assert at_r, at_r
            assert any(r["kind"] == ex.S_CONV_PAIR for r in rows)
        p.close()
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    who = [0, N // 2, N - 1]
    frames = [torch.from_numpy(np.random.default_rng(90 + i).uniform(-0.5, 0.5, (1, H, W, cfg.in_ch)).astype(np.float32)).to(DEV) for i in range(3)]
    single = {}
    for mode in (4, 0):
        reg = Regressor(P, 1, H, W, cfg, device=DEV, operand_mode=mode, fuse_unit_pairs=True)
        single[mode] = np.concatenate([reg(f).cpu().numpy() for f in frames])
        del reg
    x = torch.empty((N, H, W, cfg.in_ch), dtype=torch.float32, device=DEV)
    for i in range(N):
        x[i] = frames[who.index(i) if i in who else i % 3][0]
    dist = {}
    for mode in (4, 0):
        t0 = time.time()
        reg = Regressor(P, N, H, W, cfg, device=DEV, operand_mode=mode, fuse_unit_pairs=True)
        reg.workspace[:reg.workspace.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))   # no region may be read before it is written
        theta = reg(x).cpu().numpy()
        assert np.isfinite(theta).all(), "mode %d: theta of the batch of %d is not finite" % (mode, N)
        dist[mode] = float(np.abs(theta[who] - single[mode]).max())
        print("mode %d, N=%d, workspace %.2f GB, %.1f s" % (mode, N, 1e-9 * reg.workspace.numel(), time.time() - t0))
        del reg
        torch.cuda.empty_cache()
    print("MEASURED N=%d %dx%d rows %s against the single-sample forward: mode 4 %.3e, mode 0 %.3e" % (N, H, W, who, dist[4], dist[0]))
    assert dist[0] <= 2e-6, dist
    assert dist[4] <= 2e-6 or dist[4] <= 2 * dist[0] + 1e-7, dist


CASES = {
    "A": lambda: strided_input(1, 64, 64, 64, 64, 1, 1, 0, "conv_ring_f32_kernel<0, 4"),
    "B64": lambda: strided_input(2, 40, 40, 64, 64, 3, 1, 1, "conv_ring_f32_kernel<1, 4"),
    "B128": lambda: strided_input(2, 40, 40, 128, 128, 3, 1, 1, "conv_ring_f32_kernel<1, 4"),
    "B64patch": lambda: strided_input(2, 40, 40, 64, 64, 3, 1, 1, "conv_patch"),          # (the parent sets STABNET_CONV_PATCH_MIN_M=1)
    "B128patch": lambda: strided_input(2, 40, 40, 128, 128, 3, 1, 1, "conv_patch"),
    "C": lambda: strided_input(2, 41, 41, 64, 64, 3, 2, 1, "conv_ring_f32_kernel<1, 4"),
    "Dpair0": lambda: pair_residual(0), "Dpair3": lambda: pair_residual(3), "Dpair5": lambda: pair_residual(5), "Dpair4": lambda: pair_residual(4),
    "Db2b1": lambda: b2b_residual(1, 1), "Db2b2": lambda: b2b_residual(2, 1), "Db2b1s": lambda: b2b_residual(1, 2), "Db2b2s": lambda: b2b_residual(2, 2),
    # residual [2][2H][2W - 1][Cout] = 2^30 - 2^19 floats: register-staged (K = 16), ring (K = 32), both patch forms and the packed ring
    "Dres16": lambda: strided_residual(2, 512, 1024, 16, 256, 1, False, "conv_igemm"),
    "Dres32": lambda: strided_residual(2, 512, 1024, 32, 256, 1, False, "conv_ring_f32_kernel<0, 0"),
    "Dres64patch": lambda: strided_residual(2, 2048, 1024, 64, 64, 3, True, "conv_patch_f32_kernel<8, 8, 1"),
    "Dres128patch": lambda: strided_residual(2, 1024, 1024, 128, 128, 3, True, "conv_patch_f32_kernel<8, 8, 2"),
    "Dres64packed": lambda: strided_residual(2, 2048, 1024, 64, 64, 3, True, "conv_ring_f32_kernel<1, 4"),
    "E": lambda: dense(3, 2731, 8191, 16, 4, "conv_igemm", "input"),
    "F16": lambda: dense(3, 2047, 683, 16, 256, "conv_igemm", "output"),
    "F32": lambda: dense(3, 2047, 683, 32, 256, "conv_ring", "output"),
    "G": plan_end_to_end,
}

if __name__ == "__main__":
    bars()
    t_start = time.time()
    CASES[sys.argv[1]]()
    torch.cuda.synchronize()
    print("case %s ok in %.1f s" % (sys.argv[1], time.time() - t_start))
