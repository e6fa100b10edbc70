"""Grid independence of the persistent LDS-DMA ring kernels (conv_ring_f32_kernel<MODE, B, KG, PRO>, conv.hip launch_ring_route).

The grid is min(tiles, workgroups per CU x usable CUs); a workgroup walks tiles t_first, t_first + t_stride, ... < t_end with its
ring, its step count and the XCD range split running across tile boundaries (conv_ring_kernel.h).  On a whole MI355X the usable CU
count is always 256, so small shapes run one tile per workgroup and grids that are no multiple of 8 never run at all.
stabnet_conv_reserve_cus (read at launch time) is the lever: every case runs with U = all, 37 and CUs / 8 usable CUs.  The grid only
decides WHICH workgroup computes a tile, never the order of a tile's K sum: the three results must be bit-identical, on top of the
oracle bars of test_conv_gpu.py / test_conv_packed_gpu.py.  Every output is a freshly poisoned caller-owned buffer (_poison.py): a
tile no workgroup writes stays NaN instead of keeping the previous run's values.

Every instantiation launch_ring_operand has for the f32 (B = 0) and packed (B = 4) operands is here in two tile-count classes,
asserted from T and G: G < T < 2G, and T >= 3G + 1 with T % G != 0 -- except MODE 2 (the row-run stem), which no operator reaches:
test_conv_grid_net_gpu.py runs it inside the regressor, at one size per class.  Which kernel a case ran is the launch's own answer
(stabnet_conv_last_launch_kind), asserted after every launch.  The same sweep follows for the other launches sized from the usable CUs
that need no per-process switch: conv_b2b_f32_kernel<2 | 4> (both classes) and dgrad, plain and with split operands (class a); the
N groups of the A-stationary and patch kernels are swept by the children of test_conv_astat_gpu.py / test_conv_patch_gpu.py."""
import numpy as np
import pytest
import torch

import _poison
from _grid import cdiv, check_tile_classes, launched_kernel, reservation  # noqa: F401  (reservation: a fixture)
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu

RING_WGS_PER_CU, PACKED_WGS_PER_CU = 3, 2      # the defaults of conv.hip's ConvSwitches (no STABNET_CONV_* variable is set)

# name, kernel, packed, workgroups per CU, Cin, k, stride, pad, prologue, splitk, slabs, Cout, bias, residual, relu, out_bn
# M = 2500 rows everywhere (50 x 50 outputs): 40 M tiles, the last of 4 rows; every Cout is ragged in its last 64-column tile
CASES = [
    # ---- exact f32 (ops.conv2d under stabnet_conv_tuning_override(2, splitk))
    ("f32_m0_a", "<0, 0, 1, 0>", 0, 3, 32, 1, 1, 0, 0, 1, 1, 180, 1, 1, 0, 0),      # one-step tiles: every step is a tile boundary
    ("f32_m0_b", "<0, 0, 1, 0>", 0, 3, 128, 1, 1, 0, 0, 1, 1, 564, 0, 0, 1, 1),
    ("f32_m1_a", "<1, 0, 1, 0>", 0, 3, 32, 3, 1, 1, 0, 1, 1, 180, 0, 1, 1, 0),
    ("f32_m1_b", "<1, 0, 1, 0>", 0, 3, 32, 3, 2, 1, 0, 1, 1, 564, 1, 0, 0, 0),      # stride 2
    ("f32_pro_a", "<0, 0, 1, 1>", 0, 3, 128, 1, 1, 0, 1, 1, 1, 180, 1, 1, 1, 0),    # (an output BN would move it to the register-staged kernel)
    ("f32_pro_b", "<0, 0, 1, 1>", 0, 3, 64, 1, 1, 0, 1, 1, 1, 564, 0, 0, 0, 0),
    ("f32_pro_kg2_a", "<0, 0, 2, 1>", 0, 1, 64, 1, 1, 0, 1, 2, 1, 60, 0, 0, 1, 1),
    ("f32_pro_kg2_b", "<0, 0, 2, 1>", 0, 1, 128, 1, 1, 0, 1, 2, 1, 180, 1, 1, 0, 0),
    ("f32_kg3_m0_a", "<0, 0, 3, 0>", 0, 1, 96, 1, 1, 0, 0, 3, 1, 60, 1, 0, 0, 0),
    ("f32_kg3_m0_b", "<0, 0, 3, 0>", 0, 1, 192, 1, 1, 0, 0, 3, 1, 180, 0, 1, 1, 1),
    ("f32_kg3_m1_a", "<1, 0, 3, 0>", 0, 1, 32, 3, 1, 1, 0, 3, 1, 60, 0, 1, 0, 1),
    ("f32_kg3_m1_b", "<1, 0, 3, 0>", 0, 1, 32, 3, 1, 1, 0, 3, 1, 180, 1, 0, 1, 0),
    ("f32_slab_a", "<0, 0, 1, 0>", 0, 3, 512, 1, 1, 0, 0, 3, 3, 60, 1, 1, 1, 0),     # 16 steps in slices of 6, 6, 4 + the reduce launch
    ("f32_slab_b", "<0, 0, 1, 0>", 0, 3, 512, 1, 1, 0, 0, 3, 3, 180, 0, 0, 0, 1),
    # ---- packed split (ops.conv2d_packed, splitk=)
    ("pk_m0_a", "<0, 4, 1, 0>", 1, 2, 32, 1, 1, 0, 0, 1, 1, 116, 1, 1, 0, 0),
    ("pk_m0_b", "<0, 4, 1, 0>", 1, 2, 128, 1, 1, 0, 0, 1, 1, 372, 0, 0, 1, 1),
    ("pk_m1_a", "<1, 4, 1, 0>", 1, 2, 32, 3, 1, 1, 0, 1, 1, 116, 0, 1, 1, 0),
    ("pk_m1_b", "<1, 4, 1, 0>", 1, 2, 32, 3, 2, 1, 0, 1, 1, 372, 1, 0, 0, 0),       # stride 2
    ("pk_pro_a", "<0, 4, 1, 1>", 1, 2, 128, 1, 1, 0, 1, 1, 1, 116, 1, 1, 1, 1),
    ("pk_pro_b", "<0, 4, 1, 1>", 1, 2, 256, 1, 1, 0, 1, 1, 1, 372, 0, 0, 0, 0),
    ("pk_kg2_m0_a", "<0, 4, 2, 0>", 1, 1, 128, 1, 1, 0, 0, 2, 1, 60, 1, 0, 0, 0),
    ("pk_kg2_m0_b", "<0, 4, 2, 0>", 1, 1, 192, 1, 1, 0, 0, 2, 1, 180, 0, 1, 1, 1),
    ("pk_kg2_m1_a", "<1, 4, 2, 0>", 1, 1, 64, 3, 1, 1, 0, 2, 1, 60, 0, 1, 0, 1),
    ("pk_kg2_m1_b", "<1, 4, 2, 0>", 1, 1, 64, 3, 1, 1, 0, 2, 1, 180, 1, 0, 1, 0),   # (an even step count: equal halves)
    ("pk_kg2_pro_a", "<0, 4, 2, 1>", 1, 1, 128, 1, 1, 0, 1, 2, 1, 60, 0, 0, 1, 0),
    ("pk_kg2_pro_b", "<0, 4, 2, 1>", 1, 1, 64, 1, 1, 0, 1, 2, 1, 180, 1, 1, 0, 1),
    ("pk_slab_a", "<0, 4, 1, 0>", 1, 2, 512, 1, 1, 0, 0, 3, 3, 60, 1, 1, 1, 0),
    ("pk_slab_b", "<0, 4, 1, 0>", 1, 2, 512, 1, 1, 0, 0, 3, 3, 116, 0, 0, 0, 1),
]



@pytest.mark.parametrize("name,kernel,packed,per_cu,Cin,k,stride,pad,prologue,splitk,slabs,Cout,bias,res,relu,out_bn", CASES,
                         ids=[c[0] for c in CASES])
def test_ring_results_do_not_depend_on_the_grid(cuda, reservation, name, kernel, packed, per_cu, Cin, k, stride, pad, prologue, splitk, slabs,
                                                Cout, bias, res, relu, out_bn):
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    cus, grids = reservation
    N, Ho, Wo = 1, 50, 50
    H = W = (Ho - 1) * stride + k - 2 * pad
    M = N * Ho * Wo
    assert per_cu == (1 if splitk > 1 and slabs == 1 else (PACKED_WGS_PER_CU if packed else RING_WGS_PER_CU))
    T = cdiv(M, 64) * cdiv(Cout, 64) * slabs
    assert M % 64 != 0 and Cout % 64 != 0                       # ragged last M tile and last Cout tile
    table = check_tile_classes(name[-1], T, per_cu, [u for u, _ in grids[1:]], name)
    assert T < per_cu * cus or cus != 256                       # the unreserved run is the one-tile-per-workgroup baseline on a whole card

    rng = np.random.default_rng(Cin * 7 + Cout + k + 13 * splitk + packed)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32) if bias else None
    sc = rng.uniform(0.5, 1.5, Cin).astype(np.float32) if prologue else None
    sh = (rng.standard_normal(Cin) * 0.3).astype(np.float32) if prologue else None
    a = x if not prologue else np.maximum(x * sc + sh, 0).astype(np.float32)
    want = O.conv2d(a, w, stride, ((pad, pad), (pad, pad)), b)
    assert want.shape == (N, Ho, Wo, Cout)
    r = None
    if res:
        r = rng.standard_normal(want.shape).astype(np.float32)
        want = want + r
    osc = osh = None
    if out_bn:
        osc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
        osh = (rng.standard_normal(Cout) * 0.3).astype(np.float32)
        want = (want * osc + osh).astype(np.float32)
    if relu:
        want = np.maximum(want, 0)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(cuda)
    ss = t(np.concatenate([sc, sh])) if prologue else None      # (the prologue kernels address the shifts relative to the scales)
    tsc, tsh = (ss[:Cin], ss[Cin:]) if prologue else (None, None)
    args = (t(x), t(ops.pack_conv_weight(w)), t(b), tsc, tsh, t(r), 1, stride, pad, bool(relu))
    kw = dict(out_scale=t(osc), out_shift=t(osh))

    got = {}
    f32 = None
    if packed:
        f32 = ops.conv2d(*args, **kw).cpu().numpy()             # the exact-f32 kernels, planned, unreserved
        kind = L.stabnet_conv2d_packed_kind(N, H, W, Cin, Cout, k, k, stride, pad, prologue, splitk)
        assert L.stabnet_prof_kind_name(kind).decode() == "conv_ring_f32_kernel" + kernel, name
        ws_bytes = ops.conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, k, k, stride, pad, splitk)
    try:
        if not packed:
            L.stabnet_conv_tuning_override(2, splitk)           # the 64 x 64 tile, `splitk` K slices
            ws_bytes = ops.conv2d_workspace_bytes(N, H, W, Cin, Cout, k, k, stride, pad)
        assert (ws_bytes >= slabs * M * Cout * 4) if slabs > 1 else True
        for U, reserved in grids:
            L.stabnet_conv_reserve_cus(reserved)
            if packed:
                got[U] = _poison.run(cuda, ops.conv2d_packed, want.shape, ws_bytes, *args, splitk=splitk, what="%s U=%d" % (name, U), **kw)
            else:
                got[U] = _poison.run(cuda, ops.conv2d, want.shape, ws_bytes, *args, what="%s U=%d" % (name, U), **kw)
            # the kernel the launch itself chose with its pointers bound: T and G above describe this kernel's grid
            assert launched_kernel(L) == "conv_ring_f32_kernel" + kernel, (name, U)
    finally:
        L.stabnet_conv_tuning_override(-1, -1)
        L.stabnet_conv_reserve_cus(0)
    print("conv_ring_f32_kernel%s%s: (U, T, G) = %s" % (kernel, " + reduce" if slabs > 1 else "", [(cus, T, min(T, per_cu * cus))] + table))

    scale = np.abs(want).max()
    for U, g in got.items():
        err = np.abs(g - want).max()
        assert err <= (4e-5 if out_bn else 2e-5) * scale, "U=%d: max err vs oracle %g (scale %g)" % (U, err, scale)
        if packed:
            d = np.abs(g - f32).max()
            assert d <= 4e-6 * scale, "U=%d: max difference to the exact-f32-MFMA kernels %g (scale %g)" % (U, d, scale)
    base = got[cus]
    for U, g in got.items():
        diff = base.view(np.uint32) != g.view(np.uint32)
        assert not diff.any(), "U=%d against U=%d: %d elements differ, first rows %s" % (
            U, cus, int(diff.sum()), np.unique(np.argwhere(diff.reshape(-1, Cout))[:, 0])[:8])


def test_reserve_cus_returns_the_previous_value_and_floors(cuda, reservation):
    """stabnet_conv_reserve_cus: returns the previous value, stores 0 for a negative one, and any value from CUs - CUs / 8 on gives
    the grid of the CUs / 8 floor -- the same bits, and the same bits as no reservation."""
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    cus, _ = reservation
    assert L.stabnet_conv_reserve_cus(5) == 0
    assert L.stabnet_conv_reserve_cus(-3) == 5
    assert L.stabnet_conv_reserve_cus(7) == 0                   # the negative value stored 0
    assert L.stabnet_conv_reserve_cus(0) == 7
    # 40 x 3 tiles on the f32 ring kernel: 96 workgroups at the floor of a 256-CU card
    N, H, W, Cin, Cout = 1, 50, 50, 128, 180
    rng = np.random.default_rng(41)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((1, 1, Cin, Cout)) * np.sqrt(2.0 / Cin)).astype(np.float32)
    want = O.conv2d(x, w, 1, ((0, 0), (0, 0)), None)
    xt, wt = torch.from_numpy(x).to(cuda), torch.from_numpy(ops.pack_conv_weight(w)).to(cuda)
    got = {}
    try:
        L.stabnet_conv_tuning_override(2, 1)
        for reserved in (0, cus - cus // 8, cus, 1 << 30):
            assert L.stabnet_conv_reserve_cus(reserved) in (0, cus - cus // 8, cus)
            got[reserved] = _poison.run(cuda, ops.conv2d, want.shape, 0, xt, wt, what="reserved %d" % reserved)
            assert launched_kernel(L) == "conv_ring_f32_kernel<0, 0, 1, 0>"
    finally:
        L.stabnet_conv_tuning_override(-1, -1)
        L.stabnet_conv_reserve_cus(0)
    assert np.abs(got[0] - want).max() <= 2e-5 * np.abs(want).max()
    for reserved, g in got.items():
        assert np.array_equal(got[0].view(np.uint32), g.view(np.uint32)), reserved


# ---- conv2 (3x3) -> conv3 (1x1) back to back (conv_b2b_kernel.h): grids of 2 x usable CUs (<2>, C = 64) and usable CUs (<4>, C = 128)
# name, kernel, workgroups per CU, H = W, C, Cout, bias, residual, relu, out_bn
B2B_CASES = [
    ("b2b2_a", "<2>", 2, 70, 64, 256, 1, 1, 0, 0),           # 77 tiles of 64 rows (the last of 36)
    ("b2b2_b", "<2>", 2, 121, 64, 256, 0, 0, 1, 1),          # 229 tiles (the last of 49 rows)
    ("b2b4_a", "<4>", 1, 50, 128, 512, 1, 1, 1, 0),          # 40 tiles (the last of 4 rows)
    # 119 tiles (the last of 17 rows).  Its oracle costs 3.2 GFLOP, above the 1 GFLOP the other cases keep to: class b of <4> needs
    # 3 x 37 + 1 = 112 tiles of 64 rows at C = 128, Cout = 512, the smallest geometry the kernel takes
    ("b2b4_b", "<4>", 1, 87, 128, 512, 0, 1, 0, 1),
]


@pytest.mark.parametrize("name,kernel,per_cu,HW,C,Cout,bias,res,relu,out_bn", B2B_CASES, ids=[c[0] for c in B2B_CASES])
def test_b2b_results_do_not_depend_on_the_grid(cuda, reservation, name, kernel, per_cu, HW, C, Cout, bias, res, relu, out_bn):
    """conv_b2b_f32_kernel<2 | 4>: bit-identical for every grid and with the two-launch form (test_conv_gpu.py's bars and comparison)."""
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    cus, grids = reservation
    N = 1
    M = N * HW * HW
    T = cdiv(M, 64)
    assert M % 64 != 0 and (C == 64) == (kernel == "<2>")
    table = check_tile_classes(name[-1], T, per_cu, [u for u, _ in grids[1:]], name)
    rng = np.random.default_rng(C * 11 + Cout + HW)
    x = rng.standard_normal((N, HW, HW, C)).astype(np.float32)
    w2 = (rng.standard_normal((3, 3, C, C)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    w3 = (rng.standard_normal((1, 1, C, Cout)) * np.sqrt(2.0 / C)).astype(np.float32)
    b3 = rng.standard_normal(Cout).astype(np.float32) if bias else None
    msc = rng.uniform(0.5, 1.5, C).astype(np.float32)
    msh = (rng.standard_normal(C) * 0.3).astype(np.float32)
    mid = np.maximum(O.conv2d(x, w2, 1, ((1, 1), (1, 1)), None) * msc + msh, 0).astype(np.float32)
    want = O.conv2d(mid, w3, 1, ((0, 0), (0, 0)), b3)
    r = None
    if res:
        r = rng.standard_normal(want.shape).astype(np.float32)
        want = want + r
    osc = osh = None
    if out_bn:
        osc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
        osh = (rng.standard_normal(Cout) * 0.3).astype(np.float32)
        want = (want * osc + osh).astype(np.float32)
    if relu:
        want = np.maximum(want, 0)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(cuda)
    W2, W3 = t(ops.pack_conv_weight(w2)), t(ops.pack_conv_weight(w3))
    args = (t(x), W2, t(msc), t(msh), W3, t(b3), t(r), 1, 1, bool(relu), t(osc), t(osh))
    got = {}
    try:
        for U, reserved in grids:
            L.stabnet_conv_reserve_cus(reserved)
            got[U] = _poison.run(cuda, ops.conv3x3_conv1x1, want.shape, None, *args, what="%s U=%d" % (name, U))
            assert launched_kernel(L) == "conv_b2b_f32_kernel" + kernel, (name, U)
        L.stabnet_conv_reserve_cus(0)
        L.stabnet_conv_tuning_override(2, 1)                    # the two-launch form, K unsplit: the same products in the same order
        mid_g = ops.conv2d(t(x), W2, None, None, None, None, 1, 1, 1, True, out_scale=t(msc), out_shift=t(msh))
        two = ops.conv2d(mid_g, W3, t(b3), None, None, t(r), 1, 1, 0, bool(relu), out_scale=t(osc), out_shift=t(osh)).cpu().numpy()
    finally:
        L.stabnet_conv_tuning_override(-1, -1)
        L.stabnet_conv_reserve_cus(0)
    print("conv_b2b_f32_kernel%s: (U, T, G) = %s" % (kernel, [(cus, T, min(T, per_cu * cus))] + table))
    scale = np.abs(want).max()
    for U, g in got.items():
        assert np.abs(g - want).max() <= (6e-5 if out_bn else 3e-5) * scale, (U, np.abs(g - want).max() / scale)
        assert np.array_equal(g.view(np.uint32), got[cus].view(np.uint32)), "U=%d against U=%d" % (U, cus)
        assert np.array_equal(g.view(np.uint32), two.view(np.uint32)), "U=%d against the two launches" % U


# ---- dgrad through the forward kernels (conv_bwd.hip dgrad_launch -> conv_launch): the convolution of dy [M = N H W rows, Cout
# channels] with the re-packed weights into Cin columns.  Unsplit (tuning override), no prologue, Cout % 32 == 0 and not the dense
# 64-channel 1x1 shape: the f32 ring kernel (3 workgroups per CU), the packed one with split operands (2 per CU) -- asserted from
# the launch's own route.  120 tiles are
# between G and 2G for both: 111 / 96 and 74 / 64.
# name, split, kernel the launch must take, workgroups per CU, Cin, Cout, k, pad
DGRAD_CASES = [
    ("dgrad_3x3_a", 0, "<1, 0, 1, 0>", 3, 180, 32, 3, 1),
    ("dgrad_1x1_a", 0, "<0, 0, 1, 0>", 3, 180, 128, 1, 0),
    ("dgrad_split_3x3_a", 1, "<1, 4, 1, 0>", 2, 180, 32, 3, 1),
    ("dgrad_split_1x1_a", 1, "<0, 4, 1, 0>", 2, 180, 128, 1, 0),
]


@pytest.mark.parametrize("name,split,kernel,per_cu,Cin,Cout,k,pad", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_dgrad_results_do_not_depend_on_the_grid(cuda, reservation, name, split, kernel, per_cu, Cin, Cout, k, pad):
    import torch.nn.functional as Fnn
    from stabnet_amd import _lib, ops
    L = _lib.lib()
    cus, grids = reservation
    N, H, W = 1, 50, 50
    T = cdiv(N * H * W, 64) * cdiv(Cin, 64)
    assert (N * H * W) % 64 != 0 and Cin % 64 != 0
    table = check_tile_classes(name[-1], T, per_cu, [u for u, _ in grids[1:]], name)
    rng = np.random.default_rng(Cin + Cout + k)
    w = rng.standard_normal((Cout, k, k, Cin)) * np.sqrt(2.0 / (k * k * Cin))
    g = rng.standard_normal((N, H, W, Cout))
    res = rng.standard_normal((N, H, W, Cin))
    xt = torch.zeros((N, H, W, Cin), dtype=torch.float64, requires_grad=True)
    y = Fnn.conv2d(xt.permute(0, 3, 1, 2), torch.tensor(w).permute(0, 3, 1, 2), stride=1, padding=pad).permute(0, 2, 3, 1)
    (y * torch.tensor(g)).sum().backward()
    want = xt.grad.numpy() + res                                # torch CPU float64 autograd (test_conv_bwd_gpu.py)
    f = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float32, device=cuda)
    op = ops.conv2d_dgrad_split if split else ops.conv2d_dgrad
    got = {}
    try:
        L.stabnet_conv_tuning_override(2, 1)
        ws_bytes = ops.conv2d_dgrad_workspace_bytes((N, H, W, Cin), w.shape, 1, pad, split=bool(split))
        for U, reserved in grids:
            L.stabnet_conv_reserve_cus(reserved)
            buf = _poison.Poisoned(cuda, (N, H, W, Cin), ws_bytes)
            ret = op(f(g), f(w), (N, H, W, Cin), 1, pad, residual=f(res), out=buf.out, workspace=buf.workspace)
            if split:
                assert ret[1], "conv_route() kept this dgrad on the exact-f32 kernels"
            assert launched_kernel(L) == "conv_ring_f32_kernel" + kernel, (name, U)       # the kernel whose grid T and G describe
            got[U] = buf.result("%s U=%d" % (name, U))
    finally:
        L.stabnet_conv_tuning_override(-1, -1)
        L.stabnet_conv_reserve_cus(0)
    print("%s: (U, T, G) = %s" % (name, [(cus, T, min(T, per_cu * cus))] + table))
    for U, d in got.items():
        assert np.abs(d - want).max() <= 2e-5 * np.abs(want).max(), U
        assert np.array_equal(d.view(np.uint32), got[cus].view(np.uint32)), "U=%d against U=%d" % (U, cus)
