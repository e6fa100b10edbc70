"""GPU: convolution backward in the forms a backward stage of the training step runs (run_backward_stage, net.hip), operator by
operator against torch CPU float64 autograd and, where the arithmetic is the same, bit for bit against the stand-alone operators:

  * wgrad over T = 2 towers in one launch (grid.z = tower x split, slabs [tower][split], the fused bias sums into two destinations),
  * ONE reduce table and slab cursor over several layers: wgrad_reduce4_kernel, the flat wgrad_reduce_kernel, the mid-table flush,
  * the table forms of the dgrad weight re-pack (32 x 32 LDS tiles / element-wise, kperm) and of the three-term bf16 weight image,
  * dgrad on the packed split kernels (operand mode 4), residual == dx included, and its exact-f32 fallbacks.

Every tower draws its own x, dy, scales and shifts; dw and d_bias are seeded with random values and `got - seed` is checked;
outputs and workspaces sit between canary bands (tests/_guarded.py), the workspaces at exactly the queried size.  The float64
models are themselves held to autograd by test_conv_bwd_models_cpu.py.

The step's dgrad asks conv_route() for the packed split kernel on every launch that carries a weight image, the two-step 1x1
launches over 64 channels included (conv.h, lowk_ring), so every stride-1 dgrad case with an image must report the packed route.
"""
import functools

import numpy as np
import pytest
import torch

import conv_bwd_models as M
from _guarded import CANARY, Guarded, _check_all, _same_bits

pytestmark = pytest.mark.gpu


def _dev(cuda, v):
    return None if v is None else torch.tensor(np.asarray(v, dtype=np.float32)).to(cuda)    # (a copy: the cached data are read-only)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- wgrad ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _layer(spec, T, seed):
    """float32 data of T towers, each drawn on its own, and the float64 reference (dW, d_bias) summed over the towers."""
    N, H, W, Cin, Cout, k, stride, pad, pro = spec
    rng = np.random.default_rng(seed)
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    towers = []
    for _ in range(T):
        towers.append(_frozen(rng.standard_normal((N, H, W, Cin)).astype(np.float32),
                              rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32),
                              rng.uniform(0.5, 1.5, Cin).astype(np.float32) if pro else None,
                              (rng.standard_normal(Cin) * 0.3).astype(np.float32) if pro else None))
    want_w, want_b = _frozen(*M.towers_wgrad(towers, (Cout, k, k, Cin), stride, pad))
    return tuple(towers), want_w, want_b


def _w_shape(spec):
    return (spec[4], spec[5], spec[5], spec[3])


def _geom(spec):
    N, H, W, Cin, Cout, k, stride, pad, _ = spec
    return (N, H, W, Cin, Cout, k, k, stride, pad)


def _float64_bar(spec, T, want):
    """the project's wgrad bar (test_conv_bwd_gpu.py) over the T * M pixels the sum runs over"""
    N, H, W, _, _, k, stride, pad, _ = spec
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    return 2e-5 * np.abs(want).max() * np.sqrt(T * N * Ho * Wo / 64 + 1)


def _seeds(spec, nbias, seed, zero=False):
    rng = np.random.default_rng(seed)
    Cout = spec[4]
    draw = (lambda n: np.zeros(n, np.float32)) if zero else (lambda n: rng.standard_normal(n).astype(np.float32))
    return [draw(int(np.prod(_w_shape(spec))))] + [draw(Cout) for _ in range(nbias)]


GAP = 4                                                     # floats between two destinations (keeps them 16-byte aligned)


def _wgrad_layers(cuda, entries):
    """entries: [(spec, towers, seeds)], seeds = [dw seed, d_bias seed, second d_bias seed][:1 + number of biases].  One call of
    stabnet_conv2d_wgrad_layers over one guarded gradient buffer (destinations GAP floats apart) and a guarded workspace of exactly
    the queried size -> per layer the destinations' contents after the call.  Everything around the destinations must be unchanged."""
    from stabnet_amd import ops
    offs, off = [], GAP
    for spec, _, seeds in entries:
        o = []
        for s in seeds:
            o.append(off)
            off += s.size + GAP
        offs.append(o)
    rng = np.random.default_rng(off)
    init = rng.standard_normal(off).astype(np.float32)
    for (_, _, seeds), o in zip(entries, offs):
        for s, at in zip(seeds, o):
            init[at:at + s.size] = s
    grads = Guarded(cuda, off, init=init)
    layers, keep = [], []
    for (spec, towers, seeds), o in zip(entries, offs):
        tw = [tuple(_dev(cuda, v) for v in t) for t in towers]
        keep.append(tw)
        layers.append((_geom(spec), tw, o[0], o[1] if len(o) > 1 else None, o[2] if len(o) > 2 else None))
    nbytes = ops.conv2d_wgrad_layers_workspace_bytes(layers)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded(cuda, nbytes // 4)                          # NaN: a slab that is read without having been written shows
    ops.conv2d_wgrad_layers(layers, grads.t, ws.t)
    _check_all({"grads": grads, "workspace": ws})
    got = grads.np()
    rest = np.ones(off, bool)
    out = []
    for (_, _, seeds), o in zip(entries, offs):
        out.append([got[at:at + s.size] for s, at in zip(seeds, o)])
        for s, at in zip(seeds, o):
            rest[at:at + s.size] = False
    assert _same_bits(got[rest], init[rest]), "the call wrote between its destinations"
    return out


def _single_tower_sum(cuda, spec, towers):
    """sum of the stand-alone operator's zero-seeded gradients of each tower (float32)"""
    from stabnet_amd import ops
    _, _, _, _, _, _, stride, pad, _ = spec
    parts = [ops.conv2d_wgrad(_dev(cuda, x), _dev(cuda, dy), _w_shape(spec), _dev(cuda, sc), _dev(cuda, sh), stride, pad).cpu().numpy()
             for x, dy, sc, sh in towers]
    return parts[0] + parts[1]


# N,H,W,Cin,Cout,k,stride,pad,prologue ; destinations of the fused bias sums
TWO_TOWER_CASES = [
    ((1, 8, 8, 64, 64, 1, 1, 0, True), 0),        # 1 split per tower: the slab path exists only because T = 2
    ((2, 16, 32, 64, 64, 3, 1, 1, True), 0),      # "same" 3x3 kernel, 4 splits per tower
    ((1, 19, 23, 64, 128, 3, 2, 1, True), 0),     # general kernel, stride 2, odd sizes, ragged last 32-row step
    ((1, 12, 12, 64, 96, 1, 1, 0, False), 0),     # ragged 64-wide Cout tile
    ((2, 9, 16, 128, 256, 1, 1, 0, True), 2),     # fused bias of both towers into two destinations
    ((8, 12, 3, 64, 64, 3, 1, 1, True), 0),       # "same" kernel, W = 3: dq = 10, dr = 2; H = 12 is the smallest H it accepts for that W
    ((2, 8, 48, 64, 64, 3, 1, 1, False), 0),      # W = 48 > 32: dq = 0
    ((4, 6, 8, 64, 64, 3, 1, 1, True), 0),        # W = 8, H = 6 at the 32 / W + 1 < H boundary; steps straddle image ends
    ((4, 5, 8, 64, 64, 3, 1, 1, True), 0),        # one row below that boundary: the general kernel
]


@pytest.mark.parametrize("spec,nbias", TWO_TOWER_CASES)
def test_two_tower_wgrad(cuda, spec, nbias):
    towers, want_w, want_b = _layer(spec, 2, 1000 + sum(spec))
    seeds = _seeds(spec, nbias, 5 + sum(spec))
    after = _wgrad_layers(cuda, [(spec, towers, seeds)])[0]
    got_w = (after[0] - seeds[0]).reshape(_w_shape(spec))
    scale = np.abs(want_w).max()
    err = np.abs(got_w - want_w).max()
    bar = _float64_bar(spec, 2, want_w)
    print("%s: dW max err vs float64 %.2e of scale (bar %.2e)" % (spec, err / scale, bar / scale))
    assert err <= bar                                       # measured 2.0e-7 .. 3.6e-7 of scale over the nine cases (bars 4.4e-5 .. 1.2e-4)
    for j in range(nbias):                                  # both destinations receive the same column sums of both towers' dy
        got_b = after[1 + j] - seeds[1 + j]
        err_b = np.abs(got_b - want_b).max()
        print("    d_bias %d: max err vs float64 %.2e of scale" % (j, err_b / np.abs(want_b).max()))
        assert err_b <= _float64_bar(spec, 2, want_b)       # measured 1.2e-7 of scale (bar 6.3e-5)
    # the same products as two single-tower launches: float32 summation order only (the bar of test_conv_gpu.py)
    ref = _single_tower_sum(cuda, spec, towers)
    d = np.abs(got_w - ref).max()
    print("    dW max difference to the sum of two single-tower launches %.2e of scale" % (d / scale))
    assert d <= 1e-5 * scale                                # measured 5e-8 .. 1e-7 of scale
    # reproducible: a second identical call gives the same bits
    again = _wgrad_layers(cuda, [(spec, towers, seeds)])[0]
    assert all(_same_bits(a, b) for a, b in zip(after, again))


def test_two_tower_wgrad_is_two_sequential_launches_bit_for_bit(cuda):
    """One split per tower and dw = 0: the slab reduction computes 0 + (a + b) with a first, the two sequential single-tower
    launches (one split: each adds into dw itself) (0 + a) + b."""
    from stabnet_amd import ops
    spec = TWO_TOWER_CASES[0][0]
    towers, _, _ = _layer(spec, 2, 1000 + sum(spec))
    after = _wgrad_layers(cuda, [(spec, towers, _seeds(spec, 0, 0, zero=True))])[0]
    dw = torch.zeros(_w_shape(spec), dtype=torch.float32, device=cuda)
    for x, dy, sc, sh in towers:
        ops.conv2d_wgrad(_dev(cuda, x), _dev(cuda, dy), _w_shape(spec), _dev(cuda, sc), _dev(cuda, sh), spec[6], spec[7], dw=dw)
    assert _same_bits(after[0], dw.cpu().numpy().reshape(-1))


L_1x1 = (1, 8, 8, 64, 64, 1, 1, 0, True)
L_3x3 = (2, 8, 16, 64, 64, 3, 1, 1, True)
L_BIAS = (2, 9, 16, 64, 256, 1, 1, 0, True)
L_240 = (2, 8, 8, 12, 20, 1, 1, 0, False)                   # 240 elements: not a multiple of 256
L_TINY = (1, 4, 8, 16, 16, 1, 1, 0, False)                  # 256 elements, one 32-pixel step per tower

# layers (spec, biases) of one call; which layers, reduced alone, take the SAME reduce kernel as in the table
TABLE_CASES = {
    "reduce4": ([(L_1x1, 0), (L_3x3, 0), (L_BIAS, 1)], [True, True, True]),                       # every entry elems % 256 == 0
    "flat": ([(L_1x1, 0), (L_3x3, 0), (L_BIAS, 1), (L_240, 0)], [False, False, False, True]),     # 240 elements: the flat kernel for all
    "flush": ([(L_TINY, 0)] * 66, [True] * 66),             # the table fills at 64 entries and is flushed mid-way
}


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_shared_reduce_table(cuda, name):
    layers, same_kernel = TABLE_CASES[name]
    entries = []
    for i, (spec, nbias) in enumerate(layers):
        towers, want_w, want_b = _layer(spec, 2, 2000 + i)
        entries.append((spec, towers, _seeds(spec, nbias, 3000 + i)))
    after = _wgrad_layers(cuda, entries)
    worst = other = 0.0
    for i, ((spec, nbias), entry, got) in enumerate(zip(layers, entries, after)):
        _, want_w, want_b = _layer(spec, 2, 2000 + i)
        wants = [want_w.reshape(-1)] + [want_b] * nbias
        alone = _wgrad_layers(cuda, [entry])[0]
        for j, (g, a, s, want) in enumerate(zip(got, alone, entry[2], wants)):
            scale = np.abs(want).max()
            err = np.abs((g - s) - want).max()               # an entry left out leaves the seed, one reduced twice 2 x the gradient
            worst = max(worst, err / _float64_bar(spec, 2, want))
            # measured: at most 0.009 of the bar in all three tables
            assert err <= _float64_bar(spec, 2, want), "layer %d destination %d: err %g of scale" % (i, j, err / scale)
            if same_kernel[i]:
                assert _same_bits(g, a), "layer %d destination %d differs from the one-layer call" % (i, j)
            else:
                other = max(other, np.abs(g - a).max() / scale)
                # measured 0: with two slabs per entry the two kernels add in the same order
                assert np.abs(g - a).max() <= 1e-5 * scale, "layer %d destination %d" % (i, j)
    print("%s: %d layers, worst error vs float64 = %.3f of the bar; across reduce kernels %.2e of scale" % (name, len(layers), worst, other))


def _zero_layer(cuda, spec, T, dw_off, b1=None, b2=None):
    N, H, W, Cin, Cout, k, stride, pad, pro = spec
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
    tw = [(z(N, H, W, Cin), z(N, Ho, Wo, Cout), z(Cin) if pro else None, z(Cin) if pro else None) for _ in range(T)]
    return (_geom(spec), tw, dw_off, b1, b2)


def test_wgrad_layers_refusals_write_nothing(cuda):
    from stabnet_amd import _lib, ops
    e1, eb = 64 * 64, 256 * 64
    ok = _zero_layer(cuda, L_1x1, 2, 0)
    nbytes = ops.conv2d_wgrad_layers_workspace_bytes([ok])
    assert nbytes == 2 * e1 * 4                              # two towers, one split each
    nbytes_b = ops.conv2d_wgrad_layers_workspace_bytes([_zero_layer(cuda, L_BIAS, 2, 0, eb)])
    bad = {
        "three towers": ([_zero_layer(cuda, L_1x1, 3, 0)], nbytes * 2),
        "bias on a layer that cannot fuse it": ([_zero_layer(cuda, L_1x1, 2, 0, e1)], nbytes * 2),
        "dw not 16-byte aligned": ([_zero_layer(cuda, L_1x1, 2, 2)], nbytes),
        "d_bias not 16-byte aligned": ([_zero_layer(cuda, L_BIAS, 2, 0, eb + 2)], nbytes_b),
        "second d_bias not 16-byte aligned": ([_zero_layer(cuda, L_BIAS, 2, 0, eb, eb + 256 + 1)], nbytes_b),
        "second bias without a first": ([_zero_layer(cuda, L_BIAS, 2, 0, None, eb)], nbytes_b),
        "dw beyond the gradient buffer": ([_zero_layer(cuda, L_BIAS, 2, 4096)], nbytes_b),
        "workspace one float short": ([ok], nbytes - 4),
        "workspace short by the bias sums": ([_zero_layer(cuda, L_BIAS, 2, 0, eb)], nbytes_b - 4),
    }
    for what, (layers, ws_bytes) in bad.items():
        grads = Guarded(cuda, eb + 2 * 256 + 8, init="canary")
        ws = Guarded(cuda, ws_bytes // 4, init="canary")
        with pytest.raises(_lib.StabnetError):
            ops.conv2d_wgrad_layers(layers, grads.t, ws.t)
        torch.cuda.synchronize()
        assert grads.untouched() and ws.untouched(), what
    assert ops.conv2d_wgrad_layers_workspace_bytes([_zero_layer(cuda, L_1x1, 3, 0)]) == 0


# ---- the re-pack and image tables -----------------------------------------------------------------------------------------------

# Cout, K, Cin, stride
PACK_TILED = [(256, 1, 64, 1), (64, 3, 64, 1), (128, 3, 128, 2), (96, 1, 32, 1)]
PACK_ELEMENTWISE = PACK_TILED + [(64, 1, 16, 1)]            # Cin = 16: one layer off the 32 x 32 tiles sends ALL to the element-wise kernel


def _params_with_canaries(layers, seed):
    """the layers' weights at offsets of one buffer, canary words before, between (7, 9, 11, ... words) and behind them"""
    rng = np.random.default_rng(seed)
    ws, offs, off = [], [], 5
    for i, (Cout, K, Cin, _) in enumerate(layers):
        ws.append(rng.standard_normal((Cout, K, K, Cin)).astype(np.float32))
        offs.append(off)
        off += ws[-1].size + 7 + 2 * i
    buf = np.full(off, CANARY, np.uint32)
    for w, o in zip(ws, offs):
        buf[o:o + w.size] = w.reshape(-1).view(np.uint32)
    return ws, offs, buf.view(np.float32)


@pytest.mark.parametrize("layers", [PACK_TILED, PACK_ELEMENTWISE], ids=["tiled", "elementwise"])
def test_pack_table_and_image_table(cuda, layers):
    from stabnet_amd import _lib, ops
    from stabnet_amd._tensor import ptr, stream_ptr
    ws, offs, params = _params_with_canaries(layers, 11 + len(layers))
    model = [M.pack_dgrad_model(w, stride) for w, (_, _, _, stride) in zip(ws, layers)]
    want = np.concatenate([m.reshape(-1) for m in model])
    wt = Guarded(cuda, want.size)
    tparams = _dev(cuda, params)
    ops.pack_dgrad_weights_table(tparams, wt.t, [(o,) + l for o, l in zip(offs, layers)])
    _check_all({"wt": wt})
    assert _same_bits(wt.np(), want)                        # a pure permutation: bit-equal (a read off a tensor's end meets a canary)
    # the images of the re-packed tensors [Cin][K * K * Cout], the way the step builds them: one launch, offsets into wt
    L = _lib.lib()
    entries, singles, prefix, img_off = [], [], 0, 4
    for (Cout, K, Cin, _), m in zip(layers, model):
        Kd = K * K * Cout
        n = int(L.stabnet_conv_weight_image_floats(Cin, 1, 1, Kd))
        assert n > 0 and Kd % 32 == 0
        entries.append((prefix, img_off, Cin, Kd))
        one = Guarded(cuda, n)
        packed_copy = _dev(cuda, m)
        _lib.call("stabnet_conv_weight_split_image", ptr(packed_copy), Cin, 1, 1, Kd, ptr(one.t), stream_ptr(cuda), device=cuda)
        singles.append((img_off, n, one))
        prefix += m.size
        img_off += n + 12                                   # 12 canary words between two images
    img = Guarded(cuda, img_off, init="canary")
    ops.conv_weight_split_images_table(wt.t, img.t, entries)
    _check_all(dict({"img": img}, **{"image %d" % i: s[2] for i, s in enumerate(singles)}))
    got = img.np().view(np.uint32)
    rest = np.ones(img_off, bool)
    for off, n, one in singles:
        assert np.array_equal(got[off:off + n], one.np().view(np.uint32))
        rest[off:off + n] = False
    assert (got[rest] == CANARY).all()


def test_pack_and_image_tables_refuse_too_many_entries(cuda):
    from stabnet_amd import _lib, ops
    params = _dev(cuda, np.ones(57 * 1024 + 64, np.float32))
    wt = Guarded(cuda, 65 * 1024, init="canary")
    ops.pack_dgrad_weights_table(params, wt.t, [(1024 * i, 32, 1, 32, 1) for i in range(56)])      # 56 entries: the table's capacity
    _check_all({"wt": wt})
    assert _same_bits(wt.np()[:56 * 1024], np.ones(56 * 1024, np.float32))
    wt = Guarded(cuda, 65 * 1024, init="canary")
    with pytest.raises(_lib.StabnetError):
        ops.pack_dgrad_weights_table(params, wt.t, [(1024 * i, 32, 1, 32, 1) for i in range(57)])
    with pytest.raises(_lib.StabnetError):                  # a tensor that ends behind the parameter buffer
        ops.pack_dgrad_weights_table(params, wt.t, [(57 * 1024, 32, 1, 64, 1)])
    img = Guarded(cuda, 65 * 3072, init="canary")
    with pytest.raises(_lib.StabnetError):
        ops.conv_weight_split_images_table(params, img.t, [(0, 3072 * i, 32, 32) for i in range(65)])
    with pytest.raises(_lib.StabnetError):                  # K % 32 != 0
        ops.conv_weight_split_images_table(params, img.t, [(0, 0, 32, 48)])
    torch.cuda.synchronize()
    assert wt.untouched() and img.untouched()


# ---- dgrad on the packed split kernels ------------------------------------------------------------------------------------------

# N,H,W,Cin,Cout,k,stride,pad
DGRAD_PACKED = [
    (2, 18, 24, 64, 64, 1, 1, 0),
    (2, 18, 24, 64, 256, 1, 1, 0),
    (2, 9, 16, 256, 64, 1, 1, 0),
    (2, 16, 32, 64, 64, 3, 1, 1),
]
DGRAD_INPLACE = (2, 18, 24, 64, 256, 1, 1, 0)               # with residual == dx (the projection unit, net.hip)
DGRAD_FALLBACK = [
    (1, 19, 23, 64, 128, 3, 2, 1),                          # up = 2
    (2, 16, 128, 64, 64, 3, 2, 1),                          # up = 2, whole output rows per tile
    (2, 18, 24, 64, 48, 1, 1, 0),                           # K * K * Cout % 32 != 0: no image exists
]


@functools.lru_cache(maxsize=None)
def _dgrad_data(spec):
    N, H, W, Cin, Cout, k, stride, pad = spec
    rng = np.random.default_rng(sum(spec))
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    dy = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    res = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    want = M.tower_grads(np.zeros((N, H, W, Cin)), dy, w.shape, None, None, stride, pad, w=w)[2]
    return _frozen(dy, w, res, want)


def _dgrad_split(cuda, spec, residual=None, inplace=False):
    """stabnet_conv2d_dgrad_split into a guarded dx with a guarded workspace of exactly the queried size -> (dx, packed)"""
    from stabnet_amd import _lib, ops
    N, H, W, Cin, Cout, k, stride, pad = spec
    dy, w, _, _ = _dgrad_data(spec)
    dx = Guarded(cuda, N * H * W * Cin, init=np.array(residual) if inplace else None)
    nbytes = int(_lib.lib().stabnet_conv2d_dgrad_split_workspace_bytes(N, H, W, Cin, Cout, k, k, stride, pad))
    assert nbytes > 0
    ws = Guarded(cuda, nbytes, dtype=torch.uint8)
    res = dx.t if inplace else _dev(cuda, residual)
    _, packed = ops.conv2d_dgrad_split(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad, residual=res, dx=dx.t, workspace=ws.t)
    _check_all({"dx": dx, "workspace": ws})
    return dx.np().reshape(N, H, W, Cin), packed


@pytest.mark.parametrize("spec,inplace", [(s, False) for s in DGRAD_PACKED] + [(DGRAD_INPLACE, True)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else ("inplace" if v else "plain"))
def test_split_dgrad_route_is_packed(cuda, spec, inplace):
    _, packed = _dgrad_split(cuda, spec, residual=_dgrad_data(spec)[2] if inplace else None, inplace=inplace)
    assert packed, "conv_route() kept this dgrad on the exact-f32 kernels"


@pytest.mark.parametrize("spec", DGRAD_PACKED, ids=lambda s: "-".join(map(str, s)))
def test_split_dgrad(cuda, spec):
    """The bars of test_conv_packed_gpu.py: not a reduced-precision mode."""
    from stabnet_amd import ops
    N, H, W, Cin, Cout, k, stride, pad = spec
    dy, w, _, want = _dgrad_data(spec)
    got, packed = _dgrad_split(cuda, spec)
    f32 = ops.conv2d_dgrad(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad).cpu().numpy()
    scale = np.abs(want).max()
    e_split, e_f32 = np.abs(got - want).max() / scale, np.abs(f32 - want).max() / scale
    d = np.abs(got - f32).max() / scale
    print("%s: packed route %d; max err vs float64 of scale: split %.2e, f32 MFMA %.2e; split vs f32 %.2e" % (spec, packed, e_split, e_f32, d))
    # measured over the four cases: e_split 1.8e-7 .. 5.7e-7 beside e_f32 2.4e-7 .. 5.0e-7 (at most 1.14 x e_f32), split vs f32 3.0e-7 .. 6.9e-7
    assert e_split <= 2.0 * e_f32 + 1e-7 and e_split < 3e-6
    assert d <= 4e-6


def test_split_dgrad_residual_in_place(cuda):
    from stabnet_amd import ops
    spec = DGRAD_INPLACE
    N, H, W, Cin, Cout, k, stride, pad = spec
    dy, w, res, want = _dgrad_data(spec)
    out, packed = _dgrad_split(cuda, spec, residual=res)
    inp, packed2 = _dgrad_split(cuda, spec, residual=res, inplace=True)
    assert packed == packed2
    assert _same_bits(inp, out)                             # residual == dx: every element is read before it is written, by its own lane
    f32 = ops.conv2d_dgrad(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad, residual=_dev(cuda, res)).cpu().numpy()
    want = want + res
    scale = np.abs(want).max()
    e_split, e_f32 = np.abs(inp - want).max() / scale, np.abs(f32 - want).max() / scale
    d = np.abs(inp - f32).max() / scale
    print("%s + residual in place: packed route %d; max err vs float64 of scale: split %.2e, f32 MFMA %.2e; split vs f32 %.2e" % (
        spec, packed, e_split, e_f32, d))
    assert e_split <= 2.0 * e_f32 + 1e-7 and e_split < 3e-6
    assert d <= 4e-6


@pytest.mark.parametrize("spec", DGRAD_FALLBACK, ids=lambda s: "-".join(map(str, s)))
def test_split_dgrad_fallback_is_the_exact_f32_operator(cuda, spec):
    from stabnet_amd import ops
    N, H, W, Cin, Cout, k, stride, pad = spec
    dy, w, res, want = _dgrad_data(spec)
    got, packed = _dgrad_split(cuda, spec)
    assert not packed
    f32 = ops.conv2d_dgrad(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad).cpu().numpy()
    assert _same_bits(got, f32)                             # the table re-pack and the stand-alone one feed the same kernel the same weights
    err = np.abs(got - want).max() / np.abs(want).max()
    print("%s: exact-f32 fallback, max err vs float64 %.2e of scale" % (spec, err))
    assert err <= 2e-5                                      # (test_conv_bwd_gpu.py's dgrad bar); measured 2.5e-7 .. 5.4e-7
    got_r, _ = _dgrad_split(cuda, spec, residual=res, inplace=True)
    f32_r = ops.conv2d_dgrad(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad, residual=_dev(cuda, res)).cpu().numpy()
    assert _same_bits(got_r, f32_r)


def test_split_dgrad_refusals_write_nothing(cuda):
    from stabnet_amd import _lib, ops
    spec = DGRAD_PACKED[1]
    N, H, W, Cin, Cout, k, stride, pad = spec
    dy, w, _, _ = _dgrad_data(spec)
    nbytes = int(_lib.lib().stabnet_conv2d_dgrad_split_workspace_bytes(N, H, W, Cin, Cout, k, k, stride, pad))
    dx = Guarded(cuda, N * H * W * Cin, init="canary")
    ws = Guarded(cuda, nbytes - 4, dtype=torch.uint8, init="canary")
    with pytest.raises(_lib.StabnetError):                  # workspace one float short
        ops.conv2d_dgrad_split(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, pad, dx=dx.t, workspace=ws.t)
    ws = Guarded(cuda, nbytes, dtype=torch.uint8, init="canary")
    with pytest.raises(_lib.StabnetError):                  # Cout % 16 != 0
        ops.conv2d_dgrad_split(_dev(cuda, dy[..., :40]), _dev(cuda, w[:40]), (N, H, W, Cin), stride, pad, dx=dx.t, workspace=ws.t)
    with pytest.raises(_lib.StabnetError):                  # pad > K - 1
        ops.conv2d_dgrad_split(_dev(cuda, dy), _dev(cuda, w), (N, H, W, Cin), stride, 1, dx=dx.t, workspace=ws.t)
    torch.cuda.synchronize()
    assert dx.untouched() and ws.untouched()
    assert int(_lib.lib().stabnet_conv2d_dgrad_split_workspace_bytes(N, H, W, Cin, 40, k, k, stride, pad)) == 0
