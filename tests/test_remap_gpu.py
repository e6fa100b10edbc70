"""GPU: colour-frame remap with smoothed maps (deploy_bundle.py:136-146) vs the oracle's restatement of OpenCV's
resize/remap geometry -- smoothed pixel-coordinate maps bit-exact, uint8 output exact."""
import functools

import numpy as np
import pytest
import torch

import remap_src_model as M
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shift", [0.0, 0.45, -0.45])      # +-0.45: a fifth of the frame maps outside on the right / bottom or left / top
@pytest.mark.parametrize("H,W", [(288, 512), (90, 130), (720, 1280), (64, 96)])   # W % 4 == 0: the four-pixels-per-thread kernel; 130: the scalar one
def test_warp_rev_bundle2(cuda, H, W, shift):
    from stabnet_amd import warp
    from stabnet_amd.config import Config
    cfg, ocfg = Config(height=H, width=W), O.Config(height=H, width=W)
    rng = np.random.default_rng(H)
    theta = (rng.standard_normal((1, 50)) * 0.06).astype(np.float32)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    _, pts2 = O.get_4_pts(theta, ocfg)
    x_map, y_map, _ = O.maps_from_Hs(O.get_Hs(pts2, ocfg), H, W, ocfg)
    x_map, y_map = (x_map + np.float32(shift)).astype(np.float32), (y_map + np.float32(shift)).astype(np.float32)
    want, xs, ys = O.warpRevBundle2(img, x_map[0], y_map[0])
    got, px, py = warp.warpRevBundle2(torch.from_numpy(img).to(cuda), torch.from_numpy(x_map).to(cuda),
                                      torch.from_numpy(y_map).to(cuda), return_maps=True)
    assert np.array_equal(px.cpu().numpy()[0], xs) and np.array_equal(py.cpu().numpy()[0], ys)
    assert np.array_equal(got.cpu().numpy(), want)
    if shift:
        assert (want == 0).all(axis=2).mean() > 0.1                       # a visible black border: the BORDER_CONSTANT taps were exercised
    got2 = warp.warpRevBundle2(torch.from_numpy(img).to(cuda), torch.from_numpy(x_map).to(cuda), torch.from_numpy(y_map).to(cuda))
    assert np.array_equal(got2.cpu().numpy(), want)                          # (without the optional pixel-coordinate outputs)


@pytest.mark.parametrize("n,off", [(1, 0), (7, 0), (4096, 0), (720 * 1280, 0), (1001, 1), (4099, 3)])
def test_cvt_train2img_exact(cuda, n, off):
    """deploy_bundle.py:75: ((x + 0.5) * 255).astype(uint8) (clipped first); the vector path and the unaligned / tail path."""
    import torch
    from stabnet_amd import warp
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.7, 0.7, size=n + off).astype(np.float32)
    x[: min(n, 4)] = [-0.5, 0.5, 0.49999997, -0.49803922][: min(n, 4)]
    want = ((x[off:] + np.float32(0.5)) * np.float32(255)).clip(0, 255).astype(np.uint8)
    xd = torch.from_numpy(x).to(cuda)[off:]
    buf = torch.zeros(n + off + 8, dtype=torch.uint8, device=cuda)
    out = warp.cvt_train2img(xd, buf[off:off + n])
    assert np.array_equal(out.cpu().numpy(), want)
    assert int(buf[off + n:].sum()) == 0 and int(buf[:off].sum()) == 0        # nothing written outside


# ---- the network-size entry runs the bodies the source-size and window entries run: the cases their tests cover, at SH, SW == H, W ----
# expected values: tests/remap_src_model.py at the network's own size (s = 1, c = 0), which is O.warpRevBundle2 bit for bit.
# 32x64: W % 4 == 0, the four-pixel kernel; 30x50: the scalar kernel, small maps 7x12; 8x12: small maps 2x3, the last pixels take the
# loader's byte path; 4x4: one node.

@functools.lru_cache(maxsize=None)
def _net_case(H, W, shift, C=3, seed=5):
    """Inputs and the model's answer, computed once and shared (read-only)."""
    img = np.random.default_rng(seed * 1000 + H + W).integers(0, 256, (H, W, C), dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=seed, shift=shift)
    want, px, py, _ = M.warp_src(img, xm, ym)
    for a in (img, xm, ym, want, px, py):
        a.setflags(write=False)
    return img, xm, ym, want, px, py


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _zero_share(want):
    return (want == 0).all(axis=2).mean()


@pytest.mark.parametrize("H,W", [(32, 64), (30, 50)])
def test_network_size_batch_of_two(cuda, H, W):
    from stabnet_amd import warp
    a, b = _net_case(H, W, 0.45), _net_case(H, W, 0.45, seed=6)
    stack = lambda i: _t(np.stack([a[i], b[i]]), cuda)
    got, gx, gy = warp.warpRevBundle2(stack(0), stack(1), stack(2), return_maps=True)
    for n, c in enumerate((a, b)):
        assert _zero_share(c[3]) > 0.1, n                                     # a visible border on the model's own answer
        assert np.array_equal(_bits(gx[n].cpu().numpy()), _bits(c[4])) and np.array_equal(_bits(gy[n].cpu().numpy()), _bits(c[5])), n
        assert np.array_equal(got[n].cpu().numpy(), c[3]), n


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("H,W", [(32, 64), (8, 12)])
def test_network_size_other_channel_counts(cuda, H, W, C):
    from stabnet_amd import warp
    img, xm, ym, want, px, py = _net_case(H, W, -0.45, C=C)
    assert _zero_share(want) > 0.1
    got, gx, gy = warp.warpRevBundle2(_t(img, cuda), _t(xm[None], cuda), _t(ym[None], cuda), return_maps=True)
    assert got.shape == (H, W, C) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))


@pytest.mark.parametrize("H,W", [(32, 64), (30, 50)])
def test_network_size_nan_and_huge_map_entries_are_black(cuda, H, W):
    from stabnet_amd import warp
    img, xm, ym = _net_case(H, W, 0.0)[:3]
    xm, ym = xm.copy(), ym.copy()
    # 5x5 patches: the shrink's taps (two of every 4 or so entries per axis) land inside each
    xm[2:7, 3:8], xm[20:25, 30:35], ym[10:15, 40:45], ym[24:29, 2:7] = np.nan, np.inf, -np.inf, 3e38
    ym[2:7, 20:25], xm[12:17, 14:19] = np.nan, -3e38
    with np.errstate(invalid="ignore", over="ignore"):
        want, px, py, blk = M.warp_src(img, xm, ym)
    assert np.isnan(px).any() and np.isnan(py).any() and np.isinf(px).any() and np.isinf(py).any() and blk.any() and not blk.all()
    got, gx, gy = warp.warpRevBundle2(_t(img, cuda), _t(xm[None], cuda), _t(ym[None], cuda), return_maps=True)
    assert np.array_equal(gx.cpu().numpy()[0], px, equal_nan=True) and np.array_equal(gy.cpu().numpy()[0], py, equal_nan=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want[np.isnan(px) | np.isnan(py)] == 0).all()


@pytest.mark.parametrize("map_off", [4, 1], ids=["maps16", "maps4"])     # floats: 16-byte aligned; 4 bytes past it
@pytest.mark.parametrize("out_off", [64, 61])
@pytest.mark.parametrize("img_off", [0, 1])
def test_network_size_misaligned_pointers_and_guards(cuda, img_off, out_off, map_off):
    """The entry itself: all aligned is the four-pixel kernel's dword traffic, any misalignment the one-pixel kernel's bytes; either
    way the model's bytes, and nothing written outside out, px and py."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    H, W = 32, 64
    img, xm, ym, want, px, py = _net_case(H, W, 0.45)
    n, G = H * W * 3, 128
    ibuf = torch.full((img_off + n + 3,), 255, dtype=torch.uint8, device=cuda)
    ibuf[img_off:img_off + n] = _t(img, cuda).reshape(-1)
    obuf = torch.full((out_off + n + G,), 0xA5, dtype=torch.uint8, device=cuda)
    pbuf = torch.full((2, H * W + 16), -7.0, dtype=torch.float32, device=cuda)                # rows 16-byte aligned
    i_t, o_t, px_t, py_t = ibuf[img_off:img_off + n], obuf[out_off:out_off + n], pbuf[0, map_off:map_off + H * W], pbuf[1, map_off:map_off + H * W]
    assert pbuf.stride(0) % 4 == 0 and px_t.data_ptr() % 16 == (map_off * 4) % 16 and py_t.data_ptr() % 16 == (map_off * 4) % 16
    assert i_t.data_ptr() % 4 == img_off and o_t.data_ptr() % 4 == out_off % 4
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=cuda)
    x_t, y_t = _t(xm, cuda), _t(ym, cuda)
    _lib.call("stabnet_warp_rev_bundle2", ptr(i_t), ptr(x_t), ptr(y_t), 1, H, W, 3, 4, ptr(o_t), ptr(ws), ptr(px_t), ptr(py_t), stream_ptr(cuda),
              device=cuda)
    assert np.array_equal(o_t.cpu().numpy().reshape(H, W, 3), want)
    assert np.array_equal(_bits(px_t.cpu().numpy().reshape(H, W)), _bits(px)) and np.array_equal(_bits(py_t.cpu().numpy().reshape(H, W)), _bits(py))
    assert bool((obuf[:out_off] == 0xA5).all()) and bool((obuf[out_off + n:] == 0xA5).all())
    assert bool((pbuf[:, :map_off] == -7.0).all()) and bool((pbuf[:, map_off + H * W:] == -7.0).all())


@pytest.mark.parametrize("shift", [0.0, 0.45])
@pytest.mark.parametrize("H,W", [(8, 12), (4, 4)])
def test_network_size_tiny_frames(cuda, H, W, shift):
    from stabnet_amd import warp
    img, xm, ym, want, px, py = _net_case(H, W, shift)
    got, gx, gy = warp.warpRevBundle2(_t(img, cuda), _t(xm[None], cuda), _t(ym[None], cuda), return_maps=True)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(got.cpu().numpy(), want)
