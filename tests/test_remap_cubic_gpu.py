"""GPU: the bicubic remap (csrc/remap.hip, stabnet_warp_rev_bundle2_cubic / _i420_cubic; --interp cubic) against the NumPy model
(tests/remap_cubic_model.py), BIT FOR BIT: both kernels of every window kind, strided and misaligned sources, guards around what is
written, frames smaller than the 4x4 taps, coordinates that leave the frame on every side, NaN maps, the planar path, a captured graph.
Coordinates and coverage counts are also held to the bilinear entries' on the same inputs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_cubic_model as CM
import remap_src_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5


@functools.lru_cache(maxsize=None)
def _case(H, W, SH, SW, shift, C=3, seed=SEED):
    """Inputs and the model's answer, computed once and shared (read-only)."""
    src = np.random.default_rng(seed * 1000 + SH + SW).integers(0, 256, (SH, SW, C), dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=seed, shift=shift)
    want, px, py, blk = CM.warp_src(src, xm, ym)
    for a in (src, xm, ym, want, px, py, blk):
        a.setflags(write=False)
    return src, xm, ym, want, px, py, blk


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _names(cuda, fn, *args, **kw):
    from stabnet_amd.deploy import Profiler
    prof = Profiler(max_records=16, device=cuda)
    fn(*args, prof=prof, **kw)
    return [r[0] for r in prof.records(raw=True)]


def test_device_weights_equal_the_model_table(cuda):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    buf = torch.full((1024 * 16 + 8,), 0x5A5A, dtype=torch.int16, device=cuda)
    _lib.call("stabnet_remap_cubic_weights_dev", ptr(buf), stream_ptr(cuda), device=cuda)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:16384].reshape(1024, 16), CM.table()) and (got[16384:] == 0x5A5A).all()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shift", [0.0, 0.45])
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_cubic_remap_equals_the_model(cuda, shape, shift, C):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    src, xm, ym, want, px, py, blk = _case(H, W, SH, SW, shift, C)
    if shift:
        assert blk.mean() > 0.1                              # a visible border: taps outside the frame, the coverage rule
    else:
        inside = CM.taps_inside(px, py, SH, SW)
        assert ((want == 0) | (want == 255))[inside].mean() > 0.005      # the clamp at either end is exercised
    s, x, y = _t(src, cuda), _t(xm, cuda), _t(ym, cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_src(s, x, y, black_count=black, return_maps=True, interp="cubic")
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    # coordinates and counts are the bilinear entry's, bit for bit
    lblack = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    _, lx, ly = warp.warpRevBundle2_src(s, x, y, black_count=lblack, return_maps=True)
    assert torch.equal(lx.view(torch.int32), gx.view(torch.int32)) and torch.equal(ly.view(torch.int32), gy.view(torch.int32))
    assert torch.equal(lblack, black)
    want_kernel = "remap_cubic_kernel<4, 0>" if (C == 3 and SW % 4 == 0) else "remap_cubic_kernel<1, 0>"
    assert _names(cuda, warp.warpRevBundle2_src, s, x, y, interp="cubic") == ["map_shrink_kernel", want_kernel]
    if (SH, SW) == (H, W) and C == 3:
        # at the network's own size warpRevBundle2(interp="cubic") is the same call
        assert torch.equal(warp.warpRevBundle2(s, x[None], y[None], interp="cubic"), got)


@pytest.mark.parametrize("SH,SW", [(77, 131), (48, 80)])
def test_batch_of_two(cuda, SH, SW):
    import torch
    from stabnet_amd import warp
    H, W = (32, 64) if SH == 77 else (64, 96)
    a, b = _case(H, W, SH, SW, 0.45), _case(H, W, SH, SW, -0.45, seed=SEED + 1)
    stack = lambda i: _t(np.stack([a[i], b[i]]), cuda)
    black = torch.zeros((2, SH, SW), dtype=torch.int32, device=cuda)
    got = warp.warpRevBundle2_src(stack(0), stack(1), stack(2), black_count=black, interp="cubic")
    for n, c in enumerate((a, b)):
        assert np.array_equal(got[n].cpu().numpy(), c[3]), n
        assert np.array_equal(black[n].cpu().numpy(), c[6].astype(np.int32)), n


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W,SH,SW,pad", [(32, 64, 77, 131, 7), (64, 96, 48, 80, 5), (64, 96, 48, 80, 8), (32, 64, 4, 4, 1)])
def test_strided_and_misaligned_sources(cuda, H, W, SH, SW, pad, off):
    """Rows `stride` > SW * C bytes apart in a buffer that ENDS with the frame's last byte and starts `off` bytes before its first: the
    four-pixel kernel keeps its dword loads inside the frame's own bytes (an odd stride puts rows at every alignment)."""
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(H, W, SH, SW, 0.45 if off % 2 else 0.0)
    stride = SW * 3 + pad
    nbytes = (SH - 1) * stride + SW * 3
    buf = torch.full((off + nbytes,), 255, dtype=torch.uint8, device=cuda)
    view = torch.as_strided(buf, (1, SH, SW, 3), (SH * stride, stride, 3, 1), storage_offset=off)
    view.copy_(_t(src, cuda)[None])
    before = buf.clone()
    if SW % 4 == 0:
        assert _names(cuda, warp.warpRevBundle2_src, view, _t(xm, cuda), _t(ym, cuda), interp="cubic")[-1] == "remap_cubic_kernel<4, 0>"
    got = warp.warpRevBundle2_src(view, _t(xm, cuda), _t(ym, cuda), interp="cubic")
    assert view.data_ptr() == buf.data_ptr() + off
    assert np.array_equal(got.cpu().numpy()[0], want)
    assert torch.equal(buf, before)


@pytest.mark.parametrize("out_off", [64, 61, 62])        # 4-byte aligned: the dword stores; mid-dword: the byte stores
@pytest.mark.parametrize("H,W,SH,SW", [(32, 64, 77, 131), (64, 96, 48, 80)])
def test_nothing_is_written_outside(cuda, H, W, SH, SW, out_off):
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(H, W, SH, SW, 0.45)
    n, G = SH * SW * 3, 128
    obuf = torch.full((out_off + n + G,), 0xA5, dtype=torch.uint8, device=cuda)
    bbuf = torch.full((G + SH * SW + G,), -7, dtype=torch.int32, device=cuda)
    bbuf[G:G + SH * SW] = 0
    out, black = obuf[out_off:out_off + n], bbuf[G:G + SH * SW]
    got = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, out=out, interp="cubic")
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy().reshape(SH, SW, 3), want)
    assert bool((obuf[:out_off] == 0xA5).all()) and bool((obuf[out_off + n:] == 0xA5).all())
    assert np.array_equal(black.cpu().numpy().reshape(SH, SW), blk.astype(np.int32))
    assert bool((bbuf[:G] == -7).all()) and bool((bbuf[G + SH * SW:] == -7).all())


def test_one_pixel_kernel_by_switch_gives_the_same(cuda, tmp_path):
    """STABNET_REMAP_VEC4=0 (read once per process, so in a child): the one-pixel kernel on a shape the four-pixel kernel takes."""
    src, xm, ym, want, px, py, blk = _case(64, 96, 48, 80, 0.45)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, src=src, x_map=xm, y_map=ym)
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_REMAP_VEC4="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "remap_cubic_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert list(d["names"]) == ["map_shrink_kernel", "remap_cubic_kernel<1, 0>"]
    assert np.array_equal(d["out"], want) and np.array_equal(d["black"], blk.astype(np.int32))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("SH,SW", [(1, 1), (2, 3), (3, 5), (4, 4)])
def test_frames_smaller_than_the_taps(cuda, SH, SW, C):
    """Narrower or shorter than four pixels: every pixel has a tap outside the frame (at 4x4 only ix, iy == 1, 1 has none)."""
    from stabnet_amd import warp
    for shift in (0.0, 0.2):
        src, xm, ym, want, px, py, blk = _case(32, 64, SH, SW, shift, C)
        inside = CM.taps_inside(px, py, SH, SW)
        assert not inside.any() if min(SH, SW) < 4 else inside.sum() <= 4
        got = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), interp="cubic")
        assert np.array_equal(got.cpu().numpy(), want)


def _ramp_maps(H, W, SH, SW, lo):
    """Maps whose source coordinate runs linearly from `lo` to lo + size - 2 on both axes (a step below one pixel: no index is skipped)."""
    sx, cx, sy, cy = (float(v) for v in M.constants(H, W, SH, SW))
    p = np.linspace(lo, lo + SW - 2, W)
    q = np.linspace(lo, lo + SH - 2, H)
    xm = (2.0 * (p - cx) / (sx * W) - 1.0).astype(np.float32)
    ym = (2.0 * (q - cy) / (sy * H) - 1.0).astype(np.float32)
    return np.broadcast_to(xm[None, :], (H, W)).copy(), np.broadcast_to(ym[:, None], (H, W)).copy()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("SH,SW", [(45, 67), (40, 64)])
def test_taps_leave_the_frame_on_every_side(cuda, SH, SW, C):
    """ix from -3 to SW + 2 and iy from -3 to SH + 2 (two ramps: off the top left, off the bottom right): every mix of taps inside and
    outside, and the pixels wholly outside."""
    import torch
    from stabnet_amd import warp
    H, W = 32, 64
    src = np.random.default_rng(SH).integers(0, 256, (SH, SW, C), dtype=np.uint8)
    seen_x, seen_y = set(), set()
    for lo in (-7.0, 8.0):
        xm, ym = _ramp_maps(H, W, SH, SW, lo)
        want, px, py, blk = CM.warp_src(src, xm, ym)
        ix, iy, _, _ = CM.quantise(px, py)
        seen_x |= set(ix.ravel().tolist())
        seen_y |= set(iy.ravel().tolist())
        black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
        got = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, interp="cubic")
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    assert set(range(-3, SW + 3)) <= seen_x and set(range(-3, SH + 3)) <= seen_y


@pytest.mark.parametrize("H,W,SH,SW", [(32, 64, 77, 131), (64, 96, 48, 80)])
def test_nan_and_huge_map_entries_are_black(cuda, H, W, SH, SW):
    import torch
    from stabnet_amd import warp
    src, xm, ym = _case(H, W, SH, SW, 0.0)[:3]
    xm, ym = xm.copy(), ym.copy()
    xm[5, 9], xm[21, 41], ym[13, 50], ym[29, 5] = np.nan, 1e30, -1e30, np.nan      # entries the 4x shrink samples
    want, px, py, blk = CM.warp_src(src, xm, ym)
    assert np.isnan(px).any() and np.isnan(py).any() and blk.any() and not blk.all()
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    got = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, interp="cubic")
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    assert (want[np.isnan(px) | np.isnan(py)] == 0).all()


@pytest.mark.parametrize("H,W,SH,SW", [(32, 64, 77, 131), (64, 96, 48, 80)])
def test_windows_on_the_host_and_on_the_device(cuda, H, W, SH, SW):
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(H, W, SH, SW, 0.3)
    s, x, y = _t(src, cuda), _t(xm, cuda), _t(ym, cuda)
    dev_win = lambda w: torch.tensor(w, dtype=torch.float64, device=cuda)
    whole = (0.0, 0.0, float(SH), float(SW))
    # the whole-frame window is the call without a window; an integer window at zoom 1 is its slice
    for win in (whole, dev_win(whole)):
        black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
        got = warp.warpRevBundle2_win(s, x, y, win, black_count=black, interp="cubic")
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    cut = (5.0, 8.0, 24.0, 40.0)
    for win in (cut, dev_win(cut)):
        got = warp.warpRevBundle2_win(s, x, y, win, (24, 40), interp="cubic")
        assert np.array_equal(got.cpu().numpy(), want[5:29, 8:48])
    # a 0.8 zoom at the source's size (and at a size that is no multiple of four): the model composed from remap_win_model
    zoom = warp.ratio_window(SH, SW, 0.8)
    for out_size in ((SH, SW), (50, 70)):
        zwant, zpx, zpy, zblk = CM.warp_win(src, xm, ym, zoom, out_size)
        for win in (zoom, dev_win(zoom)):
            black = torch.zeros(out_size, dtype=torch.int32, device=cuda)
            got, gx, gy = warp.warpRevBundle2_win(s, x, y, win, out_size, black_count=black, return_maps=True, interp="cubic")
            assert np.array_equal(got.cpu().numpy(), zwant)
            assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(zpx)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(zpy))
            assert np.array_equal(black.cpu().numpy(), zblk.astype(np.int32))
            lblack = torch.zeros(out_size, dtype=torch.int32, device=cuda)
            _, lx, ly = warp.warpRevBundle2_win(s, x, y, win, out_size, black_count=lblack, return_maps=True)
            assert torch.equal(lx.view(torch.int32), gx.view(torch.int32)) and torch.equal(ly.view(torch.int32), gy.view(torch.int32))
            assert torch.equal(lblack, black)
    # a device window the host entry would refuse gives the whole frame
    for bad in ((float("nan"), 0.0, 10.0, 10.0), (0.0, 0.0, -1.0, 10.0), (0.0, 0.0, SH + 1.0, float(SW))):
        assert np.array_equal(warp.warpRevBundle2_win(s, x, y, dev_win(bad), interp="cubic").cpu().numpy(), want)
    four = SW % 4 == 0
    assert _names(cuda, warp.warpRevBundle2_win, s, x, y, zoom, interp="cubic")[-1] == "remap_cubic_kernel<%d, 1>" % (4 if four else 1)
    assert _names(cuda, warp.warpRevBundle2_win, s, x, y, dev_win(zoom), interp="cubic")[-1] == "remap_cubic_kernel<%d, 2>" % (4 if four else 1)


# (network H, W, source SH, SW): both plane kinds on the four-pixel path; Y four-pixel and chroma (width 66) one-pixel; both one-pixel
@pytest.mark.parametrize("planes,border_y,off", [(3, 0, 0), (3, 16, 1), (1, 16, 3), (1, 0, 0)])
@pytest.mark.parametrize("shape", [(32, 64, 90, 160), (32, 64, 78, 132), (32, 64, 90, 150)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_planar_frames(cuda, shape, planes, border_y, off):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    nbytes = warp.i420_frame_bytes(SH, SW, planes)
    frame = np.random.default_rng(SH + planes).integers(0, 256, nbytes, dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=SEED, shift=0.3)
    buf = torch.zeros(off + nbytes, dtype=torch.uint8, device=cuda)      # the frame ends with the buffer, and begins `off` bytes in
    buf[off:] = _t(frame, cuda)
    for window, out_size in ((None, None), (warp.ratio_window(SH, SW, 0.8), None), ((4.0, 6.0, 60.0, 100.0), (60, 100))):
        want, blk = CM.warp_i420(frame, xm, ym, SH, SW, planes, window, out_size, border_y)
        OH, OW = (SH, SW) if out_size is None else out_size
        black = torch.zeros((1, OH, OW), dtype=torch.int32, device=cuda)
        got = warp.warpRevBundle2_i420(buf[off:], _t(xm, cuda), _t(ym, cuda), (SH, SW), planes, window=window, out_size=out_size,
                                       border_y=border_y, black_count=black, interp="cubic")
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(black.cpu().numpy()[0], blk.astype(np.int32))
        lblack = torch.zeros((1, OH, OW), dtype=torch.int32, device=cuda)
        warp.warpRevBundle2_i420(buf[off:], _t(xm, cuda), _t(ym, cuda), (SH, SW), planes, window=window, out_size=out_size,
                                 border_y=border_y, black_count=lblack)
        assert torch.equal(lblack, black)
        if window is None and planes == 3:
            # the border values are visible: chroma taps outside read 128, luma border_y
            c = want[SH * SW:]
            assert (c == 128).mean() > 0.05 and (want[:SH * SW] == border_y).mean() > 0.05
    assert _names(cuda, warp.warpRevBundle2_i420, buf[off:], _t(xm, cuda), _t(ym, cuda), (SH, SW), planes, interp="cubic") \
        == ["map_shrink_kernel", "remap_i420_kernel<true>"]


def test_one_graph_replayed_three_times(cuda):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = 64, 96, 48, 80
    cases = [_case(H, W, SH, SW, 0.45, seed=SEED + k) for k in range(3)]
    src, xm, ym = (_t(cases[0][i], cuda) for i in range(3))
    out = torch.zeros((SH, SW, 3), dtype=torch.uint8, device=cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    total = np.zeros((SH, SW), np.int32)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        warp.warpRevBundle2_src(src, xm, ym, black_count=black, out=out, interp="cubic")       # eager once: loads the code objects
        s.synchronize()
        black.zero_(); out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            warp.warpRevBundle2_src(src, xm, ym, black_count=black, out=out, interp="cubic")
        s.synchronize()
        assert int(black.sum()) == 0 and int(out.sum()) == 0
        for c in cases:
            src.copy_(_t(c[0], cuda)); xm.copy_(_t(c[1], cuda)); ym.copy_(_t(c[2], cuda))
            g.replay()
            s.synchronize()
            total += c[6].astype(np.int32)
            assert np.array_equal(out.cpu().numpy(), c[3]) and np.array_equal(black.cpu().numpy(), total)


def test_refusals_launch_nothing(cuda):
    import torch
    from stabnet_amd import _lib, warp
    from stabnet_amd._tensor import ptr, stream_ptr
    H, W, SH, SW = 32, 64, 77, 131
    src, xm, ym = (_t(a, cuda) for a in _case(H, W, SH, SW, 0.0)[:3])
    out = torch.full((SH, SW, 3), 0xA5, dtype=torch.uint8, device=cuda)
    ws = torch.full((2 * (H // 4) * (W // 4),), -3.0, dtype=torch.float32, device=cuda)
    good = dict(src=ptr(src), N=1, SH=SH, SW=SW, C=3, stride=SW * 3, x_map=ptr(xm), y_map=ptr(ym), H=H, W=W, rate=4, kind=0, window=None,
                OH=SH, OW=SW, out=ptr(out), black=0, ws=ptr(ws), px=0, py=0, stream=stream_ptr(cuda), prof=0)
    for bad in (dict(src=0), dict(out=0), dict(ws=0), dict(C=2), dict(kind=3), dict(kind=-1), dict(OH=SH - 1), dict(kind=1), dict(kind=2),
                dict(stride=SW * 3 - 1), dict(SH=32768), dict(rate=0)):
        with pytest.raises(_lib.StabnetError, match="warp_rev_bundle2_cubic"):
            _lib.call("stabnet_warp_rev_bundle2_cubic", *dict(good, **bad).values(), device=cuda)
    with pytest.raises(_lib.StabnetError, match="interp"):
        warp.warpRevBundle2_src(src, xm, ym, interp="nearest")
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all())
    _lib.call("stabnet_warp_rev_bundle2_cubic", *good.values(), device=cuda)
    assert np.array_equal(out.cpu().numpy(), _case(H, W, SH, SW, 0.0)[3])
