"""GPU: the planar 4:2:0 remap (csrc/remap.hip, stabnet_warp_rev_bundle2_i420) against the NumPy model (tests/remap_i420_model.py): every
plane and the coverage counts bit for bit, for batches, Y-only frames and both border values; the Y plane against the source-resolution
entry; a black frame that must stay black; windows; guard bytes; misaligned buffers; the one-pixel path by switch; a captured graph."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_i420_model as IM
import remap_src_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 5
KINDS = ["identity", "mesh", "mesh+0.3", "mesh-0.3"]
SHIFT = {"mesh": 0.0, "mesh+0.3": 0.3, "mesh-0.3": -0.3}
IDS = ["%dx%d-%dx%d" % s for s in IM.SHAPES]


@functools.lru_cache(maxsize=None)
def _maps(H, W, kind, seed=SEED):
    xm, ym = M.identity_maps(H, W) if kind == "identity" else M.mesh_maps(H, W, seed=seed, shift=SHIFT[kind])
    xm.setflags(write=False); ym.setflags(write=False)
    return xm, ym


@functools.lru_cache(maxsize=None)
def _frame(SH, SW, seed=SEED):
    f = np.random.default_rng(seed * 1000 + SH + SW).integers(0, 256, SH * SW * 3 // 2, dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _model(shape, kind, planes=3, border_y=0, window=None, out_size=None, seed=SEED):
    """The model's (out, black) of the seeded frame, computed once and shared (read-only)."""
    H, W, SH, SW = shape
    xm, ym = _maps(H, W, kind, seed)
    nbytes = SH * SW if planes == 1 else SH * SW * 3 // 2
    out, black = IM.warp_i420(_frame(SH, SW, seed)[:nbytes], xm, ym, SH, SW, planes, window, out_size, border_y)
    out.setflags(write=False); black.setflags(write=False)
    return out, black


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(cuda, shape, kind, planes=3, border_y=0, window=None, out_size=None, seed=SEED, **kw):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    OH, OW = out_size or (SH, SW)
    xm, ym = _maps(H, W, kind, seed)
    nbytes = SH * SW if planes == 1 else SH * SW * 3 // 2
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    got = warp.warpRevBundle2_i420(_t(_frame(SH, SW, seed)[:nbytes], cuda), _t(xm, cuda), _t(ym, cuda), (SH, SW), planes, window=window,
                                   out_size=out_size, border_y=border_y, black_count=black, **kw)
    return got.cpu().numpy(), black.cpu().numpy()


@pytest.mark.parametrize("kind", ["mesh+0.3", "mesh-0.3"])
@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_the_shifted_maps_leave_a_border(shape, kind):
    """On the model alone: a shift of 0.3 moves the picture by 15 % of each side, so at least 5 % of the luma pixels read the border."""
    share = _model(shape, kind)[1].mean()
    print("uncovered luma share %s %s: %.4f" % (shape, kind, share))
    assert share >= 0.05


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_batch_of_two_equals_the_model(cuda, shape, kind):
    """N = 2 (the second frame under other maps, the frames 3 bytes more than a frame apart), planes 3 and 1, border_y 0 and 16."""
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    other = dict(kind="mesh-0.3" if kind != "mesh-0.3" else "mesh+0.3", seed=SEED + 1)
    xm = _t(np.stack([_maps(H, W, kind)[0], _maps(H, W, **other)[0]]), cuda)
    ym = _t(np.stack([_maps(H, W, kind)[1], _maps(H, W, **other)[1]]), cuda)
    for planes in (3, 1):
        nbytes = SH * SW if planes == 1 else SH * SW * 3 // 2
        buf = torch.full((2, nbytes + 3), 77, dtype=torch.uint8, device=cuda)
        buf[0, :nbytes] = _t(_frame(SH, SW)[:nbytes], cuda)
        buf[1, :nbytes] = _t(_frame(SH, SW, SEED + 1)[:nbytes], cuda)
        for border_y in (0, 16):
            black = torch.zeros((2, SH, SW), dtype=torch.int32, device=cuda)
            got = warp.warpRevBundle2_i420(buf, xm, ym, (SH, SW), planes, border_y=border_y, black_count=black)
            assert got.shape == (2, nbytes)
            for n, (want, blk) in enumerate((_model(shape, kind, planes, border_y), _model(shape, planes=planes, border_y=border_y, **other))):
                assert np.array_equal(got[n].cpu().numpy(), want), (planes, border_y, n)
                assert np.array_equal(black[n].cpu().numpy(), blk.astype(np.int32)), (planes, border_y, n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_y_plane_with_border_zero_is_the_source_resolution_remap(cuda, shape, kind):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    got, black = _run(cuda, shape, kind)
    xm, ym = _maps(H, W, kind)
    sblack = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    ref = warp.warpRevBundle2_src(_t(_frame(SH, SW)[:SH * SW].reshape(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda), black_count=sblack)
    assert np.array_equal(got[:SH * SW].reshape(SH, SW), ref.cpu().numpy())
    assert np.array_equal(black, sblack.cpu().numpy())


@pytest.mark.parametrize("kind", ["mesh+0.3", "mesh-0.3"])
@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_a_black_limited_range_frame_stays_black(cuda, shape, kind):
    """Y = 16, U = V = 128 everywhere, border_y = 16: identical under maps that read the border.  (With a zero border Y darkens there.)"""
    from stabnet_amd import warp
    H, W, SH, SW = shape
    frame = np.concatenate([np.full(SH * SW, 16, np.uint8), np.full(SH * SW // 2, 128, np.uint8)])
    xm, ym = _maps(H, W, kind)
    got = warp.warpRevBundle2_i420(_t(frame, cuda), _t(xm, cuda), _t(ym, cuda), (SH, SW), border_y=16).cpu().numpy()
    assert np.array_equal(got, frame)
    zero = warp.warpRevBundle2_i420(_t(frame, cuda), _t(xm, cuda), _t(ym, cuda), (SH, SW), border_y=0).cpu().numpy()
    assert not np.array_equal(zero[:SH * SW], frame[:SH * SW]) and np.array_equal(zero[SH * SW:], frame[SH * SW:])


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_windows(cuda, shape, planes):
    from stabnet_amd.warp import ratio_window
    H, W, SH, SW = shape
    kind = "mesh+0.3"
    null, nblack = _run(cuda, shape, kind, planes, 16)
    # the whole-frame window is the null window
    whole, wblack = _run(cuda, shape, kind, planes, 16, window=(0, 0, SH, SW))
    assert np.array_equal(whole, null) and np.array_equal(wblack, nblack)
    # an even integer window at zoom 1 is the slice, luma and chroma; flush with the bottom right corner, where the border is
    oh, ow = 2 * (SH // 4), 4 * (SW // 8)
    y0, x0 = SH - oh, SW - ow
    assert y0 % 2 == 0 and x0 % 2 == 0
    got, black = _run(cuda, shape, kind, planes, 16, window=(y0, x0, oh, ow), out_size=(oh, ow))
    full, cut = IM.split(null, SH, SW, planes), IM.split(got, oh, ow, planes)
    assert np.array_equal(cut[0], full[0][y0:y0 + oh, x0:x0 + ow]) and np.array_equal(black, nblack[y0:y0 + oh, x0:x0 + ow])
    for c, f in zip(cut[1:], full[1:]):
        assert np.array_equal(c, f[y0 // 2:(y0 + oh) // 2, x0 // 2:(x0 + ow) // 2])
    # the centred 0.8 window at the frame's own size: the model
    win = ratio_window(SH, SW, 0.8)
    got, black = _run(cuda, shape, kind, planes, 16, window=win)
    want, blk = _model(shape, kind, planes, 16, window=win)
    assert np.array_equal(got, want) and np.array_equal(black, blk.astype(np.int32))
    assert not np.array_equal(got, null)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", IM.SHAPES[1:4], ids=IDS[1:4])
def test_guard_bytes_and_buffers_one_byte_off_the_dword_grid(cuda, shape, off):
    """out between guard bytes that stay intact; src and out `off` bytes from an aligned base give the same bytes (off = 1: every plane on
    the one-pixel path, whatever its width)."""
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    nbytes, G = SH * SW * 3 // 2, 64
    want, blk = _model(shape, "mesh-0.3", 3, 16)
    xm, ym = _maps(H, W, "mesh-0.3")
    sbuf = torch.full((off + nbytes,), 255, dtype=torch.uint8, device=cuda)             # ends with the frame's last byte
    sbuf[off:] = _t(_frame(SH, SW), cuda)
    obuf = torch.full((G + off + nbytes + G,), 0xA5, dtype=torch.uint8, device=cuda)
    bbuf = torch.full((G + SH * SW + G,), -7, dtype=torch.int32, device=cuda)
    bbuf[G:G + SH * SW] = 0
    assert sbuf.data_ptr() % 4 == 0 and obuf.data_ptr() % 4 == 0
    out = obuf[G + off:G + off + nbytes]
    got = warp.warpRevBundle2_i420(sbuf[off:], _t(xm, cuda), _t(ym, cuda), (SH, SW), border_y=16, black_count=bbuf[G:G + SH * SW], out=out)
    assert got.data_ptr() == obuf.data_ptr() + G + off
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((obuf[:G + off] == 0xA5).all()) and bool((obuf[G + off + nbytes:] == 0xA5).all())
    assert np.array_equal(bbuf[G:G + SH * SW].cpu().numpy().reshape(SH, SW), blk.astype(np.int32))
    assert bool((bbuf[:G] == -7).all()) and bool((bbuf[G + SH * SW:] == -7).all())


def test_one_pixel_path_by_switch_gives_the_same(cuda, tmp_path):
    """STABNET_REMAP_VEC4=0 (read once per process, so in a child) on the shape whose planes all take the four-pixel path."""
    shape = IM.SHAPES[1]
    H, W, SH, SW = shape
    want, blk = _model(shape, "mesh+0.3", 3, 16)
    xm, ym = _maps(H, W, "mesh+0.3")
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, frame=_frame(SH, SW), x_map=xm, y_map=ym, size=np.array([SH, SW]), planes=3, border_y=16, window=np.full(4, np.nan))
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_REMAP_VEC4="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "remap_i420_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert list(d["names"]) == ["map_shrink_kernel", "remap_i420_kernel"]                 # the call is two launches
    assert np.array_equal(d["out"], want) and np.array_equal(d["black"], blk.astype(np.int32))
    got, black = _run(cuda, shape, "mesh+0.3", 3, 16)                                     # and this process, on the four-pixel path
    assert np.array_equal(got, want) and np.array_equal(black, blk.astype(np.int32))


@pytest.mark.parametrize("shape", [IM.SHAPES[1], IM.SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_captured_in_a_graph_and_replayed_with_changed_maps(cuda, shape):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    nbytes = SH * SW * 3 // 2
    a, b, c = _model(shape, "mesh+0.3", 3, 16), _model(shape, "mesh-0.3", 3, 16), _model(shape, "mesh", 3, 16, seed=SEED + 1)
    src = _t(_frame(SH, SW), cuda)
    xm, ym = (_t(m, cuda) for m in _maps(H, W, "mesh+0.3"))
    out = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=cuda)
    call = lambda: warp.warpRevBundle2_i420(src, xm, ym, (SH, SW), border_y=16, black_count=black, out=out, workspace=ws)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        call()                                                                    # eager once: loads the code objects
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), a[0])
        black.zero_(); out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                       # records only: nothing executes
            call()
        s.synchronize()
        assert int(black.sum()) == 0 and int(out.sum()) == 0
        xm.copy_(_t(_maps(H, W, "mesh-0.3")[0], cuda)); ym.copy_(_t(_maps(H, W, "mesh-0.3")[1], cuda))
        g.replay()
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), b[0]) and np.array_equal(black.cpu().numpy(), b[1].astype(np.int32))
        src.copy_(_t(_frame(SH, SW, SEED + 1), cuda))
        xm.copy_(_t(_maps(H, W, "mesh", SEED + 1)[0], cuda)); ym.copy_(_t(_maps(H, W, "mesh", SEED + 1)[1], cuda))
        g.replay()
        s.synchronize()
    assert np.array_equal(out.cpu().numpy(), c[0])
    assert np.array_equal(black.cpu().numpy(), b[1].astype(np.int32) + c[1].astype(np.int32))


def test_refusals_launch_nothing(cuda):
    import torch
    from stabnet_amd import _lib, warp
    H, W, SH, SW = IM.SHAPES[1]
    nbytes = SH * SW * 3 // 2
    src, (xm, ym) = _t(_frame(SH, SW), cuda), (_t(m, cuda) for m in _maps(H, W, "mesh"))
    out = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=cuda)
    ws = torch.full((2 * (H // 4) * (W // 4),), -3.0, dtype=torch.float32, device=cuda)     # the first launch would write it
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    ok = dict(size=(SH, SW), out=out, workspace=ws, black_count=black)
    for bad in (dict(border_y=256), dict(border_y=-1), dict(planes=2), dict(size=(SH + 2, SW)), dict(size=(SH - 1, SW)), dict(out_size=(SH - 2, SW)),
                dict(window=(0, 0, SH + 1, SW)), dict(window=(0, 0, float("nan"), SW)), dict(window=(0, 0, SH)), dict(rate=0),
                dict(out=out[:-1]), dict(black_count=black[:-1]), dict(black_count=black.float()), dict(workspace=ws[:-1])):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_i420(src, xm, ym, **dict(ok, **bad))
    for args in ((src.cpu(), xm, ym), (src.float(), xm, ym), (src[:-1], xm, ym), (src, xm[:3], ym[:3]), (src, xm, ym[:-1])):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_i420(*args, **ok)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all()) and int(black.sum()) == 0
    warp.warpRevBundle2_i420(src, xm, ym, **ok)
    assert np.array_equal(out.cpu().numpy(), _model(IM.SHAPES[1], "mesh")[0])
