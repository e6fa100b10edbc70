"""GPU: the remap through a window (csrc/remap.hip, stabnet_warp_rev_bundle2_win) against the NumPy model (tests/remap_win_model.py):
the cropped-and-zoomed frame, the source-pixel coordinates and the coverage counts at the output pixels bit for bit, through both
kernels (one output pixel per thread; four per thread for BGR outputs whose width is a multiple of 4), against the source-resolution
entry for the whole-frame window and for integer windows at zoom 1, for strided and misaligned sources, with guards around what is
written, inside a captured graph, and every refusal of the entry point."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_src_model as M
import remap_win_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = 32, 64                                                 # the network's size: 8x16 small maps
# sources: odd width, width % 4 == 0, tiny, the network's own size
SOURCES = [(77, 131), (90, 152), (9, 8), (32, 64)]
SHIFTS = [0.0, 0.45]
SEED = 5


def _windows(SH, SW):
    """name -> (window, out_size).  whole: must equal _src; ratio: 0.8 of each side at the source's size; frac-*: a fractional window
    to another size and aspect (96 % 4 == 0: the vector kernel whatever the source's width; 97: the general one); int: an integer window
    at zoom 1, the slice of _src."""
    from stabnet_amd.warp import ratio_window
    ih, iw = max(SH // 2, 1), max(4 * (SW // 8), 1)
    iy, ix = SH - ih, SW - iw                                    # flush with the bottom right corner: where a positive shift leaves the border
    return {"whole": ((0, 0, SH, SW), (SH, SW)), "ratio": (ratio_window(SH, SW, 0.8), (SH, SW)),
            "frac-60x96": ((0.1 * SH, 0.1 * SW, 0.8 * SH, 0.8 * SW), (60, 96)), "frac-61x97": ((0.1 * SH, 0.1 * SW, 0.8 * SH, 0.8 * SW), (61, 97)),
            "int": ((iy, ix, ih, iw), (ih, iw))}


WINDOWS = ["whole", "ratio", "frac-60x96", "frac-61x97", "int"]


@functools.lru_cache(maxsize=None)
def _inputs(NH, NW, SH, SW, shift, C=3, seed=SEED):
    src = np.random.default_rng(seed * 1000 + SH + SW).integers(0, 256, (SH, SW, C), dtype=np.uint8)
    xm, ym = M.mesh_maps(NH, NW, seed=seed, shift=shift)
    for a in (src, xm, ym):
        a.setflags(write=False)
    return src, xm, ym


@functools.lru_cache(maxsize=None)
def _case(SH, SW, shift, name, C=3, seed=SEED, net=(H, W), window=None, out_size=None):
    """Inputs and the model's answer, computed once and shared (read-only)."""
    src, xm, ym = _inputs(net[0], net[1], SH, SW, shift, C, seed)
    if name is not None:
        window, out_size = _windows(SH, SW)[name]
    want, px, py, blk = WM.warp_win(src, xm, ym, window, out_size)
    for a in (want, px, py, blk):
        a.setflags(write=False)
    return src, xm, ym, window, out_size, want, px, py, blk


@functools.lru_cache(maxsize=None)
def _src_model(SH, SW, shift):
    src, xm, ym = _inputs(H, W, SH, SW, shift)
    return M.warp_src(src, xm, ym)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _kernel_names(cuda, *args, **kw):
    from stabnet_amd import warp
    from stabnet_amd.deploy import Profiler
    prof = Profiler(max_records=16, device=cuda)
    warp.warpRevBundle2_win(*args, prof=prof, **kw)
    return [r[0] for r in prof.records(raw=True)]


def test_the_models_borders_are_where_the_issue_puts_them():
    """Shift 0.45: the 0.8 window of 77x131 is about 30 % black in the model (0.297 measured there), so the border taps and the counts
    are exercised; shift 0: it is fully covered."""
    blk = _case(77, 131, 0.45, "ratio")[8]
    print("black share, shift 0.45, 0.8 window of 77x131: %.4f" % blk.mean())
    assert blk.mean() > 0.1
    assert _case(77, 131, 0.0, "ratio")[8].sum() == 0


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", WINDOWS)
@pytest.mark.parametrize("size", SOURCES, ids=lambda s: "%dx%d" % s)
def test_window_remap_equals_the_model(cuda, size, name, shift):
    import torch
    from stabnet_amd import warp
    SH, SW = size
    src, xm, ym, window, (OH, OW), want, px, py, blk = _case(SH, SW, shift, name)
    s, x, y = _t(src, cuda), _t(xm, cuda), _t(ym, cuda)
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_win(s, x, y, window, (OH, OW), black_count=black, return_maps=True)
    assert got.shape == (OH, OW, 3) and gx.shape == (1, OH, OW)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    # without the optional outputs: the same frame
    assert np.array_equal(warp.warpRevBundle2_win(s, x, y, window, (OH, OW)).cpu().numpy(), want)
    # counted a second time: 2 on black pixels, 0 elsewhere
    warp.warpRevBundle2_win(s, x, y, window, (OH, OW), black_count=black)
    assert np.array_equal(black.cpu().numpy(), 2 * blk.astype(np.int32))
    if name in ("whole", "int"):
        # the source-resolution entry on the device (and its model): the whole frame, or the slice of it
        sblack = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
        ref, rx, ry = warp.warpRevBundle2_src(s, x, y, black_count=sblack, return_maps=True)
        y0, x0 = (int(window[0]), int(window[1]))
        sl = np.s_[y0:y0 + OH, x0:x0 + OW]
        assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()[sl])
        assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(rx.cpu().numpy()[0][sl])) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(ry.cpu().numpy()[0][sl]))
        assert np.array_equal(black.cpu().numpy(), 2 * sblack.cpu().numpy()[sl])
        assert np.array_equal(want, _src_model(SH, SW, shift)[0][sl])
    if name == "whole":
        # out_size defaults to the source's size
        assert np.array_equal(warp.warpRevBundle2_win(s, x, y, window).cpu().numpy(), want)


def test_the_two_kernels_are_chosen_by_shape(cuda):
    import torch
    win4, win1 = ["map_shrink_kernel", "remap_win4_kernel"], ["map_shrink_kernel", "remap_win_kernel"]
    for SH, SW in ((77, 131), (90, 152)):
        src, xm, ym = (_t(a, cuda) for a in _inputs(H, W, SH, SW, 0.45))
        fw = (0.1 * SH, 0.1 * SW, 0.8 * SH, 0.8 * SW)
        # the OUTPUT's width decides, not the source's
        assert _kernel_names(cuda, src, xm, ym, fw, (60, 96)) == win4
        assert _kernel_names(cuda, src, xm, ym, fw, (61, 97)) == win1
        assert _kernel_names(cuda, src, xm, ym, (0, 0, SH, SW)) == (win4 if SW % 4 == 0 else win1)
        # a grey source: the general kernel
        assert _kernel_names(cuda, src[..., :1].contiguous(), xm, ym, fw, (60, 96)) == win1
        # out off the dword grid: the general kernel
        buf = torch.zeros((60 * 96 * 3 + 8,), dtype=torch.uint8, device=cuda)
        assert _kernel_names(cuda, src, xm, ym, fw, (60, 96), out=buf[2:2 + 60 * 96 * 3]) == win1
        assert _kernel_names(cuda, src, xm, ym, fw, (60, 96), out=buf[4:4 + 60 * 96 * 3]) == win4


def test_full_size_once(cuda):
    """288x512 maps, a 1080p frame through the 0.8 window: many workgroups per row, two column segments of the vector kernel."""
    import torch
    from stabnet_amd import warp
    from stabnet_amd.warp import ratio_window
    window = ratio_window(1080, 1920, 0.8)
    src, xm, ym, _, _, want, px, py, blk = _case(1080, 1920, 0.45, None, net=(288, 512), window=window, out_size=(1080, 1920))
    assert blk.mean() > 0.1
    black = torch.zeros((1080, 1920), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_win(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), window, black_count=black, return_maps=True)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))


@pytest.mark.parametrize("name", ["ratio", "frac-60x96"])
@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_grey_source(cuda, SH, SW, name):
    import torch
    from stabnet_amd import warp
    src, xm, ym, window, (OH, OW), want, px, py, blk = _case(SH, SW, 0.45, name, C=1)
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    got = warp.warpRevBundle2_win(_t(src[..., 0], cuda), _t(xm, cuda), _t(ym, cuda), window, (OH, OW), black_count=black)      # [OH, OW]
    assert got.shape == (OH, OW) and np.array_equal(got.cpu().numpy(), want[..., 0])
    got3 = warp.warpRevBundle2_win(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), window, (OH, OW))                                # [OH, OW, 1]
    assert got3.shape == (OH, OW, 1) and np.array_equal(got3.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))


@pytest.mark.parametrize("name", ["ratio", "frac-60x96", "frac-61x97"])
@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_batch_of_two(cuda, SH, SW, name):
    import torch
    from stabnet_amd import warp
    a, b = _case(SH, SW, 0.45, name), _case(SH, SW, 0.0, name, seed=SEED + 1)
    window, (OH, OW) = a[3], a[4]
    stack = lambda i: _t(np.stack([a[i], b[i]]), cuda)
    black = torch.zeros((2, OH, OW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_win(stack(0), stack(1), stack(2), window, (OH, OW), black_count=black, return_maps=True)
    assert got.shape == (2, OH, OW, 3)
    for n, c in enumerate((a, b)):
        assert np.array_equal(got[n].cpu().numpy(), c[5]), n
        assert np.array_equal(_bits(gx[n].cpu().numpy()), _bits(c[6])) and np.array_equal(_bits(gy[n].cpu().numpy()), _bits(c[7])), n
        assert np.array_equal(black[n].cpu().numpy(), c[8].astype(np.int32)), n


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("SH,SW,pad,name", [(77, 131, 7, "frac-60x96"), (77, 131, 7, "frac-61x97"), (90, 152, 5, "ratio"), (90, 152, 8, "whole"),
                                            (9, 8, 1, "whole"), (9, 8, 1, "frac-60x96")])
def test_strided_and_misaligned_sources(cuda, SH, SW, pad, name, off):
    """Rows `stride` > SW * C bytes apart in a buffer that ENDS with the frame's last byte and starts `off` bytes before its first: the
    vector kernel keeps its dword loads inside the frame's own bytes (an odd stride puts rows at every alignment)."""
    import torch
    from stabnet_amd import warp
    src, xm, ym, window, (OH, OW), want, px, py, blk = _case(SH, SW, 0.45 if off % 2 else 0.0, name)
    stride = SW * 3 + pad
    nbytes = (SH - 1) * stride + SW * 3
    buf = torch.full((off + nbytes,), 255, dtype=torch.uint8, device=cuda)
    view = torch.as_strided(buf, (1, SH, SW, 3), (SH * stride, stride, 3, 1), storage_offset=off)
    view.copy_(_t(src, cuda)[None])
    before = buf.clone()
    black = torch.zeros((1, OH, OW), dtype=torch.int32, device=cuda)
    if OW % 4 == 0:
        assert _kernel_names(cuda, view, _t(xm, cuda), _t(ym, cuda), window, (OH, OW))[-1] == "remap_win4_kernel"
    got = warp.warpRevBundle2_win(view, _t(xm, cuda), _t(ym, cuda), window, (OH, OW), black_count=black)
    assert view.data_ptr() == buf.data_ptr() + off                         # read where it lies: no dense copy was made
    assert np.array_equal(got.cpu().numpy()[0], want)
    assert np.array_equal(black.cpu().numpy()[0], blk.astype(np.int32))
    assert torch.equal(buf, before)


@pytest.mark.parametrize("out_off", [64, 61])        # 4-byte aligned: the vector kernel's dword stores; 61: the byte stores
@pytest.mark.parametrize("SH,SW,name", [(77, 131, "frac-60x96"), (77, 131, "frac-61x97"), (90, 152, "ratio")])
def test_nothing_is_written_outside(cuda, SH, SW, name, out_off):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.warp import _check_window
    src, xm, ym, window, (OH, OW), want, px, py, blk = _case(SH, SW, 0.45, name)
    n, G = OH * OW * 3, 128
    obuf = torch.full((out_off + n + G,), 0xA5, dtype=torch.uint8, device=cuda)
    bbuf = torch.full((G + OH * OW + G,), -7, dtype=torch.int32, device=cuda)
    bbuf[G:G + OH * OW] = 0
    pbuf = torch.full((2, G + OH * OW + G), -9.0, dtype=torch.float32, device=cuda)
    ws = torch.empty((2 * (H // 4) * (W // 4),), dtype=torch.float32, device=cuda)
    s, x, y = _t(src, cuda), _t(xm, cuda), _t(ym, cuda)
    out, black, gx, gy = obuf[out_off:out_off + n], bbuf[G:G + OH * OW], pbuf[0, G:G + OH * OW], pbuf[1, G:G + OH * OW]
    _lib.call("stabnet_warp_rev_bundle2_win", ptr(s), 1, SH, SW, 3, SW * 3, ptr(x), ptr(y), H, W, 4, _check_window(window, "test"), OH, OW,
              ptr(out), ptr(black), ptr(ws), ptr(gx), ptr(gy), stream_ptr(cuda), 0, device=cuda)
    assert np.array_equal(out.cpu().numpy().reshape(OH, OW, 3), want)
    assert bool((obuf[:out_off] == 0xA5).all()) and bool((obuf[out_off + n:] == 0xA5).all())
    assert np.array_equal(black.cpu().numpy().reshape(OH, OW), blk.astype(np.int32))
    assert bool((bbuf[:G] == -7).all()) and bool((bbuf[G + OH * OW:] == -7).all())
    assert np.array_equal(_bits(gx.cpu().numpy().reshape(OH, OW)), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy().reshape(OH, OW)), _bits(py))
    assert bool((pbuf[:, :G] == -9.0).all()) and bool((pbuf[:, G + OH * OW:] == -9.0).all())


@pytest.mark.parametrize("SH,SW,name", [(77, 131, "frac-61x97"), (90, 152, "ratio")])
def test_nan_and_huge_map_entries_are_black(cuda, SH, SW, name):
    import torch
    from stabnet_amd import warp
    src, xm, ym = _inputs(H, W, SH, SW, 0.0)
    window, (OH, OW) = _windows(SH, SW)[name]
    xm, ym = xm.copy(), ym.copy()
    xm[9, 21], xm[21, 41], ym[13, 37], ym[17, 25] = np.nan, 1e30, -1e30, np.nan      # entries the 4x shrink samples (rows, columns 4k + 1, 4k + 2), inside the window
    want, px, py, blk = WM.warp_win(src, xm, ym, window, (OH, OW))
    assert np.isnan(px).any() and np.isnan(py).any() and blk.any() and not blk.all()
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_win(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), window, (OH, OW), black_count=black, return_maps=True)
    assert np.array_equal(gx.cpu().numpy()[0], px, equal_nan=True) and np.array_equal(gy.cpu().numpy()[0], py, equal_nan=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    assert (want[np.isnan(px) | np.isnan(py)] == 0).all()


def test_general_kernel_by_switch_gives_the_same(cuda, tmp_path):
    """STABNET_REMAP_VEC4=0 (read once per process, so in a child): the one-pixel kernel on a shape the vector kernel would take."""
    src, xm, ym, window, (OH, OW), want, px, py, blk = _case(90, 152, 0.45, "frac-60x96")
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, src=src, x_map=xm, y_map=ym, window=np.array(window, np.float64), out_size=np.array([OH, OW]))
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_REMAP_VEC4="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "remap_win_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert list(d["names"]) == ["map_shrink_kernel", "remap_win_kernel"]
    assert np.array_equal(d["out"], want) and np.array_equal(d["black"], blk.astype(np.int32))
    assert np.array_equal(_bits(d["px"][0]), _bits(px)) and np.array_equal(_bits(d["py"][0]), _bits(py))


@pytest.mark.parametrize("SH,SW,name", [(77, 131, "frac-61x97"), (90, 152, "ratio")])
def test_captured_in_a_graph_and_replayed(cuda, SH, SW, name):
    import torch
    from stabnet_amd import warp
    a, b = _case(SH, SW, 0.45, name), _case(SH, SW, 0.45, name, seed=SEED + 1)
    window, (OH, OW) = a[3], a[4]
    src, xm, ym = _t(a[0], cuda), _t(a[1], cuda), _t(a[2], cuda)
    out = torch.zeros((OH, OW, 3), dtype=torch.uint8, device=cuda)
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        warp.warpRevBundle2_win(src, xm, ym, window, (OH, OW), black_count=black, out=out)      # eager once: loads the code objects
        s.synchronize()
        black.zero_(); out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                        # records only: nothing executes
            warp.warpRevBundle2_win(src, xm, ym, window, (OH, OW), black_count=black, out=out)
        s.synchronize()
        assert int(black.sum()) == 0 and int(out.sum()) == 0
        g.replay()
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), a[5]) and np.array_equal(black.cpu().numpy(), a[8].astype(np.int32))
        src.copy_(_t(b[0], cuda)); xm.copy_(_t(b[1], cuda)); ym.copy_(_t(b[2], cuda))
        g.replay()
        s.synchronize()
    assert np.array_equal(out.cpu().numpy(), b[5])
    assert np.array_equal(black.cpu().numpy(), a[8].astype(np.int32) + b[8].astype(np.int32))


def test_every_refusal_raises_and_launches_nothing(cuda):
    import ctypes
    import torch
    from stabnet_amd import _lib, warp
    from stabnet_amd._tensor import ptr, stream_ptr
    SH, SW, OH, OW = 77, 131, 60, 96
    src, xm, ym, window, _, want = _case(SH, SW, 0.0, "frac-60x96")[:6]
    src, xm, ym = (_t(a, cuda) for a in (src, xm, ym))
    win = lambda *v: (ctypes.c_double * 4)(*v)
    out = torch.full((OH, OW, 3), 0xA5, dtype=torch.uint8, device=cuda)
    ws = torch.full((2 * (H // 4) * (W // 4),), -3.0, dtype=torch.float32, device=cuda)     # the first launch would write it
    black = torch.zeros((OH, OW), dtype=torch.int32, device=cuda)
    pxy = torch.zeros((OH, OW), dtype=torch.float32, device=cuda)
    good = dict(src=ptr(src), N=1, SH=SH, SW=SW, C=3, stride=SW * 3, x_map=ptr(xm), y_map=ptr(ym), H=H, W=W, rate=4, window=win(*window),
                OH=OH, OW=OW, out=ptr(out), black=ptr(black), ws=ptr(ws), px=0, py=0, stream=stream_ptr(cuda), prof=0)
    inf, nan = float("inf"), float("nan")
    bads = [dict(src=0), dict(x_map=0), dict(y_map=0), dict(out=0), dict(ws=0), dict(C=0), dict(C=2), dict(C=4), dict(N=0), dict(N=65536),
            dict(SH=0), dict(SW=0), dict(SH=32768), dict(SW=32768), dict(H=3), dict(W=3), dict(H=0), dict(rate=0), dict(rate=33),
            dict(stride=SW * 3 - 1), dict(px=ptr(pxy)), dict(py=ptr(pxy)),
            dict(OH=0), dict(OW=0), dict(OH=32768), dict(OW=32768), dict(window=None),
            dict(window=win(nan, 0, SH, SW)), dict(window=win(0, nan, SH, SW)), dict(window=win(0, 0, inf, SW)), dict(window=win(0, 0, SH, nan)),
            dict(window=win(0, 0, 0, SW)), dict(window=win(0, 0, SH, 0)), dict(window=win(0, 0, -1, SW)), dict(window=win(0, 0, SH, -1)),
            dict(window=win(-1e-5, 0, SH, SW)), dict(window=win(0, -1e-5, SH, SW)), dict(window=win(0, 0, SH + 1e-5, SW)),
            dict(window=win(0, 0, SH, SW + 1e-5)), dict(window=win(1, 0, SH, SW)), dict(window=win(0, 1, SH, SW))]
    for bad in bads:
        with pytest.raises(_lib.StabnetError, match="warp_rev_bundle2_win"):
            _lib.call("stabnet_warp_rev_bundle2_win", *dict(good, **bad).values(), device=cuda)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all()) and int(black.sum()) == 0
    # the Python layer's own refusals
    o = (OH, OW)
    for args, kw in (((src.cpu(), xm, ym, window, o), {}), ((src.float(), xm, ym, window, o), {}), ((src[:, :, :2], xm, ym, window, o), {}),
                     ((src, xm[None].repeat(2, 1, 1), ym, window, o), {}), ((src, xm, ym[:-1], window, o), {}), ((src, xm[:3], ym[:3], window, o), {}),
                     ((src, xm, ym, window, o), dict(out=out[:-1])), ((src, xm, ym, window, o), dict(out=out.cpu())),
                     ((src, xm, ym, window, o), dict(black_count=black.float())), ((src, xm, ym, window, o), dict(black_count=black[:-1])),
                     ((src, xm, ym, window, o), dict(rate=0)), ((src, xm, ym, window[:3], o), {}), ((src, xm, ym, None, o), {}),
                     ((src, xm, ym, window, (0, OW)), {}), ((src, xm, ym, (0, 0, SH + 1, SW), o), dict(out=out)),
                     ((src, xm, ym, window), dict(out=out))):                       # out_size defaults to the source's: out is too small
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_win(*args, **kw)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all()) and int(black.sum()) == 0
    # a window that overshoots by a rounding error is accepted; and the good call goes through
    _lib.call("stabnet_warp_rev_bundle2_win", *dict(good, window=win(-5e-7, -5e-7, SH + 1e-6, SW + 1e-6)).values(), device=cuda)
    _lib.call("stabnet_warp_rev_bundle2_win", *good.values(), device=cuda)
    assert np.array_equal(out.cpu().numpy(), want)
