"""GPU: the remap at source resolution (csrc/remap.hip, stabnet_warp_rev_bundle2_src) against the NumPy model
(tests/remap_src_model.py): the warped frame, the source-pixel coordinates and the coverage counts bit for bit, through both kernels
(one pixel per thread; four pixels per thread for BGR frames whose width is a multiple of 4), for strided and misaligned sources,
with guards around what is written, inside a captured graph, and every refusal of the entry point."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_src_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# network H, W -> source SH, SW: odd width (general kernel), width % 4 == 0 (vector kernel), tiny, the network's own size, a downscale
SHAPES = [(32, 64, 77, 131), (32, 64, 90, 152), (32, 64, 9, 8), (32, 64, 32, 64), (64, 96, 48, 80)]
SEED = 5


@functools.lru_cache(maxsize=None)
def _case(H, W, SH, SW, shift, C=3, seed=SEED):
    """Inputs and the model's answer, computed once and shared (read-only)."""
    src = np.random.default_rng(seed * 1000 + SH + SW).integers(0, 256, (SH, SW, C), dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=seed, shift=shift)
    want, px, py, blk = M.warp_src(src, xm, ym)
    for a in (src, xm, ym, want, px, py, blk):
        a.setflags(write=False)
    return src, xm, ym, want, px, py, blk


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _kernel_names(cuda, *args, **kw):
    from stabnet_amd import warp
    from stabnet_amd.deploy import Profiler
    prof = Profiler(max_records=16, device=cuda)
    warp.warpRevBundle2_src(*args, prof=prof, **kw)
    return [r[0] for r in prof.records(raw=True)]


@pytest.mark.parametrize("shift", [0.0, 0.45, -0.45])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_source_remap_equals_the_model(cuda, shape, shift):
    import torch
    from stabnet_amd import warp
    H, W, SH, SW = shape
    src, xm, ym, want, px, py, blk = _case(H, W, SH, SW, shift)
    if shift:
        # a visible border on the model's own answer: the BORDER_CONSTANT taps and the coverage rule are exercised
        assert blk.mean() > 0.1 and (want == 0).all(axis=2).mean() > 0.1
    s, x, y = _t(src, cuda), _t(xm, cuda), _t(ym, cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_src(s, x, y, black_count=black, return_maps=True)
    assert got.shape == (SH, SW, 3) and gx.shape == (1, SH, SW)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    # without the optional outputs: the same frame
    assert np.array_equal(warp.warpRevBundle2_src(s, x, y).cpu().numpy(), want)
    # counted a second time: 2 on black pixels, 0 elsewhere
    warp.warpRevBundle2_src(s, x, y, black_count=black)
    assert np.array_equal(black.cpu().numpy(), 2 * blk.astype(np.int32))
    if (SH, SW) == (H, W):
        # at the network's own size the entry is warpRevBundle2, bit for bit
        ref, rx, ry = warp.warpRevBundle2(s, x[None], y[None], return_maps=True)
        assert torch.equal(ref, got) and torch.equal(rx.view(torch.int32), gx.view(torch.int32)) and torch.equal(ry.view(torch.int32), gy.view(torch.int32))


def test_the_two_kernels_are_chosen_by_shape(cuda):
    src, xm, ym = (_t(a, cuda) for a in _case(32, 64, 90, 152, 0.45)[:3])
    assert _kernel_names(cuda, src, xm, ym) == ["map_shrink_kernel", "remap_src4_kernel"]
    src, xm, ym = (_t(a, cuda) for a in _case(32, 64, 77, 131, 0.45)[:3])
    assert _kernel_names(cuda, src, xm, ym) == ["map_shrink_kernel", "remap_src_kernel"]


def test_full_size_once(cuda):
    """288x512 maps, a 1080p frame: many workgroups per row, two column segments of the vector kernel."""
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(288, 512, 1080, 1920, 0.45)
    assert blk.mean() > 0.1
    black = torch.zeros((1080, 1920), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, return_maps=True)
    assert np.array_equal(_bits(gx.cpu().numpy()[0]), _bits(px)) and np.array_equal(_bits(gy.cpu().numpy()[0]), _bits(py))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))


@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_grey_source(cuda, SH, SW):
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(32, 64, SH, SW, -0.45, C=1)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    got = warp.warpRevBundle2_src(_t(src[..., 0], cuda), _t(xm, cuda), _t(ym, cuda), black_count=black)         # [SH, SW]
    assert got.shape == (SH, SW) and np.array_equal(got.cpu().numpy(), want[..., 0])
    got3 = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda))                                   # [SH, SW, 1]
    assert got3.shape == (SH, SW, 1) and np.array_equal(got3.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))


@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_batch_of_two(cuda, SH, SW):
    import torch
    from stabnet_amd import warp
    a, b = _case(32, 64, SH, SW, 0.45), _case(32, 64, SH, SW, -0.45, seed=SEED + 1)
    stack = lambda i: _t(np.stack([a[i], b[i]]), cuda)
    black = torch.zeros((2, SH, SW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_src(stack(0), stack(1), stack(2), black_count=black, return_maps=True)
    for n, c in enumerate((a, b)):
        assert np.array_equal(got[n].cpu().numpy(), c[3]), n
        assert np.array_equal(_bits(gx[n].cpu().numpy()), _bits(c[4])) and np.array_equal(_bits(gy[n].cpu().numpy()), _bits(c[5])), n
        assert np.array_equal(black[n].cpu().numpy(), c[6].astype(np.int32)), n


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("SH,SW,pad", [(77, 131, 7), (90, 152, 5), (90, 152, 8), (9, 8, 1)])
def test_strided_and_misaligned_sources(cuda, SH, SW, pad, off):
    """Rows `stride` > SW * C bytes apart in a buffer that ENDS with the frame's last byte and starts `off` bytes before its first: the
    vector kernel keeps its dword loads inside the frame's own bytes (an odd stride puts rows at every alignment)."""
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(32, 64, SH, SW, 0.45 if off % 2 else -0.45)
    stride = SW * 3 + pad
    nbytes = (SH - 1) * stride + SW * 3
    buf = torch.full((off + nbytes,), 255, dtype=torch.uint8, device=cuda)
    view = torch.as_strided(buf, (1, SH, SW, 3), (SH * stride, stride, 3, 1), storage_offset=off)
    view.copy_(_t(src, cuda)[None])
    before = buf.clone()
    black = torch.zeros((1, SH, SW), dtype=torch.int32, device=cuda)
    if SW % 4 == 0:
        assert _kernel_names(cuda, view, _t(xm, cuda), _t(ym, cuda))[-1] == "remap_src4_kernel"
    got = warp.warpRevBundle2_src(view, _t(xm, cuda), _t(ym, cuda), black_count=black)
    assert view.data_ptr() == buf.data_ptr() + off                         # read where it lies: no dense copy was made
    assert np.array_equal(got.cpu().numpy()[0], want)
    assert np.array_equal(black.cpu().numpy()[0], blk.astype(np.int32))
    assert torch.equal(buf, before)


@pytest.mark.parametrize("out_off", [64, 61])        # 4-byte aligned: the vector kernel's dword stores; 61: the byte stores
@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_nothing_is_written_outside(cuda, SH, SW, out_off):
    import torch
    from stabnet_amd import warp
    src, xm, ym, want, px, py, blk = _case(32, 64, SH, SW, 0.45)
    n, G = SH * SW * 3, 128
    obuf = torch.full((out_off + n + G,), 0xA5, dtype=torch.uint8, device=cuda)
    bbuf = torch.full((G + SH * SW + G,), -7, dtype=torch.int32, device=cuda)
    bbuf[G:G + SH * SW] = 0
    out, black = obuf[out_off:out_off + n], bbuf[G:G + SH * SW]
    got = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy().reshape(SH, SW, 3), want)
    assert bool((obuf[:out_off] == 0xA5).all()) and bool((obuf[out_off + n:] == 0xA5).all())
    assert np.array_equal(black.cpu().numpy().reshape(SH, SW), blk.astype(np.int32))
    assert bool((bbuf[:G] == -7).all()) and bool((bbuf[G + SH * SW:] == -7).all())


@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_nan_and_huge_map_entries_are_black(cuda, SH, SW):
    import torch
    from stabnet_amd import warp
    src, xm, ym = _case(32, 64, SH, SW, 0.0)[:3]
    xm, ym = xm.copy(), ym.copy()
    xm[5, 9], xm[21, 41], ym[13, 50], ym[29, 5] = np.nan, 1e30, -1e30, np.nan      # entries the 4x shrink samples (rows, columns 4k + 1, 4k + 2)
    want, px, py, blk = M.warp_src(src, xm, ym)
    assert np.isnan(px).any() and np.isnan(py).any() and blk.any() and not blk.all()
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    got, gx, gy = warp.warpRevBundle2_src(_t(src, cuda), _t(xm, cuda), _t(ym, cuda), black_count=black, return_maps=True)
    assert np.array_equal(gx.cpu().numpy()[0], px, equal_nan=True) and np.array_equal(gy.cpu().numpy()[0], py, equal_nan=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(black.cpu().numpy(), blk.astype(np.int32))
    assert (want[np.isnan(px) | np.isnan(py)] == 0).all()


def test_general_kernel_by_switch_gives_the_same(cuda, tmp_path):
    """STABNET_REMAP_VEC4=0 (read once per process, so in a child): the one-pixel kernel on a shape the vector kernel would take."""
    src, xm, ym, want, px, py, blk = _case(32, 64, 90, 152, 0.45)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, src=src, x_map=xm, y_map=ym)
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_REMAP_VEC4="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "remap_src_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert list(d["names"]) == ["map_shrink_kernel", "remap_src_kernel"]
    assert np.array_equal(d["out"], want) and np.array_equal(d["black"], blk.astype(np.int32))
    assert np.array_equal(_bits(d["px"][0]), _bits(px)) and np.array_equal(_bits(d["py"][0]), _bits(py))


@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_captured_in_a_graph_and_replayed(cuda, SH, SW):
    import torch
    from stabnet_amd import warp
    a, b = _case(32, 64, SH, SW, 0.45), _case(32, 64, SH, SW, 0.45, seed=SEED + 1)
    src, xm, ym = _t(a[0], cuda), _t(a[1], cuda), _t(a[2], cuda)
    out = torch.zeros((SH, SW, 3), dtype=torch.uint8, device=cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        warp.warpRevBundle2_src(src, xm, ym, black_count=black, out=out)           # eager once: loads the code objects
        s.synchronize()
        black.zero_(); out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                        # records only: nothing executes
            warp.warpRevBundle2_src(src, xm, ym, black_count=black, out=out)
        s.synchronize()
        assert int(black.sum()) == 0 and int(out.sum()) == 0
        g.replay()
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), a[3]) and np.array_equal(black.cpu().numpy(), a[6].astype(np.int32))
        src.copy_(_t(b[0], cuda)); xm.copy_(_t(b[1], cuda)); ym.copy_(_t(b[2], cuda))
        g.replay()
        s.synchronize()
    assert np.array_equal(out.cpu().numpy(), b[3])
    assert np.array_equal(black.cpu().numpy(), a[6].astype(np.int32) + b[6].astype(np.int32))


def test_every_refusal_raises_and_launches_nothing(cuda):
    import torch
    from stabnet_amd import _lib, warp
    from stabnet_amd._tensor import ptr, stream_ptr
    H, W, SH, SW = 32, 64, 77, 131
    src, xm, ym = (_t(a, cuda) for a in _case(H, W, SH, SW, 0.0)[:3])
    out = torch.full((SH, SW, 3), 0xA5, dtype=torch.uint8, device=cuda)
    ws = torch.full((2 * (H // 4) * (W // 4),), -3.0, dtype=torch.float32, device=cuda)     # the first launch would write it
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    pxy = torch.zeros((SH, SW), dtype=torch.float32, device=cuda)
    good = dict(src=ptr(src), N=1, SH=SH, SW=SW, C=3, stride=SW * 3, x_map=ptr(xm), y_map=ptr(ym), H=H, W=W, rate=4, out=ptr(out),
                black=ptr(black), ws=ptr(ws), px=0, py=0, stream=stream_ptr(cuda), prof=0)
    bads = [dict(src=0), dict(x_map=0), dict(y_map=0), dict(out=0), dict(ws=0), dict(C=0), dict(C=2), dict(C=4), dict(N=0), dict(N=65536),
            dict(SH=0), dict(SW=0), dict(SH=32768), dict(SW=32768), dict(H=3), dict(W=3), dict(H=0), dict(rate=0), dict(rate=33),
            dict(stride=SW * 3 - 1), dict(px=ptr(pxy)), dict(py=ptr(pxy))]
    for bad in bads:
        with pytest.raises(_lib.StabnetError, match="warp_rev_bundle2_src"):
            _lib.call("stabnet_warp_rev_bundle2_src", *dict(good, **bad).values(), device=cuda)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all()) and int(black.sum()) == 0
    # the Python layer's own refusals
    for args, kw in (((src.cpu(), xm, ym), {}), ((src.float(), xm, ym), {}), ((src[:, :, :2], xm, ym), {}), ((src, xm[None].repeat(2, 1, 1), ym), {}),
                     ((src, xm, ym[:-1]), {}), ((src, xm[:3], ym[:3]), {}), ((src, xm, ym), dict(out=out[:-1])),
                     ((src, xm, ym), dict(out=out.cpu())), ((src, xm, ym), dict(black_count=black.float())),
                     ((src, xm, ym), dict(black_count=black[:-1])), ((src, xm, ym), dict(rate=0))):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_src(*args, **kw)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == -3.0).all()) and int(black.sum()) == 0
    # and the good call goes through
    _lib.call("stabnet_warp_rev_bundle2_src", *good.values(), device=cuda)
    assert np.array_equal(out.cpu().numpy(), _case(H, W, SH, SW, 0.0)[3])
