"""GPU: adaptive borderless output (csrc/remap.hip).  stabnet_fill_window_update against the NumPy model (tests/fill_adaptive_model.py):
key, bad-node count, state and window compared with ==, eagerly and replayed from a captured graph.  stabnet_warp_rev_bundle2_win_dev
against stabnet_warp_rev_bundle2_win on the device, same window: frame, coordinates and counts bit for bit, through both kernels.
And the two together: the window the GPU chooses shows no uncovered pixel whenever the rule finds a ratio >= r_min."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fill_adaptive_model as FM
import remap_src_model as M
import remap_win_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "%dx%d-%dx%d" % s
H, W = 32, 64


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _maps(NH, NW, seed, shift, scale=0.06):
    xm, ym = M.mesh_maps(NH, NW, seed, shift=shift, scale=scale)
    xm.setflags(write=False); ym.setflags(write=False)
    return xm, ym


@functools.lru_cache(maxsize=None)
def _src(SH, SW, C=3):
    a = np.random.default_rng(SH * 7 + SW).integers(0, 256, (SH, SW, C), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _update(cuda, xms, yms, SH, SW, states, **params):
    """One call of the entry on a batch -> (state [N], window [N,4], stats [N,2]) as NumPy."""
    import torch
    from stabnet_amd import warp
    N = len(states)
    state = torch.tensor(list(states), dtype=torch.float64, device=cuda)
    window = torch.full((N, 4), -1.0, dtype=torch.float64, device=cuda)
    stats = torch.full((N, 2), -1, dtype=torch.int32, device=cuda)
    got = warp.fill_window_update(_t(np.stack(xms), cuda), _t(np.stack(yms), cuda), SH, SW, state, window, stats, **params)
    assert got is window
    return state.cpu().numpy(), window.cpu().numpy(), stats.cpu().numpy()


def _check(got, n, want):
    """(state, window, stats)[n] == the model's (r, window, key, count), exactly."""
    state, window, stats = got
    r, win, key, cnt = want
    assert (int(stats[n, 0]), int(stats[n, 1])) == (key, cnt), (stats[n], key, cnt)
    assert float(state[n]) == r, (float(state[n]), r)
    assert tuple(float(v) for v in window[n]) == win, (window[n], win)


@pytest.mark.parametrize("state0", [1.0, 0.7])
@pytest.mark.parametrize("shift", [0.0, 0.1, -0.2, 0.45])
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_update_equals_the_model(cuda, shape, shift, state0):
    """8x16 nodes (fewer than a workgroup), 16x24, 9x13 (odd, no multiple of a wave), to several source sizes."""
    NH, NW, SH, SW = shape
    xm, ym = _maps(NH, NW, NH + SW, shift)
    _check(_update(cuda, [xm], [ym], SH, SW, [state0]), 0, FM.frame(xm, ym, SH, SW, state0))


def test_full_size_maps_once(cuda):
    """288x512 maps to 1080p: 9216 nodes, so every thread strides over nine of them."""
    NH, NW, SH, SW = M.BIG
    for shift, scale in ((0.05, 0.06), (0.0, 0.02)):
        xm, ym = _maps(NH, NW, 3, shift, scale)
        want = FM.frame(xm, ym, SH, SW, 1.0)
        print("288x512 -> 1080p, shift %g scale %g: key %d, %d bad nodes, r %.6f" % (shift, scale, want[2], want[3], want[0]))
        _check(_update(cuda, [xm], [ym], SH, SW, [1.0]), 0, want)
    assert 0 < want[3] < 72 * 128 and 0.5 < want[0] < 1.0           # the last one: some bad nodes, a window between r_min and 1


def test_batch_of_two_streams_with_their_own_maps_and_states(cuda):
    NH, NW, SH, SW = M.SHAPES[1]
    a, b = _maps(NH, NW, 1, 0.1), _maps(NH, NW, 2, 0.0)
    got = _update(cuda, [a[0], b[0]], [a[1], b[1]], SH, SW, [1.0, 0.6], up=0.01)
    wa, wb = FM.frame(a[0], a[1], SH, SW, 1.0, up=0.01), FM.frame(b[0], b[1], SH, SW, 0.6, up=0.01)
    assert wa[2:] != wb[2:]
    _check(got, 0, wa); _check(got, 1, wb)


@pytest.mark.parametrize("shape", M.SHAPES[:3], ids=ids)
def test_identity_and_everything_bad(cuda, shape):
    NH, NW, SH, SW = shape
    h, w = NH // 4, NW // 4
    xm, ym = M.identity_maps(NH, NW)
    got = _update(cuda, [xm], [ym], SH, SW, [0.9], up=0.03)
    assert tuple(got[2][0]) == (h * w, 0) and float(got[0][0]) == 0.9 + 0.03
    _check(got, 0, FM.frame(xm, ym, SH, SW, 0.9, up=0.03))
    got = _update(cuda, [xm], [ym], SH, SW, [0.99], up=0.03)                  # never above 1
    assert float(got[0][0]) == 1.0 and tuple(got[1][0]) == (0.0, 0.0, float(SH), float(SW))
    xs, ys = (xm + np.float32(3.0)).astype(np.float32), (ym + np.float32(3.0)).astype(np.float32)
    got = _update(cuda, [xs], [ys], SH, SW, [1.0], r_min=0.4)
    assert int(got[2][0, 1]) == h * w and int(got[2][0, 0]) < 0 and float(got[0][0]) == 0.4
    _check(got, 0, FM.frame(xs, ys, SH, SW, 1.0, r_min=0.4))


def test_margin_and_parameters_travel(cuda):
    NH, NW, SH, SW = M.SHAPES[2]
    xm, ym = _maps(NH, NW, 4, 0.1)
    seen = set()
    for mq in (0, 8, 64, 16 * SH):
        want = FM.frame(xm, ym, SH, SW, 1.0, r_min=0.3, up=0.0, margin_q=mq)
        _check(_update(cuda, [xm], [ym], SH, SW, [1.0], r_min=0.3, up=0.0, margin_q=mq), 0, want)
        seen.add(want[3])
    assert len(seen) >= 3                                                     # the margin changed which nodes are bad


def test_nan_and_huge_map_entries_are_bad_nodes(cuda):
    SH, SW = 77, 131
    base = M.identity_maps(H, W)
    xm, ym = base[0].copy(), base[1].copy()
    xm[9, 21], xm[21, 41], ym[13, 37], ym[17, 25] = np.nan, 1e30, -1e30, np.nan      # entries the 4x shrink samples (rows, columns 4k + 1, 4k + 2)
    bad = FM.bad_nodes(xm, ym, SH, SW)
    assert bad.sum() == 4 and bad[2, 5] and bad[5, 10] and bad[3, 9] and bad[4, 6]
    _check(_update(cuda, [xm], [ym], SH, SW, [1.0], r_min=0.1), 0, FM.frame(xm, ym, SH, SW, 1.0, r_min=0.1))
    for k, (i, j, v) in enumerate(((9, 21, np.nan), (21, 41, 1e30), (13, 37, -1e30))):
        xm, ym = base[0].copy(), base[1].copy()
        (xm if k < 2 else ym)[i, j] = v
        want = FM.frame(xm, ym, SH, SW, 1.0, r_min=0.1)
        assert want[3] == 1
        _check(_update(cuda, [xm], [ym], SH, SW, [1.0], r_min=0.1), 0, want)


SEQ_SHIFTS = [0.0, 0.04, 0.1, 0.02, 0.0, 0.0, 0.45, 0.0, 0.0, -0.06, 0.0, 0.0]


def test_a_sequence_eagerly_and_from_a_captured_graph(cuda):
    """12 frames with changing shifts over one state: zooming in at once, back out by `up` per frame; then the same launches captured once
    and replayed 12 times over a fixed map buffer -- the window lives in device memory, so the graph does not freeze it."""
    import torch
    from stabnet_amd import warp
    NH, NW, SH, SW = M.SHAPES[1]
    params = dict(r_min=0.5, up=0.03, margin_q=8)
    frames = [_maps(NH, NW, 7, s) for s in SEQ_SHIFTS]
    want, state = [], 1.0
    for xm, ym in frames:
        w = FM.frame(xm, ym, SH, SW, state, **params)
        want.append(w)
        state = w[0]
    rs = [w[0] for w in want]
    rsafe = [FM.r_safe_of(w[2], NH // 4, NW // 4) for w in want]
    print("r:", rs, "r_safe:", rsafe)
    assert any(b < a for a, b in zip(rs, rs[1:])) and any(r == 0.5 for r in rs)                    # zooms in; is held at r_min
    assert any(b == a + 0.03 and b < s for a, b, s in zip(rs, rs[1:], rsafe[1:]))                  # grows back rate-limited
    af = warp.AdaptiveFill(1, SH, SW, device=cuda, **params)
    xb, yb = torch.empty((1, NH, NW), device=cuda), torch.empty((1, NH, NW), device=cuda)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        for mode in ("eager", "graph"):
            af.state.fill_(0.25)
            af.reset()
            g = None
            if mode == "graph":
                xb.copy_(_t(frames[0][0], cuda)[None]); yb.copy_(_t(frames[0][1], cuda)[None])
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):                                # records only: nothing executes
                    af.update(xb, yb)
                s.synchronize()
                assert float(af.state[0]) == 1.0
            for t, (xm, ym) in enumerate(frames):
                xb.copy_(_t(xm, cuda)[None]); yb.copy_(_t(ym, cuda)[None])
                if g is None:
                    assert af.update(xb, yb) is af.window
                else:
                    g.replay()
                s.synchronize()
                _check((af.state.cpu().numpy(), af.window.cpu().numpy(), af.stats.cpu().numpy()), 0, want[t])


# ---- the remap through a window in device memory, against the host-window entry on the device ----

def _win_windows(SH, SW):
    from stabnet_amd.warp import ratio_window
    return {"whole": (0.0, 0.0, float(SH), float(SW)), "ratio": ratio_window(SH, SW, 0.8),
            "frac": (0.32 * SH, 0.41 * SW, 0.61 * SH, 0.53 * SW)}               # fractional, off-centre, another aspect


def _both(cuda, src, xm, ym, window, out_size, **kw):
    """The host-window entry and the device-window entry on the same inputs -> ((out, px, py, black) of each, as NumPy)."""
    import torch
    from stabnet_amd import warp
    res = []
    N = src.shape[0] if src.dim() == 4 else 1
    for win in (window, torch.tensor(window, dtype=torch.float64, device=cuda)):
        black = torch.zeros((N,) + tuple(out_size), dtype=torch.int32, device=cuda)
        out, px, py = warp.warpRevBundle2_win(src, xm, ym, win, out_size, black_count=black, return_maps=True, **kw)
        res.append((out.cpu().numpy(), px.cpu().numpy(), py.cpu().numpy(), black.cpu().numpy()))
    return res


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert np.array_equal(a[3], b[3])


def _dev_kernel_names(cuda, src, xm, ym, window, out_size):
    import torch
    from stabnet_amd import warp
    from stabnet_amd.deploy import Profiler
    prof = Profiler(max_records=16, device=cuda)
    warp.warpRevBundle2_win(src, xm, ym, torch.tensor(window, dtype=torch.float64, device=cuda), out_size, prof=prof)
    return [r[0] for r in prof.records(raw=True)]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_size", [(60, 96), (61, 97), None], ids=["60x96", "61x97", "source"])
@pytest.mark.parametrize("name", ["whole", "ratio", "frac"])
@pytest.mark.parametrize("SH,SW", [(77, 131), (90, 152)])
def test_device_window_equals_host_window(cuda, SH, SW, name, out_size, C):
    window = _win_windows(SH, SW)[name]
    o = out_size or (SH, SW)
    xm, ym = _maps(H, W, 5, 0.45)
    src, x, y = _t(_src(SH, SW, C), cuda), _t(xm, cuda), _t(ym, cuda)
    host, dev = _both(cuda, src, x, y, window, o)
    assert host[3].any() and not host[3].all()                                  # the border is in the picture: the counts are exercised
    _same(host, dev)
    vec = C == 3 and o[1] % 4 == 0
    assert _dev_kernel_names(cuda, src, x, y, window, o) == ["map_shrink_kernel", "remap_win4_dev_kernel" if vec else "remap_win_dev_kernel"]


@pytest.mark.parametrize("out_size", [(60, 96), (61, 97)], ids=["60x96", "61x97"])
def test_batch_of_two_with_two_windows(cuda, out_size):
    import torch
    from stabnet_amd import warp
    SH, SW = 77, 131
    wins = [_win_windows(SH, SW)["ratio"], _win_windows(SH, SW)["frac"]]
    maps = [_maps(H, W, 5, 0.45), _maps(H, W, 6, 0.0)]
    srcs = [_src(SH, SW), _src(SH, SW)[::-1].copy()]
    src, x, y = _t(np.stack(srcs), cuda), _t(np.stack([m[0] for m in maps]), cuda), _t(np.stack([m[1] for m in maps]), cuda)
    black = torch.zeros((2,) + out_size, dtype=torch.int32, device=cuda)
    out, px, py = warp.warpRevBundle2_win(src, x, y, torch.tensor(wins, dtype=torch.float64, device=cuda), out_size, black_count=black,
                                          return_maps=True)
    assert out.shape == (2,) + out_size + (3,)
    for n in range(2):
        hb = torch.zeros(out_size, dtype=torch.int32, device=cuda)
        h, hx, hy = warp.warpRevBundle2_win(src[n], x[n], y[n], wins[n], out_size, black_count=hb, return_maps=True)
        _same((h.cpu().numpy(), hx.cpu().numpy()[0], hy.cpu().numpy()[0], hb.cpu().numpy()),
              (out[n].cpu().numpy(), px[n].cpu().numpy(), py[n].cpu().numpy(), black[n].cpu().numpy()))
    # one window [4] for the whole batch
    one = warp.warpRevBundle2_win(src, x, y, torch.tensor(wins[0], dtype=torch.float64, device=cuda), out_size)
    assert np.array_equal(one.cpu().numpy(), warp.warpRevBundle2_win(src, x, y, wins[0], out_size).cpu().numpy())


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("SH,SW,pad,out_size", [(77, 131, 7, (60, 96)), (77, 131, 7, (61, 97)), (9, 8, 1, (60, 96))])
def test_strided_and_misaligned_sources(cuda, SH, SW, pad, out_size, off):
    import torch
    window = _win_windows(SH, SW)["frac"]
    xm, ym = _maps(H, W, 5, 0.45 if off % 2 else 0.0)
    stride = SW * 3 + pad
    nbytes = (SH - 1) * stride + SW * 3
    buf = torch.full((off + nbytes,), 255, dtype=torch.uint8, device=cuda)          # ends with the frame's last byte
    view = torch.as_strided(buf, (1, SH, SW, 3), (SH * stride, stride, 3, 1), storage_offset=off)
    view.copy_(_t(_src(SH, SW), cuda)[None])
    before = buf.clone()
    host, dev = _both(cuda, view, _t(xm, cuda)[None], _t(ym, cuda)[None], window, out_size)
    _same(host, dev)
    dense = _both(cuda, _t(_src(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda), window, out_size)[1]
    assert np.array_equal(dev[0][0], dense[0])
    assert torch.equal(buf, before)


@pytest.mark.parametrize("out_off", [64, 61])        # 4-byte aligned: the vector kernel's dword stores; 61: the byte stores
@pytest.mark.parametrize("out_size", [(60, 96), (61, 97)], ids=["60x96", "61x97"])
def test_nothing_is_written_outside(cuda, out_size, out_off):
    import torch
    from stabnet_amd import _lib, warp
    from stabnet_amd._tensor import ptr, stream_ptr
    SH, SW = 77, 131
    OH, OW = out_size
    window = _win_windows(SH, SW)["frac"]
    xm, ym = _maps(H, W, 5, 0.45)
    s, x, y = _t(_src(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda)
    hb = torch.zeros(out_size, dtype=torch.int32, device=cuda)
    want, wx, wy = warp.warpRevBundle2_win(s, x, y, window, out_size, black_count=hb, return_maps=True)
    n, G = OH * OW * 3, 128
    obuf = torch.full((out_off + n + G,), 0xA5, dtype=torch.uint8, device=cuda)
    bbuf = torch.full((G + OH * OW + G,), -7, dtype=torch.int32, device=cuda)
    bbuf[G:G + OH * OW] = 0
    pbuf = torch.full((2, G + OH * OW + G), -9.0, dtype=torch.float32, device=cuda)
    ws = torch.empty((2 * (H // 4) * (W // 4),), dtype=torch.float32, device=cuda)
    wbuf = torch.full((3, 4), -5.0, dtype=torch.float64, device=cuda)
    wbuf[1] = torch.tensor(window, dtype=torch.float64)
    out, black, gx, gy = obuf[out_off:out_off + n], bbuf[G:G + OH * OW], pbuf[0, G:G + OH * OW], pbuf[1, G:G + OH * OW]
    _lib.call("stabnet_warp_rev_bundle2_win_dev", ptr(s), 1, SH, SW, 3, SW * 3, ptr(x), ptr(y), H, W, 4, ptr(wbuf[1]), OH, OW,
              ptr(out), ptr(black), ptr(ws), ptr(gx), ptr(gy), stream_ptr(cuda), 0, device=cuda)
    assert torch.equal(out.view(OH, OW, 3), want)
    assert bool((obuf[:out_off] == 0xA5).all()) and bool((obuf[out_off + n:] == 0xA5).all())
    assert torch.equal(black.view(OH, OW), hb)
    assert bool((bbuf[:G] == -7).all()) and bool((bbuf[G + OH * OW:] == -7).all())
    assert np.array_equal(_bits(gx.cpu().numpy()), _bits(wx.cpu().numpy().ravel())) and np.array_equal(_bits(gy.cpu().numpy()), _bits(wy.cpu().numpy().ravel()))
    assert bool((pbuf[:, :G] == -9.0).all()) and bool((pbuf[:, G + OH * OW:] == -9.0).all())
    assert bool((wbuf[0] == -5.0).all()) and bool((wbuf[2] == -5.0).all()) and tuple(wbuf[1].tolist()) == tuple(window)


@pytest.mark.parametrize("out_size", [(60, 96), (61, 97)], ids=["60x96", "61x97"])
def test_a_window_the_host_would_refuse_gives_the_whole_frame(cuda, out_size):
    import torch
    from stabnet_amd import warp
    SH, SW = 77, 131
    xm, ym = _maps(H, W, 5, 0.45)
    s, x, y = _t(_src(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda)
    hb = torch.zeros(out_size, dtype=torch.int32, device=cuda)
    want, wx, wy = warp.warpRevBundle2_win(s, x, y, (0, 0, SH, SW), out_size, black_count=hb, return_maps=True)
    ref = (want.cpu().numpy(), wx.cpu().numpy(), wy.cpu().numpy(), hb.cpu().numpy())
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 0, SH, SW), (0, nan, SH, SW), (0, 0, nan, SW), (0, 0, SH, nan), (10, 10, 0, 40), (10, 10, 40, 0), (10, 10, -3, 40),
                (0, 0, inf, SW), (-inf, 0, SH, SW), (0, 0, SH + 1, SW), (-1, 0, SH, SW), (0, 1e300, 5, 5)):
        black = torch.zeros(out_size, dtype=torch.int32, device=cuda)
        got, gx, gy = warp.warpRevBundle2_win(s, x, y, torch.tensor(bad, dtype=torch.float64, device=cuda), out_size, black_count=black,
                                              return_maps=True)
        _same(ref, (got.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy(), black.cpu().numpy()))


def test_general_kernel_by_switch_gives_the_same(cuda, tmp_path):
    """STABNET_REMAP_VEC4=0 (read once per process, so in a child): the one-pixel kernel on a shape the vector kernel would take."""
    SH, SW, o = 90, 152, (60, 96)
    xm, ym = _maps(H, W, 5, 0.45)
    window = _win_windows(SH, SW)["frac"]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, src=_src(SH, SW), x_map=xm, y_map=ym, window=np.array(window, np.float64), out_size=np.array(o))
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_REMAP_VEC4="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fill_adaptive_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert list(d["host_names"]) == ["map_shrink_kernel", "remap_win_kernel"] and list(d["dev_names"]) == ["map_shrink_kernel", "remap_win_dev_kernel"]
    _same(tuple(d["host_" + k] for k in ("out", "px", "py", "black")), tuple(d["dev_" + k] for k in ("out", "px", "py", "black")))
    want = _both(cuda, _t(_src(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda), window, o)[1]        # this process: the vector kernel
    _same((want[0], want[1], want[2], want[3][0]), tuple(d["dev_" + k] for k in ("out", "px", "py", "black")))


def test_python_layer_refuses_bad_window_tensors(cuda):
    import torch
    from stabnet_amd import _lib, warp
    SH, SW = 77, 131
    xm, ym = _maps(H, W, 5, 0.0)
    s, x, y = _t(_src(SH, SW), cuda), _t(xm, cuda), _t(ym, cuda)
    good = torch.tensor((0.0, 0.0, SH, SW), dtype=torch.float64, device=cuda)
    for bad in (good.float(), good.cpu(), good[:3], good[None].repeat(2, 1), good[None, None]):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_win(s, x, y, bad)
    state, window, stats = torch.ones(1, dtype=torch.float64, device=cuda), torch.zeros((1, 4), dtype=torch.float64, device=cuda), \
        torch.zeros((1, 2), dtype=torch.int32, device=cuda)
    for kw in (dict(state=state.float()), dict(state=state.cpu()), dict(window=window[:, :3]), dict(window=window.float()),
               dict(stats=stats.long()), dict(stats=stats[0]), dict(r_min=0.0), dict(up=-1.0), dict(margin_q=16 * SH + 1), dict(rate=0)):
        a = dict(dict(state=state, window=window, stats=stats), **kw)
        with pytest.raises(_lib.StabnetError):
            warp.fill_window_update(x, y, SH, SW, **a)
    torch.cuda.synchronize()
    assert float(state[0]) == 1.0 and not bool(window.any()) and not bool(stats.any())


# ---- the two together ----

@pytest.mark.parametrize("shape", M.SHAPES[:3], ids=ids)
def test_the_chosen_window_shows_no_uncovered_pixel(cuda, shape):
    """The grid of tests/test_fill_adaptive_cpu.py: update, then the remap through the window it wrote.  No uncovered pixel whenever
    r_safe >= r_min; otherwise the window is exactly ratio_window(r_min) and the uncovered count is the model's."""
    import torch
    from stabnet_amd import warp
    NH, NW, SH, SW = shape
    h, w = NH // 4, NW // 4
    r_min = 0.5
    af = warp.AdaptiveFill(1, SH, SW, r_min=r_min, device=cuda)
    src = _t(_src(SH, SW), cuda)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    safe = held = 0
    for seed in range(6):
        for shift in (0.0, 0.1, -0.2, 0.45):
            for scale in (0.06, 0.15):
                xm, ym = _maps(NH, NW, seed, shift, scale)
                x, y = _t(xm, cuda), _t(ym, cuda)
                af.reset()
                black.zero_()
                warp.warpRevBundle2_win(src, x, y, af.update(x, y), black_count=black)
                key, cnt = (int(v) for v in af.stats[0].cpu().numpy())
                assert (key, cnt) == FM.key_of(FM.bad_nodes(xm, ym, SH, SW))
                r_safe = FM.r_safe_of(key, h, w)
                window = tuple(float(v) for v in af.window[0].cpu().numpy())
                uncovered = int(black.sum())
                if r_safe >= r_min:
                    safe += 1
                    assert window == warp.ratio_window(SH, SW, r_safe)
                    assert uncovered == 0, (seed, shift, scale, r_safe, uncovered)
                else:
                    held += 1
                    assert window == warp.ratio_window(SH, SW, r_min)
                    px, py = WM.coords(xm, ym, SH, SW, window, SH, SW)
                    assert uncovered == int(M.black(px, py, SH, SW).sum()), (seed, shift, scale)
    assert safe >= 6 and held >= 6
