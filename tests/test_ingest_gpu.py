"""GPU: the frame ingest of csrc/ingest.hip against the installed Pillow and the NumPy model of tests/ingest_model.py.

  grey     float32 [N,H,W] equals float32(float64(PIL) * (1./255) - 0.5) BIT FOR BIT, where PIL is the real
           Image.resize(BILINEAR) (+ crop) of the model's fixed-point grey conversion; with the OpenCV 3 and the OpenCV 4 weights
  colour   uint8 [N,H,W,3] equals the model of cv2.resize exactly and lies strictly less than 1.0 grey level from float64 bilinear
  memory   outputs and the 0xA5-filled workspace sit between guard bands that stay intact; runs repeat; batch entries equal single
           calls; any row stride and any base alignment; a captured graph replayed over a changing staging frame gives the eager bytes
  errors   bad arguments are refused with a status before anything is launched
"""
import functools

import numpy as np
import pytest

import ingest_model as M

pytestmark = pytest.mark.gpu
GUARD = 4096


def _ingest(case, gray="cv3"):
    from stabnet_amd.ingest import FrameIngest
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    crop_rate = 1 if (rh, rw, dy, dx) == (H, W, 0, 0) else 0.9          # the case list states the crop_rate window itself
    ing = FrameIngest(sh, sw, C, H, W, crop_rate=crop_rate, gray=gray, batch=N, device="cuda:0")
    assert (ing.rh, ing.rw, ing.dy, ing.dx) == (rh, rw, dy, dx)
    return ing


def _guarded(n, dtype, fill):
    import torch
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda:0")
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n, fill):
    import torch
    ends = torch.cat([whole[:GUARD], whole[GUARD + n:]])
    return bool(torch.isnan(ends).all()) if fill != fill else bool((ends == fill).all())


@functools.lru_cache(maxsize=None)
def _expected(case, kind, gray):
    """(input uint8 [N,sh,sw,C], grey float32 [N,H,W] through the real Pillow, colour uint8 [N,H,W,3] of the model or None)."""
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    imgs = M.make_input(kind, sh, sw, C, N)
    grey = np.stack([M.train_from_u8(M.real_pil_resize(M.grey_u8(im, gray), rh, rw, dy, dx, H, W)) for im in imgs])
    colour = np.stack([M.cv_resize(im, H, W) for im in imgs]) if C == 3 else None
    for a in (imgs, grey, colour):
        if a is not None:
            a.setflags(write=False)
    return imgs, grey, colour


def _run_guarded(ing, u8):
    """grey and colour with output and workspace between guard bands: (grey float32, colour uint8 or None), host arrays."""
    import torch
    n = u8.shape[0]
    ws_n = ing.workspace.numel()
    ws_whole, ing.workspace = _guarded(ws_n, torch.uint8, 0xA5)
    g_whole, g = _guarded(n * ing.H * ing.W, torch.float32, float("nan"))
    got = ing.grey(u8, out=g).cpu().numpy().reshape(n, ing.H, ing.W)
    assert _intact(g_whole, g.numel(), float("nan")), "grey output guard bands"
    assert _intact(ws_whole, ws_n, 0xA5), "workspace guard bands"
    col = None
    if ing.C == 3:
        c_whole, c = _guarded(n * ing.H * ing.W * 3, torch.uint8, 0xA5)
        col = ing.colour(u8, out=c).cpu().numpy().reshape(n, ing.H, ing.W, 3)
        assert _intact(c_whole, c.numel(), 0xA5), "colour output guard bands"
    return got, col


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("kind", M.INPUT_KINDS)
@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_grey_equals_pillow_bit_for_bit_and_colour_equals_the_model(cuda, case, kind):
    import torch
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    imgs, want_grey, want_col = _expected(case, kind, "cv3")
    ing = _ingest(case)
    got, col = _run_guarded(ing, torch.tensor(imgs).to(cuda))
    bad = _bits(got) != _bits(want_grey)
    print("grey %s %s: %d of %d differ from Pillow" % (M.case_id(case), kind, bad.sum(), bad.size))
    assert not np.isnan(got).any()
    assert bad.sum() == 0, "first differing (n, y, x): %s" % np.argwhere(bad)[:5].tolist()
    if C == 3:
        wrong = col != want_col
        dist = max(np.abs(c.astype(np.float64) - M.bilinear_f64(im, H, W)).max() for c, im in zip(col, imgs))
        print("colour %s %s: %d of %d differ from the model; %.3f grey levels from float64 bilinear" % (M.case_id(case), kind, wrong.sum(), wrong.size, dist))
        assert wrong.sum() == 0, "first differing (n, y, x, c): %s" % np.argwhere(wrong)[:5].tolist()
        assert dist < 1.0


@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_grey_with_the_opencv4_weights(cuda, case):
    import torch
    imgs, want_grey, _ = _expected(case, "random", "cv4")
    got, _ = _run_guarded(_ingest(case, "cv4"), torch.tensor(imgs).to(cuda))
    assert np.array_equal(_bits(got), _bits(want_grey))


def test_the_two_weight_sets_are_told_apart():
    """The OpenCV 3 and OpenCV 4 conversions differ in few pixels (a 9x7 frame may have none), so the expectations of the cv4 test
    must not all coincide with the cv3 ones: over the BGR cases they differ somewhere, and on the largest one for certain."""
    differ = {M.case_id(c): not np.array_equal(_expected(c, "random", "cv3")[1], _expected(c, "random", "cv4")[1])
              for c in M.GPU_CASES if c[2] == 3}
    print(differ)
    assert differ[M.case_id(M.GPU_CASES[1])] and sum(differ.values()) >= len(differ) // 2


def test_custom_weights_reach_the_kernel(cuda):
    """The weights are arguments: (0, 0, 1 << 14, 14) picks the red channel."""
    import torch
    case = M.GPU_CASES[0]
    imgs = M.make_input("random", *case[:3])
    from stabnet_amd.ingest import FrameIngest
    ing = FrameIngest(case[0], case[1], 3, case[7], case[8], gray=(0, 0, 1 << 14, 14), device=cuda)
    want = M.train_from_u8(M.real_pil_resize(imgs[0, :, :, 2], case[7], case[8]))
    assert np.array_equal(_bits(ing.grey(torch.tensor(imgs).to(cuda)).cpu().numpy()[0]), _bits(want))


def test_runs_repeat_and_batch_entries_equal_single_calls(cuda):
    import torch
    case = M.GPU_CASES[-1]
    assert case[-1] == 2
    imgs, want_grey, want_col = _expected(case, "random", "cv3")
    ing = _ingest(case)
    u8 = torch.tensor(imgs).to(cuda)
    g1, c1 = ing.grey(u8).cpu().numpy(), ing.colour(u8).cpu().numpy()
    g2, c2 = ing.grey(u8).cpu().numpy(), ing.colour(u8).cpu().numpy()
    assert np.array_equal(_bits(g1), _bits(g2)) and np.array_equal(c1, c2)
    for n in range(2):
        assert np.array_equal(_bits(ing.grey(u8[n]).cpu().numpy()[0]), _bits(g1[n]))
        assert np.array_equal(ing.colour(u8[n:n + 1]).cpu().numpy()[0], c1[n])
    assert not np.array_equal(g1[0], g1[1])
    assert np.array_equal(_bits(g1), _bits(want_grey)) and np.array_equal(c1, want_col)


@pytest.mark.parametrize("case", [M.GPU_CASES[0], M.GPU_CASES[4], M.GPU_CASES[9]], ids=M.case_id)
def test_row_stride_and_base_alignment(cuda, case):
    import torch
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    imgs, want_grey, want_col = _expected(case, "random", "cv3")
    ing = _ingest(case)
    row = sw * C
    for pad, off in ((0, 1), (0, 2), (0, 3), (5, 0), (13, 3), (4, 0)):
        stride = row + pad
        flat = torch.full((off + N * sh * stride + 8,), 0x5A, dtype=torch.uint8, device=cuda)
        view = torch.as_strided(flat, (N, sh, sw, C), (sh * stride, stride, C, 1), off)
        view.copy_(torch.tensor(imgs).to(cuda))
        assert view.data_ptr() % 4 == off % 4 and (pad == 0 or not view.is_contiguous())
        got = ing.grey(view).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want_grey)), (pad, off)
        if C == 3:
            assert np.array_equal(ing.colour(view).cpu().numpy(), want_col), (pad, off)


def test_captured_graph_over_a_changing_staging_frame(cuda):
    import torch
    case = M.GPU_CASES[0]
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    ing = _ingest(case)
    frames = [torch.from_numpy(M.make_input("random", sh, sw, C, 1, seed=s)).to(cuda) for s in range(3)]
    eager = [(ing.grey(f).cpu().numpy(), ing.colour(f).cpu().numpy()) for f in frames]
    assert not np.array_equal(eager[0][0], eager[1][0])
    stage = torch.zeros_like(frames[0])
    g_out = torch.empty((1, H, W), dtype=torch.float32, device=cuda)
    c_out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ing.grey(stage, out=g_out)
        ing.colour(stage, out=c_out)
    for f, (eg, ec) in zip(frames, eager):
        stage.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(g_out.cpu().numpy()), _bits(eg)) and np.array_equal(c_out.cpu().numpy(), ec)


def test_argument_errors_return_a_status_and_launch_nothing(cuda):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr
    case = M.GPU_CASES[9]                                    # the crop_rate window: a non-trivial origin
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    ing = _ingest(case)
    imgs, want_grey, _ = _expected(case, "random", "cv3")
    u8 = torch.tensor(imgs).to(cuda)
    whole, out = _guarded(H * W, torch.float32, float("nan"))
    ws_whole, ws = _guarded(ing.workspace.numel(), torch.uint8, 0xA5)
    L = _lib.lib()

    def grey(**kw):
        a = dict(img=ptr(u8), N=1, sh=sh, sw=sw, C=C, stride=sw * C, wb=1868, wg=9617, wr=4899, shift=14, rh=rh, rw=rw, dy=dy, dx=dx, H=H, W=W,
                 xb=ptr(ing._xb_dev), xk=ptr(ing._xk_dev), xks=ing._xk, yb=ptr(ing._yb_dev), yk=ptr(ing._yk_dev), yks=ing._yk,
                 lut=ptr(ing._lut), out=ptr(out), ws=ptr(ws), wsb=ws.numel(), stream=0, prof=0)
        a.update(kw)
        return L.stabnet_ingest_grey(*a.values())

    for bad in (dict(img=0), dict(out=0), dict(ws=0), dict(lut=0), dict(xb=0), dict(xk=0), dict(yb=0), dict(yk=0), dict(N=0), dict(sh=0),
                dict(sw=0), dict(H=0), dict(W=0), dict(rh=0), dict(C=0), dict(C=2), dict(C=4), dict(dy=rh - H + 1), dict(dx=rw - W + 1),
                dict(dy=-1), dict(H=rh + 1), dict(stride=sw * C - 1), dict(xks=ing._xk + 2), dict(yks=1)):
        assert grey(**bad) == -1, bad
    assert grey(wsb=0) == -3 and grey(wsb=ws.numel() // 4) == -3
    torch.cuda.synchronize()
    assert _intact(whole, out.numel(), float("nan")) and bool(torch.isnan(out).all()), "a refused call wrote to the output"
    assert bool((ws_whole == 0xA5).all()), "a refused call wrote to the workspace"
    assert grey() == 0                                       # and the same arguments, unspoilt, run
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy().reshape(H, W)), _bits(want_grey[0]))
    assert _intact(whole, out.numel(), float("nan")) and _intact(ws_whole, ws.numel(), 0xA5)
    # a tap count over the kernel's bound: 20000 -> 1 is 40001 horizontal taps, the LDS tile holds 8193
    wide = torch.zeros((1, 1, 20000, 1), dtype=torch.uint8, device=cuda)
    assert grey(img=ptr(wide), sh=1, sw=20000, C=1, stride=20000, rh=1, rw=1, dy=0, dx=0, H=1, W=1, xks=40001) == -1
    assert b"taps" in L.stabnet_last_error()

    xo, xc, yo, yc = ing._cv
    c_whole, c_out = _guarded(H * W * 3, torch.uint8, 0xA5)

    def colour(**kw):
        a = dict(img=ptr(u8), N=1, sh=sh, sw=sw, C=3, stride=sw * 3, H=H, W=W, xo=ptr(xo), xc=ptr(xc), yo=ptr(yo), yc=ptr(yc), out=ptr(c_out),
                 stream=0, prof=0)
        a.update(kw)
        return L.stabnet_ingest_colour(*a.values())

    for bad in (dict(img=0), dict(out=0), dict(xo=0), dict(xc=0), dict(yo=0), dict(yc=0), dict(N=0), dict(sh=0), dict(H=0), dict(W=0), dict(C=1),
                dict(C=4), dict(stride=sw * 3 - 1)):
        assert colour(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((c_whole == 0xA5).all()), "a refused call wrote to the colour output"
    assert colour() == 0

    # the Python class: CPU tensors, wrong dtype, wrong shape
    for bad in (u8.cpu(), u8.float(), u8[:, :-1], u8[..., :2], torch.zeros((sh, sw), dtype=torch.uint8, device=cuda)):
        with pytest.raises(_lib.StabnetError):
            ing.grey(bad)
        with pytest.raises(_lib.StabnetError):
            ing.colour(bad)
    with pytest.raises(_lib.StabnetError):
        ing.grey(u8, out=torch.empty((1, H, W), dtype=torch.float64, device=cuda))
    with pytest.raises(_lib.StabnetError):
        _ingest(M.GPU_CASES[4]).colour(torch.zeros((1, 100, 96, 1), dtype=torch.uint8, device=cuda))      # a grey source has no colour frame


def test_profiler_names_the_three_launches(cuda):
    import torch
    from stabnet_amd.deploy import Profiler
    case = M.GPU_CASES[1]
    ing = _ingest(case)
    u8 = torch.tensor(_expected(case, "random", "cv3")[0]).to(cuda)
    prof = Profiler(16, device=cuda)
    ing.grey(u8, prof=prof)
    ing.colour(u8, prof=prof)
    recs = prof.records(raw=True)
    assert [r[0] for r in recs] == ["ingest_grey_rows_kernel", "ingest_grey_cols_kernel", "ingest_colour_kernel"]
    assert all(r[3] > 0 for r in recs)
