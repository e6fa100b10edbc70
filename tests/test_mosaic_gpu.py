"""GPU: csrc/mosaic.hip against tests/mosaic_model.py, BIT FOR BIT: the composite's canvas, ages and counts from both kernels (four
pixels per thread at 36 x 52, one pixel per thread at 37 x 45 and on misaligned coordinates), and the guard's kept rows."""
import functools

import numpy as np
import pytest

import mosaic_cases as C
import mosaic_model as MM

pytestmark = pytest.mark.gpu
F = np.float32
NET = (24, 40)                                              # the network's size beside the canvases below: the constants are not 1
NAMES = ["identity", "integer", "subpixel", "perspective", "w_crosses"]
KNOBS = [(0, 1), (3, 64), (6, 254)]                         # (feather_log2, max_age)


@functools.lru_cache(maxsize=None)
def case(N, SH, SW):
    d = C.compose_case(N, SH, SW, seed=100 * N + SW)
    for v in d.values():
        v.setflags(write=False)
    return d


def hm_of(N, SH, SW, name):
    """Stream 0 gets `name`, stream 1 the next one in the list: a launch must read its own stream's."""
    hs = C.homographies(SH, SW)
    return np.stack([hs[NAMES[(NAMES.index(name) + n) % len(NAMES)]] for n in range(N)])


@functools.lru_cache(maxsize=None)
def model(N, SH, SW, name, status, fl, max_age):
    d = case(N, SH, SW)
    return MM.compose_batch(d["warped"], d["px"], d["py"], d["canvas_prev"], d["age_prev"], hm_of(N, SH, SW, name), status, *NET,
                            feather_log2=fl, max_age=max_age)


def device(cuda, N, SH, SW, Hm, status, fl, max_age, misalign=False):
    import torch
    from stabnet_amd import mosaic
    d = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in case(N, SH, SW).items()}
    if misalign:                                            # px four bytes off a 16-byte boundary: the one-pixel kernel
        big = torch.empty(N * SH * SW + 1, dtype=torch.float32, device=cuda)
        big[1:].copy_(d["px"].reshape(-1))
        d["px"] = big[1:].view(N, SH, SW)
        assert d["px"].data_ptr() % 16 == 4 and d["px"].is_contiguous()
    out = mosaic.compose(d["warped"], d["px"], d["py"], d["canvas_prev"], d["age_prev"], torch.from_numpy(Hm).to(cuda),
                         torch.tensor(status, dtype=torch.int32, device=cuda), *NET, feather_log2=fl, max_age=max_age)
    return [t.cpu().numpy() for t in out]


def same(got, want, what):
    for g, w, name in zip(got, want, ("canvas", "age", "counts")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("size", [(36, 52), (37, 45)], ids=["36x52-four", "37x45-one"])
def test_compose_equals_the_model(cuda, size, N):
    SH, SW = size
    for name in NAMES:
        for fl, max_age in KNOBS:
            status = tuple([1, 2][:N])
            got = device(cuda, N, SH, SW, hm_of(N, SH, SW, name), status, fl, max_age)
            want = model(N, SH, SW, name, status, fl, max_age)
            same(got, want, (name, fl, max_age))
            assert (got[2].sum(axis=1) == SH * SW).all()
    # every class occurs, so do blended pixels on both sides of the age rule
    c = model(N, SH, SW, "subpixel", tuple([1, 2][:N]), 3, 64)[2]
    assert (c > 0).all(), c


@pytest.mark.parametrize("status", [(0, 1), (2, 0), (0, 0), (3, -1)])
@pytest.mark.parametrize("size", [(36, 52), (37, 45)], ids=["36x52-four", "37x45-one"])
def test_compose_status(cuda, size, status):
    SH, SW = size
    got = device(cuda, 2, SH, SW, hm_of(2, SH, SW, "subpixel"), status, 3, 64)
    same(got, model(2, SH, SW, "subpixel", status, 3, 64), status)
    for n, s in enumerate(status):
        assert (got[2][n, 1] + got[2][n, 2] > 0) == (s in (1, 2))           # no model: nothing blended, nothing from history


@pytest.mark.parametrize("N", [1, 2])
def test_the_two_kernels_agree(cuda, N):
    for name, (fl, max_age) in zip(NAMES, KNOBS + KNOBS):
        status = tuple([1, 2][:N])
        four = device(cuda, N, 36, 52, hm_of(N, 36, 52, name), status, fl, max_age)
        one = device(cuda, N, 36, 52, hm_of(N, 36, 52, name), status, fl, max_age, misalign=True)
        same(one, four, name)
        same(one, model(N, 36, 52, name, status, fl, max_age), name)


def test_graph_replay_follows_hm_in_device_memory(cuda):
    import torch
    from stabnet_amd import mosaic
    N, SH, SW = 2, 36, 52
    d = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in case(N, SH, SW).items()}
    Hm = torch.from_numpy(hm_of(N, SH, SW, "identity")).to(cuda)
    status = torch.tensor([1, 1], dtype=torch.int32, device=cuda)
    canvas, age = torch.empty_like(d["canvas_prev"]), torch.empty_like(d["age_prev"])
    counts = torch.zeros((N, 4), dtype=torch.int32, device=cuda)
    run = lambda: mosaic.compose(d["warped"], d["px"], d["py"], d["canvas_prev"], d["age_prev"], Hm, status, *NET, canvas_cur=canvas,
                                 age_cur=age, counts=counts)
    run()                                                                       # code objects load outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        counts.zero_()
        run()
    for name, st in (("identity", (1, 1)), ("subpixel", (1, 2)), ("perspective", (0, 1)), ("identity", (1, 1))):
        Hm.copy_(torch.from_numpy(hm_of(N, SH, SW, name)).to(cuda))             # changed in device memory, after the capture
        status.copy_(torch.tensor(st, dtype=torch.int32, device=cuda))
        canvas.fill_(9); age.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        same([canvas.cpu().numpy(), age.cpu().numpy(), counts.cpu().numpy()], model(N, SH, SW, name, st, 3, 64), (name, st))


def test_compose_python_argument_checks(cuda):
    import torch
    from stabnet_amd import mosaic
    from stabnet_amd._lib import StabnetError
    d = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in case(1, 36, 52).items()}
    Hm, st = torch.zeros((1, 9), device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    with pytest.raises(StabnetError, match="px"):
        mosaic.compose(d["warped"], d["px"][:, :, :48], d["py"], d["canvas_prev"], d["age_prev"], Hm, st, *NET)
    with pytest.raises(StabnetError, match="GPU"):
        mosaic.compose(d["warped"].cpu(), d["px"], d["py"], d["canvas_prev"], d["age_prev"], Hm, st, *NET)
    with pytest.raises(StabnetError, match="previous"):
        mosaic.compose(d["warped"], d["px"], d["py"], d["canvas_prev"], d["age_prev"], Hm, st, *NET, canvas_cur=d["canvas_prev"])
    with pytest.raises(StabnetError, match="feather_log2"):
        mosaic.compose(d["warped"], d["px"], d["py"], d["canvas_prev"], d["age_prev"], Hm, st, *NET, feather_log2=7)


# ---- the guard -----------------------------------------------------------------------------------------------------------------------

GH, GW = 72, 96


def guard_inputs(B, M, seed):
    r = np.random.default_rng(seed)
    px, py = r.integers(0, GW, (B, M, 2)).astype(np.float64), r.integers(0, GH, (B, M, 2)).astype(np.float64)
    px[:, ::7, 0], py[:, 1::7, 1], px[:, 2::11, 1] = 0, GH - 1, GW - 1           # ends on the image edge
    px[:, 3::13, 0] = GW + 3                                                    # and outside
    rows = np.stack([2 * px[..., 0] / GW - 1, 2 * py[..., 0] / GH - 1, 2 * px[..., 1] / GW - 1, 2 * py[..., 1] / GH - 1], axis=-1).astype(F)
    rows[:, 5::17, 2] = np.nan
    blacks = []
    for _ in range(2):
        b = np.ones((B, GH, GW), F)
        for k in range(B):
            l, rr, t, bt = r.integers(2, 12, 4)
            b[k, t:GH - bt, l:GW - rr] = r.random((GH - t - bt, GW - l - rr)).astype(F) * F(0.49)
            b[k, GH // 2, GW // 3] = 0.5
        blacks.append(b)
    return rows, blacks[0], blacks[1]


@pytest.mark.parametrize("g", [0, 8, 16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [4, 577, 1024])
def test_guard_equals_the_model(cuda, M, B, g):
    import torch
    from stabnet_amd import mosaic
    rows, b0, b1 = guard_inputs(B, M, seed=M + B)
    tb0, tb1 = torch.from_numpy(b0).to(cuda), torch.from_numpy(b1).to(cuda)
    for n0 in sorted({0, 1, min(255, M), min(256, M), min(257, M), M}):
        n = np.array([n0, M, max(n0 - 1, 0)][:B], np.int32)
        poisoned = rows.copy()
        for k in range(B):
            poisoned[k, n[k]:] = np.nan                                         # NaN past row n: never read, never written out
        out, kn = mosaic.guard_matches(torch.from_numpy(poisoned).to(cuda), torch.from_numpy(n).to(cuda), tb0, tb1, g)
        want, wn = MM.guard_batch(poisoned, n, b0, b1, g)
        out, kn = out.cpu().numpy(), kn.cpu().numpy()
        assert np.array_equal(kn, wn) and kn.dtype == np.int32, (n0, kn, wn)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (n0, g)
        assert not np.isnan(out).any()
    if M >= 577:
        assert 0 < wn[min(1, B - 1)] < M                                        # some rows kept, some dropped


def test_guard_graph_capture_and_argument_checks(cuda):
    import torch
    from stabnet_amd import mosaic
    from stabnet_amd._lib import StabnetError
    rows, b0, b1 = guard_inputs(3, 577, seed=9)
    n = np.array([577, 300, 0], np.int32)
    r, k, tb0, tb1 = (torch.from_numpy(a).to(cuda) for a in (rows, n, b0, b1))
    out, kn = torch.empty_like(r), torch.empty_like(k)
    mosaic.guard_matches(r, k, tb0, tb1, 8, out=out, out_n=kn)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mosaic.guard_matches(r, k, tb0, tb1, 8, out=out, out_n=kn)
    out.fill_(7); kn.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    want, wn = MM.guard_batch(rows, n, b0, b1, 8)
    assert np.array_equal(kn.cpu().numpy(), wn) and np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(StabnetError, match="must not be matches"):
        mosaic.guard_matches(r, k, tb0, tb1, 8, out=r)
    with pytest.raises(StabnetError, match="guard must be"):
        mosaic.guard_matches(r, k, tb0, tb1, 17)
    with pytest.raises(StabnetError, match="black0 and black1"):
        mosaic.guard_matches(r, k, tb0[:2], tb1, 8)
