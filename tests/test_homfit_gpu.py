"""GPU: csrc/homfit.hip against tests/homfit_model.py, BIT FOR BIT: Hm (the uint32 images of its float32 values), mask, count, status
and best.  Shapes where the kernel can go wrong: one pair and several with a different n each (0 and 3 among them: no model);
n of 4, 5, 255, 256, 257 (a thread's second row starts at 256) and n = M; M of 4, 577 and 1024 (all of the LDS stage); half of the
rows outliers; 64, 256 and 512 hypotheses (fewer than the threads, one each, two each); the collinear and the identical rows (every
hypothesis divides 0 by 0); 72 x 96 and 40 x 200 pixels (pixel scales that differ along x and y).  Rows from n on are NaN: a kernel
that read one would carry it into its sums.  The call is captured in a graph and replayed twice."""
import functools

import numpy as np
import pytest

import homfit_cases as C
import homfit_model as HM

pytestmark = pytest.mark.gpu
F = np.float32

# name -> (H, W, M, [(what, n, outlier share, noise px)])
CASES = {
    "one_pair_M4": (72, 96, 4, [("translation", 4, 0.0, 0.0)]),
    "three_pairs_M577": (288, 512, 577, [("similarity", 0, 0.0, 0.0), ("perspective", 3, 0.0, 0.0), ("similarity", 300, 0.5, 0.1)]),
    "n_around_256_M1024": (40, 200, 1024, [("perspective", 4, 0.0, 0.1), ("similarity", 5, 0.0, 0.1), ("translation", 255, 0.3, 0.1),
                                           ("similarity", 256, 0.3, 0.1), ("perspective", 257, 0.3, 0.1), ("similarity", 1024, 0.5, 0.1)]),
    "half_outliers_M577": (72, 96, 577, [("similarity", 577, 0.5, 0.1), ("perspective", 60, 0.5, 0.1), ("translation", 200, 0.5, 0.0),
                                         ("perspective", 5, 0.0, 0.0)]),
    "degenerate_M64": (72, 96, 64, [("collinear", 40, 0, 0), ("identical", 30, 0, 0), ("similarity", 64, 0.3, 0.1)]),
    # four of five rows are outliers: the winner comes late (beyond k = 256 with 512 hypotheses) or not at all; nothing is planted to be found
    "mostly_outliers_M256": (72, 96, 256, [("similarity", 200, 0.8, 0.5), ("perspective", 256, 0.8, 0.5), ("translation", 120, 0.8, 0.5),
                                           ("similarity", 90, 0.8, 0.5)]),
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    H, W, M, pairs = CASES[case]
    rows, n, inl = [], [], []
    for b, (what, k, share, noise) in enumerate(pairs):
        if what == "collinear":
            rows.append(C.collinear(k, M)); inl.append(None)
        elif what == "identical":
            rows.append(C.identical(k, M)); inl.append(None)
        else:
            r, i, _ = C.planted(what, max(k, 4), share, noise, H, W, seed=500 + 10 * len(case) + b, M=M)
            r[k:] = np.nan                                                         # (n = 0 and 3: planted as 4, cut here)
            rows.append(r); inl.append(i if k >= 5 and share <= 0.5 else None)
        n.append(k)
    rows, n = np.stack(rows), np.array(n, np.int32)
    assert np.isnan(rows[np.arange(M)[None, :] >= n[:, None]]).all() and np.isfinite(rows[np.arange(M)[None, :] < n[:, None]]).all()
    rows.setflags(write=False)
    return H, W, rows, n, inl


@functools.lru_cache(maxsize=None)
def model(case, hypotheses=256, seed=0):
    H, W, rows, n, _ = inputs(case)
    return HM.fit_batch(rows, n, H, W, hypotheses=hypotheses, seed=seed)


def device_fit(cuda, case, hypotheses=256, seed=0):
    import torch
    from stabnet_amd import metrics
    H, W, rows, n, _ = inputs(case)
    out = metrics.homfit(torch.from_numpy(rows.copy()).to(cuda), torch.from_numpy(n).to(cuda), H, W,
                         metrics.HomfitParams(hypotheses=hypotheses, seed=seed))
    assert [t.dtype for t in out] == [torch.float32, torch.uint8, torch.int32, torch.int32, torch.int32]
    return [t.cpu().numpy() for t in out]


def same(got, want):
    for name, g, w in zip(("Hm", "mask", "count", "status", "best"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == F else (g, w)
        bad = gv != wv
        assert not bad.any(), "%s: %d of %d values differ, first at %s: got %r, want %r" % (
            name, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), g[bad][0], w[bad][0])


@pytest.mark.parametrize("case", list(CASES))
def test_bit_for_bit(cuda, case):
    H, W, rows, n, inl = inputs(case)
    got, want = device_fit(cuda, case), model(case)
    same(got, want)
    Hm, mask, count, status, best = got
    for b, k in enumerate(n):                                                    # conditions on the inputs, checked on the model's side too
        assert not mask[b, k:].any()
        if inl[b] is not None:
            assert status[b] == 1 and np.array_equal(mask[b, :k].astype(bool), inl[b]), (case, b)
        elif k < 4 or CASES[case][3][b][0] in ("collinear", "identical"):
            assert status[b] == 0 and best[b] == -1 and count[b] == 0 and not Hm[b].any() and not mask[b].any()
        elif CASES[case][3][b][2] <= 0.5:
            assert status[b] in (1, 2) and count[b] >= 4


@pytest.mark.parametrize("hypotheses", [64, 512, 300])
def test_hypothesis_counts(cuda, hypotheses):
    """Fewer hypotheses than threads, two per thread, and a count that is no multiple of the threads."""
    same(device_fit(cuda, "half_outliers_M577", hypotheses), model("half_outliers_M577", hypotheses))
    same(device_fit(cuda, "n_around_256_M1024", hypotheses), model("n_around_256_M1024", hypotheses))
    same(device_fit(cuda, "mostly_outliers_M256", hypotheses), model("mostly_outliers_M256", hypotheses))
    if hypotheses == 512:
        assert model("mostly_outliers_M256", 512)[4].max() >= 256                  # a winner that was some thread's second hypothesis


def test_seeds(cuda):
    a, b = device_fit(cuda, "half_outliers_M577", seed=0), device_fit(cuda, "half_outliers_M577", seed=12345)
    same(b, model("half_outliers_M577", seed=12345))
    assert not np.array_equal(a[4], b[4]) and np.array_equal(a[1][:3], b[1][:3])   # other winners, the same masks (pairs of 5 rows or more)


def test_graph_capture(cuda):
    """Captured on one stream and replayed twice: the eager call's bits, and the model's."""
    import torch
    from stabnet_amd import metrics
    H, W, rows, n, _ = inputs("three_pairs_M577")
    r, k = torch.from_numpy(rows.copy()).to(cuda), torch.from_numpy(n).to(cuda)
    eager = [t.clone() for t in metrics.homfit(r, k, H, W)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.homfit(r, k, H, W)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    same([t.cpu().numpy() for t in out], model("three_pairs_M577"))
    assert torch.equal(r.isnan(), torch.from_numpy(np.isnan(rows)).to(cuda))      # the rows are only read


def test_python_argument_checks(cuda):
    import torch
    from stabnet_amd import metrics
    from stabnet_amd._lib import StabnetError
    r, k = torch.zeros((2, 8, 4), device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)
    for bad, word in ((r.cpu(), "GPU"), (r.double(), "float32"), (r[0], r"\[B,M,4\]"), (r[:, :, :3], r"\[B,M,4\]"), (r[:, :3], "M must be")):
        with pytest.raises(StabnetError, match=word):
            metrics.homfit(bad.contiguous() if bad.is_cuda else bad, k, 72, 96)
    for bad in (k.long(), k[:1], k.cpu()):
        with pytest.raises(StabnetError, match="n must be"):
            metrics.homfit(r, bad, 72, 96)
    with pytest.raises(StabnetError, match="thr_px"):
        metrics.homfit(r, k, 72, 96, metrics.HomfitParams(thr_px=0.0))
    out = metrics.homfit(r, k, 72, 96)                                           # n = 0 everywhere: no model, zeros
    assert not any(t.any() for t in out[:4]) and (out[4] == -1).all()
