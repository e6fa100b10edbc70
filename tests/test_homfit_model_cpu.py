"""CPU: tests/homfit_model.py, the yardstick of csrc/homfit.hip, against planted truth; the argument checks of the C entry point
(which need no GPU); the three metrics on hand-made homography sequences; and the host part of stabnet_amd/metrics.py against the
model's metrics.

Tolerances of the planted cases, MEASURED with the model over all 72 cases below (3 models x n of 4, 5, 60, 577 x 0 / 30 / 50 %
outliers x noise of 0 and 0.1 px, 288 x 512): the largest distance between the fitted and the true image of an inlier's source
point is 2.14e-5 px without noise (float32 coordinates: one ulp of a coordinate near 1 is 1.5e-5 px of 256) and 0.1221 px with
0.1 px of noise per axis.  The bounds are four times that: 1e-4 px and 0.5 px."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import homfit_cases as C
import homfit_model as HM

H, W = 288, 512
TOL_PX = {0.0: 1e-4, 0.1: 0.5}          # measured 2.14e-5 and 0.1221: see above
PLANTED = list(itertools.product(C.MODELS, (4, 5, 60, 577), (0.0, 0.3, 0.5), (0.0, 0.1)))


@functools.lru_cache(maxsize=None)
def planted_fit(i):
    model, n, share, noise = PLANTED[i]
    rows, inl, truth = C.planted(model, n, share, noise, H, W, seed=1000 + i)
    return rows, inl, truth, HM.fit(rows, n, H, W)


@pytest.mark.parametrize("i", range(len(PLANTED)), ids=["%s-n%d-out%d-noise%g" % (m, n, 100 * s, z) for m, n, s, z in PLANTED])
def test_planted_inliers(i):
    model, n, share, noise = PLANTED[i]
    rows, inl, truth, (Hm, mask, count, status, best) = planted_fit(i)
    assert (~inl).sum() == C.outlier_count(n, share)
    assert status == 1 and 0 <= best < 256, (status, best)                     # 256 hypotheses are a cap: none of these cases may use it up
    assert np.array_equal(mask[:n].astype(bool), inl) and count == inl.sum()
    assert Hm[8] == 1 and np.isfinite(Hm).all()
    err = C.transfer_error_px(Hm, truth, rows[:n][inl], H, W)
    print("transfer error %.3e px" % err)
    assert err <= TOL_PX[noise], err


def test_half_of_the_rows_are_outliers_somewhere():
    assert max((~planted_fit(i)[1]).sum() for i in range(len(PLANTED))) == 288


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_fewer_than_four_rows(n):
    rows, _, _ = C.planted("similarity", 8, 0.0, 0.0, H, W, seed=3)
    Hm, mask, count, status, best = HM.fit(rows, n, H, W)
    assert (status, count, best) == (0, 0, -1) and not Hm.any() and not mask.any()


@pytest.mark.parametrize("rows", [C.identical(30), C.collinear(40)], ids=["identical", "collinear"])
def test_degenerate_rows_give_no_model(rows):
    Hm, mask, count, status, best = HM.fit(rows, len(rows), H, W)
    assert (status, count, best) == (0, 0, -1) and not Hm.any() and not mask.any()
    idx, ok = HM.sample(0, 0, 256, len(rows))
    assert ok.all() and not HM.four_point(rows[idx])[1].any()                   # every sample was drawn; every model divides 0 by 0


def test_duplicated_rows_give_a_finite_result():
    rows, inl, truth = C.planted("similarity", 30, 0.0, 0.1, H, W, seed=5)
    dup = np.concatenate([rows, rows])
    Hm, mask, count, status, best = HM.fit(dup, 60, H, W)
    assert status in (1, 2) and np.isfinite(Hm).all() and count == 60
    assert C.transfer_error_px(Hm, truth, rows, H, W) <= TOL_PX[0.1]


def test_determinism_and_seeds():
    rows, inl, _ = C.planted("similarity", 60, 0.3, 0.1, H, W, seed=5)
    a, b, c = HM.fit(rows, 60, H, W, seed=0), HM.fit(rows, 60, H, W, seed=0), HM.fit(rows, 60, H, W, seed=1)
    assert a[4] == b[4] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert c[4] != a[4]                                                         # another seed: another winner ...
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[1][:60].astype(bool), inl)      # ... and the same mask
    # the pair index is part of the chain: the same rows as pair 1 draw other samples
    assert not np.array_equal(HM.sample(0, 0, 256, 60)[0], HM.sample(0, 1, 256, 60)[0])


def test_sampling_is_distinct_and_in_range():
    for n in (4, 5, 60, 577, 1024):
        idx, ok = HM.sample(7, 3, 512, n)
        assert ((idx[ok] >= 0) & (idx[ok] < n)).all()
        assert all(len(set(r)) == 4 for r in idx[ok])
        assert ok.mean() > 0.8, (n, ok.mean())                                  # (n = 4: 16 draws miss one of the four now and then)
    assert HM.mix(0) == 0 and HM.mix(1) == 0x688990c0                           # the mix itself (0 is its fixed point: the chain adds a constant)


def test_bad_arguments_through_the_c_abi():
    """-1 and a message before anything touches the GPU: the pointers are never followed."""
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096                                                                    # not null, 16-byte aligned, never read
    ok = dict(B=1, M=577, H=288, W=512, hyp=256, thr=2.0, mi=4, seed=0, wmin=1e-6)

    def call(ptrs=(p,) * 7, **kw):
        a = dict(ok, **kw)
        return L.stabnet_homfit(ptrs[0], ptrs[1], a["B"], a["M"], a["H"], a["W"], a["hyp"], a["thr"], a["mi"], a["seed"], a["wmin"],
                                ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], None, None)

    for kw, word in ((dict(M=3), b"M must be 4..1024"), (dict(M=1025), b"M must be 4..1024"), (dict(B=0), b"B must be 1..65535"),
                     (dict(B=65536), b"B must be 1..65535"), (dict(hyp=0), b"hypotheses"), (dict(thr=0.0), b"thr_px"),
                     (dict(thr=float("nan")), b"thr_px"), (dict(mi=-1), b"min_inliers"), (dict(seed=-1), b"seed"),
                     (dict(wmin=-1.0), b"w_min"), (dict(H=0), b"H and W")):
        assert call(**kw) == -1, kw
        assert word in L.stabnet_last_error(), (kw, L.stabnet_last_error())
    for i in range(7):
        ptrs = [p] * 7
        ptrs[i] = None
        assert call(tuple(ptrs)) == -1 and b"null pointer" in L.stabnet_last_error(), i
    assert call((p + 4,) + (p,) * 6) == -1 and b"16-byte aligned" in L.stabnet_last_error()


# ---- the metrics -----------------------------------------------------------------------------------------------------------------

def about_centre(A, H, W):
    """The pixel-frame homography that applies the 2 x 2 matrix A about the frame's centre."""
    c = np.array([W / 2.0, H / 2.0])
    P = np.eye(3)
    P[:2, :2] = A
    P[:2, 2] = c - A @ c
    return P


def sequence(us_px, ss_px):
    return (np.stack([C.normalised(P, H, W).reshape(9) for P in us_px]), np.ones(len(us_px), np.int32),
            np.stack([C.normalised(P, H, W).reshape(9) for P in ss_px]), np.ones(len(ss_px), np.int32))


def shift(dx, dy=0.0):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)


def both(seq, **kw):
    """The model's metrics and metrics.py's host part on the same homographies: they must agree to 1e-9."""
    from stabnet_amd import metrics
    a, b = HM.metrics(*seq, H, W), metrics.host_metrics(*seq, H, W, per_frame=True)
    for k in ("cropping", "distortion", "stability", "stability_translation", "stability_rotation"):
        assert abs(a[k] - b[k]) <= 1e-9, (k, a[k], b[k])
    assert np.allclose(a["cropping_per_frame"], b["cropping_per_frame"], rtol=0, atol=1e-9)
    assert np.allclose(a["distortion_per_frame"], b["distortion_per_frame"], rtol=0, atol=1e-9)
    return a


T = 63
STILL = [np.eye(3)] * (T - 1)


def test_uniform_zoom_gives_its_cropping():
    m = both(sequence([about_centre(1.25 * np.eye(2), H, W)] * T, STILL))
    assert abs(m["cropping"] - 0.8) <= 1e-9 and abs(m["distortion"] - 1.0) <= 1e-9
    m = both(sequence([about_centre(0.5 * np.eye(2), H, W)] * T, STILL))         # a stable frame that shows more than the unstable one: capped
    assert m["cropping"] == 1.0


def test_anisotropic_scale_gives_its_distortion():
    m = both(sequence([about_centre(np.diag([1.2, 1.0]), H, W)] * T, STILL))
    assert abs(m["distortion"] - 1 / 1.2) <= 1e-9 and abs(m["cropping"] - 1 / 1.2) <= 1e-9
    us = [about_centre(np.diag([1.2, 1.0]), H, W)] + [np.eye(3)] * (T - 1)       # the clip's value is the worst frame's
    assert abs(both(sequence(us, STILL))["distortion"] - 1 / 1.2) <= 1e-9


def test_rotation_has_no_distortion():
    a = np.deg2rad(7.0)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    m = both(sequence([about_centre(R, H, W)] * T, STILL))
    assert abs(m["distortion"] - 1.0) <= 1e-9 and abs(m["cropping"] - 1.0) <= 1e-9


def test_a_smooth_path_is_stable_and_jitter_is_not():
    t = np.arange(T)
    smooth = 10.0 * (1.0 - np.cos(2 * np.pi * t / T))                           # one cycle over the clip, from 0
    jitter = smooth + np.where(t > 0, 1.5 * (-1.0) ** t, 0.0)
    steps = lambda x: [shift(x[i + 1] - x[i]) for i in range(T - 1)]
    a = both(sequence([np.eye(3)] * T, steps(smooth)))
    b = both(sequence([np.eye(3)] * T, steps(jitter)))
    assert a["stability"] > 0.99 and a["stability_rotation"] == 1.0             # (no rotation at all: an empty spectrum counts as 1)
    assert abs(a["stability_translation"] - 1.0) <= 1e-9                        # all of the power sits in the first bin
    assert b["stability"] < a["stability"] - 1e-3, (a["stability"], b["stability"])


def test_failed_pairs_are_left_out_and_short_clips_refused():
    from stabnet_amd import metrics
    from stabnet_amd._lib import StabnetError
    us = [about_centre(1.25 * np.eye(2), H, W)] * T
    H_us, st_us, H_ss, st_ss = sequence(us, [shift(1.0)] * (T - 1))
    H_us[3], st_us[3] = 0, 0                                                    # what the kernel writes for a pair without a model
    H_ss[5], st_ss[5] = 0, 0
    m = both((H_us, st_us, H_ss, st_ss))
    assert abs(m["cropping"] - 0.8) <= 1e-9
    full = metrics.host_metrics(H_us, st_us, H_ss, st_ss, H, W, per_frame=True)
    assert full["failed_pairs_unstable_stable"] == 1 and full["failed_pairs_stable_stable"] == 1 and full["frames"] == T
    assert len(full["cropping_per_frame"]) == T - 1 and abs(full["path_translation"][-1] - (T - 2)) <= 1e-9
    short = sequence([np.eye(3)] * 13, [np.eye(3)] * 12)
    with pytest.raises(ValueError, match="14"):
        HM.metrics(*short, H, W)
    with pytest.raises(StabnetError, match="14"):
        metrics.host_metrics(*short, H, W)
    HM.metrics(*sequence([np.eye(3)] * 14, [np.eye(3)] * 13), H, W)


def test_metrics_py_against_the_model_on_random_homographies():
    rng = np.random.default_rng(11)
    def rand():
        P = np.eye(3) + rng.normal(0, [[0.02, 0.02, 3.0], [0.02, 0.02, 3.0], [2e-5, 2e-5, 0]])
        return P
    T2 = 20
    seq = sequence([rand() for _ in range(T2)], [rand() for _ in range(T2 - 1)])
    seq[1][[2, 7]] = 0
    seq[3][[0, 11]] = 0
    both(seq)
