"""CPU: tests/mosaic_model.py, the yardstick of csrc/mosaic.hip, against planted truth (facts, not the model itself); the guard against
a brute-force mask; the argument checks of the two C entry points (which need no GPU); and the reason the guard exists.

The guard experiment (mosaic_cases.border_clip: 144 x 256, 10 frames, a smooth integer pan, a black border of 19 px whose four
widths jitter by up to +-18 px) through klt_model -> guard model -> homfit_model (min_inliers 16, the full-frame default), MEASURED:
the worst image-corner transfer error against the planted translation over the 9 pairs is 8.91 px unguarded (5 pairs above 1.8 px),
1.34 px at guard 4 (3 pairs above 0.5 px), and 3.04e-5 px at guard 8 -- float32 noise of an exact result.  The bound is max(4 x that, 0.05 px) = 0.05 px."""
import functools

import numpy as np
import pytest

import homfit_model as HM
import klt_model as K
import mosaic_cases as C
import mosaic_model as MM

F = np.float32
GUARD_BOUND_PX = 0.05            # measured 3.04e-5 px at guard 8: see above
H, W, SH, SW = 36, 52, 36, 52    # the compose facts run at the network's size: canvas pixel = network pixel


# ---- the compose model against planted truth ---------------------------------------------------------------------------------------

def random_canvas(seed, SH, SW, age=0):
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (SH, SW, 3)).astype(np.uint8), np.full((SH, SW), age, np.uint8)


def test_everything_covered_deeper_than_the_band_is_the_warped_frame():
    r = np.random.default_rng(0)
    warped = r.integers(0, 256, (SH, SW, 3)).astype(np.uint8)
    # every pixel samples the frame's middle: d >= F = 32 (feather_log2 0) everywhere
    px, py = np.full((SH, SW), SW / 2, F), np.full((SH, SW), SH / 2, F)
    canvas, age = random_canvas(1, SH, SW)
    out, oage, counts = MM.compose(warped, px, py, canvas, age, C.normalised_shift(0, 0, SH, SW), 1, H, W, feather_log2=0)
    assert np.array_equal(out, warped) and not oage.any() and tuple(counts) == (SH * SW, 0, 0, 0)


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-5, 4)])
def test_integer_shift_reproduces_the_previous_canvas_in_uncovered_pixels(shift):
    dx, dy = shift
    warped = np.zeros((SH, SW, 3), np.uint8)
    px, py = np.full((SH, SW), -100.0, F), np.full((SH, SW), -100.0, F)         # nothing covered
    canvas, age = random_canvas(2, SH, SW, age=3)
    out, oage, counts, cls = MM.compose(warped, px, py, canvas, age, C.normalised_shift(dx, dy, SH, SW), 1, H, W, classes=True)
    I, J = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
    inside = (J + dx >= 0) & (J + dx < SW) & (I + dy >= 0) & (I + dy < SH)
    assert np.array_equal(cls == MM.HISTORY, inside) and np.array_equal(cls == MM.NONE, ~inside)
    assert np.array_equal(out[inside], canvas[(I + dy)[inside], (J + dx)[inside]])
    assert (oage[inside] == 4).all() and (oage[~inside] == 255).all() and not out[~inside].any()
    assert tuple(counts) == (0, 0, int(inside.sum()), int((~inside).sum()))


def test_half_pixel_shift_averages_two_neighbours():
    canvas, age = random_canvas(3, SH, SW)
    out, _, _ = MM.compose(np.zeros((SH, SW, 3), np.uint8), np.full((SH, SW), np.nan, F), np.zeros((SH, SW), F), canvas, age,
                           C.normalised_shift(0.5, 0, SH, SW), 2, H, W)
    want = (canvas[:, :-1].astype(int) * 512 + canvas[:, 1:].astype(int) * 512 + 512) >> 10
    assert np.array_equal(out[:, :-1], want) and not out[:, -1].any()           # the last column's right tap has weight and lies outside


@pytest.mark.parametrize("fl", [0, 3, 6])
def test_blend_weights_are_monotone_in_depth_and_hit_both_ends(fl):
    Fq = 32 << fl
    SWb = 2 * (Fq >> 5) + 8
    warped = np.full((129, SWb, 3), 200, np.uint8)
    canvas, age = np.full((129, SWb, 3), 40, np.uint8), np.full((129, SWb), 7, np.uint8)
    # pixel j samples x = j - 2: 32 (j - 2) from the left edge in 1/32 px, 32 (SWb + 1 - j) from the right one; y = 64 lies deeper
    # than any band from either edge of the 129 rows
    px = np.tile((np.arange(SWb, dtype=F) - F(2))[None], (129, 1))
    py = np.full((129, SWb), 64.0, F)
    out, oage, counts, cls = MM.compose(warped, px, py, canvas, age, C.normalised_shift(0, 0, 129, SWb), 1, 129, SWb, feather_log2=fl, classes=True)
    row, arow, crow = out[64, :, 0].astype(int), oage[64], cls[64]
    j = np.arange(SWb)
    d = np.minimum(32 * (j - 2), 32 * (SWb + 1 - j))
    assert (crow[d < 0] == MM.HISTORY).all() and (row[d < 0] == 40).all() and (arow[d < 0] == 8).all()
    band = (d >= 0) & (d < Fq)
    assert (crow[band] == MM.BLENDED).all() and (crow[d >= Fq] == MM.FRESH).all()
    assert row[d == 0][0] == 40 and (row[d >= Fq] == 200).all()                # both ends: pure history at the edge, pure frame past the band
    assert (np.diff(row[2:2 + (Fq >> 5) + 1]) >= 0).all() and row[2 + (Fq >> 5)] == 200      # monotone in between, from the left edge
    want = (200 * d[band] + 40 * (Fq - d[band]) + Fq // 2) >> (5 + fl)
    assert np.array_equal(row[band], want)
    assert np.array_equal(arow[band], np.where(2 * d[band] >= Fq, 0, 8))
    assert counts.sum() == 129 * SWb


def test_history_ages_and_expires():
    canvas, age = random_canvas(4, SH, SW, age=0)
    nothing = (np.zeros((SH, SW, 3), np.uint8), np.full((SH, SW), np.nan, F), np.full((SH, SW), np.nan, F))
    ident = C.normalised_shift(0, 0, SH, SW)
    for step in range(1, 5):
        out, age, counts = MM.compose(*nothing, canvas, age, ident, 1, H, W, max_age=3)
        if step <= 3:
            assert np.array_equal(out, canvas) and (age == step).all() and counts[MM.HISTORY] == SH * SW
        else:
            assert not out.any() and (age == 255).all() and counts[MM.NONE] == SH * SW      # 1 + 3 > max_age
        canvas = out
    # the oldest tap with weight decides; one empty tap with weight makes the sample unavailable; a tap without weight does neither
    canvas, age = random_canvas(5, SH, SW, age=1)
    age[10, 20], age[12, 20] = 9, 255
    half = C.normalised_shift(0.5, 0, SH, SW)
    _, oage, _ = MM.compose(*nothing, canvas, age, half, 1, H, W)
    assert oage[10, 19] == 10 and oage[10, 20] == 10 and oage[10, 21] == 2
    assert oage[12, 19] == 255 and oage[12, 20] == 255 and oage[12, 21] == 2
    _, oage, _ = MM.compose(*nothing, canvas, age, ident, 1, H, W)
    assert oage[12, 19] == 2 and oage[12, 20] == 255 and oage[10, 20] == 10 and oage[10, 19] == 2


@pytest.mark.parametrize("status", [0, 3, -1])
def test_no_model_no_history(status):
    d = C.compose_case(1, SH, SW, 6)
    out, oage, counts, cls = MM.compose(d["warped"][0], d["px"][0], d["py"][0], d["canvas_prev"][0], d["age_prev"][0],
                                        C.normalised_shift(0, 0, SH, SW), status, H, W, classes=True)
    covered = ~MM_black(d["px"][0], d["py"][0])
    assert counts[MM.BLENDED] == 0 and counts[MM.HISTORY] == 0 and counts.sum() == SH * SW
    assert np.array_equal(out[covered], d["warped"][0][covered]) and not out[~covered].any()
    assert (oage[covered] == 0).all() and (oage[~covered] == 255).all()


def MM_black(px, py):
    """remap_src_model.black, the remap's own coverage rule, written from its comment: the rounded coordinate lies outside."""
    import remap_src_model as RM
    return RM.black(px, py, *px.shape)


@pytest.mark.parametrize("name", ["identity", "integer", "subpixel", "perspective", "w_crosses"])
def test_counts_sum_and_coverage_is_the_remaps(name):
    d = C.compose_case(2, 37, 45, 7)
    Hm = C.homographies(37, 45)[name]
    for n in range(2):
        out, oage, counts, cls = MM.compose(d["warped"][n], d["px"][n], d["py"][n], d["canvas_prev"][n], d["age_prev"][n], Hm, 1, 20, 30,
                                            classes=True)
        black = MM_black(d["px"][n], d["py"][n])
        assert counts.sum() == 37 * 45 and np.array_equal(np.isin(cls, (MM.HISTORY, MM.NONE)), black)
        assert (oage[cls == MM.NONE] == 255).all() and (oage[cls != MM.NONE] < 255).all()
        assert counts[MM.NONE] > 0 and (name == "w_crosses" or counts[MM.HISTORY] > 0)


def test_w_below_w_min_has_no_history():
    canvas, age = random_canvas(8, SH, SW)
    nothing = (np.zeros((SH, SW, 3), np.uint8), np.full((SH, SW), np.nan, F), np.full((SH, SW), np.nan, F))
    Hm = C.homographies(SH, SW)["w_crosses"]
    _, oage, _ = MM.compose(*nothing, canvas, age, Hm, 1, H, W)
    G = MM.pixel_homography(Hm, SH, SW, H, W)
    I, J = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
    w = G[6] * J + G[7] * I + G[8]
    assert (w <= 1e-6).any() and (w > 1e-6).any() and (oage[w <= 1e-6] == 255).all()


def test_pixel_homography_is_the_half_pixel_convention():
    """Canvas 128 x 192 beside a network of 64 x 96: a shift by one NETWORK pixel moves the canvas sample by two canvas pixels, and
    the identity keeps every canvas pixel in place (the constants c of csrc/remap.hip cancel)."""
    G = MM.pixel_homography(C.normalised_shift(0, 0, 64, 96), 128, 192, 64, 96)
    assert np.allclose(G / G[8], [1, 0, 0, 0, 1, 0, 0, 0, 1], atol=1e-12)
    G = MM.pixel_homography(np.array([1, 0, 2.0 / 96, 0, 1, -4.0 / 64, 0, 0, 1], F), 128, 192, 64, 96)
    assert np.allclose(G / G[8], [1, 0, 2, 0, 1, -4, 0, 0, 1], atol=1e-5)


# ---- the guard -----------------------------------------------------------------------------------------------------------------------

def brute_safe(xn, yn, black, g):
    Hh, Ww = black.shape
    if not (np.isfinite(xn) and np.isfinite(yn)):
        return False
    x, y = int(np.rint(F(F(xn + F(1)) * F(Ww)) * F(0.5))), int(np.rint(F(F(yn + F(1)) * F(Hh)) * F(0.5)))
    if x - g < 0 or x + g > Ww - 1 or y - g < 0 or y + g > Hh - 1:
        return False
    return bool((black[y - g:y + g + 1, x - g:x + g + 1] < 0.5).all())


def guard_rows(seed, M, Hh, Ww):
    """Rows whose ends lie anywhere in the image, on its very edge, on the border of the black region, outside; NaN rows."""
    r = np.random.default_rng(seed)
    px = r.integers(0, Ww, (M, 2)).astype(np.float64)
    py = r.integers(0, Hh, (M, 2)).astype(np.float64)
    px[::7, 0], py[1::7, 1] = 0, Hh - 1                                        # ends on the image edge
    px[2::11, 1] = Ww - 1
    px[3::13, 0] = Ww + 3                                                       # outside
    rows = np.stack([2 * px[:, 0] / Ww - 1, 2 * py[:, 0] / Hh - 1, 2 * px[:, 1] / Ww - 1, 2 * py[:, 1] / Hh - 1], axis=1).astype(F)
    rows[5::17, r.integers(0, 4)] = np.nan
    return rows


def guard_blacks(seed, Hh, Ww):
    r = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        b = np.ones((Hh, Ww), F)
        l, rr, t, bt = r.integers(2, 12, 4)
        b[t:Hh - bt, l:Ww - rr] = r.random((Hh - t - bt, Ww - l - rr)).astype(F) * F(0.49)
        b[Hh // 2, Ww // 3] = 0.5                                                # one uncovered pixel inside, exactly on the threshold
        out.append(b)
    return out


@pytest.mark.parametrize("g", [0, 8, 16])
def test_guard_against_a_brute_force_mask(g):
    Hh, Ww, M = 72, 96, 300
    rows = guard_rows(3, M, Hh, Ww)
    b0, b1 = guard_blacks(4, Hh, Ww)
    for n in (0, 1, 255, M):
        out, k = MM.guard_matches(rows, n, b0, b1, g)
        keep = [i for i in range(n) if brute_safe(rows[i, 0], rows[i, 1], b0, g) and brute_safe(rows[i, 2], rows[i, 3], b1, g)]
        assert k == len(keep) and np.array_equal(out[:k].view(np.uint32), rows[keep].view(np.uint32)) and not out[k:].any(), (g, n)
    assert 0 < MM.guard_matches(rows, M, b0, b1, g)[1] < M - 40
    assert not np.isnan(MM.guard_matches(rows, M, b0, b1, g)[0]).any()           # no NaN row is ever kept


def test_guard_zero_keeps_an_end_on_the_image_edge():
    b = np.zeros((20, 30), F)
    rows = np.array([[-1, -1, 2 * 29 / 30 - 1, 2 * 19 / 20 - 1]], F)             # pixel (0, 0) and pixel (29, 19)
    assert MM.guard_matches(rows, 1, b, b, 0)[1] == 1 and MM.guard_matches(rows, 1, b, b, 1)[1] == 0


# ---- why the guard exists ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def border_matches():
    frames, black, pan = C.border_clip()
    ny, nx = K.cells(C.GH, C.GW)
    return [K.matches(frames[t], frames[t - 1], ny * nx + 1) for t in range(1, C.GT)]


def chain_errors(guard):
    frames, black, pan = C.border_clip()
    errs = []
    for t, (rows, n) in zip(range(1, C.GT), border_matches()):
        if guard is not None:
            rows, n = MM.guard_matches(rows, n, black[t], black[t - 1], guard)
        Hm, _, count, status, _ = HM.fit(rows, n, C.GH, C.GW, min_inliers=16)
        assert status != 0, (guard, t, n)                                       # every pair has a model, guarded or not
        errs.append(C.corner_error_px(Hm, C.planted_homography(pan, t), C.GH, C.GW))
    return errs


def test_the_guard_recovers_the_planted_motion_and_the_plain_chain_does_not():
    plain, g4, g8 = chain_errors(None), chain_errors(4), chain_errors(8)
    print("corner transfer error, px: unguarded %s\n guard 4 %s\n guard 8 %s" % (plain, g4, g8))
    print("worst: unguarded %.4g, guard 4 %.4g, guard 8 %.4g" % (max(plain), max(g4), max(g8)))
    assert max(g8) <= GUARD_BOUND_PX, g8
    assert max(plain) > GUARD_BOUND_PX and sum(e > GUARD_BOUND_PX for e in plain) >= 1, plain


# ---- the C entry points' refusals (no GPU: the pointers are never followed) ----------------------------------------------------------

def test_guard_bad_arguments_through_the_c_abi():
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096
    ok = dict(B=1, M=577, H=288, W=512, guard=8)

    def call(ptrs=(p, p, p, p, p + 65536, p), **kw):
        a = dict(ok, **kw)
        return L.stabnet_mosaic_guard_matches(ptrs[0], ptrs[1], ptrs[2], ptrs[3], a["B"], a["M"], a["H"], a["W"], a["guard"], ptrs[4], ptrs[5], None)

    for kw, word in ((dict(B=0), b"B must be 1..65535"), (dict(B=65536), b"B must be 1..65535"), (dict(M=3), b"M must be 4..1024"),
                     (dict(M=1025), b"M must be 4..1024"), (dict(guard=-1), b"guard must be 0..16"), (dict(guard=17), b"guard must be 0..16"),
                     (dict(H=0), b"H and W"), (dict(W=0), b"H and W"), (dict(H=(1 << 20) + 1), b"H and W"), (dict(W=(1 << 20) + 1), b"H and W")):
        assert call(**kw) == -1, kw
        assert word in L.stabnet_last_error(), (kw, L.stabnet_last_error())
    for i in range(6):
        ptrs = [p, p, p, p, p + 65536, p]
        ptrs[i] = None
        assert call(tuple(ptrs)) == -1 and b"null pointer" in L.stabnet_last_error(), i
    assert call((p, p, p, p, p, p)) == -1 and b"must not be matches" in L.stabnet_last_error()
    assert call((p + 4, p, p, p, p + 65536, p)) == -1 and b"16-byte aligned" in L.stabnet_last_error()


def test_compose_bad_arguments_through_the_c_abi():
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096
    good = [p + 65536 * i for i in range(10)]                 # warped px py canvas_prev age_prev Hm status canvas_cur age_cur counts
    ok = dict(N=1, SH=720, SW=1280, H=288, W=512, fl=3, age=64, wmin=1e-6)

    def call(ptrs=good, **kw):
        a = dict(ok, **kw)
        return L.stabnet_mosaic_compose(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], a["N"], a["SH"], a["SW"], a["H"], a["W"],
                                        a["fl"], a["age"], a["wmin"], ptrs[7], ptrs[8], ptrs[9], None)

    for kw, word in ((dict(N=0), b"batch"), (dict(N=65536), b"batch"), (dict(SH=0), b"1..32767"), (dict(SW=32768), b"1..32767"),
                     (dict(H=0), b"H and W"), (dict(W=(1 << 20) + 1), b"H and W"), (dict(fl=-1), b"feather_log2"), (dict(fl=7), b"feather_log2"),
                     (dict(age=0), b"max_age"), (dict(age=255), b"max_age"), (dict(wmin=-1.0), b"w_min"), (dict(wmin=float("inf")), b"w_min"),
                     (dict(wmin=float("nan")), b"w_min")):
        assert call(**kw) == -1, kw
        assert word in L.stabnet_last_error(), (kw, L.stabnet_last_error())
    for i in range(10):
        ptrs = list(good)
        ptrs[i] = None
        assert call(ptrs) == -1 and b"null pointer" in L.stabnet_last_error(), i
    same = list(good)
    same[7] = same[3]
    assert call(same) == -1 and b"must not be the previous" in L.stabnet_last_error()
    same = list(good)
    same[8] = same[4]
    assert call(same) == -1 and b"must not be the previous" in L.stabnet_last_error()
