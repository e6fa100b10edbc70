"""GPU: full-frame output end to end.  mosaic.Mosaic (tracking -> guard -> fit -> compose, all on the device) against the chained
CPU models (klt_model -> mosaic_model.guard_matches -> homfit_model -> mosaic_model.compose), bit for bit, over a 16-frame clip with
planted borders at 64 x 96 network / 128 x 192 canvas, two streams; and deploy_bundle.py --fill history as a child process: the
three new files, every other output byte-identical to a run without the flag."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import homfit_model as HM
import klt_model as K
import mosaic_model as MM
import remap_src_model as RM
import tvl1_model as TM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
T, H, W, SH, SW, N = 16, 64, 96, 128, 192, 2
KNOBS = dict(feather_log2=2, max_age=5, guard=4, hypotheses=128, thr_px=2.0, min_inliers=8, seed=3, w_min=1e-6)
KLT = dict(cell=8, levels=2)


@functools.lru_cache(maxsize=None)
def clip(seed):
    """One stream: grey float32 [T,H,W] in [-0.5, 0.5] (the network's scale; -0.5 in the border), black float32 [T,H,W], and at the
    canvas's size warped uint8 [T,SH,SW,3] with the coordinates px, py float32 [T,SH,SW] of a remap that covers exactly the content:
    a texture under a smooth integer pan, inside a border of 3..9 network pixels that changes every frame."""
    margin = 16
    tex = (TM.texture(H + 2 * margin, W + 2 * margin, seed) * 255.0).astype(F)
    r = np.random.default_rng(seed + 1)
    t = np.arange(T)
    pan = np.stack([np.rint(5.0 * (1.0 - np.cos(np.pi * t / (T - 1)))), np.rint(0.2 * t)], axis=1).astype(int)
    widths = r.integers(3, 10, (T, 4))
    grey, black = np.full((T, H, W), -0.5, F), np.ones((T, H, W), F)
    warped, px, py = np.zeros((T, SH, SW, 3), np.uint8), np.zeros((T, SH, SW), F), np.zeros((T, SH, SW), F)
    J, I = np.arange(SW, dtype=np.float64), np.arange(SH, dtype=np.float64)
    for k in range(T):
        l, rr, tp, bt = widths[k]
        view = tex[margin + pan[k, 1]:margin + pan[k, 1] + H, margin + pan[k, 0]:margin + pan[k, 0] + W]
        grey[k, tp:H - bt, l:W - rr] = view[tp:H - bt, l:W - rr] / F(255) - F(0.5)
        black[k, tp:H - bt, l:W - rr] = 0
        # canvas column 2 l samples source column 0, column SW - 2 rr - 1 samples column SW - 1; likewise the rows
        x = (J - 2 * l) * ((SW - 1) / (SW - 2 * l - 2 * rr - 1))
        y = (I - 2 * tp) * ((SH - 1) / (SH - 2 * tp - 2 * bt - 1))
        px[k], py[k] = np.broadcast_to(x[None, :], (SH, SW)).astype(F), np.broadcast_to(y[:, None], (SH, SW)).astype(F)
        big = np.kron(view, np.ones((2, 2), F))
        warped[k] = np.stack([big * 0.8 + 20, big, big * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)
        warped[k][RM.black(px[k], py[k], SH, SW)] = 0
    if seed % 2:
        px[3, 5, 7], py[9, 100, 33] = np.nan, 1e30                                   # what a broken map entry would give
    return grey, black, warped, px, py


@functools.lru_cache(maxsize=None)
def model_run():
    """The chained CPU models over both streams -> per frame (canvas [N,...], age, counts [N,4], Hm [N,9], status [N], inliers [N])."""
    kw = dict(K.DEFAULTS, **KLT)
    ny, nx = K.cells(H, W, kw["cell"])
    M = ny * nx + 1
    streams = [clip(11 + n) for n in range(N)]
    canvas, age = np.zeros((N, SH, SW, 3), np.uint8), np.full((N, SH, SW), 255, np.uint8)
    out = []
    for t in range(T):
        Hm, status, inl = np.zeros((N, 9), F), np.zeros(N, np.int32), np.zeros(N, np.int32)
        cnt = np.zeros((N, 4), np.int32)
        new_c, new_a = np.empty_like(canvas), np.empty_like(age)
        for n, (grey, black, warped, px, py) in enumerate(streams):
            if t > 0:
                g255 = lambda v: (v + F(0.5)) * F(255)
                rows, k = K.matches(g255(grey[t]), g255(grey[t - 1]), M, **kw)
                rows, k = MM.guard_matches(rows, k, black[t], black[t - 1], KNOBS["guard"])
                Hm[n], _, inl[n], status[n], _ = HM.fit(rows, k, H, W, b=n, hypotheses=KNOBS["hypotheses"], thr_px=KNOBS["thr_px"],
                                                         min_inliers=KNOBS["min_inliers"], seed=KNOBS["seed"], w_min=KNOBS["w_min"])
            new_c[n], new_a[n], cnt[n] = MM.compose(warped[t], px[t], py[t], canvas[n], age[n], Hm[n], status[n], H, W,
                                                     feather_log2=KNOBS["feather_log2"], max_age=KNOBS["max_age"], w_min=KNOBS["w_min"])
        canvas, age = new_c, new_a
        out.append((canvas, age, cnt, Hm, status, inl))
    return out


def test_mosaic_equals_the_chained_models(cuda):
    import torch
    from stabnet_amd import features, mosaic
    params = mosaic.MosaicParams(klt=features.KltParams(**KLT), **KNOBS)
    m = mosaic.Mosaic(N, SH, SW, H, W, params, device=cuda, log_frames=4)          # (the log doubles itself twice)
    streams = [clip(11 + n) for n in range(N)]
    dev = [[torch.from_numpy(np.stack([s[i] for s in streams], axis=1)).to(cuda) for i in range(5)]]      # [T,N,...] each
    grey, black, warped, px, py = dev[0]
    want = model_run()
    for rnd in range(2):                                                           # reset() starts the same clip over
        m.reset()
        for t in range(T):
            canvas = m.update(warped[t].contiguous(), px[t].contiguous(), py[t].contiguous(), grey[t].contiguous(), black[t].contiguous())
            wc, wa, wn, wh, ws, wi = want[t]
            assert np.array_equal(canvas.cpu().numpy(), wc), (rnd, t, "canvas")
            assert np.array_equal(m.ages.cpu().numpy(), wa), (rnd, t, "age")
            assert np.array_equal(m.Hm.cpu().numpy().view(np.uint32), wh.view(np.uint32)), (rnd, t, "Hm")
            assert np.array_equal(m.status.cpu().numpy(), ws) and np.array_equal(m.counts.cpu().numpy(), wn), (rnd, t)
        log = m.log()
        assert log["status"].shape == (T, N)
        assert np.array_equal(log["status"], np.stack([w[4] for w in want])) and np.array_equal(log["inliers"], np.stack([w[5] for w in want]))
        for i, name in enumerate(("fresh", "blended", "history", "empty")):
            assert np.array_equal(log[name], np.stack([w[2][:, i] for w in want])), name
        assert (log["fresh"] + log["blended"] + log["history"] + log["empty"] == SH * SW).all()
    st = np.stack([w[4] for w in want])
    hist = np.stack([w[2][:, 2] for w in want])
    print("status per frame and stream:", st.T.tolist(), "history pixels:", hist.T.tolist())
    assert (st[1:] != 0).mean() > 0.7 and (hist[1:] > 0).mean() > 0.7              # the clip exercises what it is meant to
    assert mosaic.totals(log)["frames_without_model"] == int((st == 0).sum())


def test_mosaic_refusals(cuda):
    import torch
    from stabnet_amd import features, mosaic
    from stabnet_amd._lib import StabnetError
    with pytest.raises(StabnetError, match="feather_log2"):
        mosaic.Mosaic(1, SH, SW, H, W, mosaic.MosaicParams(feather_log2=7), device=cuda)
    with pytest.raises(StabnetError, match="rows per pair"):
        mosaic.Mosaic(1, 720, 1280, 288, 512, mosaic.MosaicParams(klt=features.KltParams(cell=8)), device=cuda)
    m = mosaic.Mosaic(1, SH, SW, H, W, device=cuda)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)
    with pytest.raises(StabnetError, match="grey"):
        m.update(z(1, SH, SW, 3, dt=torch.uint8), z(1, SH, SW), z(1, SH, SW), z(1, H, W, 1), z(1, H, W))
    with pytest.raises(StabnetError, match="warped"):
        m.update(z(1, SH, SW, 3), z(1, SH, SW), z(1, SH, SW), z(1, H, W), z(1, H, W))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------

DH, DW, DSH, DSW, DT = 32, 64, 90, 150, 7


def _clip(sh, sw, n, seed=11):
    """uint8 BGR [n, sh, sw, 3]: the synthetic shaky clip, tinted (tests/test_fill_adaptive_pipeline_gpu.py's)."""
    from stabnet_amd import synthetic
    g8 = ((synthetic.make_clip(sh, sw, n, seed=seed).astype(np.float32) + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def _deploy(out_dir, *extra, ok=True, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(DH), "--width", str(DW), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r


def test_deploy_bundle_fill_history(cuda, tmp_path):
    clip8 = _clip(DSH, DSW, DT, seed=4)
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    np.save(str(prefix / "unstable" / "shaky.npy"), clip8)
    (tmp_path / "list").write_text("shaky.npy\n")
    base = ["--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg", "--ingest", "device", "--output-size", "source"]
    f = lambda d, name: str(tmp_path / d / "output" / name)
    # refused before anything is loaded
    r = _deploy(tmp_path / "no", *base, "--fill", "history", "--pipeline", ok=False)
    assert r.returncode != 0 and "--fill history runs in the serial loop only" in r.stderr
    r = _deploy(tmp_path / "no", *base, "--fill-age", "9", ok=False)
    assert r.returncode != 0 and "belong to --fill history" in r.stderr
    _deploy(tmp_path / "plain", *base)
    out = _deploy(tmp_path / "hist", *base, "--fill", "history", "--fill-age", "5", "--fill-feather", "4", "--score").stdout
    assert "--fill history" in out and "--score scores the online frames" in out
    plain, hist = sorted(os.listdir(tmp_path / "plain" / "output")), sorted(os.listdir(tmp_path / "hist" / "output"))
    assert sorted(set(hist) - set(plain)) == ["shaky_fill.avi", "shaky_fill.npy", "shaky_fill_history.json"], (plain, hist)
    for name in plain:                                                              # everything else: byte for byte
        assert open(f("hist", name), "rb").read() == open(f("plain", name), "rb").read(), name
    filled, colour, maps = np.load(f("hist", "shaky_fill.npy")), np.load(f("hist", "shaky_stable_bgr.npy")), np.load(f("hist", "shaky_maps.npz"))
    info = json.load(open(f("hist", "shaky_fill_history.json")))
    assert filled.shape == colour.shape == (DT - 1, DSH, DSW, 3) and filled.dtype == np.uint8
    assert info["mode"] == "history" and info["output_size"] == [DSH, DSW] and info["network_size"] == [DH, DW] and info["frames"] == DT - 1
    assert info["params"]["max_age"] == 5 and info["params"]["feather_log2"] == 2 and info["params"]["fill_feather"] == 4
    per = info["per_frame"]
    assert all(len(per[k]) == DT - 1 for k in ("fresh", "blended", "history", "empty", "status", "inliers"))
    from stabnet_amd.avi import AviMjpegReader
    rd = AviMjpegReader(f("hist", "shaky_fill.avi"))
    assert len(rd) == DT and (rd.height, rd.width) == (DSH, DSW)                   # the first frame as read, then every filled frame
    for i in range(DT - 1):
        px, py = RM.coords(maps["x_map"][i], maps["y_map"][i], DSH, DSW)
        uncovered = int(RM.black(px, py, DSH, DSW).sum())
        assert per["fresh"][i] + per["blended"][i] + per["history"][i] + per["empty"][i] == DSH * DSW, i
        assert per["empty"][i] <= uncovered and per["history"][i] + per["empty"][i] == uncovered, (i, per["empty"][i], uncovered)
        deep = MM.depth(px, py, DSH, DSW) >= (32 << 2)                            # deeper than the feather band: the frame itself, age 0
        assert np.array_equal(filled[i][deep], colour[i][deep]), i
        if per["status"][i] == 0:                                                   # no model: the frame where it covers, nothing elsewhere
            covered = ~RM.black(px, py, DSH, DSW)
            assert np.array_equal(filled[i][covered], colour[i][covered]) and not filled[i][~covered].any(), i
            assert per["blended"][i] == 0 and per["history"][i] == 0, i
    assert per["status"][0] == 0 and per["history"][0] == 0                        # the first frame has nothing to take from
    assert info["totals"]["empty"] == sum(per["empty"]) and info["totals"]["history"] == sum(per["history"])
