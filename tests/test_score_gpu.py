"""GPU: stabnet_amd/metrics.py end to end.  score_clip on a 16-frame 72 x 96 clip against the CPU models chained (klt_model.matches ->
homfit_model.fit -> homfit_model.metrics): every homography bit for bit, the three numbers to 1e-9 (host float64 on equal inputs:
sums of at most 16 terms of O(1)).  The clips are tests/score_cases.py's: a smooth path, the same path with a jitter of up to 3 px,
and the jittered clip magnified 1.25 times.

The zoom's margin, MEASURED with the CPU models on these clips: the mean cropping of the 16 pairs is 0.7833 where a perfect fit
would give 0.8 (translation-only windows track a magnified texture with a bias), 0.0167 off; the bound is twice that, 0.034.

deploy_bundle.py --score runs as a fresh child process: it writes <name>_score.json, and every other output is byte for byte what
a run without the flag writes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOOM_MARGIN = 0.034          # measured 0.0167 with the CPU models: see above


@functools.lru_cache(maxsize=None)
def model():
    return S.model_score(S.unstable(), S.stable())


def dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)


def test_score_against_the_models(cuda):
    from stabnet_amd import metrics
    want, H_us, st_us, H_ss, st_ss = model()
    assert (st_us != 0).all() and (st_ss != 0).all()                             # a condition on the inputs: no pair without a model
    got = metrics.score_clip(dev(cuda, S.unstable()), dev(cuda, S.stable()), per_frame=True, homographies=True)
    assert got["failed_pairs_unstable_stable"] == 0 and got["failed_pairs_stable_stable"] == 0 and got["frames"] == S.T
    for name, g, w in (("H_us", got["H_us"], H_us), ("H_ss", got["H_ss"], H_ss)):
        g = np.array(g, np.float32)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, np.abs(g - w).max())
    assert got["status_us"] == st_us.tolist() and got["status_ss"] == st_ss.tolist()
    for k in ("cropping", "distortion", "stability", "stability_translation", "stability_rotation"):
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
        assert 0.0 < got[k] <= 1.0
    assert np.allclose(got["cropping_per_frame"], want["cropping_per_frame"], rtol=0, atol=1e-9)
    assert got["mean_inliers"] >= 4 and got["size"] == [S.H, S.W] and got["params"]["fit"]["hypotheses"] == 256


def test_the_unstable_clip_is_less_stable_than_its_stabilisation(cuda):
    from stabnet_amd import metrics
    u, s = dev(cuda, S.unstable()), dev(cuda, S.stable())
    good, bad = metrics.score_clip(u, s), metrics.score_clip(u, u)
    print(good["stability"], bad["stability"])
    assert bad["stability"] < good["stability"]
    assert abs(bad["cropping"] - 1.0) <= 1e-6 and abs(bad["distortion"] - 1.0) <= 1e-6      # a clip against itself: the identity, up to float32


def test_uint8_and_bgr_inputs(cuda):
    """uint8 grey is its values; BGR is (0.114*B + 0.587*G) + 0.299*R in float32, the model's grey()."""
    import torch
    import homfit_model as HM
    from stabnet_amd import metrics
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (3, 20, 24, 3), dtype=np.uint8)
    got = metrics.grey(dev(cuda, bgr)).cpu().numpy()
    assert np.abs(got - HM.grey(bgr)).max() <= 255 * 2.0 ** -22                   # (torch may fuse a multiply-add: a few ulp of 255)
    assert np.array_equal(metrics.grey(dev(cuda, bgr[..., 0])).cpu().numpy(), bgr[..., 0].astype(np.float32))
    u8 = lambda a: dev(cuda, np.clip(np.rint(a), 0, 255).astype(np.uint8))
    a = metrics.score_clip(u8(S.unstable()), u8(S.stable()))
    b = metrics.score_clip(u8(S.unstable()).float(), u8(S.stable()).float())
    assert a["cropping"] == b["cropping"] and a["stability"] == b["stability"] and a["distortion"] == b["distortion"]
    from stabnet_amd._lib import StabnetError
    with pytest.raises(StabnetError, match="too short"):
        metrics.score_clip(u8(S.unstable())[:13], u8(S.stable())[:13])
    with pytest.raises(StabnetError, match="agree"):
        metrics.score_clip(u8(S.unstable()), u8(S.stable())[:15])
    with pytest.raises(StabnetError, match="rows per pair"):
        metrics.pair_homographies(torch.zeros((1, 720, 1280), device=cuda), torch.zeros((1, 720, 1280), device=cuda))


def test_pair_homographies_in_chunks_and_on_views(cuda):
    """S[:-1] and S[1:] of one tensor, 15 pairs in chunks of 4 (the last one short): the pair's index in the sampling chain is its
    index in the chunk, so the model is given that index."""
    import homfit_model as HM
    import klt_model as K
    from stabnet_amd import metrics
    s = dev(cuda, S.stable())
    Hm, status = metrics.pair_homographies(s[:-1], s[1:], chunk=4)
    assert Hm.shape == (S.T - 1, 9) and status.shape == (S.T - 1,)
    Hm = Hm.cpu().numpy()
    ny, nx = K.cells(S.H, S.W)
    for t in (0, 5, 14):
        rows, n = K.matches(S.stable()[t], S.stable()[t + 1], ny * nx + 1)
        want = HM.fit(rows, n, S.H, S.W, b=t % 4)[0]
        assert np.array_equal(Hm[t].view(np.uint32), want.view(np.uint32)), t


def test_zoom_gives_its_cropping(cuda):
    from stabnet_amd import metrics
    got = metrics.score_clip(dev(cuda, S.unstable()), dev(cuda, S.zoomed(1.25)))
    print("cropping", got["cropping"])
    assert got["failed_pairs_unstable_stable"] == 0
    assert abs(got["cropping"] - 0.8) <= ZOOM_MARGIN, got["cropping"]


def _deploy(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--synthetic", "20", "--height", "64", "--width", "96",
           "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Traceback" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_deploy_bundle_score(cuda, tmp_path):
    out = _deploy(tmp_path / "scored", "--score")
    plain = _deploy(tmp_path / "plain")
    assert "cropping / distortion / stability" in out and "cropping / distortion / stability" not in plain
    f = lambda d, name: str(tmp_path / d / "output" / name)
    res = json.load(open(f("scored", "synthetic_score.json")))
    assert res["frames"] == 19 and res["size"] == [64, 96]
    for k in ("cropping", "distortion", "stability"):
        assert 0.0 < res[k] <= 1.0, (k, res[k])
    names = sorted(os.listdir(tmp_path / "plain" / "output"))
    assert sorted(os.listdir(tmp_path / "scored" / "output")) == sorted(names + ["synthetic_score.json"])
    for name in names:
        assert open(f("scored", name), "rb").read() == open(f("plain", name), "rb").read(), name
