"""CPU: the scene-cut model (tests/scene_model.py) and everything of the feature that needs no GPU: the margins of the clips the GPU tests
use, the rule with its gap, the quantisation, the driver's flags, the scorer's cuts and the C entries' refusals."""
import ctypes
import math

import numpy as np
import pytest

import scene_model as M


def _margins(frames, cuts):
    _, _, d = M.run(frames, 0.35, 0)
    at = [d[c] for c in cuts]
    rest = np.delete(d, cuts)
    return (min(at) if at else None), float(rest.max())


@pytest.mark.parametrize("H,W", [(64, 96), (45, 77), (288, 512)])
def test_margins_of_the_test_clips(H, W):
    """d >= 0.6 at the cut and <= 0.25 elsewhere for exactly the clips the GPU tests use, so that no test balances on the 0.35 default."""
    A, B = M.cut_clip(H, W, 10, 6)                                         # test_scene_stream_gpu.py, test_scene_pipeline_gpu.py
    lo, hi = _margins(np.concatenate([A, B]), [10])
    print("%dx%d A ++ B: d at the cut %.3f, largest d elsewhere %.3f" % (H, W, lo, hi))
    assert lo >= 0.6 and hi <= 0.25
    assert _margins(np.concatenate([B[0:1], B]), [])[1] <= 0.25
    clip = M.multi_stream_clip(3, H, W)                                    # test_scene_gpu.py
    for n in range(3):
        lo, hi = _margins(clip[:, n], [2 + n])
        assert lo >= 0.6 and hi <= 0.25, (n, lo, hi)


def test_margins_of_the_driver_clips_and_the_uncut_stream():
    import deploy_bundle
    from stabnet_amd import synthetic
    H, W = 64, 96
    A, B = M.cut_clip(H, W, 10, 6)
    u8 = M.to_u8(np.concatenate([A, B]))                                   # the .npy / Y4M clip of test_scene_pipeline_gpu.py
    lo, hi = _margins(np.stack([deploy_bundle.grey_train(f, H, W) for f in u8]), [10])
    assert lo >= 0.6 and hi <= 0.25
    assert _margins(synthetic.make_clip(H, W, 16, seed=1, margin=32), [])[1] <= 0.25     # stream 0 of the lock-step test


def test_rule_with_gap():
    """24 frames, cuts planted at 3, 10 and 12: with min_gap 8 only frame 10 is flagged (3 comes too soon after the start, 12 too soon
    after 10); min_gap 0 flags all three."""
    H, W = 16, 24
    rng = np.random.default_rng(0)
    scenes = [np.full((H, W), v, np.float32) + rng.uniform(-0.02, 0.02, (H, W)).astype(np.float32) for v in (-0.4, -0.1, 0.2, 0.45)]
    which = [0] * 3 + [1] * 7 + [2] * 2 + [3] * 12
    frames = np.stack([scenes[k] for k in which])
    f8, D, d = M.run(frames, 0.35, 8)
    assert list(np.nonzero(f8)[0]) == [10]
    assert D[0] == 0 and all(d[c] > 0.9 for c in (3, 10, 12)) and np.delete(d, [3, 10, 12]).max() == 0.0
    f0, _, _ = M.run(frames, 0.35, 0)
    assert list(np.nonzero(f0)[0]) == [3, 10, 12]
    # the state as the device keeps it
    m = M.SceneModel(1, H, W, 0.35, 8)
    for t in range(11):
        m.update(frames[t:t + 1])
    assert m.state[0, 0] == 11 and m.state[0, 1] == 0 and not m.state[0, 2 + M.HIST:].any()
    assert np.array_equal(m.state[0, 2:2 + M.HIST].reshape(16, 32), M.hist(frames[10:11])[0])
    m.state[0, 0] = m.state[0, 1] = M.U32_MAX                              # both counters saturate
    m.update(frames[10:11])
    assert m.state[0, 0] == M.U32_MAX and m.state[0, 1] == M.U32_MAX
    assert M.thr_num(0.35, 288, 512) == math.floor(0.35 * 2.0 * 288 * 512) and M.thr_num(1.0, 4, 4) == 32


def test_quantisation():
    assert list(M.bins(np.array([np.nan, np.inf, -np.inf, -0.6, 0.7], np.float32))) == [0, 31, 0, 0, 31]
    k = np.arange(256)
    g = (k.astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    assert np.array_equal(M.bins(g), k >> 3)
    g2 = (k.astype(np.float32) * np.float32(1.0 / 255) - np.float32(0.5)).astype(np.float32)      # the driver's conversion
    assert np.array_equal(M.bins(g2), k >> 3)


def test_tiles_and_histograms():
    t = M.tiles(5, 7)
    assert t.shape == (5, 7) and t[0, 0] == 0 and t[4, 6] == 15
    assert list((4 * np.arange(7)) // 7) == [0, 0, 1, 1, 2, 2, 3] and list(t[0]) == [0, 0, 1, 1, 2, 2, 3]
    assert list(t[:, 0] // 4) == [0, 0, 1, 2, 3]
    g = np.full((2, 5, 7), -0.5, np.float32)
    g[1, 4, 6] = 0.5
    h = M.hist(g)
    assert h.dtype == np.uint32 and h.shape == (2, 16, 32) and int(h[0].sum()) == 35 and int(h[0, :, 0].sum()) == 35
    assert h[1, 15, 31] == 1 and h[1, 15, 0] == h[0, 15, 0] - 1
    assert list(M.distance(h[1:], h[:1])) == [2] and list(M.distance(h[:1], h[:1])) == [0]


def test_driver_flags():
    import deploy_bundle
    a = deploy_bundle.parse_args([])
    assert a.scene_cut is None and a.scene_gap is None
    a = deploy_bundle.parse_args(["--scene-cut"])
    assert a.scene_cut == 0.35 and a.scene_gap == 8
    a = deploy_bundle.parse_args(["--scene-cut", "0.5", "--scene-gap", "0", "--pipeline"])
    assert a.scene_cut == 0.5 and a.scene_gap == 0 and a.pipeline
    assert deploy_bundle.parse_args(["--scene-cut", "1"]).scene_cut == 1.0
    assert deploy_bundle.parse_args(["--scene-cut", "--y4m-in", "-"]).scene_cut == 0.35
    for bad in (["--scene-gap", "3"], ["--scene-cut", "0"], ["--scene-cut", "1.5"], ["--scene-cut", "-0.2"], ["--scene-cut", "nan"],
                ["--scene-cut", "x"], ["--scene-cut", "--scene-gap", "-1"], ["--scene-cut", "--scene-gap", "1.5"]):
        with pytest.raises(SystemExit):
            deploy_bundle.parse_args(bad)


def test_scene_cut_parameters_are_checked_on_the_host():
    from stabnet_amd import scene
    from stabnet_amd._lib import StabnetError
    assert scene.check_params(0.35, 8) == (0.35, 8) and scene.check_params(1, 0) == (1.0, 0)
    for bad in ((0.0, 8), (1.01, 8), (float("nan"), 8), (-0.1, 8), ("x", 8), (0.35, -1), (0.35, 1.5), (0.35, None)):
        with pytest.raises(StabnetError):
            scene.check_params(*bad)


def _path_case():
    """16 frames, every pair a small translation, pair 6 -> 7 a large jump; all statuses 1."""
    T, H, W = 16, 64, 96
    H_us = np.tile(np.eye(3).reshape(9), (T, 1))
    H_ss = np.tile(np.eye(3).reshape(9), (T - 1, 1))
    rng = np.random.default_rng(3)
    H_ss[:, 2] = rng.uniform(-0.01, 0.01, T - 1)
    H_ss[:, 5] = rng.uniform(-0.01, 0.01, T - 1)
    H_ss[:, 3] = rng.uniform(-0.002, 0.002, T - 1)
    H_ss[6, 2], H_ss[6, 5], H_ss[6, 3] = 0.9, -0.7, 0.2
    return T, H, W, H_us, H_ss, np.ones(T, np.int32), np.ones(T - 1, np.int32)


def test_host_metrics_leaves_the_pair_across_a_cut_out_of_the_path():
    from stabnet_amd import metrics
    from stabnet_amd._lib import StabnetError
    T, H, W, H_us, H_ss, s_us, s_ss = _path_case()
    plain = metrics.host_metrics(H_us, s_us, H_ss, s_ss, H, W, per_frame=True)
    assert "scene_cuts" not in plain
    cut = metrics.host_metrics(H_us, s_us, H_ss, s_ss, H, W, per_frame=True, cuts=[7])
    ident = H_ss.copy()
    ident[6] = np.eye(3).reshape(9)
    want = metrics.host_metrics(H_us, s_us, ident, s_ss, H, W, per_frame=True)
    assert cut["scene_cuts"] == 1 and cut["failed_pairs_stable_stable"] == 0
    for k in ("stability", "stability_translation", "stability_rotation", "cropping", "distortion", "path_translation", "path_rotation"):
        assert cut[k] == want[k], k
    assert cut["path_translation"] != plain["path_translation"]
    assert metrics.host_metrics(H_us, s_us, H_ss, s_ss, H, W, cuts=[])["scene_cuts"] == 0
    assert metrics.host_metrics(H_us, s_us, H_ss, s_ss, H, W, cuts=[0, 7, 7])["scene_cuts"] == 1     # no pair in front of frame 0
    for bad in ([T], [-1], [2.5]):
        with pytest.raises(StabnetError):
            metrics.host_metrics(H_us, s_us, H_ss, s_ss, H, W, cuts=bad)


def test_c_entries_refuse_before_the_device_is_touched():
    from stabnet_amd import _lib
    L = _lib.lib()
    assert L.stabnet_scene_state_words() == 1026
    one = ctypes.addressof((ctypes.c_int * 4)())                            # never dereferenced: every call below is refused first
    good = dict(grey=one, N=1, H=8, W=8, thr=10, gap=0, state=one, flag=one, dist=one, stream=0)
    for bad, word in ((dict(grey=0), b"null"), (dict(state=0), b"null"), (dict(flag=0), b"null"), (dict(dist=0), b"null"),
                      (dict(N=0), b"batch"), (dict(N=-3), b"batch"), (dict(H=3), b"outside"), (dict(W=3), b"outside"),
                      (dict(H=32768), b"outside"), (dict(W=40000), b"outside"), (dict(gap=-1), b"min_gap")):
        assert L.stabnet_scene_update(*dict(good, **bad).values()) == -1, bad
        assert word in L.stabnet_last_error(), (bad, L.stabnet_last_error())
    ring = dict(frames=one, masks=one, first=one, S=1, depth=32, H=8, W=8, flag=one, stream=0)
    for bad in (dict(frames=0), dict(masks=0), dict(first=0), dict(flag=0), dict(S=0), dict(depth=0), dict(H=0), dict(W=0)):
        assert L.stabnet_ring_reseed_if(*dict(ring, **bad).values()) == -1, bad
    assert L.stabnet_ring_reseed_if(*dict(ring, flag=0).values()) == -1 and b"flag" in L.stabnet_last_error()
