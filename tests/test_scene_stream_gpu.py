"""GPU: scene cuts inside the frame (StabNetStream.enable_scene_cut): after a flagged frame the run equals, bit for bit, a fresh run
on the clip that starts there with its first frame doubled; a detector that never fires changes nothing; streams in lock-step are
independent; all_black is not zeroed at a cut."""
import numpy as np
import pytest
import torch

import scene_model as M

pytestmark = pytest.mark.gpu

H, W, TA, TB, GAP = 64, 96, 10, 6, 8
KEYS = ("theta", "x_map", "y_map", "output", "black_pix", "frame")


@pytest.fixture(scope="module")
def setup(cuda):
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.2)
    A, B = M.cut_clip(H, W, TA, TB)
    return cfg, P, A, B


def _stream(setup, cuda, use_graph, streams=1):
    from stabnet_amd.deploy import StabNetStream
    cfg, P = setup[0], setup[1]
    return StabNetStream(P, H, W, cfg, streams=streams, device=cuda, use_graph=use_graph)


def _run(s, clip, cuda):
    """start(clip[0]) and a step per later frame -> [dict of host copies per step], the flags and D per step."""
    s.start(torch.from_numpy(clip[0:1]).to(cuda))
    outs, flags, dist = [], [], []
    for t in range(1, len(clip)):
        r = s.step(torch.from_numpy(clip[t:t + 1]).to(cuda))
        outs.append({k: r[k].cpu().numpy().copy() for k in KEYS})
        if "scene_cut" in r:
            flags.append(int(r["scene_cut"].cpu()[0])); dist.append(int(r["scene_dist"].cpu().numpy()[0]))
    return outs, flags, dist


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS)


@pytest.mark.parametrize("use_graph", [False, True])
def test_run_after_a_cut_equals_a_fresh_run(cuda, setup, use_graph):
    _, _, A, B = setup
    clip = np.concatenate([A, B])
    x = _stream(setup, cuda, use_graph)
    x.enable_scene_cut(min_gap=GAP)
    xo, flags, dist = _run(x, clip, cuda)
    assert [t + 1 for t, f in enumerate(flags) if f] == [TA], flags             # step t handles frame t + 1
    _, D, _ = M.run(clip, 0.35, GAP)
    assert dist == [int(v) for v in D[1:]]
    y = _stream(setup, cuda, use_graph)
    yo, _, _ = _run(y, np.concatenate([B[0:1], B]), cuda)                        # start(B[0]), step(B[0]), step(B[1]), ...
    for j in range(TB):
        assert _same(xo[TA - 1 + j], yo[j]), j                                   # X's frame TA + j is its step TA + j - 1
    if use_graph:
        assert x._graph is not None and y._graph is not None


@pytest.mark.parametrize("use_graph", [False, True])
def test_detector_that_never_fires_changes_nothing(cuda, setup, use_graph):
    _, _, A, B = setup
    clip = np.concatenate([A, B])
    plain = _stream(setup, cuda, use_graph)
    po, pf, _ = _run(plain, clip, cuda)
    assert pf == []                                                              # no new keys with the feature off
    never = _stream(setup, cuda, use_graph)
    never.enable_scene_cut(threshold=1.0, min_gap=GAP)
    no, nf, nd = _run(never, clip, cuda)
    assert nf == [0] * (len(clip) - 1) and max(nd) <= 2 * H * W
    for t in range(len(clip) - 1):
        assert _same(po[t], no[t]), t
    x = _stream(setup, cuda, use_graph)
    x.enable_scene_cut(min_gap=GAP)
    xo, xf, _ = _run(x, clip, cuda)
    for t in range(TA - 1):
        assert _same(po[t], xo[t]), t                                            # before the cut nothing differs
    for t in range(TA - 1, len(clip) - 1):
        assert not np.array_equal(po[t]["theta"], xo[t]["theta"]), t             # from the cut on the history is another one
        assert not np.array_equal(po[t]["output"], xo[t]["output"]), t


def test_lock_step_streams_cut_independently(cuda, setup):
    """S = 2, a cut in stream 1 only: stream 0 equals its single-stream run within test_deploy_gpu.py's lock-step tolerances, and
    stream 1 its own single-stream run with the feature on."""
    _, _, A, B = setup
    from stabnet_amd import synthetic
    A0 = synthetic.make_clip(H, W, TA + TB, seed=1, margin=32)                   # stream 0: scene A throughout
    c1 = np.concatenate([A, B])
    both = _stream(setup, cuda, False, streams=2)
    both.enable_scene_cut(min_gap=GAP)
    singles = [_stream(setup, cuda, False), _stream(setup, cuda, False)]
    for s in singles:
        s.enable_scene_cut(min_gap=GAP)
    both.start(torch.from_numpy(np.stack([A0[0], c1[0]])).to(cuda))
    singles[0].start(torch.from_numpy(A0[0:1]).to(cuda)); singles[1].start(torch.from_numpy(c1[0:1]).to(cuda))
    for t in range(1, TA + TB):
        rb = both.step(torch.from_numpy(np.stack([A0[t], c1[t]])).to(cuda))
        assert rb["scene_cut"].cpu().tolist() == [0, int(t == TA)], t
        for i, (s, c) in enumerate(zip(singles, (A0, c1))):
            r1 = s.step(torch.from_numpy(c[t:t + 1]).to(cuda))
            assert torch.allclose(rb["theta"][i], r1["theta"][0], atol=2e-6), (t, i)
            assert torch.allclose(rb["output"][i], r1["output"][0], atol=1e-4), (t, i)
            assert int(rb["scene_dist"].cpu().numpy()[i]) == int(r1["scene_dist"].cpu().numpy()[0])


def test_all_black_keeps_counting_across_a_cut(cuda, setup):
    _, _, A, B = setup
    clip = np.concatenate([A, B])
    x = _stream(setup, cuda, True)
    x.track_black()
    x.enable_scene_cut(min_gap=GAP)
    xo, flags, _ = _run(x, clip, cuda)
    assert sum(flags) == 1
    total = sum(np.rint(o["black_pix"][0]).astype(np.int64) for o in xo)
    assert np.array_equal(x.all_black[0].cpu().numpy().astype(np.int64), total)
