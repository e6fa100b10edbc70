"""GPU: the scene-cut operator (csrc/scene.hip) against the NumPy model (tests/scene_model.py), bit for bit: the tile histograms, D,
the flag and the whole state over consecutive calls; constant and special-value images; a captured graph; and the predicated ring
reseed between canary bands."""
import ctypes

import numpy as np
import pytest
import torch

import scene_model as M
from _guarded import Guarded

pytestmark = pytest.mark.gpu


_clip = M.multi_stream_clip                                   # [T,N,H,W]: stream n cuts from scene A to scene B at frame 2 + n


def _run_against_model(cuda, frames, threshold, min_gap):
    from stabnet_amd.scene import SceneCut
    T, N, H, W = frames.shape
    sc = SceneCut(N, H, W, threshold, min_gap, device=cuda)
    model = M.SceneModel(N, H, W, threshold, min_gap)
    assert sc.thr_num == model.thr_num
    flags = []
    for t in range(T):
        g = torch.from_numpy(frames[t]).to(cuda)
        sc.update(g)
        f, D, h = model.update(frames[t])
        state = sc.state.cpu().numpy().view(np.uint32)
        assert np.array_equal(state[:, 2:2 + M.HIST].reshape(N, 16, 32), h), t            # this frame's histogram, now in prev
        assert np.array_equal(sc.dist.cpu().numpy(), D), (t, sc.dist.cpu().numpy(), D)
        assert np.array_equal(sc.flag.cpu().numpy(), f), t
        assert np.array_equal(state, model.state), t                                        # seen, since, prev, cur == 0
        flags.append(f.copy())
    return np.stack(flags)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (45, 77), (64, 96)])
def test_update_matches_model(cuda, H, W, N):
    if H * W < 1000:                                         # tiny frames: any two noise images, the rule still runs on the device
        frames = np.random.default_rng(H * W + N).uniform(-0.5, 0.5, (6, N, H, W)).astype(np.float32)
        frames[3:] = frames[3:] * np.float32(0.2) - np.float32(0.3)
    else:
        frames = _clip(N, H, W)
    flags = _run_against_model(cuda, frames, 0.35, 2)
    if H * W >= 1000:
        for n in range(N):                                   # min_gap 2: the cut of stream n at frame 2 + n is flagged, nothing else
            assert list(np.nonzero(flags[:, n])[0]) == [2 + n], (n, flags[:, n])


def test_update_matches_model_288x512(cuda):
    flags = _run_against_model(cuda, _clip(1, 288, 512), 0.35, 2)
    assert list(np.nonzero(flags[:, 0])[0]) == [2]


def test_unaligned_frame_takes_the_scalar_path(cuda):
    """W % 4 == 0 but the frame starts 4 bytes off a 16-byte boundary: one pixel per load, the same counts."""
    from stabnet_amd.scene import SceneCut
    H, W = 64, 96
    frames = _clip(1, H, W)[:, 0]
    sc = SceneCut(1, H, W, 0.35, 2, device=cuda)
    model = M.SceneModel(1, H, W, 0.35, 2)
    buf = torch.empty(H * W + 1, dtype=torch.float32, device=cuda)
    g = buf[1:].view(1, H, W)
    assert g.data_ptr() % 16 == 4
    for t in range(4):
        g.copy_(torch.from_numpy(frames[t:t + 1]))
        sc.update(g)
        f, D, _ = model.update(frames[t:t + 1])
        assert np.array_equal(sc.state.cpu().numpy().view(np.uint32), model.state) and np.array_equal(sc.dist.cpu().numpy(), D), t
        assert np.array_equal(sc.flag.cpu().numpy(), f), t


@pytest.mark.parametrize("H,W", [(45, 77), (288, 512)])
def test_constant_images(cuda, H, W):
    """Every pixel in one bin: all lanes of a wave meet in one counter of each tile (the worst case of the LDS histograms)."""
    vals = np.array([-0.5, -0.5, 0.5, 0.1, 0.1, -0.2], np.float32)
    frames = np.broadcast_to(vals[:, None, None, None], (6, 2, H, W)).copy()
    frames[:, 1] = frames[::-1, 0]
    flags = _run_against_model(cuda, frames, 0.5, 0)
    assert list(flags[:, 0]) == [0, 0, 1, 1, 0, 1]           # d is 0 or 1 between constant images


def test_special_values(cuda):
    H, W = 8, 12
    g = np.zeros((1, H, W), np.float32)
    g[0, 0, :6] = [np.nan, np.inf, -np.inf, -0.6, 0.7, -np.nan]
    b = M.bins(g[0, 0, :6])
    assert list(b) == [0, 31, 0, 0, 31, 0]
    frames = np.stack([g, g[:, ::-1].copy(), g, np.full_like(g, np.nan), g, g])
    _run_against_model(cuda, frames, 0.01, 0)


def test_graph_replay_follows_the_model(cuda):
    from stabnet_amd.scene import SceneCut
    H, W = 64, 96
    frames = _clip(1, H, W, T=6)[:, 0]
    sc = SceneCut(1, H, W, 0.35, 1, device=cuda)
    model = M.SceneModel(1, H, W, 0.35, 1)
    g = torch.empty((1, H, W), dtype=torch.float32, device=cuda)
    g.copy_(torch.from_numpy(frames[0:1]))
    sc.update(g)                                             # eager: loads the module
    model.update(frames[0:1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # records only
        sc.update(g)
    got = []
    for t in range(1, 5):
        g.copy_(torch.from_numpy(frames[t:t + 1]))
        graph.replay()
        f, D, _ = model.update(frames[t:t + 1])
        assert np.array_equal(sc.dist.cpu().numpy(), D) and np.array_equal(sc.flag.cpu().numpy(), f), t
        assert np.array_equal(sc.state.cpu().numpy().view(np.uint32), model.state), t
        got.append(int(f[0]))
    assert got == [0, 1, 0, 0]                               # the cut of stream 0 sits at frame 2


@pytest.mark.parametrize("H,W", [(5, 7), (64, 96)])
def test_ring_reseed_if(cuda, H, W):
    from stabnet_amd import _lib
    S, depth, hw = 3, 32, H * W
    rng = np.random.default_rng(7)
    f0, m0 = rng.standard_normal((S, depth, hw)).astype(np.float32), rng.standard_normal((S, depth, hw)).astype(np.float32)
    first = rng.standard_normal((S, hw)).astype(np.float32)
    frames, masks, fst = Guarded(cuda, S * depth * hw, f0), Guarded(cuda, S * depth * hw, m0), Guarded(cuda, S * hw, first)
    flag = Guarded(cuda, S, np.array([0, 1, 0], np.int32).view(np.float32))
    _lib.call("stabnet_ring_reseed_if", frames.t.data_ptr(), masks.t.data_ptr(), fst.t.data_ptr(), S, depth, H, W, flag.t.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for what, b in (("frames", frames), ("masks", masks), ("first", fst), ("flag", flag)):
        b.check(what)
    fr, ma = frames.np().reshape(S, depth, hw), masks.np().reshape(S, depth, hw)
    for s in (0, 2):                                         # untouched, byte for byte
        assert np.array_equal(fr[s].view(np.uint32), f0[s].view(np.uint32)) and np.array_equal(ma[s].view(np.uint32), m0[s].view(np.uint32)), s
    assert np.array_equal(fr[1].view(np.uint32), np.broadcast_to(first[1], (depth, hw)).view(np.uint32))
    assert np.array_equal(ma[1].view(np.uint32), np.zeros((depth, hw), np.uint32))
    assert np.array_equal(fst.np().view(np.uint32), first.reshape(-1).view(np.uint32))
    # the same bits as stabnet_ring_init for that stream
    ref_f, ref_m = torch.empty(depth * hw, device=cuda), torch.empty(depth * hw, device=cuda)
    _lib.call("stabnet_ring_init", ref_f.data_ptr(), ref_m.data_ptr(), fst.t[hw:].data_ptr(), 1, depth, H, W, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(ref_f, frames.t[depth * hw:2 * depth * hw]) and torch.equal(ref_m, masks.t[depth * hw:2 * depth * hw])
    # a null flag is refused before anything is launched
    L = _lib.lib()
    assert L.stabnet_ring_reseed_if(frames.t.data_ptr(), masks.t.data_ptr(), fst.t.data_ptr(), S, depth, H, W, 0, 0) == -1
    assert b"flag" in L.stabnet_last_error()


def test_state_words_and_host_pointer_refused(cuda):
    from stabnet_amd import _lib
    L = _lib.lib()
    assert L.stabnet_scene_state_words() == 1026 == M.WORDS
    host = (ctypes.c_float * 64)()
    state = torch.zeros(1026, dtype=torch.int32, device=cuda)
    out = torch.zeros(2, dtype=torch.int32, device=cuda)
    rc = L.stabnet_scene_update(ctypes.addressof(host), 1, 8, 8, 10, 0, state.data_ptr(), out.data_ptr(), out[1:].data_ptr(), 0)
    assert rc == -1 and b"grey" in L.stabnet_last_error()
    torch.cuda.synchronize()
    assert int(state.abs().sum()) == 0
