"""CPU: tests/tvl1_model.py, the NumPy yardstick of csrc/tvl1.hip, recovers known motions; the map it writes is the one
interpolate() reads; the C entry points refuse bad arguments before they touch a GPU; make_dataset.py without --flow writes the
bytes it wrote before."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tvl1_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MARGIN = 8
MOTIONS = {"translation": (1, 0, 0, 1, 3.3, -2.1), "affine": (1.01, 0.01, -0.01, 0.99, 5.5, 2.5)}


@functools.lru_cache(maxsize=None)
def solved(H, W, motion):
    I0, I1, ux, uy = M.make_pair(H, W, 1, MOTIONS[motion])
    u1, u2 = M.solve(I0, I1)
    return I0, I1, ux, uy, u1, u2


def test_zero_motion_gives_exactly_zero_flow():
    I0, _, _, _ = M.make_pair(72, 96, 1, (1, 0, 0, 1, 0, 0))
    u1, u2 = M.solve(I0, I0.copy())
    assert not u1.any() and not u2.any()


@pytest.mark.parametrize("motion", sorted(MOTIONS))
@pytest.mark.parametrize("size", [(72, 96), (96, 160)])
def test_known_motion_is_recovered(size, motion):
    """Mean endpoint error over the interior (8 px margin) at most one tenth of the zero flow's."""
    _, _, ux, uy, u1, u2 = solved(size[0], size[1], motion)
    inner = (slice(MARGIN, -MARGIN), slice(MARGIN, -MARGIN))
    epe = np.sqrt((u1 - ux) ** 2 + (u2 - uy) ** 2)[inner].mean()
    zero = np.sqrt(ux ** 2 + uy ** 2)[inner].mean()
    print("%dx%d %s: mean endpoint error %.3f px, zero flow %.3f px" % (size + (motion, epe, zero)))
    assert epe <= 0.1 * zero, (epe, zero)


@pytest.mark.parametrize("motion", sorted(MOTIONS))
def test_map_is_what_interpolate_reads(motion):
    from oracle import stabnet_oracle as O
    I0, I1, _, _, u1, u2 = solved(72, 96, motion)
    m = M.flow_to_map(u1, u2)
    assert m.shape == (72, 96, 2) and m.dtype == F
    warped = O.interpolate(I1[None, :, :, None], m[None, :, :, 0:1], m[None, :, :, 1:2])[0, :, :, 0]
    inner = (slice(MARGIN, -MARGIN), slice(MARGIN, -MARGIN))
    assert np.abs(warped - I0)[inner].mean() < np.abs(I1 - I0)[inner].mean()
    # an identity flow samples I1 at its own pixel centres: (2j/W - 1 + 1) * W/2 is j up to a few ulps of W, under 2e-5 px here,
    # and neighbouring pixels differ by less than 255.  (The last row and column are left out: the sampler clips its corner
    # indices before it forms the weights, spatial_transformer3.py:90-93, so a sample exactly on the last pixel weighs nothing.)
    ident = M.flow_to_map(np.zeros((72, 96), F), np.zeros((72, 96), F))
    same = O.interpolate(I1[None, :, :, None], ident[None, :, :, 0:1], ident[None, :, :, 1:2])[0, :, :, 0]
    assert np.abs(same - I1)[:-1, :-1].max() <= 255 * 2e-5 * 2


def test_level_sizes():
    assert M.level_sizes(288, 512) == [(288, 512), (144, 256), (72, 128), (36, 64), (18, 32)]
    assert M.level_sizes(37, 53) == [(37, 53), (19, 27)]
    assert M.level_sizes(16, 16) == [(16, 16)]
    assert M.level_sizes(288, 512, scales=2) == [(288, 512), (144, 256)]
    from stabnet_amd import flow
    for hw in ((288, 512), (37, 53), (16, 16), (31, 200)):
        assert flow.levels(*hw) == M.level_sizes(*hw)
    assert flow.levels(64, 64, flow.Tvl1Params(scales=3, min_side=4)) == M.level_sizes(64, 64, 3, 4)
    assert flow.fused_geometry()[0] >= 4


#        i0    i1    ps off  scl  B  H   W   tau   lam   theta sc wa it  ms  ws    bytes    uv    map   stream prof
FLOW_OK = [4096, 4096, 1, 0.0, 1.0, 1, 16, 16, 0.25, 0.15, 0.3, 5, 5, 30, 16, 4096, 1 << 30, 4096, 4096, 0, 0]


def test_bad_arguments_are_refused_without_a_gpu():
    """Pointers are never followed: every case fails a check before that."""
    from stabnet_amd import _lib
    L = _lib.lib()
    need = L.stabnet_tvl1_workspace_bytes(1, 16, 16, 5, 16)
    assert need > 0
    cases = [(0, 0), (1, 0), (15, 0), (2, 0), (5, 0), (6, 7), (7, 7), (8, 0.0), (8, -0.25), (9, 0.0), (9, -1.0), (10, 0.0),
             (10, float("nan")), (11, 0), (12, 0), (13, 0), (14, 1), (16, need - 1), (4, 0.0), (3, float("inf"))]
    for i, v in cases:
        a = list(FLOW_OK)
        a[i] = v
        assert L.stabnet_tvl1_flow(*a) == -1, (i, v)
        assert b"tvl1_flow" in L.stabnet_last_error(), (i, v)
    a = list(FLOW_OK)
    a[17] = a[18] = 0                                            # either output may be null, not both
    assert L.stabnet_tvl1_flow(*a) == -1 and b"both outputs" in L.stabnet_last_error()
    assert L.stabnet_tvl1_flow(*([0] + FLOW_OK[1:])) == -1 and b"null" in L.stabnet_last_error()
    # the stage entry points: null pointers, sizes below 2, B < 1
    P = 4096
    assert L.stabnet_tvl1_pyramid_down(0, 1, 1, 16, 16, P, 0, 0) == -1 and b"null" in L.stabnet_last_error()
    assert L.stabnet_tvl1_pyramid_down(P, 0, 1, 16, 16, P, 0, 0) == -1
    assert L.stabnet_tvl1_pyramid_down(P, 1, 1, 1, 16, P, 0, 0) == -1
    assert L.stabnet_tvl1_gradient(P, 1, 1, 16, 16, P, 0, 0, 0) == -1 and b"null" in L.stabnet_last_error()
    assert L.stabnet_tvl1_gradient(P, 1, 0, 16, 16, P, P, 0, 0) == -1
    assert L.stabnet_tvl1_warp(P, P, 1, P, P, P, 0, 1, 16, 16, 0, 0) == -1 and b"null" in L.stabnet_last_error()
    assert L.stabnet_tvl1_warp(P, P, 1, P, P, P, P, 1, 16, 1, 0, 0) == -1
    assert L.stabnet_tvl1_upsample(P, 1, 8, 8, 0, 16, 16, 0, 0) == -1 and b"null" in L.stabnet_last_error()
    assert L.stabnet_tvl1_upsample(P, 1, 8, 9, P, 16, 16, 0, 0) == -1 and b"coarse" in L.stabnet_last_error()
    assert L.stabnet_tvl1_flow_to_map(P, 1, 16, 16, 0, 0, 0, 0) == -1
    assert L.stabnet_tvl1_flow_to_map(0, 1, 16, 16, P, P, 0, 0) == -1
    it_ok = [P, 2 * P, P, 1, 16, 16, 0.25, 0.15, 0.3, 1, 1, 0, 0]
    for i, v in ((0, 0), (1, 0), (2, 0), (1, P), (3, 0), (4, 1), (5, 1), (6, 0.0), (7, -0.1), (8, 0.0), (9, 0), (10, 2)):
        a = list(it_ok)
        a[i] = v
        assert L.stabnet_tvl1_iterate(*a) == -1, (i, v)
        assert b"tvl1_iterate" in L.stabnet_last_error()
    assert L.stabnet_tvl1_levels(16, 16, 0, 16, 0) == -1 and L.stabnet_tvl1_levels(16, 16, 5, 1, 0) == -1


def test_workspace_bytes():
    from stabnet_amd import flow
    from stabnet_amd._lib import StabnetError
    last = 0
    for B in (1, 2, 3, 8, 9, 32):
        n = flow.workspace_bytes(B, 288, 512)
        assert n > last
        last = n
        pyramid = sum(h * w for h, w in M.level_sizes(288, 512))
        # both images at every coarser level, and at the finest size: two gradients, four constants, two states of six planes
        assert n >= 4 * B * (2 * (pyramid - 288 * 512) + 18 * 288 * 512)
        assert n <= 4 * B * 21 * 288 * 512 + (1 << 16)
    assert flow.workspace_bytes(1, 288, 512, flow.Tvl1Params(scales=1)) < flow.workspace_bytes(1, 288, 512)
    for bad in ((0, 16, 16), (1, 7, 16), (1, 16, 7), (65536, 16, 16)):
        with pytest.raises(StabnetError, match="workspace_bytes"):
            flow.workspace_bytes(*bad)
    with pytest.raises(StabnetError):
        flow.workspace_bytes(1, 16, 16, flow.Tvl1Params(scales=0))


def test_make_dataset_without_flow_writes_the_same_bytes(tmp_path):
    """tools/make_dataset.py with no --flow (and with --flow none) against write_dataset called directly with the samples it
    always built: list.txt and the record files byte for byte; no GPU is touched (HIP_VISIBLE_DEVICES hides any)."""
    import dataset_fixture as Fx
    from PIL import Image
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import write_dataset
    clips = []
    for k in range(2):
        pair = []
        for kind in range(2):
            path = str(tmp_path / ("clip%d_%d.npy" % (k, kind)))
            np.save(path, np.stack([Fx.image(k, t, kind)[:, :, ::-1] for t in range(Fx.T)]))        # BGR, as make_dataset.py reads it
            pair.append(path)
        clips.append(pair)
    first = max(Config().indices) + 1
    samples = [{"stable_path": "stable/%d/" % k, "unstable_path": "unstable/%d/" % k, "pos": pos}
               for k in range(2) for pos in range(first, Fx.T)]
    want = tmp_path / "direct"
    names = write_dataset(str(want), "train", samples, records_per_file=10)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for extra in ([], ["--flow", "none"]):
        got = tmp_path / ("cli_" + "_".join(extra).strip("-"))
        cmd = [sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), "--out", str(got), "--split", "train"]
        for s, u in clips:
            cmd += ["--pair", s, u]
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for name in ["list.txt"] + names:
            assert (got / "train" / name).read_bytes() == (want / "train" / name).read_bytes(), name
        assert sorted(os.listdir(got / "train")) == sorted(["list.txt"] + names)
        ref = tmp_path / "frame.jpg"
        Image.fromarray(Fx.image(1, 7, 0)).save(str(ref), quality=90, subsampling=2)
        assert (got / "stable" / "1" / "7.jpg").read_bytes() == ref.read_bytes()
