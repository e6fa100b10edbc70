"""CPU checks of what the augmentation's GPU tests lean on: the resized size int(H / rate) as the host mirror, the oracle and Python
compute it, the NumPy model of the kernels' summation order (tests/augment_model.py), the oracle's crop-rate argument, and the
range of the drawn crop offsets."""
import numpy as np
import pytest

from augment_model import kernel_channel_mean
from oracle import stabnet_oracle as O

RATES = (0.9, 0.85, 0.8, 0.7, 0.6, 1.0)


@pytest.mark.parametrize("rate", RATES)
def test_resized_hw_is_pythons_float64_division(rate):
    from stabnet_amd import data
    from stabnet_amd.config import Config
    cfg = Config(random_crop_rate=rate)
    for H in range(2, 2200):
        W = 2201 - H
        want = (int(H / rate), int(W / rate))
        assert data.resized_hw(cfg, H, W) == want
        assert O.aug_resized_hw(H, W, rate) == want
    if rate == 0.8:
        assert data.resized_hw(cfg, 288, 512) == (360, 640)


def test_float32_rate_gives_another_size():
    """Why the C entry takes the rate as a double: the same division with the rate rounded to float32 first disagrees with
    int(H / rate) at many sizes for 0.8, 0.85 and 0.6 (0.9f < 0.9 happens to agree everywhere in this range)."""
    def bad(rate):
        return sum(int(H / float(np.float32(rate))) != int(H / rate) for H in range(2, 2200))
    assert bad(0.9) == 0 and bad(1.0) == 0
    assert bad(0.8) > 0 and bad(0.6) > 0 and bad(0.85) > 0
    assert int(288 / 0.8) == 360 and int(288 / float(np.float32(0.8))) == 359
    # the sizes tests/test_augment_gpu.py uses for these rates are among the disagreeing ones, in at least one dimension
    for rate, H, W in ((0.8, 16, 16), (0.8, 36, 64), (0.6, 9, 21), (0.85, 17, 34)):
        r32 = float(np.float32(rate))
        assert (int(H / r32), int(W / r32)) != (int(H / rate), int(W / rate)), (rate, H, W)


@pytest.mark.parametrize("H,W", [(1, 1), (9, 20), (16, 16), (7, 37), (129, 128), (45, 77), (288, 512), (257, 256)])
def test_kernel_channel_mean_within_one_ulp_of_float64_mean(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    for scale, shift in ((0.5, 0.0), (0.01, 0.3), (1.0, -0.25)):
        img = (rng.uniform(-1, 1, (H, W)) * scale + shift).astype(np.float32)
        got = kernel_channel_mean(img)
        want = np.float32(img.astype(np.float64).mean())
        assert got.dtype == np.float32
        assert abs(float(got) - float(want)) <= float(np.spacing(np.abs(want))), (got, want)


@pytest.mark.parametrize("H,W", [(9, 20), (16, 16), (129, 128), (45, 77)])
@pytest.mark.parametrize("v", [0.0, -0.4, 0.084375, 0.5, -0.1234567])
def test_kernel_channel_mean_of_a_constant_plane_is_the_constant(H, W, v):
    img = np.full((H, W), v, np.float32)
    assert kernel_channel_mean(img) == img[0, 0]


def _pair_inputs(rng, H, W, bc, M):
    stable = rng.uniform(-0.5, 0.5, (H, W, 2 * (bc + 1))).astype(np.float32)
    unstable = rng.uniform(-0.5, 0.5, (H, W, 2)).astype(np.float32)
    flow = rng.uniform(-1, 1, (H, W, 2)).astype(np.float32)
    m1 = rng.uniform(-1.1, 1.1, (M, 4)).astype(np.float32)
    m2 = rng.uniform(-1.1, 1.1, (M, 4)).astype(np.float32)
    Hs = np.tile(np.eye(3, dtype=np.float32), (2, bc, 1, 1)) + rng.uniform(-0.1, 0.1, (2, bc, 3, 3)).astype(np.float32)
    return stable, unstable, flow, m1, m2, Hs


def test_assemble_pair_rate_argument_is_live_and_default_is_unchanged():
    H, W, bc, M = 16, 24, 2, 7
    rng = np.random.default_rng(3)
    stable, unstable, flow, m1, m2, Hs = _pair_inputs(rng, H, W, bc, M)
    para = {"h": 1, "w": 2, "flip": 1}
    args = (stable, unstable, flow, m1, 5, m2, M, para, np.float32(1.2), np.float32(0.05), Hs[0], Hs[1])
    default = O.assemble_pair(*args, O.Config(height=H, width=W, before_ch=bc, max_matches=M))
    r09 = O.assemble_pair(*args, O.Config(height=H, width=W, before_ch=bc, max_matches=M, random_crop_rate=0.9))
    r08 = O.assemble_pair(*args, O.Config(height=H, width=W, before_ch=bc, max_matches=M, random_crop_rate=0.8))
    assert O.Config().random_crop_rate == O.RANDOM_CROP_RATE == 0.9
    for d, a in zip(default, r09):
        assert d.dtype == a.dtype and np.array_equal(d, a)
    # the default call is today's arithmetic: the module-level rate and the float64 mean, channel by channel
    st = np.stack([O.warp_img(stable[..., i], para, np.float32(1.2), np.float32(0.05)) for i in range(2 * (bc + 1))], axis=2)
    assert np.array_equal(default[1], st[..., 0:1]) and np.array_equal(default[3], st[..., bc + 1:bc + 2])
    assert np.array_equal(default[0][..., bc:2 * bc], O.add_mask(st[..., 1:1 + bc], Hs[0])[..., bc:])
    assert np.array_equal(default[4], O.warp_flow(flow, para))
    fm1, mk1 = O.warp_point(m1, np.arange(M) < 5, para, H, W)
    assert np.array_equal(default[5], fm1) and np.array_equal(default[6], mk1)
    # the rate reaches the image channels, the flow and the points
    for k in (0, 1, 2, 3, 4, 5, 7):
        assert not np.array_equal(r08[k], r09[k]), k


def test_assemble_pair_mean_of_is_used_for_every_image_channel():
    H, W, bc, M = 9, 20, 1, 3
    rng = np.random.default_rng(4)
    stable, unstable, flow, m1, m2, Hs = _pair_inputs(rng, H, W, bc, M)
    para = {"h": 0, "w": 1, "flip": 0}
    cfg = O.Config(height=H, width=W, before_ch=bc, max_matches=M)
    seen = []

    def mean_of(img):
        assert img.shape == (H, W) and img.dtype == np.float32
        seen.append(1)
        return np.float32(img.astype(np.float64).mean())
    a = O.assemble_pair(stable, unstable, flow, m1, 1, m2, 2, para, np.float32(0.7), np.float32(-0.02), Hs[0], Hs[1], cfg, mean_of=mean_of)
    b = O.assemble_pair(stable, unstable, flow, m1, 1, m2, 2, para, np.float32(0.7), np.float32(-0.02), Hs[0], Hs[1], cfg)
    assert len(seen) == 2 * (bc + 1) + 2
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    none = O.assemble_pair(stable, unstable, None, None, 0, None, 0, para, np.float32(0.7), np.float32(-0.02), Hs[0], Hs[1], cfg)
    assert none[4] is None and none[5] is None and none[8] is None and np.array_equal(none[0], b[0])


@pytest.mark.parametrize("rate", RATES)
def test_get_rand_para_stays_inside_the_resized_frame(rate):
    from stabnet_amd import data
    from stabnet_amd.config import Config
    cfg = Config(random_crop_rate=rate)
    rng = np.random.default_rng(7)
    x0s = [0, 1, (1 << 32) - 1, (1 << 31), (1 << 31) - 1] + [int(v) for v in rng.integers(0, 1 << 32, 40, dtype=np.uint64)]
    for H, W in ((9, 20), (16, 16), (7, 37), (45, 77), (288, 512), (2, 2)):
        h, w = data.resized_hw(cfg, H, W)
        assert h >= H and w >= W
        for x0 in x0s:
            p = data.get_rand_para(x0, cfg, H, W)
            assert 0 <= p["h"] < max(h - H, 1) and 0 <= p["w"] < max(w - W, 1), (rate, H, W, x0, p)
            assert p["flip"] == (p["h"] + p["w"]) % 2
            if rate == 1.0:
                assert (p["h"], p["w"], p["flip"]) == (0, 0, 0)
