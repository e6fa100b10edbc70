"""GPU parity of the training-sample assembly (stabnet_augment_pairs) against the oracle's restatement of
get_data_mini_after.py:14-147,229-253.  Image channels: the contrast mean is a float64 sum on both sides, so values agree
to the last bit except where the two means round differently (tolerance 2e-7 abs); masks, flow and points are bit-exact.
Below that first test: the C entry on canary-banded buffers against the oracle with the kernels' own summation order for the mean
(tests/augment_model.py), every output bit for bit, at the edge shapes, rates, channel counts, match counts, offsets and error paths."""
import numpy as np
import pytest
import torch

from _guarded import Guarded, _check_all, _same_bits
from augment_model import kernel_channel_mean
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,H,W,seed", [(2, 36, 64, 0), (3, 45, 77, 1), (1, 288, 512, 2)])
def test_augment_pairs_matches_oracle(cuda, N, H, W, seed):
    from stabnet_amd import data
    from stabnet_amd.config import Config
    cfg = Config(height=H, width=W, max_matches=96)
    ocfg = O.Config(height=H, width=W, max_matches=96)
    rng = np.random.default_rng(seed)
    bc = cfg.before_ch
    stable = rng.uniform(-0.5, 0.5, (N, H, W, 2 * (bc + 1))).astype(np.float32)
    unstable = rng.uniform(-0.5, 0.5, (N, H, W, 2)).astype(np.float32)
    gx, gy = np.meshgrid(np.linspace(-1, 1, W, dtype=np.float32), np.linspace(-1, 1, H, dtype=np.float32))
    flow = (np.stack([gx, gy], 2)[None] + rng.normal(0, 0.05, (N, H, W, 2))).astype(np.float32)
    m1 = rng.uniform(-1.1, 1.1, (N, cfg.max_matches, 4)).astype(np.float32)
    m2 = rng.uniform(-1.1, 1.1, (N, cfg.max_matches, 4)).astype(np.float32)
    n1 = rng.integers(0, cfg.max_matches, N).astype(np.int32)
    n2 = rng.integers(0, cfg.max_matches, N).astype(np.int32)
    para, jitter, Hs = data.draw(rng, cfg, N, H, W)
    para[0, 2] = 1                                   # make sure both flip states are exercised
    if N > 1:
        para[1, 2] = 0
    got = data.augment_pairs(torch.from_numpy(stable).to(cuda), torch.from_numpy(unstable).to(cuda), torch.from_numpy(flow).to(cuda),
                             torch.from_numpy(m1).to(cuda), n1, torch.from_numpy(m2).to(cuda), n2, para, jitter, Hs, cfg)
    got = [g.cpu().numpy() for g in got]
    for n in range(N):
        p = {"h": int(para[n, 0]), "w": int(para[n, 1]), "flip": int(para[n, 2])}
        want = O.assemble_pair(stable[n], unstable[n], flow[n], m1[n], int(n1[n]), m2[n], int(n2[n]), p, jitter[n, 0],
                               jitter[n, 1], Hs[n, 0].reshape(bc, 3, 3), Hs[n, 1].reshape(bc, 3, 3), ocfg)
        x1, y1, x2, y2, fl, f1, k1, f2, k2 = want
        for name, g, w in (("x1", got[0][n], x1), ("x2", got[2][n], x2)):
            assert np.array_equal(g[..., :bc], w[..., :bc]), name + " masks"
            assert np.abs(g[..., bc:] - w[..., bc:]).max() <= 2e-7, name
        assert np.abs(got[1][n] - y1).max() <= 2e-7 and np.abs(got[3][n] - y2).max() <= 2e-7
        assert np.array_equal(got[4][n], fl), "flow"
        assert np.array_equal(got[5][n], f1) and np.array_equal(got[7][n], f2), "points"
        assert np.array_equal(got[6][n] > 0.5, k1) and np.array_equal(got[8][n] > 0.5, k2), "point masks"
        assert 0 < got[0][n][..., :bc].mean() < 1                      # masks are neither empty nor full


# ---------------------------------------------------------------------------------------------------------------------------------
# The C entry itself, every array between canary bands (tests/_guarded.py), the workspace NaN-filled and exactly as long as
# stabnet_augment_workspace_bytes says, against O.assemble_pair with the contrast mean summed in the kernels' documented order
# (tests/augment_model.py).  With the same summation order on both sides nothing is left to a tolerance: every output array is
# compared bit for bit.
OUTS = ("x1", "y1", "x2", "y2", "flow", "fm1", "mk1", "fm2", "mk2")
F32 = np.float32


def _legal_para(rng, N, H, W, rate, flips):
    h, w = O.aug_resized_hw(H, W, rate)
    return np.array([(rng.integers(0, h - H + 1), rng.integers(0, w - W + 1), flips[n % len(flips)]) for n in range(N)], np.int32)


def _inputs(seed, N, H, W, bc, M, rate, flips=(1, 0, 1), counts=None):
    from stabnet_amd import data
    from stabnet_amd.config import Config
    rng = np.random.default_rng(seed)
    cfg = Config(height=H, width=W, before_ch=bc, max_matches=M, random_crop_rate=rate)
    gx, gy = np.meshgrid(np.linspace(-1, 1, W, dtype=F32), np.linspace(-1, 1, H, dtype=F32))
    _, jitter, Hs = data.draw(rng, cfg, N, H, W)
    if counts is None:                                   # 0 and M always occur
        counts = ([0, M, M // 2][:N], [M, 0, (M + 1) // 2][:N]) if N > 1 else ([M], [0])
    return {
        "stable": rng.uniform(-0.5, 0.5, (N, H, W, 2 * (bc + 1))).astype(F32),
        "unstable": rng.uniform(-0.5, 0.5, (N, H, W, 2)).astype(F32),
        "flow": (np.stack([gx, gy], 2)[None] + rng.normal(0, 0.05, (N, H, W, 2))).astype(F32),
        "m1": rng.uniform(-1.1, 1.1, (N, M, 4)).astype(F32), "m2": rng.uniform(-1.1, 1.1, (N, M, 4)).astype(F32),
        "n1": np.asarray(counts[0], np.int32), "n2": np.asarray(counts[1], np.int32),
        "para": _legal_para(rng, N, H, W, rate, flips), "jitter": jitter, "Hs": Hs,
    }


def _as_f32_bits(a):
    """int32 arrays travel in float32 buffers, bit for bit (Guarded counts float32 words)."""
    a = np.ascontiguousarray(a)
    return a.view(F32) if a.dtype == np.int32 else a


def _out_sizes(N, H, W, bc, M):
    nx = 2 * bc + 1
    return {"x1": N * H * W * nx, "y1": N * H * W, "x2": N * H * W * nx, "y2": N * H * W, "flow": N * H * W * 2,
            "fm1": N * M * 4, "mk1": N * M, "fm2": N * M * 4, "mk2": N * M}


def _out_shapes(N, H, W, bc, M):
    nx = 2 * bc + 1
    return {"x1": (N, H, W, nx), "y1": (N, H, W, 1), "x2": (N, H, W, nx), "y2": (N, H, W, 1), "flow": (N, H, W, 2),
            "fm1": (N, M, 4), "mk1": (N, M), "fm2": (N, M, 4), "mk2": (N, M)}


class _Call:
    """One call of stabnet_augment_pairs on guarded buffers sized by the inputs.  `geom` overrides what the entry is told (error
    paths)."""

    def __init__(self, cuda, inp, rate, with_flow=True, with_matches=True, out_init=None, ws_init=None):
        from stabnet_amd import _lib
        self.cuda, self.rate = cuda, rate
        N, H, W, C = inp["stable"].shape
        bc, M = C // 2 - 1, inp["m1"].shape[1]
        self.dims = dict(N=N, H=H, W=W, bc=bc, M=M)
        self.inb = {k: Guarded(cuda, v.size + (1 if k == "stable" else 0), init=None, dtype=torch.float32) for k, v in inp.items()}
        for k, v in inp.items():
            self.inb[k].t[:v.size].copy_(torch.from_numpy(_as_f32_bits(v).reshape(-1)).to(cuda))
        self.in_bits = {k: b.np() for k, b in self.inb.items()}
        self.outb = {k: Guarded(cuda, n, init=out_init) for k, n in _out_sizes(N, H, W, bc, M).items()}
        self.ws_bytes = int(_lib.lib().stabnet_augment_workspace_bytes(N, H, W, bc))
        assert self.ws_bytes % 4 == 0
        self.ws = Guarded(cuda, max(self.ws_bytes // 4, 64), init=ws_init)          # float32 NaN unless told otherwise
        self.with_flow, self.with_matches = with_flow, with_matches

    def run(self, stable_shift=0, ws_bytes=None, null=(), **geom):
        from stabnet_amd import _lib
        from stabnet_amd._tensor import stream_ptr
        d = dict(self.dims, rate=self.rate)
        d.update(geom)
        i, o = self.inb, self.outb
        p = lambda b: 0 if any(b is o[k] for k in null) else b.t.data_ptr()
        _lib.call("stabnet_augment_pairs", p(i["stable"]) + stable_shift, p(i["unstable"]), p(i["flow"]) if self.with_flow else 0,
                  p(i["m1"]) if self.with_matches else 0, p(i["n1"]), p(i["m2"]), p(i["n2"]), p(i["para"]), p(i["jitter"]), p(i["Hs"]),
                  d["N"], d["H"], d["W"], d["bc"], d["M"], float(d["rate"]), p(o["x1"]), p(o["y1"]), p(o["x2"]), p(o["y2"]), p(o["flow"]),
                  p(o["fm1"]), p(o["mk1"]), p(o["fm2"]), p(o["mk2"]), p(self.ws), self.ws_bytes if ws_bytes is None else ws_bytes,
                  stream_ptr(self.cuda), device=self.cuda)
        return self

    def results(self):
        """Outputs as host arrays, after checking every canary band and that no input changed."""
        named = {"in " + k: b for k, b in self.inb.items()}
        named.update({"out " + k: b for k, b in self.outb.items()})
        named["workspace"] = self.ws
        _check_all(named)
        for k, b in self.inb.items():
            assert _same_bits(b.np(), self.in_bits[k]), "input %s was written" % k
        shapes = _out_shapes(**self.dims)
        return {k: self.outb[k].np()[:int(np.prod(shapes[k]))].reshape(shapes[k]) for k in OUTS}


def _oracle(inp, rate, para=None):
    """O.assemble_pair per sample with the kernels' summation order -> the nine arrays stacked over N (masks as 0/1 float32)."""
    N, H, W, C = inp["stable"].shape
    bc, M = C // 2 - 1, inp["m1"].shape[1]
    ocfg = O.Config(height=H, width=W, before_ch=bc, max_matches=M, random_crop_rate=rate)
    para = inp["para"] if para is None else para
    per = []
    for n in range(N):
        p = {"h": int(para[n, 0]), "w": int(para[n, 1]), "flip": int(para[n, 2] != 0)}
        per.append(O.assemble_pair(inp["stable"][n], inp["unstable"][n], inp["flow"][n], inp["m1"][n], int(inp["n1"][n]), inp["m2"][n],
                                   int(inp["n2"][n]), p, inp["jitter"][n, 0], inp["jitter"][n, 1], inp["Hs"][n, 0].reshape(bc, 3, 3),
                                   inp["Hs"][n, 1].reshape(bc, 3, 3), ocfg, mean_of=kernel_channel_mean))
    return {k: np.stack([np.asarray(s[j], F32) for s in per]) for j, k in enumerate(OUTS)}


def _assert_bits(got, want, keys=OUTS, what="", nan_is_nan=False):
    """Bit equality of every element.  nan_is_nan (only where a test feeds NaN in): an element that is NaN on both sides counts as
    equal, since IEEE 754 leaves the sign and payload of an arithmetic NaN open."""
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k)
        differ = got[k].view(np.uint32) != want[k].view(np.uint32)
        if nan_is_nan:
            differ &= ~(np.isnan(got[k]) & np.isnan(want[k]))
        if differ.any():
            bad = np.argwhere(differ)
            i = tuple(bad[0])
            raise AssertionError("%s %s: %d of %d elements differ, first at %s: got %r want %r"
                                 % (what, k, len(bad), got[k].size, i, got[k][i], want[k][i]))


# (H, W): 9x20 under one 256-pixel block, 16x16 exactly one, 7x37 one block + 3 pixels, 129x128 = 65 blocks (aug_means_kernel's strided
# loop runs twice), 45x77 odd.  before_ch 1 / 6 / 14, max_matches 1 / 256 / 257 / 3000 (aug_points_kernel: one block, exactly one, one + 1
# thread, 12), counts 0 and M, flips 1, 0, 1.  0.8 at 16x16 and 36x64, 0.6 at 9x21 and 0.85 at 17x34 are sizes where int(H / rate)
# differs between a float64 and a float32 rate; 1.0 makes the resize the identity.
PARITY_CASES = [
    # N, H, W, bc, M, rate
    (3, 9, 20, 6, 1, 0.9),
    (3, 16, 16, 1, 256, 0.9),
    (3, 7, 37, 14, 257, 0.9),
    (1, 129, 128, 14, 3000, 0.9),
    (3, 45, 77, 6, 3000, 0.9),
    (3, 9, 20, 14, 257, 0.7),
    (3, 16, 16, 6, 1, 0.7),
    (3, 7, 37, 1, 256, 0.7),
    (1, 129, 128, 6, 257, 0.7),
    (3, 45, 77, 14, 256, 0.7),
    (3, 16, 16, 6, 96, 0.8),
    (3, 36, 64, 6, 96, 0.8),
    (3, 9, 21, 1, 257, 0.6),
    (3, 17, 34, 14, 256, 0.85),
    (3, 45, 77, 6, 96, 1.0),
    (3, 16, 16, 1, 1, 1.0),
    (3, 9, 20, 14, 257, 1.0),
]


@pytest.mark.parametrize("N,H,W,bc,M,rate", PARITY_CASES)
def test_augment_entry_bit_exact(cuda, N, H, W, bc, M, rate):
    inp = _inputs(H * 131 + W + bc, N, H, W, bc, M, rate)
    got = _Call(cuda, inp, rate).run().results()
    _assert_bits(got, _oracle(inp, rate), what="%dx%d bc %d M %d rate %g" % (H, W, bc, M, rate))


@pytest.mark.parametrize("H,W,rate", [(45, 77, 0.9), (16, 16, 0.8), (9, 20, 0.7)])
def test_augment_inclusive_maximum_offsets(cuda, H, W, rate):
    """(h-H, w-W) is the last legal crop (tf.random_uniform never draws it, tf.slice accepts it); its bottom-right taps are the last
    source pixel."""
    inp = _inputs(11, 3, H, W, 6, 5, rate)
    h, w = O.aug_resized_hw(H, W, rate)
    inp["para"] = np.array([(h - H, w - W, 1), (0, 0, 0), (h - H, w - W, 0)], np.int32)
    _assert_bits(_Call(cuda, inp, rate).run().results(), _oracle(inp, rate), what="max offsets")


@pytest.mark.parametrize("H,W,rate", [(45, 77, 0.9), (16, 16, 0.8), (7, 37, 1.0)])
def test_augment_out_of_range_para_is_clamped(cuda, H, W, rate):
    """para is a device array the entry cannot inspect: offsets outside [0, h-H] x [0, w-W] give the result of the clamped offsets
    (and read nothing outside the inputs), flip is para != 0."""
    inp = _inputs(12, 3, H, W, 6, 5, rate)
    h, w = O.aug_resized_hw(H, W, rate)
    clamped = np.array([(0, 0, 1), (h - H, w - W, 0), (h - H, w - W, 1)], np.int32)
    want = _oracle(inp, rate, para=clamped)
    inp["para"] = clamped
    legal = _Call(cuda, inp, rate).run().results()
    _assert_bits(legal, want, what="clamped offsets")
    inp["para"] = np.array([(-5, -7, 2), (h, w, 0), (1 << 30, 1 << 30, -1)], np.int32)
    wild = _Call(cuda, inp, rate).run().results()
    _assert_bits(wild, legal, what="out-of-range offsets against clamped ones")
    inp["para"] = np.array([(-(1 << 31), 0x7FFFFFFF, -(1 << 31)), (0x7FFFFFFF, -(1 << 31), 0), (h - H + 1, w - W + 1, 0x7FFFFFFF)], np.int64).astype(np.int32)
    want2 = _oracle(inp, rate, para=np.array([(0, w - W, 1), (h - H, 0, 0), (h - H, w - W, 1)], np.int32))
    _assert_bits(_Call(cuda, inp, rate).run().results(), want2, what="extreme offsets")


def test_augment_pairs_device_resident_draws(cuda):
    """data.augment_pairs with para / jitter / Hs / counts already on the device (the training driver's form) equals the call with
    host arrays, and both equal the oracle: at a rate and size where a float32 rate would resize to another grid."""
    from stabnet_amd import data
    from stabnet_amd.config import Config
    N, H, W, bc, M, rate = 3, 36, 64, 6, 96, 0.8
    inp = _inputs(13, N, H, W, bc, M, rate)
    cfg = Config(height=H, width=W, before_ch=bc, max_matches=M, random_crop_rate=rate)
    d = lambda a: torch.from_numpy(a).to(cuda)
    host = data.augment_pairs(d(inp["stable"]), d(inp["unstable"]), d(inp["flow"]), d(inp["m1"]), inp["n1"], d(inp["m2"]), inp["n2"],
                              inp["para"], inp["jitter"], inp["Hs"], cfg)
    dev = data.augment_pairs(d(inp["stable"]), d(inp["unstable"]), d(inp["flow"]), d(inp["m1"]), d(inp["n1"]), d(inp["m2"]), d(inp["n2"]),
                             d(inp["para"]), d(inp["jitter"]), d(inp["Hs"]), cfg)
    want = _oracle(inp, rate)
    for k, a, b in zip(OUTS, host, dev):
        assert _same_bits(a.cpu().numpy(), want[k]), k
        assert _same_bits(b.cpu().numpy(), want[k]), k


def test_augment_without_flow_and_without_matches(cuda):
    N, H, W, bc, M, rate = 3, 7, 37, 6, 257, 0.9
    inp = _inputs(14, N, H, W, bc, M, rate)
    full = _Call(cuda, inp, rate).run().results()
    no_flow = _Call(cuda, inp, rate, with_flow=False)
    no_flow.outb["flow"] = Guarded(cuda, N * H * W * 2, init="canary")
    got = no_flow.run().results()
    _assert_bits(got, full, keys=[k for k in OUTS if k != "flow"], what="flow_in NULL")
    assert no_flow.outb["flow"].untouched(), "flow_out written although flow_in is NULL"
    no_m = _Call(cuda, inp, rate, with_matches=False)
    for k in ("fm1", "mk1", "fm2", "mk2"):
        no_m.outb[k] = Guarded(cuda, no_m.outb[k].n, init="canary")
    got = no_m.run().results()
    _assert_bits(got, full, keys=("x1", "y1", "x2", "y2", "flow"), what="matches1 NULL")
    for k in ("fm1", "mk1", "fm2", "mk2"):
        assert no_m.outb[k].untouched(), k + " written although matches1 is NULL"


@pytest.mark.parametrize("bc", [1, 6, 14])
def test_augment_constant_channels_known_answer(cuda, bc):
    """Independent of the oracle.  Input channel c is the constant -0.4 + c/64 (stable 0..2*bc+1, then the two unstable channels):
    the resize of a constant is the constant, its float64 sum is exact so the mean is the constant and the contrast step leaves it
    alone; what remains is clip(const + brightness) in the channel read_and_decode routes there (get_data_mini_after.py:243-248),
    and identity homographies on a 17x33 grid (steps 1/8 and 1/16, exact) mask nothing."""
    N, H, W, M, rate = 3, 17, 33, 4, 0.9
    inp = _inputs(15 + bc, N, H, W, bc, M, rate)
    nst = 2 * (bc + 1)
    const = (F32(-0.4) + np.arange(nst + 2, dtype=F32) / F32(64)).astype(F32)
    inp["stable"] = np.broadcast_to(const[:nst], (N, H, W, nst)).copy()
    inp["unstable"] = np.broadcast_to(const[nst:], (N, H, W, 2)).copy()
    inp["Hs"] = np.broadcast_to(np.eye(3, dtype=F32).reshape(9), (N, 2, bc, 9)).copy()
    inp["jitter"] = np.array([(0.5, 0.1), (1.5, -0.12), (1.25, 0.85)], F32)      # -0.12 clips channel 0 at -0.5, 0.85 channels 4.. at 0.5
    got = _Call(cuda, inp, rate).run().results()
    for n in range(N):
        val = np.clip((const + inp["jitter"][n, 1]).astype(F32), F32(-0.5), F32(0.5)).astype(F32)
        assert (np.abs(val) < 0.5).any() and (n == 0 or (val == (-0.5, 0.5)[n - 1]).any())     # both clip sides occur, and neither everywhere
        for tower, (x, y) in enumerate((("x1", "y1"), ("x2", "y2"))):
            c0 = tower * (bc + 1)
            want_x = np.concatenate([np.zeros(bc, F32), val[c0 + 1:c0 + 1 + bc], val[nst + tower:nst + tower + 1]])
            assert _same_bits(got[x][n], np.broadcast_to(want_x, (H, W, 2 * bc + 1))), (x, n)
            assert _same_bits(got[y][n], np.full((H, W, 1), val[c0], F32)), (y, n)


def test_augment_flow_closed_form_at_rate_one(cuda):
    """Independent of the oracle.  Rate 1.0: the resize is the identity and the only legal crop is (0, 0), so lines 40-47 of the
    reference reduce to flow_x' = -flip_lr(flow_x) - 1/W, flow_y' = flip_lr(flow_y) for a flipped sample and to the input for an
    unflipped one; on a 2^-8 grid every step but the last subtraction is exact."""
    N, H, W, bc, M, rate = 3, 9, 20, 1, 1, 1.0
    inp = _inputs(16, N, H, W, bc, M, rate)
    rng = np.random.default_rng(16)
    inp["flow"] = (rng.integers(-256, 257, (N, H, W, 2)) / 256.0).astype(F32)
    assert (inp["para"][:, :2] == 0).all() and list(inp["para"][:, 2]) == [1, 0, 1]
    got = _Call(cuda, inp, rate).run().results()["flow"]
    for n in range(N):
        f = inp["flow"][n]
        if inp["para"][n, 2]:
            want = np.stack([((f[:, ::-1, 0] * F32(-1)).astype(F32) - F32(1.0 / W)).astype(F32), f[:, ::-1, 1]], axis=2)
        else:
            want = f
        assert _same_bits(got[n], want), n


def test_augment_point_masks_at_the_frame_boundary(cuda):
    """Independent of the oracle.  Rate 1.0, W = 16: an unflipped coordinate maps to v = (p + 1) - 1, a flipped x to -v - 1/16.  Points
    chosen so that the mapped value is exactly -1 or +1 (in frame: the reference's test is >= -1 and <= 1), one ulp beyond either
    (out), or NaN (out)."""
    N, H, W, bc, rate = 2, 16, 16, 1, 1.0
    e = F32(2.0 ** -23)
    one_up, m_one_dn = np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2))
    # (input value, mapped value, in frame) for an unflipped coordinate ...
    plain = [(F32(-1), F32(-1), True), (F32(1), F32(1), True), (m_one_dn, m_one_dn, False), (F32(1) + 2 * e, F32(1) + 2 * e, False),
             (one_up, F32(1), True),                       # 1 + 2^-23 + 1 rounds to 2: the reference keeps this point too
             (F32(np.nan), F32(np.nan), False), (F32(0.25), F32(0.25), True)]
    # ... and for a flipped x coordinate
    flipped = [(F32(-1.0625), F32(1), True), (F32(-1.0625) - e, one_up, False), (F32(0.9375), F32(-1), True),
               (F32(0.9375) + e, m_one_dn, False), (F32(np.nan), F32(np.nan), False), (F32(0.25), F32(-0.3125), True)]
    rows, want_pts, want_ok = [[], []], [[], []], [[], []]
    for n, xs in enumerate((flipped, plain)):                                       # sample 0 is flipped, sample 1 is not
        for k in range(4):
            for (p, v, ok) in (xs if k % 2 == 0 else plain):
                src, dst = np.zeros(4, F32), np.zeros(4, F32)
                if n == 0:
                    dst[0] = dst[2] = F32(-0.0625)                                  # a zero x, flipped
                src[k], dst[k] = p, v
                rows[n].append(src); want_pts[n].append(dst); want_ok[n].append(ok)
    M = max(len(rows[0]), len(rows[1]))
    inp = _inputs(17, N, H, W, bc, M, rate, flips=(1, 0), counts=([M, M], [M, 0]))
    for n in range(N):
        pad = M - len(rows[n])
        fill_dst = np.array([-0.0625, 0, -0.0625, 0], F32) if n == 0 else np.zeros(4, F32)
        inp["m1"][n] = np.stack(rows[n] + [np.zeros(4, F32)] * pad)
        want_pts[n] = np.stack(want_pts[n] + [fill_dst] * pad)
        want_ok[n] = np.array(want_ok[n] + [True] * pad)
    inp["m2"] = inp["m1"].copy()
    got = _Call(cuda, inp, rate).run().results()
    for n in range(N):
        _assert_bits({"fm1": got["fm1"][n], "fm2": got["fm2"][n]}, {"fm1": want_pts[n], "fm2": want_pts[n]}, keys=("fm1", "fm2"),
                     what="sample %d" % n, nan_is_nan=True)
        assert np.array_equal(got["mk1"][n], want_ok[n].astype(F32)), n
        assert np.array_equal(got["mk2"][n], want_ok[n].astype(F32) if n == 0 else np.zeros(M, F32)), n     # count 0 masks every point
    _assert_bits(got, _oracle(inp, rate), what="boundary points", nan_is_nan=True)


def test_augment_homography_masks_at_the_boundary(cuda):
    """Independent of the oracle.  On a 9x17 frame the grid (steps 1/4 and 1/8) is exact; hand-built homographies put u or v exactly
    on +-1 (not black: the reference's test is strict) or one ulp beyond (black).  Black pixels read 1 in the mask channel and -1 in
    the frame channel."""
    N, H, W, bc, M, rate = 1, 9, 17, 6, 1, 0.9
    inp = _inputs(18, N, H, W, bc, M, rate, flips=(0,))
    e = 2.0 ** -23
    I = np.eye(3)
    def shift(bx=0.0, by=0.0, s=1.0):
        m = I.copy(); m[0, 2], m[1, 2] = bx, by
        return (m * s).astype(F32).reshape(9)
    none, lastc, firstc, lastr, firstr = "none", "last column", "first column", "last row", "first row"
    towers = [[(shift(), none), (shift(bx=e), lastc), (shift(bx=-e), firstc), (shift(by=e), lastr), (shift(by=-e), firstr), (shift(s=2.0), none)],
              [(shift(bx=e, by=e), lastc + lastr), (shift(bx=-e, by=-e), firstc + firstr), (shift(bx=e, s=2.0), lastc),
               (shift(by=-e, s=0.5), firstr), (shift(bx=e / 2), none), (shift(by=-e / 2), none)]]
    # +-2^-24 does not move +-1 (1 + 2^-24 rounds to even, back to 1; -1 + 2^-24 is inside): no pixel is black
    for t in range(2):
        for k in range(bc):
            inp["Hs"][0, t, k] = towers[t][k][0]
    got = _Call(cuda, inp, rate).run().results()
    for t, x in enumerate(("x1", "x2")):
        for k in range(bc):
            what = towers[t][k][1]
            want = np.zeros((H, W), F32)
            if "last column" in what: want[:, -1] = 1
            if "first column" in what: want[:, 0] = 1
            if "last row" in what: want[-1, :] = 1
            if "first row" in what: want[0, :] = 1
            assert np.array_equal(got[x][0, ..., k], want), (x, k, what)
            assert (got[x][0, ..., bc + k][want == 1] == -1).all() and (got[x][0, ..., bc + k][want == 0] >= -0.5).all(), (x, k)
    _assert_bits(got, _oracle(inp, rate), what="boundary masks")


@pytest.mark.parametrize("what,kw", [
    ("workspace one byte short", {"ws_bytes": -1}),
    ("stable offset by 4 bytes", {"stable_shift": 4}),
    ("before_ch 0", {"bc": 0}),
    ("before_ch 15", {"bc": 15}),
    ("rate 0", {"rate": 0.0}),
    ("rate 1.5", {"rate": 1.5}),
    ("rate NaN", {"rate": float("nan")}),
    ("H 1", {"H": 1}),
    ("flow_in without flow_out", {"null": ("flow",)}),
    ("matches without a mask output", {"null": ("mk2",)}),
])
def test_augment_error_paths_launch_nothing(cuda, what, kw):
    from stabnet_amd import _lib
    N, H, W, bc, M, rate = 2, 9, 20, 6, 4, 0.9
    inp = _inputs(19, N, H, W, 15, M, rate)                      # buffers as large as the largest thing the entry is told
    c = _Call(cuda, inp, rate, out_init="canary", ws_init="canary")
    kw = dict({"bc": bc}, **kw)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = int(_lib.lib().stabnet_augment_workspace_bytes(N, H, W, bc)) - 1
    with pytest.raises(_lib.StabnetError) as err:
        c.run(**kw)
    msg = str(err.value)
    assert "stabnet_augment_pairs failed" in msg and "augment" in msg.split(":", 1)[1], msg
    torch.cuda.synchronize()
    for k, b in c.outb.items():
        assert b.untouched(), what + ": wrote " + k
    assert c.ws.untouched(), what + ": wrote the workspace"


def test_augment_is_deterministic_on_poisoned_workspaces(cuda):
    N, H, W, bc, M, rate = 3, 45, 77, 6, 257, 0.9
    inp = _inputs(20, N, H, W, bc, M, rate)
    a = _Call(cuda, inp, rate).run().results()                                  # NaN workspace
    b = _Call(cuda, inp, rate, ws_init="canary").run().results()                # canary-word workspace
    c2 = _Call(cuda, inp, rate)
    c2.run()
    c = c2.run().results()                                                      # a second call on a used workspace
    _assert_bits(b, a, what="second workspace")
    _assert_bits(c, a, what="reused workspace")


def test_augment_graph_capture_and_replay(cuda):
    N, H, W, bc, M, rate = 3, 16, 16, 6, 257, 0.8
    inp = _inputs(21, N, H, W, bc, M, rate)
    eager = _Call(cuda, inp, rate).run().results()
    c = _Call(cuda, inp, rate)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.run()                                                                 # stream_ptr() is the capturing stream here
    for b in c.outb.values():
        b.t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    _assert_bits(c.results(), eager, what="graph replay")
    _assert_bits(eager, _oracle(inp, rate), what="eager")


@pytest.mark.parametrize("N,H,W,bc", [(2, 45, 77, 6), (1, 129, 128, 1)])
def test_augment_mean_follows_the_documented_summation_order(cuda, N, H, W, bc):
    """On ordinary frames any float64 summation order rounds to the same float32 mean.  Here it does not: every channel holds as many
    +2^30 as -2^30 pixels among small ones, so a float64 partial sum near 2^30 drops the small pixels' bits below 2^-23 and the mean
    depends on which pixels met in which order (np.mean's pairwise order gives other bits: checked below).  Rate 1.0 passes the pixels
    through unchanged; the output must still equal the model of the documented order bit for bit, in the pixels that do not clip."""
    M, rate = 1, 1.0
    inp = _inputs(22, N, H, W, bc, M, rate)
    rng = np.random.default_rng(22)
    for key in ("stable", "unstable"):
        a = inp[key]
        a *= F32(0.5)                                           # |x| <= 0.25: x - mean + mean stays inside the clip
        for n in range(N):
            for c in range(a.shape[3]):
                pos = rng.choice(H * W, 2 * (H * W // 8), replace=False)
                plane = a[n, ..., c].reshape(-1)
                plane[pos[0::2]], plane[pos[1::2]] = F32(2.0 ** 30), F32(-(2.0 ** 30))
                a[n, ..., c] = plane.reshape(H, W)
    inp["jitter"][:, 0], inp["jitter"][:, 1] = F32(1.0), F32(0.0)                # contrast 1: (x - mean) + mean shows the mean's last bits
    planes = [inp["stable"][n, ..., c] for n in range(N) for c in range(2 * (bc + 1))]
    moved = sum(kernel_channel_mean(p) != F32(p.astype(np.float64).mean()) for p in planes)
    assert moved >= len(planes) // 2, "this input does not tell the summation orders apart"
    got = _Call(cuda, inp, rate).run().results()
    _assert_bits(got, _oracle(inp, rate), what="order-sensitive planes")
    assert (np.abs(got["y1"]) < 0.5).mean() > 0.5
