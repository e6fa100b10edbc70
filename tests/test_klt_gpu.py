"""GPU: csrc/klt.hip against tests/klt_model.py, BIT FOR BIT (the uint32 images of the float32 results are compared): the response
plane, detection, tracking, the whole solve and a captured graph of it.  Sizes: the smallest legal one (a single pixel has a
response; one level), odd sizes with partial cells at both edges and two levels, three levels and 30 cells, many cells in a row;
an image textured only in its border band (no match), a pair moved by a third of its width (points leave the image and are lost),
and cell = 8 with max_matches = 16 (truncation).  Contiguous input and pixel strides 14 / 2 (channels of NHWC tensors), values on
the 0..255 scale and on get_img's scale with offset 0.5 and scale 255."""
import functools

import numpy as np
import pytest

import klt_model as K
import tvl1_model as M

pytestmark = pytest.mark.gpu
F = np.float32

SIZES = [(1, 17, 17), (2, 37, 53), (3, 72, 96), (1, 40, 200)]
SIZE_IDS = ["1x17x17", "2x37x53", "3x72x96", "1x40x200"]
MOTIONS = [(1, 0, 0, 1, 1.3, -0.8), (1.01, 0.01, -0.01, 0.99, 2.5, 1.5), (1, 0, 0, 1, -3.3, 2.1)]
READS = [(1, 1, 0.0, 1.0), (14, 2, 0.5, 255.0), (1, 1, 0.5, 255.0), (14, 2, 0.0, 1.0)]       # stride of i0, of i1, offset, scale
READ_IDS = ["dense_255", "nhwc_getimg", "dense_getimg", "nhwc_255"]
MAXM = 64


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d of %d values differ, first at %s: got %r, want %r (max abs diff %g)" % (
        bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0], np.nanmax(np.abs(got - want)))


def pair(B, H, W, seed, motions=MOTIONS):
    """i0, i1 [B,H,W] float32 on the 0..255 scale: a moved texture plus noise of its own in either image."""
    rng = np.random.default_rng(seed)
    i0, i1 = [], []
    for b in range(B):
        a, c, _, _ = M.make_pair(H, W, seed + b, motions[b % len(motions)])
        i0.append((a * F(0.9) + rng.uniform(0, 12, (H, W))).astype(F))
        i1.append((c * F(0.9) + rng.uniform(0, 12, (H, W))).astype(F))
    return np.stack(i0), np.stack(i1)


def border_only(H, W, seed):
    """Flat but for the outermost 5 pixels: no box of a pixel 8 or more from the edge (r = 2, gradient 1 more) reaches them."""
    t = (M.texture(H, W, seed) * 255).astype(F)
    a = np.full((H, W), 100, F)
    for s in (np.s_[:5, :], np.s_[-5:, :], np.s_[:, :5], np.s_[:, -5:]):
        a[s] = t[s]
    return a[None]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """case: an index into SIZES, or a name -> (i0, i1, model parameters, max_matches)."""
    if case == "border_band":
        a = border_only(40, 56, 3)
        return a, np.roll(a, 1, axis=2).copy(), {}, MAXM
    if case == "third_of_the_width":
        i0, i1 = pair(2, 48, 96, 90, [(1, 0, 0, 1, 32, 0), (1, 0, 0, 1, -30, 4)])
        return i0, i1, {}, MAXM
    if case == "truncation":
        i0, i1 = pair(*SIZES[2], 80)
        return i0, i1, dict(cell=8), 16
    if case == "one_cell":
        i0, i1 = pair(*SIZES[0], 60)
        return i0, i1, dict(cell=17), MAXM
    i0, i1 = pair(*SIZES[case], 60 + case)
    return i0, i1, {}, MAXM


@functools.lru_cache(maxsize=None)
def model(case, getimg):
    """What the device is given (v0, v1) and every stage of the model on what the solve reads from it."""
    i0, i1, kw, maxm = inputs(case)
    if getimg:
        v0, v1 = (i0 / F(255) - F(0.5)).astype(F), (i1 / F(255) - F(0.5)).astype(F)
        w0, w1 = (v0 + F(0.5)) * F(255), (v1 + F(0.5)) * F(255)
    else:
        v0, v1, w0, w1 = i0, i1, i0, i1
    B = len(i0)
    out = [K.matches(w0[b], w1[b], maxm, stages=True, **kw) for b in range(B)]
    res = {"v0": v0, "v1": v1, "w0": w0, "w1": w1, "kw": kw, "maxm": maxm,
           "rows": np.stack([o[0] for o in out]), "n": np.array([o[1] for o in out], np.int32),
           "cand": np.stack([o[2] for o in out]), "trk": np.stack([o[3] for o in out])}
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def on_device(cuda, a, stride, channel):
    """a [B,H,W] -> (tensor that owns the memory, [B,H,W] view with pixel stride `stride`)."""
    import torch
    t = torch.from_numpy(np.array(a, F)).to(cuda)
    if stride == 1:
        return t, t
    full = torch.rand(a.shape + (stride,), device=cuda) * 255
    full[..., channel] = t
    return full, full[..., channel]


def params(kw):
    from stabnet_amd.features import KltParams
    return KltParams(**kw)


def device_inputs(cuda, case, read):
    s0, s1, off, scl = READS[read]
    m = model(case, off != 0.0)
    own0, a = on_device(cuda, m["v0"], s0, 3)
    own1, b = on_device(cuda, m["v1"], s1, 1)
    return m, (own0, own1), a, b, dict(offset=off, scale=scl)


CASES = list(range(len(SIZES))) + ["one_cell", "border_band", "third_of_the_width", "truncation"]
CASE_IDS = SIZE_IDS + ["one_cell", "border_band", "third_of_the_width", "truncation"]


@pytest.mark.parametrize("read", range(4), ids=READ_IDS)
@pytest.mark.parametrize("case", CASES[:4] + ["border_band"], ids=CASE_IDS[:4] + ["border_band"])
def test_response(cuda, case, read):
    from stabnet_amd import features
    m, own, a, b, aff = device_inputs(cuda, case, read)
    got = features.klt_response(a, params(m["kw"]), **aff).cpu().numpy()
    same_bits(got, np.stack([K.response(x) for x in m["w0"]]))


@pytest.mark.parametrize("read", range(4), ids=READ_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_detection(cuda, case, read):
    from stabnet_amd import features
    m, own, a, b, aff = device_inputs(cuda, case, read)
    got = features.klt_detect(a, params(m["kw"]), **aff).cpu().numpy()
    same_bits(got, m["cand"])
    if case == "border_band":
        assert not got[..., 2:].any()
    elif case != 0 and case != "one_cell":
        assert got[..., 3].sum() >= 0.5 * got[..., 3].size


@pytest.mark.parametrize("read", range(4), ids=READ_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tracking(cuda, case, read):
    """The candidates themselves, the same points off the pixel grid, and points outside the image (lost)."""
    import torch
    from stabnet_amd import features
    m, own, a, b, aff = device_inputs(cuda, case, read)
    B, H, W = m["v0"].shape
    c = m["cand"][:, :, :2]
    outside = np.broadcast_to(np.array([[-3.0, 5.0], [W + 2.0, H - 1.0], [W / 2, H + 40.0]], F), (B, 3, 2))
    pts = np.ascontiguousarray(np.concatenate([c, c + np.array([0.37, -0.61], F), outside], axis=1), F)
    p0 = [K.pyramid(x) for x in m["w0"]]
    p1 = [K.pyramid(x) for x in m["w1"]]
    want = np.stack([K.track(p0[i], p1[i], pts[i]) for i in range(B)])
    got = features.klt_track(a, b, torch.from_numpy(pts).to(cuda), params(m["kw"]), **aff).cpu().numpy()
    same_bits(got, want)
    same_bits(got[:, :c.shape[1]], m["trk"])
    assert (got[:, -3:, 2] == 1).all() and not got[:, -3:, [0, 1, 3]].any()
    if case == "third_of_the_width":
        lost = m["trk"][..., 2].sum()
        assert 0 < lost < m["trk"][..., 2].size, lost                        # some points leave the image, some stay


@pytest.mark.parametrize("read", range(4), ids=READ_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_whole_solve(cuda, case, read):
    import torch
    from stabnet_amd import features
    m, own, a, b, aff = device_inputs(cuda, case, read)
    before = [t.clone() for t in own]
    rows, n = features.klt_matches(a, b, m["maxm"], params(m["kw"]), **aff)
    assert n.dtype == torch.int32 and n.device == a.device and rows.shape == (len(m["n"]), m["maxm"], 4)
    assert all(torch.equal(t, u) for t, u in zip(own, before))               # read in place, nothing written
    assert np.array_equal(n.cpu().numpy(), m["n"]), (n.cpu().numpy(), m["n"])
    same_bits(rows.cpu().numpy(), m["rows"])
    for i, k in enumerate(m["n"]):
        assert not rows[i, int(k):].any()
    if case == "border_band":
        assert not m["n"].any()
    elif case == "truncation":
        valid = (m["cand"][..., 3] != 0) & (m["trk"][..., 2] == 0) & (m["trk"][..., 3] <= 0.25)
        assert (valid.sum(axis=1) > 15).all() and (m["n"] == 15).all()
    elif case not in (0, "one_cell", "third_of_the_width"):
        assert (m["n"] > 0).all()


def test_graph_capture(cuda):
    """Captured on one stream and replayed twice: the eager call's bits, from the workspace the caller gave."""
    import torch
    from stabnet_amd import features
    m, own, a, b, aff = device_inputs(cuda, 1, 1)
    B, H, W = a.shape
    ws = torch.empty(features.workspace_bytes(B, H, W), dtype=torch.uint8, device=cuda)
    where = ws.data_ptr()
    rows, n = features.klt_matches(a, b, MAXM, workspace=ws, **aff)
    rows, n = rows.clone(), n.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r2, n2 = features.klt_matches(a, b, MAXM, workspace=ws, **aff)
    for _ in range(2):
        r2.fill_(-7.0)
        n2.fill_(-7)
        ws.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(r2, rows) and torch.equal(n2, n)
    assert ws.data_ptr() == where
    same_bits(rows.cpu().numpy(), m["rows"])


def test_python_argument_checks(cuda):
    import torch
    from stabnet_amd import features
    from stabnet_amd._lib import StabnetError
    a = torch.zeros((1, 17, 17), device=cuda)
    for bad, word in ((a.cpu(), "GPU"), (a.double(), "float32"), (a[0], "[B,H,W]"), (a.transpose(1, 2), "strides")):
        with pytest.raises(StabnetError, match=word.replace("[", r"\[")):
            features.klt_matches(bad, a, 8)
    with pytest.raises(StabnetError, match="agree"):
        features.klt_matches(a, torch.zeros((1, 17, 24), device=cuda), 8)
    with pytest.raises(StabnetError, match="workspace"):
        features.klt_matches(a, a, 8, workspace=torch.empty(16, dtype=torch.uint8, device=cuda))
    with pytest.raises(StabnetError, match="max_matches"):
        features.klt_matches(a, a, 1)
    with pytest.raises(StabnetError, match="2 \\* border \\+ 1"):
        features.klt_matches(a[:, :16], a[:, :16], 8)
    with pytest.raises(StabnetError, match="window radius"):
        features.klt_matches(a, a, 8, features.KltParams(R=8))
    with pytest.raises(StabnetError, match="pts"):
        features.klt_track(a, a, torch.zeros((2, 3, 2), device=cuda))
    rows, n = features.klt_matches(a, a, 8)                                  # a flat image: no match, all rows zero
    assert int(n[0]) == 0 and not rows.any()
