"""GPU: csrc/tvl1.hip against tests/tvl1_model.py, BIT FOR BIT (the uint32 images of the float32 results are compared): every stage
entry point alone, the stepwise and the fused iteration, the whole solve and a captured graph of it.  Sizes: a single level, odd
sizes with two levels, a multi-tile size, one narrower than the fused kernel's halo and one that is one pixel over the fused tile in
each direction; contiguous input and pixel stride 14 (a channel of an NHWC tensor)."""
import functools

import numpy as np
import pytest

import tvl1_model as M

pytestmark = pytest.mark.gpu
F = np.float32


def _geometry():
    from stabnet_amd import flow
    return flow.fused_geometry()


def _sizes():
    K, TX, TY = _geometry()
    return [(1, 16, 16), (2, 37, 53), (3, 72, 96), (2, 11, K - 1), (1, TY + 1, TX + 1)]


SIZE_IDS = ["1x16x16", "2x37x53", "3x72x96", "narrower_than_halo", "tile_plus_one"]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%d of %d values differ, first at %s: got %r, want %r (max abs diff %g)" % (
        bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0], np.nanmax(np.abs(got - want)))


def images(B, H, W, seed):
    """[B,H,W] float32 on the 0..255 scale: a smooth texture plus noise, so that gradients of every size occur."""
    rng = np.random.default_rng(seed)
    return np.stack([(M.texture(H, W, seed + b) * 200 + rng.uniform(0, 55, (H, W))).astype(F) for b in range(B)])


def on_device(cuda, a, stride):
    """a [B,H,W] -> (tensor that owns the memory, [B,H,W] view with pixel stride `stride`)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    if stride == 1:
        return t, t
    full = torch.rand(a.shape + (stride,), device=cuda) * 255
    full[..., 3] = t
    return full, full[..., 3]


def call(name, *args):
    import torch
    from stabnet_amd import _lib
    _lib.call(name, *args, device=torch.device("cuda:0"))


def ptr(t):
    return t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("stride", [1, 14])
@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_pyramid_down(cuda, size, stride):
    import torch
    B, H, W = _sizes()[size]
    a = images(B, H, W, 10 + size)
    own, v = on_device(cuda, a, stride)
    out = torch.full((B, (H + 1) // 2, (W + 1) // 2), -7.0, device=cuda)
    call("stabnet_tvl1_pyramid_down", ptr(v), stride, B, H, W, ptr(out), stream(), 0)
    same_bits(out.cpu().numpy(), np.stack([M.pyramid_down(x) for x in a]))


@pytest.mark.parametrize("stride", [1, 14])
@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_gradient(cuda, size, stride):
    import torch
    B, H, W = _sizes()[size]
    a = images(B, H, W, 20 + size)
    own, v = on_device(cuda, a, stride)
    gx, gy = torch.full((B, H, W), -7.0, device=cuda), torch.full((B, H, W), -7.0, device=cuda)
    call("stabnet_tvl1_gradient", ptr(v), stride, B, H, W, ptr(gx), ptr(gy), stream(), 0)
    want = [M.gradient(x) for x in a]
    same_bits(gx.cpu().numpy(), np.stack([w[0] for w in want]))
    same_bits(gy.cpu().numpy(), np.stack([w[1] for w in want]))


@pytest.mark.parametrize("stride", [1, 14])
@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_warp_and_constants(cuda, size, stride):
    import torch
    B, H, W = _sizes()[size]
    rng = np.random.default_rng(30 + size)
    i0, i1 = images(B, H, W, 31 + size), images(B, H, W, 37 + size)
    u = rng.normal(0, 3, (2, B, H, W)).astype(F)                 # up to ~10 px: many samples leave the image and are clamped
    u[:, :, ::5, ::7] = 0                                       # and some sit exactly on pixel centres
    g = [M.gradient(x) for x in i1]
    gx, gy = np.stack([a[0] for a in g]), np.stack([a[1] for a in g])
    own0, v0 = on_device(cuda, i0, stride)
    own1, v1 = on_device(cuda, i1, stride)
    dgx, dgy, du = (torch.from_numpy(a).to(cuda) for a in (gx, gy, u))
    cst = torch.full((4, B, H, W), -7.0, device=cuda)
    call("stabnet_tvl1_warp", ptr(v0), ptr(v1), stride, ptr(dgx), ptr(dgy), ptr(du), ptr(cst), B, H, W, stream(), 0)
    want = [M.warp_constants(i0[b], i1[b], gx[b], gy[b], u[0, b], u[1, b]) for b in range(B)]
    got = cst.cpu().numpy()
    for k, name in enumerate(("Ix", "Iy", "rc", "g")):
        same_bits(got[k], np.stack([w[k] for w in want]))


@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_upsample(cuda, size):
    import torch
    B, H, W = _sizes()[size]
    h, w = (H + 1) // 2, (W + 1) // 2
    u = np.random.default_rng(40 + size).normal(0, 2, (2, B, h, w)).astype(F)
    out = torch.full((2, B, H, W), -7.0, device=cuda)
    du = torch.from_numpy(u).to(cuda)
    call("stabnet_tvl1_upsample", ptr(du), B, h, w, ptr(out), H, W, stream(), 0)
    same_bits(out.cpu().numpy(), np.stack([[M.upsample(u[c, b], H, W) for b in range(B)] for c in range(2)]))


@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_flow_to_map(cuda, size):
    import torch
    B, H, W = _sizes()[size]
    u = np.random.default_rng(50 + size).normal(0, 4, (2, B, H, W)).astype(F)
    uv, mp = torch.full((B, H, W, 2), -7.0, device=cuda), torch.full((B, H, W, 2), -7.0, device=cuda)
    du = torch.from_numpy(u).to(cuda)
    call("stabnet_tvl1_flow_to_map", ptr(du), B, H, W, ptr(uv), ptr(mp), stream(), 0)
    same_bits(uv.cpu().numpy(), np.stack([u[0], u[1]], axis=-1))
    same_bits(mp.cpu().numpy(), np.stack([M.flow_to_map(u[0, b], u[1, b]) for b in range(B)]))


# ---- the iteration ------------------------------------------------------------------------------------------------------------------

PARAMS = dict(tau=0.25, lam=0.15, theta=0.3)


@functools.lru_cache(maxsize=None)
def iteration_case(size):
    """A random, nonzero starting state (a wrong halo shows) and constants that reach every branch of the factor f."""
    B, H, W = _sizes()[size]
    rng = np.random.default_rng(60 + size)
    state = np.concatenate([rng.normal(0, 1, (2, B, H, W)), rng.uniform(-0.5, 0.5, (4, B, H, W))]).astype(F)
    ix, iy = rng.normal(0, 5, (B, H, W)).astype(F), rng.normal(0, 5, (B, H, W)).astype(F)
    flat = rng.random((B, H, W)) < 0.1
    ix[flat] = 0
    iy[flat] = 0                                                 # g = 0: f = 0 unless rho is not 0
    rc = rng.normal(0, 10, (B, H, W)).astype(F)
    rc[rng.random((B, H, W)) < 0.05] = 0
    consts = np.stack([ix, iy, rc, ix * ix + iy * iy]).astype(F)
    for a in (state, consts):
        a.setflags(write=False)
    return state, consts


@functools.lru_cache(maxsize=None)
def model_iterations(size, n):
    state, consts = iteration_case(size)
    B = state.shape[1]
    per = [M.iterate(state[:, b], consts[:, b], n, **PARAMS) for b in range(B)]
    return np.stack([np.stack([p[k] for p in per]) for k in range(6)])


def device_iterations(cuda, size, n, fused):
    import torch
    state, consts = iteration_case(size)
    _, B, H, W = state.shape
    s, c = torch.from_numpy(state.copy()).to(cuda), torch.from_numpy(consts.copy()).to(cuda)
    scratch = torch.full_like(s, float("nan"))
    call("stabnet_tvl1_iterate", ptr(s), ptr(scratch), ptr(c), B, H, W, PARAMS["tau"], PARAMS["lam"], PARAMS["theta"], n, int(fused),
         stream(), 0)
    assert np.array_equal(c.cpu().numpy(), consts)
    return s.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 30])
@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_stepwise_iteration_is_the_model(cuda, size, n):
    same_bits(device_iterations(cuda, size, n, fused=False), model_iterations(size, n))


@pytest.mark.parametrize("which", range(5), ids=["1", "K-1", "K", "K+1", "30"])
@pytest.mark.parametrize("size", range(5), ids=SIZE_IDS)
def test_fused_iteration_is_the_stepwise_one(cuda, size, which):
    K = _geometry()[0]
    assert K >= 4
    n = [1, K - 1, K, K + 1, 30][which]
    same_bits(device_iterations(cuda, size, n, fused=True), device_iterations(cuda, size, n, fused=False))


# ---- the whole solve ----------------------------------------------------------------------------------------------------------------

SOLVE_SIZES = [(1, 16, 16), (2, 37, 53), (3, 72, 96)]
MOTIONS = [(1, 0, 0, 1, 1.3, -0.8), (1.01, 0.01, -0.01, 0.99, 2.5, 1.5), (1, 0, 0, 1, -3.3, 2.1)]


@functools.lru_cache(maxsize=None)
def solve_case(size, quick):
    B, H, W = SOLVE_SIZES[size]
    pairs = [M.make_pair(H, W, 70 + b, MOTIONS[b]) for b in range(B)]
    i0, i1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    kw = dict(scales=1, warps=1, iters=1) if quick else {}
    uv = [M.solve(i0[b], i1[b], **kw) for b in range(B)]
    want_uv = np.stack([np.stack(x, axis=-1) for x in uv])
    want_map = np.stack([M.flow_to_map(*x) for x in uv])
    for a in (i0, i1, want_uv, want_map):
        a.setflags(write=False)
    return i0, i1, want_uv, want_map


def _params(quick):
    from stabnet_amd.flow import Tvl1Params
    return Tvl1Params(scales=1, warps=1, iters=1) if quick else Tvl1Params()


@pytest.mark.parametrize("quick", [False, True], ids=["defaults", "one_iteration"])
@pytest.mark.parametrize("size", range(3), ids=SIZE_IDS[:3])
def test_whole_solve(cuda, size, quick):
    import torch
    from stabnet_amd import flow
    i0, i1, want_uv, want_map = solve_case(size, quick)
    a, b = torch.from_numpy(i0.copy()).to(cuda), torch.from_numpy(i1.copy()).to(cuda)
    same_bits(flow.tvl1_flow(a, b, _params(quick), out="uv").cpu().numpy(), want_uv)
    same_bits(flow.tvl1_flow(a, b, _params(quick), out="map").cpu().numpy(), want_map)


def test_whole_solve_reads_nhwc_channels_in_place(cuda, monkeypatch):
    """Channels 0 and 7 of a [B,H,W,14] tensor on get_img's scale (grey / 255 - 0.5), brought to 0..255 by the solve's own
    (v + 0.5) * 255; and the stepwise leg (STABNET_TVL1_FUSED=0) gives the bits of the fused one."""
    import torch
    from stabnet_amd import flow
    i0, i1, _, _ = solve_case(1, False)
    v0, v1 = (i0 / F(255) - F(0.5)).astype(F), (i1 / F(255) - F(0.5)).astype(F)
    B, H, W = v0.shape
    full = torch.rand((B, H, W, 14), device=cuda)
    full[..., 0], full[..., 7] = torch.from_numpy(v0).to(cuda), torch.from_numpy(v1).to(cuda)
    before = full.clone()
    got = flow.tvl1_flow(full[..., 0], full[..., 7], out="uv", offset=0.5, scale=255.0)
    assert torch.equal(full, before)
    w0, w1 = (v0 + F(0.5)) * F(255), (v1 + F(0.5)) * F(255)
    same_bits(got.cpu().numpy(), np.stack([np.stack(M.solve(w0[b], w1[b]), axis=-1) for b in range(B)]))
    monkeypatch.setenv("STABNET_TVL1_FUSED", "0")
    assert torch.equal(flow.tvl1_flow(full[..., 0], full[..., 7], out="uv", offset=0.5, scale=255.0), got)


def test_graph_capture(cuda):
    """Captured on one stream and replayed twice: the eager call's bits, from the workspace the caller gave."""
    import torch
    from stabnet_amd import flow
    i0, i1, want_uv, _ = solve_case(1, False)
    B, H, W = i0.shape
    a, b = torch.from_numpy(i0.copy()).to(cuda), torch.from_numpy(i1.copy()).to(cuda)
    ws = torch.empty(flow.workspace_bytes(B, H, W), dtype=torch.uint8, device=cuda)
    where = ws.data_ptr()
    eager = flow.tvl1_flow(a, b, out="uv", workspace=ws).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = flow.tvl1_flow(a, b, out="uv", workspace=ws)
    for _ in range(2):
        out.fill_(-7.0)
        ws.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert ws.data_ptr() == where
    same_bits(eager.cpu().numpy(), want_uv)


def test_python_argument_checks(cuda):
    import torch
    from stabnet_amd import flow
    from stabnet_amd._lib import StabnetError
    a = torch.zeros((1, 16, 16), device=cuda)
    for bad, word in ((a.cpu(), "GPU"), (a.double(), "float32"), (a[0], "[B,H,W]"), (a.transpose(1, 2), "strides")):
        with pytest.raises(StabnetError, match=word.replace("[", r"\[")):
            flow.tvl1_flow(bad, a)
    with pytest.raises(StabnetError, match="agree"):
        flow.tvl1_flow(a, torch.zeros((1, 16, 24), device=cuda))
    with pytest.raises(StabnetError, match="workspace"):
        flow.tvl1_flow(a, a, workspace=torch.empty(16, dtype=torch.uint8, device=cuda))
    with pytest.raises(StabnetError, match="out must be"):
        flow.tvl1_flow(a, a, out="flow")
    with pytest.raises(StabnetError, match="8 or more"):
        flow.tvl1_flow(a[:, :4], a[:, :4])
