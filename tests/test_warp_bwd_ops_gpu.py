"""GPU: every kernel of csrc/warp_bwd.hip on its own against a float64 reference of the same operation (oracle/torch_ref.py autograd, or
plain NumPy for the elementwise ones), one loss term / one input at a time, so that a small term cannot hide behind a large one, at the
grids, sizes and call forms that the training step uses and tests/test_warp_bwd_gpu.py does not reach:
  A  mesh_losses alone: distortion / consistency / id gradient each relative to ITS OWN maximum, grids other than 4x4, N > 8,
     a vertex on the clip, a saturated one, a zero theta;
  B  transformer_bwd alone with pts2 as the leaf: d_out / dense maps / signed counts x dmap_scale, the uniform-wave branch,
     more than 16 cells, gh != gw;
  C  interp_bwd: tiled against untiled bit for bit (one child process), taps on and past the window halo, accumulate, zeros in d_out;
  D  masked MSE: 1 .. 1 049 353 elements per sample (one block, 65 and 72 partials, the capped grid), an all-black sample, accumulate;
  E  feature loss: 1 .. 7000 matches (the three-per-thread unroll, its clamp and masked tail, a third round), exact counts.
The measured error of each check is printed before it is asserted (pytest -s shows it)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import stabnet_oracle as O
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relmax(got, want):
    """max |got - want| relative to max |want|."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / (np.abs(want).max() + 1e-300))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ===================================================================================================================================
# A. mesh_losses alone, one term at a time
# (gh, gw, N): the production batch (second sample round, 2 of 8 live) / 9 / another aspect, few second differences / 81 vertices and
# 64 cells: three lane rounds / gh != gw with N > 8 / no vertical consistency term
MESH_GRIDS = [(4, 4, 10), (4, 4, 9), (2, 3, 2), (8, 8, 2), (3, 8, 9), (1, 4, 2)]
# (w_id, w_dist, w_cons): one weight at a time, then the production ratios (theta_mul + grid_theta_mul, distortion_mul, consistency_mul)
MESH_TERMS = {"dist": (0.0, 1.0, 0.0), "cons": (0.0, 0.0, 20.0), "id": (0.16, 0.0, 0.0), "all": (0.16, 1.0, 20.0)}
# Bar: the gradient of a vertex is a sum of a few dozen float32 products; the float32 evaluation of the same torch graph differs from the
# float64 one by 2e-8 .. 5e-8 of the gradient maximum on these grids.  1e-5 is 200 x that and three orders below a wrong coefficient.
# Measured on the MI355X: at most 3.4e-7 (dist), 4.5e-7 (cons), 1.1e-7 (id), 4.6e-7 (all) over the six grids.
MESH_GRAD_BAR = 1e-5
# Loss values: id is a mean of |theta| (no cancellation): 1e-5 as in test_warp_bwd_gpu.py.  The distortion and consistency terms are squares
# of differences of float32 vertices (values ~1, differences ~0.05: 2e-6 of relative rounding each before squaring): 1e-4 as there.
# Measured: at most 1.6e-7 (id), 9.2e-8 (dist), 1.1e-7 (cons).
MESH_ID_BAR, MESH_LOSS_BAR = 1e-5, 1e-4


@functools.lru_cache(maxsize=None)
def _mesh_case(gh, gw, N):
    """theta (std 0.05) with, per case: two vertices saturated well past the clip (one in the last sample, i.e. in the second sample
    round when N > 8), the x of a right-edge vertex exactly ON the clip (1.0 + 0.25 == 1.25 == float32(1 / 0.8)) in the last sample,
    one element exactly 0; and the float64 value and gradient of each term."""
    ocfg = O.Config(grid_h=gh, grid_w=gw, batch_size=N)
    nv = (gh + 1) * (gw + 1)
    rng = np.random.default_rng(100 * gh + 10 * gw + N)
    theta = (rng.standard_normal((N, 2 * nv)) * 0.05).astype(np.float32)
    sat = [(0, 0, -0.4), (N - 1, 2 * nv - 1, 0.5)]               # x of vertex (0, 0) = -1.4; y of vertex (gh, gw) = 1.5
    for n, e, v in sat:
        theta[n, e] = v
    on = (N - 1, 2 * (min(1, gh) * (gw + 1) + gw))               # x of the right-edge vertex of row 1: base 1.0
    theta[on] = 0.25
    zero = (0, 3)
    theta[zero] = 0.0
    assert np.float32(1.0) + theta[on] == np.float32(1.0) / np.float32(ocfg.do_crop_rate) == np.float32(1.25)
    th = T.t(theta, requires_grad=True)
    pts1, pts2 = T.get_4_pts(th, ocfg)
    vals = {"id": th.abs().mean() * ocfg.id_mul, "dist": T.get_distortion_loss(pts1, ocfg), "cons": T.get_consistency_loss(pts2, ocfg)}
    grads = {k: torch.autograd.grad(v, th, retain_graph=True)[0].numpy() for k, v in vals.items()}
    vals = {k: v.item() for k, v in vals.items()}
    # the reference itself: the tie passes the gradient of both mesh terms, saturation kills it
    assert grads["dist"][on] != 0.0 and grads["cons"][on] != 0.0
    assert all(grads[k][n, e] == 0.0 for k in ("dist", "cons") for n, e, _ in sat) and grads["id"][zero] == 0.0
    _ro(theta, *grads.values())
    return dict(theta=theta, sat=sat, on=on, zero=zero, vals=vals, grads=grads, nt=2 * nv)


def _mesh_cfg(gh, gw, N):
    from stabnet_amd.config import Config
    return Config(batch_size=N, grid_h=gh, grid_w=gw)


@pytest.mark.parametrize("term", list(MESH_TERMS))
@pytest.mark.parametrize("gh,gw,N", MESH_GRIDS)
def test_mesh_losses_one_term_at_a_time(cuda, gh, gw, N, term):
    from stabnet_amd import train_ops
    c = _mesh_case(gh, gw, N)
    cfg = _mesh_cfg(gh, gw, N)
    w_id, w_dist, w_cons = MESH_TERMS[term]
    want = w_id * c["grads"]["id"] + w_dist * c["grads"]["dist"] + w_cons * c["grads"]["cons"]
    losses, d_theta = train_ops.mesh_losses(_dev(c["theta"], cuda), None, cfg, w_id, w_dist, w_cons, 0.0, 0.0)
    got, lv = d_theta.cpu().numpy(), losses.cpu().numpy().astype(np.float64)
    err = relmax(got, want)
    lerr = [abs(lv[0] - c["vals"]["id"]) / c["vals"]["id"], abs(lv[2] - c["vals"]["dist"]) / c["vals"]["dist"],
            abs(lv[3] - c["vals"]["cons"]) / c["vals"]["cons"]]
    print("mesh_losses %dx%d N=%d %-4s: d_theta err %.2e of max|want| %.3e; losses id %.1e dist %.1e cons %.1e"
          % (gh, gw, N, term, err, np.abs(want).max(), *lerr))
    assert err < MESH_GRAD_BAR
    for n, e, v in c["sat"]:                                   # saturated: exactly the id term, nothing of the mesh terms
        idt = w_id * cfg.id_mul * np.sign(v) / (N * c["nt"])
        assert got[n, e] == pytest.approx(idt, rel=1e-6, abs=0.0) if w_id else got[n, e] == 0.0
    assert got[c["on"]] == pytest.approx(want[c["on"]], abs=MESH_GRAD_BAR * np.abs(want).max())
    if term in ("dist", "cons"):
        assert got[c["on"]] != 0.0                             # equality with the limit passes the gradient
        assert got[c["zero"]] == pytest.approx(want[c["zero"]], abs=MESH_GRAD_BAR * np.abs(want).max())
    if term == "id":
        assert got[c["zero"]] == 0.0                           # sign(0) = 0
    assert lerr[0] < MESH_ID_BAR and lerr[1] < MESH_LOSS_BAR and lerr[2] < MESH_LOSS_BAR
    assert lv[1] == 0.0                                        # the hinge is identically zero after the clip


@pytest.mark.parametrize("gh,gw,N", MESH_GRIDS)
def test_mesh_losses_black_hinge_adds_nothing_after_the_clip(cuda, gh, gw, N):
    from stabnet_amd import train_ops
    c = _mesh_case(gh, gw, N)
    cfg = _mesh_cfg(gh, gw, N)
    th = _dev(c["theta"], cuda)
    l0, d0 = train_ops.mesh_losses(th, None, cfg, 0.16, 1.0, 20.0, 0.0, 0.0)
    l1, d1 = train_ops.mesh_losses(th, None, cfg, 0.16, 1.0, 20.0, 1.0, 300000 / 2500)
    assert np.array_equal(_bits(d0.cpu().numpy()), _bits(d1.cpu().numpy()))
    assert l1[1].item() == 0.0 and torch.equal(l0, l1)


def test_mesh_losses_refuses_more_samples_than_its_reduction_holds(cuda):
    from stabnet_amd import train_ops
    from stabnet_amd._lib import StabnetError
    theta = torch.zeros((65, 50), device=cuda)
    with pytest.raises(StabnetError, match="mesh_losses"):
        train_ops.mesh_losses(theta, None, _mesh_cfg(4, 4, 65), 0.16, 1.0, 20.0, 0.0, 0.0)
    train_ops.mesh_losses(theta[:64].contiguous(), None, _mesh_cfg(4, 4, 64), 0.16, 1.0, 20.0, 0.0, 0.0)   # the limit itself runs
    torch.cuda.synchronize()


# ===================================================================================================================================
# B. transformer_bwd alone: d_pts2 against autograd with pts2 as the leaf, one input at a time
# (N, H, W, C, gh, gw): second block's waves wholly in the last cell column (uniform-wave branch) while the first block's are not, H % 4 != 0
# / every wave uniform (gw = 1) / 64 cells: the mesh kernel loops its waves / gh != gw / four-pixel groups straddle cell seams / C = 2
TB_CASES = [(1, 36, 300, 1, 4, 4), (2, 24, 40, 1, 2, 1), (1, 64, 64, 1, 8, 8), (2, 64, 96, 1, 2, 3), (2, 45, 77, 1, 4, 4), (1, 40, 48, 2, 4, 4)]
TB_INPUTS = ["d_out", "maps_dense", "maps_counts", "all"]
# Bar per case and input: 8 x the float32 floor of the reference, never looser than the 2e-3 of test_warp_bwd_gpu.py.  The floor is
# |float32 autograd - float64 autograd| of the same torch_ref graph relative to max|want|, measured on the CPU from the reference alone
# (tb_floors() below re-measures it; it is recorded here, not computed in the test, because it is one draw of rounding noise and
# moves by a few times between hosts: a bar must not).  The factor 8: the kernels' float32 forward values differ from torch's float32
# ones in summation order; their own sums are float64 / fixed point and should do no worse.
# What sets the error is the float32 forward state, not the backward kernels: a float64 NumPy restatement of both kernels fed with the
# oracle's float32 Hs and maps lands on the GPU's figure (8x8 maps_dense: 1.46e-4 against the GPU's 1.51e-4; fed with float64 maps:
# 2.8e-7).  The reference computes h = inv(A + 1e-4 I) b by inverting and then multiplying, which in float32 is not backward stable;
# the adjoint solve amplifies what that leaves in the maps, the more the smaller the cell.  torch_ref.get_Hs restates exactly that;
# with torch.linalg.solve in its place the float32 floor of the 8x8 case would read 1e-5 and say nothing about this graph.
#   case (N,H,W,C,gh,gw)         floor on the CPU: d_out, maps_dense, maps_counts, all         error on the MI355X, same order
TB_FLOOR = {
    (1, 36, 300, 1, 4, 4):     (4.27e-05, 1.64e-04, 5.18e-05, 1.34e-05),                     # 1.80e-05, 1.64e-05, 8.99e-06, 1.80e-05
    (2, 24, 40, 1, 2, 1):      (2.85e-06, 3.99e-07, 3.03e-07, 2.81e-06),                     # 3.47e-06, 1.28e-07, 1.26e-07, 3.48e-06
    (1, 64, 64, 1, 8, 8):      (1.84e-04, 1.61e-04, 1.92e-04, 1.55e-04),                     # 1.78e-04, 1.51e-04, 8.61e-05, 1.77e-04
    (2, 64, 96, 1, 2, 3):      (8.21e-06, 6.19e-07, 6.63e-07, 8.53e-06),                     # 8.55e-06, 3.90e-07, 7.51e-07, 8.54e-06
    (2, 45, 77, 1, 4, 4):      (1.41e-05, 5.39e-06, 5.21e-06, 1.51e-05),                     # 1.80e-05, 8.57e-06, 2.95e-06, 1.81e-05
    (1, 40, 48, 2, 4, 4):      (1.67e-05, 5.47e-06, 5.07e-06, 1.75e-05),                     # 9.33e-06, 2.20e-06, 3.84e-06, 8.93e-06
}
TB_LOOSEST = 2e-3


def _counts(rng, N, H, W):
    """Signed counts as the feature loss hands them over: sparse +-1 with some duplicates of magnitude 2..5."""
    c = np.zeros((N, H * W), np.float32)
    k = max(H * W // 16, 8)
    for n in range(N):
        idx = rng.choice(H * W, k, replace=False)
        v = rng.choice([-1.0, 1.0], k)
        v[:k // 4] *= rng.integers(2, 6, k // 4)
        c[n, idx] = v
    return c.reshape(N, H, W)


def _tb_autograd(c, dtype):
    """d L / d pts2 of each input's L in torch_ref's graph evaluated in `dtype` (the sampler corners are those of the float32 forward)."""
    saved, T.DT = T.DT, dtype
    try:
        p = T.t(c["pts2"], requires_grad=True)
        out, _, flow, _ = T.transformer(T.t(c["U"]), p, c["ocfg"], c["corners"])
        sc = T.t(c["scale"])[:, None, None]
        L = {"d_out": (out * T.t(c["g_out"])).sum(),
             "maps_dense": (flow[..., 0] * T.t(c["g_x"])).sum() + (flow[..., 1] * T.t(c["g_y"])).sum(),
             "maps_counts": (flow[..., 0] * T.t(c["c_x"]) * sc).sum() + (flow[..., 1] * T.t(c["c_y"]) * sc).sum()}
        L["all"] = L["d_out"] + L["maps_counts"]                # the form of the training step
        return {k: torch.autograd.grad(v, p, retain_graph=True)[0].double().numpy() for k, v in L.items()}
    finally:
        T.DT = saved


@functools.lru_cache(maxsize=None)
def _tb_case(N, H, W, C, gh, gw):
    ocfg = O.Config(height=H, width=W, batch_size=N, grid_h=gh, grid_w=gw)
    rng = np.random.default_rng(1000 * H + W)
    std = 0.05 * min(1.0, 4.0 / max(gh, gw))                   # 0.05 at the 0.5-wide cells of 4x4; scaled with the cell so that no cell folds over
    theta = (rng.standard_normal((N, (gh + 1) * (gw + 1) * 2)) * std).astype(np.float32)
    c = dict(ocfg=ocfg, theta=theta, U=(rng.random((N, H, W, C)) - 0.5).astype(np.float32),
             g_out=rng.standard_normal((N, H, W, C)).astype(np.float32), g_x=rng.standard_normal((N, H, W)).astype(np.float32),
             g_y=rng.standard_normal((N, H, W)).astype(np.float32), c_x=_counts(rng, N, H, W), c_y=_counts(rng, N, H, W),
             scale=np.array([0.0123, 0.0047], np.float32)[:N])  # differs between the samples
    c["pts2"] = O.get_4_pts(theta, ocfg)[1]
    c["corners"] = O.transformer(c["U"], c["pts2"], ocfg, return_all=True)[4]
    c["want"] = _tb_autograd(c, torch.float64)
    _ro(*[v for v in c.values() if isinstance(v, np.ndarray)], *c["want"].values())
    return c


def tb_floors():
    """Re-measure TB_FLOOR on the CPU (python -c "import test_warp_bwd_ops_gpu as M; M.tb_floors()" in tests/)."""
    for case in TB_CASES:
        c = _tb_case(*case)
        f32 = _tb_autograd(c, torch.float32)
        print("    %-26s (%s)," % ("%r:" % (case,), ", ".join("%.2e" % relmax(f32[k], c["want"][k]) for k in TB_INPUTS)))


def _tb_run(cuda, case, inp, c):
    from stabnet_amd import train_ops, warp
    from stabnet_amd.config import Config
    N, H, W, C, gh, gw = case
    cfg = Config(height=H, width=W, batch_size=N, grid_h=gh, grid_w=gw)
    r = warp.warp_from_theta(_dev(c["U"], cuda), _dev(c["theta"], cuda), cfg)
    a = (r["pts2"], r["Hs"], _dev(c["U"], cuda), r["x_map"], r["y_map"])
    if inp == "d_out":
        return train_ops.transformer_bwd(*a, _dev(c["g_out"], cuda), None, None, cfg)
    if inp == "maps_dense":
        return train_ops.transformer_bwd(*a, None, _dev(c["g_x"], cuda), _dev(c["g_y"], cuda), cfg)
    d_out = _dev(c["g_out"], cuda) if inp == "all" else None
    return train_ops.transformer_bwd(*a, d_out, _dev(c["c_x"], cuda), _dev(c["c_y"], cuda), cfg, dmap_scale=_dev(c["scale"], cuda))


@pytest.mark.parametrize("inp", TB_INPUTS)
@pytest.mark.parametrize("case", TB_CASES, ids=lambda c: "x".join(map(str, c)))
def test_transformer_bwd_one_input_at_a_time(cuda, case, inp):
    c = _tb_case(*case)
    got = _tb_run(cuda, case, inp, c).cpu().numpy()
    floor, err = TB_FLOOR[case][TB_INPUTS.index(inp)], relmax(got, c["want"][inp])
    bar = min(8.0 * floor, TB_LOOSEST)
    print("transformer_bwd %-16s %-11s: float32 floor of the reference %.2e, bar %.2e, GPU error %.2e (max|want| %.3e)"
          % (",".join(map(str, case)), inp, floor, bar, err, np.abs(c["want"][inp]).max()))
    assert np.isfinite(got).all()
    assert err < bar


def test_transformer_bwd_repeats_bit_for_bit_and_zero_in_gives_zero_out(cuda):
    from stabnet_amd import train_ops, warp
    from stabnet_amd.config import Config
    case = (2, 45, 77, 1, 4, 4)
    c = _tb_case(*case)
    one, two = _tb_run(cuda, case, "all", c), _tb_run(cuda, case, "all", c)
    assert torch.equal(one, two) and one.abs().max().item() > 0
    N, H, W, C, gh, gw = case
    cfg = Config(height=H, width=W, batch_size=N, grid_h=gh, grid_w=gw)
    r = warp.warp_from_theta(_dev(c["U"], cuda), _dev(c["theta"], cuda), cfg)
    z = torch.zeros((N, H, W), device=cuda)
    for scale in (None, _dev(c["scale"], cuda)):
        got = train_ops.transformer_bwd(r["pts2"], r["Hs"], _dev(c["U"], cuda), r["x_map"], r["y_map"], None, z, z, cfg, dmap_scale=scale)
        assert (got == 0).all()


# ===================================================================================================================================
# C. interp_bwd
IB_NAMES = ["one-tile", "tile+1", "near-id", "uniform", "shift+4+8", "shift-4-8", "shift+5+9", "shift-5-9"]
# float32 weights x float32 d_out, summed exactly (fixed point): the existing bar of test_warp_bwd_gpu.py.  The weights are differences such
# as x1 - xp with xp = (x + 1) * W / 2 rounded to float32 at a magnitude of up to 300: 1.5e-5 absolute on a weight of order 1.
# Measured: at most 2.5e-5 (2.0e-5 for the uniform flow at W = 300, the same for both kernels; 2.5e-5 with half of d_out zero at W = 260).
IB_BAR = 1e-4


def _near_identity(rng, N, H, W, sigma):
    gx, gy = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H))
    return (gx[None] + rng.normal(0, sigma, (N, H, W))).astype(np.float32), (gy[None] + rng.normal(0, sigma, (N, H, W))).astype(np.float32)


def _shifted(H, W, dy, dx):
    """Pixel (r, c) samples at (r + dy + 0.37, c + dx + 0.37): its taps are (r + dy, c + dx) and the next row / column (clipped to the frame).
    With the 16 x 128 tile and its halo of 4 rows and 8 columns, 4 / 8 put the first tap of a tile's edge pixels on the last window element
    and the second one just past it; 5 / 9 put both past it."""
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x = ((cc + dx + 0.37) * 2.0 / W - 1.0).astype(np.float32)
    y = ((rr + dy + 0.37) * 2.0 / H - 1.0).astype(np.float32)
    return x[None], y[None]


def _interp_want(x, y, g):
    """float64 d_im and the set of pixels that a tap of a pixel with g != 0 lands on."""
    N, H, W, C = g.shape
    zero = np.zeros(g.shape, np.float32)
    corners = O._interpolate(zero, x.reshape(-1), y.reshape(-1))[1]
    imt = T.t(zero, requires_grad=True)
    (T.interpolate(imt, T.t(x), T.t(y), corners) * T.t(g)).sum().backward()
    x0, y0, x1, y1 = (np.asarray(a).reshape(N, H, W).astype(np.int64) for a in corners)
    live = np.any(g != 0, axis=3)
    landed = np.zeros((N, H, W), bool)
    n = np.broadcast_to(np.arange(N)[:, None, None], (N, H, W))
    for yy, xx in ((y0, x0), (y1, x0), (y0, x1), (y1, x1)):
        landed[n[live], yy[live], xx[live]] = True
    return imt.grad.numpy(), landed


@functools.lru_cache(maxsize=None)
def _ib_case(name):
    rng = np.random.default_rng(IB_NAMES.index(name) + 40)
    if name == "one-tile":
        N, H, W = 1, 16, 128
        x, y = _near_identity(rng, N, H, W, 0.05)
    elif name == "tile+1":
        N, H, W = 1, 17, 129
        x, y = _near_identity(rng, N, H, W, 0.05)
    elif name == "near-id":
        N, H, W = 2, 70, 300
        x, y = _near_identity(rng, N, H, W, 0.05)
    elif name == "uniform":
        N, H, W = 2, 70, 300
        x, y = rng.uniform(-1.2, 1.2, (N, H, W)).astype(np.float32), rng.uniform(-1.2, 1.2, (N, H, W)).astype(np.float32)
    else:
        N, H, W = 1, 40, 272
        sgn, dy, dx = (1 if name[5] == "+" else -1), int(name[6]), int(name[8])
        x, y = _shifted(H, W, sgn * dy, sgn * dx)
    g = rng.standard_normal((N, H, W, 1)).astype(np.float32)
    want, landed = _interp_want(x, y, g)
    _ro(x, y, g, want, landed)
    return x, y, g, want, landed


@pytest.fixture(scope="module")
def untiled(tmp_path_factory):
    """d_im of every one-channel case from the untiled kernel: ONE child process with STABNET_INTERP_BWD_TILED=0 (read once per process)."""
    assert os.environ.get("STABNET_INTERP_BWD_TILED", "1") != "0", "the parent must run the tiled kernel"
    d = tmp_path_factory.mktemp("interp_bwd")
    inp, out = str(d / "in.npz"), str(d / "out.npz")
    arrays = {}
    for i, name in enumerate(IB_NAMES):
        arrays["x_%d" % i], arrays["y_%d" % i], arrays["g_%d" % i] = _ib_case(name)[:3]
    np.savez(inp, **arrays)
    env = dict(os.environ, STABNET_INTERP_BWD_TILED="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "interp_bwd_child.py"), inp, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    return {name: z["d_%d" % i] for i, name in enumerate(IB_NAMES)}


@pytest.mark.parametrize("name", IB_NAMES)
def test_interp_bwd_tiled_equals_untiled_and_autograd(cuda, untiled, name):
    from stabnet_amd import train_ops
    x, y, g, want, landed = _ib_case(name)
    got = train_ops.interp_bwd(_dev(x, cuda), _dev(y, cuda), _dev(g, cuda)).cpu().numpy()
    err, err_u = relmax(got, want), relmax(untiled[name], want)
    print("interp_bwd %-9s: tiled err %.2e, untiled err %.2e of max|want| %.3e" % (name, err, err_u, np.abs(want).max()))
    assert np.array_equal(_bits(got), _bits(untiled[name]))       # the same integer sums whatever the flow
    assert err < IB_BAR and err_u < IB_BAR
    assert (got[..., 0][~landed] == 0.0).all()


def test_interp_bwd_accumulates_one_float_onto_one_float(cuda):
    """d_im=base: base + plain bit for bit; untouched where no tap lands (a flow that contracts towards the centre leaves a border)."""
    from stabnet_amd import train_ops
    N, H, W = 2, 37, 150
    rng = np.random.default_rng(7)
    x, y = _near_identity(rng, N, H, W, 0.01)
    x, y = (x * np.float32(0.5)), (y * np.float32(0.5))
    g = rng.standard_normal((N, H, W, 1)).astype(np.float32)
    base = rng.standard_normal((N, H, W, 1)).astype(np.float32)
    want, landed = _interp_want(x, y, g)
    assert (~landed).sum() > H * W and landed.sum() > H * W // 4
    plain = train_ops.interp_bwd(_dev(x, cuda), _dev(y, cuda), _dev(g, cuda)).cpu().numpy()
    buf = _dev(base, cuda)
    ret = train_ops.interp_bwd(_dev(x, cuda), _dev(y, cuda), _dev(g, cuda), d_im=buf)
    assert ret.data_ptr() == buf.data_ptr()
    acc = buf.cpu().numpy()
    assert relmax(plain, want) < IB_BAR
    assert np.array_equal(_bits(acc), _bits(base + plain))
    assert np.array_equal(_bits(plain[..., 0][~landed]), np.zeros((~landed).sum(), np.int32))      # exactly +0.0
    assert np.array_equal(_bits(acc[..., 0][~landed]), _bits(base[..., 0][~landed]))


@pytest.mark.parametrize("C", [1, 2])
def test_interp_bwd_skips_exact_zeros_in_d_out(cuda, C):
    """Half of d_out exactly zero (the left half and a random sprinkle): the g == 0 skip of both kernels."""
    from stabnet_amd import train_ops
    N, H, W = 1, 33, 260
    rng = np.random.default_rng(8 + C)
    x, y = _near_identity(rng, N, H, W, 0.01)
    g = rng.standard_normal((N, H, W, C)).astype(np.float32)
    g[:, :, :W // 2] = 0.0
    g[rng.random((N, H, W)) < 0.2] = 0.0
    want, landed = _interp_want(x, y, g)
    assert (~landed).sum() > H * W // 3
    got = train_ops.interp_bwd(_dev(x, cuda), _dev(y, cuda), _dev(g, cuda)).cpu().numpy()
    err = relmax(got, want)
    print("interp_bwd zeros C=%d: err %.2e" % (C, err))
    assert err < IB_BAR
    assert (got[~landed] == 0.0).all()


@pytest.mark.parametrize("C", [2, 3])
def test_interp_bwd_more_channels(cuda, C):
    from stabnet_amd import train_ops
    N, H, W = 1, 33, 130
    rng = np.random.default_rng(20 + C)
    x, y = _near_identity(rng, N, H, W, 0.05)
    g = rng.standard_normal((N, H, W, C)).astype(np.float32)
    want, _ = _interp_want(x, y, g)
    err = relmax(train_ops.interp_bwd(_dev(x, cuda), _dev(y, cuda), _dev(g, cuda)).cpu().numpy(), want)
    print("interp_bwd C=%d: err %.2e" % (C, err))
    assert err < IB_BAR


# ===================================================================================================================================
# D. masked MSE: sums, gradient, accumulate
# (N, hw): one element / less than a block / 65 partials (the finalize kernel's lane-strided loop) / production 288x512: 72 partials /
# above 512 * 2048: the capped grid, grid-stride loop of both kernels / three samples
MSE_CASES = [(2, 1), (2, 255), (2, 2048 * 64 + 1), (2, 288 * 512), (1, 512 * 2048 + 777), (3, 777)]
# Sums: float32 partials of at most 2048 (8 per thread, then a tree) elements, added in float64: the existing 1e-5.  Measured: at most 7.0e-8.
# Gradient: elementwise float32, its only accumulated input is sums[n, 1]: 1e-5 of the sample's gradient maximum.  Measured: at most 1.4e-7.
MSE_BAR = 1e-5


@functools.lru_cache(maxsize=None)
def _mse_case(N, hw):
    rng = np.random.default_rng(hw % 9973 + N)
    a, b = rng.standard_normal((N, hw)).astype(np.float32), rng.standard_normal((N, hw)).astype(np.float32)
    black = (rng.random((N, hw)) < 0.2).astype(np.float32)
    if hw == 1:
        black[0] = 0.0
    if N > 1:
        black[N - 1] = 1.0                                       # a sample that is black everywhere: sums {0, 0}, value 0, gradient 0
    m2 = rng.random((N, hw)).astype(np.float32)
    ga0 = rng.standard_normal((N, hw)).astype(np.float32)
    _ro(a, b, black, m2, ga0)
    return a, b, black, m2, ga0


@pytest.mark.parametrize("with_m2", [False, True], ids=["img", "temporal"])
@pytest.mark.parametrize("N,hw", MSE_CASES)
def test_masked_mse_sums_and_gradient(cuda, N, hw, with_m2):
    from stabnet_amd import train_ops
    a, b, black, m2, ga0 = _mse_case(N, hw)
    coef = 3.0 / N
    # float64 of the formula in the kernels' comments
    m = (1.0 - black.astype(np.float64)) * (m2.astype(np.float64) if with_m2 else 1.0)
    e = (a.astype(np.float64) - b) * m
    s0, s1 = (e * e).sum(axis=1), m.sum(axis=1)
    g_want = coef * 2.0 * (a.astype(np.float64) - b) * m * m / (s1 + 1e-8)[:, None]

    da, db, dbl, dm = _dev(a, cuda), _dev(b, cuda), _dev(black, cuda), (_dev(m2, cuda) if with_m2 else None)
    sums = train_ops.masked_mse_sums(da, db, dbl, dm)
    s = sums.cpu().numpy().astype(np.float64)
    ga, gb = train_ops.masked_mse_grad(da, db, dbl, dm, sums, coef, want_gb=True)
    g, gbn = ga.cpu().numpy(), gb.cpu().numpy()
    live = s1 > 0
    assert (s0[live] > 0).all()
    serr = max((np.abs(s[live, 0] - s0[live]) / s0[live]).max(), (np.abs(s[live, 1] - s1[live]) / s1[live]).max())
    gerr = max(relmax(g[n], g_want[n]) for n in range(N) if live[n])
    print("masked_mse N=%d hw=%d m2=%d: sums err %.2e, gradient err %.2e" % (N, hw, with_m2, serr, gerr))
    assert serr < MSE_BAR and gerr < MSE_BAR
    assert np.isfinite(g).all()
    for n in np.nonzero(~live)[0]:                                # the all-black sample
        assert s[n, 0] == 0.0 and s[n, 1] == 0.0 and (g[n] == 0.0).all()
    assert np.array_equal(gbn, -g)
    # accumulate: ga + g, one float32 add per element
    buf = _dev(ga0, cuda)
    ret, none = train_ops.masked_mse_grad(da, db, dbl, dm, sums, coef, ga=buf, accumulate_a=True)
    assert none is None and ret.data_ptr() == buf.data_ptr()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(ga0 + g))


# ===================================================================================================================================
# E. feature loss
FL_MX = [1, 1024, 1025, 3000, 3073, 7000]
FL_N, FL_H, FL_W = 2, 32, 64                                    # powers of two: pixel coordinates are exact
# value: a float32 sum of at most 7000 non-negative terms (7 per thread, then a tree).  counts x dscale: exact counts times one float32
# quotient.  Measured: value at most 7.9e-8, gradient at most 6.7e-8.
FL_BAR = 1e-5
FL_PIX = (10, 5)                                                 # (x, y) of the pixel that a block of matches is forced onto


@functools.lru_cache(maxsize=None)
def _fl_case(Mx):
    N, H, W = FL_N, FL_H, FL_W
    cfg = O.Config(height=H, width=W, batch_size=N, max_matches=Mx)
    rng = np.random.default_rng(Mx)
    matches = rng.uniform(-1.1, 1.1, (N, Mx, 4)).astype(np.float32)             # past +-1: the clamp to the frame
    mask = (rng.random((N, Mx)) < 0.6).astype(np.float32)
    flow = rng.standard_normal((N, H, W, 2)).astype(np.float32)
    mask[0, Mx - 1] = 1.0                                                       # the last match counts, and counts once
    mask[1] = 0.0                                                               # a sample without matches
    if Mx >= 1024:
        matches[0, 5:25, 0], matches[0, 5:25, 1] = 2.0 * FL_PIX[0] / W - 1.0, 2.0 * FL_PIX[1] / H - 1.0
        matches[0, 5:25, 2:] = -10.0                                            # below every map value: all 20 push the same way
        mask[0, 5:25] = 1.0
        k = np.arange(10)
        matches[0, 30:40, 0], matches[0, 30:40, 1] = (2 * k + 1) / W - 1.0, (2 * k + 5) / H - 1.0     # px = k + 0.5, py = k + 2.5: half to even
        mask[0, 30:40] = 1.0
        (xi, yi) = O.warp_pts(matches[:, :, :2], flow, cfg)[1]
        matches[0, 40:50, 2:] = flow[0, yi[0, 40:50], xi[0, 40:50]]             # target == map value bit for bit: adds nothing
        mask[0, 40:50] = 1.0
    warped, (xi, yi) = O.warp_pts(matches[:, :, :2], flow, cfg)
    if Mx >= 1024:
        assert np.array_equal(xi[0, 30:40], [0, 2, 2, 4, 4, 6, 6, 8, 8, 10]) and np.array_equal(yi[0, 30:40], [2, 4, 4, 6, 6, 8, 8, 10, 10, 12])
        assert np.array_equal(warped[0, 40:50], matches[0, 40:50, 2:])
    # signed counts and per-sample values, float64 / integers
    cnt = np.zeros((2, N, H, W), np.int64)
    d = warped.astype(np.float64) - matches[:, :, 2:]
    for n in range(N):
        for ax in (0, 1):
            np.add.at(cnt[ax, n], (yi[n], xi[n]), (np.sign(d[n, :, ax]) * mask[n]).astype(np.int64))
    value = (np.abs(d).sum(axis=2) * mask).sum(axis=1) / np.maximum(mask.sum(axis=1, dtype=np.float64), 1.0)
    ft = T.t(flow, requires_grad=True)
    (T.feature_loss(T.t(matches), T.t(mask), ft, cfg) * 2.5).backward()
    grad = ft.grad.numpy()
    _ro(matches, mask, flow, warped, cnt, value, grad)
    return matches, mask, flow, warped, cnt, value, grad


@pytest.mark.parametrize("Mx", FL_MX)
def test_feature_loss_counts_value_and_warped(cuda, Mx):
    from stabnet_amd import train_ops
    N = FL_N
    matches, mask, flow, warped_want, cnt, value, grad = _fl_case(Mx)
    gcoef = 2.5 / N
    a = (_dev(matches, cuda), _dev(mask, cuda), _dev(flow[..., 0], cuda), _dev(flow[..., 1], cuda))
    val, dxm, dym, warped, dscale = train_ops.feature_loss(*a, gcoef, True, True)
    val2, dxm2, dym2, warped2, dscale2 = train_ops.feature_loss(*a, gcoef, True, True)
    val3 = train_ops.feature_loss(*a)[0]
    v, cx, cy, ds = val.cpu().numpy(), dxm.cpu().numpy(), dym.cpu().numpy(), dscale.cpu().numpy()
    assert np.array_equal(cx, cnt[0]) and np.array_equal(cy, cnt[1])           # exact integers, the tail match counted once
    if Mx >= 1024:
        assert cx[0, FL_PIX[1], FL_PIX[0]] >= 15 and cy[0, FL_PIX[1], FL_PIX[0]] >= 15
    assert not cx[1].any() and not cy[1].any() and v[1] == 0.0 and ds[1] == np.float32(gcoef)
    verr = abs(v[0] - value[0]) / value[0]
    gerr = max(relmax(cx * ds[:, None, None], grad[..., 0]), relmax(cy * ds[:, None, None], grad[..., 1]))
    print("feature_loss Mx=%d: value err %.2e, counts x dscale err %.2e, largest |count| %d" % (Mx, verr, gerr, np.abs(cnt).max()))
    assert verr < FL_BAR and gerr < FL_BAR
    assert np.array_equal(_bits(warped.cpu().numpy()), _bits(warped_want))
    for one, two in ((val, val2), (dxm, dxm2), (dym, dym2), (warped, warped2), (dscale, dscale2), (val, val3)):
        assert torch.equal(one, two)
