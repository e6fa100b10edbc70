"""Host wrappers of the training-side C-ABI entry points (backward of warp/sampler, loss kernels)."""
from __future__ import annotations

import torch

from . import _lib
from ._tensor import dev_f32, empty, ptr, stream_ptr
from .config import Config, v2_93


def transformer_bwd(pts2, Hs, U, x_map, y_map, d_out=None, d_xmap=None, d_ymap=None, cfg: Config = v2_93, dmap_scale=None):
    """d_xmap / d_ymap are multiplied per sample by dmap_scale [N] when given (feature_loss returns counts + that scale)."""
    U = dev_f32(U, "U")
    N, H, W, C = U.shape
    d_pts2 = empty((N, cfg.grid_h + 1, cfg.grid_w + 1, 2), U)
    ws = empty((N * cfg.grid_h * cfg.grid_w * 8 + 1,), U, dtype=torch.int64)    # fixed-point sums + the poison word
    _lib.call("stabnet_transformer_bwd", ptr(dev_f32(pts2)), ptr(dev_f32(Hs)), ptr(U), ptr(dev_f32(x_map)),
              ptr(dev_f32(y_map)), ptr(d_out), ptr(d_xmap), ptr(d_ymap), ptr(dmap_scale), N, H, W, C, cfg.grid_h, cfg.grid_w, ptr(d_pts2),
              ptr(ws), stream_ptr(U.device), device=U.device)
    return d_pts2


def interp_bwd(x, y, d_out, d_im=None):
    """d_im (+)= scatter of d_out; a given d_im is accumulated into."""
    d_out = dev_f32(d_out, "d_out")
    N, H, W, C = d_out.shape
    acc = d_im is not None
    if d_im is None:
        d_im = empty((N, H, W, C), d_out)
    ws = empty((N * H * W * C + 1,), d_out, dtype=torch.int64)       # fixed-point accumulators of the scatter + the poison word
    _lib.call("stabnet_interp_bwd", ptr(dev_f32(x)), ptr(dev_f32(y)), ptr(d_out), N, H, W, C, ptr(d_im), int(acc), ptr(ws),
              stream_ptr(d_out.device), device=d_out.device)
    return d_im


def axpb(x, a, b):
    x = dev_f32(x)
    y = torch.empty_like(x)
    _lib.call("stabnet_axpb", ptr(x), float(a), float(b), x.numel(), ptr(y), stream_ptr(x.device), device=x.device)
    return y


def masked_mse_sums(a, b, black, m2=None):
    a = dev_f32(a)
    N = a.shape[0]
    hw = a.numel() // N
    sums = empty((N, 2), a)
    ws = torch.empty(_lib.lib().stabnet_masked_mse_workspace_bytes(N), dtype=torch.uint8, device=a.device)
    _lib.call("stabnet_masked_mse_sums", ptr(a), ptr(dev_f32(b)), ptr(dev_f32(black)), ptr(m2), N, hw, ptr(sums), ptr(ws),
              stream_ptr(a.device), device=a.device)
    return sums


def masked_mse_grad(a, b, black, m2, sums, coef, ga=None, accumulate_a=False, want_gb=False):
    a = dev_f32(a)
    N = a.shape[0]
    hw = a.numel() // N
    if ga is None:
        ga = torch.empty_like(a)
        accumulate_a = False
    gb = torch.empty_like(a) if want_gb else None
    _lib.call("stabnet_masked_mse_grad", ptr(a), ptr(dev_f32(b)), ptr(dev_f32(black)), ptr(m2), ptr(sums), float(coef),
              N, hw, ptr(ga), int(accumulate_a), ptr(gb), stream_ptr(a.device), device=a.device)
    return ga, gb


def feature_loss(matches, mask, x_map, y_map, gcoef=0.0, want_grad=False, want_warped=False):
    """-> (value [N], d_xmap, d_ymap, warped, dscale): the map gradient is (d_xmap, d_ymap) [signed counts] * dscale[n]."""
    matches = dev_f32(matches)
    N, Mx, _ = matches.shape
    x_map = dev_f32(x_map)
    H, W = x_map.shape[1], x_map.shape[2]
    value = empty((N,), matches)
    dxm = empty((N, H, W), matches) if want_grad else None
    dym = empty((N, H, W), matches) if want_grad else None
    warped = empty((N, Mx, 2), matches) if want_warped else None
    dscale = empty((N,), matches) if want_grad else None
    _lib.call("stabnet_feature_loss", ptr(matches), ptr(dev_f32(mask)), ptr(x_map), ptr(dev_f32(y_map)), N, H, W, Mx,
              float(gcoef), ptr(value), ptr(dxm), ptr(dym), ptr(dscale), ptr(warped), stream_ptr(matches.device),
              device=matches.device)
    return value, dxm, dym, warped, dscale


def mesh_losses(theta, d_pts2_warp, cfg: Config, w_id, w_dist, w_cons, use_black, w_black):
    theta = dev_f32(theta)
    N = theta.shape[0]
    losses = empty((4,), theta)
    d_theta = torch.empty_like(theta)
    _lib.call("stabnet_mesh_losses", ptr(theta), ptr(d_pts2_warp), N, cfg.grid_h, cfg.grid_w, cfg.do_crop_rate,
              cfg.id_mul, float(w_id), float(w_dist), float(w_cons), float(use_black), float(w_black), ptr(losses),
              ptr(d_theta), stream_ptr(theta.device), device=theta.device)
    return losses, d_theta


# ---- the non-convolution training layers, one operator per call (the launchers of the training step) ----------------------

def col_reduce_workspace_floats(M, C, groups=1):
    return int(_lib.lib().stabnet_col_reduce_workspace_floats(M, C, groups))


def _pair(ts):
    """(ptr0, ptr1) of a 1- or 2-element list of tensors (or None)."""
    if ts is None:
        return 0, 0
    return ptr(ts[0]), (ptr(ts[1]) if len(ts) > 1 else 0)


def bn_stats_train(xs, gamma, beta, eps, decay, stats, mov_mean=None, mov_var=None, partial=None):
    """xs: one or two [M, C] tensors (the towers); stats: as many [4, C] outputs (scale, shift, mean, invstd)."""
    M, C = xs[0].shape
    if partial is None:
        partial = empty((col_reduce_workspace_floats(M, C, len(xs)),), xs[0])
    _lib.call("stabnet_bn_stats_train", len(xs), *_pair(xs), M, C, ptr(gamma), ptr(beta), float(eps), float(decay), *_pair(stats),
              ptr(mov_mean), ptr(mov_var), ptr(partial), stream_ptr(xs[0].device), device=xs[0].device)
    return stats


def bn_relu_bwd(xs, gs, stats, gamma, d_gamma, d_beta, d_xs, coefs, addends=None, add_stride=1, H=0, W=0, partial=None):
    M, C = xs[0].shape
    if partial is None:
        partial = empty((col_reduce_workspace_floats(M, C, len(xs)),), xs[0])
    x0, x1 = _pair(xs)
    g0, g1 = _pair(gs)
    s0, s1 = _pair(stats)
    a0, a1 = _pair(addends)
    d0, d1 = _pair(d_xs)
    c0, c1 = _pair(coefs)
    _lib.call("stabnet_bn_relu_bwd", len(xs), x0, x1, g0, g1, s0, s1, ptr(gamma), M, C, a0, a1, int(add_stride), int(H), int(W),
              ptr(d_gamma), ptr(d_beta), d0, d1, ptr(partial), c0, c1, stream_ptr(xs[0].device), device=xs[0].device)
    return d_xs


def bias_grad(gs, d_bias, d_bias2=None, partial=None):
    M, C = gs[0].shape
    if partial is None:
        partial = empty((col_reduce_workspace_floats(M, C, len(gs)),), gs[0])
    _lib.call("stabnet_bias_grad", len(gs), *_pair(gs), M, C, ptr(d_bias), ptr(d_bias2), ptr(partial), stream_ptr(gs[0].device),
              device=gs[0].device)
    return d_bias


def max_pool_train_fwd(x, y, argmax, k, stride, pt, pl):
    """x [N,H,W,C] -> y [N,Ho,Wo,C] and the argmax bytes (uint8, same shape); Ho, Wo are taken from y."""
    N, H, W, C = x.shape
    _lib.call("stabnet_max_pool_train_fwd", ptr(x), ptr(y), ptr(argmax), N, H, W, C, y.shape[1], y.shape[2], k, stride, pt, pl,
              stream_ptr(x.device), device=x.device)
    return y, argmax


def max_pool_bwd(argmax, dy, dx, k, stride, pt, pl):
    N, H, W, C = dx.shape
    _lib.call("stabnet_max_pool_bwd", ptr(argmax), ptr(dy), ptr(dx), N, H, W, C, dy.shape[1], dy.shape[2], k, stride, pt, pl,
              stream_ptr(dx.device), device=dx.device)
    return dx


def gap_bwd(dg, da):
    """dg [N,C] -> da [N,HW,C]."""
    N, HW, C = da.shape
    _lib.call("stabnet_gap_bwd", ptr(dg), N, HW, C, ptr(da), stream_ptr(da.device), device=da.device)
    return da


def fc_bwd_scratch_floats(M, K, Nout):
    return int(_lib.lib().stabnet_fc_bwd_scratch_floats(M, K, Nout))


def fc_bwd(x, w, y, dy, dW, db, dx=None, scratch=None):
    """y = None: no ReLU.  dW, db are accumulated into; dx (optional) is written."""
    M, K = x.shape
    Nout = w.shape[0]
    if dx is not None and scratch is None:
        scratch = empty((fc_bwd_scratch_floats(M, K, Nout),), x)
    _lib.call("stabnet_fc_bwd", ptr(x), ptr(w), ptr(y), ptr(dy), M, K, Nout, int(y is not None), ptr(dW), ptr(db), ptr(dx),
              ptr(scratch), 0 if scratch is None else scratch.numel(), stream_ptr(x.device), device=x.device)
    return dW, db, dx
