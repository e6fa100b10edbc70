"""Thin host wrappers of the regressor building blocks of the C ABI (used by tests and by regressor.py)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import StabnetError
from ._tensor import dev_f32, empty, ptr, stream_ptr


def _out(out, shape, like):
    """The tensor an operator writes: the caller's `out` (contiguous float32 of `shape` on like's device -- a view of a larger buffer
    will do) or a fresh one."""
    if out is None:
        return empty(tuple(shape), like)
    if not (isinstance(out, torch.Tensor) and out.device == like.device and out.dtype == torch.float32 and out.is_contiguous() and
            tuple(out.shape) == tuple(shape)):
        raise StabnetError("out: expected a contiguous float32 tensor of shape %s on %s" % (tuple(shape), like.device))
    return out


def _workspace(workspace, nbytes, like):
    """(tensor, bytes) of an operator's scratch: the caller's `workspace` (contiguous, at least `nbytes` long) or a fresh one."""
    if workspace is None:
        return torch.empty(max(nbytes, 4), dtype=torch.uint8, device=like.device), nbytes
    have = workspace.numel() * workspace.element_size()
    if not (workspace.device == like.device and workspace.is_contiguous() and have >= nbytes):
        raise StabnetError("workspace: expected a contiguous tensor of at least %d bytes on %s" % (nbytes, like.device))
    return workspace, have


def pack_conv_weight(w_hwio, cin_pad: int = 16) -> np.ndarray:
    """TF HWIO [kh,kw,Cin,Cout] -> the library's OHWI [Cout,kh,kw,Cin'] with Cin' = Cin rounded up to `cin_pad`."""
    w = np.asarray(w_hwio, np.float32)
    kh, kw, ci, co = w.shape
    cp = -(-ci // cin_pad) * cin_pad
    out = np.zeros((co, kh, kw, cp), np.float32)
    out[..., :ci] = np.transpose(w, (3, 0, 1, 2))
    return out


def unpack_conv_weight(w_ohwi, cin: int) -> np.ndarray:
    return np.ascontiguousarray(np.transpose(np.asarray(w_ohwi, np.float32)[..., :cin], (1, 2, 3, 0)))


def conv2d(x, w_ohwi, bias=None, in_scale=None, in_shift=None, residual=None, res_stride=1, stride=1, pad=0,
           relu_out=False, out_scale=None, out_shift=None, out=None, workspace=None):
    x = dev_f32(x, "x")
    w = dev_f32(w_ohwi, "w")
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cw = w.shape
    assert Cw == Cin, "weight Cin %d != input Cin %d" % (Cw, Cin)
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    y = _out(out, (N, Ho, Wo, Cout), x)
    L = _lib.lib()
    ws, ws_bytes = _workspace(workspace, int(L.stabnet_conv2d_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad)), x)
    rH, rW = (residual.shape[1], residual.shape[2]) if residual is not None else (0, 0)
    _lib.call("stabnet_conv2d_fwd_ex", ptr(x), ptr(w), ptr(bias), ptr(in_scale), ptr(in_shift), ptr(residual), rH, rW,
              res_stride, ptr(out_scale), ptr(out_shift), ptr(y), N, H, W, Cin, Cout, KH, KW, stride, pad,
              int(relu_out), ptr(ws), ws_bytes, stream_ptr(x.device), device=x.device)
    return y


def conv2d_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride=1, pad=0):
    """Bytes of scratch conv2d asks for (split-K slabs; 0 without a K split)."""
    return int(_lib.lib().stabnet_conv2d_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride=1, pad=0, splitk=0):
    """Bytes of scratch conv2d_packed asks for: the planned split's slabs, or those of the caller's `splitk`."""
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    return max(conv2d_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad), max(splitk, 0) * N * Ho * Wo * Cout * 4)


def conv2d_packed(x, w_ohwi, bias=None, in_scale=None, in_shift=None, residual=None, res_stride=1, stride=1, pad=0,
                  relu_out=False, out_scale=None, out_shift=None, splitk=0, out=None, workspace=None):
    """conv2d on the packed split kernels (stabnet_conv2d_fwd_packed): float32-level results on the bf16 matrix pipe."""
    x = dev_f32(x, "x")
    w = dev_f32(w_ohwi, "w")
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cw = w.shape
    assert Cw == Cin, "weight Cin %d != input Cin %d" % (Cw, Cin)
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    y = _out(out, (N, Ho, Wo, Cout), x)
    L = _lib.lib()
    n_img = int(L.stabnet_conv_weight_image_floats(Cout, KH, KW, Cin))
    img = torch.empty(max(n_img, 1), dtype=torch.float32, device=x.device)
    if n_img > 0:                      # (Cin not a multiple of 32: no image exists and the call runs the exact-f32 kernels on w_ohwi)
        _lib.call("stabnet_conv_weight_split_image", ptr(w), Cout, KH, KW, Cin, ptr(img), stream_ptr(x.device), device=x.device)
    ws, ws_bytes = _workspace(workspace, conv2d_packed_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad, splitk), x)
    rH, rW = (residual.shape[1], residual.shape[2]) if residual is not None else (0, 0)
    _lib.call("stabnet_conv2d_fwd_packed", ptr(x), ptr(w), ptr(img), ptr(bias), ptr(in_scale), ptr(in_shift), ptr(residual), rH, rW,
              res_stride, ptr(out_scale), ptr(out_shift), ptr(y), N, H, W, Cin, Cout, KH, KW, stride, pad, int(relu_out), int(splitk),
              ptr(ws), ws_bytes, stream_ptr(x.device), device=x.device)
    return y


def conv_unit_pair(x, w3_ohwi, bias3, residual, pre_scale, pre_shift, w1_ohwi, out_scale=None, out_shift=None, relu_out=True,
                   out3=None, out=None):
    """A unit's 1x1 conv3 (+ bias + residual) and the next identity unit's 1x1 conv1 as one launch (stabnet_conv_unit_pair_fwd):
    -> (y1, y3); bit-identical to conv2d_packed of the two convolutions (splitk = 1).  residual [N,H,W,Cr]: its first N1 channels are
    read with a pixel stride of Cr."""
    x = dev_f32(x, "x")
    w3 = dev_f32(w3_ohwi, "w3")
    w1 = dev_f32(w1_ohwi, "w1")
    N, H, W, K1 = x.shape
    N1, N2 = w3.shape[0], w1.shape[0]
    assert tuple(w3.shape[1:]) == (1, 1, K1) and tuple(w1.shape[1:]) == (1, 1, N1)
    y3 = _out(out3, (N, H, W, N1), x)
    y1 = _out(out, (N, H, W, N2), x)
    L = _lib.lib()
    imgs = []
    for w, co, ci in ((w3, N1, K1), (w1, N2, N1)):
        img = torch.empty(int(L.stabnet_conv_weight_image_floats(co, 1, 1, ci)), dtype=torch.float32, device=x.device)
        _lib.call("stabnet_conv_weight_split_image", ptr(w), co, 1, 1, ci, ptr(img), stream_ptr(x.device), device=x.device)
        imgs.append(img)
    res_ld = 0
    if residual is not None:
        assert tuple(residual.shape[:3]) == (N, H, W) and residual.shape[3] >= N1
        res_ld = residual.shape[3]
    _lib.call("stabnet_conv_unit_pair_fwd", ptr(x), ptr(w3), ptr(imgs[0]), ptr(bias3), ptr(residual), res_ld, ptr(pre_scale), ptr(pre_shift),
              ptr(w1), ptr(imgs[1]), ptr(out_scale), ptr(out_shift), ptr(y3), ptr(y1), N, H, W, K1, N1, N2, int(relu_out),
              stream_ptr(x.device), device=x.device)
    return y1, y3


def conv3x3_conv1x1(x, w2_ohwi, mid_scale, mid_shift, w3_ohwi, bias3=None, residual=None, res_stride=1, stride=1, relu_out=False,
                    out_scale=None, out_shift=None, x_ch0=0, res_ch0=0, out=None):
    """The tail of a bottleneck unit as one launch (stabnet_conv3x3_conv1x1_fwd): conv2 3x3 (pad 1, `stride`) -> folded BN + ReLU
    -> conv3 1x1 with conv2d's epilogue.  x [N,H,W,Cx]: the conv reads channels x_ch0 .. x_ch0 + C of every pixel (Cx > C: the
    inference plan's merged shortcut|conv1 buffer); residual [N,rH,rW,Cr]: channels res_ch0 .. res_ch0 + Cout likewise."""
    x = dev_f32(x, "x")
    w2 = dev_f32(w2_ohwi, "w2")
    w3 = dev_f32(w3_ohwi, "w3")
    N, H, W, Cx = x.shape
    C = w2.shape[0]
    Cout = w3.shape[0]
    assert tuple(w2.shape) == (C, 3, 3, C) and tuple(w3.shape[1:]) == (1, 1, C) and x_ch0 + C <= Cx
    Ho = (H + 2 - 3) // stride + 1
    Wo = (W + 2 - 3) // stride + 1
    y = _out(out, (N, Ho, Wo, Cout), x)
    rH = rW = res_ld = 0
    rp = 0
    if residual is not None:
        residual = dev_f32(residual, "residual")
        rH, rW, res_ld = residual.shape[1], residual.shape[2], residual.shape[3]
        assert res_ch0 + Cout <= res_ld
        rp = residual.data_ptr() + 4 * res_ch0
    _lib.call("stabnet_conv3x3_conv1x1_fwd", x.data_ptr() + 4 * x_ch0, Cx, ptr(w2), ptr(mid_scale), ptr(mid_shift), ptr(w3),
              ptr(bias3), rp, rH, rW, res_stride, res_ld, ptr(out_scale), ptr(out_shift), ptr(y), N, H, W, C, Cout, stride,
              int(relu_out), stream_ptr(x.device), device=x.device)
    return y


def conv2d_wgrad(x, dy, w_shape, in_scale=None, in_shift=None, stride=1, pad=0, dw=None):
    """dW (OHWI) += d conv / d W; returns dw (zero-initialised when not given)."""
    x = dev_f32(x, "x")
    dy = dev_f32(dy, "dy")
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cw = w_shape
    assert Cw == Cin
    if dw is None:
        dw = torch.zeros(w_shape, dtype=torch.float32, device=x.device)
    nbytes = _lib.lib().stabnet_conv2d_wgrad_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.call("stabnet_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(in_scale), ptr(in_shift), N, H, W, Cin, Cout, KH, KW,
              stride, pad, ptr(ws), nbytes, stream_ptr(x.device), device=x.device)
    return dw


def conv2d_wgrad_bias(x, dy, w_shape, in_scale=None, in_shift=None, dw=None, db=None):
    """1x1 layers: (dW, d_bias) += gradients, the bias sums taken from the wgrad kernel's own pass over dy."""
    x = dev_f32(x, "x")
    dy = dev_f32(dy, "dy")
    N, H, W, Cin = x.shape
    Cout = w_shape[0]
    assert tuple(w_shape[1:]) == (1, 1, Cin)
    buf = torch.zeros(Cout * Cin + Cout, dtype=torch.float32, device=x.device)      # one allocation: d_bias sits behind dW
    if dw is not None:
        buf[:Cout * Cin] = dw.reshape(-1)
    if db is not None:
        buf[Cout * Cin:] = db
    nbytes = _lib.lib().stabnet_conv2d_wgrad_bias_workspace_bytes(N, H, W, Cin, Cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.call("stabnet_conv2d_wgrad_bias", ptr(x), ptr(dy), buf.data_ptr(), buf.data_ptr() + 4 * Cout * Cin, ptr(in_scale), ptr(in_shift),
              N, H, W, Cin, Cout, ptr(ws), nbytes, stream_ptr(x.device), device=x.device)
    return buf[:Cout * Cin].reshape(w_shape), buf[Cout * Cin:]


def conv2d_wgrad_rowrun(x, dy, w_shape, stride=1, pad=0, dw=None):
    """dW (OHWI [Cout,KH,KW,CinPad], CinPad >= Cin) += d conv / d W for an input whose channel count is not a multiple of 4
    (the 13-channel stem): the filter-row-run form the training step uses.  Pad channels of dw are not written."""
    x = dev_f32(x, "x")
    dy = dev_f32(dy, "dy")
    N, H, W, Cin = x.shape
    Cout, KH, KW, CinPad = w_shape
    if dw is None:
        dw = torch.zeros(w_shape, dtype=torch.float32, device=x.device)
    nbytes = _lib.lib().stabnet_conv2d_wgrad_rowrun_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.call("stabnet_conv2d_wgrad_rowrun", ptr(x), ptr(dy), ptr(dw), N, H, W, Cin, CinPad, Cout, KH, KW, stride, pad,
              ptr(ws), nbytes, stream_ptr(x.device), device=x.device)
    return dw


def conv2d_dgrad_workspace_bytes(x_shape, w_shape, stride=1, pad=0, split=False):
    """Bytes of scratch conv2d_dgrad (split=True: conv2d_dgrad_split) asks for."""
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w_shape
    fn = _lib.lib().stabnet_conv2d_dgrad_split_workspace_bytes if split else _lib.lib().stabnet_conv2d_dgrad_workspace_bytes
    return int(fn(N, H, W, Cin, Cout, KH, KW, stride, pad))


def conv2d_dgrad(dy, w_ohwi, x_shape, stride=1, pad=0, residual=None, out=None, workspace=None):
    dy = dev_f32(dy, "dy")
    w = dev_f32(w_ohwi, "w")
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w.shape
    dx = _out(out, x_shape, dy)
    ws, nbytes = _workspace(workspace, conv2d_dgrad_workspace_bytes(x_shape, w.shape, stride, pad), dy)
    _lib.call("stabnet_conv2d_dgrad", ptr(dy), ptr(w), ptr(dx), ptr(residual), N, H, W, Cin, Cout, KH, KW, stride, pad,
              ptr(ws), nbytes, stream_ptr(dy.device), device=dy.device)
    return dx


# ---- convolution backward in the forms a backward stage of the training step runs (the step's own launchers) ----------------

def _wgrad_layers_args(layers):
    """layers: [(geom, towers, dw_off, bias_off, bias_off2)] with geom = (N, H, W, Cin, Cout, KH, KW, stride, pad) and
    towers = [(x, dy, in_scale, in_shift)] per tower -> the host arrays of stabnet_conv2d_wgrad_layers."""
    import ctypes
    L, T = len(layers), len(layers[0][1])
    assert all(len(ly[0]) == 9 and len(ly[1]) == T for ly in layers)
    geom = (ctypes.c_int * (9 * L))(*[int(v) for ly in layers for v in ly[0]])
    tensors = (ctypes.c_void_p * (4 * T * L))(*[ptr(t) or None for ly in layers for tw in ly[1] for t in tw])
    dw_off = (ctypes.c_long * L)(*[int(ly[2]) for ly in layers])
    bias_off = (ctypes.c_long * (2 * L))(*[int(-1 if b is None else b) for ly in layers for b in ly[3:5]])
    return L, T, geom, tensors, dw_off, bias_off


def conv2d_wgrad_layers_workspace_bytes(layers):
    L, T, geom, _, _, bias_off = _wgrad_layers_args(layers)
    return int(_lib.lib().stabnet_conv2d_wgrad_layers_workspace_bytes(L, T, geom, bias_off))


def conv2d_wgrad_layers(layers, grads, workspace=None):
    """The weight (and fused bias) gradients of several layers over one or two towers, accumulated into the flat float32 buffer
    `grads` at each layer's offsets: one launch per layer, one shared reduce table (`layers` as _wgrad_layers_args takes them)."""
    L, T, geom, tensors, dw_off, bias_off = _wgrad_layers_args(layers)
    if workspace is None:
        workspace = torch.empty(max(conv2d_wgrad_layers_workspace_bytes(layers) // 4, 4), dtype=torch.float32, device=grads.device)
    _lib.call("stabnet_conv2d_wgrad_layers", L, T, geom, tensors, ptr(grads), grads.numel(), dw_off, bias_off, ptr(workspace),
              workspace.numel() * workspace.element_size(), stream_ptr(grads.device), device=grads.device)
    return grads


def pack_dgrad_weights_table(params, wt, entries):
    """entries: [(w_off, Cout, K, Cin, stride)] -> the dgrad weights of every entry, one after the other in `wt`, by one launch."""
    import ctypes
    L = len(entries)
    w_off = (ctypes.c_long * L)(*[int(e[0]) for e in entries])
    dims = (ctypes.c_int * (4 * L))(*[int(v) for e in entries for v in e[1:5]])
    _lib.call("stabnet_pack_dgrad_weights_table", ptr(params), params.numel(), ptr(wt), wt.numel(), L, w_off, dims,
              stream_ptr(wt.device), device=wt.device)
    return wt


def conv_weight_split_images_table(w_base, img_base, entries):
    """entries: [(w_off, img_off, Cout, K)] -> the three-term bf16 images of the [Cout][K] matrices at w_base + w_off, by one launch."""
    import ctypes
    L = len(entries)
    w_off = (ctypes.c_long * L)(*[int(e[0]) for e in entries])
    img_off = (ctypes.c_long * L)(*[int(e[1]) for e in entries])
    dims = (ctypes.c_int * (2 * L))(*[int(v) for e in entries for v in e[2:4]])
    _lib.call("stabnet_conv_weight_split_images_table", ptr(w_base), w_base.numel(), ptr(img_base), img_base.numel(), L, w_off, img_off,
              dims, stream_ptr(w_base.device), device=w_base.device)
    return img_base


def conv2d_dgrad_split(dy, w_ohwi, x_shape, stride=1, pad=0, residual=None, dx=None, workspace=None, out=None):
    """conv2d_dgrad as the training step runs it with split operands: -> (dx, packed), packed = True if the launch went to a packed
    split kernel (False: the exact-f32 kernels took it).  residual may be dx (given; `out` is another name of `dx`)."""
    import ctypes
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w_ohwi.shape
    assert dx is None or out is None, "dx and out name the same tensor: give one"
    if dx is None:                     # (a dx of any shape with x_shape's element count is taken as it is)
        dx = _out(out, x_shape, dy)
    nbytes = conv2d_dgrad_workspace_bytes(x_shape, w_ohwi.shape, stride, pad, split=True)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dy.device)
    route = ctypes.c_int(-1)
    _lib.call("stabnet_conv2d_dgrad_split", ptr(dy), ptr(w_ohwi), ptr(dx), ptr(residual), N, H, W, Cin, Cout, KH, KW, stride, pad,
              ptr(workspace), workspace.numel() * workspace.element_size(), ctypes.byref(route), stream_ptr(dy.device), device=dy.device)
    return dx, bool(route.value)


# ---- the non-convolution inference layers and the head, one operator per call (the launchers of the plan) ------------------

def pad_channels(x, y):
    """x [..., C] -> y [..., Cp] (given, Cp % 4 == 0): zeros in the pad channels."""
    C, Cp = x.shape[-1], y.shape[-1]
    _lib.call("stabnet_pad_channels", ptr(x), ptr(y), x.numel() // C, C, Cp, stream_ptr(x.device), device=x.device)
    return y


def stem_repack(w, out, cin):
    """w OHWI [Cout, KH, KW, CinPad] -> out [Cout, KH, roundup(KW * cin, 32)]."""
    Cout, KH, KW, CinPad = w.shape
    _lib.call("stabnet_stem_repack", ptr(w), ptr(out), Cout, KH, KW, CinPad, int(cin), stream_ptr(w.device), device=w.device)
    return out


def merge_vectors(b_sc, scale1, shift1, out):
    """-> out [4, depth + dbn] = [bias | scale | shift | floor] of a merged (shortcut | conv1) launch."""
    _lib.call("stabnet_merge_vectors", ptr(b_sc), ptr(scale1), ptr(shift1), b_sc.numel(), scale1.numel(), ptr(out),
              stream_ptr(out.device), device=out.device)
    return out


def bn_fold(gamma, beta, mean, var, eps, scale, shift):
    _lib.call("stabnet_bn_fold", ptr(gamma), ptr(beta), ptr(mean), ptr(var), float(eps), gamma.numel(), ptr(scale), ptr(shift),
              stream_ptr(gamma.device), device=gamma.device)
    return scale, shift


def max_pool_fwd(x, y, k, stride, pt, pl, scale=None, shift=None):
    """x [N,H,W,C] -> y [N,Ho,Wo,C] (Ho, Wo are taken from y); scale, shift: the consumer's folded BN + ReLU on the pooled value."""
    N, H, W, C = x.shape
    _lib.call("stabnet_max_pool_fwd", ptr(x), ptr(y), N, H, W, C, y.shape[1], y.shape[2], k, stride, pt, pl, ptr(scale), ptr(shift),
              stream_ptr(x.device), device=x.device)
    return y


def gap_partial_floats(N, HW, C):
    return int(_lib.lib().stabnet_gap_partial_floats(N, HW, C))


def gap_bn_relu(x, scale, shift, out, partial=None):
    """x [N,HW,C] -> out [N,C] = mean over HW of relu(x * scale + shift)."""
    N, HW, C = x.shape
    if partial is None:
        partial = empty((gap_partial_floats(N, HW, C),), x)
    _lib.call("stabnet_gap_bn_relu", ptr(x), ptr(scale), ptr(shift), N, HW, C, ptr(out), ptr(partial), partial.numel(),
              stream_ptr(x.device), device=x.device)
    return out


def fc_fwd(x, w, b, y, relu):
    """y [M,Nout] = act(x [M,K] w [Nout,K]^T + b); b may be None."""
    M, K = x.shape
    _lib.call("stabnet_fc_fwd", ptr(x), ptr(w), ptr(b), ptr(y), M, K, w.shape[0], int(bool(relu)), stream_ptr(x.device), device=x.device)
    return y


def head_fused_supported(N, C, fc_dims):
    import ctypes
    dims = (ctypes.c_int * 5)(*[int(d) for d in fc_dims])
    return bool(_lib.lib().stabnet_head_fused_supported(N, C, ctypes.addressof(dims)))


def head_gap_partial_floats(N, HW, C):
    return int(_lib.lib().stabnet_head_gap_partial_floats(N, HW, C))


def head_gap_fc1(x, scale, shift, w, b, y, gap_out=None, partial=None):
    """x [N,HW,C] -> y [N,Nout] = relu(fc_1(mean over HW of relu(x * scale + shift))); gap_out [N,C] (optional): the pooled feature."""
    N, HW, C = x.shape
    if partial is None:
        partial = empty((head_gap_partial_floats(N, HW, C),), x)
    _lib.call("stabnet_head_gap_fc1", ptr(x), ptr(scale), ptr(shift), N, HW, C, ptr(partial), partial.numel(), ptr(gap_out), ptr(w),
              ptr(b), ptr(y), w.shape[0], stream_ptr(x.device), device=x.device)
    return y


def head_theta_mesh(x, w, b, theta, grid_h=1, grid_w=1, do_crop_rate=1.0, Hs=None, head_adv=None, depth=1, prefetch_src=None,
                    prefetch_hw=(0, 0), prefetch_ptr=None):
    """x [N,512] -> theta [N,n_theta] (output layer); Hs [N,gh,gw,9] (optional): the mesh homographies of that theta; head_adv
    (optional, int32 [1]): advanced by one modulo depth; prefetch_src [N,H,W] (optional): a frame the launch only reads
    (prefetch_ptr: a raw address in its place)."""
    N, K = x.shape
    pf = prefetch_ptr if prefetch_ptr is not None else ptr(prefetch_src)
    _lib.call("stabnet_head_theta_mesh", ptr(x), ptr(w), ptr(b), N, K, w.shape[0], ptr(theta), int(grid_h), int(grid_w),
              float(do_crop_rate), ptr(Hs), ptr(head_adv), int(depth), pf, int(prefetch_hw[0]), int(prefetch_hw[1]),
              stream_ptr(x.device), device=x.device)
    return theta
