"""Host mirror of the reference's warp operators over the C ABI (same names, argument meaning, returns).

  transformer(U, theta)            spatial_transformer3.py:19   -> (output, black_pix, img)
  interpolate(im, x, y, out_size)  spatial_transformer.py:200   -> output
  get_4_pts(theta, batch_size)     s_net_bundle_nobm.py:29      -> (pts1, pts2)

Tensors are torch CUDA(HIP) float32, NHWC.  No CPU fallback."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._tensor import dev_f32, empty, ptr, stream_ptr
from .config import Config, v2_93


def get_4_pts(theta: torch.Tensor, batch_size=None, cfg: Config = v2_93, with_Hs: bool = False):
    theta = dev_f32(theta, "theta")
    N = theta.shape[0]
    gh, gw = cfg.grid_h, cfg.grid_w
    assert theta.shape[1] == (gh + 1) * (gw + 1) * 2
    pts2 = empty((N, gh + 1, gw + 1, 2), theta)
    Hs = empty((N, gh, gw, 9), theta)
    pts1 = empty((N, gh, gw, 8), theta)      # per cell [xTL,xTR,xBL,xBR,yTL,yTR,yBL,yBR] (s_net_bundle_nobm.py:65-66)
    _lib.call("stabnet_get_4_pts", ptr(theta), N, gh, gw, cfg.do_crop_rate, ptr(pts1), ptr(pts2), ptr(Hs),
              stream_ptr(theta.device), device=theta.device)
    if with_Hs:
        return pts1, pts2, Hs
    return pts1, pts2


def transformer(U: torch.Tensor, theta: torch.Tensor, name="SpatialTransformer", cfg: Config = v2_93,
                return_Hs: bool = False):
    """U [N,H,W,C]; theta = pts2 [N,gh+1,gw+1,2] -> (output [N,H,W,C], black_pix [N,H,W], img [N,H,W,2])."""
    U = dev_f32(U, "U")
    pts2 = dev_f32(theta, "theta")
    N, H, W, C = U.shape
    out = empty((N, H, W, C), U)
    black = empty((N, H, W), U)
    xm = empty((N, H, W), U)
    ym = empty((N, H, W), U)
    Hs = empty((N, cfg.grid_h, cfg.grid_w, 9), U)
    _lib.call("stabnet_transformer_fwd", ptr(pts2), ptr(U), N, H, W, C, cfg.grid_h, cfg.grid_w, ptr(out), ptr(black),
              ptr(xm), ptr(ym), ptr(Hs), stream_ptr(U.device), device=U.device)
    img = empty((N, H, W, 2), U)                            # img = [x_map, y_map] (spatial_transformer3.py:295)
    _lib.call("stabnet_interleave2", ptr(xm), ptr(ym), N * H * W, ptr(img), stream_ptr(U.device), device=U.device)
    if return_Hs:
        return out, black, img, Hs
    return out, black, img


def warp_from_theta(U: torch.Tensor, theta: torch.Tensor, cfg: Config = v2_93):
    """Fused get_4_pts + transformer on the raw regressor output theta [N,50].
    -> dict(output, black_pix, x_map, y_map, Hs, pts2) with the deploy tensor shapes (deploy_bundle.py:48-56)."""
    U = dev_f32(U, "U")
    theta = dev_f32(theta, "theta")
    N, H, W, C = U.shape
    out = empty((N, H, W, C), U)
    black = empty((N, H, W), U)
    xm = empty((N, H, W, 1), U)
    ym = empty((N, H, W, 1), U)
    Hs = empty((N, cfg.grid_h, cfg.grid_w, 9), U)
    pts2 = empty((N, cfg.grid_h + 1, cfg.grid_w + 1, 2), U)
    _lib.call("stabnet_warp_fwd", ptr(theta), ptr(U), N, H, W, C, cfg.grid_h, cfg.grid_w, cfg.do_crop_rate, ptr(out),
              ptr(black), ptr(xm), ptr(ym), ptr(Hs), ptr(pts2), stream_ptr(U.device), device=U.device)
    return {"output": out, "black_pix": black, "x_map": xm, "y_map": ym, "Hs": Hs, "pts2": pts2}


def slice_channel(x: torch.Tensor, c: int) -> torch.Tensor:
    """x [..., C] -> x[..., c:c+1] as its own contiguous tensor (x_tensor[..., 12:13], s_net_bundle_nobm.py:281)."""
    x = dev_f32(x, "x")
    C = x.shape[-1]
    out = empty(tuple(x.shape[:-1]) + (1,), x)
    _lib.call("stabnet_slice_channel", ptr(x), x.numel() // C, C, int(c), ptr(out), stream_ptr(x.device), device=x.device)
    return out


def maps_from_Hs(U: torch.Tensor, Hs: torch.Tensor, cfg: Config = v2_93):
    U = dev_f32(U, "U")
    Hs = dev_f32(Hs, "Hs")
    N, H, W, C = U.shape
    out = empty((N, H, W, C), U)
    black = empty((N, H, W), U)
    xm = empty((N, H, W), U)
    ym = empty((N, H, W), U)
    _lib.call("stabnet_maps_from_hs_fwd", ptr(Hs), ptr(U), N, H, W, C, cfg.grid_h, cfg.grid_w, ptr(out), ptr(black),
              ptr(xm), ptr(ym), stream_ptr(U.device), device=U.device)
    return out, black, xm, ym


def interpolate(im: torch.Tensor, x: torch.Tensor, y: torch.Tensor, out_size=None, name="SpatialInterpolate"):
    """im [N,H,W,C]; x,y [N,H,W,1] (or [N,H,W]) normalised coords -> [N,H,W,C]."""
    im = dev_f32(im, "im")
    x = dev_f32(x, "x")
    y = dev_f32(y, "y")
    N, H, W, C = im.shape
    assert x.numel() == N * H * W and y.numel() == N * H * W
    out = empty((N, H, W, C), im)
    _lib.call("stabnet_interp_fwd", ptr(im), ptr(x), ptr(y), N, H, W, C, ptr(out), stream_ptr(im.device), device=im.device)
    return out


INTERPS = ("linear", "cubic")


def check_interp(interp, what):
    """interp: "linear" (cv2.INTER_LINEAR, the reference's) or "cubic" (cv2.INTER_CUBIC: 16 taps, csrc/remap.hip remap_cubic_kernel)."""
    if interp not in INTERPS:
        raise _lib.StabnetError("%s: interp must be one of %s, got %r" % (what, list(INTERPS), interp))
    return interp == "cubic"


def warpRevBundle2(img: torch.Tensor, x_map: torch.Tensor, y_map: torch.Tensor, rate: int = 4, return_maps: bool = False,
                   interp: str = "linear"):
    """deploy_bundle.py:136-146 on the device.  img uint8 [N,H,W,3] (or [H,W,3]); x_map, y_map [N,H,W(,1)] normalised.
    interp="cubic": cv2.remap's INTER_CUBIC in place of INTER_LINEAR (stabnet_warp_rev_bundle2_cubic at the network's own size)."""
    cubic = check_interp(interp, "warpRevBundle2")
    squeeze = img.dim() == 3
    if squeeze:
        img = img[None]
    if not img.is_cuda or img.dtype != torch.uint8:
        raise _lib.StabnetError("warpRevBundle2: img must be a uint8 tensor on the GPU")
    img = img.contiguous()
    N, H, W, C = img.shape
    xm = dev_f32(x_map, "x_map").reshape(N, H, W)
    ym = dev_f32(y_map, "y_map").reshape(N, H, W)
    out = torch.empty_like(img)
    ws = torch.empty(2 * N * (H // rate) * (W // rate), dtype=torch.float32, device=img.device)
    px = empty((N, H, W), xm) if return_maps else None
    py = empty((N, H, W), xm) if return_maps else None
    if cubic:
        _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(img), N, H, W, C, W * C, ptr(xm), ptr(ym), H, W, int(rate), 0, None, H, W, ptr(out), None,
                  ptr(ws), ptr(px), ptr(py), stream_ptr(img.device), 0, device=img.device)
        if squeeze:
            out = out[0]
        return (out, px, py) if return_maps else out
    _lib.call("stabnet_warp_rev_bundle2", ptr(img), ptr(xm), ptr(ym), N, H, W, C, rate, ptr(out), ptr(ws), ptr(px), ptr(py),
              stream_ptr(img.device), device=img.device)
    if squeeze:
        out = out[0]
    return (out, px, py) if return_maps else out


def _check_src_u8(u8, what):
    """uint8 GPU frames [N,SH,SW,C] / [SH,SW,C] / [SH,SW] -> (tensor [N,SH,SW,C] with dense pixels, row stride in bytes, the shape to
    hand back).  Rows may be strided (a view of a wider buffer is read where it lies), as in ingest.FrameIngest._check."""
    if not isinstance(u8, torch.Tensor) or not u8.is_cuda:
        raise _lib.StabnetError("%s: expected a uint8 tensor on the GPU (there is no CPU fallback)" % what)
    if u8.dtype != torch.uint8:
        raise _lib.StabnetError("%s: expected uint8, got %s" % (what, u8.dtype))
    shape = tuple(u8.shape)
    if u8.dim() == 2:
        u8 = u8[None, :, :, None]
    elif u8.dim() == 3:
        u8 = u8[None]
    if u8.dim() != 4 or u8.shape[3] not in (1, 3) or min(u8.shape) < 1:
        raise _lib.StabnetError("%s: expected [N, SH, SW, C] / [SH, SW, C] / [SH, SW] with C = 3 (BGR) or 1 (grey), got %s" % (what, list(shape)))
    n, sh, sw, c = u8.shape
    dense = u8.stride(3) == 1 and u8.stride(2) == c and u8.stride(1) >= sw * c and (n == 1 or u8.stride(0) == sh * u8.stride(1))
    if not dense:
        u8 = u8.contiguous()
    return u8, u8.stride(1), shape


def _check_maps(x_map, y_map, N, dev, rate, what):
    """The network-size maps [N,H,W(,1)] / [H,W] of a batch of N frames on `dev` -> (x_map, y_map as float32 tensors, H, W)."""
    xm, ym = dev_f32(x_map, "x_map"), dev_f32(y_map, "y_map")
    if xm.device != dev or ym.device != dev:
        raise _lib.StabnetError("%s: maps on %s / %s, frame on %s" % (what, xm.device, ym.device, dev))
    ms = tuple(xm.shape)
    if xm.dim() == 4 and ms[3] == 1:
        ms = ms[:3]
    elif xm.dim() == 3 and ms[2] == 1 and ms[0] != N:
        ms = (1,) + ms[:2]
    elif xm.dim() == 2:
        ms = (1,) + ms
    if len(ms) != 3 or ms[0] != N or ym.numel() != xm.numel():
        raise _lib.StabnetError("%s: maps must be [%d, H, W] like the frames' batch, got %s and %s" % (what, N, list(xm.shape), list(ym.shape)))
    H, W = ms[1], ms[2]
    if rate < 1 or H // rate < 1 or W // rate < 1:
        raise _lib.StabnetError("%s: maps %dx%d leave nothing at rate %d" % (what, H, W, rate))
    return xm, ym, H, W


def _check_out_and_count(out, black_count, N, OH, OW, C, dev, what):
    """The optional `out` (uint8, N*OH*OW*C elements; allocated when None) and `black_count` (int32, N*OH*OW) of a remap on `dev` -> out."""
    if out is None:
        out = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or out.numel() != N * OH * OW * C or not out.is_contiguous():
        raise _lib.StabnetError("%s: out must be a contiguous uint8 tensor of %s on %s" % (what, [N, OH, OW, C], dev))
    if black_count is not None and (not isinstance(black_count, torch.Tensor) or black_count.device != dev or black_count.dtype != torch.int32
                                    or black_count.numel() != N * OH * OW or not black_count.is_contiguous()):
        raise _lib.StabnetError("%s: black_count must be a contiguous int32 tensor of %s on %s" % (what, [N, OH, OW], dev))
    return out


def warpRevBundle2_src(src_u8: torch.Tensor, x_map: torch.Tensor, y_map: torch.Tensor, rate: int = 4, black_count: torch.Tensor = None,
                       out: torch.Tensor = None, return_maps: bool = False, prof=None, interp: str = "linear"):
    """warpRevBundle2 at SOURCE resolution (csrc/remap.hip, stabnet_warp_rev_bundle2_src): the frame as read -- uint8 [N,SH,SW,C] /
    [SH,SW,C] / [SH,SW], any size, rows may be strided -- remapped by the network-size maps x_map, y_map [N,H,W(,1)] / [H,W].
    -> uint8 of src_u8's shape (with return_maps: (out, px, py), the float32 [N,SH,SW] source-pixel coordinates).
    black_count: optional int32 [N,SH,SW] (or [SH,SW] for one frame), += 1 where the frame does not cover the pixel -- what
    max_inscribed_rect reads.  out: optional contiguous uint8 tensor of the result's size.  interp: "linear" or "cubic" (INTER_CUBIC,
    stabnet_warp_rev_bundle2_cubic; coordinates and black_count are the same).  Nothing synchronises."""
    what = "warpRevBundle2_src"
    cubic = check_interp(interp, what)
    u8, stride, shape = _check_src_u8(src_u8, what)
    N, SH, SW, C = u8.shape
    dev = u8.device
    xm, ym, H, W = _check_maps(x_map, y_map, N, dev, rate, what)
    out = _check_out_and_count(out, black_count, N, SH, SW, C, dev, what)
    ws = torch.empty(2 * N * (H // rate) * (W // rate), dtype=torch.float32, device=dev)
    px = empty((N, SH, SW), xm) if return_maps else None
    py = empty((N, SH, SW), xm) if return_maps else None
    if cubic:
        _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(u8), N, SH, SW, C, stride, ptr(xm), ptr(ym), H, W, int(rate), 0, None, SH, SW, ptr(out),
                  ptr(black_count), ptr(ws), ptr(px), ptr(py), stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)
    else:
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(u8), N, SH, SW, C, stride, ptr(xm), ptr(ym), H, W, int(rate), ptr(out), ptr(black_count),
                  ptr(ws), ptr(px), ptr(py), stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)
    res = out.view(shape)
    return (res, px, py) if return_maps else res


def ratio_window(SH: int, SW: int, r: float):
    """(y0, x0, wh, ww): the centred window of an SH x SW frame that keeps `r` of each side, 0 < r <= 1."""
    r = float(r)
    if not 0.0 < r <= 1.0:
        raise ValueError("ratio_window: r must lie in (0, 1], got %r" % (r,))
    wh, ww = SH * r, SW * r
    return ((SH - wh) / 2, (SW - ww) / 2, wh, ww)


def fit_window(rect, OH: int, OW: int):
    """(y0, x0, wh, ww): the largest window of the output's aspect ratio OW : OH inside rect = [i0, j0, i1, j1] (inclusive, as
    max_inscribed_rect returns it), centred in it.  Plain Python floats."""
    i0, j0, i1, j1 = (int(v) for v in rect)
    rh, rw = i1 - i0 + 1, j1 - j0 + 1
    if rh < 1 or rw < 1 or OH < 1 or OW < 1:
        raise ValueError("fit_window: empty rectangle %r or output %dx%d" % (list(rect), OH, OW))
    if rw * OH > rh * OW:                                # the rectangle is wider than the output: its height binds
        wh, ww = float(rh), rh * OW / OH
    else:
        wh, ww = rw * OH / OW, float(rw)
    return (i0 + (rh - wh) / 2, j0 + (rw - ww) / 2, wh, ww)


def _check_window(window, what):
    try:
        win = tuple(float(v) for v in window)
    except (TypeError, ValueError):
        win = ()
    if len(win) != 4:
        raise _lib.StabnetError("%s: window must be four numbers (y0, x0, wh, ww), got %r" % (what, window))
    return (ctypes.c_double * 4)(*win)


def warpRevBundle2_win(src_u8: torch.Tensor, x_map: torch.Tensor, y_map: torch.Tensor, window, out_size=None, rate: int = 4,
                       black_count: torch.Tensor = None, out: torch.Tensor = None, return_maps: bool = False, prof=None,
                       interp: str = "linear"):
    """warpRevBundle2_src through a WINDOW of the stabilised frame (csrc/remap.hip, stabnet_warp_rev_bundle2_win): crop and zoom in the
    one gather.  window = (y0, x0, wh, ww) in pixel-edge units of the stabilised frame at the source's size (the whole frame is
    (0, 0, SH, SW); ratio_window / fit_window make one); out_size = (OH, OW), default the source's size.  A float64 tensor [4] or [N,4]
    on the frames' device is a window in DEVICE memory (stabnet_warp_rev_bundle2_win_dev: the kernels load it when they run, so an
    earlier launch on the stream -- AdaptiveFill.update -- may have written it; values the host entry would refuse give the whole frame).
    -> uint8 [N,OH,OW,C] / [OH,OW,C] / [OH,OW] after src_u8's layout (with return_maps: (out, px, py), float32 [N,OH,OW]).
    black_count: optional int32 [N,OH,OW], += 1 where the frame does not cover the OUTPUT pixel.  interp: "linear" or "cubic"
    (INTER_CUBIC, stabnet_warp_rev_bundle2_cubic with window_kind 1 / 2).  Nothing synchronises."""
    what = "warpRevBundle2_win"
    cubic = check_interp(interp, what)
    u8, stride, shape = _check_src_u8(src_u8, what)
    N, SH, SW, C = u8.shape
    dev = u8.device
    entry = "stabnet_warp_rev_bundle2_win"
    if isinstance(window, torch.Tensor):
        if window.dtype != torch.float64 or window.device != dev or tuple(window.shape) not in ((4,), (N, 4)):
            raise _lib.StabnetError("%s: a window tensor must be float64 [4] or [%d, 4] on %s, got %s %s on %s"
                                    % (what, N, dev, window.dtype, list(window.shape), window.device))
        win_t = window.expand(N, 4).contiguous()             # (kept alive until the launch is enqueued)
        win, entry = ptr(win_t), entry + "_dev"
    else:
        win = _check_window(window, what)
    OH, OW = (SH, SW) if out_size is None else (int(out_size[0]), int(out_size[1]))
    xm, ym, H, W = _check_maps(x_map, y_map, N, dev, rate, what)
    if OH < 1 or OW < 1:
        raise _lib.StabnetError("%s: out_size %dx%d is empty" % (what, OH, OW))
    out = _check_out_and_count(out, black_count, N, OH, OW, C, dev, what)
    ws = torch.empty(2 * N * (H // rate) * (W // rate), dtype=torch.float32, device=dev)
    px = empty((N, OH, OW), xm) if return_maps else None
    py = empty((N, OH, OW), xm) if return_maps else None
    if cubic:
        _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(u8), N, SH, SW, C, stride, ptr(xm), ptr(ym), H, W, int(rate),
                  2 if entry.endswith("_dev") else 1, win, OH, OW, ptr(out), ptr(black_count), ptr(ws), ptr(px), ptr(py), stream_ptr(dev),
                  prof.handle if prof is not None else 0, device=dev)
    else:
        _lib.call(entry, ptr(u8), N, SH, SW, C, stride, ptr(xm), ptr(ym), H, W, int(rate), win, OH, OW, ptr(out),
                  ptr(black_count), ptr(ws), ptr(px), ptr(py), stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)
    res = out.view({2: (OH, OW), 3: (OH, OW, C), 4: (N, OH, OW, C)}[len(shape)])
    return (res, px, py) if return_maps else res


def i420_frame_bytes(SH: int, SW: int, planes: int = 3) -> int:
    """Bytes of one planar frame: the Y plane, and with planes == 3 the U and V planes of a 4:2:0 frame behind it."""
    return SH * SW if planes == 1 else SH * SW * 3 // 2


def warpRevBundle2_i420(src_u8: torch.Tensor, x_map: torch.Tensor, y_map: torch.Tensor, size, planes: int = 3, window=None, out_size=None,
                        border_y: int = 0, rate: int = 4, black_count: torch.Tensor = None, out: torch.Tensor = None,
                        workspace: torch.Tensor = None, prof=None, interp: str = "linear"):
    """warpRevBundle2_win of planar YUV 4:2:0 frames as a Y4M stream carries them (csrc/remap.hip, stabnet_warp_rev_bundle2_i420): no
    colour conversion, the Y plane and the two half-size chroma planes are warped as the single-channel images they are, in one gather
    launch.  src_u8: uint8 on the GPU, [N, B] or [B] with B >= the frame's bytes (i420_frame_bytes(SH, SW, planes)): per frame Y [SH,SW],
    then U, V [SH/2,SW/2], dense, at any byte alignment; size = (SH, SW); planes = 3, or 1 for Y only (Cmono).  window = (y0, x0, wh, ww)
    in pixel-edge units of the stabilised LUMA frame (host numbers; None: the whole frame), out_size = (OH, OW), default the source's.
    A tap outside a plane reads border_y (Y; 16 for a limited-range stream) or 128 (U, V).  black_count: optional int32 [N,OH,OW], += 1
    where the frame does not cover the luma output pixel.  out: optional contiguous uint8 tensor of N * i420_frame_bytes(OH, OW, planes)
    elements; workspace: optional float32 tensor of 2*N*(H//rate)*(W//rate) elements.  With both given nothing allocates, and nothing
    ever synchronises.  interp: "linear" or "cubic" (INTER_CUBIC on every plane, stabnet_warp_rev_bundle2_i420_cubic).
    -> uint8 [N, bytes] ([bytes] for a 1-D source)."""
    what = "warpRevBundle2_i420"
    cubic = check_interp(interp, what)
    if not isinstance(src_u8, torch.Tensor) or not src_u8.is_cuda:
        raise _lib.StabnetError("%s: expected a uint8 tensor on the GPU (there is no CPU fallback)" % what)
    if src_u8.dtype != torch.uint8:
        raise _lib.StabnetError("%s: expected uint8, got %s" % (what, src_u8.dtype))
    try:
        SH, SW = int(size[0]), int(size[1])
    except (TypeError, ValueError, IndexError):
        raise _lib.StabnetError("%s: size must be (SH, SW), got %r" % (what, size))
    if planes not in (1, 3) or SH < 1 or SW < 1 or (planes == 3 and (SH % 2 or SW % 2)):
        raise _lib.StabnetError("%s: planes must be 1 or 3 and a 4:2:0 frame has even sides, got planes %r, size %dx%d" % (what, planes, SH, SW))
    flat = src_u8.dim() == 1
    u8 = src_u8[None] if flat else src_u8
    need = i420_frame_bytes(SH, SW, planes)
    if u8.dim() != 2 or u8.stride(1) != 1 or u8.shape[1] < need or (u8.shape[0] > 1 and u8.stride(0) < need):
        raise _lib.StabnetError("%s: expected [N, >= %d] or [>= %d] dense bytes per frame, got %s" % (what, need, need, list(src_u8.shape)))
    N, dev = u8.shape[0], u8.device
    stride = u8.stride(0) if N > 1 else u8.shape[1]
    win = None if window is None else _check_window(window, what)
    OH, OW = (SH, SW) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if OH < 1 or OW < 1 or (planes == 3 and (OH % 2 or OW % 2)):
        raise _lib.StabnetError("%s: out_size %dx%d is empty or odd" % (what, OH, OW))
    xm, ym, H, W = _check_maps(x_map, y_map, N, dev, rate, what)
    obytes = i420_frame_bytes(OH, OW, planes)
    if out is None:
        out = torch.empty((N, obytes), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or out.numel() != N * obytes or not out.is_contiguous():
        raise _lib.StabnetError("%s: out must be a contiguous uint8 tensor of %s on %s" % (what, [N, obytes], dev))
    if black_count is not None and (not isinstance(black_count, torch.Tensor) or black_count.device != dev or black_count.dtype != torch.int32
                                    or black_count.numel() != N * OH * OW or not black_count.is_contiguous()):
        raise _lib.StabnetError("%s: black_count must be a contiguous int32 tensor of %s on %s" % (what, [N, OH, OW], dev))
    n_ws = 2 * N * (H // rate) * (W // rate)
    if workspace is None:
        workspace = torch.empty(n_ws, dtype=torch.float32, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.float32 or workspace.numel() < n_ws \
            or not workspace.is_contiguous():
        raise _lib.StabnetError("%s: workspace must be a contiguous float32 tensor of >= %d elements on %s" % (what, n_ws, dev))
    _lib.call("stabnet_warp_rev_bundle2_i420_cubic" if cubic else "stabnet_warp_rev_bundle2_i420", ptr(u8), N, SH, SW, int(planes), stride,
              ptr(xm), ptr(ym), H, W, int(rate), win, OH, OW, int(border_y), ptr(out), ptr(black_count), ptr(workspace), stream_ptr(dev),
              prof.handle if prof is not None else 0, device=dev)
    return out.view(obytes) if flat else out.view(N, obytes)


def check_fill_params(r_min=0.5, up=0.002, margin_q=8, SH=None, SW=None):
    """The ranges stabnet_fill_window_update accepts, checked on the host (ValueError): r_min in (0, 1], up finite and >= 0, margin_q an
    integer in 0 .. 16 * min(SH, SW) (the upper end only when the size is given).  -> (float r_min, float up, int margin_q)."""
    try:
        r_min, up, mq = float(r_min), float(up), int(margin_q)
    except (TypeError, ValueError):
        raise ValueError("adaptive fill: r_min, up, margin_q must be numbers, got %r, %r, %r" % (r_min, up, margin_q))
    if not 0.0 < r_min <= 1.0:
        raise ValueError("adaptive fill: r_min must lie in (0, 1], got %r" % (r_min,))
    if not (up >= 0.0 and up != float("inf")):
        raise ValueError("adaptive fill: up must be finite and >= 0, got %r" % (up,))
    if mq != margin_q or mq < 0 or (SH is not None and mq > 16 * min(int(SH), int(SW))):
        raise ValueError("adaptive fill: margin_q must be an integer in 0 .. 16 * min(SH, SW), got %r" % (margin_q,))
    return r_min, up, mq


def fill_window_update(x_map: torch.Tensor, y_map: torch.Tensor, SH: int, SW: int, state: torch.Tensor, window: torch.Tensor,
                       stats: torch.Tensor, r_min: float = 0.5, up: float = 0.002, margin_q: int = 8, rate: int = 4,
                       workspace: torch.Tensor = None):
    """The adaptive window of one frame per stream (csrc/remap.hip, stabnet_fill_window_update): from the network-size maps x_map, y_map
    [N,H,W(,1)] / [H,W] of the frame, the largest centred window of the SH x SW stabilised frame that reads no small-map node whose
    coordinate leaves the frame shrunk by margin_q / 32 px; zooming in at once, back out by at most `up` per call, never below r_min.
    state float64 [N] (the previous ratio; 1.0 at the start of a clip) is advanced, window float64 [N,4] = (y0, x0, wh, ww) and
    stats int32 [N,2] = (key, bad nodes) are written; r_safe = 1 if key >= h * w else key / (h * w).  All on the maps' device;
    nothing synchronises.  -> window."""
    what = "fill_window_update"
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float64 or state.dim() != 1 or not state.is_contiguous():
        raise _lib.StabnetError("%s: state must be a contiguous float64 tensor [N] on the GPU (there is no CPU fallback)" % what)
    N, dev = state.numel(), state.device
    xm, ym, H, W = _check_maps(x_map, y_map, N, dev, rate, what)
    for t, dt, shape, name in ((window, torch.float64, (N, 4), "window"), (stats, torch.int32, (N, 2), "stats")):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.StabnetError("%s: %s must be a contiguous %s tensor %s on %s" % (what, name, dt, list(shape), dev))
    n_ws = 2 * N * (H // rate) * (W // rate)
    if workspace is None:
        workspace = torch.empty(n_ws, dtype=torch.float32, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.float32 or workspace.numel() < n_ws \
            or not workspace.is_contiguous():
        raise _lib.StabnetError("%s: workspace must be a contiguous float32 tensor of >= %d elements on %s" % (what, n_ws, dev))
    _lib.call("stabnet_fill_window_update", ptr(xm), ptr(ym), N, H, W, int(rate), int(SH), int(SW), float(r_min), float(up), int(margin_q),
              ptr(state), ptr(window), ptr(stats), ptr(workspace), stream_ptr(dev), device=dev)
    return window


class AdaptiveFill:
    """The per-frame window of adaptive borderless output for N streams of SH x SW kept frames: `state` float64 [N], `window` float64
    [N,4], `stats` int32 [N,2] on `device`.  reset() at the start of a clip; update(x_map, y_map) per frame, in frame order, on the
    stream that carries the frame's launches -> window, which warpRevBundle2_win takes as it is.  No host round trip."""

    def __init__(self, N: int, SH: int, SW: int, r_min: float = 0.5, up: float = 0.002, margin_q: int = 8, device="cuda", rate: int = 4):
        self.r_min, self.up, self.margin_q = check_fill_params(r_min, up, margin_q, SH, SW)
        self.N, self.SH, self.SW, self.rate = int(N), int(SH), int(SW), int(rate)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.StabnetError("AdaptiveFill: the window lives on the GPU (there is no CPU fallback), got device %s" % dev)
        self.state = torch.ones(self.N, dtype=torch.float64, device=dev)
        self.window = torch.tensor([ratio_window(SH, SW, 1.0)] * self.N, dtype=torch.float64, device=dev)
        self.stats = torch.zeros((self.N, 2), dtype=torch.int32, device=dev)

    def reset(self):
        self.state.fill_(1.0)

    def update(self, x_map: torch.Tensor, y_map: torch.Tensor):
        return fill_window_update(x_map, y_map, self.SH, self.SW, self.state, self.window, self.stats, self.r_min, self.up, self.margin_q,
                                  self.rate)


def cvt_train2img(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """deploy_bundle.py:75 on the device: uint8((x + 0.5) * 255), clipped; same shape as x."""
    x = dev_f32(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if out.dtype != torch.uint8 or not out.is_cuda or out.numel() != x.numel() or not out.is_contiguous():
        raise _lib.StabnetError("cvt_train2img: out must be a contiguous uint8 GPU tensor of x's size")
    _lib.call("stabnet_cvt_train2img", ptr(x), ptr(out), x.numel(), stream_ptr(x.device), device=x.device)
    return out


def black_accumulate(black: torch.Tensor, all_black: torch.Tensor):
    """all_black (int32, same numel) += round(black)   (deploy_bundle.py:291)."""
    black = dev_f32(black, "black")
    assert all_black.dtype == torch.int32 and all_black.is_cuda and all_black.numel() == black.numel()
    _lib.call("stabnet_black_accumulate", ptr(black), ptr(all_black), black.numel(), stream_ptr(black.device),
              device=black.device)
    return all_black


def max_inscribed_rect(all_black: torch.Tensor, step: int = 10):
    """deploy_bundle.py:344-366 on the device.  all_black int32 [H,W] -> ([i, j, hh, ww], area) as Python ints
    (([], 0) when there is no free start pixel).  Synchronises (one 20-byte read-back per video)."""
    assert all_black.dtype == torch.int32 and all_black.is_cuda and all_black.dim() == 2
    all_black = all_black.contiguous()
    H, W = all_black.shape
    nbytes = _lib.lib().stabnet_crop_search_workspace_bytes(H, W, step)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=all_black.device)
    ans = torch.empty(5, dtype=torch.int32, device=all_black.device)
    _lib.call("stabnet_crop_search", ptr(all_black), H, W, step, ptr(ans), ptr(ws), ws.numel() * 8,
              stream_ptr(all_black.device), device=all_black.device)
    a = ans.cpu().tolist()
    return (a[:4], a[4]) if a[4] > 0 else ([], 0)
