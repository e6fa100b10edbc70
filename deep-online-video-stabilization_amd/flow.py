"""TV-L1 optical flow on the device (csrc/tvl1.hip): what fills a record's `flow`.  Zach / Pock / Bischof in the IPOL formulation
with a fixed number of inner iterations, no median filter, bilinear warps and a pyramid factor of 2 -- every step a deterministic
float32 stencil, bit for bit tests/tvl1_model.py.  The iteration runs fused (several sweeps per launch, temporal blocking in LDS)
unless the environment holds STABNET_TVL1_FUSED=0 (one launch per sweep; the same bits)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import StabnetError
from ._tensor import ptr, stream_ptr


@dataclass(frozen=True)
class Tvl1Params:
    """OpenCV's DualTVL1 defaults where it has them; `iters` inner iterations per warp are always run (there is no epsilon stop)."""
    tau: float = 0.25
    lam: float = 0.15
    theta: float = 0.3
    scales: int = 5
    warps: int = 5
    iters: int = 30
    min_side: int = 16


def levels(H: int, W: int, params: Tvl1Params = None):
    """[(h, w)] of the pyramid, finest first."""
    p = params or Tvl1Params()
    hw = (ctypes.c_int * 32)()
    n = _lib.lib().stabnet_tvl1_levels(int(H), int(W), int(p.scales), int(p.min_side), hw)
    if n < 1:
        _lib.check(n, "stabnet_tvl1_levels")
    return [(hw[2 * i], hw[2 * i + 1]) for i in range(n)]


def fused_geometry():
    """(K, tile width, tile height) of the fused iteration kernel."""
    g = (ctypes.c_int * 3)()
    _lib.lib().stabnet_tvl1_fused_geometry(g)
    return tuple(g)


def workspace_bytes(B: int, H: int, W: int, params: Tvl1Params = None) -> int:
    p = params or Tvl1Params()
    n = _lib.lib().stabnet_tvl1_workspace_bytes(int(B), int(H), int(W), int(p.scales), int(p.min_side))
    if n == 0:
        raise StabnetError("flow.workspace_bytes: bad arguments: B %d (1..65535), H x W %d x %d (8 or more each, B*H*W below 2^31), "
                           "scales %d (1 or more), min_side %d (2 or more)" % (B, H, W, p.scales, p.min_side))
    return n


def image_view(t, name: str):
    """-> (tensor, pixel stride in floats) of a float32 [B,H,W] device tensor whose rows and images are dense at that stride: a
    contiguous tensor (stride 1) or one channel of a contiguous NHWC tensor (stride C).  Nothing is copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise StabnetError("flow.tvl1_flow: %s must be a tensor on the GPU (there is no CPU fallback)" % name)
    if t.dtype != torch.float32 or t.dim() != 3:
        raise StabnetError("flow.tvl1_flow: %s must be float32 [B,H,W], got %s %s" % (name, t.dtype, tuple(t.shape)))
    B, H, W = t.shape
    sb, sh, sw = t.stride()
    if sw < 1 or (W > 1 and sh != W * sw) or (B > 1 and sb != H * W * sw) or (H == 1 and W == 1):
        raise StabnetError("flow.tvl1_flow: %s has strides %s; pixels must lie ps floats apart with rows W*ps and images H*W*ps apart "
                           "(a contiguous [B,H,W] tensor or one channel of a contiguous [B,H,W,C] tensor)" % (name, (sb, sh, sw)))
    return t, int(sw)


def tvl1_flow(i0, i1, params: Tvl1Params = None, out: str = "map", workspace=None, prof=None, offset: float = 0.0,
              scale: float = 1.0):
    """i0, i1: float32 [B,H,W] device tensors, contiguous or NHWC channel views of equal stride (read in place).  The solve works
    on (v + offset) * scale, which must be the 0..255 scale: the defaults for tensors that are, offset=0.5, scale=255 for get_img
    channels.  -> [B,H,W,2]: out="uv" the flow in pixels, i1(x + u1, y + u2) ~ i0(x, y); out="map" the record's map,
    2*(j + u1)/W - 1 and 2*(i + u2)/H - 1, which interpolate() reads.  workspace: a uint8 device tensor of at least
    workspace_bytes(B, H, W, params) bytes (allocated when None).  Nothing synchronises or allocates inside the solve; non-finite
    pixel values are the caller's error."""
    p = params or Tvl1Params()
    if out not in ("map", "uv"):
        raise StabnetError("flow.tvl1_flow: out must be 'map' or 'uv', got %r" % (out,))
    i0, ps0 = image_view(i0, "i0")
    i1, ps1 = image_view(i1, "i1")
    if i0.shape != i1.shape or ps0 != ps1 or i0.device != i1.device:
        raise StabnetError("flow.tvl1_flow: i0 is %s with pixel stride %d on %s, i1 %s with %d on %s; they must agree"
                           % (tuple(i0.shape), ps0, i0.device, tuple(i1.shape), ps1, i1.device))
    B, H, W = i0.shape
    need = workspace_bytes(B, H, W, p)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=i0.device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.device != i0.device or workspace.numel() < need:
        raise StabnetError("flow.tvl1_flow: the workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (need, i0.device))
    res = torch.empty((B, H, W, 2), dtype=torch.float32, device=i0.device)
    _lib.call("stabnet_tvl1_flow", ptr(i0), ptr(i1), ps0, float(offset), float(scale), B, H, W, float(p.tau), float(p.lam),
              float(p.theta), int(p.scales), int(p.warps), int(p.iters), int(p.min_side), ptr(workspace), workspace.numel(),
              ptr(res) if out == "uv" else 0, ptr(res) if out == "map" else 0, stream_ptr(i0.device),
              prof.handle if prof is not None else 0, device=i0.device)
    return res
