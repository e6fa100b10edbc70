"""Feature matches on the device (csrc/klt.hip): what fills a record's `feature_matches1 / 2`.  Shi-Tomasi corners, one per grid
cell of the stable frame, tracked into the unstable frame of the same instant by pyramidal Lucas-Kanade with a fixed number of
iterations, and kept when the track back ends within `fb` pixels of where it started -- every step deterministic float32, bit for
bit tests/klt_model.py.  A row is (stable x, stable y, unstable x, unstable y) as 2*x/W - 1, 2*y/H - 1."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import StabnetError
from ._tensor import ptr, stream_ptr
from .flow import image_view


@dataclass(frozen=True)
class KltParams:
    """levels, min_side: the pyramid (TV-L1's rule).  r, border: box radius of the corner response and the band at the image edge
    that has none.  cell, floor, quality: one candidate per cell x cell pixels, detected when its response is at least `floor` and
    `quality` times the image's largest.  R, iters, min_eig: window radius, iterations per level (always run) and the smallest
    eigenvalue per window sample below which a point is lost.  fb: the largest forward-backward distance in pixels."""
    levels: int = 4
    min_side: int = 16
    r: int = 2
    border: int = 8
    cell: int = 16
    floor: float = 1.0
    quality: float = 0.01
    R: int = 7
    iters: int = 10
    min_eig: float = 1e-3
    fb: float = 0.5


def cells(H: int, W: int, params: KltParams = None):
    """(rows, columns) of the grid of cells; partial cells at the right and bottom edges count."""
    p = params or KltParams()
    rc = (ctypes.c_int * 2)()
    n = _lib.lib().stabnet_klt_cells(int(H), int(W), int(p.cell), rc)
    if n < 1:
        _lib.check(n, "stabnet_klt_cells")
    return rc[0], rc[1]


def workspace_bytes(B: int, H: int, W: int, params: KltParams = None) -> int:
    p = params or KltParams()
    n = _lib.lib().stabnet_klt_workspace_bytes(int(B), int(H), int(W), int(p.levels), int(p.min_side), int(p.cell))
    if n == 0:
        raise StabnetError("features.workspace_bytes: bad arguments: B %d (1..65535), H x W %d x %d (3 or more each, B*H*W below 2^31), "
                           "levels %d (1..8), min_side %d (2 or more), cell %d (2 or more)" % (B, H, W, p.levels, p.min_side, p.cell))
    return n


def _pair(i0, i1, what):
    i0, ps0 = image_view(i0, "i0")
    i1, ps1 = image_view(i1, "i1")
    if i0.shape != i1.shape or i0.device != i1.device:
        raise StabnetError("features.%s: i0 is %s on %s, i1 %s on %s; they must agree"
                           % (what, tuple(i0.shape), i0.device, tuple(i1.shape), i1.device))
    return i0, ps0, i1, ps1


def _workspace(workspace, need, dev, what):
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.device != dev or workspace.numel() < need:
        raise StabnetError("features.%s: the workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (what, need, dev))
    return workspace


def _prof(prof):
    return prof.handle if prof is not None else 0


def klt_response(i0, params: KltParams = None, prof=None, offset: float = 0.0, scale: float = 1.0):
    """Stage: the corner response plane [B,H,W] of i0."""
    p = params or KltParams()
    i0, ps = image_view(i0, "i0")
    B, H, W = i0.shape
    out = torch.empty((B, H, W), dtype=torch.float32, device=i0.device)
    _lib.call("stabnet_klt_response", ptr(i0), ps, float(offset), float(scale), B, H, W, int(p.r), int(p.border), ptr(out),
              stream_ptr(i0.device), _prof(prof), device=i0.device)
    return out


def klt_detect(i0, params: KltParams = None, prof=None, offset: float = 0.0, scale: float = 1.0):
    """Stage: [B,cells,4] = x, y, response, detected (1 / 0) of every cell's candidate, cells in row-major order."""
    p = params or KltParams()
    i0, ps = image_view(i0, "i0")
    B, H, W = i0.shape
    ny, nx = cells(H, W, p)
    out = torch.empty((B, ny * nx, 4), dtype=torch.float32, device=i0.device)
    _lib.call("stabnet_klt_detect", ptr(i0), ps, float(offset), float(scale), B, H, W, int(p.r), int(p.border), int(p.cell), float(p.floor),
              float(p.quality), ptr(out), stream_ptr(i0.device), _prof(prof), device=i0.device)
    return out


def klt_track(i0, i1, pts, params: KltParams = None, workspace=None, prof=None, offset: float = 0.0, scale: float = 1.0):
    """Stage: pts [B,N,2] (x, y in pixels of i0) -> [B,N,4] = q.x, q.y in i1, lost (1 / 0), the forward-backward distance squared;
    the row of a lost point is (0, 0, 1, 0)."""
    p = params or KltParams()
    i0, ps0, i1, ps1 = _pair(i0, i1, "klt_track")
    B, H, W = i0.shape
    if not isinstance(pts, torch.Tensor) or pts.device != i0.device or pts.dtype != torch.float32 or pts.dim() != 3 \
            or pts.shape[0] != B or pts.shape[2] != 2 or pts.shape[1] < 1 or not pts.is_contiguous():
        raise StabnetError("features.klt_track: pts must be a contiguous float32 [B,N,2] tensor on %s with B = %d" % (i0.device, B))
    N = pts.shape[1]
    workspace = _workspace(workspace, workspace_bytes(B, H, W, p), i0.device, "klt_track")
    out = torch.empty((B, N, 4), dtype=torch.float32, device=i0.device)
    _lib.call("stabnet_klt_track", ptr(i0), ptr(i1), ps0, ps1, float(offset), float(scale), B, H, W, ptr(pts), N, int(p.levels),
              int(p.min_side), int(p.R), int(p.iters), float(p.min_eig), ptr(workspace), workspace.numel(), ptr(out),
              stream_ptr(i0.device), _prof(prof), device=i0.device)
    return out


def klt_matches(i0, i1, max_matches: int, params: KltParams = None, workspace=None, prof=None, offset: float = 0.0, scale: float = 1.0):
    """i0 (stable), i1 (unstable): float32 [B,H,W] device tensors, contiguous or NHWC channel views (read in place; the two strides
    may differ).  The solve works on (v + offset) * scale, which must be the 0..255 scale: the defaults for tensors that are,
    offset=0.5, scale=255 for get_img channels.  -> (matches [B,max_matches,4] float32, n [B] int32), both on the device: the valid
    matches in cell order, at most max_matches - 1 of them (the reference wants the count below max_matches), zeros from row n[b]
    on.  workspace: a uint8 device tensor of at least workspace_bytes(B, H, W, params) bytes (allocated when None).  Nothing
    synchronises or allocates inside the solve; non-finite pixel values are the caller's error."""
    p = params or KltParams()
    i0, ps0, i1, ps1 = _pair(i0, i1, "klt_matches")
    B, H, W = i0.shape
    if int(max_matches) < 2:
        raise StabnetError("features.klt_matches: max_matches must be at least 2 (one row less is kept), got %r" % (max_matches,))
    workspace = _workspace(workspace, workspace_bytes(B, H, W, p), i0.device, "klt_matches")
    m = torch.empty((B, int(max_matches), 4), dtype=torch.float32, device=i0.device)
    n = torch.empty((B,), dtype=torch.int32, device=i0.device)
    _lib.call("stabnet_klt_matches", ptr(i0), ptr(i1), ps0, ps1, float(offset), float(scale), B, H, W, int(p.levels), int(p.min_side),
              int(p.r), int(p.border), int(p.cell), float(p.floor), float(p.quality), int(p.R), int(p.iters), float(p.min_eig),
              float(p.fb), int(max_matches), ptr(workspace), workspace.numel(), ptr(m), ptr(n), stream_ptr(i0.device), _prof(prof),
              device=i0.device)
    return m, n
