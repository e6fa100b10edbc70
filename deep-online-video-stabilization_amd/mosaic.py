"""Full-frame output (csrc/mosaic.hip): a pixel the current stabilised frame does not cover is taken from what earlier stabilised
frames showed there, moved by the homography between the two stabilised frames; inside a feather band at the frame's edge the two
are blended.  Per frame, all on the device and on the caller's stream:

  track    corners of the network's stabilised grey frame t tracked into frame t - 1 (features / csrc/klt.hip)
  guard    matches within `guard` pixels of an uncovered pixel are dropped, either end (stabnet_mosaic_guard_matches): the
           content / black edge is the strongest corner of its cell and follows the border, not the scene
  fit      a robust homography frame t -> frame t - 1 in the normalised frame (metrics / csrc/homfit.hip)
  compose  stabnet_mosaic_compose over the source-size warped frame and the coordinates its remap wrote

Bit for bit tests/mosaic_model.py chained with klt_model.py and homfit_model.py."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, features
from ._lib import StabnetError
from ._tensor import ptr, stream_ptr

MAX_ROWS = 1024          # the guard's and the fit's rows per pair
LOG_FIELDS = ("fresh", "blended", "history", "empty", "status", "inliers", "matches", "guarded")


@dataclass(frozen=True)
class MosaicParams:
    """feather_log2: the blend band at the frame's edge is 2^feather_log2 pixels wide (0..6).  max_age: a canvas pixel last seen
    more than this many frames ago is not used (1..254).  guard: matches closer than this many pixels to an uncovered pixel are
    dropped (0..16; 8 measured on the model: DESIGN.md Round 17).  hypotheses, thr_px, min_inliers, seed: the fit's (a fit with
    fewer inliers than min_inliers gives no model, and the frame uses no history).  w_min: a pixel whose projective weight is not
    above it has no history.  klt: the tracker's; its relative `quality` threshold stays at the default 0.01 (the C entry refuses 0,
    and with the guard in place the model's experiment needed no lower one)."""
    feather_log2: int = 3
    max_age: int = 64
    guard: int = 8
    hypotheses: int = 256
    thr_px: float = 2.0
    min_inliers: int = 16
    seed: int = 0
    w_min: float = 1e-6
    klt: features.KltParams = field(default_factory=features.KltParams)


def guard_matches(matches, n, black0, black1, guard: int = 8, out=None, out_n=None):
    """matches float32 [B,M,4] and n int32 [B] as features.klt_matches returns them; black0, black1 float32 [B,H,W]: the network's
    `black` of the frame each end lives in -> (kept rows [B,M,4] in their order, zeros after them; their number int32 [B])."""
    if not isinstance(matches, torch.Tensor) or not matches.is_cuda or matches.dtype != torch.float32 or matches.dim() != 3 \
            or matches.shape[2] != 4 or not matches.is_contiguous():
        raise StabnetError("mosaic.guard_matches: matches must be a contiguous float32 [B,M,4] tensor on the GPU (there is no CPU fallback)")
    B, M = int(matches.shape[0]), int(matches.shape[1])
    dev = matches.device
    if not isinstance(n, torch.Tensor) or n.device != dev or n.dtype != torch.int32 or tuple(n.shape) != (B,) or not n.is_contiguous():
        raise StabnetError("mosaic.guard_matches: n must be a contiguous int32 [B] tensor on %s with B = %d" % (dev, B))
    for b in (black0, black1):
        if not isinstance(b, torch.Tensor) or b.device != dev or b.dtype != torch.float32 or b.dim() != 3 or b.shape[0] != B \
                or b.shape != black0.shape or not b.is_contiguous():
            raise StabnetError("mosaic.guard_matches: black0 and black1 must be contiguous float32 [B,H,W] tensors on %s with B = %d" % (dev, B))
    H, W = int(black0.shape[1]), int(black0.shape[2])
    out = torch.empty_like(matches) if out is None else out
    out_n = torch.empty_like(n) if out_n is None else out_n
    _lib.call("stabnet_mosaic_guard_matches", ptr(matches), ptr(n), ptr(black0), ptr(black1), B, M, H, W, int(guard), ptr(out), ptr(out_n),
              stream_ptr(dev), device=dev)
    return out, out_n


def compose(warped, px, py, canvas_prev, age_prev, Hm, status, H: int, W: int, feather_log2: int = 3, max_age: int = 64,
            w_min: float = 1e-6, canvas_cur=None, age_cur=None, counts=None):
    """One frame of every stream: warped uint8 [N,SH,SW,3], px, py float32 [N,SH,SW] (warp.warpRevBundle2_src with return_maps),
    the previous canvas and ages, Hm float32 [N,9] and status int32 [N] (frame t -> frame t - 1) -> (canvas uint8 [N,SH,SW,3], age
    uint8 [N,SH,SW], counts int32 [N,4] = fresh, blended, history, empty).  counts, when given, is added to."""
    if not isinstance(warped, torch.Tensor) or not warped.is_cuda or warped.dtype != torch.uint8 or warped.dim() != 4 or warped.shape[3] != 3:
        raise StabnetError("mosaic.compose: warped must be a uint8 [N,SH,SW,3] tensor on the GPU (BGR; there is no CPU fallback)")
    N, SH, SW, _ = (int(v) for v in warped.shape)
    dev = warped.device
    for t, dt, shape, what in ((px, torch.float32, (N, SH, SW), "px"), (py, torch.float32, (N, SH, SW), "py"),
                               (canvas_prev, torch.uint8, (N, SH, SW, 3), "canvas_prev"), (age_prev, torch.uint8, (N, SH, SW), "age_prev"),
                               (Hm, torch.float32, (N, 9), "Hm"), (status, torch.int32, (N,), "status"), (warped, torch.uint8, (N, SH, SW, 3), "warped")):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise StabnetError("mosaic.compose: %s must be a contiguous %s tensor of %s on %s" % (what, dt, list(shape), dev))
    canvas_cur = torch.empty_like(canvas_prev) if canvas_cur is None else canvas_cur
    age_cur = torch.empty_like(age_prev) if age_cur is None else age_cur
    counts = torch.zeros((N, 4), dtype=torch.int32, device=dev) if counts is None else counts
    _lib.call("stabnet_mosaic_compose", ptr(warped), ptr(px), ptr(py), ptr(canvas_prev), ptr(age_prev), ptr(Hm), ptr(status), N, SH, SW,
              int(H), int(W), int(feather_log2), int(max_age), float(w_min), ptr(canvas_cur), ptr(age_cur), ptr(counts), stream_ptr(dev),
              device=dev)
    return canvas_cur, age_cur, counts


class Mosaic:
    """The canvas of N streams at SH x SW (uint8 BGR) beside a network of H x W.  update() per frame; log() once after the clip."""

    def __init__(self, N: int, SH: int, SW: int, H: int, W: int, params: MosaicParams = None, device=None, grey_offset: float = 0.5,
                 grey_scale: float = 255.0, log_frames: int = 4096):
        """grey_offset, grey_scale: (grey + offset) * scale must be the 0..255 scale the tracker works on, as metrics.score_clip's
        frames are; the defaults take the network's grey output in [-0.5, 0.5].  log_frames: frames the log holds before it is
        doubled (the only allocation after construction)."""
        self.p = p = params or MosaicParams()
        self.N, self.SH, self.SW, self.H, self.W = (int(v) for v in (N, SH, SW, H, W))
        self.dev = dev = torch.device(device if device is not None else "cuda:0")
        if dev.type != "cuda":
            raise StabnetError("mosaic.Mosaic: the device must be a GPU (there is no CPU fallback)")
        if not 0 <= p.feather_log2 <= 6 or not 1 <= p.max_age <= 254 or not 0 <= p.guard <= 16:
            raise StabnetError("mosaic.Mosaic: feather_log2 0..6, max_age 1..254 and guard 0..16, got %d, %d, %d" % (p.feather_log2, p.max_age, p.guard))
        ny, nx = features.cells(self.H, self.W, p.klt)
        self.M = ny * nx + 1                                   # every cell can keep its row
        if not 4 <= self.M <= MAX_ROWS:
            raise StabnetError("mosaic.Mosaic: %d x %d pixels in cells of %d give %d rows per pair; the fit takes 4..%d: choose a larger "
                               "KltParams.cell" % (self.H, self.W, p.klt.cell, self.M, MAX_ROWS))
        self.offset, self.scale = float(grey_offset), float(grey_scale)
        u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.canvas = [u8(self.N, self.SH, self.SW, 3), u8(self.N, self.SH, self.SW, 3)]
        self.age = [u8(self.N, self.SH, self.SW), u8(self.N, self.SH, self.SW)]
        self.prev_grey, self.prev_black = f32(self.N, self.H, self.W), f32(self.N, self.H, self.W)
        self.klt_ws = torch.empty(features.workspace_bytes(self.N, self.H, self.W, p.klt), dtype=torch.uint8, device=dev)
        self.matches, self.guarded = f32(self.N, self.M, 4), f32(self.N, self.M, 4)
        self.n, self.gn = i32(self.N), i32(self.N)
        self.Hm, self.mask = f32(self.N, 9), u8(self.N, self.M)
        self.count, self.status, self.best = i32(self.N), i32(self.N), i32(self.N)
        self.counts = i32(self.N, 4)
        self._log = i32(max(int(log_frames), 1), self.N, len(LOG_FIELDS))
        self.cur = 0                                            # canvas[cur], age[cur]: the last frame's
        self.reset()

    def reset(self, keep_log: bool = False):
        """Empty canvases (every age 255); the next frame has no model (status 0) and is not tracked.  keep_log (a scene cut inside a
        clip): the per-frame log goes on where it is."""
        for a in self.age:
            a.fill_(255)
        for c in self.canvas:
            c.zero_()
        self.frames, self._have_prev = (self.frames if keep_log else 0), False

    def _check(self, t, dtype, shape, what):
        if not isinstance(t, torch.Tensor) or t.device != self.dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise StabnetError("mosaic.Mosaic.update: %s must be a contiguous %s tensor of %s on %s" % (what, dtype, list(shape), self.dev))

    def update(self, warped, px, py, grey, black, prof=None):
        """warped uint8 [N,SH,SW,3], px, py float32 [N,SH,SW]: this frame through warp.warpRevBundle2_src(..., return_maps=True);
        grey float32 [N,H,W]: the network's stabilised grey output; black float32 [N,H,W]: its `black`.  -> the current canvas
        uint8 [N,SH,SW,3], a view that stays valid until the next update.  Allocates nothing, reads nothing back, synchronises
        nothing (the log doubles itself every log_frames frames)."""
        N, SH, SW, H, W, p, dev = self.N, self.SH, self.SW, self.H, self.W, self.p, self.dev
        self._check(warped, torch.uint8, (N, SH, SW, 3), "warped")
        self._check(px, torch.float32, (N, SH, SW), "px")
        self._check(py, torch.float32, (N, SH, SW), "py")
        self._check(grey, torch.float32, (N, H, W), "grey")
        self._check(black, torch.float32, (N, H, W), "black")
        st, ph, k = stream_ptr(dev), (prof.handle if prof is not None else 0), p.klt
        if self._have_prev:
            _lib.call("stabnet_klt_matches", ptr(grey), ptr(self.prev_grey), 1, 1, self.offset, self.scale, N, H, W, int(k.levels),
                      int(k.min_side), int(k.r), int(k.border), int(k.cell), float(k.floor), float(k.quality), int(k.R), int(k.iters),
                      float(k.min_eig), float(k.fb), self.M, ptr(self.klt_ws), self.klt_ws.numel(), ptr(self.matches), ptr(self.n), st, ph,
                      device=dev)
            _lib.call("stabnet_mosaic_guard_matches", ptr(self.matches), ptr(self.n), ptr(black), ptr(self.prev_black), N, self.M, H, W,
                      int(p.guard), ptr(self.guarded), ptr(self.gn), st, device=dev)
            _lib.call("stabnet_homfit", ptr(self.guarded), ptr(self.gn), N, self.M, H, W, int(p.hypotheses), float(p.thr_px),
                      int(p.min_inliers), int(p.seed), float(p.w_min), ptr(self.Hm), ptr(self.mask), ptr(self.count), ptr(self.status),
                      ptr(self.best), st, ph, device=dev)
        else:
            for t in (self.Hm, self.count, self.status, self.n, self.gn):
                t.zero_()
        new = 1 - self.cur
        self.counts.zero_()
        _lib.call("stabnet_mosaic_compose", ptr(warped), ptr(px), ptr(py), ptr(self.canvas[self.cur]), ptr(self.age[self.cur]), ptr(self.Hm),
                  ptr(self.status), N, SH, SW, H, W, int(p.feather_log2), int(p.max_age), float(p.w_min), ptr(self.canvas[new]),
                  ptr(self.age[new]), ptr(self.counts), st, device=dev)
        self.prev_grey.copy_(grey)
        self.prev_black.copy_(black)
        if self.frames >= self._log.shape[0]:
            self._log = torch.cat([self._log, torch.zeros_like(self._log)])
        row = self._log[self.frames]
        row[:, 0:4].copy_(self.counts)
        row[:, 4].copy_(self.status)
        row[:, 5].copy_(self.count)
        row[:, 6].copy_(self.n)
        row[:, 7].copy_(self.gn)
        self.cur, self.frames, self._have_prev = new, self.frames + 1, True
        return self.canvas[new]

    @property
    def ages(self):
        """uint8 [N,SH,SW]: the current canvas's ages (255: empty)."""
        return self.age[self.cur]

    def log(self) -> dict:
        """One readback: per frame and stream the four counts, the fit's status and inlier count, the matches before and after
        the guard -> {field: int array [frames, N]}."""
        back = self._log[:self.frames].cpu().numpy()
        return {name: back[:, :, i].copy() for i, name in enumerate(LOG_FIELDS)}

    def params_dict(self) -> dict:
        return dataclasses.asdict(self.p)


def totals(log: dict) -> dict:
    """Sums over a clip's log, for a report."""
    out = {k: int(np.asarray(log[k]).sum()) for k in ("fresh", "blended", "history", "empty")}
    out["frames_without_model"] = int((np.asarray(log["status"]) == 0).sum())
    return out
