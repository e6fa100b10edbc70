"""Frame ingest on the device (csrc/ingest.hip): the uint8 frame as it was read from the video -- any size, BGR or grey -- to the
network's grey input and the network-size colour frame, with the reference's own arithmetic: config.cvt_img2train (config.py:6-21:
cv2.cvtColor(BGR2GRAY), PIL.Image.resize(BILINEAR), * (1./255) - 0.5) and cv2.resize (deploy_bundle.py:215,303)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._tensor import ptr, stream_ptr

# cv2.cvtColor(BGR2GRAY) on uint8, (WB, WG, WR, shift): OpenCV 3 (the reference's era) and OpenCV 4
GRAY_WEIGHTS = {"cv3": (1868, 9617, 4899, 14), "cv4": (3735, 19235, 9798, 15)}


def pil_taps(n_in: int, n_out: int):
    """(ksize, bounds int32 [n_out, 2] = (first sample, taps), kk int32 [n_out, ksize]): Pillow's BILINEAR taps of one axis."""
    L = _lib.lib()
    ks = ctypes.c_int()
    n = L.stabnet_ingest_pil_taps(int(n_in), int(n_out), ctypes.byref(ks), None, None, 0)
    if n < 0:
        _lib.check(n, "stabnet_ingest_pil_taps")
    bounds, kk = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ks.value), np.int32)
    rc = L.stabnet_ingest_pil_taps(int(n_in), int(n_out), ctypes.byref(ks), bounds.ctypes.data, kk.ctypes.data, n)
    if rc < 0:
        _lib.check(rc, "stabnet_ingest_pil_taps")
    return ks.value, bounds, kk


def cv_taps(n_src: int, n_dst: int):
    """(ofs int32 [n_dst, 2], coef int16 [n_dst, 2]): cv2.resize INTER_LINEAR's taps of one axis."""
    ofs, coef = np.zeros((n_dst, 2), np.int32), np.zeros((n_dst, 2), np.int16)
    _lib.call("stabnet_ingest_cv_taps", int(n_src), int(n_dst), ofs.ctypes.data, coef.ctypes.data)
    return ofs, coef


def lut256() -> np.ndarray:
    """float32(float64(u) * (1./255) - 0.5): cvt_img2train computes in float64, TensorFlow casts the feed to float32."""
    return (np.arange(256, dtype=np.float64) * (1. / 255) - 0.5).astype(np.float32)


def lut256_limited() -> np.ndarray:
    """lut256 for a LIMITED-range Y plane (16..235): float32(clip((u - 16) * 255/219, 0, 255) * (1./255) - 0.5), computed in float64."""
    u = np.arange(256, dtype=np.float64)
    return (np.clip((u - 16.0) * 255 / 219, 0.0, 255.0) * (1. / 255) - 0.5).astype(np.float32)


class FrameIngest:
    """Tables of one geometry on the device: source src_h x src_w x channels (3 = BGR, 1 = grey) -> network H x W.

    grey(u8, out=None)   -> float32 [N,H,W], the network's input: BGR2GRAY, Pillow BILINEAR to (H, W) -- or, with crop_rate != 1, to
                            (int(H/crop_rate), int(W/crop_rate)) and the centred H x W window of that (config.py:8-15) --, normalised
    colour(u8, out=None) -> uint8 [N,H,W,3]: cv2.resize(frame, (W, H)), the frame that is warped and written
    u8: uint8 device tensor [N,src_h,src_w,channels] ([src_h,src_w,channels] / [src_h,src_w]: N = 1); rows may be strided
    (u8.stride(-3) bytes apart), pixels must be dense.  Nothing synchronises: both calls can be captured in a hipGraph.
    lut: float32 [256], the normalisation of the resized grey value (default lut256(); lut256_limited() for a limited-range Y plane)."""

    def __init__(self, src_h: int, src_w: int, channels: int, H: int, W: int, crop_rate=1, gray="cv3", batch: int = 1, device="cuda:0",
                 lut=None):
        self.sh, self.sw, self.C, self.H, self.W = int(src_h), int(src_w), int(channels), int(H), int(W)
        if self.C not in (1, 3):
            raise _lib.StabnetError("FrameIngest: channels must be 1 (grey) or 3 (BGR), got %r" % (channels,))
        if min(self.sh, self.sw, self.H, self.W) < 1:
            raise _lib.StabnetError("FrameIngest: every size must be >= 1")
        if isinstance(gray, str):
            if gray not in GRAY_WEIGHTS:
                raise _lib.StabnetError("FrameIngest: gray must be one of %s or (wb, wg, wr, shift)" % sorted(GRAY_WEIGHTS))
            gray = GRAY_WEIGHTS[gray]
        self.weights = tuple(int(v) for v in gray)
        self.device = torch.device(device)
        if crop_rate == 1:
            self.rh, self.rw, self.dy, self.dx = self.H, self.W, 0, 0
        else:
            self.rh, self.rw = int(self.H / crop_rate), int(self.W / crop_rate)
            self.dy, self.dx = int((self.rh - self.H) / 2), int((self.rw - self.W) / 2)
            if self.dy < 0 or self.dx < 0:
                raise _lib.StabnetError("FrameIngest: crop_rate %r > 1 leaves no %dx%d window in %dx%d" % (crop_rate, self.H, self.W, self.rh, self.rw))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device)
        # Pillow's tables; a pass whose sizes agree is skipped (no table)
        self._xk = self._yk = 0
        self._xb_dev = self._xk_dev = self._yb_dev = self._yk_dev = None
        if self.rw != self.sw:
            self._xk, b, k = pil_taps(self.sw, self.rw)
            self._xb_dev, self._xk_dev = up(b), up(k)
        if self.rh != self.sh:
            self._yk, b, k = pil_taps(self.sh, self.rh)
            self._yb_dev, self._yk_dev = up(b), up(k)
        lut = lut256() if lut is None else np.ascontiguousarray(lut)
        if lut.dtype != np.float32 or lut.shape != (256,):
            raise _lib.StabnetError("FrameIngest: lut must be a float32 array of 256 entries, got %s %s" % (lut.dtype, list(lut.shape)))
        self._lut = torch.from_numpy(lut.copy()).to(self.device)
        self._cv = None
        if self.C == 3:
            (xo, xc), (yo, yc) = cv_taps(self.sw, self.W), cv_taps(self.sh, self.H)
            self._cv = (up(xo), up(xc), up(yo), up(yc))           # int16 has no use as a torch dtype here: the tables travel as bytes
        self._batch = 0
        self._reserve(batch)

    def _reserve(self, n: int):
        if n <= self._batch:
            return
        ws = _lib.lib().stabnet_ingest_workspace_bytes(n, self.sh, self.sw, self.C, self.rh, self.rw, self.H, self.W)
        if ws == 0:
            _lib.check(-1, "stabnet_ingest_workspace_bytes")
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self._batch = n

    def _check(self, u8, what):
        if not isinstance(u8, torch.Tensor) or not u8.is_cuda:
            raise _lib.StabnetError("FrameIngest.%s: expected a uint8 tensor on the GPU (there is no CPU fallback)" % what)
        if u8.dtype != torch.uint8:
            raise _lib.StabnetError("FrameIngest.%s: expected uint8, got %s" % (what, u8.dtype))
        if u8.device != self.device:
            raise _lib.StabnetError("FrameIngest.%s: tensor on %s, tables on %s" % (what, u8.device, self.device))
        shp = tuple(u8.shape)
        if self.C == 1 and shp[-2:] == (self.sh, self.sw) and (u8.dim() == 2 or shp[-3:] != (self.sh, self.sw, 1)):
            u8 = u8.unsqueeze(-1)
            shp = tuple(u8.shape)
        if u8.dim() == 3:
            u8 = u8.unsqueeze(0)
            shp = tuple(u8.shape)
        if u8.dim() != 4 or shp[1:] != (self.sh, self.sw, self.C):
            raise _lib.StabnetError("FrameIngest.%s: expected [N, %d, %d, %d], got %s" % (what, self.sh, self.sw, self.C, list(shp)))
        n = shp[0]
        dense = u8.stride(3) == 1 and u8.stride(2) == self.C and u8.stride(1) >= self.sw * self.C and (n == 1 or u8.stride(0) == self.sh * u8.stride(1))
        if not dense:
            u8 = u8.contiguous()
        return u8, n, u8.stride(1)

    def _out(self, out, shape, dtype, what):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != dtype or out.numel() != int(np.prod(shape)) \
                or not out.is_contiguous():
            raise _lib.StabnetError("FrameIngest.%s: out must be a contiguous %s tensor of %s on %s" % (what, dtype, list(shape), self.device))
        return out

    def grey(self, u8, out=None, prof=None):
        u8, n, stride = self._check(u8, "grey")
        out = self._out(out, (n, self.H, self.W), torch.float32, "grey")
        self._reserve(n)
        wb, wg, wr, shift = self.weights
        _lib.call("stabnet_ingest_grey", ptr(u8), n, self.sh, self.sw, self.C, stride, wb, wg, wr, shift, self.rh, self.rw, self.dy, self.dx,
                  self.H, self.W, ptr(self._xb_dev), ptr(self._xk_dev), self._xk, ptr(self._yb_dev), ptr(self._yk_dev), self._yk,
                  ptr(self._lut), ptr(out), ptr(self.workspace), self.workspace.numel(), stream_ptr(self.device),
                  prof.handle if prof is not None else 0, device=self.device)
        return out

    def colour(self, u8, out=None, prof=None):
        if self.C != 3:
            raise _lib.StabnetError("FrameIngest.colour: the source has %d channel(s); the colour frame needs BGR" % self.C)
        u8, n, stride = self._check(u8, "colour")
        out = self._out(out, (n, self.H, self.W, 3), torch.uint8, "colour")
        xo, xc, yo, yc = self._cv
        _lib.call("stabnet_ingest_colour", ptr(u8), n, self.sh, self.sw, 3, stride, self.H, self.W, ptr(xo), ptr(xc), ptr(yo), ptr(yc),
                  ptr(out), stream_ptr(self.device), prof.handle if prof is not None else 0, device=self.device)
        return out
