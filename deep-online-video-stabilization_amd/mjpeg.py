"""Baseline JPEG encoding of uint8 frames on the device (csrc/mjpeg.hip): the last step of the reference's deploy loop
(deploy_bundle.py:197-198,305: cv2.VideoWriter with fourcc MJPG), done where the stabilised frame already lies."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._tensor import ptr, stream_ptr

# Restart interval in MCUs when the caller does not choose.  One lane codes one interval, so the entropy launch takes as long as one
# interval and the stream grows by about 2.5 bytes per interval.  Measured on the MI355X, BGR 4:2:0 q75 (profiles/r05_mjpeg_bench.json):
# 720p 1 / 2 / 4 / 8 / one MCU row = 47 / 73 / 130 / 241 / 1648 us and +11.8 / +5.8 / +2.8 / +1.4 / 0 % bytes.  2 MCUs (12 blocks, 512
# pixels) is the knee: 5 % of the frame's 1.5 ms for 6 % of the bytes.  4:4:4 and grey MCUs are a quarter of the pixels; they get the
# same pixels per interval (12 and 8 blocks per lane) -- scaled from the 4:2:0 sweep, not swept themselves.
DEFAULT_RESTART_MCUS = 2


def default_restart_mcus(channels: int = 3, subsampling="420") -> int:
    if int(channels) == 1:
        return 8
    return DEFAULT_RESTART_MCUS if int(subsampling) == 420 else 4


def quant_tables(quality: int = 75):
    """(luma, chroma) uint16 [64], natural order: Annex K scaled by the IJG rule."""
    ql, qc = (ctypes.c_ushort * 64)(), (ctypes.c_ushort * 64)()
    _lib.call("stabnet_jpeg_quant_tables", int(quality), ql, qc)
    return np.array(ql, np.uint16), np.array(qc, np.uint16)


def header_bytes(H, W, channels, subsampling, restart_mcus, q_luma, q_chroma) -> bytes:
    """SOI .. SOS of the streams the encoder writes for these arguments."""
    ql = (ctypes.c_ushort * 64)(*[int(v) for v in q_luma])
    qc = (ctypes.c_ushort * 64)(*[int(v) for v in q_chroma])
    buf = (ctypes.c_ubyte * 1024)()
    n = _lib.lib().stabnet_mjpeg_header(H, W, channels, int(subsampling), restart_mcus, ql, qc, buf, 1024)
    if n < 0:
        _lib.check(n, "stabnet_mjpeg_header")
    return bytes(buf[:n])


class MjpegEncoder:
    """Owns tables, header, workspace and output buffers on the device.

    encode(img_u8) -> (buf uint8 [N, max_bytes], nbytes int32 [N]): device tensors, nothing synchronises, so the call can be
    captured in a hipGraph together with the launches that produce the frame.  Stream n is buf[n, :nbytes[n]]; the bytes behind it
    are undefined.  The buffers are sized for the worst case, so there is no overflow to report.
    encode_bytes(img_u8) -> list[bytes] (synchronises, downloads)."""

    def __init__(self, H: int, W: int, channels: int = 3, quality: int = 75, subsampling="420", restart_mcus=None, device="cuda:0",
                 batch: int = 1, q_luma=None, q_chroma=None):
        self.H, self.W, self.C, self.quality = int(H), int(W), int(channels), int(quality)
        self.subsampling = int(subsampling)
        self.restart_mcus = int(default_restart_mcus(channels, subsampling) if restart_mcus is None else restart_mcus)
        self.device = torch.device(device)
        if q_luma is None:
            q_luma, q_chroma = quant_tables(quality)
        self.q_luma, self.q_chroma = np.asarray(q_luma, np.uint16).reshape(64), np.asarray(q_chroma, np.uint16).reshape(64)
        self.header = header_bytes(self.H, self.W, self.C, self.subsampling, self.restart_mcus, self.q_luma, self.q_chroma)
        L = _lib.lib()
        self.max_bytes = L.stabnet_mjpeg_max_bytes(self.H, self.W, self.C, self.subsampling, self.restart_mcus)
        if self.max_bytes == 0:
            _lib.check(-1, "stabnet_mjpeg_max_bytes")
        # uint16 has no torch dtype on every build: the tables travel as raw bytes
        self._tables = torch.from_numpy(np.concatenate([self.q_luma, self.q_chroma]).view(np.uint8).copy()).to(self.device)
        self._header = torch.from_numpy(np.frombuffer(self.header, np.uint8).copy()).to(self.device)
        self._batch = 0
        self._reserve(batch)

    def _reserve(self, n: int):
        if n <= self._batch:
            return
        ws = _lib.lib().stabnet_mjpeg_workspace_bytes(n, self.H, self.W, self.C, self.subsampling, self.restart_mcus)
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.out = torch.empty((n, self.max_bytes), dtype=torch.uint8, device=self.device)
        self.nbytes = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._batch = n

    def _check(self, img):
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8:
            raise _lib.StabnetError("MjpegEncoder: expected a uint8 tensor on the GPU (there is no CPU fallback)")
        return img.reshape(-1, self.H, self.W, self.C).contiguous()

    def encode(self, img, out=None, nbytes=None, prof=None):
        """img uint8 [N,H,W,C] ([H,W,C] / [H,W]: N = 1) on the device.  out / nbytes: caller's buffers ([N, >= max_bytes] uint8,
        [N] int32) instead of the encoder's own."""
        img = self._check(img)
        n = img.shape[0]
        if out is None:
            self._reserve(n)
            out, nbytes = self.out[:n], self.nbytes[:n]
        elif n > self._batch:
            self._reserve(n)
        _lib.call("stabnet_mjpeg_encode", ptr(img), n, self.H, self.W, self.C, self.subsampling, self.restart_mcus,
                  ptr(self._tables), self._tables.data_ptr() + 128, ptr(self._header), len(self.header), ptr(out), out.stride(0),
                  ptr(nbytes), ptr(self.workspace), self.workspace.numel(), stream_ptr(self.device),
                  prof.handle if prof is not None else 0, device=self.device)
        return out, nbytes

    def encode_bytes(self, img):
        out, nbytes = self.encode(img)
        lens = nbytes.cpu().tolist()
        return [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lens)]
