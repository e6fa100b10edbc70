"""Baseline JPEG encoding of uint8 frames on the device (csrc/mjpeg.hip): the last step of the reference's deploy loop
(deploy_bundle.py:197-198,305: cv2.VideoWriter with fourcc MJPG), done where the stabilised frame already lies -- and its mirror
image, MjpegDecoder (csrc/mjpeg_decode.hip): the frames of a Motion-JPEG clip decoded where the ingest reads them, bit for bit what
libjpeg-turbo (Pillow, OpenCV) decodes."""
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


def planar_frame_bytes(H: int, W: int, channels: int = 3) -> int:
    """Bytes of one dense planar frame: Y [H,W] and, for channels = 3, U and V [H/2,W/2] (I420)."""
    return int(H) * int(W) * 3 // 2 if int(channels) == 3 else int(H) * int(W)


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
    encode_bytes(img_u8) -> list[bytes] (synchronises, downloads).
    planar=True: the frames are planar instead, uint8 [N, frame_bytes] (rows frame_bytes or more apart): Y [H,W] and, for channels = 3,
    U and V [H/2,W/2] behind it -- what warpRevBundle2_i420 writes and a planar MjpegDecoder fills (stabnet_mjpeg_encode_i420: no
    colour conversion, no chroma averaging).  The streams are 4:2:0 (grey for channels = 1); colour needs even H and W."""

    def __init__(self, H: int, W: int, channels: int = 3, quality: int = 75, subsampling="420", restart_mcus=None, device="cuda:0",
                 batch: int = 1, q_luma=None, q_chroma=None, planar: bool = False):
        self.H, self.W, self.C, self.quality = int(H), int(W), int(channels), int(quality)
        self.subsampling = int(subsampling)
        self.planar = bool(planar)
        if self.planar:
            if self.C == 3 and self.subsampling != 420:
                raise _lib.StabnetError("MjpegEncoder: planar frames are 4:2:0, not %d" % self.subsampling)
            if self.C == 3 and (self.H | self.W) & 1:
                raise _lib.StabnetError("MjpegEncoder: a planar 4:2:0 frame of %dx%d has an odd side" % (self.W, self.H))
        self.frame_bytes = planar_frame_bytes(self.H, self.W, self.C)
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
        if self.planar:
            if img.dim() == 1:
                img = img.view(1, -1)
            if img.dim() != 2 or img.shape[1] != self.frame_bytes or img.stride(1) != 1 or (img.shape[0] > 1 and img.stride(0) < self.frame_bytes):
                raise _lib.StabnetError("MjpegEncoder: planar frames are uint8 [N, %d] with dense rows, got %s" % (self.frame_bytes, tuple(img.shape)))
            return img
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
        if self.planar:
            _lib.call("stabnet_mjpeg_encode_i420", ptr(img), n, self.H, self.W, self.C, max(img.stride(0), self.frame_bytes), self.restart_mcus,
                      ptr(self._tables), self._tables.data_ptr() + 128, ptr(self._header), len(self.header), ptr(out), out.stride(0),
                      ptr(nbytes), ptr(self.workspace), self.workspace.numel(), stream_ptr(self.device),
                      prof.handle if prof is not None else 0, device=self.device)
            return out, nbytes
        _lib.call("stabnet_mjpeg_encode", ptr(img), n, self.H, self.W, self.C, self.subsampling, self.restart_mcus,
                  ptr(self._tables), self._tables.data_ptr() + 128, ptr(self._header), len(self.header), ptr(out), out.stride(0),
                  ptr(nbytes), ptr(self.workspace), self.workspace.numel(), stream_ptr(self.device),
                  prof.handle if prof is not None else 0, device=self.device)
        return out, nbytes

    def encode_bytes(self, img):
        out, nbytes = self.encode(img)
        lens = nbytes.cpu().tolist()
        return [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lens)]


class Unsupported(_lib.StabnetError):
    """A JPEG stream the device decoder does not take (progressive, 4:2:2, 12-bit, several scans ...): decode it with Pillow."""


def planar_refusal(H, W, channels, subsampling):
    """None when the planar decoder takes such a stream, else the phrase that names the sampling and the odd side."""
    if int(channels) != 3:
        return None
    if int(subsampling) != 420:
        return "a %dx%d stream sampled 4:4:4 (planar frames are 4:2:0 or grey)" % (W, H)
    odd = [n for n, v in (("width %d" % W, W), ("height %d" % H, H)) if v & 1]
    if odd:
        return "a 4:2:0 stream of %dx%d with an odd %s (its chroma planes are not H/2 x W/2)" % (W, H, " and ".join(odd))
    return None


def parse(jpeg, blob_ptr=0, blob_cap=0):
    """stabnet_mjpeg_parse -> dict(H, W, C, subsampling, restart (0: no DRI), intervals, mcus, scan, eoi, blob_bytes, has_dht, blocks).
    Raises Unsupported for a stream outside the decoder's scope, StabnetError for one that is no complete JPEG stream."""
    jpeg = bytes(jpeg)
    info = (ctypes.c_int * 16)()
    rc = _lib.lib().stabnet_mjpeg_parse(jpeg, len(jpeg), info, blob_ptr, blob_cap)
    if rc != 0:
        msg = _lib.lib().stabnet_last_error()
        msg = msg.decode() if msg else "?"
        raise (Unsupported if rc == 1 else _lib.StabnetError)(msg)
    keys = ("H", "W", "C", "subsampling", "restart", "intervals", "mcus", "scan", "eoi", "blob_bytes", "has_dht", "blocks")
    return dict(zip(keys, list(info)))


class MjpegDecoder:
    """Owns the pinned staging slots, their device copies, the workspace and the status words of one frame geometry.

    decode(list_of_bytes) -> uint8 [N,H,W,3] BGR ([N,H,W] for grey streams) on the device.  Per frame the parsed description (tables,
    restart-interval offsets: stabnet_mjpeg_parse) and the compressed bytes travel in ONE copy; streams with restart intervals (DRI)
    are entropy-decoded on the device, one lane per interval.  host_entropy=True (the default for a decoder made from a stream
    without DRI, which is a single interval): the coefficients are decoded on the CPU by the same routine and uploaded instead; the
    IDCT and colour stages are the device's either way, so the pixels are the same.
    parallel=True (opt-in; excludes host_entropy): the second entropy back end, for streams WITHOUT restart markers -- the slot holds
    blob + bytes and the one interval is decoded on the device by self-synchronising parallel Huffman decoding
    (csrc/mjpeg_decode_sync.hip: one lane per chunk of chunk_bytes, at most sync_rounds rounds of state hand-over, a sequential
    repair of what is left); the same coefficients, hence the same pixels.  None for chunk_bytes / sync_rounds: the library's defaults.
    enqueue(...) only launches (capturable in a hipGraph); decode(...) also checks the status words, which synchronises.
    planar=True (any back end): the frame is left in YCbCr -- enqueue / decode fill uint8 [N, frame_bytes], each row Y [H,W] and, for colour,
    U (Cb) and V (Cr) [H/2,W/2] behind it, dense: what warpRevBundle2_i420 and a planar MjpegEncoder read (stabnet_mjpeg_decode_i420 /
    _sync_i420).  Grey streams of any size and 4:2:0 streams with even H and W; Unsupported for 4:4:4 and for an odd side."""

    def __init__(self, H: int, W: int, channels: int = 3, subsampling="420", device="cuda:0", batch: int = 1, host_entropy: bool = False,
                 max_bytes=None, parallel: bool = False, chunk_bytes=None, sync_rounds=None, planar: bool = False):
        self.H, self.W, self.C = int(H), int(W), int(channels)
        self.subsampling = int(subsampling) if self.C == 3 else 0
        self.planar = bool(planar)
        why = planar_refusal(self.H, self.W, self.C, self.subsampling) if self.planar else None
        if why:
            raise Unsupported("MjpegDecoder: planar=True does not take " + why)
        self.frame_bytes = planar_frame_bytes(self.H, self.W, self.C)
        self.device = torch.device(device)
        self.host_entropy = bool(host_entropy)
        self.parallel = bool(parallel)
        if self.parallel and self.host_entropy:
            raise _lib.StabnetError("MjpegDecoder: parallel=True decodes the entropy-coded bytes on the device; it excludes host_entropy=True")
        if not self.parallel and (chunk_bytes is not None or sync_rounds is not None):
            raise _lib.StabnetError("MjpegDecoder: chunk_bytes / sync_rounds belong to parallel=True")
        self.chunk_bytes = 0 if chunk_bytes is None else int(chunk_bytes)
        self.sync_rounds = -1 if sync_rounds is None else int(sync_rounds)
        if self.parallel and (self.chunk_bytes < 0 or self.sync_rounds < -1):
            raise _lib.StabnetError("MjpegDecoder: chunk_bytes %d / sync_rounds %d" % (self.chunk_bytes, self.sync_rounds))
        L = _lib.lib()
        self.blob_max = L.stabnet_mjpeg_decode_blob_bytes(self.H, self.W, self.C, self.subsampling)
        if self.blob_max == 0:
            _lib.check(-1, "stabnet_mjpeg_decode_blob_bytes")
        lay = (ctypes.c_size_t * 10)()
        _lib.call("stabnet_mjpeg_decode_layout", self.H, self.W, self.C, self.subsampling, lay)
        self.layout = dict(zip(("frame", "coef", "blocks", "y", "cb", "cr", "yh", "yw", "ch", "cw"), [int(v) for v in lay]))
        self.coef_count = self.layout["blocks"] * 64
        # a JPEG frame is rarely longer than the raw one; a longer one makes the slots grow
        payload = 2 * self.coef_count if self.host_entropy else int(max_bytes or (self.H * self.W * self.C + 4096))
        self.in_stride = (self.blob_max + payload + 15) & ~15
        self._batch = 0
        self._ev = None
        self._reserve(batch)

    @classmethod
    def for_stream(cls, jpeg, device="cuda:0", batch: int = 1, host_entropy=None, parallel=None, chunk_bytes=None, sync_rounds=None,
                   planar: bool = False):
        """A decoder for streams shaped like this one (raises Unsupported).  parallel=True: a stream without DRI gets the parallel
        entropy back end; one with DRI keeps one lane per restart interval.  The default (None) is host_entropy for a stream without DRI."""
        i = parse(jpeg)
        if parallel and i["restart"] == 0 and not host_entropy:
            return cls(i["H"], i["W"], i["C"], i["subsampling"] or 420, device=device, batch=batch, parallel=True, chunk_bytes=chunk_bytes,
                       sync_rounds=sync_rounds, planar=planar)
        return cls(i["H"], i["W"], i["C"], i["subsampling"] or 420, device=device, batch=batch,
                   host_entropy=(i["restart"] == 0) if host_entropy is None else host_entropy, planar=planar)

    def _reserve(self, n: int, in_stride=None):
        if n <= self._batch and in_stride is None:
            return
        if self._ev is not None:
            self._ev.synchronize()
        n = max(n, self._batch)
        self.in_stride = in_stride or self.in_stride
        self.h_in = torch.zeros((n, self.in_stride), dtype=torch.uint8).pin_memory()
        self.d_in = torch.zeros((n, self.in_stride), dtype=torch.uint8, device=self.device)
        if self.parallel:
            ws = _lib.lib().stabnet_mjpeg_decode_sync_workspace_bytes(n, self.H, self.W, self.C, self.subsampling, self.in_stride, self.chunk_bytes)
        else:
            ws = _lib.lib().stabnet_mjpeg_decode_workspace_bytes(n, self.H, self.W, self.C, self.subsampling)
        if ws == 0:
            _lib.check(-1, "stabnet_mjpeg_decode%s_workspace_bytes" % ("_sync" if self.parallel else ""))
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.sync_stats = torch.zeros((n, 2), dtype=torch.int32, device=self.device) if self.parallel else None
        if self.planar:
            self.out = torch.empty((n, self.frame_bytes), dtype=torch.uint8, device=self.device)
        else:
            self.out = torch.empty((n, self.H, self.W, self.C), dtype=torch.uint8, device=self.device)
        self._batch = n

    def slot_bytes(self, nbytes: int) -> int:
        return self.blob_max + (2 * self.coef_count if self.host_entropy else int(nbytes))

    def stage(self, jpeg, slot, frame=None) -> int:
        """Parse one stream into a pinned slot (uint8 [>= in_stride]: blob, then the bytes or the host-decoded coefficients).
        -> the bytes of the slot to upload.  `frame` names the frame in errors."""
        jpeg = bytes(jpeg)
        what = "MjpegDecoder" if frame is None else "MjpegDecoder: frame %s" % (frame,)
        base = slot.data_ptr()
        try:
            i = parse(jpeg, base, self.blob_max)
        except _lib.StabnetError as e:
            raise type(e)("%s: %s" % (what, e))
        if (i["H"], i["W"], i["C"], i["subsampling"]) != (self.H, self.W, self.C, self.subsampling):
            raise _lib.StabnetError("%s is %dx%dx%d sampled %d, the decoder was made for %dx%dx%d sampled %d"
                                    % (what, i["W"], i["H"], i["C"], i["subsampling"], self.W, self.H, self.C, self.subsampling))
        used = self.slot_bytes(len(jpeg))
        if used > slot.numel():
            raise _lib.StabnetError("%s: %d bytes do not fit the slot of %d" % (what, used, slot.numel()))
        if self.parallel and i["intervals"] != 1:
            raise _lib.StabnetError("%s has %d restart intervals (DRI %d); the decoder was made with parallel=True for streams without "
                                    "restart markers" % (what, i["intervals"], i["restart"]))
        if self.host_entropy:
            rc = _lib.lib().stabnet_mjpeg_entropy_host(jpeg, len(jpeg), base, i["blob_bytes"], base + self.blob_max, self.coef_count)
            if rc != 0:
                msg = _lib.lib().stabnet_last_error()
                raise _lib.StabnetError("%s: %s" % (what, msg.decode() if msg else "?"))
        else:
            slot[self.blob_max:used].numpy()[...] = np.frombuffer(jpeg, np.uint8)
        return used

    def enqueue(self, d_in, n: int, out, status, stages: int = 3, prof=None):
        """The launches alone, on the current stream: d_in uint8 [n, in_stride] as uploaded, out uint8 [n,H,W,C] (rows and frames at
        its strides), status int32 [n].  parallel: the chunk statistics of the call land in sync_stats[:n] when d_in is the decoder's
        own batch (otherwise they are not kept).  planar: out uint8 [n, frame_bytes] (rows at its stride), stages must stay 3; prof
        records the launch that crops the planes."""
        if self.planar:
            if stages != 3:
                raise _lib.StabnetError("MjpegDecoder: planar=True has no stages; the BGR decoder stops early for tests")
            if out is None or out.dim() != 2 or out.shape[1] != self.frame_bytes or out.stride(1) != 1:
                raise _lib.StabnetError("MjpegDecoder: planar=True fills uint8 [n, %d] with dense rows" % self.frame_bytes)
            stride = max(out.stride(0), self.frame_bytes)
            hp = prof.handle if prof is not None else 0
            if self.parallel:
                stats = self.sync_stats if d_in is self.d_in and n <= self.sync_stats.shape[0] else None
                _lib.call("stabnet_mjpeg_decode_sync_i420", ptr(d_in), d_in.stride(0), n, self.H, self.W, self.C, self.subsampling, ptr(out),
                          stride, ptr(status), ptr(self.workspace), self.workspace.numel(), self.chunk_bytes, self.sync_rounds, ptr(stats),
                          stream_ptr(self.device), hp, device=self.device)
            else:
                _lib.call("stabnet_mjpeg_decode_i420", ptr(d_in), d_in.stride(0), n, self.H, self.W, self.C, self.subsampling,
                          int(self.host_entropy), ptr(out), stride, ptr(status), ptr(self.workspace), self.workspace.numel(),
                          stream_ptr(self.device), hp, device=self.device)
            return
        if self.parallel:
            stats = self.sync_stats if d_in is self.d_in and n <= self.sync_stats.shape[0] else None
            _lib.call("stabnet_mjpeg_decode_sync", ptr(d_in), d_in.stride(0), n, self.H, self.W, self.C, self.subsampling, ptr(out),
                      out.stride(1) if out is not None else 0, out.stride(0) if out is not None else 0, ptr(status), ptr(self.workspace),
                      self.workspace.numel(), stages, self.chunk_bytes, self.sync_rounds, ptr(stats), stream_ptr(self.device),
                      device=self.device)
            return
        _lib.call("stabnet_mjpeg_decode", ptr(d_in), d_in.stride(0), n, self.H, self.W, self.C, self.subsampling, int(self.host_entropy),
                  ptr(out), out.stride(1) if out is not None else 0, out.stride(0) if out is not None else 0, ptr(status),
                  ptr(self.workspace), self.workspace.numel(), stages, stream_ptr(self.device), device=self.device)

    def check(self, status, first_frame: int = 0):
        bad = [(first_frame + i, int(v)) for i, v in enumerate(status.cpu().tolist()) if v]
        if bad:
            raise _lib.StabnetError("MjpegDecoder: frame %d does not decode on the device (status %d: 1 data ran out, 2 no such Huffman "
                                    "code, 4 run past coefficient 63, 8 bad description)" % bad[0])

    def decode(self, jpegs, out=None, first_frame: int = 0, check: bool = True):
        """jpegs: list of bytes of one geometry.  out: the caller's uint8 [N,H,W,C] device tensor ([N, frame_bytes] for planar=True)
        instead of the decoder's own."""
        if isinstance(jpegs, (bytes, bytearray, memoryview)):
            jpegs = [jpegs]
        n = len(jpegs)
        need = max(self.slot_bytes(len(j)) for j in jpegs)
        self._reserve(n, ((need + 4095) & ~4095) if need > self.in_stride else None)
        if self._ev is not None:
            self._ev.synchronize()                     # the staging slots are free again once their last upload has landed
        used = [self.stage(j, self.h_in[k], first_frame + k) for k, j in enumerate(jpegs)]
        for k, u in enumerate(used):
            self.d_in[k, :u].copy_(self.h_in[k, :u], non_blocking=True)
        self._ev = torch.cuda.Event()
        self._ev.record(torch.cuda.current_stream(self.device))
        if out is None:
            out = self.out[:n]
        self.enqueue(self.d_in, n, out if self.planar else out.view(n, self.H, self.W, self.C), self.status[:n])
        if check:
            self.check(self.status[:n], first_frame)
        if self.planar:
            return out
        return out if self.C == 3 else out.view(n, self.H, self.W)


class DeviceClip:
    """The frames of an MJPG .avi (avi.AviMjpegReader) decoded on the device as they are asked for: what crosses PCIe per frame is the
    compressed frame.  device_frame(t) -> uint8 [H,W,3] BGR / [H,W] grey in the decoder's own buffer (valid until the next call):
    the tensor the ingest reads.  clip[t] is the same frame downloaded (NumPy), for the few places that want it on the host.
    parallel=True: a clip without restart markers is entropy-decoded on the device too (MjpegDecoder parallel=True) instead of on the host.
    Raises Unsupported when the first frame is outside the decoder's scope."""

    def __init__(self, reader, device="cuda:0", parallel: bool = False):
        self.reader = reader
        self.decoder = MjpegDecoder.for_stream(reader.jpeg(0), device=device, parallel=True if parallel else None)

    def __len__(self):
        return len(self.reader)

    def jpeg(self, t: int) -> bytes:
        return self.reader.jpeg(t)

    def device_frame(self, t: int):
        return self.decoder.decode([self.reader.jpeg(t)], first_frame=t)[0]

    def __getitem__(self, t: int):
        return self.device_frame(t).cpu().numpy()
