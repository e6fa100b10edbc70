"""Motion-JPEG in RIFF AVI 1.0, plain Python (host code only): what cv2.VideoWriter(path, fourcc('MJPG'), fps, (w, h)) of the reference
(deploy_bundle.py:197-198) produces, without OpenCV.  One video stream, every frame a complete JPEG in a `00dc` chunk, an `idx1` index.

Layout:  RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' (vids / MJPG), 'strf' (BITMAPINFOHEADER, biCompression MJPG) } },
                       LIST 'movi' { '00dc' ... }, 'idx1' }
Chunks are padded to even length (the pad byte is not counted in the chunk's size).  AVI 1.0 sizes are 32-bit and most readers treat
them as signed: the writer refuses the frame that would take the file past 2 GiB - 1 and leaves a valid file behind."""
from __future__ import annotations

import io
import struct
from fractions import Fraction

AVI_MAX_BYTES = (1 << 31) - 1
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


class AviError(RuntimeError):
    pass


def _rate_scale(fps):
    f = Fraction(fps).limit_denominator(100000)
    if f <= 0:
        raise AviError("fps must be positive")
    return f.numerator, f.denominator


class AviMjpegWriter:
    def __init__(self, path, width: int, height: int, fps=30):
        self.path, self.width, self.height, self.fps = path, int(width), int(height), fps
        self.rate, self.scale = _rate_scale(fps)
        self._index = []                   # (offset from the 'movi' fourcc, size)
        self._max_frame = 0
        self._f = open(path, "wb")
        self._write_headers(0)
        self._movi_fourcc = self._f.tell() - 4
        self.closed = False

    def _write_headers(self, nframes: int):
        f = self._f
        usec = int(round(1e6 * self.scale / self.rate))
        avih = struct.pack("<14I", usec, int(self._max_frame * self.rate / self.scale), 0, AVIF_HASINDEX, nframes, 0, 1,
                           self._max_frame, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, nframes, self._max_frame,
                           0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        movi_size = 4 + sum(8 + s + (s & 1) for _, s in self._index)
        idx_size = 16 * len(self._index)
        riff_size = 4 + (8 + len(hdrl)) + (8 + movi_size) + (8 + idx_size)
        f.seek(0)
        f.write(b"RIFF" + struct.pack("<I", riff_size) + b"AVI ")
        f.write(b"LIST" + struct.pack("<I", len(hdrl)) + hdrl)
        f.write(b"LIST" + struct.pack("<I", movi_size) + b"movi")

    def write(self, jpeg):
        """Append one frame: a complete JPEG stream (bytes-like)."""
        if self.closed:
            raise AviError("write on a closed AviMjpegWriter")
        jpeg = bytes(jpeg)
        n = len(jpeg)
        pos = self._f.tell()
        after = pos + 8 + n + (n & 1) + 8 + 16 * (len(self._index) + 1)
        if after > AVI_MAX_BYTES:
            self.close()
            raise AviError("%s: frame %d would take the file to %d bytes, past the %d of AVI 1.0 (OpenDML is not written); "
                           "the file was closed with %d frames" % (self.path, len(self._index), after, AVI_MAX_BYTES, len(self._index)))
        self._f.write(b"00dc" + struct.pack("<I", n) + jpeg + (b"\0" if n & 1 else b""))
        self._index.append((pos - self._movi_fourcc, n))
        self._max_frame = max(self._max_frame, n)

    @property
    def frames_written(self):
        return len(self._index)

    def close(self):
        if self.closed:
            return
        f = self._f
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        for off, n in self._index:
            f.write(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, n))
        self._write_headers(len(self._index))            # sizes, dwTotalFrames, dwLength, buffer sizes
        f.close()
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class AviMjpegReader:
    """Frame count, fps, size and the JPEG bytes of frame i of an MJPG AVI; frames() decodes with Pillow, device_clip() on the GPU."""

    def __init__(self, path, mapped: bool = False):
        """mapped=True: the file is memory-mapped, not read: a clip of any length costs its index (two ints per frame), and jpeg(i)
        copies one frame out of the page cache."""
        self.path = path
        with open(path, "rb") as f:
            if mapped:
                import mmap
                f.seek(0, 2)
                data = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if f.tell() > 0 else b""
            else:
                data = f.read()
        if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise AviError("%s: not a RIFF AVI file" % path)
        self._data = data
        self.width = self.height = 0
        self.fps = 0.0
        self.rate = self.scale = 0
        self.handler = self.compression = b""
        self.total_frames = 0
        self._frames = []                  # (offset of the payload, size)
        self._walk(12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0]))
        if self.compression.upper() != b"MJPG" and self.handler.upper() != b"MJPG":
            raise AviError("%s: video stream is %r / %r, only MJPG is read" % (path, self.handler, self.compression))

    def _walk(self, p, end):
        d = self._data
        while p + 8 <= end:
            cid, size = d[p:p + 4], struct.unpack_from("<I", d, p + 4)[0]
            body = p + 8
            if cid == b"LIST":
                kind = d[body:body + 4]
                if kind == b"movi":
                    self._walk_movi(body + 4, body + size)
                else:
                    self._walk(body + 4, body + size)
            elif cid == b"avih":
                v = struct.unpack_from("<14I", d, body)
                self.usec_per_frame, self.total_frames = v[0], v[4]
            elif cid == b"strh" and d[body:body + 4] == b"vids":
                self.handler = d[body + 4:body + 8]
                self.scale, self.rate = struct.unpack_from("<II", d, body + 20)
                self.fps = self.rate / self.scale if self.scale else 0.0
            elif cid == b"strf" and not self.compression:
                _, self.width, self.height, _, _, self.compression = struct.unpack_from("<IiiHH4s", d, body)
                self.height = abs(self.height)
            p = body + size + (size & 1)

    def _walk_movi(self, p, end):
        d = self._data
        while p + 8 <= end:
            cid, size = d[p:p + 4], struct.unpack_from("<I", d, p + 4)[0]
            if cid == b"LIST":                             # 'rec ' groups
                self._walk_movi(p + 12, p + 8 + size)
            elif cid[2:4] in (b"dc", b"db") and size > 0:
                self._frames.append((p + 8, size))
            p += 8 + size + (size & 1)

    def __len__(self):
        return len(self._frames)

    @property
    def size(self):
        return self.width, self.height

    def jpeg(self, i: int) -> bytes:
        off, n = self._frames[i]
        return bytes(self._data[off:off + n])

    def frame(self, i: int):
        """Frame i decoded by Pillow: uint8 [H,W] (grey JPEG) or [H,W,3] in BGR order (as the rest of the project keeps colour)."""
        import numpy as np
        from PIL import Image
        im = Image.open(io.BytesIO(self.jpeg(i)))
        if im.mode == "L":
            return np.asarray(im)
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])

    def frames(self):
        for i in range(len(self)):
            yield self.frame(i)

    def device_clip(self, device="cuda:0", parallel: bool = False):
        """The same frames decoded on the device from jpeg(i), bit for bit what frame(i) gives where Pillow is built on libjpeg-turbo
        (mjpeg.DeviceClip; raises mjpeg.Unsupported for streams outside the device decoder's scope)."""
        from .mjpeg import DeviceClip
        return DeviceClip(self, device, parallel=parallel)
