"""YUV4MPEG2 ("Y4M") streams on the host, pure Python: a text header line, then per frame a `FRAME` line and the raw planar bytes -- Y
[H,W], then U and V [H/2,W/2] for the 4:2:0 kinds, nothing after Y for `Cmono`.  The dependency-free bridge every video tool speaks,
through a file or a pipe:  ffmpeg -i in.mp4 -f yuv4mpegpipe - | deploy_bundle.py --y4m-in - --y4m-out - | ffmpeg -i - out.mp4

Read and written: 8-bit progressive 4:2:0 (`C420jpeg`, `C420mpeg2`, `C420paldv`, `C420`; a missing C token means `C420`) and `Cmono`.
The four 4:2:0 tags differ in where the chroma samples sit; that difference is IGNORED (the planar warp treats chroma as
centred) and the tag is passed through.  Everything else is refused with Y4mError."""
from __future__ import annotations

import sys

MAGIC = b"YUV4MPEG2"
MAX_HEADER = 256                     # bytes of a header or FRAME line, the newline included
CHROMA_420 = ("420jpeg", "420mpeg2", "420paldv", "420")
CHROMA = CHROMA_420 + ("mono",)
MAX_SIDE = 32767                     # the remap's 16-bit pixel index


class Y4mError(ValueError):
    pass


def default_range(chroma: str) -> str:
    """'full' for C420jpeg and Cmono, 'limited' otherwise (the convention of the tools that write these tags)."""
    return "full" if chroma in ("420jpeg", "mono") else "limited"


def frame_size(width: int, height: int, chroma: str) -> int:
    return width * height if chroma == "mono" else width * height * 3 // 2


def _check_geometry(width, height, chroma):
    if chroma not in CHROMA:
        raise Y4mError("Y4M: chroma 'C%s' is not supported: only 8-bit 4:2:0 (%s) and Cmono streams are"
                       % (chroma, ", ".join("C" + c for c in CHROMA_420)))
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise Y4mError("Y4M: frame size %dx%d outside 1..%d" % (width, height, MAX_SIDE))
    if chroma != "mono" and (width % 2 or height % 2):
        raise Y4mError("Y4M: a 4:2:0 stream needs an even width and height, got %dx%d" % (width, height))


class Y4mReader:
    """Y4mReader(path or '-' or a binary file object).  Attributes: width, height, fps (num, den), aspect (num, den) or None, chroma
    ('420jpeg' ..., 'mono': the C token without its C; '420' when there is none), colour_range ('full' / 'limited'), range_given (the
    header had an XCOLORRANGE token), frame_bytes, frames_read.  read_into(buf) fills a caller-owned writable buffer with the next frame."""

    def __init__(self, path_or_file):
        self._own = False
        if path_or_file == "-":
            self._f = sys.stdin.buffer
        elif isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__"):
            self._f, self._own = open(path_or_file, "rb"), True
        else:
            self._f = path_or_file
        self.frames_read = 0
        try:
            self._parse_header()
        except Exception:
            self.close()
            raise

    def _read_line(self, what):
        """One line without its newline; None at a clean end of stream before the line's first byte."""
        line = bytearray()
        while True:
            c = self._f.read(1)
            if not c:
                if line:
                    raise Y4mError("Y4M: %s: the stream ends inside the line %r" % (what, bytes(line[:40])))
                return None
            if c == b"\n":
                return bytes(line)
            line += c
            if len(line) >= MAX_HEADER:
                raise Y4mError("Y4M: %s: a line longer than %d bytes" % (what, MAX_HEADER))

    def _parse_header(self):
        line = self._read_line("header")
        tokens = (line or b"").split(b" ")
        if tokens[0] != MAGIC:
            raise Y4mError("Y4M: the stream does not start with %s" % MAGIC.decode())
        width = height = None
        self.fps, self.aspect, self.interlace = (0, 0), None, None
        chroma, rng = None, None
        try:
            for tok in tokens[1:]:
                if not tok:
                    continue
                key, val = tok[:1], tok[1:].decode("ascii")
                if key == b"W":
                    width = int(val)
                elif key == b"H":
                    height = int(val)
                elif key == b"F":
                    n, d = val.split(":")
                    self.fps = (int(n), int(d))
                    if self.fps[0] <= 0 or self.fps[1] <= 0:
                        raise Y4mError("Y4M: frame rate F%s has a zero term" % val)
                elif key == b"A":
                    n, d = val.split(":")
                    self.aspect = (int(n), int(d))
                elif key == b"I":
                    self.interlace = val
                elif key == b"C":
                    chroma = val
                elif key == b"X" and val.startswith("COLORRANGE="):
                    rng = val[len("COLORRANGE="):].lower()
                    if rng not in ("full", "limited"):
                        raise Y4mError("Y4M: XCOLORRANGE=%s is neither FULL nor LIMITED" % val[len("COLORRANGE="):])
                # other X tokens, and unknown keys: ignored
        except (ValueError, UnicodeDecodeError) as e:
            if isinstance(e, Y4mError):
                raise
            raise Y4mError("Y4M: malformed header token in %r" % line[:80])
        if width is None or height is None:
            raise Y4mError("Y4M: the header names no W and H")
        if self.fps == (0, 0):
            raise Y4mError("Y4M: the header names no frame rate F")
        if self.interlace not in (None, "p", "?"):
            raise Y4mError("Y4M: interlaced streams (I%s) are not supported: only progressive (Ip, I? or no I token)" % self.interlace)
        self.chroma = "420" if chroma is None else chroma
        _check_geometry(width, height, self.chroma)
        self.width, self.height = width, height
        self.colour_range = rng if rng is not None else default_range(self.chroma)
        self.range_given = rng is not None
        self.frame_bytes = frame_size(width, height, self.chroma)

    def read_into(self, buf) -> bool:
        """Fill `buf` (writable, frame_bytes long) with the next frame, Y then U then V.  False at a clean end of stream on a frame
        boundary; Y4mError naming the frame on a truncated frame or a line that is not `FRAME[ params]`."""
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("Y4mReader.read_into: the buffer holds %d bytes, a frame has %d" % (len(mv), self.frame_bytes))
        n = self.frames_read
        line = self._read_line("frame %d" % n)
        if line is None:
            return False
        if line != b"FRAME" and not line.startswith(b"FRAME "):
            raise Y4mError("Y4M: frame %d: expected a FRAME line, got %r" % (n, line[:40]))
        got = 0
        readinto = getattr(self._f, "readinto", None)
        while got < len(mv):                                 # a pipe hands over what it has: loop over short reads
            if readinto is not None:
                k = readinto(mv[got:])
            else:
                chunk = self._f.read(len(mv) - got)
                k = len(chunk)
                mv[got:got + k] = chunk
            if not k:
                raise Y4mError("Y4M: frame %d is truncated: %d of %d bytes" % (n, got, len(mv)))
            got += k
        self.frames_read = n + 1
        return True

    def header_fields(self):
        return {"width": self.width, "height": self.height, "fps": list(self.fps), "aspect": list(self.aspect) if self.aspect else None,
                "chroma": self.chroma, "colour_range": self.colour_range, "frame_bytes": self.frame_bytes}

    def close(self):
        if self._own:
            self._f.close()
            self._own = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4mWriter:
    """Y4mWriter(path or '-' or a binary file object, width, height, fps=(num, den), chroma, aspect=None, colour_range=None): the header
    is written on construction (C<chroma>, Ip, and XCOLORRANGE when colour_range is given); write(buf) writes `FRAME` and the bytes;
    close() flushes.  A consumer that closes the pipe ends the writing quietly: write() then returns False (broken is set) and every
    later write is dropped."""

    def __init__(self, path_or_file, width, height, fps, chroma, aspect=None, colour_range=None):
        width, height, fps = int(width), int(height), (int(fps[0]), int(fps[1]))
        _check_geometry(width, height, chroma)
        if fps[0] <= 0 or fps[1] <= 0:
            raise Y4mError("Y4M: frame rate %d:%d has a zero term" % fps)
        if colour_range not in (None, "full", "limited"):
            raise Y4mError("Y4M: colour_range must be 'full', 'limited' or None, got %r" % (colour_range,))
        self.width, self.height, self.fps, self.chroma = width, height, fps, chroma
        self.frame_bytes = frame_size(width, height, chroma)
        self.frames_written, self.broken, self._own = 0, False, False
        if path_or_file == "-":
            self._f = sys.stdout.buffer
        elif isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__"):
            self._f, self._own = open(path_or_file, "wb"), True
        else:
            self._f = path_or_file
        head = "%s W%d H%d F%d:%d Ip" % (MAGIC.decode(), width, height, fps[0], fps[1])
        if aspect is not None:
            head += " A%d:%d" % (int(aspect[0]), int(aspect[1]))
        head += " C%s" % chroma
        if colour_range is not None:
            head += " XCOLORRANGE=%s" % colour_range.upper()
        self._put(head.encode("ascii") + b"\n")

    def _put(self, *parts):
        if self.broken:
            return False
        try:
            for p in parts:
                self._f.write(p)
            return True
        except BrokenPipeError:
            self.broken = True
            return False

    def write(self, buf) -> bool:
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("Y4mWriter.write: the buffer holds %d bytes, a frame has %d" % (len(mv), self.frame_bytes))
        ok = self._put(b"FRAME\n", mv)
        if ok:
            self.frames_written += 1
        return ok

    def close(self):
        if self._f is None:
            return
        try:
            if not self.broken:
                self._f.flush()
            if self._own:
                self._f.close()
        except BrokenPipeError:
            self.broken = True
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
