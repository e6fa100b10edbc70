"""CPU: the plain-Python Motion-JPEG AVI writer and reader (stabnet_amd/avi.py).  Frames encoded by Pillow go through writer -> reader
byte for byte; tests/riff_walk.py walks the RIFF tree on its own and checks every chunk size, the even padding and the index."""
import io

import numpy as np
import pytest

import riff_walk


def _jpegs(n, W=40, H=24, odd=None):
    from PIL import Image
    rng = np.random.default_rng(3)
    out = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(buf, "JPEG", quality=30 + 5 * i)
        b = buf.getvalue()
        if odd is not None and (len(b) & 1) != odd:
            b = b[:-2] + b"\x00" + b[-2:]           # a fill byte before EOI: still a JPEG for our purposes, parity as asked
        out.append(b)
    return out


@pytest.mark.parametrize("n,fps", [(5, 30), (1, 25), (7, 29.97), (0, 30)])
def test_writer_reader_round_trip_and_riff_arithmetic(tmp_path, n, fps):
    from stabnet_amd.avi import AviMjpegReader, AviMjpegWriter
    frames = _jpegs(n)
    path = str(tmp_path / "a.avi")
    with AviMjpegWriter(path, 40, 24, fps) as w:
        for f in frames:
            w.write(f)
    assert w.closed and w.frames_written == n
    t = riff_walk.walk(path)
    assert len(t["frames"]) == n == len(t["idx1"])
    assert t["avih"][4] == n and t["strh"]["length"] == n                                      # dwTotalFrames, dwLength
    assert t["avih"][0] == int(round(1e6 / fps))                                               # dwMicroSecPerFrame
    assert t["avih"][3] & 0x10 and t["avih"][6] == 1 and (t["avih"][8], t["avih"][9]) == (40, 24)
    assert abs(t["strh"]["rate"] / t["strh"]["scale"] - fps) < 1e-3
    assert t["strh"]["type"] == b"vids" and t["strh"]["handler"] == b"MJPG" and t["strh"]["rect"] == (0, 0, 40, 24)
    assert t["strf"] == dict(size=40, width=40, height=24, planes=1, bits=24, compression=b"MJPG")
    assert [riff_walk.jpeg_of(t, i) for i in range(n)] == frames
    r = AviMjpegReader(path)
    assert len(r) == n and r.size == (40, 24) and abs(r.fps - fps) < 1e-3 and r.total_frames == n
    assert [r.jpeg(i) for i in range(n)] == frames
    dec = list(r.frames())
    assert len(dec) == n and all(f.shape == (24, 40, 3) and f.dtype == np.uint8 for f in dec)


def test_odd_and_even_lengths_are_padded_to_even_offsets(tmp_path):
    from stabnet_amd.avi import AviMjpegReader, AviMjpegWriter
    frames = _jpegs(3, odd=1) + _jpegs(2, odd=0) + [b"\xff\xd8\xff\xd9", b"\xff\xd8\x00\xff\xd9"]
    assert {len(f) & 1 for f in frames} == {0, 1}
    path = str(tmp_path / "odd.avi")
    w = AviMjpegWriter(path, 40, 24, 30)
    for f in frames:
        w.write(f)
    w.close()
    w.close()                                       # idempotent
    t = riff_walk.walk(path)
    assert [riff_walk.jpeg_of(t, i) for i in range(len(frames))] == frames
    assert all(p % 2 == 0 for p, _ in t["frames"])
    assert [AviMjpegReader(path).jpeg(i) for i in range(len(frames))] == frames


def test_two_gib_guard_closes_a_valid_file(tmp_path, monkeypatch):
    from stabnet_amd import avi
    frames = _jpegs(4)
    path = str(tmp_path / "big.avi")
    head = 12 + 8 + 4 + 8 + 56 + 8 + 4 + 8 + 56 + 8 + 40 + 12                       # everything before the first 00dc chunk
    room = head + sum(8 + len(f) + (len(f) & 1) for f in frames[:2]) + 8 + 16 * 2    # exactly two frames and their index fit
    monkeypatch.setattr(avi, "AVI_MAX_BYTES", room)
    w = avi.AviMjpegWriter(path, 40, 24, 30)
    w.write(frames[0])
    w.write(frames[1])
    with pytest.raises(avi.AviError, match="AVI 1.0"):
        w.write(frames[2])
    assert w.closed
    with pytest.raises(avi.AviError):
        w.write(frames[3])
    t = riff_walk.walk(path)
    assert len(t["data"]) == room and len(t["frames"]) == 2 and t["avih"][4] == 2
    assert [avi.AviMjpegReader(path).jpeg(i) for i in range(2)] == frames[:2]


def test_reader_rejects_other_files(tmp_path):
    from stabnet_amd import avi
    p = tmp_path / "x.avi"
    p.write_bytes(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(avi.AviError):
        avi.AviMjpegReader(str(p))
    with pytest.raises(avi.AviError):
        avi.AviMjpegWriter(str(tmp_path / "y.avi"), 8, 8, 0)
