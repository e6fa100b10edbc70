"""CPU: the Y4M reader and writer (stabnet_amd/y4m.py), the driver's new flags, and the limited-range table of the ingest."""
import io
import os
import random
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stabnet_amd import y4m  # noqa: E402


def _stream(header, frames, frame_line=b"FRAME\n"):
    return header + b"".join(frame_line + bytes(f) for f in frames)


def _frames(n, nbytes, seed=0):
    return list(np.random.default_rng(seed).integers(0, 256, (n, nbytes), dtype=np.uint8))


def _read_all(rd):
    buf, out = bytearray(rd.frame_bytes), []
    while rd.read_into(buf):
        out.append(bytes(buf))
    return out


@pytest.mark.parametrize("chroma,w,h", [("420mpeg2", 16, 10), ("420jpeg", 6, 4), ("420paldv", 2, 2), ("420", 18, 6), ("mono", 7, 5)])
def test_writer_to_reader_round_trip_is_byte_for_byte(tmp_path, chroma, w, h):
    nbytes = y4m.frame_size(w, h, chroma)
    assert nbytes == (w * h if chroma == "mono" else w * h * 3 // 2)
    frames = _frames(5, nbytes, seed=w)
    path = str(tmp_path / "a.y4m")
    with y4m.Y4mWriter(path, w, h, (30000, 1001), chroma, aspect=(4, 3), colour_range="full") as wr:
        for f in frames:
            assert wr.write(f)
        assert wr.frames_written == 5
    with y4m.Y4mReader(path) as rd:
        assert (rd.width, rd.height, rd.fps, rd.aspect, rd.chroma, rd.colour_range, rd.frame_bytes) == (w, h, (30000, 1001), (4, 3), chroma, "full", nbytes)
        assert _read_all(rd) == [bytes(f) for f in frames] and rd.frames_read == 5
    # file objects on both sides, and a wrong-sized buffer
    bio = io.BytesIO()
    wr = y4m.Y4mWriter(bio, w, h, (25, 1), chroma)
    wr.write(frames[0])
    with pytest.raises(ValueError):
        wr.write(bytes(nbytes + 1))
    wr.close()
    assert bio.getvalue().startswith(b"YUV4MPEG2 W%d H%d F25:1 Ip C%s\n" % (w, h, chroma.encode()))
    rd = y4m.Y4mReader(io.BytesIO(bio.getvalue()))
    with pytest.raises(ValueError):
        rd.read_into(bytearray(nbytes - 1))
    assert _read_all(rd) == [bytes(frames[0])]


def test_header_tokens_in_any_order_with_unknown_x_tokens():
    tokens = [b"W12", b"H8", b"F24000:1001", b"Ip", b"A1:1", b"C420mpeg2", b"XYSCSS=420MPEG2", b"XFOO=bar", b"XCOLORRANGE=LIMITED"]
    frames = _frames(2, 12 * 8 * 3 // 2)
    rng = random.Random(3)
    for _ in range(20):
        rng.shuffle(tokens)
        rd = y4m.Y4mReader(io.BytesIO(_stream(b"YUV4MPEG2 " + b" ".join(tokens) + b"\n", frames, b"FRAME Xparam=1\n")))
        assert (rd.width, rd.height, rd.fps, rd.aspect, rd.chroma, rd.colour_range) == (12, 8, (24000, 1001), (1, 1), "420mpeg2", "limited")
        assert _read_all(rd) == [bytes(f) for f in frames]


@pytest.mark.parametrize("tokens,chroma,rng", [
    (b"C420jpeg", "420jpeg", "full"), (b"Cmono", "mono", "full"), (b"C420mpeg2", "420mpeg2", "limited"), (b"C420paldv", "420paldv", "limited"),
    (b"C420", "420", "limited"), (b"", "420", "limited"), (b"I?", "420", "limited"),
    (b"C420jpeg XCOLORRANGE=LIMITED", "420jpeg", "limited"), (b"C420mpeg2 XCOLORRANGE=FULL", "420mpeg2", "full"), (b"Cmono XCOLORRANGE=LIMITED", "mono", "limited")])
def test_range_defaults_and_xcolorrange(tokens, chroma, rng):
    rd = y4m.Y4mReader(io.BytesIO(b"YUV4MPEG2 W4 H2 F25:1 " + tokens + b"\n"))
    assert (rd.chroma, rd.colour_range) == (chroma, rng)
    assert rd.range_given == (b"XCOLORRANGE" in tokens)


def test_reader_through_a_pipe_in_seven_byte_chunks():
    frames = _frames(3, 16 * 10 * 3 // 2, seed=9)
    data = _stream(b"YUV4MPEG2 W16 H10 F25:1 Ip C420mpeg2\n", frames)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb", buffering=0) as f:
            for i in range(0, len(data), 7):
                f.write(data[i:i + 7])

    t = threading.Thread(target=feed)
    t.start()
    try:
        with os.fdopen(r, "rb", buffering=0) as f:                     # unbuffered: every read returns what the pipe holds, a short read
            rd = y4m.Y4mReader(f)
            assert _read_all(rd) == [bytes(x) for x in frames]
    finally:
        t.join()


def test_clean_eof_and_truncation_name_the_frame():
    head = b"YUV4MPEG2 W4 H2 F25:1 C420jpeg\n"
    frames = _frames(3, 12)
    data = _stream(head, frames)
    buf = bytearray(12)
    rd = y4m.Y4mReader(io.BytesIO(data))
    assert [rd.read_into(buf) for _ in range(5)] == [True, True, True, False, False]
    assert len(_read_all(y4m.Y4mReader(io.BytesIO(head)))) == 0                    # a header alone: no frames, a clean end
    for cut, frame in ((5, 2), (1, 2), (12 + 6 + 3, 1)):                             # inside the last frame's bytes; inside frame 1's
        rd = y4m.Y4mReader(io.BytesIO(data[:-cut]))
        with pytest.raises(y4m.Y4mError, match="frame %d" % frame):
            _read_all(rd)
        assert rd.frames_read == frame
    rd = y4m.Y4mReader(io.BytesIO(data[:-12 - 3]))                                 # inside the last FRAME line
    with pytest.raises(y4m.Y4mError, match="frame 2"):
        _read_all(rd)
    for line in (b"FRAMES\n", b"frame\n", b"FRAMEX\n", b"\n"):
        rd = y4m.Y4mReader(io.BytesIO(_stream(head, frames[:1]) + line + bytes(12)))
        with pytest.raises(y4m.Y4mError, match="frame 1"):
            _read_all(rd)


@pytest.mark.parametrize("header,word", [
    (b"YUV4MPEG2 W4 H2 F25:1 C422\n", "C422"), (b"YUV4MPEG2 W4 H2 F25:1 C444\n", "C444"), (b"YUV4MPEG2 W4 H2 F25:1 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W4 H2 F25:1 C411\n", "C411"), (b"YUV4MPEG2 W4 H2 F25:1 C444alpha\n", "C444alpha"),
    (b"YUV4MPEG2 W4 H2 F25:1 It\n", "interlaced"), (b"YUV4MPEG2 W4 H2 F25:1 Ib\n", "interlaced"), (b"YUV4MPEG2 W4 H2 F25:1 Im\n", "interlaced"),
    (b"YUV4MPEG2 W5 H2 F25:1 C420jpeg\n", "even"), (b"YUV4MPEG2 W4 H3 F25:1\n", "even"),
    (b"YUV4MPEG2 W0 H2 F25:1\n", "outside"), (b"YUV4MPEG2 W4 H0 F25:1\n", "outside"), (b"YUV4MPEG2 W32768 H2 F25:1\n", "outside"),
    (b"YUV4MPEG2 W4 H32768 F25:1 Cmono\n", "outside"), (b"YUV4MPEG2 W-4 H2 F25:1\n", "outside"),
    (b"YUV4MPEG2 W4 H2 F0:1\n", "zero"), (b"YUV4MPEG2 W4 H2 F25:0\n", "zero"),
    (b"YUV4MPEG2 W4 H2 F25:1 " + b"X" * 240 + b"\n", "longer"), (b"YUV4MPEG2 W4 H2 F25:1 XCOLORRANGE=WIDE\n", "XCOLORRANGE"),
    (b"YUV4MPEG W4 H2 F25:1\n", "YUV4MPEG2"), (b"", "YUV4MPEG2"), (b"YUV4MPEG2 H2 F25:1\n", "W and H"), (b"YUV4MPEG2 W4 H2\n", "frame rate"),
    (b"YUV4MPEG2 Wx H2 F25:1\n", "malformed"), (b"YUV4MPEG2 W4 H2 F25\n", "malformed"), (b"YUV4MPEG2 W4 H2 F25:1", "ends inside")])
def test_every_refusal(header, word):
    with pytest.raises(y4m.Y4mError, match=word):
        y4m.Y4mReader(io.BytesIO(header + (b"FRAME\n" + bytes(12) if header.endswith(b"\n") else b"")))


def test_accepted_edges():
    assert y4m.Y4mReader(io.BytesIO(b"YUV4MPEG2 W5 H3 F25:1 Cmono\n")).frame_bytes == 15      # Cmono: any size
    line = b"YUV4MPEG2 W4 H2 F25:1 "
    line += b"X" * (255 - len(line))                                                           # 255 bytes and the newline: 256
    assert y4m.Y4mReader(io.BytesIO(line + b"\n")).width == 4
    with pytest.raises(y4m.Y4mError, match="longer"):
        y4m.Y4mReader(io.BytesIO(line + b"X\n"))
    for bad in (dict(chroma="422"), dict(width=5), dict(fps=(0, 1)), dict(width=40000), dict(colour_range="wide")):
        kw = dict(dict(width=4, height=2, fps=(25, 1), chroma="420jpeg"), **bad)
        with pytest.raises(y4m.Y4mError):
            y4m.Y4mWriter(io.BytesIO(), **kw)


def test_a_consumer_that_closes_the_pipe_ends_the_writing_quietly():
    r, w = os.pipe()
    os.close(r)
    f = os.fdopen(w, "wb", buffering=0)
    wr = y4m.Y4mWriter(f, 4, 2, (25, 1), "420jpeg")
    assert wr.broken and wr.write(bytes(12)) is False and wr.frames_written == 0
    wr.close()
    try:
        f.close()
    except BrokenPipeError:
        pass


def test_driver_flags():
    import deploy_bundle
    a = deploy_bundle.parse_args([])
    assert a.y4m_in is None and a.y4m_out is None and a.ingest == "host" and a.output_size == "network"
    a = deploy_bundle.parse_args(["--y4m-in", "-"])
    assert (a.y4m_in, a.y4m_out, a.ingest, a.output_size) == ("-", None, "device", "source")
    a = deploy_bundle.parse_args(["--y4m-in", "a.y4m", "--y4m-out", "-", "--fill", "0.8", "--height", "64", "--width", "96", "--refine", "2",
                                  "--operand-mode", "0", "--device", "cuda:0", "--model-dir", "m", "--model-name", "n"])
    assert (a.y4m_in, a.y4m_out, a.fill, a.height, a.width, a.refine, a.operand_mode) == ("a.y4m", "-", 0.8, 64, 96, 2, 0)
    for bad in (["--y4m-out", "b.y4m"], ["--y4m-in", "a", "--pipeline"], ["--y4m-in", "a", "--mjpg"], ["--y4m-in", "a", "--score"],
                ["--y4m-in", "a", "--decode", "device"], ["--y4m-in", "a", "--synthetic", "8"], ["--y4m-in", "a", "--fill", "auto"],
                ["--y4m-in", "a", "--fill", "adaptive"], ["--y4m-in", "a", "--fill", "history"], ["--y4m-in", "a", "--fill", "1.5"]):
        with pytest.raises(SystemExit):
            deploy_bundle.parse_args(bad)


def test_refusal_messages_are_one_sentence_each(capsys):
    import deploy_bundle
    for bad, word in ((["--y4m-out", "b"], "--y4m-out needs --y4m-in"), (["--y4m-in", "a", "--pipeline"], "--pipeline"),
                      (["--y4m-in", "a", "--mjpg"], "--mjpg"), (["--y4m-in", "a", "--score"], "--score"),
                      (["--y4m-in", "a", "--decode", "device"], "--decode device"), (["--y4m-in", "a", "--synthetic", "8"], "--synthetic"),
                      (["--y4m-in", "a", "--fill", "history"], "--fill history")):
        with pytest.raises(SystemExit):
            deploy_bundle.parse_args(bad)
        assert word in capsys.readouterr().err


def test_limited_range_table_and_the_default():
    from stabnet_amd import ingest
    lim = ingest.lut256_limited()
    assert lim.dtype == np.float32 and lim.shape == (256,)
    assert lim[16] == np.float32(-0.5) and lim[235] == np.float32(0.5)
    assert (np.diff(lim) >= 0).all() and (np.diff(lim[16:236]) > 0).all()
    assert (lim[:16] == np.float32(-0.5)).all() and (lim[235:] == np.float32(0.5)).all()
    u = np.arange(256, dtype=np.float64)
    assert np.array_equal(lim, (np.clip((u - 16) * 255 / 219, 0, 255) * (1. / 255) - 0.5).astype(np.float32))
    # the default is untouched: float32(float64(u) * (1./255) - 0.5)
    assert np.array_equal(ingest.lut256(), (u * (1. / 255) - 0.5).astype(np.float32))
    import inspect
    assert inspect.signature(ingest.FrameIngest.__init__).parameters["lut"].default is None
