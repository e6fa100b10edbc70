"""CPU: self-synchronising parallel Huffman decoding (csrc/jpeg_sync.h) through its host twin, stabnet_mjpeg_entropy_sync_host -- the
phases of csrc/mjpeg_decode_sync.hip with the lanes in a loop.  The reference is the sequential routine, stabnet_mjpeg_entropy_host
(which tests/test_mjpeg_decode_cpu.py ties to the NumPy model), never the new code.
  twin      coefficients and result equal the host routine's for the fixture's streams without restart markers and Pillow streams
            (grey, 4:4:4, 4:2:0; 33x50, 40x56; optimised tables; q100 noise: full blocks without EOB, ZRL, long codes), chunk_bytes in
            {1, 2, 4, 16, 64, 4096} (at 1, 2, 4 a symbol spans several chunks) and rounds in {0, 1, 8}
  first     an FF at a chunk's last byte is among the cases; trailing 1-padding gives status 0; with rounds = 0 nothing behind chunk 0
            is accepted before the repair
  corrupt   truncations, flipped bytes, early EOIs: an error, or the host routine's coefficients -- through ctypes, and once through
            tests/mjpeg_sync_fuzz_main.cpp built with the address and undefined-behaviour sanitizers.  None goes to the GPU.
  refusals  of the new entries
  stats     shares of chunks accepted after 1, 2, 4, 8 rounds, printed for DESIGN (not asserted)"""
import ctypes
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_model as D
from test_mjpeg_decode_cpu import corrupt_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = D.load_golden()
CHUNKS = [1, 2, 4, 16, 64, 4096]
ROUNDS = [0, 1, 8]


def _picture(H, W, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 6.0 + y / 9.0), 128 + 90 * np.cos(x / 4.0 - y / 7.0), 30 + 3.0 * x + 2.0 * y], -1)
    return np.clip(np.rint(base + rng.normal(0.0, noise, base.shape)), 0, 255).astype(np.uint8)


def _pillow(img, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **opts)
    return buf.getvalue()


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _parse(jpeg):
    from stabnet_amd import _lib
    L = _lib.lib()
    info = (ctypes.c_int * 16)()
    rc = L.stabnet_mjpeg_parse(jpeg, len(jpeg), info, None, 0)
    if rc != 0:
        return rc, list(info), None
    blob = np.zeros(info[9], np.uint8)
    assert L.stabnet_mjpeg_parse(jpeg, len(jpeg), info, blob.ctypes.data, blob.size) == 0
    return 0, list(info), blob


def _host(jpeg, info, blob):
    from stabnet_amd import _lib
    coef = np.full(info[11] * 64, 0x5A5A, np.int16)
    rc = _lib.lib().stabnet_mjpeg_entropy_host(jpeg, len(jpeg), blob.ctypes.data, blob.size, coef.ctypes.data, coef.size)
    return rc, coef


def _twin(jpeg, info, blob, chunk, rounds):
    from stabnet_amd import _lib
    coef = np.full(info[11] * 64, 0x5A5A, np.int16)
    stats = (ctypes.c_int * 2)(-1, -1)
    rc = _lib.lib().stabnet_mjpeg_entropy_sync_host(jpeg, len(jpeg), blob.ctypes.data, blob.size, coef.ctypes.data, coef.size, chunk, rounds,
                                                    stats)
    return rc, coef, list(stats)


def _streams():
    s = {n: GOLD[n][0] for n in GOLD if _parse(GOLD[n][0])[1][5] == 1}
    for H, W in ((33, 50), (40, 56)):
        img = _picture(H, W, H)
        s["grey_%dx%d" % (H, W)] = _pillow(np.ascontiguousarray(img[..., 0]), quality=80)
        s["444_%dx%d" % (H, W)] = _pillow(img, quality=80, subsampling="4:4:4")
        s["420_%dx%d" % (H, W)] = _pillow(img, quality=80, subsampling="4:2:0")
    s["420_40x56_optimize"] = _pillow(_picture(40, 56, 6, noise=30.0), quality=92, subsampling="4:2:0", optimize=True)
    s["444_33x50_optimize"] = _pillow(_picture(33, 50, 7, noise=30.0), quality=92, subsampling="4:4:4", optimize=True)
    s["420_40x56_q100_noise"] = _pillow(_noise(40, 56, 8), quality=100, subsampling="4:2:0")
    s["444_33x50_q100_noise"] = _pillow(_noise(33, 50, 9), quality=100, subsampling="4:4:4")
    s["grey_40x56_q100_noise"] = _pillow(np.ascontiguousarray(_noise(40, 56, 10)[..., 0]), quality=100)
    return s


STREAMS = _streams()


def test_the_streams_are_what_the_cases_need():
    assert sum(n in GOLD for n in STREAMS) == 5                    # the fixture's streams without restart markers
    for n, j in STREAMS.items():
        assert _parse(j)[1][4:6] == [0, 1] or n in GOLD, n          # no DRI, one interval
    # q100 noise: blocks that are full (no EOB: 63 AC coefficients) and ZRL-free long codes; a ZRL somewhere among the cases
    c = D.coefficients(STREAMS["420_40x56_q100_noise"])["coef"].reshape(-1, 64)
    assert (np.count_nonzero(c, axis=1) == 64).any()
    # an FF at a chunk's last byte (its stuffed 00 opens the next chunk), for a tested stream and chunk size
    hit = []
    for n, j in STREAMS.items():
        _, info, _ = _parse(j)
        a = info[7]
        for chunk in CHUNKS[1:5]:
            hit += [(n, chunk) for p in range(a + chunk - 1, info[8] - 1, chunk) if j[p] == 0xFF and j[p + 1] == 0]
    assert hit
    print("FF at a chunk's last byte:", hit[:4], "...", len(hit))


@pytest.mark.parametrize("name", list(STREAMS))
def test_twin_equals_host_routine(name):
    jpeg = STREAMS[name]
    rc, info, blob = _parse(jpeg)
    assert rc == 0
    rc, ref = _host(jpeg, info, blob)
    assert rc == 0
    for chunk in CHUNKS:
        for rounds in ROUNDS:
            rc, got, stats = _twin(jpeg, info, blob, chunk, rounds)
            assert rc == 0, (chunk, rounds)
            assert np.array_equal(got, ref), (chunk, rounds)
            nc = max(1, -(-(info[8] - info[7]) // chunk))
            assert stats[0] == nc and 1 <= stats[1] <= nc
            if rounds == 0:
                assert stats[1] == 1, (chunk, stats)                # nothing behind chunk 0 is accepted before the repair


def test_trailing_one_padding_gives_status_0():
    """The bits behind the last block are 1s up to the byte boundary; some stream of the set has seven of them, and a decoder that
    took them for a symbol would report a code error."""
    pads = []
    for n, jpeg in STREAMS.items():
        rc, info, blob = _parse(jpeg)
        last = jpeg[info[8] - 1] if jpeg[info[8] - 1] != 0 or jpeg[info[8] - 2] != 0xFF else 0xFF
        pad = 0
        while pad < 8 and (last >> pad) & 1:
            pad += 1
        pads.append(pad)
        for chunk in (4, 16):
            assert _twin(jpeg, info, blob, chunk, 8)[0] == 0
    assert max(pads) >= 3
    # a whole byte of padding appended in front of EOI: still status 0, the same coefficients
    jpeg = STREAMS["420_40x56"]
    rc, info, blob = _parse(jpeg)
    ref = _host(jpeg, info, blob)[1]
    padded = jpeg[:-2] + b"\xff\x00" + jpeg[-2:]
    rc, info, blob = _parse(padded)
    assert rc == 0 and _host(padded, info, blob)[0] == 0
    for chunk in (1, 4, 16, 64):
        rc, got, _ = _twin(padded, info, blob, chunk, 8)
        assert rc == 0 and np.array_equal(got, ref)


def test_corrupt_streams_status_or_host_coefficients():
    n_err = n_same = 0
    for kind, jpeg in corrupt_streams():
        rc, info, blob = _parse(jpeg) if len(jpeg) else (-1, None, None)
        if rc != 0 or info[5] != 1:
            continue
        hrc, ref = _host(jpeg, info, blob)
        for chunk, rounds in ((1, 1), (4, 0), (16, 8), (64, 1)):
            rc, got, _ = _twin(jpeg, info, blob, chunk, rounds)
            assert rc in (0, -1)
            assert rc != 0 or (hrc == 0 and np.array_equal(got, ref)), (kind, chunk, rounds)
            if hrc != 0:
                assert rc != 0, (kind, chunk, rounds)             # what the sequential decode refuses, the parallel one refuses
            n_err += rc != 0
            n_same += rc == 0
    print("corrupt streams: %d runs refused, %d with the host routine's coefficients" % (n_err, n_same))
    assert n_err > 100 and n_same > 0


def test_corrupt_streams_under_the_sanitizers(tmp_path):
    """The same inputs through the twin built with -fsanitize=address,undefined, as a program of its own (nothing preloaded)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    streams = [j for _, j in corrupt_streams()] + list(STREAMS.values())
    data = tmp_path / "streams.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for j in streams:
            f.write(struct.pack("<I", len(j)) + j)
    exe = str(tmp_path / "mjpeg_sync_fuzz")
    csrc = os.path.join(ROOT, "deep-online-video-stabilization_amd", "csrc")
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-I", csrc, "-o", exe,
           "-x", "c++", os.path.join(csrc, "mjpeg_parse.hip"), os.path.join(ROOT, "tests", "mjpeg_sync_fuzz_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    runs, same, refused, skipped = (int(v) for v in r.stdout.split())
    assert runs == same + refused and same >= len(STREAMS) and refused > 100 and skipped > 100


def test_refusals():
    from stabnet_amd import _lib
    L = _lib.lib()
    jpeg = STREAMS["420_40x56"]
    rc, info, blob = _parse(jpeg)
    coef = np.zeros(info[11] * 64, np.int16)
    args = lambda **k: [k.get("jpeg", jpeg), len(jpeg), k.get("blob", blob.ctypes.data), k.get("blob_bytes", blob.size),
                        k.get("coef", coef.ctypes.data), k.get("count", coef.size), k.get("chunk", 16), k.get("rounds", 1), None]
    assert L.stabnet_mjpeg_entropy_sync_host(*args()) == 0
    for bad in (dict(chunk=0), dict(chunk=-4), dict(count=coef.size - 1), dict(blob=None), dict(coef=None), dict(blob_bytes=64)):
        assert L.stabnet_mjpeg_entropy_sync_host(*args(**bad)) == -1, bad
    assert L.stabnet_mjpeg_entropy_sync_host(*args(chunk=0)) == -1 and b"chunk_bytes" in L.stabnet_last_error()
    # a blob of several intervals is not this back end's
    dri, _ = GOLD["420_45x77_q75_r3"]
    rc, dinfo, dblob = _parse(dri)
    assert dinfo[5] > 1
    dcoef = np.zeros(dinfo[11] * 64, np.int16)
    assert L.stabnet_mjpeg_entropy_sync_host(dri, len(dri), dblob.ctypes.data, dblob.size, dcoef.ctypes.data, dcoef.size, 16, 1, None) == -1
    assert b"interval" in L.stabnet_last_error()
    # the device entry's workspace size: 0 for arguments it refuses, the decoder's own workspace plus the chunk states otherwise
    base = L.stabnet_mjpeg_decode_workspace_bytes(2, 40, 56, 3, 420)
    bm = L.stabnet_mjpeg_decode_blob_bytes(40, 56, 3, 420)
    stride = (bm + 8192 + 15) & ~15
    for chunk in (0, 8, 16, 128, 4096):
        assert L.stabnet_mjpeg_decode_sync_workspace_bytes(2, 40, 56, 3, 420, stride, chunk) > base
    for chunk in (-1, 4, 6, 18, 4100):
        assert L.stabnet_mjpeg_decode_sync_workspace_bytes(2, 40, 56, 3, 420, stride, chunk) == 0
        assert b"chunk_bytes" in L.stabnet_last_error()
    assert L.stabnet_mjpeg_decode_sync_workspace_bytes(0, 40, 56, 3, 420, stride, 16) == 0
    assert L.stabnet_mjpeg_decode_sync_workspace_bytes(1, 40, 56, 3, 422, stride, 16) == 0
    assert L.stabnet_mjpeg_decode_sync_workspace_bytes(1, 40, 56, 3, 420, bm - 16, 16) == 0
    # every refusal of the device entry comes before any launch: bad arguments never reach the GPU (there is none here)
    def dec(**k):
        return L.stabnet_mjpeg_decode_sync(k.get("inp", 4096), k.get("stride", stride), k.get("N", 1), 40, 56, 3, k.get("sub", 420), 4096, 56 * 3,
                                           40 * 56 * 3, k.get("status", 4096), k.get("ws", 4096), k.get("ws_bytes", 1 << 30), k.get("stages", 3),
                                           k.get("chunk", 0), k.get("rounds", -1), None, None)
    for bad, word in ((dict(inp=None), b"null"), (dict(status=None), b"null"), (dict(ws=None), b"null"), (dict(N=0), b"batch"),
                      (dict(sub=422), b"subsampling"), (dict(stages=4), b"stages"), (dict(chunk=12345), b"chunk_bytes"), (dict(chunk=6), b"chunk_bytes"),
                      (dict(rounds=-2), b"rounds"), (dict(stride=stride + 8), b"aligned"), (dict(inp=4100), b"aligned"),
                      (dict(stride=bm - 16), b"in_stride"), (dict(ws=4104), b"aligned")):
        assert dec(**bad) == -1 and word in L.stabnet_last_error(), (bad, L.stabnet_last_error())
    assert dec(ws_bytes=base // 2) == -3 and b"workspace" in L.stabnet_last_error()


def _synthetic_720p():
    from stabnet_amd import synthetic
    g8 = ((synthetic.make_clip(720, 1280, 1, seed=3)[0] + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def test_print_sync_statistics():
    """Recorded in DESIGN, not asserted: the share of chunks accepted before the repair after 1, 2, 4, 8 rounds."""
    frame = _synthetic_720p()
    streams = {n: STREAMS[n] for n in STREAMS if n in GOLD}
    streams["720p_q75"] = _pillow(frame, quality=75, subsampling="4:2:0")
    streams["720p_q95"] = _pillow(frame, quality=95, subsampling="4:2:0")
    print()
    for n, jpeg in streams.items():
        rc, info, blob = _parse(jpeg)
        assert rc == 0
        ref = _host(jpeg, info, blob)[1]
        for chunk in (16, 32, 64, 128):
            shares = []
            for rounds in (1, 2, 4, 8):
                rc, got, stats = _twin(jpeg, info, blob, chunk, rounds)
                assert rc == 0 and np.array_equal(got, ref)
                shares.append(100.0 * stats[1] / stats[0])
            print("sync %-28s %7d bytes chunk %3d: %5d chunks, accepted after 1/2/4/8 rounds %5.1f %5.1f %5.1f %5.1f %%"
                  % (n, len(jpeg), chunk, stats[0], *shares))
