"""CPU: the JPEG decoder's arithmetic and its host half.
  model     tests/jpeg_decode_model.py (libjpeg-turbo's JDCT_ISLOW + fancy upsampling + jdcolor in NumPy) equals the golden pixels of
            tests/golden/mjpeg_decode_streams.npz (decoded by Pillow on libjpeg-turbo when the fixture was made) and, where this
            Pillow is built on libjpeg-turbo, live Pillow: zero differing samples
  host      stabnet_mjpeg_parse: geometry, tables, interval offsets; "unsupported" for progressive and 4:2:2 files;
            stabnet_mjpeg_entropy_host: the model's coefficients
  corrupt   truncated streams, flipped bytes, an early EOI: an error status, never a crash -- through ctypes, and once through a
            stand-alone C++ program built with the address and undefined-behaviour sanitizers (tests/mjpeg_decode_fuzz_main.cpp)
Corrupt streams never go to the GPU: the device kernel runs the same bounded routine (csrc/jpeg_entropy.h)."""
import ctypes
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_model as D
import jpeg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = D.load_golden()
NAMES = list(GOLD)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_golden_pixels(name):
    jpeg, px = GOLD[name]
    got = D.decode(jpeg)
    assert got.shape == px.shape and got.dtype == np.uint8
    assert int((got != px).sum()) == 0
    if D.have_turbo():                                   # live Pillow only where it is built on libjpeg-turbo
        assert int((got != D.pillow_bgr(jpeg)).sum()) == 0


def test_fixture_covers_the_issue_streams():
    assert len(NAMES) == 10 and os.path.getsize(D.GOLDEN) < 100 << 10
    info = {n: D.coefficients(GOLD[n][0]) for n in NAMES}
    assert sorted((i["H"], i["W"]) for i in info.values()) == sorted(
        [(45, 77), (45, 77), (16, 16), (33, 50), (45, 77), (64, 96), (17, 31), (8, 8), (40, 56), (24, 40)])
    assert [info[n]["restart"] for n in NAMES] == [0, 3, 1, 2, 4, 0, 0, 0, 2, 2]
    assert b"\xff\xc4" not in GOLD["420_24x40_q75_nodht_r2"][0][:200]
    # custom tables: the optimised stream's DHT is not Annex K's
    assert D.annexk_dht()[4:33] not in GOLD["420_40x56_q85_optimize_r2"][0]


def _parse(jpeg, with_blob=True):
    from stabnet_amd import _lib
    L = _lib.lib()
    info = (ctypes.c_int * 16)()
    rc = L.stabnet_mjpeg_parse(jpeg, len(jpeg), info, None, 0)
    if rc != 0 or not with_blob:
        return rc, list(info), None
    blob = np.zeros(info[9], np.uint8)
    assert L.stabnet_mjpeg_parse(jpeg, len(jpeg), info, blob.ctypes.data, blob.size) == 0
    return 0, list(info), blob


def _entropy_host(jpeg, info, blob):
    from stabnet_amd import _lib
    coef = np.full(info[11] * 64, 0x5A5A, np.int16)
    rc = _lib.lib().stabnet_mjpeg_entropy_host(jpeg, len(jpeg), blob.ctypes.data, blob.size, coef.ctypes.data, coef.size)
    return rc, coef


@pytest.mark.parametrize("name", NAMES)
def test_parser_geometry_tables_offsets(name):
    jpeg, px = GOLD[name]
    ref = D.coefficients(jpeg)
    rc, info, blob = _parse(jpeg)
    assert rc == 0
    H, W, C = ref["H"], ref["W"], ref["C"]
    sub = 0 if C == 1 else (420 if ref["sampling"][0] == (2, 2) else 444)
    ms = 16 if sub == 420 else 8
    nmcu = -(-H // ms) * -(-W // ms)
    R = ref["restart"] or nmcu
    nint = -(-nmcu // min(R, nmcu))
    assert info[:7] == [H, W, C, sub, ref["restart"], nint, nmcu]
    assert info[7] == M.decode(D.with_dht(jpeg))["header_bytes"] - (len(D.with_dht(jpeg)) - len(jpeg)) and info[8] == len(jpeg) - 2
    assert info[10] == int(b"\xff\xc4" in jpeg[:info[7]]) and info[11] == nmcu * {0: 1, 444: 3, 420: 6}[sub]
    head = blob[:96].view(np.int32)
    assert head[0] == 0x4A504744 and list(head[1:4]) == [H, W, {0: 0, 444: 1, 420: 2}[sub]]
    assert list(head[4:8]) == [min(R, nmcu), nint, nmcu, len(jpeg)]
    # quantiser tables in natural order, by table id
    q = blob[96:96 + 512].view(np.uint16).reshape(4, 64)
    for t, tab in ref["qtables"].items():
        assert np.array_equal(q[t], tab)
    assert list(head[14:17]) == ref["tq"] + [0] * (3 - C)
    # interval offsets: every interval starts behind a restart marker and ends in front of the next one (or EOI)
    starts = blob[96 + 512 + 4 * 1416:].view(np.int32)[:nint + 1]
    assert starts[0] == info[7] and starts[nint] == len(jpeg)
    for i in range(1, nint):
        assert jpeg[starts[i] - 2] == 0xFF and jpeg[starts[i] - 1] == 0xD0 + ((i - 1) & 7)
    # Huffman tables: every code of the stream's (or Annex K's) DHT decodes to its symbol through look / maxcode / valoff / huffval
    segs = D.with_dht(jpeg)
    tables, p = {}, 2
    for mk, off, ln in D.segments(segs):
        if mk == 0xC4:
            s = off + 4
            while s < off + ln:
                bits = list(segs[s + 1:s + 17])
                tables[segs[s]] = (bits, list(segs[s + 17:s + 17 + sum(bits)]))
                s += 17 + sum(bits)
    for tc_th, (bits, vals) in tables.items():
        h = blob[96 + 512 + ((tc_th >> 4) * 2 + (tc_th & 15)) * 1416:][:1416]
        look, maxcode = h[:1024].view(np.uint16), h[1024:1092].view(np.int32)
        valoff, huffval = h[1092:1160].view(np.int32), h[1160:]
        for sym, (code, ln) in M.huff_codes(bits, vals).items():
            if ln <= 9:
                assert all(look[(code << (9 - ln)) + f] == (ln << 8 | sym) for f in range(1 << (9 - ln)))
            else:
                assert look[code >> (ln - 9)] == 0 and code <= maxcode[ln] and huffval[valoff[ln] + code] == sym
                assert all(code >> (ln - l) > maxcode[l] for l in range(10, ln))


@pytest.mark.parametrize("name", NAMES)
def test_entropy_host_equals_model_coefficients(name):
    jpeg, _ = GOLD[name]
    rc, info, blob = _parse(jpeg)
    assert rc == 0
    rc, coef = _entropy_host(jpeg, info, blob)
    assert rc == 0
    assert np.array_equal(coef.astype(np.int32), D.coefficients(jpeg)["coef"].reshape(-1))


def _pillow_jpeg(**opts):
    from PIL import Image
    img = np.clip(np.add.outer(np.arange(40) * 3, np.arange(48) * 2)[..., None] + np.array([0, 40, 90]), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=80, **opts)
    return buf.getvalue()


def test_parser_says_unsupported():
    from stabnet_amd import _lib, mjpeg
    for jpeg, word in ((_pillow_jpeg(progressive=True), b"SOF2"), (_pillow_jpeg(subsampling="4:2:2"), b"sampling")):
        rc, _, _ = _parse(jpeg, with_blob=False)
        assert rc == 1 and b"unsupported" in _lib.lib().stabnet_last_error() and word in _lib.lib().stabnet_last_error()
        with pytest.raises(mjpeg.Unsupported):
            mjpeg.parse(jpeg)
    # a 16-bit quantiser table, 12-bit samples, a restart-marker count that disagrees with DRI
    base = GOLD["420_45x77_q75_r3"][0]
    dqt = base.index(b"\xff\xdb")
    assert _parse(base[:dqt + 4] + bytes([base[dqt + 4] | 0x10]) + base[dqt + 5:], False)[0] == 1
    sof = base.index(b"\xff\xc0")
    assert _parse(base[:sof + 4] + b"\x0c" + base[sof + 5:], False)[0] == 1
    dri = base.index(b"\xff\xdd")
    assert _parse(base[:dri + 4] + b"\x00\x02" + base[dri + 6:], False)[0] == 1
    with pytest.raises(_lib.StabnetError):
        mjpeg.parse(base[:-2])


def corrupt_streams():
    """[(kind, bytes)]: seeded, the same on every run.  kind: 'truncated' and 'early_eoi' must give an error; a 'flipped' byte may leave
    a stream that still decodes."""
    rng = np.random.default_rng(20240607)
    out = []
    for name in NAMES:
        jpeg, _ = GOLD[name]
        scan = D.segments(jpeg)[-1]
        scan = scan[1] + scan[2]
        cuts = sorted(set(list(range(0, len(jpeg), 53)) + [1, 2, 3, scan - 1, scan, scan + 1, len(jpeg) - 3, len(jpeg) - 2, len(jpeg) - 1]))
        out += [("truncated", jpeg[:c]) for c in cuts if 0 <= c < len(jpeg)]
        for _ in range(40):
            b = bytearray(jpeg)
            for pos in rng.integers(2, len(jpeg) - 2, size=int(rng.integers(1, 4))):
                b[pos] ^= int(rng.integers(1, 256))
            out.append(("flipped", bytes(b)))
        for frac in (0.1, 0.5, 0.9):
            at = scan + int((len(jpeg) - 2 - scan) * frac)
            while jpeg[at - 1] == 0xFF:                    # not between FF and its stuffed 00
                at += 1
            out.append(("early_eoi", jpeg[:at] + b"\xff\xd9" + jpeg[at:]))
    return out


def test_corrupt_streams_give_a_status():
    n_err = 0
    for kind, jpeg in corrupt_streams():
        rc, info, blob = _parse(jpeg) if len(jpeg) else (-1, None, None)
        assert rc in (0, 1, -1)
        if rc == 0:
            rc, coef = _entropy_host(jpeg, info, blob)
            assert rc in (0, -1)
        if kind != "flipped":
            assert rc != 0, kind
        n_err += rc != 0
    assert n_err > 100


def test_corrupt_streams_under_the_sanitizers(tmp_path):
    """The same inputs through the host decoder built with -fsanitize=address,undefined, as a program of its own."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    streams = [j for _, j in corrupt_streams()] + [GOLD[n][0] for n in NAMES]
    data = tmp_path / "streams.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for j in streams:
            f.write(struct.pack("<I", len(j)) + j)
    exe = str(tmp_path / "mjpeg_decode_fuzz")
    csrc = os.path.join(ROOT, "deep-online-video-stabilization_amd", "csrc")
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []          # no dependence on the library load order
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-I", csrc, "-o", exe,
           "-x", "c++", os.path.join(csrc, "mjpeg_parse.hip"), os.path.join(ROOT, "tests", "mjpeg_decode_fuzz_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    ok, unsupported, corrupt, undecodable = (int(v) for v in r.stdout.split())
    assert ok + unsupported + corrupt + undecodable == len(streams) and ok >= len(NAMES) and corrupt + undecodable > 100
