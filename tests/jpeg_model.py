"""Helper of the MJPEG tests (not a test): baseline JPEG written down from ITU-T T.81 and the JFIF note, independent of the HIP code.

  transform()      float64 NumPy statement of the encoder's arithmetic: JFIF full-range BT.601 without rounding to 8 bits, 2x2 chroma
                   mean (4:2:0), level shift, orthonormal 8x8 DCT-II, rint(coef / Q), AC clamped to +-1023 and DC to +-1024;
                   returns the quantised coefficients in scan order [mcu][block][64 zig-zag] AND the unrounded coef / Q
  entropy_encode() plain-Python Huffman coder with the Annex K tables: restart intervals (byte-aligned, DC predictors 0, padded with
                   1-bits, RSTm mod 8 between them), 0xFF stuffing; returns the scan bytes WITHOUT the final EOI
  header()         SOI .. SOS as this project lays it out (JFIF APP0, one DQT, SOF0, one DHT, DRI, SOS)
  decode()         plain-Python baseline decoder: parses the markers of a stream, builds the Huffman decoders from ITS DHT segments,
                   returns the quantised coefficients in scan order plus what the header said
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

# Table K.1 / K.2
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)

# Tables K.3 - K.6: (number of codes of each length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def quant_tables(quality):
    """IJG scaling of the Annex K tables, natural order (jcparam.c: jpeg_quality_scaling / jpeg_add_quant_table, force_baseline)."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    f = lambda t: np.clip((t * s + 50) // 100, 1, 255).astype(np.int64)
    return f(Q_LUMA), f(Q_CHROMA)


def geometry(H, W, C, subsampling):
    """(MCU size, blocks per MCU, MCUs per row, MCU rows, component of each block of an MCU)"""
    if C == 1:
        ms, comps = 8, [0]
    elif str(subsampling) == "420":
        ms, comps = 16, [0, 0, 0, 0, 1, 2]
    else:
        assert str(subsampling) == "444"
        ms, comps = 8, [0, 1, 2]
    return ms, len(comps), -(-W // ms), -(-H // ms), comps


def dct_matrix():
    u = np.arange(8)[:, None]
    x = np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] *= 1 / np.sqrt(2)
    return d


def _blocks(plane):
    """[h, w] (multiples of 8) -> [h/8, w/8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def transform(img, subsampling="420", q_luma=None, q_chroma=None, dtype=np.float64):
    """img uint8 [H,W] / [H,W,1] (grey) or [H,W,3] (BGR).  Returns (coef int [nmcu, bpm, 64] zig-zag, ratio float [nmcu, bpm, 64]:
    the unrounded coef / Q of the same positions)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    ms, bpm, mcux, mcuy, comps = geometry(H, W, C, subsampling)
    pad = np.pad(img, ((0, mcuy * ms - H), (0, mcux * ms - W), (0, 0)), mode="edge").astype(dtype)
    if C == 1:
        planes = [pad[..., 0] - 128.0]
    else:
        B, G, R = pad[..., 0], pad[..., 1], pad[..., 2]
        Y = 0.299 * R + 0.587 * G + 0.114 * B - 128.0
        Cb = -0.168735892 * R - 0.331264108 * G + 0.5 * B
        Cr = 0.5 * R - 0.418687589 * G - 0.081312411 * B
        if ms == 16:
            mean = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) * 0.25
            Cb, Cr = mean(Cb), mean(Cr)
        planes = [Y, Cb, Cr]
    D = dct_matrix().astype(dtype)
    ratio = np.zeros((mcuy, mcux, bpm, 64), dtype)
    qn = [np.asarray(q_luma, dtype).reshape(8, 8)] + [np.asarray(q_chroma if q_chroma is not None else q_luma, dtype).reshape(8, 8)] * 2
    for c, plane in enumerate(planes):
        blk = _blocks(plane)
        co = (D @ blk @ D.T) / qn[c]                     # [by, bx, 8(v), 8(u)]
        co = co.reshape(co.shape[0], co.shape[1], 64)[..., ZIGZAG]
        if ms == 16 and c == 0:
            for j in range(4):
                ratio[:, :, j] = co[(j >> 1)::2, (j & 1)::2]
        else:
            ratio[:, :, comps.index(c)] = co
    ratio = ratio.reshape(mcuy * mcux, bpm, 64)
    coef = np.rint(ratio).astype(np.int64)
    coef[..., 1:] = np.clip(coef[..., 1:], -1023, 1023)
    coef[..., 0] = np.clip(coef[..., 0], -1024, 1024)
    return coef, ratio


def huff_codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _stuff(acc, nbits):
    """nbits (multiple of 8) of the integer acc as bytes, 0xFF followed by 0x00"""
    raw = acc.to_bytes(nbits // 8, "big") if nbits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def entropy_encode(coef, C, subsampling, restart_mcus, tables=None):
    """coef int [nmcu, bpm, 64] -> scan bytes: intervals with RSTm between them, no EOI."""
    comps = geometry(8, 8, C, subsampling)[4]
    dc_t = [huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA)] if tables is None else tables[0]
    ac_t = [huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA)] if tables is None else tables[1]
    coef = np.asarray(coef)
    nmcu = coef.shape[0]
    rows = coef.tolist()
    out = bytearray()
    nint = -(-nmcu // restart_mcus)
    for it in range(nint):
        acc, nb = 0, 0
        pred = [0, 0, 0]
        for m in range(it * restart_mcus, min(nmcu, (it + 1) * restart_mcus)):
            for j, comp in enumerate(comps):
                blk = rows[m][j]
                t = 1 if comp else 0
                diff = blk[0] - pred[comp]
                pred[comp] = blk[0]
                size = abs(diff).bit_length()
                code, ln = dc_t[t][size]
                acc = (acc << ln) | code
                nb += ln
                if size:
                    acc = (acc << size) | ((diff if diff >= 0 else diff - 1) & ((1 << size) - 1))
                    nb += size
                run = 0
                last = 63
                while last > 0 and blk[last] == 0:
                    last -= 1
                for k in range(1, last + 1):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        code, ln = ac_t[t][0xF0]
                        acc = (acc << ln) | code
                        nb += ln
                        run -= 16
                    size = abs(v).bit_length()
                    code, ln = ac_t[t][(run << 4) | size]
                    acc = (acc << (ln + size)) | (code << size) | ((v if v >= 0 else v - 1) & ((1 << size) - 1))
                    nb += ln + size
                    run = 0
                if last < 63:
                    code, ln = ac_t[t][0]
                    acc = (acc << ln) | code
                    nb += ln
        padn = (-nb) % 8
        acc = (acc << padn) | ((1 << padn) - 1)
        nb += padn
        out += _stuff(acc, nb)
        if it != nint - 1:
            out += bytes([0xFF, 0xD0 + (it & 7)])
    return bytes(out)


def header(H, W, C, subsampling, restart_mcus, q_luma, q_chroma=None):
    be = lambda v: bytes([v >> 8, v & 255])
    ntab = 1 if C == 1 else 2
    o = b"\xff\xd8" + b"\xff\xe0" + be(16) + b"JFIF\0" + b"\x01\x01" + b"\x00" + be(1) + be(1) + b"\x00\x00"
    o += b"\xff\xdb" + be(2 + 65 * ntab)
    for t in range(ntab):
        o += bytes([t]) + bytes(int(v) for v in np.asarray(q_chroma if t else q_luma)[ZIGZAG])
    o += b"\xff\xc0" + be(8 + 3 * C) + b"\x08" + be(H) + be(W) + bytes([C])
    for c in range(C):
        o += bytes([c + 1, 0x22 if (c == 0 and C == 3 and str(subsampling) == "420") else 0x11, 1 if c else 0])
    o += b"\xff\xc4" + be(2 + ntab * 208)
    for t in range(ntab):
        dc, ac = (DC_CHROMA, AC_CHROMA) if t else (DC_LUMA, AC_LUMA)
        o += bytes([t]) + bytes(dc[0]) + bytes(dc[1]) + bytes([0x10 | t]) + bytes(ac[0]) + bytes(ac[1])
    o += b"\xff\xdd" + be(4) + be(restart_mcus)
    o += b"\xff\xda" + be(6 + 2 * C) + bytes([C])
    for c in range(C):
        o += bytes([c + 1, 0x11 if c else 0x00])
    return o + b"\x00\x3f\x00"


def encode(img, quality=75, subsampling="420", restart_mcus=1, q_luma=None, q_chroma=None):
    """The whole model: a complete JFIF stream."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    if q_luma is None:
        q_luma, q_chroma = quant_tables(quality)
    coef, _ = transform(img, subsampling, q_luma, q_chroma)
    return header(H, W, C, subsampling, restart_mcus, q_luma, q_chroma) + entropy_encode(coef, C, subsampling, restart_mcus) + b"\xff\xd9"


def _decoder_lut(bits, vals):
    """16-bit prefix -> (symbol, code length)"""
    lut = [None] * 65536
    for sym, (code, ln) in huff_codes(bits, vals).items():
        base = code << (16 - ln)
        for i in range(base, base + (1 << (16 - ln))):
            lut[i] = (sym, ln)
    return lut


def decode(data):
    """Baseline decoder down to the quantised coefficients.  Returns dict: H, W, C, sampling [(h, v)], qtables {id: natural-order
    array}, restart (0 = none), coef int64 [nmcu, bpm, 64] (zig-zag), header_bytes (offset of the entropy-coded data), n_rst."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    p = 2
    qt, dc_l, ac_l, info = {}, {}, {}, {"restart": 0}
    while True:
        assert data[p] == 0xFF, "marker expected at %d" % p
        mk = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + ln]
        p += 2 + ln
        if mk == 0xDB:
            s = 0
            while s < len(seg):
                assert seg[s] >> 4 == 0, "8-bit tables only"
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(seg[s + 1:s + 65])
                qt[seg[s] & 15] = t
                s += 65
        elif mk == 0xC0:
            assert seg[0] == 8
            info["H"], info["W"], info["C"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            info["sampling"] = [(seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(seg[5])]
            info["tq"] = [seg[8 + 3 * c] for c in range(seg[5])]
        elif mk == 0xC4:
            s = 0
            while s < len(seg):
                bits = list(seg[s + 1:s + 17])
                n = sum(bits)
                vals = list(seg[s + 17:s + 17 + n])
                (ac_l if seg[s] >> 4 else dc_l)[seg[s] & 15] = _decoder_lut(bits, vals)
                s += 17 + n
        elif mk == 0xDD:
            info["restart"] = (seg[0] << 8) | seg[1]
        elif mk == 0xDA:
            ns = seg[0]
            sel = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            assert list(seg[1 + 2 * ns:4 + 2 * ns]) == [0, 63, 0]
            break
        else:
            assert mk in (0xE0, 0xFE) or 0xE0 <= mk <= 0xEF, "unexpected marker %02x" % mk
    info["header_bytes"] = p
    info["qtables"] = qt
    C = info["C"]
    hmax = max(h for h, _ in info["sampling"])
    comps = []
    for c, (h, v) in enumerate(info["sampling"]):
        comps += [c] * (h * v)
    ms = 8 * hmax
    mcux, mcuy = -(-info["W"] // ms), -(-info["H"] // ms)
    nmcu = mcux * mcuy
    assert data[-2:] == b"\xff\xd9", "no EOI at the end"
    body = data[p:-2]
    # split at RSTm: after un-stuffing, an 0xFF followed by 0xD0..0xD7 can only be a marker
    intervals, start, i, n_rst = [], 0, 0, 0
    while True:
        j = body.find(b"\xff", i)
        if j < 0 or j + 1 >= len(body):
            assert j < 0, "dangling 0xFF"
            break
        nxt = body[j + 1]
        if nxt == 0:
            i = j + 2
        else:
            assert 0xD0 <= nxt <= 0xD7 and nxt == 0xD0 + (n_rst & 7), "unexpected marker %02x in the scan" % nxt
            intervals.append(body[start:j])
            n_rst += 1
            start = i = j + 2
    intervals.append(body[start:])
    R = info["restart"] or nmcu
    assert len(intervals) == -(-nmcu // R), "%d intervals for %d MCUs at DRI %d" % (len(intervals), nmcu, R)
    info["n_rst"] = n_rst
    coef = np.zeros((nmcu, len(comps), 64), np.int64)
    for it, raw in enumerate(intervals):
        buf = raw.replace(b"\xff\x00", b"\xff")
        nbits = len(buf) * 8
        acc = int.from_bytes(buf, "big") << 32           # room to peek 16 bits past the end
        total = nbits + 32
        pos = 0
        pred = [0, 0, 0]
        for m in range(it * R, min(nmcu, (it + 1) * R)):
            for j, c in enumerate(comps):
                blk = [0] * 64
                td, ta = sel[c]
                sym, ln = dc_l[td][(acc >> (total - pos - 16)) & 0xFFFF]
                pos += ln
                if sym:
                    v = (acc >> (total - pos - sym)) & ((1 << sym) - 1)
                    pos += sym
                    if v < (1 << (sym - 1)):
                        v -= (1 << sym) - 1
                    pred[c] += v
                blk[0] = pred[c]
                k = 1
                lut = ac_l[ta]
                while k < 64:
                    sym, ln = lut[(acc >> (total - pos - 16)) & 0xFFFF]
                    pos += ln
                    r, s = sym >> 4, sym & 15
                    if s == 0:
                        if r == 15:
                            k += 16
                            continue
                        assert r == 0
                        break
                    k += r
                    v = (acc >> (total - pos - s)) & ((1 << s) - 1)
                    pos += s
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                    assert k < 64, "run past the end of a block"
                    blk[k] = v
                    k += 1
                coef[m, j] = blk
        assert nbits - 8 < pos <= nbits, "interval %d: %d bits used of %d" % (it, pos, nbits)
        tail = nbits - pos
        assert (acc >> 32) & ((1 << tail) - 1) == (1 << tail) - 1, "interval %d is not padded with 1-bits" % it
    info["coef"] = coef
    return info


def near_tie(ratio, margin=0.01):
    """True where the unrounded coef / Q lies within `margin` of a half-integer (where float32 and float64 may round apart)."""
    f = np.abs(ratio) % 1.0
    return np.abs(f - 0.5) <= margin


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    m = (d * d).mean()
    return float("inf") if m == 0 else 10 * np.log10(255.0 ** 2 / m)


# ---- inputs and cases shared by the CPU test of the model and the GPU tests ---------------------------------------------------------
def make_input(kind, H, W, C, batch=1, seed=0):
    """uint8 [batch,H,W,C].  clip: seeded frames of synthetic.make_clip, BGR by per-channel gains; texture: smooth texture + sinusoid +
    step + noise; noise: uniform; zeros / ones: constant 0 / 255; checker1 / checker8: 0 / 255 checkerboards of 1 / 8 pixels."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((batch, H, W, C), np.uint8)
    for b in range(batch):
        if kind == "clip":
            from stabnet_amd import synthetic
            g = (synthetic.make_clip(H, W, batch, seed=77 + seed, margin=32)[b].astype(np.float64) + 0.5) * 255.0
            gains, offs = (0.80, 1.00, 0.65), (20.0, 0.0, 60.0)
            f = np.stack([g * gains[c] + offs[c] for c in range(C)], -1) if C == 3 else g[..., None]
        elif kind == "texture":
            f = np.zeros((H, W, C))
            for c in range(C):
                smooth = 60 * np.sin(xx / (7.0 + 3 * c) + b) * np.cos(yy / (11.0 - 2 * c))
                sinus = 30 * np.sin(2 * np.pi * (xx + 2 * yy) / (5.0 + c))
                step = 50.0 * ((xx > W // 2 + 3 * c) ^ (yy > H // 3))
                f[..., c] = 100 + smooth + sinus + step + rng.normal(0, 6, (H, W))
        elif kind == "noise":
            f = rng.integers(0, 256, (H, W, C)).astype(np.float64)
        elif kind in ("zeros", "ones"):
            f = np.full((H, W, C), 0.0 if kind == "zeros" else 255.0)
        elif kind in ("checker1", "checker8"):
            s = 1 if kind == "checker1" else 8
            f = np.repeat((255.0 * (((xx // s) + (yy // s)) & 1))[..., None], C, -1)
        else:
            raise ValueError(kind)
        out[b] = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return out


def restart_of(R, H, W, C, subsampling):
    """'row' = one MCU row, 'all' = larger than the image (no RST at all)"""
    ms, _, mcux, mcuy, _ = geometry(H, W, C, subsampling)
    return mcux if R == "row" else (65535 if R == "all" else int(R))


# (kind, H, W, C, subsampling, quality, restart, batch): every size, subsampling, channel count, quality and restart shape at least once
GPU_CASES = [
    ("clip", 16, 16, 3, "420", 75, 1, 1),
    ("clip", 16, 16, 1, "420", 50, 2, 1),
    ("texture", 45, 77, 3, "420", 75, 7, 3),
    ("texture", 45, 77, 3, "444", 95, 1, 1),
    ("noise", 45, 77, 1, "420", 50, "all", 1),
    ("ones", 45, 77, 3, "444", 75, "row", 1),
    ("clip", 144, 176, 3, "420", 75, "row", 3),
    ("clip", 144, 176, 3, "444", 50, 2, 1),
    ("texture", 144, 176, 1, "420", 95, 7, 1),
    ("noise", 144, 176, 3, "420", 95, "all", 1),
    ("zeros", 144, 176, 3, "420", 75, 1, 1),
    ("texture", 288, 512, 3, "420", 75, 1, 1),
    ("clip", 288, 512, 3, "444", 95, "row", 1),
    ("clip", 288, 512, 1, "420", 50, 1, 3),
    ("clip", 720, 1280, 3, "420", 75, 1, 1),
    ("texture", 720, 1280, 1, "420", 75, "row", 1),
    ("clip", 1080, 1920, 3, "420", 75, 1, 1),
]


def case_id(c):
    return "%s-%dx%d-c%d-%s-q%d-r%s-n%d" % c
