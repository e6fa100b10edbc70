"""TFRecord files and tf.train.Example messages without TensorFlow or a protobuf package: what the reference's
tf.TFRecordReader / tf.parse_single_example (get_data_mini_after.py:166-176) read, and the writer that inverts it.

Framing of one record [external: TensorFlow's record writer]: uint64 little-endian payload length, uint32 masked CRC32C of those 8
bytes, the payload, uint32 masked CRC32C of the payload.  CRC32C is the Castagnoli polynomial (reflected 0x82F63B78); the mask is
((c >> 15 | c << 17) + 0xa282ead8) mod 2^32.

Wire format read [external: protobuf encoding; tensorflow/core/example/{example,feature}.proto]: Example.features = 1;
Features.feature = map at 1 (entry: key = 1, value = 2); Feature = oneof bytes_list = 1 / float_list = 2 / int64_list = 3; every list
`repeated value = 1`, float and int64 accepted packed and unpacked; unknown fields are skipped by their wire type."""
from __future__ import annotations

import struct

import numpy as np

from ._lib import StabnetError

_POLY = 0x82F63B78
_MASK_DELTA = 0xA282EAD8


def _make_tables():
    t0 = np.zeros(256, np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ _POLY if c & 1 else c >> 1
        t0[i] = c
    t = np.zeros((8, 256), np.uint32)
    t[0] = t0
    for k in range(1, 8):
        t[k] = (t[k - 1] >> np.uint32(8)) ^ t0[t[k - 1] & np.uint32(0xFF)]
    return t


_T = _make_tables()
_T0 = [int(v) for v in _T[0]]


def crc32c(data) -> int:
    """CRC32C (Castagnoli) of a bytes-like.  Slicing-by-8 over NumPy columns for the bulk (flow payloads are megabytes), a plain
    table walk for the remainder."""
    b = np.frombuffer(bytes(data), np.uint8)
    c = 0xFFFFFFFF
    n8 = len(b) // 8
    if n8 >= 64:
        # the table terms of each 8-byte word that do not depend on the running CRC, for all words at once
        w = b[:n8 * 8].reshape(n8, 8)
        hi = (_T[3][w[:, 4]] ^ _T[2][w[:, 5]] ^ _T[1][w[:, 6]] ^ _T[0][w[:, 7]]).tolist()
        lo = (w[:, 0].astype(np.uint32) | (w[:, 1].astype(np.uint32) << 8) | (w[:, 2].astype(np.uint32) << 16)
              | (w[:, 3].astype(np.uint32) << 24)).tolist()
        t7, t6, t5, t4 = ([int(v) for v in _T[k]] for k in (7, 6, 5, 4))
        for i in range(n8):
            x = c ^ lo[i]
            c = t7[x & 0xFF] ^ t6[(x >> 8) & 0xFF] ^ t5[(x >> 16) & 0xFF] ^ t4[x >> 24] ^ hi[i]
        rest = b[n8 * 8:].tolist()
    else:
        rest = b.tolist()
    for v in rest:
        c = _T0[(c ^ v) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc(data) -> int:
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + _MASK_DELTA) & 0xFFFFFFFF


def read_record_at(f, path, index, check=True):
    """The record at the file object's position -> payload, or None at a clean end of file."""
    head = f.read(12)
    if not head:
        return None
    what = "%s: record %d" % (path, index)
    if len(head) < 12:
        raise StabnetError("%s is truncated (%d of 12 header bytes)" % (what, len(head)))
    n, crc = struct.unpack("<QI", head)
    if check and masked_crc(head[:8]) != crc:
        raise StabnetError("%s: the CRC of the length field does not match (corrupt file)" % what)
    body = f.read(n + 4) if n < (1 << 40) else b""
    if len(body) < n + 4:
        raise StabnetError("%s is truncated (%d of %d payload + CRC bytes)" % (what, len(body), n + 4))
    if check and masked_crc(body[:n]) != struct.unpack("<I", body[n:])[0]:
        raise StabnetError("%s: the CRC of the payload does not match (corrupt file)" % what)
    return body[:n]


def read_records(path, with_offsets=False):
    """Yields the payloads of a TFRecord file (with_offsets: (byte offset of the record, payload))."""
    with open(path, "rb") as f:
        i = 0
        while True:
            off = f.tell()
            p = read_record_at(f, path, i)
            if p is None:
                return
            yield (off, p) if with_offsets else p
            i += 1


def write_records(path, payloads):
    with open(path, "wb") as f:
        for p in payloads:
            p = bytes(p)
            head = struct.pack("<Q", len(p))
            f.write(head + struct.pack("<I", masked_crc(head)) + p + struct.pack("<I", masked_crc(p)))


# ---- protobuf wire format -------------------------------------------------------------------------------------------------------

def _varint(b, i):
    v = s = 0
    while True:
        if i >= len(b):
            raise StabnetError("parse_example: a varint runs past the end of the message")
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        if c < 0x80:
            return v & 0xFFFFFFFFFFFFFFFF, i
        s += 7
        if s > 63:
            raise StabnetError("parse_example: a varint is longer than ten bytes")


def _fields(b):
    """(field number, wire type, value) of every field of a message: value = int (varint), bytes (64-bit, length-delimited, 32-bit)."""
    i = 0
    while i < len(b):
        key, i = _varint(b, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(b, i)
        elif wt in (1, 5):
            n = 8 if wt == 1 else 4
            v, i = b[i:i + n], i + n
        elif wt == 2:
            n, i = _varint(b, i)
            v, i = b[i:i + n], i + n
            if i > len(b):
                raise StabnetError("parse_example: field %d (%d bytes) runs past the end of the message" % (num, n))
        else:
            raise StabnetError("parse_example: field %d has wire type %d (groups are not read)" % (num, wt))
        if i > len(b):
            raise StabnetError("parse_example: field %d runs past the end of the message" % num)
        yield num, wt, v


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def _feature(b, name):
    kind, val = None, None
    for num, wt, v in _fields(b):
        if wt != 2 or num not in (1, 2, 3):
            continue                                           # unknown field
        kind = num
        if num == 1:                                           # BytesList
            val = [bytes(x) for n2, w2, x in _fields(v) if n2 == 1 and w2 == 2]
        elif num == 2:                                         # FloatList: packed (wire type 2) or unpacked (5)
            parts = [bytes(x) for n2, w2, x in _fields(v) if n2 == 1 and w2 in (2, 5)]
            raw = b"".join(parts)
            if len(raw) % 4:
                raise StabnetError("parse_example: float_list of %r holds %d bytes, no multiple of 4" % (name, len(raw)))
            val = np.frombuffer(raw, "<f4").astype(np.float32)
        else:                                                  # Int64List: packed (2) or unpacked (0)
            out = []
            for n2, w2, x in _fields(v):
                if n2 != 1:
                    continue
                if w2 == 0:
                    out.append(_signed(x))
                elif w2 == 2:
                    j = 0
                    while j < len(x):
                        u, j = _varint(x, j)
                        out.append(_signed(u))
            val = np.array(out, np.int64)
    if kind is None:
        return np.zeros(0, np.float32)                         # a Feature with no list set
    if kind == 1:
        return val[0] if len(val) == 1 else val                # the reference's string features are scalars
    return val


def parse_example(data) -> dict:
    """tf.train.Example -> {name: bytes (a one-element bytes_list; a list of bytes otherwise) | np.float32 array | np.int64 array}."""
    data = bytes(data)
    out = {}
    for num, wt, feats in _fields(data):
        if num != 1 or wt != 2:
            continue
        for n1, w1, entry in _fields(feats):
            if n1 != 1 or w1 != 2:
                continue
            key, value = None, b""
            for n2, w2, v in _fields(entry):
                if n2 == 1 and w2 == 2:
                    key = bytes(v).decode("utf-8")
                elif n2 == 2 and w2 == 2:
                    value = v
            if key is not None:
                out[key] = _feature(value, key)
    return out


def _enc_varint(v):
    v &= 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _ld(num, payload):
    return _enc_varint(num << 3 | 2) + _enc_varint(len(payload)) + payload


def encode_example(features: dict) -> bytes:
    """The inverse of parse_example: keys sorted, float and int64 lists packed (an empty list is an empty message)."""
    entries = b""
    for key in sorted(features):
        v = features[key]
        if isinstance(v, (bytes, bytearray, str)):
            v = v.encode("utf-8") if isinstance(v, str) else bytes(v)
            feat = _ld(1, _ld(1, v))
        elif isinstance(v, (list, tuple)) and v and all(isinstance(x, (bytes, bytearray)) for x in v):
            feat = _ld(1, b"".join(_ld(1, bytes(x)) for x in v))
        else:
            a = np.asarray(v)
            if a.dtype.kind in "iub":
                body = b"".join(_enc_varint(int(x)) for x in a.reshape(-1))
                feat = _ld(3, _ld(1, body) if a.size else b"")
            else:
                a = a.astype("<f4").reshape(-1)
                feat = _ld(2, _ld(1, a.tobytes()) if a.size else b"")
        entries += _ld(1, _ld(1, key.encode("utf-8")) + _ld(2, feat))
    return _ld(1, entries)
