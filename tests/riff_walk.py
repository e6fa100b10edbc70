"""Helper of the AVI tests (not a test): an independent walk over a RIFF AVI file that checks the container's arithmetic as it goes.
Returns {"avih": tuple of 14 dwords, "strh": dict, "strf": dict, "frames": [(offset of the chunk, size)], "idx1": [(ckid, flags, offset,
size)], "movi_fourcc": offset}."""
import struct


def walk(path):
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:12] == b"AVI "
    riff_size = struct.unpack_from("<I", d, 4)[0]
    assert riff_size == len(d) - 8, "RIFF size %d, file %d" % (riff_size, len(d))
    out = {"frames": [], "idx1": [], "lists": []}

    def chunks(p, end, depth):
        while p < end:
            assert p + 8 <= end, "truncated chunk header at %d" % p
            cid, size = d[p:p + 4], struct.unpack_from("<I", d, p + 4)[0]
            body = p + 8
            assert body + size <= end, "chunk %r at %d runs past its parent" % (cid, p)
            if cid == b"LIST":
                kind = d[body:body + 4]
                out["lists"].append(kind)
                if kind == b"movi":
                    out["movi_fourcc"] = body
                chunks(body + 4, body + size, depth + 1)
            elif cid == b"avih":
                assert size == 56
                out["avih"] = struct.unpack_from("<14I", d, body)
            elif cid == b"strh":
                assert size == 56
                v = struct.unpack_from("<4s4sIHHIIIIIIII4H", d, body)
                out["strh"] = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], length=v[9], rect=v[13:17])
            elif cid == b"strf":
                assert size == 40
                v = struct.unpack_from("<IiiHH4sIiiII", d, body)
                out["strf"] = dict(size=v[0], width=v[1], height=v[2], planes=v[3], bits=v[4], compression=v[5])
            elif cid == b"00dc":
                out["frames"].append((p, size))
            elif cid == b"idx1":
                assert size % 16 == 0
                out["idx1"] = [struct.unpack_from("<4sIII", d, body + 16 * i) for i in range(size // 16)]
            else:
                raise AssertionError("unexpected chunk %r at %d" % (cid, p))
            if size & 1:
                assert d[body + size] == 0, "pad byte"
            p = body + size + (size & 1)
            assert p % 2 == 0, "chunks start at even offsets"
        assert p == end, "chunks do not fill their parent"

    chunks(12, len(d), 0)
    assert out["lists"] == [b"hdrl", b"strl", b"movi"]
    for ckid, flags, off, size in out["idx1"]:
        at = out["movi_fourcc"] + off
        assert ckid == b"00dc" and d[at:at + 4] == b"00dc" and struct.unpack_from("<I", d, at + 4)[0] == size
        assert flags & 0x10
    assert [(out["movi_fourcc"] + e[2], e[3]) for e in out["idx1"]] == out["frames"]
    out["data"] = d
    return out


def jpeg_of(w, i):
    p, n = w["frames"][i]
    return w["data"][p + 8:p + 8 + n]
