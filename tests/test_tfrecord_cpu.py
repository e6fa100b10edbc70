"""CPU: stabnet_amd/tfrecord.py -- CRC32C, the record framing and the tf.train.Example wire format, against known answers and one
record that was serialised by Google's protobuf (not by this project's writer) and framed with an independently checked CRC."""
import os

import numpy as np
import pytest

from stabnet_amd import tfrecord
from stabnet_amd._lib import StabnetError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tfrecord_protobuf_example.tfrecords")
EXPECT = {"stable_path": b"stable/7/", "unstable_path": b"unstable/7/", "pos": [300], "flow": [0.5, -1.0],
          "feature_matches1": [0.25, -0.75, 1.0, 0.0], "feature_matches2": []}


def test_crc32c_known_answers():
    assert tfrecord.crc32c(b"123456789") == 0xE3069283
    assert tfrecord.crc32c(bytes(32)) == 0x8A9136AA
    assert tfrecord.crc32c(b"\xff" * 32) == 0x62A8AB43


def test_crc32c_bulk_path_agrees_with_the_byte_walk():
    data = np.random.default_rng(0).integers(0, 256, 4099, dtype=np.uint8).tobytes()     # long enough for the 8-bytes-a-step path
    c = 0xFFFFFFFF
    for v in data:
        c = tfrecord._T0[(c ^ v) & 0xFF] ^ (c >> 8)
    assert tfrecord.crc32c(data) == c ^ 0xFFFFFFFF


def _check(ex):
    assert sorted(ex) == sorted(EXPECT)
    assert ex["stable_path"] == EXPECT["stable_path"] and ex["unstable_path"] == EXPECT["unstable_path"]
    assert ex["pos"].dtype == np.int64 and ex["pos"].tolist() == EXPECT["pos"]
    for k in ("flow", "feature_matches1", "feature_matches2"):
        assert ex[k].dtype == np.float32 and ex[k].tolist() == EXPECT[k], k


def test_protobuf_written_record_reads_and_is_reproduced(tmp_path):
    raw = open(GOLDEN, "rb").read()
    assert len(raw) == 186
    recs = list(tfrecord.read_records(GOLDEN))
    assert len(recs) == 1 and len(recs[0]) == 170
    ex = tfrecord.parse_example(recs[0])
    _check(ex)
    out = str(tmp_path / "again.tfrecords")
    tfrecord.write_records(out, [tfrecord.encode_example(ex)])
    assert open(out, "rb").read() == raw
    # from plain Python values as well
    tfrecord.write_records(out, [tfrecord.encode_example({
        "stable_path": b"stable/7/", "unstable_path": b"unstable/7/", "pos": np.array([300], np.int64),
        "flow": np.array([0.5, -1.0], np.float32), "feature_matches1": np.array([0.25, -0.75, 1.0, 0.0], np.float32),
        "feature_matches2": np.zeros(0, np.float32)})])
    assert open(out, "rb").read() == raw


def test_negative_int64_is_a_ten_byte_varint():
    ex = tfrecord.parse_example(bytes.fromhex("0a170a150a03706f73120e1a0c0a0affffffffffffffffff01"))
    assert ex["pos"].dtype == np.int64 and ex["pos"].tolist() == [-1]
    assert tfrecord.encode_example({"pos": np.array([-1], np.int64)}) == bytes.fromhex("0a170a150a03706f73120e1a0c0a0affffffffffffffffff01")


def test_unpacked_lists_and_unknown_fields_parse():
    def ld(num, payload):                                           # a length-delimited field, written by hand
        n, ln = len(payload), b""
        while n >= 0x80:
            ln, n = ln + bytes([n & 0x7F | 0x80]), n >> 7
        return bytes([num << 3 | 2]) + ln + bytes([n]) + payload
    f32 = lambda v: np.float32(v).tobytes()
    # FloatList with two UNPACKED values (tag 0x0d = field 1, 32-bit), Int64List with unpacked varints (tag 0x08)
    flow = ld(2, b"\x0d" + f32(0.5) + b"\x0d" + f32(-1.0))
    pos = ld(3, b"\x08\x07" + b"\x08" + b"\xff" * 9 + b"\x01")
    # unknown fields of all four readable wire types in front of the known one: varint (field 9), 64-bit (10), bytes (11), 32-bit (12)
    junk = b"\x48\x96\x01" + b"\x51" + bytes(8) + ld(11, b"abc") + b"\x65" + bytes(4)
    entry = lambda key, feat: ld(1, junk + ld(1, key) + ld(2, junk + feat))
    msg = junk + ld(1, junk + entry(b"flow", flow) + entry(b"pos", pos)) + junk
    ex = tfrecord.parse_example(msg)
    assert ex["flow"].dtype == np.float32 and ex["flow"].tolist() == [0.5, -1.0]
    assert ex["pos"].tolist() == [7, -1]


@pytest.mark.parametrize("what", ["payload bit", "length bit", "truncated"])
def test_damaged_files_are_refused(tmp_path, what):
    raw = bytearray(open(GOLDEN, "rb").read() * 2)                 # two records: the second one is damaged
    if what == "payload bit":
        raw[186 + 12 + 40] ^= 0x10
    elif what == "length bit":
        raw[186 + 1] ^= 0x01
    else:
        raw = raw[:-9]
    path = str(tmp_path / "bad.tfrecords")
    open(path, "wb").write(bytes(raw))
    with pytest.raises(StabnetError) as e:
        list(tfrecord.read_records(path))
    assert path in str(e.value) and "record 1" in str(e.value)
    it = tfrecord.read_records(path)
    assert len(next(it)) == 170                                     # the first record is intact and is delivered
