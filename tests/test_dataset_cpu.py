"""CPU: the host side of stabnet_amd/dataset.py on tiny frame-less records (write_dataset in tmp_path): which frame feeds which
channel, the shard split, the reproducible order, and what is refused.  No frame file is opened and no GPU is touched."""
import os

import numpy as np
import pytest

from stabnet_amd._lib import StabnetError
from stabnet_amd.config import Config
from stabnet_amd.dataset import PairDataset, write_dataset

H, W = 4, 6


def _samples(n, rng, flow=True):
    out = []
    for i in range(n):
        k = int(rng.integers(0, 5))
        out.append({"stable_path": "stable/%d/" % (i % 3), "unstable_path": "/abs/unstable/%d/" % (i % 3), "pos": 40 + i,
                    "flow": rng.normal(size=(H, W, 3)).astype(np.float32) if flow else (),
                    "feature_matches1": rng.uniform(-1, 1, (k, 4)).astype(np.float32),
                    "feature_matches2": rng.uniform(-1, 1, (k + 1, 4)).astype(np.float32)})
    return out


@pytest.fixture()
def data(tmp_path):
    rng = np.random.default_rng(0)
    samples = _samples(23, rng)
    names = write_dataset(str(tmp_path), "train", samples, records_per_file=10)
    assert len(names) == 3 and open(os.path.join(str(tmp_path), "train", "list.txt")).read() == " ".join(names)
    return str(tmp_path), samples


def _ds(d, **kw):
    cfg = kw.pop("cfg", Config(max_matches=8))
    return PairDataset(d, "train", cfg, H, W, batch=2, **kw)


def test_channel_to_position_map(data):
    d, samples = data
    cfg = Config(max_matches=8)
    ds = _ds(d, cfg=cfg)
    assert len(ds.records) == 23 and cfg.indices == (0, 1, 2, 4, 8, 16, 32)
    rec = ds.records[5]
    assert rec.pos == 45 and rec.number == 5 and rec.file.endswith("train_00000.tfrecords")
    st, un = ds.frame_files(rec)
    rel = lambda n: os.path.join(d, "stable/2/%d.jpg" % n)               # a path that is not absolute is relative to data_dir
    assert st[:7] == [rel(45 - 1 - i) for i in cfg.indices]              # tower 1: pos - 1 - indices[k]
    assert st[7:] == [rel(45 - i) for i in cfg.indices]                  # tower 2: pos - indices[k]
    assert st[0] == rel(44) and st[7] == rel(45) and st[13] == rel(13)   # no zero padding
    assert un == ["/abs/unstable/2/44.jpg", "/abs/unstable/2/45.jpg"]    # unstable: pos - 1 and pos
    assert st[0] == st[8] and st[1] == st[9]                             # pos-1 and pos-2 feed both towers:
    assert len(st + un) == 16 and len(set(st + un)) == 14                # 16 frames per sample, 14 distinct files


def test_host_sample_passes_flow_and_matches_through(data):
    d, samples = data
    ds = _ds(d)
    s = ds.host_sample(ds.records[12])
    src = samples[12]
    assert np.array_equal(s["flow"], src["flow"][:, :, :2]) and s["flow"].dtype == np.float32
    n1, n2 = len(src["feature_matches1"]), len(src["feature_matches2"])
    assert (s["n1"], s["n2"]) == (n1, n2) and s["matches1"].shape == (8, 4)
    assert np.array_equal(s["matches1"][:n1], src["feature_matches1"]) and not s["matches1"][n1:].any()
    assert np.array_equal(s["matches2"][:n2], src["feature_matches2"]) and not s["matches2"][n2:].any()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_shards_are_disjoint_and_complete(data, world):
    d, _ = data
    shards = [_ds(d, rank=r, world=world, shuffle=False) for r in range(world)]
    got = [s.shard for s in shards]
    assert sorted(sum(got, [])) == list(range(23))
    assert all(g == list(range(r, 23, world)) for r, g in enumerate(got))
    # unshuffled, a rank walks its shard in order and starts again (num_epochs=None)
    n = len(got[-1])
    assert shards[-1].next_indices(n + 2) == got[-1] + got[-1][:2]


def test_order_is_a_function_of_seed_rank_world(data):
    d, _ = data
    a = _ds(d, seed=7, rank=1, world=2).next_indices(300)
    assert a == _ds(d, seed=7, rank=1, world=2, prefetch=0, workers=1).next_indices(300)
    b = _ds(d, seed=7, rank=1, world=2)
    assert a == b.next_indices(100) + b.next_indices(200)               # however the draws are batched
    assert set(a) == set(range(1, 23, 2))                                # only its own shard, all of it
    assert a != _ds(d, seed=8, rank=1, world=2).next_indices(300)
    assert a != sorted(a) and a[:11] != list(range(1, 23, 2))            # shuffled
    # the buffer holds 120 and more than 80 stay after a draw: nothing is drawn before 120 went in, so one record can recur early
    assert len(b._buffer) == 119


def test_too_many_matches_are_refused(tmp_path):
    rng = np.random.default_rng(1)
    s = _samples(3, rng)
    s[2]["feature_matches2"] = np.zeros((8, 4), np.float32)              # == max_matches: the reference asserts count < max_matches
    write_dataset(str(tmp_path), "train", s)
    with pytest.raises(StabnetError) as e:
        _ds(str(tmp_path))
    assert "record 2" in str(e.value) and "train_00000.tfrecords" in str(e.value) and "max_matches" in str(e.value)
    s[2]["feature_matches2"] = np.zeros((7, 4), np.float32)
    write_dataset(str(tmp_path), "train", s)
    assert _ds(str(tmp_path)).records[2].n2 == 7


@pytest.mark.parametrize("shape", [(H, W, 1), (H * W * 2 + 1,)])
def test_bad_flow_length_is_refused(tmp_path, shape):
    s = _samples(2, np.random.default_rng(2))
    s[1]["flow"] = np.zeros(shape, np.float32)                           # fewer than 2 channels / no multiple of H * W
    write_dataset(str(tmp_path), "train", s)
    with pytest.raises(StabnetError) as e:
        _ds(str(tmp_path))
    assert "record 1" in str(e.value) and "flow" in str(e.value)


def test_empty_flow_becomes_zeros_and_says_so_once(tmp_path, capsys):
    write_dataset(str(tmp_path), "train", _samples(4, np.random.default_rng(3), flow=False))
    ds = _ds(str(tmp_path))
    for r in ds.records:
        f = ds.host_sample(r)["flow"]
        assert f.shape == (H, W, 2) and f.dtype == np.float32 and not f.any()
    assert capsys.readouterr().out.count("empty flow") == 1
