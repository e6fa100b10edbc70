"""GPU: the records' feature matches.  tools/make_dataset.py --features klt, run as a child process, stores for every record the
matches of the channels PairDataset yields for it; PairDataset(matches="klt") computes the same rows for records written without
any; records that carry rows keep them; and a training step on such a batch has a feature loss that no matches do not give.
Everything bit for bit (torch.equal).  The clips are made here from tvl1_model.texture: the unstable clip is the stable one
shifted by a few pixels per frame (the frames of dataset_fixture are noise-dominated and give almost no matches)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tvl1_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 64, 96, 36
RECORDS = 2 * (T - 33)                     # positions 33 .. T - 1 of two clip pairs


def clip_pair(k):
    """uint8 [T,H,W] grey clips: windows of one texture; the stable window drifts slowly, the unstable one jumps round it."""
    tex = np.round(M.texture(H + 24, W + 24, 40 + k) * 255).astype(np.uint8)
    stable, unstable = [], []
    for t in range(T):
        y, x = 10 + t // 12, 10 + t // 9
        dy, dx = (t * 5) % 7 - 3, (t * 3) % 9 - 4
        stable.append(tex[y:y + H, x:x + W])
        unstable.append(tex[y + dy:y + dy + H, x + dx:x + dx + W])
    return np.stack(stable), np.stack(unstable)


def _make(clips, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), "--out", out, "--split", "train"]
    for s, u in clips:
        cmd += ["--pair", s, u]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(dataset written with --features klt, the same written with --features none)."""
    d = tmp_path_factory.mktemp("features")
    clips = []
    for k in range(2):
        paths = [str(d / ("clip%d_%d.npy" % (k, kind))) for kind in range(2)]
        for p, c in zip(paths, clip_pair(k)):
            np.save(p, c)
        clips.append(paths)
    out = _make(clips, str(d / "klt"), "--features", "klt", "--flow-batch", "4", "--height", str(H), "--width", str(W))
    assert "features: KLT at %dx%d for %d records" % (W, H, RECORDS) in out
    _make(clips, str(d / "none"), "--features", "none")
    return str(d / "klt"), str(d / "none")


def _cfg(**kw):
    from stabnet_amd.config import Config
    return Config(height=H, width=W, **kw)


KEYS = ("stable", "unstable", "matches1", "n1", "matches2", "n2")


def _all_batches(ds, batch, split_records=RECORDS):
    out = []
    for _ in range(split_records // batch):
        b = ds.next_batch()
        out.append({k: b[k] for k in KEYS})
    return out


def _counts(n):
    import torch
    return n.cpu().numpy() if torch.is_tensor(n) else np.asarray(n)


def test_stored_rows_are_the_matches_of_what_training_reads(cuda, roots):
    import torch
    from stabnet_amd import features
    from stabnet_amd.dataset import PairDataset
    cfg = _cfg()
    y2 = len(cfg.indices)                                            # stable frame pos; channel 0: frame pos - 1
    with PairDataset(roots[0], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=1) as ds:
        assert len(ds.records) == RECORDS
        batches = _all_batches(ds, 2)
    total = 0
    for b in batches:
        assert isinstance(b["n1"], np.ndarray)                       # the default mode: counts on the host, as before
        for k, cs, cu in (("1", 0, 0), ("2", y2, 1)):
            rows, n = features.klt_matches(b["stable"][..., cs], b["unstable"][..., cu], cfg.max_matches, offset=0.5, scale=255.0)
            assert np.array_equal(n.cpu().numpy(), b["n" + k])
            assert b["matches" + k].shape == (2, cfg.max_matches, 4) and torch.equal(b["matches" + k], rows)
            total += int(n.sum())
    assert total >= 10 * 2 * RECORDS                                 # of 24 cells a list; the texture gives corners in most


def test_dataset_computes_the_same_rows_for_records_without_any(cuda, roots):
    import torch
    from stabnet_amd.dataset import PairDataset
    cfg = _cfg()
    with PairDataset(roots[0], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=0) as ds:
        stored = _all_batches(ds, 2)
    for prefetch in (0, 1):
        with PairDataset(roots[1], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=prefetch, matches="klt") as ds:
            assert all(r.n1 == 0 and r.n2 == 0 for r in ds.records)
            got = _all_batches(ds, 2)
        for g, s in zip(got, stored):
            assert torch.equal(g["stable"], s["stable"]) and torch.equal(g["unstable"], s["unstable"])
            for k in ("1", "2"):
                assert torch.is_tensor(g["n" + k]) and g["n" + k].dtype == torch.int32 and g["n" + k].is_cuda
                assert np.array_equal(_counts(g["n" + k]), s["n" + k])
                assert torch.equal(g["matches" + k], s["matches" + k])
    # the default keeps the empty lists
    with PairDataset(roots[1], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=0) as ds:
        b = ds.next_batch()
        assert not b["n1"].any() and not b["n2"].any() and not b["matches1"].any() and not b["matches2"].any()


def test_records_that_carry_rows_keep_them(cuda, roots):
    """A split whose records hold rows of their own in one list, the other, both or neither: only the empty lists are computed."""
    import torch
    from stabnet_amd.dataset import PairDataset, write_dataset
    cfg = _cfg()
    rng = np.random.default_rng(7)
    own = {}
    samples = []
    for i, pos in enumerate((33, 34, 35, 33)):
        s = {"stable_path": "stable/0/", "unstable_path": "unstable/0/", "pos": pos}
        for k in ("1", "2"):
            if (i >> (k == "2")) & 1:
                own[i, k] = s["feature_matches" + k] = rng.uniform(-1, 1, (3 + i, 4)).astype(np.float32)
        samples.append(s)
    write_dataset(roots[1], "mixed", samples)
    with PairDataset(roots[0], "train", cfg, H, W, batch=3, device=cuda, shuffle=False, prefetch=0) as ds:
        klt = ds.next_batch()                                        # records 0, 1, 2: positions 33, 34, 35 of pair 0
    with PairDataset(roots[1], "mixed", cfg, H, W, batch=4, device=cuda, shuffle=False, prefetch=0, matches="klt") as ds:
        b = ds.next_batch()
    for i in range(4):
        for k in ("1", "2"):
            rows, n = b["matches" + k][i], int(b["n" + k][i])
            if (i, k) in own:
                assert n == len(own[i, k]) and np.array_equal(rows[:n].cpu().numpy(), own[i, k]) and not rows[n:].any()
            else:
                assert n == int(klt["n" + k][i % 3]) and n > 0 and torch.equal(rows, klt["matches" + k][i % 3])
    # a dataset whose records all carry rows comes through matches="klt" as it is (with the counts on the device)
    with PairDataset(roots[0], "train", cfg, H, W, batch=3, device=cuda, shuffle=False, prefetch=0, matches="klt") as ds:
        again = ds.next_batch()
    for k in ("1", "2"):
        assert torch.equal(again["matches" + k], klt["matches" + k]) and np.array_equal(_counts(again["n" + k]), klt["n" + k])


def test_bad_matches_mode_is_refused(roots):
    from stabnet_amd._lib import StabnetError
    from stabnet_amd.dataset import PairDataset
    with pytest.raises(StabnetError, match="matches must be"):
        PairDataset(roots[1], "train", _cfg(), H, W, batch=2, matches="surf")


def test_a_training_step_sees_the_matches(cuda, roots):
    """One step at 64x96 on a batch whose matches the dataset computed: the feature loss is finite and is not the one that no
    matches give."""
    import torch
    from stabnet_amd import data, synthetic
    from stabnet_amd.dataset import PairDataset
    from stabnet_amd.train import Trainer, loss_gates
    N = 2
    cfg = _cfg(batch_size=N)
    with PairDataset(roots[1], "train", cfg, H, W, batch=N, device=cuda, seed=1, matches="klt") as ds:
        raw = ds.next_batch()
    assert int(raw["n1"].max()) > 0 and int(raw["n2"].max()) > 0
    tr = Trainer(synthetic.make_params(cfg, seed=0, theta_scale=0.2), N, H, W, cfg, device=cuda)
    gates = loss_gates(cfg.do_temp_loss_iter, cfg)
    feat = []
    for n1, n2 in ((raw["n1"], raw["n2"]), (torch.zeros_like(raw["n1"]), torch.zeros_like(raw["n2"]))):
        para, jitter, Hs = data.draw(np.random.default_rng(0), cfg, N, H, W)
        x1, y1, x2, y2, f, fm1, mk1, fm2, mk2 = data.augment_pairs(raw["stable"], raw["unstable"], raw["flow"], raw["matches1"], n1,
                                                                   raw["matches2"], n2, para, jitter, Hs, cfg)
        batch = {"x1": x1, "y1": y1, "x2": x2, "y2": y2, "flow": f, "matches1": fm1, "mask1": mk1, "matches2": fm2, "mask2": mk2}
        tr.forward_backward(batch, gates, apply_update=False)
        torch.cuda.synchronize()
        feat.append(tr.losses()["feature_loss"])
    assert np.isfinite(feat[0]) and np.isfinite(feat[1]), feat
    assert feat[0] != feat[1], feat
