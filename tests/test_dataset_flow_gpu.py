"""GPU: the records' flow.  tools/make_dataset.py --flow tvl1, run as a child process, stores for every record the TV-L1 map of
the y1 / y2 channels PairDataset yields for it; PairDataset(flow="tvl1") computes that same map for records written without one;
and a training step on such a batch has a temporal loss that zeros do not give.  Everything bit for bit (torch.equal)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dataset_fixture as Fx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = Fx.H, Fx.W
RECORDS = 2 * (Fx.T - 33)                  # positions 33 .. T - 1 of two clip pairs


def _make(clips, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), "--out", out, "--split", "train"]
    for s, u in clips:
        cmd += ["--pair", s, u]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(dataset written with --flow tvl1, the same written with --flow none)."""
    d = tmp_path_factory.mktemp("flow")
    clips = []
    for k in range(2):
        pair = []
        for kind in range(2):
            path = str(d / ("clip%d_%d.npy" % (k, kind)))
            np.save(path, np.stack([Fx.image(k, t, kind)[:, :, ::-1] for t in range(Fx.T)]))        # BGR
            pair.append(path)
        clips.append(pair)
    out = _make(clips, str(d / "tvl1"), "--flow", "tvl1", "--flow-batch", "3", "--height", str(H), "--width", str(W))
    assert "flow: TV-L1 at %dx%d for %d records" % (W, H, RECORDS) in out
    _make(clips, str(d / "none"), "--flow", "none")
    return str(d / "tvl1"), str(d / "none")


def _cfg(h=H, w=W, **kw):
    from stabnet_amd.config import Config
    return Config(height=h, width=w, **kw)


def _all_batches(ds, batch):
    out = []
    for _ in range(RECORDS // batch):
        b = ds.next_batch()
        out.append((b["stable"], b["flow"]))
    return out


def test_stored_flow_is_the_flow_of_what_training_reads(cuda, roots):
    import torch
    from stabnet_amd import flow
    from stabnet_amd.dataset import PairDataset
    cfg = _cfg()
    y2 = len(cfg.indices)                                            # = before_ch + 1: stable frame pos; channel 0: frame pos - 1
    with PairDataset(roots[0], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=1) as ds:
        assert len(ds.records) == RECORDS and all(r.flow_len == H * W * 2 for r in ds.records)
        batches = _all_batches(ds, 2)
    moved = 0
    for stable, stored in batches:
        want = flow.tvl1_flow(stable[..., 0], stable[..., y2], out="map", offset=0.5, scale=255.0)
        assert stored.shape == (2, H, W, 2) and torch.equal(stored, want)
        ident = flow.tvl1_flow(stable[..., 0], stable[..., 0], out="map", offset=0.5, scale=255.0)
        moved += int((stored != ident).sum())
    assert moved > 0                                                 # the frames of the fixture differ: the flow is not the identity


def test_dataset_computes_the_same_flow_for_records_without_one(cuda, roots):
    import torch
    from stabnet_amd.dataset import PairDataset
    cfg = _cfg()
    with PairDataset(roots[0], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=0) as ds:
        stored = _all_batches(ds, 2)
    got = {}
    for prefetch in (0, 1):
        with PairDataset(roots[1], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=prefetch, flow="tvl1") as ds:
            assert all(r.flow_len == 0 for r in ds.records)
            got[prefetch] = _all_batches(ds, 2)
    for (s0, f0), (s1, f1), (s, f) in zip(got[0], got[1], stored):
        assert torch.equal(s0, s) and torch.equal(s1, s)
        assert torch.equal(f0, f) and torch.equal(f1, f)
    # the default keeps the zeros (and records that carry a flow keep it under flow="tvl1")
    with PairDataset(roots[1], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=0) as ds:
        assert not ds.next_batch()["flow"].any()
    with PairDataset(roots[0], "train", cfg, H, W, batch=2, device=cuda, shuffle=False, prefetch=0, flow="tvl1") as ds:
        assert torch.equal(ds.next_batch()["flow"], stored[0][1])


def test_bad_flow_mode_is_refused(roots):
    from stabnet_amd._lib import StabnetError
    from stabnet_amd.dataset import PairDataset
    with pytest.raises(StabnetError, match="flow must be"):
        PairDataset(roots[1], "train", _cfg(), H, W, batch=2, flow="farneback")


def test_a_training_step_sees_the_flow(cuda, roots):
    """One step at 64x96 (the smallest size the other dataset tests train at) on a batch whose flow the dataset computed: the
    temporal loss is finite and is not the one zeros give."""
    import torch
    from stabnet_amd import data, synthetic
    from stabnet_amd.dataset import PairDataset
    from stabnet_amd.train import Trainer, loss_gates
    N, h, w = 2, 64, 96
    cfg = _cfg(h, w, batch_size=N)
    with PairDataset(roots[1], "train", cfg, h, w, batch=N, device=cuda, seed=1, flow="tvl1") as ds:
        raw = ds.next_batch()
    assert raw["flow"].shape == (N, h, w, 2) and bool(torch.isfinite(raw["flow"]).all())
    tr = Trainer(synthetic.make_params(cfg, seed=0, theta_scale=0.2), N, h, w, cfg, device=cuda)
    gates = loss_gates(cfg.do_temp_loss_iter, cfg)
    assert gates["use_temp_loss"] == 1
    temp = []
    for fl in (raw["flow"], torch.zeros_like(raw["flow"])):
        para, jitter, Hs = data.draw(np.random.default_rng(0), cfg, N, h, w)
        x1, y1, x2, y2, f, fm1, mk1, fm2, mk2 = data.augment_pairs(raw["stable"], raw["unstable"], fl, raw["matches1"], raw["n1"],
                                                                   raw["matches2"], raw["n2"], para, jitter, Hs, cfg)
        batch = {"x1": x1, "y1": y1, "x2": x2, "y2": y2, "flow": f, "matches1": fm1, "mask1": mk1, "matches2": fm2, "mask2": mk2}
        tr.forward_backward(batch, gates, apply_update=False)
        torch.cuda.synchronize()
        temp.append(tr.losses()["temp_loss"])
    assert np.isfinite(temp[0]) and np.isfinite(temp[1]), temp
    assert temp[0] != temp[1], temp
