"""GPU: stabnet_amd/dataset.py end to end on a small dataset written here with Pillow: numbered JPEG frames (quality 90, 4:2:0) of two
clip pairs, TFRecord files through write_dataset.  stable / unstable must equal tests/tf_image_model.py applied to PILLOW'S decode of
the same files BIT FOR BIT (the device decoder is libjpeg-turbo's arithmetic, the get_img kernel TensorFlow 1.3's); flow, matches
and counts pass through; prefetch 0 and 1 give the same bytes; a 4:2:2 clip takes the Pillow fallback; and the batch trains."""
import functools
import os

import numpy as np
import pytest

import tf_image_model as M
from dataset_fixture import H, MAXM, W, image as _image, samples as _samples, write_frames as _write_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    from stabnet_amd.dataset import write_dataset
    d = str(tmp_path_factory.mktemp("pairs"))
    _write_frames(d)
    write_dataset(d, "train", _samples((H, W)), records_per_file=5)
    write_dataset(d, "big", _samples((64, 96), flow=False), records_per_file=5)          # for the 64x96 training step: empty flow
    return d


@functools.lru_cache(maxsize=None)
def _want(path, h, w):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "RGB"
    return M.get_img(np.asarray(im), h, w)


def _cfg():
    from stabnet_amd.config import Config
    return Config(height=H, width=W, max_matches=MAXM)


def _check_batch(ds, batch, indices, samples, h, w):
    import torch
    assert batch["stable"].shape == (len(indices), h, w, 14) and batch["unstable"].shape == (len(indices), h, w, 2)
    assert batch["stable"].dtype == torch.float32 and batch["stable"].is_cuda
    st_d, un_d = batch["stable"].cpu(), batch["unstable"].cpu()
    for n, i in enumerate(indices):
        st, un = ds.frame_files(ds.records[i])
        for c, f in enumerate(st):
            assert torch.equal(st_d[n, :, :, c], torch.from_numpy(_want(f, h, w))), (i, "stable", c, f)
        for c, f in enumerate(un):
            assert torch.equal(un_d[n, :, :, c], torch.from_numpy(_want(f, h, w))), (i, "unstable", c, f)
        s = samples[i]
        if len(s["flow"]):
            assert np.array_equal(batch["flow"][n].cpu().numpy(), s["flow"][:, :, :2])
        else:
            assert not batch["flow"][n].any()
        for k in ("1", "2"):
            m = s["feature_matches" + k]
            assert batch["n" + k].dtype == np.int32 and batch["n" + k][n] == len(m)
            got = batch["matches" + k][n].cpu().numpy()
            assert got.shape == (MAXM, 4) and np.array_equal(got[:len(m)], m) and not got[len(m):].any()


def test_batches_equal_the_model_on_pillows_decode(cuda, root):
    from stabnet_amd.dataset import PairDataset
    samples = _samples((H, W))
    with PairDataset(root, "train", _cfg(), H, W, batch=2, device=cuda, shuffle=False, prefetch=1, workers=4) as ds:
        for step in range(3):                                        # the third batch reuses the first slot set
            b = ds.next_batch()
            _check_batch(ds, b, [2 * step, 2 * step + 1], samples, H, W)
    # a shard of another rank, batch 3, inline
    with PairDataset(root, "train", _cfg(), H, W, batch=3, device=cuda, rank=1, world=2, shuffle=False, prefetch=0) as ds:
        _check_batch(ds, ds.next_batch(), [1, 3, 5], samples, H, W)


def test_prefetch_0_and_1_give_identical_batches(cuda, root):
    import torch
    from stabnet_amd.dataset import PairDataset
    a = PairDataset(root, "train", _cfg(), H, W, batch=2, device=cuda, seed=3, prefetch=0)
    b = PairDataset(root, "train", _cfg(), H, W, batch=2, device=cuda, seed=3, prefetch=1, workers=3)
    seen = []
    for _ in range(5):
        x, y = a.next_batch(), b.next_batch()
        for k in ("stable", "unstable", "flow", "matches1", "matches2"):
            assert torch.equal(x[k], y[k]), k
        assert np.array_equal(x["n1"], y["n1"]) and np.array_equal(x["n2"], y["n2"])
        seen.append(x["stable"].cpu())
    assert not torch.equal(seen[0], seen[1])
    a.close()
    b.close()


def test_a_422_clip_takes_the_pillow_fallback(cuda, tmp_path, capsys):
    from stabnet_amd.dataset import PairDataset, write_dataset
    d = str(tmp_path)
    _write_frames(d, subsampling=(1, 2))                             # stable clips 4:2:2 (outside the device decoder), unstable 4:2:0
    samples = _samples((H, W))
    write_dataset(d, "train", samples)
    with PairDataset(d, "train", _cfg(), H, W, batch=2, device=cuda, shuffle=False, prefetch=1) as ds:
        for step in range(2):
            _check_batch(ds, ds.next_batch(), [2 * step, 2 * step + 1], samples, H, W)
    out = capsys.readouterr().out
    assert out.count("decoded on the host with Pillow") == 1, out    # said once per geometry


def test_grey_and_missing_frames_are_errors(cuda, tmp_path):
    from PIL import Image
    from stabnet_amd._lib import StabnetError
    from stabnet_amd.dataset import PairDataset, write_dataset
    d = str(tmp_path)
    _write_frames(d)
    write_dataset(d, "train", _samples((H, W)))
    grey = os.path.join(d, "stable", "0", "33.jpg")
    Image.fromarray(_image(0, 33, 0)[:, :, 0]).save(grey, quality=90)
    with PairDataset(d, "train", _cfg(), H, W, batch=1, device=cuda, shuffle=False, prefetch=0) as ds:
        with pytest.raises(StabnetError) as e:
            ds.next_batch()
        assert grey in str(e.value) and "grey" in str(e.value)
    os.remove(grey)
    with PairDataset(d, "train", _cfg(), H, W, batch=1, device=cuda, shuffle=False, prefetch=1) as ds:
        with pytest.raises(StabnetError) as e:
            ds.next_batch()
        assert grey in str(e.value)


def test_the_batch_augments_and_trains(cuda, root):
    import torch
    from stabnet_amd import data, synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import PairDataset
    from stabnet_amd.train import Trainer, loss_gates
    N, h, w = 2, 64, 96
    cfg = Config(height=h, width=w, batch_size=N, max_matches=MAXM)
    with PairDataset(root, "big", cfg, h, w, batch=N, device=cuda, seed=1) as ds:
        raw = ds.next_batch()
    assert raw["stable"].shape == (N, h, w, 14) and not raw["flow"].any()
    para, jitter, Hs = data.draw(np.random.default_rng(0), cfg, N, h, w)
    x1, y1, x2, y2, flow, fm1, mk1, fm2, mk2 = data.augment_pairs(raw["stable"], raw["unstable"], raw["flow"], raw["matches1"], raw["n1"],
                                                                  raw["matches2"], raw["n2"], para, jitter, Hs, cfg)
    batch = {"x1": x1, "y1": y1, "x2": x2, "y2": y2, "flow": flow, "matches1": fm1, "mask1": mk1, "matches2": fm2, "mask2": mk2}
    tr = Trainer(synthetic.make_params(cfg, seed=0, theta_scale=0.2), N, h, w, cfg, device=cuda)
    tr.forward_backward(batch, loss_gates(0, cfg))
    torch.cuda.synchronize()
    loss = tr.losses()["total_loss"]
    assert np.isfinite(loss), loss
