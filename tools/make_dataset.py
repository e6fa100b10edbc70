#!/usr/bin/env python3
"""Turns pairs of stable / unstable clips into a dataset folder in the reference's layout, as train_bundle_nobm.py --data-dir reads it
(stabnet_amd/dataset.py; get_data_mini_after.py:149-176):

    OUT/stable/<k>/<t>.jpg, OUT/unstable/<k>/<t>.jpg     the frames of pair k, numbered from 0 without zero padding, written with Pillow
    OUT/<split>/list.txt, OUT/<split>/<split>_00000.tfrecords ...   one record per position: the two folder prefixes (relative to
                                                          OUT), pos, an empty flow (the loader fills in zeros, as the published
                                                          data has it) and the feature matches

A clip is a uint8 .npy ([T,H,W,3] in BGR order, or [T,H,W] grey, which is written as three equal channels) or an MJPG .avi (decoded
with Pillow through stabnet_amd.avi.AviMjpegReader).  A record needs max(indices) + 1 = 33 frames of history, so positions run from
33 to T - 1.  Matches are optional: --matches K.npy with an array [T, 2, M, 4] (NaN rows = no match) gives feature_matches1 / 2 of
position t of pair k; without it both lists are empty.  No GPU is used -- unless --flow tvl1 asks for the records' flow: then,
after the frames and records are laid out, every record gets the TV-L1 flow (stabnet_amd/flow.py, csrc/tvl1.hip) from stable frame
pos - 1 to stable frame pos, computed on the GPU from the WRITTEN JPEG files through get_img's arithmetic at the network's size
(--height x --width) -- the very values a training step will see as y1 and y2 -- and stored as the map [H,W,2] that interpolate()
reads.  The default --flow none writes the records with an empty flow, as before.

    python tools/make_dataset.py --out data --split train --pair stable0.npy unstable0.npy --pair stable1.avi unstable1.avi
    python tools/make_dataset.py --out data --split train --pair stable0.npy unstable0.npy --flow tvl1 --flow-batch 8
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def read_clip(path):
    """-> iterator of uint8 [H,W,3] RGB frames."""
    if path.lower().endswith(".npy"):
        clip = np.load(path, mmap_mode="r")
        if clip.dtype != np.uint8 or clip.ndim not in (3, 4) or (clip.ndim == 4 and clip.shape[3] != 3):
            raise SystemExit("make_dataset.py: %s: expected uint8 [T,H,W,3] (BGR) or [T,H,W] (grey), got %s %s" % (path, clip.dtype, clip.shape))
        for f in clip:
            f = np.asarray(f)
            yield np.repeat(f[:, :, None], 3, axis=2) if f.ndim == 2 else f[:, :, ::-1]
    elif path.lower().endswith(".avi"):
        from stabnet_amd.avi import AviMjpegReader
        for f in AviMjpegReader(path).frames():
            yield np.repeat(f[:, :, None], 3, axis=2) if f.ndim == 2 else f[:, :, ::-1]
    else:
        raise SystemExit("make_dataset.py: %s: only .npy clips and MJPG .avi files are read" % path)


def write_clip(path, folder, quality):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    n = 0
    for n, f in enumerate(read_clip(path), 1):
        Image.fromarray(np.ascontiguousarray(f)).save(os.path.join(folder, "%d.jpg" % (n - 1)), quality=quality, subsampling=2)    # 4:2:0
    return n


def tvl1_flows(out, split, H, W, batch, count):
    """The TV-L1 map [H,W,2] of records 0 .. count - 1 of the dataset just written, in order: PairDataset decodes stable frames
    pos - 1 and pos from the written files and runs get_img, so the flow belongs to exactly what training reads."""
    import dataclasses
    from stabnet_amd import flow
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import PairDataset
    cfg = dataclasses.replace(Config(), indices=(0,))            # stable [N,H,W,2] = frames pos - 1, pos: nothing else is decoded
    maps = []
    with PairDataset(out, split, cfg, H, W, batch, shuffle=False, prefetch=0) as ds:
        while len(maps) < count:
            stable = ds.next_batch()["stable"]                  # (the last batch wraps round to the first records: ignored)
            m = flow.tvl1_flow(stable[..., 0], stable[..., 1], out="map", offset=0.5, scale=255.0)
            maps.extend(m.cpu().numpy())
    return maps[:count]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="the data_dir to write")
    ap.add_argument("--split", default="train", help="train or test (the folder that holds list.txt and the record files)")
    ap.add_argument("--pair", nargs=2, action="append", required=True, metavar=("STABLE", "UNSTABLE"), help="one clip pair; repeat")
    ap.add_argument("--matches", action="append", default=None, help="one .npy [T,2,M,4] per --pair, in order (optional)")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--records-per-file", type=int, default=10)
    ap.add_argument("--flow", default="none", choices=["none", "tvl1"], help="none: every record's flow is empty; tvl1: computed on the GPU")
    ap.add_argument("--flow-batch", type=int, default=8, help="--flow tvl1: pairs per solve")
    ap.add_argument("--height", type=int, default=None, help="--flow tvl1: the network's input height (default: the configuration's)")
    ap.add_argument("--width", type=int, default=None, help="--flow tvl1: the network's input width")
    a = ap.parse_args()
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import write_dataset
    if a.matches is not None and len(a.matches) != len(a.pair):
        raise SystemExit("make_dataset.py: %d --matches for %d --pair" % (len(a.matches), len(a.pair)))
    first = max(Config().indices) + 1
    samples = []
    for k, (stable, unstable) in enumerate(a.pair):
        counts = [write_clip(p, os.path.join(a.out, kind, str(k)), a.quality) for kind, p in (("stable", stable), ("unstable", unstable))]
        T = min(counts)
        if T <= first:
            raise SystemExit("make_dataset.py: pair %d has %d frames; a record needs %d frames of history" % (k, T, first))
        m = np.load(a.matches[k]) if a.matches is not None else None
        if m is not None and (m.ndim != 4 or m.shape[0] < T or m.shape[1] != 2 or m.shape[3] != 4):
            raise SystemExit("make_dataset.py: %s: expected [T >= %d, 2, M, 4], got %s" % (a.matches[k], T, m.shape))
        for pos in range(first, T):
            s = {"stable_path": "stable/%d/" % k, "unstable_path": "unstable/%d/" % k, "pos": pos}
            if m is not None:
                for j, key in enumerate(("feature_matches1", "feature_matches2")):
                    rows = np.asarray(m[pos, j], np.float32)
                    s[key] = rows[~np.isnan(rows).any(axis=1)]
            samples.append(s)
        print("pair %d: %d + %d frames, positions %d..%d" % (k, counts[0], counts[1], first, T - 1))
    names = write_dataset(a.out, a.split, samples, records_per_file=a.records_per_file)
    if a.flow == "tvl1":
        if a.flow_batch < 1:
            raise SystemExit("make_dataset.py: --flow-batch must be at least 1, got %d" % a.flow_batch)
        H, W = a.height or Config().height, a.width or Config().width
        for s, m in zip(samples, tvl1_flows(a.out, a.split, H, W, a.flow_batch, len(samples))):
            s["flow"] = m
        names = write_dataset(a.out, a.split, samples, records_per_file=a.records_per_file)
        print("flow: TV-L1 at %dx%d for %d records" % (W, H, len(samples)))
    print("%s: %d records in %d file(s)" % (os.path.join(a.out, a.split, "list.txt"), len(samples), len(names)))


if __name__ == "__main__":
    main()
