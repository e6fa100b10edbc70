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
reads.  The default --flow none writes the records with an empty flow, as before.  --features klt fills feature_matches1 / 2 in
the same way (stabnet_amd/features.py, csrc/klt.hip): corners of stable frame pos - 1 tracked into unstable frame pos - 1, and
those of stable frame pos into unstable frame pos, from the written files at --height x --width; it cannot be combined with
--matches.  With both --flow tvl1 and --features klt the dataset is read back once.

    python tools/make_dataset.py --out data --split train --pair stable0.npy unstable0.npy --pair stable1.avi unstable1.avi
    python tools/make_dataset.py --out data --split train --pair stable0.npy unstable0.npy --flow tvl1 --flow-batch 8
    python tools/make_dataset.py --out data --split train --pair stable0.npy unstable0.npy --features klt --height 288 --width 512
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


def read_back(out, split, H, W, batch, count, want_flow, want_features):
    """-> (maps, matches) of records 0 .. count - 1 of the dataset just written, in order (either None when not wanted): the TV-L1
    map [H,W,2] and the two match lists ([n,4] each).  PairDataset decodes frames pos - 1 and pos of both clips from the written
    files and runs get_img, so both belong to exactly what training reads."""
    import dataclasses
    from stabnet_amd import features, flow
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import PairDataset
    cfg = dataclasses.replace(Config(), indices=(0,))            # stable [N,H,W,2] = frames pos - 1, pos: nothing else is decoded
    maps, lists = [], []
    with PairDataset(out, split, cfg, H, W, batch, shuffle=False, prefetch=0) as ds:
        for _ in range(0, count, batch):                         # (the last batch wraps round to the first records: ignored)
            b = ds.next_batch()
            stable, unstable = b["stable"], b["unstable"]
            if want_flow:
                maps.extend(flow.tvl1_flow(stable[..., 0], stable[..., 1], out="map", offset=0.5, scale=255.0).cpu().numpy())
            if want_features:
                both = []
                for c in (0, 1):
                    m, n = features.klt_matches(stable[..., c], unstable[..., c], cfg.max_matches, offset=0.5, scale=255.0)
                    m, n = m.cpu().numpy(), n.cpu().numpy()
                    both.append([m[i, :n[i]] for i in range(len(n))])
                lists.extend(zip(*both))
    return (maps[:count] if want_flow else None), (lists[:count] if want_features else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="the data_dir to write")
    ap.add_argument("--split", default="train", help="train or test (the folder that holds list.txt and the record files)")
    ap.add_argument("--pair", nargs=2, action="append", required=True, metavar=("STABLE", "UNSTABLE"), help="one clip pair; repeat")
    ap.add_argument("--matches", action="append", default=None, help="one .npy [T,2,M,4] per --pair, in order (optional)")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--records-per-file", type=int, default=10)
    ap.add_argument("--flow", default="none", choices=["none", "tvl1"], help="none: every record's flow is empty; tvl1: computed on the GPU")
    ap.add_argument("--features", default="none", choices=["none", "klt"],
                    help="none: the feature matches are those of --matches, or empty; klt: corners tracked on the GPU")
    ap.add_argument("--flow-batch", type=int, default=8, help="--flow tvl1 / --features klt: records per solve")
    ap.add_argument("--height", type=int, default=None, help="--flow tvl1 / --features klt: the network's input height (default: the configuration's)")
    ap.add_argument("--width", type=int, default=None, help="--flow tvl1 / --features klt: the network's input width")
    a = ap.parse_args()
    from stabnet_amd.config import Config
    from stabnet_amd.dataset import write_dataset
    if a.matches is not None and len(a.matches) != len(a.pair):
        raise SystemExit("make_dataset.py: %d --matches for %d --pair" % (len(a.matches), len(a.pair)))
    if a.features == "klt" and a.matches is not None:
        raise SystemExit("make_dataset.py: --features klt computes the feature matches; it cannot be combined with --matches")
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
    if a.flow == "tvl1" or a.features == "klt":
        if a.flow_batch < 1:
            raise SystemExit("make_dataset.py: --flow-batch must be at least 1, got %d" % a.flow_batch)
        H, W = a.height or Config().height, a.width or Config().width
        maps, lists = read_back(a.out, a.split, H, W, a.flow_batch, len(samples), a.flow == "tvl1", a.features == "klt")
        for i, s in enumerate(samples):
            if maps is not None:
                s["flow"] = maps[i]
            if lists is not None:
                s["feature_matches1"], s["feature_matches2"] = lists[i]
        names = write_dataset(a.out, a.split, samples, records_per_file=a.records_per_file)
        if maps is not None:
            print("flow: TV-L1 at %dx%d for %d records" % (W, H, len(samples)))
        if lists is not None:
            print("features: KLT at %dx%d for %d records, %d matches" % (W, H, len(samples), sum(len(m) for l in lists for m in l)))
    print("%s: %d records in %d file(s)" % (os.path.join(a.out, a.split, "list.txt"), len(samples), len(names)))


if __name__ == "__main__":
    main()
