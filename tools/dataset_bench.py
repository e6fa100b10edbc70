#!/usr/bin/env python3
"""The training input alone (stabnet_amd/dataset.py, csrc/tf_image.hip): 720p JPEG frames to 288x512 training tensors.

  get_img   stabnet_tf_get_img for one batch -- 8 pairs, stable [8,288,512,14] from 96 distinct resident 720p BGR frames, then unstable
            [8,288,512,2] from 16 --: the Profiler's event median of each launch, the bytes it has to move (4 B written per value; of the
            source the 12 tap bytes per value, which at this 2.5x downscale overlap nowhere) and the time a device-to-device copy of that
            many bytes takes in the same process (the byte floor), three alternating legs each
  loader    PairDataset.next_batch() in pairs per second over a dataset written here with Pillow (two clip pairs of --frames 720p
            frames, quality 90, 4:2:0, no restart markers: the host entropy path, as ffmpeg's files take it), with prefetch 0 and 1,
            alternating; every call is followed by a device synchronise, nothing consumes the batch, so with prefetch 1 this is the
            rate of the host work alone

    python tools/dataset_bench.py [--reps 200] [--batches 12] [--workers 8] [--out profiles/r12_dataset_bench.json]     one JSON object on stdout"""
import argparse
import functools
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from stabnet_amd import tf_image
from stabnet_amd.config import Config
from stabnet_amd.dataset import PairDataset, write_dataset
from stabnet_amd.deploy import Profiler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--batches", type=int, default=12, help="timed next_batch() calls per loader leg")
ap.add_argument("--frames", type=int, default=48, help="frames per clip of the loader's dataset (at least 34)")
ap.add_argument("--workers", type=int, default=8)
ap.add_argument("--skip-loader", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
SH, SW, H, W, N = 720, 1280, 288, 512, 8
cfg = Config()


def median(v):
    return sorted(v)[len(v) // 2]


@functools.lru_cache(maxsize=None)
def frame(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SH, 0:SW]
    g = np.stack([(xx // 5 + seed) % 256, (yy // 3 + 2 * seed) % 256, ((xx + yy) // 8) % 256], axis=-1)
    return np.clip(g + rng.integers(-20, 21, (SH, SW, 3)), 0, 255).astype(np.uint8)


# ---- the get_img launches ------------------------------------------------------------------------------------------------------------
fb = SH * SW * 3
per_pair = 14                                                                  # distinct frames of a pair: 12 stable + 2 unstable
arena = torch.empty(N * per_pair * fb, dtype=torch.uint8, device=dev)
for k in range(N * per_pair):
    arena[k * fb:(k + 1) * fb] = torch.from_numpy(frame(k % 7).reshape(-1)).to(dev).roll(k * 37)
ind = cfg.indices
lags = sorted(set([1 + i for i in ind] + list(ind)))                           # frames pos - lag of the stable clip: 12 distinct
slot = {lag: j for j, lag in enumerate(lags)}
entries = {"stable": [], "unstable": []}
for n in range(N):
    base = n * per_pair
    for c, i in enumerate(ind):
        entries["stable"].append(((base + slot[1 + i]) * fb, SH, SW, 3 * SW, n, c))
        entries["stable"].append(((base + slot[i]) * fb, SH, SW, 3 * SW, n, len(ind) + c))
    for c in range(2):
        entries["unstable"].append(((base + 12 + c) * fb, SH, SW, 3 * SW, n, c))
legs = {}
for name, C in (("stable", 2 * len(ind)), ("unstable", 2)):
    table = torch.from_numpy(tf_image.make_table(entries[name], arena.numel(), N, C)).to(dev)
    dst = torch.empty((N, H, W, C), dtype=torch.float32, device=dev)
    values = N * H * W * C
    nbytes = values * (4 + 12)
    src, cp = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    legs[name] = {"table": table, "dst": dst, "C": C, "bytes": nbytes, "copy": (src, cp), "us": [], "copy_us": []}
prof = Profiler(a.reps + 16, device=dev)
prof.calibrate()
for leg in legs.values():
    tf_image.get_img(arena, leg["table"], leg["dst"], prof=prof)               # loads the code object, outside the records
    leg["copy"][1].copy_(leg["copy"][0])
torch.cuda.synchronize()
for _ in range(3):
    for leg in legs.values():
        prof.reset()
        for _ in range(a.reps):
            tf_image.get_img(arena, leg["table"], leg["dst"], prof=prof)
        leg["us"].append(1e3 * median([r[1] for r in prof.records() if r[0] == "tf_get_img_kernel"]))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            leg["copy"][1].copy_(leg["copy"][0])                               # reads bytes / 2, writes bytes / 2
            e1.record()
        torch.cuda.synchronize()
        leg["copy_us"].append(1e3 * median([e0.elapsed_time(e1) for e0, e1 in ev]) - 1e3 * prof.overhead_ms)
out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "source": [SH, SW, 3], "batch": N, "target": [H, W],
       "idle_event_pair_us": 1e3 * prof.idle_pair_ms, "get_img": {}}
for name, leg in legs.items():
    us, cu = median(leg["us"]), median(leg["copy_us"])
    out["get_img"][name] = {"C": leg["C"], "us_medians": leg["us"], "us_median_of_legs": us, "bytes": leg["bytes"],
                            "GBps": leg["bytes"] / us * 1e-3, "copy_of_the_same_bytes_us_medians": leg["copy_us"],
                            "copy_of_the_same_bytes_us": cu, "times_the_byte_floor": us / cu if cu > 0 else None}
del arena, legs

# ---- the loader ------------------------------------------------------------------------------------------------------------------
if not a.skip_loader:
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="dataset_bench_")
    try:
        t0 = time.time()
        T = max(a.frames, max(ind) + 2)
        for kind in ("stable", "unstable"):
            for clip in range(2):
                d = os.path.join(tmp, kind, str(clip))
                os.makedirs(d)
                for t in range(T):
                    Image.fromarray(np.roll(frame((t + 3 * clip) % 11), 4 * t, axis=1)).save(os.path.join(d, "%d.jpg" % t), quality=90, subsampling=2)
        samples = [{"stable_path": "stable/%d/" % c, "unstable_path": "unstable/%d/" % c, "pos": p} for c in range(2) for p in range(max(ind) + 1, T)]
        write_dataset(tmp, "train", samples)
        out["loader"] = {"frames_per_clip": T, "records": len(samples), "batches_per_leg": a.batches, "workers": a.workers,
                         "write_s": time.time() - t0, "pairs_per_s": {"prefetch0": [], "prefetch1": []}}
        sets = {p: PairDataset(tmp, "train", cfg, H, W, N, device=dev, seed=1, prefetch=p, workers=a.workers) for p in (0, 1)}
        for ds in sets.values():
            for _ in range(2):                                                 # buffers grow, code objects load
                ds.next_batch()
            torch.cuda.synchronize()
        for _ in range(3):
            for p, ds in sets.items():
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    ds.next_batch()
                    torch.cuda.synchronize()
                out["loader"]["pairs_per_s"]["prefetch%d" % p].append(a.batches * N / (time.perf_counter() - t0))
        for ds in sets.values():
            ds.close()
        for k, v in list(out["loader"]["pairs_per_s"].items()):
            out["loader"]["pairs_per_s"][k + "_median_of_legs"] = median(v)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
