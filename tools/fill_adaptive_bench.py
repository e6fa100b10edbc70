#!/usr/bin/env python3
"""Adaptive borderless output (csrc/remap.hip) beside the fixed window: 288x512 maps, a 1080p BGR frame, all resident in HBM.
Three legs alternate in one process, three times each, so that they see the same clocks and neighbours:
  win      stabnet_warp_rev_bundle2_win with the host window ratio_window(.., 0.8)
  win_dev  stabnet_warp_rev_bundle2_win_dev with the same four doubles in device memory (each thread then divides twice in double)
  update   stabnet_fill_window_update alone (the shrink + the one-workgroup-per-stream reduce and window update)
The remap legs report the Profiler's event median of the remap launch; win_dev passes when its median is no further from win's than
the spread of win's own three legs.  The update entry takes no profiler: its two launches are timed together by an event pair around
the call (the idle event pair's own duration is reported beside it), as a share of the 720p frame time of profiles/r04_bench_720p.json,
and once more at a 1080x1920 network size (270x480 = 129 600 nodes: one workgroup strides 127 times) beside the remap launch.
   python tools/fill_adaptive_bench.py [--reps 300] [--out profiles/r09_fill_adaptive_bench.json]     one JSON object on stdout"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from stabnet_amd import _lib
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.deploy import Profiler
from stabnet_amd.warp import ratio_window

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--ratio", type=float, default=0.8)
ap.add_argument("--shift", type=float, default=0.05, help="added to the identity maps: the share of the frame that maps outside")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
SH, SW = 1080, 1920


def maps(h, w, seed):
    """[1, h, w] x 2: the identity plus a smooth wobble and the shift (what a mild mesh gives)."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + a.shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + a.shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def median(v):
    return sorted(v)[len(v) // 2]


class Update:
    """stabnet_fill_window_update on maps of one network size, timed by an event pair around the call."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.xm, self.ym = maps(H, W, 2)
        self.ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
        self.state = torch.ones(1, dtype=torch.float64, device=dev)
        self.window = torch.zeros((1, 4), dtype=torch.float64, device=dev)
        self.stats = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        self.ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]

    def call(self):
        _lib.call("stabnet_fill_window_update", ptr(self.xm), ptr(self.ym), 1, self.H, self.W, 4, SH, SW, 0.5, 0.002, 8, ptr(self.state),
                  ptr(self.window), ptr(self.stats), ptr(self.ws), stream_ptr(dev), device=dev)

    def leg(self):
        for e0, e1 in self.ev:
            e0.record()
            self.call()
            e1.record()
        torch.cuda.synchronize()
        us = [1e3 * e0.elapsed_time(e1) for e0, e1 in self.ev]
        return {"us_median": median(us), "us_min": min(us)}


H, W = 288, 512
frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, SH, SW, 3), dtype=np.uint8)).to(dev)
xm, ym = maps(H, W, 2)
o = torch.empty((1, SH, SW, 3), dtype=torch.uint8, device=dev)
black = torch.zeros((1, SH, SW), dtype=torch.int32, device=dev)
ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
host_win = (ctypes.c_double * 4)(*ratio_window(SH, SW, a.ratio))
dev_win = torch.tensor([ratio_window(SH, SW, a.ratio)], dtype=torch.float64, device=dev)
upd = Update(H, W)
count = {"i": 0}


def remap(leg, prof, xm=xm, ym=ym, H=H, W=W, ws=ws):
    count["i"] += 1
    f = frames[count["i"] % 4:count["i"] % 4 + 1]
    entry, win = ("stabnet_warp_rev_bundle2_win", host_win) if leg == "win" else ("stabnet_warp_rev_bundle2_win_dev", ptr(dev_win))
    _lib.call(entry, ptr(f), 1, SH, SW, 3, SW * 3, ptr(xm), ptr(ym), H, W, 4, win, SH, SW, ptr(o), ptr(black), ptr(ws), 0, 0,
              stream_ptr(dev), prof.handle, device=dev)


def remap_leg(leg, prof, **kw):
    prof.reset()
    for _ in range(a.reps):
        remap(leg, prof, **kw)
    recs = [r for r in prof.records() if r[0].startswith("remap_")]
    return {"kernel": recs[0][0], "us_median": 1e3 * median([r[1] for r in recs]), "us_min": 1e3 * min(r[1] for r in recs)}


prof = Profiler(2 * a.reps + 16, device=dev)
prof.calibrate()
for leg in ("win", "win_dev"):                                              # loads the code objects, outside the records
    remap(leg, prof)
upd.call()
torch.cuda.synchronize()
legs = {"win": [], "win_dev": [], "update": []}
for _ in range(3):
    for leg in legs:
        legs[leg].append(upd.leg() if leg == "update" else remap_leg(leg, prof))
out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "ratio": a.ratio, "shift": a.shift, "maps": [H, W], "frame": [SH, SW, 3],
       "idle_event_pair_us": 1e3 * prof.idle_pair_ms, "legs": {}}
for leg, runs in legs.items():
    meds = [r["us_median"] for r in runs]
    out["legs"][leg] = dict({"us_median_of_legs": median(meds), "us_medians": meds, "us_min": min(r["us_min"] for r in runs)},
                            **({"kernel": runs[0]["kernel"]} if "kernel" in runs[0] else {"timed": "event pair around the entry: map_shrink_kernel + fill_window_kernel"}))
win, wdev, up = (out["legs"][k] for k in ("win", "win_dev", "update"))
out["win_spread_us"] = max(win["us_medians"]) - min(win["us_medians"])
out["win_dev_minus_win_us"] = wdev["us_median_of_legs"] - win["us_median_of_legs"]
out["win_dev_within_win_spread"] = abs(out["win_dev_minus_win_us"]) <= out["win_spread_us"]
try:
    frame_us = 1e3 * json.load(open(os.path.join(ROOT, "profiles", "r04_bench_720p.json")))["ms_per_step"]
    out["update_share_of_720p_frame"] = {"frame_us": frame_us, "share": up["us_median_of_legs"] / frame_us,
                                         "share_less_idle_event_pair": max(up["us_median_of_legs"] - out["idle_event_pair_us"], 0.0) / frame_us}
except (OSError, KeyError, ValueError) as e:
    out["update_share_of_720p_frame"] = "profiles/r04_bench_720p.json not readable: %s" % e

# a 1080x1920 network: 270x480 = 129 600 nodes for the one workgroup; the remap launch that follows it, at the same size, beside it
BH, BW = 1080, 1920
big = Update(BH, BW)
bxm, bym = big.xm, big.ym
big.call()
remap("win_dev", prof, xm=bxm, ym=bym, H=BH, W=BW, ws=big.ws)
torch.cuda.synchronize()
b_up, b_re = [], []
for _ in range(3):
    b_up.append(big.leg())
    b_re.append(remap_leg("win_dev", prof, xm=bxm, ym=bym, H=BH, W=BW, ws=big.ws))
out["network_1080x1920"] = {"nodes": (BH // 4) * (BW // 4),
                            "update_us_medians": [r["us_median"] for r in b_up], "update_us_median_of_legs": median([r["us_median"] for r in b_up]),
                            "remap_win_dev_us_medians": [r["us_median"] for r in b_re],
                            "remap_win_dev_us_median_of_legs": median([r["us_median"] for r in b_re])}
n = out["network_1080x1920"]
n["update_costs_more_than_the_remap_launch"] = n["update_us_median_of_legs"] - out["idle_event_pair_us"] > n["remap_win_dev_us_median_of_legs"]
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
