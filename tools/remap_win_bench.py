#!/usr/bin/env python3
"""stabnet_warp_rev_bundle2_win beside stabnet_warp_rev_bundle2_src (csrc/remap.hip): BGR frames and 288x512 maps resident in HBM.
Three legs alternate in one run, three times each, so that they see the same clocks and neighbours: _src, the window entry with the
whole-frame window (the same gather plus one double multiply per tap axis), the window entry with ratio_window(.., 0.8) (the same
output, less of the source read).  Per leg the Profiler's event median of the remap launch, the bytes the shapes fix (the part of the
frame gathered once + the output written once + the two small maps) and that floor at the box's measured copy rate
(tools/copy_probe.hip, profiles/r03_copy_probe.txt: 6530 GB/s).  The spread of _src's own three legs is the yardstick for the others.
   python tools/remap_win_bench.py [--shapes 288x512-720x1280,...] [--reps 300]      one JSON object on stdout"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import _lib
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.deploy import Profiler
from stabnet_amd.warp import ratio_window

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="288x512-720x1280,288x512-1080x1920")
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--ratio", type=float, default=0.8)
ap.add_argument("--shift", type=float, default=0.05, help="added to the identity maps: the share of the frame that maps outside")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "shift": a.shift, "ratio": a.ratio,
       "shapes": {}}


def maps(h, w, seed):
    """[1, h, w] x 2: the identity plus a smooth wobble and the shift (what a mild mesh gives)."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + a.shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + a.shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def median(v):
    return sorted(v)[len(v) // 2]


for shape in a.shapes.split(","):
    (H, W), (sh, sw) = ((int(v) for v in part.split("x")) for part in shape.split("-"))
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, sh, sw, 3), dtype=np.uint8)).to(dev)
    xm, ym = maps(H, W, 2)
    o = torch.empty((1, sh, sw, 3), dtype=torch.uint8, device=dev)
    black = torch.zeros((1, sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    windows = {"win_whole": (ctypes.c_double * 4)(0, 0, sh, sw), "win_ratio": (ctypes.c_double * 4)(*ratio_window(sh, sw, a.ratio))}
    state = {"i": 0}

    def call(leg, prof):
        state["i"] += 1
        f = frames[state["i"] % 4:state["i"] % 4 + 1]
        if leg == "src":
            _lib.call("stabnet_warp_rev_bundle2_src", ptr(f), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, ptr(o), ptr(black), ptr(ws), 0, 0,
                      stream_ptr(dev), prof.handle, device=dev)
        else:
            _lib.call("stabnet_warp_rev_bundle2_win", ptr(f), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, windows[leg], sh, sw, ptr(o),
                      ptr(black), ptr(ws), 0, 0, stream_ptr(dev), prof.handle, device=dev)

    prof = Profiler(2 * a.reps + 16, device=dev)
    prof.calibrate()
    legs = {"src": [], "win_whole": [], "win_ratio": []}
    row = {"source_bytes": sh * sw * 3, "small_map_bytes": 8 * (H // 4) * (W // 4), "legs": {}}
    for leg in legs:                                                        # loads the code objects, outside the records
        call(leg, prof)
    for _ in range(3):
        for leg in legs:
            prof.reset()
            for _ in range(a.reps):
                call(leg, prof)
            recs = [r for r in prof.records() if r[0].startswith("remap_")]
            legs[leg].append({"kernel": recs[0][0], "us_median": 1e3 * median([r[1] for r in recs]), "us_min": 1e3 * min(r[1] for r in recs),
                              "bytes": recs[0][3]})
    for leg, runs in legs.items():
        meds = [r["us_median"] for r in runs]
        row["legs"][leg] = {"kernel": runs[0]["kernel"], "us_median_of_legs": median(meds), "us_medians": meds, "us_min": min(r["us_min"] for r in runs),
                            "bytes": runs[0]["bytes"], "copy_rate_floor_us": 1e6 * runs[0]["bytes"] / COPY_RATE,
                            "share_of_copy_rate_floor": 1e6 * runs[0]["bytes"] / COPY_RATE / median(meds)}
    src = row["legs"]["src"]
    row["src_spread_us"] = max(src["us_medians"]) - min(src["us_medians"])
    row["win_whole_minus_src_us"] = row["legs"]["win_whole"]["us_median_of_legs"] - src["us_median_of_legs"]
    row["win_ratio_minus_win_whole_us"] = row["legs"]["win_ratio"]["us_median_of_legs"] - row["legs"]["win_whole"]["us_median_of_legs"]
    row["idle_event_pair_us"] = 1e3 * prof.idle_pair_ms
    out["shapes"][shape] = row
print(json.dumps(out))
