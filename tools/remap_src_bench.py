#!/usr/bin/env python3
"""stabnet_warp_rev_bundle2_src alone (csrc/remap.hip): BGR frames and network-size maps resident in HBM, per launch the Profiler's
event time beside the bytes the shapes fix (the frame gathered once + the frame written once + the two small maps) and that floor at
the box's measured copy rate (tools/copy_probe.hip, profiles/r03_copy_probe.txt: 6530 GB/s, one float4 per thread, nt).  In the same
run, alternating with it, stabnet_warp_rev_bundle2 at H, W = SH, SW: the same per-pixel work on maps as large as the frame.
   python tools/remap_src_bench.py [--shapes 288x512-720x1280,...] [--reps 300] [--trace]      one JSON object on stdout
--trace: a short run, to be wrapped in `rocprofv3 --kernel-trace --stats -- python tools/remap_src_bench.py --trace`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import warp
from stabnet_amd.deploy import Profiler

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="288x512-720x1280,288x512-1080x1920")
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--shift", type=float, default=0.05, help="added to the identity maps: the share of the frame that maps outside")
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "shift": a.shift, "shapes": {}}


def maps(h, w, seed):
    """[1, h, w] x 2: the identity plus a smooth wobble and the shift (what a mild mesh gives)."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + a.shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + a.shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def us(fn, reps):
    for _ in range(10):
        fn(None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(None)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


for shape in a.shapes.split(","):
    (H, W), (sh, sw) = ((int(v) for v in part.split("x")) for part in shape.split("-"))
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, sh, sw, 3), dtype=np.uint8)).to(dev)
    xm, ym = maps(H, W, 2)
    xl, yl = maps(sh, sw, 2)                                                # the unchanged entry: maps at the frame's own size
    o = torch.empty((1, sh, sw, 3), dtype=torch.uint8, device=dev)
    black = torch.zeros((1, sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (sh // 4) * (sw // 4), dtype=torch.float32, device=dev)
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    state = {"i": 0}

    def src_call(prof, count=True):
        state["i"] += 1
        f = frames[state["i"] % 4:state["i"] % 4 + 1]
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(f), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, ptr(o), ptr(black) if count else 0,
                  ptr(ws), 0, 0, stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)

    def old_call(_):
        state["i"] += 1
        f = frames[state["i"] % 4:state["i"] % 4 + 1]
        _lib.call("stabnet_warp_rev_bundle2", ptr(f), ptr(xl), ptr(yl), 1, sh, sw, 3, 4, ptr(o), ptr(ws), 0, 0, stream_ptr(dev), device=dev)

    reps = 20 if a.trace else a.reps
    row = {"source_bytes": sh * sw * 3, "small_map_bytes": 8 * (H // 4) * (W // 4)}
    b2b = {"src_entry": [], "src_entry_no_count": [], "rev_bundle2_at_source_size": []}
    for _ in range(1 if a.trace else 3):                                    # alternated: the legs see the same clocks and neighbours
        b2b["src_entry"].append(us(src_call, reps))
        b2b["rev_bundle2_at_source_size"].append(us(old_call, reps))
        b2b["src_entry_no_count"].append(us(lambda p: src_call(p, False), reps))
    row["us_per_call_back_to_back"] = {k: sorted(v)[len(v) // 2] for k, v in b2b.items()}
    row["black_share"] = float((black[0] > 0).float().mean())
    if not a.trace:
        # event time of the unchanged entry (it takes no profiler): events around each call on the stream
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        prof = Profiler(2 * reps + 16, device=dev)
        prof.calibrate()
        for e0, e1 in evs:
            src_call(prof)
            e0.record(); old_call(None); e1.record()
        rows = {}
        for name, ms, _, by in prof.records():
            rows.setdefault(name, []).append((ms, by))
        row["launches"] = {name: {"us_median": 1e3 * sorted(x[0] for x in v)[len(v) // 2], "us_min": 1e3 * min(x[0] for x in v),
                                  "bytes": v[0][1], "copy_rate_floor_us": 1e6 * v[0][1] / COPY_RATE} for name, v in rows.items()}
        k = "remap_src4_kernel" if "remap_src4_kernel" in row["launches"] else "remap_src_kernel"
        row["share_of_copy_rate_floor"] = row["launches"][k]["copy_rate_floor_us"] / row["launches"][k]["us_median"]
        old = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
        row["rev_bundle2_at_source_size_event_us"] = {"median_two_launches_raw": 1e3 * old[len(old) // 2], "min": 1e3 * old[0],
                                                      "idle_event_pair_us": 1e3 * prof.idle_pair_ms}
    out["shapes"][shape] = row
print(json.dumps(out))
