#!/usr/bin/env python3
"""stabnet_ingest_grey / stabnet_ingest_colour alone (csrc/ingest.hip): BGR frames resident in HBM, per launch the Profiler's event
time beside the bytes the shapes fix (source rows read once + the 8-bit intermediate written and read + the output) and that floor at
the box's measured copy rate (tools/copy_probe.hip, profiles/r03_copy_probe.txt: 6530 GB/s, one float4 per thread, nt).
   python tools/ingest_bench.py [--shapes 720x1280-288x512,...] [--reps 300] [--trace]      one JSON object on stdout
--trace: a short run, to be wrapped in `rocprofv3 --kernel-trace --stats -- python tools/ingest_bench.py --trace`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd.deploy import Profiler
from stabnet_amd.ingest import FrameIngest

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="720x1280-288x512,1080x1920-288x512,1080x1920-720x1280,720x1280-720x1280")
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "shapes": {}}
for shape in a.shapes.split(","):
    (sh, sw), (H, W) = ((int(v) for v in part.split("x")) for part in shape.split("-"))
    ing = FrameIngest(sh, sw, 3, H, W, device=dev)
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, sh, sw, 3), dtype=np.uint8)).to(dev)
    g, c = torch.empty((1, H, W), dtype=torch.float32, device=dev), torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
    reps = 20 if a.trace else a.reps
    for i in range(10):
        ing.grey(frames[i % 4:i % 4 + 1], out=g); ing.colour(frames[i % 4:i % 4 + 1], out=c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        ing.grey(frames[i % 4:i % 4 + 1], out=g); ing.colour(frames[i % 4:i % 4 + 1], out=c)
    torch.cuda.synchronize()
    row = {"us_per_frame_back_to_back": 1e6 * (time.perf_counter() - t0) / reps, "source_bytes": sh * sw * 3,
           "taps": [ing._yk, ing._xk], "workspace_bytes": ing.workspace.numel()}
    if not a.trace:
        prof = Profiler(3 * reps + 16, device=dev)
        prof.calibrate()
        for i in range(reps):
            ing.grey(frames[i % 4:i % 4 + 1], out=g, prof=prof); ing.colour(frames[i % 4:i % 4 + 1], out=c, prof=prof)
        rows = {}
        for name, ms, _, by in prof.records():
            rows.setdefault(name, []).append((ms, by))
        row["launches"] = {name: {"us_median": 1e3 * sorted(x[0] for x in v)[len(v) // 2], "us_min": 1e3 * min(x[0] for x in v),
                                  "bytes": v[0][1], "copy_rate_floor_us": 1e6 * v[0][1] / COPY_RATE} for name, v in rows.items()}
    out["shapes"][shape] = row
print(json.dumps(out))
