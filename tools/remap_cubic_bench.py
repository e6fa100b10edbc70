#!/usr/bin/env python3
"""The bicubic remap beside the bilinear one (csrc/remap.hip: stabnet_warp_rev_bundle2_cubic / _i420_cubic against _src / _i420), the
launches alternating on the same frames and maps resident in HBM.  Per launch the Profiler's event time beside the bytes the shapes
fix (the frame gathered once + the frame written once + the two small maps: the same for both -- the 16 taps re-read what the caches
hold) and that floor at the box's measured copy rate (tools/copy_probe.hip, profiles/r03_copy_probe.txt: 6530 GB/s).  Then the whole
loop: ClipPipeline(ingest, output='source', jpeg) on a 1080p clip -- what deploy_bundle.py --pipeline --ingest device --output-size
source --mjpg runs -- with each interp, alternating, frames per second of wall time.
   python tools/remap_cubic_bench.py [--shapes 288x512-720x1280,...] [--reps 300] [--frames 1000] [--no-pipeline]    one JSON object"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import _lib, synthetic
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.config import Config
from stabnet_amd.deploy import ClipPipeline, Profiler, StabNetStream

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="288x512-720x1280,288x512-1080x1920")
ap.add_argument("--i420", default="288x512-1080x1920")
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--shift", type=float, default=0.05, help="added to the identity maps: the share of the frame that maps outside")
ap.add_argument("--frames", type=int, default=1000, help="frames of the pipeline legs")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-pipeline", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "shift": a.shift, "shapes": {}}
med = lambda v: sorted(v)[len(v) // 2]


def maps(h, w, seed):
    """[1, h, w] x 2: the identity plus a smooth wobble and the shift (what a mild mesh gives)."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + a.shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + a.shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def us_back_to_back(fn, reps):
    for _ in range(10):
        fn(None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(None)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def measure(calls, reps):
    """calls: {name: fn(prof)}; the legs alternate call by call under one Profiler, and block by block back to back."""
    row = {}
    b2b = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            b2b[k].append(us_back_to_back(fn, reps))
    row["us_per_call_back_to_back"] = {k: med(v) for k, v in b2b.items()}
    prof = Profiler(2 * len(calls) * reps + 16, device=dev)
    prof.calibrate()
    for _ in range(reps):
        for fn in calls.values():
            fn(prof)
    rows = {}
    for name, ms, _, by in prof.records():
        rows.setdefault(name, []).append((ms, by))
    row["launches"] = {name: {"us_median": 1e3 * med([x[0] for x in v]), "us_min": 1e3 * min(x[0] for x in v), "bytes": v[0][1],
                              "copy_rate_floor_us": 1e6 * v[0][1] / COPY_RATE} for name, v in rows.items()}
    return row


for shape in a.shapes.split(","):
    (H, W), (sh, sw) = ((int(v) for v in part.split("x")) for part in shape.split("-"))
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, sh, sw, 3), dtype=np.uint8)).to(dev)
    xm, ym = maps(H, W, 2)
    o = torch.empty((1, sh, sw, 3), dtype=torch.uint8, device=dev)
    black = torch.zeros((1, sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    state = {"i": 0}

    def frame():
        state["i"] += 1
        return frames[state["i"] % 4:state["i"] % 4 + 1]

    def linear(prof):
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(frame()), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, ptr(o), ptr(black), ptr(ws), 0, 0,
                  stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)

    def cubic(prof):
        _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(frame()), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, 0, None, sh, sw, ptr(o),
                  ptr(black), ptr(ws), 0, 0, stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)

    row = measure({"linear": linear, "cubic": cubic}, a.reps)
    row["source_bytes"] = sh * sw * 3
    L = row["launches"]
    row["cubic_over_linear_event_time"] = L["remap_cubic_kernel<4, 0>"]["us_median"] / L["remap_src4_kernel"]["us_median"]
    out["shapes"][shape] = row

if a.i420:
    (H, W), (sh, sw) = ((int(v) for v in part.split("x")) for part in a.i420.split("-"))
    nb = sh * sw * 3 // 2
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, nb), dtype=np.uint8)).to(dev)
    xm, ym = maps(H, W, 2)
    o = torch.empty(nb, dtype=torch.uint8, device=dev)
    black = torch.zeros((1, sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    state = {"i": 0}

    def planar(entry):
        def call(prof):
            state["i"] += 1
            _lib.call(entry, ptr(frames[state["i"] % 4]), 1, sh, sw, 3, nb, ptr(xm), ptr(ym), H, W, 4, None, sh, sw, 16, ptr(o), ptr(black), ptr(ws),
                      stream_ptr(dev), prof.handle if prof is not None else 0, device=dev)
        return call

    row = measure({"linear": planar("stabnet_warp_rev_bundle2_i420"), "cubic": planar("stabnet_warp_rev_bundle2_i420_cubic")}, a.reps)
    L = row["launches"]
    row["cubic_over_linear_event_time"] = L["remap_i420_kernel<true>"]["us_median"] / L["remap_i420_kernel"]["us_median"]
    out["i420"] = {a.i420: row}

if not a.no_pipeline:
    from stabnet_amd.ingest import FrameIngest
    H, W, sh, sw, T = 288, 512, 1080, 1920, a.frames
    cfg = Config(height=H, width=W)
    params = synthetic.make_params(cfg, seed=0, theta_scale=0.2)
    g8 = ((synthetic.make_clip(sh, sw, 40, seed=1234).astype(np.float32) + 0.5) * 255).clip(0, 255)
    raw40 = np.ascontiguousarray(np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8))

    class Clip:                                                                   # T frames cycling through the 40 that exist
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, t):
            return raw40[t % len(raw40)]

    opts = dict(quality=75, subsampling="420")
    pipes = {k: ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, jpeg=opts,
                             ingest=FrameIngest(sh, sw, 3, H, W, device=dev), output="source", interp=k) for k in ("linear", "cubic")}
    keep = np.zeros(sh * sw * 3, np.uint8)

    def sink(r):                                                                  # the consumer touches what it was given
        keep[:len(r["jpeg"])] = r["jpeg"]

    legs = {k: {"fps": [], "host_wait_s": []} for k in pipes}
    for pipe in pipes.values():
        pipe.run(Clip(min(T, 60)), sink=sink, raw=False)                          # graph capture + warm-up
    for _ in range(a.repeats):
        for k, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.run(Clip(T), sink=sink, raw=False)
            legs[k]["fps"].append((T - 1) / (time.perf_counter() - t0))
            legs[k]["host_wait_s"].append(pipe.host_wait_s)
    for k in legs:
        legs[k]["fps_median"] = med(legs[k]["fps"])
        legs[k]["spread"] = (max(legs[k]["fps"]) - min(legs[k]["fps"])) / med(legs[k]["fps"])
    out["pipeline_1080p_mjpg"] = {"network": [H, W], "source": [sh, sw], "frames": T - 1, "legs": legs,
                                  "cubic_over_linear_fps": legs["cubic"]["fps_median"] / legs["linear"]["fps_median"]}
print(json.dumps(out))
