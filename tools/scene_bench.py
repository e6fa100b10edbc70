#!/usr/bin/env python3
"""Scene cuts (csrc/scene.hip): what the detector and the predicated reseed cost, alone and inside the frame's graph.
  update   stabnet_scene_update (histogram + decide launch) at 288x512 and 720x1280, N = 1, timed by an event pair around the call,
           alternating with a device copy of the same H*W*4 bytes timed the same way; the idle event pair's own duration beside them.
  reseed   stabnet_ring_reseed_if with the flag 0 (every workgroup loads it and returns) and 1 (32 frame and 32 mask slots written).
  frame    StabNetStream with use_graph (operand mode 4, what the driver runs) with the feature off and on: the two streams alternate
           in one process, `--rounds` times each, `--frames` replays per round after a warm-up, host clock around replays that end in a
           synchronise.  The difference of the medians stands beside the spread of the off leg's own rounds.
  --off-only: the frame leg's off stream alone -- for a run with STABNET_LIB pointing at another build of the library (the parent's), to
           confirm that "off" is that build's path.
   python tools/scene_bench.py [--reps 300] [--frames 300] [--rounds 3] [--out profiles/rNN_scene_bench.json]     one JSON object on stdout"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from stabnet_amd import _lib, synthetic
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.config import Config
from stabnet_amd.deploy import StabNetStream

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
SIZES = [(288, 512), (720, 1280)]


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps):
    """fn() between an event pair, reps times -> {us_median, us_min}."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = [1e3 * e0.elapsed_time(e1) for e0, e1 in ev]
    return {"us_median": median(us), "us_min": min(us)}


def summary(runs):
    meds = [r["us_median"] for r in runs]
    return {"us_median_of_legs": median(meds), "us_medians": meds, "us_min": min(r["us_min"] for r in runs)}


def operator_legs(H, W):
    from stabnet_amd.scene import SceneCut
    clip = torch.from_numpy(synthetic.make_clip(H, W, 4, seed=1, margin=32)).to(dev)
    sc = SceneCut(1, H, W, device=dev)
    dst = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    depth = 32
    ring_f, ring_m = (torch.empty((1, depth, H, W), dtype=torch.float32, device=dev) for _ in range(2))
    flags = {0: torch.zeros(1, dtype=torch.int32, device=dev), 1: torch.ones(1, dtype=torch.int32, device=dev)}
    i = {"n": 0}

    def update():
        i["n"] += 1
        sc.update(clip[i["n"] % 4:i["n"] % 4 + 1])

    def copy():
        i["n"] += 1
        dst.copy_(clip[i["n"] % 4:i["n"] % 4 + 1])

    def reseed(f):
        _lib.call("stabnet_ring_reseed_if", ptr(ring_f), ptr(ring_m), ptr(clip), 1, depth, H, W, ptr(flags[f]), stream_ptr(dev), device=dev)

    legs = {"idle_event_pair": lambda: None, "update": update, "copy_same_bytes": copy, "reseed_flag_0": lambda: reseed(0),
            "reseed_flag_1": lambda: reseed(1)}
    for fn in legs.values():                                                 # loads the code objects, outside the records
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            runs[k].append(timed(fn, a.reps))
    out = {k: summary(v) for k, v in runs.items()}
    out["bytes"] = H * W * 4
    out["update_launches"] = "scene_hist_kernel (%d workgroups) + scene_decide_kernel (1)" % (4 * -(-((H + 3) // 4 * W) // 2048))
    return out


def frame_legs(H, W):
    cfg = Config(height=H, width=W)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.2)
    clip = torch.from_numpy(synthetic.make_clip(H, W, 8, seed=5, margin=32)).to(dev)
    streams = {}
    for name in (("off",) if a.off_only else ("off", "on")):
        s = StabNetStream(P, H, W, cfg, streams=1, device=dev, use_graph=True, operand_mode=4)
        s.track_black()
        if name == "on":
            s.enable_scene_cut()
        s.start(clip[0:1])
        for t in range(1, 3 + a.warmup):                                     # the eager frame, the capture, then replays
            s.step(clip[t % 8:t % 8 + 1])
        torch.cuda.synchronize()
        assert s._graph is not None, "no frame graph: the leg would time eager launches"
        streams[name] = s

    def leg(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(a.frames):
            s.step(clip[t % 8:t % 8 + 1])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.frames

    ms = {k: [] for k in streams}
    for _ in range(a.rounds):
        for k, s in streams.items():
            ms[k].append(leg(s))
    out = {k: {"ms_per_frame_median": median(v), "ms_per_frame": v} for k, v in ms.items()}
    out["off_spread_ms"] = max(ms["off"]) - min(ms["off"])
    if "on" in ms:
        out["on_minus_off_ms"] = median(ms["on"]) - median(ms["off"])
        out["on_minus_off_within_off_spread"] = abs(out["on_minus_off_ms"]) <= out["off_spread_ms"]
        seen, since = (int(v) for v in streams["on"].scene.state[0, :2].cpu())
        out["on_leg_frames_seen"], out["on_leg_frames_since_last_cut"] = seen, since      # equal: no cut was flagged, every reseed launch returned at the flag
    return out


out = {"device": torch.cuda.get_device_name(0), "library": "STABNET_LIB (another build)" if os.environ.get("STABNET_LIB") else "the tree's own", "reps": a.reps, "frames": a.frames, "rounds": a.rounds,
       "timed": {"operator": "event pair around the entry", "frame": "host clock around graph replays ending in a synchronise; one "
                 "step = a device copy of the frame into the staging buffer + one graph launch"}}
if not a.off_only:
    out["operator"] = {"%dx%d" % s: operator_legs(*s) for s in SIZES}
out["frame"] = {"%dx%d" % s: frame_legs(*s) for s in SIZES}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
