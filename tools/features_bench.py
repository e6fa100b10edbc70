#!/usr/bin/env python3
"""Corner tracking alone (stabnet_amd/features.py, csrc/klt.hip) at the training size 288x512: B = 16 image pairs (one batch of 8
records, both towers) and B = 64, beside the fused TV-L1 solve of 8 records that the loader already pays for.

  legs      the match of B pairs and the TV-L1 solve of 8 pairs ALTERNATE, --legs times each; every leg is --reps solves with the
            Profiler's event records and --reps without (the whole solve between two events).  Medians everywhere.
  stages    per kernel: launches per solve and the sum of their event times per solve -- detection, the pyramids and gradients
            (TV-L1's kernels), tracking, finish
  floor     a device-to-device copy that reads one image batch and writes one (the two images' bytes), timed in the same
            process: what detection, which reads i0 once, cannot beat by much
  bar       the match of B = 16 against the TV-L1 solve of 8 pairs, leg by leg

    python tools/features_bench.py [--reps 5] [--legs 3] [--out profiles/r15_features_bench.json]      one JSON object on stdout"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stabnet_amd import features, flow
from stabnet_amd.deploy import Profiler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
ap.add_argument("--max-matches", type=int, default=3000)
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
H, W = 288, 512
P = features.KltParams()
STAGE = {"klt_detect_kernel": "detect", "tvl1_down_kernel": "pyramids_and_gradients", "tvl1_grad_kernel": "pyramids_and_gradients",
         "klt_track_kernel": "track", "klt_finish_kernel": "finish"}


def median(v):
    return sorted(v)[len(v) // 2]


def pair(B):
    """A smooth random texture on the 0..255 scale and the same texture moved by a few pixels."""
    g = torch.Generator(device=dev).manual_seed(B)
    up = lambda n: torch.nn.functional.interpolate(torch.rand((B, 1, H // n + 3, W // n + 3), device=dev, generator=g),
                                                   size=(H + 16, W + 16), mode="bilinear", align_corners=False)[:, 0]
    t = (0.6 * up(4) + 0.4 * up(12)) * 255.0
    return t[:, 8:8 + H, 8:8 + W].contiguous(), t[:, 6:6 + H, 11:11 + W].contiguous()


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return median([e0.elapsed_time(e1) for e0, e1 in ev])


prof = Profiler(8192, device=dev)
prof.calibrate()
out = {"device": torch.cuda.get_device_name(0), "size": [H, W], "params": dataclasses.asdict(P), "cells": list(features.cells(H, W, P)),
       "max_matches": a.max_matches, "reps": a.reps, "legs": a.legs, "idle_event_pair_us": 1e3 * prof.idle_pair_ms, "batches": {}}
f0, f1 = pair(8)
fws = torch.empty(flow.workspace_bytes(8, H, W), dtype=torch.uint8, device=dev)
os.environ.pop("STABNET_TVL1_FUSED", None)
flow.tvl1_flow(f0, f1, out="map", workspace=fws)                             # code objects load outside the records
for B in a.batches:
    i0, i1 = pair(B)
    ws = torch.empty(features.workspace_bytes(B, H, W, P), dtype=torch.uint8, device=dev)
    src, dst = (torch.empty(4 * B * H * W, dtype=torch.uint8, device=dev) for _ in range(2))
    rows, n = features.klt_matches(i0, i1, a.max_matches, P, workspace=ws)
    dst.copy_(src)
    torch.cuda.synchronize()
    res = {"match_ms": [], "tvl1_8_pairs_ms": [], "stages": [], "copy_us": []}
    for _ in range(a.legs):
        prof.reset()
        for _ in range(a.reps):
            features.klt_matches(i0, i1, a.max_matches, P, workspace=ws, prof=prof)
        stages = {}
        for name, ms, _, nbytes, shape in prof.records_with_shapes():
            s = stages.setdefault(STAGE.get(name, name), [0, 0.0])
            s[0] += 1
            s[1] += ms
        res["stages"].append({k: {"launches_per_solve": v[0] / a.reps, "ms_per_solve": v[1] / a.reps} for k, v in stages.items()})
        res["match_ms"].append(timed(lambda: features.klt_matches(i0, i1, a.max_matches, P, workspace=ws), a.reps))
        res["tvl1_8_pairs_ms"].append(timed(lambda: flow.tvl1_flow(f0, f1, out="map", workspace=fws), a.reps))
        res["copy_us"].append(1e3 * timed(lambda: dst.copy_(src), 20) - 1e3 * prof.overhead_ms)
    mid = res["stages"][len(res["stages"]) // 2]
    ms, tv = median(res["match_ms"]), median(res["tvl1_8_pairs_ms"])
    out["batches"]["B%d" % B] = {
        "matches_per_pair_mean": float(n.float().mean()), "matches_per_pair_min": int(n.min()),
        "match_ms_medians": res["match_ms"], "match_ms": ms, "ms_per_pair": ms / B,
        "tvl1_fused_8_pairs_ms_medians": res["tvl1_8_pairs_ms"], "tvl1_fused_8_pairs_ms": tv,
        "match_faster_than_tvl1_of_8_pairs_in_every_leg": all(m < t for m, t in zip(res["match_ms"], res["tvl1_8_pairs_ms"])),
        "stages": mid, "stage_sum_ms": sum(v["ms_per_solve"] for v in mid.values()),
        "copy_of_two_image_batches_us_medians": res["copy_us"], "copy_of_two_image_batches_us": median(res["copy_us"]),
        "copy_bytes": 8 * B * H * W}
    del ws, src, dst, i0, i1
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
