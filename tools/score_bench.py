#!/usr/bin/env python3
"""The homography fit alone (stabnet_amd/metrics.py, csrc/homfit.hip) at M = 577 rows per pair, the row count of 288x512 in cells of
16, for B = 16 and 64 pairs, beside the corner-tracking solve of the same batch that feeds it, and the whole score of a 64-frame clip.

  legs    the fit of B pairs and the KLT solve of the same B pairs ALTERNATE, --legs times each; every leg is --reps calls between
          two events each.  Medians everywhere.
  floor   a device-to-device copy of the rows' bytes (16 * M * B read, as many written), timed in the same process
  bar     the fit costs less than the KLT solve of the same batch, in every leg
  score   metrics.score_clip of a 64-frame 288x512 clip, host wall time with the readback and the host float64 part

    python tools/score_bench.py [--reps 5] [--legs 3] [--out profiles/r16_score_bench.json]      one JSON object on stdout"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stabnet_amd import features, metrics
from stabnet_amd.deploy import Profiler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
H, W = 288, 512
KP, FP = features.KltParams(), metrics.HomfitParams()
ny, nx = features.cells(H, W, KP)
M = ny * nx + 1


def median(v):
    return sorted(v)[len(v) // 2]


def pair(B):
    """A smooth random texture on the 0..255 scale and the same texture moved by a few pixels (tools/features_bench.py's)."""
    g = torch.Generator(device=dev).manual_seed(B)
    up = lambda n: torch.nn.functional.interpolate(torch.rand((B, 1, H // n + 3, W // n + 3), device=dev, generator=g),
                                                   size=(H + 16, W + 16), mode="bilinear", align_corners=False)[:, 0]
    t = (0.6 * up(4) + 0.4 * up(12)) * 255.0
    return t[:, 8:8 + H, 8:8 + W].contiguous(), t[:, 6:6 + H, 11:11 + W].contiguous()


def clip(T):
    """T frames cut from one texture along a smooth path (stable) and along the same path with a jitter of a few pixels (unstable)."""
    g = torch.Generator(device=dev).manual_seed(T)
    up = lambda n: torch.nn.functional.interpolate(torch.rand((1, 1, (H + 64) // n + 3, (W + 64) // n + 3), device=dev, generator=g),
                                                   size=(H + 64, W + 64), mode="bilinear", align_corners=False)[0, 0]
    tex = (0.6 * up(4) + 0.4 * up(12)) * 255.0
    t = torch.arange(T, dtype=torch.float64)
    sx, sy = 16 + 10 * torch.sin(2 * torch.pi * t / T), 16 + 6 * torch.cos(2 * torch.pi * t / T)
    j = torch.randint(-4, 5, (T, 2), generator=torch.Generator().manual_seed(T))
    cut = lambda x, y: tex[int(y) + 16:int(y) + 16 + H, int(x) + 16:int(x) + 16 + W]
    stable = torch.stack([cut(sx[i].round(), sy[i].round()) for i in range(T)]).contiguous()
    unstable = torch.stack([cut(sx[i].round() + j[i, 0], sy[i].round() + j[i, 1]) for i in range(T)]).contiguous()
    return unstable, stable


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return median([e0.elapsed_time(e1) for e0, e1 in ev])


prof = Profiler(64, device=dev)
prof.calibrate()
out = {"device": torch.cuda.get_device_name(0), "size": [H, W], "rows_per_pair": M, "klt": dataclasses.asdict(KP), "fit": dataclasses.asdict(FP),
       "reps": a.reps, "legs": a.legs, "idle_event_pair_us": 1e3 * prof.idle_pair_ms, "batches": {}}
for B in a.batches:
    i0, i1 = pair(B)
    ws = torch.empty(features.workspace_bytes(B, H, W, KP), dtype=torch.uint8, device=dev)
    rows, n = features.klt_matches(i0, i1, M, KP, workspace=ws)
    Hm, mask, count, status, best = metrics.homfit(rows, n, H, W, FP)             # code objects load outside the timed part
    src, dst = (torch.empty(16 * M * B, dtype=torch.uint8, device=dev) for _ in range(2))
    dst.copy_(src)
    torch.cuda.synchronize()
    res = {"fit_us": [], "klt_ms": [], "copy_us": []}
    for _ in range(a.legs):
        res["fit_us"].append(1e3 * (timed(lambda: metrics.homfit(rows, n, H, W, FP), a.reps) - prof.overhead_ms))
        res["klt_ms"].append(timed(lambda: features.klt_matches(i0, i1, M, KP, workspace=ws), a.reps))
        res["copy_us"].append(1e3 * (timed(lambda: dst.copy_(src), 20) - prof.overhead_ms))
    out["batches"]["B%d" % B] = {
        "rows_per_pair_mean": float(n.float().mean()), "rows_per_pair_min": int(n.min()), "inliers_per_pair_mean": float(count.float().mean()),
        "pairs_without_model": int((status == 0).sum()), "pairs_refit": int((status == 1).sum()),
        "fit_us_medians": res["fit_us"], "fit_us": median(res["fit_us"]), "fit_us_per_pair": median(res["fit_us"]) / B,
        "klt_ms_medians": res["klt_ms"], "klt_ms": median(res["klt_ms"]),
        "fit_cheaper_than_klt_in_every_leg": all(f * 1e-3 < k for f, k in zip(res["fit_us"], res["klt_ms"])),
        "copy_of_the_rows_us_medians": res["copy_us"], "copy_of_the_rows_us": median(res["copy_us"]), "copy_bytes": 32 * M * B}
    del ws, src, dst, i0, i1
u, s = clip(64)
metrics.score_clip(u, s)
torch.cuda.synchronize()
walls = []
for _ in range(a.legs):
    t0 = time.perf_counter()
    r = metrics.score_clip(u, s)
    walls.append(1e3 * (time.perf_counter() - t0))
out["score_64_frames"] = {"wall_ms_runs": walls, "wall_ms": median(walls),
                          "result": {k: r[k] for k in ("cropping", "distortion", "stability", "stability_translation", "stability_rotation",
                                                       "failed_pairs_unstable_stable", "failed_pairs_stable_stable", "mean_inliers")}}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
