#!/usr/bin/env python3
"""Full-frame output (stabnet_amd/mosaic.py, csrc/mosaic.hip) at the network's 288x512 beside 720p and 1080p sources.

  frame   a smooth random BGR frame remapped at its own size by maps that zoom out by 5-6 % and shift (a wide border on every side:
          an eighth of the pixels are band or uncovered), its px / py written; a canvas built by composing two such frames
  legs    the compose launch, the source-size remap of the same frame (stabnet_warp_rev_bundle2_src with px_out / py_out: its shrink
          launch and its remap launch) and a device-to-device copy moving the compose's streamed bytes ALTERNATE, --legs times each;
          every leg is --reps calls between two events each.  Medians everywhere; half an idle event pair is subtracted (Profiler).
  bar     in every leg the compose launch costs no more than the remap of the same frame
  motion  at B = 1, stage by stage: corner tracking of frame t into frame t - 1 (its kernels from the library's own events), the
          guard, the fit.  Latency, not throughput: recorded, not barred.

    python tools/mosaic_bench.py [--reps 20] [--legs 5] [--out profiles/r17_mosaic_bench.json]      one JSON object on stdout"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stabnet_amd import _lib, features, mosaic, warp
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.deploy import Profiler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--legs", type=int, default=5)
ap.add_argument("--sources", default="720x1280,1080x1920")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
H, W = 288, 512
P = mosaic.MosaicParams()


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return median([e0.elapsed_time(e1) for e0, e1 in ev])


def texture(h, w, seed, ch=None):
    g = torch.Generator(device=dev).manual_seed(seed)
    up = lambda n: torch.nn.functional.interpolate(torch.rand((1, ch or 1, h // n + 3, w // n + 3), device=dev, generator=g), size=(h, w),
                                                   mode="bilinear", align_corners=False)[0]
    t = (0.6 * up(4) + 0.4 * up(12)) * 255.0
    return t.permute(1, 2, 0).contiguous() if ch else t[0].contiguous()


def maps(zoom, dx, dy):
    """Network-size normalised maps: the identity scaled about the centre and shifted (in network pixels)."""
    x = (2.0 * torch.arange(W, dtype=torch.float64, device=dev) / W - 1.0) * zoom + 2.0 * dx / W
    y = (2.0 * torch.arange(H, dtype=torch.float64, device=dev) / H - 1.0) * zoom + 2.0 * dy / H
    return x[None, None, :].expand(1, H, W).float().contiguous(), y[None, :, None].expand(1, H, W).float().contiguous()


prof = Profiler(4096, device=dev)
prof.calibrate()
out = {"device": torch.cuda.get_device_name(0), "network_size": [H, W], "params": dataclasses.asdict(P), "reps": a.reps, "legs": a.legs,
       "idle_event_pair_us": 1e3 * prof.idle_pair_ms, "sources": {}}
st = stream_ptr(dev)

for src in a.sources.split(","):
    SH, SW = (int(v) for v in src.split("x"))
    frames = [texture(SH, SW, 7 + k, ch=3).to(torch.uint8)[None].contiguous() for k in range(2)]
    geo = [maps(1.05, 3.0, -2.0), maps(1.06, -2.0, 1.5)]
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    warped, px, py = torch.empty_like(frames[0]), torch.empty((1, SH, SW), device=dev), torch.empty((1, SH, SW), device=dev)

    def remap(k, p=0):
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(frames[k]), 1, SH, SW, 3, SW * 3, ptr(geo[k][0]), ptr(geo[k][1]), H, W, 4, ptr(warped), 0,
                  ptr(ws), ptr(px), ptr(py), st, p, device=dev)

    canvas = [torch.zeros_like(warped), torch.zeros_like(warped)]
    age = [torch.full((1, SH, SW), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
    counts = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # the motion between the two stabilised frames: a shift by 5 and -3.5 network pixels
    Hm = torch.tensor([[1, 0, 2 * 5.0 / W, 0, 1, 2 * -3.5 / H, 0, 0, 1]], dtype=torch.float32, device=dev)

    def compose(prev, cur):
        _lib.call("stabnet_mosaic_compose", ptr(warped), ptr(px), ptr(py), ptr(canvas[prev]), ptr(age[prev]), ptr(Hm), ptr(status), 1, SH, SW,
                  H, W, P.feather_log2, P.max_age, P.w_min, ptr(canvas[cur]), ptr(age[cur]), ptr(counts), st, device=dev)

    remap(0)
    compose(1, 0)                                              # the first frame: no model, fresh and empty only
    status.fill_(1)
    remap(1)
    counts.zero_()
    compose(0, 1)
    torch.cuda.synchronize()
    share = counts[0].cpu().tolist()
    streamed = SH * SW * (3 + 8 + 3 + 1)                       # warped and the two coordinates in; canvas and age out
    a_buf, b_buf = (torch.empty(streamed // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    b_buf.copy_(a_buf)
    res = {"compose_us": [], "remap_us": [], "copy_us": [], "remap_kernels_us": []}
    for _ in range(a.legs):
        res["compose_us"].append(1e3 * (timed(lambda: compose(0, 1), a.reps) - prof.overhead_ms))
        res["remap_us"].append(1e3 * (timed(lambda: remap(1), a.reps) - prof.overhead_ms))
        res["copy_us"].append(1e3 * (timed(lambda: b_buf.copy_(a_buf), a.reps) - prof.overhead_ms))
        prof.reset()
        for _ in range(a.reps):
            remap(1, prof.handle)
        by = {}
        for name, ms, _, _ in prof.records():
            by.setdefault(name, []).append(1e3 * ms)
        res["remap_kernels_us"].append({k: median(v) for k, v in by.items()})
    # where the compose's time goes: the same launch without a model (no history sample: band pixels are the frame's or empty), and
    # on coordinates that lie deep inside the frame everywhere (no band at all: the streaming path and one add per workgroup)
    status.fill_(0)
    no_model = [1e3 * (timed(lambda: compose(0, 1), a.reps) - prof.overhead_ms) for _ in range(a.legs)]
    status.fill_(1)
    keep = (px.clone(), py.clone())
    px.fill_(SW / 2.0); py.fill_(SH / 2.0)
    all_fresh = [1e3 * (timed(lambda: compose(0, 1), a.reps) - prof.overhead_ms) for _ in range(a.legs)]
    px.copy_(keep[0]); py.copy_(keep[1])
    c, r = median(res["compose_us"]), median(res["remap_us"])
    out["sources"][src] = {
        "pixels": SH * SW, "counts_fresh_blended_history_empty": share, "band_share": (share[1] + share[2] + share[3]) / float(SH * SW),
        "compose_us_medians": res["compose_us"], "compose_us": c, "remap_src_call_us_medians": res["remap_us"], "remap_src_call_us": r,
        "remap_kernels_us_by_leg": res["remap_kernels_us"],
        "compose_no_more_than_remap_in_every_leg": all(x <= y for x, y in zip(res["compose_us"], res["remap_us"])),
        "compose_without_model_us_medians": no_model, "compose_without_model_us": median(no_model),
        "compose_all_fresh_us_medians": all_fresh, "compose_all_fresh_us": median(all_fresh),
        "rows_per_workgroup": int(os.environ.get("STABNET_MOSAIC_ROWS", "2")),
        "compose_streamed_bytes": streamed, "compose_streamed_GBps": streamed / (c * 1e-6) / 1e9,
        "copy_of_the_streamed_bytes_us_medians": res["copy_us"], "copy_of_the_streamed_bytes_us": median(res["copy_us"]),
        "compose_over_copy": c / median(res["copy_us"])}
    del frames, canvas, age, warped, px, py, a_buf, b_buf

# ---- the motion leg at B = 1 ----
KP = P.klt
ny, nx = features.cells(H, W, KP)
M = ny * nx + 1
tex = texture(H + 32, W + 32, 3)
i0, i1 = tex[16:16 + H, 16:16 + W][None].contiguous(), tex[13:13 + H, 21:21 + W][None].contiguous()
black = torch.zeros((2, 1, H, W), device=dev)
for k, (l, r, t, b) in enumerate(((14, 9, 7, 12), (6, 17, 11, 5))):
    black[k, 0, :t], black[k, 0, H - b:], black[k, 0, :, :l], black[k, 0, :, W - r:] = 1, 1, 1, 1
i0, i1 = i0 * (1 - black[0]), i1 * (1 - black[1])
kws = torch.empty(features.workspace_bytes(1, H, W, KP), dtype=torch.uint8, device=dev)
rows, n = features.klt_matches(i0, i1, M, KP, workspace=kws)
g_rows, g_n = mosaic.guard_matches(rows, n, black[0], black[1], P.guard)
Hm, mask, count, status, best = (torch.empty(s, dtype=d, device=dev) for s, d in (((1, 9), torch.float32), ((1, M), torch.uint8), ((1,), torch.int32),
                                                                                  ((1,), torch.int32), ((1,), torch.int32)))


def fit():
    _lib.call("stabnet_homfit", ptr(g_rows), ptr(g_n), 1, M, H, W, P.hypotheses, P.thr_px, P.min_inliers, P.seed, P.w_min, ptr(Hm), ptr(mask),
              ptr(count), ptr(status), ptr(best), st, 0, device=dev)


fit()
torch.cuda.synchronize()
mo = {"klt_ms": [], "guard_us": [], "fit_us": [], "klt_kernels_us": []}
for _ in range(a.legs):
    mo["klt_ms"].append(timed(lambda: features.klt_matches(i0, i1, M, KP, workspace=kws), a.reps))
    mo["guard_us"].append(1e3 * (timed(lambda: mosaic.guard_matches(rows, n, black[0], black[1], P.guard, out=g_rows, out_n=g_n), a.reps) - prof.overhead_ms))
    mo["fit_us"].append(1e3 * (timed(fit, a.reps) - prof.overhead_ms))
    prof.reset()
    for _ in range(a.reps):
        features.klt_matches(i0, i1, M, KP, workspace=kws, prof=prof)
    by = {}
    for name, ms, _, _ in prof.records():
        by.setdefault(name, []).append(1e3 * ms)
    mo["klt_kernels_us"].append({k: median(v) * (len(v) // a.reps) for k, v in by.items()})
out["motion_B1"] = {"rows": int(n[0]), "rows_after_guard": int(g_n[0]), "inliers": int(count[0]), "status": int(status[0]),
                    "klt_ms_medians": mo["klt_ms"], "klt_ms": median(mo["klt_ms"]), "klt_kernels_us_by_leg": mo["klt_kernels_us"],
                    "guard_us_medians": mo["guard_us"], "guard_us": median(mo["guard_us"]), "fit_us_medians": mo["fit_us"], "fit_us": median(mo["fit_us"]),
                    "total_ms": median(mo["klt_ms"]) + 1e-3 * (median(mo["guard_us"]) + median(mo["fit_us"]))}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
