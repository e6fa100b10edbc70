#!/usr/bin/env python3
"""stabnet_mjpeg_encode alone (csrc/mjpeg.hip): BGR 4:2:0 q75 on frames of the synthetic clip resident in HBM, 720p and 1080p.
Per launch: the Profiler's event time and the byte floor computed from the shapes (transform: read 3 H W, write 1.5 H W int16
coefficients; entropy: read them, write the intervals; gather: read and write the stream) over the HBM peak; and the restart-interval
sweep (1, 2, 4, 8, one MCU row: time and bytes per frame) from which mjpeg.DEFAULT_RESTART_MCUS is chosen.
   python tools/mjpeg_bench.py [--seconds 1.0] [--sizes 720x1280,1080x1920] [--trace]      one JSON object on stdout
--trace: a short run of the default configuration only, to be wrapped in `rocprofv3 --kernel-trace --stats -- python tools/mjpeg_bench.py --trace`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import synthetic
from stabnet_amd.deploy import Profiler
from stabnet_amd.mjpeg import DEFAULT_RESTART_MCUS, MjpegEncoder

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--sizes", default="720x1280,1080x1920")
ap.add_argument("--quality", type=int, default=75)
ap.add_argument("--subsampling", default="420")
ap.add_argument("--trace", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)


def frames(H, W, n=8):
    g = ((synthetic.make_clip(H, W, n, seed=1234) + 0.5) * 255).clip(0, 255)
    return torch.from_numpy(np.stack([g * 0.8 + 20, g, g * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)).to(dev)


def timed(enc, imgs, seconds):
    """Wall time per encode over `seconds` of back-to-back launches (one synchronisation at the end), mean stream length."""
    for i in range(20):
        enc.encode(imgs[i % len(imgs):i % len(imgs) + 1])
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for i in range(50):
            enc.encode(imgs[(n + i) % len(imgs):(n + i) % len(imgs) + 1])
        n += 50
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    size = float(np.mean([int(enc.encode(imgs[i:i + 1])[1][0].item()) for i in range(len(imgs))]))
    return 1e6 * dt / n, size, n


def per_launch(enc, imgs, size, reps=200):
    prof = Profiler(4 * reps + 16, device=dev)
    prof.calibrate()
    for i in range(reps):
        enc.encode(imgs[i % len(imgs):i % len(imgs) + 1], prof=prof)
    rows = {}
    for name, ms, _, by in prof.records():
        rows.setdefault(name, []).append((ms, by))
    out = {}
    for name, v in rows.items():
        ms = sorted(x[0] for x in v)
        by = v[0][1] + {"mjpeg_entropy_kernel": size, "mjpeg_gather_kernel": 2 * size}.get(name, 0.0)
        out[name] = {"us_median": 1e3 * ms[len(ms) // 2], "us_min": 1e3 * ms[0], "algorithmic_bytes": by,
                     "hbm_floor_us": 1e6 * by / HBM_PEAK}
    return out


out = {"device": torch.cuda.get_device_name(0), "quality": a.quality, "subsampling": a.subsampling, "default_restart_mcus": DEFAULT_RESTART_MCUS,
       "hbm_peak_bytes_per_s": HBM_PEAK, "sizes": {}}
for sz in a.sizes.split(","):
    H, W = (int(v) for v in sz.split("x"))
    imgs = frames(H, W)
    if a.trace:
        enc = MjpegEncoder(H, W, 3, quality=a.quality, subsampling=a.subsampling, device=dev)
        us, size, n = timed(enc, imgs, 0.2)
        out["sizes"][sz] = {"us_per_frame": us, "bytes_per_frame": size, "encodes": n}
        continue
    row = (W + 15) // 16
    sweep = {}
    for R in (1, 2, 4, 8, row):
        enc = MjpegEncoder(H, W, 3, quality=a.quality, subsampling=a.subsampling, restart_mcus=R, device=dev)
        reps = [timed(enc, imgs, a.seconds / 3) for _ in range(3)]
        sweep["row" if R == row else str(R)] = {"restart_mcus": R, "us_per_frame": [r[0] for r in reps], "bytes_per_frame": reps[0][1],
                                                "encodes": sum(r[2] for r in reps), "max_bytes": enc.max_bytes,
                                                "workspace_bytes": enc.workspace.numel()}
        del enc
    enc = MjpegEncoder(H, W, 3, quality=a.quality, subsampling=a.subsampling, device=dev)
    us, size, n = timed(enc, imgs, a.seconds)
    out["sizes"][sz] = {"restart_sweep": sweep, "default": {"restart_mcus": enc.restart_mcus, "us_per_frame": us, "bytes_per_frame": size,
                                                             "encodes": n, "launches": per_launch(enc, imgs, size)}}
print(json.dumps(out))
