#!/usr/bin/env python3
"""stabnet_warp_rev_bundle2_i420 (csrc/remap.hip) beside stabnet_warp_rev_bundle2_src of a BGR frame of the same size, alternating in
one run: frames and network-size maps resident in HBM, per launch the Profiler's event time beside the bytes the shapes fix (every
plane gathered once + written once + the two small maps: 1.5 bytes per pixel each way against 3) and that floor at the box's measured
copy rate (tools/copy_probe.hip, profiles/r03_copy_probe.txt: 6530 GB/s).  A third leg, the I420 call with planes = 1, times the Y plane
alone (the chroma planes' share is the difference).  Then the whole Y4M loop of the driver (deploy_bundle.run_y4m) host to host, in
frames per second, on a generated 720p stream read from a file and written to a file.
   python tools/remap_i420_bench.py [--shapes 288x512-720x1280,...] [--reps 300] [--loop-frames 120]      one JSON object on stdout"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import _lib, y4m
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.deploy import Profiler

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="288x512-720x1280,288x512-1080x1920")
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--shift", type=float, default=0.05, help="added to the identity maps: the share of the frame that maps outside")
ap.add_argument("--loop-frames", type=int, default=120, help="frames of the generated 720p stream of the host-to-host leg (0: skip it)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "shift": a.shift, "shapes": {}}


def maps(h, w, seed):
    """[1, h, w] x 2: the identity plus a smooth wobble and the shift (what a mild mesh gives); as tools/remap_src_bench.py."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + a.shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + a.shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def stats(v):
    v = sorted(v)
    return {"us_median": 1e3 * v[len(v) // 2], "us_min": 1e3 * v[0]}


for shape in a.shapes.split(","):
    (H, W), (sh, sw) = ((int(v) for v in part.split("x")) for part in shape.split("-"))
    rng = np.random.default_rng(1)
    bgr = torch.from_numpy(rng.integers(0, 256, (4, sh, sw, 3), dtype=np.uint8)).to(dev)
    yuv = torch.from_numpy(rng.integers(0, 256, (4, sh * sw * 3 // 2), dtype=np.uint8)).to(dev)
    xm, ym = maps(H, W, 2)
    o_bgr = torch.empty((sh, sw, 3), dtype=torch.uint8, device=dev)
    o_yuv = torch.empty(sh * sw * 3 // 2, dtype=torch.uint8, device=dev)
    black = torch.zeros((sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    state = {"i": 0}

    def bgr_call(prof):
        state["i"] += 1
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(bgr[state["i"] % 4]), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), H, W, 4, ptr(o_bgr), ptr(black),
                  ptr(ws), 0, 0, stream_ptr(dev), prof.handle, device=dev)

    def i420_call(prof, planes=3):
        state["i"] += 1
        _lib.call("stabnet_warp_rev_bundle2_i420", ptr(yuv[state["i"] % 4]), 1, sh, sw, planes, sh * sw * 3 // 2, ptr(xm), ptr(ym), H, W, 4, None,
                  sh, sw, 16, ptr(o_yuv), ptr(black), ptr(ws), stream_ptr(dev), prof.handle, device=dev)

    warm = Profiler(64, device=dev)
    for _ in range(10):
        bgr_call(warm); i420_call(warm); i420_call(warm, 1)
    torch.cuda.synchronize()
    legs = {"bgr_src": [], "i420": [], "i420_y_only": []}
    byts = {}
    prof = Profiler(6 * a.reps + 16, device=dev)
    prof.calibrate()
    order = []
    for _ in range(a.reps):                                        # alternated: the legs see the same clocks and neighbours
        bgr_call(prof); i420_call(prof); i420_call(prof, 1)
        order += ["bgr_src", "i420", "i420_y_only"]
    recs = [r for r in prof.records() if r[0] != "map_shrink_kernel"]
    assert len(recs) == len(order), (len(recs), len(order))
    for leg, (name, ms, _, by) in zip(order, recs):
        legs[leg].append(ms)
        byts[leg] = (name, by)
    row = {"pixels": sh * sw, "small_map_bytes": 8 * (H // 4) * (W // 4), "black_share": float((black > 0).float().mean()), "launches": {}}
    for leg, v in legs.items():
        row["launches"][leg] = dict(stats(v), kernel=byts[leg][0], bytes=byts[leg][1], copy_rate_floor_us=1e6 * byts[leg][1] / COPY_RATE)
    row["i420_over_bgr_event_time"] = row["launches"]["i420"]["us_median"] / row["launches"]["bgr_src"]["us_median"]
    row["i420_chroma_planes_us_by_difference"] = row["launches"]["i420"]["us_median"] - row["launches"]["i420_y_only"]["us_median"]
    out["shapes"][shape] = row

if a.loop_frames > 0:
    import deploy_bundle
    sh, sw = 720, 1280
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.y4m"), os.path.join(d, "out.y4m")
        rng = np.random.default_rng(7)
        base = np.kron(rng.integers(16, 236, (sh // 16 + 4, sw // 16 + 4)), np.ones((16, 16))).astype(np.uint8)
        with y4m.Y4mWriter(src, sw, sh, (30, 1), "420mpeg2") as w:
            for t in range(a.loop_frames):
                dy, dx = 16 + int(rng.integers(-8, 9)), 16 + int(rng.integers(-8, 9))
                y = base[dy:dy + sh, dx:dx + sw]
                w.write(np.concatenate([y.reshape(-1), y[::2, ::2].reshape(-1), 255 - y[::2, ::2].reshape(-1)]))
        args = deploy_bundle.parse_args(["--y4m-in", src, "--y4m-out", dst, "--height", "288", "--width", "512"])
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):
            stream, H, W, sdev = deploy_bundle.setup_stream(args)
            walls = []
            for _ in range(3):                                     # the first run loads code objects; the median of the rest is reported
                rd = y4m.Y4mReader(src)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rep = deploy_bundle.run_y4m(args, rd, stream, H, W, sdev, dst)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
                rd.close()
        out["y4m_loop_720p"] = {"frames": rep["frames"], "network_size": [H, W], "wall_s_per_run": walls,
                                "host_to_host_frames_per_s": rep["frames"] / sorted(walls[1:])[len(walls[1:]) // 2],
                                "what": "file to file, reading, upload, ingest + network, planar warp, download, writing; each run captures its frame graph once"}
print(json.dumps(out))
