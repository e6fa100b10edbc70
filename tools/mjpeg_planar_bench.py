#!/usr/bin/env python3
"""The planar (YCbCr) Motion-JPEG route beside the BGR route, alternating in one process, at 720p and 1080p sources (network 288x512):
  decode   the decoder's last launch: mjpegd_planes_kernel (stabnet_mjpeg_decode_i420) against mjpegd_colour_kernel (stabnet_mjpeg_decode,
           stages 3).  The BGR entry has no profiler, so all three calls -- stages 2 (entropy + IDCT, shared), BGR, I420 -- are timed
           with device events around the call, and the last launch is the difference to the stages-2 call; the planes launch's own
           Profiler record is given beside it
  remap    stabnet_warp_rev_bundle2_i420 against stabnet_warp_rev_bundle2_src on BGR (Profiler records, as tools/remap_i420_bench.py)
  encode   the transform launch: mjpeg_transform_planar_kernel against mjpeg_transform_kernel (Profiler records)
  chain    the whole per-frame chain host to host: deploy_bundle.py --avi-in A --avi-out B beside the test-list route (--ingest device
           --decode device --output-size source --mjpg) on the same clip, each as a process of its own on a clip of N and of 2 N frames:
           seconds per frame = (wall(2 N) - wall(N)) / N, which leaves start-up, graph capture and the files' headers out
Bytes are the algorithm's, from the shapes: colour 1.5 read + 3 written per pixel, planes 1.5 + 1.5; remap 3 + 3 against 1.5 + 1.5 (+ the
small maps); transform 3 (1.5) read + the coefficients (3 bytes per pixel of 4:2:0) written.
   python tools/mjpeg_planar_bench.py [--sizes 720x1280,1080x1920] [--reps 200] [--chain-frames 100] > profiles/r22_mjpeg_planar_bench.json"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from stabnet_amd import _lib
from stabnet_amd._tensor import ptr, stream_ptr
from stabnet_amd.avi import AviMjpegWriter
from stabnet_amd.deploy import Profiler
from stabnet_amd.mjpeg import MjpegDecoder, MjpegEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="720x1280,1080x1920")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--chain-frames", type=int, default=100, help="N of the host-to-host leg (0: skip it)")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU: there is nothing to report without one"
dev = torch.device("cuda", 0)
NH, NW = 288, 512
out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "network_size": [NH, NW], "sizes": {}}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def picture(sh, sw, seed):
    rng = np.random.default_rng(seed)
    base = np.kron(rng.integers(16, 236, (sh // 16 + 4, sw // 16 + 4, 3)), np.ones((16, 16, 1)))
    return base, rng


def frames_bgr(sh, sw, n, seed=7):
    """n shaky BGR frames of a blocky picture with mild noise (so that the streams are of a usual length)."""
    base, rng = picture(sh, sw, seed)
    for _ in range(n):
        dy, dx = 16 + int(rng.integers(-8, 9)), 16 + int(rng.integers(-8, 9))
        f = base[dy:dy + sh, dx:dx + sw] + rng.normal(0, 3.0, (sh, sw, 3))
        yield np.clip(np.rint(f), 0, 255).astype(np.uint8)


def maps(h, w, seed, shift=0.05):
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(w) / w - 1.0)[None, :] + 0.02 * np.sin(np.arange(h) / h * 6.0 + rng.uniform(0, 3))[:, None] + shift
    y = (2.0 * np.arange(h) / h - 1.0)[:, None] + 0.02 * np.cos(np.arange(w) / w * 5.0 + rng.uniform(0, 3))[None, :] + shift
    return (torch.from_numpy(np.broadcast_to(v, (h, w)).astype(np.float32)[None].copy()).to(dev) for v in (x, y))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


for size in a.sizes.split(","):
    sh, sw = (int(v) for v in size.split("x"))
    px = sh * sw
    row = {"pixels": px}
    enc_bgr = MjpegEncoder(sh, sw, 3, quality=75, device=dev)
    enc_pl = MjpegEncoder(sh, sw, 3, quality=75, device=dev, planar=True)
    src = [torch.from_numpy(f).to(dev) for f in frames_bgr(sh, sw, 4)]
    jpegs = [enc_bgr.encode_bytes(f)[0] for f in src]

    # ---- decode: stages 2 | BGR | I420, device events around each call, alternating ------------------------------------------------------
    d_bgr = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4)
    d_pl = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4, planar=True)
    for d in (d_bgr, d_pl):
        for k, j in enumerate(jpegs):
            used = d.stage(j, d.h_in[k])
            d.d_in[k, :used].copy_(d.h_in[k, :used])
    torch.cuda.synchronize()
    calls = {"stages2": lambda k: d_bgr.enqueue(d_bgr.d_in[k:k + 1], 1, None, d_bgr.status[:1], stages=2),
             "bgr": lambda k: d_bgr.enqueue(d_bgr.d_in[k:k + 1], 1, d_bgr.out[:1], d_bgr.status[:1]),
             "i420": lambda k: d_pl.enqueue(d_pl.d_in[k:k + 1], 1, d_pl.out[:1], d_pl.status[:1])}
    for k in range(12):
        for c in calls.values():
            c(k % 4)
    torch.cuda.synchronize()
    evs = {n: [] for n in calls}
    for i in range(a.reps):
        for n, c in calls.items():
            evs[n].append(event_ms(lambda: c(i % 4)))
    torch.cuda.synchronize()
    t = {n: med([e0.elapsed_time(e1) for e0, e1 in v]) for n, v in evs.items()}
    prof = Profiler(2 * a.reps + 16, device=dev)
    prof.calibrate()
    for i in range(a.reps):
        d_pl.enqueue(d_pl.d_in[i % 4:i % 4 + 1], 1, d_pl.out[:1], d_pl.status[:1], prof=prof)
    planes_rec = [r[1] for r in prof.records() if r[0] == "mjpegd_planes_kernel"]
    assert len(planes_rec) == a.reps and not int(d_pl.status[0]) and not int(d_bgr.status[0])
    row["decode"] = {"call_us_median": {n: 1e3 * v for n, v in t.items()},
                     "last_launch_us_by_difference": {"colour": 1e3 * (t["bgr"] - t["stages2"]), "planes": 1e3 * (t["i420"] - t["stages2"])},
                     "planes_kernel_profiler_us_median": 1e3 * med(planes_rec),
                     "bytes": {"colour": 4.5 * px, "planes": 3.0 * px}, "stream_bytes": len(jpegs[0])}

    # ---- remap: _src on BGR | _i420, Profiler records, alternating -----------------------------------------------------------------------
    planes4 = torch.stack([d_pl.decode([j])[0].clone() for j in jpegs])
    xm, ym = maps(NH, NW, 2)
    o_bgr = torch.empty((sh, sw, 3), dtype=torch.uint8, device=dev)
    o_yuv = torch.empty(px * 3 // 2, dtype=torch.uint8, device=dev)
    black = torch.zeros((sh, sw), dtype=torch.int32, device=dev)
    ws = torch.empty(2 * (NH // 4) * (NW // 4), dtype=torch.float32, device=dev)

    def remap_bgr(p, k):
        _lib.call("stabnet_warp_rev_bundle2_src", ptr(src[k]), 1, sh, sw, 3, sw * 3, ptr(xm), ptr(ym), NH, NW, 4, ptr(o_bgr), ptr(black), ptr(ws), 0, 0,
                  stream_ptr(dev), p.handle, device=dev)

    def remap_i420(p, k):
        _lib.call("stabnet_warp_rev_bundle2_i420", ptr(planes4[k]), 1, sh, sw, 3, px * 3 // 2, ptr(xm), ptr(ym), NH, NW, 4, None, sh, sw, 0, ptr(o_yuv),
                  ptr(black), ptr(ws), stream_ptr(dev), p.handle, device=dev)

    def enc_call(enc, frame, p):
        enc.encode(frame, prof=p)

    warm = Profiler(512, device=dev)
    for k in range(8):
        remap_bgr(warm, k % 4); remap_i420(warm, k % 4)
        enc_call(enc_bgr, src[k % 4], warm); enc_call(enc_pl, planes4[k % 4:k % 4 + 1], warm)
    torch.cuda.synchronize()
    prof = Profiler(12 * a.reps + 16, device=dev)
    prof.calibrate()
    for i in range(a.reps):
        k = i % 4
        remap_bgr(prof, k); remap_i420(prof, k)
        enc_call(enc_bgr, src[k], prof); enc_call(enc_pl, planes4[k:k + 1], prof)
    by_name = {}
    for name, ms, _, by in prof.records():
        by_name.setdefault(name, ([], by))[0].append(ms)
    pick = lambda name: {"kernel": name, "us_median": 1e3 * med(by_name[name][0]), "us_min": 1e3 * min(by_name[name][0]), "bytes": by_name[name][1],
                         "launches": len(by_name[name][0])}
    remap_names = [n for n in by_name if n.startswith("remap_src")]
    assert len(remap_names) == 1, remap_names
    row["remap"] = {"bgr_src": pick(remap_names[0]), "i420": pick("remap_i420_kernel")}
    row["encode_transform"] = {"bgr": pick("mjpeg_transform_kernel"), "planar": pick("mjpeg_transform_planar_kernel")}
    row["ratios_planar_over_bgr"] = {
        "decode_last_launch_time": row["decode"]["last_launch_us_by_difference"]["planes"] / row["decode"]["last_launch_us_by_difference"]["colour"],
        "decode_last_launch_bytes": 3.0 / 4.5,
        "remap_time": row["remap"]["i420"]["us_median"] / row["remap"]["bgr_src"]["us_median"],
        "remap_bytes": row["remap"]["i420"]["bytes"] / row["remap"]["bgr_src"]["bytes"],
        "transform_time": row["encode_transform"]["planar"]["us_median"] / row["encode_transform"]["bgr"]["us_median"],
        "transform_bytes": row["encode_transform"]["planar"]["bytes"] / row["encode_transform"]["bgr"]["bytes"]}

    # ---- the whole chain, host to host: two processes per route, N and 2 N frames -------------------------------------------------------
    if a.chain_frames > 0:
        N = a.chain_frames
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "unstable"))
            walls = {}
            for n in (N, 2 * N):
                name = "clip%d.avi" % n
                with AviMjpegWriter(os.path.join(d, "unstable", name), sw, sh, 30) as w:
                    for f in frames_bgr(sh, sw, n, seed=11):
                        w.write(enc_bgr.encode_bytes(torch.from_numpy(f).to(dev))[0])
                open(os.path.join(d, "list%d" % n), "w").write(name + "\n")
                routes = {"planar": ["--avi-in", os.path.join(d, "unstable", name), "--avi-out", os.path.join(d, "planar%d.avi" % n)],
                          "bgr_test_list": ["--test-list", os.path.join(d, "list%d" % n), "--prefix", d, "--output-dir", os.path.join(d, "out%d" % n),
                                            "--ingest", "device", "--decode", "device", "--output-size", "source", "--mjpg"]}
                for rep in range(2):                               # alternating; the faster of the two runs of a route is kept
                    for route, flags in routes.items():
                        t0 = time.perf_counter()
                        r = subprocess.run([sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(NH), "--width", str(NW)] + flags,
                                           capture_output=True, text=True, cwd=ROOT)
                        wall = time.perf_counter() - t0
                        assert r.returncode == 0 and "Traceback" not in r.stderr, r.stderr[-2000:]
                        walls[(route, n)] = min(wall, walls.get((route, n), 1e9))
                        print("chain %s %s frames %d run %d: %.2f s" % (size, route, n, rep, wall), file=sys.stderr, flush=True)
            chain = {}
            for route in ("planar", "bgr_test_list"):
                per = (walls[(route, 2 * N)] - walls[(route, N)]) / N
                chain[route] = {"wall_s": {str(N): walls[(route, N)], str(2 * N): walls[(route, 2 * N)]}, "ms_per_frame": 1e3 * per,
                                "frames_per_s": 1.0 / per if per > 0 else None}
            chain["what"] = ("a process per run; seconds per frame = (wall(2 N) - wall(N)) / N; the test-list route also writes its .npy outputs and "
                             "keeps the clip's frames in lists, which is part of what that route costs")
            row["chain_host_to_host"] = chain
    out["sizes"][size] = row
print(json.dumps(out, indent=1))
