#!/usr/bin/env python3
"""stabnet_mjpeg_decode alone (csrc/mjpeg_decode.hip) beside Pillow's decode of the same streams on the same box, and a whole clip
through deploy_bundle.py with --decode host against --decode device.
Per size (BGR 4:2:0 q75 streams written by Pillow with a restart interval of --restart MCUs, resident in HBM): device-event time of the
whole decode and of its stages (runs stopped after the entropy launch, after the IDCT, complete: stages by difference), the bytes the
shapes fix (compressed bytes read, coefficients and planes written and read once, the frame written) and that floor at the box's
measured copy rate (profiles/r03_copy_probe.txt), the host-to-host time of MjpegDecoder.decode (parse + one upload + launches +
status check), the same for a stream without DRI (coefficients decoded on the host), and Pillow's single-process decode time.
   python tools/mjpeg_decode_bench.py [--sizes 720x1280,1080x1920] [--reps 200] [--restart 2]      one JSON object on stdout
   python tools/mjpeg_decode_bench.py --clip 720x1280 --frames 120 --rounds 3      + "clip": wall time of deploy_bundle.py --mjpg
        --pipeline --ingest device on an MJPG .avi of that size, --decode host and --decode device alternating"""
import argparse
import io
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

from stabnet_amd import synthetic
from stabnet_amd.mjpeg import MjpegDecoder

COPY_RATE = 6.53e12        # bytes/s moved (read + written) by the best plain copy kernel measured on this box


def frames_bgr(H, W, T, seed=3):
    g8 = ((synthetic.make_clip(H, W, T, seed=seed) + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def pillow_jpeg(img, restart, quality=75):
    from PIL import Image
    buf = io.BytesIO()
    opts = {"restart_marker_blocks": restart} if restart else {}
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling="4:2:0", **opts)
    return buf.getvalue()


def pillow_decode_ms(jpegs, reps):
    from PIL import Image
    t0 = time.perf_counter()
    for i in range(reps):
        np.asarray(Image.open(io.BytesIO(jpegs[i % len(jpegs)])).convert("RGB"))
    return 1e3 * (time.perf_counter() - t0) / reps


def event_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_size(H, W, reps, restart, dev):
    imgs = frames_bgr(H, W, 4)
    row = {}
    for kind, R in (("dri", restart), ("no_dri", 0)):
        jpegs = [pillow_jpeg(f, R) for f in imgs]
        dec = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4)
        lay = dec.layout
        used = [dec.stage(j, dec.h_in[k]) for k, j in enumerate(jpegs)]
        for k, u in enumerate(used):
            dec.d_in[k, :u].copy_(dec.h_in[k, :u])
        out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        state = {"i": 0}

        def launch(stages):
            k = state["i"] = (state["i"] + 1) % 4
            dec.enqueue(dec.d_in[k:k + 1], 1, out, dec.status[:1], stages)

        t = [event_ms(lambda s=s: launch(s), reps) for s in (1, 2, 3)]
        assert int(dec.status[0]) == 0
        mean_bytes = sum(len(j) for j in jpegs) / 4.0
        coef, planes = 2.0 * dec.coef_count, lay["yh"] * lay["yw"] + 2.0 * lay["ch"] * lay["cw"]
        # compressed bytes (or nothing) + coefficients zeroed/written and read + planes written and read + the frame written
        moved = (0.0 if dec.host_entropy else mean_bytes + coef) + coef + 2.0 * planes + H * W * 3
        t0 = time.perf_counter()
        for i in range(reps):
            dec.decode([jpegs[i % 4]])
        host_to_host = 1e3 * (time.perf_counter() - t0) / reps
        row[kind] = {"restart_mcus": R, "host_entropy": dec.host_entropy, "jpeg_bytes_mean": mean_bytes,
                     "upload_bytes_mean": float(np.mean(used)), "raw_frame_bytes": H * W * 3,
                     "device_event_us": {"decode": 1e3 * t[2], "through_entropy": 1e3 * t[0], "idct": 1e3 * (t[1] - t[0]),
                                         "colour": 1e3 * (t[2] - t[1])},
                     "bytes_moved": moved, "copy_rate_floor_us": 1e6 * moved / COPY_RATE,
                     "decode_host_to_host_ms": host_to_host, "pillow_decode_ms": pillow_decode_ms(jpegs, max(20, reps // 4))}
    return row


def bench_clip(H, W, T, rounds, restart):
    from stabnet_amd.avi import AviMjpegWriter
    res = {"frames": T, "size": [H, W], "host_s": [], "device_s": []}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data", "unstable"))
        with AviMjpegWriter(os.path.join(tmp, "data", "unstable", "clip.avi"), W, H, 30) as w:
            for f in frames_bgr(H, W, T):
                w.write(pillow_jpeg(f, restart))
        with open(os.path.join(tmp, "list"), "w") as f:
            f.write("clip.avi\n")
        for r in range(rounds):
            for mode in ("host", "device"):
                cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--output-dir", os.path.join(tmp, "out_" + mode),
                       "--test-list", os.path.join(tmp, "list"), "--prefix", os.path.join(tmp, "data"), "--ingest", "device", "--mjpg",
                       "--pipeline", "--decode", mode]
                t0 = time.perf_counter()
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
                dt = time.perf_counter() - t0
                if p.returncode != 0 or "Traceback" in p.stderr:
                    raise SystemExit("deploy_bundle.py --decode %s failed:\n%s" % (mode, p.stderr[-2000:]))
                res[mode + "_s"].append(dt)
                fps = [float(l.split("=")[1]) for l in p.stdout.splitlines() if l.startswith("fps=")]
                res.setdefault(mode + "_loop_fps", []).append(fps[-1] if fps else None)
        same = all(open(os.path.join(tmp, "out_host", "output", n), "rb").read() == open(os.path.join(tmp, "out_device", "output", n), "rb").read()
                   for n in ("clip.avi", "clip_stable.npy", "clip_stable_bgr.npy"))
    res["same_output_bytes"] = same
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="720x1280,1080x1920")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--restart", type=int, default=2)
    ap.add_argument("--clip", default=None, metavar="HxW")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "sizes": {}}
    for size in [s for s in a.sizes.split(",") if s]:
        H, W = (int(v) for v in size.split("x"))
        out["sizes"][size] = bench_size(H, W, a.reps, a.restart, dev)
    if a.clip:
        H, W = (int(v) for v in a.clip.split("x"))
        out["clip"] = bench_clip(H, W, a.frames, a.rounds, a.restart)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
