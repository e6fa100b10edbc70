#!/usr/bin/env python3
"""The parallel entropy back end (csrc/mjpeg_decode_sync.hip, MjpegDecoder parallel=True) beside the two ways the same streams were
decoded before it: host_entropy=True (Huffman decode on one CPU core, the coefficients uploaded) and the one-lane device decode.
Streams: Pillow BGR 4:2:0 WITHOUT restart markers of the synthetic clip, 720p and 1080p at q75 and 1080p at q95.  The legs alternate
inside one run (--alternations passes over all of them; the median is reported).  Per stream and chunk_bytes of --chunks:
  device-event time of the whole decode, of its phases (runs stopped after the guess launch, the hand-over, the repair and scan, the
  write, the IDCT, complete: phases by difference), the share of chunks left to the repair, the host-to-host time of
  MjpegDecoder.decode (parse + one upload + launches + status check) and the bytes uploaded -- and the same two numbers for the
  host_entropy decoder and the one-lane decoder.
--clip HxW: wall time of deploy_bundle.py --decode device --pipeline on an MJPG .avi of that size without restart markers, --entropy
auto and parallel alternating.
   python tools/mjpeg_sync_bench.py [--reps 100] [--chunks 16,32,64,128,256] [--clip 1080x1920 --frames 60]     one JSON object on stdout"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from mjpeg_decode_bench import event_ms, frames_bgr, pillow_jpeg
from stabnet_amd.mjpeg import MjpegDecoder


def _prepared(dec, jpegs):
    used = [dec.stage(j, dec.h_in[k]) for k, j in enumerate(jpegs)]
    for k, u in enumerate(used):
        dec.d_in[k, :u].copy_(dec.h_in[k, :u])
    torch.cuda.synchronize()
    return used


def _host_to_host_ms(dec, jpegs, reps):
    dec.decode([jpegs[0]])
    t0 = time.perf_counter()
    for i in range(reps):
        dec.decode([jpegs[i % len(jpegs)]])
    return 1e3 * (time.perf_counter() - t0) / reps


def bench_stream(H, W, quality, reps, chunks, alternations, dev, one_lane=True):
    jpegs = [pillow_jpeg(f, 0, quality) for f in frames_bgr(H, W, 4)]
    out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
    legs = {}
    host = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4)
    assert host.host_entropy
    legs["host_entropy"] = (host, _prepared(host, jpegs))
    if one_lane:
        lane = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4, host_entropy=False)
        legs["one_lane"] = (lane, _prepared(lane, jpegs))
    for c in chunks:
        d = MjpegDecoder.for_stream(jpegs[0], device=dev, batch=4, parallel=True, chunk_bytes=c)
        legs["parallel_%d" % c] = (d, _prepared(d, jpegs))
    samples = {}
    state = {"i": 0}
    for _ in range(alternations):
        for name, (dec, used) in legs.items():
            def launch(stages, dec=dec):
                k = state["i"] = (state["i"] + 1) % 4
                dec.enqueue(dec.d_in[k:k + 1], 1, out, dec.status[:1], stages)
            r = 3 if name == "one_lane" else reps                       # one lane walks the whole frame: hundreds of milliseconds
            stops = (-1, -2, -3, 1, 2, 3) if dec.parallel else (1, 2, 3)
            s = samples.setdefault(name, {"event_ms": {k: [] for k in stops}, "host_to_host_ms": []})
            for st in stops:
                if st == 1 and dec.host_entropy:
                    s["event_ms"][st].append(0.0)
                    continue
                s["event_ms"][st].append(event_ms(lambda st=st: launch(st), r))
            assert int(dec.status[0]) == 0
            s["host_to_host_ms"].append(_host_to_host_ms(dec, jpegs, max(3, r // 2)))
    row = {"jpeg_bytes_mean": sum(len(j) for j in jpegs) / 4.0, "raw_frame_bytes": H * W * 3, "legs": {}}
    for name, (dec, used) in legs.items():
        s = samples[name]
        ev = {k: statistics.median(v) for k, v in s["event_ms"].items()}
        leg = {"upload_bytes_mean": sum(used) / 4.0, "decode_host_to_host_ms": statistics.median(s["host_to_host_ms"]),
               "device_event_us": {"decode": 1e3 * ev[3], "through_entropy": 1e3 * ev[1], "idct": 1e3 * (ev[2] - ev[1]), "colour": 1e3 * (ev[3] - ev[2])}}
        if dec.parallel:
            leg["device_event_us"].update({"guess": 1e3 * ev[-1], "hand_over": 1e3 * (ev[-2] - ev[-1]), "repair_scan": 1e3 * (ev[-3] - ev[-2]),
                                           "write": 1e3 * (ev[1] - ev[-3])})
            shares = []
            for j in jpegs:                                             # the decoder's own batch keeps the chunk statistics
                dec.decode([j])
                n, ok = dec.sync_stats[0].cpu().tolist()
                shares.append((n - ok) / float(n))
            leg["chunks"] = n
            leg["share_left_to_repair"] = sum(shares) / len(shares)
        row["legs"][name] = leg
    return row


def bench_clip(H, W, T, rounds):
    from stabnet_amd.avi import AviMjpegWriter
    res = {"frames": T, "size": [H, W], "auto_s": [], "parallel_s": []}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data", "unstable"))
        with AviMjpegWriter(os.path.join(tmp, "data", "unstable", "clip.avi"), W, H, 30) as w:
            for f in frames_bgr(H, W, T):
                w.write(pillow_jpeg(f, 0))
        with open(os.path.join(tmp, "list"), "w") as f:
            f.write("clip.avi\n")
        for r in range(rounds):
            for mode in ("auto", "parallel"):
                cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--output-dir", os.path.join(tmp, "out_" + mode),
                       "--test-list", os.path.join(tmp, "list"), "--prefix", os.path.join(tmp, "data"), "--mjpg", "--pipeline",
                       "--decode", "device", "--entropy", mode]
                t0 = time.perf_counter()
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
                dt = time.perf_counter() - t0
                if p.returncode != 0 or "Traceback" in p.stderr:
                    raise SystemExit("deploy_bundle.py --entropy %s failed:\n%s" % (mode, p.stderr[-2000:]))
                res[mode + "_s"].append(dt)
                fps = [float(l.split("=")[1]) for l in p.stdout.splitlines() if l.startswith("fps=")]
                res.setdefault(mode + "_loop_fps", []).append(fps[-1] if fps else None)
        same = all(open(os.path.join(tmp, "out_auto", "output", n), "rb").read() == open(os.path.join(tmp, "out_parallel", "output", n), "rb").read()
                   for n in ("clip.avi", "clip_stable.npy", "clip_stable_bgr.npy"))
    res["same_output_bytes"] = same
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="720x1280q75,1080x1920q75,1080x1920q95")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--chunks", default="16,32,64,128,256")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--skip-one-lane", action="store_true", help="leave out the one-lane device decode (hundreds of milliseconds per frame)")
    ap.add_argument("--clip", default=None, metavar="HxW")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "alternations": a.alternations, "streams": {}}
    chunks = [int(c) for c in a.chunks.split(",") if c]
    for spec in [s for s in a.streams.split(",") if s]:
        size, q = spec.split("q")
        H, W = (int(v) for v in size.split("x"))
        out["streams"][spec] = bench_stream(H, W, int(q), a.reps, chunks, a.alternations, dev, one_lane=not a.skip_one_lane)
        print("measured %s" % spec, file=sys.stderr, flush=True)
    if a.clip:
        H, W = (int(v) for v in a.clip.split("x"))
        out["clip"] = bench_clip(H, W, a.frames, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
