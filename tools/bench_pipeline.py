#!/usr/bin/env python3
"""Host-to-host rate of the deploy loop ("Host buffers"): a 720p clip that lives in HOST memory (grey float32 +
colour uint8 frames) in, stabilised colour frame + the network's grey output back in host memory, per frame.
  serial    the loop as the reference writes it (deploy_bundle.py:244-342) and as ./deploy_bundle.py runs it: upload, frame, remap,
            download, one after the other with the host waiting in between
  pipeline  stabnet_amd.deploy.ClipPipeline: the same work with upload / frame / download on three HIP streams (pinned staging)
  resident  the frame alone, inputs already in HBM (= what bench.py reports as `value`)
  --jpeg    instead of the legs above: the pipeline with the raw download (today's leg), with the JPEG encoder in every frame graph
            + the raw download, and with the encoder and NO raw download (what crosses PCIe per frame is the compressed frame); the
            three alternate, each repeated --repeats times, fps, host_wait_s and bytes downloaded per frame beside each
  --ingest  instead of the legs above: the pipeline as above (float32 grey + uint8 BGR uploaded at the network's size, converted by the
            host beforehand) against ClipPipeline(ingest=FrameIngest): ONE uint8 BGR frame uploaded at the source size
            (--src-height / --src-width, default the network's) and converted in the frame graph (csrc/ingest.hip); the two
            alternate, each repeated --repeats times, fps, host_wait_s and bytes uploaded per frame beside each
  --ingest --output-size source   instead of the legs above: three routes from a raw uint8 BGR clip of --src-height x --src-width to a
            stabilised clip, every one through ClipPipeline(ingest=FrameIngest): (a) network_size: the network at --height x --width,
            frames kept at that size (resize, then remap); (b) source_size: the same network, output="source" -- the raw frame warped at
            its own size by the network-size maps (csrc/remap.hip, stabnet_warp_rev_bundle2_src); (c) network_at_source_size: the
            network itself run at the source's size, the only other way to frames of that size.  With --jpeg every graph also encodes
            the kept frame and only the compressed frame is downloaded.  The three alternate, each repeated --repeats times; fps,
            host_wait_s and the bytes that cross PCIe per frame beside each.  --fill R adds a fourth leg, source_size_fill: (b) with
            ClipPipeline(window=ratio_window(.., R)) -- the borderless frame, same size, through stabnet_warp_rev_bundle2_win
One JSON object on stdout.   python tools/bench_pipeline.py [--frames 300] [--height 720 --width 1280] [--jpeg | --ingest [--output-size source [--jpeg]]]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stabnet_amd import synthetic, warp
from stabnet_amd.config import Config
from stabnet_amd.deploy import ClipPipeline, StabNetStream

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--slots", type=int, default=3)
ap.add_argument("--jpeg", action="store_true")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--ingest", action="store_true")
ap.add_argument("--src-height", type=int, default=None)
ap.add_argument("--src-width", type=int, default=None)
ap.add_argument("--jpeg-quality", type=int, default=75)
ap.add_argument("--output-size", default="network", choices=["network", "source"])
ap.add_argument("--fill", type=float, default=None, help="with --ingest --output-size source: a leg with the centred window that keeps this share of each side")
a = ap.parse_args()
H, W, T = a.height, a.width, a.frames
dev = torch.device("cuda", 0)
cfg = Config(height=H, width=W)
params = synthetic.make_params(cfg, seed=0, theta_scale=0.2)
base = synthetic.make_clip(H, W, 40, seed=1234).astype(np.float32)
grey = np.ascontiguousarray(base[np.arange(T) % len(base)])                       # T host frames
bgr = np.ascontiguousarray(np.repeat(((grey + 0.5) * 255).clip(0, 255).astype(np.uint8)[..., None], 3, axis=3))
out = {"device": torch.cuda.get_device_name(0), "height": H, "width": W, "frames": T - 1,
       "host_bytes_per_frame": {"up": H * W * 4 + H * W * 3, "down": H * W * 3 + H * W}}


def serial():
    st = StabNetStream(params, H, W, cfg, device=dev, use_graph=True)
    st.start(torch.from_numpy(grey[0][None]).to(dev))
    for t in range(1, 4):                                                        # graph capture + warm-up
        st.step(torch.from_numpy(grey[t][None]).to(dev))
    torch.cuda.synchronize()
    st.start(torch.from_numpy(grey[0][None]).to(dev))
    t0 = time.perf_counter()
    for t in range(1, T):
        cur = torch.from_numpy(grey[t][None]).to(dev)
        r = st.step(cur)
        c = warp.warpRevBundle2(torch.from_numpy(bgr[t]).to(dev), r["x_map"], r["y_map"]).cpu().numpy()
        o = ((r["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
    dt = time.perf_counter() - t0
    return (T - 1) / dt, (c, o)


def pipeline(consume=True):
    st = StabNetStream(params, H, W, cfg, device=dev, use_graph=True)
    pipe = ClipPipeline(st, colour=True, slots=a.slots)
    pipe.run(grey[:120], bgr[:120], sink=lambda r: None)                         # graph capture + warm-up (clocks: a run that follows the
                                                                                 # half-idle serial loop is ~6 % slower for its first 0.3 s)
    got_c, got_o = np.zeros((T, H, W, 3), np.uint8), np.zeros((T, H, W), np.uint8)   # the consumer's own (touched) arrays
    def sink(r):
        if consume:
            np.copyto(got_c[r["t"]], r["bgr"]); np.copyto(got_o[r["t"]], r["output"])
        else:
            got_c[T - 1, 0, 0, 0] = r["bgr"][0, 0, 0]
    t0 = time.perf_counter()
    pipe.run(grey, bgr, sink=sink)
    dt = time.perf_counter() - t0
    out.setdefault('pipeline_host_blocked_ms_per_frame', []).append(1e3 * pipe.host_wait_s / (T - 1))
    return (T - 1) / dt, (got_c[T - 1], got_o[T - 1])


def resident():
    st = StabNetStream(params, H, W, cfg, device=dev, use_graph=True)
    d = torch.from_numpy(grey[:8]).to(dev)
    st.start(d[0:1])
    for t in range(1, 4):
        st.step(d[t:t + 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(1, T):
        st.step(d[t % 8:t % 8 + 1])
    torch.cuda.synchronize()
    return (T - 1) / (time.perf_counter() - t0)


def jpeg_legs():
    """raw / jpeg + raw / jpeg only, alternating in one process: the legs see the same clocks and the same neighbours."""
    opts = dict(quality=a.jpeg_quality, subsampling="420")
    pipes = {"raw": (ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, slots=a.slots), True),
             "jpeg_and_raw": (ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, slots=a.slots, jpeg=opts), True),
             "jpeg_only": (ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, slots=a.slots, jpeg=opts), False)}
    legs = {k: {"fps": [], "host_wait_s": [], "bytes_down_per_frame": []} for k in pipes}
    got_c, got_o, got_j = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), np.zeros(H * W * 3, np.uint8)
    def sink(r):                                                                  # the consumer touches everything it was given
        if "bgr" in r:
            np.copyto(got_c, r["bgr"]); np.copyto(got_o, r["output"])
        if "jpeg" in r:
            got_j[:len(r["jpeg"])] = r["jpeg"]
    for pipe, raw in pipes.values():
        pipe.run(grey[:120], bgr[:120], sink=sink, **({} if raw else {"raw": False}))      # graph capture + warm-up
    for _ in range(a.repeats):
        for name, (pipe, raw) in pipes.items():
            t0 = time.perf_counter()
            pipe.run(grey, bgr, sink=sink, **({} if raw else {"raw": False}))
            dt = time.perf_counter() - t0
            legs[name]["fps"].append((T - 1) / dt)
            legs[name]["host_wait_s"].append(pipe.host_wait_s)
            legs[name]["bytes_down_per_frame"].append((H * W * 4 if raw else 0) + getattr(pipe, "jpeg_bytes_down", 0) / (T - 1))
    med = lambda v: sorted(v)[len(v) // 2]
    out["jpeg_legs"] = legs
    out["jpeg_chunk_bytes"] = pipes["jpeg_only"][0].jpeg_chunk
    out["jpeg_only_over_raw"] = med(legs["jpeg_only"]["fps"]) / med(legs["raw"]["fps"])
    out["jpeg_and_raw_over_raw"] = med(legs["jpeg_and_raw"]["fps"]) / med(legs["raw"]["fps"])


def ingest_legs():
    """upload at the network's size (host-converted) / one raw uint8 frame + ingest launches, alternating in one process."""
    from stabnet_amd.ingest import FrameIngest
    sh, sw = a.src_height or H, a.src_width or W
    src = synthetic.make_clip(sh, sw, 40, seed=1234).astype(np.float32) if (sh, sw) != (H, W) else base
    g8 = ((src + 0.5) * 255).clip(0, 255)
    raw = np.ascontiguousarray(np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)[np.arange(T) % len(src)])
    ing = FrameIngest(sh, sw, 3, H, W, device=dev)
    pipes = {"uploaded_at_network_size": ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, slots=a.slots),
             "ingest": ClipPipeline(StabNetStream(params, H, W, cfg, device=dev, use_graph=True), colour=True, slots=a.slots, ingest=ing)}
    args = {"uploaded_at_network_size": (grey, bgr), "ingest": (raw,)}
    legs = {k: {"fps": [], "host_wait_s": []} for k in pipes}
    legs["uploaded_at_network_size"]["bytes_up_per_frame"] = H * W * 4 + H * W * 3
    legs["ingest"]["bytes_up_per_frame"] = sh * sw * 3
    got_c, got_o = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    def sink(r):                                                                  # the consumer touches everything it was given
        np.copyto(got_c, r["bgr"]); np.copyto(got_o, r["output"])
    for name, pipe in pipes.items():
        pipe.run(*(v[:120] for v in args[name]), sink=sink)                       # graph capture + warm-up
    for _ in range(a.repeats):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.run(*args[name], sink=sink)
            dt = time.perf_counter() - t0
            legs[name]["fps"].append((T - 1) / dt)
            legs[name]["host_wait_s"].append(pipe.host_wait_s)
    med = lambda v: sorted(v)[len(v) // 2]
    out["ingest_legs"] = legs
    out["source"] = [sh, sw]
    out["ingest_over_uploaded"] = med(legs["ingest"]["fps"]) / med(legs["uploaded_at_network_size"]["fps"])
    f = legs["uploaded_at_network_size"]["fps"]
    out["uploaded_leg_spread"] = (max(f) - min(f)) / med(f)


def source_legs():
    """frames kept at the network's size / at the source's size by the source-size remap / by running the network at the source's size,
    alternating in one process."""
    from stabnet_amd.ingest import FrameIngest
    sh, sw = a.src_height or H, a.src_width or W
    src = synthetic.make_clip(sh, sw, 40, seed=1234).astype(np.float32)
    g8 = ((src + 0.5) * 255).clip(0, 255)
    raw40 = np.ascontiguousarray(np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8))

    class Clip:                                                                   # T frames cycling through the 40 that exist
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, t):
            return raw40[t % len(raw40)]

    opts = dict(quality=a.jpeg_quality, subsampling="420") if a.jpeg else None
    cfg_s = Config(height=sh, width=sw)
    params_s = synthetic.make_params(cfg_s, seed=0, theta_scale=0.2)
    small = lambda: StabNetStream(params, H, W, cfg, device=dev, use_graph=True)
    pipes = {"network_size": ClipPipeline(small(), colour=True, slots=a.slots, jpeg=opts, ingest=FrameIngest(sh, sw, 3, H, W, device=dev)),
             "source_size": ClipPipeline(small(), colour=True, slots=a.slots, jpeg=opts, ingest=FrameIngest(sh, sw, 3, H, W, device=dev),
                                         output="source"),
             "network_at_source_size": ClipPipeline(StabNetStream(params_s, sh, sw, cfg_s, device=dev, use_graph=True), colour=True, slots=a.slots,
                                                    jpeg=opts, ingest=FrameIngest(sh, sw, 3, sh, sw, device=dev))}
    kept = {"network_size": (H, W), "source_size": (sh, sw), "network_at_source_size": (sh, sw)}
    net = {"network_size": (H, W), "source_size": (H, W), "network_at_source_size": (sh, sw)}
    if a.fill is not None:
        pipes["source_size_fill"] = ClipPipeline(small(), colour=True, slots=a.slots, jpeg=opts, ingest=FrameIngest(sh, sw, 3, H, W, device=dev),
                                                 output="source", window=warp.ratio_window(sh, sw, a.fill))
        kept["source_size_fill"], net["source_size_fill"] = (sh, sw), (H, W)
    legs = {k: {"fps": [], "host_wait_s": [], "bytes_down_per_frame": [], "network": list(net[k]), "kept_frame": list(kept[k]),
                "bytes_up_per_frame": sh * sw * 3} for k in pipes}
    got = {k: (np.zeros(kept[k] + (3,), np.uint8), np.zeros(net[k], np.uint8), np.zeros(kept[k][0] * kept[k][1] * 3, np.uint8)) for k in pipes}
    kw = {"raw": False} if a.jpeg else {}
    def sink_of(name):
        c, o, j = got[name]
        def sink(r):                                                              # the consumer touches everything it was given
            if "bgr" in r:
                np.copyto(c, r["bgr"]); np.copyto(o, r["output"])
            if "jpeg" in r:
                j[:len(r["jpeg"])] = r["jpeg"]
        return sink
    for name, pipe in pipes.items():
        pipe.run(Clip(min(T, 120)), sink=sink_of(name), **kw)                     # graph capture + warm-up
    for _ in range(a.repeats):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.run(Clip(T), sink=sink_of(name), **kw)
            dt = time.perf_counter() - t0
            legs[name]["fps"].append((T - 1) / dt)
            legs[name]["host_wait_s"].append(pipe.host_wait_s)
            raw_bytes = 0 if a.jpeg else kept[name][0] * kept[name][1] * 3 + net[name][0] * net[name][1]
            legs[name]["bytes_down_per_frame"].append(raw_bytes + getattr(pipe, "jpeg_bytes_down", 0) / (T - 1))
    med = lambda v: sorted(v)[len(v) // 2]
    out["source_legs"] = legs
    out["source"] = [sh, sw]
    out["jpeg"] = bool(a.jpeg)
    out["source_size_over_network_at_source_size"] = med(legs["source_size"]["fps"]) / med(legs["network_at_source_size"]["fps"])
    out["source_size_over_network_size"] = med(legs["source_size"]["fps"]) / med(legs["network_size"]["fps"])
    if a.fill is not None:
        out["fill"] = a.fill
        out["source_size_fill_over_source_size"] = med(legs["source_size_fill"]["fps"]) / med(legs["source_size"]["fps"])
    for k in legs:
        f = legs[k]["fps"]
        legs[k]["spread"] = (max(f) - min(f)) / med(f)


if a.output_size == "source" and not a.ingest:
    ap.error("--output-size source goes with --ingest")
if a.fill is not None and not (a.ingest and a.output_size == "source" and 0.0 < a.fill <= 1.0):
    ap.error("--fill R (0 < R <= 1) goes with --ingest --output-size source")

if a.ingest and a.output_size == "source":
    source_legs()
    out["slots"] = a.slots
    print(json.dumps(out))
    sys.exit(0)

if a.ingest:
    ingest_legs()
    out["slots"] = a.slots
    print(json.dumps(out))
    sys.exit(0)

if a.jpeg:
    jpeg_legs()
    out["slots"] = a.slots
    print(json.dumps(out))
    sys.exit(0)

fs, last_s = serial()
fp, last_p = pipeline()
out["serial_fps"] = fs
out["pipeline_fps"] = fp
out["pipeline_fps_results_left_in_staging"] = pipeline(consume=False)[0]
out["resident_fps"] = resident()
out["pipeline_over_serial"] = fp / fs
out["pipeline_of_resident"] = fp / out["resident_fps"]
out["same_bytes_last_frame"] = bool(np.array_equal(last_s[0], last_p[0]) and np.array_equal(last_s[1], last_p[1]))
out["slots"] = a.slots
print(json.dumps(out))
