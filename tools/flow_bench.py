#!/usr/bin/env python3
"""TV-L1 optical flow alone (stabnet_amd/flow.py, csrc/tvl1.hip) at the training size 288x512, B = 8 and B = 32 pairs.

  legs      stepwise (STABNET_TVL1_FUSED=0: one launch per inner iteration) and fused (K iterations per launch) ALTERNATE, --legs
            times each; every leg is --reps solves with the Profiler's event records and --reps without (the whole solve between
            two events: the records' own events cost time the solve does not have).  Medians everywhere.
  stages    per kernel: launches per solve and the sum of their event times per solve
  iteration one inner iteration on the finest level: the stepwise launch, the fused launch divided by its K, the bytes an iteration
            has to move (ten planes read, six written) and a device-to-device copy of as many bytes timed in the same process -- the
            byte floor
  solve     per batch, per pair, and as a share of the 8-pair training step (ms_per_step of profiles/r03_bench_train_1gpu.json,
            or --train-step-ms)

    python tools/flow_bench.py [--reps 5] [--legs 3] [--out profiles/r13_flow_bench.json]        one JSON object on stdout"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stabnet_amd import flow
from stabnet_amd.deploy import Profiler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
ap.add_argument("--train-step-ms", type=float, default=None)
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
H, W = 288, 512
P = flow.Tvl1Params()
K = flow.fused_geometry()[0]


def median(v):
    return sorted(v)[len(v) // 2]


def pair(B):
    """A smooth random texture on the 0..255 scale and the same texture moved by a few pixels."""
    g = torch.Generator(device=dev).manual_seed(B)
    up = lambda n: torch.nn.functional.interpolate(torch.rand((B, 1, H // n + 3, W // n + 3), device=dev, generator=g),
                                                   size=(H + 16, W + 16), mode="bilinear", align_corners=False)[:, 0]
    t = (0.6 * up(4) + 0.4 * up(12)) * 255.0
    return t[:, 8:8 + H, 8:8 + W].contiguous(), t[:, 6:6 + H, 11:11 + W].contiguous()


train_ms, train_src = a.train_step_ms, "--train-step-ms"
if train_ms is None:
    src = os.path.join(ROOT, "profiles", "r03_bench_train_1gpu.json")
    with open(src) as f:
        train_ms, train_src = json.load(f)["ms_per_step"], "profiles/r03_bench_train_1gpu.json ms_per_step"

prof = Profiler(8192, device=dev)
prof.calibrate()
out = {"device": torch.cuda.get_device_name(0), "size": [H, W], "params": vars(P) if hasattr(P, "__dict__") else str(P), "fused_K": K,
       "fused_tile": list(flow.fused_geometry()[1:]), "reps": a.reps, "legs": a.legs, "idle_event_pair_us": 1e3 * prof.idle_pair_ms,
       "train_step_ms_8_pairs": train_ms, "train_step_source": train_src, "batches": {}}
MODES = (("stepwise", "0"), ("fused", "1"))
for B in a.batches:
    i0, i1 = pair(B)
    ws = torch.empty(flow.workspace_bytes(B, H, W, P), dtype=torch.uint8, device=dev)
    it_bytes = 64 * B * H * W
    src, dst = (torch.empty(it_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    res = {m: {"solve_ms": [], "iteration_us": [], "stages": []} for m, _ in MODES}
    copy_us, results = [], {}
    for m, env in MODES:                                                     # code objects load outside the records
        os.environ["STABNET_TVL1_FUSED"] = env
        results[m] = flow.tvl1_flow(i0, i1, P, out="uv", workspace=ws)
    dst.copy_(src)
    torch.cuda.synchronize()
    same = bool(torch.equal(results["stepwise"], results["fused"]))
    for _ in range(a.legs):
        for m, env in MODES:
            os.environ["STABNET_TVL1_FUSED"] = env
            prof.reset()
            for _ in range(a.reps):
                flow.tvl1_flow(i0, i1, P, out="uv", workspace=ws, prof=prof)
            stages, fine = {}, []
            for name, ms, _, nbytes, shape in prof.records_with_shapes():
                s = stages.setdefault(name, [0, 0.0])
                s[0] += 1
                s[1] += ms
                if name in ("tvl1_step_kernel", "tvl1_fused_kernel") and nbytes == it_bytes:
                    fine.append(1e3 * ms / max(shape[0], 1))
            res[m]["stages"].append({k: {"launches_per_solve": v[0] / a.reps, "ms_per_solve": v[1] / a.reps} for k, v in stages.items()})
            res[m]["iteration_us"].append(median(fine))
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                flow.tvl1_flow(i0, i1, P, out="uv", workspace=ws)
                e1.record()
            torch.cuda.synchronize()
            res[m]["solve_ms"].append(median([e0.elapsed_time(e1) for e0, e1 in ev]))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for e0, e1 in ev:
            e0.record()
            dst.copy_(src)                                                   # reads bytes / 2, writes bytes / 2
            e1.record()
        torch.cuda.synchronize()
        copy_us.append(1e3 * median([e0.elapsed_time(e1) for e0, e1 in ev]) - 1e3 * prof.overhead_ms)
    cu = median(copy_us)
    entry = {"same_bits": same, "iteration_bytes": it_bytes, "copy_of_the_same_bytes_us_medians": copy_us, "copy_of_the_same_bytes_us": cu,
             "fused_faster_in_every_leg": all(f < s for f, s in zip(res["fused"]["solve_ms"], res["stepwise"]["solve_ms"]))}
    for m, _ in MODES:
        ms, it = median(res[m]["solve_ms"]), median(res[m]["iteration_us"])
        entry[m] = {"solve_ms_medians": res[m]["solve_ms"], "solve_ms": ms, "ms_per_pair": ms / B,
                    "share_of_the_8_pair_training_step": ms * 8 / B / train_ms,
                    "finest_iteration_us_medians": res[m]["iteration_us"], "finest_iteration_us": it,
                    "finest_iteration_GBps": it_bytes / it * 1e-3, "times_the_byte_floor": it / cu if cu > 0 else None,
                    "stages": res[m]["stages"][len(res[m]["stages"]) // 2]}
    out["batches"]["B%d" % B] = entry
    del ws, src, dst, i0, i1
os.environ.pop("STABNET_TVL1_FUSED", None)
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
