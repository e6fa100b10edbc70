"""Child of tests/test_remap_i420_gpu.py (not a test module): stabnet_warp_rev_bundle2_i420 on the inputs of <in>.npz (frame, x_map, y_map,
size, planes, border_y, window -- four NaNs for none) in a process of its own, so that the switch the library reads once per process
(STABNET_REMAP_VEC4) can be set; dumps the output frame, the coverage counts and the Profiler's kernel names to <out>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(inp, out):
    from stabnet_amd import warp
    from stabnet_amd.deploy import Profiler
    dev = torch.device("cuda:0")
    z = np.load(inp)
    frame, xm, ym = (torch.from_numpy(z[k]).to(dev) for k in ("frame", "x_map", "y_map"))
    SH, SW = (int(v) for v in z["size"])
    window = None if np.isnan(z["window"]).any() else tuple(float(v) for v in z["window"])
    black = torch.zeros((SH, SW), dtype=torch.int32, device=dev)
    prof = Profiler(max_records=16, device=dev)
    got = warp.warpRevBundle2_i420(frame, xm, ym, (SH, SW), int(z["planes"]), window=window, border_y=int(z["border_y"]), black_count=black, prof=prof)
    names = [r[0] for r in prof.records(raw=True)]
    np.savez(out, out=got.cpu().numpy(), black=black.cpu().numpy(), names=np.array(names))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
