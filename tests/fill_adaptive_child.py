"""Child of tests/test_fill_adaptive_gpu.py (not a test module): stabnet_warp_rev_bundle2_win and stabnet_warp_rev_bundle2_win_dev on the
inputs of <in>.npz (src, x_map, y_map, window, out_size) in a process of its own, so that STABNET_REMAP_VEC4 (read once per process)
can be set; dumps both results and the Profiler's kernel names of the device-window call to <out>.npz."""
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
    src, xm, ym = (torch.from_numpy(z[k]).to(dev) for k in ("src", "x_map", "y_map"))
    window, (OH, OW) = tuple(float(v) for v in z["window"]), (int(v) for v in z["out_size"])
    res = {}
    for tag, win in (("host", window), ("dev", torch.tensor(window, dtype=torch.float64, device=dev))):
        black = torch.zeros((OH, OW), dtype=torch.int32, device=dev)
        prof = Profiler(max_records=16, device=dev)
        got, px, py = warp.warpRevBundle2_win(src, xm, ym, win, (OH, OW), black_count=black, return_maps=True, prof=prof)
        res.update({tag + "_out": got.cpu().numpy(), tag + "_px": px.cpu().numpy(), tag + "_py": py.cpu().numpy(),
                    tag + "_black": black.cpu().numpy(), tag + "_names": np.array([r[0] for r in prof.records(raw=True)])})
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
