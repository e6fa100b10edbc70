"""Child of tests/test_remap_win_gpu.py (not a test module): stabnet_warp_rev_bundle2_win on the inputs of <in>.npz (src, x_map, y_map,
window, out_size) in a process of its own, so that switches the library reads once per process (STABNET_REMAP_VEC4) can be set; dumps
out, px, py, the coverage counts and the Profiler's kernel names to <out>.npz."""
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
    black = torch.zeros((OH, OW), dtype=torch.int32, device=dev)
    prof = Profiler(max_records=16, device=dev)
    got, px, py = warp.warpRevBundle2_win(src, xm, ym, window, (OH, OW), black_count=black, return_maps=True, prof=prof)
    names = [r[0] for r in prof.records(raw=True)]
    np.savez(out, out=got.cpu().numpy(), px=px.cpu().numpy(), py=py.cpu().numpy(), black=black.cpu().numpy(), names=np.array(names))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
