"""Child of tests/test_remap_cubic_gpu.py (not a test module): the bicubic remap on the inputs of <in>.npz (src, x_map, y_map) in a
process of its own, so that STABNET_REMAP_VEC4 (read once per process) can be set; dumps out, the coverage counts and the Profiler's
kernel names to <out>.npz."""
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
    black = torch.zeros(src.shape[:-1], dtype=torch.int32, device=dev)
    prof = Profiler(max_records=16, device=dev)
    got = warp.warpRevBundle2_src(src, xm, ym, black_count=black, prof=prof, interp="cubic")
    names = [r[0] for r in prof.records(raw=True)]
    np.savez(out, out=got.cpu().numpy(), black=black.cpu().numpy(), names=np.array(names))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
