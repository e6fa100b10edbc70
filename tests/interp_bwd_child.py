"""Child of tests/test_warp_bwd_ops_gpu.py (not a test module): train_ops.interp_bwd on every case of <in>.npz (x_<i>, y_<i>, g_<i>) in a
process of its own, so that the switch the library reads once per process (STABNET_INTERP_BWD_TILED=0: the untiled scatter also for one
channel) can be set; dumps d_<i> to <out>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(inp, out):
    from stabnet_amd import train_ops
    assert os.environ.get("STABNET_INTERP_BWD_TILED") == "0", "this child is the untiled arm"
    dev = torch.device("cuda:0")
    z = np.load(inp)
    res = {}
    for i in range(len(z.files) // 3):
        x, y, g = (torch.from_numpy(z["%s_%d" % (k, i)]).to(dev) for k in ("x", "y", "g"))
        res["d_%d" % i] = train_ops.interp_bwd(x, y, g).cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
