"""Child of tests/test_bwd_stages_gpu.py (not a test module): the bucket contract of the staged backward with the plan switches of
the environment (STABNET_STEM_ROWRUN is read once per process).  argv: N H W T split <workspace bytes of the parent's plan>.  Exits
non-zero on the first broken rule; the parent's plan has the row-run stem, this one must not (another input tensor and no row-run
gradient scratch: another workspace size)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import _bwd_stages as BS
    N, H, W, T, split, parent_nb = (int(a) for a in argv[:6])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    r = BS.run_case(dev, N, H, W, T, bool(split))
    assert r["workspace_bytes"] != parent_nb, "the child's plan has the parent's stem: the switch did not arrive"


if __name__ == "__main__":
    main(sys.argv[1:])
