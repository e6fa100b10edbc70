"""Child of tests/test_multistream_gpu.py (not a test module): one eager step of an S-stream StabNetStream from the random state of the
parent's case, with the plan switches of the environment (STABNET_STEM_ROWRUN is read once per process); dumps to <out>.npz what
_multistream.snapshot() reads back, the current frames, the Profiler's launch names, the bytes of the stack assembly's record and the
number of canary-banded buffers that were written outside."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out, S, H, W, mode, refine, head0):
    import _multistream as M
    from stabnet_amd.deploy import Profiler
    dev = torch.device("cuda:0")
    cfg, ocfg, P = M.make_params(H, W)
    st, guards = M.guarded_stream(P, H, W, cfg, S, dev, mode, refine=refine)
    st.start(torch.zeros((S, H, W), dtype=torch.float32, device=dev))
    state = M.random_state([S, H, W, mode, refine, head0, 0], S, st.depth, H, W)
    M.load_state(st, state, head0)
    prof = Profiler(max_records=4096, device=dev)
    st.step(torch.from_numpy(state["cur"]).to(dev), prof=prof)
    res = M.snapshot(st)
    recs = prof.records(raw=True)
    res["names"] = np.array([r[0] for r in recs])
    res["assemble_bytes"] = np.float64(sum(r[3] for r in recs if r[0].startswith("stack_assemble")))
    res["cur"] = state["cur"]
    bad = 0
    for name, g in guards.items():
        try:
            g.check(name)
        except AssertionError:
            bad += 1
    res["canaries_bad"] = np.int64(bad)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], *(int(v) for v in sys.argv[2:8]))
