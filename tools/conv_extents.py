#!/usr/bin/env python
"""Writes tests/golden/conv_extents.json: the largest batch stabnet_net_create() accepts at each frame size of tests/_extents.py, per
operand mode and fusion, and for training plans.  Host only; run it after a change to the extent guard (conv.h SN_CONV_EXTENT_LIMIT,
conv_extent_over) or to the plan's buffers: tests/test_conv_extents_cpu.py fails until the file matches.

    python tools/conv_extents.py            # rewrite the file
    python tools/conv_extents.py --check    # exit 1 if the file is stale"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _extents_search as ex  # noqa: E402


def main():
    text = ex.golden_text(ex.boundaries())
    print(text, end="")
    if "--check" in sys.argv:
        same = os.path.exists(ex.GOLDEN) and open(ex.GOLDEN).read() == text
        print("up to date" if same else "STALE: " + ex.GOLDEN)
        return 0 if same else 1
    with open(ex.GOLDEN, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
