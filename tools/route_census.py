#!/usr/bin/env python
"""Writes tests/golden/route_census.json: every structurally distinct conv launch of the inference plan over the sweep of frame
sizes, with its exemplar (tests/_route_census.py).  Host only; run it after any change to conv_route(), conv_plan(), the tuning
tables, the launchers' grid rule or the plan: tests/test_route_census_cpu.py fails until the file matches.

    python tools/route_census.py            # rewrite the file
    python tools/route_census.py --check    # exit 1 if the file is stale"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _route_census as rc  # noqa: E402


def main():
    t0 = time.time()
    got = rc.census()
    text = rc.golden_text(got)
    print("%d plans, %d conv launches, %d signatures in %.1f s (%d bytes)" % (got["plans"], got["conv_launches"], len(got["signatures"]),
                                                                           time.time() - t0, len(text)))
    by_kernel = {}
    for s in got["signatures"]:
        by_kernel[s["kernel"]] = by_kernel.get(s["kernel"], 0) + 1
    for k in sorted(by_kernel):
        print("  %4d  %s" % (by_kernel[k], k))
    if "--check" in sys.argv:
        same = os.path.exists(rc.GOLDEN) and open(rc.GOLDEN).read() == text
        print("up to date" if same else "STALE: " + rc.GOLDEN)
        return 0 if same else 1
    assert len(text) < (1 << 20), "the census outgrew the size limit of a committed file"
    with open(rc.GOLDEN, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
