#!/usr/bin/env python3
"""tests/remap_cubic_model.py against a real OpenCV: cv2.remap(u8, map_x, map_y, INTER_CUBIC, BORDER_CONSTANT) on random frames and
maps, byte for byte.  The model restates OpenCV's published fixed-point path and was written where no cv2 was installed; whoever has
one can close that gap here.  No GPU, not run by any test.
   python tools/check_cubic_against_cv2.py [--cases 200] [--seed 0]
Exits 0 when every case is equal, 1 with the first differences otherwise, 2 with "cv2 not installed" where there is none."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:
    import cv2
except ImportError:
    print("cv2 not installed")
    sys.exit(2)

import numpy as np

import remap_cubic_model as CM

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=200)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
cv2.setUseOptimized(True)
rng = np.random.default_rng(a.seed)
bad = 0
for case in range(a.cases):
    h, w = int(rng.integers(1, 80)), int(rng.integers(1, 120))
    oh, ow = int(rng.integers(1, 80)), int(rng.integers(1, 120))
    C = int(rng.choice([1, 3]))
    border = int(rng.choice([0, 16, 128]))
    img = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
    # coordinates from well outside to well outside, on the 1/32 grid's ties as well as off it
    mx = rng.uniform(-5, w + 4, (oh, ow)).astype(np.float32)
    my = rng.uniform(-5, h + 4, (oh, ow)).astype(np.float32)
    if case % 3 == 0:
        mx, my = np.round(mx * 64) / 64, np.round(my * 64) / 64
    want = cv2.remap(img, mx.astype(np.float32), my.astype(np.float32), cv2.INTER_CUBIC, borderMode=cv2.BORDER_CONSTANT,
                     borderValue=(border,) * 3).reshape(oh, ow, C)
    got = CM.cv_remap_cubic_u8(img, mx, my, border=border)
    if not np.array_equal(got, want):
        bad += 1
        d = np.argwhere(got != want)
        print("case %d (%dx%dx%d -> %dx%d, border %d): %d of %d values differ, max |d| %d; first at %s: model %d, cv2 %d"
              % (case, h, w, C, oh, ow, border, len(d), got.size, int(np.abs(got.astype(int) - want.astype(int)).max()), d[0].tolist(),
                 got[tuple(d[0])], want[tuple(d[0])]))
print("cv2 %s: %d of %d cases equal" % (cv2.__version__, a.cases - bad, a.cases))
sys.exit(1 if bad else 0)
