#!/usr/bin/env python3
"""Writes tests/golden/mjpeg_decode_streams.npz: small JPEG streams written by Pillow and the pixels Pillow (libjpeg-turbo) decodes
from them -- what the device decoder (csrc/mjpeg_decode.hip) and the NumPy model (tests/jpeg_decode_model.py) must reproduce bit for
bit.  Needs a Pillow built on libjpeg-turbo; refuses to run otherwise.
   python tools/make_mjpeg_decode_golden.py"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_decode_model as D  # noqa: E402

# name, H, W, mode, quality, noise (standard deviation added to a smooth picture), restart MCUs (0 = none), extra
STREAMS = [
    ("420_45x77_q75", 45, 77, "420", 75, 0, 0, {}),
    ("420_45x77_q75_r3", 45, 77, "420", 75, 0, 3, {}),
    ("420_16x16_q95_noisy_r1", 16, 16, "420", 95, 25, 1, {}),
    ("444_33x50_q75_r2", 33, 50, "444", 75, 0, 2, {}),
    ("grey_45x77_q75_r4", 45, 77, "grey", 75, 0, 4, {}),
    ("420_64x96_q30_noisy", 64, 96, "420", 30, 25, 0, {}),
    ("420_17x31_q100_verynoisy", 17, 31, "420", 100, 120, 0, {}),
    ("420_8x8_q75", 8, 8, "420", 75, 0, 0, {}),
    ("420_40x56_q85_optimize_r2", 40, 56, "420", 85, 10, 2, {"optimize": True}),     # custom Huffman tables
    ("420_24x40_q75_nodht_r2", 24, 40, "420", 75, 5, 2, {"strip_dht": True}),         # as cameras write into AVI
]


def picture(H, W, grey, noise, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 7.0 + y / 11.0), 128 + 90 * np.cos(x / 5.0 - y / 9.0), 40 + 3.0 * x + 1.5 * y], -1)
    if noise:
        base = base + rng.normal(0.0, noise, base.shape)
    img = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    return img[..., 0].copy() if grey else img


def main():
    from PIL import Image
    if not D.have_turbo():
        sys.exit("this Pillow is not built on libjpeg-turbo: the golden pixels would not be libjpeg-turbo's")
    out = {"names": np.array([s[0] for s in STREAMS])}
    for seed, (name, H, W, mode, quality, noise, restart, extra) in enumerate(STREAMS):
        img = picture(H, W, mode == "grey", noise, seed)
        buf = io.BytesIO()
        opts = dict(quality=quality, optimize=bool(extra.get("optimize")))
        if mode != "grey":
            opts["subsampling"] = "4:2:0" if mode == "420" else "4:4:4"
        if restart:
            opts["restart_marker_blocks"] = restart
        Image.fromarray(img).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        if extra.get("strip_dht"):
            data = D.strip_dht(data)
        out["jpeg_" + name] = np.frombuffer(data, np.uint8)
        out["pixels_" + name] = D.pillow_bgr(data)
        print("%-30s %5d bytes" % (name, len(data)))
    np.savez_compressed(D.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (D.GOLDEN, os.path.getsize(D.GOLDEN)))


if __name__ == "__main__":
    main()
