#!/usr/bin/env python3
"""Writes tests/golden/mjpeg_planar_streams.npz: small grey and even-sided 4:2:0 JPEG streams written by Pillow and, for each, Pillow's
own decode left in YCbCr (im.draft("YCbCr", size)): libjpeg-turbo's Y plane exactly, plus its fancy-upsampled Cb / Cr.  The planar
decoder (stabnet_mjpeg_decode_i420) and its NumPy model (tests/jpeg_planar_model.py) must give that Y bit for bit, and chroma planes
whose h2v2 fancy upsampling is that Cb / Cr.  Needs a Pillow built on libjpeg-turbo; refuses to run otherwise.
   python tools/make_mjpeg_planar_golden.py"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import jpeg_decode_model as D  # noqa: E402
import jpeg_planar_model as P  # noqa: E402
from make_mjpeg_decode_golden import picture  # noqa: E402

# name, H, W, mode, quality, noise, restart MCUs (0 = none), extra: the smallest shapes at which the crop, the partial MCUs and each
# entropy back end (restart lanes; host coefficients and the parallel one for streams without DRI) can go wrong
STREAMS = [
    ("420_2x2_q75", 2, 2, "420", 75, 0, 0, {}),
    ("420_16x16_q95_noisy_r1", 16, 16, "420", 95, 25, 1, {}),
    ("420_18x34_q75_r3", 18, 34, "420", 75, 0, 3, {}),
    ("420_46x78_q30_noisy", 46, 78, "420", 30, 25, 0, {}),
    ("420_40x56_q85_optimize_r2", 40, 56, "420", 85, 10, 2, {"optimize": True}),
    ("420_24x40_q75_nodht_r2", 24, 40, "420", 75, 5, 2, {"strip_dht": True}),
    ("grey_45x77_q75_r4", 45, 77, "grey", 75, 0, 4, {}),
    ("grey_8x8_q75", 8, 8, "grey", 75, 0, 0, {}),
]


def main():
    from PIL import Image
    if not D.have_turbo():
        sys.exit("this Pillow is not built on libjpeg-turbo: the golden planes would not be libjpeg-turbo's")
    out = {"names": np.array([s[0] for s in STREAMS])}
    for seed, (name, H, W, mode, quality, noise, restart, extra) in enumerate(STREAMS):
        img = picture(H, W, mode == "grey", noise, 100 + seed)
        buf = io.BytesIO()
        opts = dict(quality=quality, optimize=bool(extra.get("optimize")))
        if mode != "grey":
            opts["subsampling"] = "4:2:0"
        if restart:
            opts["restart_marker_blocks"] = restart
        Image.fromarray(img).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        if extra.get("strip_dht"):
            data = D.strip_dht(data)
        out["jpeg_" + name] = np.frombuffer(data, np.uint8)
        # a stream without DHT is decoded by Pillow with the Annex K tables put back
        out["ycc_" + name] = P.pillow_draft_planes(D.with_dht(data))
        print("%-30s %5d bytes" % (name, len(data)))
    np.savez_compressed(P.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (P.GOLDEN, os.path.getsize(P.GOLDEN)))


if __name__ == "__main__":
    main()
