"""A small dataset in the reference's layout for the dataset tests: numbered JPEG frames of two clip pairs written with Pillow, and
the samples that write_dataset turns into TFRecord files."""
import os

import numpy as np

FH, FW, T = 48, 64, 40           # frames
H, W = 32, 48                    # network input of the bit-exact tests
MAXM = 48


def image(clip, t, kind):
    rng = np.random.default_rng(1000 * clip + 10 * t + kind)
    yy, xx = np.mgrid[0:FH, 0:FW]
    g = np.stack([(xx * 4 + 3 * t) % 256, (yy * 5 + 2 * t) % 256, ((xx + yy) * 2 + 40 * kind) % 256], axis=-1)
    return np.clip(g + rng.integers(-30, 31, (FH, FW, 3)), 0, 255).astype(np.uint8)      # R, G, B


def write_frames(root, subsampling=(2, 2)):
    """stable/<clip>/<t>.jpg and unstable/<clip>/<t>.jpg; subsampling: Pillow's code per kind (2 = 4:2:0, 1 = 4:2:2)."""
    from PIL import Image
    for kind, name in enumerate(("stable", "unstable")):
        for clip in range(2):
            d = os.path.join(root, name, str(clip))
            os.makedirs(d, exist_ok=True)
            for t in range(T):
                Image.fromarray(image(clip, t, kind)).save(os.path.join(d, "%d.jpg" % t), quality=90, subsampling=subsampling[kind])


def samples(hw, flow=True):
    rng = np.random.default_rng(5)
    out = []
    for clip in range(2):
        for pos in range(34, 40):
            k1, k2 = int(rng.integers(0, MAXM)), int(rng.integers(0, MAXM))
            out.append({"stable_path": "stable/%d/" % clip, "unstable_path": "unstable/%d/" % clip, "pos": pos,
                        "flow": rng.normal(size=hw + (3,)).astype(np.float32) if flow else (),
                        "feature_matches1": rng.uniform(-1, 1, (k1, 4)).astype(np.float32),
                        "feature_matches2": rng.uniform(-1, 1, (k2, 4)).astype(np.float32)})
    return out
