#!/usr/bin/env python3
"""Score a stabilised clip against its unstable source: the literature's cropping ratio, distortion value and stability score
(stabnet_amd/metrics.py; the corner tracks and the robust homography fit run on the GPU).

    python tools/score_clip.py --unstable A --stable B [--height 288 --width 512] [--thr-px 2] [--per-frame] [--json OUT] [--scenes FILE.json]

A and B: uint8 .npy clips ([T,H,W] grey or [T,H,W,3] BGR) or Motion-JPEG .avi files with the same number of frames, read the way
deploy_bundle.py reads its inputs (--decode device: decoded on the GPU where the stream allows it, else with Pillow).  Frames that
are not --height x --width are converted by the ingest stage (cv2.cvtColor and Pillow's BILINEAR resize, csrc/ingest.hip).
One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_clip(path, dev, decode):
    """-> frame(t) -> uint8 device tensor, number of frames, (h, w, channels)."""
    import torch
    if path.lower().endswith('.avi'):
        from stabnet_amd.avi import AviMjpegReader
        rd = AviMjpegReader(path)
        if decode == 'device':
            from stabnet_amd.mjpeg import Unsupported
            try:
                clip = rd.device_clip(dev)
                f0 = clip.device_frame(0)
                return clip.device_frame, len(rd), tuple(f0.shape) if f0.dim() == 3 else tuple(f0.shape) + (1,)
            except Unsupported as e:
                print('note: --decode device: %s: %s; decoded on the host with Pillow' % (path, e), file=sys.stderr)
        frames = np.stack(list(rd.frames()))
    else:
        frames = np.load(path, mmap_mode='r')
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] not in (1, 3)):
        raise SystemExit('%s: expected uint8 [T,H,W] or [T,H,W,3], got %s %s' % (path, frames.dtype, list(frames.shape)))
    shape = tuple(frames.shape[1:3]) + (frames.shape[3] if frames.ndim == 4 else 1,)
    return (lambda t: torch.from_numpy(np.ascontiguousarray(frames[t])).to(dev)), len(frames), shape


def to_network(frame, n, shape, H, W, dev, gray):
    """Every frame as float32 [T,H,W] on the 0..255 scale: as read when it is grey at the network's size, else through the ingest."""
    import torch
    from stabnet_amd import metrics
    from stabnet_amd.ingest import FrameIngest
    h, w, c = shape
    if (h, w) == (H, W):
        # (clone: a decoder hands out its own buffer, valid until the next frame)
        return metrics.grey(torch.stack([(frame(t).reshape(h, w, c)[..., 0] if c == 1 else frame(t)).clone() for t in range(n)]))
    ing = FrameIngest(h, w, c, H, W, gray=gray, device=dev)
    return (torch.cat([ing.grey(frame(t)) for t in range(n)]) + 0.5) * 255.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--unstable', required=True)
    ap.add_argument('--stable', required=True)
    ap.add_argument('--height', type=int, default=288)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--thr-px', type=float, default=2.0)
    ap.add_argument('--hypotheses', type=int, default=256)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--per-frame', action='store_true')
    ap.add_argument('--decode', default='host', choices=['host', 'device'])
    ap.add_argument('--gray-weights', default='cv3', choices=['cv3', 'cv4'])
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--json', default=None, metavar='OUT', help='also write the result to this file')
    ap.add_argument('--scenes', default=None, metavar='FILE.json',
                    help='<name>_scenes.json of a deploy_bundle.py --scene-cut run: the stable pair across each cut is left out of the stability '
                         'path and counted as scene_cuts')
    ap.add_argument('--scenes-offset', type=int, default=1,
                    help='frame of the input clip that the first scored frame is (default 1: the driver\'s outputs start at the clip\'s frame 1)')
    a = ap.parse_args()
    cuts = None
    if a.scenes:
        with open(a.scenes) as f:
            cuts = [int(c) - a.scenes_offset for c in json.load(f)['cuts']]
    import torch
    from stabnet_amd import metrics
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    fu, nu, su = read_clip(a.unstable, dev, a.decode)
    fs, ns, ss = read_clip(a.stable, dev, a.decode)
    if nu != ns:
        raise SystemExit('the clips must have the same number of frames: %s has %d, %s has %d' % (a.unstable, nu, a.stable, ns))
    u = to_network(fu, nu, su, a.height, a.width, dev, a.gray_weights)
    s = to_network(fs, ns, ss, a.height, a.width, dev, a.gray_weights)
    if cuts is not None:
        cuts = [c for c in cuts if 0 <= c < nu]
    res = metrics.score_clip(u, s, fit=metrics.HomfitParams(hypotheses=a.hypotheses, thr_px=a.thr_px, seed=a.seed), per_frame=a.per_frame,
                             cuts=cuts)
    res.update(unstable=a.unstable, stable=a.stable)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
