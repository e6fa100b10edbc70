#!/usr/bin/env python3
"""Online stabilisation driver on MI355X -- drop-in for the reference's deploy_bundle.py call surface.

Same flags as the reference CLI (deploy_bundle.py:12-31).  What runs on the GPU is the part the reference times
(deploy_bundle.py:285-287): 13-channel stack -> regressor -> multi-grid warp, plus the history ring and the feedback,
which the reference does in NumPy on the host.  Differences forced by the offline image, stated rather than hidden:
  * --model-dir/--model-name take either a TF checkpoint prefix (`model-80000.index` + `.data-*`, read by
    stabnet_amd/tf_checkpoint.py without TensorFlow; the `.meta` graph is not needed) or a `.npz` written by
    train_bundle_nobm.py (TF variable names); without one, seeded synthetic weights are used and said so.
  * OpenCV is absent: clips are `.npy` arrays ([T,H,W] grey in [0,255] or [T,H,W,3] BGR) or Motion-JPEG `.avi` files
    (read on the host with Pillow, stabnet_amd/avi.py) under <prefix>/unstable/<name>; results are written as `.npy`
    (stabilised grey frames, x/y maps, black masks).  --mjpg also writes what the reference's cv2.VideoWriter('MJPG')
    writes (deploy_bundle.py:197-198,215,305,366-371): <name>.avi (the first frame as read, then every stabilised frame)
    and <name>_cut.avi (the crop), every frame a baseline JPEG encoded on the GPU (csrc/mjpeg.hip).
  * --ingest device: the frame as read (uint8, any size, BGR or grey) is uploaded once and converted on the GPU with the reference's
    own arithmetic (csrc/ingest.hip: cv2.cvtColor + PIL BILINEAR resize + normalisation for the network, cv2.resize for the colour
    frame that is warped and written), so a 720p colour clip run at 288x512 keeps its colour outputs.  The default, --ingest host,
    converts on the host with a two-tap resize and keeps colour only for clips that already have the network's size.
  * --output-size source (with --ingest device): the frame that is kept is the frame AS READ, warped at its own size by the
    network-size maps (csrc/remap.hip, stabnet_warp_rev_bundle2_src) instead of the reference's resize-then-warp (deploy_bundle.py:303):
    a 1080p clip run at 288x512 comes back as a 1080p <name>.avi, <name>_stable_bgr.npy and <name>_cut.*; <name>_stable.npy (the
    network's grey output) and <name>_maps.npz keep the network's size.
  * --fill R|auto (with --ingest device): borderless output.  The kept frame is a window of the stabilised frame, zoomed to the kept
    frame's own size in the remap's one gather (csrc/remap.hip, stabnet_warp_rev_bundle2_win).  --fill R (0 < R <= 1) runs online:
    <name>.avi, <name>_stable_bgr.npy and <name>_cut.* hold the centred window that keeps R of each side.  --fill auto runs a second
    pass after the clip: the largest window of the output's aspect ratio inside the black-free rectangle, written as <name>_fill.npy
    and, with --mjpg, <name>_fill.avi; everything else is written as without it.  --fill adaptive runs online too, with a window
    chosen per frame on the GPU (stabnet_fill_window_update, then stabnet_warp_rev_bundle2_win_dev): the largest centred window that
    provably shows no uncovered pixel, never below --fill-min, growing back by at most --fill-up per frame.  All three write
    <name>_fill_window.json.
  * --fill history [--fill-age 64] [--fill-feather 8] (with --ingest device, a colour clip, the serial loop): full-frame output.  Nothing
    is cut: a pixel the stabilised frame does not cover is taken from what earlier stabilised frames showed there, moved by a
    homography between the two stabilised frames that is fitted on the GPU (stabnet_amd/mosaic.py, csrc/mosaic.hip: corner tracks of
    the network's grey output, a coverage guard, the robust fit, one composing launch), at most --fill-age frames old, blended over
    --fill-feather pixels at the frame's edge.  Written beside everything the run writes without the flag: <name>_fill.npy, with
    --mjpg <name>_fill.avi, and <name>_fill_history.json (parameters, per frame the fresh / blended / history / empty pixel counts,
    the fit's status and inliers, the totals).
  * --decode device: the frames of a Motion-JPEG .avi are not decoded up front with Pillow; per frame the compressed bytes and their
    parsed description are uploaded in one copy and decoded on the GPU (csrc/mjpeg_decode.hip: bit for bit libjpeg-turbo's pixels)
    into the buffer the ingest reads.  Implies --ingest device.  A clip the decoder does not take (progressive, 4:2:2 ...) is read
    with Pillow as with --decode host, and a note says so.  --entropy parallel: a clip without restart markers, whose coefficients
    are otherwise decoded on the host and uploaded, is entropy-decoded on the GPU as well (csrc/mjpeg_decode_sync.hip); the same
    pixels, the compressed bytes cross PCIe instead of the coefficients.
  * --score: after a clip, the kept stabilised frames are scored against the input frames, both at the network's size
    (stabnet_amd/metrics.py: corner tracks and a robust homography per frame pair on the GPU, then the literature's cropping ratio,
    distortion value and stability score); <name>_score.json is written and the three numbers are printed.  The stabilised frames
    are the network's grey output, or, with --fill R / adaptive, the window that was written, converted by the ingest stage.  Off by
    default; no other output changes with it.
  * --y4m-in PATH|- [--y4m-out PATH|-]: a YUV4MPEG2 stream (8-bit 4:2:0 or mono; stabnet_amd/y4m.py) from a file or stdin, frame by
    frame in bounded memory, to a stream of the same size, chroma tag, frame rate, aspect and range in a file or on stdout:
      ffmpeg -i in.mp4 -f yuv4mpegpipe - | deploy_bundle.py --y4m-in - --y4m-out - | ffmpeg -i - out.mp4
    No colour conversion: the network reads the Y plane (range-expanded by the ingest's table when the stream is limited-range), and
    the frame's three planes are warped as they are in one gather (csrc/remap.hip, stabnet_warp_rev_bundle2_i420; taps outside the
    frame read black: Y 0 or 16, U = V = 128).  The test list is not read; --fill R is honoured; every message goes to stderr; at the
    end frames, fps and the luma pixels ever uncovered are reported, and <out>.json is written beside a --y4m-out file.  Without
    --y4m-out nothing is written but the report.
  * --avi-in PATH [--avi-out PATH] [--y4m-out PATH|-]: a 4:2:0 (or grey) Motion-JPEG .avi in YCbCr end to end, frame by frame in bounded
    memory.  Per frame the compressed bytes are uploaded once, the decoder leaves its Y / Cb / Cr planes as they are
    (csrc/mjpeg_decode.hip, stabnet_mjpeg_decode_i420), the network reads the Y plane (JFIF is full range: no table), the planes are
    warped as they are (stabnet_warp_rev_bundle2_i420; taps outside the frame read Y 0, U = V = 128) and the encoder starts from the
    planes (csrc/mjpeg.hip, stabnet_mjpeg_encode_i420): no colour conversion and no chroma resampling in either direction, and only
    compressed bytes cross PCIe.  --avi-out writes a 4:2:0 (grey) MJPG .avi at --jpeg-quality and the input's rate (or --fps), --y4m-out
    a C420jpeg / Cmono full-range stream at the input's rate; both may be given, with neither the run is a dry run.  Frame 0 seeds the
    ring and is written as decoded.  --fill R, --interp cubic, --scene-cut and --entropy parallel work as elsewhere; <out>.json holds
    the Y4M loop's report plus decode_backend and jpeg.  The test list is not read; every message goes to stderr.  A file that is no
    MJPG .avi, a first frame the planar decoder does not take (4:4:4, 4:2:2, an odd side: such clips keep the test-list route), and a
    later frame that differs or does not decode each end the run with one sentence and a non-zero status; the files written so far are
    closed valid.
  * --scene-cut [T] [--scene-gap 8]: scene cuts.  The loop is recurrent -- every frame is regressed against 32 earlier stabilised frames
    -- so after a cut the network would warp the new scene against the old one.  With the flag, the frame's graph starts with a cut
    decision on the GPU (csrc/scene.hip: the distance d between the 4 x 4 x 32 tile histograms of consecutive grey frames, a cut when
    d > T, default 0.35, and at least --scene-gap frames after the last one) and a ring reseed predicated on it: the run from a cut on
    equals a fresh run that starts there.  Works in the serial loop, with --pipeline and with --y4m-in; <name>_scenes.json holds the
    cuts and d per frame, the Y4M report scene_cuts; --fill history empties its canvas at a cut and --score leaves the pair across a
    cut out of the stability path.  Off by default; without it nothing differs.
  * --interp cubic: every colour, grey or planar frame that is kept is gathered with cv2.remap's INTER_CUBIC (16 taps, OpenCV's fixed-point
    weights; csrc/remap.hip, stabnet_warp_rev_bundle2_cubic / _i420_cubic) instead of INTER_LINEAR: a sharper picture from the same maps,
    the same coordinates and the same coverage counts.  In the serial loop, with --pipeline, with every --fill mode and with --y4m-in;
    --fill adaptive then keeps one more pixel of margin (margin_q = 8 + 32) so that no tap of the window leaves the frame, and --fill
    history composes the cubic frame.  The JSON reports record "interp".  The default, linear, is the reference's and changes nothing.
  * --before-ch is parsed and ignored exactly as in the reference (deploy_bundle.py:15,41): the ring depth is
    max(indices[1:]) = 32 and six frames are sampled at lags 1,2,4,8,16,32.
"""
import argparse
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--model-dir')
    p.add_argument('--model-name')
    p.add_argument('--before-ch', type=int)
    p.add_argument('--output-dir', default='data_video_local')
    p.add_argument('--infer-with-stable', action='store_true')
    p.add_argument('--infer-with-last', action='store_true')
    p.add_argument('--test-list', nargs='+', default=['data_video/test_list', 'data_video/train_list_deploy'])
    p.add_argument('--prefix', default='data_video')
    p.add_argument('--max-span', type=int, default=1)
    p.add_argument('--random-black', type=int, default=None)
    p.add_argument('--start-with-stable', action='store_true')
    p.add_argument('--refine', type=int, default=1)
    p.add_argument('--no_bm', type=int, default=1)
    p.add_argument('--gpu_memory_fraction', type=float, default=0.1)
    p.add_argument('--deploy-vis', action='store_true')
    # extensions of this build
    p.add_argument('--height', type=int, default=None, help='network/warp height (reference: fixed 288)')
    p.add_argument('--width', type=int, default=None, help='network/warp width (reference: fixed 512)')
    p.add_argument('--synthetic', type=int, default=0, help='stabilise a synthetic shaky clip of this many frames')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--pipeline', action='store_true',
                   help='overlap upload / frame / download of neighbouring frames on three HIP streams (stabnet_amd.deploy.ClipPipeline); '
                        'same output bytes, fps is then the host-to-host rate of the whole loop')
    p.add_argument('--operand-mode', type=int, default=4, choices=[0, 1, 2, 3, 4],
                   help='conv operand mode of the regressor (include/stabnet_hip.h): 4 = packed split kernels -- float32 operands as exact '
                        'sums of three bf16 terms on the bf16 matrix pipe, float32 accumulation, float32-level results (default); '
                        '0 = exact f32 MFMA; 1 = bf16 operands (reduced precision)')
    p.add_argument('--mjpg', action='store_true',
                   help='also write <output-dir>/output/<name>.avi and <name>_cut.avi (Motion-JPEG, encoded on the GPU) as the reference does')
    p.add_argument('--jpeg-quality', type=int, default=75)
    p.add_argument('--jpeg-subsampling', default='420', choices=['420', '444'])
    p.add_argument('--ingest', default='host', choices=['host', 'device'],
                   help='where a frame becomes the network input: host = NumPy (two-tap resize, colour only at the network size); device = '
                        'stabnet_amd.ingest.FrameIngest, the reference\'s cv2/PIL chain on the GPU for uint8 clips of any size')
    p.add_argument('--decode', default='host', choices=['host', 'device'],
                   help='where the frames of a Motion-JPEG .avi are decoded: host = Pillow, the whole clip up front; device = '
                        'stabnet_amd.mjpeg.MjpegDecoder, frame by frame on the GPU from the uploaded compressed bytes (implies --ingest device)')
    p.add_argument('--entropy', default='auto', choices=['auto', 'parallel'],
                   help='--decode device: how a clip WITHOUT restart markers (what OpenCV, ffmpeg and cameras write) is entropy-decoded: '
                        'auto = on the host, the coefficients are uploaded; parallel = on the GPU from the uploaded compressed bytes, by '
                        'self-synchronising parallel Huffman decoding (csrc/mjpeg_decode_sync.hip).  A clip with restart markers is '
                        'decoded one lane per restart interval either way')
    p.add_argument('--gray-weights', default='cv3', choices=['cv3', 'cv4'],
                   help='--ingest device: fixed-point BGR2GRAY weights of OpenCV 3 (the reference\'s era) or OpenCV 4')
    p.add_argument('--output-size', default='network', choices=['network', 'source'],
                   help='size of the frames that are written: network = --height x --width, the frame resized and then warped as the '
                        'reference does; source (needs --ingest device) = the frame as read, warped at its own size by the network-size maps')
    p.add_argument('--fill', default=None, metavar='R|auto|adaptive|history',
                   help='borderless output (needs --ingest device): crop-and-zoom the stabilised frame to the kept frame\'s own size in the '
                        'remap\'s one gather (stabnet_warp_rev_bundle2_win).  R in (0, 1]: online, every kept frame is the centred window that '
                        'keeps R of each side; auto: a second pass through the largest window of the output\'s aspect ratio inside the '
                        'clip\'s black-free rectangle, written as <name>_fill.npy / _fill.avi; adaptive: online, the window is chosen per '
                        'frame on the GPU (stabnet_fill_window_update): the largest centred one that shows no uncovered pixel; history: '
                        'nothing is cut, uncovered pixels are filled from earlier stabilised frames (stabnet_amd.mosaic), written as '
                        '<name>_fill.npy / _fill.avi / _fill_history.json')
    p.add_argument('--fill-min', type=float, default=None, metavar='R',
                   help='--fill adaptive: the smallest ratio the window may shrink to, in (0, 1] (default 0.5); a frame that needs less '
                        'is cut at this ratio and may show uncovered pixels')
    p.add_argument('--fill-up', type=float, default=None, metavar='D',
                   help='--fill adaptive: how much the ratio may grow back per frame, >= 0 (default 0.002); zooming in is immediate')
    p.add_argument('--fill-age', type=int, default=None, metavar='N',
                   help='--fill history: the oldest earlier frame a filled pixel may come from, 1..254 frames back (default 64)')
    p.add_argument('--fill-feather', type=int, default=None, metavar='PX',
                   help='--fill history: width of the blend band at the stabilised frame\'s edge, a power of two 1..64 pixels (default 8)')
    p.add_argument('--score', action='store_true',
                   help='after a clip, score the kept stabilised frames against the input frames at the network\'s size: cropping ratio, '
                        'distortion value, stability score (stabnet_amd.metrics.score_clip); writes <name>_score.json')
    p.add_argument('--scene-cut', nargs='?', type=float, const=0.35, default=None, metavar='T',
                   help='detect scene cuts on the GPU inside the frame (stabnet_scene_update: the distance d in [0, 1] between the tile '
                        'histograms of consecutive grey frames; a cut is d > T, default 0.35, T in (0, 1]) and re-seed the history ring '
                        'with the first frame of the new scene (stabnet_ring_reseed_if); writes <name>_scenes.json')
    p.add_argument('--scene-gap', type=int, default=None, metavar='N',
                   help='--scene-cut: no cut is flagged within N frames of the last one or of the start, N >= 0 (default 8)')
    p.add_argument('--interp', default='linear', choices=['linear', 'cubic'],
                   help='how the kept frame is gathered from the source: linear (cv2.INTER_LINEAR, the reference\'s) or cubic '
                        '(cv2.INTER_CUBIC, 16 taps: sharper; stabnet_warp_rev_bundle2_cubic); the maps, the network and the ingest are unchanged')
    p.add_argument('--fps', type=float, default=30.0, help='frame rate written to the .avi (taken from the input when that is an .avi)')
    p.add_argument('--y4m-in', default=None, metavar='PATH|-',
                   help='stabilise a YUV4MPEG2 stream (8-bit 4:2:0 or mono) from this file, or from stdin with -, frame by frame in bounded '
                        'memory; the planes are warped as they are (stabnet_warp_rev_bundle2_i420); the test list is not read; implies '
                        '--ingest device --output-size source; every message goes to stderr')
    p.add_argument('--y4m-out', default=None, metavar='PATH|-',
                   help='with --y4m-in: write the stabilised stream (the input\'s size, chroma tag, frame rate, aspect and range) to this '
                        'file, with <PATH>.json beside it, or to stdout with -; without it only the report is printed')
    p.add_argument('--avi-in', default=None, metavar='PATH',
                   help='stabilise a 4:2:0 (or grey) Motion-JPEG .avi frame by frame in bounded memory, in YCbCr end to end: the planes are '
                        'decoded on the GPU as they are (stabnet_mjpeg_decode_i420), warped as they are (stabnet_warp_rev_bundle2_i420) and '
                        'encoded as they are (stabnet_mjpeg_encode_i420); only compressed bytes cross PCIe; the test list is not read; '
                        'every message goes to stderr')
    p.add_argument('--avi-out', default=None, metavar='PATH',
                   help='with --avi-in: write the stabilised clip as a 4:2:0 (or grey) Motion-JPEG .avi at --jpeg-quality and the input\'s '
                        'frame rate (or --fps), with <PATH>.json beside it; --y4m-out PATH|- may be given as well or instead (C420jpeg / '
                        'Cmono, full range); with neither only the report is printed')
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    given = sys.argv[1:] if argv is None else list(argv)
    args.fps_given = any(a == '--fps' or a.startswith('--fps=') for a in given)
    if args.avi_out is not None and args.avi_in is None:
        p.error('--avi-out needs --avi-in: it is the output of the Motion-JPEG stream loop')
    if args.avi_in is not None:
        if args.y4m_in is not None:
            p.error('--avi-in and --y4m-in each name the input of a stream loop: give one of them')
        if args.jpeg_subsampling != '420':
            p.error('--avi-in keeps the planes of a 4:2:0 clip as they are: --jpeg-subsampling 444 is not available in the Motion-JPEG stream loop')
        if args.pipeline:
            p.error('--avi-in runs its own serial loop: it is not available with --pipeline')
        if args.mjpg:
            p.error('--avi-in writes its Motion-JPEG clip with --avi-out: it is not available with --mjpg')
        if args.score:
            p.error('--avi-in keeps no frames to score: it is not available with --score')
        if args.synthetic:
            p.error('--avi-in names the input: it is not available with --synthetic')
        if args.fill in ('auto', 'adaptive', 'history'):
            p.error('--avi-in honours --fill R only: --fill %s is not available in the Motion-JPEG stream loop' % args.fill)
        if not 1 <= args.jpeg_quality <= 100:
            p.error('--jpeg-quality needs 1 <= Q <= 100, got %r' % (args.jpeg_quality,))
        if args.fps_given and not 0.0 < args.fps < float('inf'):
            p.error('--fps needs a positive finite rate, got %r' % (args.fps,))
        args.ingest, args.output_size, args.decode = 'device', 'source', 'device'
    if args.y4m_out is not None and args.y4m_in is None and args.avi_in is None:
        p.error('--y4m-out needs --y4m-in: it is the output of the Y4M loop')
    if args.y4m_in is not None:
        if args.pipeline:
            p.error('--y4m-in runs its own serial loop: it is not available with --pipeline')
        if args.mjpg:
            p.error('--y4m-in writes a Y4M stream (--y4m-out): it is not available with --mjpg')
        if args.score:
            p.error('--y4m-in keeps no frames to score: it is not available with --score')
        if args.decode == 'device':
            p.error('--y4m-in reads raw planes, there is nothing to decode: it is not available with --decode device')
        if args.synthetic:
            p.error('--y4m-in names the input: it is not available with --synthetic')
        if args.fill in ('auto', 'adaptive', 'history'):
            p.error('--y4m-in honours --fill R only: --fill %s is not available in the Y4M loop' % args.fill)
        args.ingest, args.output_size = 'device', 'source'
    if args.scene_cut is None and args.scene_gap is not None:
        p.error('--scene-gap belongs to --scene-cut')
    if args.scene_cut is not None:
        args.scene_gap = 8 if args.scene_gap is None else args.scene_gap
        if not 0.0 < args.scene_cut <= 1.0:                    # (a NaN fails both comparisons)
            p.error('--scene-cut needs 0 < T <= 1, got %r' % (args.scene_cut,))
        if args.scene_gap < 0:
            p.error('--scene-gap needs N >= 0, got %r' % (args.scene_gap,))
    if args.entropy != 'auto' and args.decode != 'device':
        p.error('--entropy %s belongs to --decode device' % args.entropy)
    if args.decode == 'device':
        args.ingest = 'device'                                 # the decoded frame lies on the GPU: that is where it is converted
    if args.output_size == 'source' and args.ingest != 'device':
        p.error('--output-size source needs --ingest device: the frame as read must lie on the GPU')
    if args.fill != 'adaptive' and (args.fill_min is not None or args.fill_up is not None):
        p.error('--fill-min / --fill-up belong to --fill adaptive')
    if args.fill == 'adaptive':
        args.fill_min = 0.5 if args.fill_min is None else args.fill_min
        args.fill_up = 0.002 if args.fill_up is None else args.fill_up
        if not 0.0 < args.fill_min <= 1.0:                     # (a NaN fails both comparisons)
            p.error('--fill-min needs 0 < R <= 1, got %r' % (args.fill_min,))
        if not 0.0 <= args.fill_up < float('inf'):
            p.error('--fill-up needs a finite D >= 0, got %r' % (args.fill_up,))
    if args.fill != 'history' and (args.fill_age is not None or args.fill_feather is not None):
        p.error('--fill-age / --fill-feather belong to --fill history')
    if args.fill == 'history':
        args.fill_age = 64 if args.fill_age is None else args.fill_age
        args.fill_feather = 8 if args.fill_feather is None else args.fill_feather
        if not 1 <= args.fill_age <= 254:
            p.error('--fill-age needs 1 <= N <= 254, got %r' % (args.fill_age,))
        if args.fill_feather not in (1, 2, 4, 8, 16, 32, 64):
            p.error('--fill-feather needs a power of two in 1..64, got %r' % (args.fill_feather,))
        if args.pipeline:
            p.error('--fill history runs in the serial loop only: it is not available with --pipeline')
    if args.fill is not None:
        if args.fill not in ('auto', 'adaptive', 'history'):
            try:
                args.fill = float(args.fill)
            except ValueError:
                p.error('--fill takes a ratio in (0, 1] or one of the words auto, adaptive, history, got %r' % (args.fill,))
            if not 0.0 < args.fill <= 1.0:                     # (a NaN fails both comparisons)
                p.error('--fill R needs 0 < R <= 1, got %r' % (args.fill,))
        if args.ingest != 'device':
            p.error('--fill needs --ingest device: the frame as read must lie on the GPU')
    return args


def grey_train(frame, H, W):
    """config.cvt_img2train (config.py:6-21) without cv2/PIL: BGR->grey (OpenCV weights), nearest-size bilinear
    resize when needed, scale to [-0.5, 0.5]."""
    f = np.asarray(frame, np.float32)
    if f.ndim == 3:
        f = 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]
    if f.shape != (H, W):
        ys = (np.arange(H) + 0.5) * f.shape[0] / H - 0.5
        xs = (np.arange(W) + 0.5) * f.shape[1] / W - 0.5
        y0 = np.clip(np.floor(ys).astype(int), 0, f.shape[0] - 1); y1 = np.clip(y0 + 1, 0, f.shape[0] - 1)
        x0 = np.clip(np.floor(xs).astype(int), 0, f.shape[1] - 1); x1 = np.clip(x0 + 1, 0, f.shape[1] - 1)
        wy = np.clip(ys - y0, 0, 1)[:, None]; wx = np.clip(xs - x0, 0, 1)[None, :]
        f = (f[y0][:, x0] * (1 - wy) * (1 - wx) + f[y0][:, x1] * (1 - wy) * wx
             + f[y1][:, x0] * wy * (1 - wx) + f[y1][:, x1] * wy * wx)
    return (f * (1.0 / 255) - 0.5).astype(np.float32)


def load_weights(args, cfg):
    from stabnet_amd import synthetic
    if args.model_dir and args.model_name:
        path = os.path.join(args.model_dir, args.model_name)
        for cand in (path, path + '.npz'):
            if os.path.exists(cand) and cand.endswith('.npz'):
                z = np.load(cand)
                print('restored weights from', cand)
                return {k: z[k] for k in z.files if not k.startswith('__')}
        if os.path.exists(path + '.index'):
            # the reference's own checkpoint format (new_saver.restore, deploy_bundle.py:45-47): read without TensorFlow
            from stabnet_amd import tf_checkpoint
            params, _ = tf_checkpoint.load_stabnet_variables(path)
            print('restored weights from TF checkpoint', path)
            return params
        print('WARNING: neither %s.npz nor %s.index found' % (path, path))
    print('using seeded synthetic weights (no trained model is available offline)')
    return synthetic.make_params(cfg, seed=0, theta_scale=0.2)


def is_colour(frame, H, W):
    f = np.asarray(frame)
    return f.ndim == 3 and f.shape[:2] == (H, W)


def first_frame_u8(clip, H, W):
    """The frame the reference writes before the loop (deploy_bundle.py:215): the first frame as read, at the network's size."""
    if is_colour(clip[0], H, W):
        return np.ascontiguousarray(clip[0], dtype=np.uint8)
    return ((grey_train(clip[0], H, W) + 0.5) * 255).clip(0, 255).astype(np.uint8)


def jpeg_options(args):
    return dict(quality=args.jpeg_quality, subsampling=args.jpeg_subsampling)


def scene_note(scene_log, t, cut, D, H, W, say=print):
    """--scene-cut: frame t's flag and D (host ints) into scene_log as (t, cut, d = D / (2*H*W)); a cut is said.  -> cut"""
    d = int(D) / (2.0 * H * W)
    scene_log.append((int(t), int(cut), d))
    if cut:
        say('scene cut at frame %d (d = %.2f)' % (t, d))
    return bool(cut)


def write_scenes_json(path, args, scene_log, say=print):
    """<name>_scenes.json: the threshold, the gap, the frames of the clip at which a new scene starts and d of every frame (0 for the
    first, which has nothing to differ from)."""
    import json
    with open(path, 'w') as f:
        json.dump({'threshold': args.scene_cut, 'gap': args.scene_gap, 'cuts': [t for t, cut, _ in scene_log if cut],
                   'd': [0.0] + [d for _, _, d in scene_log]}, f, indent=1)
        f.write('\n')
    say('wrote', path)


def run_serial(stream, clip, H, W, dev, frames_out, colour_out, xmaps, ymaps, blacks, jpeg_sink=None, enc=None, ing=None, black_src=None,
               window=None, black_win=None, adaptive=None, fill_log=None, mosaic=None, fill_frames=None, scene_log=None, interp='linear'):
    """The loop as the reference writes it (deploy_bundle.py:244-342): one frame at a time, the host waiting for each step;
    fps = frames / time inside the step, as the reference prints it (:285-289).  ing (--ingest device): the raw uint8 frame is
    uploaded and converted on the GPU inside the step.  black_src (--output-size source; int32 [src_h, src_w] on the device): the
    raw frame is warped at its own size and its coverage counted there.  window, black_win (--fill R): the kept frame is that window of
    the stabilised frame at the kept frame's size, its coverage counted at the output pixels.  adaptive (--fill adaptive; a
    warp.AdaptiveFill): the window is the one the GPU chooses for the frame; fill_log gets (window, stats) per frame.  mosaic (--fill
    history; a mosaic.Mosaic): the kept colour frame is remapped with its coordinates written out, composed over the canvas of the
    earlier frames, and the canvas goes to fill_frames; every other output is the one of a run without it.  scene_log (--scene-cut; the
    stream has enable_scene_cut()): gets (frame, cut, d) per frame from the step's device flag, read outside the timed part; at a cut the
    mosaic's canvas is emptied before the frame is composed.  interp (--interp): the taps of every remap of a kept frame."""
    import torch
    from stabnet_amd import warp
    tot_time, length = 0.0, 0
    # the frame as read on the device: uploaded, or (--decode device) decoded there from its compressed bytes
    raw = (lambda t: clip.device_frame(t)) if hasattr(clip, 'device_frame') else (lambda t: torch.from_numpy(np.ascontiguousarray(clip[t], dtype=np.uint8)).to(dev))
    if adaptive is not None:
        adaptive.reset()
    if mosaic is not None:
        mosaic.reset()
    if ing is not None:
        stream.start_u8(raw(0), ing)
    else:
        first = grey_train(clip[0], H, W)
        stream.start(torch.from_numpy(first[None]).to(dev))                   # ring = 32 x first frame, zero masks
    for t in range(1, len(clip)):
        cur = raw(t) if ing is not None else torch.from_numpy(grey_train(clip[t], H, W)[None]).to(dev)
        torch.cuda.synchronize()
        start = time.time()
        r = stream.step_u8(cur, ing) if ing is not None else stream.step(cur)     # one sess.run-equivalent
        torch.cuda.synchronize()
        tot_time += time.time() - start
        if scene_log is not None:
            if scene_note(scene_log, t, int(r['scene_cut'][0]), int(r['scene_dist'].cpu().numpy()[0]), H, W) and mosaic is not None:
                mosaic.reset(keep_log=True)                                       # the earlier frames show another scene
        if window is not None or adaptive is not None:
            # the window of the stabilised frame in the one gather: of the frame as read, or of the cv2-resized colour frame
            frame = cur if black_src is not None else ing.colour(cur)[0]
            win = window if adaptive is None else adaptive.update(r['x_map'], r['y_map'])     # (on the device: read there by the remap)
            colour_out.append(warp.warpRevBundle2_win(frame, r['x_map'], r['y_map'], win, black_count=black_win, interp=interp).cpu().numpy())
            if adaptive is not None:
                fill_log.append((adaptive.window[0].cpu().numpy(), adaptive.stats[0].cpu().numpy()))
        elif mosaic is not None:
            # the same remap as below with px_out / py_out written (the same output bytes), then the composite over the earlier frames
            if black_src is not None:
                kept_frame, px, py = warp.warpRevBundle2_src(cur, r['x_map'], r['y_map'], black_count=black_src, return_maps=True, interp=interp)
            else:
                kept_frame, px, py = warp.warpRevBundle2(ing.colour(cur)[0], r['x_map'], r['y_map'], return_maps=True, interp=interp)
            colour_out.append(kept_frame.cpu().numpy())
            canvas = mosaic.update(kept_frame.reshape(1, mosaic.SH, mosaic.SW, 3), px, py, r['output'][..., 0], r['black_pix'])
            fill_frames.append(canvas[0].cpu().numpy())
        elif black_src is not None:
            # where the reference resizes the colour frame down and warps it (deploy_bundle.py:303): the frame as read, warped as it is
            colour_out.append(warp.warpRevBundle2_src(cur, r['x_map'], r['y_map'], black_count=black_src, interp=interp).cpu().numpy())
        elif ing is not None and ing.C == 3:
            # cv2.resize of the colour frame (deploy_bundle.py:303), then warpRevBundle2, both on the device
            colour_out.append(warp.warpRevBundle2(ing.colour(cur)[0], r['x_map'], r['y_map'], interp=interp).cpu().numpy())
        elif ing is None and is_colour(clip[t], H, W):
            # warpRevBundle2 (deploy_bundle.py:136-146,303) on the device: colour frame remapped by the smoothed maps
            bgr = torch.from_numpy(np.ascontiguousarray(clip[t], dtype=np.uint8)).to(dev)
            colour_out.append(warp.warpRevBundle2(bgr, r['x_map'], r['y_map'], interp=interp).cpu().numpy())
        net_output = ((r['output'][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
        frames_out.append(net_output)
        if jpeg_sink is not None:                                             # the frame that is kept, compressed on the device
            kept = colour_out[-1] if (black_src is not None or (ing.C == 3 if ing is not None else is_colour(clip[t], H, W))) else net_output
            jpeg_sink(enc.encode_bytes(torch.from_numpy(np.ascontiguousarray(kept)).to(dev))[0])
        xmaps.append(r['x_map'][0, :, :, 0].cpu().numpy()); ymaps.append(r['y_map'][0, :, :, 0].cpu().numpy())
        blacks.append(r['black_pix'][0].cpu().numpy().astype(np.uint8))
        length += 1
        if length % 10 == 0:
            print('length: ' + str(length))
            print('fps={}'.format(length / tot_time))
    return length, tot_time


def run_pipelined(stream, clip, H, W, frames_out, colour_out, xmaps, ymaps, blacks, jpeg_sink=None, jpeg=None, ing=None, source=False,
                  window=None, fill=None, fill_log=None, scene_log=None, interp='linear'):
    """--pipeline: the same frames through stabnet_amd.deploy.ClipPipeline (upload / frame / download of neighbouring frames on
    three HIP streams).  Same output bytes; fps = frames / wall time of the whole loop, host conversion and copies included.
    window='adaptive' with fill=dict(r_min, up, margin_q): the per-frame window of --fill adaptive; fill_log gets (window, stats).
    scene_log (--scene-cut): gets (frame, cut, d) per frame.
    -> (frames, seconds, coverage at source size or None, coverage at the output pixels of the window or None)."""
    from stabnet_amd.deploy import ClipPipeline
    colour = ing.C == 3 if ing is not None else is_colour(clip[0], H, W)

    class Grey:                                                               # frames converted as the pipeline asks for them
        def __len__(self):
            return len(clip)

        def __getitem__(self, t):
            return grey_train(clip[t], H, W)

    def sink(r):                                                              # views of pinned staging memory: copy out
        frames_out.append(r['output'].copy())
        if colour or source:
            colour_out.append(r['bgr'].copy())
        if jpeg_sink is not None:
            jpeg_sink(bytes(r['jpeg']))
        xmaps.append(r['x_map'].copy()); ymaps.append(r['y_map'].copy()); blacks.append(r['black'].copy())
        if 'window' in r:
            fill_log.append((r['window'].copy(), r['fill_stats'].copy()))
        if 'scene_cut' in r:                                                  # --scene-cut: downloaded with the slot's other outputs
            scene_note(scene_log, r['t'], r['scene_cut'], r['scene_dist'], H, W)
        if len(frames_out) % 10 == 0:
            print('length: ' + str(len(frames_out)))

    start = time.time()
    black_src = black_win = None
    if ing is not None:                                                       # the raw clip: one uint8 upload per frame, nothing converted here
        pipe = ClipPipeline(stream, colour=colour, jpeg=jpeg, ingest=ing, output='source' if source else 'network', window=window,
                            fill=fill, decoder=getattr(clip, 'decoder', None), interp=interp)
        pipe.run(clip, sink=sink, maps=True)
        black_src = pipe.all_black_src if source else None
        black_win = pipe.all_black_win if window is not None else None
    else:
        ClipPipeline(stream, colour=colour, jpeg=jpeg, interp=interp).run(Grey(), clip if colour else None, sink=sink, maps=True)
    tot_time = time.time() - start
    if frames_out:
        print('fps={}'.format(len(frames_out) / tot_time))
    return len(frames_out), tot_time, black_src, black_win


def uncovered_per_frame(frame0, xmaps, ymaps, window, out_size, dev):
    """[pixels of frame t that the window leaves uncovered], from the maps the run kept: the coverage rule depends on the maps and the
    window alone, so any frame of the right size stands for the source.  window: one for the clip, or a list with one per frame.
    Outside the timed part."""
    import torch
    from stabnet_amd import warp
    cnt = torch.zeros(out_size, dtype=torch.int32, device=dev)
    per = []
    windows = window if isinstance(window, list) else [window] * len(xmaps)
    for xm, ym, win in zip(xmaps, ymaps, windows):
        cnt.zero_()
        warp.warpRevBundle2_win(frame0, torch.from_numpy(xm).to(dev), torch.from_numpy(ym).to(dev), win, out_size, black_count=cnt)
        per.append(int(cnt.sum().item()))
    return per


def write_fill_json(stem, mode, window, rect, out_size, uncovered, pixels_ever, interp='linear'):
    import json
    if pixels_ever is not None:
        uncovered = dict(uncovered, pixels_ever_uncovered=pixels_ever)
    with open(stem + '_fill_window.json', 'w') as f:
        json.dump({'mode': mode, 'window': [float(v) for v in window], 'rect': [int(v) for v in rect] if rect else None,
                   'output_size': [int(out_size[0]), int(out_size[1])], 'interp': interp, 'uncovered': uncovered}, f, indent=1)
        f.write('\n')
    print('wrote', stem + '_fill_window.json')


def write_fill_adaptive_json(stem, params, fill_log, nodes, out_size, uncovered, pixels_ever, interp='linear'):
    """<name>_fill_window.json of --fill adaptive: the parameters, and per frame the window the GPU chose, r_safe (the largest ratio its
    rule proves free of uncovered pixels; <= 0: none) and the number of bad nodes.  held_at_min: the frames whose r_safe lay below
    r_min -- cut at r_min, the only ones that may show uncovered pixels."""
    import json
    r_safe = [1.0 if int(st[0]) >= nodes else float(int(st[0])) / float(nodes) for _, st in fill_log]
    with open(stem + '_fill_window.json', 'w') as f:
        json.dump({'mode': 'adaptive', 'params': params, 'output_size': [int(out_size[0]), int(out_size[1])], 'interp': interp,
                   'windows': [[float(v) for v in w] for w, _ in fill_log], 'r_safe': r_safe,
                   'bad_nodes': [int(st[1]) for _, st in fill_log],
                   'held_at_min': sum(1 for r in r_safe if r < params['r_min']),
                   'uncovered': dict(uncovered, pixels_ever_uncovered=pixels_ever)}, f, indent=1)
        f.write('\n')
    print('wrote', stem + '_fill_window.json')


def write_fill_history(stem, mosaic, fill_frames, first, enc_options, fps, dev, args):
    """--fill history: <name>_fill.npy, with --mjpg <name>_fill.avi (as <name>.avi: the first frame as read comes first), and
    <name>_fill_history.json from the one readback of the per-frame log."""
    import json
    import torch
    from stabnet_amd import mosaic as mosaic_mod
    filled = np.stack(fill_frames)
    np.save(stem + '_fill.npy', filled)
    print('wrote', stem + '_fill.npy')
    if args.mjpg:
        from stabnet_amd.avi import AviMjpegWriter
        from stabnet_amd.mjpeg import MjpegEncoder
        oh, ow = filled.shape[1:3]
        enc = MjpegEncoder(oh, ow, 3, device=dev, **enc_options)
        with AviMjpegWriter(stem + '_fill.avi', ow, oh, fps) as w:
            w.write(enc.encode_bytes(torch.from_numpy(first).to(dev))[0])
            for f in filled:
                w.write(enc.encode_bytes(torch.from_numpy(np.ascontiguousarray(f)).to(dev))[0])
        print('wrote %s (%d frames %dx%d)' % (stem + '_fill.avi', len(filled) + 1, ow, oh))
    log = mosaic.log()
    tot = mosaic_mod.totals(log)
    with open(stem + '_fill_history.json', 'w') as f:
        json.dump({'mode': 'history', 'params': dict(mosaic.params_dict(), fill_age=args.fill_age, fill_feather=args.fill_feather),
                   'output_size': [mosaic.SH, mosaic.SW], 'network_size': [mosaic.H, mosaic.W], 'frames': int(len(filled)),
                   'per_frame': {k: [int(v) for v in log[k][:, 0]] for k in mosaic_mod.LOG_FIELDS}, 'totals': tot}, f, indent=1)
        f.write('\n')
    px = max(tot['fresh'] + tot['blended'] + tot['history'] + tot['empty'], 1)
    print('fill history: %.3f %% of the pixels came from earlier frames, %.3f %% were blended at the edge, %.3f %% stayed empty; '
          '%d of %d frames had no motion model' % (100.0 * tot['history'] / px, 100.0 * tot['blended'] / px, 100.0 * tot['empty'] / px,
                                                   tot['frames_without_model'], len(filled)))
    print('wrote', stem + '_fill_history.json')


def fill_report(per_frame, out_size):
    """The uncovered counts of a --fill run, printed and kept for <name>_fill_window.json."""
    n, px = len(per_frame), out_size[0] * out_size[1]
    bad = sum(1 for c in per_frame if c > 0)
    worst = max(per_frame) / px if per_frame else 0.0
    print('fill: %d of %d frames (%.1f %%) left some pixel uncovered; the worst frame left %.3f %% of its pixels uncovered'
          % (bad, n, 100.0 * bad / max(n, 1), 100.0 * worst))
    return {'frames': n, 'frames_uncovered': bad, 'worst_frame_share': worst, 'per_frame': per_frame}


def fill_second_pass(clip, ing, source, xmaps, ymaps, window, out_size, dev, stem, args, fps, first):
    """--fill auto: every frame again through the window -- the frame as read (or its cv2-resized colour frame) and its maps uploaded,
    stabnet_warp_rev_bundle2_win, the encoder.  -> [uncovered pixels per frame]."""
    import torch
    from stabnet_amd import warp
    from stabnet_amd.avi import AviMjpegWriter
    from stabnet_amd.mjpeg import MjpegEncoder
    oh, ow = out_size
    enc = writer = None
    if args.mjpg:
        enc = MjpegEncoder(oh, ow, 3 if ing.C == 3 else 1, device=dev, **jpeg_options(args))
        writer = AviMjpegWriter(stem + '_fill.avi', ow, oh, fps)
        writer.write(enc.encode_bytes(torch.from_numpy(first).to(dev))[0])       # as <name>.avi: the first frame as read comes first
    cnt = torch.zeros((oh, ow), dtype=torch.int32, device=dev)
    filled, per = [], []
    torch.cuda.synchronize()
    start = time.time()
    for t in range(1, len(xmaps) + 1):
        raw = torch.from_numpy(np.ascontiguousarray(clip[t], dtype=np.uint8)).to(dev)
        frame = raw if source else ing.colour(raw)[0]
        xm, ym = torch.from_numpy(xmaps[t - 1]).to(dev), torch.from_numpy(ymaps[t - 1]).to(dev)
        cnt.zero_()
        out = warp.warpRevBundle2_win(frame, xm, ym, window, (oh, ow), black_count=cnt, interp=args.interp)
        if writer is not None:
            writer.write(enc.encode_bytes(out)[0])
        filled.append(out.cpu().numpy())
        per.append(int(cnt.sum().item()))
    torch.cuda.synchronize()
    tot = time.time() - start
    if writer is not None:
        writer.close()
        print('wrote %s (%d frames %dx%d)' % (stem + '_fill.avi', writer.frames_written, ow, oh))
    np.save(stem + '_fill.npy', np.stack(filled))
    print('wrote', stem + '_fill.npy')
    print('fill pass: fps={}'.format(len(filled) / tot))
    return per


def score_outputs(clip, frames_out, colour_out, ing, filled, H, W, dev, stem, cuts=None, interp='linear'):
    """--score: frames 1.. of the clip as ingested (the network's grey input on the 0..255 scale) against the kept frames of the same
    instants: the network's grey output, or (filled) the window that was written, brought to the network's size by the ingest stage.
    cuts (--scene-cut): the frames of the CLIP at which a new scene starts; kept frame k is the clip's frame k + 1."""
    import json
    import torch
    from stabnet_amd import metrics
    from stabnet_amd.ingest import FrameIngest
    n = len(frames_out)
    if n < metrics.MIN_FRAMES:
        print('note: --score needs %d kept frames or more; this clip has %d and is not scored' % (metrics.MIN_FRAMES, n))
        return
    raw = (lambda t: clip.device_frame(t)) if hasattr(clip, 'device_frame') else (lambda t: torch.from_numpy(np.ascontiguousarray(clip[t], dtype=np.uint8)).to(dev))
    if ing is not None:
        unstable = torch.cat([ing.grey(raw(t)) for t in range(1, n + 1)])
    else:
        unstable = torch.from_numpy(np.stack([grey_train(clip[t], H, W) for t in range(1, n + 1)])).to(dev)
    unstable = (unstable + 0.5) * 255.0
    if filled and colour_out:
        kept = torch.from_numpy(np.stack(colour_out)).to(dev)
        kh, kw = kept.shape[1], kept.shape[2]
        stable = (FrameIngest(kh, kw, 3 if kept.dim() == 4 else 1, H, W, gray=ing.weights, batch=n, device=dev).grey(kept) + 0.5) * 255.0
        what = 'the written window'
    else:
        stable = torch.from_numpy(np.stack(frames_out)).to(dev)
        what = 'the network\'s grey output'
    res = metrics.score_clip(unstable, stable, cuts=None if cuts is None else [c - 1 for c in cuts if c - 1 < n])
    res['stable_frames'] = what
    res['interp'] = interp
    with open(stem + '_score.json', 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('score (%s, %d frames at %dx%d): cropping / distortion / stability = %.4f / %.4f / %.4f'
          % (what, n, W, H, res['cropping'], res['distortion'], res['stability']))
    print('wrote', stem + '_score.json')


def run_y4m(args, rd, stream, H, W, dev, out_file):
    """--y4m-in: the online loop over a Y4M stream of unknown length, in bounded memory -- one pinned and one device buffer per
    direction, no per-frame list; only the coverage image accumulates.  Per frame: read_into the pinned buffer, one upload, the frame's
    graph on the Y plane's view of the uploaded buffer (ingest, then the network: stream.step_u8), the planar warp of the uploaded
    buffer by the frame's maps into the fixed output buffer, one download, Y4mWriter.write.  Frame 0 seeds the ring and is written as
    read.  rd: the opened y4m.Y4mReader; out_file: '-' given as the process's real stdout, a path, or None (a dry run).  Everything
    printed goes to stderr.  -> the report that <out>.json holds."""
    import torch
    from stabnet_amd import warp, y4m
    from stabnet_amd.ingest import FrameIngest, lut256_limited
    say = lambda *a: print(*a, file=sys.stderr)
    SH, SW = rd.height, rd.width
    planes = 1 if rd.chroma == 'mono' else 3
    limited = rd.colour_range == 'limited'
    border_y = 16 if limited else 0
    window = warp.ratio_window(SH, SW, args.fill) if args.fill is not None else None
    say('note: --y4m-in: %dx%d C%s frames at %d:%d fps, %s range; the Y plane feeds the %dx%d network, the planes are warped as they are '
        '(taps outside the frame read Y = %d, U = V = 128)' % (SW, SH, rd.chroma, rd.fps[0], rd.fps[1], rd.colour_range, W, H, border_y))
    if window is not None:
        say('note: --fill %g: every written frame is the window (y0, x0, wh, ww) = %s of the stabilised frame, at %dx%d' % (args.fill, list(window), SW, SH))
    ing = FrameIngest(SH, SW, 1, H, W, gray=args.gray_weights, device=dev, lut=lut256_limited() if limited else None)
    pin_in, pin_out = (torch.empty(rd.frame_bytes, dtype=torch.uint8).pin_memory() for _ in range(2))
    dev_in, dev_out = (torch.empty(rd.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(2))
    host_in, host_out = pin_in.numpy(), pin_out.numpy()
    y_view = dev_in[:SH * SW].view(SH, SW)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=dev)
    wr = None
    if out_file is not None:
        wr = y4m.Y4mWriter(out_file, SW, SH, rd.fps, rd.chroma, aspect=rd.aspect, colour_range=rd.colour_range if rd.range_given else None)
    length, tot_time = 0, 0.0
    scene_cuts = [] if args.scene_cut is not None else None                        # --scene-cut: the flagged frames (no per-frame list here)
    try:
        if not rd.read_into(host_in):
            raise y4m.Y4mError('Y4M: the stream holds no frame')
        dev_in.copy_(pin_in)
        stream.start_u8(y_view, ing)                                               # ring = 32 x the first frame
        torch.cuda.synchronize()
        alive = wr is None or wr.write(host_in)                                    # the first frame as read (deploy_bundle.py:215)
        while alive and rd.read_into(host_in):
            dev_in.copy_(pin_in)
            torch.cuda.synchronize()
            start = time.time()
            r = stream.step_u8(y_view, ing)
            warp.warpRevBundle2_i420(dev_in, r['x_map'], r['y_map'], (SH, SW), planes, window=window, border_y=border_y, black_count=black,
                                     out=dev_out, workspace=ws, interp=args.interp)
            torch.cuda.synchronize()
            tot_time += time.time() - start
            if scene_cuts is not None and int(r['scene_cut'][0]):
                scene_note(scene_cuts, length + 1, 1, int(r['scene_dist'].cpu().numpy()[0]), H, W, say)
            pin_out.copy_(dev_out)
            torch.cuda.synchronize()
            alive = wr is None or wr.write(host_out)
            length += 1
            if length % 10 == 0:
                say('length: ' + str(length))
                say('fps={}'.format(length / tot_time))
    finally:
        say('total length={}'.format(length + 2))
        if wr is not None:
            wr.close()
    if wr is not None and wr.broken:
        say('note: the consumer of --y4m-out closed the stream after %d frames' % wr.frames_written)
    report = {'input': rd.header_fields(), 'network_size': [H, W], 'colour_range': rd.colour_range, 'border_y': border_y, 'interp': args.interp,
              'window': [float(v) for v in window] if window is not None else None, 'frames': length + 1,
              'pixels_ever_uncovered': int((black > 0).sum().item()), 'max_uncovered_count': int(black.max().item())}
    if scene_cuts is not None:
        report.update(scene_cuts=[t for t, _, _ in scene_cuts], scene_threshold=args.scene_cut)
    say('y4m: %d frames (the first as read, %d stabilised), fps=%s (the step and the warp), %d of %d luma pixels were uncovered in some frame'
        % (length + 1, length, length / tot_time if tot_time > 0 else 'n/a', report['pixels_ever_uncovered'], SH * SW))
    if wr is not None and isinstance(out_file, str):
        import json
        with open(out_file + '.json', 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')
        say('wrote %s (%d frames) and %s' % (out_file, wr.frames_written, out_file + '.json'))
    return report


def main_y4m(args):
    """--y4m-in: stdout may be the video, so everything the driver prints goes to stderr; a stream that is refused (y4m.Y4mError) ends
    the run with its sentence and a non-zero status, before anything touches the GPU when the header is what is refused."""
    import contextlib
    from stabnet_amd import y4m
    real_stdout = sys.stdout.buffer
    with contextlib.redirect_stdout(sys.stderr):
        try:
            rd = y4m.Y4mReader(args.y4m_in)
        except (y4m.Y4mError, OSError) as e:
            sys.exit('deploy_bundle.py: --y4m-in %s: %s' % (args.y4m_in, e))
        import torch
        stream, H, W, dev = setup_stream(args)
        try:
            run_y4m(args, rd, stream, H, W, dev, real_stdout if args.y4m_out == '-' else args.y4m_out)
        except (y4m.Y4mError, OSError) as e:
            sys.exit('deploy_bundle.py: --y4m-in %s: %s' % (args.y4m_in, e))
        finally:
            rd.close()
            torch.cuda.synchronize()
    if args.y4m_out == '-':
        try:
            real_stdout.flush()
        except BrokenPipeError:
            os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())          # nothing more to say to a closed pipe, at exit either


class AviStreamError(RuntimeError):
    """--avi-in: a sentence that ends the run (a file, a first frame or a later frame that is refused)."""


def avi_probe(args):
    """--avi-in, before the GPU is touched: the opened reader and the parsed header of its first frame, or AviStreamError with the sentence.
    -> (reader, info of mjpeg.parse)"""
    from stabnet_amd import _lib, avi, mjpeg
    try:
        rd = avi.AviMjpegReader(args.avi_in, mapped=True)
    except (avi.AviError, OSError, ValueError) as e:
        raise AviStreamError('%s is not a Motion-JPEG .avi that can be read: %s' % (args.avi_in, e))
    if len(rd) == 0:
        raise AviStreamError('%s holds no frame' % args.avi_in)
    route = 'the test-list route (--decode device, or Pillow) still reads such clips'
    try:
        info = mjpeg.parse(rd.jpeg(0))
    except mjpeg.Unsupported as e:
        raise AviStreamError('the first frame of %s is outside the planar decoder\'s scope (%s); %s' % (args.avi_in, e, route))
    except _lib.StabnetError as e:
        raise AviStreamError('the first frame of %s is no complete baseline JPEG stream (%s)' % (args.avi_in, e))
    why = mjpeg.planar_refusal(info['H'], info['W'], info['C'], info['subsampling'])
    if why:
        raise AviStreamError('the planar decoder does not take the first frame of %s: %s; %s' % (args.avi_in, why, route))
    return rd, info


def run_avi(args, rd, info, stream, H, W, dev, y4m_file, avi_path):
    """--avi-in: the online loop over the frames of a 4:2:0 (or grey) Motion-JPEG .avi, in YCbCr end to end and in bounded memory -- one
    pinned slot and fixed device buffers, no per-frame list; only the coverage image accumulates (the reader keeps two ints per frame).
    Per frame: the compressed bytes (blob + stream, or blob + host coefficients for a clip without restart markers under --entropy auto)
    into the pinned slot and up in one copy; the planes decoded as they are into a fixed buffer (stabnet_mjpeg_decode_i420); the frame's
    graph on the Y plane's view (ingest without a table: JFIF is full range; then the network); the planar warp into the fixed output
    buffer; for --avi-out the planar encoder and the download of the stream's bytes, for --y4m-out the download of the planes.  Frame 0
    seeds the ring and is written as decoded (re-encoded from its planes for the .avi, so that every frame has the run's tables and
    restart interval).  A later frame that is refused ends the run with AviStreamError after the outputs are closed valid.
    -> the report that <out>.json holds."""
    import json
    import torch
    from stabnet_amd import _lib, warp, y4m
    from stabnet_amd.avi import AviMjpegWriter
    from stabnet_amd.ingest import FrameIngest
    from stabnet_amd.mjpeg import MjpegDecoder, MjpegEncoder, default_restart_mcus
    say = lambda *a: print(*a, file=sys.stderr)
    SH, SW, planes = info['H'], info['W'], info['C']
    lanes = info['restart'] != 0
    parallel = not lanes and args.entropy == 'parallel'
    backend = 'restart lanes' if lanes else ('parallel' if parallel else 'host coefficients')
    fps = args.fps if args.fps_given else (rd.rate / rd.scale if rd.rate > 0 and rd.scale > 0 else args.fps)
    rate_scale = (rd.rate, rd.scale) if rd.rate > 0 and rd.scale > 0 else (30, 1)
    window = warp.ratio_window(SH, SW, args.fill) if args.fill is not None else None
    say('note: --avi-in: %d MJPG frames %dx%d (%s) at %.3f fps, entropy decoding: %s; the planes stay YCbCr: the Y plane feeds the %dx%d network, '
        'the planes are warped as they are (taps outside the frame read Y = 0, U = V = 128)'
        % (len(rd), SW, SH, 'grey' if planes == 1 else '4:2:0', rd.fps, backend, W, H))
    if window is not None:
        say('note: --fill %g: every written frame is the window (y0, x0, wh, ww) = %s of the stabilised frame, at %dx%d' % (args.fill, list(window), SW, SH))
    dec = MjpegDecoder(SH, SW, planes, info['subsampling'] or 420, device=dev, host_entropy=not lanes and not parallel, parallel=parallel, planar=True)
    fb = dec.frame_bytes
    ing = FrameIngest(SH, SW, 1, H, W, gray=args.gray_weights, device=dev)
    dev_in, dev_out = (torch.empty((1, fb), dtype=torch.uint8, device=dev) for _ in range(2))
    y_view = dev_in[0, :SH * SW].view(SH, SW)
    ws = torch.empty(2 * (H // 4) * (W // 4), dtype=torch.float32, device=dev)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=dev)
    enc = aw = yw = pin_out = None
    restart = default_restart_mcus(planes, 420)
    if avi_path is not None:
        enc = MjpegEncoder(SH, SW, planes, quality=args.jpeg_quality, restart_mcus=restart, device=dev, planar=True)
        aw = AviMjpegWriter(avi_path, SW, SH, fps)
    if y4m_file is not None:
        yw = y4m.Y4mWriter(y4m_file, SW, SH, rate_scale, 'mono' if planes == 1 else '420jpeg', colour_range='full')
        pin_out = torch.empty(fb, dtype=torch.uint8).pin_memory()

    def decode(t):
        """frame t -> dev_in; StabnetError names the frame"""
        jpeg = rd.jpeg(t)
        need = dec.slot_bytes(len(jpeg))
        if need > dec.in_stride:
            dec._reserve(1, (need + 4095) & ~4095)
        used = dec.stage(jpeg, dec.h_in[0], t)
        dec.d_in[0, :used].copy_(dec.h_in[0, :used], non_blocking=True)
        dec.enqueue(dec.d_in, 1, dev_in, dec.status[:1])
        dec.check(dec.status[:1], t)                                               # (synchronises: the slot is free again)

    def write(frame):
        """the planes of one output frame (device, [1, fb]) to the outputs; False when the consumer of a Y4M pipe has gone"""
        if aw is not None:
            aw.write(enc.encode_bytes(frame)[0])
        if yw is not None:
            pin_out.copy_(frame[0])
            torch.cuda.synchronize()
            return yw.write(pin_out.numpy())
        return True

    length, tot_time, failed = 0, 0.0, None
    scene_cuts = [] if args.scene_cut is not None else None
    try:
        decode(0)
        stream.start_u8(y_view, ing)                                               # ring = 32 x the first frame
        torch.cuda.synchronize()
        alive = write(dev_in)                                                      # the first frame as decoded (deploy_bundle.py:215)
        for t in range(1, len(rd)):
            if not alive:
                break
            try:
                decode(t)
            except _lib.StabnetError as e:
                failed = 'frame %d of %s is refused: %s; the outputs hold the %d frames before it' % (t, args.avi_in, e, t)
                break
            torch.cuda.synchronize()
            start = time.time()
            r = stream.step_u8(y_view, ing)
            warp.warpRevBundle2_i420(dev_in[0], r['x_map'], r['y_map'], (SH, SW), planes, window=window, border_y=0, black_count=black,
                                     out=dev_out[0], workspace=ws, interp=args.interp)
            torch.cuda.synchronize()
            tot_time += time.time() - start
            if scene_cuts is not None and int(r['scene_cut'][0]):
                scene_note(scene_cuts, t, 1, int(r['scene_dist'].cpu().numpy()[0]), H, W, say)
            alive = write(dev_out)
            length += 1
            if length % 10 == 0:
                say('length: ' + str(length))
                say('fps={}'.format(length / tot_time))
    finally:
        say('total length={}'.format(length + 2))
        if aw is not None:
            aw.close()
        if yw is not None:
            yw.close()
    if yw is not None and yw.broken:
        say('note: the consumer of --y4m-out closed the stream after %d frames' % yw.frames_written)
    report = {'input': {'path': args.avi_in, 'width': SW, 'height': SH, 'frames': len(rd), 'rate': rd.rate, 'scale': rd.scale,
                        'sampling': 'grey' if planes == 1 else '420', 'restart': info['restart']},
              'network_size': [H, W], 'colour_range': 'full', 'border_y': 0, 'interp': args.interp,
              'window': [float(v) for v in window] if window is not None else None, 'frames': length + 1,
              'pixels_ever_uncovered': int((black > 0).sum().item()), 'max_uncovered_count': int(black.max().item()),
              'decode_backend': backend, 'jpeg': {'quality': args.jpeg_quality, 'restart_mcus': restart} if aw is not None else None}
    if scene_cuts is not None:
        report.update(scene_cuts=[t for t, _, _ in scene_cuts], scene_threshold=args.scene_cut)
    if failed:
        report['stopped'] = failed
    say('avi: %d frames (the first as decoded, %d stabilised), fps=%s (the step and the warp), %d of %d luma pixels were uncovered in some frame'
        % (length + 1, length, length / tot_time if tot_time > 0 else 'n/a', report['pixels_ever_uncovered'], SH * SW))
    for path in [p for p in (avi_path, y4m_file if isinstance(y4m_file, str) else None) if p is not None][:1]:
        with open(path + '.json', 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')
        say('wrote %s' % (path + '.json'))
    if aw is not None:
        say('wrote %s (%d frames, MJPG q%d 4:2:0 planar, %.3f fps)' % (avi_path, aw.frames_written, args.jpeg_quality, fps))
    if yw is not None and isinstance(y4m_file, str):
        say('wrote %s (%d frames)' % (y4m_file, yw.frames_written))
    if failed:
        raise AviStreamError(failed)
    return report


def main_avi(args):
    """--avi-in: stdout may be the video (--y4m-out -), so everything the driver prints goes to stderr; whatever is refused ends the run
    with its sentence and a non-zero status -- before anything touches the GPU when the file or its first frame is what is refused."""
    import contextlib
    real_stdout = sys.stdout.buffer
    with contextlib.redirect_stdout(sys.stderr):
        try:
            rd, info = avi_probe(args)
        except AviStreamError as e:
            sys.exit('deploy_bundle.py: --avi-in: %s' % e)
        import torch
        from stabnet_amd import _lib, avi, y4m
        stream, H, W, dev = setup_stream(args)
        try:
            run_avi(args, rd, info, stream, H, W, dev, real_stdout if args.y4m_out == '-' else args.y4m_out, args.avi_out)
        except (AviStreamError, avi.AviError, y4m.Y4mError, _lib.StabnetError, OSError) as e:
            sys.exit('deploy_bundle.py: --avi-in: %s' % e)
        finally:
            torch.cuda.synchronize()
    if args.y4m_out == '-':
        try:
            real_stdout.flush()
        except BrokenPipeError:
            os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())          # nothing more to say to a closed pipe, at exit either


def setup_stream(args):
    """The network of a run from the flags: the size, the weights, the stream with its frame graph.  -> (stream, H, W, device)"""
    import torch
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream

    base = Config()
    H, W = args.height or base.height, args.width or base.width
    cfg = Config(height=H, width=W)
    lags = cfg.indices[1:]
    print('inference with {}'.format(list(lags)))
    if args.before_ch is not None and args.before_ch != max(lags):
        print('note: --before-ch %d is ignored (as in the reference); ring depth = %d' % (args.before_ch, max(lags)))
    ignored = [flag for flag, on in (('--max-span', args.max_span != 1), ('--random-black', args.random_black is not None),
                                     ('--no_bm=0', args.no_bm == 0), ('--infer-with-last', args.infer_with_last),
                                     ('--infer-with-stable', args.infer_with_stable),
                                     ('--start-with-stable', args.start_with_stable), ('--deploy-vis', args.deploy_vis)) if on]
    if ignored:
        # --infer-with-stable / --start-with-stable / --deploy-vis read the ground-truth STABLE video (deploy_bundle.py:73,
        # 88-89,237-246,319-320): debugging aids that need the paired clip; with --infer-with-stable the reference also stops
        # appending to before_masks while still popping it (:319-328), i.e. it only runs for 32 frames.
        print('note: %s: debugging paths of the reference that are not on the timed path; accepted and ignored'
              % '/'.join(ignored))
    params = load_weights(args, cfg)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    stream = StabNetStream(params, H, W, cfg, streams=1, device=dev, refine=args.refine, before_ch=args.before_ch,
                           use_graph=True, operand_mode=args.operand_mode)   # one frame = fixed-argument launches: captured once, replayed per frame
    stream.track_black()            # all_black += round(black) inside every refine pass (deploy_bundle.py:234,291), on the device
    if args.scene_cut is not None:
        stream.enable_scene_cut(args.scene_cut, args.scene_gap)
        print('note: --scene-cut %g: a frame whose tile histograms differ from the previous frame\'s by d > %g, %d frames or more after the '
              'last cut, starts a new scene: the history ring is re-seeded with it on the GPU' % (args.scene_cut, args.scene_cut, args.scene_gap))
    return stream, H, W, dev


def main():
    args = parse_args()
    if args.y4m_in is not None:
        return main_y4m(args)
    if args.avi_in is not None:
        return main_avi(args)
    import torch
    from stabnet_amd import synthetic, warp
    stream, H, W, dev = setup_stream(args)

    clips, fps_of = [], {}
    if args.synthetic > 0:
        clips.append(('synthetic', (synthetic.make_clip(H, W, args.synthetic, seed=1234) + 0.5) * 255.0))
    else:
        for lst in args.test_list:
            if not os.path.exists(lst):
                continue
            for name in open(lst).read().splitlines():
                if not name:
                    continue
                path = os.path.join(args.prefix, 'unstable', name)
                if os.path.exists(path) and path.endswith('.npy'):
                    clips.append((name, np.load(path, mmap_mode='r')))
                elif os.path.exists(path + '.npy'):
                    clips.append((name, np.load(path + '.npy', mmap_mode='r')))
                elif os.path.exists(path) and path.lower().endswith('.avi'):
                    from stabnet_amd.avi import AviMjpegReader
                    rd = AviMjpegReader(path)
                    dclip = None
                    if args.decode == 'device':
                        from stabnet_amd.mjpeg import Unsupported
                        try:
                            dclip = rd.device_clip(dev, parallel=args.entropy == 'parallel')
                        except Unsupported as e:
                            print('note: --decode device: %s: %s; this clip is decoded on the host with Pillow' % (path, e))
                    if rd.fps > 0:
                        fps_of[name] = rd.fps
                    if dclip is not None:
                        clips.append((name, dclip))
                        print('read %s: %d MJPG frames %dx%d at %.3f fps, decoded on the GPU frame by frame (%s)'
                              % (path, len(rd), rd.width, rd.height, rd.fps, 'coefficients from the host: the streams have no restart '
                                 'intervals' if dclip.decoder.host_entropy else ('parallel entropy decoding on the GPU: the streams have '
                                 'no restart intervals' if dclip.decoder.parallel else 'one lane per restart interval')))
                        continue
                    clips.append((name, np.stack(list(rd.frames()))))
                    print('read %s: %d MJPG frames %dx%d at %.3f fps, decoded on the host with Pillow (outside the timed part)'
                          % (path, len(rd), rd.width, rd.height, rd.fps))
                else:
                    print('skipping %s: only .npy clips and MJPG .avi files can be read without OpenCV' % path)
    out_dir = os.path.join(args.output_dir, 'output')
    os.makedirs(out_dir, exist_ok=True)

    for name, clip in clips:
        print(name)
        tot_time, length = 0.0, 0
        frames_out, xmaps, ymaps, blacks, colour_out = [], [], [], [], []
        stem = os.path.join(out_dir, os.path.splitext(os.path.basename(name))[0])
        writer, enc, fps = None, None, fps_of.get(name, args.fps)
        ing, black_src = None, None          # black_src: coverage at source size (--output-size source), int32 on the device
        window, black_win, first, source = None, None, None, False      # --fill R: the window, the coverage at its output pixels
        fill, kept = None, (H, W)            # --fill as it applies to this clip; the kept frame's size
        adaptive, fill_params, fill_log = None, None, []     # --fill adaptive: the window's state on the device; (window, stats) per frame
        mosaic, fill_frames = None, []       # --fill history: the canvas of the earlier frames on the device; the filled frames
        scene_log = [] if args.scene_cut is not None else None      # --scene-cut: (frame, cut, d) per frame
        try:
            if args.ingest == 'device':
                shp = np.shape(clip[0])
                if np.asarray(clip[0]).dtype == np.uint8 and (len(shp) == 2 or (len(shp) == 3 and shp[2] in (1, 3))):
                    from stabnet_amd.ingest import FrameIngest
                    ing = FrameIngest(shp[0], shp[1], 1 if len(shp) == 2 else shp[2], H, W, gray=args.gray_weights, device=dev)
                    print('note: --ingest device: %dx%dx%d uint8 frames -> %dx%d on the GPU as the reference\'s cv2/PIL chain '
                          '(cv2.cvtColor %s weights, PIL BILINEAR resize, * (1./255) - 0.5; cv2.resize for the colour frame)'
                          % (ing.sh, ing.sw, ing.C, H, W, args.gray_weights))
                else:
                    print('note: --ingest device reads uint8 frames; this clip is %s %s: converted on the host as with --ingest host'
                          % (np.asarray(clip[0]).dtype, list(shp)))
                    if args.output_size == 'source':
                        print('note: --output-size source needs the uint8 frame on the GPU; this clip is written at the network\'s size')
            source = args.output_size == 'source' and ing is not None
            if source:
                black_src = torch.zeros((ing.sh, ing.sw), dtype=torch.int32, device=dev)
                print('note: --output-size source: frames are written at %dx%d, warped at that size by the %dx%d maps' % (ing.sw, ing.sh, W, H))
            # --fill cuts a remapped frame: the frame as read, or the colour frame at the network's size
            fill = args.fill if ing is not None and (source or ing.C == 3) else None
            kept = (ing.sh, ing.sw) if source else (H, W)
            if args.fill is not None and fill is None:
                print('note: --fill needs a remapped frame to cut; this clip keeps the network\'s grey output and is written as without it')
            elif fill == 'history' and ing.C != 3:
                fill = None
                print('note: --fill history composes colour frames; this clip is grey and is written as without it')
            elif fill == 'history':
                from stabnet_amd.mosaic import Mosaic, MosaicParams
                mosaic = Mosaic(1, kept[0], kept[1], H, W, MosaicParams(feather_log2=args.fill_feather.bit_length() - 1, max_age=args.fill_age),
                                device=dev)
                print('note: --fill history: pixels the stabilised frame does not cover are filled from earlier stabilised frames (at most %d '
                      'frames old, a %d px blend band), at %dx%d; written as %s_fill.npy beside the usual outputs'
                      % (args.fill_age, args.fill_feather, kept[1], kept[0], os.path.basename(stem)))
                if args.score:
                    print('note: --score scores the online frames (the network\'s grey output) as without --fill history, not the filled ones')
            elif fill == 'adaptive':
                # (cubic: one more pixel, so that no 4x4 tap of the window leaves the frame: no darkened rim)
                fill_params = dict(r_min=args.fill_min, up=args.fill_up, margin_q=8 + 32 if args.interp == 'cubic' else 8)
                black_win = torch.zeros(kept, dtype=torch.int32, device=dev)
                if not args.pipeline:
                    adaptive = warp.AdaptiveFill(1, kept[0], kept[1], device=dev, **fill_params)
                print('note: --fill adaptive: every kept frame is the largest centred window of the stabilised frame that shows no uncovered '
                      'pixel (ratio >= %g, growing back by <= %g per frame), chosen on the GPU, at %dx%d'
                      % (args.fill_min, args.fill_up, kept[1], kept[0]))
            elif fill is not None and fill != 'auto':
                window = warp.ratio_window(kept[0], kept[1], fill)
                black_win = torch.zeros(kept, dtype=torch.int32, device=dev)
                print('note: --fill %g: every kept frame is the window (y0, x0, wh, ww) = %s of the stabilised frame, at %dx%d'
                      % (fill, list(window), kept[1], kept[0]))
            if args.mjpg:
                from stabnet_amd.avi import AviMjpegWriter
                from stabnet_amd.mjpeg import MjpegEncoder
                if source:                           # deploy_bundle.py:215 at the frame's own size: cv2.resize is the identity there
                    first = np.ascontiguousarray(clip[0], dtype=np.uint8)
                    first = first[..., 0] if first.ndim == 3 and first.shape[2] == 1 else first
                elif ing is not None:                # deploy_bundle.py:215: the cv2-resized first frame
                    f0 = torch.from_numpy(np.ascontiguousarray(clip[0], dtype=np.uint8)).to(dev)
                    first = (ing.colour(f0)[0] if ing.C == 3 else ((ing.grey(f0)[0] + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)).cpu().numpy()
                else:
                    first = first_frame_u8(clip, H, W)
                oh, ow = first.shape[:2]             # the network's size, or the source's with --output-size source
                enc = MjpegEncoder(oh, ow, 3 if first.ndim == 3 else 1, device=dev, **jpeg_options(args))
                writer = AviMjpegWriter(stem + '.avi', ow, oh, fps)
                writer.write(enc.encode_bytes(torch.from_numpy(first).to(dev))[0])          # deploy_bundle.py:215
            sink = writer.write if writer is not None else None
            if args.pipeline:
                length, tot_time, pipe_black, pipe_win = run_pipelined(stream, clip, H, W, frames_out, colour_out, xmaps, ymaps, blacks, sink,
                                                                       jpeg_options(args) if args.mjpg else None, ing, source,
                                                                       'adaptive' if fill_params else window, fill_params, fill_log, scene_log,
                                                                       args.interp)
                black_src = pipe_black if source else None
                black_win = pipe_win if (window is not None or fill_params) else None
            else:
                length, tot_time = run_serial(stream, clip, H, W, dev, frames_out, colour_out, xmaps, ymaps, blacks, sink, enc, ing, black_src,
                                              window, black_win, adaptive, fill_log, mosaic, fill_frames, scene_log, args.interp)
        except Exception:
            traceback.print_exc()                    # the reference swallows per-video errors and still finalises
        finally:
            print('total length={}'.format(length + 2))
            if writer is not None:
                writer.close()
                print('wrote %s (%d frames, MJPG q%d %s, %.3f fps)' % (stem + '.avi', writer.frames_written, args.jpeg_quality,
                                                                        args.jpeg_subsampling, fps))
            if frames_out:
                np.save(stem + '_stable.npy', np.stack(frames_out))
                if colour_out:
                    np.save(stem + '_stable_bgr.npy', np.stack(colour_out))
                np.savez_compressed(stem + '_maps.npz', x_map=np.stack(xmaps), y_map=np.stack(ymaps), black=np.stack(blacks))
                print('wrote', stem + '_stable.npy')
                if scene_log is not None:
                    write_scenes_json(stem + '_scenes.json', args, scene_log)
                # max-inscribed black-free rectangle over the whole clip (deploy_bundle.py:344-371), searched on the device
                # (--output-size source: over the coverage counted at source size, and the frames are cut there)
                # (--fill R: over the coverage counted at the window's output pixels)
                coverage = black_win if (window is not None or fill_params) and colour_out else (black_src if black_src is not None and colour_out else stream.all_black[0])
                ans, area = warp.max_inscribed_rect(coverage)
                if ans:
                    src = np.stack(colour_out) if colour_out else np.stack(frames_out)
                    cut = src[:, ans[0]:ans[2] + 1, ans[1]:ans[3] + 1]
                    np.save(stem + '_cut.npy', cut)
                    print('crop', ans, 'area', area)
                    if args.mjpg:                    # deploy_bundle.py:366-371: the cropped frames as a second video
                        ch, cw = cut.shape[1], cut.shape[2]
                        cenc = MjpegEncoder(ch, cw, 3 if cut.ndim == 4 else 1, device=dev, **jpeg_options(args))
                        with AviMjpegWriter(stem + '_cut.avi', cw, ch, fps) as wcut:
                            for f in cut:
                                wcut.write(cenc.encode_bytes(torch.from_numpy(np.ascontiguousarray(f)).to(dev))[0])
                        print('wrote %s (%d frames %dx%d)' % (stem + '_cut.avi', len(cut), cw, ch))
                try:
                    if window is not None and colour_out:                # --fill R: what the online window left uncovered
                        f0 = torch.from_numpy(np.ascontiguousarray(colour_out[0])).to(dev)
                        per = uncovered_per_frame(f0, xmaps, ymaps, window, kept, dev)
                        if sum(per) != int(black_win.sum().item()):
                            print('WARNING: the coverage counted online (%d) is not the sum over the frames (%d)' % (int(black_win.sum().item()), sum(per)))
                        write_fill_json(stem, 'ratio', window, None, kept, fill_report(per, kept), int((black_win > 0).sum().item()), args.interp)
                        if tot_time > 0:
                            print('fps={}'.format(length / tot_time))
                    elif fill_params and colour_out:                      # --fill adaptive: each frame recounted through its own window
                        f0 = torch.from_numpy(np.ascontiguousarray(colour_out[0])).to(dev)
                        per = uncovered_per_frame(f0, xmaps, ymaps, [tuple(float(v) for v in w) for w, _ in fill_log], kept, dev)
                        if sum(per) != int(black_win.sum().item()):
                            print('WARNING: the coverage counted online (%d) is not the sum over the frames (%d)' % (int(black_win.sum().item()), sum(per)))
                        write_fill_adaptive_json(stem, fill_params, fill_log, (H // 4) * (W // 4), kept, fill_report(per, kept),
                                                 int((black_win > 0).sum().item()), args.interp)
                        if tot_time > 0:
                            print('fps={}'.format(length / tot_time))
                    elif mosaic is not None and fill_frames:
                        if first is None:
                            first = np.ascontiguousarray(fill_frames[0])      # (only used with --mjpg, which sets it)
                        write_fill_history(stem, mosaic, fill_frames, first, jpeg_options(args), fps, dev, args)
                    elif fill == 'auto' and colour_out:
                        if not ans:
                            print('note: --fill auto: no black-free rectangle in this clip; no _fill files are written')
                        else:
                            fwin = warp.fit_window(ans, kept[0], kept[1])
                            print('fill: window (y0, x0, wh, ww) = %s of the stabilised frame inside the rectangle %s, at %dx%d'
                                  % (list(fwin), ans, kept[1], kept[0]))
                            per = fill_second_pass(clip, ing, source, xmaps, ymaps, fwin, kept, dev, stem, args, fps, first)
                            write_fill_json(stem, 'auto', fwin, ans, kept, fill_report(per, kept), None, args.interp)
                except Exception:
                    traceback.print_exc()
                if args.score:
                    try:
                        score_outputs(clip, frames_out, colour_out, ing, window is not None or bool(fill_params), H, W, dev, stem,
                                      None if scene_log is None else [t for t, cut, _ in scene_log if cut], interp=args.interp)
                    except Exception:
                        traceback.print_exc()


if __name__ == '__main__':
    main()
