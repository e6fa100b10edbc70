"""Host side of the online loop (deploy_bundle.py:183-342, the network + feedback part): an on-device history ring
per stream and ONE C call per frame (StabNetStream); ClipPipeline drives it from a clip in HOST memory with the PCIe copies
of neighbouring frames overlapped, the colour remap (warpRevBundle2) and, when asked for, the JPEG encoding of the stabilised frame
(mjpeg.MjpegEncoder) on the device, and so is the decoding of Motion-JPEG input (mjpeg.MjpegDecoder).  The container (avi.py)
stays on the host."""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch

from . import _lib
from ._tensor import dev_f32, ptr, stream_ptr
from .config import Config, v2_93
from .regressor import Regressor


class Profiler:
    """Per-launch HIP-event records taken inside the library (bench.py roofline leg)."""

    def __init__(self, max_records: int = 65536, device=None):
        self._h = ctypes.c_void_p()
        self.overhead_ms = 0.0
        self.idle_pair_ms = 0.0
        self.offsets_us = {}
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        _lib.call("stabnet_prof_create", ctypes.byref(self._h), max_records)

    @property
    def handle(self):
        return self._h

    def reset(self):
        _lib.call("stabnet_prof_reset", self._h)

    def calibrate(self, n: int = 200) -> float:
        """Median duration (ms) of an event pair with NOTHING between on an idle stream = two hipEventRecords.  Around a kernel
        in a busy stream only about half of it is added to the kernel's own duration (the start event is processed while the
        previous kernel drains): measured against rocprofv3 on every conv kernel of a 720p frame, raw event time - rocprofv3
        time = 2.55 +- 0.1 us with an idle pair of 4.6 us.  The default correction is therefore HALF the idle pair; a
        per-kernel offset table (set_offsets: calibrated against the committed rocprofv3 averages of the same build by
        tools/profile_stamp.py) replaces it where it exists."""
        from ._tensor import stream_ptr
        self.reset()
        saved = (self.overhead_ms, self.offsets_us)
        self.overhead_ms, self.offsets_us = 0.0, {}
        for _ in range(n):
            _lib.call("stabnet_prof_record_empty", self._h, stream_ptr(self.device), device=self.device)
        ms = sorted(r[1] for r in self.records())
        self.reset()
        self.idle_pair_ms = ms[len(ms) // 2]
        self.overhead_ms, self.offsets_us = 0.5 * self.idle_pair_ms, saved[1]
        return self.overhead_ms

    def set_offsets(self, offsets_us: dict):
        """{kernel name: us to subtract from its raw event time} -- kernels not in the table get the default (calibrate())."""
        self.offsets_us = dict(offsets_us or {})

    def offset_ms(self, name: str) -> float:
        if name in self.offsets_us:
            return 1e-3 * self.offsets_us[name]
        return self.overhead_ms

    def records(self, raw: bool = False):
        """[(kernel name, ms, flops, bytes)] -- synchronises the device first.  ms = event time minus the kernel's offset
        (raw=True: the event time itself)."""
        torch.cuda.synchronize()
        L = _lib.lib()
        out = []
        kind, ms, fl, by = ctypes.c_int(), ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
        for i in range(L.stabnet_prof_num_records(self._h)):
            _lib.call("stabnet_prof_record", self._h, i, ctypes.byref(kind), ctypes.byref(ms), ctypes.byref(fl),
                      ctypes.byref(by))
            name = L.stabnet_prof_kind_name(kind.value).decode()
            out.append((name, ms.value if raw else max(ms.value - self.offset_ms(name), 0.0), fl.value, by.value))
        return out

    def records_with_shapes(self):
        recs = self.records()
        shp = (ctypes.c_int * 4)()
        out = []
        for i, r in enumerate(recs):
            _lib.call("stabnet_prof_record_shape", self._h, i, shp)
            out.append(r + (tuple(shp),))
        return out

    def __del__(self):
        try:
            if self._h:
                _lib.lib().stabnet_prof_destroy(self._h)
                self._h = None
        except Exception:
            pass


class StabNetStream:
    """S independent video streams stabilised in lock-step on one GPU.

    step(cur) takes the next unstable frames [S,H,W] (train-normalised grey, [-0.5,0.5]) and returns the tensors the
    reference fetches at deploy_bundle.py:286 -- output_img, black_pix, Hs, x_map, y_map -- plus theta and the fed-back
    frame (img - black).  before_ch is accepted and ignored exactly like the reference (deploy_bundle.py:15,41): the
    ring depth is max(indices[1:])."""

    def __init__(self, params, H: int, W: int, cfg: Config = v2_93, streams: int = 1, device="cuda:0", refine: int = 1,
                 before_ch=None, use_graph: bool = False, bf16_operands=False, operand_mode=None):
        """operand_mode: conv operand mode of the regressor (regressor.Regressor; 4 = packed split kernels, what bench.py and
        deploy_bundle.py run; default 0 = exact f32 MFMA); bf16_operands=True is the older spelling of mode 1."""
        self.cfg, self.H, self.W, self.S, self.refine = cfg, H, W, streams, refine
        self.reg = Regressor(params, streams, H, W, cfg, device, bf16_operands=bf16_operands, operand_mode=operand_mode, fuse_unit_pairs=True)
        dev = self.reg.device
        self.lags = [i for i in cfg.indices[1:] if i > 0]
        self.depth = max(self.lags)
        self._lags_c = (ctypes.c_int * len(self.lags))(*self.lags)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self.frames_ring = f(streams, self.depth, H, W)
        self.masks_ring = f(streams, self.depth, H, W)
        self.theta = f(streams, cfg.n_theta)
        self.out_img = f(streams, H, W, 1)
        self.black = f(streams, H, W)
        self.x_map = f(streams, H, W, 1)
        self.y_map = f(streams, H, W, 1)
        self.Hs = f(streams, cfg.grid_h, cfg.grid_w, 9)
        self.frame_fb = f(streams, H, W)
        self.cur = f(streams, H, W)                       # fixed-address staging buffer of the current frame
        self.head_dev = torch.zeros(2, dtype=torch.int32, device=dev)     # {ring head, ticket}: on the device (graph replay)
        self.all_black = None                             # optional int32 [S,H,W]: += round(black) per refine pass (:291)
        self.use_graph = use_graph
        self._graph = None
        self._graph_u8 = None                             # step_u8's frame graph: ingest launches + the frame
        self.cur_u8 = None                                # fixed-address uint8 staging buffer of the raw frame (step_u8)
        self._ingest = None
        self.scene = None                                 # optional scene.SceneCut: detect cuts and re-seed the ring inside the frame
        self.started = False

    @property
    def head(self) -> int:
        """Ring slot the NEXT frame's push writes (host read-back; synchronises)."""
        return int(self.head_dev[0].item())

    def start(self, first_frame: torch.Tensor):
        first = dev_f32(first_frame, "first_frame").reshape(self.S, self.H, self.W)
        _lib.call("stabnet_ring_init", ptr(self.frames_ring), ptr(self.masks_ring), ptr(first), self.S, self.depth,
                  self.H, self.W, stream_ptr(self.reg.device), device=self.reg.device)
        self.head_dev.zero_()
        if self.all_black is not None:
            self.all_black.zero_()
        if self.scene is not None:
            self.scene.reset()
            self.scene.update(first)                      # seen == 0: no flag; the next frame is compared with this one
        self.started = True

    def track_black(self, enable: bool = True):
        """Accumulate all_black (deploy_bundle.py:234,291) on the device for the crop search; reset by start()."""
        self.all_black = (torch.zeros((self.S, self.H, self.W), dtype=torch.int32, device=self.reg.device) if enable else None)
        self._graph = self._graph_u8 = None
        return self.all_black

    def enable_scene_cut(self, threshold: float = 0.35, min_gap: int = 8):
        """Detect scene cuts on the device and re-seed the ring inside the frame (scene.SceneCut, csrc/scene.hip): in front of every
        frame, stabnet_scene_update compares the incoming frame's tile histograms with the previous frame's, and
        stabnet_ring_reseed_if turns the ring of a flagged stream into 32 x that frame with zero masks; the frame is then stabilised
        like any other, so the run from a cut on equals a fresh run that starts there with its first frame doubled.  step() then also
        returns "scene_cut" (int32 [S]) and "scene_dist" (uint32 [S], D; d = D / (2*H*W)), device tensors.  all_black is not zeroed
        at a cut.  threshold in (0, 1], min_gap >= 0 frames since the last cut (or the start); reset by start()."""
        from .scene import SceneCut
        self.scene = SceneCut(self.S, self.H, self.W, threshold, min_gap, device=self.reg.device)
        self._graph = self._graph_u8 = None
        return self.scene

    def _outputs(self):
        out = {"output": self.out_img, "black_pix": self.black, "Hs": self.Hs, "x_map": self.x_map,
               "y_map": self.y_map, "theta": self.theta, "frame": self.frame_fb}
        if self.scene is not None:
            out["scene_cut"], out["scene_dist"] = self.scene.flag, self.scene.dist
        return out

    def _enqueue(self, prof=None, cur=None):
        """One frame on the current stream.  cur: the frame to read instead of the fixed staging buffer self.cur (ClipPipeline hands
        its upload slot over directly)."""
        r = self.reg
        if self.scene is not None:
            # the cut decision and the predicated reseed read the frame stabnet_deploy_frame is about to read
            frame = ptr(self.cur if cur is None else cur)
            self.scene.enqueue(frame)
            _lib.call("stabnet_ring_reseed_if", ptr(self.frames_ring), ptr(self.masks_ring), frame, self.S, self.depth, self.H, self.W,
                      ptr(self.scene.flag), stream_ptr(r.device), device=r.device)
        _lib.call("stabnet_deploy_frame", r.plan.handle, ptr(r.params), ptr(r.fold), ptr(self.frames_ring),
                  ptr(self.masks_ring), self.depth, ptr(self.head_dev), self._lags_c, len(self.lags), ptr(self.cur if cur is None else cur),
                  self.refine, self.cfg.grid_h, self.cfg.grid_w, self.cfg.do_crop_rate, ptr(self.theta), ptr(self.out_img),
                  ptr(self.black), ptr(self.x_map), ptr(self.y_map), ptr(self.Hs), ptr(self.frame_fb), ptr(self.all_black),
                  ptr(r.workspace), r.workspace.numel(), stream_ptr(r.device), prof.handle if prof is not None else 0,
                  device=r.device)

    def step(self, cur: torch.Tensor, prof: Profiler = None):
        if not self.started:
            raise _lib.StabnetError("StabNetStream.step before start(first_frame)")
        self.cur.copy_(dev_f32(cur, "cur").reshape(self.S, self.H, self.W))            # D2D into the fixed buffer
        if self.use_graph and prof is None:
            if self._graph is None:
                # one frame = ~95 launches with fixed arguments: capture once, replay per frame (hipGraph)
                self._enqueue()                  # this frame runs eagerly (also loads modules / sets kernel attributes)
                torch.cuda.synchronize()
                try:
                    with torch.cuda.device(self.reg.device):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):    # capture records only; nothing executes here
                            self._enqueue()
                    self._graph = g
                except Exception as e:               # capture unsupported on this runtime: stay eager, say so once
                    import sys
                    print("StabNetStream: hipGraph capture failed (%s); continuing without a graph" % e, file=sys.stderr)
                    self.use_graph = False
            else:
                self._graph.replay()
        else:
            self._enqueue(prof)
        return self._outputs()

    def _bind_ingest(self, ingest):
        if (ingest.H, ingest.W) != (self.H, self.W) or ingest.device != self.reg.device:
            raise _lib.StabnetError("StabNetStream: ingest produces %dx%d on %s, the stream runs %dx%d on %s"
                                    % (ingest.H, ingest.W, ingest.device, self.H, self.W, self.reg.device))
        if ingest is not self._ingest:
            self._ingest, self._graph_u8 = ingest, None
            self.cur_u8 = torch.empty((self.S, ingest.sh, ingest.sw, ingest.C), dtype=torch.uint8, device=self.reg.device)
            ingest._reserve(self.S)

    def _stage_u8(self, frame_u8, ingest, what):
        self._bind_ingest(ingest)
        if not isinstance(frame_u8, torch.Tensor) or not frame_u8.is_cuda or frame_u8.dtype != torch.uint8:
            raise _lib.StabnetError("%s: expected a uint8 tensor on the GPU (there is no CPU fallback)" % what)
        if frame_u8.numel() != self.cur_u8.numel():
            raise _lib.StabnetError("%s: expected %s, got %s" % (what, list(self.cur_u8.shape), list(frame_u8.shape)))
        self.cur_u8.copy_(frame_u8.reshape(self.cur_u8.shape))                         # D2D into the fixed buffer

    def start_u8(self, frame_u8: torch.Tensor, ingest):
        """start() from the raw first frames: uint8 [S,src_h,src_w,C] as read from the video; `ingest` (ingest.FrameIngest) converts
        them on the device (cvt_img2train, config.py:6-21) straight into the staging buffer the ring is seeded from."""
        self._stage_u8(frame_u8, ingest, "start_u8")
        ingest.grey(self.cur_u8, out=self.cur)
        self.start(self.cur)

    def _enqueue_u8(self, prof=None):
        self._ingest.grey(self.cur_u8, out=self.cur, prof=prof)
        self._enqueue(prof)

    def step_u8(self, frame_u8: torch.Tensor, ingest, prof: Profiler = None):
        """step() from the raw frames: the ingest launches write the grey frame into self.cur in front of the frame's own launches;
        with use_graph they are captured with it and read the fixed uint8 staging buffer self.cur_u8."""
        if not self.started:
            raise _lib.StabnetError("StabNetStream.step_u8 before start_u8(first_frame, ingest)")
        self._stage_u8(frame_u8, ingest, "step_u8")
        if self.use_graph and prof is None:
            if self._graph_u8 is None:
                self._enqueue_u8()                   # this frame runs eagerly (also loads modules / sets kernel attributes)
                torch.cuda.synchronize()
                try:
                    with torch.cuda.device(self.reg.device):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):    # capture records only; nothing executes here
                            self._enqueue_u8()
                    self._graph_u8 = g
                except Exception as e:               # capture unsupported on this runtime: stay eager, say so once
                    import sys
                    print("StabNetStream: hipGraph capture failed (%s); continuing without a graph" % e, file=sys.stderr)
                    self.use_graph = False
            else:
                self._graph_u8.replay()
        else:
            self._enqueue_u8(prof)
        return self._outputs()


class ClipPipeline:
    """A clip that lives in HOST memory through one StabNetStream, with upload, frame and download on three HIP streams.

    The reference's loop (deploy_bundle.py:244-342) is strictly serial per frame: feed the frame, `sess.run`, `cv2.remap` the colour
    frame, write it.  The frame itself is recurrent (frame t reads what frame t-1 fed back through the ring), so frames cannot overlap
    each other -- but their PCIe traffic can hide behind the neighbours' compute: while frame t is on the compute stream, frame t+1
    (grey float32 + colour uint8, 6.4 MB at 720p) is uploaded from pinned memory on a second stream and the results of frame t-1
    (stabilised colour frame + the network's grey output, 3.7 MB) are downloaded on a third.  `slots` (>= 2) staging buffers per
    direction; events order the three streams, the host only blocks when it reuses a slot.  Results are the same bytes the serial
    loop produces (tests/test_pipeline_gpu.py).

    run(grey, bgr=None, sink=None, maps=False): grey = sequence of host float32 [H,W] frames in the training normalisation, frame 0 seeds
    the ring (deploy_bundle.py:206-222); bgr = matching uint8 [H,W,3] frames or None.  Per processed frame t >= 1 the host gets
    {"t", "output" uint8 [H,W], "bgr" uint8 [H,W,3] (if bgr), "x_map"/"y_map"/"black" (if maps)}: passed to `sink` as views of pinned
    staging memory that stay valid until the sink returns, or -- without a sink -- copied and returned as a list.

    jpeg=dict(quality=.., subsampling=.., restart_mcus=..): every slot's frame graph also encodes the stabilised frame (the BGR frame
    when colour, else the grey output) as a baseline JPEG (csrc/mjpeg.hip) and the result carries "jpeg" (uint8 view of pinned memory,
    valid until the sink returns).  run(..., raw=False) then skips the raw downloads ("output" / "bgr" are absent): what crosses PCIe
    per frame is the compressed frame.  Its length is only known on the device, so the download is a FIXED first chunk (jpeg_chunk
    bytes: a quarter of the raw frame, several times a q75 frame) together with the length; the rare frame that is longer gets the
    rest by a second, synchronous copy when it is handed over.

    ingest=FrameIngest: the clip is the RAW one -- run(frames_u8, ...), uint8 [src_h,src_w,C] frames of any size as read from the
    video.  A slot then uploads ONE uint8 frame at source size, and the slot's frame graph starts with the ingest launches
    (csrc/ingest.hip: grey conversion + Pillow resize into the stream's staging buffer; cv2.resize of the colour frame, which the
    remap then reads).  The host converts nothing.

    output="source" (needs ingest): the frame that is kept is the frame AS READ, warped at its own size by the network-size maps
    (csrc/remap.hip, stabnet_warp_rev_bundle2_src) -- the slot's graph then has no colour resize and remaps the upload slot itself.
    "bgr" is uint8 [src_h,src_w,3] ([src_h,src_w] for a grey source, colour=False) and "jpeg" its encoding; all_black_src (int32
    [src_h,src_w], zeroed by run) counts per pixel the frames that did not cover it, for warp.max_inscribed_rect.  "output", the maps
    and the stream's all_black stay at the network's size.  The default, "network", is the reference's order: resize, then remap.

    window=(y0, x0, wh, ww) (warp.ratio_window / warp.fit_window), in pixel-edge units of the kept frame: borderless output.  The kept
    frame is that window of the stabilised frame, zoomed to the kept frame's own size in the remap's one gather (csrc/remap.hip,
    stabnet_warp_rev_bundle2_win, where the slot's graph calls the remap today) -- the frame, its JPEG and every buffer keep their
    sizes.  all_black_win (int32, the kept frame's size, zeroed by run) counts per OUTPUT pixel the frames that did not cover it;
    all_black_src is then not updated.  A pipeline that keeps no remapped frame (colour=False at the network's size) refuses it.

    window='adaptive', fill=dict(r_min=0.5, up=0.002, margin_q=8): the window is chosen per frame ON THE DEVICE, inside the slot's
    graph: stabnet_fill_window_update (the largest centred window that reads no uncovered small-map node, zooming in at once and back
    out by `up` per frame, never below r_min) writes the slot's 32-byte window, and stabnet_warp_rev_bundle2_win_dev reads it from
    there -- both on the stream that carries the frame's launches, so the ratio advances in frame order; no host round trip.  The
    result carries "window" (float64 [4]: y0, x0, wh, ww) and "fill_stats" (int32 [2]: key, bad nodes; r_safe = key / (h * w), 1 if
    key >= h * w), downloaded with the slot's other outputs; all_black_win counts as with a fixed window.

    decoder=mjpeg.MjpegDecoder (needs ingest): the clip is a Motion-JPEG one -- run(clip, ...) with clip.jpeg(t) the compressed frame
    (mjpeg.DeviceClip).  A slot then uploads the compressed bytes and their parsed description in one copy on the upload stream, and
    the slot's frame graph starts with the decode launches (csrc/mjpeg_decode.hip) into the buffer the ingest reads.  The frame's
    status word comes down with its outputs; a frame that does not decode raises StabnetError naming it.

    A stream with enable_scene_cut(): the detector's launches and the predicated reseed come with stream._enqueue inside every slot's
    graph, its state advancing in frame order on the run stream; the frame's 8 bytes {flag, D} are copied into the slot inside the
    graph and downloaded with the slot's other outputs: the result carries "scene_cut" (0 / 1) and "scene_dist" (D; d = D / (2*H*W)).

    interp="cubic": wherever the slot's graph calls the remap, it calls stabnet_warp_rev_bundle2_cubic (cv2.remap's INTER_CUBIC, 16 taps)
    with the same frame, maps, window and coverage count; the default "linear" is the reference's INTER_LINEAR."""

    def __init__(self, stream: StabNetStream, colour: bool = True, slots: int = 3, rate: int = 4, jpeg=None, ingest=None,
                 output: str = "network", window=None, fill=None, decoder=None, interp: str = "linear"):
        if stream.S != 1:
            raise _lib.StabnetError("ClipPipeline: one video stream per pipeline")
        from .warp import check_interp
        self.cubic = check_interp(interp, "ClipPipeline")
        if slots < 2:
            raise _lib.StabnetError("ClipPipeline: slots must be >= 2")
        if output not in ("network", "source"):
            raise _lib.StabnetError("ClipPipeline: output must be 'network' or 'source', got %r" % (output,))
        if output == "source":
            if ingest is None:
                raise _lib.StabnetError("ClipPipeline: output='source' needs ingest=FrameIngest: the raw frame must lie on the device")
            if not colour and ingest.C != 1:
                raise _lib.StabnetError("ClipPipeline: output='source' with colour=False needs a grey source, the ingest reads %d channels" % ingest.C)
        self.st, self.colour, self.slots, self.rate = stream, colour, slots, rate
        self.src_out = output == "source"
        self.window = None
        self.windowed = window is not None
        self.adaptive = isinstance(window, str)
        if self.adaptive and window != "adaptive":
            raise _lib.StabnetError("ClipPipeline: window must be (y0, x0, wh, ww) or 'adaptive', got %r" % (window,))
        if fill is not None and not self.adaptive:
            raise _lib.StabnetError("ClipPipeline: fill=... belongs to window='adaptive'")
        if window is not None:
            if output != "source" and not colour:
                raise _lib.StabnetError("ClipPipeline: window needs a remapped frame to cut (colour=True or output='source'); "
                                        "this pipeline keeps the network's grey output")
            kh, kw = (ingest.sh, ingest.sw) if output == "source" else (stream.H, stream.W)
        if self.adaptive:
            from .warp import check_fill_params
            try:
                self.fill = check_fill_params(SH=kh, SW=kw, **(fill or {}))
            except (TypeError, ValueError) as e:
                raise _lib.StabnetError("ClipPipeline: %s" % e)
        elif window is not None:
            try:
                win = tuple(float(v) for v in window)
            except (TypeError, ValueError):
                win = ()
            if len(win) != 4 or not all(np.isfinite(win)) or win[2] <= 0 or win[3] <= 0 or min(win[:2]) < -1e-6 \
                    or win[0] + win[2] > kh + 1e-6 or win[1] + win[3] > kw + 1e-6:
                raise _lib.StabnetError("ClipPipeline: window must be (y0, x0, wh, ww) inside the %dx%d kept frame, got %r" % (kh, kw, window))
            self.window = (ctypes.c_double * 4)(*win)
        dev = stream.reg.device
        H, W = stream.H, stream.W
        self.dev = dev
        pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
        on = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.ingest = ingest
        if ingest is not None:
            if colour and ingest.C != 3:
                raise _lib.StabnetError("ClipPipeline: colour=True needs a BGR source, the ingest reads %d channel(s)" % ingest.C)
            stream._bind_ingest(ingest)
            src = (ingest.sh, ingest.sw, ingest.C)
            if decoder is None:
                self.h_u8 = [pin(src, torch.uint8) for _ in range(slots)]
            self.d_u8 = [on((1,) + src, torch.uint8) for _ in range(slots)]
        else:
            self.h_grey = [pin((H, W), torch.float32) for _ in range(slots)]
            self.d_grey = [on((1, H, W), torch.float32) for _ in range(slots)]
        self.h_out = [pin((H, W), torch.uint8) for _ in range(slots)]
        self.d_out = [on((H, W), torch.uint8) for _ in range(slots)]
        if self.src_out:
            # the warped frame has the source's shape; h_warp drops the channel axis of a grey source
            self.h_warp = [pin(src if ingest.C == 3 else src[:2], torch.uint8) for _ in range(slots)]
            self.d_warp = [on((1,) + src, torch.uint8) for _ in range(slots)]
            self.remap_ws = on((2 * (H // rate) * (W // rate),), torch.float32)
            self.all_black_src = torch.zeros(src[:2], dtype=torch.int32, device=dev)
        elif colour:
            if ingest is None:
                self.h_bgr = [pin((H, W, 3), torch.uint8) for _ in range(slots)]
            self.d_bgr = [on((1, H, W, 3), torch.uint8) for _ in range(slots)]
            self.h_warp = [pin((H, W, 3), torch.uint8) for _ in range(slots)]
            self.d_warp = [on((1, H, W, 3), torch.uint8) for _ in range(slots)]
            self.remap_ws = on((2 * (H // rate) * (W // rate),), torch.float32)
        if self.windowed:
            self.all_black_win = torch.zeros(src[:2] if self.src_out else (H, W), dtype=torch.int32, device=dev)
        if self.adaptive:
            # the ratio of the previous frame (one per pipeline: frames run in order on s_run); per slot the frame's window (4 doubles)
            # and stats (2 ints) in one 40-byte buffer, so that they come down in one copy
            self.fill_state = torch.ones(1, dtype=torch.float64, device=dev)
            self.d_fill = [on((40,), torch.uint8) for _ in range(slots)]
            self.h_fill = [pin((40,), torch.uint8) for _ in range(slots)]
            self.d_win = [b[:32].view(torch.float64) for b in self.d_fill]
            self.d_stats = [b[32:].view(torch.int32) for b in self.d_fill]
        self.decoder = decoder
        if decoder is not None:
            if ingest is None or (decoder.H, decoder.W, decoder.C) != (ingest.sh, ingest.sw, ingest.C):
                raise _lib.StabnetError("ClipPipeline: decoder=... needs ingest=FrameIngest of the decoder's frame size and channels")
            self.h_jin = [pin((decoder.in_stride,), torch.uint8) for _ in range(slots)]
            self.d_jin = [on((1, decoder.in_stride), torch.uint8) for _ in range(slots)]
            self.d_jstat = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(slots)]
            self.h_jstat = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(slots)]
        self.enc = None
        if jpeg is not None:
            from .mjpeg import MjpegEncoder
            eh, ew, C = (ingest.sh, ingest.sw, ingest.C) if self.src_out else (H, W, 3 if colour else 1)
            self.enc = MjpegEncoder(eh, ew, C, device=dev, **jpeg)
            mb = self.enc.max_bytes
            self.jpeg_chunk = min(mb, (eh * ew * C // 4 + 4095) & ~4095)
            self.d_jpeg = [on((1, mb), torch.uint8) for _ in range(slots)]
            self.d_jlen = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(slots)]
            self.h_jpeg = [pin((mb,), torch.uint8) for _ in range(slots)]
            self.h_jlen = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(slots)]
        self.h_maps = None
        self.h_scene = None                                   # per slot {flag, D} of a stream with enable_scene_cut(): made by run()
        self.use_graph = True
        self._graphs = {}
        self.s_in, self.s_run, self.s_out = (torch.cuda.Stream(device=dev) for _ in range(3))
        self.ev_up = [torch.cuda.Event() for _ in range(slots)]
        self.ev_run = [torch.cuda.Event() for _ in range(slots)]
        self.ev_down = [torch.cuda.Event() for _ in range(slots)]

    def _frame(self, k: int, maps: bool):
        """Everything frame-shaped of slot k on the current stream: the frame, its results into the slot's buffers."""
        st, H, W = self.st, self.st.H, self.st.W
        if self.decoder is not None:
            # the compressed frame in the upload slot -> the raw frame, where an uploaded one would lie
            self.decoder.enqueue(self.d_jin[k], 1, self.d_u8[k], self.d_jstat[k])
        if self.ingest is not None:
            # cvt_img2train (config.py:6-21) and cv2.resize (deploy_bundle.py:303) of the raw frame in the upload slot
            self.ingest.grey(self.d_u8[k], out=st.cur)
            if self.colour and not self.src_out:
                self.ingest.colour(self.d_u8[k], out=self.d_bgr[k])
            st._enqueue()
        else:
            st._enqueue(cur=self.d_grey[k])                  # the frame reads the upload slot itself: no staging copy
        if st.scene is not None:
            self.d_scene[k].copy_(st.scene.out)              # this frame's {flag, D}: the next frame overwrites the detector's own
        # cvt_train2img (deploy_bundle.py:75)
        _lib.call("stabnet_cvt_train2img", ptr(st.out_img), ptr(self.d_out[k]), H * W, stream_ptr(self.dev), device=self.dev)
        if self.windowed:
            # the window of the stabilised frame, zoomed to the kept frame's size in the remap's gather; coverage counted at the output
            if self.src_out:
                frame, (sh, sw, C) = self.d_u8[k], (self.ingest.sh, self.ingest.sw, self.ingest.C)
            else:
                frame, (sh, sw, C) = self.d_bgr[k], (H, W, 3)
            entry, win = "stabnet_warp_rev_bundle2_win", self.window
            if self.adaptive:
                # this frame's window, chosen on the device from its maps and the previous frame's ratio; the remap loads it from there
                r_min, up, margin_q = self.fill
                _lib.call("stabnet_fill_window_update", ptr(st.x_map), ptr(st.y_map), 1, H, W, self.rate, sh, sw, r_min, up, margin_q,
                          ptr(self.fill_state), ptr(self.d_win[k]), ptr(self.d_stats[k]), ptr(self.remap_ws), stream_ptr(self.dev),
                          device=self.dev)
                entry, win = entry + "_dev", ptr(self.d_win[k])
            if self.cubic:
                _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(frame), 1, sh, sw, C, sw * C, ptr(st.x_map), ptr(st.y_map), H, W, self.rate,
                          2 if self.adaptive else 1, win, sh, sw, ptr(self.d_warp[k]), ptr(self.all_black_win), ptr(self.remap_ws), 0, 0,
                          stream_ptr(self.dev), 0, device=self.dev)
            else:
                _lib.call(entry, ptr(frame), 1, sh, sw, C, sw * C, ptr(st.x_map), ptr(st.y_map), H, W, self.rate,
                          win, sh, sw, ptr(self.d_warp[k]), ptr(self.all_black_win), ptr(self.remap_ws), 0, 0, stream_ptr(self.dev), 0,
                          device=self.dev)
        elif self.src_out:
            # the raw frame in the upload slot, warped at its own size by the network-size maps; coverage counted on the way
            ing = self.ingest
            if self.cubic:
                _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(self.d_u8[k]), 1, ing.sh, ing.sw, ing.C, ing.sw * ing.C, ptr(st.x_map),
                          ptr(st.y_map), H, W, self.rate, 0, None, ing.sh, ing.sw, ptr(self.d_warp[k]), ptr(self.all_black_src),
                          ptr(self.remap_ws), 0, 0, stream_ptr(self.dev), 0, device=self.dev)
            else:
                _lib.call("stabnet_warp_rev_bundle2_src", ptr(self.d_u8[k]), 1, ing.sh, ing.sw, ing.C, ing.sw * ing.C, ptr(st.x_map),
                          ptr(st.y_map), H, W, self.rate, ptr(self.d_warp[k]), ptr(self.all_black_src), ptr(self.remap_ws), 0, 0,
                          stream_ptr(self.dev), 0, device=self.dev)
        elif self.colour and self.cubic:
            _lib.call("stabnet_warp_rev_bundle2_cubic", ptr(self.d_bgr[k]), 1, H, W, 3, W * 3, ptr(st.x_map), ptr(st.y_map), H, W, self.rate,
                      0, None, H, W, ptr(self.d_warp[k]), None, ptr(self.remap_ws), 0, 0, stream_ptr(self.dev), 0, device=self.dev)
        elif self.colour:
            _lib.call("stabnet_warp_rev_bundle2", ptr(self.d_bgr[k]), ptr(st.x_map), ptr(st.y_map), 1, H, W, 3, self.rate,
                      ptr(self.d_warp[k]), ptr(self.remap_ws), 0, 0, stream_ptr(self.dev), device=self.dev)
        if self.enc is not None:
            self.enc.encode(self.d_warp[k] if (self.colour or self.src_out) else self.d_out[k], out=self.d_jpeg[k], nbytes=self.d_jlen[k])
        if maps:
            self.d_maps[0][k].copy_(st.x_map.view(H, W)); self.d_maps[1][k].copy_(st.y_map.view(H, W))
            self.d_maps[2][k].copy_(st.black.view(H, W))

    def _capture(self, k: int, maps: bool):
        try:
            with torch.cuda.device(self.dev):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._frame(k, maps)
            return g
        except Exception as e:                       # capture unsupported on this runtime: stay eager, say so once
            import sys
            print("ClipPipeline: hipGraph capture failed (%s); continuing without graphs" % e, file=sys.stderr)
            self.use_graph = False
            return None

    def _result(self, slot: int, t: int, maps: bool, raw: bool = True):
        r = {"t": t}
        if self.decoder is not None:
            self.decoder.check(self.h_jstat[slot], t)
        if raw:
            r["output"] = self.h_out[slot].numpy()
            if self.colour or self.src_out:
                r["bgr"] = self.h_warp[slot].numpy()
        if self.enc is not None:
            n = int(self.h_jlen[slot][0])
            if n > self.jpeg_chunk:                           # longer than the chunk that came with the length: fetch the rest now
                with torch.cuda.stream(self.s_out):
                    self.h_jpeg[slot][self.jpeg_chunk:n].copy_(self.d_jpeg[slot][0, self.jpeg_chunk:n], non_blocking=True)
                self.s_out.synchronize()
            self.jpeg_bytes_down += max(n, self.jpeg_chunk) + 4
            r["jpeg"] = self.h_jpeg[slot].numpy()[:n]
        if maps:
            r["x_map"], r["y_map"], r["black"] = (m[slot].numpy() for m in self.h_maps)
        if self.adaptive:
            r["window"] = self.h_fill[slot][:32].view(torch.float64).numpy()
            r["fill_stats"] = self.h_fill[slot][32:].view(torch.int32).numpy()
        if self.st.scene is not None:
            r["scene_cut"], r["scene_dist"] = int(self.h_scene[slot][0]), int(self.h_scene[slot][1]) & 0xffffffff
        return r

    def run(self, grey, bgr=None, sink=None, maps: bool = False, raw: bool = True):
        st, H, W, K = self.st, self.st.H, self.st.W, self.slots
        if not raw and self.enc is None:
            raise _lib.StabnetError("ClipPipeline.run: raw=False needs a pipeline built with jpeg=...: nothing would come back")
        self.jpeg_bytes_down = 0
        if self.colour and bgr is None and self.ingest is None:
            raise _lib.StabnetError("ClipPipeline.run: this pipeline was built with colour=True, bgr frames are required")
        if maps and self.h_maps is None:
            self.h_maps = tuple([torch.empty((H, W), dtype=dt, pin_memory=True) for _ in range(K)]
                                for dt in (torch.float32, torch.float32, torch.uint8))
            self.d_maps = tuple([torch.empty((H, W), dtype=dt, device=self.dev) for _ in range(K)]
                                for dt in (torch.float32, torch.float32, torch.uint8))
        if st.scene is not None and self.h_scene is None:
            self.h_scene = [torch.zeros(2, dtype=torch.int32).pin_memory() for _ in range(K)]
            self.d_scene = [torch.zeros(2, dtype=torch.int32, device=self.dev) for _ in range(K)]
        results = []
        emit = sink if sink is not None else (lambda r: results.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}))
        n = len(grey)
        self.host_wait_s = 0.0                                # time the host spent blocked on a slot: ~0 means the HOST is the bound
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(self.s_run):
            if self.ingest is not None:
                if self.decoder is not None:
                    first = self.decoder.decode([grey.jpeg(0)])[0]
                else:
                    first = torch.from_numpy(np.ascontiguousarray(grey[0], dtype=np.uint8)).to(self.dev)
                st.start_u8(first, self.ingest)
                if self.src_out:
                    self.all_black_src.zero_()
            else:
                first = torch.from_numpy(np.ascontiguousarray(grey[0], dtype=np.float32)).to(self.dev)
                st.start(first[None])
            if self.windowed:
                self.all_black_win.zero_()
            if self.adaptive:
                self.fill_state.fill_(1.0)
        pending = [None] * K                                  # frame number whose results sit in (or are on their way to) slot k
        for t in range(1, n):
            k = t % K
            if pending[k] is not None:                        # slot reuse: its download must have landed; hand the frame over
                w0 = time.perf_counter()
                self.ev_down[k].synchronize()
                self.host_wait_s += time.perf_counter() - w0
                emit(self._result(k, pending[k], maps, raw))
                pending[k] = None
            if self.decoder is not None:
                used = self.decoder.stage(grey.jpeg(t), self.h_jin[k], frame=t)
            elif self.ingest is not None:
                self.h_u8[k].numpy()[...] = np.asarray(grey[t]).reshape(self.h_u8[k].shape)
            else:
                self.h_grey[k].numpy()[...] = grey[t]
                if self.colour:
                    self.h_bgr[k].numpy()[...] = bgr[t]
            with torch.cuda.stream(self.s_in):
                if self.decoder is not None:
                    self.d_jin[k][0, :used].copy_(self.h_jin[k][:used], non_blocking=True)
                elif self.ingest is not None:
                    self.d_u8[k].copy_(self.h_u8[k].view(self.d_u8[k].shape), non_blocking=True)
                else:
                    self.d_grey[k].copy_(self.h_grey[k].view(1, H, W), non_blocking=True)
                if self.colour and self.ingest is None:
                    self.d_bgr[k].copy_(self.h_bgr[k].view(1, H, W, 3), non_blocking=True)
                self.ev_up[k].record(self.s_in)
            with torch.cuda.stream(self.s_run):
                self.s_run.wait_event(self.ev_up[k])
                key = (k, maps, ptr(st.all_black)) if st.scene is None else (k, maps, ptr(st.all_black), ptr(st.scene.out))
                g = self._graphs.get(key)
                if g is not None:
                    g.replay()
                else:
                    # first use of this slot: the frame runs eagerly, then the same launches are RECORDED (nothing executes during a
                    # capture) into the slot's own hipGraph: in steady state a frame is one graph launch per slot, no eager kernels
                    self._frame(k, maps)
                    if self.use_graph:
                        self._graphs[key] = self._capture(k, maps)
                self.ev_run[k].record(self.s_run)
            with torch.cuda.stream(self.s_out):
                self.s_out.wait_event(self.ev_run[k])
                if raw:
                    self.h_out[k].copy_(self.d_out[k], non_blocking=True)
                    if self.colour or self.src_out:
                        self.h_warp[k].copy_(self.d_warp[k].view(self.h_warp[k].shape), non_blocking=True)
                if self.enc is not None:
                    self.h_jlen[k].copy_(self.d_jlen[k], non_blocking=True)
                    self.h_jpeg[k][:self.jpeg_chunk].copy_(self.d_jpeg[k][0, :self.jpeg_chunk], non_blocking=True)
                if maps:
                    for h, d in zip(self.h_maps, self.d_maps):
                        h[k].copy_(d[k], non_blocking=True)
                if self.decoder is not None:
                    self.h_jstat[k].copy_(self.d_jstat[k], non_blocking=True)
                if self.adaptive:
                    self.h_fill[k].copy_(self.d_fill[k], non_blocking=True)
                if st.scene is not None:
                    self.h_scene[k].copy_(self.d_scene[k], non_blocking=True)
                self.ev_down[k].record(self.s_out)
            pending[k] = t                                    # (the slot's next upload follows the host's wait on ev_down[k])
        order = sorted((p, k) for k, p in enumerate(pending) if p is not None)
        for p, k in order:
            self.ev_down[k].synchronize()
            emit(self._result(k, p, maps, raw))
        torch.cuda.synchronize(self.dev)
        return results if sink is None else None
