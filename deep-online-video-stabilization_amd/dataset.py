"""The reference's dataset on the device: get_data_mini_after.read_and_decode (get_data_mini_after.py:158-226) up to its random
operations.  TFRecord files of tf.train.Example (stabnet_amd/tfrecord.py) name two folders of numbered JPEG frames and a position;
the frames are decoded by MjpegDecoder (csrc/mjpeg_decode.hip), turned into the channels of stable [N,H,W,14] / unstable [N,H,W,2] by
one stabnet_tf_get_img launch each (csrc/tf_image.hip), and the batch goes to data.augment_pairs as synthetic.make_raw_pairs' does.

Threads: worker threads only read files, parse streams, run the host entropy decoder (or Pillow, for streams the device decoder
does not take) and fill pinned slots.  Every HIP call -- allocation, upload, launch, event -- is made by the thread that calls
next_batch(), on the current stream."""
from __future__ import annotations

import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, tfrecord
from ._lib import StabnetError
from .config import Config

SHUFFLE_CAPACITY = 120              # train_bundle_nobm.py:172-176: shuffle_batch(capacity=120, min_after_dequeue=80)
SHUFFLE_MIN_AFTER_DEQUEUE = 80
FEATURES = ("stable_path", "unstable_path", "pos", "flow", "feature_matches1", "feature_matches2")     # get_data_mini_after.py:168-176


def _align(v, a=256):
    return (v + a - 1) // a * a


class Record:
    """The index entry of one record: where it lies and what it holds, without the flow and match arrays themselves."""
    __slots__ = ("file", "offset", "number", "stable_path", "unstable_path", "pos", "flow_len", "n1", "n2")

    def name(self):
        return "%s: record %d" % (self.file, self.number)


def write_dataset(data_dir, split, samples, records_per_file=10):
    """Writes <data_dir>/<split>/list.txt and the record files it names.  samples: dicts with stable_path, unstable_path (str or
    bytes: the folder prefix, '/' included, to which str(pos) + '.jpg' is appended), pos, and optionally flow, feature_matches1,
    feature_matches2 (float arrays, flattened; missing = empty)."""
    d = os.path.join(data_dir, split)
    os.makedirs(d, exist_ok=True)
    names = []
    for i in range(0, len(samples), records_per_file):
        name = "%s_%05d.tfrecords" % (split, i // records_per_file)
        payloads = []
        for s in samples[i:i + records_per_file]:
            b = lambda v: v.encode("utf-8") if isinstance(v, str) else bytes(v)
            payloads.append(tfrecord.encode_example({
                "stable_path": b(s["stable_path"]), "unstable_path": b(s["unstable_path"]),
                "pos": np.array([int(s["pos"])], np.int64),
                "flow": np.asarray(s.get("flow", ()), np.float32).reshape(-1),
                "feature_matches1": np.asarray(s.get("feature_matches1", ()), np.float32).reshape(-1),
                "feature_matches2": np.asarray(s.get("feature_matches2", ()), np.float32).reshape(-1)}))
        tfrecord.write_records(os.path.join(d, name), payloads)
        names.append(name)
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write(" ".join(names))
    return names


class _Plan:
    """The host side of one batch: which files, how each is decoded, where its pixels land, and the two get_img tables."""


class PairDataset:
    """next_batch() -> {'stable' [N,H,W,2*len(indices)], 'unstable' [N,H,W,2], 'flow' [N,H,W,2], 'matches1' / 'matches2'
    [N,max_matches,4]: float32 device tensors; 'n1' / 'n2': int32 arrays}, for ever (num_epochs=None).  Rank `rank` of `world`
    reads records rank, rank + world, ...; the sequence of samples is a function of (seed, rank, world) alone.
    prefetch=1: the host work of the next batch runs on worker threads while the caller trains on this one; prefetch=0: inline.
    flow="record": a record's flow as it stands, zeros when it is empty.  flow="tvl1": records whose flow is empty get the TV-L1
    flow (stabnet_amd.flow, csrc/tvl1.hip) from stable frame pos - 1 to stable frame pos, as the map interpolate() reads, computed
    on the device from the `stable` tensor the batch has just produced; records that carry a flow keep it.
    matches="record": a record's feature matches as they stand (none when a list is empty).  matches="klt": a list that is empty
    in the record is computed on the device behind the get_img launches (stabnet_amd.features, csrc/klt.hip): feature_matches1
    from stable frame pos - 1 to unstable frame pos - 1 (tower 1), feature_matches2 from stable frame pos to unstable frame pos
    (tower 2); a list that carries rows keeps them.  In this mode 'n1' / 'n2' are int32 DEVICE tensors (nothing is read back;
    data.augment_pairs takes either)."""

    def __init__(self, data_dir, split, cfg: Config, H: int, W: int, batch: int, device="cuda:0", rank: int = 0, world: int = 1,
                 seed: int = 0, shuffle: bool = True, prefetch: int = 1, workers: int = 8, flow: str = "record",
                 matches: str = "record"):
        self.data_dir, self.split, self.cfg = str(data_dir), str(split), cfg
        self.H, self.W, self.batch = int(H), int(W), int(batch)
        self.device_spec = device
        self.rank, self.world, self.seed, self.shuffle = int(rank), int(world), int(seed), bool(shuffle)
        if not (0 <= self.rank < self.world):
            raise StabnetError("PairDataset: rank %d outside world %d" % (self.rank, self.world))
        if prefetch not in (0, 1):
            raise StabnetError("PairDataset: prefetch must be 0 (inline) or 1 (one batch ahead), got %r" % (prefetch,))
        self.prefetch = int(prefetch)
        if flow not in ("record", "tvl1"):
            raise StabnetError("PairDataset: flow must be 'record' (as stored; zeros when empty) or 'tvl1' (empty flows are computed "
                               "on the device), got %r" % (flow,))
        self.flow_mode = flow
        self._flow_ws = None
        if matches not in ("record", "klt"):
            raise StabnetError("PairDataset: matches must be 'record' (as stored; none when empty) or 'klt' (empty lists are computed "
                               "on the device), got %r" % (matches,))
        self.matches_mode = matches
        self._klt_ws = None
        self.workers = max(1, min(int(workers), 16))            # never sized from the machine's CPU count
        if any(i < 0 for i in cfg.indices):
            raise StabnetError("PairDataset: negative entries of cfg.indices (future frames) are not supported")
        self.C = 2 * len(cfg.indices)
        self.records = self._index()
        self.shard = list(range(self.rank, len(self.records), self.world))
        if not self.shard:
            raise StabnetError("PairDataset: %s holds %d record(s), none for rank %d of %d"
                               % (os.path.join(self.data_dir, self.split), len(self.records), self.rank, self.world))
        self._rng = np.random.default_rng([self.seed, self.rank, self.world])
        self._stream_pos = 0
        self._buffer = []
        self._noted = set()
        self._pool = None
        self._coord = None
        self._pending = None
        self._dev = None

    # ---- index, order, host side of a sample (no GPU) -----------------------------------------------------------------------------

    def _note(self, key, msg):
        if key not in self._noted:
            self._noted.add(key)
            print("note: " + msg, flush=True)

    def _index(self):
        d = os.path.join(self.data_dir, self.split)
        lst = os.path.join(d, "list.txt")
        if not os.path.isfile(lst):
            raise StabnetError("PairDataset: %s not found" % lst)
        with open(lst) as f:
            names = [n.strip() for n in f.read().split(" ")]                 # get_data_mini_after.py:159-163
        recs = []
        hw = self.H * self.W
        for name in [n for n in names if n]:
            path = os.path.join(d, name)
            if not os.path.isfile(path):
                raise StabnetError("PairDataset: %s names %s, which does not exist" % (lst, path))
            for k, (off, payload) in enumerate(tfrecord.read_records(path, with_offsets=True)):
                ex = tfrecord.parse_example(payload)
                r = Record()
                r.file, r.offset, r.number = path, off, k
                missing = [n for n in FEATURES[:3] if n not in ex]            # FixedLenFeature; a VarLenFeature may be absent (empty)
                if missing:
                    raise StabnetError("%s lacks the feature(s) %s" % (r.name(), ", ".join(missing)))
                for n in ("stable_path", "unstable_path"):
                    if not isinstance(ex[n], bytes):
                        raise StabnetError("%s: %s must be one string" % (r.name(), n))
                if not (isinstance(ex["pos"], np.ndarray) and ex["pos"].dtype == np.int64 and ex["pos"].size == 1):
                    raise StabnetError("%s: pos must be one int64" % r.name())
                r.stable_path, r.unstable_path = ex["stable_path"].decode("utf-8"), ex["unstable_path"].decode("utf-8")
                r.pos = int(ex["pos"][0])
                r.flow_len = int(np.asarray(ex.get("flow", ())).size)
                if r.flow_len and (r.flow_len % hw or r.flow_len // hw < 2):
                    raise StabnetError("%s: flow holds %d values, which is not %d x %d x (2 or more channels)"
                                       % (r.name(), r.flow_len, self.H, self.W))
                for n, a in (("n1", "feature_matches1"), ("n2", "feature_matches2")):
                    size = int(np.asarray(ex.get(a, ())).size)
                    if size % 4:
                        raise StabnetError("%s: %s holds %d values, no multiple of 4" % (r.name(), a, size))
                    if size // 4 >= self.cfg.max_matches:                      # get_data_mini_after.py:217-218: assert_less
                        raise StabnetError("%s: %s holds %d matches, max_matches is %d (the count must be smaller)"
                                           % (r.name(), a, size // 4, self.cfg.max_matches))
                    setattr(r, n, size // 4)
                if r.pos - 1 - max(self.cfg.indices) < 0:
                    raise StabnetError("%s: pos %d reaches %d frames back, before frame 0" % (r.name(), r.pos, 1 + max(self.cfg.indices)))
                recs.append(r)
        if not recs:
            raise StabnetError("PairDataset: %s names no record" % lst)
        return recs

    def frame_files(self, rec):
        """(stable files, one per channel: tower 1 then tower 2; unstable files: [pos - 1, pos]) -- get_data_mini_after.py:177-209."""
        def f(path, pos):
            p = path + str(pos) + ".jpg"                                      # get_data_mini_after.py:150, no zero padding
            return p if os.path.isabs(p) else os.path.join(self.data_dir, p)
        ind = self.cfg.indices
        stable = [f(rec.stable_path, rec.pos - 1 - i) for i in ind] + [f(rec.stable_path, rec.pos - i) for i in ind]
        return stable, [f(rec.unstable_path, rec.pos - 1), f(rec.unstable_path, rec.pos)]

    def _next_in_stream(self):
        i = self.shard[self._stream_pos % len(self.shard)]                    # num_epochs=None: the shard repeats for ever
        self._stream_pos += 1
        return i

    def next_indices(self, n: int):
        """The record numbers (into self.records) of the next n samples.  shuffle: a buffer that is refilled to 120 before every
        draw (so more than 80 are always left after it), drawn from by the seeded generator."""
        out = []
        for _ in range(n):
            if not self.shuffle:
                out.append(self._next_in_stream())
                continue
            while len(self._buffer) < SHUFFLE_CAPACITY:
                self._buffer.append(self._next_in_stream())
            assert len(self._buffer) - 1 >= SHUFFLE_MIN_AFTER_DEQUEUE
            j = int(self._rng.integers(0, len(self._buffer)))
            self._buffer[j], self._buffer[-1] = self._buffer[-1], self._buffer[j]
            out.append(self._buffer.pop())
        return out

    def host_sample(self, rec):
        """flow [H,W,2], matches1 / matches2 [max_matches,4] zero-padded, n1, n2 of one record, read again from its file."""
        with open(rec.file, "rb") as f:
            f.seek(rec.offset)
            ex = tfrecord.parse_example(tfrecord.read_record_at(f, rec.file, rec.number, check=False))   # the index checked the CRCs
        M = self.cfg.max_matches
        flow = np.asarray(ex.get("flow", ()), np.float32)
        empty = flow.size == 0
        if empty:
            if self.flow_mode == "record":
                self._note("flow", "PairDataset: records with an empty flow get zeros (the published data has its flow zeroed)")
            flow = np.zeros((self.H, self.W, 2), np.float32)
        else:
            flow = np.ascontiguousarray(flow.reshape(self.H, self.W, -1)[:, :, :2])       # get_data_mini_after.py:210
        out = {"flow": flow, "flow_empty": empty}
        for k in ("1", "2"):
            m = np.asarray(ex.get("feature_matches" + k, ()), np.float32).reshape(-1, 4)         # :212-213
            p = np.zeros((M, 4), np.float32)                                              # :221-222
            p[:len(m)] = m
            out["matches" + k] = p
            out["n" + k] = len(m)
        return out

    # ---- host work of a batch (worker threads: no HIP call below this line until _launch) ---------------------------------------

    def _map(self, fn, items):
        if self._pool is None or len(items) <= 1:               # prefetch=0: everything inline, in the calling thread
            return [fn(x) for x in items]
        return list(self._pool.map(fn, items))

    @staticmethod
    def _read_parse(path):
        from . import mjpeg
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise StabnetError("PairDataset: cannot read the frame file %s (%s)" % (path, e.strerror or e))
        try:
            return data, mjpeg.parse(data), None
        except mjpeg.Unsupported as e:
            return data, None, str(e)
        except StabnetError as e:
            raise StabnetError("PairDataset: %s: %s" % (path, e))

    @staticmethod
    def _pillow_bgr(path, data):
        from PIL import Image
        im = Image.open(io.BytesIO(data))
        if im.mode not in ("RGB", "YCbCr"):
            raise StabnetError("PairDataset: %s is a %s JPEG; the reference's rgb_to_grayscale wants three channels" % (path, im.mode))
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])

    def _plan(self, indices):
        """Phase A: read and parse every distinct file of the batch, decide how each is decoded and lay the decoded frames out."""
        p = _Plan()
        p.indices = indices
        p.samples = [self.host_sample(self.records[i]) for i in indices]
        files, order = {}, []
        chans = []                                                            # (tensor 0 stable / 1 unstable, n, c, file number)
        for n, i in enumerate(indices):
            st, un = self.frame_files(self.records[i])
            for t, lst in ((0, st), (1, un)):
                for c, path in enumerate(lst):
                    if path not in files:                                     # a frame named twice is read and decoded once
                        files[path] = len(order)
                        order.append(path)
                    chans.append((t, n, c, files[path]))
        parsed = self._map(self._read_parse, order)
        p.files, p.data = order, [d for d, _, _ in parsed]
        groups, raws = {}, []                                                 # geometry -> file numbers; Pillow-decoded file numbers
        for k, (data, info, why) in enumerate(parsed):
            if info is None:
                raws.append(k)
                continue
            if info["C"] != 3:
                raise StabnetError("PairDataset: %s is a grey JPEG; the reference's rgb_to_grayscale wants three channels" % order[k])
            groups.setdefault((info["H"], info["W"], info["subsampling"], info["restart"] == 0), []).append(k)
        p.groups = sorted(groups.items())
        p.raw = list(zip(raws, self._map(lambda k: self._pillow_bgr(order[k], p.data[k]), raws)))
        for k, a in p.raw:
            self._note(("pillow", a.shape), "PairDataset: %dx%d frames such as %s are outside the device decoder's scope (%s); they are "
                       "decoded on the host with Pillow and uploaded" % (a.shape[1], a.shape[0], order[k], parsed[k][2]))
        # the arena of decoded frames: one dense block per geometry, then the Pillow-decoded frames
        geo = [None] * len(order)                                             # file number -> (offset, sh, sw, row stride)
        off = 0
        p.group_off = []
        for (h, w, _, _), ks in p.groups:
            p.group_off.append(off)
            for j, k in enumerate(ks):
                geo[k] = (off + j * h * w * 3, h, w, 3 * w)
            off = _align(off + len(ks) * h * w * 3)
        p.raw_off = off
        for k, a in p.raw:
            geo[k] = (off, a.shape[0], a.shape[1], 3 * a.shape[1])
            off = _align(off + a.size)
        p.arena_bytes = max(off, 256)
        p.tables = [np.array([geo[k] + (n, c) for t, n, c, k in chans if t == which], np.int64) for which in (0, 1)]
        p.staged = False
        return p

    def _fits(self, p, s):
        """Can plan p be staged into slot set s as it stands?  (Reads sizes only.)"""
        for (key, ks) in p.groups:
            g = s["geom"].get(key)
            if g is None or g["cap"] < len(ks) or g["stride"] < max(g["dec"].slot_bytes(len(p.data[k])) for k in ks):
                return False
        return s["raw_cap"] >= p.arena_bytes - p.raw_off

    def _stage(self, p, s):
        """Phase B: parse + host entropy decoding into the pinned slots of set s; Pillow-decoded frames into its raw buffer."""
        jobs = []
        for key, ks in p.groups:
            g = s["geom"][key]
            for j, k in enumerate(ks):
                jobs.append((g, j, k))
        used = self._map(lambda job: job[0]["dec"].stage(p.data[job[2]], job[0]["h_in"][job[1]], p.files[job[2]]), jobs)
        p.used = {}
        for (g, j, k), u in zip(jobs, used):
            p.used[k] = u
        raw = s["h_raw_np"]
        off = 0
        for k, a in p.raw:
            raw[off:off + a.size] = a.reshape(-1)
            off = _align(off + a.size)
        for which in (0, 1):
            s["h_tab_np"][which][:len(p.tables[which])] = p.tables[which]
        p.staged = True
        return p

    def _prepare(self, indices, s):
        p = self._plan(indices)
        if s is not None and self._fits(p, s):
            self._stage(p, s)
        return p

    # ---- device side (the calling thread only) ------------------------------------------------------------------------------------

    def _device_init(self):
        import torch
        self._torch = torch
        self._dev = torch.device(self.device_spec)
        if self._dev.type != "cuda":
            raise StabnetError("PairDataset: device %s: the frames are decoded and converted on the GPU (there is no CPU fallback)" % self._dev)
        _lib.lib()                                                            # bound before any worker thread calls into it
        self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="pairdataset") if self.prefetch else None
        self._coord = ThreadPoolExecutor(1, thread_name_prefix="pairdataset-batch") if self.prefetch else None
        self._decoders = {}
        self._arena = torch.empty(256, dtype=torch.uint8, device=self._dev)
        ncap = [self.batch * self.C, self.batch * 2]
        self._sets = []
        for _ in range(2):
            h_tab = [torch.zeros((n, 6), dtype=torch.int64).pin_memory() for n in ncap]
            self._sets.append({"geom": {}, "raw_cap": 0, "h_raw": None, "h_raw_np": np.zeros(0, np.uint8), "event": None,
                               "h_tab": h_tab, "h_tab_np": [t.numpy() for t in h_tab],
                               "d_tab": [torch.zeros((n, 6), dtype=torch.int64, device=self._dev) for n in ncap]})
        self._turn = 0

    def _grow(self, p, s):
        """Make slot set s large enough for plan p: decoders, pinned slots and their device copies (allocation is a HIP call)."""
        torch = self._torch
        from .mjpeg import MjpegDecoder
        for key, ks in p.groups:
            h, w, sub, host = key
            dec = self._decoders.get(key)
            if dec is None:
                dec = self._decoders[key] = MjpegDecoder(h, w, 3, sub or 420, device=self._dev, batch=1, host_entropy=host)
            need = max(dec.slot_bytes(len(p.data[k])) for k in ks)
            g = s["geom"].get(key)
            if g is None or g["cap"] < len(ks) or g["stride"] < need:
                cap = max(len(ks), g["cap"] if g else 0, min(self.batch * (self.C + 2), 2 * len(ks)))
                stride = max(_align(need, 4096), g["stride"] if g else 0, dec.in_stride)
                h_in = torch.zeros((cap, stride), dtype=torch.uint8).pin_memory()
                s["geom"][key] = {"dec": dec, "cap": cap, "stride": stride, "h_in": h_in,
                                  "d_in": torch.zeros((cap, stride), dtype=torch.uint8, device=self._dev),
                                  "status": torch.zeros(cap, dtype=torch.int32, device=self._dev)}
        raw_need = p.arena_bytes - p.raw_off
        if s["raw_cap"] < raw_need and p.raw:
            s["h_raw"] = torch.zeros(_align(raw_need, 1 << 16), dtype=torch.uint8).pin_memory()
            s["h_raw_np"], s["raw_cap"] = s["h_raw"].numpy(), s["h_raw"].numel()

    def _launch(self, p, s):
        torch = self._torch
        from . import tf_image
        dev = self._dev
        if self._arena.numel() < p.arena_bytes:
            self._arena = torch.empty(_align(p.arena_bytes, 1 << 20), dtype=torch.uint8, device=dev)
        checks = []
        with torch.cuda.device(dev):
            for (key, ks), off in zip(p.groups, p.group_off):
                g, n = s["geom"][key], len(ks)
                dec = g["dec"]
                ws = _lib.lib().stabnet_mjpeg_decode_workspace_bytes(n, dec.H, dec.W, dec.C, dec.subsampling)
                if dec.workspace.numel() < ws:                                # the decoder's workspace, for n frames
                    dec.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
                h, w = key[0], key[1]
                if dec.host_entropy:                                          # the slots are full: one copy
                    g["d_in"][:n].copy_(g["h_in"][:n], non_blocking=True)
                else:
                    for j, k in enumerate(ks):
                        g["d_in"][j, :p.used[k]].copy_(g["h_in"][j, :p.used[k]], non_blocking=True)
                out = self._arena[off:off + n * h * w * 3].view(n, h, w, 3)
                dec.enqueue(g["d_in"], n, out, g["status"][:n])
                checks.append((g, ks))
            if p.raw:
                nb = p.arena_bytes - p.raw_off
                self._arena[p.raw_off:p.raw_off + nb].copy_(s["h_raw"][:nb], non_blocking=True)
            ne = [len(t) for t in p.tables]
            for which in (0, 1):
                s["d_tab"][which][:ne[which]].copy_(s["h_tab"][which][:ne[which]], non_blocking=True)
            s["event"] = torch.cuda.Event()
            s["event"].record(torch.cuda.current_stream(dev))                 # the pinned slots of this set are free once this has passed
            N = len(p.indices)
            stable = torch.empty((N, self.H, self.W, self.C), dtype=torch.float32, device=dev)
            unstable = torch.empty((N, self.H, self.W, 2), dtype=torch.float32, device=dev)
            tf_image.get_img(self._arena, s["d_tab"][0][:ne[0]], stable)
            tf_image.get_img(self._arena, s["d_tab"][1][:ne[1]], unstable)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            batch = {"stable": stable, "unstable": unstable,
                     "flow": up(np.stack([x["flow"] for x in p.samples])),
                     "matches1": up(np.stack([x["matches1"] for x in p.samples])),
                     "matches2": up(np.stack([x["matches2"] for x in p.samples])),
                     "n1": np.array([x["n1"] for x in p.samples], np.int32),
                     "n2": np.array([x["n2"] for x in p.samples], np.int32)}
            empty = [n for n, x in enumerate(p.samples) if x["flow_empty"]]
            if self.flow_mode == "tvl1" and empty:
                batch["flow"] = self._tvl1(stable, batch["flow"], empty)
            if self.matches_mode == "klt":
                for k, cs, cu in (("1", 0, 0), ("2", self.C // 2, 1)):
                    batch["matches" + k], batch["n" + k] = self._klt(stable[..., cs], unstable[..., cu], batch["matches" + k], batch["n" + k])
        return batch, checks

    def _tvl1(self, stable, flow, empty):
        """The TV-L1 map of every pair of the batch from stable frame pos - 1 (channel 0: what training sees as y1) to stable
        frame pos (channel len(indices): y2), read in place on get_img's scale; the pairs listed in `empty` take it."""
        from . import flow as tvl1
        N = stable.shape[0]
        need = tvl1.workspace_bytes(N, self.H, self.W)
        if self._flow_ws is None or self._flow_ws.numel() < need:
            self._flow_ws = self._torch.empty(need, dtype=self._torch.uint8, device=self._dev)
        m = tvl1.tvl1_flow(stable[..., 0], stable[..., self.C // 2], out="map", workspace=self._flow_ws, offset=0.5, scale=255.0)
        if len(empty) == N:
            return m
        idx = self._torch.tensor(empty, dtype=self._torch.int64, device=self._dev)
        flow[idx] = m[idx]
        return flow

    def _klt(self, stable, unstable, rows, n):
        """The matches of every pair of the batch from one stable channel to the unstable channel of the same instant, read in
        place on get_img's scale; the records whose list is empty (n == 0 on the host) take them.  -> rows, n (int32, on the device)."""
        from . import features
        torch = self._torch
        N = stable.shape[0]
        need = features.workspace_bytes(N, self.H, self.W)
        if self._klt_ws is None or self._klt_ws.numel() < need:
            self._klt_ws = torch.empty(need, dtype=torch.uint8, device=self._dev)
        m, cnt = features.klt_matches(stable, unstable, self.cfg.max_matches, workspace=self._klt_ws, offset=0.5, scale=255.0)
        empty = np.flatnonzero(n == 0)
        if len(empty) == N:
            return m, cnt
        idx = torch.from_numpy(empty.astype(np.int64)).to(self._dev)
        n = torch.from_numpy(n).to(self._dev)
        rows[idx] = m[idx]
        n[idx] = cnt[idx]
        return rows, n

    def _free_set(self, s):
        if s["event"] is not None:
            s["event"].synchronize()                                          # its last uploads have landed: the workers may write again

    def next_batch(self):
        if self._dev is None:
            self._device_init()
        s = self._sets[self._turn]
        if self._pending is not None:
            fut, self._pending = self._pending, None
            p = fut.result()
        else:
            self._free_set(s)
            p = self._prepare(self.next_indices(self.batch), s)
        if not p.staged:                                                      # the set has to grow first: allocation belongs to this thread
            self._free_set(s)
            self._grow(p, s)
            self._stage(p, s)
        batch, checks = self._launch(p, s)
        self._turn ^= 1
        if self.prefetch:
            nxt = self._sets[self._turn]
            self._free_set(nxt)
            self._pending = self._coord.submit(self._prepare, self.next_indices(self.batch), nxt)
        for g, ks in checks:                                                  # (synchronises) a stream that does not decode is an error
            bad = [(k, int(v)) for k, v in zip(ks, g["status"][:len(ks)].cpu().tolist()) if v]
            if bad:
                raise StabnetError("PairDataset: %s does not decode on the device (status %d)" % (p.files[bad[0][0]], bad[0][1]))
        return batch

    def close(self):
        """Waits for the batch in flight and ends the worker threads."""
        if self._pending is not None:
            try:
                self._pending.result()
            except Exception:
                pass
            self._pending = None
        for ex in (self._coord, self._pool):
            if ex is not None:
                ex.shutdown(wait=True)
        self._coord = self._pool = None
        if self._dev is not None:
            self._torch.cuda.synchronize(self._dev)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
