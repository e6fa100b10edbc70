"""How good is a stabilised clip: cropping ratio, distortion value and stability score, the three numbers of Liu et al. 2013
("Bundled Camera Paths") that the stabilisation literature, the StabNet paper included, reports per clip.

The device part: corners of one frame tracked into the other (features.klt_matches, csrc/klt.hip), then a robust homography per
frame pair (homfit, csrc/homfit.hip: RANSAC with a fixed number of hypotheses, a float64 refit, bit for bit tests/homfit_model.py).
The homographies live in the frame x' = 2x/W - 1, y' = 2y/H - 1 and map (x0, y0, 1) to (x1, y1, 1) with h33 = 1.  score_clip reads
them back once; everything after that is host float64:

  pixel frame  H_px = N^-1 H N with N = [[2/W, 0, -1], [0, 2/H, -1], [0, 0, 1]], divided by H_px[2,2]; A = its upper-left 2 x 2.
  cropping     per frame 1 / sqrt(A00^2 + A01^2) of the homography unstable frame t -> stable frame t; the clip's value is
               min(mean over the frames, 1).
  distortion   per frame |lambda_small| / |lambda_large| of A's two eigenvalues (a complex pair: 1); the clip's value is the
               minimum over the frames.
  stability    P_0 = I, P_(t+1) = P_t H_px,t over the stable clip's consecutive pairs, P divided by P22 after every step; the series
               |t| = sqrt(P02^2 + P12^2) and theta = atan2(P10, P00), T values each; p = |fft(series)|^2 [1 : T//2]; the share
               sum(p[:5]) / sum(p) (1 when sum(p) is 0); the clip's value is the smaller of the two shares.  T >= 14.
  failed pair  a pair without a model (status 0) is left out of cropping and distortion and is the identity in the path.
  scene cut    with cuts=[c, ...] the stable pair (c - 1, c) joins two scenes: it is the identity in the path like a failed pair.

Grey of a uint8 BGR frame: (0.114*B + 0.587*G) + 0.299*R in float32 (torch arithmetic: plumbing); a uint8 grey frame is its values."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, features
from ._lib import StabnetError
from ._tensor import ptr, stream_ptr

MAX_ROWS = 1024          # a pair's rows are staged in 16 KiB of LDS
MIN_FRAMES = 14          # p = |fft|^2 [1 : T//2] needs more than five bins to say anything


@dataclass(frozen=True)
class HomfitParams:
    """hypotheses: four-point models tried per pair (thread k of 256 owns k, k + 256, ...).  thr_px: the largest transfer error of
    an inlier, in pixels.  min_inliers: fewer (or fewer than 4) give no model.  seed: of the sampling, 0..2^31 - 1.  w_min: a row
    whose projective weight h6*x + h7*y + 1 is not above it is no inlier.  Defaults, not tuned."""
    hypotheses: int = 256
    thr_px: float = 2.0
    min_inliers: int = 4
    seed: int = 0
    w_min: float = 1e-6


def homfit(matches, n, H: int, W: int, params: HomfitParams = None, prof=None):
    """matches float32 [B,M,4] and n int32 [B] on the device, as features.klt_matches returns them (rows (x0, y0, x1, y1) in the
    normalised frame of H x W pixels; only the first n[b] rows of pair b are read) -> (Hm float32 [B,9], mask uint8 [B,M],
    count int32 [B], status int32 [B]: 0 no model, 1 refit model, 2 the hypothesis kept because the refit failed, best int32 [B]:
    the winning hypothesis or -1), all on the device.  Nothing synchronises or allocates inside the call."""
    p = params or HomfitParams()
    if not isinstance(matches, torch.Tensor) or not matches.is_cuda:
        raise StabnetError("metrics.homfit: matches must be a tensor on the GPU (there is no CPU fallback)")
    if matches.dtype != torch.float32 or matches.dim() != 3 or matches.shape[2] != 4 or not matches.is_contiguous():
        raise StabnetError("metrics.homfit: matches must be a contiguous float32 [B,M,4] tensor, got %s %s" % (matches.dtype, tuple(matches.shape)))
    B, M = int(matches.shape[0]), int(matches.shape[1])
    if not isinstance(n, torch.Tensor) or n.device != matches.device or n.dtype != torch.int32 or tuple(n.shape) != (B,) or not n.is_contiguous():
        raise StabnetError("metrics.homfit: n must be a contiguous int32 [B] tensor on %s with B = %d" % (matches.device, B))
    if not 4 <= M <= MAX_ROWS:
        raise StabnetError("metrics.homfit: M must be 4..%d rows per pair, got %d" % (MAX_ROWS, M))
    dev = matches.device
    Hm = torch.empty((B, 9), dtype=torch.float32, device=dev)
    mask = torch.empty((B, M), dtype=torch.uint8, device=dev)
    count, status, best = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    _lib.call("stabnet_homfit", ptr(matches), ptr(n), B, M, int(H), int(W), int(p.hypotheses), float(p.thr_px), int(p.min_inliers), int(p.seed),
              float(p.w_min), ptr(Hm), ptr(mask), ptr(count), ptr(status), ptr(best), stream_ptr(dev), prof.handle if prof is not None else 0,
              device=dev)
    return Hm, mask, count, status, best


def pair_homographies(i0, i1, klt: features.KltParams = None, fit: HomfitParams = None, chunk: int = 64, offset: float = 0.0,
                      scale: float = 1.0, counts: bool = False, prof=None):
    """i0, i1: float32 [T,H,W] device tensors on the 0..255 scale after (v + offset) * scale; they may be the views S[:-1] and S[1:]
    of one tensor.  Corners of i0[t] tracked into i1[t] (max_matches = cells + 1: every cell can keep its row), then the fit, `chunk`
    pairs at a time with one reused workspace.  -> (Hm [T,9], status [T]) on the device (and the inlier counts [T] with counts=True);
    Hm[t] maps frame i0[t]'s normalised coordinates to i1[t]'s."""
    klt = klt or features.KltParams()
    if not isinstance(i0, torch.Tensor) or i0.dim() != 3 or int(chunk) < 1:
        raise StabnetError("metrics.pair_homographies: i0 and i1 must be float32 [T,H,W] device tensors and chunk at least 1")
    T, H, W = (int(v) for v in i0.shape)
    ny, nx = features.cells(H, W, klt)
    M = ny * nx + 1
    if not 4 <= M <= MAX_ROWS:
        raise StabnetError("metrics.pair_homographies: %d x %d pixels in cells of %d give %d rows per pair; the fit takes 4..%d: "
                           "choose a larger KltParams.cell or a smaller frame" % (H, W, klt.cell, M, MAX_ROWS))
    chunk = min(int(chunk), T)
    ws = torch.empty(features.workspace_bytes(chunk, H, W, klt), dtype=torch.uint8, device=i0.device)
    Hs, st, cn = [], [], []
    for a in range(0, T, chunk):
        rows, n = features.klt_matches(i0[a:a + chunk], i1[a:a + chunk], M, klt, workspace=ws, prof=prof, offset=offset, scale=scale)
        Hm, _, count, status, _ = homfit(rows, n, H, W, fit, prof=prof)
        Hs.append(Hm); st.append(status); cn.append(count)
    out = (torch.cat(Hs), torch.cat(st))
    return out + (torch.cat(cn),) if counts else out


def grey(frames):
    """float32 [T,H,W] (as it is), uint8 [T,H,W] or uint8 BGR [T,H,W,3] on the device -> float32 [T,H,W] on the 0..255 scale."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise StabnetError("metrics.grey: the frames must be a tensor on the GPU (there is no CPU fallback)")
    if frames.dtype == torch.float32 and frames.dim() == 3:
        return frames
    if frames.dtype == torch.uint8 and frames.dim() == 3:
        return frames.float()
    if frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3:
        f = frames.float()
        return ((0.114 * f[..., 0] + 0.587 * f[..., 1]) + 0.299 * f[..., 2]).contiguous()
    raise StabnetError("metrics.grey: the frames must be float32 [T,H,W], uint8 [T,H,W] or uint8 BGR [T,H,W,3], got %s %s"
                       % (frames.dtype, tuple(frames.shape)))


# ---- host float64 ----------------------------------------------------------------------------------------------------------------

def pixel_homography(Hn, H: int, W: int) -> np.ndarray:
    N = np.array([[2.0 / W, 0.0, -1.0], [0.0, 2.0 / H, -1.0], [0.0, 0.0, 1.0]])
    Ninv = np.array([[W / 2.0, 0.0, W / 2.0], [0.0, H / 2.0, H / 2.0], [0.0, 0.0, 1.0]])
    P = Ninv @ np.asarray(Hn, np.float64).reshape(3, 3) @ N
    return P / P[2, 2]


def frame_cropping(P: np.ndarray) -> float:
    return 1.0 / math.sqrt(P[0, 0] * P[0, 0] + P[0, 1] * P[0, 1])


def frame_distortion(P: np.ndarray) -> float:
    lam = np.abs(np.linalg.eigvals(P[:2, :2]))
    big = float(lam.max())
    return float(lam.min()) / big if big > 0.0 else 1.0


def spectrum_share(series) -> float:
    s = np.asarray(series, np.float64)
    p = np.abs(np.fft.fft(s)) ** 2
    p = p[1:len(s) // 2]
    tot = float(p.sum())
    return 1.0 if tot == 0.0 else float(p[:5].sum()) / tot


def cut_pairs(cuts, T: int):
    """The stable pairs (c - 1, c) that the scene cuts `cuts` (frame indices of the scored clip) break, as sorted pair indices c - 1.  A cut
    at frame 0 has no pair in front of it; one outside 0..T-1 is an error."""
    pairs = set()
    for c in cuts:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < T:
            raise StabnetError("metrics: scene cut %r is no frame of a clip of %d frames" % (c, T))
        if int(c) >= 1:
            pairs.add(int(c) - 1)
    return sorted(pairs)


def host_metrics(H_us, status_us, H_ss, status_ss, H: int, W: int, per_frame: bool = False, cuts=None) -> dict:
    """The three numbers from the homographies unstable -> stable [T,9] and stable t -> t + 1 [T-1,9] with their statuses.
    cuts (optional): frames of the clip at which a new scene starts; the stable pair (c - 1, c) of each joins two scenes and is treated
    as a failed pair -- the identity in the path -- and counted under "scene_cuts" (present only when cuts is given)."""
    H_us, H_ss = np.asarray(H_us, np.float64).reshape(-1, 9), np.asarray(H_ss, np.float64).reshape(-1, 9)
    T = len(H_us)
    broken = cut_pairs(cuts, T) if cuts is not None else []
    if T < MIN_FRAMES:
        raise StabnetError("metrics.score_clip: a clip of %d frames is too short to score: the stability spectrum needs %d or more" % (T, MIN_FRAMES))
    if len(H_ss) != T - 1 or len(status_us) != T or len(status_ss) != T - 1:
        raise StabnetError("metrics.host_metrics: %d frames need %d consecutive pairs, got %d (statuses %d, %d)"
                           % (T, T - 1, len(H_ss), len(status_us), len(status_ss)))
    crop, dist = [], []
    for h, s in zip(H_us, status_us):
        if int(s) != 0:
            P = pixel_homography(h, H, W)
            crop.append(frame_cropping(P))
            dist.append(frame_distortion(P))
    path = np.eye(3)
    tr, th = [0.0], [0.0]
    for i, (h, s) in enumerate(zip(H_ss, status_ss)):
        if int(s) != 0 and i not in broken:
            path = path @ pixel_homography(h, H, W)
        path = path / path[2, 2]
        tr.append(math.hypot(path[0, 2], path[1, 2]))
        th.append(math.atan2(path[1, 0], path[0, 0]))
    s_t, s_r = spectrum_share(tr), spectrum_share(th)
    out = {"cropping": min(float(np.mean(crop)), 1.0) if crop else 0.0, "distortion": float(min(dist)) if dist else 0.0,
           "stability": min(s_t, s_r), "stability_translation": s_t, "stability_rotation": s_r, "frames": T,
           "failed_pairs_unstable_stable": int(sum(1 for s in status_us if int(s) == 0)),
           "failed_pairs_stable_stable": int(sum(1 for s in status_ss if int(s) == 0))}
    if cuts is not None:
        out["scene_cuts"] = len(broken)
    if per_frame:
        out.update(cropping_per_frame=crop, distortion_per_frame=dist, path_translation=tr, path_rotation=th)
    return out


def score_clip(unstable, stable, klt: features.KltParams = None, fit: HomfitParams = None, chunk: int = 64, per_frame: bool = False,
               homographies: bool = False, prof=None, cuts=None) -> dict:
    """unstable, stable: device tensors of the same T x H x W -- float32 [T,H,W] on the 0..255 scale, uint8 [T,H,W], or uint8 BGR
    [T,H,W,3] (see grey()).  Two batched solves (unstable t -> stable t for every t; stable t -> stable t + 1), one readback of the
    homographies, their statuses and inlier counts, then host float64.  -> a dict: cropping, distortion, stability (each in (0, 1]
    for a sane clip), stability_translation, stability_rotation, frames, failed_pairs_*, mean_inliers, the parameters; the per-frame
    lists with per_frame=True; the homographies read back (H_us, status_us, H_ss, status_ss as lists) with homographies=True.
    cuts: see host_metrics (frames of THESE clips at which a new scene starts; "scene_cuts" in the result)."""
    klt, fit = klt or features.KltParams(), fit or HomfitParams()
    u, s = grey(unstable), grey(stable)
    if u.shape != s.shape or u.device != s.device:
        raise StabnetError("metrics.score_clip: unstable is %s on %s, stable %s on %s; they must agree" % (tuple(u.shape), u.device, tuple(s.shape), s.device))
    T, H, W = (int(v) for v in u.shape)
    if T < MIN_FRAMES:
        raise StabnetError("metrics.score_clip: a clip of %d frames is too short to score: the stability spectrum needs %d or more" % (T, MIN_FRAMES))
    u, s = u.contiguous(), s.contiguous()
    H_us, st_us, c_us = pair_homographies(u, s, klt, fit, chunk, counts=True, prof=prof)
    H_ss, st_ss, c_ss = pair_homographies(s[:-1], s[1:], klt, fit, chunk, counts=True, prof=prof)
    back = torch.cat([H_us.reshape(-1), H_ss.reshape(-1), st_us.float(), st_ss.float(), c_us.float(), c_ss.float()]).cpu().numpy()   # the one readback
    a, b = 9 * T, 9 * T + 9 * (T - 1)
    H_us, H_ss = back[:a].reshape(T, 9), back[a:b].reshape(T - 1, 9)
    st_us, st_ss = back[b:b + T].astype(np.int32), back[b + T:b + 2 * T - 1].astype(np.int32)
    inl = back[b + 2 * T - 1:]
    out = host_metrics(H_us, st_us, H_ss, st_ss, H, W, per_frame, cuts=cuts)
    out["mean_inliers"] = float(inl.mean())
    out["size"] = [H, W]
    out["params"] = {"klt": dataclasses.asdict(klt), "fit": dataclasses.asdict(fit)}
    if homographies:
        out.update(H_us=H_us.tolist(), status_us=st_us.tolist(), H_ss=H_ss.tolist(), status_ss=st_ss.tolist())
    return out
