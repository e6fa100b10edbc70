"""Shared by test_reference_run_cpu.py / test_reference_run_gpu.py: reading tests/golden/reference_run_<case>.npz (the recorded results of
the reference's own warp and loss code, oracle/run_reference.py) and the summation bars built from what those runs recorded.

BARS.  A float32 sum of n terms t_i, added in any order, differs from the exact sum by at most (n - 1) * 2^-24 * sum |t_i| (first order);
the terms themselves differ between a float32 and a float64 evaluation by what the reference's two runs show, sum |t_i(f32) - t_i(f64)|.
`red_<name>` in a fixture holds [n, sum |t|, sum |t32 - t64|] per output element of that reduction.  Elementwise operations behind a
reduction (the division of a mean, a multiplier) add 2^-24 of the value each; 4 of them are allowed per quantity.  Nested reductions
(feature loss: pairs -> matches -> samples; image loss: pixels -> samples) propagate the inner bound through the quotient, whose
denominators -- a count of matches, a count of kept pixels -- are exact in float32; the + 1e-8 of the image loss's denominator vanishes
in float32 and is 1e-8 / count relative in float64, which is added.  `terms=` replaces n by the number of terms a kernel adds where it
sums more elementary terms than the reference's reduce op (the distortion kernel adds the 8 rotations' squares itself)."""
import os

import numpy as np

from oracle import run_reference as RR
from oracle import stabnet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U24 = 2.0 ** -24
AFTER = 4 * U24


def load(case):
    with np.load(os.path.join(GOLDEN, RR.fixture_name(case)), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def geom(rec):
    N, H, W, C, gh, gw, M = (int(v) for v in rec["geom"])
    return N, H, W, C, gh, gw, M


def ocfg(rec):
    N, H, W, C, gh, gw, M = geom(rec)
    return O.Config(height=H, width=W, batch_size=N, grid_h=gh, grid_w=gw, max_matches=M)


def f64(rec, name):
    """The f64-mode value of an image stored as float32 + float32 difference (oracle/run_reference.py), and the storage slack of that."""
    d = rec[name + "_d"].astype(np.float64)
    return rec[name].astype(np.float64) + d, U24 * np.abs(d)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def sum_bar(red, terms=None):
    """Bound on |float32 sum in any order - float64 sum| per output element."""
    n, s, d = red
    n = n if terms is None else terms
    return (n - 1) * U24 * s + d


def mean_bar(red, value, scale=1.0, terms=None):
    return float(np.sum(sum_bar(red, terms) / red[0]) * abs(scale) + AFTER * abs(value))


def loss_bars(rec, gate, cfg, terms=None, cap=None):
    """Bars of the entries of inference_stable_net's dict (RR.SCALARS) at gate setting `gate` (index into RR.GATES), against their f64
    values.  terms: {'dist': n, ...} term counts of a kernel, where they differ from the reference's.  cap: {entry: relative bar} that
    an entry's bar may not exceed (the total is composed from the capped bars)."""
    terms, cap = terms or {}, cap or {}
    use_black, use_theta_only = RR.GATES[gate]
    v = {k: float(rec["ret_" + k + "_f64"][gate]) for k in RR.SCALARS}
    b = {}
    id2 = mean_bar(rec["red_id2"], v["theta_loss"] / cfg.theta_mul, cfg.id_mul, terms.get("id2"))
    b["theta_loss"] = id2 * cfg.theta_mul
    b["grid_theta_loss"] = id2 * cfg.grid_theta_mul
    b["black_loss"] = mean_bar(rec["red_black"], v["black_loss"], cfg.black_mul * use_black, terms.get("black"))
    b["distortion_loss"] = mean_bar(rec["red_dist"], v["distortion_loss"], cfg.distortion_mul / 8.0, terms.get("dist"))
    b["consistency_loss"] = mean_bar(rec["red_cons"], v["consistency_loss"], cfg.consistency_mul, terms.get("cons"))
    # feature: after_b = S_b / max(count_b, 1), S_b over M matches of |dx| + |dy| (pair sums: 1 addition each, inside the terms of S_b)
    n, s, d = rec["red_feat_num"]
    pair = U24 * np.sum(rec["red_feat_pair"][1] * rec["mask"], axis=1)       # |dx| + |dy| added apart from the pair by a kernel
    den = np.maximum(rec["red_feat_den"][1], 1.0)
    d_after = ((n - 1) * U24 * s + d + pair) / den
    nb, sb, _ = rec["red_feat"]
    b["feature_loss"] = float((np.sum(d_after) + (nb - 1) * U24 * sb) / nb * cfg.feature_mul + AFTER * abs(v["feature_loss"]))
    # image: r_b = num_b / (kept_b + 1e-8), summed over the batch and divided by batch_size
    kept = rec["red_img_den"][1]
    r = rec["red_img_num"][1] / kept                                       # (the terms err^2 are >= 0: sum |t| is the sum)
    d_r = sum_bar(rec["red_img_num"]) / kept + r * 1e-8 / kept + U24 * r
    nb = rec["red_img"][0]
    b["img_loss"] = float((np.sum(d_r) + (nb - 1) * U24 * np.sum(r)) / cfg.batch_size * cfg.img_mul + AFTER * abs(v["img_loss"]))
    b["regu_loss"] = AFTER * abs(v["regu_loss"])
    for k, r in cap.items():
        b[k] = min(b[k], r * abs(v[k]))
    live = 1.0 - use_theta_only
    inner = ("img_loss", "regu_loss", "black_loss", "distortion_loss", "consistency_loss", "feature_loss")
    b["total_loss"] = float(b["theta_loss"] + b["grid_theta_loss"] + live * sum(b[k] for k in inner)
                            + 8 * U24 * (abs(v["theta_loss"]) + abs(v["grid_theta_loss"]) + live * sum(abs(v[k]) for k in inner)))
    return b, v
