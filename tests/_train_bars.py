"""Test helper (not a test module): what float32 itself costs the training step's gradient, per shape, from the oracle alone --
and the bars the GPU step is held to, derived from it by a rule.

REFERENCE FLOORS.  reference_floors(N, H, W, seed) evaluates oracle/torch_ref.train_objective twice on the CPU: in float64
(gradient, and the evaluation's own decisions: record=), and in float32 (T.DT switched) with those decisions forced, so that both
differentiate the same smooth piece.  The difference is the rounding of a plain float32 evaluation of the same graph: no kernel of
the project is involved (the float32 pass runs on one thread: its summation order, and so the floors, do not depend on the machine's
thread count).  It is summarised with the normalisation of tests/_decisions.gradient_errors (element error over
max(|tensor|_max, 1e-5 gmax), relative L2 over max(|tensor|_2, 1e-5 gmax sqrt(n))) for two classes of trainable tensors, told apart
on float64 values only:

    class Z   float64 max|g| < 1e-9 gmax: tensors whose gradient is analytically zero -- every `/biases` in front of a
              batch-statistics BN.  Their float64 gradient is 1e-16 .. 1e-17 of gmax, they are judged against 1e-5 gmax, and what a
              float32 evaluation leaves there is cancellation noise: 1e-2 per element, 3e-3 .. 7e-3 in L2.
    class R   everything else: weights, gamma, beta, FC biases.  float32 reaches 2e-5 per element and in L2.

BARS, as a rule (bars()):  class R element error and L2 <= 8 x the shape's class R floor (the float32 oracle and the step both
accumulate sums of the same lengths in float32, and the error is dominated by forward rounding carried through 50 layers, which
both share; 8 is for the different summation order: MFMA tiles, split-K, wgrad slabs) and never above R_BAR_MAX = 1e-3; class Z
<= 4 x the shape's class Z floor (pure cancellation noise, its size depends on the summation order); whole gradient <= 8 x the
whole-gradient floor.  The factors are not fitted to what the step gives.

FLOORS holds the floors as constants (tests/test_train_bars_cpu.py recomputes them and asserts the table within a factor 1.5), so
that a GPU test needs no float32 oracle pass.
"""
import contextlib

import numpy as np
import torch

from oracle import stabnet_oracle as O
from oracle import torch_ref as T

R_FACTOR, Z_FACTOR, WHOLE_FACTOR = 8.0, 4.0, 8.0
R_BAR_MAX = 1e-3                    # a twelfth of the smallest tail share measured (1.2e-2): no class R bar may exceed it
Z_CLASS_BELOW = 1e-9                # class Z: float64 max|g| < this x gmax
BATCH_SEED = 5

# the five weights whose tail share (rows M % 32 of each tower) test_train_bars_cpu.py measures: 1x1, stride 1
SAMPLED = tuple("resnet_v2_50/block%d/unit_1/bottleneck_v2/conv1/weights" % k for k in (1, 2, 3, 4)) + (
    "resnet_v2_50/block1/unit_1/bottleneck_v2/conv3/weights",)

# (N, H, W) -> float32-oracle floors: class R (worst element, worst tensor L2), class Z (same), whole gradient L2.
# Recomputed by tests/test_train_bars_cpu.py; batch seed 5, parameters seed 0, theta_scale 0.3, max_matches 48.
FLOORS = {
    (2, 64, 96): {"R": (2.09e-5, 1.55e-5), "Z": (2.72e-2, 7.05e-3), "whole": 1.01e-5},
    (3, 64, 96): {"R": (1.42e-5, 1.11e-5), "Z": (1.52e-2, 4.09e-3), "whole": 7.63e-6},
    (3, 90, 130): {"R": (2.79e-5, 1.86e-5), "Z": (2.16e-2, 6.02e-3), "whole": 1.49e-5},
    (1, 75, 101): {"R": (2.73e-5, 1.84e-5), "Z": (1.01e-2, 3.19e-3), "whole": 1.32e-5},
    (5, 40, 56): {"R": (1.56e-5, 8.56e-6), "Z": (2.35e-2, 6.61e-3), "whole": 5.61e-6},
}


def setup(N, H, W, seed=BATCH_SEED, bn_decay=None):
    """The step tests' inputs (tests/test_train_gpu.py _setup): -> cfg, oracle cfg, parameters, batch."""
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    kw = {} if bn_decay is None else {"bn_decay": bn_decay}
    cfg = Config(height=H, width=W, batch_size=N, max_matches=48, **kw)
    ocfg = O.Config(height=H, width=W, batch_size=N, max_matches=48)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    b = synthetic.make_train_batch(cfg, N, H, W, seed)
    b["flow"] = (b["flow"] + np.random.default_rng(1).normal(0, 0.02, b["flow"].shape)).astype(np.float32)
    return cfg, ocfg, P, b


def trainable(name):
    return not (name.endswith("/moving_mean") or name.endswith("/moving_variance"))


def oracle_gradient(P, b, ocfg, decisions=None, record=None, stats=None):
    """All gates on, in the precision T.DT names.  -> total, parts, {trainable name: gradient as float64 ndarray}."""
    pt = {k: T.t(v, requires_grad=True) for k, v in P.items()}
    total, parts = T.train_objective(pt, b, ocfg, 1.0, 1.0, 0.0, training=True, batch_stats=stats, decisions=decisions, record=record)
    total.backward()
    g = {k: (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)) for k, v in pt.items() if trainable(k)}
    return total, parts, g, pt


def tensor_errors(got, want):
    """tests/_decisions.gradient_errors on {name: array} dicts (TF layout: no channel padding).  want: float64.
    -> [(name, element error, relative L2)], whole-gradient relative L2, gmax."""
    gmax = max(np.abs(w).max() for w in want.values())
    rows, num, den = [], 0.0, 0.0
    for name in sorted(want):
        ww, gg = np.asarray(want[name], np.float64).ravel(), np.asarray(got[name], np.float64).ravel()
        scale = max(np.abs(ww).max(), 1e-5 * gmax)
        err = np.abs(gg - ww).max() / scale
        l2 = np.linalg.norm(gg - ww) / max(np.linalg.norm(ww), 1e-5 * gmax * np.sqrt(ww.size))
        rows.append((name, float(err), float(l2)))
        num += float(((gg - ww) ** 2).sum())
        den += float((ww ** 2).sum())
    return rows, float(np.sqrt(num / den)), gmax


def classes(want):
    """{name: 'Z' | 'R'} from float64 gradients only."""
    gmax = max(np.abs(w).max() for w in want.values())
    return {name: ("Z" if np.abs(w).max() < Z_CLASS_BELOW * gmax else "R") for name, w in want.items()}


def class_worst(rows, cls):
    """-> {'R': (worst element, worst L2, tensor of the worst element, tensor of the worst L2), 'Z': ...}"""
    out = {}
    for c in ("R", "Z"):
        mine = [r for r in rows if cls[r[0]] == c]
        e, l = max(mine, key=lambda r: r[1]), max(mine, key=lambda r: r[2])
        out[c] = (e[1], l[2], e[0], l[0])
    return out


@contextlib.contextmanager
def conv_taps(pt, names):
    """Inside the block T._conv keeps, for each of the named weights, the conv's input and the gradient of its output (one entry
    per call: tower 1, tower 2).  Test code only: the oracle file itself is not changed."""
    by_id = {id(pt[n]): n for n in names}
    taps = {n: [] for n in names}
    orig = T._conv

    def tapped(x, w, stride=1, pads=(0, 0, 0, 0), bias=None):
        y = orig(x, w, stride, pads, bias)
        name = by_id.get(id(w))
        if name is not None:
            slot = {"x": x.detach()}
            y.register_hook(lambda g, slot=slot: slot.__setitem__("dy", g.detach().clone()))
            taps[name].append(slot)
        return y

    T._conv = tapped
    try:
        yield taps
    finally:
        T._conv = orig


def tail_shares(taps, grads, P, ocfg):
    """{name: (tower rows M, share, dW of the tail rows [1,1,Cin,Cout])} for the 1x1 stride-1 convs tapped.  share = |dW from the
    last M % 32 pixel rows of each tower|_F over |dW from all rows|_F (dW = X^T dY summed over both towers).  Checked on the way: X^T dY plus the weight-decay term (the
    regulariser counts once per tower) IS the autograd gradient of the weight."""
    out = {}
    for name, slots in taps.items():
        assert len(slots) == 2, (name, len(slots))
        full = tail = 0.0
        for s in slots:
            x, dy = s["x"].reshape(-1, s["x"].shape[-1]).numpy(), s["dy"].reshape(-1, s["dy"].shape[-1]).numpy()
            M = x.shape[0]
            r = M % 32
            full = full + x.T @ dy
            if r:
                tail = tail + x[M - r:].T @ dy[M - r:]
        decay = 2.0 * ocfg.regu_mul * ocfg.weight_decay_conv * np.asarray(P[name], np.float64)[0, 0]
        assert np.linalg.norm(full + decay - grads[name][0, 0]) <= 1e-9 * np.linalg.norm(grads[name]), name
        out[name] = (M, float(np.linalg.norm(tail) / np.linalg.norm(full)) if M % 32 else 0.0, tail[None, None] if M % 32 else None)
    return out


def reference_floors(N, H, W, seed=BATCH_SEED, taps=False):
    """CPU, oracle only.  -> {'R': (element, L2), 'Z': (element, L2), 'whole': L2, 'flips': [...], 'n_flips': int, 'rows': [...],
    'classes': {...}, 'g32' / 'g64': the two gradients, 'tail': {name: (M, share, tail dW)} (taps=True)}."""
    from _decisions import flips
    cfg, ocfg, P, b = setup(N, H, W, seed)
    assert T.DT == torch.float64
    own = {}
    pt = {k: T.t(v, requires_grad=True) for k, v in P.items()}
    with conv_taps(pt, SAMPLED if taps else ()) as tapped:
        total, _ = T.train_objective(pt, b, ocfg, 1.0, 1.0, 0.0, training=True, record=own)
        total.backward()
    g64 = {k: v.grad.numpy().astype(np.float64) for k, v in pt.items() if trainable(k)}
    rec32 = {}
    # ONE thread for the float32 pass: the floors are maxima of rounding noise, and with the work cut over 2 .. 16 threads the
    # summation order, and with it the class Z element floor, moves by up to a factor 3 (3x90x130: 1.2e-2 .. 3.7e-2).  On one
    # thread the order is the library's own and the floors reproduce to the last digit whatever the machine's thread settings.
    threads = torch.get_num_threads()
    T.DT = torch.float32
    torch.set_num_threads(1)
    try:
        _, _, g32, _ = oracle_gradient(P, b, ocfg, decisions=own, record=rec32)
    finally:
        T.DT = torch.float64
        torch.set_num_threads(threads)
    rows, whole, _ = tensor_errors(g32, g64)
    cls = classes(g64)
    worst = class_worst(rows, cls)
    flipped = flips(rec32, own)
    res = {"R": worst["R"][:2], "Z": worst["Z"][:2], "whole": whole, "flips": flipped, "n_flips": sum(n for _, _, n, _ in flipped),
           "rows": rows, "classes": cls, "worst": worst, "g32": g32, "g64": g64}
    if taps:
        res["tail"] = tail_shares(tapped, g64, P, ocfg)
    return res


def bars(N, H, W):
    """The bars in force at a shape, from the committed floors: {'R': (element, L2), 'Z': (element, L2), 'whole': L2}."""
    f = FLOORS[(N, H, W)]
    out = {"R": tuple(R_FACTOR * v for v in f["R"]), "Z": tuple(Z_FACTOR * v for v in f["Z"]), "whole": WHOLE_FACTOR * f["whole"]}
    assert max(out["R"]) <= R_BAR_MAX, (N, H, W, out["R"])
    return out


def measure_gradient(got, want):
    """got against want (float64, the forward's decisions forced) -> {'rows', 'classes', 'R': (element, L2, tensor, tensor),
    'Z': ..., 'whole': L2}: what check_gradient asserts, for printing first."""
    rows, whole, _ = tensor_errors(got, want)
    cls = classes(want)
    worst = class_worst(rows, cls)
    return {"rows": rows, "classes": cls, "R": worst["R"], "Z": worst["Z"], "whole": whole}


def check_gradient(m, N, H, W, which=("R", "Z", "whole")):
    """Assert every trainable tensor of the measurement m (measure_gradient) against its class bar at this shape."""
    bar = bars(N, H, W)
    rows, cls, whole = m["rows"], m["classes"], m["whole"]
    for name, err, l2 in rows:
        c = cls[name]
        if c in which:
            assert err <= bar[c][0], "%s (class %s): element err %.3e > %.3e with the forward's decisions forced" % (name, c, err, bar[c][0])
            assert l2 <= bar[c][1], "%s (class %s): relative L2 err %.3e > %.3e with the forward's decisions forced" % (name, c, l2, bar[c][1])
    if "whole" in which:
        assert whole <= bar["whole"], "whole gradient %.3e > %.3e" % (whole, bar["whole"])


def report(tag, m, N, H, W):
    f = FLOORS[(N, H, W)]
    return ("%s: class R element %.3e L2 %.3e (floor %.3e / %.3e; %s)  class Z element %.3e L2 %.3e (floor %.3e / %.3e)  whole %.3e (floor %.3e)"
            % (tag, m["R"][0], m["R"][1], f["R"][0], f["R"][1], m["R"][2].replace("resnet_v2_50/", "").replace("bottleneck_v2/", ""),
               m["Z"][0], m["Z"][1], f["Z"][0], f["Z"][1], m["whole"], f["whole"]))
