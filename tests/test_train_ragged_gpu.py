"""GPU: one full training step at RAGGED sizes -- odd batch, H and W no multiple of 32, so that none of the five halvings lands on
an even size -- against the float64 autograd oracle, into poisoned workspaces, with per-tensor bars derived from a float32
reference (tests/_train_bars.py) and with the launches the step really made counted and compared with the routing predicates.

The step decides its kernels from the tower rows M = N x h x w of each layer (csrc/net.hip, csrc/conv_bwd.hip): a forward conv is
ONE launch for both towers only where M % 64 == 0; the stride-1 wgrad kernel (conv_wgrad_same_f32_kernel) needs M % 32 == 0, and
every other layer runs the general conv_wgrad_f32_kernel, with wgrad_splits() pixel splits per tower, slabs [tower][split] and a
reduce entry when there is more than one; the separate bias reduction runs where conv3's wgrad cannot carry it; slim's SAME
max-pool pads on top / left only when the stem's output is odd.  The suite's other step tests (2x64x96, 4x96x160, 8x288x512) keep
every M a multiple of 32 wherever M >= 64.

    N x H x W     tower rows: pool / block1 / 2 / 3   what it reaches
    3 x 64 x 96   1152 / 288 / 72 / 18                odd batch only: block 1 pairs, block 2 (M % 64 = 32) gets per-tower forward
                                                      launches with the stride-1 wgrad, FC head over 6 rows
    3 x 90 x 130  2277 / 612 / 162 / 45               nothing divides: general wgrad with several ragged splits, separate bias
                                                      reduction at large M, pool pad on top and left, odd sizes into every stride-2 unit
    1 x 75 x 101  494 / 130 / 35 / 12                 N = 1, odd width from the input on (odd stem row pitch), stem output 38 x 51
    5 x 40 x 56   700 / 175 / 60 / 20                 odd batch, small odd maps, the last stage 2 x 2
    3 x 90 x 130, split_operands=True                 the packed split dgrad / 1x1 forward route and its fallbacks at ragged M

Per parameter (max_matches 48, parameters seed 0 / theta_scale 0.3, batch seed 5 + flow noise, all gates on, bn_decay 0.9 -- the
reasoning is in tests/test_train_trajectory_gpu.py): POISON (both workspaces, grads, regu_val, wd_ws, both theta buffers filled with
0xFF; a second Trainer that is never poisoned gives the same gradient, theta, losses and parameters bit for bit); FORWARD (theta,
loss terms, total: the bars of tests/test_train_gpu.py); GRADIENT (the step's decisions forced onto the oracle; every tensor
against its class bar: class R <= 8 x the shape's float32 floor and <= 1e-3, class Z <= 4 x, whole gradient <= 8 x; un-forced:
whole < 5e-3, cosine > 1 - 1e-5; at most 200 flips); MOVING STATISTICS (every mean and variance, tower 1's update then tower 2's,
1e-5 absolute); ADAM (a third trainer's update is the oracle's AdamTF step of the GPU's own gradient to 1 ulp); ROUTES (below).

ROUTES.  deploy.Profiler records every conv / wgrad launch with its GEMM shape.  The wgrad records of the step must be EXACTLY the
restatement _wgrad_launches() makes of the predicates over the unit table: which kernel (stride 1, output = input, M % 32 == 0,
32 / w + 1 < h -> the stride-1 kernel, else the general one), Cout, K, 2 M, and 2 x wgrad_splits() slabs.  Forward launches named
conv_igemm_f32_pair_kernel (the 3x3 pairs; 1x1 pairs run the ring kernel's prologue form under its own name) number at least the
3x3 layers with M % 64 == 0 and at most all layers with M % 64 == 0.  At the three ragged sizes both counts are 0 and at least one
stride-1 layer runs the general wgrad with more than one pixel split; at 3 x 64 x 96 pair, stride-1-kernel and general stride-1
launches are all positive.

MEASURED when the test was written (f32 MFMA step unless `split`; decisions forced; worst element / worst tensor L2 of each class
with the float32-oracle floor in brackets; whole gradient; flipped decisions; launches pair / stride-1 wgrad / general wgrad, the
stem's included; un-forced whole gradient and 1 - cosine; worst moving statistic):

    3x64x96        R 1.10e-5 / 9.80e-6 (1.42e-5 / 1.11e-5)  Z 7.2e-3 / 2.6e-3 (1.52e-2 / 4.09e-3)  whole 7.02e-6 (7.63e-6)   2 flips
                   launches 2 / 20 / 33   un-forced 5.0e-4, 1.3e-7   moving 9.9e-7
    3x90x130       R 2.36e-5 / 2.00e-5 (2.79e-5 / 1.86e-5)  Z 9.0e-3 / 3.1e-3 (2.16e-2 / 6.02e-3)  whole 1.21e-5 (1.49e-5)  11 flips
                   launches 0 / 0 / 53    un-forced 3.7e-3, 6.9e-6   moving 6.7e-7
    1x75x101       R 2.77e-5 / 1.99e-5 (2.73e-5 / 1.84e-5)  Z 5.8e-3 / 2.0e-3 (1.01e-2 / 3.19e-3)  whole 1.39e-5 (1.32e-5)   3 flips
                   launches 0 / 0 / 53    un-forced 1.6e-3, 1.2e-6   moving 1.3e-6
    5x40x56        R 1.30e-5 / 1.02e-5 (1.56e-5 / 8.56e-6)  Z 7.8e-3 / 3.0e-3 (2.35e-2 / 6.61e-3)  whole 7.54e-6 (5.61e-6)   1 flip
                   launches 0 / 0 / 53    un-forced 1.9e-4, 1.8e-8   moving 7.4e-7
    3x90x130 split R 2.14e-5 / 1.46e-5 (2.79e-5 / 1.86e-5)  Z 8.6e-3 / 3.1e-3 (2.16e-2 / 6.02e-3)  whole 1.25e-5 (1.49e-5)   9 flips
                   launches 0 / 0 / 53    un-forced 1.7e-3, 1.5e-6   moving 4.5e-7

The step sits AT the float32 floor in class R (0.8 .. 1.2 x) and below it in class Z: the factors 8 and 4 of the rule are not used
up, and the class R bars in force are 1.1e-4 .. 2.2e-4 per element, 6.8e-5 .. 1.5e-4 in L2 -- all under 1e-3.  The un-forced
comparison at 3x90x130 (11 flips) comes to 3.7e-3 / 1 - 6.9e-6 against the project's 5e-3 / 1 - 1e-5: the
step is reproducible bit for bit, so the set of flips is fixed.  2 .. 3.6 s per parameter.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _train_bars as B
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu

BN_DECAY = 0.9
BN_BAR = 1e-5
CASES = [(3, 64, 96, False), (3, 90, 130, False), (1, 75, 101, False), (5, 40, 56, False), (3, 90, 130, True)]
RAGGED = {(3, 90, 130), (1, 75, 101), (5, 40, 56)}


def _cdiv(a, b):
    return -(-a // b)


def _units(N, H, W):
    """The bottleneck units' geometry restated from the graph (slim resnet_v2_50: 7x7 / 2 stem with explicit padding 3, 3x3 / 2 SAME
    max-pool, stride on the LAST unit of a block, 3x3 with explicit padding 1): [(h, w, cin, dbn, depth, stride, ho, wo, proj)],
    and the stem's output size."""
    h1, w1 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    h, w, cin = _cdiv(h1, 2), _cdiv(w1, 2), 64
    units = []
    for bname, depth, dbn, n_units, bstride in O.RESNET_V2_50_BLOCKS:
        for u in range(1, n_units + 1):
            s = bstride if u == n_units else 1
            ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
            units.append((h, w, cin, dbn, depth, s, ho, wo, depth != cin))
            h, w, cin = ho, wo, depth
    return units, (h1, w1)


def _wgrad_splits(Cout, K, M):
    """csrc/conv_bwd.hip wgrad_splits(): ~1024 blocks in all, at least 256 pixel rows per block, whole 32-row steps."""
    tiles = _cdiv(Cout, 64) * _cdiv(K, 64)
    splits = max(1, min(_cdiv(1024, tiles), _cdiv(M, 256)))
    rps = _cdiv(_cdiv(M, splits), 32) * 32
    return _cdiv(M, rps), rps


def _wgrad_launches(N, H, W):
    """The wgrad launches of the units, restated: [(same kernel?, Cout, K, rows of both towers, slabs of both towers, stride, rows per split)]."""
    out = []
    units, _ = _units(N, H, W)
    for h, w, cin, dbn, depth, s, ho, wo, proj in units:
        layers = [(ho, wo, dbn, depth, 1, 1), (h, w, dbn, dbn, 3, s), (h, w, cin, dbn, 1, 1)] + ([(h, w, cin, depth, 1, 1)] if proj else [])
        for lh, lw, ci, co, k, st in layers:
            pad = 1 if k == 3 else 0
            oh, ow = (lh + 2 * pad - k) // st + 1, (lw + 2 * pad - k) // st + 1
            M, K = N * oh * ow, k * k * ci
            same = st == 1 and oh == lh and ow == lw and M % 32 == 0 and co % 64 == 0 and K % 64 == 0 and 32 // lw + 1 < lh
            splits, rps = _wgrad_splits(co, K, M)
            out.append((same, co, K, 2 * M, 2 * splits, st, rps))
    return out


def _forward_rows(N, H, W):
    """Tower rows of every unit conv's output: ([all layers], [the 3x3 layers])."""
    every, k3 = [], []
    for h, w, cin, dbn, depth, s, ho, wo, proj in _units(N, H, W)[0]:
        every += [N * h * w, N * ho * wo, N * ho * wo] + ([N * ho * wo] if proj else [])
        k3.append(N * ho * wo)
    return every, k3


def test_the_restated_table_is_the_issue_s():
    """The rows the module docstring lists (no GPU work: the restatement itself)."""
    want = {(3, 64, 96): (1152, 288, 72, 18), (3, 90, 130): (2277, 612, 162, 45), (1, 75, 101): (494, 130, 35, 12), (5, 40, 56): (700, 175, 60, 20)}
    for (N, H, W), rows in want.items():
        units, stem = _units(N, H, W)
        got = tuple(N * units[i][0] * units[i][1] for i in (0, 3, 7, 13))
        assert got == rows, (N, H, W, got)
    assert _units(1, 75, 101)[1] == (38, 51) and _units(3, 90, 130)[1] == (45, 65)


@pytest.mark.parametrize("N,H,W,split", CASES)
def test_ragged_step_matches_float64(cuda, N, H, W, split):
    from _decisions import flips, gpu_decisions
    from stabnet_amd.deploy import Profiler
    from stabnet_amd.regressor import KIND_MEAN, KIND_VAR
    from stabnet_amd.train import Trainer
    from test_train_trajectory_gpu import _moving, _poison
    cfg, ocfg, P, b = B.setup(N, H, W, bn_decay=BN_DECAY)
    gates = {"use_theta_loss": 1, "use_temp_loss": 1, "use_black_loss": 1, "use_theta_only": 0}
    stats, own = {}, {}
    total, parts, want_g, _ = B.oracle_gradient(P, b, ocfg, record=own, stats=stats)

    dev_b = {k: torch.from_numpy(v).to(cuda) for k, v in b.items()}
    tr = Trainer(P, N, H, W, cfg, device=cuda, split_operands=split)
    clean = Trainer(P, N, H, W, cfg, device=cuda, split_operands=split)             # never poisoned
    assert tr.split_operands == split
    nt = tr.nt
    p0 = tr.params.clone()
    _poison(tr)
    prof = Profiler(8000)
    tr.prof = prof
    tr.forward_backward(dev_b, gates, apply_update=False)
    torch.cuda.synchronize()
    tr.prof = None
    clean.forward_backward(dev_b, gates, apply_update=False)
    torch.cuda.synchronize()
    recs = prof.records_with_shapes()
    got_flat = tr.grad_flat().cpu().numpy().copy()
    assert np.isfinite(got_flat).all() and np.isfinite(tr.theta[0].cpu().numpy()).all() and np.isfinite(tr.theta[1].cpu().numpy()).all()

    # ---- poison: the poisoned trainer and the clean one agree bit for bit
    lo = tr.losses()
    assert torch.equal(tr.grads, clean.grads) and torch.equal(tr.theta[0], clean.theta[0]) and torch.equal(tr.theta[1], clean.theta[1])
    assert torch.equal(tr.params, clean.params)
    assert clean.losses() == lo

    # ---- forward: theta of both towers, the loss terms, the total (bars of tests/test_train_gpu.py)
    for k, key in enumerate(("tower1", "tower2")):
        assert np.abs(tr.theta[k].cpu().numpy() - parts[key]["theta"].detach().numpy()).max() < 5e-5, key
        assert lo[key]["img_loss"] == pytest.approx(float(parts[key]["img"].detach()) * cfg.img_mul, rel=2e-3), key
        assert lo[key]["feature_loss"] == pytest.approx(float(parts[key]["feature"].detach()), rel=2e-3), key
    assert lo["total_loss"] == pytest.approx(float(total.detach()), rel=2e-3)
    assert lo["regu_loss"] == pytest.approx(2 * float(parts["regu_loss"].detach()) * cfg.regu_mul, rel=2e-3)
    assert float(parts["temp_loss"].detach()) > 0
    assert lo["temp_loss"] == pytest.approx(float(parts["temp_loss"].detach()) * cfg.temp_mul, rel=5e-3, abs=1e-6)

    # ---- gradient (a): against float64 of the piece the step's forward took, every tensor with its class bar
    full = np.zeros(tr.plan.n_floats, np.float32)
    full[:nt] = got_flat
    got_g = {n: v for n, v in tr.plan.unpack(full).items() if B.trainable(n)}
    assert set(got_g) == set(want_g)
    # (the flat buffer holds nothing but these tensors: the channel padding of the stem's weights received exactly zero)
    assert np.array_equal(tr.plan.pack({n: got_g.get(n, np.zeros_like(P[n])) for n in P})[:nt], got_flat)
    dec = gpu_decisions(tr)
    flipped = flips(dec, own)
    n_flips = sum(n for _, _, n, _ in flipped)
    print("%dx%dx%d split=%d DECISIONS that differ between the float32 forward and float64 (%d): %s" % (N, H, W, split, n_flips, flipped))
    _, _, forced_g, _ = B.oracle_gradient(P, b, ocfg, decisions=dec)
    m = B.measure_gradient(got_g, forced_g)
    print(B.report("MEASURED %dx%dx%d split=%d (decisions forced)" % (N, H, W, split), m, N, H, W))
    rows_u, whole_u, _ = B.tensor_errors(got_g, want_g)
    names = sorted(want_g)
    gv, wv = np.concatenate([got_g[n].ravel().astype(np.float64) for n in names]), np.concatenate([want_g[n].ravel() for n in names])
    cos = float(np.dot(gv, wv) / (np.linalg.norm(gv) * np.linalg.norm(wv)))
    print("MEASURED %dx%dx%d split=%d (un-forced) worst element %.3e worst tensor L2 %.3e whole L2 %.3e cosine 1 - %.2e"
          % (N, H, W, split, max(r[1] for r in rows_u), max(r[2] for r in rows_u), whole_u, 1 - cos))

    # ---- routes: what ran (counted before the numerical asserts, so that a failing bar still says which kernels it judged)
    names_r = [r[0] for r in recs]
    n_pair = sum(1 for n in names_r if n.startswith("conv_igemm_f32_pair_kernel"))
    wg = [(r[0].startswith("conv_wgrad_same_f32_kernel"),) + tuple(r[4]) for r in recs if r[0].startswith("conv_wgrad_")]
    n_same, n_general = sum(1 for w in wg if w[0]), sum(1 for w in wg if not w[0])
    print("LAUNCHES %dx%dx%d split=%d: pair %d, stride-1 wgrad %d, general wgrad %d (of %d records)" % (N, H, W, split, n_pair, n_same, n_general, len(recs)))
    assert len(recs) < 8000                                                           # the profiler kept every launch
    want_wg = _wgrad_launches(N, H, W)
    stem_rows = 2 * N * _units(N, H, W)[1][0] * _units(N, H, W)[1][1]
    stem = [w for w in wg if w[1] == 64 and w[3] == stem_rows]
    assert len(stem) == 1 and not stem[0][0], stem                                    # the 7x7 / 2 stem: the general kernel
    wg.remove(stem[0])
    assert sorted(wg) == sorted(w[:5] for w in want_wg), "the wgrad launches are not what the predicates say"
    every, k3 = _forward_rows(N, H, W)
    pairable, pairable3 = sum(1 for M in every if M % 64 == 0), sum(1 for M in k3 if M % 64 == 0)
    assert pairable3 <= n_pair <= pairable, (n_pair, pairable3, pairable)
    general_s1_split = [w for w in want_wg if not w[0] and w[5] == 1 and w[4] > 2]
    if (N, H, W) in RAGGED:
        assert n_pair == 0 and n_same == 0 and pairable == 0
        assert general_s1_split and any(w[3] // 2 % w[6] != 0 for w in general_s1_split)     # several splits, the last one short
    else:
        assert n_pair > 0 and n_same > 0 and sum(1 for w in want_wg if not w[0] and w[5] == 1) > 0

    # ---- gradient bars
    assert n_flips <= 200, flipped
    B.check_gradient(m, N, H, W)
    # (b) un-forced: the project's whole-gradient bars
    assert whole_u < 5e-3, whole_u
    assert cos > 1 - 1e-5, "gradient cosine %r" % cos

    # ---- moving statistics: every BN layer, mean and variance, tower 1's update then tower 2's
    moving_names = [name for name, off, kind, dims, aux in tr.plan.table if kind in (KIND_MEAN, KIND_VAR)]
    assert moving_names and set(moving_names) == {n for n in P if not B.trainable(n)}
    after = tr.plan.unpack(tr.params.cpu().numpy())
    worst_bn = 0.0
    for name in moving_names:
        prefix, which = name.rsplit("/", 1)
        j = 0 if which == "moving_mean" else 1
        want_m = _moving(P[name], stats["1"][prefix][j], stats["2"][prefix][j], cfg.bn_decay)
        err = float(np.abs(after[name] - want_m).max())
        worst_bn = max(worst_bn, err)
        assert err < BN_BAR, (name, err)
    print("MEASURED %dx%dx%d split=%d moving statistics: worst absolute error %.2e" % (N, H, W, split, worst_bn))
    assert torch.equal(tr.params[:nt], p0[:nt])                   # apply_update=False left the trainables alone

    # ---- Adam: a third trainer's applied update is the oracle's TF Adam step of the GPU's own gradient
    tr3 = Trainer(P, N, H, W, cfg, device=cuda, split_operands=split)
    tr3.forward_backward(dev_b, gates, apply_update=True)
    torch.cuda.synchronize()
    assert np.array_equal(tr3.grad_flat().cpu().numpy(), got_flat)
    adam = O.AdamTF(nt)
    want_w = adam.step(p0[:nt].cpu().numpy(), got_flat, float(O.exponential_decay_staircase(cfg.initial_learning_rate, 0, cfg.step_size, 0.1)))
    got_w = tr3.params[:nt].cpu().numpy()
    assert (np.abs(got_w - want_w) <= np.spacing(np.abs(want_w))).all()
    assert np.array_equal(tr3.adam_m.cpu().numpy(), adam.m) and np.array_equal(tr3.adam_v.cpu().numpy(), adam.v)
    assert torch.equal(tr3.params[nt:], tr.params[nt:])
