"""GPU: three CONSECUTIVE training steps, each against the float64 autograd oracle, with the Trainer's own schedule.

tests/test_train_gpu.py compares step 1 of a fresh Trainer with float64, and checks later steps only against themselves, on one
batch.  Here the schedule boundaries sit inside three steps (do_theta_only_iter = 0, do_black_loss_iter = do_temp_loss_iter = 2,
step_size = 2), the gates are the Trainer's own (gates=None), and every step has its own batch:

    step 0  theta-only                      lr0
    step 1  live, black loss off, temp off  lr0
    step 2  everything on                   lr0 * 0.1

TEACHER FORCING.  A float32 and a float64 trajectory diverge legitimately (ReLU / arg-max flips), so they are never compared over
several steps: before step k the GPU's parameters are read back, the oracle is evaluated at exactly those parameters on step k's
batch with step k's gates, and the results of that ONE step are compared, with the bars of test_training_step_matches_autograd_oracle.

WORKSPACE POISON.  The training workspace (TrainLayout, csrc/net.hip) holds activations, the BN scale / shift / mean / invstd of
the step, gradient scratch, reduction partials, split-K and wgrad slabs, re-packed weights and the arg-max bytes: every region is
written by the step that reads it, and the Trainer allocates it uninitialised.  NOTHING in tr.ws outlives a step -- the state
that does is tr.params (moving statistics in its tail), adam_m, adam_v and global_step.  So before every step both workspaces, the
gradient buffer, regu_val (forward_backward clears those two), the weight-decay partials and the theta outputs are filled with
0xFF bytes (NaN as float32, 255 as arg-max bytes); the three steps must pass unchanged, and a second trainer that is never
poisoned must give the same bits.

MEASURED when the test was written (f32 MFMA step; decisions forced: worst element / worst tensor L2 / whole gradient; un-forced
whole gradient; flipped decisions): step 0  1.8e-2 / 4.6e-3 / 3.8e-6, 9.6e-4, 3 flips;  step 1  3.8e-3 / 1.4e-3 / 4.5e-6, 7.6e-4,
2 flips;  step 2  1.3e-2 / 4.4e-3 / 9.4e-6, 2.5e-4, 5 flips -- no step is worse than the single step of test_train_gpu.py (1.7e-2 /
4.9e-3 / 1.0e-5).  Split operands, step 0: 1.1e-2 / 4.3e-3 / 4.1e-6.  Smallest moving-statistics change a candidate error would cause
at decay 0.9: second tower missing 4.7e-2, order swapped 5.7e-4, variance of the wrong tower 3.0e-2 (at 0.997 a swapped order moves
some tensor by 5e-7 only: under the bar).  Wall time 7 s per run (six float64 backward passes) against 2.7 s of the single-step test."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import stabnet_oracle as O
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu

N, H, W = 2, 64, 96                 # the step test's size: the smallest at which all four ResNet blocks have more than one pixel
SEEDS = (5, 6, 7)                   # one batch per step: what step k - 1 left behind is not step k's data
BN_BAR = 1e-5                       # moving statistics, absolute (test_train_gpu.py)
# 0.9, not the reference's 0.997: at 0.997 one update moves a statistic by 0.3 % of its distance to the batch statistic, and a
# missing second-tower update or a swapped order changes several tensors by less than BN_BAR.  _bn_sensitivity() asserts, on
# oracle values, that at this decay each of those errors moves EVERY moving tensor it concerns by >= 10 x BN_BAR.
BN_DECAY = 0.9


def _configs():
    from stabnet_amd.config import Config
    cfg = Config(height=H, width=W, batch_size=N, max_matches=48, do_theta_only_iter=0, do_black_loss_iter=2,
                 do_temp_loss_iter=2, step_size=2, bn_decay=BN_DECAY)
    ocfg = O.Config(height=H, width=W, batch_size=N, max_matches=48)
    return cfg, ocfg


def _batches(cfg):
    from stabnet_amd import synthetic
    out = []
    for seed in SEEDS:
        b = synthetic.make_train_batch(cfg, N, H, W, seed)
        b["flow"] = (b["flow"] + np.random.default_rng(1).normal(0, 0.02, b["flow"].shape)).astype(np.float32)
        out.append(b)
    return out


def _oracle(P, b, ocfg, g, decisions=None, stats=None, record=None):
    """float64 objective and gradient at the float32 parameters P with the gates g.  -> total, parts, {name: gradient}."""
    pt = {k: T.t(v, requires_grad=True) for k, v in P.items()}
    total, parts = T.train_objective(pt, b, ocfg, float(g["use_temp_loss"]), float(g["use_black_loss"]), float(g["use_theta_only"]),
                                     training=True, batch_stats=stats, decisions=decisions, record=record)
    total.backward()
    return total, parts, {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in pt.items()}


def _moving(m0, s1, s2, decay):
    """slim's assign_moving_average, tower 1's update then tower 2's (UPDATE_OPS order, s_net_bundle_nobm.py:355-357)."""
    m = np.asarray(m0, np.float64)
    for s in (s1, s2):
        m = m - (m - s) * (1 - decay)
    return m


def _bn_sensitivity(before, stats, moving_names, decay):
    """Input condition, oracle values only: the smallest change, over the moving tensors concerned, that each candidate error
    would cause (a tensor's change = its largest element change, which is what the BN_BAR check sees)."""
    worst = {"tower 2 not applied": np.inf, "order swapped": np.inf, "variance of the wrong tower": np.inf}
    for name in moving_names:
        prefix, which = name.rsplit("/", 1)
        j = 0 if which == "moving_mean" else 1
        s1, s2 = stats["1"][prefix][j], stats["2"][prefix][j]
        right = _moving(before[name], s1, s2, decay)
        m0 = np.asarray(before[name], np.float64)
        worst["tower 2 not applied"] = min(worst["tower 2 not applied"], np.abs(right - (m0 - (m0 - s1) * (1 - decay))).max())
        worst["order swapped"] = min(worst["order swapped"], np.abs(right - _moving(before[name], s2, s1, decay)).max())
        if j == 1:                  # tower 2's update reads tower 1's variance
            worst["variance of the wrong tower"] = min(worst["variance of the wrong tower"],
                                                       np.abs(right - _moving(before[name], s1, s1, decay)).max())
    return worst


def _poison(tr):
    for t in (tr.ws[0], tr.ws[1], tr.grads, tr.regu_val, tr.wd_ws, tr.theta[0], tr.theta[1]):
        t.view(torch.uint8).fill_(0xFF)


def _run(cuda, split):
    from _decisions import flips, gpu_decisions, gradient_errors
    from stabnet_amd import synthetic
    from stabnet_amd.regressor import KIND_MEAN, KIND_VAR
    from stabnet_amd.train import Trainer, loss_gates
    cfg, ocfg = _configs()
    P0 = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    batches = _batches(cfg)
    dev = [{k: torch.from_numpy(v).to(cuda) for k, v in b.items()} for b in batches]
    want_gates = [{"use_theta_loss": 1, "use_temp_loss": 0, "use_black_loss": 0, "use_theta_only": 1},
                  {"use_theta_loss": 1, "use_temp_loss": 0, "use_black_loss": 0, "use_theta_only": 0},
                  {"use_theta_loss": 1, "use_temp_loss": 1, "use_black_loss": 1, "use_theta_only": 0}]
    tr = Trainer(P0, N, H, W, cfg, device=cuda, split_operands=split)
    clean = Trainer(P0, N, H, W, cfg, device=cuda, split_operands=split)            # never poisoned
    assert tr.split_operands == split
    nt = tr.nt
    moving_names = [name for name, off, kind, dims, aux in tr.plan.table if kind in (KIND_MEAN, KIND_VAR)]
    assert moving_names and set(moving_names) == {n for n in P0 if n.endswith("/moving_mean") or n.endswith("/moving_variance")}
    adam = O.AdamTF(nt)                                                             # ONE instance for the three steps
    lrs = []
    for k in range(3):
        g = loss_gates(k, cfg)
        assert g == want_gates[k]
        flat0 = tr.params.cpu().numpy().copy()
        before = tr.plan.unpack(flat0)
        b = batches[k]
        stats, own = {}, {}
        total, parts, want_g = _oracle(before, b, ocfg, g, stats=stats, record=own)

        _poison(tr)
        tr.forward_backward(dev[k])                                                 # gates=None: the Trainer's own schedule
        clean.forward_backward(dev[k])
        torch.cuda.synchronize()
        assert tr.last["gates"] == want_gates[k]
        assert tr.global_step == clean.global_step == k + 1

        # ---- theta and every loss term
        for j, key in enumerate(("tower1", "tower2")):
            assert np.abs(tr.theta[j].cpu().numpy() - parts[key]["theta"].detach().numpy()).max() < 5e-5, (k, key)
        lo = tr.losses()
        print("step %d losses %s" % (k, {a: v for a, v in lo.items() if not isinstance(v, dict)}))
        assert lo["total_loss"] == pytest.approx(float(total), rel=2e-3), k
        assert lo["regu_loss"] == pytest.approx(2 * float(parts["regu_loss"]) * cfg.regu_mul, rel=2e-3), k
        want_temp = float(parts["temp_loss"]) * cfg.temp_mul
        if g["use_temp_loss"]:
            assert want_temp > 0
            assert lo["temp_loss"] == pytest.approx(want_temp, rel=5e-3, abs=1e-6), k
        else:
            assert lo["temp_loss"] == 0.0 and want_temp == 0.0, k
        for key in ("tower1", "tower2"):
            p, t = parts[key], lo[key]
            want = {"theta_loss": float(p["theta"].abs().mean()) * cfg.id_mul * cfg.theta_mul,
                    "grid_theta_loss": float(p["theta"].abs().mean()) * cfg.id_mul * cfg.grid_theta_mul,
                    "black_loss": float(p["black_pos_loss"]) * cfg.black_mul, "distortion_loss": float(p["distortion"]) * cfg.distortion_mul,
                    "consistency_loss": float(p["consistency"]) * cfg.consistency_mul, "feature_loss": float(p["feature"]) * cfg.feature_mul,
                    "img_loss": float(p["img"]) * cfg.img_mul, "total_loss": float(p["total"])}
            assert set(want) == set(t)
            for term, w in want.items():
                if term == "grid_theta_loss" or (term == "black_loss" and not g["use_black_loss"]):
                    assert t[term] == 0.0 and w == 0.0, (k, key, term, t[term], w)          # gated off: exactly 0 on both sides
                else:
                    assert t[term] == pytest.approx(w, rel=2e-3), (k, key, term)
        if g["use_theta_only"]:
            assert lo["total_loss"] == lo["tower1"]["theta_loss"] + lo["tower2"]["theta_loss"]

        # ---- gradient: (a) against float64 of the piece the GPU forward took, (b) un-forced, whole-gradient bars
        got = tr.grad_flat().cpu().numpy().copy()
        want_flat = tr.plan.pack({n: want_g[n] for n in P0})[:nt]
        dec = gpu_decisions(tr)
        flipped = flips(dec, own)
        print("step %d DECISIONS that differ between the float32 forward and float64: %s" % (k, flipped))
        assert sum(n for _, _, n, _ in flipped) <= 200, (k, flipped)
        _, _, forced_g = _oracle(before, b, ocfg, g, decisions=dec)
        forced_flat = tr.plan.pack({n: forced_g[n] for n in P0})[:nt]
        worst_abs, worst_l2, whole, rows = gradient_errors(tr.plan, got, forced_flat)
        print("step %d MEASURED (decisions forced) worst element %.3e worst tensor L2 %.3e whole L2 %.3e" % (k, worst_abs, worst_l2, whole))
        for name, err, l2 in rows:
            assert err < 2e-2, "step %d %s: element err %g with the forward's decisions forced" % (k, name, err)
            assert l2 < 6e-3, "step %d %s: relative L2 err %g with the forward's decisions forced" % (k, name, l2)
        assert whole < 1e-4, (k, whole)
        u_abs, u_l2, whole_u, _ = gradient_errors(tr.plan, got, want_flat)
        cos = float(np.dot(got, want_flat) / (np.linalg.norm(got) * np.linalg.norm(want_flat)))
        print("step %d MEASURED (un-forced) worst element %.3e worst tensor L2 %.3e whole L2 %.3e cosine 1 - %.2e" % (k, u_abs, u_l2, whole_u, 1 - cos))
        assert whole_u < 5e-3, (k, whole_u)
        assert cos > 1 - 1e-5, (k, cos)

        # ---- Adam with the staircase learning rate, fed the GPU's own gradient
        lr = float(O.exponential_decay_staircase(cfg.initial_learning_rate, k, cfg.step_size, 0.1))
        lrs.append(lr)
        want_w = adam.step(flat0[:nt], got, lr)
        flat1 = tr.params.cpu().numpy()
        assert (np.abs(flat1[:nt] - want_w) <= np.spacing(np.abs(want_w))).all(), k
        assert np.array_equal(tr.adam_m.cpu().numpy(), adam.m) and np.array_equal(tr.adam_v.cpu().numpy(), adam.v), k

        # ---- moving statistics: every BN layer, mean and variance, tower 1 then tower 2
        sens = _bn_sensitivity(before, stats, moving_names, cfg.bn_decay)
        print("step %d smallest moving-statistics change a candidate error would cause: %s" % (k, sens))
        assert min(sens.values()) >= 10 * BN_BAR, (k, sens)
        after = tr.plan.unpack(flat1)
        checked = set()
        for name in moving_names:
            prefix, which = name.rsplit("/", 1)
            j = 0 if which == "moving_mean" else 1
            want_m = _moving(before[name], stats["1"][prefix][j], stats["2"][prefix][j], cfg.bn_decay)
            assert np.abs(after[name] - want_m).max() < BN_BAR, (k, name, float(np.abs(after[name] - want_m).max()))
            checked.add(name)
        assert checked == {name for name, off, kind, dims, aux in tr.plan.table if "/moving_" in name}

        # ---- the poisoned trainer and the clean one agree bit for bit
        assert torch.equal(tr.params, clean.params) and torch.equal(tr.adam_m, clean.adam_m) and torch.equal(tr.adam_v, clean.adam_v), k
        assert torch.equal(tr.grads, clean.grads) and torch.equal(tr.theta[0], clean.theta[0]) and torch.equal(tr.theta[1], clean.theta[1]), k
        lc = clean.losses()
        assert lc == lo, k
    assert lrs[0] == lrs[1] and lrs[2] == pytest.approx(lrs[0] * 0.1, rel=1e-6)      # the checked steps include the drop


def test_three_steps_each_match_float64(cuda):
    _run(cuda, split=False)


def test_three_steps_each_match_float64_split_operands(cuda):
    """The same three steps on the opt-in packed split kernels (Trainer(split_operands=True)), same references, same bars."""
    _run(cuda, split=True)
