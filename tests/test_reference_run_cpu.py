"""CPU: the oracle and torch_ref against the reference's OWN warp and loss code, executed.

oracle/run_reference.py runs the reference's files, imported unchanged, on tests/tf_eager_standin.py (an eager NumPy stand-in for the
tf.* calls they make) in a child process, in two modes: f32 (one float32 rounding per op) and f64 (the same text in float64).  What it
computed is committed as tests/golden/reference_run_<case>.npz.  Every comparison below reads those fixtures and always runs; with a
checkout of the reference present (STABNET_REFERENCE, or a `reference` directory beside the repository) the fixtures are regenerated in a
temporary directory and must come out byte-equal, which is what ties them to the reference's text.  Without a checkout only that part
skips.

  bit for bit (uint32 images), oracle/stabnet_oracle.py against the f32 record:
      get_4_pts, get_black_pos, transformer (output, black, both maps), interpolate, warp_pts (indices and gathered values)
  within a float32 summation bar (tests/_reference_run.py), the oracle's float32 value against the f64 record:
      distortion, consistency, feature, image, id2 losses, every scalar of inference_stable_net's dict, the total under each gate setting
  at 1e-12 relative, oracle/torch_ref.py (`with constants(np.float64)`) against the f64 record, decisions (black, corner indices, warp_pts
  indices) equal outright:
      get_4_pts, transformer, interpolate, the five losses, tower_losses / tower_total
  torch_ref's autograd gradient of the total and of each loss term in the 50 theta components against central differences of the
  reference's f64-mode text; bar per component = 4 |FD(h) - FD(h / 4)| + 1e-9 max |gradient|, both from the reference's run alone.

The one stand-in op taken on trust is tf.matrix_inverse (tests/tf_eager_standin.py): in f32 mode it IS the oracle's inv8_partial_piv_lu.

MEASURED (-s prints every figure):
  bit-for-bit comparisons: 0 differing words in every case, the ragged 45x77 and the 2x3-grid one included.
  oracle f32 vs reference f64, |diff| / bar: distortion 9.4e-10 / 4.5e-7, consistency 6.7e-8 / 2.5e-5, id2 (theta_loss) 2.7e-12 / 1.4e-9,
  feature 1.3e-7 / 5.1e-6, image 3.3e-6 / 1.2e-3, black position 0 / 0, regulariser 2.0e-10 / 2.3e-9, total 3.3e-6 / 1.2e-3.
  torch_ref vs reference f64, fraction of 1e-12 * max(|value|, 1): points and mesh losses 0, maps <= 0.39, output <= 0.72,
  interpolate <= 0.11, the tower's scalars <= 0.01.
  gradient, worst |autograd - FD(h)| / bar: 0.71 (image loss 2.0e-9 of a bar 2.8e-9 at max |grad| 2.8); h = 1e-5, three components took h / 2.
"""
import os
import sys

import numpy as np
import pytest
import torch

import _reference_run as RF
from oracle import run_reference as RR
from oracle import stabnet_oracle as O
from oracle import torch_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP = [c for c, d in RR.CASES.items() if d["kind"] == "warp"]
INTERP = [c for c, d in RR.CASES.items() if d["kind"] == "interp"]
REL = 1e-12


def _reference_dir():
    for d in (os.environ.get("STABNET_REFERENCE"), os.path.join(os.path.dirname(ROOT), "reference"), "/root/reference"):
        if d and os.path.isfile(os.path.join(d, "spatial_transformer3.py")) and os.path.isfile(os.path.join(d, "s_net_bundle_nobm.py")):
            return d
    return None


@pytest.fixture(scope="module")
def regenerated(tmp_path_factory):
    ref = _reference_dir()
    if ref is None:
        pytest.skip("no checkout of the reference (set STABNET_REFERENCE): the fixtures cannot be regenerated from its text")
    out = str(tmp_path_factory.mktemp("reference_run"))
    before = set(sys.modules)
    RR.run(ref, out)
    assert not {m for m in set(sys.modules) - before if m.split(".")[0] in (
        "tensorflow", "config", "configs", "utils", "resnet", "get_data", "tf_utils", "hyper_parameters", "cv2", "spatial_transformer3",
        "s_net_bundle_nobm", "tf_eager_standin")}, "the reference or the stand-in leaked into the test process"
    return ref, out


def _near(got, want, slack=0.0):
    """max over elements of |got - want| / (REL * max(|want|, 1) + slack)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (REL * np.maximum(np.abs(want), 1.0) + slack))) if want.size else 0.0


# ============================================================================================ the fixtures themselves
@pytest.mark.parametrize("case", list(RR.CASES))
def test_fixture_regenerates_byte_equal_from_the_reference_text(regenerated, case):
    ref, out = regenerated
    new = np.load(os.path.join(out, RR.fixture_name(case)), allow_pickle=False)
    old = RF.load(case)
    assert sorted(new.files) == sorted(old)
    for k in new.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (case, k)
    assert not [f for f in os.listdir(ref) if f.endswith(".npz")] and os.path.getsize(os.path.join(RF.GOLDEN, RR.fixture_name(case))) < 195000


@pytest.mark.parametrize("case", list(RR.CASES))
def test_fixture_holds_arrays_of_the_declared_shapes_and_the_input_conditions(case):
    rec = RF.load(case)
    c = RR.CASES[case]
    N, H, W, C, gh, gw, M = RF.geom(rec)
    assert (N, H, W, C, gh, gw, M) == tuple(c[k] for k in ("N", "H", "W", "C", "gh", "gw", "M"))
    want = RR.make_inputs(case, c["seed"])
    for k, v in want.items():                                        # the inputs are the seeded ones
        assert rec[k].dtype == v.dtype and np.array_equal(rec[k], v), k
    nt = (gh + 1) * (gw + 1) * 2
    if c["kind"] == "warp":
        shapes = {"pts1": (N, gh, gw, 8), "pts2": (N, gh + 1, gw + 1, 2), "black_pos": (N, gh * gw * 8), "out": (N, H, W, C),
                  "x_map": (N, H, W), "y_map": (N, H, W), "warp_val": (N, M, 2), "warp_idx": (N, M), "dist": (), "cons": ()}
        for k, s in shapes.items():
            assert rec[k].shape == s and rec[k].dtype == (np.int32 if k == "warp_idx" else np.float32), k
            two = rec.get(k + "_f64", rec.get(k + "_d"))
            assert two.shape == s and two.dtype in (np.float64, np.int32, np.float32), k
        assert rec["black"].dtype == np.uint8 and rec["black"].shape == (N, H, W) and rec["theta"].shape == (N, nt)
        share = rec["black"].mean()
        lim = np.float32(1.25)
        at = (np.abs(rec["pts2"]) == lim).mean()
        inside = (np.abs(rec["pts2"]) == np.nextafter(lim, np.float32(0))).sum()
        # the pixel coordinate before tf.round, as the reference's float32 text forms it: (v + 1) / 2 * size, clipped
        px = np.clip((rec["pts"][..., 0] + np.float32(1)) / np.float32(2) * np.float32(W), 0, W - 1)
        py = np.clip((rec["pts"][..., 1] + np.float32(1)) / np.float32(2) * np.float32(H), 0, H - 1)
        ties = ((px - np.floor(px) == 0.5).sum(), (py - np.floor(py) == 0.5).sum())
        print("%s: black share %.3f, pts2 at the limit %.3f, one step inside %d, warp_pts ties x %d y %d, z of both signs in a cell %d"
              % (case, share, at, inside, ties[0], ties[1], rec["zsign"][0]))
        assert 0.05 <= share <= 0.6 and at >= 0.05 and inside >= 1 and min(ties) >= 1
        assert (rec["pts"] < -1).any() and (rec["pts"] > 1).any()
        assert np.array_equal(rec["warp_idx"], rec["warp_idx_f64"])
        if c.get("zsign"):
            assert rec["zsign"][0] == 1
    elif c["kind"] == "interp":
        assert rec["out"].shape == (N, H, W, C) and rec["out"].dtype == np.float32 and rec["out_d"].shape == (N, H, W, C)
        assert (np.abs(rec["x"]) > 2.0 ** 31).any() and (rec["x"] == 1).any() and (rec["y"] == -1).any()
    elif c["kind"] == "loss":
        for k in RR.SCALARS:
            assert rec["ret_" + k].shape == (4,) and rec["ret_" + k].dtype == np.float32 and rec["ret_" + k + "_f64"].dtype == np.float64
        assert rec["output"].shape == (N, H, W, 1) and rec["black_pix"].shape == (N, H, W) and rec["stable_warpped"].shape == (N, M, 2)
        kept = (1 - rec["black_pix"].astype(np.int64)).reshape(N, -1).sum(axis=1)
        print("%s: matches per sample %s, kept pixels per sample %s" % (case, rec["mask"].sum(axis=1), kept))
        assert rec["mask"][0].sum() == 0 and rec["mask"][1].sum() == M          # maximum(sum, 1) reached; a full mask
        assert 0 < kept.min() <= 0.02 * H * W                                   # one sample almost fully black
        assert np.array_equal(rec["black_pix"], rec["black_pix_f64"]) and np.array_equal(rec["warp_idx"], rec["warp_idx_f64"])
    else:
        assert rec["fd_h"].shape == (len(RR.GRAD_TERMS), nt) and rec["fd_h4"].shape == rec["fd_h"].shape and rec["h_used"].shape == (nt,)
        assert (rec["h_used"] <= RR.GRAD_H).all() and (rec["h_used"] >= RR.GRAD_H / 2).all()
    assert all(v.dtype != object for v in rec.values())


# ============================================================================================ oracle, bit for bit against the f32 record
@pytest.mark.parametrize("case", WARP)
def test_oracle_points_transformer_and_warp_pts_bit_for_bit(case):
    rec = RF.load(case)
    cfg = RF.ocfg(rec)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    pts1, pts2 = O.get_4_pts(rec["theta"], cfg)
    out, black, img = O.transformer(rec["U"], pts2, cfg)
    val, (xi, yi) = O.warp_pts(rec["pts"], img, cfg)
    got = {"pts1": pts1, "pts2": pts2, "black_pos": O.get_black_pos(pts1, cfg), "out": out, "x_map": img[..., 0], "y_map": img[..., 1],
           "warp_val": val}
    bad = {k: int((RF.bits(v) != RF.bits(rec[k])).sum()) for k, v in got.items()}
    bad["black"] = int((black.astype(np.uint8) != rec["black"]).sum())
    bad["warp_idx"] = int(((xi + yi * W).astype(np.int32) != rec["warp_idx"]).sum())
    print("%s: differing words %s" % (case, bad))
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", INTERP)
def test_oracle_interpolate_bit_for_bit(case):
    rec = RF.load(case)
    got = O.interpolate(rec["im"], rec["x"], rec["y"])
    bad = int((RF.bits(got) != RF.bits(rec["out"])).sum())
    print("%s: %d differing words of %d" % (case, bad, got.size))
    assert bad == 0


# ============================================================================================ oracle reductions against the f64 record
@pytest.mark.parametrize("case", WARP)
def test_oracle_mesh_losses_within_the_summation_bar(case):
    rec = RF.load(case)
    cfg = RF.ocfg(rec)
    for name, fn, arg in (("dist", O.get_distortion_loss, rec["pts1"]), ("cons", O.get_consistency_loss, rec["pts2"])):
        got, want = float(fn(arg, cfg)), float(rec[name + "_f64"])
        bar = RF.mean_bar(rec["red_" + name], want, 1.0 / 8 if name == "dist" else 1.0)
        print("%s %s: oracle %.9g reference f64 %.17g |diff| %.3e bar %.3e (reference f32 %.9g)"
              % (case, name, got, want, abs(got - want), bar, float(rec[name])))
        assert abs(got - want) <= bar
        assert abs(float(rec[name]) - want) <= bar


def _oracle_dict(rec, cfg, gate, monkeypatch):
    """O.inference_stable_net with the backbone cut where the recipe cuts the reference's: get_resnet hands back the supplied theta with the
    oracle's own id2 expression, the regulariser is the supplied value."""
    N, H, W, C, gh, gw, M = RF.geom(rec)
    ub, uto = RR.GATES[gate]
    theta = rec["theta"]

    def get_resnet(x_tensor, p, c, training=False, stats_out=None, taps=None):
        id2 = O.F(np.mean(np.abs(theta), dtype=np.float64)) * O.F(c.id_mul)              # stabnet_oracle.get_resnet's last line
        return theta, id2, id2
    monkeypatch.setattr(O, "get_resnet", get_resnet)
    monkeypatch.setattr(O, "regu_loss", lambda p, c: O.F(RR.REGU))
    xt = np.zeros((N, H, W, cfg.in_ch), np.float32)
    xt[..., 2 * cfg.before_ch] = rec["x_cur"][..., 0]
    return O.inference_stable_net(xt, {}, cfg, y=rec["y"], matches=rec["matches"], mask=rec["mask"], use_black_loss=ub, use_theta_only=uto)


@pytest.mark.parametrize("gate", range(len(RR.GATES)))
def test_oracle_inference_dict_against_the_reference_run(gate, monkeypatch):
    rec = RF.load("loss_45x77")
    cfg = RF.ocfg(rec)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    r = _oracle_dict(rec, cfg, gate, monkeypatch)
    # tensors of the dict: bit for bit against the f32 record
    bad = {"output": int((RF.bits(r["output"]) != RF.bits(rec["output"])).sum()),
           "black_pix": int((r["black_pix"].astype(np.uint8) != rec["black_pix"]).sum()),
           "stable_warpped": int((RF.bits(r["stable_warpped"]) != RF.bits(rec["stable_warpped"])).sum()),
           "black_pos": int((RF.bits(r["black_pos"]) != RF.bits(rec["black_pos"][gate])).sum())}
    assert not any(bad.values()), bad
    bars, want = RF.loss_bars(rec, gate, cfg)
    for k in RR.SCALARS:
        got = float(r[k])
        print("gate %s %-16s oracle %.9g reference f64 %.17g |diff| %.3e bar %.3e" % (RR.GATES[gate], k, got, want[k], abs(got - want[k]), bars[k]))
        assert abs(got - want[k]) <= bars[k], k
        assert abs(float(rec["ret_" + k][gate]) - want[k]) <= bars[k], k                  # the reference's own f32 run sits inside too
    if RR.GATES[gate][1] == 1.0:                                                          # theta only: the gated sum is switched off
        assert want["total_loss"] == want["theta_loss"] + want["grid_theta_loss"]


# ============================================================================================ torch_ref against the f64 record
@pytest.mark.parametrize("case", WARP)
def test_torch_ref_forward_against_the_f64_run(case):
    rec = RF.load(case)
    cfg = RF.ocfg(rec)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    with T.constants(np.float64):
        own = {}
        pts1, pts2 = T.get_4_pts(T.t(rec["theta"]), cfg)
        out, black, maps, _ = T.transformer(T.t(rec["U"]), pts2, cfg, record=own)
        dist, cons = float(T.get_distortion_loss(pts1, cfg)), float(T.get_consistency_loss(pts2, cfg))
        bp = T.get_black_pos(pts1, cfg)
    e = {"pts1": _near(pts1.numpy(), rec["pts1_f64"]), "pts2": _near(pts2.numpy(), rec["pts2_f64"]),
         "black_pos": _near(bp.numpy(), rec["black_pos_f64"]), "dist": _near(dist, rec["dist_f64"]), "cons": _near(cons, rec["cons_f64"])}
    for k, got in (("out", out), ("x_map", maps[..., 0]), ("y_map", maps[..., 1])):
        want, slack = RF.f64(rec, k)
        e[k] = _near(got.numpy(), want, slack)
    print("%s: torch_ref vs reference f64, |diff| / (1e-12 max(|v|, 1)): %s" % (case, {k: "%.3g" % v for k, v in e.items()}))
    # decisions: outright
    assert np.array_equal(black.numpy().astype(np.uint8), rec["black_f64"])
    assert np.array_equal(RR.corner_digest_of(*own["corners"], N, H, W), rec["corner_sha_f64"])
    assert max(e.values()) <= 1.0, e


@pytest.mark.parametrize("case", INTERP)
def test_torch_ref_interpolate_against_the_f64_run(case):
    rec = RF.load(case)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    x, y = T.t(rec["x"]).reshape(N, H, W), T.t(rec["y"]).reshape(N, H, W)
    corners = T._own_corners(x, y, H, W)                               # decided in float64, as the f64 run decides them
    assert np.array_equal(RR.corner_digest_of(*corners, N, H, W), rec["corner_sha_f64"])
    got = T.interpolate(T.t(rec["im"]), x, y, corners).numpy()
    want, slack = RF.f64(rec, "out")
    # outside the frame the clipped corners leave weights of the size of the distance, which cancel: the value is held relative to the sum of
    # the four weights' magnitudes (1 inside the frame), not to itself
    x0, y0, x1, y1 = (c.astype(np.float64) for c in corners)
    xp, yp = (x.numpy() + 1.0) * W / 2.0, (y.numpy() + 1.0) * H / 2.0
    wsum = (np.abs(x1 - xp) + np.abs(xp - x0)) * (np.abs(y1 - yp) + np.abs(yp - y0))
    scale = np.maximum(np.maximum(np.abs(want), 1.0), wsum.reshape(N, H, W, 1))
    err = float(np.max(np.abs(got - want) / (REL * scale + slack)))
    print("%s: torch_ref.interpolate vs reference f64: %.3g of the 1e-12 bar" % (case, err))
    assert err <= 1.0


def _torch_tower(rec, cfg, gate, theta=None):
    ub, uto = RR.GATES[gate]
    th = T.t(rec["theta"]) if theta is None else theta
    L = T.tower_losses(th, T.t(rec["x_cur"]), T.t(rec["y"]), T.t(rec["matches"]), T.t(rec["mask"]), cfg, use_black_loss=ub)
    id2 = th.abs().mean() * cfg.id_mul                                  # torch_ref.get_resnet's id2 line
    regu = T.t(RR.REGU)
    d = {"theta_loss": id2 * cfg.theta_mul, "grid_theta_loss": id2 * cfg.grid_theta_mul, "black_loss": L["black_pos_loss"] * cfg.black_mul,
         "distortion_loss": L["distortion"] * cfg.distortion_mul, "consistency_loss": L["consistency"] * cfg.consistency_mul,
         "feature_loss": L["feature"] * cfg.feature_mul, "img_loss": L["img"] * cfg.img_mul, "regu_loss": regu * cfg.regu_mul,
         "total_loss": T.tower_total(id2, id2, L, regu, cfg, use_theta_only=uto)}
    return d, L


@pytest.mark.parametrize("gate", range(len(RR.GATES)))
def test_torch_ref_tower_against_the_f64_run(gate):
    rec = RF.load("loss_45x77")
    cfg = RF.ocfg(rec)
    with T.constants(np.float64):
        d, L = _torch_tower(rec, cfg, gate)
    assert np.array_equal(L["black_pix"].numpy().astype(np.uint8), rec["black_pix_f64"])
    want, slack = RF.f64(rec, "output")
    e = {"output": _near(L["output"].numpy(), want, slack)}
    for k in RR.SCALARS:
        w = float(rec["ret_" + k + "_f64"][gate])
        e[k] = abs(float(d[k]) - w) / (REL * abs(w)) if w != 0 else (0.0 if float(d[k]) == 0 else np.inf)
    print("gate %s: torch_ref vs reference f64, fraction of the 1e-12 relative bar: %s" % (RR.GATES[gate], {k: "%.3g" % v for k, v in e.items()}))
    assert max(e.values()) <= 1.0, e


def test_torch_ref_gradient_against_central_differences_of_the_reference_text():
    rec = RF.load("grad_32x64")
    cfg = RF.ocfg(rec)
    fd, fd4 = rec["fd_h"], rec["fd_h4"]
    with T.constants(np.float64):
        th = T.t(rec["theta"], requires_grad=True)
        d, _ = _torch_tower(rec, cfg, RR.GATES.index((1.0, 0.0)), th)
        worst = 0.0
        for i, k in enumerate(RR.GRAD_TERMS):
            assert abs(float(d[k].detach()) - rec["value_f64"][i]) <= REL * abs(rec["value_f64"][i])
            g = torch.autograd.grad(d[k], th, retain_graph=True, allow_unused=True)[0]
            g = np.zeros(fd.shape[1]) if g is None else g.numpy().reshape(-1)
            bar = 4 * np.abs(fd[i] - fd4[i]) + 1e-9 * np.abs(fd[i]).max()
            err = np.abs(g - fd[i])
            j = int(np.argmax(err / np.maximum(bar, 1e-300)))
            print("d %-16s / d theta: max |grad| %.3e, worst |autograd - FD| %.3e at component %d (bar %.3e, h %.2e)"
                  % (k, np.abs(fd[i]).max(), err[j], j, bar[j], rec["h_used"][j]))
            if np.abs(fd[i]).max() == 0:
                assert not g.any(), k
                continue
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (k, j, err[j], bar[j])
    print("gradient: worst |autograd - FD(h)| / bar %.3f; components that needed h / 2: %d" % (worst, int((rec["h_used"] != RR.GRAD_H).sum())))
