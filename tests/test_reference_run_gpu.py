"""GPU: the warp and loss kernels against what the reference's OWN text computed (tests/golden/reference_run_<case>.npz, recorded by
oracle/run_reference.py; tests/test_reference_run_cpu.py ties those files to the reference's text).  Reads the fixtures only.

Through the C ABI, every output in a NaN-filled buffer of the test's own:
  bit for bit against the f32 record (uint32 words):
      stabnet_get_4_pts (pts1, pts2); stabnet_transformer_fwd (x map, y map, black, output); stabnet_interp_fwd; the warp_pts gather inside
      stabnet_feature_loss (want_warped)
  within a bar against the f64 record:
      stabnet_mesh_losses (id2, black-position, distortion, consistency), stabnet_feature_loss, the masked-MSE image loss, and the total as
      Trainer.losses composes it (float64 on the host from the kernels' float32 parts), under each gate setting.
      bar = the float32 summation bound of tests/_reference_run.py for the KERNEL's term count (the distortion kernel adds 16 squares per
      cell where the reference reduces sums of eight), and never looser than the relative bar of the older oracle comparison of the same
      quantity (tests/test_warp_bwd_gpu.py: id2 1e-5, distortion and consistency 1e-4, feature and image 1e-5; black position: exactly 0).

MEASURED on an MI355X (N = 3 at 45x77, 40 matches; the same under all four gate settings):
  bit-for-bit comparisons: 0 differing words in every case (32x64, the ragged 45x77, the 2x3 grid with 3 channels).
  |kernels - reference f64| and its bar:  id2 (as theta_loss) 1.1e-11 / 1.4e-9;  black position 0 / 0;  distortion 9.4e-10 / 3.5e-6;
  consistency 2.2e-8 / 2.5e-5;  feature 1.7e-7 / 5.1e-6;  image 3.3e-6 / 5.4e-5 (the older 1e-5 relative bar binds; the summation bound is
  1.2e-3, 3 464 additions of squares);  regulariser 0;  total 3.5e-6 / 9.1e-5.
"""
import numpy as np
import pytest
import torch

import _reference_run as RF
from oracle import run_reference as RR

pytestmark = pytest.mark.gpu

WARP = [c for c, d in RR.CASES.items() if d["kind"] == "warp"]
INTERP = [c for c, d in RR.CASES.items() if d["kind"] == "interp"]
OLDER_REL = {"theta_loss": 1e-5, "grid_theta_loss": 1e-5, "distortion_loss": 1e-4, "consistency_loss": 1e-4, "feature_loss": 1e-5,
             "img_loss": 1e-5}


class Outputs:
    """NaN-filled device buffers for one call; result() hands them back on the host and refuses an element that was never written."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def new(self, name, shape):
        self.bufs[name] = torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=self.dev)
        return self.bufs[name].data_ptr()

    def result(self):
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.bufs.items()}
        for k, v in out.items():
            assert not np.isnan(v).any(), "%s: %d elements never written" % (k, int(np.isnan(v).sum()))
        return out


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _cfg(rec):
    from stabnet_amd.config import Config
    N, H, W, C, gh, gw, M = RF.geom(rec)
    return Config(height=H, width=W, batch_size=N, grid_h=gh, grid_w=gw, max_matches=M)


def _words(got, want):
    return int((RF.bits(got).reshape(-1) != RF.bits(want).reshape(-1)).sum())


def _get_4_pts(theta, cfg, dev):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    N, gh, gw = theta.shape[0], cfg.grid_h, cfg.grid_w
    o = Outputs(dev)
    th = _dev(theta, dev)
    _lib.call("stabnet_get_4_pts", th.data_ptr(), N, gh, gw, cfg.do_crop_rate, o.new("pts1", (N, gh, gw, 8)), o.new("pts2", (N, gh + 1, gw + 1, 2)),
              o.new("Hs", (N, gh, gw, 9)), stream_ptr(dev), device=dev)
    return o.result()


def _transformer(U, pts2, cfg, dev):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    N, H, W, C = U.shape
    o = Outputs(dev)
    u, p = _dev(U, dev), _dev(pts2, dev)
    _lib.call("stabnet_transformer_fwd", p.data_ptr(), u.data_ptr(), N, H, W, C, cfg.grid_h, cfg.grid_w, o.new("out", (N, H, W, C)),
              o.new("black", (N, H, W)), o.new("x_map", (N, H, W)), o.new("y_map", (N, H, W)), o.new("Hs", (N, cfg.grid_h, cfg.grid_w, 9)),
              stream_ptr(dev), device=dev)
    return o.result()


def _feature_loss(matches, mask, x_map, y_map, dev):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    N, M, _ = matches.shape
    H, W = x_map.shape[1], x_map.shape[2]
    o = Outputs(dev)
    m, k, xm, ym = _dev(matches, dev), _dev(mask, dev), _dev(x_map, dev), _dev(y_map, dev)
    _lib.call("stabnet_feature_loss", m.data_ptr(), k.data_ptr(), xm.data_ptr(), ym.data_ptr(), N, H, W, M, 0.0, o.new("value", (N,)), 0, 0, 0,
              o.new("warped", (N, M, 2)), stream_ptr(dev), device=dev)
    return o.result()


@pytest.mark.parametrize("case", WARP)
def test_get_4_pts_bit_for_bit(cuda, case):
    rec = RF.load(case)
    got = _get_4_pts(rec["theta"], _cfg(rec), cuda)
    bad = {k: _words(got[k], rec[k]) for k in ("pts1", "pts2")}
    print("%s: differing words %s" % (case, bad))
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", WARP)
def test_transformer_forward_bit_for_bit(cuda, case):
    rec = RF.load(case)
    got = _transformer(rec["U"], rec["pts2"], _cfg(rec), cuda)
    bad = {k: _words(got[k], rec[k]) for k in ("x_map", "y_map", "out")}
    bad["black"] = int((got["black"] != rec["black"].astype(np.float32)).sum())
    print("%s: differing words %s of %d per image" % (case, bad, rec["x_map"].size))
    assert not any(bad.values()), bad


@pytest.mark.parametrize("case", INTERP)
def test_interpolate_bit_for_bit(cuda, case):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    rec = RF.load(case)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    o = Outputs(cuda)
    im, x, y = _dev(rec["im"], cuda), _dev(rec["x"], cuda), _dev(rec["y"], cuda)
    _lib.call("stabnet_interp_fwd", im.data_ptr(), x.data_ptr(), y.data_ptr(), N, H, W, C, o.new("out", (N, H, W, C)), stream_ptr(cuda), device=cuda)
    bad = _words(o.result()["out"], rec["out"])
    print("%s: %d differing words of %d" % (case, bad, rec["out"].size))
    assert bad == 0


@pytest.mark.parametrize("case", WARP)
def test_warp_pts_gather_bit_for_bit(cuda, case):
    rec = RF.load(case)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    matches = np.concatenate([rec["pts"], np.zeros_like(rec["pts"])], axis=2)
    got = _feature_loss(matches, np.ones((N, M), np.float32), rec["x_map"], rec["y_map"], cuda)
    bad = _words(got["warped"], rec["warp_val"])
    # the gathered values name the pixel: the record's index picks the same values out of the maps
    flat = np.stack([rec["x_map"].reshape(N, -1), rec["y_map"].reshape(N, -1)], axis=2)
    assert np.array_equal(np.take_along_axis(flat, rec["warp_idx"][:, :, None].astype(np.int64), axis=1), rec["warp_val"])
    print("%s: %d differing words of %d" % (case, bad, rec["warp_val"].size))
    assert bad == 0


def test_losses_and_composed_total_within_bars(cuda):
    from stabnet_amd import _lib
    from stabnet_amd._tensor import stream_ptr
    rec = RF.load("loss_45x77")
    cfg = _cfg(rec)
    N, H, W, C, gh, gw, M = RF.geom(rec)
    nt = (gh + 1) * (gw + 1) * 2
    pts = _get_4_pts(rec["theta"], cfg, cuda)
    warp = _transformer(rec["x_cur"], pts["pts2"], cfg, cuda)
    assert _words(warp["out"], rec["output"]) == 0 and np.array_equal(warp["black"], rec["black_pix"].astype(np.float32))
    feat = _feature_loss(rec["matches"], rec["mask"], warp["x_map"], warp["y_map"], cuda)
    assert _words(feat["warped"], rec["stable_warpped"]) == 0
    o = Outputs(cuda)
    a, b, bl = _dev(warp["out"], cuda), _dev(rec["y"], cuda), _dev(warp["black"], cuda)
    ws = torch.empty(_lib.lib().stabnet_masked_mse_workspace_bytes(N), dtype=torch.uint8, device=cuda)
    _lib.call("stabnet_masked_mse_sums", a.data_ptr(), b.data_ptr(), bl.data_ptr(), 0, N, H * W, o.new("sums", (N, 2)), ws.data_ptr(),
              stream_ptr(cuda), device=cuda)
    s = o.result()["sums"].astype(np.float64)
    assert np.array_equal(s[:, 1], (1 - rec["black_pix"].reshape(N, -1).astype(np.float64)).sum(axis=1))       # the kept-pixel counts are exact
    img = float((s[:, 0] / (s[:, 1] + 1e-8)).sum() / cfg.batch_size)                                            # as Trainer.losses forms it
    fl = float(feat["value"].astype(np.float64).mean())
    n_ref = rec["red_dist"][0]
    worst = {}
    for gate, (ub, uto) in enumerate(RR.GATES):
        live = 1.0 - uto
        o = Outputs(cuda)
        th = _dev(rec["theta"], cuda)
        _lib.call("stabnet_mesh_losses", th.data_ptr(), 0, N, gh, gw, cfg.do_crop_rate, cfg.id_mul, cfg.theta_mul + cfg.grid_theta_mul,
                  live * cfg.distortion_mul, live * cfg.consistency_mul, float(ub), live * cfg.black_mul, o.new("losses", (4,)),
                  o.new("d_theta", (N, nt)), stream_ptr(cuda), device=cuda)
        m = o.result()["losses"].astype(np.float64)
        t = {"theta_loss": m[0] * cfg.theta_mul, "grid_theta_loss": m[0] * cfg.grid_theta_mul, "black_loss": m[1] * cfg.black_mul,
             "distortion_loss": m[2] * cfg.distortion_mul, "consistency_loss": m[3] * cfg.consistency_mul, "feature_loss": fl * cfg.feature_mul,
             "img_loss": img * cfg.img_mul, "regu_loss": RR.REGU * cfg.regu_mul}
        t["total_loss"] = t["theta_loss"] + t["grid_theta_loss"] + live * (t["img_loss"] + t["regu_loss"] + t["black_loss"]
                                                                             + t["distortion_loss"] + t["consistency_loss"] + t["feature_loss"])
        bars, want = RF.loss_bars(rec, gate, cfg, terms={"dist": 8 * n_ref}, cap=OLDER_REL)
        for k in RR.SCALARS:
            bar = bars[k]
            err = abs(t[k] - want[k])
            print("gate %s %-16s kernels %.9g reference f64 %.17g |diff| %.3e bar %.3e" % ((ub, uto), k, t[k], want[k], err, bar))
            if bar > 0:
                worst[k] = max(worst.get(k, 0.0), err / bar)
            assert err <= bar, (k, gate, err, bar)
    print("worst |diff| / bar over the gate settings: %s" % {k: "%.3g" % v for k, v in worst.items()})
