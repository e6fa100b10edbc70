"""GPU: the path a user walks -- train, save, resume, deploy -- with the state handed over through FILES.

A Trainer runs three steps (its own schedule, one batch per step), train_bundle_nobm.save_checkpoint writes the file the driver
writes, and that file is what everything below reads: deploy_bundle.load_weights, a Regressor at the training size and at another
one, a deploy stream, Regressor.load_params + refold(), the TensorFlow bundle route, and restore_checkpoint into a trainer that
was built from OTHER parameters.  References: float64 inference of oracle/torch_ref.py and the oracle's deploy loop, both on the
float32 parameters the file holds.

So that a test can tell WHICH parameter set was deployed, the training config uses bn_decay 0.5 and the smallest learning rate of
{2e-5, 2e-4, 1e-3} at which three float64 oracle steps (autograd + AdamTF + the moving-average recurrence, no GPU value involved)
move the inference theta by >= 100 x the theta bar on each test input: 2e-5, the reference's own rate, is enough (theta moves by
4.6e-1 / 4.4e-1 at 64 x 96 / 96 x 160, by 7.6e-2 / 7.7e-2 through the weights alone: the moving statistics travel most of the way
to the batch statistics).  test_trained_model_is_distinguishable asserts that distance."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import stabnet_oracle as O
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, H, W = 2, 64, 96
SEEDS = (5, 6, 7)
LEARNING_RATE = 2e-5
DEPLOY_SIZES = [(64, 96), (96, 160)]            # the training size, and another one with ragged conv tiles
# theta of a Regressor against float64 inference: the f32 bar of test_operand_routes_gpu.py (measured there 1.1e-7 at 96 x 160)
F32_BAR = 2e-6


def _cfg():
    from stabnet_amd.config import Config
    return Config(height=H, width=W, batch_size=N, max_matches=48, initial_learning_rate=LEARNING_RATE, bn_decay=0.5)


def _batches(cfg):
    from stabnet_amd import synthetic
    out = []
    for seed in SEEDS:
        b = synthetic.make_train_batch(cfg, N, H, W, seed)
        b["flow"] = (b["flow"] + np.random.default_rng(1).normal(0, 0.02, b["flow"].shape)).astype(np.float32)
        out.append(b)
    return out


def _input(h, w, cfg):
    return np.random.default_rng(11).uniform(-0.5, 0.5, (1, h, w, cfg.in_ch)).astype(np.float32)


def _theta64(P, x, h, w):
    with torch.no_grad():
        theta, _, _ = T.get_resnet(T.t(x), {k: T.t(v) for k, v in P.items()}, O.Config(height=h, width=w), False)
    return theta.numpy()


def _oracle_trained(P0, batches, cfg):
    """Three training steps WITHOUT the GPU: float64 autograd at the float32 parameters, AdamTF, slim's moving averages."""
    from stabnet_amd.train import loss_gates
    ocfg = O.Config(height=H, width=W, batch_size=N, max_matches=48)
    P = {k: np.asarray(v, np.float32) for k, v in P0.items()}
    names = [k for k in P if "/moving_" not in k]
    sizes = [P[k].size for k in names]
    adam = O.AdamTF(sum(sizes))
    for k, b in enumerate(batches):
        g = loss_gates(k, cfg)
        pt = {n: T.t(v, requires_grad=True) for n, v in P.items()}
        stats = {}
        total, _ = T.train_objective(pt, b, ocfg, float(g["use_temp_loss"]), float(g["use_black_loss"]), float(g["use_theta_only"]),
                                     training=True, batch_stats=stats)
        total.backward()
        grad = np.concatenate([(pt[n].grad.numpy() if pt[n].grad is not None else np.zeros(P[n].shape)).reshape(-1) for n in names])
        lr = float(O.exponential_decay_staircase(cfg.initial_learning_rate, k, cfg.step_size, 0.1))
        new = adam.step(np.concatenate([P[n].reshape(-1) for n in names]), grad, lr)
        for n, chunk in zip(names, np.split(new, np.cumsum(sizes)[:-1])):
            P[n] = chunk.reshape(P[n].shape)
        for n in list(P):
            if "/moving_" in n:
                prefix, which = n.rsplit("/", 1)
                m = P[n].astype(np.float64)
                for key in ("1", "2"):
                    m = m - (m - stats[key][prefix][0 if which == "moving_mean" else 1]) * (1 - cfg.bn_decay)
                P[n] = m.astype(np.float32)
    return P


@pytest.fixture(scope="module")
def run(cuda, tmp_path_factory):
    """Trainer A: steps 0, 1, 2; trainer B: steps 0, 1, then save_checkpoint (the resume tests); A's checkpoint after step 2 is the
    trained model of the deploy tests.  Shared, never modified."""
    import train_bundle_nobm as drv
    from stabnet_amd import synthetic
    from stabnet_amd.train import Trainer
    cfg = _cfg()
    P0 = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    batches = _batches(cfg)
    dev = [{k: torch.from_numpy(v).to(cuda) for k, v in b.items()} for b in batches]
    d = tmp_path_factory.mktemp("handoff")
    a = Trainer(P0, N, H, W, cfg, device=cuda)
    b = Trainer(P0, N, H, W, cfg, device=cuda)
    for k in (0, 1):
        a.forward_backward(dev[k])
        b.forward_backward(dev[k])
    drv.save_checkpoint(b, str(d / "model-2.npz"))
    a.forward_backward(dev[2])
    torch.cuda.synchronize()
    drv.save_checkpoint(a, str(d / "model-3.npz"))
    trained = a.plan.unpack(a.params.cpu().numpy())
    return {"cfg": cfg, "P0": P0, "batches": batches, "dev": dev, "dir": d, "a": a, "b": b, "trained": trained,
            "losses_a": a.losses(), "names": [row[0] for row in a.plan.table]}


def _load(run, model_name):
    import deploy_bundle
    return deploy_bundle.load_weights(argparse.Namespace(model_dir=str(run["dir"]), model_name=model_name), run["cfg"])


def test_trained_model_is_distinguishable(run):
    """Input condition (oracle values only): three float64 steps move the inference theta by >= 100 x the theta bar on both
    inputs, so `within the bar of the trained model` excludes the initial one."""
    P3 = _oracle_trained(run["P0"], run["batches"], run["cfg"])
    for h, w in DEPLOY_SIZES:
        x = _input(h, w, run["cfg"])
        d = float(np.abs(_theta64(P3, x, h, w) - _theta64(run["P0"], x, h, w)).max())
        print("%d x %d: float64 inference theta moves by %.3e in three oracle steps (bar %g)" % (h, w, d, F32_BAR))
        assert d >= 100 * F32_BAR, (h, w, d)
    # ... and the GPU's three steps did train: the file does not hold the initial parameters
    assert any(not np.array_equal(run["trained"][n], run["P0"][n]) for n in run["names"] if "/moving_" not in n)
    assert all(not np.array_equal(run["trained"][n], run["P0"][n]) for n in run["names"] if "/moving_" in n)


@pytest.mark.parametrize("model_name", ["model-3.npz", "model-3"])
def test_file_round_trip(run, model_name):
    """save_checkpoint -> deploy_bundle.load_weights: exactly the plan's variables, none of the `__` keys, every array bit for bit."""
    loaded = _load(run, model_name)
    assert set(loaded) == set(run["names"]) and len(run["names"]) == len(set(run["names"]))
    assert not any(k.startswith("__") for k in loaded)
    for n in run["names"]:
        want = run["trained"][n]
        assert loaded[n].dtype == np.float32 and loaded[n].shape == want.shape, n
        assert np.array_equal(loaded[n].view(np.uint32), want.view(np.uint32)), n
    z = np.load(str(run["dir"] / "model-3.npz"))
    assert sorted(k for k in z.files if k.startswith("__")) == ["__adam_m", "__adam_v", "__global_step"]
    assert z["__global_step"].dtype == np.int64 and z["__global_step"].shape == () and int(z["__global_step"]) == 3


@pytest.mark.parametrize("h,w", DEPLOY_SIZES)
@pytest.mark.parametrize("mode", [0, 4])
def test_deploy_of_the_trained_model(cuda, run, h, w, mode):
    """A Regressor built from the loaded file against float64 inference on the same float32 parameters, F32_BAR (2e-6: the wider
    2e-5 of test_baseline_sizes_gpu.py is not needed.  MEASURED 7.5e-7 / 5.2e-7 in mode 0 and 6.9e-7 / 9.9e-7 in mode 4 at
    64 x 96 / 96 x 160, against 1.1e-7 at the synthetic parameters)."""
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import Regressor
    loaded = _load(run, "model-3")
    x = _input(h, w, run["cfg"])
    want = _theta64(loaded, x, h, w)
    reg = Regressor(loaded, 1, h, w, Config(height=h, width=w), device=cuda, operand_mode=mode)
    got = reg(torch.from_numpy(x).to(cuda)).cpu().numpy()
    err = float(np.abs(got - want).max())
    print("%d x %d mode %d: theta of the trained model vs float64 %.3e (bar %g)" % (h, w, mode, err, F32_BAR))
    assert err < F32_BAR


@pytest.mark.parametrize("mode", [0, 4])
def test_deploy_stream_of_the_trained_model(cuda, run, mode):
    """Three frames of the online loop on the trained parameters against the oracle's loop (bars of test_deploy_gpu.py)."""
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    loaded = _load(run, "model-3")
    cfg, ocfg = Config(height=H, width=W), O.Config(height=H, width=W)
    clip = synthetic.make_clip(H, W, 3, seed=3, margin=32)
    s = StabNetStream(loaded, H, W, cfg, streams=1, device=cuda, operand_mode=mode)
    s.start(torch.from_numpy(clip[0:1]).to(cuda))
    ring = O.DeployRing(clip[0], ocfg)
    for t in (1, 2):
        got = s.step(torch.from_numpy(clip[t:t + 1]).to(cuda))
        ref, frame = O.deploy_step(ring, clip[t], loaded, ocfg)
        assert np.abs(got["theta"].cpu().numpy() - ref["theta"]).max() < 5e-5, t
        assert np.abs(got["x_map"].cpu().numpy() - ref["x_map"]).max() < 3e-4, t
        d = np.abs(got["frame"].cpu().numpy()[0] - frame)
        assert np.quantile(d, 0.999) < 5e-3, (t, float(d.max()))


@pytest.mark.parametrize("mode", [0, 4])
def test_load_params_and_refold(cuda, run, mode):
    """Following a training run: a Regressor built from the INITIAL parameters, load_params(trained) + refold(), equals a Regressor
    built from the trained parameters bit for bit -- from a dict and from the flat buffer."""
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import Regressor
    cfg = Config(height=H, width=W)
    x = torch.from_numpy(_input(H, W, run["cfg"])).to(cuda)
    fresh = Regressor(run["trained"], 1, H, W, cfg, device=cuda, operand_mode=mode)
    want = fresh(x).clone()
    reg = Regressor(run["P0"], 1, H, W, cfg, device=cuda, operand_mode=mode)
    before = reg(x).clone()
    assert not torch.equal(before, want)
    reg.load_params(run["trained"])
    reg.refold()
    assert torch.equal(reg(x), want)
    reg.load_params(run["P0"])
    reg.refold()
    assert torch.equal(reg(x), before)
    reg.load_params(fresh.plan.pack(run["trained"]))
    reg.refold()
    assert torch.equal(reg(x), want) and torch.equal(reg.params, fresh.params) and torch.equal(reg.fold, fresh.fold)
    from stabnet_amd import _lib
    with pytest.raises(_lib.StabnetError):
        reg.load_params(np.zeros(3, np.float32))


def test_tf_bundle_route(run, tmp_path):
    """The same variables written as a TensorFlow V2 bundle under the reference's scope and read through load_weights' `.index`
    branch: the arrays of the npz route, bit for bit."""
    import deploy_bundle
    from stabnet_amd import tf_checkpoint
    loaded = _load(run, "model-3")
    tf_checkpoint.write_bundle(str(tmp_path / "model-80000"), {tf_checkpoint.STABNET_SCOPE + k: v for k, v in loaded.items()})
    assert os.path.exists(tmp_path / "model-80000.index") and not os.path.exists(tmp_path / "model-80000.npz")
    via_tf = deploy_bundle.load_weights(argparse.Namespace(model_dir=str(tmp_path), model_name="model-80000"), run["cfg"])
    assert set(via_tf) == set(loaded)
    for n, v in loaded.items():
        assert via_tf[n].dtype == np.float32 and via_tf[n].shape == v.shape, n
        assert np.array_equal(via_tf[n].view(np.uint32), v.view(np.uint32)), n


def test_resume_through_a_file_is_bit_exact(cuda, run):
    """A: steps 0, 1, 2 straight.  B: steps 0, 1, save_checkpoint.  C: built from DIFFERENT initial parameters, restore_checkpoint,
    step 2.  C equals A bit for bit: parameters with the moving-statistics tail, Adam moments, step count, the losses of step 2."""
    import train_bundle_nobm as drv
    from stabnet_amd import synthetic
    from stabnet_amd.train import Trainer
    a, cfg = run["a"], run["cfg"]
    other = synthetic.make_params(cfg, seed=1, theta_scale=0.3)
    c = Trainer(other, N, H, W, cfg, device=cuda)
    assert not torch.equal(c.params, run["b"].params)
    drv.restore_checkpoint(c, str(run["dir"] / "model-2.npz"))
    assert c.global_step == 2 and torch.equal(c.params, run["b"].params)
    c.forward_backward(run["dev"][2])
    torch.cuda.synchronize()
    assert c.global_step == a.global_step == 3
    assert torch.equal(c.params, a.params) and torch.equal(c.params[c.nt:], a.params[a.nt:])
    assert torch.equal(c.adam_m, a.adam_m) and torch.equal(c.adam_v, a.adam_v)
    assert c.losses() == run["losses_a"]


def test_driver_resume_is_bit_exact(cuda, tmp_path):
    """train_bundle_nobm.py --iters 4 against --iters 2 followed by --restore --iters 4: every array of the two model-3.npz files
    is the same, `__adam_*` and `__global_step` included.  (The synthetic batches are keyed by the step index.)

    The driver's held-out evaluations run the training forward, so they MOVE the moving statistics -- by design: the reference's
    update ops are a control dependency of total_loss (s_net_bundle_nobm.py:355-357).  Both runs still see the same evaluations
    before model-3.npz is written, namely none: an iteration writes its checkpoint BEFORE its evaluations; the straight run
    evaluates only in iteration 3 (the last one; iteration 0 is excluded, test_freq is 500), after model-3.npz; the short run
    evaluates in its last iteration 1, after model-1.npz, which is the file the resumed run starts from; and the resumed run
    (start step 1) skips save and evaluation in iteration 1 (`i > st_step`) and then behaves as the straight run."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "train_bundle_nobm.py"), "--no-imagenet-init", "--batch-size", "2", "--height", "64",
            "--width", "96"]

    def drive(extra, model_dir):
        out = subprocess.run(base + extra + ["--model-dir", str(model_dir)], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout

    drive(["--iters", "4"], tmp_path / "straight")
    drive(["--iters", "2"], tmp_path / "resumed")
    assert sorted(os.listdir(tmp_path / "resumed")) == ["model-1.npz"]
    assert "restoring" in drive(["--restore", "--iters", "4"], tmp_path / "resumed")
    za, zb = np.load(tmp_path / "straight" / "model-3.npz"), np.load(tmp_path / "resumed" / "model-3.npz")
    assert sorted(za.files) == sorted(zb.files) and {"__adam_m", "__adam_v", "__global_step"} <= set(za.files)
    assert int(za["__global_step"]) == 3
    for k in za.files:
        assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), k
