"""GPU: the online loop with S > 1 streams, every stream held to the oracle on its own.

stabnet_deploy_frame reads the ring [S][32][H*W], runs the regressor at batch S, warps and pushes; every stream offset on the way is a
hand-written s * depth * hw product (csrc/ring.hip, warp_sample_kernel<1>, stabnet_black_accumulate, the fused head).  bench.py
--streams feeds the SAME frame to every stream, so it cannot show a cross-stream error; these tests give every stream its own content.

  1. test_step_from_random_state: rings that differ in every (stream, slot, pixel), a random head (0, 1, depth-1: the wrap), a
     different current frame per stream, all_black preset to random counts.  After one step, per stream against
     O.deploy_step(DeployRing of that stream): theta <= 2e-5, maps < 1e-4, black flips only where the map is within 1e-4 of +-1 (the
     bars of test_baseline_sizes_gpu.py); for refine == 1 Hs / maps / black / output equal O.get_4_pts + O.transformer at the GPU's own
     theta bit for bit; the feedback bit for bit (frame_fb = output - black in slot head0 of the stream's own planes, every other slot
     of every stream untouched, head + 1 mod depth); all_black grew by the stream's own masks.  With use_graph the first step is the
     eager one that is captured, the second -- from another random state -- a replay; both are checked.
     refine == 2: the first pass is a refine=1 stream stepped from the identical state (held to the oracle's single pass and to the
     exact warp like any other); its mask is the first half of all_black, and its DECISIONS are forced onto the oracle's second pass
     (as tests/_decisions.py does for the training step): at the pixels where the oracle's own first-pass map sits within the map bar
     of a discontinuity of the warp -- the black test at +-1, the clipped-corner sampler at the frame's first / last row and column --
     the second pass reads the GPU's first-pass pixel, everywhere else the oracle's own.  Unforced, two float32 evaluations whose maps
     differ by 1e-6 can land on different sides: in case S3-64x96-mode0-refine2-head1, pixel (63, 89) of stream 1 samples column
     95 -+ 3e-5 (x_map 0.9791660 / 0.9791671), the oracle's pixel is 0.428, the GPU's -- bit-exact at its own theta -- 0.0, and theta
     of the unforced second pass is 5.4e-5 off (forced: 7.2e-7; from the GPU's whole first-pass frame: 1.8e-7).
  2. test_lock_step_across_the_wrap: S = 3, three clips, 40 frames (the 32-deep ring wraps), operand mode 4, graph replay, against three
     single-stream objects that are handed the S-stream object's ring planes before every step (bench.py's f32 leg does the same): no
     trajectory divergence, so theta <= 2e-6 and output <= 1e-4 (the lock-step bars of test_deploy_gpu.py) hold on all 39 steps; the
     ring between two steps is exactly what the steps before pushed; at steps 1, 17, 33, 39 the oracle comparison of (1) from that
     state, where lags 8, 16, 32 hold real, distinct frames on both sides of the wrap.  S = 4 on one clip (bench.py's feed): the four
     streams agree.  test_planted_copy_is_noticed: stream 0's pushed frame copied over stream 1's by hand fails the run.
  3. test_batched_regressor_mode4: N in {3, 4, 5, 8, 9} at 64x96 and N = 3 at 72x136 (the conv plan -- tiles, split-K, B2B -- depends
     on N), operand modes 4 and 0 against the float64 evaluation (oracle/torch_ref.py) at test_operand_routes_gpu.py's F32_BAR;
     err(mode 4) <= 2 err(mode 0) + 1e-7 (test_conv_packed_gpu.py's relation); row i within 2e-6 of the single-sample forward.
  4. test_padded_stack_assembly: stack_assemble_kernel (16-channel pixels) only runs with STABNET_STEM_ROWRUN=0, read once per
     process: case S = 2, 45x77, mode 0 of (1) in a fresh child (tests/multistream_child.py); the parent makes the comparisons.

MEASURED (MI355X; the module takes 12 s):
  1. theta against the oracle per case (graph cases: captured step, replayed step; refine 2: forced / unforced second pass)
       S1 64x96 mode0 refine1 head0 eager  1.40e-07          S5 45x77 mode0 refine1 head31 graph 1.45e-07 1.94e-07
       S2 45x77 mode0 refine1 head1 eager  1.94e-07          S2 45x77 mode4 refine2 head31 eager 5.59e-07 / 5.59e-07
       S2 64x96 mode4 refine1 head31 graph 2.85e-07 2.01e-07 S3 64x96 mode4 refine2 head0 graph  4.47e-07 / 4.47e-07, 4.25e-07 / 4.32e-07
       S3 45x77 mode4 refine1 head31 eager 1.71e-07          S5 45x77 mode4 refine2 head1 eager  7.86e-07 / 7.86e-07
       S3 64x96 mode0 refine2 head1 eager  7.15e-07 / 5.39e-05 (above)   S1 45x77 mode4 refine1 head1 graph  1.56e-07 1.42e-07
       S5 64x96 mode4 refine1 head0 graph  1.71e-07 1.86e-07 S2 64x96 mode0 refine2 head31 graph 5.81e-07 / 5.81e-07, 5.40e-07 / 5.40e-07
     the warp at the GPU's own theta (fused head and mesh kernel alike), the feedback and all_black: exact in every case
  2. S = 3 over the wrap: all 39 steps BIT-IDENTICAL to the three single streams (theta, output, ring planes); theta against the oracle at
     steps 1 / 17 / 33 / 39: 9.7e-08 / 1.4e-07 / 1.3e-07 / 1.1e-07.  S = 4 on one clip: the four streams bit-identical on all 39 steps
  3. theta against float64, mode 4 / mode 0: N = 3, 4, 5 at 64x96 1.253e-07 / 9.779e-08; N = 8, 9 1.404e-07 / 1.248e-07; N = 3 at 72x136
     9.458e-08 / 8.716e-08
  4. STABNET_STEM_ROWRUN=0, S2 45x77 mode0 head1: theta against the oracle 1.97e-07
Each test was seen to fail once against a library with one in-bounds mistake: stream 0's planes for every stream in
stack_assemble_bordered_kernel (1, 2), lags 1 and 2 swapped in stack_assemble_kernel (4), the push into slot head instead of head - 1 in
warp_sample_kernel<1> (1, 2, 4), all_black without its n * hw term (1, 2, 4), sample 0's activations for every sample in the GAP (3).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _multistream as M
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32_BAR = 2e-6                        # tests/test_operand_routes_gpu.py
LOCK_THETA, LOCK_OUT = 2e-6, 1e-4     # tests/test_deploy_gpu.py::test_two_streams_equal_two_single_streams
DEPTH = 32


@functools.lru_cache(maxsize=None)
def _setup(H, W):
    return M.make_params(H, W)


# S, H, W, operand_mode, refine, head0, use_graph: every S, both sizes, both modes, both refines, all three heads, graph on and off
STEP_CASES = [
    (1, 64, 96, 0, 1, 0, False),
    (2, 45, 77, 0, 1, 1, False),              # (the case test_padded_stack_assembly repeats with the other stack assembly)
    (2, 64, 96, 4, 1, DEPTH - 1, True),
    (3, 45, 77, 4, 1, DEPTH - 1, False),
    (3, 64, 96, 0, 2, 1, False),
    (5, 64, 96, 4, 1, 0, True),
    (5, 45, 77, 0, 1, DEPTH - 1, True),
    (2, 45, 77, 4, 2, DEPTH - 1, False),
    (3, 64, 96, 4, 2, 0, True),
    (5, 45, 77, 4, 2, 1, False),
    (1, 45, 77, 4, 1, 1, True),
    (2, 64, 96, 0, 2, DEPTH - 1, True),
]


def _case_seed(S, H, W, mode, refine, head0, rep=0):
    return [S, H, W, mode, refine, head0, rep]


@pytest.mark.parametrize("S,H,W,mode,refine,head0,use_graph", STEP_CASES,
                         ids=["S%d-%dx%d-mode%d-refine%d-head%d-%s" % (c[:6] + ("graph" if c[6] else "eager",)) for c in STEP_CASES])
def test_step_from_random_state(cuda, S, H, W, mode, refine, head0, use_graph):
    cfg, ocfg, P = _setup(H, W)
    st, guards = M.guarded_stream(P, H, W, cfg, S, cuda, mode, refine=refine, use_graph=use_graph)
    assert st.depth == DEPTH
    # refine == 2: the first pass's mask is the black of a refine=1 stream stepped from the identical state
    first = M.guarded_stream(P, H, W, cfg, S, cuda, mode, refine=1)[0] if refine == 2 else None
    zeros = torch.zeros((S, H, W), dtype=torch.float32, device=cuda)
    st.start(zeros)
    if first is not None:
        first.start(zeros)
    what = "S=%d %dx%d mode %d refine %d head %d" % (S, H, W, mode, refine, head0)
    errs = []
    for rep in range(2 if use_graph else 1):              # graph: step 0 runs eagerly and is captured, step 1 is a replay
        state = M.random_state(_case_seed(S, H, W, mode, refine, head0, rep), S, DEPTH, H, W)
        M.load_state(st, state, head0)
        cur = torch.from_numpy(state["cur"]).to(cuda)
        st.step(cur)
        got = M.snapshot(st)
        pass1 = None
        if first is not None:
            M.load_state(first, state, head0)
            first.step(cur)
            pass1 = M.snapshot(first)
        errs.append(M.check_step(got, state, head0, DEPTH, P, ocfg, refine, "%s step %d" % (what, rep), pass1))
        M.check_guards(guards, what)
    if use_graph:
        assert st._graph is not None, "the second step was not a graph replay"
    print("MEASURED %s %s: theta vs oracle %s" % (what, "graph" if use_graph else "eager", " ".join(
        ("%.2e" % e) if refine == 1 else ("%.2e (unforced %.2e)" % (e, p)) for e, p in errs)))


def _clips(seeds, H, W, T):
    from stabnet_amd import synthetic
    return np.stack([synthetic.make_clip(H, W, T, seed=s, margin=32) for s in seeds], axis=1)      # [T][S][H][W]


def _run_lock_step(cuda, seeds, T, singles=False, agree=False, oracle_at=(), tamper=None):
    """The S-stream object (operand mode 4, graph replay, canary-banded buffers) over T frames of len(seeds) clips.  Per step: the ring
    is what the steps before left (bit for bit), the push and the head as in test 1, all_black grows by the stream's own mask; with
    `singles` every stream against a single-stream object stepped from the same ring planes; with `agree` (one clip for every stream)
    the streams against each other; at the steps of `oracle_at` the oracle comparison of test 1.  tamper(st, t): called after step t
    (test_planted_copy_is_noticed)."""
    from stabnet_amd.deploy import StabNetStream
    H, W, S = 64, 96, len(seeds)
    cfg, ocfg, P = _setup(H, W)
    clips = _clips(seeds, H, W, T)
    dclips = torch.from_numpy(clips).to(cuda)
    st, guards = M.guarded_stream(P, H, W, cfg, S, cuda, 4, use_graph=True)
    st.start(dclips[0])
    ones = []
    if singles:
        for s in range(S):
            one = StabNetStream(P, H, W, cfg, streams=1, device=cuda, use_graph=True, operand_mode=4)
            one.start(dclips[0, s:s + 1])
            ones.append(one)
    expect_f, expect_m = st.frames_ring.clone(), st.masks_ring.clone()
    assert torch.equal(expect_f, dclips[0][:, None].expand(S, DEPTH, H, W)) and not bool(expect_m.any())
    res = {"theta": 0.0, "out": 0.0, "bits": True, "oracle": {}, "cross_theta": 0.0, "cross_out": 0.0, "cross_bits": True}
    for t in range(1, T):
        head0 = (t - 1) % DEPTH
        assert st.head == head0, t
        # the ring between two steps is what the steps so far pushed
        assert torch.equal(st.frames_ring, expect_f) and torch.equal(st.masks_ring, expect_m), "step %d: the ring is not what the earlier steps pushed" % t
        state = {"frames": expect_f.cpu().numpy(), "masks": expect_m.cpu().numpy(), "cur": clips[t],
                 "preset": st.all_black.cpu().numpy()}
        for s, one in enumerate(ones):
            one.frames_ring[0].copy_(st.frames_ring[s]); one.masks_ring[0].copy_(st.masks_ring[s]); one.head_dev.copy_(st.head_dev)
        st.step(dclips[t])
        got = M.snapshot(st)
        what = "S=%d step %d" % (S, t)
        M.check_movement(got, state, head0, DEPTH, what)
        M.check_all_black(got, state, what)
        for s, one in enumerate(ones):
            r1 = one.step(dclips[t, s:s + 1])
            dth = float((r1["theta"][0] - st.theta[s]).abs().max())
            dout = float((r1["output"][0] - st.out_img[s]).abs().max())
            res["theta"], res["out"] = max(res["theta"], dth), max(res["out"], dout)
            res["bits"] &= torch.equal(r1["theta"][0], st.theta[s]) and torch.equal(r1["output"][0], st.out_img[s]) \
                and torch.equal(one.frames_ring[0], st.frames_ring[s]) and torch.equal(one.masks_ring[0], st.masks_ring[s])
            assert dth <= LOCK_THETA and dout <= LOCK_OUT, "%s stream %d against its single stream: theta %.3e output %.3e" % (what, s, dth, dout)
            assert one.head == (head0 + 1) % DEPTH
        if agree:                                          # one clip for every stream: the streams agree with each other
            dth = float((st.theta - st.theta[0:1]).abs().max())
            dout = float((st.out_img - st.out_img[0:1]).abs().max())
            res["cross_theta"], res["cross_out"] = max(res["cross_theta"], dth), max(res["cross_out"], dout)
            res["cross_bits"] &= dth == 0.0 and dout == 0.0
            assert dth <= LOCK_THETA and dout <= LOCK_OUT, "%s: streams fed one clip differ: theta %.3e output %.3e" % (what, dth, dout)
        if t in oracle_at:
            res["oracle"][t] = M.check_numerics(got, M.oracle_step(state, head0, P, ocfg, 1), what)
            M.check_warp_exact(got, state, ocfg, what)
        expect_f[:, head0] = st.frame_fb
        expect_m[:, head0] = st.black
        M.check_guards(guards, what)
        if tamper is not None:
            tamper(st, t)
    assert st._graph is not None
    return res


def test_lock_step_across_the_wrap(cuda):
    res = _run_lock_step(cuda, (1, 2, 3), 40, singles=True, oracle_at=(1, 17, 33, 39))
    print("MEASURED S=3 lock step over the wrap, 39 steps: against the single streams theta %.2e output %.2e, bit-identical: %s; "
          "theta vs oracle at steps %s" % (res["theta"], res["out"], res["bits"],
                                           " ".join("%d: %.2e" % kv for kv in sorted(res["oracle"].items()))))
    same = _run_lock_step(cuda, (1, 1, 1, 1), 40, agree=True)
    print("MEASURED S=4 on one clip, 39 steps: streams differ by theta %.2e output %.2e, bit-identical: %s" % (
        same["cross_theta"], same["cross_out"], same["cross_bits"]))


def test_planted_copy_is_noticed(cuda):
    """The guard of the guard: stream 0's pushed frame copied by hand over stream 1's slot after step 2 fails the lock-step run."""
    def plant(st, t):
        if t == 2:
            st.frames_ring[1, (st.head - 1) % DEPTH].copy_(st.frames_ring[0, (st.head - 1) % DEPTH])
    with pytest.raises(AssertionError, match="step 3: the ring is not what the earlier steps pushed"):
        _run_lock_step(cuda, (1, 2, 3), 5, tamper=plant)


# ------------------------------------------------------------------------------------------------ 3. batched regressor, mode 4
@functools.lru_cache(maxsize=None)
def _regressor_reference(H, W, N):
    """N distinct samples, theta of the float64 evaluation of the same float32 parameters and input (moving-average BN; rows are
    independent, so the first n rows are the reference of batch n), and the single-sample GPU forwards of both operand modes."""
    from oracle import torch_ref as T
    from stabnet_amd.regressor import Regressor
    cfg, ocfg, P = _setup(H, W)
    x = np.random.default_rng([H, W]).uniform(-0.5, 0.5, (N, H, W, cfg.in_ch)).astype(np.float32)
    with torch.no_grad():
        want, _, _ = T.get_resnet(T.t(x), {k: T.t(v) for k, v in P.items()}, ocfg, False)
    dev = torch.device("cuda:0")
    xt = torch.from_numpy(x).to(dev)
    single = {}
    for mode in (0, 4):
        reg = Regressor(P, 1, H, W, cfg, device=dev, operand_mode=mode)
        single[mode] = np.concatenate([reg(xt[i:i + 1]).cpu().numpy() for i in range(N)])
    return x, want.numpy(), single


@pytest.mark.parametrize("N,H,W", [(3, 64, 96), (4, 64, 96), (5, 64, 96), (8, 64, 96), (9, 64, 96), (3, 72, 136)])
def test_batched_regressor_mode4(cuda, N, H, W):
    from stabnet_amd.regressor import Regressor
    cfg, ocfg, P = _setup(H, W)
    x, want, single = _regressor_reference(H, W, 9 if (H, W) == (64, 96) else N)
    xt = torch.from_numpy(x[:N]).to(cuda)
    err = {}
    for mode in (0, 4):
        theta = Regressor(P, N, H, W, cfg, device=cuda, operand_mode=mode)(xt).cpu().numpy()
        assert np.isfinite(theta).all()
        err[mode] = float(np.abs(theta.astype(np.float64) - want[:N]).max())
        rows = float(np.abs(theta - single[mode][:N]).max())
        assert rows <= F32_BAR, "mode %d N=%d: a row is %.3e off the single-sample forward of its sample" % (mode, N, rows)
    print("MEASURED N=%d %dx%d: theta vs float64 mode 4 %.3e, mode 0 %.3e" % (N, H, W, err[4], err[0]))
    assert err[0] < F32_BAR and err[4] < F32_BAR, err
    assert err[4] <= 2 * err[0] + 1e-7, err


# ------------------------------------------------------------------------------------------------ 4. the padded stack assembly
def test_padded_stack_assembly(cuda, tmp_path):
    S, H, W, mode, refine, head0, _ = STEP_CASES[1]
    out = str(tmp_path / "padded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_STEM_ROWRUN="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multistream_child.py"), out, str(S), str(H), str(W), str(mode),
                        str(refine), str(head0)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(np.load(out))
    cfg, ocfg, P = _setup(H, W)
    state = M.random_state(_case_seed(S, H, W, mode, refine, head0), S, DEPTH, H, W)
    assert np.array_equal(got["cur"], state["cur"])
    # the child ran the 16-channel assembly: its launch record moves in_ch + 16 floats per pixel (the bordered one: in_ch + in_ch),
    # and no conv launch is the row-run stem (conv_ring_f32_kernel<2, ..>)
    names = [str(n) for n in got["names"]]
    assert float(got["assemble_bytes"]) == 4.0 * S * H * W * (cfg.in_ch + 16), float(got["assemble_bytes"])
    assert not any(n.startswith("conv_ring_f32_kernel<2,") for n in names), names
    assert int(got["canaries_bad"]) == 0
    what = "STABNET_STEM_ROWRUN=0 S=%d %dx%d mode %d head %d" % (S, H, W, mode, head0)
    worst, _ = M.check_step(got, state, head0, DEPTH, P, ocfg, refine, what)
    print("MEASURED %s: theta vs oracle %.2e" % (what, worst))
