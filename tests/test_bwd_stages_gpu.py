"""GPU: the device-side promise that data-parallel overlap rests on, at the C ABI (no Trainer, no process group).

stabnet_towers_bwd_stage(k) / stabnet_tower_bwd_stage(k) promise that when the stage's kernels are done the float range
stabnet_net_grad_bucket(k) of the ONE gradient buffer is final.  train.py hands that range to the collective on a second stream while
stages k+1.. keep writing into the same buffer, so a late write into an earlier bucket, a slab reduction still pending when a stage
returns, or a 16-byte read-modify-write across a bucket boundary would corrupt an N > 1 run and show nothing on one GPU: the other
tests only see the gradient after all four stages.  The gradients themselves are held to float64 elsewhere (test_train_gpu.py,
test_train_ragged_gpu.py, test_train_trajectory_gpu.py); this file pins WHEN and WHERE they are written.

Per case (tests/_bwd_stages.py): the lockstep (T = 2) or single-tower (T = 1) training forward once, into workspaces of exactly the
queried size between canary bands and filled with 0xEE; then stages 0..3 one call at a time into a canary-banded gradient buffer,
with a synchronize and a copy of the buffer's bits after each call: S_-1 (before), S_0 .. S_3.  B_k = grad_bucket(k),
BN = bn_grad_range().  Rules 1-5 are equalities of uint32 images of the same code's output at different moments: no tolerance.

  1. FINAL       S_k[B_k] == S_3[B_k].
  2. ISOLATION   S_k differs from S_k-1 only inside B_k and BN.
  3. BN RANGE    printed per stage (first / last tensor that changed); asserted: every gamma / beta tensor moved at some stage, and
                 for T = 1 the range after stage 3 is the one-shot backward's (rule 5).  The header promises no more.
  4. NOT VACUOUS every conv / FC weight and bias tensor of plan.table inside B_k changed between S_k-1 and S_k.  The pad channels
                 of the stem's OHWI weight (in_ch .. in_ch_pad - 1, from the table's dims) are left out of "changed" and must stay
                 untouched: the row-run scatter never writes them, the padded path adds exact zeros.
  5. STAGED = ONE SHOT  T = 1: stabnet_tower_bwd_stage x 4 gives the bits of one stabnet_tower_bwd.
  6. ACCUMULATION the same four stages into a base G0 = N(0, 1) x (RMS of the tensor's own zero-base gradient), tensor by tensor.
                 Rules 1, 2 and 4 again, and |(result - G0) - Z| <= eps32 (|G0| + 2 P) per element in float64, Z the zero-base
                 gradient, eps32 = 2^-23, P the magnitudes of the partial sums added into the element.
  7. GUARDS      the canary bands around the gradient buffer and around every workspace are intact.

THE ADD COUNT of rule 6, from the code.  Per backward an element of the buffer receives ONE add, or with T = 2 TWO in these places:
  * conv weights: one wgrad launch per layer for both towers writes slabs [tower][split] with plain stores, and the stage's
    wgrad_reduce_flush adds their ordered sum into the gradient ONCE (conv_bwd.hip, wgrad_reduce_kernel: o += acc); a layer with a
    single split and T = 1 adds its accumulator directly, once.  The stem's row-run gradient is reduced into a zeroed scratch and
    the scatter adds it into the OHWI tensor once.  Biases that ride in conv3's wgrad pass are slab entries: once.
  * fc_1..3: ONE fc_bwd launch over the [T N] pair: once.  The OUTPUT layer (fc_weights, fc_bias): one launch per tower: T adds.
  * biases on the separate reduction (bias_grad_finalize_kernel) and BN gamma / beta (bn_bwd_finalize_kernel): the finalize adds
    group after group: T adds.
With n adds a_1..a_n the base run rounds n times, the zero-base run n - 1 times (0 + a_1 is exact), each by at most eps32 / 2 of
the running sum: |difference| <= eps32 / 2 (n |G0| + (2 n - 1) sum |a_j|), which for n <= 2 is within eps32 (|G0| + 2 sum |a_j|).
sum |a_j|: T = 1: |Z|.  T = 2: the towers' partial gradients come from the same stages with the OTHER tower's d_theta zero (its
backward is then exactly zero); P = max(|Z|, |a_1| + |a_2|) covers the once-added elements as well.  A store in place of an add
misses the bound by |G0| / (eps32 |G0|) ~ 1e7.

CASES, the smallest that reach each route (route table: tests/test_train_ragged_gpu.py):
    2 x 64 x 96, T = 1 and 2   stride-1 wgrad with the bias in its pass, pair launches
    3 x 90 x 130, T = 2        general wgrad with ragged pixel splits; the separate bias reduction writes b3 and b_sc together
    1 x 75 x 101, T = 1        N = 1, odd sizes from the input on
    3 x 90 x 130, T = 2, stabnet_net_set_bf16_operands(plan, 4): the dgrad weight images written in stage 0, read by later stages
    2 x 64 x 96, T = 2, STABNET_STEM_ROWRUN=0 in a fresh child process (the switch is read once per process): the stem's general wgrad

MEASURED when the test was written (worst element of rule 6 as a fraction of its bound; wall time per case, plan creation included):
    2x64x96  T=1        0.499   1.50 s (the first case of the process)
    2x64x96  T=2        0.844   0.43 s
    3x90x130 T=2        0.824   0.33 s
    1x75x101 T=1        0.499   0.33 s
    3x90x130 T=2 split  0.901   0.34 s
    2x64x96  T=2, padded stem (child process)  0.849   0.73 s in the child, 2.79 s with its start
T = 1 sits at 1/2 -- one add, eps32 / 2 (|G0| + |Z|) against eps32 (|G0| + 2 |Z|) -- and T = 2 below 1, as the derivation says.
Per stage 86-99.99 % of a bucket's floats change (dead ReLU channels and the 2 floats of layout padding do not); the BN range changes
in disjoint pieces, stage 0: block4 + postnorm (20 480 of 45 440 floats), 1: block3 (17 408), 2: block2 (5 632), 3: block1 (1 920).

MUTATIONS tried on a scratch copy when the test was written, with what caught them:
    1. stabnet_net_grad_bucket(1).lo one layer too low (block2's last conv3 moved into bucket 1, the partition still tiles):
       rule 1, "bucket 1 changed after stage 1 returned, first at block2/unit_4/conv3/weights[0]".  test_lockstep_gpu.py stayed green.
    2. the projection shortcut's wgrad moved behind the stage's wgrad_reduce_flush, so its slabs are never reduced in that stage.
       For block1 only: rule 4, "stage 3 left block1/unit_1/shortcut/weights as it was"; test_lockstep_gpu.py stayed green (both of
       its forms lose the same tensor, and it skips tensors with no gradient).  For every projection unit: rule 4 at stage 0
       (block4/unit_1/shortcut/weights) -- and test_lockstep_gpu.py went red too (whole gradient 0.19 against 0.02): in block4
       the single-tower form has one split and adds its accumulator directly, so only the lockstep form loses the tensor.
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _bwd_stages as BS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(2, 64, 96, 1, False), (2, 64, 96, 2, False), (3, 90, 130, 2, False), (1, 75, 101, 1, False), (3, 90, 130, 2, True)]


@pytest.mark.parametrize("N,H,W,T,split", CASES)
def test_stage_buckets_are_final_and_isolated(cuda, N, H, W, T, split):
    BS.run_case(cuda, N, H, W, T, split)


def test_stage_buckets_with_the_padded_stem(cuda):
    """The stem on its other path (channels padded to 16, general wgrad straight into the OHWI tensor, no scatter)."""
    from stabnet_amd import _lib
    from stabnet_amd.config import Config
    from stabnet_amd.regressor import NetPlan
    N, H, W, T = 2, 64, 96, 2
    here = _lib.lib().stabnet_net_train_workspace_bytes(NetPlan(N, H, W, Config(height=H, width=W, batch_size=N), keep_activations=True).handle)
    env = dict(os.environ, PYTHONPATH=ROOT, STABNET_STEM_ROWRUN="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bwd_stages_child.py"), str(N), str(H), str(W), str(T), "0", str(here)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]
