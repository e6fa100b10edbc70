"""GPU: the Trainer's data-parallel overlap path with a world of IDENTICAL ranks, in one process and without a process group.

torch.distributed.all_reduce is replaced (Trainer._allreduce_async looks it up at call time) by a stand-in for `world` ranks that
all hold this rank's gradient: on the current stream -- the communication stream -- it records (lo, hi, a clone of the slice) and
then multiplies the slice by `world`, which is what the sum over identical ranks is.  Trainer(process_group=None, world_size=world)
switches the communication path on (buckets handed over stage by stage, wait_stream joins) exactly as a real group would.

Unlike the one-rank RCCL test (test_rccl_gpu.py: a sum over one rank is the identity, so a `+=` that lands in a bucket after it was
reduced changes nothing) the factor makes every ordering mistake visible: a float that is written after its bucket went to the wire
misses the factor, a bucket that weight decay or Adam reads before the join misses it as well.

WHY BIT EQUALITY.  For world in {2, 8} every operation that carries the factor is an exact power-of-two scaling: the emulated sum is
world * g; the weight-decay coefficient is 2 regu_mul live world, rounded to float32 AFTER the (exact) multiplication, and the kernel's
gscale * coef, (gscale coef) * w and g + .. then scale exactly; Adam multiplies by gscale = 1 / world first and sees the plain
gradient.  Barring overflow (gradients are O(1)) and products below 2^-126, the DP step IS the plain step.  So:

  1. after forward_backward(apply_update=False): grads == world * plain.grads bit for bit, L2 term included;
  2. after 3 more steps with the update: params (trainables AND moving statistics), adam_m, adam_v and losses() are the plain
     trainer's bit for bit;
  3. the wire, every step: exactly n_stages + 1 calls, on the communication stream, on slices of the ONE gradient buffer, in the
     order buckets[0..3] then bn_bucket; the ranges tile [0, nt); every recorded clone equals that range of the step's RAW gradient
     (both towers, no L2 term) -- taken from a plain trainer with regu_mul = 0 that is given the DP trainer's parameters before each
     step (the tower gradient does not depend on regu_mul; adding 0 * w can only change the sign of a zero, so +0 == -0 here);
  4. the compute stream really joins the communication stream before weight decay: the same with a stand-in that sleeps ~3 ms on
     the communication stream before it multiplies (torch.cuda._sleep, calibrated with events).  Without the final wait_stream
     weight decay and Adam read unreduced buckets.

Cases (max_matches 48, all gates on, as tests/dp_child.py): 2 x 64 x 96 with world 2 and 8; 3 x 90 x 130 with world 2; the same with
split_operands=True; 2 x 64 x 96 world 2 with the slow stand-in.

MEASURED when the test was written (wall time per case: three Trainers, 4 steps each):
    2x64x96 world 2 1.28 s (first case of the process) | world 8 0.62 s | 3x90x130 world 2 0.67 s | split 0.67 s | slow 0.70 s
Every assertion held bit for bit as argued above; no operation broke the power-of-two argument.

FOUND when the test was written: Trainer(split_operands=<given>, world_size > 1) raised UnboundLocalError -- an `import os` inside
the `split_operands is None` branch of __init__ made `os` a local of the whole function, so the STABNET_COMM_RESERVED_CUS lookup of
the communication path failed whenever that branch was skipped.  Fixed in train.py (the module-level import serves both).

MUTATIONS tried on a scratch copy when the test was written, with what caught them:
    3. the final wait_stream(comm_stream) of forward_backward dropped, slow stand-in: assertion 3 of the first step, "what went to
       the wire as [264256, 1479232) against the raw gradient: 1 208 265 of 1 214 976 floats differ" -- bucket 2's turn on the
       communication stream comes behind the sleeps of buckets 0 and 1, and by then weight decay, which no longer waits, has added
       its L2 term to what is sent.  (The wire is checked first; assertion 1 is not reached.)
    4. `self.world` -> 1 in the weight-decay coefficient: assertion 1, "grads against world x the plain trainer's: 23 370 192 of
       30 405 108 floats differ".
"""
import dataclasses
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GATES = {"use_theta_loss": 1, "use_temp_loss": 1, "use_black_loss": 1, "use_theta_only": 0}
STEPS = 3
_ticks_per_ms = []


def _sleep_ticks(ms):
    """torch.cuda._sleep counts device clock ticks whose rate differs between runtimes: measure it once."""
    if not _ticks_per_ms:
        probe = 200000
        torch.cuda._sleep(probe)                                   # first launch: module load
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        torch.cuda.synchronize()
        _ticks_per_ms.append(probe / max(e0.elapsed_time(e1), 1e-3))
    return int(ms * _ticks_per_ms[0])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(got, want, what, zero_sign_free=False):
    neq = _bits(got) != _bits(want)
    if zero_sign_free:
        neq &= ~((got == 0) & (want == 0))
    if bool(neq.any()):
        i = int(torch.nonzero(neq.flatten())[0])
        raise AssertionError("%s: %d of %d floats differ, first at %d: %r against %r" % (
            what, int(neq.sum()), neq.numel(), i, float(got.flatten()[i]), float(want.flatten()[i])))


def _run(cuda, monkeypatch, N, H, W, world, split, sleep_ms=0.0):
    import torch.distributed as dist
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.train import Trainer
    t0 = time.perf_counter()
    cfg = Config(height=H, width=W, batch_size=N, max_matches=48)
    P = synthetic.make_params(cfg, seed=0, theta_scale=0.3)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in synthetic.make_train_batch(cfg, N, H, W, 5).items()}
    ticks = _sleep_ticks(sleep_ms) if sleep_ms else 0
    wire = []

    def all_reduce(tensor, op=None, group=None, async_op=False):
        assert group is None and not async_op
        lo = tensor.storage_offset()
        wire.append((lo, lo + tensor.numel(), tensor.clone(), torch.cuda.current_stream(cuda), tensor.untyped_storage().data_ptr()))
        if ticks:
            torch.cuda._sleep(ticks)
        tensor.mul_(world)

    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    plain = Trainer(P, N, H, W, cfg, device=cuda, split_operands=split)
    raw = Trainer(P, N, H, W, dataclasses.replace(cfg, regu_mul=0.0), device=cuda, split_operands=split)
    dp = Trainer(P, N, H, W, cfg, device=cuda, process_group=None, world_size=world, split_operands=split)
    assert dp.comm and dp.comm_stream is not None and not plain.comm and not raw.comm
    nt = dp.nt
    what = "%dx%dx%d world %d%s%s" % (N, H, W, world, " split" if split else "", " slow" if sleep_ms else "")

    def step(update):
        raw.params.copy_(dp.params)                # the raw gradient of THIS step: the DP trainer's weights and moving statistics
        del wire[:]
        plain.forward_backward(batch, GATES, apply_update=update)
        raw.forward_backward(batch, GATES, apply_update=False)
        dp.forward_backward(batch, GATES, apply_update=update)
        torch.cuda.synchronize()
        assert not plain.comm_stream and len(wire) == dp.n_stages + 1, (what, len(wire))
        # 3. the wire
        want = list(dp.buckets) + [dp.bn_bucket]
        assert [(lo, hi) for lo, hi, _, _, _ in wire] == want, (what, [(lo, hi) for lo, hi, _, _, _ in wire], want)
        edge = 0
        for lo, hi in sorted(want):
            assert lo == edge and hi > lo, (what, sorted(want))
            edge = hi
        assert edge == nt
        for lo, hi, sent, stream, storage in wire:
            assert stream == dp.comm_stream, "%s: bucket [%d, %d) was not reduced on the communication stream" % (what, lo, hi)
            assert storage == dp.grads.untyped_storage().data_ptr(), "%s: bucket [%d, %d) is not a slice of the gradient buffer" % (what, lo, hi)
            _assert_same_bits(sent, raw.grads[lo:hi], "%s: what went to the wire as [%d, %d) against the raw gradient" % (what, lo, hi),
                              zero_sign_free=True)

    # 1. (and 4. with the slow stand-in) the summed gradient, L2 term included
    step(False)
    assert bool(torch.isfinite(plain.grads).all()) and float(plain.grads.abs().max()) > 0
    _assert_same_bits(dp.grads, plain.grads * world, "%s: grads against world x the plain trainer's" % what)
    # 2. three updates
    for _ in range(STEPS):
        step(True)
        _assert_same_bits(dp.grads, plain.grads * world, "%s: grads against world x the plain trainer's, step %d" % (what, dp.global_step))
    assert dp.global_step == plain.global_step == STEPS + 1
    _assert_same_bits(dp.params[:nt], plain.params[:nt], what + ": trainables after %d updates" % STEPS)
    _assert_same_bits(dp.params[nt:], plain.params[nt:], what + ": moving statistics after %d updates" % STEPS)
    _assert_same_bits(dp.adam_m, plain.adam_m, what + ": adam_m")
    _assert_same_bits(dp.adam_v, plain.adam_v, what + ": adam_v")
    assert float((dp.params[:nt] - torch.from_numpy(dp.plan.pack(P)[:nt]).to(cuda)).abs().max()) > 0      # the updates happened
    assert dp.losses() == plain.losses(), (what, dp.losses(), plain.losses())
    print("MEASURED %s: %.2f s" % (what, time.perf_counter() - t0))


@pytest.mark.parametrize("N,H,W,world,split", [(2, 64, 96, 2, False), (2, 64, 96, 8, False), (3, 90, 130, 2, False),
                                               (3, 90, 130, 2, True)])
def test_emulated_world_step_is_the_plain_step(cuda, monkeypatch, N, H, W, world, split):
    _run(cuda, monkeypatch, N, H, W, world, split)


def test_compute_stream_joins_a_slow_collective(cuda, monkeypatch):
    _run(cuda, monkeypatch, 2, 64, 96, 2, False, sleep_ms=3.0)
