"""GPU: the conv kernels at the TOP of the range the extent guards declare ("Conv extents"; tests/test_conv_extents_cpu.py holds
the guards themselves): ordinary parity tests of valid launches whose operands end just below 2^30 floats (4 GiB) from their pointers.

The extent comes from strides wherever an entry takes them, so the buffers are large and the work is tiny.  Every case is one run of
tests/conv_extents_child.py in a fresh process with its own time limit; the child allocates its large buffer once, NaN all over between
two canary bands, writes only the columns the launch reads, and gives every output a poisoned caller-owned buffer (_poison.py).

  A       1x1, stabnet_conv2d_fwd_packed_ld, M = 64 x 64, 64 -> 64 channels, x_ld = 262 140 (the largest multiple of 4 with M x_ld < 2^30)
  B       3x3 / stride 1 / pad 1, N = 2, 40 x 40, 64 and 128 channels, x_ld over the zero-padded pixel count (what the entry counts): the packed
          ring kernel (MODE 1) and, with STABNET_CONV_PATCH_MIN_M=1, both forms of the patch-stationary kernel
  C       3x3 / stride 2 / pad 1, N = 2, 41 x 41
  D       res_ld at the limit through the two entries that take one: stabnet_conv_unit_pair_fwd (M = 99 and 2 x 99 of
          unit_pair_child.CASES, the f32 and the packed form) and stabnet_conv3x3_conv1x1_fwd (plain and res_stride 2, N = 1 and 2)
  Dres    the residual's own size at the limit through the epilogues that no entry gives a res_ld: a stride-1 convolution + bias + a
          residual [2][2H][2W - 1][Cout] of 2^30 - 2^19 floats read at (2 oy, 2 ox), beside an output a quarter of that -- the strided
          m * res_ld of the register-staged (K = 16) and ring (K = 32) kernels (stabnet_conv2d_fwd_ex), both patch forms and the packed
          ring (stabnet_conv2d_fwd_packed; STABNET_CONV_PATCH_MIN_M=1 / STABNET_CONV_PATCH=0).  Its twin reads the same values from a
          dense [2][H][W][Cout] residual with res_stride 1 (the plain m * res_ld): all output bits agree.  About 7.5 GB at the peak
  E       dense input on the register-staged kernel: 1x1, 16 -> 4 channels, M 16 = 2^30 - 16
  F       dense output: 1x1, K = 16 (register-staged) and K = 32 (ring), 256 channels out, M 256 = 2^30 - 256
  G       the boundary plan of test_conv_extents_cpu.py at 1080 x 1920 (N = 25) end to end, operand mode 4 with fused unit pairs (what
          StabNetStream runs) AND operand mode 0, on a NaN-filled workspace

A - D run the launch twice, at the limit and re-laid at a small stride (Cin + 4: a multiple of 4 that is not Cin, so the route is the same),
and compare ALL output bits with == : only the offsets differ between the two.  A - D also hold every output element (a superset of the
sampled rows; Dres is sampled as E - F are, with the rows taken around those byte offsets of the residual), E - F the first and last 64-row tile, the rows on both sides of byte offsets 2^31 and 3 * 2^30 of the large operand and 64
rows drawn with a fixed seed, to a float64 evaluation of the float32 inputs, by test_route_census_gpu.py's bars (BAR_PLAIN, BAR_OUT_BN).
Every case asserts the kernel it ran (stabnet_conv_last_launch_kind), the canary bands, that no output stays NaN and that the large
buffer holds exactly the columns written, bit for bit.  G: the theta rows of samples 0, N / 2 and N - 1 (three different frames) within
2e-6 of the single-sample forwards (test_multistream_gpu.py F32_BAR; the N = 1 forward is held to the oracle by
test_baseline_sizes_gpu.py), or err(mode 4) <= 2 err(mode 0) + 1e-7.

G asserts from stabnet_net_step_info (host) what the plan holds at 96.6 % of the limit before it runs: mode 0, the exact-f32 ring kernel
(MODE 1) reading x_ld = 320 and the register-staged epilogue reading res_ld = 320 -- neither reachable through an entry, which take an
x_ld only together with a weight image and a res_ld only for the fused kernels; mode 4, the patch kernel reading x_ld = 320 and fused unit
pairs.  G does NOT put a residual near the limit on the ring or patch epilogues (the Dres cases do), and the row-run stem (MODE 2) is at
63 % of its limit there: a genuinely large bordered image is not built, the host-side guard (test_conv_extents_cpu.py) covers it.

MEASURED (MI355X; every child prints its own MEASURED lines): the first 18 children together 51 s, the five Dres children and G 18 s, most
of it starting Python; the launches and checks of a child take 0.2 - 0.7 s, case G 2.4 s with its host-side route assertions.  Dres, error
as a fraction of the bar: register-staged 0.005, ring 0.008, patch 0.021 (64 channels) and 0.037 (128), packed ring 0.021 (the patch
form's bits); every Dres launch gave the bits of its dense twin.  Error against float64 as a fraction of the bar: A 0.010; B 0.034 (64 channels) and 0.055
(128), the patch forms bit-identical to the ring forms; C 0.045; D unit pair 0.007 - 0.012, back-to-back 0.010 - 0.016; E 0.004; F 0.006
(register-staged) and 0.007 (ring).  Every at-the-limit launch of A - D gave the bits of its near-base twin.  G: rows 0, 12 and 24 of the
batch of 25 against the single-sample forwards 1.60e-7 in mode 4 with fused pairs, 1.49e-7 in mode 0 (bar 2e-6): the bar holds at N = 25."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "conv_extents_child.py")

# (case, environment of the child, time limit in seconds)
CASES = [("A", {}, 120), ("B64", {}, 120), ("B128", {}, 120), ("B64patch", {"STABNET_CONV_PATCH_MIN_M": "1"}, 120),
         ("B128patch", {"STABNET_CONV_PATCH_MIN_M": "1"}, 120), ("C", {}, 120),
         ("Dpair0", {}, 120), ("Dpair5", {}, 120), ("Dpair4", {}, 120), ("Dpair3", {}, 120),
         ("Db2b1", {}, 120), ("Db2b2", {}, 120), ("Db2b1s", {}, 120), ("Db2b2s", {}, 120),
         ("Dres16", {}, 180), ("Dres32", {}, 180), ("Dres64patch", {"STABNET_CONV_PATCH_MIN_M": "1"}, 180),
         ("Dres128patch", {"STABNET_CONV_PATCH_MIN_M": "1"}, 180), ("Dres64packed", {"STABNET_CONV_PATCH": "0"}, 180),
         ("E", {}, 180), ("F16", {}, 180), ("F32", {}, 180), ("G", {}, 300)]


@pytest.mark.parametrize("case,env,limit", CASES, ids=[c[0] for c in CASES])
def test_at_the_top_of_the_range(cuda, case, env, limit):
    r = subprocess.run([sys.executable, CHILD, case], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True, text=True, timeout=limit)
    print(r.stdout[-4000:])
    assert r.returncode == 0, "case %s: exit %d\n%s\n%s" % (case, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "case %s ok" % case in r.stdout
