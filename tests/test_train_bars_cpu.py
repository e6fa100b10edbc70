"""CPU, the oracle alone: the float32 floors behind the training step's gradient bars (tests/_train_bars.py), and the input
conditions under which those bars mean something.

Per shape, ONE float64 forward + backward and one float32 pass of oracle/torch_ref.train_objective with the float64 decisions forced:

  * the committed table _train_bars.FLOORS reproduces within a factor 1.5 (the float32 pass runs on ONE thread, where it reproduces
    to the last digit under 2 / 3 / 8 / 16 threads for everything else; the factor is for another BLAS.  With the float32 pass
    itself spread over 1 .. 16 threads the class R floors move by up to 1.5, the class Z element floor -- a maximum of cancellation
    noise -- by up to 3);
  * no class R bar in force exceeds 1e-3, and class Z is what it is said to be: exactly the 21 `/biases` of resnet_v2_50, each in
    front of a batch-statistics BN;
  * (a) the decisions that differ between the float32 and the float64 evaluation number at most 20 (measured 2, 5, 13, 6, 1): the
    float32 gradient really is the float64 one of the same piece plus rounding;
  * (b) tail share: for the four sampled conv1 weights and block1/unit_1/conv3, the part of the data gradient X^T dY that comes from
    the last M % 32 pixel rows of each tower -- the rows a tile loop over 32 rows would drop -- is, wherever M % 32 != 0, at least
    10 x the shape's class R bar (measured 1.15e-2 .. 1.0 against bars of 1.1e-4 .. 2.2e-4): a kernel that lost them fails the bar.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _train_bars as B

SHAPES = [(2, 64, 96), (3, 64, 96), (3, 90, 130), (1, 75, 101), (5, 40, 56)]
# tower rows M at the five sampled layers: block{1,2,3,4}/unit_1/conv1, block1/unit_1/conv3
ROWS = {(2, 64, 96): (768, 192, 48, 12, 768), (3, 64, 96): (1152, 288, 72, 18, 1152), (3, 90, 130): (2277, 612, 162, 45, 2277),
        (1, 75, 101): (494, 130, 35, 12, 494), (5, 40, 56): (700, 175, 60, 20, 700)}


def test_table_covers_the_shapes():
    assert set(B.FLOORS) == set(SHAPES)
    for s in SHAPES:
        bar = B.bars(*s)                                     # asserts the 1e-3 condition itself
        assert max(bar["R"]) <= 1e-3 and bar["whole"] < 1e-3
        print(s, "bars in force: class R %.2e / %.2e, class Z %.2e / %.2e, whole %.2e" % (bar["R"] + bar["Z"] + (bar["whole"],)))


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_float32_floors_flips_and_tail_share(N, H, W):
    r = B.reference_floors(N, H, W, B.BATCH_SEED, taps=True)
    f = B.FLOORS[(N, H, W)]
    print("floors %dx%dx%d: class R %.3e / %.3e  class Z %.3e / %.3e  whole %.3e  flips %d %s"
          % ((N, H, W) + r["R"] + r["Z"] + (r["whole"], r["n_flips"], r["flips"])))
    print("tail shares", {n: v[:2] for n, v in r["tail"].items()})
    # ---- the table
    for got, want, what in ((r["R"][0], f["R"][0], "R element"), (r["R"][1], f["R"][1], "R L2"), (r["Z"][0], f["Z"][0], "Z element"),
                            (r["Z"][1], f["Z"][1], "Z L2"), (r["whole"], f["whole"], "whole")):
        assert want / 1.5 <= got <= want * 1.5, "%s floor: table %.3e, recomputed %.3e" % (what, want, got)
    # ---- the classes
    z = sorted(n for n, c in r["classes"].items() if c == "Z")
    assert len(z) == 21 and all(n.startswith("resnet_v2_50/") and n.endswith("/biases") for n in z), z
    assert not [n for n, c in r["classes"].items() if c == "R" and n.startswith("resnet_v2_50/") and n.endswith("/biases")]
    # ---- (a) decision flips
    assert r["n_flips"] <= 20, r["flips"]
    # ---- (b) tail share
    bar = max(B.bars(N, H, W)["R"])
    assert tuple(r["tail"][n][0] for n in B.SAMPLED) == ROWS[(N, H, W)]
    # the float32 oracle itself passes the bars made from its floors
    B.check_gradient({"rows": r["rows"], "classes": r["classes"], "whole": r["whole"]}, N, H, W)
    ragged = [n for n in B.SAMPLED if r["tail"][n][0] % 32]
    for name in B.SAMPLED:
        M, share, tail = r["tail"][name]
        if M % 32:
            assert share >= 10 * bar, "%s: the last %d of %d rows carry %.3e of the data gradient, bar %.3e" % (name, M % 32, M, share, bar)
        else:
            assert share == 0.0 and tail is None
    # ... and the same float32 gradient WITHOUT those rows -- what a 32-row tile loop that forgot its tail would give -- does not
    # (the weight with the smallest share: the hardest to notice)
    name = min(ragged, key=lambda n: r["tail"][n][1])
    lost = dict(r["g32"])
    lost[name] = r["g32"][name] - r["tail"][name][2]
    with pytest.raises(AssertionError, match="class R"):
        B.check_gradient(B.measure_gradient(lost, r["g64"]), N, H, W)
