"""CPU: the float64 models test_conv_bwd_step_gpu.py holds the backward kernels to (tests/conv_bwd_models.py) against torch
autograd -- a wrong model must not be able to agree with a wrong kernel."""
import numpy as np
import pytest

import conv_bwd_models as M

# N,H,W,Cin,Cout,k,stride,pad: a 1x1, a 3x3 / stride 1 and a 3x3 / stride 2 layer (tap rows stored 1, 0, 2), odd sizes
PACK_CASES = [(2, 5, 7, 8, 12, 1, 1, 0), (2, 5, 7, 8, 12, 3, 1, 1), (2, 7, 9, 8, 12, 3, 2, 1), (1, 8, 6, 4, 8, 3, 2, 1)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad", PACK_CASES)
def test_repack_model_convolved_with_dilated_dy_is_autograd_dx(N, H, W, Cin, Cout, k, stride, pad):
    rng = np.random.default_rng(100 * k + stride)
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    x = rng.standard_normal((N, H, W, Cin))
    w = rng.standard_normal((Cout, k, k, Cin))
    dy = rng.standard_normal((N, Ho, Wo, Cout))
    _, _, want = M.tower_grads(x, dy, w.shape, None, None, stride, pad, w=w)
    wt = M.pack_dgrad_model(w, stride)
    assert wt.shape == (Cin, k, k, Cout) and wt.dtype == w.dtype
    # the layout, element by element (written out, not by the slicing the model itself uses)
    rows = M.KPERM_ROWS if (k == 3 and stride == 2) else tuple(range(k))
    for ci in (0, Cin - 1):
        for j in range(k):
            for kw in range(k):
                for co in (0, Cout - 1):
                    assert wt[ci, j, kw, co] == w[co, k - 1 - rows[j], k - 1 - kw, ci]
    got = M.dgrad_from_packed(dy, wt, (N, H, W, Cin), stride, pad)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    if k == 3 and stride == 2:                               # the row order matters: the unpermuted tensor must NOT pass
        bad = M.dgrad_from_packed(dy, np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)), (N, H, W, Cin), stride, pad)
        assert np.abs(bad - want).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("k,stride,pad,pro", [(1, 1, 0, True), (3, 1, 1, True), (3, 2, 1, False)])
def test_two_tower_reference_is_the_sum_of_per_tower_autograd(k, stride, pad, pro):
    rng = np.random.default_rng(7 + k + stride)
    N, H, W, Cin, Cout = 2, 6, 5, 4, 8
    Ho, Wo = M.conv_out(H, W, k, stride, pad)
    towers = []
    for _ in range(2):
        towers.append((rng.standard_normal((N, H, W, Cin)), rng.standard_normal((N, Ho, Wo, Cout)),
                       rng.uniform(0.5, 1.5, Cin) if pro else None, rng.standard_normal(Cin) * 0.3 if pro else None))
    dw, db = M.towers_wgrad(towers, (Cout, k, k, Cin), stride, pad)
    parts = [M.tower_grads(x, dy, (Cout, k, k, Cin), sc, sh, stride, pad) for x, dy, sc, sh in towers]
    want_w = parts[0][0] + parts[1][0]
    want_b = towers[0][1].reshape(-1, Cout).sum(0) + towers[1][1].reshape(-1, Cout).sum(0)
    assert np.abs(dw - want_w).max() <= 1e-12 * np.abs(want_w).max()
    assert np.abs(db - want_b).max() <= 1e-12 * np.abs(want_b).max()
    assert np.abs(parts[0][1] + parts[1][1] - want_b).max() <= 1e-12 * np.abs(want_b).max()
    # the towers' data are independent: tower 0's gradient alone is far from the sum
    assert np.abs(parts[0][0] - want_w).max() > 1e-2 * np.abs(want_w).max()
