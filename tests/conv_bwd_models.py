"""Float64 references of the convolution backward operators, shared by test_conv_bwd_step_gpu.py (which holds the kernels to them)
and test_conv_bwd_models_cpu.py (which holds THEM to torch autograd, so that a wrong model cannot agree with a wrong kernel)."""
import numpy as np
import torch
import torch.nn.functional as Fnn


def conv_out(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def tower_grads(x, dy, w_shape, sc, sh, stride, pad, w=None):
    """One tower by torch CPU float64 autograd (the construction of test_conv_backward): -> (dW OHWI, d_bias, d act(x)).
    w: the weights dx is taken at (zeros when only dW is wanted)."""
    xt = torch.tensor(np.asarray(x, np.float64))
    wt = torch.tensor(np.zeros(w_shape) if w is None else np.asarray(w, np.float64), requires_grad=True)
    a = torch.relu(xt * torch.tensor(np.asarray(sc, np.float64)) + torch.tensor(np.asarray(sh, np.float64))) if sc is not None else xt
    a = a.detach().requires_grad_(True)
    y = Fnn.conv2d(a.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
    g = torch.tensor(np.asarray(dy, np.float64))
    assert tuple(y.shape) == tuple(g.shape)
    (y * g).sum().backward()
    return wt.grad.numpy(), g.reshape(-1, g.shape[-1]).sum(0).numpy(), a.grad.numpy()


def towers_wgrad(towers, w_shape, stride, pad):
    """The two-tower reference: ONE autograd graph in which every tower (x, dy, in_scale, in_shift) convolves its own input with
    the SHARED weight leaf and the losses are added -- the weight gradient autograd leaves on that leaf -> (dW, d_bias)."""
    wt = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(w_shape[0], dtype=torch.float64, requires_grad=True)
    loss = 0.0
    for x, dy, sc, sh in towers:
        xt = torch.tensor(np.asarray(x, np.float64))
        a = torch.relu(xt * torch.tensor(np.asarray(sc, np.float64)) + torch.tensor(np.asarray(sh, np.float64))) if sc is not None else xt
        y = Fnn.conv2d(a.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), bias=bias, stride=stride, padding=pad).permute(0, 2, 3, 1)
        loss = loss + (y * torch.tensor(np.asarray(dy, np.float64))).sum()
    loss.backward()
    return wt.grad.numpy(), bias.grad.numpy()


KPERM_ROWS = (1, 0, 2)                                     # stored tap row j of a 3x3 stride-2 layer holds tap row KPERM_ROWS[j]


def dgrad_kperm(k, stride):
    return k == 3 and stride == 2


def pack_dgrad_model(w, stride):
    """w OHWI [Cout][K][K][Cin] -> the dgrad weights wt[ci][kh'][kw][co] = w[co][K-1-kh][K-1-kw][ci] (same dtype: a pure
    permutation), the tap rows kh' stored in the order (1, 0, 2) for the 3x3 filters of stride-2 layers."""
    w = np.asarray(w)
    k = w.shape[1]
    wt = np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))
    if dgrad_kperm(k, stride):
        wt = np.ascontiguousarray(wt[:, list(KPERM_ROWS)])
    return wt


def dgrad_from_packed(dy, wt_stored, x_shape, stride, pad):
    """dx [N,H,W,Cin] in float64 from dy and the re-packed weights as stored: the stride-dilated dy, zero-padded by K - 1 - pad,
    convolved at stride 1 with wt[ci][kh][kw][co] (the convolution the dgrad kernel runs)."""
    N, H, W, Cin = x_shape
    wt = np.asarray(wt_stored, np.float64)
    k = wt.shape[1]
    if dgrad_kperm(k, stride):
        logical = np.empty_like(wt)
        logical[:, list(KPERM_ROWS)] = wt                  # stored row j is tap row KPERM_ROWS[j]
        wt = logical
    dy = np.asarray(dy, np.float64)
    _, Ho, Wo, Cout = dy.shape
    lo = k - 1 - pad
    canvas = np.zeros((N, H + k - 1, W + k - 1, Cout))
    canvas[:, lo:lo + (Ho - 1) * stride + 1:stride, lo:lo + (Wo - 1) * stride + 1:stride, :] = dy
    dx = np.zeros((N, H, W, Cin))
    for kh in range(k):
        for kw in range(k):
            dx += canvas[:, kh:kh + H, kw:kw + W, :] @ wt[:, kh, kw, :].T
    return dx
