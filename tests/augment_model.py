"""NumPy model of the contrast mean as csrc/augment.hip sums it (aug_resize_crop_kernel + aug_means_kernel).  The kernels add in a
fixed, documented order, so the float32 mean can be stated exactly instead of being compared through a tolerance:
  * the row-major [H,W] plane is cut into blocks of 256 pixels, lanes past the end of the plane hold 0.0;
  * per block, lane l (0..63) adds ((t[l] + t[l+64]) + t[l+128]) + t[l+192] in float64, then the 64 lanes go through the xor
    butterfly s = s + s[lane ^ off], off = 32, 16, ..., 1, and lane 0 holds the block's partial sum;
  * across blocks, lane l adds the partials l, l+64, ... in that order to 0.0, the same butterfly follows, and the mean is
    float32(s / float64(H*W))."""
import numpy as np

BLOCK = 256
WAVE = 64


def _butterfly(s):
    """s [..., 64] float64 -> lane 0 after s += s[lane ^ off], off = 32..1 (every lane takes part in every step)."""
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off >= 1:
        s = s + s[..., lanes ^ off]
        off >>= 1
    return s[..., 0]


def kernel_channel_mean(img):
    """The float32 mean of one [H,W] float32 plane, in the kernels' summation order."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 2
    count = img.size
    nblk = (count + BLOCK - 1) // BLOCK
    t = np.zeros(nblk * BLOCK, np.float64)
    t[:count] = img.reshape(-1)
    t = t.reshape(nblk, 4, WAVE)
    partial = _butterfly(((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3])              # [nblk]
    rounds = (nblk + WAVE - 1) // WAVE
    p = np.zeros(rounds * WAVE, np.float64)
    p[:nblk] = partial
    live = (np.arange(rounds * WAVE) < nblk).reshape(rounds, WAVE)
    p = p.reshape(rounds, WAVE)
    s = np.zeros(WAVE, np.float64)
    for r in range(rounds):
        s = np.where(live[r], s + p[r], s)                                        # a lane adds only the partials that exist
    return np.float32(_butterfly(s) / np.float64(count))
