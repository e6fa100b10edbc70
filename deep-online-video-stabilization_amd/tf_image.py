"""The reference's get_img (get_data_mini_after.py:149-156) on the device (csrc/tf_image.hip): decoded uint8 BGR frames to channels
of a training tensor, TensorFlow 1.3's rgb_to_grayscale / convert_image_dtype / resize_images(method=0) / - 0.5, one launch per
destination tensor."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._tensor import ptr, stream_ptr

FIELDS = 6            # int64 per entry: byte offset from the frames' base, sh, sw, row stride in bytes, n, c
MAX_C = 32


def make_table(entries, frames_bytes: int, N: int, C: int) -> np.ndarray:
    """entries: iterable of (byte offset, sh, sw, row stride in bytes, n, c) -> int64 [n_entries, 6], checked on the host (the
    kernel does not follow an entry that fails these checks; here it is an error that says which)."""
    t = np.asarray(list(entries), np.int64).reshape(-1, FIELDS)
    if len(t) == 0:
        raise _lib.StabnetError("tf_image: the table has no entry")
    for i, (off, sh, sw, rs, n, c) in enumerate(t.tolist()):
        if not (1 <= sh <= 65536 and 1 <= sw <= 65536 and 3 * sw <= rs <= 1 << 31):
            raise _lib.StabnetError("tf_image: entry %d: bad frame %dx%d with rows %d bytes apart" % (i, sw, sh, rs))
        if off < 0 or off + (sh - 1) * rs + 3 * sw > frames_bytes:
            raise _lib.StabnetError("tf_image: entry %d: frame at byte %d (%dx%d, rows %d bytes apart) does not lie inside the %d bytes "
                                    "of frames" % (i, off, sw, sh, rs, frames_bytes))
        if not (0 <= n < N and 0 <= c < C):
            raise _lib.StabnetError("tf_image: entry %d: destination (n %d, c %d) outside [%d, H, W, %d]" % (i, n, c, N, C))
    return t


def get_img(frames_u8, table, dst, prof=None):
    """frames_u8: uint8 device tensor that holds every source frame (1-D or any shape; byte offsets count from its first byte);
    table: int64 [n_entries, 6] -- a host array (make_table checks it, then it is uploaded) or a device tensor made earlier
    (nothing is copied: the call can be captured in a hipGraph); dst: contiguous float32 [N,H,W,C] device tensor, written in place."""
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
        raise _lib.StabnetError("tf_image.get_img: frames must be a contiguous uint8 tensor on the GPU (there is no CPU fallback)")
    if not isinstance(dst, torch.Tensor) or not dst.is_cuda or dst.dtype != torch.float32 or dst.dim() != 4 or not dst.is_contiguous():
        raise _lib.StabnetError("tf_image.get_img: dst must be a contiguous float32 [N,H,W,C] tensor on the GPU")
    if dst.device != frames_u8.device:
        raise _lib.StabnetError("tf_image.get_img: frames on %s, dst on %s" % (frames_u8.device, dst.device))
    N, H, W, C = dst.shape
    if C > MAX_C:
        raise _lib.StabnetError("tf_image.get_img: dst has %d channels, the kernel takes at most %d" % (C, MAX_C))
    if not isinstance(table, torch.Tensor):
        table = torch.from_numpy(make_table(table, frames_u8.numel(), N, C)).to(dst.device)
    if not table.is_cuda or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != FIELDS or not table.is_contiguous() \
            or table.device != dst.device:
        raise _lib.StabnetError("tf_image.get_img: table must be a contiguous int64 [n, %d] tensor on %s" % (FIELDS, dst.device))
    _lib.call("stabnet_tf_get_img", ptr(frames_u8), frames_u8.numel(), ptr(table), table.shape[0], ptr(dst), N, H, W, C,
              stream_ptr(dst.device), prof.handle if prof is not None else 0, device=dst.device)
    return dst
