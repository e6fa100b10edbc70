"""GPU: csrc/tf_image.hip (stabnet_tf_get_img) against tests/tf_image_model.py, BIT FOR BIT (torch.equal).

  sizes    down- and upscale, same size, a 5x1 source, strided rows with guard bytes between them
  layout   C = 14 and C = 2; entries of two source sizes in one launch; one source feeding three destinations
  memory   the destination sits between sentinel-filled guard bands and has a channel no entry names: both keep the sentinel; an
           entry whose frame or destination lies outside is not followed
  grey     a 4096x4096 frame that holds every RGB triple once, at its own size: all 2^24 grey bytes
  graph    the launch captured once and replayed twice over changing frames gives the eager tensor
"""
import functools

import numpy as np
import pytest

import tf_image_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
GUARD = 4096            # floats in front of and behind dst; bytes in front of and behind the frames


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], axis=-1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)          # B, G, R


@functools.lru_cache(maxsize=None)
def _expected(h, w, seed, H, W):
    return M.get_img_bgr(_frame(h, w, seed), H, W)


def _pack(frames, pad=0):
    """Frames (uint8 [h,w,3]) into one byte buffer between guards, rows `pad` bytes apart beyond their own; the pad bytes and the
    guards are 0xEE, which no test frame region relies on.  -> (uint8 array, [(offset, sh, sw, stride)])."""
    geo, off = [], GUARD
    for f in frames:
        h, w = f.shape[:2]
        stride = 3 * w + pad
        geo.append((off, h, w, stride))
        off += h * stride + 61                                       # odd gaps: no frame is aligned to anything
    buf = np.full(off + GUARD, 0xEE, np.uint8)
    for f, (o, h, w, stride) in zip(frames, geo):
        rows = buf[o:o + h * stride].reshape(h, stride)
        rows[:, :3 * w] = f.reshape(h, 3 * w)
    return buf, geo


def _run(cuda, frames, dests, N, H, W, C, pad=0):
    """dests: [(frame number, n, c)].  -> dst [N,H,W,C] as a CPU tensor, after checking the guard bands."""
    import torch
    from stabnet_amd import tf_image
    buf, geo = _pack(frames, pad)
    d_buf = torch.from_numpy(buf).to(cuda)
    big = torch.full((2 * GUARD + N * H * W * C,), SENTINEL, dtype=torch.float32, device=cuda)
    dst = big[GUARD:GUARD + N * H * W * C].view(N, H, W, C)
    tf_image.get_img(d_buf, [geo[k] + (n, c) for k, n, c in dests], dst)
    torch.cuda.synchronize()
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[-GUARD:] == SENTINEL).all()), "a guard band of dst was written"
    assert torch.equal(d_buf.cpu(), torch.from_numpy(buf)), "the frames were written"
    return dst.cpu()


def _check(dst, specs, dests, H, W, N, C):
    import torch
    named = set()
    for k, n, c in dests:
        h, w, seed = specs[k]
        assert torch.equal(dst[n, :, :, c], torch.from_numpy(_expected(h, w, seed, H, W))), (specs[k], n, c)
        named.add((n, c))
    for n in range(N):
        for c in range(C):
            if (n, c) not in named:
                assert bool((dst[n, :, :, c] == SENTINEL).all()), "channel (%d, %d) is named by no entry and was written" % (n, c)


@pytest.mark.parametrize("sh,sw,pad", [(37, 53, 0), (8, 8, 0), (16, 24, 0), (5, 1, 0), (37, 53, 13)],
                         ids=["37x53", "8x8-upscale", "16x24-same", "5x1", "37x53-strided"])
def test_sizes_bit_exact(cuda, sh, sw, pad):
    H, W = 16, 24
    specs = [(sh, sw, 3)]
    dests = [(0, 0, 0)]
    dst = _run(cuda, [_frame(*s) for s in specs], dests, 1, H, W, 1, pad)
    _check(dst, specs, dests, H, W, 1, 1)


def test_more_than_one_workgroup_and_a_ragged_last_tile(cuda):
    H, W = 33, 47                                                    # 1551 pixels: seven tiles of 256, the last one of 15
    specs = [(37, 53, 4), (50, 31, 5)]
    dests = [(0, 0, 0), (1, 0, 1), (1, 1, 2), (0, 1, 0)]
    dst = _run(cuda, [_frame(*s) for s in specs], dests, 2, H, W, 3)
    _check(dst, specs, dests, H, W, 2, 3)


def test_c14_with_mixed_sizes_a_shared_source_and_an_unnamed_channel(cuda):
    H, W, N, C = 16, 24, 2, 14
    specs = [(37, 53, 10), (8, 8, 11), (16, 24, 12), (5, 1, 13), (40, 64, 14)]
    dests = []
    for n in range(N):
        for c in range(C):
            if (n, c) == (1, 5):
                continue                                             # named by no entry: keeps the sentinel
            dests.append(((3 * n + c) % len(specs), n, c))
    dests += [(4, 0, 3), (4, 1, 3), (4, 1, 13)]                      # one source, three destinations; a later entry replaces an earlier one
    last = {(n, c): k for k, n, c in dests}
    dst = _run(cuda, [_frame(*s) for s in specs], dests, N, H, W, C, pad=7)
    _check(dst, specs, [(k, n, c) for (n, c), k in last.items()], H, W, N, C)


def test_c2(cuda):
    H, W = 16, 24
    specs = [(37, 53, 20), (8, 8, 21)]
    dests = [(0, 0, 0), (1, 0, 1), (1, 1, 0), (0, 1, 1), (0, 2, 1)]  # (2, 0) unnamed
    dst = _run(cuda, [_frame(*s) for s in specs], dests, 3, H, W, 2)
    _check(dst, specs, dests, H, W, 3, 2)


def test_entries_that_point_outside_are_not_followed(cuda):
    """The table is device memory the host cannot inspect at launch time: an entry whose frame does not lie inside the frames, or
    whose destination does not exist, is skipped by the kernel (the Python wrapper refuses such a table before it is uploaded)."""
    import torch
    from stabnet_amd import _lib, tf_image
    H, W, N, C = 16, 24, 2, 3
    f = _frame(20, 30, 30)
    buf, geo = _pack([f])
    d_all = torch.from_numpy(buf).to(cuda)
    visible = geo[0][0] + 20 * 90                                    # the frames end with the frame; the rest of d_all is slack
    d_buf = d_all[:visible]
    off, sh, sw, rs = geo[0]
    rows = [(off, sh, sw, rs, 0, 0),                                 # good
            (off + 1, sh, sw, rs, 0, 1),                             # one byte past the end
            (off, sh + 1, sw, rs, 0, 2),                             # one row too many
            (-1, sh, sw, rs, 1, 0), (off, sh, sw, 3 * sw - 1, 1, 1), (off, 0, sw, rs, 1, 2), (off, sh, 1 << 20, rs, 1, 2),
            (off, sh, sw, rs, 2, 0), (off, sh, sw, rs, 0, 3), (off, sh, sw, rs, -1, 0), (off, sh, sw, rs, 0, -1)]
    for r in rows[1:]:
        with pytest.raises(_lib.StabnetError):
            tf_image.get_img(d_buf, [r], torch.empty((N, H, W, C), device=cuda))
    big = torch.full((2 * GUARD + N * H * W * C,), SENTINEL, dtype=torch.float32, device=cuda)
    dst = big[GUARD:-GUARD].view(N, H, W, C)
    tf_image.get_img(d_buf, torch.tensor(rows, dtype=torch.int64, device=cuda), dst)
    torch.cuda.synchronize()
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[-GUARD:] == SENTINEL).all())
    out = dst.cpu()
    assert torch.equal(out[0, :, :, 0], torch.from_numpy(M.get_img_bgr(f, H, W)))
    out[0, :, :, 0] = SENTINEL
    assert bool((out == SENTINEL).all())


def test_argument_errors_return_a_status(cuda):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr
    L = _lib.lib()
    fr = torch.zeros(64, dtype=torch.uint8, device=cuda)
    tab = torch.zeros((1, 6), dtype=torch.int64, device=cuda)
    dst = torch.zeros((1, 2, 2, 1), device=cuda)
    ok = [ptr(fr), 64, ptr(tab), 1, ptr(dst), 1, 2, 2, 1, 0, 0]
    for i, v in ((0, 0), (2, 0), (4, 0), (1, 2), (3, 0), (5, 0), (5, 65536), (6, 0), (7, 65537), (8, 0), (8, 33)):
        a = list(ok)
        a[i] = v
        assert L.stabnet_tf_get_img(*a) == -1, (i, v)
        assert b"tf_get_img" in L.stabnet_last_error()
    with pytest.raises(_lib.StabnetError):
        from stabnet_amd import tf_image
        tf_image.get_img(fr.cpu(), [(0, 1, 1, 3, 0, 0)], dst)        # there is no CPU path


def test_every_rgb_triple(cuda):
    """4096 x 4096 pixels, every (r, g, b) once, resized to its own size: all 2^24 grey bytes, summed in TensorFlow's order."""
    import torch
    from stabnet_amd import tf_image
    a = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([a & 255, (a >> 8) & 255, (a >> 16) & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    want = M.get_img_bgr(bgr, 4096, 4096)
    assert np.array_equal(want, (M.grey_u8(bgr[..., ::-1]).astype(np.float32) * M.K255 - np.float32(0.5)))
    frames = torch.from_numpy(bgr).to(cuda)
    dst = torch.full((1, 4096, 4096, 1), SENTINEL, dtype=torch.float32, device=cuda)
    tf_image.get_img(frames.view(-1), [(0, 4096, 4096, 3 * 4096, 0, 0)], dst)
    torch.cuda.synchronize()
    got = dst.view(4096, 4096)
    want_d = torch.from_numpy(want).to(cuda)
    if not torch.equal(got, want_d):
        bad = (got != want_d).nonzero()
        y, x = (int(v) for v in bad[0])
        pytest.fail("%d of 2^24 triples differ; first (b, g, r) = %s: got %r, model %r"
                    % (len(bad), bgr[y, x].tolist(), float(got[y, x]), float(want_d[y, x])))


def test_graph_capture_and_two_replays(cuda):
    import torch
    from stabnet_amd import tf_image
    H, W, N, C = 16, 24, 2, 3
    specs = [(37, 53, 40), (8, 8, 41)]
    dests = [(0, 0, 0), (1, 0, 2), (0, 1, 1), (1, 1, 0)]
    variants = []
    for shift in (0, 7):
        frames = [np.roll(_frame(*s), shift, axis=1) for s in specs]
        variants.append(_pack(frames)[0])
    geo = _pack([_frame(*s) for s in specs])[1]
    table = torch.from_numpy(tf_image.make_table([geo[k] + (n, c) for k, n, c in dests], len(variants[0]), N, C)).to(cuda)
    stage = torch.zeros(len(variants[0]), dtype=torch.uint8, device=cuda)
    eager = []
    for v in variants:
        stage.copy_(torch.from_numpy(v))
        out = torch.full((N, H, W, C), SENTINEL, dtype=torch.float32, device=cuda)
        eager.append(tf_image.get_img(stage, table, out).clone())
    assert not torch.equal(eager[0], eager[1])
    dst = torch.full((N, H, W, C), SENTINEL, dtype=torch.float32, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tf_image.get_img(stage, table, dst)
    for v, e in zip(variants, eager):
        stage.copy_(torch.from_numpy(v))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, e)
