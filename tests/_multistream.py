"""Shared by tests/test_multistream_gpu.py and its child (tests/multistream_child.py; not a test module): an S-stream
StabNetStream whose device buffers lie between canary bands, random ring states that differ in every (stream, slot, pixel), and the
per-stream comparison of one step against oracle/stabnet_oracle.py (DeployRing / deploy_step, which restate deploy_bundle.py).
There is no model of csrc/ring.hip here: the ring's reference is the oracle's Python lists."""
import numpy as np
import torch

from oracle import stabnet_oracle as O

from _guarded import Guarded, _check_all, _same_bits

# the project's single-frame bars (tests/test_baseline_sizes_gpu.py)
THETA_BAR = 2e-5
MAP_BAR = 1e-4

GUARDED = ("frames_ring", "masks_ring", "frame_fb", "black", "out_img", "x_map", "y_map", "theta", "all_black")
SNAP = GUARDED + ("Hs",)


def make_params(H, W):
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    cfg, ocfg = Config(height=H, width=W), O.Config(height=H, width=W)
    return cfg, ocfg, synthetic.make_params(cfg, seed=0, theta_scale=0.2)


def guarded_stream(P, H, W, cfg, S, dev, operand_mode, refine=1, use_graph=False):
    """StabNetStream whose ring planes, outputs and all_black are views into canary-banded buffers (assigned before the first step:
    with use_graph the pointers are captured there).  -> (stream, {name: Guarded})."""
    from stabnet_amd.deploy import StabNetStream
    st = StabNetStream(P, H, W, cfg, streams=S, device=dev, refine=refine, use_graph=use_graph, operand_mode=operand_mode)
    st.track_black()
    guards = {}
    for name in GUARDED:
        t = getattr(st, name)
        g = Guarded(dev, t.numel())                        # float32 words; all_black (int32) is a view of the same bytes
        guards[name] = g
        setattr(st, name, g.t.view(t.dtype).view(t.shape))
    return st, guards


def random_state(seed, S, depth, H, W):
    """Ring content that is different for every (stream, slot, pixel), a different current frame per stream, and the preset of
    all_black."""
    rng = np.random.default_rng(seed)
    return {"frames": rng.uniform(-0.5, 0.5, (S, depth, H, W)).astype(np.float32),
            "masks": (rng.random((S, depth, H, W)) < 0.1).astype(np.float32),
            "cur": rng.uniform(-0.5, 0.5, (S, H, W)).astype(np.float32),
            "preset": rng.integers(0, 1 << 20, (S, H, W)).astype(np.int32)}


def load_state(st, state, head):
    """In place (a captured graph keeps reading the same addresses)."""
    dev = st.frames_ring.device
    st.frames_ring.copy_(torch.from_numpy(state["frames"]).to(dev))
    st.masks_ring.copy_(torch.from_numpy(state["masks"]).to(dev))
    st.head_dev[0] = head
    if st.all_black is not None:
        st.all_black.copy_(torch.from_numpy(state["preset"]).to(dev))


def snapshot(st):
    torch.cuda.synchronize()
    d = {k: getattr(st, k).cpu().numpy().copy() for k in SNAP}
    d["head"] = np.int64(st.head)
    return d


def oracle_ring(frames, masks, head, ocfg):
    """O.DeployRing holding the planes [depth][H][W] of one stream: ring.frames[-i] is slot (head - i) % depth."""
    depth, H, W = frames.shape
    ring = O.DeployRing(frames[0], ocfg)
    assert len(ring.frames) == depth
    ring.frames = [frames[(head + k) % depth].reshape(1, H, W, 1).copy() for k in range(depth)]
    ring.masks = [masks[(head + k) % depth].reshape(1, H, W, 1).copy() for k in range(depth)]
    return ring


def discontinuous(r, H, W):
    """Pixels [H][W] at which the reference's warp is discontinuous within the map bar, from the reference's own maps: the black test
    flips where a map is within MAP_BAR of +-1 (the edge zone of test_baseline_sizes_gpu.py), and the sampler -- corners clipped BEFORE
    the weights are formed -- jumps where the sample position crosses column 0 or W-1 / row 0 or H-1 (_lipschitz_pixel_check's border),
    which a map that moves by MAP_BAR crosses from MAP_BAR * W / 2 (H / 2) pixels away."""
    xm, ym = r["x_map"][0, ..., 0].astype(np.float64), r["y_map"][0, ..., 0].astype(np.float64)
    edge = (np.abs(np.abs(xm) - 1) < MAP_BAR) | (np.abs(np.abs(ym) - 1) < MAP_BAR)
    xp, yp = (xm + 1) * W / 2, (ym + 1) * H / 2
    tx, ty = 1.01 * MAP_BAR * W / 2, 1.01 * MAP_BAR * H / 2          # (1 %: float32 rounding of the position itself)
    return edge | (np.abs(xp) < tx) | (np.abs(xp - (W - 1)) < tx) | (np.abs(yp) < ty) | (np.abs(yp - (H - 1)) < ty)


def oracle_step(state, head, P, ocfg, refine, pass1_frame=None):
    """Per stream: O.deploy_step from the stream's own ring and current frame.

    refine == 2 with pass1_frame (the frame_fb [S][H][W] of a refine=1 GPU stream stepped from the identical state): deploy_step's two
    passes with the first pass's DECISIONS forced, as tests/_decisions.py does for the training step -- the second pass reads the
    oracle's own first-pass frame except at the pixels of discontinuous(), where two float32 evaluations whose maps differ by 1e-6 may
    land on different sides (a mask bit, or a clipped corner: the pixel then differs by its whole value and moves theta by ~5e-5),
    and where it reads the GPU's.  The result also carries "plain_theta", the unforced deploy_step's, for the record."""
    S, H, W = state["cur"].shape
    refs = []
    for s in range(S):
        ring = oracle_ring(state["frames"][s], state["masks"][s], head, ocfg)
        if refine == 1 or pass1_frame is None:
            refs.append(O.deploy_step(ring, state["cur"][s], P, ocfg, refine=refine)[0])
            continue
        assert refine == 2
        x = ring.stack(state["cur"][s])
        r1 = O.inference_stable_net(x, P, ocfg)
        frame = r1["output"][0, :, :, 0] + r1["black_pix"][0] * np.float32(-1)             # deploy_step / deploy_bundle.py:293
        zone = discontinuous(r1, H, W)
        x[..., -1] = np.where(zone, pass1_frame[s], frame)[None]
        r = O.inference_stable_net(x, P, ocfg)
        r["plain_theta"] = O.deploy_step(ring, state["cur"][s], P, ocfg, refine=2)[0]["theta"]
        r["forced_pixels"] = int(zone.sum())
        refs.append(r)
    return refs


def _bit_equal_pm0(got, want):
    """The bit comparison of tests/test_warp_gpu.py: the same bits, +0.0 and -0.0 being one value."""
    got = np.asarray(got, np.float32).reshape(want.shape)
    neq = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    neq &= ~((got == 0) & (want == 0))
    return int(neq.sum())


def check_numerics(got, refs, what):
    """theta / maps / black of every stream against the oracle's step from the same state, at the bars of
    test_baseline_sizes_gpu.py.  -> worst theta error over the streams."""
    worst = 0.0
    for s, ref in enumerate(refs):
        dth = float(np.abs(got["theta"][s] - ref["theta"][0]).max())
        worst = max(worst, dth)
        assert dth <= THETA_BAR, "%s stream %d: theta off the oracle by %.3e" % (what, s, dth)
        dx = float(np.abs(got["x_map"][s] - ref["x_map"][0]).max())
        dy = float(np.abs(got["y_map"][s] - ref["y_map"][0]).max())
        assert dx < MAP_BAR and dy < MAP_BAR, "%s stream %d: maps off the oracle by %.3e / %.3e" % (what, s, dx, dy)
        flips = got["black"][s] != ref["black_pix"][0]
        edge = (np.abs(np.abs(ref["x_map"][0, ..., 0]) - 1) < MAP_BAR) | (np.abs(np.abs(ref["y_map"][0, ..., 0]) - 1) < MAP_BAR)
        assert not (flips & ~edge).any(), "%s stream %d: %d black pixels differ away from the +-1 edge" % (
            what, s, int((flips & ~edge).sum()))
    return worst


def check_warp_exact(got, state, ocfg, what):
    """refine == 1: the step's Hs, maps, black and output are the oracle's get_4_pts + transformer of the stream's current frame at
    the GPU's OWN theta of that stream, bit for bit."""
    S, H, W = state["cur"].shape
    for s in range(S):
        _, pts2 = O.get_4_pts(got["theta"][s:s + 1], ocfg)
        out, black, img, Hs, _ = O.transformer(state["cur"][s].reshape(1, H, W, 1), pts2, ocfg, return_all=True)
        for name, g, w in (("Hs", got["Hs"][s], Hs[0]), ("x_map", got["x_map"][s, ..., 0], img[0, ..., 0]),
                           ("y_map", got["y_map"][s, ..., 0], img[0, ..., 1]), ("black", got["black"][s], black[0]),
                           ("output", got["out_img"][s, ..., 0], out[0, ..., 0])):
            n = _bit_equal_pm0(g, w)
            assert n == 0, "%s stream %d: %s differs from the oracle's warp at the GPU's theta in %d of %d elements" % (
                what, s, name, n, w.size)


def check_movement(got, state, head0, depth, what):
    """The feedback, exactly: frame_fb = output + black * -1 (float32), pushed with black into slot head0 of the stream's OWN ring
    planes; every other slot of every stream keeps its bits; the head advances by one, modulo the depth."""
    S = state["cur"].shape[0]
    assert int(got["head"]) == (head0 + 1) % depth, "%s: head %d after a step from %d" % (what, int(got["head"]), head0)
    fb = got["out_img"][..., 0] + got["black"] * np.float32(-1)
    assert fb.dtype == np.float32
    others = [k for k in range(depth) if k != head0]
    for s in range(S):
        assert _same_bits(got["frame_fb"][s], fb[s]), "%s stream %d: frame_fb is not output - black" % (what, s)
        assert _same_bits(got["frames_ring"][s, head0], got["frame_fb"][s]), "%s stream %d: slot %d does not hold frame_fb" % (what, s, head0)
        assert _same_bits(got["masks_ring"][s, head0], got["black"][s]), "%s stream %d: slot %d does not hold black" % (what, s, head0)
        for name in ("frames", "masks"):
            same = (got[name + "_ring"][s, others].view(np.uint32) == state[name][s, others].view(np.uint32)).all(axis=(1, 2))
            assert same.all(), "%s stream %d: %s slots %s changed" % (what, s, name, [others[i] for i in np.flatnonzero(~same)])


def check_all_black(got, state, what, pass1_black=None):
    """all_black += rint(black) once per refine pass (deploy_bundle.py:291): the final mask, plus -- refine == 2 -- the first
    pass's (the black of a refine=1 stream stepped from the identical state)."""
    want = np.rint(got["black"]).astype(np.int64)
    if pass1_black is not None:
        want = want + np.rint(pass1_black).astype(np.int64)
    inc = got["all_black"].astype(np.int64) - state["preset"].astype(np.int64)
    for s in range(want.shape[0]):
        assert np.array_equal(inc[s], want[s]), "%s stream %d: all_black grew by something else than the stream's masks at %d pixels" % (
            what, s, int((inc[s] != want[s]).sum()))


def check_step(got, state, head0, depth, P, ocfg, refine, what, pass1=None):
    """Everything test 1 of test_multistream_gpu.py asks of one step.  pass1 (refine == 2): the snapshot of a refine=1 stream stepped
    from the identical state, itself held to the oracle's single pass and to the exact warp.  -> worst theta error against the oracle
    (refine == 2: and against the unforced deploy_step)."""
    if refine == 1:
        worst = check_numerics(got, oracle_step(state, head0, P, ocfg, 1), what)
        check_warp_exact(got, state, ocfg, what)
        plain = worst
    else:
        check_numerics(pass1, oracle_step(state, head0, P, ocfg, 1), what + " (first pass)")
        check_warp_exact(pass1, state, ocfg, what + " (first pass)")
        refs = oracle_step(state, head0, P, ocfg, 2, pass1["frame_fb"])
        worst = check_numerics(got, refs, what)
        plain = max(float(np.abs(got["theta"][s] - r["plain_theta"][0]).max()) for s, r in enumerate(refs))
    check_movement(got, state, head0, depth, what)
    check_all_black(got, state, what, pass1["black"] if pass1 is not None else None)
    return worst, plain


def check_guards(guards, what):
    _check_all({"%s %s" % (what, k): g for k, g in guards.items()})
