"""The boundary search of the conv extent guard (helper, not a test): the largest batch stabnet_net_create() accepts per frame size,
operand mode and fusion.  tools/conv_extents.py writes the result to tests/golden/conv_extents.json; test_conv_extents_cpu.py recomputes
it and judges the accepted plans by the table in tests/_extents.py, which this module does not use."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_extents.json")
SIZES = [(288, 512), (720, 1280), (1080, 1920), (1079, 1919), (2160, 3840)]
TRAIN_SIZES = [(288, 512), (64, 96)]
N_MAX = 4096                                               # stabnet_net_create's own bound on the batch
# (name, operand mode, fused unit pairs, STABNET_CONV_B2B_PLAN=1 in a child process)
CONFIGS = [("mode0", 0, 0, 0), ("mode4", 4, 0, 0), ("mode4_pairs", 4, 1, 0), ("mode0_b2b", 0, 0, 1), ("mode4_b2b", 4, 0, 1)]


def is_extent_refusal(msg):
    """stabnet_net_create's extent wording: "net_create: N=.. H=.. W=..: the <operand> of <layer> (plan step k) spans n floats; every conv
    operand must stay below 2^30 floats ..." """
    return ("net_create: N=" in msg and "spans" in msg and "every conv operand must stay below 2^30 floats" in msg
            and any(" the %s of resnet_v2_50/" % op in msg for op in ("input", "output", "residual", "weights")))


def make_plan(mode, N, H, W, pairs=0):
    """(plan, None) or (None, the refusal's message)."""
    import _route_census as rc
    try:
        p = rc.Plan(mode, N, H, W)
    except RuntimeError as e:
        if not is_extent_refusal(str(e)):
            raise                                          # anything else (no library, a bad shape) is no refusal of an extent
        return None, str(e)
    if pairs:
        assert rc._lib().stabnet_net_fuse_unit_pairs(p.h, 1) == 0
        p.num_steps = rc._lib().stabnet_net_num_steps(p.h)
    return p, None


def accepts_training(N, H, W):
    import _route_census as rc
    L, h = rc._lib(), C.c_void_p()
    rc_ = L.stabnet_net_create(C.byref(h), N, H, W, rc.IN_CH, rc.N_THETA, 1)
    if rc_ == 0:
        L.stabnet_net_destroy(h)
        return True, None
    msg = L.stabnet_last_error().decode()
    assert is_extent_refusal(msg) or N > N_MAX, msg
    return False, msg


def bisect_boundary(accepts):
    """Largest N in [1, N_MAX] that accepts(N) takes (acceptance is monotone in N: every extent grows with it)."""
    assert accepts(1)
    if accepts(N_MAX):
        return N_MAX
    lo, hi = 1, N_MAX                                      # accepts(lo), not accepts(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepts(mid):
            lo = mid
        else:
            hi = mid
    return lo


def boundary(mode, H, W, pairs=0):
    def accepts(N):
        p, _ = make_plan(mode, N, H, W, pairs)
        if p is not None:
            p.close()
        return p is not None
    return bisect_boundary(accepts)


def step_kinds(plan):
    import _route_census as rc
    return [int(v) for v in plan.infos()[:, rc.col("kind")]]


def b2b_child(mode):
    """In a process started with STABNET_CONV_B2B_PLAN=1 (the switch is read once per process): {"HxW": {"N": boundary, "kinds": {N:
    step kinds of the plan at N and N // 2}}}."""
    out = {}
    for H, W in SIZES:
        N = boundary(mode, H, W)
        kinds = {}
        for n in sorted({N, max(1, N // 2)}):
            p, _ = make_plan(mode, n, H, W)
            kinds[str(n)] = step_kinds(p)
            p.close()
        _, msg = make_plan(mode, N + 1, H, W)
        out["%dx%d" % (H, W)] = {"N": N, "kinds": kinds, "refusal": msg}
    return out


def run_b2b_child(mode):
    env = dict(os.environ, STABNET_CONV_B2B_PLAN="1")
    root = os.path.dirname(HERE)
    code = "import sys, json; sys.path[:0] = [%r, %r]; import _extents_search; print('RESULT ' + json.dumps(_extents_search.b2b_child(%d)))" % (root, HERE, mode)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def boundaries():
    """The record: {"inference": {"HxW": {config: N}}, "training": {"HxW": N}}."""
    inf = {"%dx%d" % s: {} for s in SIZES}
    for name, mode, pairs, b2b in CONFIGS:
        if b2b:
            for key, v in run_b2b_child(mode).items():
                inf[key][name] = v["N"]
        else:
            for H, W in SIZES:
                inf["%dx%d" % (H, W)][name] = boundary(mode, H, W, pairs)
    trn = {"%dx%d" % (H, W): bisect_boundary(lambda N, H=H, W=W: accepts_training(N, H, W)[0]) for H, W in TRAIN_SIZES}
    return {"limit_floats": 1 << 30, "n_max": N_MAX, "inference": inf, "training": trn}


def golden_text(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"
