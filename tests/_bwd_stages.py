"""The staged backward's bucket contract, checked on snapshots of the ONE gradient buffer (shared by tests/test_bwd_stages_gpu.py and
its child tests/bwd_stages_child.py; not a test module).  run_case() does everything for one (N, H, W, T, operand mode) and raises
AssertionError with the offending tensor's name; the rules and their reasoning are in the docstring of test_bwd_stages_gpu.py."""
import ctypes
import time

import numpy as np
import torch

from _guarded import Guarded

EPS32 = 2.0 ** -23
STEM_W = "resnet_v2_50/conv1/weights"
KIND_W, KIND_B, KIND_GAMMA, KIND_BETA, KIND_FC_W, KIND_FC_B = 0, 1, 2, 3, 6, 7


def tensor_size(kind, dims):
    return int(np.prod([d for d in dims if d > 0]))


def read_ranges(plan):
    """([(lo, hi)] of the stage buckets, (lo, hi) of the BN gamma / beta range) as the library reports them."""
    from stabnet_amd import _lib
    lo, hi = ctypes.c_long(), ctypes.c_long()
    buckets = []
    for k in range(_lib.lib().stabnet_net_num_grad_stages()):
        _lib.call("stabnet_net_grad_bucket", plan.handle, k, ctypes.byref(lo), ctypes.byref(hi))
        buckets.append((lo.value, hi.value))
    _lib.call("stabnet_net_bn_grad_range", plan.handle, ctypes.byref(lo), ctypes.byref(hi))
    return buckets, (lo.value, hi.value)


def _where(plan, idx):
    for name, off, kind, dims, aux in plan.table:
        if off <= idx < off + tensor_size(kind, dims):
            return "%s[%d]" % (name, idx - off)
    return "float %d (no tensor: layout padding)" % idx


def _first(mask):
    return int(torch.nonzero(mask)[0])


class Case:
    def __init__(self, dev, N, H, W, T, split=False):
        from stabnet_amd import _lib, synthetic
        from stabnet_amd._tensor import stream_ptr
        from stabnet_amd.config import Config
        from stabnet_amd.regressor import NetPlan
        self.dev, self.N, self.T = dev, N, T
        self.cfg = cfg = Config(height=H, width=W, batch_size=N)
        self.plan = plan = NetPlan(N, H, W, cfg, keep_activations=True)
        if split:
            _lib.call("stabnet_net_set_bf16_operands", plan.handle, 4)
        self.nt = nt = plan.n_trainable
        self.trainables = [(n, o, k, d, a) for n, o, k, d, a in plan.table if o < nt]
        self.buckets, self.bn = read_ranges(plan)
        self.params = torch.from_numpy(plan.pack(synthetic.make_params(cfg, seed=0, theta_scale=0.3))).to(dev)
        rng = np.random.default_rng(3)
        self.xs = [torch.from_numpy(rng.uniform(-0.5, 0.5, (N, H, W, cfg.in_ch)).astype(np.float32)).to(dev) for _ in range(T)]
        self.dth = [torch.from_numpy(rng.standard_normal((N, cfg.n_theta)).astype(np.float32)).to(dev) for _ in range(T)]
        self.nb = _lib.lib().stabnet_net_train_workspace_bytes(plan.handle)
        self.ws = [Guarded(dev, self.nb, dtype=torch.uint8) for _ in range(T)]         # exactly the queried size, 0xEE inside
        self.th = [torch.empty((N, cfg.n_theta), dtype=torch.float32, device=dev) for _ in range(T)]
        self.grads = Guarded(dev, nt, init="canary")
        self.st = stream_ptr(dev)
        # the stem's pad channels (OHWI, Cin padded to in_ch_pad): from the table's dims, never from a snapshot
        name, off, kind, dims, aux = next(e for e in plan.table if e[0] == STEM_W)
        assert kind == KIND_W and dims[3] > aux == cfg.in_ch, (dims, aux)
        self.stem_off, self.stem_n = off, tensor_size(kind, dims)
        self.stem_pad = (torch.arange(self.stem_n, device=dev) % dims[3]) >= aux

    # ---------------------------------------------------------------------------------------------------------
    def forward(self):
        from stabnet_amd import _lib
        from stabnet_amd._tensor import ptr
        p, cfg = self.plan.handle, self.cfg
        if self.T == 2:
            _lib.call("stabnet_towers_fwd_train", p, ptr(self.params), ptr(self.xs[0]), ptr(self.xs[1]), ptr(self.th[0]), ptr(self.th[1]),
                      ptr(self.ws[0].t), ptr(self.ws[1].t), self.nb, cfg.bn_eps, cfg.bn_decay, self.st, 0, device=self.dev)
        else:
            _lib.call("stabnet_tower_fwd_train", p, ptr(self.params), ptr(self.xs[0]), ptr(self.th[0]), ptr(self.ws[0].t), self.nb,
                      cfg.bn_eps, cfg.bn_decay, self.st, 0, device=self.dev)
        torch.cuda.synchronize()

    def _bits(self):
        return self.grads.t.view(torch.int32).clone()

    def staged(self, base=None, dth=None):
        """Stages 0..3 one call at a time into `base` (None: zeros); the buffer's bits before and after each call: [S_-1, S_0 .. S_3]."""
        from stabnet_amd import _lib
        from stabnet_amd._tensor import ptr
        dth = self.dth if dth is None else dth
        if base is None:
            self.grads.t.zero_()
        else:
            self.grads.t.copy_(base)
        torch.cuda.synchronize()
        snaps = [self._bits()]
        for stage in range(len(self.buckets)):
            if self.T == 2:
                _lib.call("stabnet_towers_bwd_stage", self.plan.handle, ptr(self.params), ptr(dth[0]), ptr(dth[1]), ptr(self.grads.t),
                          ptr(self.ws[0].t), ptr(self.ws[1].t), self.nb, stage, self.st, 0, device=self.dev)
            else:
                _lib.call("stabnet_tower_bwd_stage", self.plan.handle, ptr(self.params), ptr(dth[0]), ptr(self.grads.t), ptr(self.ws[0].t),
                          self.nb, stage, self.st, 0, device=self.dev)
            torch.cuda.synchronize()
            snaps.append(self._bits())
        return snaps

    def one_shot(self):
        from stabnet_amd import _lib
        from stabnet_amd._tensor import ptr
        assert self.T == 1
        self.grads.t.zero_()
        _lib.call("stabnet_tower_bwd", self.plan.handle, ptr(self.params), ptr(self.dth[0]), ptr(self.grads.t), ptr(self.ws[0].t), self.nb,
                  self.st, 0, device=self.dev)
        torch.cuda.synchronize()
        return self._bits()

    # ---------------------------------------------------------------------------------------------------------
    def check_snapshots(self, S, what, log):
        """Rules 1-4 on one staged run."""
        plan, (bn_lo, bn_hi) = self.plan, self.bn
        final = S[-1]
        n_bn = bn_hi - bn_lo
        for k, (lo, hi) in enumerate(self.buckets):
            before, after = S[k], S[k + 1]
            # 1. final: what stage k leaves in its bucket is what the whole backward leaves there
            late = after[lo:hi] != final[lo:hi]
            assert not bool(late.any()), "%s: bucket %d changed after stage %d returned, first at %s" % (
                what, k, k, _where(plan, lo + _first(late)))
            # 2. isolation: stage k writes inside its bucket and the BN range only
            diff = after != before
            for a, b in ((0, lo), (hi, bn_lo), (bn_hi, self.nt)):
                if b > a and bool(diff[a:b].any()):
                    i = a + _first(diff[a:b])
                    owner = next((j for j, (x, y) in enumerate(self.buckets) if x <= i < y), None)
                    raise AssertionError("%s: stage %d wrote outside its bucket [%d, %d) and the BN range: %s, in bucket %s" % (
                        what, k, lo, hi, _where(plan, i), owner))
            # 3. the BN range: reported, not asserted per stage (the header promises it final after the last stage only)
            d = diff[bn_lo:bn_hi]
            idx = torch.nonzero(d).flatten()
            log("  %s stage %d: %d of %d floats of its bucket changed; BN range: %d of %d changed%s" % (
                what, k, int(diff[lo:hi].sum()), hi - lo, idx.numel(), n_bn,
                ", first %s last %s" % (_where(plan, bn_lo + int(idx[0])), _where(plan, bn_lo + int(idx[-1]))) if idx.numel() else ""))
            # 4. not vacuous: every weight and bias tensor of the bucket received its gradient in this stage
            seen = 0
            for name, off, kind, dims, aux in self.trainables:
                if kind not in (KIND_W, KIND_B, KIND_FC_W, KIND_FC_B) or not lo <= off < hi:
                    continue
                n = tensor_size(kind, dims)
                assert off + n <= hi, (name, off, n, hi)
                ch = diff[off:off + n]
                if name == STEM_W:
                    assert not bool(ch[self.stem_pad].any()), "%s: the stem's pad channels were written" % what
                    ch = ch[~self.stem_pad]
                assert bool(ch.any()), "%s: stage %d left %s as it was (its gradient never arrived)" % (what, k, name)
                seen += 1
            assert seen > 0, (what, k)
        # every BN gamma / beta tensor moved at some stage (rule 4's counterpart for the range every stage shares)
        moved = S[-1] != S[0]
        for name, off, kind, dims, aux in self.trainables:
            if kind in (KIND_GAMMA, KIND_BETA):
                assert bn_lo <= off and off + dims[0] <= bn_hi, name
                assert bool(moved[off:off + dims[0]].any()), "%s: %s never received a gradient" % (what, name)

    def tensor_scaled_base(self, Z, seed=11):
        """A random base with each tensor's own gradient magnitude (RMS of the zero-base gradient over the tensor)."""
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(seed)
        G0 = torch.randn(self.nt, generator=gen, device=self.dev, dtype=torch.float32)
        scale = torch.zeros(self.nt, dtype=torch.float32, device=self.dev)
        for name, off, kind, dims, aux in self.trainables:
            n = tensor_size(kind, dims)
            rms = Z[off:off + n].double().pow(2).mean().sqrt()
            assert float(rms) > 0.0, name
            scale[off:off + n] = rms.float()
        return G0 * scale

    def guards(self):
        torch.cuda.synchronize()
        self.grads.check("grads")
        for t, w in enumerate(self.ws):
            w.check("workspace %d" % t)


def run_case(dev, N, H, W, T, split=False, log=print):
    t0 = time.perf_counter()
    c = Case(dev, N, H, W, T, split)
    what = "%dx%dx%d T=%d%s" % (N, H, W, T, " split" if split else "")
    c.forward()
    S = c.staged()
    c.check_snapshots(S, what + " zero base", log)
    Z = S[-1].view(torch.float32)
    assert bool(torch.isfinite(Z).all()), what
    if T == 1:
        # 5. staged = one shot, and the BN range after stage 3 is the one-shot backward's
        one = c.one_shot()
        bad = one != S[-1]
        assert not bool(bad.any()), "%s: four stage calls differ from stabnet_tower_bwd, first at %s" % (what, _where(c.plan, _first(bad)))
        parts = Z.double().abs()
    else:
        # per-tower partial sums: the same stages with the other tower's d_theta zero (its whole backward is then exactly zero)
        zero = torch.zeros_like(c.dth[0])
        a1 = c.staged(dth=[c.dth[0], zero])[-1].view(torch.float32).double().abs()
        a2 = c.staged(dth=[zero, c.dth[1]])[-1].view(torch.float32).double().abs()
        parts = torch.maximum(Z.double().abs(), a1 + a2)
        del a1, a2
    # 6. accumulation into a nonzero base
    G0 = c.tensor_scaled_base(Z)
    SA = c.staged(base=G0)
    c.check_snapshots(SA, what + " base G0", log)
    R = SA[-1].view(torch.float32)
    assert bool(torch.isfinite(R).all()), what
    err =(R.double() - G0.double() - Z.double()).abs()
    bound = EPS32 * (G0.double().abs() + 2.0 * parts)
    over = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    log("MEASURED %s: accumulation error / bound, worst element %.3f" % (what, worst))
    assert not bool(over.any()), "%s: (result - G0) is off the zero-base gradient by %.3g x the rounding bound at %s" % (
        what, worst, _where(c.plan, _first(over)))
    # 7. guards
    c.guards()
    dt = time.perf_counter() - t0
    log("MEASURED %s: %.2f s, workspace %d bytes" % (what, dt, c.nb))
    return {"seconds": dt, "workspace_bytes": c.nb, "worst": worst}
