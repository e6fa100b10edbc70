"""Census of the conv launches of the inference plan over the frame sizes deploy_bundle.py accepts (helper, not a test).

Every S_CONV step of every plan of the sweep is reduced to a SIGNATURE: what selects a code path in the kernels, and nothing else
("Census of conv routes").  Each signature keeps one EXEMPLAR -- the occurrence with the fewest multiply-adds, then the
smallest frame, then the smallest batch, operand mode and step index -- and the number of launches of the sweep that fall under it.
tools/route_census.py writes the result to tests/golden/route_census.json; test_route_census_cpu.py recomputes it and compares both
ways; test_route_census_gpu.py runs every exemplar alone against float64.

Host only: plans are host objects and stabnet_net_step_info() reads no device."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "route_census.json")

CUS = 256                      # an MI355X; the census does not read the device
IN_CH, N_THETA = 13, 50        # the shipped configuration (stabnet_amd.config.v2_93)
S_CONV = 1
RING_STAGES = 3                # conv_ring_kernel.h: "a ring of 3 stages"

SWEEP = {
    "modes": [0, 4],
    "step": 8,
    "H": [32, 1088], "W": [32, 1920],
    "batches": [1],
    "small_batches": [2, 4, 8], "small_up_to": [288, 512],
    "extra_sizes": [[45, 77], [90, 130], [270, 480], [1079, 1919], [1080, 1920]],
    "cus": CUS,
}

# the signature's fields in the order they are packed (name, bits)
SIG_FIELDS = (("kind", 10), ("splitk", 3), ("reduce", 1), ("short_last_slice", 1), ("k_steps", 4), ("ragged_m", 2), ("ragged_cout", 1),
              ("tiles", 2), ("batched", 1), ("stride", 2), ("pad", 2), ("prologue", 1), ("bias", 1), ("residual", 2), ("res_ld", 1),
              ("x_ld", 1), ("out_bn", 1), ("floor", 1), ("relu", 1), ("rowrun", 1))
FAMILY_ASTAT, FAMILY_PATCH = 6, 7


def _lib():
    from stabnet_amd import _lib as lib_mod
    return lib_mod.lib()


@functools.lru_cache(maxsize=None)
def fields():
    """Names of stabnet_net_step_info()'s fields, from the STABNET_SI_* enum of the header (the single source of the ABI)."""
    from stabnet_amd import _lib as lib_mod
    txt = open(lib_mod.HEADER_PATH).read()
    body = re.search(r"enum\s*\{\s*(STABNET_SI_KIND.*?)STABNET_SI_FIELDS", txt, flags=re.S).group(1)
    names = [n.lower() for n in re.findall(r"STABNET_SI_(\w+)", body)]
    assert len(names) == _lib().stabnet_net_step_info_fields(), (len(names), _lib().stabnet_net_step_info_fields())
    return tuple(names)


def col(name):
    return fields().index(name)


def kind_name(kind):
    return _lib().stabnet_prof_kind_name(int(kind)).decode()


class Plan:
    """An inference plan made as stabnet_amd.regressor.Regressor makes it: the tuning profile of the packed kernels while a mode-4
    plan is built, then the operand mode."""

    def __init__(self, mode, N, H, W):
        L = _lib()
        self.mode, self.N, self.H, self.W = mode, N, H, W
        self.h = C.c_void_p()
        if mode == 4:
            L.stabnet_conv_tuning_profile(1)
        try:
            rc = L.stabnet_net_create(C.byref(self.h), N, H, W, IN_CH, N_THETA, 0)
        finally:
            if mode == 4:
                L.stabnet_conv_tuning_profile(0)
        if rc != 0:
            raise RuntimeError("net_create(%d, %d, %d): %s" % (N, H, W, L.stabnet_last_error().decode()))
        if mode:
            assert L.stabnet_net_set_bf16_operands(self.h, mode) == 0
        self.num_steps = L.stabnet_net_num_steps(self.h)
        self.workspace_bytes = L.stabnet_net_workspace_bytes(self.h)

    def infos(self, cus=CUS):
        """[steps][fields] int64"""
        L = _lib()
        nf = len(fields())
        out = np.zeros((self.num_steps, nf), np.int64)
        for i in range(self.num_steps):
            rc = L.stabnet_net_step_info(self.h, i, cus, out[i].ctypes.data, nf)
            assert rc == 0, L.stabnet_last_error()
        return out

    def info(self, step, cus=CUS):
        L = _lib()
        nf = len(fields())
        out = np.zeros(nf, np.int64)
        rc = L.stabnet_net_step_info(self.h, step, cus, out.ctypes.data, nf)
        assert rc == 0, L.stabnet_last_error()
        return dict(zip(fields(), (int(v) for v in out)))

    def close(self):
        if self.h:
            _lib().stabnet_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sweep_sizes(sweep=SWEEP):
    """[(N, H, W)] of the sweep, frame-major."""
    st = sweep["step"]
    sizes = [(H, W) for H in range(sweep["H"][0], sweep["H"][1] + 1, st) for W in range(sweep["W"][0], sweep["W"][1] + 1, st)]
    sizes += [tuple(s) for s in sweep["extra_sizes"] if tuple(s) not in set(sizes)]
    out = []
    for H, W in sizes:
        batches = list(sweep["batches"])
        if H <= sweep["small_up_to"][0] and W <= sweep["small_up_to"][1]:
            batches += sweep["small_batches"]
        out += [(N, H, W) for N in batches]
    return out


def k_step_class(steps):
    """K steps of a slice, in classes that separate the 3-stage ring's fill (fewer steps than stages: 1, 2), one full ring (3), a
    steady loop of one or two steps behind it (4, 5), and from 6 on the slot the slice ends in (steps mod 3: the epilogue's scratch
    overlays the stage consumed last) -- 6, 7 and 8 stand for 6+ with remainder 0, 1, 2."""
    steps = np.asarray(steps)
    return np.where(steps < 2 * RING_STAGES, steps, 2 * RING_STAGES + steps % RING_STAGES)


def signature_columns(info):
    """info [rows][fields] of conv steps -> {signature field: int array}"""
    f = lambda name: info[:, col(name)]                                        # noqa: E731
    fam = f("family")
    patch, astat = fam == FAMILY_PATCH, fam == FAMILY_ASTAT
    ragged = np.where(patch, (f("ho") % 8 != 0) * 1 + (f("wo") % 8 != 0) * 2, np.where(astat, f("m") % 32 != 0, f("m") % 64 != 0) * 1)
    tiles, wgs = f("tiles"), f("wgs")
    merged = f("merged_off") >= 0
    same = (f("res_stride") == 1) & (f("res_h") == f("ho")) & (f("res_w") == f("wo"))
    return {
        "kind": f("prof_kind"),
        "splitk": np.minimum(f("splitk"), 4),
        "reduce": f("reduce"),
        "short_last_slice": (f("splitk") * f("steps_per_split") != f("total_steps")) * 1,
        "k_steps": k_step_class(f("steps_per_split")),
        "ragged_m": ragged,
        "ragged_cout": (f("cout") % 64 != 0) * 1,
        "tiles": np.where(tiles <= wgs, 0, np.where(tiles % np.maximum(wgs, 1) == 0, 1, 2)),
        "batched": (f("n") > 1) * 1,
        "stride": f("stride"),
        "pad": f("pad"),
        "prologue": f("prologue"),
        "bias": ((f("bias_off") >= 0) | merged) * 1,
        "residual": np.where(f("res_off") < 0, 0, np.where(same, 1, 2)),
        "res_ld": ((f("res_off") >= 0) & (f("res_ld") != f("cout"))) * 1,
        "x_ld": (f("x_ld") != f("cin")) * 1,
        "out_bn": ((f("out_bn_off") >= 0) | merged) * 1,
        "floor": merged * 1,
        "relu": f("relu_out"),
        "rowrun": f("rowrun"),
    }


def pack_signature(cols):
    key = np.zeros(len(cols["kind"]), np.int64)
    for name, bits in SIG_FIELDS:
        v = np.asarray(cols[name], np.int64)
        assert (v >= 0).all() and (v < (1 << bits)).all(), (name, int(v.min()), int(v.max()))
        key = (key << bits) | v
    return key


def unpack_signature(key):
    out = {}
    for name, bits in reversed(SIG_FIELDS):
        out[name] = int(key & ((1 << bits) - 1))
        key >>= bits
    return {name: out[name] for name, _ in SIG_FIELDS}


def check_invariants(info, ws_bytes):
    """Properties every conv step of the sweep has; info [rows][fields], ws_bytes [rows] = the plan's workspace.  Raises."""
    f = lambda name: info[:, col(name)]                                        # noqa: E731

    def need(ok, what):
        if not np.all(ok):
            bad = info[np.argmax(~ok)]
            raise AssertionError("%s: %s" % (what, dict(zip(fields(), (int(v) for v in bad)))))
    sk, sps, tot = f("splitk"), f("steps_per_split"), f("total_steps")
    need((sk >= 1) & (sk * sps >= tot) & ((sk - 1) * sps < tot), "the K slices do not cover the reduction exactly once")
    need(np.where(f("reduce") == 1, f("scratch_floats") == sk * f("m") * f("cout"), f("scratch_floats") == 0), "scratch length")
    need(f("reduce") == ((sk > 1) & (f("kg") == 1)), "a K split is reduced by a launch or inside the workgroup, never both or neither")
    need((f("scratch_off") + f("scratch_floats")) * 4 <= ws_bytes, "the slabs do not fit the plan's workspace")
    need((f("kg") == 1) | ((sk == f("kg")) & (sk * sps == tot)), "K groups with unequal slices")
    fam = f("family")
    lds = (fam == FAMILY_ASTAT) | (fam == FAMILY_PATCH)
    need(~lds | ((f("lds_bytes") > 0) & (f("lds_bytes") <= f("lds_limit"))), "planes do not fit LDS")
    need((fam != FAMILY_ASTAT) | ((f("astat_bm") * f("k") * 6 <= f("lds_limit")) & (sk == 1)), "A-stationary planes")
    need((f("family") != 0) | (f("x_ld") == f("cin")), "a strided input on the register-staged kernel")
    need((f("tiles") >= 1) & (f("wgs") >= 1) & (f("wgs") <= f("tiles")) & (f("wgs") == f("gx") * f("gy") * f("gz")), "grid")
    # a step's output range overlaps none of its input, residual or scratch ranges (all inside the workspace)
    o0, o1 = f("out_off"), f("out_off") + f("out_floats")
    need((o0 >= 0) & (o1 <= f("scratch_off")), "output outside the activation region")
    i0, i1 = f("in_base"), f("in_base") + f("in_floats")
    need((i0 <= f("in_off")) & (i1 <= f("scratch_off")), "input outside the activation region")
    need((o1 <= i0) | (i1 <= o0), "output overlaps the input")
    r0, r1 = f("res_off"), f("res_off") + f("res_floats")
    need((r0 < 0) | (((o1 <= r0) | (r1 <= o0)) & (r1 <= f("scratch_off"))), "output overlaps the residual")
    # what the kernels read stays inside the buffers: the last pixel's last channel / the strided residual's last element
    need(f("in_off") + (f("n") * f("h") * f("w") - 1) * f("x_ld") + f("cin") <= i1, "input read behind its buffer")
    last_res = ((f("n") - 1) * f("res_h") * f("res_w") + (f("ho") - 1) * f("res_stride") * f("res_w") + (f("wo") - 1) * f("res_stride")) * f("res_ld") + f("cout")
    need((r0 < 0) | (r0 + last_res <= r1), "residual read behind its buffer")


def fastdiv(n, mul, shift):
    """sn_fastdiv (conv.h) in the device's 32-bit arithmetic"""
    return (((int(mul) * int(n)) >> 32) + int(n) & 0xFFFFFFFF) >> int(shift)


def check_fastdiv(info):
    """The multiply-high constants give m / (Ho*Wo) and r / Wo exactly at m = 0, M - 1 and on both sides of every image and row
    boundary.  info: a dict (Plan.info)."""
    hw, wo, M = info["ho"] * info["wo"], info["wo"], info["m"]
    ms = {0, M - 1}
    for img in range(1, info["n"]):
        ms |= {img * hw - 1, img * hw}
    for m in sorted(ms):
        assert fastdiv(m, info["div_hw_mul"], info["div_hw_shift"]) == m // hw, ("m / (Ho*Wo)", m, hw)
    rs = {0, hw - 1}
    for row in range(1, info["ho"]):
        rs |= {row * wo - 1, row * wo}
    for r in sorted(rs):
        assert fastdiv(r, info["div_w_mul"], info["div_w_shift"]) == r // wo, ("r / Wo", r, wo)


@functools.lru_cache(maxsize=None)
def census(check=True):
    """The whole sweep -> {"sweep", "plans", "conv_launches", "signatures": [{"signature": {...}, "kernel", "exemplar": {mode, N, H, W,
    step}, "launches"}]} sorted by packed signature.  check: run check_invariants() over every conv step on the way."""
    best = {}                                              # packed signature -> [launches, exemplar key tuple]
    c_kind, c_m, c_k, c_cout = col("kind"), col("m"), col("k"), col("cout")
    plans = launches = 0
    kinds = set()
    rows, meta = [], []

    def flush():
        nonlocal launches
        if not rows:
            return
        info, m = np.concatenate(rows), np.concatenate(meta)
        rows.clear(), meta.clear()
        if check:
            check_invariants(info, m[:, 5])
        key = pack_signature(signature_columns(info))
        macs = info[:, c_m] * info[:, c_k] * info[:, c_cout]
        # exemplar order: multiply-adds, frame area, H, W, batch, mode, step
        order = np.lexsort((m[:, 4], m[:, 0], m[:, 1], m[:, 3], m[:, 2], m[:, 2] * m[:, 3], macs, key))
        key_s = key[order]
        first = np.flatnonzero(np.r_[True, key_s[1:] != key_s[:-1]])
        counts = np.diff(np.r_[first, len(key_s)])
        for k, i, n in zip(key_s[first], order[first], counts):
            cand = (int(macs[i]), int(m[i, 2] * m[i, 3]), int(m[i, 2]), int(m[i, 3]), int(m[i, 1]), int(m[i, 0]), int(m[i, 4]))
            e = best.get(int(k))
            if e is None:
                best[int(k)] = [int(n), cand]
            else:
                e[0] += int(n)
                if cand < e[1]:
                    e[1] = cand
        kinds.update(int(v) for v in np.unique(info[:, col("prof_kind")]))
        launches += len(key)

    for N, H, W in sweep_sizes():
        for mode in SWEEP["modes"]:
            p = Plan(mode, N, H, W)
            info = p.infos()
            sel = np.flatnonzero(info[:, c_kind] == S_CONV)
            if check:
                # the plan's launch count (what a captured frame is sized by) is the launches the BOUND routes make: every conv and
                # its reduce launch + pad, pool, pooled partials, fc_1, fc_2, fc_3 and the output layer (the fused head, batch <= 8)
                n_conv = int(len(sel) + info[sel, col("reduce")].sum())
                assert _lib().stabnet_net_num_launches(p.h) == n_conv + 7, (mode, N, H, W, _lib().stabnet_net_num_launches(p.h), n_conv)
            rows.append(info[sel])
            meta.append(np.column_stack([np.full(len(sel), mode), np.full(len(sel), N), np.full(len(sel), H), np.full(len(sel), W), sel,
                                         np.full(len(sel), p.workspace_bytes)]).astype(np.int64))
            p.close()
            plans += 1
        if len(rows) >= 512:
            flush()
    flush()
    names = {k: kind_name(k) for k in kinds}
    assert all(n and n != "?" for n in names.values()), "a route without a kernel name: %s" % names
    sigs = []
    for k in sorted(best):
        n, (macs, _, H, W, N, mode, step) = best[k]
        sig = unpack_signature(k)
        kernel = names[sig.pop("kind")]
        sigs.append({"kernel": kernel, "signature": sig, "exemplar": {"mode": mode, "N": N, "H": H, "W": W, "step": step},
                     "multiply_adds": macs, "launches": n})
    return {"sweep": SWEEP, "signature_fields": [n for n, _ in SIG_FIELDS], "plans": plans, "conv_launches": launches, "signatures": sigs}


def exemplar_id(e):
    x = e["exemplar"]
    return "m%d-%dx%dx%d-s%d" % (x["mode"], x["N"], x["H"], x["W"], x["step"])


ROW = "[kernel index, signature digits in the order of signature_fields (without kind), mode, N, H, W, step, launches]"


def golden_text(doc):
    """The census as committed: one short row per signature (every signature value is one digit), so the file stays small."""
    fields_ = [n for n in doc["signature_fields"] if n != "kind"]
    kernels = sorted({e["kernel"] for e in doc["signatures"]})
    rows = []
    for e in doc["signatures"]:
        assert all(0 <= e["signature"][n] <= 9 for n in fields_)
        x = e["exemplar"]
        rows.append(json.dumps([kernels.index(e["kernel"]), "".join(str(e["signature"][n]) for n in fields_), x["mode"], x["N"], x["H"],
                                x["W"], x["step"], e["launches"]], separators=(",", ":")))
    head = {k: doc[k] for k in ("sweep", "signature_fields", "plans", "conv_launches")}
    head.update(kernels=kernels, row=ROW)
    return json.dumps(head, sort_keys=True)[:-1] + ', "signatures": [\n' + ",\n".join(rows) + "\n]}\n"


def load_golden():
    """The committed census in the form census() returns (without multiply_adds)."""
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    fields_ = [n for n in doc["signature_fields"] if n != "kind"]
    sigs = []
    for k, digits, mode, N, H, W, step, launches in doc["signatures"]:
        assert len(digits) == len(fields_)
        sigs.append({"kernel": doc["kernels"][k], "signature": {n: int(d) for n, d in zip(fields_, digits)},
                     "exemplar": {"mode": mode, "N": N, "H": H, "W": W, "step": step}, "launches": launches})
    doc["signatures"] = sigs
    return doc


def reference_step(info, params, scale, shift, merged, x_buf=None, res_buf=None, frame=None):
    """ONE conv step in float64, from float32 parameters and inputs -> [N, Ho, Wo, Cout] float64.

    info: Plan.info(step).  params: the flat float32 parameter buffer (numpy).  scale / shift: the folded BN sections of `fold`
    ([bn_channels] each); merged: the [4][Cout] vectors of a merged shortcut | conv1 launch (None: not merged).  x_buf: the whole
    buffer the input lives in (IN_FLOATS floats from IN_BASE); res_buf: the whole residual buffer.  frame: [N, H, W, in_ch], the
    row-run stem's input as the caller gave it (the OHWI weights of `params`, not the row-run copy, multiply it)."""
    import torch
    i = info
    N, H, W, Cin, Ho, Wo, Cout, KH, KW = (i[k] for k in ("n", "h", "w", "cin", "ho", "wo", "cout", "kh", "kw"))
    if i["rowrun"]:
        cin_pad = (Cin + 15) // 16 * 16
        x = np.asarray(frame, np.float64).reshape(N, H, W, Cin)
        w = params[i["w_off"]:i["w_off"] + Cout * KH * KW * cin_pad].reshape(Cout, KH, KW, cin_pad)[..., :Cin].astype(np.float64)
    else:
        assert len(x_buf) == N * H * W * i["x_ld"]
        c0 = i["in_off"] - i["in_base"]
        x = x_buf.reshape(N, H, W, i["x_ld"])[..., c0:c0 + Cin].astype(np.float64)
        w = params[i["w_off"]:i["w_off"] + Cout * KH * KW * Cin].reshape(Cout, KH, KW, Cin).astype(np.float64)
    if i["prologue"]:
        c = i["pro_bn_off"]
        x = np.maximum(x * scale[c:c + Cin].astype(np.float64) + shift[c:c + Cin].astype(np.float64), 0.0)
    if KH == 1 and KW == 1 and i["pad"] == 0:
        xs = x[:, ::i["stride"], ::i["stride"]]
        y = (xs.reshape(-1, Cin) @ w.reshape(Cout, Cin).T).reshape(N, xs.shape[1], xs.shape[2], Cout)
    else:
        y = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))),
                                       torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))), stride=i["stride"], padding=i["pad"])
        y = y.permute(0, 2, 3, 1).numpy()
    assert y.shape == (N, Ho, Wo, Cout), (y.shape, (N, Ho, Wo, Cout))
    if merged is not None:
        y = y + merged[0].astype(np.float64)
    elif i["bias_off"] >= 0:
        y = y + params[i["bias_off"]:i["bias_off"] + Cout].astype(np.float64)
    if i["res_off"] >= 0:
        rs = i["res_stride"]
        r = res_buf.reshape(N, i["res_h"], i["res_w"], i["res_ld"])
        y = y + r[:, :rs * (Ho - 1) + 1:rs, :rs * (Wo - 1) + 1:rs, :Cout].astype(np.float64)
    if merged is not None:
        y = np.maximum(y * merged[1].astype(np.float64) + merged[2].astype(np.float64), merged[3].astype(np.float64))
    else:
        if i["out_bn_off"] >= 0:
            c = i["out_bn_off"]
            y = y * scale[c:c + Cout].astype(np.float64) + shift[c:c + Cout].astype(np.float64)
        if i["relu_out"]:
            y = np.maximum(y, 0.0)
    return y


def signature_of(info_row):
    """Signature dict (with the kernel name) of ONE step's info (dict, Plan.info)."""
    arr = np.array([[info_row[n] for n in fields()]], np.int64)
    sig = {k: int(v[0]) for k, v in signature_columns(arr).items()}
    kernel = kind_name(sig.pop("kind"))
    return kernel, sig
