"""Everything a caller can see of an inference plan without a device, over the plan variants (helper, not a test).

For each frame size of SIZES, operand modes 0-4 and the variants
  default     the plan as stabnet_net_create + stabnet_net_set_bf16_operands leave it,
  pairs       ... then stabnet_net_fuse_unit_pairs(1) (mode 4 only: a no-op elsewhere),
  b2b         STABNET_CONV_B2B_PLAN=1 with STABNET_CONV_B2B_MIN_TILES=1 (all five modes),
  b2b+pairs   ... then stabnet_net_fuse_unit_pairs(1) (mode 4),
the record holds num_steps, num_launches, deploy_frame_launches(4, 4), workspace_bytes, fold_floats and the whole
stabnet_net_step_info matrix at 256 CUs; a training plan (keep_activations = 1) of each size adds its step count and workspace.
The file keeps the matrix without repetition (pack() below).
The B2B switches are read once per process, so those variants come from a child process (`python tests/_plan_views.py child`).
`python tests/_plan_views.py record <commit>` writes tests/golden/plan_views.json, stamped with the commit it was recorded at."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _route_census as RC  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "plan_views.json")
SIZES = [(1, 96, 160), (2, 72, 136), (1, 288, 512), (1, 360, 640), (1, 720, 1280), (1, 1080, 1920)]
MODES = [0, 1, 2, 3, 4]
B2B_ENV = {"STABNET_CONV_B2B_PLAN": "1", "STABNET_CONV_B2B_MIN_TILES": "1"}


def key(size, mode, variant):
    return "%dx%dx%d/mode%d/%s" % (size + (mode, variant))


def view(plan):
    """The host-visible numbers of `plan` as it stands; "info" = [steps][fields] ints."""
    L = RC._lib()
    plan.num_steps = L.stabnet_net_num_steps(plan.h)
    return {"num_steps": int(plan.num_steps), "num_launches": int(L.stabnet_net_num_launches(plan.h)),
            "deploy_frame_launches": int(L.stabnet_deploy_frame_launches(plan.h, 4, 4)),
            "workspace_bytes": int(L.stabnet_net_workspace_bytes(plan.h)), "fold_floats": int(L.stabnet_net_fold_floats(plan.h)),
            "info": plan.infos().tolist()}


def views(b2b):
    """{key: view} of this process's variants: default / pairs, or with the B2B switches in the environment b2b / b2b+pairs."""
    L = RC._lib()
    name, name_pairs = ("b2b", "b2b+pairs") if b2b else ("default", "pairs")
    out = {}
    for size in SIZES:
        for mode in MODES:
            plan = RC.Plan(mode, *size)
            out[key(size, mode, name)] = view(plan)
            if mode == 4:
                assert L.stabnet_net_fuse_unit_pairs(plan.h, 1) == 0
                out[key(size, mode, name_pairs)] = view(plan)
            plan.close()
        if not b2b:            # a training plan (keep_activations = 1) has no step_info: its steps and workspace alone.  (Not its
            # num_launches: at the recorded commit that was the plan-time view, which took conv2 / conv3 of such a plan to carry the
            # prologue they do not run with.  tests/test_regressor_gpu.py compares the count with the Profiler's records.)
            h = C.c_void_p()
            assert L.stabnet_net_create(C.byref(h), *size, RC.IN_CH, RC.N_THETA, 1) == 0
            out["%dx%dx%d/train" % size] = {"num_steps": int(L.stabnet_net_num_steps(h)), "workspace_bytes": int(L.stabnet_net_workspace_bytes(h)),
                                            "info": []}
            L.stabnet_net_destroy(h)
    return out


def child_views():
    """The B2B variants, from a fresh process that reads the switches."""
    env = dict(os.environ, PYTHONPATH=ROOT, **B2B_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


# step_info fields that open a group of the golden file: geometry | workspace | params and fold | K split | route | grid | index math, LDS
GROUP_STARTS = ("kind", "in_off", "w_off", "splitk", "family", "tiles", "div_hw_mul")


def _groups():
    cuts = [RC.col(n) for n in GROUP_STARTS] + [len(RC.fields())]
    return [slice(a, b) for a, b in zip(cuts, cuts[1:])]


def pack(all_views, commit):
    """The golden file's form, lossless: a step_info row is cut into the field groups above and each group's distinct value tuples are
    kept once ("tables"); a distinct row is its tuple of table indices ("rows"); a plan lists row indices ("steps")."""
    tables, rows, plans = [{} for _ in GROUP_STARTS], {}, {}
    for k in sorted(all_views):
        v = dict(all_views[k])
        v["steps"] = [rows.setdefault(tuple(t.setdefault(tuple(r[g]), len(t)) for t, g in zip(tables, _groups())), len(rows)) for r in v.pop("info")]
        plans[k] = v
    return {"commit": commit, "cus": RC.CUS, "fields": list(RC.fields()), "group_starts": list(GROUP_STARTS),
            "tables": [[list(r) for r in t] for t in tables], "rows": [list(r) for r in rows], "plans": plans}


def unpack(golden):
    assert golden["group_starts"] == list(GROUP_STARTS)
    full = [sum((t[i] for t, i in zip(golden["tables"], r)), []) for r in golden["rows"]]
    return {k: dict({f: v[f] for f in v if f != "steps"}, info=[full[i] for i in v["steps"]]) for k, v in golden["plans"].items()}


def dump(golden, path):
    """One line per table, one for the rows, one per plan."""
    enc = lambda o: json.dumps(o, separators=(",", ":"))                        # noqa: E731
    head = {k: golden[k] for k in ("commit", "cus", "fields", "group_starts")}
    with open(path, "w") as f:
        f.write(enc(head)[:-1] + ',\n"tables":[\n' + ",\n".join(enc(t) for t in golden["tables"]) + '],\n"rows":' + enc(golden["rows"]) + ',\n"plans":{\n')
        f.write(",\n".join("%s:%s" % (enc(k), enc(v)) for k, v in golden["plans"].items()) + "}}\n")


if __name__ == "__main__":
    if sys.argv[1] == "child":
        json.dump(views(True), sys.stdout)
    elif sys.argv[1] == "record":
        both = dict(views(False), **child_views())
        dump(pack(both, sys.argv[2]), GOLDEN)
        print("%d plans, %d bytes" % (len(both), os.path.getsize(GOLDEN)))
