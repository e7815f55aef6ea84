#!/usr/bin/env python3
"""What the contact report costs per step, and what it replaces.  Two resident worlds under TGS_Soft 8/4 -- the standing base-N pyramid
(every contact touching, nothing begins or ends) and wreck_world at base N (tests/world_chain.py: balls ploughing through the pile,
contacts created and destroyed all the time, the whole loop per step as tools/churn_bench.py runs it) -- `--steps` steps after `--warmup`:

    off        no report flag: s2amd_world_step as it always was
    touch      S2AMD_REPORT_TOUCH      + s2amd_world_touch_events every step
    contacts   S2AMD_REPORT_CONTACTS   + s2amd_world_touching every step
    sums       S2AMD_REPORT_BODY_SUMS  + s2amd_world_body_sums every step
    all        all three flags and all three getters
    download   no report flag, and every step the s2amd_world_download of contacts, pairs, bodies and origins that a caller needs
               today for the same information

The joint report (s2amd_world_set_joint_report) is measured the same way on a jointed world with shapes -- world `jointed`: the
--grid x --grid lattice of synthetic.joint_grid (every third joint limited to +-0.1 rad so that limits come and go), one small box
per body that collides with nothing -- in the modes of --joint-modes:

    off        no joint-report flag
    states     S2AMD_JOINT_REPORT_STATES    + s2amd_world_joint_states every step
    limits     S2AMD_JOINT_REPORT_LIMITS    + s2amd_world_joint_limit_events every step
    sums       S2AMD_JOINT_REPORT_BODY_SUMS + s2amd_world_body_joint_sums every step
    all        all three flags, their getters and s2amd_world_joint_summary
    download   no flag, and every step the s2amd_world_download of joints, bodies and origins the report replaces

The shape report (s2amd_world_set_shape_report, s2amd_world_set_shape_view) is measured the same way on the standing base-N pyramid --
world `shaped`: 20,101 shapes at base 200 -- once with a view that holds about a tenth of the shapes (the middle tenth of their centres
along x, every y) and once with none, in the modes of --shape-modes:

    off            no shape-report flag
    draw           S2AMD_SHAPE_REPORT_DRAW   + s2amd_world_shape_draws every step
    view           S2AMD_SHAPE_REPORT_VIEW   + s2amd_world_shape_view_events every step
    bounds         S2AMD_SHAPE_REPORT_BOUNDS + s2amd_world_shape_summary every step
    all            all three flags and all three getters
    download       no flag, and every step the s2amd_world_download of shapes, bodies and origins the report replaces
    download_step  no flag, and every step s2amd_world_download_step: poses only, transforms and culling left to the host

The body report (s2amd_world_set_body_report) is measured the same way -- world `bodies`: the standing base-N pyramid (20,100 bodies at
base 200, all of them one island) and 512 pyramids of base 40 (420,352 bodies, 512 islands) -- in the modes of --body-modes:

    off        no body-report flag
    states     S2AMD_BODY_REPORT_STATES  + s2amd_world_body_states every step
    moved      ... with S2AMD_BODY_REPORT_MOVED_ONLY
    rest       S2AMD_BODY_REPORT_REST    + s2amd_world_body_rest_events every step
    islands    S2AMD_BODY_REPORT_ISLANDS + s2amd_world_islands every step
    all        STATES, REST and ISLANDS, their getters and s2amd_world_body_summary
    download   no flag, and every step what the report replaces: the s2amd_world_download of bodies, origins, contacts and joints, then
               islands.find_islands on the host

The step metrics (s2amd_world_set_metrics) are measured the same way on the standing base-N pyramid -- world `metrics` -- in the modes of
--metrics-modes:

    off        no metrics flag
    contacts   S2AMD_METRICS_CONTACTS + s2amd_world_metrics every step
    bodies     S2AMD_METRICS_BODIES   + s2amd_world_metrics every step
    joints     S2AMD_METRICS_JOINTS   + s2amd_world_metrics every step
    all        all three flags + s2amd_world_metrics every step
    history    all three flags, a ring of --steps records, no getter in the loop and ONE s2amd_world_metrics_history behind the last step
               (its time is `history_fetch_ms` and part of `total_ms`; `all` is the same run with one getter per step)
    download   no flag, and every step what the record replaces: the s2amd_world_download of bodies, origins, contacts, pairs and
               joints, then the numpy statement tests/step_metrics_ref.py on the host

One JSON object per line and mode.  All read-backs land in buffers allocated once, through the raw C calls.

    python tools/contact_report_bench.py --tree . --label this [--rep N] [--modes off,all,download] [--base 200]
                                         [--worlds pyramid,wreck,jointed,shaped,bodies] [--joint-modes off,all,download] [--grid 64]
                                         [--shape-modes off,all,download,download_step] [--body-modes off,all,download]
                                         [--worlds metrics --metrics-modes off,all,history,download]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built; a tree without the report API can run `off` and `download`).  Run two trees alternately, several repeats each, in ONE
session, so that the run-to-run spread is known before a difference is read (profiles/contact_report.jsonl)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=".")
ap.add_argument("--label", default="this")
ap.add_argument("--rep", type=int, default=0)
ap.add_argument("--modes", default="off,touch,contacts,sums,all,download")
ap.add_argument("--worlds", default="pyramid,wreck,jointed")
ap.add_argument("--joint-modes", default="off,states,limits,sums,all,download")
ap.add_argument("--shape-modes", default="off,draw,view,bounds,all,download,download_step")
ap.add_argument("--body-modes", default="off,states,moved,rest,islands,all,download")
ap.add_argument("--metrics-modes", default="off,contacts,bodies,joints,all,history,download")
ap.add_argument("--grid", type=int, default=64)
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=60)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
FLAGS = {"off": 0, "download": 0, "touch": 1, "contacts": 2, "sums": 4, "all": 7}
JOINT_FLAGS = {"off": 0, "download": 0, "states": 1, "limits": 2, "sums": 4, "all": 7}
SHAPE_FLAGS = {"off": 0, "download": 0, "download_step": 0, "draw": 1, "view": 2, "bounds": 4, "all": 7}
BODY_FLAGS = {"off": 0, "download": 0, "states": 1, "moved": 9, "rest": 2, "islands": 4, "all": 7}
METRICS_FLAGS = {"off": 0, "download": 0, "contacts": 1, "bodies": 2, "joints": 4, "all": 7, "history": 7}
SOLVER = "TGS_Soft"


def create_contacts(world, free, new_pairs):
    """The caller's s2CreateContact on its own copy of the pool (tools/churn_bench.py)."""
    n = len(new_pairs)
    slots = np.array([free.pop() for _ in range(n)], dtype=np.int32)
    contacts = np.zeros(n, dtype=wire.contact_dtype)
    pairs = np.zeros(n, dtype=wire.pair_state_dtype)
    contacts["bodyA"] = world["shapes"]["body"][new_pairs[:, 0]]
    contacts["bodyB"] = world["shapes"]["body"][new_pairs[:, 1]]
    contacts["friction"] = 0.6
    contacts["constraintIndex"] = -1
    pairs["shapeA"], pairs["shapeB"] = new_pairs[:, 0], new_pairs[:, 1]
    return slots, contacts, pairs


def run(world, mode, loop):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, nc = len(world["bodies"]), len(world["contacts"])
    free = sorted(np.flatnonzero(world["pairs"]["shapeA"] < 0).tolist(), reverse=True)
    flags = FLAGS[mode]
    ms, touching, began, ended = [], 0, 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if flags:
            s.world_set_report(flags)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if flags:
            b_buf, e_buf = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32)
            t_buf = np.zeros(nc, dtype=wire.touching_contact_dtype)
            s_buf = np.zeros(nb, dtype=wire.body_contact_sum_dtype)
        if mode == "download":
            d_bodies, d_contacts, d_pairs = np.zeros(nb, dtype=wire.body_dtype), np.zeros(nc, dtype=wire.contact_dtype), np.zeros(nc, dtype=wire.pair_state_dtype)
            d_origins = np.zeros((nb, 2), dtype=np.float32)
        n1, n2 = ctypes.c_int32(), ctypes.c_int32()
        moved = 1 if loop else 0
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            if loop and moved > 0:
                new = s.world_find_pairs()
                if len(new):
                    s.world_set_contacts(*create_contacts(world, free, new))
            info = s.world_step(params)
            if loop and info["separatedCount"] > 0:
                free.extend(s.world_separated(info["separatedCount"]).tolist())
            moved = info["movedCount"]
            if flags & 1:
                s._ck(L.s2amd_world_touch_events(h, wire.as_ptr(b_buf), nc, ctypes.byref(n1), wire.as_ptr(e_buf), nc, ctypes.byref(n2)))
                began, ended = began + n1.value, ended + n2.value
            if flags & 2:
                s._ck(L.s2amd_world_touching(h, wire.as_ptr(t_buf), nc, ctypes.byref(n1)))
                touching = n1.value
            if flags & 4:
                s._ck(L.s2amd_world_body_sums(h, wire.as_ptr(s_buf), nb))
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, wire.as_ptr(d_contacts), nc, None, 0, None, 0, wire.as_ptr(d_pairs), wire.as_ptr(d_origins), None))
                touching = int(((d_contacts["pointCount"] > 0) & (d_pairs["shapeA"] >= 0)).sum()) if step == a.warmup + a.steps - 1 else touching
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        active = info["activeContacts"]
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "active_contacts_last": active, "touching_last": touching, "began_total": began, "ended_total": ended, "bodies": nb, "contact_slots": nc}


def jointed_world(grid):
    bodies, _, joints = synthetic.joint_grid(grid)
    limited = np.arange(len(joints)) % 3 == 0
    joints["enableLimit"][limited], joints["lowerAngle"][limited], joints["upperAngle"][limited] = 1, -0.1, 0.1
    shapes = np.zeros(len(bodies), dtype=wire.shape_dtype)
    for i, b in enumerate(bodies):
        synthetic._box_shape(shapes[i], i, b["type"], 0.125, 0.125, b["position"][0], b["position"][1], i)
    shapes["maskBits"] = 0
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": shapes, "pairs": pairs,
            "origins": np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()}


def run_joints(world, mode):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, nj = len(world["bodies"]), len(world["joints"])
    flags = JOINT_FLAGS[mode]
    ms, live, began, ended = [], 0, 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if flags:
            s.world_set_joint_report(flags)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if flags:
            b_buf, e_buf = np.zeros(2 * nj, dtype=np.int32), np.zeros(2 * nj, dtype=np.int32)
            j_buf = np.zeros(nj, dtype=wire.joint_state_dtype)
            s_buf = np.zeros(nb, dtype=wire.body_joint_sum_dtype)
            m_buf = np.zeros(1, dtype=wire.joint_summary_dtype)
        if mode == "download":
            d_bodies, d_joints, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(nj, dtype=wire.joint_dtype), np.zeros((nb, 2), dtype=np.float32)
        n1, n2 = ctypes.c_int32(), ctypes.c_int32()
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if flags & 1:
                s._ck(L.s2amd_world_joint_states(h, wire.as_ptr(j_buf), nj, ctypes.byref(n1)))
                live = n1.value
            if flags & 2:
                s._ck(L.s2amd_world_joint_limit_events(h, wire.as_ptr(b_buf), 2 * nj, ctypes.byref(n1), wire.as_ptr(e_buf), 2 * nj, ctypes.byref(n2)))
                began, ended = began + n1.value, ended + n2.value
            if flags & 4:
                s._ck(L.s2amd_world_body_joint_sums(h, wire.as_ptr(s_buf), nb))
            if flags == 7:
                s._ck(L.s2amd_world_joint_summary(h, wire.as_ptr(m_buf)))
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, wire.as_ptr(d_joints), nj, None, 0, None, wire.as_ptr(d_origins), None))
                live = int((d_joints["type"] != wire.JOINT_FREE).sum()) if step == a.warmup + a.steps - 1 else live
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "live_joints_last": live, "limits_began_total": began, "limits_ended_total": ended, "bodies": nb, "joint_slots": nj}


def tenth_view(world):
    """A box that holds about a tenth of the live shapes: the middle tenth of their box centres along x, every y."""
    shapes = world["shapes"]
    box = shapes["aabb"][shapes["type"] != wire.SHAPE_FREE]
    cx = 0.5 * (box[:, 0] + box[:, 2])
    lo, hi = np.quantile(cx, [0.45, 0.55])
    return np.array([lo, box[:, 1].min() - 1.0, hi, box[:, 3].max() + 1.0], dtype=np.float32)


def run_shapes(world, mode, view):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, ns = len(world["bodies"]), len(world["shapes"])
    flags = SHAPE_FLAGS[mode]
    ms, in_view, entered, left = [], 0, 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if flags:
            s.world_set_shape_report(flags)
            s.world_set_shape_view(view)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if flags:
            e_buf, l_buf = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
            d_buf = np.zeros(ns, dtype=wire.shape_draw_dtype)
            m_buf = np.zeros(1, dtype=wire.shape_summary_dtype)
        if mode == "download":
            d_bodies, d_shapes, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(ns, dtype=wire.shape_dtype), np.zeros((nb, 2), dtype=np.float32)
        if mode == "download_step":
            d_poses, d_moved = np.zeros((nb, 4), dtype=np.float32), np.zeros(ns, dtype=np.dtype([("shape", np.int32), ("fatAABB", np.float32, 4)]))
        n1, n2 = ctypes.c_int32(), ctypes.c_int32()
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if flags & 1:
                s._ck(L.s2amd_world_shape_draws(h, wire.as_ptr(d_buf), ns, ctypes.byref(n1)))
                in_view = n1.value
            if flags & 2:
                s._ck(L.s2amd_world_shape_view_events(h, wire.as_ptr(e_buf), ns, ctypes.byref(n1), wire.as_ptr(l_buf), ns, ctypes.byref(n2)))
                entered, left = entered + n1.value, left + n2.value
            if flags & 4:
                s._ck(L.s2amd_world_shape_summary(h, wire.as_ptr(m_buf)))
                in_view = int(m_buf[0]["inView"])
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, wire.as_ptr(d_shapes), ns, None, wire.as_ptr(d_origins), None))
            if mode == "download_step":
                s._ck(L.s2amd_world_download_step(h, wire.as_ptr(d_poses), nb, wire.as_ptr(d_moved), ns, ctypes.byref(n1)))
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "in_view_last": in_view, "entered_total": entered, "left_total": left, "bodies": nb, "shape_slots": ns}


def run_bodies(world, mode):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, nc, nj = len(world["bodies"]), len(world["contacts"]), len(world["joints"])
    flags = BODY_FLAGS[mode]
    ms, records, rested, woke, n_islands = [], 0, 0, 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if flags:
            s.world_set_body_report(flags)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if flags:
            r_buf, w_buf = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
            b_buf = np.zeros(nb, dtype=wire.body_state_dtype)
            i_buf = np.zeros(nb, dtype=wire.island_state_dtype)
            m_buf = np.zeros(1, dtype=wire.body_summary_dtype)
        if mode == "download":
            from solver2d_amd import islands
            d_bodies, d_contacts, d_joints = np.zeros(nb, dtype=wire.body_dtype), np.zeros(nc, dtype=wire.contact_dtype), np.zeros(nj, dtype=wire.joint_dtype)
            d_origins = np.zeros((nb, 2), dtype=np.float32)
        n1, n2 = ctypes.c_int32(), ctypes.c_int32()
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if flags & 1:
                s._ck(L.s2amd_world_body_states(h, wire.as_ptr(b_buf), nb, ctypes.byref(n1)))
                records = n1.value
            if flags & 2:
                s._ck(L.s2amd_world_body_rest_events(h, wire.as_ptr(r_buf), nb, ctypes.byref(n1), wire.as_ptr(w_buf), nb, ctypes.byref(n2)))
                rested, woke = rested + n1.value, woke + n2.value
            if flags & 4:
                s._ck(L.s2amd_world_islands(h, wire.as_ptr(i_buf), nb, ctypes.byref(n1)))
                n_islands = n1.value
            if flags == 7:
                s._ck(L.s2amd_world_body_summary(h, wire.as_ptr(m_buf)))
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, wire.as_ptr(d_contacts), nc, wire.as_ptr(d_joints), nj, None, 0, None, wire.as_ptr(d_origins), None))
                _, n_islands = islands.find_islands(d_bodies, d_contacts, d_joints)
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "records_last": records, "rested_total": rested, "woke_total": woke, "islands_last": n_islands, "bodies": nb, "contact_slots": nc}


def run_metrics(world, mode):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, nc, nj = len(world["bodies"]), len(world["contacts"]), len(world["joints"])
    flags = METRICS_FLAGS[mode]
    ms, last, fetch_ms, fetched = [], None, 0.0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if flags:
            s.world_set_metrics(flags, a.steps if mode == "history" else 1)
            m_buf = np.zeros(a.steps if mode == "history" else 1, dtype=wire.step_metrics_dtype)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if mode == "download":
            from tests import step_metrics_ref
            d = {"bodies": np.zeros(nb, dtype=wire.body_dtype), "contacts": np.zeros(nc, dtype=wire.contact_dtype), "joints": np.zeros(nj, dtype=wire.joint_dtype),
                 "pairs": np.zeros(nc, dtype=wire.pair_state_dtype), "origins": np.zeros((nb, 2), dtype=np.float32)}
        n1 = ctypes.c_int32()
        for step in range(a.warmup + a.steps):
            if mode == "history" and step == a.warmup:
                s.world_set_metrics(flags, a.steps)  # (restarts the recorder: the ring holds exactly the timed steps)
            t0 = time.perf_counter()
            s.world_step(params)
            if flags and mode != "history":
                s._ck(L.s2amd_world_metrics(h, wire.as_ptr(m_buf)))
                last = m_buf[0]
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d["bodies"]), nb, wire.as_ptr(d["contacts"]), nc, wire.as_ptr(d["joints"]), nj, None, 0,
                                             wire.as_ptr(d["pairs"]), wire.as_ptr(d["origins"]), None))
                last = step_metrics_ref.record(d, params, 7, step)
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        if mode == "history":
            t0 = time.perf_counter()
            s._ck(L.s2amd_world_metrics_history(h, wire.as_ptr(m_buf), len(m_buf), ctypes.byref(n1)))
            fetch_ms = 1e3 * (time.perf_counter() - t0)
            fetched, last = n1.value, m_buf[n1.value - 1]
    total = sum(ms) + fetch_ms
    ms.sort()
    out = {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
           "total_ms": round(total, 3), "history_fetch_ms": round(fetch_ms, 4), "history_records": fetched, "bodies": nb, "contact_slots": nc}
    if last is not None:
        out.update({"touching_last": int(last["touchingContacts"]), "min_gap_last": float(last["minGap"]), "kinetic_energy_last": float(last["kineticEnergy"]),
                    "record_step_last": int(last["step"])})
    return out


for name in a.worlds.split(","):
    if name == "metrics":
        world = synthetic.pyramid_world(a.base)
        for mode in a.metrics_modes.split(","):
            r = run_metrics(world_chain.copy_world(world), mode)
            r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "report": "metrics", "mode": mode, "steps": a.steps,
                      "warmup": a.warmup})
            print(json.dumps(r), flush=True)
        continue
    if name == "bodies":
        for world_name, world in (("pyramid base %d" % a.base, synthetic.pyramid_world(a.base)), ("512 x pyramid base 40", synthetic.pyramid_world(40, 512))):
            for mode in a.body_modes.split(","):
                r = run_bodies(world_chain.copy_world(world), mode)
                r.update({"tree": a.label, "rep": a.rep, "world": world_name, "solver": SOLVER, "report": "body", "mode": mode, "steps": a.steps,
                          "warmup": a.warmup})
                print(json.dumps(r), flush=True)
        continue
    if name == "shaped":
        world = synthetic.pyramid_world(a.base)
        for view_name, view in (("tenth", tenth_view(world)), ("none", None)):
            for mode in a.shape_modes.split(","):
                if view_name == "none" and SHAPE_FLAGS[mode] == 0:
                    continue  # (without a flag the view is not looked at: these rows are the ones above)
                r = run_shapes(world_chain.copy_world(world), mode, view)
                r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "report": "shape", "view": view_name,
                          "mode": mode, "steps": a.steps, "warmup": a.warmup})
                print(json.dumps(r), flush=True)
        continue
    if name == "jointed":
        world = jointed_world(a.grid)
        for mode in a.joint_modes.split(","):
            r = run_joints(world_chain.copy_world(world), mode)
            r.update({"tree": a.label, "rep": a.rep, "world": "joint grid %d x %d" % (a.grid, a.grid), "solver": SOLVER, "report": "joint", "mode": mode,
                      "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(r), flush=True)
        continue
    world = synthetic.pyramid_world(a.base) if name == "pyramid" else world_chain.wreck_world(a.seed, a.base)
    for mode in a.modes.split(","):
        r = run(world_chain.copy_world(world), mode, name == "wreck")
        r.update({"tree": a.label, "rep": a.rep, "world": "%s base %d" % (name, a.base), "solver": SOLVER, "mode": mode, "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
