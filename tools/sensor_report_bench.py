#!/usr/bin/env python3
"""What the sensor report costs per step, and what it replaces.  The standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft
8/4, uploaded and stepped `--settle` times, with 1 / 64 / 1,024 sensors of about 3 m, half of them fixed over the pile and half attached
to bricks; then per mode `--steps` steps after `--warmup`, each timed on the host from the call of s2amd_world_step to the return of the
last getter:

    step0          the step with the sensors set and no flag: nothing is enqueued for them (what the parent commit's step is compared to)
    inside         the step under S2AMD_SENSOR_REPORT_INSIDE and s2amd_world_sensor_inside
    events         ... under EVENTS and s2amd_world_sensor_events
    states         ... under STATES and s2amd_world_sensor_states
    host_route     what the report replaces: the step, a download of the body poses (s2amd_world_download of bodies and origins), the
                   transforms composed on the host, s2amd_world_shapes_in_range, and the set difference against last step's lists

One JSON object per line, mode and sensor count, on standard output, as the other bench tools print them: profiles/sensor_report.jsonl is
this output redirected, run by run.  All answers land in buffers allocated once, through the raw C calls.

    python tools/sensor_report_bench.py --tree . --label this [--rep N] [--modes step0,inside] [--sensors 1,64,1024] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built; a tree without the sensor API can run `step0`, where it sets no sensors).  Run two trees alternately, several repeats
each, in ONE session, so that the run-to-run spread is known before a difference is read (profiles/sensor_report.jsonl)."""
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
ap.add_argument("--modes", default="step0,inside,events,states,host_route")
ap.add_argument("--sensors", default="1,64,1024")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--list-capacity", type=int, default=65536)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
ALL = 0xFFFFFFFF
f32 = np.float32
HAVE_SENSORS = hasattr(wire, "sensor_dtype")


def sensor_fields(world, count, rng):
    """(vertices, radius, position, rot, margin, body) per sensor: rounded boxes of about 3 m, the even ones fixed at a brick's place,
    the odd ones attached to that brick"""
    shapes = world["shapes"]
    bricks = np.flatnonzero(world["bodies"]["type"][shapes["body"]] != wire.BODY_STATIC)
    pick = bricks[rng.randint(len(bricks), size=count)]
    out = []
    for i, slot in enumerate(pick):
        body = int(shapes["body"][slot])
        hx, hy = 1.0 + rng.rand(), 1.0 + rng.rand()
        attached = i % 2 == 1
        out.append(([(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)], 0.25, (0.0, 0.0) if attached else tuple(world["origins"][body]), (0.0, 1.0), 0.1,
                    body if attached else -1))
    return out


def run(world, mode, count):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb = len(world["bodies"])
    rng = np.random.RandomState(a.seed)
    fields = sensor_fields(world, count, rng)
    ms, answered = [], 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if HAVE_SENSORS:
            sensors = np.zeros(count, dtype=wire.sensor_dtype)
            for q, (verts, radius, position, rot, margin, body) in zip(sensors, fields):
                q["vertices"][:4], q["count"], q["radius"], q["position"], q["rot"], q["margin"], q["maskBits"], q["body"] = verts, 4, radius, position, rot, margin, ALL, body
            s.world_set_sensors(sensors)
            flag = {"step0": 0, "host_route": 0, "inside": wire.SENSOR_REPORT_INSIDE, "events": wire.SENSOR_REPORT_EVENTS, "states": wire.SENSOR_REPORT_STATES}[mode]
            s.world_set_sensor_report(flag, a.list_capacity)
        else:
            assert mode in ("step0", "host_route"), mode
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        offsets, out, total = np.zeros(count + 1, dtype=np.int32), np.zeros(a.list_capacity, dtype=np.int32), ctypes.c_int32()
        if mode == "events":
            entered, left = np.zeros(a.list_capacity, dtype=wire.sensor_event_dtype), np.zeros(a.list_capacity, dtype=wire.sensor_event_dtype)
            ne, nl = ctypes.c_int32(), ctypes.c_int32()
        elif mode == "states":
            states, n = np.zeros(count, dtype=wire.sensor_state_dtype), ctypes.c_int32()
        elif mode == "host_route":
            d_bodies, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros((nb, 2), dtype=np.float32)
            queries = np.zeros(count, dtype=wire.proximity_query_dtype)
            for q, (verts, radius, position, rot, margin, body) in zip(queries, fields):
                q["vertices"][:4], q["count"], q["radius"], q["position"], q["rot"], q["maxDistance"], q["maskBits"] = verts, 4, radius, position, rot, margin, ALL
            attached = np.array([f[5] for f in fields], dtype=np.int64)
            rel = np.array([f[2] for f in fields], dtype=f32)
            last = [set() for _ in range(count)]
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if mode == "inside":
                s._ck(L.s2amd_world_sensor_inside(h, wire.as_ptr(offsets), wire.as_ptr(out), len(out), ctypes.byref(total)))
            elif mode == "events":
                s._ck(L.s2amd_world_sensor_events(h, wire.as_ptr(entered), len(entered), ctypes.byref(ne), wire.as_ptr(left), len(left), ctypes.byref(nl)))
            elif mode == "states":
                s._ck(L.s2amd_world_sensor_states(h, wire.as_ptr(states), count, ctypes.byref(n)))
            elif mode == "host_route":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, None, 0, None, wire.as_ptr(d_origins), None))
                on = attached >= 0
                b = attached[on]
                bs, bc = d_bodies["rot"][b, 0], d_bodies["rot"][b, 1]
                queries["position"][on] = np.stack([(bc * rel[on, 0] - bs * rel[on, 1]) + d_origins[b, 0], (bs * rel[on, 0] + bc * rel[on, 1]) + d_origins[b, 1]], axis=1)
                queries["rot"][on] = np.stack([bs, bc], axis=1)  # (the sensors' own rotation is the identity here)
                s._ck(L.s2amd_world_shapes_in_range(h, wire.as_ptr(queries), count, wire.as_ptr(offsets), wire.as_ptr(out), None, len(out), ctypes.byref(total)))
                now = [set(out[offsets[i]:offsets[i + 1]].tolist()) for i in range(count)]
                events = sum(len(x - y) + len(y - x) for x, y in zip(now, last))
                last = now
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        if mode in ("inside", "host_route"):
            answered = int(total.value)
        elif mode == "events":
            answered = int(ne.value + nl.value)
        elif mode == "states":
            answered = int(states["inside"].sum())
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "step_ms_min": round(ms[0], 4), "answered": answered, "bodies": nb, "shape_slots": len(world["shapes"])}


world = synthetic.pyramid_world(a.base)
for count in [int(x) for x in a.sensors.split(",")]:
    for mode in a.modes.split(","):
        r = run(world_chain.copy_world(world), mode, count)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "sensor_report", "mode": mode, "sensors": count,
                  "steps": a.steps, "warmup": a.warmup, "list_capacity": a.list_capacity})
        print(json.dumps(r), flush=True)
