#!/usr/bin/env python3
"""What the ray report costs per step, and what it replaces.  The standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft
8/4, uploaded and stepped `--settle` times, with 64 / 1,024 / 4,096 / 16,384 rays of 3 m in one of two layouts:

    fans        lidar fans of 64 rays each, mounted on bricks (a fan's rays leave its brick's centre in 64 directions); the bricks are
                taken in slot order, so the four fans of a chunk of 256 rays ride on bricks of one neighbourhood
    scattered   fixed rays spread uniformly over the pile with random directions: the chunk box's worst case (every chunk's box is the
                whole pile)

then per mode `--steps` steps after `--warmup`, each timed on the host from the call of s2amd_world_step to the return of the last call:

    step0       the step with the rays set and no flag: nothing is enqueued for them (what the parent commit's step is compared to)
    states      the step under S2AMD_RAY_REPORT_STATES and s2amd_world_ray_states
    ranges      ... under RANGES and s2amd_world_ray_ranges
    events      ... under EVENTS and s2amd_world_ray_events
    export      ... under RANGES and s2amd_world_export_ray_ranges into a device buffer, no getter
    host_route  what the report replaces: the step, s2amd_world_download_step's poses, s2TransformPoint on both ends in numpy, and
                s2amd_world_ray_cast of the world rays

One JSON object per line, mode, layout and ray count, on standard output, as the other bench tools print them: profiles/ray_report.jsonl
is this output redirected, run by run.  All answers land in buffers allocated once, through the raw C calls.  Host wall time only: no
kernel times are collected.

    python tools/ray_report_bench.py --tree . --label this [--rep N] [--modes step0,states] [--rays 64,1024] [--layouts fans] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built; a tree without the ray API can run `step0`, where it sets no rays, and `host_route`).  Run two trees alternately, several
repeats each, in ONE session, so that the run-to-run spread is known before a difference is read (profiles/ray_report.jsonl)."""
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
ap.add_argument("--modes", default="step0,states,ranges,events,export,host_route")
ap.add_argument("--rays", default="64,1024,4096,16384")
ap.add_argument("--layouts", default="fans,scattered")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
ALL = 0xFFFFFFFF
REACH = 3.0
HAVE_RAYS = hasattr(wire, "ray_sensor_dtype")


def ray_fields(world, count, layout, rng):
    """(p1, p2, body) per ray, float32 arrays"""
    shapes, bodies = world["shapes"], world["bodies"]
    bricks = np.flatnonzero(bodies["type"][shapes["body"]] != wire.BODY_STATIC)
    if layout == "fans":
        fans = (count + 63) // 64
        pick = np.sort(bricks[rng.randint(len(bricks), size=fans)])
        body = np.repeat(shapes["body"][pick].astype(np.int32), 64)[:count]
        angle = (np.arange(count) % 64) * (2.0 * np.pi / 64.0)
        p1 = np.zeros((count, 2), dtype=np.float32)
        p2 = np.stack([REACH * np.cos(angle), REACH * np.sin(angle)], axis=1).astype(np.float32)
        return p1, p2, body
    origins = world["origins"][shapes["body"][bricks]]
    lower, upper = origins.min(axis=0) - 1.0, origins.max(axis=0) + 1.0
    p1 = (lower + rng.rand(count, 2) * (upper - lower)).astype(np.float32)
    angle = rng.rand(count) * 2.0 * np.pi
    p2 = (p1 + np.stack([REACH * np.cos(angle), REACH * np.sin(angle)], axis=1)).astype(np.float32)
    return p1, p2, np.full(count, -1, dtype=np.int32)


def run(world, mode, count, layout):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, ns = len(world["bodies"]), len(world["shapes"])
    p1, p2, body = ray_fields(world, count, layout, np.random.RandomState(a.seed))
    ms, answered, buf = [], 0, None
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if HAVE_RAYS:
            rays = np.zeros(count, dtype=wire.ray_sensor_dtype)
            rays["p1"], rays["p2"], rays["maxFraction"], rays["maskBits"], rays["body"] = p1, p2, 1.0, ALL, body
            s.world_set_ray_sensors(rays)
            flag = {"step0": 0, "host_route": 0, "states": wire.RAY_REPORT_STATES, "ranges": wire.RAY_REPORT_RANGES, "export": wire.RAY_REPORT_RANGES,
                    "events": wire.RAY_REPORT_EVENTS}[mode]
            s.world_set_ray_report(flag)
        else:
            assert mode in ("step0", "host_route"), mode
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        n = ctypes.c_int32()
        if mode == "states":
            states = np.zeros(count, dtype=wire.ray_state_dtype)
        elif mode == "ranges":
            ranges = np.zeros(count, dtype=np.float32)
        elif mode == "events":
            events = np.zeros(count, dtype=wire.ray_event_dtype)
        elif mode == "export":
            buf = s.device_alloc(4 * count)
        elif mode == "host_route":
            poses, moved, n_moved = np.zeros((nb, 4), dtype=np.float32), np.zeros(ns, dtype=np.dtype([("shape", np.int32), ("fatAABB", np.float32, 4)])), ctypes.c_int32()
            world_rays, hits = np.zeros(count, dtype=wire.ray_dtype), np.zeros(count, dtype=wire.ray_hit_dtype)
            world_rays["maxFraction"], world_rays["maskBits"] = 1.0, ALL
            on = body >= 0
            b = body[on]
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if mode == "states":
                s._ck(L.s2amd_world_ray_states(h, wire.as_ptr(states), count, ctypes.byref(n)))
            elif mode == "ranges":
                s._ck(L.s2amd_world_ray_ranges(h, wire.as_ptr(ranges), count, ctypes.byref(n)))
            elif mode == "events":
                s._ck(L.s2amd_world_ray_events(h, wire.as_ptr(events), count, ctypes.byref(n)))
            elif mode == "export":
                s._ck(L.s2amd_world_export_ray_ranges(h, ctypes.c_void_p(buf), count))
            elif mode == "host_route":
                s._ck(L.s2amd_world_download_step(h, wire.as_ptr(poses), nb, wire.as_ptr(moved), ns, ctypes.byref(n_moved)))
                ox, oy, bs, bc = poses[b, 0], poses[b, 1], poses[b, 2], poses[b, 3]
                for name, p in (("p1", p1), ("p2", p2)):
                    world_rays[name] = p
                    world_rays[name][on] = np.stack([(bc * p[on, 0] - bs * p[on, 1]) + ox, (bs * p[on, 0] + bc * p[on, 1]) + oy], axis=1)
                s._ck(L.s2amd_world_ray_cast(h, wire.as_ptr(world_rays), count, wire.as_ptr(hits)))
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        if mode == "states":
            answered = int((states["shape"] >= 0).sum())
        elif mode == "ranges":
            answered = int((ranges < 1.0).sum())
        elif mode == "events":
            answered = int(n.value)
        elif mode == "export":
            answered = int((s.device_read(buf, (count,), np.float32) < 1.0).sum())
            s.device_free(buf)
        elif mode == "host_route":
            answered = int((hits["shape"] >= 0).sum())
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "step_ms_min": round(ms[0], 4), "answered": answered, "bodies": nb, "shape_slots": ns}


world = synthetic.pyramid_world(a.base)
for layout in a.layouts.split(","):
    for count in [int(x) for x in a.rays.split(",")]:
        for mode in a.modes.split(","):
            r = run(world_chain.copy_world(world), mode, count, layout)
            r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "ray_report", "mode": mode, "layout": layout,
                      "rays": count, "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(r), flush=True)
