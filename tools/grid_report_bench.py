#!/usr/bin/env python3
"""What the grid report costs per step, and what it replaces.  The standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft
8/4, uploaded and stepped `--settle` times, under one of five lists of occupancy grids with cells of 0.25 m:

    1x16, 64x16, 1024x16    1, 64 and 1,024 grids of 16 x 16, every second one mounted on a brick and centred on it, the others fixed
                            over the pile
    16x64                   16 grids of 64 x 64, likewise
    1x256                   one fixed grid of 256 x 256 centred on the pile

then per mode `--steps` steps after `--warmup`, each timed on the host from the call of s2amd_world_step to the return of the last call:

    step0       the step with the grids set and no flag: nothing is enqueued for them (what the parent commit's step is compared to)
    categories  the step under S2AMD_GRID_REPORT_CATEGORIES and s2amd_world_grid_categories
    shapes      ... under SHAPES and s2amd_world_grid_shapes
    occupancy   ... under OCCUPANCY and s2amd_world_grid_occupancy
    states      ... under STATES and s2amd_world_grid_states
    export      ... under OCCUPANCY and s2amd_world_export_grid_occupancy into a device buffer, no getter
    host_route  what the report replaces: the step, s2amd_world_download_step's poses, the cell points in numpy, one
                s2amd_world_point_probe of them, and the fold of its lists into the shapes image in numpy

One JSON object per line, mode and list, on standard output, as the other bench tools print them: profiles/grid_report.jsonl is this
output redirected, run by run.  All answers land in buffers allocated once, through the raw C calls.  Host wall time only: no kernel
times are collected.

    python tools/grid_report_bench.py --tree . --label this [--rep N] [--modes step0,shapes] [--lists 1x16,16x64] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built; a tree without the grid API can run `step0`, where it sets no grids, and `host_route`).  Run two trees alternately, several
repeats each, in ONE session, so that the run-to-run spread is known before a difference is read (profiles/grid_report.jsonl)."""
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
ap.add_argument("--modes", default="step0,categories,shapes,occupancy,states,export,host_route")
ap.add_argument("--lists", default="1x16,64x16,1024x16,16x64,1x256")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
ALL = 0xFFFFFFFF
CELL = np.float32(0.25)
HAVE_GRIDS = hasattr(wire, "grid_sensor_dtype")
BATCH = 65536  # probes per s2amd_world_point_probe call of the host route
f32 = np.float32


def grid_fields(world, name, rng):
    """(position, side, body) per grid"""
    count, side = (int(x) for x in name.split("x"))
    shapes, bodies = world["shapes"], world["bodies"]
    bricks = np.flatnonzero(bodies["type"][shapes["body"]] != wire.BODY_STATIC)
    origins = world["origins"][shapes["body"][bricks]]
    lower, upper = origins.min(axis=0), origins.max(axis=0)
    if count == 1:
        return ((lower + upper) / 2).astype(f32)[None, :], side, np.full(1, -1, dtype=np.int32)
    position = (lower + rng.rand(count, 2) * (upper - lower)).astype(f32)
    body = np.full(count, -1, dtype=np.int32)
    pick = np.sort(bricks[rng.randint(len(bricks), size=count)])
    body[1::2] = shapes["body"][pick][1::2]
    position[1::2] = 0.0
    return position, side, body


def run(world, mode, name):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, ns = len(world["bodies"]), len(world["shapes"])
    position, side, body = grid_fields(world, name, np.random.RandomState(a.seed))
    count, cells = len(body), len(body) * side * side
    ms, answered, buf = [], 0, None
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if HAVE_GRIDS:
            grids = np.zeros(count, dtype=wire.grid_sensor_dtype)
            grids["position"], grids["rot"], grids["cellSize"], grids["width"], grids["height"] = position, (0.0, 1.0), CELL, side, side
            grids["maskBits"], grids["body"] = ALL, body
            s.world_set_grid_sensors(grids)
            flag = {"step0": 0, "host_route": 0, "categories": wire.GRID_REPORT_CATEGORIES, "shapes": wire.GRID_REPORT_SHAPES, "occupancy": wire.GRID_REPORT_OCCUPANCY,
                    "export": wire.GRID_REPORT_OCCUPANCY, "states": wire.GRID_REPORT_STATES}[mode]
            s.world_set_grid_report(flag)
        else:
            assert mode in ("step0", "host_route"), mode
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        n = ctypes.c_int32()
        if mode in ("categories", "shapes", "occupancy"):
            out = np.zeros(cells, dtype={"categories": np.uint32, "shapes": np.int32, "occupancy": np.float32}[mode])
            fn = getattr(L, "s2amd_world_grid_" + mode)
        elif mode == "states":
            out, fn = np.zeros(count, dtype=wire.grid_state_dtype), L.s2amd_world_grid_states
        elif mode == "export":
            buf = s.device_alloc(4 * cells)
        elif mode == "host_route":
            poses, moved, n_moved = np.zeros((nb, 4), dtype=f32), np.zeros(ns, dtype=np.dtype([("shape", np.int32), ("fatAABB", np.float32, 4)])), ctypes.c_int32()
            probes = np.zeros(cells, dtype=wire.point_probe_dtype)
            probes["maskBits"] = ALL
            local = ((np.arange(side, dtype=f32) + f32(0.5)) - f32(0.5) * f32(side)) * CELL
            lx, ly = np.tile(local, side), np.repeat(local, side)
            capacity = 4 * cells + 64
            offsets, flat, total = np.zeros(cells + 1, dtype=np.int32), np.zeros(capacity, dtype=np.int32), ctypes.c_int32()
            image = np.zeros(cells, dtype=np.int32)
            on = body >= 0
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if mode in ("categories", "shapes", "occupancy", "states"):
                s._ck(fn(h, wire.as_ptr(out), len(out), ctypes.byref(n)))
            elif mode == "export":
                s._ck(L.s2amd_world_export_grid_occupancy(h, ctypes.c_void_p(buf), cells))
            elif mode == "host_route":
                s._ck(L.s2amd_world_download_step(h, wire.as_ptr(poses), nb, wire.as_ptr(moved), ns, ctypes.byref(n_moved)))
                px, py, gs, gc = position[:, 0].copy(), position[:, 1].copy(), np.zeros(count, dtype=f32), np.ones(count, dtype=f32)
                px[on], py[on], gs[on], gc[on] = poses[body[on], 0], poses[body[on], 1], poses[body[on], 2], poses[body[on], 3]
                probes["p"][:, 0] = ((gc[:, None] * lx[None, :] - gs[:, None] * ly[None, :]) + px[:, None]).ravel()
                probes["p"][:, 1] = ((gs[:, None] * lx[None, :] + gc[:, None] * ly[None, :]) + py[:, None]).ravel()
                image[:] = -1
                for at in range(0, cells, BATCH):  # (one call takes at most 2^31 probes x shape slots)
                    m = min(BATCH, cells - at)
                    s._ck(L.s2amd_world_point_probe(h, wire.as_ptr(probes[at: at + m]), m, wire.as_ptr(offsets), wire.as_ptr(flat), capacity, ctypes.byref(total)))
                    hit = offsets[1: m + 1] > offsets[:m]
                    image[at: at + m][hit] = flat[offsets[:m][hit]]  # (ascending by slot per probe: the first entry is the lowest)
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        if mode == "categories":
            answered = int((out != 0).sum())
        elif mode == "shapes":
            answered = int((out >= 0).sum())
        elif mode == "occupancy":
            answered = int(out.sum())
        elif mode == "states":
            answered = int(out["occupied"].sum())
        elif mode == "export":
            answered = int(s.device_read(buf, (cells,), np.float32).sum())
            s.device_free(buf)
        elif mode == "host_route":
            answered = int((image >= 0).sum())
    ms.sort()
    return {"step_ms_mean": round(sum(ms) / len(ms), 4), "step_ms_median": round(ms[len(ms) // 2], 4), "step_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "step_ms_min": round(ms[0], 4), "step_ms_max": round(ms[-1], 4), "answered": answered, "cells": cells, "bodies": nb, "shape_slots": ns}


world = synthetic.pyramid_world(a.base)
for name in a.lists.split(","):
    for mode in a.modes.split(","):
        r = run(world_chain.copy_world(world), mode, name)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "grid_report", "mode": mode, "list": name,
                  "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
