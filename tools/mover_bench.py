#!/usr/bin/env python3
"""What move-and-slide on the resident world costs per call, and what it replaces (the sibling of tools/shape_cast_bench.py).  The
standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft 8/4, uploaded and stepped `--settle` times in ONE solver; then
`--reps` passes over the modes, per pass and mode `--calls` calls after `--warmup`, each timed on the host from the call to its return
-- the copy of the movers up and the read-back of the answers included:

    move1, move64, move4096      s2amd_world_move_shapes with that many movers of four iterations, planes asked for
    casts1, casts64, casts4096   the route the call replaces: four s2amd_world_cast_shape calls with the clip of the statement's steps
                                 6 and 8 in numpy between them (every mover cast every time, no exclusion lists, no status: the least a
                                 host loop does)
    step                         s2amd_world_step alone

A mover is a circle of radius 0.25 that starts 1.5 m above the pile's surface over a random brick and wants to go 6 m down and 3 m across: onto
the pile and along it.
One JSON object per line, pass and mode, and one summary line per mode (median and range of the passes' medians); all answers land in
buffers allocated once, through the raw C calls.  The times are the host's, around whole calls: the kernels' own times are not measured.

`--tree DIR` times another checkout of the project with its library built (the parent commit's: `--modes step`) in the same session, so
that the step of this tree can be laid beside the step of the tree before it; `--tag` names the tree in the output.

    python tools/mover_bench.py [--reps 3] [--modes move64,casts64,step] [--base 200] >> profiles/mover.jsonl"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="move1,move64,move4096,casts1,casts64,casts4096,step")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="this tree")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

SOLVER = "TGS_Soft"
ITERATIONS = 4
f32 = np.float32


def starts(world, n, rng):
    """Above the pile's surface, clear of it: over a random brick, 1.5 m above the highest brick top within 1.5 m to either side"""
    shapes = world["shapes"]
    bricks = np.flatnonzero(world["bodies"]["type"][shapes["body"]] != wire.BODY_STATIC)
    box = shapes["aabb"][bricks]
    cx = 0.5 * (box[:, 0] + box[:, 2])
    x = cx[rng.randint(len(cx), size=n)] + (rng.rand(n) - 0.5)
    top = np.array([box[:, 3][np.abs(cx - xi) < 1.5].max() for xi in x])
    side = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    position = np.stack([x, top + 1.5], axis=1).astype(f32)
    translation = np.stack([-3.0 * side, np.full(n, -6.0)], axis=1).astype(f32)
    return position, translation


def movers_of(position, translation):
    m = np.zeros(len(position), dtype=wire.mover_dtype)
    m["count"], m["radius"], m["maxIterations"], m["maskBits"], m["ignoreBody"] = 1, 0.25, ITERATIONS, 0xFFFFFFFF, -1
    m["position"], m["translation"], m["rot"] = position, translation, (0.0, 1.0)
    return m


def host_loop(s, position, translation, casts, hits):
    """Four first-hit casts with the clip between them, vectorised over the batch"""
    L, h, n = s._L, s._h, len(position)
    p, r = position.copy(), translation.copy()
    for _ in range(ITERATIONS):
        casts["position"], casts["translation"] = p, r
        s._ck(L.s2amd_world_cast_shape(h, wire.as_ptr(casts), n, wire.as_ptr(hits)))
        t = np.where(hits["shape"] >= 0, hits["fraction"], f32(1.0)).astype(f32)[:, None]
        p = (p + t * r).astype(f32)
        rem = ((f32(1.0) - t) * r).astype(f32)
        normal = hits["normal"]
        into = np.minimum((rem * normal).sum(axis=1, dtype=f32), f32(0.0))[:, None]
        r = (rem - into * normal).astype(f32)
    return p


def timed(call):
    ms = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        call()
        if i >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"call_ms_mean": round(sum(ms) / len(ms), 4), "call_ms_median": round(ms[len(ms) // 2], 4), "call_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "call_ms_min": round(ms[0], 4)}


world = synthetic.pyramid_world(a.base)
params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
nb, ns = len(world["bodies"]), len(world["shapes"])
common = {"world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "mover", "tree": a.tag, "calls": a.calls, "warmup": a.warmup, "bodies": nb,
          "shape_slots": ns, "kernel_times": "not measured"}
medians = {}
with hip.Solver(0) as s:
    L, h = s._L, s._h
    s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
    for _ in range(a.settle):
        s.world_step(params)
    info = wire.WorldStepInfo()
    for rep in range(a.reps):
        rng = np.random.RandomState(a.seed)
        for mode in a.modes.split(","):
            extra = {}
            if mode == "step":
                # (the steps come last in a pass: the world the movers are timed on is the settled one)
                r = timed(lambda: s._ck(L.s2amd_world_step(h, ctypes.byref(params), ctypes.byref(info))))
            else:
                n = int(mode.lstrip("movecasts"))
                position, translation = starts(world, n, rng)
                if mode.startswith("move"):
                    m = movers_of(position, translation)
                    results, planes = np.zeros(n, dtype=wire.mover_result_dtype), np.zeros(8 * n, dtype=wire.mover_plane_dtype)
                    r = timed(lambda: s._ck(L.s2amd_world_move_shapes(h, wire.as_ptr(m), n, wire.as_ptr(results), wire.as_ptr(planes))))
                    extra = {"movers": n, "iterations": ITERATIONS, "with_a_plane": int((results["planeCount"] >= 1).sum()),
                             "statuses": np.bincount(results["status"], minlength=5).tolist(), "casts_made": int(results["iterations"].sum())}
                else:
                    casts = np.zeros(n, dtype=wire.shape_cast_dtype)
                    casts["count"], casts["radius"], casts["maxFraction"], casts["maskBits"], casts["rot"] = 1, 0.25, 1.0, 0xFFFFFFFF, (0.0, 1.0)
                    hits = np.zeros(n, dtype=wire.shape_cast_hit_dtype)
                    r = timed(lambda: host_loop(s, position, translation, casts, hits))
                    extra = {"movers": n, "iterations": ITERATIONS}
            r.update(common, mode=mode, rep=rep, **extra)
            medians.setdefault(mode, []).append(r["call_ms_median"])
            print(json.dumps(r), flush=True)
for mode, m in medians.items():
    print(json.dumps(dict(common, mode=mode, summary="median and range of the passes' medians", reps=len(m), call_ms_median=sorted(m)[len(m) // 2],
                          call_ms_lowest=min(m), call_ms_highest=max(m))), flush=True)
