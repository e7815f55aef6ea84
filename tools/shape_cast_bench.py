#!/usr/bin/env python3
"""What a shape cast on the resident world costs per call, and what it replaces (the sibling of tools/proximity_query_bench.py).  The
standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft 8/4, uploaded and stepped `--settle` times in ONE solver; then
`--reps` passes over the modes, per pass and mode `--calls` calls after `--warmup`, each timed on the host from the call to its return
-- the copy of the casts up and the read-back of the answers included:

    first1, first64, first4096   s2amd_world_cast_shape with that many casts
    all1, all64, all4096         s2amd_world_cast_shape_all with that many casts
    download                     what a host-side loop over s2ShapeDistance needs first: s2amd_world_download of shapes, bodies and origins
    step                         s2amd_world_step alone
    step_after_first64           s2amd_world_step with a 64-cast s2amd_world_cast_shape in front of it: the step's own time

A cast is a circle of radius 0.25 that starts 3 m above a random brick, to its side, and sweeps 6 m down and across.  One JSON object
per line, pass and mode, and one summary line per mode (median and range of the passes' medians); all answers land in buffers allocated
once, through the raw C calls.

    python tools/shape_cast_bench.py [--reps 3] [--modes first1,all4096,download] [--base 200] > profiles/shape_casts.jsonl"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="first1,first64,first4096,all1,all64,all4096,download,step,step_after_first64")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
SOLVER = "TGS_Soft"


def casts(world, n, rng):
    shapes = world["shapes"]
    bricks = np.flatnonzero(world["bodies"]["type"][shapes["body"]] != wire.BODY_STATIC)
    centre = 0.5 * (shapes["aabb"][bricks][:, :2] + shapes["aabb"][bricks][:, 2:])
    c = np.zeros(n, dtype=wire.shape_cast_dtype)
    c["count"], c["radius"], c["maxFraction"], c["maskBits"] = 1, 0.25, 1.0, 0xFFFFFFFF
    side = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    c["position"] = (centre[rng.randint(len(centre), size=n)] + np.stack([1.5 * side, np.full(n, 3.0)], axis=1)).astype(np.float32)
    c["translation"] = np.stack([-3.0 * side, np.full(n, -6.0)], axis=1).astype(np.float32)
    c["rot"] = (0.0, 1.0)
    return c


def timed(call, before=None):
    ms = []
    for i in range(a.warmup + a.calls):
        if before is not None:
            before()
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
common = {"world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "shape_cast", "calls": a.calls, "warmup": a.warmup, "bodies": nb,
          "shape_slots": ns}
medians = {}
with hip.Solver(0) as s:
    L, h = s._L, s._h
    s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
    for _ in range(a.settle):
        s.world_step(params)
    d_bodies, d_shapes, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(ns, dtype=wire.shape_dtype), np.zeros((nb, 2), dtype=np.float32)
    info = wire.WorldStepInfo()
    for rep in range(a.reps):
        rng = np.random.RandomState(a.seed)
        for mode in a.modes.split(","):
            answered, advances = 0, 0
            if mode == "download":
                r = timed(lambda: s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, wire.as_ptr(d_shapes), ns, None,
                                                               wire.as_ptr(d_origins), None)))
            elif mode.startswith("step"):
                # (the steps come last in a pass: the world the casts are timed on is the settled one)
                c = casts(world, 64, rng)
                hits = np.zeros(64, dtype=wire.shape_cast_hit_dtype)
                front = (lambda: s._ck(L.s2amd_world_cast_shape(h, wire.as_ptr(c), 64, wire.as_ptr(hits)))) if mode == "step_after_first64" else None
                r = timed(lambda: s._ck(L.s2amd_world_step(h, ctypes.byref(params), ctypes.byref(info))), front)
            else:
                n = int(mode.lstrip("firstal"))
                c = casts(world, n, rng)
                if mode.startswith("first"):
                    hits = np.zeros(n, dtype=wire.shape_cast_hit_dtype)
                    r = timed(lambda: s._ck(L.s2amd_world_cast_shape(h, wire.as_ptr(c), n, wire.as_ptr(hits))))
                    answered, advances = int((hits["shape"] >= 0).sum()), int(hits["iterations"].max())
                else:
                    offsets, out, total = np.zeros(n + 1, dtype=np.int32), np.zeros(32 * n + 1024, dtype=wire.shape_cast_hit_dtype), ctypes.c_int32()
                    r = timed(lambda: s._ck(L.s2amd_world_cast_shape_all(h, wire.as_ptr(c), n, wire.as_ptr(offsets), wire.as_ptr(out), len(out),
                                                                         ctypes.byref(total))))
                    answered, advances = int(total.value), int(out["iterations"][:total.value].max()) if total.value else 0
            r.update(common, mode=mode, rep=rep, hits=answered, most_advances=advances)
            medians.setdefault(mode, []).append(r["call_ms_median"])
            print(json.dumps(r), flush=True)
for mode, m in medians.items():
    print(json.dumps(dict(common, mode=mode, summary="median and range of the passes' medians", reps=len(m), call_ms_median=sorted(m)[len(m) // 2],
                          call_ms_lowest=min(m), call_ms_highest=max(m))), flush=True)
