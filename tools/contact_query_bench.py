#!/usr/bin/env python3
"""What a contact query on the resident world costs per call, and what it replaces (the sibling of tools/proximity_query_bench.py).  The
standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft 8/4, uploaded and stepped `--settle` times in ONE solver; then
`--reps` passes over the modes, per pass and mode `--calls` calls after `--warmup`, each timed on the host from the call to its return
-- the copy of the queries up and the read-back of the answers included:

    deepest1, deepest64, deepest4096   s2amd_world_deepest_contact with that many queries
    collide1, collide64, collide4096   s2amd_world_collide_shape with that many queries, room for 16 hits a query
    download                           what a host-side s2Collide* needs first: s2amd_world_download of shapes, bodies and origins

A query is a brick's own polygon laid over a random brick, a third of its width and a fifth of its height off the brick's place.  One
JSON object per line, pass and mode, and one summary line per mode (median and range of the passes' medians); all answers land in buffers
allocated once, through the raw C calls.

    python tools/contact_query_bench.py [--reps 3] [--modes deepest1,collide4096,download] [--base 200] > profiles/contact_queries.jsonl"""
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
ap.add_argument("--modes", default="deepest1,deepest64,deepest4096,collide1,collide64,collide4096,download")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
SOLVER = "TGS_Soft"


def queries(world, n, rng):
    shapes, bodies = world["shapes"], world["bodies"]
    bricks = np.flatnonzero((shapes["type"] == wire.SHAPE_POLYGON) & (bodies["type"][shapes["body"]] != wire.BODY_STATIC))
    brick = shapes[bricks[0]]
    size = brick["vertices"][:brick["count"]].max(axis=0) - brick["vertices"][:brick["count"]].min(axis=0)
    q = np.zeros(n, dtype=wire.contact_query_dtype)
    q["vertices"], q["normals"], q["type"], q["count"], q["radius"] = brick["vertices"], brick["normals"], brick["type"], brick["count"], brick["radius"]
    q["maskBits"] = 0xFFFFFFFF
    centre = 0.5 * (shapes["aabb"][bricks][:, :2] + shapes["aabb"][bricks][:, 2:])
    q["position"] = (centre[rng.randint(len(centre), size=n)] + size * np.array([1.0 / 3.0, 0.2])).astype(np.float32)
    q["rot"] = (0.0, 1.0)
    return q


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
common = {"world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "contact_query", "calls": a.calls, "warmup": a.warmup, "bodies": nb,
          "shape_slots": ns}
medians = {}
with hip.Solver(0) as s:
    L, h = s._L, s._h
    s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
    for _ in range(a.settle):
        s.world_step(params)
    d_bodies, d_shapes, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(ns, dtype=wire.shape_dtype), np.zeros((nb, 2), dtype=np.float32)
    for rep in range(a.reps):
        rng = np.random.RandomState(a.seed)
        for mode in a.modes.split(","):
            answered = 0
            if mode == "download":
                r = timed(lambda: s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, wire.as_ptr(d_shapes), ns, None,
                                                               wire.as_ptr(d_origins), None)))
            else:
                n = int(mode.lstrip("depstcoli"))
                q = queries(world, n, rng)
                if mode.startswith("deepest"):
                    hits = np.zeros(n, dtype=wire.contact_hit_dtype)
                    r = timed(lambda: s._ck(L.s2amd_world_deepest_contact(h, wire.as_ptr(q), n, wire.as_ptr(hits))))
                    answered = int((hits["shape"] >= 0).sum())
                else:
                    offsets, out, total = np.zeros(n + 1, dtype=np.int32), np.zeros(16 * n + 64, dtype=wire.contact_hit_dtype), ctypes.c_int32()
                    r = timed(lambda: s._ck(L.s2amd_world_collide_shape(h, wire.as_ptr(q), n, wire.as_ptr(offsets), wire.as_ptr(out), len(out),
                                                                        ctypes.byref(total))))
                    answered = int(total.value)
            r.update(common, mode=mode, rep=rep, hits=answered)
            medians.setdefault(mode, []).append(r["call_ms_median"])
            print(json.dumps(r), flush=True)
for mode, m in medians.items():
    print(json.dumps(dict(common, mode=mode, summary="median and range of the passes' medians", reps=len(m), call_ms_median=sorted(m)[len(m) // 2],
                          call_ms_lowest=min(m), call_ms_highest=max(m))), flush=True)
