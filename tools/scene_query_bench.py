#!/usr/bin/env python3
"""What a scene query on the resident world costs per call, and what it replaces.  The standing base-N pyramid (20,101 shapes at base
200) under TGS_Soft 8/4, uploaded and stepped `--settle` times; then per mode `--calls` calls after `--warmup`, each timed on the host
from the call to its return -- the copy of the queries up and the read-back of the answers included:

    ray1, ray64, ray4096   s2amd_world_ray_cast with that many rays (from beside and above the pile through random bricks' centres)
    probe64                s2amd_world_point_probe with 64 points (brick centres and points around them)
    box64                  s2amd_world_query_boxes with 64 boxes of up to 3 m
    download               what a host-side query needs first: s2amd_world_download of shapes, bodies and origins
    download_boxes         ... or, for box queries alone, s2amd_world_download_boxes

One JSON object per line and mode.  All answers land in buffers allocated once, through the raw C calls.

    python tools/scene_query_bench.py --tree . --label this [--rep N] [--modes ray1,ray4096,download] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built; a tree without the query API can run `download` and `download_boxes`).  Run two trees alternately, several repeats each,
in ONE session, so that the run-to-run spread is known before a difference is read (profiles/scene_queries.jsonl)."""
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
ap.add_argument("--modes", default="ray1,ray64,ray4096,probe64,box64,download,download_boxes")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
ALL = 0xFFFFFFFF
f32 = np.float32


def queries(world, mode, rng):
    shapes = world["shapes"]
    bricks = np.flatnonzero(world["bodies"]["type"][shapes["body"]] != wire.BODY_STATIC)
    centre = 0.5 * (shapes["aabb"][bricks][:, :2] + shapes["aabb"][bricks][:, 2:])
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    n = int(mode.lstrip("rayprobex"))
    pick = centre[rng.randint(len(centre), size=n)]
    if mode.startswith("ray"):
        q = np.zeros(n, dtype=wire.ray_dtype)
        side = rng.randint(3, size=n)
        start = np.where((side == 0)[:, None], np.stack([np.full(n, lo[0] - 20.0), lo[1] + (hi[1] - lo[1]) * rng.rand(n)], axis=1),
                         np.where((side == 1)[:, None], np.stack([np.full(n, hi[0] + 20.0), lo[1] + (hi[1] - lo[1]) * rng.rand(n)], axis=1),
                                  np.stack([lo[0] + (hi[0] - lo[0]) * rng.rand(n), np.full(n, hi[1] + 20.0)], axis=1)))
        q["p1"], q["p2"] = start.astype(f32), (start + 1.25 * (pick - start)).astype(f32)
        q["maxFraction"], q["maskBits"] = 1.0, ALL
    elif mode.startswith("probe"):
        q = np.zeros(n, dtype=wire.point_probe_dtype)
        q["p"], q["maskBits"] = (pick + (rng.rand(n, 2) - 0.5) * (np.arange(n) % 2)[:, None]).astype(f32), ALL
    else:
        q = np.zeros(n, dtype=wire.box_query_dtype)
        size = 3.0 * rng.rand(n, 2)
        q["box"], q["maskBits"] = np.concatenate([pick - 0.5 * size, pick + 0.5 * size], axis=1).astype(f32), ALL
    return q


def run(world, mode):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, ns = len(world["bodies"]), len(world["shapes"])
    rng = np.random.RandomState(a.seed)
    ms, answered = [], 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        if mode == "download":
            d_bodies, d_shapes, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(ns, dtype=wire.shape_dtype), np.zeros((nb, 2), dtype=np.float32)
        elif mode == "download_boxes":
            d_boxes = np.zeros(ns, dtype=wire.shape_box_dtype)
        else:
            q = queries(world, mode, rng)
            n = len(q)
            if mode.startswith("ray"):
                hits = np.zeros(n, dtype=wire.ray_hit_dtype)
            else:
                offsets, out, total = np.zeros(n + 1, dtype=np.int32), np.zeros(64 * n + 1024, dtype=np.int32), ctypes.c_int32()
                fn = L.s2amd_world_point_probe if mode.startswith("probe") else L.s2amd_world_query_boxes
        for call in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            if mode == "download":
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, wire.as_ptr(d_shapes), ns, None, wire.as_ptr(d_origins), None))
            elif mode == "download_boxes":
                s._ck(L.s2amd_world_download_boxes(h, wire.as_ptr(d_boxes), ns))
            elif mode.startswith("ray"):
                s._ck(L.s2amd_world_ray_cast(h, wire.as_ptr(q), n, wire.as_ptr(hits)))
            else:
                s._ck(fn(h, wire.as_ptr(q), n, wire.as_ptr(offsets), wire.as_ptr(out), len(out), ctypes.byref(total)))
            if call >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        if mode.startswith("ray"):
            answered = int((hits["shape"] >= 0).sum())
        elif mode not in ("download", "download_boxes"):
            answered = int(total.value)
    ms.sort()
    return {"call_ms_mean": round(sum(ms) / len(ms), 4), "call_ms_median": round(ms[len(ms) // 2], 4), "call_ms_p90": round(ms[(9 * len(ms)) // 10], 4),
            "call_ms_min": round(ms[0], 4), "hits": answered, "bodies": nb, "shape_slots": ns}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    r = run(world_chain.copy_world(world), mode)
    r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "scene_query", "mode": mode, "calls": a.calls,
              "warmup": a.warmup})
    print(json.dumps(r), flush=True)
