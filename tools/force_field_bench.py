#!/usr/bin/env python3
"""What the force fields cost, and what they replace.  The standing base-N pyramid (20,101 shapes at base 200) under TGS_Soft 8/4,
uploaded and stepped `--settle` times, with 1 / 64 / 1,024 point fields of 2-4 m reach at bricks' places (radial, uniform and drag in
turn, as forces of a strength that leaves the pile standing); then per mode `--steps` rounds after `--warmup`, each timed on the host
from the first call to the return of the last, which waits for the device:

    step0            s2amd_world_step alone, no list set: what the parent commit's step is compared to (the only mode a tree without
                     the field API can run)
    oneshot          s2amd_world_apply_fields with states == NULL, then s2amd_synchronize
    oneshot_enqueue  ... without the synchronize: what the caller's thread pays (the device work is still in flight)
    oneshot_states   s2amd_world_apply_fields with the states read back
    persistent       s2amd_world_step with the list set by s2amd_world_set_fields, then s2amd_world_field_states
    host_route       the route replaced: s2amd_world_shapes_in_range for the slots in reach, s2amd_world_download of bodies, shapes and
                     origins, the terms in numpy (directions from the body origins -- cheaper than the witness points the statement
                     uses, so this is a lower bound of the route), s2amd_world_edit, then the step

One JSON object per line on standard output; profiles/force_fields.jsonl is this output, run by run.

    python tools/force_field_bench.py --tree . --label this [--rep N] [--modes step0,persistent] [--fields 1,64,1024] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built).  Run two trees alternately, several repeats each, in ONE session, so that the run-to-run spread is known before a
difference is read."""
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
ap.add_argument("--modes", default="step0,oneshot,oneshot_enqueue,oneshot_states,persistent,host_route")
ap.add_argument("--fields", default="1,64,1024")
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
HAVE_FIELDS = hasattr(wire, "field_dtype")
f32 = np.float32


def make_fields(world, count, rng):
    shapes = world["shapes"]
    bricks = np.flatnonzero(world["bodies"]["type"][shapes["body"]] == wire.BODY_DYNAMIC)
    pick = bricks[rng.randint(len(bricks), size=count)]
    out = np.zeros(count, dtype=wire.field_dtype)
    for i, (f, slot) in enumerate(zip(out, pick)):
        f["count"], f["rot"], f["maskBits"], f["body"] = 1, (0.0, 1.0), 0xFFFFFFFF, -1
        f["position"] = world["origins"][shapes["body"][slot]] + f32((0.1, 0.2))
        f["range"], f["kind"], f["strength"], f["direction"] = 2.0 + 2.0 * rng.rand(), 1 + i % 3, 0.01, (0.6, 0.8)
    return out


def host_terms(fields, offsets, slots, bodies, shapes, origins):
    """The edit list of the host route: one APPLY_FORCE_TO_CENTER per (field, slot in reach on a dynamic body)"""
    edits = []
    for i, f in enumerate(fields):
        mine = slots[offsets[i]:offsets[i + 1]]
        body = shapes["body"][mine]
        keep = bodies["type"][body] == wire.BODY_DYNAMIC
        body = body[keep]
        if len(body) == 0:
            continue
        m = f32(f["strength"])
        if f["kind"] == wire.FIELD_RADIAL:
            d = origins[body] - f["position"]
            n = np.sqrt((d * d).sum(axis=1, keepdims=True))
            g = m * d / np.maximum(n, f32(1e-9))
        elif f["kind"] == wire.FIELD_UNIFORM:
            g = np.broadcast_to(m * f["direction"], (len(body), 2))
        else:
            g = -m * bodies["linearVelocity"][body]
        e = np.zeros(len(body), dtype=wire.world_edit_dtype)
        e["kind"], e["target"] = wire.EDIT_BODY_APPLY_FORCE_TO_CENTER, body
        e["v"][:, :2] = g
        edits.append(e)
    return np.concatenate(edits) if edits else np.zeros(0, dtype=wire.world_edit_dtype)


def run(world, mode, count):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    nb, ns = len(world["bodies"]), len(world["shapes"])
    ms, terms = [], 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        if mode != "step0":
            fields = make_fields(world, count, np.random.RandomState(a.seed))
            states, n = np.zeros(count, dtype=wire.field_state_dtype), ctypes.c_int32()
            if mode == "persistent":
                s.world_set_fields(fields)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        if mode == "host_route":
            d_bodies, d_shapes, d_origins = np.zeros(nb, dtype=wire.body_dtype), np.zeros(ns, dtype=wire.shape_dtype), np.zeros((nb, 2), dtype=f32)
            queries = np.zeros(count, dtype=wire.proximity_query_dtype)
            for name in ("vertices", "count", "radius", "position", "rot", "maskBits"):
                queries[name] = fields[name]
            queries["maxDistance"] = fields["range"]
            capacity = 64 * 1024 * max(1, count // 64)
            offsets, out, total = np.zeros(count + 1, dtype=np.int32), np.zeros(capacity, dtype=np.int32), ctypes.c_int32()
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            if mode in ("step0", "persistent"):
                s.world_step(params)
                if mode == "persistent":
                    s._ck(L.s2amd_world_field_states(h, wire.as_ptr(states), count, ctypes.byref(n)))
            elif mode in ("oneshot", "oneshot_enqueue"):
                s._ck(L.s2amd_world_apply_fields(h, wire.as_ptr(fields), count, None))
                if mode == "oneshot":
                    s._ck(L.s2amd_synchronize(h))
            elif mode == "oneshot_states":
                s._ck(L.s2amd_world_apply_fields(h, wire.as_ptr(fields), count, wire.as_ptr(states)))
            else:
                s._ck(L.s2amd_world_shapes_in_range(h, wire.as_ptr(queries), count, wire.as_ptr(offsets), wire.as_ptr(out), None, len(out), ctypes.byref(total)))
                s._ck(L.s2amd_world_download(h, wire.as_ptr(d_bodies), nb, None, 0, None, 0, wire.as_ptr(d_shapes), ns, None, wire.as_ptr(d_origins), None))
                edits = host_terms(fields, offsets, out, d_bodies, d_shapes, d_origins)
                s._ck(L.s2amd_world_edit(h, wire.as_ptr(edits), len(edits), None))
                s.world_step(params)
                terms = len(edits)
            dt = 1e3 * (time.perf_counter() - t0)
            if mode == "oneshot_enqueue":
                s._ck(L.s2amd_synchronize(h))  # (outside the timed span: the next round starts on an idle device)
            if mode.startswith("oneshot"):
                s.world_step(params)  # (untimed: consumes the forces, so that the sums stay small)
            if step >= a.warmup:
                ms.append(dt)
        if mode == "oneshot":
            s._ck(L.s2amd_world_apply_fields(h, wire.as_ptr(fields), count, wire.as_ptr(states)))
        if mode in ("oneshot", "oneshot_states", "persistent"):
            terms = int(states["terms"].sum())
    ms.sort()
    return {"ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_p90": round(ms[(9 * len(ms)) // 10], 4), "ms_min": round(ms[0], 4),
            "terms": terms, "bodies": nb, "shape_slots": ns}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    assert mode == "step0" or HAVE_FIELDS, mode
    for count in ([0] if mode == "step0" else [int(x) for x in a.fields.split(",")]):
        r = run(world_chain.copy_world(world), mode, count)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "force_fields", "mode": mode, "fields": count,
                  "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
