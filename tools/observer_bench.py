#!/usr/bin/env python3
"""What the observers cost, and what they replace.  The standing base-N pyramid (20,101 bodies at base 200) under TGS_Soft 8/4, uploaded
and stepped `--settle` times, with 1 / 64 / 4,096 / 16,384 observers on random bricks -- kinds 1-5 in turn, every second one in another
brick's frame, and every sixth a BODY_CONTACT with the contact report's body sums on -- and a history of 1 or 8 frames; the vector goes
into a device buffer the caller owns, as a policy's input would.  Per mode `--steps` rounds after `--warmup`, each timed on the host
from the first call to the return of the last, which waits for the device:

    step0          s2amd_world_step alone, no list set, s2amd_synchronize: what the parent commit's step is compared to (the only mode a
                   tree without the observer API can run)
    step_idle      the same with a list of 16,384 observers set and the report flags at 0
    step_sums      the step with the contact report's body sums on and no observers: what the observers' own cost is read against
    device         the body sums on: s2amd_world_step, s2amd_world_export_observations_async, s2amd_export_wait
    host_route     the route replaced: the step with the body report's states and the contact report's body sums on,
                   s2amd_world_body_states, s2amd_world_body_sums, the arithmetic vectorised in numpy (float32, arctan2 for the angles),
                   s2amd_device_write of the vector

The pyramid has no joints: kinds 6-8, and the joint-report read-back their host route needs, are not measured here.
One JSON object per line on standard output; profiles/observers.jsonl is this output, run by run.

    python tools/observer_bench.py --tree . --label this [--rep N] [--modes step0,device] [--observers 1,64,4096,16384] [--frames 1,8] [--base 200]

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
ap.add_argument("--modes", default="step0,step_idle,step_sums,device,host_route")
ap.add_argument("--observers", default="1,64,4096,16384")
ap.add_argument("--frames", default="1,8")
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
HAVE_OBSERVERS = hasattr(wire, "observer_dtype")
f32 = np.float32


def make_observers(world, count, rng):
    """-> (list, channels)"""
    bricks = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)
    out = np.zeros(count, dtype=wire.observer_dtype)
    k = np.arange(count)
    out["kind"] = np.where(k % 6 == 5, wire.OBSERVER_BODY_CONTACT, 1 + k % 5)
    out["target"] = bricks[rng.randint(len(bricks), size=count)]
    out["frame"] = np.where((k % 2 == 1) & (out["kind"] <= 5), bricks[rng.randint(len(bricks), size=count)], -1)
    out["flags"] = np.where(k % 4 == 3, wire.OBSERVER_RELATIVE, 0)
    widths = np.array([wire.OBSERVER_WIDTH[int(x)] for x in out["kind"]])
    out["channel"] = np.concatenate([[0], np.cumsum(widths)[:-1]])
    out["gain"], out["bias"], out["lower"], out["upper"], out["local"] = 0.5, 0.1, -10.0, 10.0, (0.25, -0.25)
    return out, int(widths.sum())


def host_vector(o, widths, channels, states, sums, row_of_body):
    """The vector of the host route from s2amd_world_body_states' records and s2amd_world_body_sums: vectorised float32"""
    t, fr = states[row_of_body[o["target"]]], states[row_of_body[np.maximum(o["frame"], 0)]]
    framed, relative = o["frame"] >= 0, (o["frame"] >= 0) & ((o["flags"] & wire.OBSERVER_RELATIVE) != 0)
    ts, tc, fs, fc = t["rot"][:, 0], t["rot"][:, 1], np.where(framed, fr["rot"][:, 0], f32(0)), np.where(framed, fr["rot"][:, 1], f32(1))
    fo = np.where(framed[:, None], fr["origin"], f32(0))
    px = (tc * o["local"][:, 0] - ts * o["local"][:, 1]) + t["origin"][:, 0] - fo[:, 0]
    py = (ts * o["local"][:, 0] + tc * o["local"][:, 1]) + t["origin"][:, 1] - fo[:, 1]
    qs, qc = fc * ts - fs * tc, fc * tc + fs * ts
    v = t["linearVelocity"] - np.where(relative[:, None], fr["linearVelocity"], f32(0))
    w = t["angularVelocity"] - np.where(relative, fr["angularVelocity"], f32(0))
    kind = o["kind"]
    x0 = np.select([kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [fc * px + fs * py, qs, np.arctan2(qs, qc), fc * v[:, 0] + fs * v[:, 1], w],
                   (sums["touching"][o["target"]] > 0).astype(f32))
    x1 = np.select([kind == 1, kind == 2, kind == 4], [fc * py - fs * px, qc, fc * v[:, 1] - fs * v[:, 0]], sums["normalImpulse"][o["target"]])
    y0 = np.clip(o["gain"] * x0 + o["bias"], o["lower"], o["upper"]).astype(f32)
    y1 = np.clip(o["gain"] * x1 + o["bias"], o["lower"], o["upper"]).astype(f32)
    out = np.zeros(channels, dtype=f32)
    out[o["channel"]] = y0
    wide = widths == 2
    out[o["channel"][wide] + 1] = y1[wide]
    return out


def run(world, mode, count, frames):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    ms, observed, channels = [], 0, 0
    nb = len(world["bodies"])
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        buf = 0
        if mode not in ("step0", "step_sums"):
            rng = np.random.RandomState(a.seed)
            observers, channels = make_observers(world, count, rng)
            widths = np.array([wire.OBSERVER_WIDTH[int(x)] for x in observers["kind"]])
            buf = s.device_alloc(4 * channels * frames)
            if mode != "host_route":
                s.world_set_observers(observers, channels, frames)
        if mode in ("step_sums", "device", "host_route"):
            s.world_set_report(wire.REPORT_BODY_SUMS)
        if mode == "device":
            s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        if mode == "host_route":
            s.world_set_body_report(wire.BODY_REPORT_STATES)
            states, n = np.zeros(nb, dtype=wire.body_state_dtype), ctypes.c_int32()
            sums = np.zeros(nb, dtype=wire.body_contact_sum_dtype)
            row_of_body = np.zeros(nb, dtype=np.int64)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if mode in ("step0", "step_idle", "step_sums"):
                s._ck(L.s2amd_synchronize(h))
            elif mode == "device":
                s._ck(L.s2amd_world_export_observations_async(h, ctypes.c_void_p(buf), channels * frames, 0))
                s._ck(L.s2amd_export_wait(h, 0))
            else:
                s._ck(L.s2amd_world_body_states(h, wire.as_ptr(states), nb, ctypes.byref(n)))
                s._ck(L.s2amd_world_body_sums(h, wire.as_ptr(sums), nb))
                got = states[: n.value]
                row_of_body[got["slot"]] = np.arange(n.value)
                vector = host_vector(observers, widths, channels, got, sums, row_of_body)
                s._ck(L.s2amd_device_write(h, ctypes.c_void_p(buf), wire.as_ptr(vector), vector.nbytes))
            dt = 1e3 * (time.perf_counter() - t0)
            if step >= a.warmup:
                ms.append(dt)
        if mode == "device":
            observed = int(s.world_observer_counts()[0])
        if buf:
            s.device_free(buf)
    ms.sort()
    return {"ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_p90": round(ms[(9 * len(ms)) // 10], 4), "ms_min": round(ms[0], 4),
            "observed": observed, "channels": channels, "bodies": nb}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    assert mode in ("step0", "step_sums") or HAVE_OBSERVERS, mode
    fixed = mode in ("step0", "step_sums", "step_idle")
    for count in ([0] if mode in ("step0", "step_sums") else [16384] if mode == "step_idle" else [int(x) for x in a.observers.split(",")]):
        for frames in ([1] if fixed or mode == "host_route" else [int(x) for x in a.frames.split(",")]):
            r = run(world_chain.copy_world(world), mode, count, frames)
            r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "observers", "mode": mode, "observers": count,
                      "frames": frames, "steps": a.steps, "warmup": a.warmup})
            print(json.dumps(r), flush=True)
