#!/usr/bin/env python3
"""What the actuators cost, and what they replace.  The standing base-N pyramid (20,101 bodies at base 200) under TGS_Soft 8/4, uploaded
and stepped `--settle` times, with 1 / 64 / 4,096 / 16,384 actuators on distinct bricks (forces and thrusters in turn, of a gain that
leaves the pile standing) and 4,096 actuators on 64 bricks (`4096x64`: targets repeat, the walk); the actions lie in a device buffer the
caller owns, as a policy's output would.  Per mode `--steps` rounds after `--warmup`, each timed on the host from the first call to the
return of the last, which waits for the device:

    step0          s2amd_world_step alone, no list set: what the parent commit's step is compared to (the only mode a tree without the
                   actuator API can run)
    device         s2amd_world_import_actions from the device buffer, s2amd_world_step, s2amd_synchronize
    device_states  ... and s2amd_world_actuator_states
    host_route     the route replaced: s2amd_device_read of the actions, the commands and the terms in numpy, s2amd_world_edit, the step
                   (a thruster's rotation is taken as the identity -- the pile stands -- which spares this route a download of the
                   bodies: a lower bound of the route)

The pyramid has no joints: servos and motor speeds, and the joint-report read-back their host route needs, are not measured here.
One JSON object per line on standard output; profiles/actuators.jsonl is this output, run by run.

    python tools/actuator_bench.py --tree . --label this [--rep N] [--modes step0,device] [--actuators 1,64,4096,16384,4096x64] [--base 200]

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
ap.add_argument("--modes", default="step0,device,device_states,host_route")
ap.add_argument("--actuators", default="1,64,4096,16384,4096x64")
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
HAVE_ACTUATORS = hasattr(wire, "actuator_dtype")
f32 = np.float32


def make_actuators(world, spec, rng):
    """`spec`: "N" (N distinct bricks) or "NxT" (N actuators on T bricks) -> (list, channels)"""
    count, targets = ([int(x) for x in spec.split("x")] + [None])[:2]
    bricks = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)
    pick = rng.permutation(bricks)[:targets or count]
    assert len(pick) == (targets or count), "the world has %d bricks" % len(bricks)
    out = np.zeros(count, dtype=wire.actuator_dtype)
    out["target"] = pick[np.arange(count) % len(pick)]
    out["kind"] = np.where(np.arange(count) % 2 == 0, wire.ACTUATOR_BODY_FORCE, wire.ACTUATOR_BODY_THRUST)
    widths = np.where(out["kind"] == wire.ACTUATOR_BODY_FORCE, 2, 1)
    out["channel"] = np.concatenate([[0], np.cumsum(widths)[:-1]])
    out["gain"], out["bias"], out["lower"], out["upper"], out["axis"] = 0.01, 0.0, -1.0, 1.0, (0.0, 1.0)
    return out, int(widths.sum())


def host_terms(actuators, actions):
    """The edit list of the host route: one APPLY_FORCE_TO_CENTER per actuator"""
    c = actuators["channel"]
    wide = actuators["kind"] == wire.ACTUATOR_BODY_FORCE
    a0, a1 = actions[c], actions[np.where(wide, c + 1, c)]
    u0 = np.clip(actuators["gain"] * a0 + actuators["bias"], actuators["lower"], actuators["upper"])
    u1 = np.clip(actuators["gain"] * a1 + actuators["bias"], actuators["lower"], actuators["upper"])
    e = np.zeros(len(actuators), dtype=wire.world_edit_dtype)
    e["kind"], e["target"] = wire.EDIT_BODY_APPLY_FORCE_TO_CENTER, actuators["target"]
    e["v"][:, 0] = np.where(wide, u0, u0 * actuators["axis"][:, 0])
    e["v"][:, 1] = np.where(wide, u1, u0 * actuators["axis"][:, 1])
    return e


def run(world, mode, spec):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    ms, applied, channels = [], 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        buf = 0
        if mode != "step0":
            rng = np.random.RandomState(a.seed)
            actuators, channels = make_actuators(world, spec, rng)
            count = len(actuators)
            states, n = np.zeros(count, dtype=wire.actuator_state_dtype), ctypes.c_int32()
            host_actions = np.zeros(channels, dtype=f32)
            buf = s.device_alloc(4 * channels)
            s.device_write(buf, rng.uniform(-1.0, 1.0, channels).astype(f32))
            if mode != "host_route":
                s.world_set_actuators(actuators, channels)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            if mode == "step0":
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
            elif mode in ("device", "device_states"):
                s._ck(L.s2amd_world_import_actions(h, ctypes.c_void_p(buf), 0, channels))
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
                if mode == "device_states":
                    s._ck(L.s2amd_world_actuator_states(h, wire.as_ptr(states), count, ctypes.byref(n)))
            else:
                s._ck(L.s2amd_device_read(h, wire.as_ptr(host_actions), ctypes.c_void_p(buf), host_actions.nbytes))
                edits = host_terms(actuators, host_actions)
                s._ck(L.s2amd_world_edit(h, wire.as_ptr(edits), len(edits), None))
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
            dt = 1e3 * (time.perf_counter() - t0)
            if step >= a.warmup:
                ms.append(dt)
        if mode in ("device", "device_states"):
            applied = int(s.world_actuator_counts()[0])
        if buf:
            s.device_free(buf)
    ms.sort()
    return {"ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_p90": round(ms[(9 * len(ms)) // 10], 4), "ms_min": round(ms[0], 4),
            "applied": applied, "channels": channels, "bodies": len(world["bodies"])}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    assert mode == "step0" or HAVE_ACTUATORS, mode
    for spec in (["0"] if mode == "step0" else a.actuators.split(",")):
        r = run(world_chain.copy_world(world), mode, spec)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "actuators", "mode": mode, "actuators": spec,
                  "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
