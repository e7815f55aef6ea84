#!/usr/bin/env python3
"""Two builds side by side on worlds of resident islands: BASELINE config 5 (512 and 64 x pyramid base-40) and one island of growing
size (pyramid base 10, 20, 30, 40) under SoftStep, PGS_Soft and TGS_Soft, with the defaults and with option "wide" = 0 -- the timing
loop of tools/solver_table.py (frozen snapshot, steps enqueued back to back, one synchronize).  One JSON object per line.

    python tools/island_kinds_ab.py --tree DIR --label NAME [--rep N] [--what config5,sizes]

--tree: a directory that holds a built `solver2d_amd` package (this checkout: `.`; another commit: an export of it, built).  Run the
two trees alternately, several repeats each, in ONE session, so that the run-to-run spread is known before a difference is read
(profiles/island_kinds_*.jsonl).  A tree older than s2amd_get_resident_kernel reports "resident_kernel": null."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True)
ap.add_argument("--label", required=True)
ap.add_argument("--rep", type=int, default=0)
ap.add_argument("--what", default="config5,sizes")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
IT = {"TGS_Soft": (8, 4), "SoftStep": (8, 4), "PGS_Soft": (4, 2)}


def run(state, solver, opts, steps, warm=8):
    vel, pos = IT[solver]
    params = wire.StepParams.make(solver, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as gpu:
        for k, v in opts.items():
            gpu.set_option(k, v)
        gpu.set_option("strip_patience", 0)
        gpu.upload(*state)
        gpu.save_bodies()
        gpu.set_option("async", 1)
        for _ in range(warm):
            gpu.restore_bodies()
            gpu.step_resident(params)
        gpu.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            gpu.restore_bodies()
            gpu.step_resident(params)
        gpu.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        gpu.set_option("async", 0)
        gpu.restore_bodies()
        gpu.step_resident(params)
        st = gpu.stats()
        k = gpu.resident_kernel() if hasattr(gpu, "resident_kernel") else None
    return {"ms_per_step": round(ms, 5), "device_ms": round(st["deviceMs"], 5), "launches": st["kernelLaunches"], "groups": st["groupCount"],
            "strips": st["stripCount"], "resident_kernel": k}


if "config5" in a.what:
    for count in (512, 64):
        state = synthetic.pyramid(40, count=count)
        for solver in ("SoftStep", "PGS_Soft", "TGS_Soft"):
            for opts in ({}, {"wide": 0}):
                r = run(state, solver, opts, 100)
                r.update({"tree": a.label, "rep": a.rep, "world": "%d x pyramid40" % count, "solver": solver, "opts": opts})
                print(json.dumps(r), flush=True)
if "sizes" in a.what:
    for base in (10, 20, 30, 40):
        state = synthetic.pyramid(base)
        for solver in ("SoftStep", "PGS_Soft", "TGS_Soft"):
            for opts in ({}, {"wide": 0}):
                r = run(state, solver, opts, 200)
                r.update({"tree": a.label, "rep": a.rep, "world": "pyramid%d" % base, "solver": solver, "opts": opts})
                print(json.dumps(r), flush=True)
