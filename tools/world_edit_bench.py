#!/usr/bin/env python3
"""What an edit of the resident world costs per call, and what it replaces (the sibling of tools/contact_query_bench.py).  The standing
base-N pyramid (20,101 bodies at base 200) under TGS_Soft 8/4, uploaded and stepped `--settle` times in ONE solver; then `--reps` passes
over the modes, per pass and mode `--calls` timed iterations after `--warmup`, each timed on the host:

    edit1, edit64, edit4096, edit20100             s2amd_world_edit with that many edits on distinct targets and the skip count read
                                                   back: from the call to its return, the edits applied
    edit1_enqueue ... edit20100_enqueue            the same with skipped == NULL: from the call to its return (the edits enqueued); the
                                                   stream is drained outside the timing before the next call
    edit1_enqueue_sync ... edit20100_enqueue_sync  ... and with s2amd_synchronize inside the timing: the edits applied
    sorted4096x64                                  4,096 edits on 64 targets (the sorted path), the skip count read back
    edit64_step                                    one edit call of 64 edits (count read back) and the s2amd_world_step after it
    step                                           the s2amd_world_step alone
    reload_step                                    the route the call replaces: s2amd_world_download of bodies and joints,
                                                   s2amd_world_upload of the whole world, the first s2amd_world_step after it (its
                                                   structure build included); the three parts are also recorded on their own

The edits are the four body kinds in turn with values that leave the standing pyramid as it is (zero velocities, forces and impulses).
One JSON object per line, pass and mode, and one summary line per mode (median and range of the passes' medians).

    python tools/world_edit_bench.py [--reps 3] [--modes edit64,reload_step] [--base 200] > profiles/world_edits.jsonl"""
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

SIZES = (1, 64, 4096, 20100)
DEFAULT = (["edit%d" % n for n in SIZES] + ["edit%d_enqueue" % n for n in SIZES] + ["edit%d_enqueue_sync" % n for n in SIZES] +
           ["sorted4096x64", "edit64_step", "step", "reload_step"])
ap = argparse.ArgumentParser()
ap.add_argument("--modes", default=",".join(DEFAULT))
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reload-calls", type=int, default=15)
ap.add_argument("--reload-warmup", type=int, default=3)
a = ap.parse_args()
SOLVER = "TGS_Soft"


def edit_list(world, n, targets, rng):
    """n edits, the four body kinds in turn, on `targets` distinct dynamic bodies (n of them: all targets distinct)"""
    bodies = world["bodies"]
    dynamic = np.flatnonzero(bodies["type"] == wire.BODY_DYNAMIC)
    chosen = rng.permutation(dynamic)[:min(targets, len(dynamic))]
    e = np.zeros(n, dtype=wire.world_edit_dtype)
    e["kind"] = 1 + np.arange(n) % 4
    e["target"] = chosen[np.arange(n) % len(chosen)] if targets < n else chosen[:n]
    e["v"][:, 2:] = bodies["position"][e["target"]]  # an impulse of zero at the centre of mass
    return e


def timed(call, calls, warmup, between=None):
    ms = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
        if between:
            between()
    return stats(ms)


def stats(ms, prefix="call_ms"):
    ms = sorted(ms)
    return {prefix + "_mean": round(sum(ms) / len(ms), 4), prefix + "_median": round(ms[len(ms) // 2], 4), prefix + "_p90": round(ms[(9 * len(ms)) // 10], 4),
            prefix + "_min": round(ms[0], 4)}


world = synthetic.pyramid_world(a.base)
params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
nb, nc, nj, ns = len(world["bodies"]), len(world["contacts"]), len(world["joints"]), len(world["shapes"])
common = {"world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "world_edit", "calls": a.calls, "warmup": a.warmup, "bodies": nb,
          "contact_slots": nc}
medians = {}
with hip.Solver(0) as s:
    L, h = s._L, s._h
    s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
    s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
    for _ in range(a.settle):
        s.world_step(params)
    info = wire.WorldStepInfo()
    skipped = ctypes.c_int32()

    def step():
        s._ck(L.s2amd_world_step(h, ctypes.byref(params), ctypes.byref(info)))

    for rep in range(a.reps):
        rng = np.random.RandomState(a.seed)
        for mode in a.modes.split(","):
            extra = {}
            if mode == "step":
                r = timed(step, a.calls, a.warmup)
            elif mode == "reload_step":
                host = world_chain.copy_world(world)
                parts = {"download": [], "upload": [], "first_step": [], "total": []}
                for i in range(a.reload_warmup + a.reload_calls):
                    # (outside the timing: the host copies of everything a binding keeps itself, as of now)
                    s.world_download(*[host[k] for k in world_chain.WORLD_KEYS])
                    t0 = time.perf_counter()
                    s._ck(L.s2amd_world_download(h, wire.as_ptr(host["bodies"]), nb, None, 0, wire.as_ptr(host["joints"]), nj, None, 0, None, None, None))
                    t1 = time.perf_counter()
                    host["bodies"]["force"][1] += np.float32(0.0)  # the eight bytes the caller wanted to change
                    s.world_upload(*[host[k] for k in world_chain.WORLD_KEYS])
                    t2 = time.perf_counter()
                    step()
                    t3 = time.perf_counter()
                    if i >= a.reload_warmup:
                        for key, dt in (("download", t1 - t0), ("upload", t2 - t1), ("first_step", t3 - t2), ("total", t3 - t0)):
                            parts[key].append(1e3 * dt)
                r = stats(parts["total"])
                for key in ("download", "upload", "first_step"):
                    extra.update(stats(parts[key], key + "_ms"))
                extra.update(calls=a.reload_calls, warmup=a.reload_warmup, structure_builds=s.stats()["structureBuilds"])
            else:
                kind, _, how = mode.partition("_")
                if kind.startswith("sorted"):
                    n, targets = (int(x) for x in kind[len("sorted"):].split("x"))
                else:
                    n = targets = int(kind[len("edit"):])
                e = edit_list(world, n, targets, rng)
                ptr = wire.as_ptr(e)
                if how == "":
                    r = timed(lambda: s._ck(L.s2amd_world_edit(h, ptr, n, ctypes.byref(skipped))), a.calls, a.warmup)
                elif how == "enqueue":
                    r = timed(lambda: s._ck(L.s2amd_world_edit(h, ptr, n, None)), a.calls, a.warmup, between=s.synchronize)
                elif how == "enqueue_sync":
                    r = timed(lambda: (s._ck(L.s2amd_world_edit(h, ptr, n, None)), s.synchronize()), a.calls, a.warmup)
                else:
                    assert how == "step", mode
                    r = timed(lambda: (s._ck(L.s2amd_world_edit(h, ptr, n, ctypes.byref(skipped))), step()), a.calls, a.warmup)
                    extra.update(structure_builds=s.stats()["structureBuilds"])
                assert skipped.value == 0
                extra.update(edits=n, targets=min(targets, n))
            r.update(common, mode=mode, rep=rep)
            r.update(extra)
            medians.setdefault(mode, []).append(r["call_ms_median"])
            print(json.dumps(r), flush=True)
for mode, m in medians.items():
    print(json.dumps(dict(common, mode=mode, summary="median and range of the passes' medians", reps=len(m), call_ms_median=sorted(m)[len(m) // 2],
                          call_ms_lowest=min(m), call_ms_highest=max(m))), flush=True)
