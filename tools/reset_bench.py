#!/usr/bin/env python3
"""What the resets cost, and what they replace.  The standing base-N pyramid (20,101 bodies at base 200) under TGS_Soft 8/4, uploaded
and stepped `--settle` times; the boxes form agents of 64 bodies in slot order (315 agents at base 200), the reset pose of a body is its
uploaded pose at rest with a position jitter of 1 mm, and an episode list without rules ends the episode of the first `finishing` agents
in every step (a step limit of 1).  Per mode `--steps` rounds after `--warmup`, each timed on the host from the first call to the return
of the last, which waits for the device:

    step0          s2amd_world_step alone, no list set, s2amd_synchronize: what the parent commit's step is compared to (the only mode a
                   tree without the reset API can run)
    step_idle      the same with the reset list set and the reset flags at 0
    step_pass      the step with the episode report and S2AMD_RESET_ON_EPISODE_END on, `finishing` agents finishing in every step,
                   s2amd_synchronize (finishing 0: the two near-empty launches)
    one_shot       s2amd_world_reset_agents for `finishing` agents and s2amd_synchronize, between steps that are not timed
    host_route     the route replaced: s2amd_world_download of bodies and joints, the writes in numpy, s2amd_world_upload, the first step

One JSON object per line on standard output; profiles/resets.jsonl is this output, run by run.

    python tools/reset_bench.py --tree . --label this [--rep N] [--modes step0,step_idle] [--finishing 0,1,64,all] [--base 200]

--tree: a directory that holds a built `solver2d_amd` package and `tests/world_chain.py` (this checkout: `.`; another commit: an export
of it, built).  Run two trees alternately, several repeats each, in ONE session, so that the run-to-run spread is known before a
difference is read."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=".")
ap.add_argument("--label", default="this")
ap.add_argument("--rep", type=int, default=0)
ap.add_argument("--modes", default="step0,step_idle,step_pass,one_shot,host_route")
ap.add_argument("--finishing", default="0,1,64,all")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
HAVE_RESETS = hasattr(wire, "reset_body_dtype")
PER_AGENT = 64


def make_resets(world):
    """-> (body records, joint records, agents): agents of PER_AGENT boxes in slot order, each box back to its uploaded pose at rest"""
    boxes = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)
    agent_of_body = np.full(len(world["bodies"]), -1, dtype=np.int32)
    agent_of_body[boxes] = np.arange(len(boxes)) // PER_AGENT
    bodies, joints = wire.resets_from_world(world["bodies"], world["joints"], agent_of_body, np.full(len(world["joints"]), -1, dtype=np.int32))
    bodies["linearVelocity"], bodies["angularVelocity"], bodies["positionJitter"] = 0.0, 0.0, 0.001
    return bodies, joints, int(agent_of_body.max()) + 1


def run(world, mode, finishing):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    ms, counts = [], [0] * 8
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        agents = 0
        if mode != "step0":
            bodies, joints, agents = make_resets(world)
            finishing = agents if finishing < 0 else min(finishing, agents)
        if mode in ("step_idle", "step_pass", "one_shot"):
            s.world_set_resets(bodies, joints, agents, seed=7)
        if mode == "step_pass":
            limits = np.zeros(agents, dtype=np.int32)
            limits[:finishing] = 1
            s.world_set_episodes(wire.episode_rule_list([]), agents, limits)
            s.world_set_episode_report(wire.EPISODE_REPORT_STEP)
            s.world_set_reset_report(wire.RESET_ON_EPISODE_END)
        who = np.arange(finishing, dtype=np.int32)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        rounds = a.warmup + a.steps if mode != "host_route" else 5 + max(a.steps // 10, 10)
        warmup = a.warmup if mode != "host_route" else 5
        for step in range(rounds):
            if mode == "one_shot":
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
            t0 = time.perf_counter()
            if mode == "one_shot":
                s.world_reset_agents(who)
                s._ck(L.s2amd_synchronize(h))
            elif mode == "host_route":
                b, j = world["bodies"].copy(), world["joints"].copy()
                s._ck(L.s2amd_world_download(h, wire.as_ptr(b), len(b), None, len(world["contacts"]), wire.as_ptr(j) if len(j) else None, len(j), None,
                                             len(world["shapes"]), None, None, None))
                rows = bodies["body"][bodies["agent"] < finishing]
                for name in ("position", "rot", "linearVelocity", "angularVelocity"):
                    b[name][rows] = bodies[name][bodies["agent"] < finishing]
                b["deltaPosition"][rows], b["force"][rows], b["torque"][rows] = 0.0, 0.0, 0.0
                world["bodies"] = b
                s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
            else:
                s.world_step(params)
                s._ck(L.s2amd_synchronize(h))
            dt = 1e3 * (time.perf_counter() - t0)
            if step >= warmup:
                ms.append(dt)
        if mode in ("step_pass", "one_shot") and finishing >= 0:
            counts = s.world_reset_counts().tolist()
    ms.sort()
    return {"ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_p90": round(ms[(9 * len(ms)) // 10], 4), "ms_min": round(ms[0], 4),
            "agents": agents, "finishing": finishing, "counts": counts, "bodies": len(world["bodies"]), "rounds": len(ms)}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    assert mode == "step0" or HAVE_RESETS, mode
    for f in ([0] if mode in ("step0", "step_idle") else [-1 if x == "all" else int(x) for x in a.finishing.split(",")]):
        if mode in ("one_shot", "host_route") and f == 0:
            continue
        r = run(world_chain.copy_world(world), mode, f)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "resets", "mode": mode, "per_agent": PER_AGENT,
                  "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
