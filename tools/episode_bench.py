#!/usr/bin/env python3
"""What the episodes cost, and what they replace.  The standing base-N pyramid (20,101 bodies at base 200) under TGS_Soft 8/4, uploaded
and stepped `--settle` times, with 256 observers of kinds 1-5 on random bricks over 2 frames, and 1 / 64 / 4,096 / 16,384 agents of 4 rules
each on those channels -- a progress reward (a DIFFERENCE against frame 1), a squared penalty, an alive bonus (REWARD_TEST) and a
TERMINATE | OUTSIDE rule -- with a time limit of 200 steps; rewards and flags go into device buffers the caller owns, as a learner's
input would.  Per mode `--steps` rounds after `--warmup`, each timed on the host from the first call to the return of the last, which
waits for the device:

    step0          s2amd_world_step alone, no list set, s2amd_synchronize: what the parent commit's step is compared to (the only mode a
                   tree without the episode API can run)
    step_idle      the same with 16,384 agents of 4 rules set and the episode report flags at 0
    step_obs       the step with the observers on and their vector exported (s2amd_world_export_observations_async, s2amd_export_wait)
                   and no episodes: what the episodes' own cost is read against
    device         the same plus s2amd_world_export_episode_step_async behind the observations' export, one s2amd_export_wait
    host_route     the route replaced: the step with the observers on, s2amd_world_observations to the host, the rules vectorised in
                   numpy (float32), the counters (length, return, episodes, time limit) on the host, two s2amd_device_write calls

One JSON object per line on standard output; profiles/episodes.jsonl is this output, run by run.

    python tools/episode_bench.py --tree . --label this [--rep N] [--modes step0,device] [--agents 1,64,4096,16384] [--base 200] [--events]

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
ap.add_argument("--modes", default="step0,step_idle,step_obs,device,host_route")
ap.add_argument("--agents", default="1,64,4096,16384")
ap.add_argument("--base", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--events", action="store_true", help="device mode: S2AMD_EPISODE_REPORT_EVENTS on as well (the third kernel)")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(a.tree)), hip.__file__
SOLVER = "TGS_Soft"
HAVE_EPISODES = hasattr(wire, "episode_rule_dtype")
OBSERVERS, FRAMES, LIMIT = 256, 2, 200
f32 = np.float32


def make_observers(world, rng):
    """-> (list, channels): kinds 1-5 in turn on random bricks, every second one in another brick's frame"""
    bricks = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)
    out = np.zeros(OBSERVERS, dtype=wire.observer_dtype)
    k = np.arange(OBSERVERS)
    out["kind"] = 1 + k % 5
    out["target"] = bricks[rng.randint(len(bricks), size=OBSERVERS)]
    out["frame"] = np.where(k % 2 == 1, bricks[rng.randint(len(bricks), size=OBSERVERS)], -1)
    widths = np.array([wire.OBSERVER_WIDTH[int(x)] for x in out["kind"]])
    out["channel"] = np.concatenate([[0], np.cumsum(widths)[:-1]])
    out["gain"], out["bias"], out["lower"], out["upper"], out["local"] = 0.5, 0.1, -10.0, 10.0, (0.25, -0.25)
    return out, int(widths.sum())


def make_rules(agents, channels):
    """4 rules per agent, one agent's rules adjacent in the list"""
    r = np.zeros(4 * agents, dtype=wire.episode_rule_dtype)
    k = np.arange(4 * agents)
    r["agent"], r["channelA"] = k // 4, (7 * k) % channels
    which = k % 4
    r["kind"] = np.select([which == 0, which == 1, which == 2], [wire.EPISODE_REWARD_VALUE, wire.EPISODE_REWARD_VALUE, wire.EPISODE_REWARD_TEST], wire.EPISODE_TERMINATE)
    r["shape"] = np.where(which == 1, wire.EPISODE_SHAPE_SQUARE, np.where(which == 3, wire.EPISODE_SHAPE_ABS, wire.EPISODE_SHAPE_LINEAR))
    r["flags"] = np.where(which == 0, wire.EPISODE_RULE_DIFFERENCE, np.where(which == 3, wire.EPISODE_RULE_OUTSIDE, 0))
    r["channelB"], r["frameB"] = np.where(which == 0, r["channelA"], 0), np.where(which == 0, 1, 0)
    r["gain"] = np.select([which == 0, which == 1, which == 2], [10.0, -0.01, 0.05], -1.0)
    r["lower"] = np.select([which == 0, which == 1, which == 2], [-1.0, -1.0, -5.0], 0.0)
    r["upper"] = np.select([which == 0, which == 1, which == 2], [1.0, 0.0, 5.0], 9.0)
    return r


def host_step(obs, r, agents, limits, acc):
    """The rules of the host route, vectorised float32, and the counters -> (rewards, flags)"""
    x = obs[r["frameA"], r["channelA"]]
    difference = (r["flags"] & wire.EPISODE_RULE_DIFFERENCE) != 0
    x = np.where(difference, x - obs[r["frameB"], r["channelB"]], x)
    f = np.select([r["shape"] == wire.EPISODE_SHAPE_ABS, r["shape"] == wire.EPISODE_SHAPE_SQUARE], [np.abs(x), x * x], x)
    test = ((r["lower"] <= f) & (f <= r["upper"])) != ((r["flags"] & wire.EPISODE_RULE_OUTSIDE) != 0)
    ending = r["kind"] >= wire.EPISODE_TERMINATE
    y = np.select([r["kind"] == wire.EPISODE_REWARD_VALUE, r["kind"] == wire.EPISODE_REWARD_TEST],
                  [np.clip(r["gain"] * f + r["bias"], r["lower"], r["upper"]), np.where(test, r["gain"], r["bias"])], np.where(test, r["gain"], f32(0)))
    rewards = y.astype(f32).reshape(agents, 4).sum(axis=1, dtype=f32)
    fired = (test & ending).reshape(agents, 4)
    flags = np.where(fired.any(axis=1), 1, 0).astype(np.int32)
    restart = (acc["flags"] & 3) != 0
    acc["length"] = np.where(restart, 0, acc["length"]) + 1
    flags |= np.where((limits > 0) & (acc["length"] >= limits), 6, 0).astype(np.int32)
    acc["return"] = np.where(restart, f32(0), acc["return"]) + rewards
    acc["episodes"] += (flags & 3) != 0
    acc["flags"] = flags
    return rewards, flags


def run(world, mode, agents):
    params = wire.StepParams.make(SOLVER, 1.0 / 60.0, 8, 4, True)
    ms, evaluated, done = [], 0, 0
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        s.set_option("prebuild_solver", wire.SOLVER_ID[SOLVER])
        obs_buf = reward_buf = flag_buf = 0
        channels = 0
        if mode != "step0":
            rng = np.random.RandomState(a.seed)
            observers, channels = make_observers(world, rng)
            obs_buf = s.device_alloc(4 * channels * FRAMES)
        if mode in ("step_obs", "device", "host_route"):
            s.world_set_observers(observers, channels, FRAMES)
            s.world_set_observation_report(wire.OBSERVATION_REPORT_VECTOR)
        if mode in ("step_idle", "device", "host_route"):
            rules = make_rules(agents, channels)
            limits = np.full(agents, LIMIT, dtype=np.int32)
            reward_buf, flag_buf = s.device_alloc(4 * agents), s.device_alloc(4 * agents)
        if mode in ("step_idle", "device"):
            s.world_set_episodes(rules, agents, limits)
        if mode == "device":
            s.world_set_episode_report(wire.EPISODE_REPORT_STEP | (wire.EPISODE_REPORT_EVENTS if a.events else 0))
        if mode == "host_route":
            obs, n = np.zeros((FRAMES, channels), dtype=f32), ctypes.c_int32()
            acc = {"flags": np.zeros(agents, dtype=np.int32), "length": np.zeros(agents, dtype=np.int32), "return": np.zeros(agents, dtype=f32),
                   "episodes": np.zeros(agents, dtype=np.int32)}
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        for _ in range(a.settle):
            s.world_step(params)
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            s.world_step(params)
            if mode in ("step0", "step_idle"):
                s._ck(L.s2amd_synchronize(h))
            elif mode in ("step_obs", "device"):
                s._ck(L.s2amd_world_export_observations_async(h, ctypes.c_void_p(obs_buf), channels * FRAMES, 0))
                if mode == "device":
                    s._ck(L.s2amd_world_export_episode_step_async(h, ctypes.c_void_p(reward_buf), ctypes.c_void_p(flag_buf), agents, 0))
                s._ck(L.s2amd_export_wait(h, 0))
            else:
                s._ck(L.s2amd_world_observations(h, wire.as_ptr(obs.reshape(-1)), obs.size, ctypes.byref(n)))
                rewards, flags = host_step(obs, rules, agents, limits, acc)
                s._ck(L.s2amd_device_write(h, ctypes.c_void_p(reward_buf), wire.as_ptr(rewards), rewards.nbytes))
                s._ck(L.s2amd_device_write(h, ctypes.c_void_p(flag_buf), wire.as_ptr(flags), flags.nbytes))
            dt = 1e3 * (time.perf_counter() - t0)
            if step >= a.warmup:
                ms.append(dt)
        if mode == "device":
            counts = s.world_episode_counts()
            evaluated, done = int(counts[0]), int(counts[4])
        for buf in (obs_buf, reward_buf, flag_buf):
            if buf:
                s.device_free(buf)
    ms.sort()
    return {"ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_p90": round(ms[(9 * len(ms)) // 10], 4), "ms_min": round(ms[0], 4),
            "evaluated": evaluated, "done": done, "channels": channels, "bodies": len(world["bodies"])}


world = synthetic.pyramid_world(a.base)
for mode in a.modes.split(","):
    assert mode == "step0" or HAVE_EPISODES, mode
    for agents in ([0] if mode in ("step0", "step_obs") else [16384] if mode == "step_idle" else [int(x) for x in a.agents.split(",")]):
        r = run(world_chain.copy_world(world), mode, agents)
        r.update({"tree": a.label, "rep": a.rep, "world": "pyramid base %d" % a.base, "solver": SOLVER, "bench": "episodes", "mode": mode, "agents": agents,
                  "rules": 4 * agents, "events": bool(a.events and mode == "device"), "steps": a.steps, "warmup": a.warmup})
        print(json.dumps(r), flush=True)
