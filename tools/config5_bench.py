#!/usr/bin/env python3
"""BASELINE config 5 (512 x pyramid base-40 in one world, TGS_Soft 8/4) resident on one GPU: the LDS group kernel in its
HBM-bound regime.  Meant to be run under rocprofv3 (kernel trace, FETCH_SIZE / WRITE_SIZE passes):

    python tools/config5_bench.py [--count 512] [--steps 30] [--solver TGS_Soft|SoftStep|PGS_Soft] [--opt wide=0]

--solver: the sibling soft solvers keep the same islands in registers (SoftStep 8/4, PGS_Soft 4/2); --opt wide=0 puts any of the
three back on the 256-thread islandStepKernel (prologue + kernel + epilogue).  The line says which kernel ran (s2amd_get_resident_kernel).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from solver2d_amd import hip, synthetic, wire  # noqa: E402


ITERATIONS = {"TGS_Soft": (8, 4), "SoftStep": (8, 4), "PGS_Soft": (4, 2)}  # (tests/common.py: DEFAULT_ITERS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--solver", default="TGS_Soft", choices=sorted(ITERATIONS))
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    state = synthetic.pyramid(40, count=a.count)
    vel, pos = ITERATIONS[a.solver]
    params = wire.StepParams.make(a.solver, 1.0 / 60.0, vel, pos, True)
    with hip.Solver(0) as gpu:
        for kv in a.opt:
            key, value = kv.split("=")
            gpu.set_option(key, int(value))
        gpu.upload(*state)
        gpu.save_bodies()
        for _ in range(5):
            gpu.restore_bodies()
            gpu.step_resident(params)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            gpu.restore_bodies()
            gpu.step_resident(params)
        ms = 1e3 * (time.perf_counter() - t0) / a.steps
        st = gpu.stats()
        kernel, rounds = gpu.resident_kernel()
    C = len(state[1])
    sweeps = 2 * vel if a.solver != "PGS_Soft" else vel + pos  # solve + relax sweeps of a step
    print(json.dumps({"config": "5: %d x pyramid base-40" % a.count, "solver": a.solver, "options": a.opt, "resident_kernel": kernel, "rounds": rounds, "constraints": C, "bodies": len(state[0]), "ms_per_step": ms,
                      "device_ms": st["deviceMs"], "groups": st["groupCount"], "launches": st["kernelLaunches"],
                      "constraint_iters_per_s": C * sweeps / (ms / 1e3)}))


if __name__ == "__main__":
    main()
