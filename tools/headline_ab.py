#!/usr/bin/env python3
"""Builds of the library side by side on the headline (bench.py's flagship workload), run ALTERNATELY, several repeats each, in one
session, so that the run-to-run spread is known before a difference is read (profiles/headline_hoist_ab.jsonl).  One JSON object per
run: ms_per_step, the dominant kernel's us per launch, device ms per step.

    python tools/headline_ab.py --lib parent=PATH/libs2amd.so --lib branch=solver2d_amd/libs2amd.so [--reps 3] [--seconds 150]

A build is a libs2amd.so loaded through S2AMD_LIB (the Python side of two commits that differ in native code only is the same): an
export of another commit built with its own Makefile, or `make -C solver2d_amd/csrc variant NAME=... EXTRA=...` of this one.  Every run
is a process of its own under a time limit; the first one that fails ends the session."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", required=True, help="LABEL=PATH")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seconds", type=int, default=150)
ap.add_argument("--bench", default="--steps 200 --warmup 60 --no-cpu --no-extras --no-fast")
a = ap.parse_args()
libs = [x.split("=", 1) for x in a.lib]
for label, path in libs:
    assert os.path.exists(path), path
for rep in range(a.reps):
    for label, path in libs:
        env = dict(os.environ, S2AMD_LIB=os.path.abspath(path))
        cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.join(ROOT, "bench.py")] + a.bench.split()
        p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit("%s rep %d: exit status %d" % (label, rep, p.returncode))
        d = json.loads(p.stdout.strip().split("\n")[-1])
        print(json.dumps({"build": label, "rep": rep, "ms_per_step": d["ms_per_step"], "avg_launch_us": d["roofline"]["avg_launch_us"],
                          "device_ms_per_step": d["config"]["device_ms_per_step"], "kernel_launches_per_step": d["config"]["kernel_launches_per_step"]}), flush=True)
