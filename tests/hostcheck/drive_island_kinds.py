"""TEST INFRASTRUCTURE.  Which kernel the host picks for a world of resident islands only, under the three soft solvers that keep
their islands in registers (TGS_Soft, SoftStep, PGS_Soft), with the defaults and with option "wide" = 0 -- on the stand-in HIP
runtime of tests/hostcheck (kernels never run: the launch count, the group tables and s2amd_get_resident_kernel are host state).
Run by tests/test_wide_island_kinds_host.py in a child process; prints one JSON line per (world, solver, wide) case."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import common  # noqa: E402

WORLDS = [("pyramid10x8", 10, 8), ("pyramid40x4", 40, 4)]
SOLVERS = ["TGS_Soft", "SoftStep", "PGS_Soft"]


def main():
    for name, base, count in WORLDS:
        pre = synthetic.pyramid(base, count=count)
        for solver_name in SOLVERS:
            vel, pos = common.DEFAULT_ITERS[solver_name]
            params = wire.StepParams.make(solver_name, 1.0 / 60.0, vel, pos, True)
            for wide in (1, 0):
                steps = []
                with hip.Solver(0) as s:
                    if not wide:
                        s.set_option("wide", 0)
                    s.upload(*pre)
                    for _ in range(3):
                        s.step_resident(params)
                        st = s.stats()
                        kernel, rounds = s.resident_kernel()
                        steps.append({"kernelLaunches": st["kernelLaunches"], "groupCount": st["groupCount"], "stripCount": st["stripCount"],
                                      "kernel": kernel, "rounds": rounds})
                print("CASE " + json.dumps({"world": name, "solver": solver_name, "wide": wide, "steps": steps}), flush=True)
    print("ISLAND KINDS DRIVER OK", flush=True)


if __name__ == "__main__":
    main()
