"""TEST INFRASTRUCTURE.  The host side of the joint report (solver2d_amd/csrc/joint_report.hip: layout, prepare, enqueue, getters)
on the stand-in HIP runtime of tests/hostcheck: upload -> set_joint_report(all) -> step -> the four getters -> capacity errors ->
upload again, on worlds with and without joints, bodies and joint slots.  Kernels never run there, so the report's contents are
whatever the zeroed "device" block holds; what is checked is that the host code touches only memory it owns (ASan + UBSan).
Run by tests/test_joint_report_host.py in a child process."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from solver2d_amd import hip, synthetic, wire  # noqa: E402
from tests import world_chain  # noqa: E402

E_INVALID, E_STATE, E_CAPACITY = -1, -4, -5


def jointed_world(numi):
    """synthetic.joint_grid with one small box per body that collides with nothing, and a few free joint and contact slots"""
    bodies, contacts, joints = synthetic.joint_grid(numi)
    spare = np.zeros(3, dtype=wire.joint_dtype)
    spare["type"] = wire.JOINT_FREE
    joints = np.concatenate([joints[:5], spare, joints[5:]])
    shapes = np.zeros(len(bodies), dtype=wire.shape_dtype)
    for i, b in enumerate(bodies):
        synthetic._box_shape(shapes[i], i, b["type"], 0.125, 0.125, b["position"][0], b["position"][1], i)
    shapes["maskBits"] = 0
    contacts = np.zeros(4, dtype=wire.contact_dtype)
    contacts["constraintIndex"] = -1
    pairs = np.zeros(4, dtype=wire.pair_state_dtype)
    pairs["shapeA"] = pairs["shapeB"] = -1
    return {"bodies": bodies, "contacts": contacts, "joints": joints, "shapes": shapes, "pairs": pairs,
            "origins": np.ascontiguousarray(bodies["position"], dtype=np.float32).copy()}


def expect(rc, want, what):
    assert rc == want, "%s: rc %d, expected %d" % (what, rc, want)


def drive(world, params, flags_first):
    nj, nb = len(world["joints"]), len(world["bodies"])
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        expect(L.s2amd_world_set_joint_report(h, 8), E_INVALID, "unknown bits")
        expect(L.s2amd_world_set_joint_report(h, -1), E_INVALID, "unknown bits")
        summary = np.zeros(1, dtype=wire.joint_summary_dtype)
        expect(L.s2amd_world_joint_summary(h, wire.as_ptr(summary)), E_STATE, "no resident world")
        if flags_first:
            s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
        if not flags_first:
            s.world_set_joint_report(wire.JOINT_REPORT_ALL)  # prepares on the resident world
        expect(L.s2amd_world_joint_summary(h, wire.as_ptr(summary)), E_STATE, "no step yet")
        for round_ in range(2):
            for _ in range(3):
                s.world_step(params)
                states = s.world_joint_states(expected=1)
                began, ended = s.world_joint_limit_events(expected=1)
                sums = s.world_body_joint_sums()
                s.world_joint_summary()
                assert len(states) <= nj and len(began) <= 2 * nj and len(ended) <= 2 * nj and len(sums) == nb
                count = ctypes.c_int32(-7)
                expect(L.s2amd_world_joint_states(h, None, -1, ctypes.byref(count)), E_INVALID, "negative capacity")
                if nb > 0:
                    out = np.zeros(nb, dtype=wire.body_joint_sum_dtype)
                    expect(L.s2amd_world_body_joint_sums(h, wire.as_ptr(out), nb - 1), E_CAPACITY, "short body-sum array")
                    expect(L.s2amd_world_body_joint_sums(h, wire.as_ptr(out), nb), 0, "body sums")
            # a flag cleared, the others stay; then off and on again between steps
            s.world_set_joint_report(wire.JOINT_REPORT_STATES)
            s.world_step(params)
            s.world_joint_states()
            expect(L.s2amd_world_body_joint_sums(h, None, 0), E_STATE, "flag not set before the last step")
            s.world_set_joint_report(0)
            s.world_step(params)
            expect(L.s2amd_world_joint_summary(h, wire.as_ptr(summary)), E_STATE, "report off")
            s.world_set_joint_report(wire.JOINT_REPORT_ALL)
            # upload again: the flags survive, the block is prepared for the new sizes
            s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
            expect(L.s2amd_world_joint_summary(h, wire.as_ptr(summary)), E_STATE, "no step since the upload")


def main():
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    for flags_first in (True, False):
        drive(jointed_world(6), params, flags_first)
        drive(jointed_world(18), params, flags_first)  # more than one tile of joint slots
        drive(synthetic.pyramid_world(4), params, flags_first)  # no joint slots at all
    small = jointed_world(6)
    big = jointed_world(20)
    with hip.Solver(0) as s:  # a bigger world uploaded over a smaller one: the block grows
        s.world_set_joint_report(wire.JOINT_REPORT_ALL)
        for world in (small, big, small):
            s.world_upload(*[world[k] for k in world_chain.WORLD_KEYS])
            s.world_step(params)
            s.world_joint_states(), s.world_joint_limit_events(), s.world_body_joint_sums(), s.world_joint_summary()
    print("JOINT REPORT DRIVER OK", flush=True)


if __name__ == "__main__":
    main()
