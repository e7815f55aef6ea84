"""What the parity tests of the raw s2Solve_* calls share (tests/test_gpu_parity.py and the tests built on its gate): one solve against
the oracle swept in the device's own order, bit for bit, the checks on that order, the same for consecutive resident steps, the
narrow phase against a captured reference step, and the made-up solver inputs several of them use.  Test infrastructure only."""
import numpy as np

from solver2d_amd import hip, synthetic, wire
from tests import common, oraclebind


def check_order_is_valid(order, offsets, contacts, bodies, colourless=False):
    """Every active contact appears exactly once; inside one colour batch no dynamic body repeats (s2Solve_Jacobi's contact
    pass writes no body -- solve_jacobi.c:21-132 accumulates per-constraint deltas -- so its sweep is one batch in pool
    order and has no colours to check)."""
    active = np.flatnonzero(contacts["pointCount"] > 0)
    assert sorted(order.tolist()) == active.tolist()
    assert offsets[0] == 0 and offsets[-1] == len(order)
    if colourless:
        return
    movable = (bodies["invMass"] != 0) | (bodies["invI"] != 0)
    for c in range(len(offsets) - 1):
        ids = order[offsets[c]:offsets[c + 1]]
        touched = np.concatenate([contacts["bodyA"][ids], contacts["bodyB"][ids]])
        touched = touched[movable[touched]]
        assert len(np.unique(touched)) == len(touched), "colour %d reuses a dynamic body" % c


def gpu_vs_oracle(solver, params, pre, what):
    got = common.copy3(pre)
    solver.solve(params, *got)
    order, offsets = solver.contact_order()
    jorder, joffsets = solver.joint_order()
    check_order_is_valid(order, offsets, pre[1], pre[0], colourless=params.solverType == wire.SOLVER_ID["Jacobi"])
    want = common.copy3(pre)
    oraclebind.solve(params, *want, contact_order=order, joint_order=jorder)
    common.compare_exact(got, want, what)
    return got


def gpu_vs_oracle_loose(solver, params, pre, what):
    """gpu_vs_oracle for arbitrary inputs: NaN == NaN bitwise is still required, but the colour check
    uses the library's own notion of a writable body (rotated statics count for position solvers)."""
    got = common.copy3(pre)
    solver.solve(params, *got)
    order, offsets = solver.contact_order()
    jorder, _ = solver.joint_order()
    active = np.flatnonzero(pre[1]["pointCount"] > 0)
    assert sorted(order.tolist()) == active.tolist()
    assert offsets[0] == 0 and offsets[-1] == len(order)
    if params.solverType != wire.SOLVER_ID["Jacobi"]:
        # no colour holds two constraints on one body its sweeps write (s2amd_get_writable_bodies: the library's own rule, which for
        # the position passes counts a rotated static body as written -- solve_common.c:383-392)
        writable, _cls = solver.writable_bodies(len(pre[0]))
        a, b = pre[1]["bodyA"][order], pre[1]["bodyB"][order]
        colour = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        touched = np.concatenate([a, b]).astype(np.int64)
        keys = np.concatenate([colour, colour]).astype(np.int64)[writable[touched] != 0] * (len(pre[0]) + 1) + touched[writable[touched] != 0]
        assert len(np.unique(keys)) == len(keys), "%s: a colour holds two constraints on one writable body" % what
    want = common.copy3(pre)
    oraclebind.solve(params, *want, contact_order=order, joint_order=jorder)
    common.compare_exact(got, want, what)
    return got


def resident_vs_oracle(s, params, pre, steps, what, launches=None):
    """`steps` consecutive resident steps, every one compared with the oracle swept in the device's order; returns the final state"""
    s.upload(*pre)
    want = common.copy3(pre)
    seen = []
    for step in range(steps):
        s.step_resident(params)
        order, _ = s.contact_order()
        oraclebind.solve(params, *want, contact_order=order)
        got = common.copy3(pre)
        s.download(*got)
        common.compare_exact(got, want, "%s step %d" % (what, step))
        seen.append(s.stats()["kernelLaunches"])
    if launches is not None:
        assert seen[1:] == [launches] * (steps - 1), seen
    return want


def _resident_states(options, steps, checkpoints, base=120, concurrent=None):
    """Body arrays of a resident base-`base` pyramid after every checkpoint step under `options`."""
    pre = synthetic.pyramid(base)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    out = []
    with hip.Solver(0) as s:
        for k, v in options.items():
            s.set_option(k, v)
        s.set_option("strip_patience", 0)
        s.upload(*pre)
        for step in range(1, steps + 1):
            s.step_resident(params)
            if concurrent is not None:
                concurrent()
            if step in checkpoints:
                b, c, _j = common.copy3(pre)
                s.download(b, c, _j)
                out.append((b.copy(), c["points"].copy()))
        assert s.stats()["persistent"] == options.get("persist", 1)
    return out


def compare_narrowphase(cap, pairs, contacts, status, what):
    post_p, post_c = cap["pairs_post"], cap["contacts_post"]
    live_pre = cap["pairs_pre"]["shapeA"] >= 0
    live_post = post_p["shapeA"] >= 0
    # a contact Stage 3 destroyed is free at solver entry
    assert np.array_equal(status == wire.PAIR_SEPARATED, live_pre & ~live_post), what
    assert np.array_equal(status == wire.PAIR_FREE, ~live_pre), what
    upd = status == wire.PAIR_UPDATED
    for f in ("cacheMetric", "cacheCount", "id", "cacheIndexA", "cacheIndexB", "persisted"):
        a, b = pairs[f][upd], post_p[f][upd]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s: pair field %s" % (what, f)
    for f in ("pointCount", "frictionPersisted", "constraintIndex"):
        assert np.array_equal(contacts[f][upd], post_c[f][upd]), "%s: contact field %s" % (what, f)
    for f in ("normal", "friction"):
        assert np.array_equal(contacts[f][upd].view(np.uint32), post_c[f][upd].view(np.uint32)), "%s: contact field %s" % (what, f)
    got, want = contacts["points"][upd], post_c["points"][upd]
    for f in got.dtype.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s: point field %s" % (what, f)
    return int(upd.sum())


def _with_spare_slots(state, spare):
    b, c, j = state
    free = np.zeros(spare, dtype=wire.contact_dtype)
    free["bodyA"], free["bodyB"], free["constraintIndex"] = -1, -1, -1  # free pool slots as the reference binding packs them
    return b, np.concatenate([c, free]), j


def _artificial_contact(rng, bodies, template, exclude):
    """A two- or one-point manifold between two dynamic boxes that share no contact yet (the geometry is made up: this
    is a solver input, not a scene)."""
    dyn = np.flatnonzero(bodies["type"] == wire.BODY_DYNAMIC)
    while True:
        a, b = (int(x) for x in rng.choice(dyn, size=2, replace=False))
        if (min(a, b), max(a, b)) not in exclude:
            break
    exclude.add((min(a, b), max(a, b)))
    c = template.copy()
    c["bodyA"], c["bodyB"] = a, b
    c["pointCount"] = int(rng.integers(1, 3))
    ang = rng.uniform(0, 2 * np.pi)
    c["normal"] = (np.cos(ang), np.sin(ang))
    c["friction"] = rng.uniform(0.2, 0.9)
    for p in range(2):
        c["points"][p]["localAnchorA"] = rng.uniform(-0.5, 0.5, 2)
        c["points"][p]["localAnchorB"] = rng.uniform(-0.5, 0.5, 2)
        c["points"][p]["separation"] = rng.uniform(-0.02, 0.01)
        c["points"][p]["normalImpulse"] = 0.0
        c["points"][p]["tangentImpulse"] = 0.0
    return c
