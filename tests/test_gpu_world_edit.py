"""World edits on the resident world (s2amd_world_edit; solver2d_amd/csrc/world_edit.hip) against their statement (tests/world_edit_ref.py:
numpy, pinned to the compiled reference's own setters by tests/test_world_edit_host.py): the resident bodies and joints after a call equal
the statement applied to the arrays before it byte for byte, every other array is untouched, and a chain of edited steps equals the
oracle chain of tests/world_chain.py with the statement applied before each step.  The worlds are the committed
tests/golden/world_*_step*.npz (6-211 body slots; free, static, kinematic and dynamic slots; mouse and revolute joints); one case needs
more targets than any of them has and takes a synthetic pyramid (see test_order_on_one_target)."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import body_report_ref, world_chain, world_edit_ref as ref
from tests.body_report_world import assert_body_report_equals_reference, thresholds_of
from tests.resident import E_INVALID, E_STATE, OTHER_KEYS, assert_metrics_equal_reference, assert_same_world, download, slots_of, step_both, upload
from tests.world_chain import golden

pytestmark = pytest.mark.gpu

STEPS = 12


def edit_both(s, ref_world, edits, what, want_skipped=True):
    """One s2amd_world_edit and the statement on the reference arrays; the skip counts agree."""
    skipped = s.world_edit(edits, want_skipped=want_skipped)
    want = ref.apply(ref_world["bodies"], ref_world["joints"], edits)
    assert skipped == (want if want_skipped else None), "%s: %s edits skipped, the statement skips %d" % (what, skipped, want)
    return want


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
def test_every_kind_once_on_distinct_targets(fast):
    """mixed24_PGS: the eight kinds on eight targets (a velocity on the static body among them: kinds 1-3 write whatever the type is) --
    bodies and joints equal the statement, everything else what was uploaded; the same bits from the tolerance-mode library."""
    _, world = golden("mixed24_PGS")
    at = slots_of(world)
    assert len(at["static"]) and len(at["kinematic"]) and len(at["dynamic"]) >= 2 and len(at["revolute"]) >= 3 and len(at["mouse"]), at
    d0, d1 = int(at["dynamic"][0]), int(at["dynamic"][-1])
    p = world["bodies"]["position"][d1]
    edits = wire.edit_list([
        wire.edit_revolute_set_motor_speed(at["revolute"][2], -1.75), wire.edit_set_linear_velocity(at["static"][0], (0.25, -0.5)),
        wire.edit_apply_linear_impulse(d1, (0.3, 1.1), (p[0] + 0.2, p[1] - 0.1)), wire.edit_mouse_set_target(at["mouse"][0], (1.5, 2.5)),
        wire.edit_set_angular_velocity(at["kinematic"][0], 0.7), wire.edit_revolute_enable_limit(at["revolute"][0], 1),
        wire.edit_apply_force_to_center(d0, (3.0, -4.0)), wire.edit_revolute_enable_motor(at["revolute"][1], 1)])
    with hip.Solver(0, fast=fast) as s:
        upload(s, world)
        before, status0 = download(s, world)
        assert_same_world(before, world, "upload")
        want = world_chain.copy_world(world)
        assert edit_both(s, want, edits, "mixed24") == 0
        got, status = download(s, world)
        assert_same_world(got, want, "mixed24 after the edits", ("bodies", "joints"))
        assert_same_world(got, world, "mixed24 after the edits", OTHER_KEYS)
        assert status.tobytes() == status0.tobytes()
        assert got["bodies"].tobytes() != world["bodies"].tobytes() and got["joints"].tobytes() != world["joints"].tobytes()
        assert got["bodies"]["linearVelocity"][at["static"][0]].tolist() == [0.25, -0.5]


def test_order_on_one_target():
    """The order of the edits on one target, to the bit.  The implementation does not chunk a list.
    (a) 5,000 random edits over all 42 body and 13 joint slots of mixed24 (free slots and joints of the other type among them): every
        target many times, sets and applies interleaved.
    (b) 1,500 force adds of different values and 300 impulses, shuffled, on one body.
    (c) 1,024 edits on distinct targets -- the one-lane-per-edit path, four full workgroups -- then the same list with one more edit on
        its first target: 1,025 edits, the sorted path, one lane into a fifth workgroup.  No committed world has 1,024 slots: a
        base-45 pyramid (1,036 body slots) stands in for this case alone."""
    _, world = golden("mixed24_PGS")
    nb, nj = len(world["bodies"]), len(world["joints"])
    assert (nb, nj) == (42, 13)
    rng = np.random.RandomState(5)
    with hip.Solver(0) as s:
        upload(s, world)
        want = world_chain.copy_world(world)
        everything = ref.random_edits(rng, world["bodies"], world["joints"], 5000, np.arange(nb), np.arange(nj), np.arange(nj))
        assert len(set(zip((everything["kind"] >= 5).tolist(), everything["target"].tolist()))) == nb + nj
        assert edit_both(s, want, everything, "5,000 edits") > 0
        got, _ = download(s, world)
        assert_same_world(got, want, "5,000 edits", ("bodies", "joints"))
        assert_same_world(got, world, "5,000 edits", OTHER_KEYS)

        body = int(slots_of(world)["dynamic"][3])
        one = ref.random_edits(rng, world["bodies"], world["joints"], 1800, [body], kinds=[wire.EDIT_BODY_APPLY_FORCE_TO_CENTER])
        one["kind"][rng.permutation(1800)[:300]] = wire.EDIT_BODY_APPLY_LINEAR_IMPULSE
        assert (one["kind"] == wire.EDIT_BODY_APPLY_LINEAR_IMPULSE).sum() == 300 and len(np.unique(one["v"][:, 0])) >= 1790
        assert edit_both(s, want, one, "1,800 edits on one body") == 0
        got, _ = download(s, world)
        assert_same_world(got, want, "1,800 edits on one body", ("bodies", "joints"))
        # (the sums are order-dependent in this very list: the statement on the reversed list gives other bits)
        other = world_chain.copy_world(world)
        ref.apply(other["bodies"], other["joints"], everything)
        ref.apply(other["bodies"], other["joints"], one[::-1])
        assert other["bodies"][body].tobytes() != want["bodies"][body].tobytes()

    big = synthetic.pyramid_world(45)
    live = np.flatnonzero(big["bodies"]["type"] != wire.BODY_FREE)
    assert len(live) >= 1024
    distinct = ref.random_edits(rng, big["bodies"], big["joints"], 1024, kinds=[1, 2, 3, 4])
    distinct["target"] = rng.permutation(live)[:1024]
    again = wire.edit_apply_linear_impulse(distinct["target"][0], (0.5, -0.25), (0.0, 1.0))
    repeated = np.concatenate([distinct, wire.edit_list([again])])
    assert len(repeated) == 1025
    with hip.Solver(0) as s:
        upload(s, big)
        want = world_chain.copy_world(big)
        for edits, what in ((distinct, "1,024 distinct"), (repeated, "1,025 with one repeated")):
            assert edit_both(s, want, edits, what) == 0
            got, _ = download(s, big)
            assert_same_world(got, want, what, ("bodies", "joints"))
            assert_same_world(got, big, what, OTHER_KEYS)


def chain_edits(style, world, rng, step):
    """The edits of one step of a chain, from the oracle's world as it stands.  Velocities are set on dynamic and kinematic bodies only."""
    b, j = world["bodies"], world["joints"]
    at = slots_of(world)
    out = []
    if style == "mouse":  # the mouse target moved, the kinematic body's velocity changed
        for m in at["mouse"]:
            out.append(wire.edit_mouse_set_target(m, j["targetA"][m] + np.float32([0.05, 0.02 * (step % 3 - 1)])))
        for k in at["kinematic"]:
            out.append(wire.edit_set_linear_velocity(k, (0.5 * np.cos(0.5 * step), 0.25 * np.sin(0.5 * step))))
            out.append(wire.edit_set_angular_velocity(k, 0.3 * (step % 4) - 0.4))
    elif style == "joints":  # limits and motors switched on and off, motor speeds changed
        for r in at["revolute"][rng.rand(len(at["revolute"])) < 0.5]:
            out.append(wire.edit_revolute_enable_limit(r, rng.randint(2)))
            out.append(wire.edit_revolute_enable_motor(r, rng.randint(2)))
            out.append(wire.edit_revolute_set_motor_speed(r, rng.uniform(-2.0, 2.0)))
    elif style == "drum":  # the drum's motor speed
        motors = at["revolute"][j["enableMotor"][at["revolute"]] != 0]
        assert len(motors)
        for r in motors:
            out.append(wire.edit_revolute_set_motor_speed(r, j["motorSpeed"][r] * np.float32(1.0 + 0.25 * np.sin(step))))
    elif style == "impulses":  # impulses and forces on many bodies; a body may get both, and two impulses
        for d in at["dynamic"][rng.rand(len(at["dynamic"])) < 0.6]:
            for _ in range(rng.randint(1, 3)):
                out.append(wire.edit_apply_linear_impulse(d, b["mass"][d] * rng.uniform(-0.4, 0.4, 2), b["position"][d] + rng.uniform(-0.1, 0.1, 2)))
            if rng.rand() < 0.5:
                out.append(wire.edit_apply_force_to_center(d, b["mass"][d] * rng.uniform(-6.0, 6.0, 2)))
    else:  # "forces": forces and velocities
        for d in at["dynamic"][rng.rand(len(at["dynamic"])) < 0.5]:
            out.append(wire.edit_apply_force_to_center(d, b["mass"][d] * rng.uniform(-6.0, 6.0, 2)))
            if rng.rand() < 0.3:
                out.append(wire.edit_apply_force_to_center(d, b["mass"][d] * rng.uniform(-1.0, 1.0, 2)))
        for d in np.concatenate([at["dynamic"][rng.rand(len(at["dynamic"])) < 0.2], at["kinematic"]]):
            out.append(wire.edit_set_linear_velocity(d, b["linearVelocity"][d] + rng.uniform(-0.3, 0.3, 2).astype(np.float32)))
            out.append(wire.edit_set_angular_velocity(d, b["angularVelocity"][d] + np.float32(rng.uniform(-0.2, 0.2))))
    edits = wire.edit_list(out)
    return edits[rng.permutation(len(edits))] if style in ("impulses", "forces") else edits


def run_edited_chain(s, params, world, style, what, after_step=None):
    """upload -> STEPS x (edit, step) on the device and on the oracle chain; the checks every chain makes.

    The edits cost no structure build.  The issue put that as "structureBuilds after the twelve steps equals structureBuilds after the
    first"; measured, that does not hold for a chain WITHOUT edits either, so it cannot be what an edit costs: the world chain builds once
    more in its second step on every world but Jacobi's (unedited, builds after each step: mixed24_PGS, joint_grid6, pyramid8, shapes_zoo40
    1,2,2,...,2; mixed24_Jacobi 1,1,...,1), and a manifold on a hub body that gains or loses its points rebuilds the structure in that
    step and the next (unedited tumbler60 1,2,2,2,2,2,2,2,2,3,4,4; far_ragdoll_pile0 1,2,3,4,4,4,4,4,5,6,6,7 -- with the edits
    1,2,3,4,4,...,4 and 1,2,3,4,5,5,5,5,6,7,8,9: other contacts flip when bodies are pushed).  What is asserted instead, step by step:
    the edit call itself never changes the count, and from the third step on a step builds only if the contact graph changed in it or in
    the step before (s2amdWorldStepInfo.graphChanged) -- a call that marked the structure stale would build in every step."""
    rng = np.random.RandomState(len(what))
    ref_world = world_chain.copy_world(world)
    upload(s, world)
    builds, changed, edited = [], [], 0
    for step in range(STEPS):
        edits = chain_edits(style, ref_world, rng, step)
        edited += len(edits)
        before = s.stats()["structureBuilds"]
        assert edit_both(s, ref_world, edits, "%s step %d" % (what, step), want_skipped=step % 2 == 0) == 0
        assert s.stats()["structureBuilds"] == before
        changed.append(step_both(s, params, ref_world)["graphChanged"])
        builds.append(s.stats()["structureBuilds"])
        if after_step is not None:
            after_step(step, ref_world)
        got, _ = download(s, world)
        assert not got["bodies"]["force"].any() and not got["bodies"]["torque"].any(), "%s step %d: applied forces left" % (what, step)
        if step % 4 == 3:
            assert_same_world(got, ref_world, "%s step %d" % (what, step), ("bodies",))
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    assert edited >= STEPS, what
    print("%s: structureBuilds after each step %s, graphChanged %s" % (what, builds, changed))
    assert builds[0] == 1 and builds[1] <= 2, (what, builds)
    for step in range(2, STEPS):
        assert builds[step] == builds[step - 1] or changed[step] or changed[step - 1], \
            "%s step %d: a structure build without a change of the contact graph: builds %s, graphChanged %s" % (what, step, builds, changed)
    assert np.isfinite(ref_world["bodies"]["position"]).all(), what
    return ref_world


@pytest.mark.parametrize("name,style", [("mixed24_Jacobi", "mouse"), ("mixed24_PGS", "mouse"), ("joint_grid6_TGS_NGS", "joints"), ("tumbler60_TGS_Soft", "drum"),
                                        ("far_ragdoll_pile0_PGS_Soft", "impulses"), ("pyramid8_TGS_Soft", "forces"), ("shapes_zoo40_PGS_NGS_Block", "forces")])
def test_edited_chains_equal_the_oracle_chain(name, style):
    params, world = golden(name)
    with hip.Solver(0) as s:
        run_edited_chain(s, params, world, style, name)


def test_skipped_edits_write_nothing_and_are_counted():
    _, world = golden("mixed24_PGS")
    at = slots_of(world)
    assert len(at["free"]) and len(at["free_joint"]) and len(at["revolute"]) and len(at["mouse"]), at
    f, fj, r, m = int(at["free"][0]), int(at["free_joint"][0]), int(at["revolute"][0]), int(at["mouse"][0])
    skips = wire.edit_list([wire.edit_set_linear_velocity(f, (1, 2)), wire.edit_set_angular_velocity(f, 3), wire.edit_apply_force_to_center(f, (4, 5)),
                            wire.edit_apply_linear_impulse(f, (1, 1), (0, 0)), wire.edit_mouse_set_target(fj, (1, 1)), wire.edit_revolute_enable_motor(fj, 1),
                            wire.edit_mouse_set_target(r, (1, 1)), wire.edit_revolute_enable_limit(m, 1), wire.edit_revolute_enable_motor(m, 1),
                            wire.edit_revolute_set_motor_speed(m, 2.0)])
    impulses = wire.edit_list([wire.edit_apply_linear_impulse(at["static"][0], (1, 1), (0, 0)), wire.edit_apply_linear_impulse(at["kinematic"][0], (1, 1), (0, 0))])
    with hip.Solver(0) as s:
        upload(s, world)
        for edits, count, what in ((skips, 10, "distinct skips"), (np.concatenate([skips, skips[::-1], skips[:3]]), 23, "repeated skips"),
                                   (impulses, 0, "impulses on a static and a kinematic body"), (np.concatenate([impulses, impulses]), 0, "the same twice")):
            assert s.world_edit(edits) == count, what
            assert ref.apply(world["bodies"].copy(), world["joints"].copy(), edits) == count, what
            assert_same_world(download(s, world)[0], world, what)
            assert s.world_edit(edits, want_skipped=False) is None
            assert_same_world(download(s, world)[0], world, what + ", skipped == NULL")
        # skipped == NULL gives the same world where something is written, too
        mixed = np.concatenate([skips, wire.edit_list([wire.edit_set_angular_velocity(at["dynamic"][0], 2.5), wire.edit_revolute_set_motor_speed(r, 0.5)])])
        want = world_chain.copy_world(world)
        assert ref.apply(want["bodies"], want["joints"], mixed) == 10
        s.world_edit(mixed, want_skipped=False)
        assert_same_world(download(s, world)[0], want, "skipped == NULL")
        assert s.world_edit(mixed) == 10
        assert_same_world(download(s, world)[0], want, "and with the count")


def test_errors_leave_the_world_as_it_was():
    _, world = golden("mixed24_PGS")
    nb, nj = len(world["bodies"]), len(world["joints"])
    at = slots_of(world)
    good = wire.edit_list([wire.edit_set_angular_velocity(at["dynamic"][0], 9.0), wire.edit_revolute_set_motor_speed(at["revolute"][0], 9.0)])
    with hip.Solver(0) as s:
        L, h = s._L, s._h
        skipped = ctypes.c_int32(-7)

        def call(edits, count=None, with_count=True):
            return L.s2amd_world_edit(h, wire.as_ptr(edits) if edits is not None else None, len(edits) if count is None else count,
                                      ctypes.byref(skipped) if with_count else None)

        assert call(good) == E_STATE  # before any upload
        with pytest.raises(hip.S2AmdError):
            s.world_edit(good)
        s.upload(world["bodies"], world["contacts"], world["joints"])
        assert call(good) == E_STATE  # a plain upload: no resident world
        upload(s, world)
        hundred = ref.random_edits(np.random.RandomState(3), world["bodies"], world["joints"], 100)
        bad_lists = []
        for field, value, kind in (("kind", 0, None), ("kind", 9, None), ("kind", -1, None), ("target", -1, 1), ("target", nb, 1), ("target", nb, 4),
                                   ("target", -1, 5), ("target", nj, 5), ("target", nj, 8), ("reserved", 1, None), ("reserved", -1, None)):
            bad = good.copy()
            if kind is not None:
                bad[1]["kind"] = kind
            bad[1][field] = value
            bad_lists.append((bad, (field, value, kind)))
            last = np.concatenate([hundred, bad[1:]])  # 100 valid entries, then the invalid one
            assert len(last) == 101
            bad_lists.append((last, ("after 100 valid", field, value, kind)))
        for bad, what in bad_lists:
            for with_count in (True, False):
                assert call(bad, with_count=with_count) == E_INVALID, what
                assert skipped.value == -7
            assert_same_world(download(s, world)[0], world, str(what))
            with pytest.raises(hip.S2AmdError):
                s.world_edit(bad)
        assert call(good, count=-1) == E_INVALID and call(None, count=2) == E_INVALID
        assert_same_world(download(s, world)[0], world, "bad arguments")
        # a target inside the joint capacity but outside the body capacity is a joint's, and the converse
        # (an edit the last joint slot skips, whatever its type is: the world stays as it was)
        inert = wire.edit_revolute_enable_limit if world["joints"]["type"][nj - 1] == wire.JOINT_MOUSE else wire.edit_mouse_set_target
        assert nb > nj and call(wire.edit_list([inert(nj - 1, (0, 0))])) == 0 and skipped.value == 1
        skipped.value = -7
        assert call(wire.edit_list([inert(nb - 1, (0, 0))])) == E_INVALID and skipped.value == -7
        # count == 0: fine, nothing happens, with and without a list
        assert call(good, count=0) == 0 and skipped.value == 0
        assert call(None, count=0, with_count=False) == 0
        assert s.world_edit(good[:0]) == 0
        assert_same_world(download(s, world)[0], world, "count == 0")
        # ... and the world still takes edits
        want = world_chain.copy_world(world)
        edit_both(s, want, np.concatenate([hundred, good]), "after the errors")
        assert_same_world(download(s, world)[0], want, "after the errors")


def test_an_edited_chain_beside_the_body_report_and_the_step_metrics():
    """far_ragdoll_pile0 with the body report and the step metrics on: both still equal their own statements on the edited oracle chain."""
    params, world = golden("far_ragdoll_pile0_PGS_Soft")
    thresholds = thresholds_of(0.05, params.dt)
    with hip.Solver(0) as s:
        s.world_set_body_report(wire.BODY_REPORT_ALL)
        s.world_set_rest_thresholds(*thresholds)
        s.world_set_metrics(wire.METRICS_ALL, 4)
        state = {}

        def reports(step, ref_world):
            what = "far_ragdoll_pile0 step %d" % step
            assert_body_report_equals_reference(s, state["body"], ref_world, thresholds, params.dt, what)
            assert_metrics_equal_reference(s, ref_world, params, wire.METRICS_ALL, step, what)

        state["body"] = body_report_ref.new_state(world_chain.copy_world(world))
        run_edited_chain(s, params, world, "impulses", "far_ragdoll_pile0 with reports", after_step=reports)
