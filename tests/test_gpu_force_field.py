"""Force fields on the resident world (s2amd_world_apply_fields / _set_fields / _field_states; solver2d_amd/csrc/force_field.hip)
against their statement (tests/force_field_ref.py: numpy float32 around the compiled reference's own s2ShapeDistance and the statement
of the two setters), byte for byte: the resident bodies after a call, every other array untouched, the states, the route through
s2amd_world_edit that the call replaces, and chains of steps with a persistent list against the oracle chain of tests/world_chain.py
with the statement applied before each step.  The worlds are the committed tests/golden/world_*_step*.npz; one case needs more than
1,024 body slots and takes a synthetic pyramid.  Every case asserts on the statement's own output that its fields act."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import body_report_ref, force_field_ref as ref, sensor_report_ref, world_chain
from tests.body_report_world import assert_body_report_equals_reference, thresholds_of
from tests.force_field_ref import assert_zoo_condition
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, OTHER_KEYS, assert_same_world, download, step_both, upload
from tests.world_chain import golden

pytestmark = pytest.mark.gpu
# (the cases on a committed fixture of tests/golden/force_fields take its recorded distance outputs and run without the compiled reference)
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")

STEPS = 12
IMPULSE, FALLOFF, DISABLED = wire.FIELD_AS_IMPULSE, wire.FIELD_LINEAR_FALLOFF, wire.FIELD_DISABLED


def assert_states(got, want, what):
    assert got.dtype == wire.field_state_dtype and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = [n for n in got.dtype.names if got[n].tobytes() != want[n].tobytes()]
        rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
        raise AssertionError("%s: states differ in %s, first rows %s: %s / %s" % (what, bad, rows[:3].tolist(), got[rows[:2]], want[rows[:2]]))


def apply_both(s, world, fields, what, want_states=True, recorded=None):
    """One s2amd_world_apply_fields on the resident copy of `world` and the statement on `world`: bodies and states equal, every other
    array as it was.  -> (the world after, the statement's states, its term list)"""
    bodies, states, edits = ref.apply(world, fields, recorded=recorded)
    got_states = s.world_apply_fields(fields, want_states=want_states)
    if want_states:
        assert_states(got_states, states, what)
    else:
        assert got_states is None
    want = world_chain.copy_world(world)
    want["bodies"] = bodies
    got, _ = download(s, world)
    assert_same_world(got, want, what, ("bodies",))
    assert_same_world(got, world, what, ("joints",) + OTHER_KEYS)
    return want, states, edits


def mixed_fields(rng, count, centre, spread, reach):
    """`count` overlapping fields of all three kinds and both forms around `centre`"""
    out = []
    for k in range(count):
        kind = (wire.FIELD_RADIAL, wire.FIELD_UNIFORM, wire.FIELD_DRAG)[k % 3]
        flags = (IMPULSE if rng.rand() < 0.5 else 0) | (FALLOFF if rng.rand() < 0.5 else 0)
        strength = rng.uniform(-2.0, 2.0) * (0.05 if kind == wire.FIELD_DRAG else 1.0) * (0.1 if flags & IMPULSE else 1.0)
        out.append(wire.field(kind, centre + rng.uniform(-spread, spread, 2), rng.uniform(0.5 * reach, reach), strength, flags=flags,
                              direction=rng.uniform(-1.0, 1.0, 2), radius=rng.choice([0.0, 0.1])))
    return wire.field_list(out)


def dynamic_centre(world):
    b = world["bodies"]
    return np.median(b["position"][b["type"] == wire.BODY_DYNAMIC], axis=0).astype(np.float32)


@pytest.mark.parametrize("fast", [False, True], ids=["libs2amd", "libs2amd_fast"])
def test_every_kind_in_both_forms_once(fast):
    """shapes_zoo40: radial, uniform and drag, each as a force and as an impulse, with and without falloff, over three overlapping
    regions -- bodies and states equal the statement, everything else is what was uploaded; the same bytes with states == NULL and
    from the tolerance-mode library."""
    _, world = golden("shapes_zoo40_PGS_NGS_Block")
    fields, recorded = ref.load_fixture("shapes_zoo40_PGS_NGS_Block")
    assert fields.tobytes() == ref.zoo_fields().tobytes()
    assert sorted(zip(fields["kind"].tolist(), (fields["flags"] & IMPULSE).tolist())) == [(k, f) for k in (1, 2, 3) for f in (0, IMPULSE)]
    with hip.Solver(0, fast=fast) as s:
        upload(s, world)
        before, status0 = download(s, world)
        assert_same_world(before, world, "upload")
        want, states, edits = apply_both(s, world, fields, "shapes_zoo40", recorded=recorded)
        assert_zoo_condition(world, states, edits)
        assert want["bodies"].tobytes() != world["bodies"].tobytes()
        assert download(s, world)[1].tobytes() == status0.tobytes()
        upload(s, world)
        apply_both(s, world, fields, "shapes_zoo40, states == NULL", want_states=False, recorded=recorded)
        # a second call acts on what the first left (the drag terms read the new velocities; no pose moved, so the distances stand)
        again, _, _ = apply_both(s, want, fields, "shapes_zoo40, second call", recorded=recorded)
        assert again["bodies"].tobytes() != want["bodies"].tobytes()


@needs_reference
def test_order_on_one_body_hundreds_of_terms():
    """(a) ragdoll0 under 300 overlapping fields of mixed kinds: every body takes hundreds of terms, and the statement on the reversed
    list gives other bytes, so an order error cannot pass."""
    _, world = golden("ragdoll0_PGS_NGS_Block")
    fields = mixed_fields(np.random.RandomState(7), 300, dynamic_centre(world), 0.5, 2.5)
    with hip.Solver(0) as s:
        upload(s, world)
        want, states, edits = apply_both(s, world, fields, "ragdoll0, 300 fields")
    per = ref.terms_per_body(world, edits)
    dynamic = world["bodies"]["type"] == wire.BODY_DYNAMIC
    assert per[dynamic].min() >= 200 and (states["terms"] >= 2).sum() >= 250, (per, states["terms"])
    reversed_bodies, _, _ = ref.apply(world, fields[::-1].copy())
    differ = [b for b in np.flatnonzero(dynamic) if reversed_bodies[b].tobytes() != want["bodies"][b].tobytes()]
    assert len(differ) >= 5, differ


@needs_reference
def test_order_on_one_body_four_shapes():
    """(b) tumbler60: the drum is one dynamic body with four shapes, so every field that covers it puts four terms on one body."""
    _, world = golden("tumbler60_TGS_Soft")
    counts = np.bincount(world["shapes"]["body"][world["shapes"]["type"] != wire.SHAPE_FREE], minlength=len(world["bodies"]))
    drum = int(np.argmax(counts))
    assert counts[drum] == 4 and world["bodies"]["type"][drum] == wire.BODY_DYNAMIC
    fields = np.concatenate([ref.fixture_fields("tumbler60_TGS_Soft"), mixed_fields(np.random.RandomState(3), 21, np.float32((0.0, 4.0)), 0.25, 8.0)])
    fields["range"] = np.maximum(fields["range"], 6.5)
    with hip.Solver(0) as s:
        upload(s, world)
        want, states, edits = apply_both(s, world, fields, "tumbler60")
    assert (states["terms"] == 64).all() and np.bincount(edits["target"])[drum] == 4 * len(fields)
    reversed_bodies, _, _ = ref.apply(world, fields[::-1].copy())
    assert reversed_bodies[drum].tobytes() != want["bodies"][drum].tobytes()


@needs_reference
def test_the_maximum_of_fields_crosses_every_chunk():
    """(c) 1,024 fields on mixed24: every staged chunk of the apply pass and the boundaries between them."""
    _, world = golden("mixed24_PGS")
    rng = np.random.RandomState(11)
    fields = mixed_fields(rng, wire.MAX_FIELDS, np.float32((0.0, 3.0)), 8.0, 4.0)
    fields["flags"][rng.permutation(len(fields))[:40]] |= DISABLED
    with hip.Solver(0) as s:
        upload(s, world)
        _, states, edits = apply_both(s, world, fields, "mixed24, 1,024 fields")
    acting = np.flatnonzero(states["terms"] > 0)
    assert len(acting) >= 500 and acting[0] < 8 and acting[-1] >= 1016 and len(edits) >= 2000
    # fields with terms on both sides of every 128-field boundary
    assert all((states["terms"][b - 8:b] > 0).any() and (states["terms"][b:b + 8] > 0).any() for b in range(128, 1024, 128))


@needs_reference
def test_more_bodies_than_four_workgroups():
    """(d) a base-45 pyramid has 1,036 body slots: the apply pass runs a fifth workgroup, whose bodies three fields reach."""
    world = synthetic.pyramid_world(45)
    nb = len(world["bodies"])
    assert nb > 1024
    late = np.flatnonzero(world["bodies"]["type"] == wire.BODY_DYNAMIC)[-1]
    assert late >= 1024
    p = world["bodies"]["position"][late]
    fields = wire.field_list([wire.field_radial(p + np.float32((0.3, 1.0)), 3.0, 5.0, flags=IMPULSE | FALLOFF), wire.field_uniform((0.0, 20.0), 60.0, 2.0, (1.0, 0.5)),
                              wire.field_drag(p, 4.0, 0.5, flags=IMPULSE)])
    world["bodies"]["linearVelocity"][world["bodies"]["type"] == wire.BODY_DYNAMIC] = (0.25, -0.5)
    with hip.Solver(0) as s:
        upload(s, world)
        _, states, edits = apply_both(s, world, fields, "pyramid 45")
    per = ref.terms_per_body(world, edits)
    assert per[1024:].sum() >= 3 and per[late] == 3 and states["terms"][1] >= 1000 and (states["terms"] > 0).all()


def test_the_route_it_replaces():
    """The statement's term list through s2amd_world_edit on a second solver gives the bytes s2amd_world_apply_fields gives on the first;
    and for a uniform field without falloff the slots s2amd_world_shapes_in_range answers, filtered to dynamic bodies, are its terms."""
    _, world = golden("shapes_zoo40_PGS_NGS_Block")
    fields, recorded = ref.load_fixture("shapes_zoo40_PGS_NGS_Block")
    _, states, edits = ref.apply(world, fields, recorded=recorded)
    assert len(edits) >= 72
    with hip.Solver(0) as a, hip.Solver(0) as b:
        upload(a, world), upload(b, world)
        a.world_apply_fields(fields, want_states=False)
        assert b.world_edit(edits) == 0
        got_a, got_b = download(a, world)[0], download(b, world)[0]
        assert_same_world(got_a, got_b, "apply_fields against the edit route")
        assert got_a["bodies"].tobytes() != world["bodies"].tobytes()
        # the device's own proximity query against the device's field: the same slots (and the statement's, where the reference is built)
        wind = wire.field_list([wire.field_uniform((0.0, 2.0), 3.0, 1.0, (1.0, 0.0), vertices=((-1.0, -0.5), (1.0, -0.5), (1.0, 0.5), (-1.0, 0.5)), radius=0.25)])
        upload(a, world)
        offsets, shapes = a.world_shapes_in_range(np.array([ref.as_query(world, wind[0])], dtype=wire.proximity_query_dtype))
        dynamic = world["bodies"]["type"][world["shapes"]["body"][shapes]] == wire.BODY_DYNAMIC
        slots = [int(x) for x in shapes[dynamic]]
        assert 12 <= len(slots) < len(shapes)
        if ref.available():
            assert slots == ref.in_reach(world, wind[0])
        st = a.world_apply_fields(wind)
        assert st["terms"].tolist() == [len(slots)] and st["lowestShape"].tolist() == [slots[0]]
        moved = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(download(a, world)[0]["bodies"], world["bodies"])])
        assert sorted(set(world["shapes"]["body"][slots].tolist())) == moved.tolist()


@needs_reference
def test_attached_and_inactive_fields():
    _, world = golden("mixed24_PGS")
    b = world["bodies"]
    kinematic = int(np.flatnonzero(b["type"] == wire.BODY_KINEMATIC)[0])
    free = int(np.flatnonzero(b["type"] == wire.BODY_FREE)[0])
    # a dynamic body with dynamic neighbours within 1.5
    dyn = np.flatnonzero(b["type"] == wire.BODY_DYNAMIC)
    near = [(int(d), ((np.abs(b["position"][dyn] - b["position"][d]).max(axis=1) < 1.5).sum())) for d in dyn]
    carrier = max(near, key=lambda x: x[1])[0]
    fields = wire.field_list([wire.field_radial((0.0, 0.0), 2.0, -1.5, body=carrier, rot=(0.6, 0.8)),  # a magnet carried by a dynamic body
                              wire.field_uniform((0.5, 0.0), 3.0, 2.0, (0.0, 1.0), body=kinematic, flags=IMPULSE),  # carried by the kinematic body
                              wire.field_uniform((0.0, 0.0), 50.0, 1.0, (1.0, 0.0), body=free),  # on a free slot
                              wire.field_uniform((0.0, 3.0), 50.0, 1.0, (1.0, 0.0), flags=DISABLED),
                              wire.field_drag((100.0, 100.0), 1.0, 1.0)])  # acts on nothing
    with hip.Solver(0) as s:
        upload(s, world)
        want, states, edits = apply_both(s, world, fields, "mixed24 attached")
        assert states["active"].tolist() == [1, 1, 0, 0, 1] and states["terms"][2:].tolist() == [0, 0, 0] and states["terms"][0] >= 2 and states["terms"][1] >= 2
        own = np.flatnonzero(world["shapes"]["body"] == carrier)
        assert len(own) and carrier not in edits["target"][:states["terms"][0]].tolist()  # its own shapes, at distance 0, are excluded
        assert states["rot"][0].tolist() != [0.0, 1.0] and states["position"][1].tolist() != world["origins"][kinematic].tolist()
        # a list that acts on nothing leaves every byte as it was
        upload(s, world)
        nothing, quiet, none = apply_both(s, world, fields[2:], "mixed24, nothing in reach")
        assert len(none) == 0 and nothing["bodies"].tobytes() == world["bodies"].tobytes() and quiet["lowestShape"].tolist() == [-1, -1, -1]


# ---- chains: a persistent list, applied by every step in front of stage 3 ----
def chain_case(name, world):
    """-> (persistent list, {step: one-shot list})"""
    b = world["bodies"]
    c = dynamic_centre(world)
    if name == "shapes_zoo40_PGS_NGS_Block":  # wind with falloff
        return wire.field_list([wire.field_uniform((0.0, 2.0), 6.0, 3.0, (1.0, 0.25), flags=FALLOFF, vertices=((-6.0, 0.0), (6.0, 0.0)), radius=0.5)]), {}
    if name == "tumbler60_TGS_Soft":  # a pull towards the drum's centre
        return wire.field_list([wire.field_radial((0.0, 4.0), 6.0, -4.0)]), {}
    if name == "far_ragdoll_pile0_PGS_Soft":  # a drag pool, and an explosion every fourth step
        blast = wire.field_list([wire.field_radial(c + np.float32((0.1, -0.3)), 1.5, 0.4, flags=IMPULSE | FALLOFF)])
        return wire.field_list([wire.field_drag(c, 1.0, 0.3, vertices=((-1.0, -0.5), (1.0, -0.5), (1.0, 0.5), (-1.0, 0.5)))]), {k: blast for k in range(0, STEPS, 4)}
    if name == "mixed24_Jacobi":  # a field carried by the kinematic body
        kinematic = int(np.flatnonzero(b["type"] == wire.BODY_KINEMATIC)[0])
        return wire.field_list([wire.field_radial((0.0, 0.5), 4.0, 6.0, body=kinematic, flags=FALLOFF), wire.field_drag((0.0, 0.0), 3.0, 0.2, body=kinematic, flags=IMPULSE)]), {}
    assert name == "pyramid8_TGS_Soft"  # an explosion before step 3 only
    return wire.field_list([]), {3: wire.field_list([wire.field_radial((0.25, 1.0), 4.0, 3.0, flags=IMPULSE | FALLOFF)])}


def run_field_chain(s, params, world, persistent, shots, what, after_step=None):
    ref_world = world_chain.copy_world(world)
    s.world_set_fields(persistent)
    upload(s, world)
    builds, changed, terms = [], [], 0
    for step in range(STEPS):
        if step in shots:
            before = s.stats()["structureBuilds"]
            want = ref.apply_in_place(ref_world, shots[step])
            assert_states(s.world_apply_fields(shots[step]), want, "%s step %d, one-shot" % (what, step))
            assert s.stats()["structureBuilds"] == before and want["terms"].sum() > 0
            terms += int(want["terms"].sum())
        want = ref.apply_in_place(ref_world, persistent)
        terms += int(want["terms"].sum())
        changed.append(step_both(s, params, ref_world)["graphChanged"])
        builds.append(s.stats()["structureBuilds"])
        assert_states(s.world_field_states(), want, "%s step %d" % (what, step))
        if after_step is not None:
            after_step(step, ref_world)
        got, _ = download(s, world)
        assert not got["bodies"]["force"].any() and not got["bodies"]["torque"].any(), "%s step %d: applied forces left" % (what, step)
        if step % 4 == 3:
            assert_same_world(got, ref_world, "%s step %d" % (what, step), ("bodies",))
    world_chain.assert_device_equals_oracle(got, ref_world, what)
    assert terms >= STEPS or (len(persistent) == 0 and terms > 0), (what, terms)
    print("%s: structureBuilds after each step %s, graphChanged %s, %d terms" % (what, builds, changed, terms))
    assert builds[0] == 1 and builds[1] <= 2, (what, builds)
    for step in range(2, STEPS):
        assert builds[step] == builds[step - 1] or changed[step] or changed[step - 1], \
            "%s step %d: a structure build without a change of the contact graph: builds %s, graphChanged %s" % (what, step, builds, changed)
    assert np.isfinite(ref_world["bodies"]["position"]).all(), what
    return ref_world


@needs_reference
@pytest.mark.parametrize("name", ["shapes_zoo40_PGS_NGS_Block", "tumbler60_TGS_Soft", "far_ragdoll_pile0_PGS_Soft", "mixed24_Jacobi", "pyramid8_TGS_Soft"])
def test_chains_with_a_persistent_list_equal_the_oracle_chain(name):
    params, world = golden(name)
    persistent, shots = chain_case(name, world)
    with hip.Solver(0) as s:
        after = run_field_chain(s, params, world, persistent, shots, name)
    # the fields changed the chain: the plain oracle chain ends elsewhere
    plain = world_chain.copy_world(world)
    for _ in range(STEPS):
        world_chain.oracle_world_step(params, plain)
    assert plain["bodies"]["position"].tobytes() != after["bodies"]["position"].tobytes()


@needs_reference
def test_a_chain_beside_the_sensor_report_and_the_body_report():
    params, world = golden("shapes_zoo40_PGS_NGS_Block")
    persistent, shots = chain_case("shapes_zoo40_PGS_NGS_Block", world)
    thresholds = thresholds_of(0.05, params.dt)
    sensors = np.zeros(2, dtype=wire.sensor_dtype)
    sensors["count"], sensors["rot"], sensors["maskBits"], sensors["body"] = 1, (0.0, 1.0), 0xFFFFFFFF, -1
    sensors["position"], sensors["margin"] = ((-4.0, 1.0), (5.0, 3.0)), (2.5, 4.0)
    with hip.Solver(0) as s:
        s.world_set_body_report(wire.BODY_REPORT_ALL)
        s.world_set_rest_thresholds(*thresholds)
        s.world_set_sensors(sensors)
        s.world_set_sensor_report(wire.SENSOR_REPORT_INSIDE)
        state = {"body": body_report_ref.new_state(world_chain.copy_world(world)), "held": 0}

        def reports(step, ref_world):
            what = "shapes_zoo40 step %d" % step
            assert_body_report_equals_reference(s, state["body"], ref_world, thresholds, params.dt, what)
            want_offsets, want_shapes = sensor_report_ref.csr(sensor_report_ref.inside_lists(ref_world, sensors))
            offsets, shapes = s.world_sensor_inside()
            assert offsets.tolist() == want_offsets.tolist() and shapes.tolist() == want_shapes.tolist(), what
            state["held"] += len(shapes)

        run_field_chain(s, params, world, persistent, shots, "shapes_zoo40 with reports", after_step=reports)
        assert state["held"] >= STEPS


def test_no_list_no_difference():
    """With the list cleared, and with no list ever set, a chain is the plain oracle chain and field_states answers count 0."""
    params, world = golden("pyramid8_TGS_Soft")
    for cleared in (False, True):
        with hip.Solver(0) as s:
            if cleared:
                s.world_set_fields(ref.zoo_fields())
                s.world_set_fields(wire.field_list([]))
            ref_world = world_chain.copy_world(world)
            upload(s, world)
            for step in range(STEPS):
                step_both(s, params, ref_world)
                assert len(s.world_field_states()) == 0
            world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "pyramid8, cleared %s" % cleared)


def test_errors():
    params, world = golden("mixed24_PGS")
    nb = len(world["bodies"])
    good, recorded = ref.load_fixture("mixed24_PGS")  # (its recorded distances are of the world as uploaded, which the first step's list sees)

    def bad_lists():
        for name, value in (("count", 0), ("count", 9), ("kind", 0), ("kind", 4), ("flags", 8), ("flags", -1), ("reserved", 1), ("radius", -0.5), ("radius", np.nan),
                            ("range", -1.0), ("range", np.inf), ("strength", np.nan), ("strength", np.inf), ("body", nb)):
            wrong = good.copy()
            wrong[name][1] = value  # a bad record in the middle of the list
            yield name, wrong
        for name, index in (("direction", 1), ("position", 0), ("rot", 1), ("vertices", (0, 1))):
            wrong = good.copy()
            wrong[name][1][index] = np.nan
            yield name, wrong

    with hip.Solver(0) as s:
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_apply_fields(good)  # no resident world
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_field_states()
        s.world_set_fields(good)  # accepted before any world
        upload(s, world)
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_field_states()  # no step since the upload
        L, h = s._L, s._h
        many = np.zeros(wire.MAX_FIELDS + 1, dtype=wire.field_dtype)
        many[:] = good[0]
        for call in (lambda p, n: L.s2amd_world_apply_fields(h, p, n, None), lambda p, n: L.s2amd_world_set_fields(h, p, n)):
            assert call(wire.as_ptr(good), -1) == E_INVALID and call(None, 2) == E_INVALID and call(wire.as_ptr(many), len(many)) == E_INVALID
        for name, wrong in bad_lists():
            for call in (s.world_apply_fields, s.world_set_fields):
                with pytest.raises(hip.S2AmdError, match="error %d" % E_INVALID):
                    call(wrong)
        # the world and the old list stand: the next step applies `good`
        assert_same_world(download(s, world)[0], world, "after the refused lists")
        ref_world = world_chain.copy_world(world)
        ref_world["bodies"], want, _ = ref.apply(ref_world, good, recorded=recorded)
        assert want["terms"].sum() >= 6
        step_both(s, params, ref_world)
        assert_states(s.world_field_states(), want, "after the refused lists")
        n = ctypes.c_int32(-7)
        out = np.zeros(3, dtype=wire.field_state_dtype)
        assert L.s2amd_world_field_states(h, wire.as_ptr(out), 2, ctypes.byref(n)) == E_CAPACITY and n.value == 3 and out.tobytes() == bytes(192)
        assert L.s2amd_world_field_states(h, wire.as_ptr(out), -1, ctypes.byref(n)) == E_INVALID
        world_chain.assert_device_equals_oracle(download(s, world)[0], ref_world, "the step after the refused lists")
        s.world_set_fields(good[::-1].copy())
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_field_states()  # no step since the list was set
        assert len(s.world_apply_fields(wire.field_list([]))) == 0  # count == 0 succeeds and does nothing


@needs_reference
def test_a_step_the_library_repeats_applies_the_list_once():
    """The base-100 pyramid stepped by the one-launch kernel with a hand-off that never arrives (option persist_debug 8, as
    tests/test_gpu_strips.py injects it): the library repeats the solve on another path, and the persistent list -- impulses, which a
    second application would add again -- has acted once: the chain equals the oracle chain with the statement applied once a step."""
    world = synthetic.pyramid_world(100)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 8, 4, True)
    top = world["bodies"]["position"][len(world["bodies"]) - 1]
    fields = wire.field_list([wire.field_radial(top + np.float32((0.2, 1.0)), 4.0, 0.5, flags=IMPULSE | FALLOFF), wire.field_drag(top, 3.0, 0.25, flags=IMPULSE),
                              wire.field_uniform(top, 3.0, 2.0, (1.0, 0.0))])
    ref_world = world_chain.copy_world(world)
    with hip.Solver(0) as s:
        s.set_option("strip_patience", 0)
        s.set_option("persist_spin_limit", 4096)
        s.set_option("persist_debug", 8)
        s.world_set_fields(fields)
        upload(s, world)
        for step in range(2):
            want = ref.apply_in_place(ref_world, fields)
            assert (want["terms"] >= 10).all(), want["terms"]
            step_both(s, params, ref_world)
            if step == 0:
                assert s.stats()["persistFallbacks"] >= 1
            assert_states(s.world_field_states(), want, "the repeated step" if step == 0 else "the step after it")
            got, _ = download(s, world)
            assert_same_world(got, ref_world, "step %d" % step, ("bodies",))
        world_chain.assert_device_equals_oracle(got, ref_world, "pyramid 100 with a repeated step")
