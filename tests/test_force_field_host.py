"""The force fields without a GPU: the interface as declared and bound with the header's sizes and offsets, the statement
(tests/force_field_ref.py) on hand-made cases whose products are exact, the statement against tests/world_edit_ref.apply of its own
term list on the fixtures tests/golden/force_fields/*.npz (the reference's recorded distance outputs, so this runs where the compiled
reference is absent; where it is built the fixtures are made again and compared), the compiler's resource report of the new kernels,
and the host side under ASan + UBSan on the stand-in HIP runtime of tests/hostcheck (a stand-alone program, nothing preloaded)."""
import numpy as np
import pytest

from solver2d_amd import wire
from tests import force_field_ref as ref, hostcheck_util, world_edit_ref
from tests.world_chain import golden

needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
CALLS = ("s2amd_world_apply_fields", "s2amd_world_set_fields", "s2amd_world_field_states")
F = np.float32


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    hostcheck_util.assert_struct_layout(tmp_path, {"s2amdField": wire.field_dtype, "s2amdFieldState": wire.field_state_dtype})
    assert (wire.FIELD_SIZE, wire.FIELD_STATE_SIZE) == (128, 64)


def test_header_defines_and_bindings():
    defines = {"S2AMD_MAX_FIELDS": 1024, "S2AMD_FIELD_RADIAL": 1, "S2AMD_FIELD_UNIFORM": 2, "S2AMD_FIELD_DRAG": 3, "S2AMD_FIELD_DISABLED": 1,
               "S2AMD_FIELD_AS_IMPULSE": 2, "S2AMD_FIELD_LINEAR_FALLOFF": 4, "S2AMD_API_VERSION": 5}
    hostcheck_util.assert_header_and_bindings(CALLS, defines, methods=True, argtypes=True)
    assert (wire.MAX_FIELDS, wire.FIELD_RADIAL, wire.FIELD_UNIFORM, wire.FIELD_DRAG) == (1024, 1, 2, 3)
    assert (wire.FIELD_DISABLED, wire.FIELD_AS_IMPULSE, wire.FIELD_LINEAR_FALLOFF) == (1, 2, 4)
    assert wire.API_VERSION == 5


# ---- the statement on hand-made cases whose products are exact: the distance is given, not computed ----
def tiny_world():
    """body 0 static with a box, body 1 dynamic: a circle of radius 0.5 resting at (0, 0.5), mass 2 (invMass 0.5), invI 4; body 2
    kinematic with a circle; body 3 a free slot that a stale shape names; body 4 dynamic with a circle at (8, 0.5)"""
    bodies = np.zeros(5, dtype=wire.body_dtype)
    bodies["rot"] = (0.0, 1.0)
    bodies["type"] = (wire.BODY_STATIC, wire.BODY_DYNAMIC, wire.BODY_KINEMATIC, wire.BODY_FREE, wire.BODY_DYNAMIC)
    bodies["position"] = ((0.0, -1.0), (0.0, 0.5), (3.0, 0.5), (0.0, 0.0), (8.0, 0.5))
    for b in (1, 4):
        bodies[b]["mass"], bodies[b]["invMass"], bodies[b]["I"], bodies[b]["invI"] = 2.0, 0.5, 0.25, 4.0
    shapes = np.zeros(5, dtype=wire.shape_dtype)
    shapes["body"] = (0, 1, 2, 3, 4)
    shapes["type"] = (wire.SHAPE_POLYGON, wire.SHAPE_CIRCLE, wire.SHAPE_CIRCLE, wire.SHAPE_FREE, wire.SHAPE_CIRCLE)
    shapes["categoryBits"], shapes["radius"] = 1, 0.5
    for k in range(5):
        x, y = bodies["position"][k]
        shapes[k]["fatAABB"] = (x - 0.6, y - 0.6, x + 0.6, y + 0.6)
    shapes[0]["fatAABB"] = (-10.0, -2.0, 10.0, 0.0)
    return {"bodies": bodies, "shapes": shapes, "origins": np.ascontiguousarray(bodies["position"]).copy()}


def given(world, fields, distances):
    """recorded D outputs for every candidate: the given ones, anything else far away"""
    out = {}
    for i, f in enumerate(fields):
        if ref.is_active(world, f):
            for slot in ref.candidates(world, f):
                out[(i, slot)] = distances.get((i, slot), (F(1e9), F(0.0), F(0.0)))
    return out


def test_point_field_straight_above_a_resting_circle():
    """The field at (0, 3), the circle's top at (0, 1): distance 2, pointB (0, 1), the direction (0, -1) exactly.  An impulse of 4 on
    invMass 0.5 gives -2 in y; a force of 4 adds (0, -4); falloff at half the range of 4 gives scale 0.5."""
    world = tiny_world()
    d = {(0, 1): (F(2.0), F(0.0), F(1.0))}
    for flags, rng, want_v, want_f in ((wire.FIELD_AS_IMPULSE, 2.0, (0.0, -2.0), (0.0, 0.0)), (0, 2.0, (0.0, 0.0), (0.0, -4.0)),
                                       (wire.FIELD_LINEAR_FALLOFF, 4.0, (0.0, 0.0), (0.0, -2.0)), (wire.FIELD_AS_IMPULSE | wire.FIELD_LINEAR_FALLOFF, 4.0, (0.0, -1.0), (0.0, 0.0)),
                                       (wire.FIELD_LINEAR_FALLOFF, 0.0, (0.0, 0.0), (0.0, 0.0))):  # range 0: out of reach at distance 2
        fields = wire.field_list([wire.field_radial((0.0, 3.0), rng, 4.0, flags=flags)])
        bodies, states, edits = ref.apply(world, fields, recorded=given(world, fields, d))
        assert bodies["linearVelocity"][1].tolist() == list(want_v) and bodies["force"][1].tolist() == list(want_f), (flags, rng)
        assert bodies["angularVelocity"][1] == 0.0  # the point (0, 1) is straight above the centre
        assert states["terms"].tolist() == [1 if rng > 0 else 0] and states["lowestShape"].tolist() == [1 if rng > 0 else -1]
        others = [0, 2, 3, 4]
        assert bodies[others].tobytes() == world["bodies"][others].tobytes()
    # an impulse off the centre line turns the body: point (0.5, 0.5), direction (1, 0) from a centre at (-1, 0.5): w += invI * (0.5 * 0 - 0 * 4)
    fields = wire.field_list([wire.field_radial((-1.0, 0.5), 2.0, 4.0, flags=wire.FIELD_AS_IMPULSE), wire.field_uniform((0.0, 3.0), 2.0, 2.0, (0.0, 1.0), flags=wire.FIELD_AS_IMPULSE)])
    bodies, states, edits = ref.apply(world, fields, recorded=given(world, fields, {(0, 1): (F(0.5), F(-0.5), F(1.0)), (1, 1): (F(2.0), F(0.0), F(1.0))}))
    # term 0: n = normalize((0.5, 0.5)); term 1 at the body's own position: no turn
    inv = F(1.0) / F(np.sqrt(F(0.5)))
    g = F(4.0) * F(inv * F(0.5))
    assert bodies["linearVelocity"][1].tolist() == [F(0.5) * g, F(F(0.5) * g) + F(1.0)]
    assert bodies["angularVelocity"][1] == F(F(4.0) * F(F(F(-0.5) * g) - F(F(0.5) * g)))
    assert edits["kind"].tolist() == [4, 4] and edits["v"][1].tolist() == [0.0, 2.0, 0.0, 0.5]


def test_centre_on_point_b_takes_the_zero_vector_branch():
    world = tiny_world()
    fields = wire.field_list([wire.field_radial((0.0, 1.0), 1.0, 4.0, flags=wire.FIELD_AS_IMPULSE), wire.field_radial((0.0, 1.0), 1.0, 4.0)])
    bodies, states, edits = ref.apply(world, fields, recorded=given(world, fields, {(0, 1): (F(0.0), F(0.0), F(1.0)), (1, 1): (F(0.0), F(0.0), F(1.0))}))
    assert bodies.tobytes() == world["bodies"].tobytes()  # no change ...
    assert states["terms"].tolist() == [1, 1] and len(edits) == 2 and not edits["v"][:, :2].any()  # ... but a term counted, and applied
    assert ref.normalize(1e-12, 0.0) == (0.0, 0.0) and ref.normalize(3.0, 4.0) == (F(F(1.0) / F(5.0)) * F(3.0), F(F(1.0) / F(5.0)) * F(4.0))


def test_drag_twice_reads_the_velocity_the_first_left():
    world = tiny_world()
    world["bodies"]["linearVelocity"][1] = (8.0, -4.0)
    fields = wire.field_list([wire.field_drag((0.0, 3.0), 2.0, 0.5, flags=wire.FIELD_AS_IMPULSE)] * 2)
    d = {(0, 1): (F(2.0), F(0.0), F(1.0)), (1, 1): (F(2.0), F(0.0), F(1.0))}
    bodies, states, edits = ref.apply(world, fields, recorded=given(world, fields, d))
    # g0 = -0.5 * (8, -4) = (-4, 2), v = (8, -4) + 0.5 * g0 = (6, -3); g1 = -0.5 * (6, -3) = (-3, 1.5), v = (4.5, -2.25)
    assert edits["v"][:, :2].tolist() == [[-4.0, 2.0], [-3.0, 1.5]] and bodies["linearVelocity"][1].tolist() == [4.5, -2.25]
    assert edits["v"][:, 2:].tolist() == [[0.0, 0.5], [0.0, 0.5]] and bodies["angularVelocity"][1] == 0.0
    # as a force it reads the velocity, which a force does not change: the same term twice
    fields["flags"] = 0
    bodies, _, edits = ref.apply(world, fields, recorded=given(world, fields, d))
    assert edits["v"][:, :2].tolist() == [[-4.0, 2.0], [-4.0, 2.0]] and bodies["force"][1].tolist() == [-8.0, 4.0]


def test_static_kinematic_free_and_own_body_shapes_yield_no_term():
    world = tiny_world()
    everywhere = wire.field_list([wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0)), wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0), body=1),
                                  wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0), body=3), wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0), flags=wire.FIELD_DISABLED),
                                  wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0), mask=2), wire.field_uniform((0.0, 0.0), 100.0, 1.0, (1.0, 0.0), body=2)])
    assert [ref.candidates(world, f) if ref.is_active(world, f) else None for f in everywhere] == [[1, 4], [4], None, None, [], [1, 4]]
    near = {(i, s): (F(0.0), F(0.0), F(0.0)) for i in range(6) for s in range(5)}
    bodies, states, edits = ref.apply(world, everywhere, recorded=near)
    assert states["terms"].tolist() == [2, 1, 0, 0, 0, 2] and states["active"].tolist() == [1, 1, 0, 0, 1, 1]
    assert states["lowestShape"].tolist() == [1, 4, -1, -1, -1, 1]
    assert bodies["force"][:, 0].tolist() == [0.0, 2.0, 0.0, 0.0, 3.0]
    for i in (2, 3):  # inactive: transform and box +0
        assert states[i]["position"].tobytes() + states[i]["rot"].tobytes() + states[i]["box"].tobytes() == bytes(32)
    assert states[1]["position"].tolist() == [0.0, 0.5] and states[5]["position"].tolist() == [3.0, 0.5]  # attached: the body's origin
    assert states[0]["box"].tolist() == [-100.0, -100.0, 100.0, 100.0]


# ---- the fixtures ----
@pytest.mark.parametrize("name", sorted(ref.FIXTURES))
def test_statement_equals_the_edit_route_on_the_fixtures(name):
    """On a committed world with the recorded distances: the bodies the statement gives are what tests/world_edit_ref.apply gives for
    the statement's own term list, and the fields act (terms, a body with several, the order matters)."""
    _, world = golden(name)
    fields, recorded = ref.load_fixture(name)
    assert fields.tobytes() == ref.fixture_fields(name).tobytes()
    bodies, states, edits = ref.apply(world, fields, recorded=recorded)
    route = world["bodies"].copy()
    assert world_edit_ref.apply(route, world["joints"], edits) == 0
    assert route.tobytes() == bodies.tobytes() and bodies.tobytes() != world["bodies"].tobytes()
    assert int(states["terms"].sum()) == len(edits) >= 6
    dynamic = world["bodies"]["type"] == wire.BODY_DYNAMIC
    assert dynamic[edits["target"]].all()
    untouched = np.setdiff1d(np.arange(len(bodies)), edits["target"])
    assert bodies[untouched].tobytes() == world["bodies"][untouched].tobytes()
    assert ref.terms_per_body(world, edits).max() >= 2
    other = [n for n in bodies.dtype.names if n not in ("linearVelocity", "angularVelocity", "force")]
    assert all(bodies[n].tobytes() == world["bodies"][n].tobytes() for n in other)
    if name == "shapes_zoo40_PGS_NGS_Block":
        ref.assert_zoo_condition(world, states, edits)
    if name == "tumbler60_TGS_Soft":  # the drum: one dynamic body with four shapes -- four terms per field on it
        assert np.bincount(edits["target"]).max() == 4 * len(fields) and (states["terms"] == 64).all()


@needs_reference
@pytest.mark.parametrize("name", sorted(ref.FIXTURES))
def test_recorded_fixtures_equal_the_compiled_reference(name):
    _, world = golden(name)
    built = ref.record(name, world)
    with np.load(ref.fixture_path(name)) as fx:
        assert sorted(built) == sorted(fx.files)
        for key in built:
            assert np.ascontiguousarray(built[key]).tobytes() == fx[key].tobytes(), (name, key)


def test_kernels_use_no_scratch():
    """hipcc's own report for force_field.hip (make resources-force-field), through tools/kernel_resources.py: every kernel of the file
    is there, none has a private frame or spills."""
    kernels = dict.fromkeys(("fieldKeysKernel", "fieldPrepareKernel", "fieldApplyKernel", "reportBodyRangesKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-force-field", "resources_force_field.txt", kernels, floor=3)


@hostcheck_util.needs_sanitizers
def test_force_field_host_code_under_asan_and_ubsan(tmp_path):
    """Every validation rule through both entry points, with and without a world -> the list held across uploads with other capacities
    -> one-shot calls with and without states, shorter and longer than the pinned stage -> the body -> shapes list built once per upload
    and only when fields are used -> the states getter with too-small, exact and ample heap buffers of exactly the size passed, before
    a step, after it, after the list was replaced, refused and cleared -> destroy, for 0, 1, 129, 257 and 1,024 fields, on the sanitizer
    build of tests/test_hostcheck.py (kernels never run there)."""
    hostcheck_util.run_sanitized(tmp_path, "force_field_main.cpp", "FORCE FIELD MAIN OK", timeout=600)
