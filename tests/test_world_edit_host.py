"""World edits on the resident world (s2amd_world_edit), the part that needs no GPU: the interface as declared and bound, the statement
(tests/world_edit_ref.py) against the compiled reference's own eight setters and against the fixtures tests/golden/world_edit/*.npz,
the statement's skip rules on synthetic records, and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import hostcheck_util, refbind, world_edit_ref as ref, world_edit_world as ew

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not refbind.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")


def _header():
    return open(os.path.join(ROOT, "include", "solver2d_amd.h")).read()


def test_header_declares_the_call_the_struct_and_the_kinds():
    header = _header()
    assert re.search(r"\bint s2amd_world_edit\(s2amdSolver\* solver, const s2amdWorldEdit\* edits, int32_t count, int32_t\* skipped", header)
    assert re.search(r"#define S2AMD_API_VERSION 5\b", header) and wire.API_VERSION == 5
    for name, value in wire.EDIT_KINDS.items():
        m = re.search(r"#define S2AMD_EDIT_%s\s+(\d+)\b" % name, header)
        assert m and int(m.group(1)) == value == getattr(wire, "EDIT_" + name), name
    assert sorted(wire.EDIT_KINDS.values()) == list(range(1, 9))
    for word in ("s2Body_SetTransform", "sharded worlds", "device memory"):  # what is not offered is said there
        assert word in header[header.index("World edits:"):header.index("typedef struct s2amdWorldEdit")], word


def test_wire_layout_equals_the_headers_struct_and_both_libraries_export_the_call():
    body = re.search(r"typedef struct s2amdWorldEdit[^{]*\{(.*?)\}\s*s2amdWorldEdit;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, offset = [], 0
    for ctype, names in re.findall(r"\b(int32_t|float)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            count = int(m.group(2) or 1)
            fields.append((m.group(1), np.int32 if ctype == "int32_t" else np.float32, count, offset))
            offset += 4 * count
    assert offset == 32 == wire.world_edit_dtype.itemsize == wire.WORLD_EDIT_SIZE
    assert [f[0] for f in fields] == list(wire.world_edit_dtype.names) == ["kind", "target", "flag", "reserved", "v"]
    for name, base, count, at in fields:
        dt, off = wire.world_edit_dtype.fields[name][:2]
        assert off == at and dt.base == np.dtype(base) and (dt.shape or (1,)) == (count,), name
    for fast in (False, True):
        lib = hip.load(fast=fast)
        assert "s2amd_world_edit" in hip.EXPORTS and lib.s2amd_world_edit.argtypes is not None
    assert callable(hip.Solver.world_edit)
    e = wire.edit_apply_linear_impulse(7, (1.0, 2.0), (3.0, 4.0))
    assert (e["kind"], e["target"], e["flag"], e["reserved"], e["v"].tolist()) == (4, 7, 0, 0, [1.0, 2.0, 3.0, 4.0])
    e = wire.edit_revolute_enable_motor(3, True)
    assert (e["kind"], e["target"], e["flag"]) == (7, 3, 1)
    assert wire.edit_list([wire.edit_mouse_set_target(1, (2.0, 3.0)), wire.edit_set_angular_velocity(0, 5.0)]).dtype == wire.world_edit_dtype


def _synthetic():
    bodies = np.zeros(4, dtype=wire.body_dtype)
    bodies["type"] = (wire.BODY_FREE, wire.BODY_STATIC, wire.BODY_KINEMATIC, wire.BODY_DYNAMIC)
    bodies["invMass"], bodies["invI"] = (9.0, 0.0, 0.0, 0.5), (9.0, 0.0, 0.0, 0.25)
    bodies["position"] = [(0, 0), (1, 1), (2, 2), (1.0, -1.0)]
    bodies["linearVelocity"] = [(7, 7), (0, 0), (1, 0), (0.5, 0.25)]
    joints = np.zeros(3, dtype=wire.joint_dtype)
    joints["type"] = (wire.JOINT_FREE, wire.JOINT_REVOLUTE, wire.JOINT_MOUSE)
    return bodies, joints


def test_the_statements_skip_rules_on_synthetic_records():
    bodies, joints = _synthetic()
    b0, j0 = bodies.copy(), joints.copy()
    # a free body slot: every body kind is skipped and counted
    free = [wire.edit_set_linear_velocity(0, (1, 2)), wire.edit_set_angular_velocity(0, 3), wire.edit_apply_force_to_center(0, (4, 5)),
            wire.edit_apply_linear_impulse(0, (1, 1), (0, 0))]
    assert ref.apply(bodies, joints, wire.edit_list(free)) == 4
    # a free joint slot, a mouse edit on a revolute joint, the three revolute edits on a mouse joint
    wrong = [wire.edit_mouse_set_target(0, (1, 1)), wire.edit_revolute_enable_limit(0, 1), wire.edit_mouse_set_target(1, (1, 1)),
             wire.edit_revolute_enable_limit(2, 1), wire.edit_revolute_enable_motor(2, 1), wire.edit_revolute_set_motor_speed(2, 4.0)]
    assert ref.apply(bodies, joints, wire.edit_list(wrong)) == 6
    # an impulse on a static and on a kinematic body: the reference's early return -- nothing written, nothing counted
    assert ref.apply(bodies, joints, wire.edit_list([wire.edit_apply_linear_impulse(1, (1, 1), (0, 0)), wire.edit_apply_linear_impulse(2, (1, 1), (0, 0))])) == 0
    assert bodies.tobytes() == b0.tobytes() and joints.tobytes() == j0.tobytes()
    # kinds 1-3 write whatever the live body's type is; the impulse on the dynamic body, by hand:
    # v = (0.5, 0.25) + 0.5 * (2, 4) = (1.5, 2.25); r = (3, 1) - (1, -1) = (2, 2); w = 0 + 0.25 * (2 * 4 - 2 * 2) = 1
    edits = [wire.edit_set_linear_velocity(1, (1, 2)), wire.edit_set_angular_velocity(2, 3), wire.edit_apply_force_to_center(1, (4, 5)),
             wire.edit_apply_force_to_center(1, (0.5, 0.5)), wire.edit_apply_linear_impulse(3, (2, 4), (3, 1)),
             wire.edit_revolute_enable_limit(1, -5), wire.edit_revolute_enable_motor(1, 7), wire.edit_revolute_enable_motor(1, 0),
             wire.edit_revolute_set_motor_speed(1, -2.5), wire.edit_mouse_set_target(2, (8, 9))]
    assert ref.apply(bodies, joints, wire.edit_list(edits)) == 0
    assert bodies["linearVelocity"].tolist() == [[7, 7], [1, 2], [1, 0], [1.5, 2.25]] and bodies["angularVelocity"].tolist() == [0, 0, 3, 1]
    assert bodies["force"].tolist() == [[0, 0], [4.5, 5.5], [0, 0], [0, 0]]
    assert (joints["enableLimit"].tolist(), joints["enableMotor"].tolist()) == ([0, 1, 0], [0, 0, 0])
    assert joints["motorSpeed"].tolist() == [0, -2.5, 0] and joints["targetA"].tolist() == [[0, 0], [0, 0], [8, 9]]
    # a set passes a NaN's payload through
    nan = wire.edit_set_angular_velocity(3, 0.0)
    nan["v"].view(np.uint32)[0] = 0x7FC12345
    ref.apply(bodies, joints, wire.edit_list([nan]))
    assert bodies["angularVelocity"].view(np.uint32)[3] == 0x7FC12345
    # what the host refuses
    ok = wire.edit_list(edits)
    assert ref.valid(ok, 4, 3) == -1
    for field, value, kind in (("kind", 0, None), ("kind", 9, None), ("target", -1, None), ("target", 4, 1), ("target", 3, 8), ("reserved", 1, None)):
        bad = ok.copy()
        bad[5 if kind is None else 0][field] = value
        if kind is not None:
            bad[0]["kind"] = kind
        assert ref.valid(bad, 4, 3) == (5 if kind is None else 0), (field, value)


def test_the_float_sums_depend_on_the_order_on_one_target():
    """Why only the order on one target matters, and matters to the bit."""
    bodies, joints = _synthetic()
    a = wire.edit_list([wire.edit_apply_force_to_center(3, (1e8, 0)), wire.edit_apply_force_to_center(3, (1.0, 0)), wire.edit_apply_force_to_center(3, (-1e8, 0))])
    one, two = bodies.copy(), bodies.copy()
    ref.apply(one, joints, a)
    ref.apply(two, joints, a[[0, 2, 1]])
    assert one["force"][3, 0] == 0.0 and two["force"][3, 0] == 1.0


def _check_case(case, what):
    bodies, joints = case["bodies_before"].copy(), case["joints_before"].copy()
    edits = case["edits"]
    assert edits.dtype == wire.world_edit_dtype and bodies.dtype == wire.body_dtype and joints.dtype == wire.joint_dtype
    # a few hundred edits, repeated targets, only targets the reference accepts
    targets = list(zip((edits["kind"] >= 5).tolist(), edits["target"].tolist()))
    assert len(edits) >= 300 and len(set(targets)) < len(targets), what
    assert ref.apply(bodies, joints, edits) == 0, what
    assert bodies.tobytes() == case["bodies_after"].tobytes(), what + ": bodies"
    assert joints.tobytes() == case["joints_after"].tobytes(), what + ": joints"
    # ... and the edits did something: the ids reached the records they name
    assert bodies.tobytes() != case["bodies_before"].tobytes(), what
    if (edits["kind"] >= 5).any():
        assert joints.tobytes() != case["joints_before"].tobytes(), what


def test_the_reference_recipe_compiles_without_asserts():
    """reference_apply passes revision 0 in every id: with NDEBUG no setter reads it (their only uses are in S2_ASSERT)."""
    assert re.search(r"^CFLAGS_COMMON\s*=.*-DNDEBUG\b", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)


@needs_reference
@pytest.mark.parametrize("name", sorted(ew.CASES))
def test_statement_equals_the_compiled_references_setters(name):
    case = ew.reference_case(name)
    _check_case(case, name)
    kinds = set(case["edits"]["kind"].tolist())
    assert {1, 2, 3, 4} <= kinds and (name != "mixed24" or kinds == set(range(1, 9))), kinds


@needs_reference
@pytest.mark.parametrize("name", sorted(ew.CASES))
def test_fixtures_are_what_the_compiled_reference_gives_today(name):
    case, fixture = ew.reference_case(name), ew.load_fixture(name)
    for key in ew.FIXTURE_KEYS:
        assert case[key].tobytes() == fixture[key].tobytes(), (name, key)


@pytest.mark.parametrize("name", sorted(ew.CASES))
def test_statement_equals_the_fixtures(name):
    _check_case(ew.load_fixture(name), name)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_use_no_scratch():
    """hipcc's own report for world_edit.hip (make resources-world-edit), through tools/kernel_resources.py: the file's three kernels are
    there, none has a private frame or spills a register."""
    kernels = dict.fromkeys(("editDistinctKernel", "editKeysKernel", "editWalkKernel"), 1)
    hostcheck_util.assert_kernel_resources("resources-world-edit", "resources_world_edit.txt", kernels, floor=4)
