"""numpy / ctypes mirrors of the C-ABI structs in include/solver2d_amd.h.

The dtypes are laid out exactly as the C compiler lays out the structs (all members are 4-byte
scalars, so there is no padding); `tests/test_abi.py` checks the sizes against the built
library.  Arrays of these dtypes are what the Python host side hands to the C entry points.
"""
import ctypes
import numpy as np

API_VERSION = 5

SOLVER_NAMES = [
    "Jacobi", "PGS", "PGS_NGS", "PGS_NGS_Block", "PGS_Soft",
    "SoftStep", "TGS_Sticky", "TGS_Soft", "TGS_NGS", "XPBD",
]
SOLVER_ID = {n: i for i, n in enumerate(SOLVER_NAMES)}

BODY_FREE, BODY_STATIC, BODY_KINEMATIC, BODY_DYNAMIC = -1, 0, 1, 2
JOINT_FREE, JOINT_REVOLUTE, JOINT_MOUSE = -1, 0, 1

f32, i32 = np.float32, np.int32

body_dtype = np.dtype([
    ("position", f32, 2), ("rot", f32, 2), ("linearVelocity", f32, 2), ("angularVelocity", f32),
    ("deltaPosition", f32, 2), ("localCenter", f32, 2), ("force", f32, 2), ("torque", f32),
    ("mass", f32), ("invMass", f32), ("I", f32), ("invI", f32),
    ("linearDamping", f32), ("angularDamping", f32), ("gravityScale", f32), ("type", i32),
])

manifold_point_dtype = np.dtype([
    ("localAnchorA", f32, 2), ("localAnchorB", f32, 2),
    ("frictionAnchorA", f32, 2), ("frictionAnchorB", f32, 2),
    ("frictionNormalA", f32, 2), ("frictionNormalB", f32, 2),
    ("separation", f32), ("normalImpulse", f32), ("tangentImpulse", f32),
])

contact_dtype = np.dtype([
    ("bodyA", i32), ("bodyB", i32), ("pointCount", i32), ("frictionPersisted", i32),
    ("normal", f32, 2), ("friction", f32), ("constraintIndex", i32),
    ("points", manifold_point_dtype, 2),
])

joint_dtype = np.dtype([
    ("type", i32), ("bodyA", i32), ("bodyB", i32), ("enableMotor", i32), ("enableLimit", i32),
    ("localOriginAnchorA", f32, 2), ("localOriginAnchorB", f32, 2),
    ("impulse", f32, 2), ("motorImpulse", f32), ("lowerImpulse", f32), ("upperImpulse", f32),
    ("maxMotorTorque", f32), ("motorSpeed", f32), ("referenceAngle", f32),
    ("lowerAngle", f32), ("upperAngle", f32),
    ("hertz", f32), ("dampingRatio", f32), ("targetA", f32, 2),
])

u32 = np.uint32
shape_dtype = np.dtype([
    ("body", i32), ("type", i32), ("categoryBits", u32), ("maskBits", u32), ("groupIndex", i32),
    ("proxyKey", i32), ("enlarged", i32), ("count", i32), ("radius", f32),
    ("aabb", f32, 4), ("fatAABB", f32, 4), ("vertices", f32, (8, 2)), ("normals", f32, (8, 2)),
])
SHAPE_FREE, SHAPE_CAPSULE, SHAPE_CIRCLE, SHAPE_POLYGON, SHAPE_SEGMENT = -1, 0, 1, 2, 3
SHAPE_SIZE = shape_dtype.itemsize
assert SHAPE_SIZE == 196

u16, u8 = np.uint16, np.uint8
pair_state_dtype = np.dtype([
    ("shapeA", i32), ("shapeB", i32), ("cacheMetric", f32), ("cacheCount", u16), ("id", u16, 2),
    ("cacheIndexA", u8, 3), ("cacheIndexB", u8, 3), ("persisted", u8, 2), ("pad", u8, 2),
])
PAIR_STATE_SIZE = pair_state_dtype.itemsize
assert PAIR_STATE_SIZE == 28
PAIR_UPDATED, PAIR_SEPARATED, PAIR_FREE = 0, 1, -1

BODY_SIZE, CONTACT_SIZE, JOINT_SIZE = body_dtype.itemsize, contact_dtype.itemsize, joint_dtype.itemsize
assert BODY_SIZE == 88 and manifold_point_dtype.itemsize == 60 and CONTACT_SIZE == 152 and JOINT_SIZE == 92


class StepParams(ctypes.Structure):
    _fields_ = [
        ("solverType", ctypes.c_int32), ("dt", ctypes.c_float), ("velIters", ctypes.c_int32),
        ("posIters", ctypes.c_int32), ("warmStart", ctypes.c_int32), ("gravity", ctypes.c_float * 2),
    ]

    @classmethod
    def make(cls, solver, dt=1.0 / 60.0, vel_iters=4, pos_iters=2, warm_start=True, gravity=(0.0, -10.0)):
        sid = SOLVER_ID[solver] if isinstance(solver, str) else int(solver)
        return cls(sid, np.float32(dt), int(vel_iters), int(pos_iters), 1 if warm_start else 0,
                   (ctypes.c_float * 2)(*gravity))

    def as_dict(self):
        return dict(solverType=int(self.solverType), dt=float(self.dt), velIters=int(self.velIters),
                    posIters=int(self.posIters), warmStart=int(self.warmStart),
                    gravity=[float(self.gravity[0]), float(self.gravity[1])])


class StepStats(ctypes.Structure):
    _fields_ = [
        ("constraintCount", ctypes.c_int32), ("jointCount", ctypes.c_int32),
        ("contactColors", ctypes.c_int32), ("jointColors", ctypes.c_int32),
        ("solveSweeps", ctypes.c_int32), ("kernelLaunches", ctypes.c_int32),
        ("deviceMs", ctypes.c_float), ("solveKernelMs", ctypes.c_float), ("hostPrepMs", ctypes.c_float),
        ("graphReplayed", ctypes.c_int32), ("solveLaunches", ctypes.c_int32),
        ("eventPairOverheadMs", ctypes.c_float), ("groupCount", ctypes.c_int32), ("messagePassing", ctypes.c_int32),
        ("stripCount", ctypes.c_int32), ("seamCount", ctypes.c_int32), ("persistent", ctypes.c_int32), ("persistFallbacks", ctypes.c_int32),
        ("structureBuilds", ctypes.c_int32), ("placedContacts", ctypes.c_int32), ("potentialConstraints", ctypes.c_int32), ("pairLanes", ctypes.c_int32),
        ("asyncBuildsRequested", ctypes.c_int32), ("asyncBuildsAdopted", ctypes.c_int32), ("asyncWaitMs", ctypes.c_float),
        ("bodiesAdopted", ctypes.c_int32), ("seamBodiesAdded", ctypes.c_int32), ("roundsOpened", ctypes.c_int32),
        ("overflowContacts", ctypes.c_int32), ("slicedStep", ctypes.c_int32), ("slicedSteps", ctypes.c_int32), ("nearHandoffTimeouts", ctypes.c_int32),
    ]


class WorldStepInfo(ctypes.Structure):
    """s2amdWorldStepInfo"""
    _fields_ = [
        ("separatedCount", ctypes.c_int32), ("activeContacts", ctypes.c_int32), ("graphChanged", ctypes.c_int32),
        ("movedCount", ctypes.c_int32), ("contactsMs", ctypes.c_float), ("solveMs", ctypes.c_float), ("stepMs", ctypes.c_float),
    ]


def solve_sweeps_per_step(solver, vel_iters, pos_iters):
    """Full passes of a s2SolveContacts_* function per s2World_Step, per reference driver.

    TGS_Soft / SoftStep: velIters * (1 + [posIters > 0])   (solve_tgs_soft.c:211-269)
    Jacobi / PGS_Soft:   velIters + posIters                 (solve_jacobi.c:218,255)
    PGS:                 velIters                            (solve_pgs.c:186-199)
    PGS_NGS / Block:     velIters velocity + posIters position sweeps
    TGS_NGS:             velIters * 2 (velocity + NGS position per sub-step)
    TGS_Sticky:          velIters + posIters
    XPBD:                velIters * 2 (position + velocity relax per sub-step)
    """
    name = solver if isinstance(solver, str) else SOLVER_NAMES[int(solver)]
    if name in ("TGS_Soft", "SoftStep"):
        return vel_iters * (2 if pos_iters > 0 else 1)
    if name in ("Jacobi", "PGS_Soft", "TGS_Sticky", "PGS_NGS", "PGS_NGS_Block"):
        return vel_iters + pos_iters
    if name == "PGS":
        return vel_iters
    if name in ("TGS_NGS", "XPBD"):
        return 2 * vel_iters
    raise ValueError(name)


def as_ptr(arr, ctype=ctypes.c_void_p):
    if arr is None or len(arr) == 0:
        return ctypes.c_void_p(0)
    assert arr.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(arr.ctypes.data)


# s2amdShapeBox (include/solver2d_amd.h): what stage 4 changed in a shape
# s2TreeNode byte for byte (include/solver2d/dynamic_tree.h:14-41; s2amdTreeNode)
tree_node_dtype = np.dtype([("aabb", np.float32, 4), ("categoryBits", np.uint32), ("parent", np.int32), ("child1", np.int32), ("child2", np.int32),
                            ("userData", np.int32), ("height", np.int16), ("enlarged", np.uint8), ("pad", np.uint8, 9)])
assert tree_node_dtype.itemsize == 48
shape_box_dtype = np.dtype([("aabb", np.float32, 4), ("fatAABB", np.float32, 4), ("enlarged", np.int32)])
assert shape_box_dtype.itemsize == 36

# contact report of the resident world (include/solver2d_amd.h: s2amd_world_set_report)
REPORT_TOUCH, REPORT_CONTACTS, REPORT_BODY_SUMS = 1, 2, 4
REPORT_ALL = REPORT_TOUCH | REPORT_CONTACTS | REPORT_BODY_SUMS
# s2amdTouchingContact, s2amdBodyContactSum
touching_contact_dtype = np.dtype([("slot", np.int32), ("bodyA", np.int32), ("bodyB", np.int32), ("pointCount", np.uint8), ("persisted", np.uint8, 2),
                                   ("pad", np.uint8), ("normal", np.float32, 2), ("point", np.float32, (2, 2)), ("separation", np.float32, 2),
                                   ("normalImpulse", np.float32, 2), ("tangentImpulse", np.float32, 2)])
assert touching_contact_dtype.itemsize == 64
body_contact_sum_dtype = np.dtype([("impulse", np.float32, 2), ("normalImpulse", np.float32), ("touching", np.int32)])
assert body_contact_sum_dtype.itemsize == 16

# joint report of the resident world (include/solver2d_amd.h: s2amd_world_set_joint_report)
JOINT_REPORT_STATES, JOINT_REPORT_LIMITS, JOINT_REPORT_BODY_SUMS = 1, 2, 4
JOINT_REPORT_ALL = JOINT_REPORT_STATES | JOINT_REPORT_LIMITS | JOINT_REPORT_BODY_SUMS
# s2amdJointState, s2amdBodyJointSum, s2amdJointSummary
joint_state_dtype = np.dtype([("slot", np.int32), ("type", np.int32), ("bodyA", np.int32), ("bodyB", np.int32), ("anchorA", np.float32, 2),
                              ("anchorB", np.float32, 2), ("impulse", np.float32, 2), ("axialImpulse", np.float32), ("motorImpulse", np.float32),
                              ("angle", np.float32), ("angularSpeed", np.float32), ("lowerImpulse", np.float32), ("upperImpulse", np.float32)])
assert joint_state_dtype.itemsize == 64
body_joint_sum_dtype = np.dtype([("impulse", np.float32, 2), ("axialImpulse", np.float32), ("joints", np.int32)])
assert body_joint_sum_dtype.itemsize == 16
joint_summary_dtype = np.dtype([("liveJoints", np.int32), ("revoluteJoints", np.int32), ("atLower", np.int32), ("atUpper", np.int32),
                                ("maxGapSlot", np.int32), ("maxGapSquared", np.float32), ("pad", np.int32, 2)])
assert joint_summary_dtype.itemsize == 32

# shape report of the resident world (include/solver2d_amd.h: s2amd_world_set_shape_report, s2amd_world_set_shape_view)
SHAPE_REPORT_DRAW, SHAPE_REPORT_VIEW, SHAPE_REPORT_BOUNDS = 1, 2, 4
SHAPE_REPORT_ALL = SHAPE_REPORT_DRAW | SHAPE_REPORT_VIEW | SHAPE_REPORT_BOUNDS
# s2amdShapeDraw, s2amdShapeSummary
shape_draw_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("type", np.int32), ("vertexCount", np.int32), ("bodyClass", np.int32),
                             ("radius", np.float32), ("axis", np.float32, 2), ("vertices", np.float32, (8, 2)), ("aabb", np.float32, 4),
                             ("fatAABB", np.float32, 4)])
assert shape_draw_dtype.itemsize == 128
shape_summary_dtype = np.dtype([("liveShapes", np.int32), ("inView", np.int32), ("byType", np.int32, 4), ("badBodyShapes", np.int32), ("pad", np.int32),
                                ("movableBounds", np.float32, 4), ("viewBounds", np.float32, 4)])
assert shape_summary_dtype.itemsize == 64

# body report of the resident world (include/solver2d_amd.h: s2amd_world_set_body_report, s2amd_world_set_rest_thresholds)
BODY_REPORT_STATES, BODY_REPORT_REST, BODY_REPORT_ISLANDS, BODY_REPORT_MOVED_ONLY = 1, 2, 4, 8
BODY_REPORT_ALL = BODY_REPORT_STATES | BODY_REPORT_REST | BODY_REPORT_ISLANDS | BODY_REPORT_MOVED_ONLY
BODY_STATE_MOVED, BODY_STATE_AT_REST, BODY_STATE_ISLAND_AT_REST = 1, 2, 4
# s2amdBodyState, s2amdIslandState, s2amdBodySummary
body_state_dtype = np.dtype([("slot", np.int32), ("type", np.int32), ("island", np.int32), ("flags", np.int32), ("origin", np.float32, 2),
                             ("position", np.float32, 2), ("rot", np.float32, 2), ("angle", np.float32), ("angularVelocity", np.float32),
                             ("linearVelocity", np.float32, 2), ("restTime", np.float32), ("speedSquared", np.float32)])
assert body_state_dtype.itemsize == 64
island_state_dtype = np.dtype([("firstBody", np.int32), ("bodyCount", np.int32), ("contactCount", np.int32), ("jointCount", np.int32),
                               ("restingBodies", np.int32), ("fastestBody", np.int32), ("maxSpeedSquared", np.float32), ("minRestTime", np.float32)])
assert island_state_dtype.itemsize == 32
body_summary_dtype = np.dtype([("bodies", np.int32), ("dynamicBodies", np.int32), ("kinematicBodies", np.int32), ("movedBodies", np.int32),
                               ("restingBodies", np.int32), ("islands", np.int32), ("restingIslands", np.int32), ("largestIsland", np.int32),
                               ("largestIslandBodies", np.int32), ("fastestBody", np.int32), ("maxSpeedSquared", np.float32), ("pad", np.int32, 5)])
assert body_summary_dtype.itemsize == 64

# step metrics of the resident world (include/solver2d_amd.h: s2amd_world_set_metrics)
METRICS_CONTACTS, METRICS_BODIES, METRICS_JOINTS = 1, 2, 4
METRICS_ALL = METRICS_CONTACTS | METRICS_BODIES | METRICS_JOINTS
METRICS_MAX_HISTORY = 4096
# s2amdStepMetrics
step_metrics_dtype = np.dtype([("step", np.int32), ("flags", np.int32), ("solverType", np.int32), ("dt", np.float32),
                               ("touchingContacts", np.int32), ("touchingPoints", np.int32), ("penetratingPoints", np.int32), ("approachingPoints", np.int32),
                               ("minGap", np.float32), ("minGapSlot", np.int32), ("maxApproachSpeed", np.float32), ("maxApproachSlot", np.int32),
                               ("sumPenetration", np.float32), ("sumNormalImpulse", np.float32), ("energyBodies", np.int32), ("kineticEnergy", np.float32),
                               ("potentialEnergy", np.float32), ("momentum", np.float32, 2), ("spin", np.float32),
                               ("revoluteJoints", np.int32), ("maxJointGapSlot", np.int32), ("maxJointGapSquared", np.float32), ("sumJointGapSquared", np.float32),
                               ("pad", np.int32, 8)])
assert step_metrics_dtype.itemsize == 128

# scene queries on the resident world (include/solver2d_amd.h: s2amd_world_ray_cast, s2amd_world_point_probe, s2amd_world_query_boxes)
# s2amdRay, s2amdRayHit, s2amdPointProbe, s2amdBoxQuery
ray_dtype = np.dtype([("p1", np.float32, 2), ("p2", np.float32, 2), ("maxFraction", np.float32), ("maskBits", np.uint32)])
ray_hit_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("fraction", np.float32), ("point", np.float32, 2), ("normal", np.float32, 2),
                          ("pad", np.int32)])
point_probe_dtype = np.dtype([("p", np.float32, 2), ("maskBits", np.uint32)])
box_query_dtype = np.dtype([("box", np.float32, 4), ("maskBits", np.uint32)])
RAY_SIZE, RAY_HIT_SIZE, POINT_PROBE_SIZE, BOX_QUERY_SIZE = ray_dtype.itemsize, ray_hit_dtype.itemsize, point_probe_dtype.itemsize, box_query_dtype.itemsize
assert RAY_SIZE == 24 and RAY_HIT_SIZE == 32 and POINT_PROBE_SIZE == 12 and BOX_QUERY_SIZE == 20

# proximity queries on the resident world (include/solver2d_amd.h: s2amd_world_closest_shape, s2amd_world_shapes_in_range)
# s2amdProximityQuery, s2amdProximityHit
proximity_query_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("count", np.int32), ("radius", np.float32), ("position", np.float32, 2),
                                  ("rot", np.float32, 2), ("maxDistance", np.float32), ("maskBits", np.uint32)])
proximity_hit_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("distance", np.float32), ("pointA", np.float32, 2),
                                ("pointB", np.float32, 2), ("iterations", np.int32)])
PROXIMITY_QUERY_SIZE, PROXIMITY_HIT_SIZE = proximity_query_dtype.itemsize, proximity_hit_dtype.itemsize
assert PROXIMITY_QUERY_SIZE == 96 and PROXIMITY_HIT_SIZE == 32

# sensor report of the resident world (include/solver2d_amd.h: s2amd_world_set_sensors, s2amd_world_set_sensor_report)
MAX_SENSORS = 1024
SENSOR_DISABLED, SENSOR_SKIP_STATIC = 1, 2
SENSOR_REPORT_INSIDE, SENSOR_REPORT_EVENTS, SENSOR_REPORT_STATES = 1, 2, 4
SENSOR_REPORT_ALL = SENSOR_REPORT_INSIDE | SENSOR_REPORT_EVENTS | SENSOR_REPORT_STATES
# s2amdSensor, s2amdSensorEvent, s2amdSensorState
sensor_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("count", np.int32), ("radius", np.float32), ("position", np.float32, 2),
                         ("rot", np.float32, 2), ("margin", np.float32), ("maskBits", np.uint32), ("body", np.int32), ("flags", np.int32),
                         ("pad", np.int32, 2)])
sensor_event_dtype = np.dtype([("sensor", np.int32), ("shape", np.int32), ("body", np.int32), ("sensorBody", np.int32)])
sensor_state_dtype = np.dtype([("sensor", np.int32), ("body", np.int32), ("active", np.int32), ("inside", np.int32), ("entered", np.int32),
                               ("left", np.int32), ("lowestShape", np.int32), ("pad", np.int32), ("position", np.float32, 2),
                               ("rot", np.float32, 2), ("box", np.float32, 4)])
SENSOR_SIZE, SENSOR_EVENT_SIZE, SENSOR_STATE_SIZE = sensor_dtype.itemsize, sensor_event_dtype.itemsize, sensor_state_dtype.itemsize
assert SENSOR_SIZE == 112 and SENSOR_EVENT_SIZE == 16 and SENSOR_STATE_SIZE == 64

# ray report of the resident world (include/solver2d_amd.h: s2amd_world_set_ray_sensors, s2amd_world_set_ray_report)
MAX_RAY_SENSORS = 16384
RAY_SENSOR_DISABLED, RAY_SENSOR_SKIP_STATIC = 1, 2
RAY_REPORT_STATES, RAY_REPORT_RANGES, RAY_REPORT_EVENTS = 1, 2, 4
RAY_REPORT_ALL = RAY_REPORT_STATES | RAY_REPORT_RANGES | RAY_REPORT_EVENTS
# s2amdRaySensor, s2amdRayState, s2amdRayEvent
ray_sensor_dtype = np.dtype([("p1", np.float32, 2), ("p2", np.float32, 2), ("maxFraction", np.float32), ("maskBits", np.uint32), ("body", np.int32),
                             ("flags", np.int32), ("pad", np.int32, 4)])
ray_state_dtype = np.dtype([("ray", np.int32), ("body", np.int32), ("active", np.int32), ("shape", np.int32), ("hitBody", np.int32),
                            ("shapeBefore", np.int32), ("fraction", np.float32), ("p1", np.float32, 2), ("p2", np.float32, 2),
                            ("point", np.float32, 2), ("normal", np.float32, 2), ("pad", np.int32)])
ray_event_dtype = np.dtype([("ray", np.int32), ("shapeBefore", np.int32), ("shapeNow", np.int32), ("bodyNow", np.int32)])
RAY_SENSOR_SIZE, RAY_STATE_SIZE, RAY_EVENT_SIZE = ray_sensor_dtype.itemsize, ray_state_dtype.itemsize, ray_event_dtype.itemsize
assert RAY_SENSOR_SIZE == 48 and RAY_STATE_SIZE == 64 and RAY_EVENT_SIZE == 16

# grid report of the resident world (include/solver2d_amd.h: s2amd_world_set_grid_sensors, s2amd_world_set_grid_report)
MAX_GRID_SENSORS, MAX_GRID_SIDE, MAX_GRID_CELLS = 1024, 256, 1048576
GRID_SENSOR_DISABLED, GRID_SENSOR_SKIP_STATIC = 1, 2
GRID_REPORT_CATEGORIES, GRID_REPORT_SHAPES, GRID_REPORT_OCCUPANCY, GRID_REPORT_STATES = 1, 2, 4, 8
GRID_REPORT_ALL = GRID_REPORT_CATEGORIES | GRID_REPORT_SHAPES | GRID_REPORT_OCCUPANCY | GRID_REPORT_STATES
# s2amdGridSensor, s2amdGridState
grid_sensor_dtype = np.dtype([("position", np.float32, 2), ("rot", np.float32, 2), ("cellSize", np.float32), ("width", np.int32), ("height", np.int32),
                              ("maskBits", np.uint32), ("body", np.int32), ("flags", np.int32), ("pad", np.int32, 6)])
grid_state_dtype = np.dtype([("grid", np.int32), ("body", np.int32), ("active", np.int32), ("firstCell", np.int32), ("cells", np.int32),
                             ("occupied", np.int32), ("lowestShape", np.int32), ("candidates", np.int32), ("position", np.float32, 2),
                             ("rot", np.float32, 2), ("box", np.float32, 4)])
GRID_SENSOR_SIZE, GRID_STATE_SIZE = grid_sensor_dtype.itemsize, grid_state_dtype.itemsize
assert GRID_SENSOR_SIZE == 64 and GRID_STATE_SIZE == 64

# contact queries on the resident world (include/solver2d_amd.h: s2amd_world_collide_shape, s2amd_world_deepest_contact)
# s2amdContactQuery, s2amdContactHit
contact_query_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("normals", np.float32, (8, 2)), ("type", np.int32), ("count", np.int32),
                                ("radius", np.float32), ("position", np.float32, 2), ("rot", np.float32, 2), ("maskBits", np.uint32)])
contact_hit_point_dtype = np.dtype([("localAnchorA", np.float32, 2), ("localAnchorB", np.float32, 2), ("separation", np.float32), ("id", np.uint32)])
contact_hit_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("pointCount", np.int32), ("queryIsB", np.int32), ("normal", np.float32, 2),
                              ("points", contact_hit_point_dtype, 2), ("pad", np.int32, 2)])
CONTACT_QUERY_SIZE, CONTACT_HIT_SIZE = contact_query_dtype.itemsize, contact_hit_dtype.itemsize
assert CONTACT_QUERY_SIZE == 160 and CONTACT_HIT_SIZE == 80

# shape casts on the resident world (include/solver2d_amd.h: s2amd_world_cast_shape, s2amd_world_cast_shape_all)
# s2amdShapeCast, s2amdShapeCastHit
shape_cast_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("count", np.int32), ("radius", np.float32), ("position", np.float32, 2),
                             ("rot", np.float32, 2), ("translation", np.float32, 2), ("maxFraction", np.float32), ("maskBits", np.uint32),
                             ("pad", np.int32, 2)])
shape_cast_hit_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("fraction", np.float32), ("distance", np.float32),
                                 ("point", np.float32, 2), ("normal", np.float32, 2), ("iterations", np.int32), ("pad", np.int32, 3)])
SHAPE_CAST_SIZE, SHAPE_CAST_HIT_SIZE = shape_cast_dtype.itemsize, shape_cast_hit_dtype.itemsize
assert SHAPE_CAST_SIZE == 112 and SHAPE_CAST_HIT_SIZE == 48

# move-and-slide on the resident world (include/solver2d_amd.h: s2amd_world_move_shapes): s2amdMover, s2amdMoverResult, s2amdMoverPlane
mover_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("count", np.int32), ("radius", np.float32), ("position", np.float32, 2),
                        ("rot", np.float32, 2), ("translation", np.float32, 2), ("maxIterations", np.int32), ("maskBits", np.uint32),
                        ("ignoreBody", np.int32), ("flags", np.uint32), ("reserved", np.int32, 4)])
mover_result_dtype = np.dtype([("position", np.float32, 2), ("remaining", np.float32, 2), ("status", np.int32), ("planeCount", np.int32),
                               ("iterations", np.int32), ("advances", np.int32)])
mover_plane_dtype = np.dtype([("shape", np.int32), ("body", np.int32), ("fraction", np.float32), ("distance", np.float32),
                              ("point", np.float32, 2), ("normal", np.float32, 2)])
MOVER_SIZE, MOVER_RESULT_SIZE, MOVER_PLANE_SIZE = mover_dtype.itemsize, mover_result_dtype.itemsize, mover_plane_dtype.itemsize
assert MOVER_SIZE == 128 and MOVER_RESULT_SIZE == 32 and MOVER_PLANE_SIZE == 32
MOVER_MAX_ITERATIONS, MOVER_STATIC_ONLY = 8, 1
MOVER_REACHED, MOVER_BLOCKED, MOVER_CORNERED, MOVER_OVERLAPPED, MOVER_OUT_OF_ITERATIONS = 0, 1, 2, 3, 4

# world edits on the resident world (include/solver2d_amd.h: s2amd_world_edit): s2amdWorldEdit and the S2AMD_EDIT_* kinds
world_edit_dtype = np.dtype([("kind", np.int32), ("target", np.int32), ("flag", np.int32), ("reserved", np.int32), ("v", np.float32, 4)])
WORLD_EDIT_SIZE = world_edit_dtype.itemsize
assert WORLD_EDIT_SIZE == 32
EDIT_BODY_SET_LINEAR_VELOCITY, EDIT_BODY_SET_ANGULAR_VELOCITY, EDIT_BODY_APPLY_FORCE_TO_CENTER, EDIT_BODY_APPLY_LINEAR_IMPULSE = 1, 2, 3, 4
EDIT_MOUSE_SET_TARGET, EDIT_REVOLUTE_ENABLE_LIMIT, EDIT_REVOLUTE_ENABLE_MOTOR, EDIT_REVOLUTE_SET_MOTOR_SPEED = 5, 6, 7, 8
EDIT_KINDS = {"BODY_SET_LINEAR_VELOCITY": 1, "BODY_SET_ANGULAR_VELOCITY": 2, "BODY_APPLY_FORCE_TO_CENTER": 3, "BODY_APPLY_LINEAR_IMPULSE": 4,
              "MOUSE_SET_TARGET": 5, "REVOLUTE_ENABLE_LIMIT": 6, "REVOLUTE_ENABLE_MOTOR": 7, "REVOLUTE_SET_MOTOR_SPEED": 8}


def _edit(kind, target, v=(), flag=0):
    e = np.zeros(1, dtype=world_edit_dtype)[0]
    e["kind"], e["target"], e["flag"] = kind, target, flag
    e["v"][:len(v)] = v
    return e


def edit_set_linear_velocity(body, velocity):
    return _edit(EDIT_BODY_SET_LINEAR_VELOCITY, body, velocity)


def edit_set_angular_velocity(body, w):
    return _edit(EDIT_BODY_SET_ANGULAR_VELOCITY, body, (w,))


def edit_apply_force_to_center(body, force):
    return _edit(EDIT_BODY_APPLY_FORCE_TO_CENTER, body, force)


def edit_apply_linear_impulse(body, impulse, point):
    return _edit(EDIT_BODY_APPLY_LINEAR_IMPULSE, body, tuple(impulse) + tuple(point))


def edit_mouse_set_target(joint, target):
    return _edit(EDIT_MOUSE_SET_TARGET, joint, target)


def edit_revolute_enable_limit(joint, flag):
    return _edit(EDIT_REVOLUTE_ENABLE_LIMIT, joint, flag=1 if flag else 0)


def edit_revolute_enable_motor(joint, flag):
    return _edit(EDIT_REVOLUTE_ENABLE_MOTOR, joint, flag=1 if flag else 0)


def edit_revolute_set_motor_speed(joint, speed):
    return _edit(EDIT_REVOLUTE_SET_MOTOR_SPEED, joint, (speed,))


def edit_list(edits):
    """A list of the records above (or an array of them) as one contiguous wire.world_edit_dtype array."""
    return np.ascontiguousarray(np.array(list(edits), dtype=world_edit_dtype)) if len(edits) else np.zeros(0, dtype=world_edit_dtype)


# force fields on the resident world (include/solver2d_amd.h: s2amd_world_apply_fields, s2amd_world_set_fields, s2amd_world_field_states)
MAX_FIELDS = 1024
FIELD_RADIAL, FIELD_UNIFORM, FIELD_DRAG = 1, 2, 3
FIELD_DISABLED, FIELD_AS_IMPULSE, FIELD_LINEAR_FALLOFF = 1, 2, 4
# s2amdField, s2amdFieldState
field_dtype = np.dtype([("vertices", np.float32, (8, 2)), ("count", np.int32), ("radius", np.float32), ("position", np.float32, 2),
                        ("rot", np.float32, 2), ("range", np.float32), ("maskBits", np.uint32), ("body", np.int32), ("kind", np.int32),
                        ("flags", np.int32), ("strength", np.float32), ("direction", np.float32, 2), ("reserved", np.int32), ("pad", np.int32)])
field_state_dtype = np.dtype([("field", np.int32), ("body", np.int32), ("active", np.int32), ("terms", np.int32), ("lowestShape", np.int32),
                              ("pad", np.int32, 3), ("position", np.float32, 2), ("rot", np.float32, 2), ("box", np.float32, 4)])
FIELD_SIZE, FIELD_STATE_SIZE = field_dtype.itemsize, field_state_dtype.itemsize
assert FIELD_SIZE == 128 and FIELD_STATE_SIZE == 64


def field(kind, position, range_, strength, flags=0, body=-1, direction=(0.0, 0.0), vertices=((0.0, 0.0),), radius=0.0, rot=(0.0, 1.0),
          mask=0xFFFFFFFF):
    """One wire.field_dtype record: a region (by default a point) at `position` that reaches `range_` beyond its proxy."""
    f = np.zeros(1, dtype=field_dtype)[0]
    f["vertices"][:len(vertices)] = vertices
    f["count"], f["radius"], f["position"], f["rot"], f["range"] = len(vertices), radius, position, rot, range_
    f["maskBits"], f["body"], f["kind"], f["flags"], f["strength"], f["direction"] = mask, body, kind, flags, strength, direction
    return f


def field_radial(position, range_, strength, **kw):
    return field(FIELD_RADIAL, position, range_, strength, **kw)


def field_uniform(position, range_, strength, direction, **kw):
    return field(FIELD_UNIFORM, position, range_, strength, direction=direction, **kw)


def field_drag(position, range_, strength, **kw):
    return field(FIELD_DRAG, position, range_, strength, **kw)


def field_list(fields):
    """A list of the records above (or an array of them) as one contiguous wire.field_dtype array."""
    return np.ascontiguousarray(np.array(list(fields), dtype=field_dtype)) if len(fields) else np.zeros(0, dtype=field_dtype)


# actuators on the resident world (include/solver2d_amd.h: s2amd_world_set_actuators, s2amd_world_set_actions, s2amd_world_import_actions)
MAX_ACTUATORS, MAX_ACTION_CHANNELS = 16384, 65536
ACTUATOR_BODY_FORCE, ACTUATOR_BODY_THRUST, ACTUATOR_BODY_LINEAR_VELOCITY, ACTUATOR_BODY_ANGULAR_VELOCITY = 1, 2, 3, 4
ACTUATOR_REVOLUTE_MOTOR_SPEED, ACTUATOR_REVOLUTE_SERVO, ACTUATOR_MOUSE_TARGET = 5, 6, 7
ACTUATOR_WIDTH = {1: 2, 2: 1, 3: 2, 4: 1, 5: 1, 6: 1, 7: 2}
ACTUATOR_DISABLED = 1
ACTUATOR_STATUS_APPLIED, ACTUATOR_STATUS_DISABLED, ACTUATOR_STATUS_SKIPPED, ACTUATOR_STATUS_NONFINITE = 0, 1, 2, 3
# s2amdActuator, s2amdActuatorState
actuator_dtype = np.dtype([("kind", np.int32), ("target", np.int32), ("channel", np.int32), ("flags", np.int32), ("gain", np.float32),
                           ("bias", np.float32), ("lower", np.float32), ("upper", np.float32), ("axis", np.float32, 2), ("kp", np.float32),
                           ("maxSpeed", np.float32), ("reserved", np.int32, 4)])
actuator_state_dtype = np.dtype([("actuator", np.int32), ("target", np.int32), ("status", np.int32), ("pad", np.int32), ("action", np.float32, 2),
                                 ("command", np.float32, 2), ("output", np.float32, 2), ("angle", np.float32), ("pad2", np.int32)])
ACTUATOR_SIZE, ACTUATOR_STATE_SIZE = actuator_dtype.itemsize, actuator_state_dtype.itemsize
assert ACTUATOR_SIZE == 64 and ACTUATOR_STATE_SIZE == 48


def actuator(kind, target, channel, gain=1.0, bias=0.0, lower=-np.inf, upper=np.inf, axis=(0.0, 0.0), kp=0.0, max_speed=0.0, flags=0):
    """One wire.actuator_dtype record: channels [channel, channel + ACTUATOR_WIDTH[kind]) of the action vector drive `target`."""
    a = np.zeros(1, dtype=actuator_dtype)[0]
    a["kind"], a["target"], a["channel"], a["flags"] = kind, target, channel, flags
    a["gain"], a["bias"], a["lower"], a["upper"], a["axis"], a["kp"], a["maxSpeed"] = gain, bias, lower, upper, axis, kp, max_speed
    return a


def actuator_list(actuators):
    """A list of the records above (or an array of them) as one contiguous wire.actuator_dtype array."""
    return np.ascontiguousarray(np.array(list(actuators), dtype=actuator_dtype)) if len(actuators) else np.zeros(0, dtype=actuator_dtype)


# observers on the resident world (include/solver2d_amd.h: s2amd_world_set_observers, s2amd_world_set_observation_report)
MAX_OBSERVERS, MAX_OBSERVATION_CHANNELS, MAX_OBSERVATION_FRAMES = 16384, 65536, 16
OBSERVER_BODY_POINT, OBSERVER_BODY_ROTATION, OBSERVER_BODY_ANGLE, OBSERVER_BODY_LINEAR_VELOCITY, OBSERVER_BODY_ANGULAR_VELOCITY = 1, 2, 3, 4, 5
OBSERVER_REVOLUTE_ANGLE, OBSERVER_REVOLUTE_SPEED, OBSERVER_REVOLUTE_MOTOR_IMPULSE = 6, 7, 8
OBSERVER_BODY_CONTACT, OBSERVER_RAY_RANGE, OBSERVER_ACTION = 9, 10, 11
OBSERVER_WIDTH = {1: 2, 2: 2, 3: 1, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1, 9: 2, 10: 1, 11: 1}
OBSERVER_DISABLED, OBSERVER_RELATIVE = 1, 2
OBSERVER_STATUS_OBSERVED, OBSERVER_STATUS_DISABLED, OBSERVER_STATUS_SKIPPED, OBSERVER_STATUS_SOURCE_OFF = 0, 1, 2, 3
OBSERVATION_REPORT_VECTOR, OBSERVATION_REPORT_STATES = 1, 2
# s2amdObserver, s2amdObserverState
observer_dtype = np.dtype([("kind", np.int32), ("target", np.int32), ("frame", np.int32), ("channel", np.int32), ("flags", np.int32),
                           ("gain", np.float32), ("bias", np.float32), ("lower", np.float32), ("upper", np.float32), ("local", np.float32, 2),
                           ("reserved", np.int32, 5)])
observer_state_dtype = np.dtype([("observer", np.int32), ("status", np.int32), ("raw", np.float32, 2), ("value", np.float32, 2), ("pad", np.int32, 2)])
OBSERVER_SIZE, OBSERVER_STATE_SIZE = observer_dtype.itemsize, observer_state_dtype.itemsize
assert OBSERVER_SIZE == 64 and OBSERVER_STATE_SIZE == 32


def observer(kind, target, channel, frame=-1, gain=1.0, bias=0.0, lower=-np.inf, upper=np.inf, local=(0.0, 0.0), flags=0):
    """One wire.observer_dtype record: `target`'s quantity `kind` goes to channels [channel, channel + OBSERVER_WIDTH[kind]) of the
    observation vector, expressed in body `frame`'s frame (-1: the world's)."""
    o = np.zeros(1, dtype=observer_dtype)[0]
    o["kind"], o["target"], o["frame"], o["channel"], o["flags"] = kind, target, frame, channel, flags
    o["gain"], o["bias"], o["lower"], o["upper"], o["local"] = gain, bias, lower, upper, local
    return o


def observer_list(observers):
    """A list of the records above (or an array of them) as one contiguous wire.observer_dtype array."""
    return np.ascontiguousarray(np.array(list(observers), dtype=observer_dtype)) if len(observers) else np.zeros(0, dtype=observer_dtype)


# episodes on the resident world (include/solver2d_amd.h: s2amd_world_set_episodes, s2amd_world_set_episode_report)
MAX_EPISODE_AGENTS, MAX_EPISODE_RULES = 16384, 65536
EPISODE_REWARD_VALUE, EPISODE_REWARD_TEST, EPISODE_TERMINATE, EPISODE_TRUNCATE = 1, 2, 3, 4
EPISODE_SHAPE_LINEAR, EPISODE_SHAPE_ABS, EPISODE_SHAPE_SQUARE = 0, 1, 2
EPISODE_RULE_DISABLED, EPISODE_RULE_DIFFERENCE, EPISODE_RULE_OUTSIDE = 1, 2, 4
EPISODE_STATUS_EVALUATED, EPISODE_STATUS_DISABLED, EPISODE_STATUS_SKIPPED, EPISODE_STATUS_SOURCE_OFF = 0, 1, 2, 3
EPISODE_TERMINATED, EPISODE_TRUNCATED, EPISODE_TIME_LIMIT = 1, 2, 4
EPISODE_REPORT_STEP, EPISODE_REPORT_STATES, EPISODE_REPORT_RULE_STATES, EPISODE_REPORT_EVENTS = 1, 2, 4, 8
EPISODE_REPORT_ALL = 15
# s2amdEpisodeRule, s2amdEpisodeState, s2amdEpisodeRuleState, s2amdEpisodeEvent
episode_rule_dtype = np.dtype([("kind", np.int32), ("agent", np.int32), ("channelA", np.int32), ("frameA", np.int32), ("channelB", np.int32),
                               ("frameB", np.int32), ("shape", np.int32), ("flags", np.int32), ("gain", np.float32), ("bias", np.float32),
                               ("lower", np.float32), ("upper", np.float32), ("reserved", np.int32, 4)])
episode_state_dtype = np.dtype([("flags", np.int32), ("rule", np.int32), ("reward", np.float32), ("episodeReturn", np.float32),
                                ("episodeLength", np.int32), ("episodes", np.int32), ("lastReturn", np.float32), ("lastLength", np.int32)])
episode_rule_state_dtype = np.dtype([("rule", np.int32), ("status", np.int32), ("x", np.float32), ("f", np.float32), ("value", np.float32),
                                     ("fired", np.int32), ("pad", np.int32, 2)])
episode_event_dtype = np.dtype([("agent", np.int32), ("flags", np.int32), ("episodeLength", np.int32), ("episodeReturn", np.float32)])
EPISODE_RULE_SIZE, EPISODE_STATE_SIZE, EPISODE_RULE_STATE_SIZE, EPISODE_EVENT_SIZE = (episode_rule_dtype.itemsize, episode_state_dtype.itemsize,
                                                                                      episode_rule_state_dtype.itemsize, episode_event_dtype.itemsize)
assert (EPISODE_RULE_SIZE, EPISODE_STATE_SIZE, EPISODE_RULE_STATE_SIZE, EPISODE_EVENT_SIZE) == (64, 32, 32, 16)


def episode_rule(kind, agent, channel=-1, frame=0, minus=None, shape=0, gain=1.0, bias=0.0, lower=-np.inf, upper=np.inf, flags=0):
    """One wire.episode_rule_dtype record of agent `agent`: x = obs[frame][channel] (channel -1: no source, x = +0); with
    minus=(channelB, frameB) the DIFFERENCE flag is set and x = obs[frame][channel] - obs[frameB][channelB]."""
    r = np.zeros(1, dtype=episode_rule_dtype)[0]
    r["kind"], r["agent"], r["channelA"], r["frameA"], r["shape"], r["flags"] = kind, agent, channel, frame, shape, flags
    if minus is not None:
        r["channelB"], r["frameB"] = minus
        r["flags"] |= EPISODE_RULE_DIFFERENCE
    r["gain"], r["bias"], r["lower"], r["upper"] = gain, bias, lower, upper
    return r


def episode_rule_list(rules):
    """A list of the records above (or an array of them) as one contiguous wire.episode_rule_dtype array."""
    return np.ascontiguousarray(np.array(list(rules), dtype=episode_rule_dtype)) if len(rules) else np.zeros(0, dtype=episode_rule_dtype)


# resets on the resident world (include/solver2d_amd.h: s2amd_world_set_resets, s2amd_world_set_reset_report, s2amd_world_reset_agents)
MAX_RESET_AGENTS, MAX_RESET_BODIES, MAX_RESET_JOINTS = 16384, 65536, 65536
RESET_DISABLED, RESET_JOINT_SETTINGS = 1, 2
RESET_ON_EPISODE_END, RESET_REPORT_STATES = 1, 2
RESET_ALL = -1
# the counts of a pass, in order
RESET_COUNT_AGENTS, RESET_COUNT_BODIES, RESET_COUNT_BODIES_SKIPPED, RESET_COUNT_JOINTS, RESET_COUNT_JOINTS_SKIPPED, RESET_COUNT_SHAPES, RESET_COUNT_CONTACTS, RESET_COUNT_SOURCE_OFF = range(8)
# s2amdResetBody, s2amdResetJoint, s2amdResetState
reset_body_dtype = np.dtype([("agent", np.int32), ("body", np.int32), ("flags", np.int32), ("position", np.float32, 2), ("rot", np.float32, 2),
                             ("linearVelocity", np.float32, 2), ("angularVelocity", np.float32), ("positionJitter", np.float32, 2),
                             ("velocityJitter", np.float32, 2), ("angularJitter", np.float32), ("reserved", np.int32)])
reset_joint_dtype = np.dtype([("agent", np.int32), ("joint", np.int32), ("flags", np.int32), ("enableMotor", np.int32), ("enableLimit", np.int32),
                              ("motorSpeed", np.float32), ("targetA", np.float32, 2)])
reset_state_dtype = np.dtype([("resets", np.int32), ("triggered", np.int32), ("pad", np.int32, 2)])
RESET_BODY_SIZE, RESET_JOINT_SIZE, RESET_STATE_SIZE = reset_body_dtype.itemsize, reset_joint_dtype.itemsize, reset_state_dtype.itemsize
assert (RESET_BODY_SIZE, RESET_JOINT_SIZE, RESET_STATE_SIZE) == (64, 32, 16)


def resets_from_world(bodies, joints, agent_of_body, agent_of_joint, joint_flags=RESET_JOINT_SETTINGS):
    """The reset records of the arrays a caller uploads: one body record per body slot with agent_of_body[slot] >= 0 that is neither
    free nor static, holding the slot's pose and velocities with no jitter, and one joint record per live joint slot with
    agent_of_joint[slot] >= 0, holding the slot's settings (flags = joint_flags).  -> (wire.reset_body_dtype array, wire.reset_joint_dtype
    array), each in slot order."""
    agent_of_body, agent_of_joint = np.asarray(agent_of_body, dtype=np.int32), np.asarray(agent_of_joint, dtype=np.int32)
    assert len(agent_of_body) == len(bodies) and len(agent_of_joint) == len(joints)
    slots = np.flatnonzero((agent_of_body >= 0) & (bodies["type"] != BODY_FREE) & (bodies["type"] != BODY_STATIC))
    rb = np.zeros(len(slots), dtype=reset_body_dtype)
    rb["agent"], rb["body"] = agent_of_body[slots], slots
    for name in ("position", "rot", "linearVelocity", "angularVelocity"):
        rb[name] = bodies[name][slots]
    slots = np.flatnonzero((agent_of_joint >= 0) & (joints["type"] != JOINT_FREE))
    rj = np.zeros(len(slots), dtype=reset_joint_dtype)
    rj["agent"], rj["joint"], rj["flags"] = agent_of_joint[slots], slots, joint_flags
    for name in ("enableMotor", "enableLimit", "motorSpeed", "targetA"):
        rj[name] = joints[name][slots]
    return rb, rj
