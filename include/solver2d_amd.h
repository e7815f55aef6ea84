/*
 * solver2d_amd.h -- C-ABI of the MI355X constraint-solve hot path.
 *
 * This is the drop-in boundary for the ten solver variants of erincatto/solver2d.  The
 * reference's plug point is
 *
 *     void s2Solve_<Variant>(s2World* world, s2StepContext* context);   (src/solvers.h:70-79)
 *
 * called from the switch in s2World_Step (src/world.c:206-256).  Each s2Solve_* reads and
 * mutates three pooled arrays -- world->bodies (src/body.h:16-76), world->contacts with their
 * embedded s2Manifold (src/contact.h:44-61, include/solver2d/manifold.h:19-46) and
 * world->joints (src/joint.h:28-103) -- and nothing else.  The structs below are plain-C
 * mirrors of exactly the fields those functions touch, indexed the same way (array index ==
 * pool index, free slots flagged), so a reference-side shim is a field-for-field gather
 * before the call and a scatter after it.
 *
 * Plain pointers and sizes only; no C++ / torch / HIP types cross this boundary.
 * All functions return 0 on success and a negative S2AMD_E_* code on failure;
 * s2amd_last_error() returns a human readable message for the calling thread.
 */
#ifndef SOLVER2D_AMD_H
#define SOLVER2D_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2AMD_API_VERSION 5

/* error codes */
#define S2AMD_OK 0
#define S2AMD_E_INVALID (-1)   /* bad argument (null pointer, negative size, unknown solver) */
#define S2AMD_E_DEVICE (-2)    /* HIP runtime failure (message has the hipError string) */
#define S2AMD_E_NODEVICE (-3)  /* no gfx950 device visible: the library never falls back to the CPU */
#define S2AMD_E_STATE (-4)     /* call sequence error (e.g. step_resident before upload) */
#define S2AMD_E_CAPACITY (-5)  /* output buffer too small */

/* Solver selector: values and order are the reference ABI (include/solver2d/types.h:75-88). */
typedef enum s2amdSolverType
{
	s2amd_solverJacobi = 0,
	s2amd_solverPGS = 1,
	s2amd_solverPGS_NGS = 2,
	s2amd_solverPGS_NGS_Block = 3,
	s2amd_solverPGS_Soft = 4,
	s2amd_solverSoftStep = 5,
	s2amd_solverTGS_Sticky = 6,
	s2amd_solverTGS_Soft = 7,
	s2amd_solverTGS_NGS = 8,
	s2amd_solverXPBD = 9,
	s2amd_solverTypeCount = 10
} s2amdSolverType;

/* Body type values are the reference's s2BodyType (types.h:99-105); -1 marks a free pool slot
 * (s2IsFree, src/pool.h). */
#define S2AMD_BODY_FREE (-1)
#define S2AMD_BODY_STATIC 0
#define S2AMD_BODY_KINEMATIC 1
#define S2AMD_BODY_DYNAMIC 2

/* Solver-visible part of s2Body (src/body.h:16-76).  In/out fields are marked. */
typedef struct s2amdBody
{
	float position[2];       /* in/out  center of mass, body.h:24 */
	float rot[2];            /* in/out  {s, c}, body.h:34 */
	float linearVelocity[2]; /* in/out  body.h:39 */
	float angularVelocity;   /* in/out  body.h:40 */
	float deltaPosition[2];  /* in/out  body.h:27 (zero between steps except kinematic bodies under XPBD) */
	float localCenter[2];    /* in      body.h:37 */
	float force[2];          /* in      body.h:49 */
	float torque;            /* in      body.h:50 */
	float mass, invMass;     /* in      body.h:61 */
	float I, invI;           /* in      body.h:64 */
	float linearDamping;     /* in      body.h:66 */
	float angularDamping;    /* in      body.h:67 */
	float gravityScale;      /* in      body.h:68 */
	int32_t type;            /* in      S2AMD_BODY_* */
} s2amdBody;

/* s2ManifoldPoint (include/solver2d/manifold.h:19-38) minus id/persisted, which no solver reads. */
typedef struct s2amdManifoldPoint
{
	float localAnchorA[2];    /* in  relative to body origin */
	float localAnchorB[2];    /* in */
	float frictionAnchorA[2]; /* in/out TGS_Sticky only (solve_tgs_sticky.c:87-163) */
	float frictionAnchorB[2]; /* in/out */
	float frictionNormalA[2]; /* in/out */
	float frictionNormalB[2]; /* in/out */
	float separation;         /* in */
	float normalImpulse;      /* in/out (warm start in, stored impulse out) */
	float tangentImpulse;     /* in/out */
} s2amdManifoldPoint;

/* s2Contact as the solvers see it (src/contact.h:44-61): body indices from edges[0/1].bodyIndex,
 * mixed friction, and the manifold.  pointCount == 0 marks a slot the gather loop skips
 * (free contact or no manifold points; e.g. src/solve_tgs_soft.c:162-179). */
typedef struct s2amdContact
{
	int32_t bodyA, bodyB;
	int32_t pointCount;        /* 0, 1 or 2 */
	int32_t frictionPersisted; /* in/out TGS_Sticky, manifold.h:45 */
	float normal[2];
	float friction;
	int32_t constraintIndex;   /* out  manifold.constraintIndex written by the gather loop; -1 if skipped */
	s2amdManifoldPoint points[2];
} s2amdContact;

#define S2AMD_JOINT_FREE (-1)
#define S2AMD_JOINT_REVOLUTE 0 /* s2_revoluteJoint, src/joint.h:17 */
#define S2AMD_JOINT_MOUSE 1    /* s2_mouseJoint,   src/joint.h:18 */

/* Persistent part of s2Joint + s2RevoluteJoint / s2MouseJoint (src/joint.h:28-103).  The
 * "solver temp" members are recomputed by every prepare function and never cross the boundary. */
typedef struct s2amdJoint
{
	int32_t type; /* S2AMD_JOINT_* */
	int32_t bodyA, bodyB;
	int32_t enableMotor, enableLimit; /* revolute */
	float localOriginAnchorA[2], localOriginAnchorB[2];
	float impulse[2];   /* in/out revolute + mouse */
	float motorImpulse; /* in/out revolute + mouse */
	float lowerImpulse; /* in/out revolute */
	float upperImpulse; /* in/out revolute */
	float maxMotorTorque, motorSpeed, referenceAngle, lowerAngle, upperAngle; /* revolute */
	float hertz, dampingRatio; /* mouse */
	float targetA[2];          /* mouse */
} s2amdJoint;

/* The arguments of s2World_Step (include/solver2d/solver2d.h:25) + world->gravity and
 * world->solverType; s2StepContext (src/solvers.h:13-24) is derived from these exactly as
 * src/world.c:170-202 does. */
typedef struct s2amdStepParams
{
	int32_t solverType; /* s2amdSolverType */
	float dt;
	int32_t velIters;
	int32_t posIters;
	int32_t warmStart;
	float gravity[2];
} s2amdStepParams;

/* Wall/device timing of the last step (filled by s2amd_solve / s2amd_step_resident). */
typedef struct s2amdStepStats
{
	int32_t constraintCount;   /* active contact constraints this step */
	int32_t jointCount;        /* active joints */
	int32_t contactColors;     /* colour batches of the contact graph (0 for Jacobi contacts) */
	int32_t jointColors;
	int32_t solveSweeps;       /* full passes of a s2SolveContacts_* kernel family this step */
	int32_t kernelLaunches;    /* launches enqueued for the step */
	float deviceMs;            /* HIP-event time of the whole device step */
	float solveKernelMs;       /* HIP-event time summed over the individual contact solve-sweep launches (0 unless profiling is on) */
	float hostPrepMs;          /* host time spent colouring/packing */
	int32_t graphReplayed;     /* 1 when the step ran as a hipGraph replay */
	int32_t solveLaunches;     /* contact solve-sweep kernel launches timed into solveKernelMs (profiling only) */
	float eventPairOverheadMs; /* elapsed time of an EMPTY HIP event pair on the stream (profiling only): subtract per launch */
	int32_t groupCount;        /* LDS groups (small islands advanced whole-step by one workgroup each) */
	int32_t messagePassing;    /* 1 when the big-island sweeps read bodies from per-constraint copies (no gather) */
	int32_t stripCount;        /* strips (BFS level ranges) a big island was cut into: phase A workgroups per sweep */
	int32_t seamCount;         /* seams between adjacent strips that carry constraints: phase B workgroups per sweep */
	int32_t persistent;        /* 1 when the strips ran as ONE persistent launch (constraints resident in registers all step) */
	int32_t persistFallbacks;  /* times a persistent step was abandoned (workgroups not co-resident) and repeated on the multi-launch path */
	int32_t structureBuilds;   /* full builds of the constraint-graph structure (islands, colours, tables) since s2amd_create */
	int32_t placedContacts;    /* created contacts that were given a place in the existing structure instead (no build) */
	int32_t potentialConstraints; /* contact slots the structure holds: constraintCount + manifolds without points + destroyed contacts not yet dropped */
	int32_t pairLanes;         /* (API 2) which persistent kernel ran: 2 = 512 threads per strip (wide_kernel.hip), 1 = two lanes per constraint (pair_kernel.hip), 0 = strip_kernel.hip */
	int32_t asyncBuildsRequested; /* (API 3) structure builds handed to the worker thread since s2amd_create (world chain: the strip structure, the strip-width search) */
	int32_t asyncBuildsAdopted;   /* (API 3) ... whose result replaced the live structure (the others were overtaken by the graph) */
	float asyncWaitMs;            /* (API 3) time the caller spent waiting for a worker that was not done when its build fell due, since s2amd_create */
	int32_t bodiesAdopted;        /* (API 3) bodies without constraints that moved to the strip of the body they first touched (no build), in the structure in use */
	int32_t seamBodiesAdded;      /* (API 3) bodies a seam between two strips came to carry after the build (one more export / import of its strips) */
	int32_t roundsOpened;         /* (API 3) spare colour rounds of strips and seams opened for created contacts */
	int32_t overflowContacts;     /* (API 4) contacts that fit nowhere in the strips and wait in the overflow positions behind them for a worker thread's structure (0: none) */
	int32_t slicedStep;           /* (API 4) 1: this step ran sliced -- the persistent strip kernel launched once per sweep, the overflow contacts swept behind each launch */
	int32_t slicedSteps;          /* (API 4) ... steps that did, since s2amd_create */
	int32_t nearHandoffTimeouts;  /* (API 3) hand-off time-outs while the same-XCD path (workgroup-scope stores between neighbours on one L2) was in use: the step was tried again with agent-scope stores, which the solver keeps */
} s2amdStepStats;

typedef struct s2amdSolver s2amdSolver;

/* ---- lifecycle ---- */
int s2amd_api_version(void);
int s2amd_device_count(void);
/* (API 2) PCI bus id of HIP device `device` ("0000:05:00.0"): what tells two ranks' GPUs apart (bench.py: ranks_seen / devices). */
int s2amd_device_bus_id(int device, char* out, int32_t capacity);
const char* s2amd_last_error(void);
/* The floating-point contract this library was compiled under: "fp-contract=off" (libs2amd.so: every result equal to the
 * reference's, bit for bit -- the reference's own build, gcc -O2 on x86-64 without -mfma, contracts nothing) or
 * "fp-contract=fast" (libs2amd_fast.so, the tolerance mode: the compiler may fuse a*b+c into one rounding; results within
 * the tolerances DESIGN.md section 2 states and tests/test_gpu_fast.py checks).  A static string. */
const char* s2amd_build_flags(void);
/* device: HIP ordinal.  Fails with S2AMD_E_NODEVICE when no GPU is visible. */
int s2amd_create(int device, s2amdSolver** out);
void s2amd_destroy(s2amdSolver* solver);

/* ---- drop-in entry point: == s2Solve_<params->solverType>(world, context) ----
 * Host arrays in, same arrays mutated on return (bodies: position/rot/velocities/deltaPosition;
 * contacts: impulses, constraintIndex, sticky cache; joints: impulses).  Any of the array
 * pointers may be NULL when its count is 0. */
int s2amd_solve(s2amdSolver* solver, const s2amdStepParams* params, s2amdBody* bodies, int32_t bodyCapacity,
				s2amdContact* contacts, int32_t contactCapacity, s2amdJoint* joints, int32_t jointCapacity);

/* ---- split phases, for callers that keep the world resident in HBM ---- */
int s2amd_upload(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdContact* contacts,
				 int32_t contactCapacity, const s2amdJoint* joints, int32_t jointCapacity);
/* One s2Solve_* on the resident arrays; results stay on the device (impulses are stored back
 * into the resident contact array, so consecutive calls warm start like consecutive steps). */
int s2amd_step_resident(s2amdSolver* solver, const s2amdStepParams* params);
int s2amd_download(s2amdSolver* solver, s2amdBody* bodies, int32_t bodyCapacity, s2amdContact* contacts,
				   int32_t contactCapacity, s2amdJoint* joints, int32_t jointCapacity);
/* Snapshot / restore of the resident body array on the device (bench: re-solve one snapshot). */
int s2amd_save_bodies(s2amdSolver* solver);
/* With option "async" = 1, s2amd_step_resident returns once the step is enqueued on the solver's stream (no
 * device time in the stats); this call waits for everything enqueued so far and reports a deferred device error. */
int s2amd_synchronize(s2amdSolver* solver);
int s2amd_restore_bodies(s2amdSolver* solver);

/* ---- the stages either side of the solver ---- */

/* Shape type values are the reference's s2ShapeType (src/shape.h:14-21). */
#define S2AMD_SHAPE_FREE (-1)
#define S2AMD_SHAPE_CAPSULE 0
#define S2AMD_SHAPE_CIRCLE 1
#define S2AMD_SHAPE_POLYGON 2
#define S2AMD_SHAPE_SEGMENT 3

/* The part of s2Shape (src/shape.h:23-47) that Stage 4 of s2World_Step (AABB refit,
 * src/world.c:259-301) and the broad phase (src/broad_phase.c:166-307) read and write.
 * Geometry: polygon = vertices[0..count) + radius; circle = vertices[0] center, radius;
 * capsule = vertices[0], vertices[1], radius; segment = vertices[0], vertices[1]. */
typedef struct s2amdShape
{
	int32_t body;          /* s2Shape.bodyIndex; -1 with type S2AMD_SHAPE_FREE for a free pool slot */
	int32_t type;          /* S2AMD_SHAPE_* */
	uint32_t categoryBits; /* s2Filter, include/solver2d/types.h:141-146 */
	uint32_t maskBits;
	int32_t groupIndex;
	int32_t proxyKey;      /* (tree proxy id << 4) | body type, src/broad_phase.h:18-20: orders a pair's A/B */
	int32_t enlarged;      /* out of s2amd_refit_shapes: fat AABB grew, the proxy enters the move buffer */
	int32_t count;         /* polygon vertex count */
	float radius;
	float aabb[4];         /* in/out {lower.x, lower.y, upper.x, upper.y} */
	float fatAABB[4];      /* in/out */
	float vertices[8][2];
	float normals[8][2];   /* polygon edge normals (s2Polygon.normals, include/solver2d/geometry.h:44-50): read by the narrow phase */
} s2amdShape;

/* == Stage 4 of s2World_Step (src/world.c:259-301) for every non-static body: origin = position -
 * R * localCenter (written to origins[2 * body]), per shape the tight AABB + speculative margin, and
 * the fat AABB re-inflated where the tight one escaped it (`enlarged` = 1).  Host arrays in and out. */
int s2amd_refit_shapes(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, s2amdShape* shapes, int32_t shapeCapacity,
					   float* origins);

/* == the pair discovery of s2UpdateBroadPhasePairs (src/broad_phase.c:166-307): every moved proxy
 * (moved[shape] != 0) against every proxy whose fat AABB overlaps its own, with the reference's
 * rules (dynamic queries all three trees, kinematic only the dynamic one; no self pairs; when both
 * moved the lower proxy key reports; existing pairs, same-body pairs, filtered pairs and bodies
 * connected by a joint are skipped; shape A is the one with the lower proxy key), followed by
 * s2CreateContact's type rules (src/contact.c:137-175): segment/segment pairs are dropped, a pair
 * whose shape-type order has no primary manifold function is flipped.
 * existingPairs: shapeIndexA/B of the live contacts.  Output: the NEW pairs, sorted by (A, B) -- the
 * same SET the reference creates contacts for.  The reference's creation ORDER is a function of its own
 * trees (move-array order, then s2DynamicTree_Query's traversal order reversed, broad_phase.c:253-254,
 * :332-357): the caller, who owns those trees and the contact pool, sorts the set on that key before
 * calling s2CreateContact (shim/s2_amd_binding.c: s2amdBinding_OrderPairs), which gives every contact
 * the reference's pool slot.  Returns S2AMD_E_CAPACITY (with *pairCount = needed) when outPairs is too small. */
int s2amd_find_pairs(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdShape* shapes, int32_t shapeCapacity,
					 const uint8_t* moved, const int32_t* existingPairs, int32_t existingPairCount, const s2amdJoint* joints,
					 int32_t jointCapacity, int32_t* outPairs, int32_t pairCapacity, int32_t* pairCount);

/* Narrow-phase state of one contact slot that persists between steps: the shape pair, the GJK simplex cache
 * (s2DistanceCache, include/solver2d/distance.h:31-37, a member of s2Contact) and per manifold point the feature
 * id and `persisted` flag (s2ManifoldPoint, include/solver2d/manifold.h:19-38). */
typedef struct s2amdPairState
{
	int32_t shapeA, shapeB; /* s2Contact.shapeIndexA/B; -1: free contact slot */
	float cacheMetric;
	uint16_t cacheCount;
	uint16_t id[2];
	uint8_t cacheIndexA[3];
	uint8_t cacheIndexB[3];
	uint8_t persisted[2];
	uint8_t pad[2];
} s2amdPairState;

#define S2AMD_PAIR_UPDATED 0   /* manifold recomputed */
#define S2AMD_PAIR_SEPARATED 1 /* fat AABBs no longer overlap: the caller destroys the contact (src/world.c:149-167) */
#define S2AMD_PAIR_FREE (-1)

/* == Stage 3 of s2World_Step, "update contacts" (src/world.c:132-168): for every live contact slot whose shapes'
 * fat AABBs still overlap, s2UpdateContact (src/contact.c:296-358): the manifold function of the shape-type pair
 * (src/manifold.c: s2CollideCircles, s2CollideCapsuleAndCircle, s2CollidePolygonAndCircle, s2CollidePolygons with
 * its GJK distance query src/distance.c:485-604, SAT fallback and clipper; capsules and segments go through the
 * polygon path exactly as the reference's s2MakeCapsule does), then the id matching that carries impulses and the
 * sticky-friction cache from the old manifold to the new one.
 * In:  bodies (rot), origins[2 * body] (s2Body.origin: s2amd_refit_shapes writes them), shapes (geometry in the
 *      body frame, fatAABB), pairs, contacts (the old manifolds).
 * Out: contacts (pointCount, normal, points, frictionPersisted; bodyA/B, friction and constraintIndex are kept),
 *      pairs (ids, persisted, cache), status[contact] = S2AMD_PAIR_*.  Host arrays in and out. */
int s2amd_update_contacts(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const float* origins, const s2amdShape* shapes,
						  int32_t shapeCapacity, s2amdPairState* pairs, s2amdContact* contacts, int32_t contactCapacity, int32_t* status);

/* ---- resident world: stage 3, the solve and stage 4 of s2World_Step chained in HBM ----
 * The stage functions above take host arrays in and out.  These three keep the shapes, the pair states and the body
 * origins on the device beside the bodies / contacts / joints of s2amd_upload, so a step moves 32 bytes of counters, read
 * back once, after stage 4.  The constraint-graph structure (islands, colours, strips) covers every live pair slot
 * whether its manifold has points or not, so manifolds that gain or lose their points cost the host nothing; it is
 * touched when contact slots are written.  Pair creation (stage 1, src/world.c:125-130) stays with the caller: when
 * movedCount > 0 it downloads the shapes, runs s2amd_find_pairs, creates its contacts and uploads again, as the
 * reference does before the next step's stage 3. */
typedef struct s2amdWorldStepInfo
{
	int32_t separatedCount; /* pairs whose fat AABBs parted: destroyed on the device (pointCount 0, pair slot free,
	                           src/world.c:149-167); status[] of s2amd_world_download says which */
	int32_t activeContacts; /* manifolds with points after stage 3 */
	int32_t graphChanged;   /* a manifold went between zero and non-zero points this step.  Informational: the solve's structure
	                           covers every live pair slot, with or without points, and is only rebuilt when contact slots are
	                           written (s2amd_world_set_contacts) */
	int32_t movedCount;     /* shapes whose fat AABB the refit re-inflated (s2amdShape.enlarged) */
	float contactsMs;       /* host wall time of enqueueing stage 3 (its counters come back with the step's one read-back) */
	float solveMs;          /* device time of the s2Solve_* part (HIP events) */
	float stepMs;           /* host wall time of the whole call */
} s2amdWorldStepInfo;

/* bodies/contacts/joints as s2amd_upload; shapes (with valid aabb/fatAABB), pairs[contactCapacity] (the narrow-phase
 * state of every contact slot), origins[2 * bodyCapacity] (s2Body.origin). */
int s2amd_world_upload(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdContact* contacts, int32_t contactCapacity,
					   const s2amdJoint* joints, int32_t jointCapacity, const s2amdShape* shapes, int32_t shapeCapacity, const s2amdPairState* pairs,
					   const float* origins);
/* == s2World_Step without stage 1: update contacts (src/world.c:132-168), s2Solve_* (src/world.c:206-256), refit
 * (src/world.c:259-301).  info may be NULL. */
int s2amd_world_step(s2amdSolver* solver, const s2amdStepParams* params, s2amdWorldStepInfo* info);
/* == the pair discovery of stage 1 (s2amd_find_pairs above) on the resident shapes: moved = the shapes the last refit
 * enlarged, existing pairs = the live pair slots, jointed bodies as uploaded.  New pairs sorted by (A, B) into the host
 * array outPairs.  Call it when info.movedCount > 0, before the next s2amd_world_step (the refit overwrites the flags).
 * A successful query consumes the move buffer as s2UpdateBroadPhasePairs does (src/broad_phase.c: moveArray and moveSet
 * are cleared): every shape's `enlarged` flag is zero afterwards, static shapes included. */
int s2amd_world_find_pairs(s2amdSolver* solver, int32_t* outPairs, int32_t pairCapacity, int32_t* pairCount);
/* The contact slots whose pairs the last s2amd_world_step found separated (fat AABBs apart) and destroyed on the device, in
 * ascending order: the slots the caller's own pool frees (s2DestroyContact, src/world.c:163-167).  info.separatedCount of them. */
int s2amd_world_separated(s2amdSolver* solver, int32_t* slots, int32_t capacity, int32_t* count);
/* What stage 4 (src/world.c:259-297) changed in a shape, without the rest of the 196-byte record: the tight box of every live
 * shape, its fat box, and whether the refit re-inflated it (== the shapes s2BroadPhase_EnlargeProxy is called for). */
typedef struct s2amdShapeBox
{
	float aabb[4];
	float fatAABB[4];
	int32_t enlarged;
} s2amdShapeBox;
/* boxes[shapeCapacity of the upload]: the boxes of the resident shapes after the last s2amd_world_step (36 bytes per shape
 * instead of s2amd_world_download's whole shape records). */
int s2amd_world_download_boxes(s2amdSolver* solver, s2amdShapeBox* boxes, int32_t shapeCapacity);
/* (API 2) The per-step read-back of a caller that keeps its own copy of the world and its own broad-phase trees (the binding,
 * shim/s2_amd_binding.c): after an s2amd_world_step, instead of the whole body and box arrays,
 *   poses[4 * body]  {origin.x, origin.y, rot.s, rot.c} of every body slot (what s2Body_GetPosition / GetAngle read), and
 *   moved[]          the shapes whose fat box the refit re-inflated (src/world.c:283-290), with the new fat box, IN THE ORDER the
 *                    reference's refit visits them -- `shapeOrder` of s2amd_world_set_refit_order: bodies in pool order, each
 *                    body's shape list -- which is the order s2BroadPhase_EnlargeProxy puts them into the move buffer in.
 * *movedCount == s2amdWorldStepInfo.movedCount of that step.  A new s2amd_world_upload forgets the order (send it again).  Velocities, manifolds, tight boxes stay in HBM until somebody
 * asks for them (s2amd_world_download / _download_boxes). */
typedef struct s2amdMovedBox
{
	int32_t shape;
	float fatAABB[4];
} s2amdMovedBox;
int s2amd_world_set_refit_order(s2amdSolver* solver, const int32_t* shapeOrder, int32_t count);
int s2amd_world_download_step(s2amdSolver* solver, float* poses, int32_t bodyCapacity, s2amdMovedBox* moved, int32_t movedCapacity, int32_t* movedCount);
/* (API 5) The reference's broad-phase trees on the device.  s2UpdateBroadPhasePairs creates a step's contacts in the order its tree
 * queries call back (src/broad_phase.c:253-254, :288-320, :332-357: move-buffer order of the asking proxies; per proxy the trees in
 * reverse query order and each tree's callbacks reversed), and that order decides every new contact's pool slot.  It is a function of
 * the topology of the reference's three trees (src/broad_phase.h:27), which is history: stage 2 rebuilds only what stage 4 flagged
 * (s2DynamicTree_Rebuild(tree, false), src/dynamic_tree.c:1764-1874).  A caller that hands the device those trees once --
 *   s2amd_world_set_tree(solver, bodyType, tree.nodes, tree.nodeCapacity, tree.root)   for s2_staticBody, s2_kinematicBody, s2_dynamicBody
 * after s2amd_world_upload, in the state stage 2 leaves them in (no internal node flagged `enlarged`; refused otherwise) -- gets
 *   - s2amd_world_step keeping them as the reference would: its stage 2 rebuilds them (same topology, same node ids, same boxes),
 *     its stage 4 enlarges the proxies of the shapes it re-inflates (src/world.c:283-290, src/dynamic_tree.c:803-839);
 *   - s2amd_world_find_pairs returning the new pairs IN THE REFERENCE'S CREATION ORDER instead of sorted by (A, B): calling
 *     s2CreateContact down the list gives every contact the reference's pool slot (the position of an asking proxy in the move buffer
 *     is its shape's position in the refit order of s2amd_world_set_refit_order; without one, its shape index);
 *   - s2amd_world_get_tree copying a tree back (node array as the reference would hold it now -- the free list's nodes are untouched
 *     by a rebuild, which takes exactly the nodes it frees, src/dynamic_tree.c:105-139 -- and the root), for the caller's own
 *     s2DynamicTree when it needs one: s2World_QueryAABB, s2World_Draw, a proxy created or destroyed.
 * A new s2amd_world_upload forgets the trees.  s2amdTreeNode is s2TreeNode byte for byte (include/solver2d/dynamic_tree.h:14-41). */
typedef struct s2amdTreeNode
{
	float aabb[4];
	uint32_t categoryBits;
	int32_t parent; /* `next` of a free node */
	int32_t child1, child2;
	int32_t userData;
	int16_t height; /* leaf 0, free node -1 */
	uint8_t enlarged;
	uint8_t pad[9];
} s2amdTreeNode;
int s2amd_world_set_tree(s2amdSolver* solver, int32_t bodyType, const s2amdTreeNode* nodes, int32_t nodeCapacity, int32_t root);
int s2amd_world_get_tree(s2amdSolver* solver, int32_t bodyType, s2amdTreeNode* nodes, int32_t nodeCapacity, int32_t* root);
/* Writes `count` contact slots of the resident world (slot indices < contactCapacity of the upload): the caller's
 * s2CreateContact (src/contact.c:137-203: pool slot, pair flip, mixed friction, empty manifold) or s2DestroyContact
 * (pairs[i].shapeA = -1, contacts[i].pointCount = 0).  A world that needs more slots, bodies or shapes is uploaded again. */
int s2amd_world_set_contacts(s2amdSolver* solver, const int32_t* slots, int32_t count, const s2amdContact* contacts, const s2amdPairState* pairs);
/* Any output pointer may be NULL.  status[contactCapacity]: S2AMD_PAIR_* of the last step's stage 3. */
int s2amd_world_download(s2amdSolver* solver, s2amdBody* bodies, int32_t bodyCapacity, s2amdContact* contacts, int32_t contactCapacity,
						 s2amdJoint* joints, int32_t jointCapacity, s2amdShape* shapes, int32_t shapeCapacity, s2amdPairState* pairs, float* origins,
						 int32_t* status);

/* (additive, API 5) The contact report: what touches what, and how hard, without moving the world.  s2World_Draw's contact pass
 * (src/world.c:486-561) reads, for every valid contact, manifold.pointCount and manifold.normal and, per point, localAnchorA through
 * S2_TRANSFORM(bodyA), separation, persisted, normalImpulse and tangentImpulse; a sensor, a foot-contact force or a "began touching"
 * trigger reads the same.  With a report flag set, s2amd_world_step compacts that on the device behind its stage 4, in a defined order,
 * and the three getters below hand it out; with no flag set (the default) a step enqueues what it always did.
 *   A contact slot is TOUCHING after a step when its pair slot is live and pointCount > 0 after that step's stage 3 (src/world.c:132-168):
 *   the contacts the solve swept.
 *   S2AMD_REPORT_TOUCH     `began`: the slots touching now that were not touching before the step; `ended`: the reverse -- a pair stage 3
 *                          found separated and destroyed while it was touching is in `ended`.  Both ascending.  "Before" is, after
 *                          s2amd_world_upload, pointCount > 0 of the uploaded contacts (resting manifolds report no begin), and a slot
 *                          written by s2amd_world_set_contacts takes pointCount > 0 of what was written: no event, the caller did that itself.
 *                          A step the library repeats internally (a lost hand-off) reports once, as finally executed.
 *   S2AMD_REPORT_CONTACTS  one s2amdTouchingContact per touching slot, ascending: point[j] = s2TransformPoint({origin, rot} of bodyA after
 *                          the step, localAnchorA) in the operation order of include/solver2d/math.h:350-356 -- what a s2World_Draw called
 *                          right after the step would draw (src/world.c:518) --, persisted from s2amdPairState, everything else from the
 *                          resident contact; the entries of unused points are zero.
 *   S2AMD_REPORT_BODY_SUMS per body slot, static ones included: with P = s2Add(s2MulSV(normalImpulse, normal), s2MulSV(tangentImpulse,
 *                          s2RightPerp(normal))) of a contact point (src/solve_common.c:304-314), `impulse` is the float32 sum, from +0, left
 *                          to right over the body's touching contacts in ascending slot order, points in index order, of -P where the body
 *                          is bodyA and +P where it is bodyB; `normalImpulse` the same ordered sum of the points' normalImpulse; `touching`
 *                          the number of contacts.  No floating-point atomics: the result is a pure function of the arrays.
 * Every getter describes the last s2amd_world_step: S2AMD_E_STATE without a resident world, when its flag was not set before that step or
 * no step has run since; S2AMD_E_CAPACITY when a buffer is too small -- the counts are set, nothing is consumed, the caller asks again
 * (as s2amd_world_find_pairs).  s2amd_world_set_report: S2AMD_E_INVALID for unknown bits; the flags hold from the next step on, across
 * uploads.  The step itself gains no host wait: the getters wait for what they need. */
#define S2AMD_REPORT_TOUCH 1     /* begin / end lists */
#define S2AMD_REPORT_CONTACTS 2  /* one record per touching contact */
#define S2AMD_REPORT_BODY_SUMS 4 /* per body: net contact impulse, normal load, touching count */
int s2amd_world_set_report(s2amdSolver* solver, int32_t flags);
typedef struct s2amdTouchingContact /* 64 bytes */
{
	int32_t slot, bodyA, bodyB;
	uint8_t pointCount, persisted[2], pad; /* persisted: s2amdPairState.persisted */
	float normal[2];
	float point[2][2]; /* world space, as src/world.c:518 computes it */
	float separation[2], normalImpulse[2], tangentImpulse[2];
} s2amdTouchingContact;
typedef struct s2amdBodyContactSum /* 16 bytes */
{
	float impulse[2];
	float normalImpulse;
	int32_t touching;
} s2amdBodyContactSum;
int s2amd_world_touch_events(s2amdSolver* solver, int32_t* began, int32_t beganCapacity, int32_t* beganCount, int32_t* ended,
							 int32_t endedCapacity, int32_t* endedCount);
int s2amd_world_touching(s2amdSolver* solver, s2amdTouchingContact* out, int32_t capacity, int32_t* count);
/* out[bodyCapacity of the upload] */
int s2amd_world_body_sums(s2amdSolver* solver, s2amdBodyContactSum* out, int32_t bodyCapacity);

/* (additive, API 5) The joint report: the joint half of what s2World_Draw, a ragdoll controller or a "what breaks" test reads -- anchors,
 * angles, speeds, limit contacts, motor torque, reactions -- without moving the world.  s2World_Draw's joint pass (src/world.c:423,
 * s2DrawJoint src/joint.c:469-505, s2DrawRevolute src/revolute_joint.c:942-984) and s2RevoluteJoint_GetMotorTorque
 * (src/revolute_joint.c:929-940) read the same.  It has a setter and a flag space of its own (the contact report's flags above are
 * unchanged); with a flag set, s2amd_world_step compacts the report on the device behind its stage 4 and behind the contact report,
 * and the four getters below hand it out; with no flag set (the default) a step enqueues nothing for it.
 * Everything is float32, one rounding per operation in the order stated, read from the resident arrays AFTER the step's stage 4:
 * origins, bodies.rot, bodies.angularVelocity and the joints.  A joint slot is LIVE when type != S2AMD_JOINT_FREE.
 *   anchorB (every type)  s2TransformPoint({origin, rot} of bodyB, localOriginAnchorB), include/solver2d/math.h:350-356 (src/joint.c:474-477).
 *   revolute record       anchorA the same transform of bodyA's localOriginAnchorA; angle = s2RelativeAngle(rotB, rotA) - referenceAngle
 *                         (math.h:320-327 with glibc's atan2f, src/revolute_joint.c:190); angularSpeed = wB - wA;
 *                         axialImpulse = (motorImpulse + lowerImpulse) - upperImpulse (src/revolute_joint.c:137); impulse, motorImpulse,
 *                         lowerImpulse and upperImpulse as stored.
 *   mouse record          anchorA = targetA verbatim (what src/joint.c:485-492 draws); angle, lowerImpulse, upperImpulse = +0 whatever the
 *                         wire record holds; angularSpeed = wB; axialImpulse = motorImpulse (src/mouse_joint.c:102-103).
 *   S2AMD_JOINT_REPORT_STATES     one s2amdJointState per live slot, ascending by slot.
 *   S2AMD_JOINT_REPORT_LIMITS     a revolute joint with enableLimit != 0 is AT ITS LOWER LIMIT when the stored lowerImpulse > 0 and AT ITS
 *                         UPPER LIMIT when upperImpulse > 0.  `began`: the codes 2 * slot + side (side 0 lower, 1 upper) at the limit now
 *                         that were not before the step; `ended`: the reverse.  Both ascending.  "Before" is, after s2amd_world_upload,
 *                         the same rule on the uploaded joints.  A step the library repeats internally reports once, as finally
 *                         executed (the report owns its state bytes).  The report states what the solver STORES: a solver that stores
 *                         no limit impulses reports no events -- s2Solve_XPBD leaves lowerImpulse and upperImpulse at zero.
 *   S2AMD_JOINT_REPORT_BODY_SUMS  per body slot, static and free ones included: sums from +0, left to right over the body's live joints in
 *                         ascending slot order, within one joint the bodyA term before the bodyB term.  A revolute joint adds -impulse
 *                         and -axialImpulse where the body is its bodyA, +impulse and +axialImpulse where it is its bodyB
 *                         (src/revolute_joint.c:140-144); a mouse joint adds +impulse and +motorImpulse to its bodyB only and adds and
 *                         counts nothing for its bodyA.  `joints` is the number of terms.  No floating-point atomics: the result is a
 *                         pure function of the arrays.  (The body -> joint adjacency is built at s2amd_world_upload and when the report
 *                         is turned on: no resident-world call changes a joint's type, bodyA or bodyB in between.)
 *   s2amd_world_joint_summary   answers whenever ANY joint-report flag was set before the last step: the live and revolute joint counts,
 *                         atLower / atUpper by the rule above, and the largest anchor gap: over the live revolute joints,
 *                         g = dx * dx + dy * dy with d = anchorB - anchorA; the largest g wins, ties go to the lowest slot
 *                         (maxGapSlot), a NaN g never wins; with no revolute joint (or none whose g is a number) maxGapSquared = -1.0f
 *                         and maxGapSlot = -1.
 * Errors as the contact report's: S2AMD_E_STATE without a resident world, when the getter's flag was not set before the last
 * s2amd_world_step or no step has run since; S2AMD_E_CAPACITY when a buffer is too small -- the counts are set, nothing is consumed;
 * s2amd_world_set_joint_report: S2AMD_E_INVALID for unknown bits; the flags hold from the next step on, across uploads.  The step gains
 * no host wait: the getters wait. */
#define S2AMD_JOINT_REPORT_STATES 1    /* one s2amdJointState per live joint slot */
#define S2AMD_JOINT_REPORT_LIMITS 2    /* limit began / ended lists */
#define S2AMD_JOINT_REPORT_BODY_SUMS 4 /* per body: net joint impulse, axial impulse, joint count */
int s2amd_world_set_joint_report(s2amdSolver* solver, int32_t flags);
typedef struct s2amdJointState /* 64 bytes */
{
	int32_t slot, type, bodyA, bodyB;
	float anchorA[2], anchorB[2]; /* world space */
	float impulse[2];
	float axialImpulse, motorImpulse;
	float angle, angularSpeed;
	float lowerImpulse, upperImpulse;
} s2amdJointState;
typedef struct s2amdBodyJointSum /* 16 bytes */
{
	float impulse[2];
	float axialImpulse;
	int32_t joints;
} s2amdBodyJointSum;
typedef struct s2amdJointSummary /* 32 bytes */
{
	int32_t liveJoints, revoluteJoints, atLower, atUpper;
	int32_t maxGapSlot;
	float maxGapSquared;
	int32_t pad[2];
} s2amdJointSummary;
int s2amd_world_joint_states(s2amdSolver* solver, s2amdJointState* out, int32_t capacity, int32_t* count);
/* began / ended hold up to 2 * jointCapacity codes each */
int s2amd_world_joint_limit_events(s2amdSolver* solver, int32_t* began, int32_t beganCapacity, int32_t* beganCount, int32_t* ended,
								   int32_t endedCapacity, int32_t* endedCount);
/* out[bodyCapacity of the upload] */
int s2amd_world_body_joint_sums(s2amdSolver* solver, s2amdBodyJointSum* out, int32_t bodyCapacity);
int s2amd_world_joint_summary(s2amdSolver* solver, s2amdJointSummary* out);

/* (additive, API 5) The shape report: the shape half of what s2World_Draw, a culling pass, a camera fit or a "left the arena" trigger reads
 * -- world-space vertices, the body's class, the boxes, what is on screen -- without moving the world.  s2World_Draw's shape pass
 * (src/world.c:373-410, s2DrawShape :308-367) and its AABB pass (:427-460) read the same.  It has a setter and a flag space of its own
 * (the flags of the two reports above are unchanged); with a flag set, s2amd_world_step compacts the report on the device behind its
 * stage 4 and behind the joint report, and the three getters below hand it out; with no flag set (the default) a step enqueues nothing
 * for it.  Everything is float32, one rounding per operation in the order stated, read from the resident arrays AFTER the step's stage 4:
 * shapes, origins, bodies.rot, bodies.type and bodies.mass.
 *   A shape slot is LIVE when type != S2AMD_SHAPE_FREE.  A live shape is IN VIEW when no view is set, or when
 *   s2AABB_Overlaps(view, shape.aabb) holds as include/solver2d/aabb.h:111-123 writes it: false only when one of the four differences
 *   aabb.lower - view.upper, view.lower - aabb.upper is > 0 -- a box that touches the view's edge is in view, and so is one with a NaN.
 *   s2amd_world_set_shape_view   box = {lower.x, lower.y, upper.x, upper.y}, NULL: no view, every live shape is in view (the default).
 *                         S2AMD_E_INVALID for lower > upper or a NaN.  Holds from the next step on, across uploads.
 *   S2AMD_SHAPE_REPORT_DRAW    one s2amdShapeDraw per live shape in view, ascending by shape slot.  With the transform {origins[body],
 *                         bodies[body].rot}: vertices[i] = s2TransformPoint(transform, shape.vertices[i]) in the operation order of
 *                         include/solver2d/math.h:350-356 for i < vertexCount -- a polygon's count (taken as 0 below 0 and 8 above 8),
 *                         2 for a capsule and a segment, 1 for a circle -- and +0 beyond; axis = s2RotateVector(rot, {1, 0})
 *                         (math.h:330-341: {c * 1 - s * 0, s * 1 + c * 0}) for every type; bodyClass by the precedence of
 *                         src/world.c:389-405: 3 for a dynamic body with mass == 0.0f before anything else, then 0 static, 1 kinematic,
 *                         2 otherwise; radius, aabb and fatAABB verbatim.  The record names no colours: the class is what the
 *                         reference picks them by.
 *   S2AMD_SHAPE_REPORT_VIEW    `entered`: the shape slots in view now that were not in view before the step; `left`: the reverse.  Both
 *                         ascending.  "Before" is the same rule on the resident shapes, evaluated at s2amd_world_upload, when the report
 *                         is turned on and when s2amd_world_set_shape_view changes the view: the caller's own acts raise no events, and
 *                         the step after a change of view reports against the new view.  A step the library repeats internally reports
 *                         once, as finally executed (the report owns its state bytes).
 *   S2AMD_SHAPE_REPORT_BOUNDS / s2amd_world_shape_summary   answers whenever ANY shape-report flag was set before the last step: liveShapes;
 *                         inView; byType[t] the live shapes of type t = S2AMD_SHAPE_CAPSULE .. S2AMD_SHAPE_SEGMENT; badBodyShapes the
 *                         live shapes on bodies of class 3; movableBounds over shape.aabb of the live shapes whose body is neither
 *                         static nor free; viewBounds over shape.aabb of the shapes in view, static ones included.  A box starts as
 *                         {+INF, +INF, -INF, -INF} -- also the answer when no shape qualifies -- and takes the shapes in ascending slot
 *                         order: lower = x < cur ? x : cur, upper = x > cur ? x : cur.  A NaN never wins.
 * Errors as the other reports': S2AMD_E_STATE without a resident world, when the getter's flag was not set before the last
 * s2amd_world_step or no step has run since; S2AMD_E_CAPACITY when a buffer is too small -- the counts are set, nothing is consumed;
 * s2amd_world_set_shape_report: S2AMD_E_INVALID for unknown bits; the flags hold from the next step on, across uploads.  The step gains
 * no host wait: the getters wait. */
#define S2AMD_SHAPE_REPORT_DRAW 1   /* one s2amdShapeDraw per live shape in view */
#define S2AMD_SHAPE_REPORT_VIEW 2   /* entered / left lists */
#define S2AMD_SHAPE_REPORT_BOUNDS 4 /* summary incl. world bounds */
int s2amd_world_set_shape_report(s2amdSolver* solver, int32_t flags);
int s2amd_world_set_shape_view(s2amdSolver* solver, const float* box /* {lx,ly,ux,uy}; NULL = everything */);
typedef struct s2amdShapeDraw /* 128 bytes = two 64-byte lines */
{
	int32_t shape, body, type, vertexCount; /* valid entries of vertices[]: polygon count; capsule, segment 2; circle 1 */
	int32_t bodyClass;                      /* 0 static, 1 kinematic, 2 dynamic, 3 dynamic with mass == 0 */
	float radius;
	float axis[2];                          /* s2RotateVector(rot, {1, 0}) */
	float vertices[8][2];                   /* world space; unused entries +0 */
	float aabb[4], fatAABB[4];              /* as resident after stage 4 */
} s2amdShapeDraw;
typedef struct s2amdShapeSummary /* 64 bytes */
{
	int32_t liveShapes, inView, byType[4], badBodyShapes, pad;
	float movableBounds[4];                 /* over live shapes of non-static bodies */
	float viewBounds[4];                    /* over the shapes in view, static ones included */
} s2amdShapeSummary;
int s2amd_world_shape_draws(s2amdSolver* solver, s2amdShapeDraw* out, int32_t capacity, int32_t* count);
/* entered / left hold up to shapeCapacity slots each */
int s2amd_world_shape_view_events(s2amdSolver* solver, int32_t* entered, int32_t enteredCapacity, int32_t* enteredCount, int32_t* left,
								  int32_t leftCapacity, int32_t* leftCount);
int s2amd_world_shape_summary(s2amdSolver* solver, s2amdShapeSummary* out);

/* (additive, API 5) The body report: what a HUD, a trail, a sound trigger, a recorder or a "may I stop stepping" test asks of the bodies
 * -- velocities, which poses changed, which bodies came to rest or woke up, which islands exist and whether a whole pile is at rest --
 * without moving the world.  The fourth setter and flag space (the flags of the three reports above are unchanged); with a flag set,
 * s2amd_world_step compacts the report on the device behind its stage 4 and behind the shape report, and the getters below hand it out;
 * with no flag set (the default) a step enqueues nothing for it.  The reference has no sleeping and the solve skips nobody: "at rest" is
 * something the report says, never something the step acts on.  Everything is float32, one rounding per operation in the order stated,
 * read from the resident arrays AFTER the step's stage 4: bodies, origins, contacts, joints.
 *   A body slot is REPORTED when its type is neither S2AMD_BODY_FREE nor S2AMD_BODY_STATIC.
 *   S2AMD_BODY_REPORT_STATES   one s2amdBodyState per reported body, ascending by slot: origin = origins[slot]; position, rot and the
 *                         velocities verbatim; angle = s2Rot_GetAngle(rot) = atan2f(rot.s, rot.c) (include/solver2d/math.h:267-270, what
 *                         s2Body_GetAngle returns; glibc's atan2f); speedSquared = vx * vx + vy * vy; restTime the body's timer (below);
 *                         island the index into the island list, -1 without ISLANDS; flags bit 0 MOVED, bit 1 AT REST, bit 2 the body's
 *                         island is at rest (0 without ISLANDS).
 *   MOVED                 the 16 bytes {origin.x, origin.y, rot.s, rot.c}, compared as four uint32, differ from the copy the report keeps
 *                         from before the step.  The copy is taken at s2amd_world_upload and when the report is turned on (flags from 0 to
 *                         non-zero), and refreshed by every reporting step.
 *   S2AMD_BODY_REPORT_MOVED_ONLY   modifies STATES: only the reported bodies that moved are listed.
 *   S2AMD_BODY_REPORT_REST     The report owns one float timer per body slot: +0 after an upload and whenever the flags go from 0 to non-zero.
 *                         A step with ANY flag set advances the timer of every reported body: the body is a candidate when
 *                         speedSquared <= lin2 && w * w <= ang2 (a NaN on either side fails), lin2 = linearSpeed * linearSpeed and
 *                         ang2 = angularSpeed * angularSpeed rounded once on the host; timer = candidate ? timer + dt : +0 with that
 *                         step's params->dt.  AT REST: timer >= seconds.  `rested`: the slots at rest now that were not at rest before
 *                         the step; `woke`: the reverse; both ascending.  "At rest before" is the same rule on the timer as it stood
 *                         before the step under the thresholds as they are now, so s2amd_world_set_rest_thresholds -- the caller's own
 *                         act -- raises no event.  A step with every flag at 0 advances nothing.
 *   s2amd_world_set_rest_thresholds   defaults 0.01f, 0.0349065850f (2 degrees / s), 0.5f; S2AMD_E_INVALID for a negative value or a NaN
 *                         (the thresholds that hold stay); holds from the next step on, across uploads.
 *   S2AMD_BODY_REPORT_ISLANDS  the islands of the world as it stands after the step, by the rule of s2amd_find_islands below on the
 *                         resident arrays: MOVABLE bodies (reported, invMass != 0 || invI != 0) are joined by contacts with
 *                         pointCount > 0 and by revolute joints between two of them; every other reported body is an island of its own;
 *                         an edge that names a body outside [0, bodyCapacity) joins nothing.  Islands are numbered by their lowest body
 *                         slot, which is firstBody.  A touching contact / a live joint counts (contactCount, jointCount) for the island
 *                         of bodyA when bodyA is movable, else for that of bodyB when it is movable, else for none; a mouse joint looks at
 *                         bodyB only.  restingBodies: the island's bodies at rest -- the island is AT REST when that equals bodyCount;
 *                         minRestTime the minimum of their timers; fastestBody / maxSpeedSquared the largest speedSquared, of equal ones
 *                         the lowest slot, a NaN never wins, -1 and -1.0f when every speed is a NaN.
 *   s2amd_world_body_summary   answers whenever ANY body-report flag was set before the last step: bodies (reported), dynamicBodies,
 *                         kinematicBodies, movedBodies, restingBodies; islands, restingIslands, largestIsland (most bodies, of equal ones
 *                         the lowest index), largestIslandBodies -- 0, 0, -1, 0 without ISLANDS; fastestBody / maxSpeedSquared by the
 *                         per-island rule over all reported bodies; pad is 0.
 * Errors as the other reports': S2AMD_E_STATE without a resident world, when the getter's flag was not set before the last
 * s2amd_world_step or no step has run since; S2AMD_E_CAPACITY when a buffer is too small -- the counts are set, nothing is consumed;
 * s2amd_world_set_body_report: S2AMD_E_INVALID for unknown bits; the flags hold from the next step on, across uploads.  The step gains
 * no host wait: the getters wait.  A step the library repeats internally reports once, as finally executed.
 * Byte for byte this is what libs2amd.so returns; libs2amd_fast.so builds the same code under its own contraction rule
 * (speedSquared and w * w may be fused there). */
#define S2AMD_BODY_REPORT_STATES 1     /* one s2amdBodyState per reported body */
#define S2AMD_BODY_REPORT_REST 2       /* rested / woke lists */
#define S2AMD_BODY_REPORT_ISLANDS 4    /* islands of the world as it stands after the step */
#define S2AMD_BODY_REPORT_MOVED_ONLY 8 /* modifies STATES: only bodies whose pose changed in the step */
#define S2AMD_BODY_STATE_MOVED 1
#define S2AMD_BODY_STATE_AT_REST 2
#define S2AMD_BODY_STATE_ISLAND_AT_REST 4
int s2amd_world_set_body_report(s2amdSolver* solver, int32_t flags);
int s2amd_world_set_rest_thresholds(s2amdSolver* solver, float linearSpeed, float angularSpeed, float seconds);
typedef struct s2amdBodyState /* 64 bytes = one line */
{
	int32_t slot, type, island, flags; /* flags: S2AMD_BODY_STATE_* */
	float origin[2], position[2], rot[2]; /* rot = {s, c} */
	float angle, angularVelocity;
	float linearVelocity[2];
	float restTime, speedSquared;
} s2amdBodyState;
typedef struct s2amdIslandState /* 32 bytes */
{
	int32_t firstBody, bodyCount, contactCount, jointCount, restingBodies, fastestBody;
	float maxSpeedSquared, minRestTime;
} s2amdIslandState;
typedef struct s2amdBodySummary /* 64 bytes */
{
	int32_t bodies, dynamicBodies, kinematicBodies, movedBodies, restingBodies;
	int32_t islands, restingIslands, largestIsland, largestIslandBodies, fastestBody;
	float maxSpeedSquared;
	int32_t pad[5];
} s2amdBodySummary;
int s2amd_world_body_states(s2amdSolver* solver, s2amdBodyState* out, int32_t capacity, int32_t* count);
/* rested / woke hold up to bodyCapacity slots each */
int s2amd_world_body_rest_events(s2amdSolver* solver, int32_t* rested, int32_t restedCapacity, int32_t* restedCount, int32_t* woke,
								 int32_t wokeCapacity, int32_t* wokeCount);
int s2amd_world_islands(s2amdSolver* solver, s2amdIslandState* out, int32_t capacity, int32_t* count);
int s2amd_world_body_summary(s2amdSolver* solver, s2amdBodySummary* out);

/* (additive, API 5) The step metrics: how well the solver did in a step -- how deep the contacts still sit, how fast bodies still
 * approach, whether the energy drifts, whether the joints pull apart -- without moving the world, and with a history: what the samples of
 * the reference are watched for.  A fifth, independent facility behind the four reports (their flags are unchanged); with a flag set,
 * every s2amd_world_step reduces the world as it stands after its stage 4 -- what s2amd_world_download would return -- to ONE 128-byte
 * s2amdStepMetrics on the device and stores it in a ring in device memory; s2amd_world_metrics hands out the last record,
 * s2amd_world_metrics_history the whole history in one read.  With no flag set (the default) a step enqueues nothing for it.
 * Everything is float32, one rounding per operation in the order stated, read from the resident arrays AFTER the step's stage 4:
 * bodies, origins, contacts, pairs, joints.
 *   o_X = origins[X]; q_X = bodies[X].rot = {s, c}; T(X, p) = s2TransformPoint({o_X, q_X}, p) (include/solver2d/math.h:350-356):
 *   ((c * p.x - s * p.y) + o.x, (s * p.x + c * p.y) + o.y).
 *   PSUM                  the one shape of every float sum.  The terms are indexed by slot over the array's whole capacity; a slot that
 *                         contributes nothing has the term +0.0f.  The slots are cut into tiles of 256 consecutive slots, the last tile
 *                         padded with +0.0f.  Inside a tile, eight levels: at level k = 0..7, t[i] = t[i] + t[i + 2^k] for every i that is
 *                         a multiple of 2^(k+1) (in numpy, eight rounds of x = x[:, 0::2] + x[:, 1::2]).  The tile sums are then added left
 *                         to right from +0.0f.  No floating-point atomics: the result is a pure function of the arrays.  Of a sum that is
 *                         a NaN only "is a NaN" is specified, not its bits.
 *   S2AMD_METRICS_CONTACTS   A contact slot is TOUCHING as the contact report defines it (pair slot live, pointCount > 0), and not
 *                         touching when it names a body outside [0, bodyCapacity); pointCount above 2 counts as 2.  For point j of a
 *                         touching slot with bodies A, B and n = normal: d = T(B, localAnchorB) - T(A, localAnchorA) componentwise;
 *                         gap = (d.x * n.x + d.y * n.y) + separation.  For X in {A, B}: a = localAnchorX - localCenter_X;
 *                         r = (c * a.x - s * a.y, s * a.x + c * a.y); u_X = (v.x - w * r.y, v.y + w * r.x) with X's velocities;
 *                         e = u_B - u_A; vn = e.x * n.x + e.y * n.y.
 *                         touchingContacts, touchingPoints: the counts.  penetratingPoints: the points with gap < -0.005f
 *                         (s2_linearSlop); approachingPoints: those with vn < 0.  minGap / minGapSlot: the smallest gap; of equal gaps
 *                         the lowest slot (inside a slot the lower point) wins, a NaN never wins; +0.0f and -1 without a point whose gap
 *                         is a number.  maxApproachSpeed / maxApproachSlot: the largest -vn over the points with vn < 0 under the same
 *                         rules; +0.0f and -1 with none.  sumPenetration: PSUM over the contact slots, a touching slot's term p0 for one
 *                         point and p0 + p1 for two, p = gap < 0 ? -gap : +0.0f.  sumNormalImpulse: the same PSUM with the points'
 *                         normalImpulse.
 *   S2AMD_METRICS_BODIES  over the body slots whose type is neither S2AMD_BODY_FREE nor S2AMD_BODY_STATIC; energyBodies their count.
 *                         Each a PSUM over the body slots: kineticEnergy of ((0.5f * mass) * (vx * vx + vy * vy)) + ((0.5f * I) * (w * w));
 *                         potentialEnergy of -((mass * gravityScale) * (gx * position.x + gy * position.y)) with that step's
 *                         params->gravity; momentum of mass * vx and mass * vy; spin of I * w.
 *   S2AMD_METRICS_JOINTS  over the live revolute joints: g = dx * dx + dy * dy, d = T(bodyB, localOriginAnchorB) - T(bodyA,
 *                         localOriginAnchorA) (a body outside the array stands at the origin, unrotated, as in the joint report).
 *                         revoluteJoints the count; maxJointGapSquared / maxJointGapSlot exactly by the rule of
 *                         s2amd_world_joint_summary: the largest g, ties to the lowest slot, a NaN never wins, -1.0f and -1 with none;
 *                         sumJointGapSquared: PSUM of g over the joint slots.
 *   Every record          step: the number of records written since the recorder was restarted; flags: as set; solverType, dt: that
 *                         step's params.  The fields of a section whose flag is off are zero bytes; pad is 0.
 *   The recorder          s2amd_world_set_metrics: S2AMD_E_INVALID for unknown bits, and for a historyLength outside 1..4096 while
 *                         flags != 0 (the length is ignored when flags is 0; what was set before stays).  Every accepted call restarts
 *                         the recorder -- the ring is empty, the next record has step 0 --, and so does every s2amd_world_upload.  Flags
 *                         and length hold from the next step on, across uploads.  A step with flags != 0 writes one record into ring
 *                         position step % historyLength; a step with flags 0 writes nothing and advances nothing.  A step the library
 *                         repeats internally records once, as finally executed.
 *   s2amd_world_metrics   the last step's record; S2AMD_E_STATE without a resident world, when no step has run since the restart, or
 *                         when the flags were 0 before the last step.
 *   s2amd_world_metrics_history   the last min(records written, historyLength) records, oldest first: their `step` values are
 *                         consecutive.  *count is always set (it may be 0); S2AMD_E_CAPACITY when capacity < *count -- nothing is
 *                         consumed; S2AMD_E_STATE without a resident world or with the recorder off.  Reading never clears the ring.
 * The step gains no host wait: the getters wait.
 * Byte for byte this is what libs2amd.so returns; libs2amd_fast.so builds the same code under its own contraction rule (the products
 * that feed an addition may be fused there). */
#define S2AMD_METRICS_CONTACTS 1 /* gaps, approach speeds, penetration and impulse sums of the touching contacts */
#define S2AMD_METRICS_BODIES 2   /* energy, momentum and spin of the non-static bodies */
#define S2AMD_METRICS_JOINTS 4   /* anchor gaps of the revolute joints */
#define S2AMD_METRICS_MAX_HISTORY 4096
int s2amd_world_set_metrics(s2amdSolver* solver, int32_t flags, int32_t historyLength);
typedef struct s2amdStepMetrics /* 128 bytes */
{
	int32_t step, flags, solverType;
	float dt;
	int32_t touchingContacts, touchingPoints, penetratingPoints, approachingPoints;
	float minGap;
	int32_t minGapSlot;
	float maxApproachSpeed;
	int32_t maxApproachSlot;
	float sumPenetration, sumNormalImpulse;
	int32_t energyBodies;
	float kineticEnergy;
	float potentialEnergy, momentum[2], spin;
	int32_t revoluteJoints, maxJointGapSlot;
	float maxJointGapSquared, sumJointGapSquared;
	int32_t pad[8];
} s2amdStepMetrics;
int s2amd_world_metrics(s2amdSolver* solver, s2amdStepMetrics* out);
int s2amd_world_metrics_history(s2amdSolver* solver, s2amdStepMetrics* out, int32_t capacity, int32_t* count);

/* (additive, API 5) Scene queries: "what is here?" asked of the resident world -- a mouse pick, a sensor sweep, a line-of-sight test --
 * without a host copy of the shapes or the trees.  The reference's world query is s2World_QueryAABB (src/world.c:605-615); picking in its
 * samples is that query followed by s2Shape_TestPoint (src/shape.c:110-137); its ray functions are s2RayCastCircle / Capsule / Segment /
 * Polygon (src/geometry.c:393-730) and s2DynamicTree_RayCast (src/dynamic_tree.c:1213-1290).  The three batched calls below answer from the
 * resident arrays.  They describe the world as it stands -- after the last s2amd_world_upload, s2amd_world_step or
 * s2amd_world_set_contacts --, are enqueued behind it on the solver's stream, may be called any number of times between steps, change
 * nothing resident, add no host wait to a step, and do not need the device trees of s2amd_world_set_tree.  S2AMD_E_STATE without a
 * resident world; count == 0 succeeds and touches nothing.  Every answer is an order-free statement:
 *   A shape slot is LIVE when type != S2AMD_SHAPE_FREE.  xf(body) = {origins[body], bodies[body].rot}, the resident arrays S2_TRANSFORM
 *   reads.  A shape s PASSES a query q when (s.categoryBits & q.maskBits) != 0, as in the trees' filtered walks
 *   (src/dynamic_tree.c:1145, :1253).
 *   s2amd_world_query_boxes   the hits of box q: the live shapes that pass and satisfy s2AABB_Overlaps(fatAABB, q.box)
 *                             (include/solver2d/aabb.h:111), ascending by slot.  With maskBits 0xFFFFFFFF this is the set s2World_QueryAABB
 *                             calls back for, in every world whose shapes have non-zero category bits.
 *   s2amd_world_point_probe   candidates: live, passing, s2AABB_Overlaps(fatAABB, {p, p}).  A candidate is a hit when s2PointInCircle /
 *                             Capsule / Polygon(s2InvTransformPoint(xf(body), p), geometry) is true (src/shape.c:110-137; s2PointInPolygon
 *                             is the GJK call of src/geometry.c:376-389); segments never hit.  Ascending by slot.
 *   Both lists come in CSR form: the hits of query i are shapes[offsets[i] .. offsets[i + 1]), *total = offsets[count].  When capacity <
 *   *total the call returns S2AMD_E_CAPACITY with offsets and *total filled and shapes untouched; the caller asks again (as
 *   s2amd_world_find_pairs).
 *   s2amd_world_ray_cast      s2IsValidRay (src/geometry.c:15-20) is checked on the host for every ray before anything is enqueued: one
 *                             failing ray makes the whole call return S2AMD_E_INVALID with hits untouched (the reference only asserts).
 *                             The segment box runs from s2Min(p1, t) to s2Max(p1, t) with t = s2MulAdd(p1, maxFraction, s2Sub(p2, p1))
 *                             (src/dynamic_tree.c:1231-1238).  Candidates: live, passing, s2AABB_Overlaps(fatAABB, segment box) -- no other
 *                             pruning decides a result.  For a candidate both p1 and p2 go through s2InvTransformPoint(xf(body), .),
 *                             maxFraction unchanged, then s2RayCast<type>, capsules through the circle fallbacks as src/geometry.c:450-581.
 *                             The answer is the candidate with hit == true and the smallest fraction, compared as float values (-0 equals
 *                             +0), ties to the lowest shape slot.  fraction = the winner's own bits; normal = s2RotateVector(rot,
 *                             output.normal); point = s2MulAdd(p1, fraction, s2Sub(p2, p1)) on the world-space inputs; body = the shape's
 *                             body.  No hit: shape = body = -1, fraction = maxFraction, the rest +0.
 *                             The reference has no world-level ray cast: this composition is ours -- the closest-hit use of
 *                             s2DynamicTree_RayCast restated without its traversal order (shrinking maxFraction during a walk only changes
 *                             hit or no-hit for shapes beyond the current best).
 * All arithmetic is fp32 in the reference's operation order without contraction, with correctly rounded divide and square root, in
 * libs2amd.so and in libs2amd_fast.so alike. */
typedef struct s2amdRay /* 24 bytes */
{
	float p1[2], p2[2];
	float maxFraction;
	uint32_t maskBits;
} s2amdRay;
typedef struct s2amdRayHit /* 32 bytes */
{
	int32_t shape, body;
	float fraction;
	float point[2];
	float normal[2];
	int32_t pad;
} s2amdRayHit;
typedef struct s2amdPointProbe /* 12 bytes */
{
	float p[2];
	uint32_t maskBits;
} s2amdPointProbe;
typedef struct s2amdBoxQuery /* 20 bytes */
{
	float box[4]; /* {lower.x, lower.y, upper.x, upper.y} */
	uint32_t maskBits;
} s2amdBoxQuery;
int s2amd_world_ray_cast(s2amdSolver* solver, const s2amdRay* rays, int32_t count, s2amdRayHit* hits /* [count] */);
int s2amd_world_point_probe(s2amdSolver* solver, const s2amdPointProbe* probes, int32_t count, int32_t* offsets /* [count + 1] */, int32_t* shapes,
							int32_t capacity, int32_t* total);
int s2amd_world_query_boxes(s2amdSolver* solver, const s2amdBoxQuery* boxes, int32_t count, int32_t* offsets /* [count + 1] */, int32_t* shapes,
							int32_t capacity, int32_t* total);

/* (additive, API 5) Proximity queries: "what is near this shape, and how near?" asked of the resident world -- a blast radius, a
 * spawn-clearance test, a trigger volume that is not a box, a proximity sensor, picking with a tolerance.  The reference answers it with
 * s2ShapeDistance (include/solver2d/distance.h:71, src/distance.c:485-636) over the proxies of s2Shape_MakeDistanceProxy
 * (src/shape.c:75-93); the two batched calls below answer from the resident arrays, under the general terms of the scene queries above:
 * the world as it stands, enqueued behind whatever changed it last on the solver's stream, any number of times between steps, nothing
 * resident written, no host wait added to a step, no device trees needed, S2AMD_E_STATE without a resident world, count == 0 succeeds
 * and touches nothing.  LIVE, xf(body) and PASSES are the scene queries' definitions.
 *   Validation    on the host, for every query before anything is enqueued: 1 <= count <= 8; vertices[0 .. count), radius, position, rot
 *                 and maxDistance finite; radius >= 0; maxDistance >= 0.  One failing query makes the whole call return S2AMD_E_INVALID
 *                 with every output untouched.  rot is not checked for normalisation.
 *   Query box     w_i = s2TransformPoint({position, rot}, vertices[i]) for i < count; lower = w_0 folded with s2Min over w_1, w_2, ... in
 *                 index order (lower = s2Min(lower, w_i)), upper likewise with s2Max; r = radius + maxDistance (one fp32 add); the box is
 *                 {lower.x - r, lower.y - r, upper.x + r, upper.y + r}.
 *   Candidates    live, passing, s2AABB_Overlaps(fatAABB, box).  No other pruning decides a result.
 *   D(q, s)       s2ShapeDistance with a cache of count == 0, proxyA = s2MakeProxy(q.vertices, q.count, q.radius), proxyB =
 *                 s2Shape_MakeDistanceProxy(s) -- capsule: 2 points + radius; circle: 1 point + radius; polygon: count vertices (clamped
 *                 to 8) + radius; segment: 2 points, radius 0 --, transformA = {q.position, q.rot}, transformB = xf(s.body), useRadii =
 *                 true, the distance < FLT_EPSILON branch of src/distance.c:612-619 included.  D is a whole s2DistanceOutput.
 *   In range      a candidate s with D.distance <= q.maxDistance, compared as floats.  maxDistance 0 asks what overlaps or touches.
 *   s2amd_world_shapes_in_range  the in-range shapes of every query, ascending by slot, in the CSR form and with the S2AMD_E_CAPACITY
 *                 protocol of s2amd_world_point_probe (offsets and *total filled, shapes and distances untouched, the caller asks
 *                 again).  Where distances != NULL, distances[k] holds the bits of D.distance for shapes[k].
 *   s2amd_world_closest_shape    the in-range shape of least distance, ties to the lowest slot (distances are >= +0, so their bits order
 *                 as their values).  The record holds that shape's own D -- distance, pointA (on the query), pointB (on the shape),
 *                 iterations -- and its body.  Nothing in range: shape = body = -1, distance = maxDistance, points +0, iterations 0.
 * The composition is ours (the reference has no world-level distance query); every D is the reference's bit for bit.  All arithmetic is
 * fp32 in the reference's operation order without contraction, with correctly rounded divide and square root, in libs2amd.so and in
 * libs2amd_fast.so alike.  Not offered: sharded worlds, a simplex cache kept between calls, queries or answers in device memory. */
typedef struct s2amdProximityQuery /* 96 bytes */
{
	float vertices[8][2]; /* the query's proxy in its own frame: s2MakeProxy(vertices, count, radius) */
	int32_t count;		  /* 1..8: 1 = circle / point, 2 = capsule / segment, 3.. = (rounded) polygon */
	float radius;		  /* >= 0 */
	float position[2];	  /* transformA.p */
	float rot[2];		  /* transformA.q {s, c} */
	float maxDistance;	  /* >= 0, finite: 0 asks "what overlaps or touches" */
	uint32_t maskBits;
} s2amdProximityQuery;
typedef struct s2amdProximityHit /* 32 bytes */
{
	int32_t shape, body;
	float distance;
	float pointA[2];	/* on the query */
	float pointB[2];	/* on the shape */
	int32_t iterations; /* s2DistanceOutput.iterations */
} s2amdProximityHit;
int s2amd_world_closest_shape(s2amdSolver* solver, const s2amdProximityQuery* queries, int32_t count, s2amdProximityHit* hits /* [count] */);
int s2amd_world_shapes_in_range(s2amdSolver* solver, const s2amdProximityQuery* queries, int32_t count, int32_t* offsets /* [count + 1] */,
								int32_t* shapes, float* distances /* [capacity], may be NULL */, int32_t capacity, int32_t* total);

/* (additive, API 5) Sensor report: "which shapes are inside this region now, which came in during this step, which went out?" --
 * a pressure plate, a goal line, a kill zone, a pick-up radius carried by a body.  A list of up to S2AMD_MAX_SENSORS regions, each a
 * proxy shape fixed in the world or attached to a body, is evaluated on the resident arrays behind stage 4 of every s2amd_world_step (a
 * step the library repeats internally reports once), after the other five reports; the report owns its "before" state on the device.
 * It generalises the shape report's one view box with its entered / left lists.  With no flag set a step enqueues nothing for it; the
 * step gains no host wait, the getters wait.  LIVE, xf(body) and PASSES are the scene queries' definitions; every answer is an
 * order-free statement:
 *   Validation    on the host, in s2amd_world_set_sensors, before anything is changed: 0 <= count <= S2AMD_MAX_SENSORS; per sensor
 *                 1 <= count <= 8; vertices[0 .. count), radius, position, rot and margin finite; radius >= 0; margin >= 0; no flag
 *                 bits beyond the two below; body < bodyCapacity of the resident world (with no world resident, body is not bounded).
 *                 One bad record refuses the whole list with S2AMD_E_INVALID, and the old list stands.  rot is not checked for
 *                 normalisation.  The list holds across uploads; a sensor whose body is outside the new world's bodyCapacity is
 *                 inactive there.  While the report is on, sensors x shapeCapacity of the resident world must stay below 2^31 (the lists are
 *                 indexed by int32): s2amd_world_set_sensors refuses a list that exceeds it with S2AMD_E_INVALID (the old list
 *                 stands), and so does s2amd_world_upload for a world of more than 2^31 / sensors shape slots.  Should the device
 *                 block of the new list fail to be made, the error is returned and the old list stands as well.
 *   Active        not S2AMD_SENSOR_DISABLED, and body < 0 or (body < bodyCapacity and bodies[body].type != S2AMD_BODY_FREE).  An
 *                 inactive sensor holds nothing; its state has active = 0, transform and box +0, lowestShape = -1.
 *   Transform     body < 0: {position, rot}.  Otherwise s2MulTransforms(xf(body), {position, rot}) (include/solver2d/math.h:368-374,
 *                 s2MulRot :291-300): q.s = b.s * rot.c + b.c * rot.s, q.c = b.c * rot.c - b.s * rot.s, p = s2Add(s2RotateVector(b,
 *                 position), origins[body]) with b = bodies[body].rot.
 *   Box           the proximity queries' query box of {vertices, count, radius} under the transform with maxDistance = margin.
 *   Candidates    live; (categoryBits & maskBits) != 0; s2AABB_Overlaps(fatAABB, box); shape.body != sensor.body; with
 *                 S2AMD_SENSOR_SKIP_STATIC, bodies[shape.body].type != S2AMD_BODY_STATIC.  No other pruning decides a result.
 *   Inside        a candidate with D.distance <= margin, D the proximity queries' D(q, s) with transformA = the transform above:
 *                 empty cache, useRadii, the FLT_EPSILON branch included.
 *   "Before"      the same rule evaluated at s2amd_world_upload, when the report is turned on (or its listCapacity changes), and
 *                 whenever s2amd_world_set_sensors succeeds on a resident world: the caller's own acts raise no events, as with the shape
 *                 view.  Each of these voids the last step's report: the getters answer S2AMD_E_STATE until the next step.
 *   INSIDE        s2amd_world_sensor_inside: a CSR list over all sensors in list order, shape slots ascending; inactive sensors have
 *                 empty ranges; the S2AMD_E_CAPACITY protocol of s2amd_world_point_probe (offsets and *total filled, shapes untouched).
 *   EVENTS        s2amd_world_sensor_events: `entered` holds the (sensor, shape) pairs inside now and not before, `left` the reverse,
 *                 both ascending by (sensor, shape); body = the shape's body as the resident array holds it, sensorBody = the sensor's.
 *                 A sensor that turned inactive leaves everything it held; one that turned active enters everything it holds.  With a
 *                 capacity too small both counts are filled and both lists untouched (S2AMD_E_CAPACITY).
 *   STATES        s2amd_world_sensor_states: one record per sensor in list order (S2AMD_E_CAPACITY with *count filled when capacity is
 *                 less); lowestShape = the lowest inside slot or -1; the inside / entered / left counts are filled whatever other flags
 *                 are set.
 *   Errors        those of the other reports: S2AMD_E_STATE without a resident world, when the getter's flag was not set before the
 *                 last step, or when no step has run since; unknown flag bits and listCapacity < 0 give S2AMD_E_INVALID.
 *   listCapacity  sizes the three device lists a step writes (entries per list).  A cost knob that never changes an answer: when a
 *                 step's total exceeds it, the getter rebuilds that list from the kept masks into scratch of the needed size -- one more
 *                 launch and one more wait.  listCapacity 0 gives the same bytes as an ample value.  A call that changes listCapacity,
 *                 whatever its flags, voids the last step's report (its lists were laid out under the old value).
 *   Memory        the masks cost sensors x ceil(shapeCapacity / 256) x 32 bytes per set, and there are four sets (now, before, entered,
 *                 left); beside them 128 + 64 + 112 bytes per sensor, 12 bytes per sensor and tile of prefix sums, and 36 bytes per list
 *                 entry of listCapacity.  s2amd_world_set_sensors on a resident world with the report on waits for the stream once (the
 *                 list is copied to the device before the call returns).
 * The reference has no sensors: the composition is ours; every distance is the reference's s2ShapeDistance bit for bit.  All arithmetic
 * is fp32 in the reference's operation order without contraction, in libs2amd.so and in libs2amd_fast.so alike.  Not offered:
 * body-level events, sensors in device memory, sharded worlds. */
#define S2AMD_MAX_SENSORS 1024
#define S2AMD_SENSOR_DISABLED 1	   /* holds nothing, raises no events */
#define S2AMD_SENSOR_SKIP_STATIC 2 /* shapes on static bodies are not candidates */
typedef struct s2amdSensor /* 112 bytes */
{
	float vertices[8][2]; /* the sensor's proxy in its own frame: s2MakeProxy(vertices, count, radius) */
	int32_t count;		  /* 1..8 */
	float radius;		  /* >= 0 */
	float position[2];	  /* the frame: in the world (body < 0) or relative to the body */
	float rot[2];		  /* {s, c} */
	float margin;		  /* inside when D.distance <= margin; >= 0, finite */
	uint32_t maskBits;
	int32_t body;  /* < 0: fixed in the world */
	int32_t flags; /* S2AMD_SENSOR_* */
	int32_t pad[2];
} s2amdSensor;
int s2amd_world_set_sensors(s2amdSolver* solver, const s2amdSensor* sensors, int32_t count); /* replaces the whole list; count 0 clears */
#define S2AMD_SENSOR_REPORT_INSIDE 1
#define S2AMD_SENSOR_REPORT_EVENTS 2
#define S2AMD_SENSOR_REPORT_STATES 4
int s2amd_world_set_sensor_report(s2amdSolver* solver, int32_t flags, int32_t listCapacity);
typedef struct s2amdSensorEvent /* 16 bytes */
{
	int32_t sensor, shape, body, sensorBody;
} s2amdSensorEvent;
typedef struct s2amdSensorState /* 64 bytes */
{
	int32_t sensor, body, active, inside, entered, left, lowestShape, pad;
	float position[2], rot[2]; /* the world transform used */
	float box[4];			   /* the candidate box used */
} s2amdSensorState;
int s2amd_world_sensor_inside(s2amdSolver* solver, int32_t* offsets /* [sensorCount + 1] */, int32_t* shapes, int32_t capacity, int32_t* total);
int s2amd_world_sensor_events(s2amdSolver* solver, s2amdSensorEvent* entered, int32_t enteredCapacity, int32_t* enteredCount, s2amdSensorEvent* left,
							  int32_t leftCapacity, int32_t* leftCount);
int s2amd_world_sensor_states(s2amdSolver* solver, s2amdSensorState* out, int32_t capacity, int32_t* count);

/* (additive, API 5) Ray sensors: "what does this ray see now, and did that change during the step?" -- a range finder or a lidar fan on
 * a robot, a suspension ray under a wheel, a ground probe under a character, a line of sight between two bodies.  A list of up to
 * S2AMD_MAX_RAY_SENSORS rays, each fixed in the world or mounted on a body, is cast on the resident arrays behind stage 4 of every
 * s2amd_world_step (a step the library repeats internally reports once), after the other six reports; the report owns its "before"
 * state on the device.  It replaces, per step, a pose read-back (s2amd_world_download_step), the host's own s2TransformPoint on both
 * ends and a s2amd_world_ray_cast call.  With no flag set a step enqueues nothing for the rays; the step gains no host wait, the
 * getters wait.  LIVE, xf(body) and PASSES are the scene queries' definitions; every answer is an order-free statement:
 *   Validation    on the host, in s2amd_world_set_ray_sensors, before anything is changed: 0 <= count <= S2AMD_MAX_RAY_SENSORS; per ray
 *                 s2IsValidRay (src/geometry.c:15-20) on the local {p1, p2, maxFraction}; no flag bits beyond the two below; body <
 *                 bodyCapacity of the resident world (with no world resident, body is not bounded).  One bad record refuses the whole
 *                 list with S2AMD_E_INVALID, and the old list stands.  The list holds across uploads; a ray whose body is outside the new
 *                 world's bodyCapacity is inactive there.
 *   World ray     body < 0: the ends as given.  Otherwise P = s2TransformPoint(xf(body), p) (include/solver2d/math.h:350-356) on both
 *                 ends.  maxFraction is unchanged.
 *   Active        not S2AMD_RAY_SENSOR_DISABLED; body < 0 or (body < bodyCapacity and bodies[body].type != S2AMD_BODY_FREE); and the
 *                 world ray satisfies s2IsValidRay -- a body with a non-finite pose switches its rays off, it does not poison the answers.
 *   Answer        s2amd_world_ray_cast's statement for {P1, P2, maxFraction, maskBits} -- the same segment box, "no other pruning
 *                 decides a result", the least fraction as float values with ties to the lowest slot, point from the world-space ends,
 *                 normal = s2RotateVector(rot, output.normal) -- with two further exclusions from the candidates: for a mounted ray
 *                 (body >= 0) the shapes with shape.body == ray.body, so that it never hits its own body; with
 *                 S2AMD_RAY_SENSOR_SKIP_STATIC the shapes with bodies[shape.body].type == S2AMD_BODY_STATIC.
 *   STATES        s2amd_world_ray_states: one record per ray in list order.  A miss has shape = hitBody = -1, fraction = maxFraction,
 *                 point and normal +0.  An inactive ray has the same, plus active = 0 and p1, p2 +0.  body is the ray's own.
 *                 shapeBefore is filled whatever other flags are set.
 *   RANGES        s2amd_world_ray_ranges: one float per ray in list order, the state's fraction -- the observation vector.
 *                 s2amd_world_export_ray_ranges copies the same bytes into a caller's device buffer (s2amd_device_alloc or any
 *                 allocation of the solver's device) behind the step on the solver's stream, device to device, and returns when the
 *                 copy is done, as s2amd_export_poses; capacity counts floats.
 *   EVENTS        s2amd_world_ray_events: the rays with shapeNow != shapeBefore, ascending by ray; bodyNow = the hit shape's body or
 *                 -1.  Hit to miss, miss to hit and shape to shape are all events.  A ray that turned inactive counts as a miss.
 *   "Before"      the same rule evaluated at s2amd_world_upload, when the report is turned on, and whenever
 *                 s2amd_world_set_ray_sensors succeeds on a resident world: the caller's own acts raise no events.  Each of these voids
 *                 the last step's report, as with the sensors: the getters answer S2AMD_E_STATE until the next step.
 *   Errors        those of the other reports: S2AMD_E_STATE without a resident world, when the getter's flag was not set before the
 *                 last step, or when no step has run since; S2AMD_E_CAPACITY with *count filled and nothing consumed; unknown flag bits
 *                 give S2AMD_E_INVALID.
 *   Memory        196 bytes per ray (the list 48, the posed ray 48, the key 8, the state 64, the range 4, "before" and "now" 8, one
 *                 event 16), 32 bytes per group of 64 rays (its box) and per 256 rays (their ballots), each piece rounded up to 256
 *                 bytes: 3.1 MiB for 16,384 rays.  s2amd_world_set_ray_sensors on a resident world with the report on waits for the
 *                 stream once (the list is copied to the device before the call returns).
 * The reference has no ray sensors: the composition is ours; every cast is the reference's s2RayCast<type> bit for bit.  All arithmetic is
 * fp32 in the reference's operation order without contraction, in libs2amd.so and in libs2amd_fast.so alike.  Not offered: all-hits
 * or sorted results, rays in device memory, sharded worlds, forces applied along a ray. */
#define S2AMD_MAX_RAY_SENSORS 16384
#define S2AMD_RAY_SENSOR_DISABLED 1	   /* sees nothing, raises no events */
#define S2AMD_RAY_SENSOR_SKIP_STATIC 2 /* shapes on static bodies are not candidates */
typedef struct s2amdRaySensor /* 48 bytes */
{
	float p1[2], p2[2]; /* in the world (body < 0) or in the body's frame */
	float maxFraction;
	uint32_t maskBits;
	int32_t body;  /* < 0: fixed in the world */
	int32_t flags; /* S2AMD_RAY_SENSOR_* */
	int32_t pad[4];
} s2amdRaySensor;
int s2amd_world_set_ray_sensors(s2amdSolver* solver, const s2amdRaySensor* rays, int32_t count); /* replaces the whole list; count 0 clears */
#define S2AMD_RAY_REPORT_STATES 1
#define S2AMD_RAY_REPORT_RANGES 2
#define S2AMD_RAY_REPORT_EVENTS 4
int s2amd_world_set_ray_report(s2amdSolver* solver, int32_t flags);
typedef struct s2amdRayState /* 64 bytes */
{
	int32_t ray, body, active, shape, hitBody, shapeBefore;
	float fraction;
	float p1[2], p2[2]; /* the world ray used */
	float point[2], normal[2];
	int32_t pad;
} s2amdRayState;
typedef struct s2amdRayEvent /* 16 bytes */
{
	int32_t ray, shapeBefore, shapeNow, bodyNow;
} s2amdRayEvent;
int s2amd_world_ray_states(s2amdSolver* solver, s2amdRayState* out, int32_t capacity, int32_t* count);
int s2amd_world_ray_ranges(s2amdSolver* solver, float* out, int32_t capacity, int32_t* count);
int s2amd_world_export_ray_ranges(s2amdSolver* solver, void* deviceRanges, int32_t capacity); /* device-to-device, as s2amd_export_poses */
int s2amd_world_ray_events(s2amdSolver* solver, s2amdRayEvent* out, int32_t capacity, int32_t* count);

/* (additive, API 5) Occupancy grids: "what does the world look like around here, as an image?" -- an egocentric occupancy map around a
 * vehicle, a local cost map under a character, a coarse minimap for a culling or AI pass.  A list of up to S2AMD_MAX_GRID_SENSORS
 * grids, each fixed in the world or mounted on a body, is rasterised on the resident arrays behind stage 4 of every s2amd_world_step (a
 * step the library repeats internally reports once), after the other seven reports.  It replaces, per step, a pose read-back
 * (s2amd_world_download_step), width x height cell centres computed on the host, one s2amd_world_point_probe call and a fold of its CSR
 * list into an image.  With no flag set a step enqueues nothing for the grids; the step gains no host wait, the getters wait; nothing
 * resident is written.  LIVE, xf(body) and PASSES are the scene queries' definitions; every answer is an order-free statement:
 *   Validation    on the host, in s2amd_world_set_grid_sensors, before anything is changed: 0 <= count <= S2AMD_MAX_GRID_SENSORS; per
 *                 grid 1 <= width, height <= S2AMD_MAX_GRID_SIDE; position, rot and cellSize finite, cellSize > 0; no flag bits beyond
 *                 the two below; body < bodyCapacity of the resident world (with no world resident, body is not bounded); and over the
 *                 list sum(width * height) <= S2AMD_MAX_GRID_CELLS.  One bad record refuses the whole list with S2AMD_E_INVALID, and
 *                 the old list stands.  rot is not checked for normalisation.  The list holds across uploads; a grid whose body is
 *                 outside the new world's bodyCapacity is inactive there.
 *   Cell order    firstCell[g] is the exclusive prefix sum of width * height in list order; cell (i, j) of grid g, i along the
 *                 frame's x and j along its y, is at firstCell[g] + j * width + i.  Every per-cell array has exactly
 *                 sum(width * height) entries, those of inactive grids included.
 *   Frame         body < 0: G = {position, rot}.  Otherwise G = s2MulTransforms(xf(body), {position, rot})
 *                 (include/solver2d/math.h:368-374), in the operation order the sensor report's paragraph spells out.
 *   Cell point    l.x = (((float)i + 0.5f) - 0.5f * (float)width) * cellSize, l.y the same with j and height (everything in front of
 *                 the one multiply is exact for these integers: the grid is centred on its frame); P = s2TransformPoint(G, l)
 *                 (math.h:350-356).
 *   Active        not S2AMD_GRID_SENSOR_DISABLED; body < 0 or (body < bodyCapacity and bodies[body].type != S2AMD_BODY_FREE); and the P
 *                 of the four corner cells are finite -- a body with a non-finite pose switches its grids off.
 *   Box           the componentwise min and max of the four corner cells' P.  It contains every cell's P: each coordinate of P is a
 *                 composition of correctly rounded operations, each weakly monotone in i and in j, so its extremes over the grid lie at
 *                 corners.  This is why the grid-level cull below decides no result.
 *   Candidates    of a grid: the LIVE shapes with (categoryBits & maskBits) != 0 and s2AABB_Overlaps(fatAABB, box); for a mounted grid
 *                 (body >= 0) not those with shape.body == grid.body, so that a grid never sees its own body; with
 *                 S2AMD_GRID_SENSOR_SKIP_STATIC not those with bodies[shape.body].type == S2AMD_BODY_STATIC.
 *   Hit           of a cell: a candidate with s2AABB_Overlaps(fatAABB, {P, P}) that passes s2PointInCircle / Capsule / Polygon
 *                 (s2InvTransformPoint(xf(shape.body), P), geometry) -- s2amd_world_point_probe's statement for {P, maskBits} minus the
 *                 two exclusions.  Segments never hit.
 *   CATEGORIES    s2amd_world_grid_categories: per cell the OR of categoryBits over the cell's hits.
 *   SHAPES        s2amd_world_grid_shapes: per cell the lowest hit slot, or -1.
 *   OCCUPANCY     s2amd_world_grid_occupancy: per cell 1.0f if there is a hit, else +0.0f -- the observation image.
 *                 s2amd_world_export_grid_occupancy copies the same bytes into a caller's device buffer (s2amd_device_alloc or any
 *                 allocation of the solver's device) behind the step on the solver's stream, device to device, and returns when the
 *                 copy is done, as s2amd_world_export_ray_ranges; capacity counts floats.  Cells of an inactive grid read 0, -1, +0.
 *   STATES        s2amd_world_grid_states: one record per grid in list order.  occupied is the number of cells with a hit,
 *                 lowestShape the least SHAPES value >= 0 over the grid or -1, candidates the number of the grid's candidates; the
 *                 three are filled whatever other flags are set.  An inactive grid has active = 0, frame and box +0, occupied =
 *                 candidates = 0, lowestShape = -1; it keeps firstCell and cells.
 *   Lifetime      the report keeps nothing from step to step: there is no "before" and there are no events.  s2amd_world_upload,
 *                 turning the report on, and a s2amd_world_set_grid_sensors that succeeds on a resident world each void the last
 *                 step's report: the getters answer S2AMD_E_STATE until the next step.
 *   Errors        those of the other reports: S2AMD_E_STATE without a resident world, when the getter's flag was not set before the
 *                 last step, or when no step has run since; S2AMD_E_CAPACITY with *count filled and nothing written; unknown flag bits
 *                 give S2AMD_E_INVALID.
 *   Memory        192 bytes per grid (the list 64, the posed grid 64, the state 64) plus 8 bytes per grid and 64 shape slots (the
 *                 candidate mask, shape slots rounded up to 256), 12 bytes per cell (the three arrays) and 16 bytes per tile of 64
 *                 cells, each piece rounded up to 256 bytes: 14.9 MiB for 1,048,576 cells in 1,024 grids over 20,101 shape slots.
 *                 s2amd_world_set_grid_sensors on a resident world with the report on waits for the stream once (the list is copied
 *                 to the device before the call returns).
 * The reference has no occupancy grids: the composition is ours; every cell test is the reference's s2PointIn<type> bit for bit.  All
 * arithmetic is fp32 in the reference's operation order without contraction, in libs2amd.so and in libs2amd_fast.so alike.  Not
 * offered: events, distances per cell, grids or cell arrays in device memory other than the occupancy export, sharded worlds, a
 * one-shot call (s2amd_world_point_probe is the one-shot). */
#define S2AMD_MAX_GRID_SENSORS 1024
#define S2AMD_MAX_GRID_SIDE 256		 /* width and height, each 1..256 */
#define S2AMD_MAX_GRID_CELLS 1048576 /* over the whole list */
#define S2AMD_GRID_SENSOR_DISABLED 1	/* every cell reads empty */
#define S2AMD_GRID_SENSOR_SKIP_STATIC 2 /* shapes on static bodies are not candidates */
typedef struct s2amdGridSensor /* 64 bytes */
{
	float position[2], rot[2]; /* the grid's frame ({s, c}), in the world (body < 0) or relative to the body; the grid is centred on it */
	float cellSize;			   /* > 0, finite */
	int32_t width, height;	   /* cells along the frame's x and y */
	uint32_t maskBits;
	int32_t body;  /* < 0: fixed in the world */
	int32_t flags; /* S2AMD_GRID_SENSOR_* */
	int32_t pad[6];
} s2amdGridSensor;
int s2amd_world_set_grid_sensors(s2amdSolver* solver, const s2amdGridSensor* grids, int32_t count); /* replaces the whole list; count 0 clears */
#define S2AMD_GRID_REPORT_CATEGORIES 1
#define S2AMD_GRID_REPORT_SHAPES 2
#define S2AMD_GRID_REPORT_OCCUPANCY 4
#define S2AMD_GRID_REPORT_STATES 8
int s2amd_world_set_grid_report(s2amdSolver* solver, int32_t flags);
typedef struct s2amdGridState /* 64 bytes */
{
	int32_t grid, body, active, firstCell, cells, occupied, lowestShape, candidates;
	float position[2], rot[2]; /* the world frame used */
	float box[4];			   /* the candidate box used */
} s2amdGridState;
int s2amd_world_grid_categories(s2amdSolver* solver, uint32_t* out, int32_t capacity, int32_t* count); /* one word per cell */
int s2amd_world_grid_shapes(s2amdSolver* solver, int32_t* out, int32_t capacity, int32_t* count);
int s2amd_world_grid_occupancy(s2amdSolver* solver, float* out, int32_t capacity, int32_t* count);
int s2amd_world_export_grid_occupancy(s2amdSolver* solver, void* deviceCells, int32_t capacity); /* device-to-device, as s2amd_world_export_ray_ranges */
int s2amd_world_grid_states(s2amdSolver* solver, s2amdGridState* out, int32_t capacity, int32_t* count);

/* (additive, API 5) Contact queries: "if this shape stood here, what would it touch, where, and how deep?" asked of the resident world
 * -- a character controller, a ghost or trigger shape, spawn placement with push-out, a "will this fit" test.  The reference answers it
 * with its nine manifold functions s2Collide* (include/solver2d/manifold.h:56-85), dispatched by s_registers (src/contact.c:139-151);
 * the two batched calls below answer from the resident arrays, under the general terms of the scene queries above: the world as it
 * stands, enqueued behind whatever changed it last on the solver's stream, any number of times between steps, nothing resident written,
 * no host wait added to a step, no device trees needed, S2AMD_E_STATE without a resident world, count == 0 succeeds and touches nothing.
 * LIVE, xf(body) and PASSES are the scene queries' definitions.
 *   Validation    on the host, for every query before anything is enqueued: type is one of the four; a polygon has 3 <= count <= 8; the
 *                 vertices the type reads (circle 1, capsule and segment 2, polygon count) are finite, and for a polygon so are
 *                 normals[0 .. count); position and rot are finite; radius is finite and >= 0 where the type reads it (not for a
 *                 segment).  One failing query makes the whole call return S2AMD_E_INVALID with every output untouched.  rot is not
 *                 checked for normalisation, the normals not for length.
 *   Query box     what stage 4 would store in shape->aabb for this shape at the transform {position, rot}: s2Shape_ComputeAABB
 *                 (src/geometry.c:288-339) per type, grown by s2_speculativeDistance on every side (src/world.c:286-290).
 *   Candidates    live, passing, s2AABB_Overlaps(fatAABB, query box), and a type pair that has a manifold function: segment against
 *                 segment has none.  No other pruning decides a result.  (A slot whose type is none of the four, or a polygon slot
 *                 with count > 8 -- no s2Polygon holds one -- is never a candidate.)
 *   Order         the manifold's shape A is the query when s_registers[q.type][s.type].primary is true: for equal types and when the
 *                 query's type is the pair's first at src/contact.c:143-151 (capsule-circle, polygon-circle, polygon-capsule,
 *                 segment-circle, segment-capsule, segment-polygon).  Otherwise shape A is the world shape, as s2CreateContact flips it,
 *                 and queryIsB = 1.  The query's transform is {position, rot}, the world shape's xf(body).
 *   M(q, s)       the pair's s2Collide* with a distance cache of count == 0 where the function takes one: what a contact created this
 *                 step gets from its first s2UpdateContact.  Capsules and segments go through s2MakeCapsule as src/manifold.c sends
 *                 them; a segment's radius is 0.
 *   Hit           a candidate with M.pointCount > 0.  Speculative points (separation > 0) are included as in the reference: the caller
 *                 reads `separation`.  The record is M: normal (from A to B, world space), per point localAnchorA (the contact point in
 *                 A's frame), localAnchorB (the same point in B's frame), separation and id, as the s2Collide* function leaves them.
 *   s2amd_world_collide_shape    the hits of every query, ascending by slot, in the CSR form and with the S2AMD_E_CAPACITY protocol of
 *                 s2amd_world_point_probe: with capacity < *total, offsets and *total are filled, hits is untouched, the caller asks
 *                 again.
 *   s2amd_world_deepest_contact  per query the hit whose least point separation (over its pointCount points) is smallest, compared as
 *                 float values (-0 equals +0), ties to the lowest slot; the record is that hit's own.  No hit: shape = body = -1 and
 *                 every other field zero.
 * The composition is ours (the reference has no world-level manifold query); every M is the reference's bit for bit.  All arithmetic is
 * fp32 in the reference's operation order without contraction, with correctly rounded divide and square root, in libs2amd.so and in
 * libs2amd_fast.so alike.  Not offered: sharded worlds, a simplex cache kept between calls, queries or answers in device
 * memory, the drop-in's contacts routed through these calls, the device trees as an accelerator. */
typedef struct s2amdContactQuery /* 160 bytes */
{
	float vertices[8][2]; /* geometry as s2amdShape holds it: circle = vertices[0]; capsule / segment = vertices[0..1]; polygon = [0..count) */
	float normals[8][2];  /* polygon edge normals as the caller's s2Polygon has them; not recomputed, not checked for length */
	int32_t type;		  /* S2AMD_SHAPE_CAPSULE / _CIRCLE / _POLYGON / _SEGMENT */
	int32_t count;		  /* polygon: 3..8; ignored otherwise */
	float radius;		  /* circle, capsule, rounded polygon; ignored for a segment */
	float position[2];	  /* the query's transform: p (the "body origin" its anchors are relative to) */
	float rot[2];		  /* q {s, c}; not checked for normalisation */
	uint32_t maskBits;
} s2amdContactQuery;
typedef struct s2amdContactHit /* 80 bytes */
{
	int32_t shape, body; /* the world shape and its body */
	int32_t pointCount;	 /* 1 or 2 in a hit */
	int32_t queryIsB;	 /* 0: the manifold's shape A is the query; 1: shape A is the world shape (see "Order") */
	float normal[2];	 /* s2Manifold.normal: from A to B */
	struct
	{
		float localAnchorA[2], localAnchorB[2];
		float separation;
		uint32_t id;
	} points[2];		 /* a point >= pointCount is all zero bits */
	int32_t pad[2];		 /* 0 */
} s2amdContactHit;
int s2amd_world_collide_shape(s2amdSolver* solver, const s2amdContactQuery* queries, int32_t count, int32_t* offsets /* [count + 1] */,
							  s2amdContactHit* hits, int32_t capacity, int32_t* total);
int s2amd_world_deepest_contact(s2amdSolver* solver, const s2amdContactQuery* queries, int32_t count, s2amdContactHit* hits /* [count] */);

/* (additive, API 5) Shape casts: "this shape moves from here along this vector: what does it hit first, where, and at which fraction of
 * the way?" asked of the resident world -- a bullet, a character controller's move-and-slide, a thick ray, a swept placement test, a
 * swept sensor.  The reference has no continuous collision at all (a fast body tunnels); the composition below is ours: conservative
 * advancement in which every distance is the reference's own s2ShapeDistance (src/distance.c:485-636), bit for bit.  The two batched
 * calls answer from the resident arrays, under the general terms of the scene queries above: the world as it stands, enqueued behind
 * whatever changed it last on the solver's stream, any number of times between steps, nothing resident written, no host wait added to a
 * step, no device trees needed, S2AMD_E_STATE without a resident world, count == 0 succeeds and touches nothing.  LIVE, xf(body) and
 * PASSES are the scene queries' definitions.
 *   Validation    on the host, for every cast before anything is enqueued: 1 <= count <= 8; vertices[0 .. count), radius, position, rot,
 *                 translation and maxFraction finite; radius >= 0; maxFraction >= 0.  One failing cast makes the whole call return
 *                 S2AMD_E_INVALID with every output untouched.  rot is not checked for normalisation.
 *   Constants     all fp32: target = s2_linearSlop (0.005f); tolerance = 0.25f * s2_linearSlop; threshold = target + tolerance (one
 *                 add); CAP = 20.
 *   Swept box     e = s2MulAdd(position, maxFraction, translation).  lower0 / upper0: the bounds of s2TransformPoint({position, rot},
 *                 vertices[i]) for i < count, folded from vertex 0 in index order with s2Min / s2Max as the proximity queries' box is;
 *                 lower1 / upper1: the same fold at {e, rot}.  lower = s2Min(lower0, lower1), upper = s2Max(upper0, upper1);
 *                 r = radius + s2_speculativeDistance (one add; 0.02 >= threshold, so no shape within reach of the path is pruned);
 *                 the box is {lower.x - r, lower.y - r, upper.x + r, upper.y + r}.
 *   Candidates    live, passing, s2AABB_Overlaps(fatAABB, box).  No other pruning decides a result.
 *   C(q, s)       the proxies and xfB = xf(s.body) are those of the proximity queries' D(q, s); the cache is empty, useRadii = true.
 *                 t_0 = +0.  For k = 0, 1, ...:
 *                   1. D_k = s2ShapeDistance with transformA = {s2MulAdd(position, t_k, translation), rot}.
 *                   2. D_k.distance < threshold: HIT at t_k.
 *                   3. Otherwise, k == CAP: HIT at t_k -- the sweep stops short and never passes through; the record's
 *                      distance >= threshold says so.
 *                   4. n = s2Normalize(s2Sub(D_k.pointB, D_k.pointA)), approach = s2Dot(translation, n).  approach <= 0: MISS (moving
 *                      away or along; a zero translation ends here).
 *                   5. t_{k+1} = t_k + (D_k.distance - target) / approach.  !(t_{k+1} <= maxFraction): MISS.
 *                 The hit record is {s, s.body, t_k, D_k.distance, D_k.pointB, s2Normalize(s2Sub(D_k.pointA, D_k.pointB)), k}.
 *   s2amd_world_cast_shape_all   the hits of every cast, ascending by slot, in the CSR form and with the S2AMD_E_CAPACITY protocol of
 *                 s2amd_world_point_probe: with capacity < *total, offsets and *total are filled, hits is untouched, the caller asks
 *                 again.
 *   s2amd_world_cast_shape       per cast the hit of least fraction, ties to the lowest slot (fractions are >= +0, so their bits order
 *                 as their values); the record is that hit's own.  No hit: shape = body = -1, fraction = maxFraction and every other
 *                 field zero.
 * All arithmetic is fp32 in the reference's operation order without contraction, with correctly rounded divide and square root, in
 * libs2amd.so and in libs2amd_fast.so alike.  Not offered: rotation during the sweep, sharded worlds, casts or answers in device
 * memory, the device trees as an accelerator. */
typedef struct s2amdShapeCast /* 112 bytes */
{
	float vertices[8][2]; /* the moving proxy in its own frame: s2MakeProxy(vertices, count, radius) */
	int32_t count;		  /* 1..8 */
	float radius;		  /* >= 0 */
	float position[2];	  /* transform at fraction 0: p */
	float rot[2];		  /* q {s, c}; the cast does not rotate; not checked for normalisation */
	float translation[2]; /* the sweep: at fraction t the proxy stands at position + t * translation */
	float maxFraction;	  /* >= 0, finite */
	uint32_t maskBits;
	int32_t pad[2];		  /* ignored */
} s2amdShapeCast;
typedef struct s2amdShapeCastHit /* 48 bytes */
{
	int32_t shape, body;
	float fraction;		/* t_k */
	float distance;		/* D_k.distance at that fraction */
	float point[2];		/* D_k.pointB: on the world shape */
	float normal[2];	/* from the world shape towards the moving one; zero when they overlap */
	int32_t iterations; /* k: the advances made; 0 = already within reach at the start */
	int32_t pad[3];		/* 0 */
} s2amdShapeCastHit;
int s2amd_world_cast_shape(s2amdSolver* solver, const s2amdShapeCast* casts, int32_t count, s2amdShapeCastHit* hits /* [count] */);
int s2amd_world_cast_shape_all(s2amdSolver* solver, const s2amdShapeCast* casts, int32_t count, int32_t* offsets /* [count + 1] */,
							   s2amdShapeCastHit* hits, int32_t capacity, int32_t* total);

/* (additive, API 5) Move-and-slide: "this character wants to go by this displacement: where does it end up, against what did it slide, and
 * what is left?" asked of the resident world for a batch of movers -- the loop a character controller builds on the shape casts above
 * (cast, stop a skin short, clip the rest of the displacement to the plane met, cast again), kept on the device: one call, one host
 * wait, however many bounces.  The reference has no mover; the composition is ours, as the shape casts' is: every distance is the
 * reference's s2ShapeDistance and every advancement loop is C(q, s) above, unchanged.  The general terms are the scene queries': the
 * world as it stands, enqueued behind whatever changed it last on the solver's stream, nothing resident written, no host wait added to a
 * step, no device trees needed, S2AMD_E_STATE without a resident world, count == 0 succeeds and touches nothing, count at most the
 * queries' batch limit (65535 * 256).  LIVE, PASSES, xf(body), the swept box, C(q, s), target, threshold and CAP are the shape casts'.
 *   Validation    on the host, for every mover before anything is enqueued: the shape casts' checks of the proxy (1 <= count <= 8,
 *                 vertices[0 .. count) finite), radius (finite, >= 0), position, rot and translation (finite);
 *                 1 <= maxIterations <= 8; no flag bit beyond S2AMD_MOVER_STATIC_ONLY; reserved == 0; ignoreBody < the world's body
 *                 slots (any negative value: none).  One failing mover makes the whole call return S2AMD_E_INVALID with every output
 *                 untouched.  rot is not checked for normalisation.
 *   GRAZE         1e-4f.  A displacement r GRAZES a normal N when s2Dot(r, N) >= -(GRAZE * s2Length(r)) -- one multiply and one negation,
 *                 s2Length as math.h:169-172.  The tolerance is part of the statement, not a tuning knob: with strict sign tests the
 *                 clipped displacement keeps a residue of one ulp against the normal of the next floor tile, and a box walking over
 *                 unit boxes laid edge to edge reports a false corner within a few metres.
 *   The loop      p = position, r = translation, no planes, advances = 0.  For b = 0 .. maxIterations - 1:
 *                   1. c = {the proxy, p, rot, translation = r, maxFraction = 1.0f, maskBits}.
 *                   2. The candidates are the cast's candidates for c, minus the shapes whose slot is in the plane list already, minus
 *                      the shapes with shape.body == ignoreBody, minus -- under S2AMD_MOVER_STATIC_ONLY -- the shapes whose
 *                      bodies[shape.body].type is not S2AMD_BODY_STATIC.
 *                   3. A candidate BLOCKS when C(c, s) is a HIT (t, D, k), except when k == 0, N = s2Normalize(s2Sub(D.pointA,
 *                      D.pointB)) is not the zero vector and r grazes N: the mover touches the shape where it stands and is leaving
 *                      it or sliding along.
 *                   4. The winner is the blocker of least t, ties to the lowest slot (the casts' 64-bit key).
 *                   5. No blocker: p = s2Add(p, r), r = 0, status REACHED, iterations = b + 1, end.
 *                   6. Otherwise p = s2MulAdd(p, t, r), rem = s2MulSV(1.0f - t, r), advances += k, and the plane {s, s.body, t,
 *                      D.distance, D.pointB, N} is appended.
 *                   7. N zero: r = rem, status OVERLAPPED, end.  The mover stands inside something: no normal says which way is out;
 *                      s2amd_world_deepest_contact does.
 *                   8. into = s2Dot(rem, N); into < 0: rem = s2MulSub(rem, into, N).
 *                   9. r = rem.  rem fails to graze the normal of an earlier plane: status CORNERED, end (in two dimensions two planes
 *                      that both bind leave no motion).
 *                  10. rem is the zero vector: status BLOCKED, end.
 *                 The loop running out: status OUT_OF_ITERATIONS.  Then iterations is the number of casts made, remaining = r,
 *                 planeCount the number of planes, and planes[i * 8 + j] for j >= planeCount is zero bytes.
 *   The skin      The shapes of recorded planes are no candidates any more.  That is sound: every shape is convex and r is kept within
 *                 their half-planes.  A mover comes closer to a recorded plane than where it stopped (target, 0.005) only by the
 *                 rounding of step 8, or by at most GRAZE times the distance travelled while it slides along one.  The next call
 *                 restores the skin wherever its displacement has a component into the plane: its first cast stops at target again.
 * All arithmetic is fp32 in the reference's operation order without contraction, with correctly rounded divide and square root, in
 * libs2amd.so and in libs2amd_fast.so alike.  Not offered: rotation of the mover, pushing dynamic bodies, step-up and step-down, movers
 * or answers in device memory, sharded worlds, the device trees as an accelerator. */
#define S2AMD_MOVER_MAX_ITERATIONS 8
#define S2AMD_MOVER_STATIC_ONLY 1		/* flags: only shapes on S2AMD_BODY_STATIC bodies are candidates */
#define S2AMD_MOVER_REACHED 0			/* the last cast met nothing: the whole remaining displacement was spent */
#define S2AMD_MOVER_BLOCKED 1			/* the clip left a zero displacement */
#define S2AMD_MOVER_CORNERED 2			/* the clipped displacement heads into an earlier plane */
#define S2AMD_MOVER_OVERLAPPED 3		/* the winner overlaps the mover where it stands: no normal, no move */
#define S2AMD_MOVER_OUT_OF_ITERATIONS 4 /* maxIterations casts made and displacement left */
typedef struct s2amdMover /* 128 bytes */
{
	float vertices[8][2];  /* the proxy, as s2amdShapeCast's */
	int32_t count;		   /* 1..8 */
	float radius;		   /* >= 0 */
	float position[2];	   /* where the mover stands */
	float rot[2];		   /* q {s, c}; the mover does not rotate; not checked for normalisation */
	float translation[2];  /* the displacement wanted this call */
	int32_t maxIterations; /* 1..8 casts */
	uint32_t maskBits;
	int32_t ignoreBody;	   /* shapes of this body slot are not candidates (the character's own body); < 0: none */
	uint32_t flags;		   /* S2AMD_MOVER_STATIC_ONLY or 0 */
	int32_t reserved[4];   /* 0 */
} s2amdMover;
typedef struct s2amdMoverResult /* 32 bytes */
{
	float position[2];	/* p: where the mover ends */
	float remaining[2]; /* r: the displacement not spent */
	int32_t status;		/* S2AMD_MOVER_* */
	int32_t planeCount; /* planes recorded, 0..8 */
	int32_t iterations; /* casts made, 1..maxIterations */
	int32_t advances;	/* the sum of the winners' k */
} s2amdMoverResult;
typedef struct s2amdMoverPlane /* 32 bytes */
{
	int32_t shape, body;
	float fraction;	 /* t: of the displacement that was left when the plane was met */
	float distance;	 /* D.distance where the mover stopped */
	float point[2];	 /* D.pointB: on the world shape */
	float normal[2]; /* from the world shape towards the mover; zero when they overlap */
} s2amdMoverPlane;
int s2amd_world_move_shapes(s2amdSolver* solver, const s2amdMover* movers, int32_t count, s2amdMoverResult* results /* [count] */,
							s2amdMoverPlane* planes /* [count * 8], may be NULL */);

/* (additive, API 5) World edits: the reference's eight cheap setters an interactive program calls every frame -- a body dragged by the
 * mouse joint, a motor whose speed follows a controller, wind, a thrown ball, an explosion -- applied to the resident world where it
 * lies.  Nothing is downloaded, nothing uploaded again and the constraint-graph structure is kept: no colouring, strip table or tree
 * depends on a field an edit writes.
 *   Result        the resident `bodies` and `joints` after the call are what applying edits[0], edits[1], ... one after another to the
 *                 wire records gives, each as the reference's function of the same name does it (the lines are beside the kinds):
 *                   SET_LINEAR_VELOCITY    linearVelocity = {v[0], v[1]}
 *                   SET_ANGULAR_VELOCITY   angularVelocity = v[0]
 *                   APPLY_FORCE_TO_CENTER  force = s2Add(force, {v[0], v[1]})
 *                   APPLY_LINEAR_IMPULSE   on a body of type S2AMD_BODY_DYNAMIC only (any other live type: nothing, the reference's early
 *                                          return): linearVelocity = s2MulAdd(linearVelocity, invMass, impulse); angularVelocity +=
 *                                          invI * s2Cross(s2Sub(point, position), impulse), impulse = {v[0], v[1]}, point = {v[2], v[3]}
 *                   MOUSE_SET_TARGET       targetA = {v[0], v[1]}
 *                   REVOLUTE_ENABLE_LIMIT  enableLimit = (flag != 0);  REVOLUTE_ENABLE_MOTOR  enableMotor = (flag != 0)
 *                   REVOLUTE_SET_MOTOR_SPEED  motorSpeed = v[0]
 *                 fp32 in the reference's operation order without contraction, in libs2amd.so and in libs2amd_fast.so alike.  Kinds 1-3
 *                 write whatever the body's type is, as the reference does.  Every other array of the world -- contacts, shapes, pairs,
 *                 origins, trees, the reports' state -- is untouched byte for byte.  An edit reads and writes its own target's record
 *                 only: edits on different targets commute, and only the order of the edits on one target matters (to the bit: force
 *                 adds and impulse adds are float sums).
 *   Targets       `target` is a body slot for kinds 1-4 and a joint slot for kinds 5-8.
 *   Validation    on the host, for every edit before anything is applied: a kind outside 1..8, a target outside the uploaded capacity,
 *                 reserved != 0, a NULL list with count > 0 or a negative count return S2AMD_E_INVALID and the world is unchanged -- by
 *                 valid entries earlier in the list too.  S2AMD_E_STATE without a resident world (no s2amd_world_upload, or the solver
 *                 has left the world chain).  count == 0 succeeds and does nothing.  Float values are not checked: their bits pass through.
 *   Skipped       only the device knows a slot's type: an edit whose target is a free body slot, a free joint slot or a joint of the
 *                 other type (a mouse edit on a revolute joint, a revolute edit on a mouse joint) writes nothing and is counted in
 *                 *skipped.  An APPLY_LINEAR_IMPULSE on a static or kinematic body writes nothing and is NOT counted.
 *   Ordering      the edits are enqueued on the stream s2amd_world_step uses: they land after the step before and before the step after.
 *                 With skipped == NULL the call only enqueues and reads nothing back; with a pointer it reads back one int.  The caller
 *                 may reuse `edits` as soon as the call returns.  Forces are consumed by the next step's stage 4, as the reference's are.
 * Not offered: s2Body_SetTransform (the reference declares it and never defines it; it would also move boxes and trees); mass, type or
 * damping edits; creating or destroying anything; sharded worlds; edit lists in device memory (values that live in device memory reach
 * these edits through the actuators below: s2amd_world_set_actuators, s2amd_world_import_actions); the drop-in's setters routed through
 * this call. */
#define S2AMD_EDIT_BODY_SET_LINEAR_VELOCITY 1	/* v[0..1]                      src/body.c:337-342 */
#define S2AMD_EDIT_BODY_SET_ANGULAR_VELOCITY 2	/* v[0]                         src/body.c:344-350 */
#define S2AMD_EDIT_BODY_APPLY_FORCE_TO_CENTER 3 /* v[0..1] added to force       src/body.c:352-357 */
#define S2AMD_EDIT_BODY_APPLY_LINEAR_IMPULSE 4	/* v[0..1] impulse, v[2..3] world point; dynamic bodies only, src/body.c:359-370 */
#define S2AMD_EDIT_MOUSE_SET_TARGET 5			/* v[0..1]                      src/mouse_joint.c:18-29 */
#define S2AMD_EDIT_REVOLUTE_ENABLE_LIMIT 6		/* flag                         src/revolute_joint.c:890-901 */
#define S2AMD_EDIT_REVOLUTE_ENABLE_MOTOR 7		/* flag                         src/revolute_joint.c:903-914 */
#define S2AMD_EDIT_REVOLUTE_SET_MOTOR_SPEED 8	/* v[0]                         src/revolute_joint.c:916-927 */
typedef struct s2amdWorldEdit /* 32 bytes */
{
	int32_t kind;	  /* S2AMD_EDIT_* */
	int32_t target;	  /* body slot (kinds 1-4) or joint slot (kinds 5-8) */
	int32_t flag;	  /* kinds 6, 7: stored as flag != 0 */
	int32_t reserved; /* 0 */
	float v[4];
} s2amdWorldEdit;
int s2amd_world_edit(s2amdSolver* solver, const s2amdWorldEdit* edits, int32_t count, int32_t* skipped /* may be NULL */);

/* (additive, API 5) Force fields: a write addressed by region instead of by slot -- "everything within 3 m of this point gets an impulse
 * away from it", "whatever is inside this box feels wind", "the ball carries a magnet", "this pool slows what is in it".  A field is a
 * region (a proxy with a reach, fixed in the world or attached to a body, as a sensor's) and a rule that turns every shape of a dynamic
 * body within reach into one term: an APPLY_FORCE_TO_CENTER or an APPLY_LINEAR_IMPULSE of s2amd_world_edit on the shape's body.  Two
 * entry points share their kernels: s2amd_world_apply_fields applies a list once, enqueued like an edit; s2amd_world_set_fields keeps a
 * list that the head of every s2amd_world_step applies.  Nothing is downloaded and the structure is kept, as with an edit.  LIVE and
 * xf(body) are the scene queries' definitions; D is the proximity queries' D(q, s) with transformA = the field's transform: empty cache,
 * useRadii, the FLT_EPSILON branch included.
 *   Active        the sensor report's rule: not S2AMD_FIELD_DISABLED, and body < 0 or (body < bodyCapacity and bodies[body].type !=
 *                 S2AMD_BODY_FREE).  An inactive field yields no terms; its state has active = 0, transform and box +0, lowestShape = -1.
 *   Transform T   the sensor report's: body < 0: {position, rot}; otherwise s2MulTransforms(xf(body), {position, rot}).  The centre
 *                 is c = T.p.
 *   Box           the sensor report's with `margin` read as `range`: the proximity queries' query box of {vertices, count, radius}
 *                 under T with maxDistance = range.
 *   Candidates    live; (categoryBits & maskBits) != 0; s2AABB_Overlaps(fatAABB, box); shape.body != field.body;
 *                 bodies[shape.body].type == S2AMD_BODY_DYNAMIC.  No other pruning decides a result.
 *   Term (f, s)   a candidate with D.distance <= range.  scale = 1.0f - D.distance / range (one correctly rounded divide, one
 *                 subtract) when S2AMD_FIELD_LINEAR_FALLOFF is set and range > 0, else 1.0f; m = strength * scale (one multiply);
 *                   RADIAL   g = s2MulSV(m, s2Normalize(s2Sub(D.pointB, c))), s2Normalize as src/math.c:41-52 with its zero-vector
 *                            branch: a centre on pointB gives g = 0 and the term is still applied
 *                   UNIFORM  g = s2MulSV(m, direction)
 *                   DRAG     g = s2MulSV(-m, linearVelocity), read from the body record as the earlier terms of this call left it
 *                 Without S2AMD_FIELD_AS_IMPULSE the term is APPLY_FORCE_TO_CENTER(shape.body, g); with it APPLY_LINEAR_IMPULSE(
 *                 shape.body, g, point), point = D.pointB for RADIAL and bodies[shape.body].position for the other two kinds -- both
 *                 exactly as s2amd_world_edit defines them.
 *   Result        the resident `bodies` after the call are what applying every term one after another gives, ascending by field index
 *                 and inside a field ascending by shape slot.  No term changes a pose, so every D, T and box is that of the world as
 *                 the call found it.  Terms on different bodies commute; only the order of the terms on one body matters, to the bit.
 *                 A body with no term keeps its bytes; a term of zero magnitude is still applied.  Every other array is untouched byte
 *                 for byte.  All arithmetic is fp32 in the reference's operation order without contraction, in libs2amd.so and in
 *                 libs2amd_fast.so alike; no float atomics take part: one lane sums a body's terms in the stated order.
 *   States        one record per field in list order: terms = the number of the field's terms, lowestShape = the lowest shape slot
 *                 among them or -1, the transform and the box used.  With states == NULL s2amd_world_apply_fields reads nothing back
 *                 and does not wait; with a pointer it waits for the stream once.
 *   Validation    on the host, before anything is enqueued or replaced: 0 <= count <= S2AMD_MAX_FIELDS and a non-NULL list when
 *                 count > 0; per field the sensors' checks (1 <= count <= 8; vertices[0 .. count), radius, position and rot finite;
 *                 radius >= 0; body < bodyCapacity of the resident world -- with no world resident, body is not bounded), kind in
 *                 1..3, no flag bits beyond the four below, reserved == 0, strength, direction and range finite, range >= 0.  One bad
 *                 record refuses the whole list with S2AMD_E_INVALID, and the world and the old list stand.  S2AMD_E_STATE without a
 *                 resident world for s2amd_world_apply_fields and s2amd_world_field_states; s2amd_world_set_fields is accepted before
 *                 any world and the list holds across uploads, as the sensors do (a field whose body is outside the new world's
 *                 bodyCapacity is inactive there).
 *   Ordering      s2amd_world_apply_fields is enqueued on the stream s2amd_world_step uses, like an edit; the caller may reuse
 *                 `fields` as soon as it returns.  A non-empty persistent list is applied once per s2amd_world_step call, in front of
 *                 stage 3 -- outside the loop that repeats a step the library has to run again, so a repeated step applies it once --
 *                 and the effect is what s2amd_world_apply_fields(list) immediately before the step would give.  Forces are consumed by
 *                 that step's stage 4.  s2amd_world_field_states returns the states of the last step's application (S2AMD_E_CAPACITY
 *                 with *count filled when capacity is less): S2AMD_E_STATE if no step ran since the list was set or since the last
 *                 upload, *count = 0 with an empty list.  With an empty list a step enqueues nothing and allocates nothing.  The first
 *                 use of fields after an upload builds a body -> shapes list on the device (a stable radix sort; no host sort, no wait).
 * The reference has no fields: the composition is ours; every distance is the reference's s2ShapeDistance and every term the
 * reference's setter, bit for bit.  Not offered: torque (the reference has no setter for it); fields that act on kinematic or static
 * bodies; sharded worlds; lists in device memory (forces whose values live in device memory are the actuators' below:
 * s2amd_world_set_actuators, s2amd_world_import_actions); the drop-in routed through this call; the device trees as an accelerator (a field
 * looks at every shape of every dynamic body, and a body with hundreds of shapes is walked by one lane: correct, not fast). */
#define S2AMD_MAX_FIELDS 1024
#define S2AMD_FIELD_RADIAL 1  /* along s2Normalize(pointB - centre) */
#define S2AMD_FIELD_UNIFORM 2 /* along `direction` */
#define S2AMD_FIELD_DRAG 3	  /* against the body's linear velocity as it stands */
#define S2AMD_FIELD_DISABLED 1
#define S2AMD_FIELD_AS_IMPULSE 2	 /* the term is an APPLY_LINEAR_IMPULSE instead of an APPLY_FORCE_TO_CENTER */
#define S2AMD_FIELD_LINEAR_FALLOFF 4 /* scale = 1 - distance / range instead of 1 */
typedef struct s2amdField /* 128 bytes */
{
	float vertices[8][2]; /* the region's proxy in its own frame, as s2amdSensor's */
	int32_t count;		  /* 1..8 */
	float radius;		  /* >= 0 */
	float position[2];	  /* the frame: in the world (body < 0) or relative to the body */
	float rot[2];		  /* {s, c} */
	float range;		  /* reach beyond the proxy: acts where D.distance <= range; >= 0, finite */
	uint32_t maskBits;
	int32_t body;		/* < 0: fixed in the world */
	int32_t kind;		/* S2AMD_FIELD_RADIAL, _UNIFORM, _DRAG */
	int32_t flags;		/* S2AMD_FIELD_DISABLED, _AS_IMPULSE, _LINEAR_FALLOFF */
	float strength;		/* finite, either sign (a negative RADIAL pulls) */
	float direction[2]; /* UNIFORM only; finite, not normalised by the library */
	int32_t reserved;	/* 0 */
	int32_t pad;		/* (fills the record to 128 bytes; not read) */
} s2amdField;
typedef struct s2amdFieldState /* 64 bytes */
{
	int32_t field, body, active, terms, lowestShape, pad[3];
	float position[2], rot[2]; /* the world transform used */
	float box[4];			   /* the candidate box used */
} s2amdFieldState;
int s2amd_world_apply_fields(s2amdSolver* solver, const s2amdField* fields, int32_t count, s2amdFieldState* states /* [count], may be NULL */);
int s2amd_world_set_fields(s2amdSolver* solver, const s2amdField* fields, int32_t count); /* replaces the whole list; count 0 clears */
int s2amd_world_field_states(s2amdSolver* solver, s2amdFieldState* out, int32_t capacity, int32_t* count);

/* (additive, API 5) Actuators: the write half of a control loop that stays on the device.  A persistent list of actuators maps channels
 * of an ACTION VECTOR that lives in device memory onto s2amd_world_edit's edits, in front of every s2amd_world_step: a policy network's
 * output, a PD controller's set points or a scripted platform's velocities arrive device to device (s2amd_world_import_actions), the
 * observations leave device to device (s2amd_world_export_observations, s2amd_world_export_ray_ranges, s2amd_world_export_grid_occupancy,
 * s2amd_export_poses), and a step with actuators gains no host wait.  Nothing is downloaded and the structure is kept, as with an edit.
 *   Action buffer the library owns one float[channels] in device memory, zeroed whenever the list is replaced; values hold until they
 *                 are overwritten (zero-order hold), across steps and uploads.  s2amd_world_set_actions copies host values into
 *                 [first, first + count) through pinned memory: the caller may reuse its array on return.  s2amd_world_import_actions
 *                 copies them from device memory, as s2amd_export_poses in reverse.  Both are enqueued on the stream s2amd_world_step
 *                 uses and do not wait.  The SOURCE of s2amd_world_import_actions must be complete when the call is made: a caller that
 *                 fills it on a stream of its own synchronises that stream first (the library's stream does not wait for any other).
 *   Command       for each component i < width of the kind: a_i = actions[channel + i]; t = gain * a_i (one multiply); t = t + bias (one
 *                 add); u_i = t < lower ? lower : (t > upper ? upper : t).  fp32 without contraction, in libs2amd.so and in
 *                 libs2amd_fast.so alike.
 *   Kinds         1 BODY_FORCE            width 2  APPLY_FORCE_TO_CENTER(target, {u0, u1})
 *                 2 BODY_THRUST           width 1  APPLY_FORCE_TO_CENTER(target, s2MulSV(u0, s2RotateVector(rot(target), axis)))
 *                 3 BODY_LINEAR_VELOCITY  width 2  SET_LINEAR_VELOCITY(target, {u0, u1})
 *                 4 BODY_ANGULAR_VELOCITY width 1  SET_ANGULAR_VELOCITY(target, u0)
 *                 5 REVOLUTE_MOTOR_SPEED  width 1  REVOLUTE_SET_MOTOR_SPEED(target, u0)
 *                 6 REVOLUTE_SERVO        width 1  angle = s2RelativeAngle(rot(bodyB), rot(bodyA)) - referenceAngle (the joint report's
 *                                                  formula and its atan2; a body outside the body array counts as unrotated);
 *                                                  v = kp * (u0 - angle); speed = v < -maxSpeed ? -maxSpeed : (v > maxSpeed ? maxSpeed : v);
 *                                                  REVOLUTE_SET_MOTOR_SPEED(target, speed)
 *                 7 MOUSE_TARGET          width 2  MOUSE_SET_TARGET(target, {u0, u1})
 *                 `target` is a body slot for kinds 1-4 and a joint slot for kinds 5-7.
 *   Status        decided in this order.  DISABLED: S2AMD_ACTUATOR_DISABLED is set.  SKIPPED: the target is outside the resident
 *                 capacities, a free body slot, a free joint slot or a joint of the other type -- only the device knows, as with edits.
 *                 NONFINITE: some a_i has all exponent bits set (a NaN or an infinity) -- a policy that diverges must not poison the
 *                 world.  APPLIED: everything else.  Only an APPLIED actuator yields a term.
 *   Result        the resident `bodies` and `joints` after the pass are what s2amd_world_edit gives for the terms of the APPLIED
 *                 actuators in list order, each term exactly the edit of that name.  No term changes a pose, so every rot and angle
 *                 read is that of the world as the pass found it; terms on different targets commute, and only the order of the terms
 *                 on one target matters, to the bit.  Every other array is untouched byte for byte.
 *   When          a non-empty list is applied once per s2amd_world_step call, in front of the persistent force fields (a DRAG field
 *                 sees the velocity an actuator set), in front of stage 3 and outside the loop that repeats a solve.  The list and the
 *                 buffer hold across uploads; an actuator whose target is outside the new capacities is SKIPPED.  With no list a step
 *                 enqueues nothing and allocates nothing.
 *   States        one record per actuator in list order, of the last step's pass: `action` as read (+0 when DISABLED), `command` = u,
 *                 `output` = the term's v[0..1] (the servo's output[0] is the speed), `angle` = the servo's measured angle; command,
 *                 output and angle are +0 unless APPLIED, and every component beyond the kind's width is +0.
 *                 s2amd_world_actuator_counts gives the number of actuators per status in one 16-byte read.  Both getters wait for the
 *                 stream; the step does not.  S2AMD_E_STATE if no step ran since the list was set or since the last upload;
 *                 S2AMD_E_CAPACITY with *count filled when the buffer is too small; *count = 0 (and zero counts) with an empty list.
 *   Validation    on the host, before anything is replaced: 0 <= count <= S2AMD_MAX_ACTUATORS; with count > 0 a non-NULL list and
 *                 1 <= channels <= S2AMD_MAX_ACTION_CHANNELS; per record kind in 1..7, target >= 0 (and below the resident body or
 *                 joint capacity when a world is resident), channel >= 0 and channel + width <= channels, no flag bits beyond
 *                 DISABLED, reserved all 0, gain, bias, axis and kp finite, lower <= upper and neither a NaN (infinities are allowed),
 *                 maxSpeed >= 0 and not a NaN.  One bad record refuses the whole list with S2AMD_E_INVALID, and the old list and the
 *                 buffer stand.  The two writers return S2AMD_E_INVALID for a NULL pointer with count > 0, a negative first or count or
 *                 a range past `channels`, and S2AMD_E_STATE with no list set.  The setter and the writers need no resident world.
 *   Cost          the list is static, so its grouping by target is made once, in the setter: a step launches one kernel when all
 *                 targets are distinct and two when some target occurs twice.  No sort, no float atomics, no host wait in the step.
 * The reference has no actuators: the composition is ours, every term the reference's setter, bit for bit.  Not offered: torque (the
 * reference has no setter for it); impulses; actuator lists themselves in device memory; sharded worlds; the drop-in routed through
 * this; PD on anything but a revolute angle. */
#define S2AMD_MAX_ACTUATORS 16384
#define S2AMD_MAX_ACTION_CHANNELS 65536
#define S2AMD_ACTUATOR_BODY_FORCE 1
#define S2AMD_ACTUATOR_BODY_THRUST 2
#define S2AMD_ACTUATOR_BODY_LINEAR_VELOCITY 3
#define S2AMD_ACTUATOR_BODY_ANGULAR_VELOCITY 4
#define S2AMD_ACTUATOR_REVOLUTE_MOTOR_SPEED 5
#define S2AMD_ACTUATOR_REVOLUTE_SERVO 6
#define S2AMD_ACTUATOR_MOUSE_TARGET 7
#define S2AMD_ACTUATOR_DISABLED 1
#define S2AMD_ACTUATOR_STATUS_APPLIED 0
#define S2AMD_ACTUATOR_STATUS_DISABLED 1
#define S2AMD_ACTUATOR_STATUS_SKIPPED 2
#define S2AMD_ACTUATOR_STATUS_NONFINITE 3
typedef struct s2amdActuator /* 64 bytes */
{
	int32_t kind;	 /* S2AMD_ACTUATOR_BODY_FORCE .. _MOUSE_TARGET */
	int32_t target;	 /* body slot (kinds 1-4) or joint slot (kinds 5-7) */
	int32_t channel; /* the first of the kind's `width` channels */
	int32_t flags;	 /* S2AMD_ACTUATOR_DISABLED */
	float gain, bias, lower, upper; /* u = clamp(gain * a + bias, lower, upper) */
	float axis[2];	 /* BODY_THRUST: the direction in the body's frame; not normalised by the library */
	float kp, maxSpeed; /* REVOLUTE_SERVO */
	int32_t reserved[4]; /* 0 */
} s2amdActuator;
typedef struct s2amdActuatorState /* 48 bytes */
{
	int32_t actuator, target, status, pad;
	float action[2], command[2], output[2];
	float angle;
	int32_t pad2;
} s2amdActuatorState;
int s2amd_world_set_actuators(s2amdSolver* solver, const s2amdActuator* list, int32_t count, int32_t channels); /* replaces the list; count 0 clears */
int s2amd_world_set_actions(s2amdSolver* solver, const float* hostValues, int32_t first, int32_t count);	   /* host -> the library's action buffer */
int s2amd_world_import_actions(s2amdSolver* solver, const void* deviceValues, int32_t first, int32_t count); /* device -> the same, as s2amd_export_poses in reverse */
int s2amd_world_actuator_states(s2amdSolver* solver, s2amdActuatorState* out, int32_t capacity, int32_t* count);
int s2amd_world_actuator_counts(s2amdSolver* solver, int32_t counts[4]); /* actuators per status {APPLIED, DISABLED, SKIPPED, NONFINITE} */

/* (additive, API 5) Observers: the read half of a control loop that stays on the device.  A persistent list of observers maps quantities
 * of the resident world, and of the reports that already run behind the step, onto channels of an OBSERVATION VECTOR in the library's
 * device memory: joint angles and speeds, a body's pose and velocity in another body's frame, whether a foot touches, a ray range, the
 * previous action.  The vector is normalised per observer, optionally stacked over the last `frames` steps, and leaves in one
 * device-to-device call (s2amd_world_export_observations_async) that does not wait for the host.  Everything is read from the resident
 * arrays AFTER the step's stage 4, like the other reports; the pass is read-only on the world.
 *   Kinds         xf(b) = {origins[b], bodies[b].rot}; frame < 0 is the world frame.  The raw value x:
 *                 1 BODY_POINT             width 2  p = s2TransformPoint(xf(target), local); with a frame s2InvTransformPoint(xf(frame), p)
 *                 2 BODY_ROTATION          width 2  q = rot(target), with a frame s2InvMulRot(rot(frame), rot(target)); x = {q.s, q.c}
 *                 3 BODY_ANGLE             width 1  atan2f(q.s, q.c) of kind 2's q (the atan2 of the body and joint reports)
 *                 4 BODY_LINEAR_VELOCITY   width 2  v = linearVelocity(target); with S2AMD_OBSERVER_RELATIVE and a frame
 *                                                   v = s2Sub(v, linearVelocity(frame)); with a frame s2InvRotateVector(rot(frame), v)
 *                 5 BODY_ANGULAR_VELOCITY  width 1  w(target); with S2AMD_OBSERVER_RELATIVE and a frame w(target) - w(frame)
 *                 6 REVOLUTE_ANGLE         width 1  the joint report's `angle` of joint `target` (what the servo actuator measures)
 *                 7 REVOLUTE_SPEED         width 1  the joint report's `angularSpeed`, w(bodyB) - w(bodyA)
 *                 8 REVOLUTE_MOTOR_IMPULSE width 1  joints[target].motorImpulse as stored
 *                 9 BODY_CONTACT           width 2  {touching > 0 ? 1.0f : +0.0f, normalImpulse} of s2amd_world_body_sums' record of body
 *                                                   `target`, this step
 *                 10 RAY_RANGE             width 1  entry `target` of s2amd_world_ray_ranges, this step, verbatim
 *                 11 ACTION                width 1  channel `target` of the actuators' action buffer as it stands when the pass runs,
 *                                                   which is what this step's actuator pass read
 *                 `target` is a body slot for kinds 1-5 and 9, a joint slot for kinds 6-8, a ray for kind 10, an action channel for 11.
 *   Value         for each component i < width: t = gain * x_i (one multiply); t = t + bias (one add);
 *                 y_i = t < lower ? lower : (t > upper ? upper : t): the actuators' command rule, so a NaN passes through unclamped.
 *                 fp32, one rounding per operation in the order given, without contraction, in libs2amd.so and libs2amd_fast.so alike.
 *   Status        decided in this order.  DISABLED: S2AMD_OBSERVER_DISABLED is set.  SKIPPED: the target or the frame is outside the
 *                 resident capacities or a free slot; a joint that is not revolute (kinds 6-8); kinds 10 and 11 with a target at or
 *                 beyond the ray count of the ray list or the channels of the actuator list, where such a list is set (with no list
 *                 there is no count to be beyond: that is SOURCE_OFF).  SOURCE_OFF: kind 9 when the step did not run with
 *                 S2AMD_REPORT_BODY_SUMS; kind 10 without S2AMD_RAY_REPORT_RANGES or without a ray list; kind 11 without an actuator
 *                 list.  OBSERVED: everything else.
 *   Result        float[frames][channels]: frame 0 is this step, frame k the k-th reporting step before it.  An observer that is not
 *                 OBSERVED writes +0 to its channels and has raw and value +0; channels no observer covers read +0; components beyond
 *                 the kind's width are +0 in the state.  The first reporting step after a re-base fills every frame with its own
 *                 vector; a re-base happens at s2amd_world_upload, when the list is replaced, and when the report flags go from 0 to
 *                 non-zero.  The frames are a ring: a step writes one row and moves no old one, an export is at most two copies.
 *   When          the ninth report of a step, behind the grid report, so the contact sums and the ray ranges it reads are this
 *                 step's.  A step with the report flags at 0 neither advances the history nor enqueues anything; any non-zero flags
 *                 run the pass, S2AMD_OBSERVATION_REPORT_VECTOR opens the vector's three getters and _STATES writes and opens the
 *                 states.  A step the library repeats reports once.  The list, `channels` and `frames` hold across uploads.  The step
 *                 gains no host wait; s2amd_world_observations, s2amd_world_export_observations, s2amd_world_observer_states and
 *                 s2amd_world_observer_counts wait for the stream, s2amd_world_export_observations_async enqueues the copies and an
 *                 event in `slot` (0..3; s2amd_export_wait) and waits for nothing.  An export is frames * channels floats, a size
 *                 known on the host.
 *   Validation    on the host, before anything is replaced: 0 <= count <= S2AMD_MAX_OBSERVERS; with count > 0 a non-NULL list,
 *                 1 <= channels <= S2AMD_MAX_OBSERVATION_CHANNELS and 1 <= frames <= S2AMD_MAX_OBSERVATION_FRAMES; per record kind in
 *                 1..11, target >= 0, frame -1 or >= 0 and -1 for kinds 6-11, channel >= 0 and channel + width <= channels, no flag
 *                 bits beyond DISABLED | RELATIVE, reserved all 0, gain, bias and local finite, lower <= upper and neither a NaN
 *                 (infinities are allowed); no two observers' channel ranges overlap.  One bad record refuses the whole list with
 *                 S2AMD_E_INVALID, and the old list, vector and history stand.  The getters: S2AMD_E_STATE without a resident world
 *                 or when the getter's flag was not set before the last step; S2AMD_E_CAPACITY with *count filled; *count = 0 (and
 *                 zero counts) with an empty list.
 *   Cost          channel ranges are disjoint, so the pass is one launch of one lane per observer with no ordering rule; the vector
 *                 is zeroed once, in the setter.  No float atomics, no sort, no scratch, no host wait in the step.
 * The reference has no observers: the composition is ours, every term the reference's function of that name.  Not offered: sharded
 * worlds; observer lists themselves in device memory; mouse-joint quantities; grid cells in the vector (they have their own export,
 * s2amd_world_export_grid_occupancy); running normalisation statistics.  Rewards and termination are the episode report's, below
 * (s2amd_world_set_episodes); resetting the bodies of a finished agent is the resets', below them (s2amd_world_set_resets). */
#define S2AMD_MAX_OBSERVERS 16384
#define S2AMD_MAX_OBSERVATION_CHANNELS 65536
#define S2AMD_MAX_OBSERVATION_FRAMES 16
#define S2AMD_OBSERVER_BODY_POINT 1
#define S2AMD_OBSERVER_BODY_ROTATION 2
#define S2AMD_OBSERVER_BODY_ANGLE 3
#define S2AMD_OBSERVER_BODY_LINEAR_VELOCITY 4
#define S2AMD_OBSERVER_BODY_ANGULAR_VELOCITY 5
#define S2AMD_OBSERVER_REVOLUTE_ANGLE 6
#define S2AMD_OBSERVER_REVOLUTE_SPEED 7
#define S2AMD_OBSERVER_REVOLUTE_MOTOR_IMPULSE 8
#define S2AMD_OBSERVER_BODY_CONTACT 9
#define S2AMD_OBSERVER_RAY_RANGE 10
#define S2AMD_OBSERVER_ACTION 11
#define S2AMD_OBSERVER_DISABLED 1
#define S2AMD_OBSERVER_RELATIVE 2
#define S2AMD_OBSERVER_STATUS_OBSERVED 0
#define S2AMD_OBSERVER_STATUS_DISABLED 1
#define S2AMD_OBSERVER_STATUS_SKIPPED 2
#define S2AMD_OBSERVER_STATUS_SOURCE_OFF 3
#define S2AMD_OBSERVATION_REPORT_VECTOR 1
#define S2AMD_OBSERVATION_REPORT_STATES 2
typedef struct s2amdObserver /* 64 bytes */
{
	int32_t kind;	 /* S2AMD_OBSERVER_BODY_POINT .. _ACTION */
	int32_t target;	 /* body slot, joint slot, ray or action channel: see Kinds */
	int32_t frame;	 /* kinds 1-5: the body whose frame the value is expressed in, or -1 for the world frame; -1 otherwise */
	int32_t channel; /* the first of the kind's `width` channels */
	int32_t flags;	 /* S2AMD_OBSERVER_DISABLED | S2AMD_OBSERVER_RELATIVE */
	float gain, bias, lower, upper; /* y = clamp(gain * x + bias, lower, upper) */
	float local[2];	 /* BODY_POINT: the point in the target's frame */
	int32_t reserved[5]; /* 0 */
} s2amdObserver;
typedef struct s2amdObserverState /* 32 bytes */
{
	int32_t observer, status;
	float raw[2], value[2];
	int32_t pad[2];
} s2amdObserverState;
int s2amd_world_set_observers(s2amdSolver* solver, const s2amdObserver* list, int32_t count, int32_t channels, int32_t frames); /* replaces the list; count 0 clears */
int s2amd_world_set_observation_report(s2amdSolver* solver, int32_t flags); /* S2AMD_OBSERVATION_REPORT_* */
int s2amd_world_observations(s2amdSolver* solver, float* out, int32_t capacity, int32_t* count); /* host; frames * channels floats */
int s2amd_world_export_observations(s2amdSolver* solver, void* deviceVector, int32_t capacity); /* device to device, waits, as s2amd_world_export_ray_ranges */
int s2amd_world_export_observations_async(s2amdSolver* solver, void* deviceVector, int32_t capacity, int32_t slot); /* enqueued, an event in slot 0..3: s2amd_export_wait(slot) */
int s2amd_world_observer_states(s2amdSolver* solver, s2amdObserverState* out, int32_t capacity, int32_t* count);
int s2amd_world_observer_counts(s2amdSolver* solver, int32_t counts[4]); /* observers per status {OBSERVED, DISABLED, SKIPPED, SOURCE_OFF} */

/* (additive, API 5) Episodes: the last leg of a control loop that stays on the device.  A persistent list of EPISODE RULES over AGENTS is
 * evaluated on the device as the tenth report of a step, on the observation vector of THIS step: it gives one reward and one flags word
 * per agent, keeps the episode accounting (length, return, automatic restart, time limit) in device memory, and lists the agents that
 * finished.  Rewards and flags leave in one device-to-device call (s2amd_world_export_episode_step_async) that does not wait for the
 * host.  The pass is read-only on the world and touches no step kernel.  All arithmetic is fp32, one rounding per operation in the order
 * given, without contraction, in libs2amd.so and libs2amd_fast.so alike.
 *   Source        a rule reads the observation vector of this step (the pass runs behind the observers'): a = obs[frameA][channelA],
 *                 where frame k is row (head + k) % frames of the observers' ring.  With S2AMD_EPISODE_RULE_DIFFERENCE
 *                 x = a - obs[frameB][channelB] (one subtract), otherwise x = a.  channelA == -1 means no source: x = +0.0f, and the
 *                 rule is never SKIPPED or SOURCE_OFF.  The first reporting step after the observers' re-base has every frame equal,
 *                 so a progress rule (frameB = 1 on the same channel) reads +0 there.
 *   Status        decided in this order.  DISABLED: S2AMD_EPISODE_RULE_DISABLED is set.  SKIPPED: a channel read is at or beyond the
 *                 current observer list's `channels`, or a frame at or beyond its `frames`, where a list is set (the observer list was
 *                 replaced by a narrower one).  SOURCE_OFF: a channel is read and the observation report did not run this step, or no
 *                 observer list is set.  EVALUATED: everything else.  A rule that is not EVALUATED contributes nothing and has
 *                 x = f = value = +0 and fired = 0.
 *   Rule value    f = shape(x): LINEAR x, ABS fabsf(x), SQUARE x * x (one multiply).  inside = lower <= f && f <= upper (a NaN is not
 *                 inside); test = inside != (flags & S2AMD_EPISODE_RULE_OUTSIDE).
 *                 1 REWARD_VALUE  y = clamp(gain * f + bias, lower, upper): the actuators' and observers' rule, a NaN passes through
 *                 2 REWARD_TEST   y = test ? gain : bias
 *                 3 TERMINATE     fired = test; y = test ? gain : +0.0f (gain is the terminal bonus or penalty; bias must be 0)
 *                 4 TRUNCATE      as TERMINATE, for the other bit
 *   Agent         per reporting step, one agent's rules taken in LIST ORDER (the reward is a float sum: the order matters to the bit).
 *                 1. if the pass is fresh (a re-base) or the agent's previous flags & 3 != 0: episodeLength = 0, episodeReturn = +0.
 *                 2. r = +0; for every EVALUATED rule r = r + y; a fired TERMINATE rule sets S2AMD_EPISODE_TERMINATED, a fired TRUNCATE
 *                    rule S2AMD_EPISODE_TRUNCATED; `rule` is the list index of the first fired rule, else -1.
 *                 3. episodeLength += 1; with stepLimits[a] > 0 && episodeLength >= stepLimits[a]: TRUNCATED | TIME_LIMIT.
 *                 4. episodeReturn = episodeReturn + r; reward = r.
 *                 5. if flags & 3: episodes += 1, lastReturn = episodeReturn, lastLength = episodeLength; the accounting restarts by
 *                    itself at the next reporting step (step 1), the vector-environment convention.
 *                 An agent with no rules has reward +0 and still counts steps.
 *   Re-base       all accumulators, `episodes` and the last* fields go to zero and the next pass is fresh: at s2amd_world_upload, when
 *                 the rule list is replaced, and when the report flags go from 0 to non-zero.  A step with the flags at 0 neither
 *                 counts nor enqueues anything.  A step the library repeats reports once.  The list holds across uploads.
 *   Events        one record per agent with flags & 3 this step, ascending by agent, with the values of step 5.
 *   Counts        counts[0..3]: rules per status; counts[4..7]: agents done (flags & 3), terminated, truncated, at the time limit.
 *                 Integers only, from wave ballots.
 *   Report flags  any non-zero flags run the pass.  S2AMD_EPISODE_REPORT_STEP opens s2amd_world_episode_rewards, _flags and the two
 *                 exports; _STATES opens s2amd_world_episode_states; _RULE_STATES writes and opens s2amd_world_episode_rule_states;
 *                 _EVENTS runs the compaction and opens s2amd_world_episode_events.  s2amd_world_episode_counts answers for any.
 *   Validation    on the host, before anything is replaced: 0 <= agents <= S2AMD_MAX_EPISODE_AGENTS, 0 <= ruleCount <=
 *                 S2AMD_MAX_EPISODE_RULES; ruleCount > 0 needs agents > 0 and a non-NULL list; per record kind in 1..4, shape in 0..2,
 *                 agent in [0, agents), channelA >= -1, frameA >= 0, channelB and frameB >= 0 with DIFFERENCE and 0 without,
 *                 DIFFERENCE needs channelA >= 0, no unknown flag bits, reserved all 0, gain and bias finite, lower <= upper and
 *                 neither a NaN (infinities are allowed), bias == 0 for kinds 3 and 4; stepLimits[i] >= 0.  One bad record refuses the
 *                 whole call with S2AMD_E_INVALID, and the old list and its accounting stand.  Whether a channel fits the observer list
 *                 is the device's to judge (SKIPPED).  The getters: S2AMD_E_STATE without a resident world or when the getter's flag
 *                 was not set before the last step; S2AMD_E_CAPACITY with *count filled; *count = 0 (and zero counts) with no list.
 *   Cost          the setter groups the static list once, stably by (agent, list index).  A reporting step is two launches -- one lane
 *                 per rule, then one lane per agent walking its contiguous run in order -- and a third, one workgroup, only with
 *                 S2AMD_EPISODE_REPORT_EVENTS.  No float atomics, no sort, no scratch, no memset and no host wait in the step.
 * The reference has no episodes: the statement is ours.  Not offered here: resetting the bodies of a finished agent (that is
 * s2amd_world_set_resets, below, which reads this pass's flags); sharded worlds; rules in device memory; transcendental reward shapes
 * such as exp or tanh (they cannot be stated bit for bit); discounting; float sums across agents. */
#define S2AMD_MAX_EPISODE_AGENTS 16384
#define S2AMD_MAX_EPISODE_RULES 65536
#define S2AMD_EPISODE_REWARD_VALUE 1
#define S2AMD_EPISODE_REWARD_TEST 2
#define S2AMD_EPISODE_TERMINATE 3
#define S2AMD_EPISODE_TRUNCATE 4
#define S2AMD_EPISODE_SHAPE_LINEAR 0
#define S2AMD_EPISODE_SHAPE_ABS 1
#define S2AMD_EPISODE_SHAPE_SQUARE 2
#define S2AMD_EPISODE_RULE_DISABLED 1
#define S2AMD_EPISODE_RULE_DIFFERENCE 2
#define S2AMD_EPISODE_RULE_OUTSIDE 4
#define S2AMD_EPISODE_STATUS_EVALUATED 0
#define S2AMD_EPISODE_STATUS_DISABLED 1
#define S2AMD_EPISODE_STATUS_SKIPPED 2
#define S2AMD_EPISODE_STATUS_SOURCE_OFF 3
#define S2AMD_EPISODE_TERMINATED 1
#define S2AMD_EPISODE_TRUNCATED 2
#define S2AMD_EPISODE_TIME_LIMIT 4
#define S2AMD_EPISODE_REPORT_STEP 1
#define S2AMD_EPISODE_REPORT_STATES 2
#define S2AMD_EPISODE_REPORT_RULE_STATES 4
#define S2AMD_EPISODE_REPORT_EVENTS 8
typedef struct s2amdEpisodeRule /* 64 bytes */
{
	int32_t kind;	  /* S2AMD_EPISODE_REWARD_VALUE .. _TRUNCATE */
	int32_t agent;	  /* [0, agents) */
	int32_t channelA; /* the observation channel read, or -1 for no source (x = +0) */
	int32_t frameA;	  /* ... and its frame (0: this step) */
	int32_t channelB, frameB; /* with S2AMD_EPISODE_RULE_DIFFERENCE: what is subtracted; 0 otherwise */
	int32_t shape;	  /* S2AMD_EPISODE_SHAPE_* */
	int32_t flags;	  /* S2AMD_EPISODE_RULE_DISABLED | _DIFFERENCE | _OUTSIDE */
	float gain, bias, lower, upper;
	int32_t reserved[4]; /* 0 */
} s2amdEpisodeRule;
typedef struct s2amdEpisodeState /* 32 bytes */
{
	int32_t flags; /* S2AMD_EPISODE_TERMINATED | _TRUNCATED | _TIME_LIMIT of this step */
	int32_t rule;  /* the list index of the first fired rule, else -1 */
	float reward, episodeReturn;
	int32_t episodeLength, episodes;
	float lastReturn;
	int32_t lastLength;
} s2amdEpisodeState;
typedef struct s2amdEpisodeRuleState /* 32 bytes */
{
	int32_t rule, status;
	float x, f, value;
	int32_t fired;
	int32_t pad[2];
} s2amdEpisodeRuleState;
typedef struct s2amdEpisodeEvent /* 16 bytes */
{
	int32_t agent, flags, episodeLength;
	float episodeReturn;
} s2amdEpisodeEvent;
int s2amd_world_set_episodes(s2amdSolver* solver, const s2amdEpisodeRule* rules, int32_t ruleCount, int32_t agents, const int32_t* stepLimits); /* replaces everything; agents 0 clears; stepLimits: [agents], NULL or 0 = no limit */
int s2amd_world_set_episode_report(s2amdSolver* solver, int32_t flags); /* S2AMD_EPISODE_REPORT_* */
int s2amd_world_episode_rewards(s2amdSolver* solver, float* out, int32_t capacity, int32_t* count); /* host; one float per agent */
int s2amd_world_episode_flags(s2amdSolver* solver, int32_t* out, int32_t capacity, int32_t* count); /* host; one word per agent */
int s2amd_world_export_episode_step(s2amdSolver* solver, void* deviceRewards, void* deviceFlags, int32_t capacity); /* device to device, both arrays, waits */
int s2amd_world_export_episode_step_async(s2amdSolver* solver, void* deviceRewards, void* deviceFlags, int32_t capacity, int32_t slot); /* enqueued, an event in slot 0..3: s2amd_export_wait(slot) */
int s2amd_world_episode_states(s2amdSolver* solver, s2amdEpisodeState* out, int32_t capacity, int32_t* count);
int s2amd_world_episode_rule_states(s2amdSolver* solver, s2amdEpisodeRuleState* out, int32_t capacity, int32_t* count); /* in list order */
int s2amd_world_episode_events(s2amdSolver* solver, s2amdEpisodeEvent* out, int32_t capacity, int32_t* count); /* agents done this step, ascending */
int s2amd_world_episode_counts(s2amdSolver* solver, int32_t counts[8]); /* rules per status [0..3]; agents done, terminated, truncated, at the time limit [4..7] */

/* (additive, API 5) Resets: the bodies and joints of a finished agent go back to a start state the caller gave, on the device.  A
 * persistent list of body records and joint records over agents; the pass runs behind the episode pass of a step for the agents whose
 * episode ended in it, or between steps for the agents a call names.  Nothing is downloaded, uploaded or re-based, and no structure is
 * built: the boxes, contacts and pair states a teleport invalidates are put right as the reference's own functions would -- stage 4's
 * box arithmetic (src/world.c:259-297), s2BroadPhase_MoveProxy's "new fat box, into the move buffer" and s2CreateContact's empty
 * manifold (src/contact.c:137-203).  The reference declares s2Body_SetTransform and never defines it: the composition is ours.
 *   Trigger       step mode (S2AMD_RESET_ON_EPISODE_END): trigger[a] = episode flags[a] & 3 of this step's episode pass, 0 for a >= the
 *                 episode list's agents, and 0 for everybody when the episode pass did not run this step (counts[7] = 1, source off, and
 *                 nothing is enqueued).  One-shot (s2amd_world_reset_agents): the agents listed, or all of them with NULL and
 *                 S2AMD_RESET_ALL; enqueued like an edit behind the last step, it waits for nothing.
 *   The pass      stated sequentially (== tests/reset_ref.py); n = the agent's `resets` counter before the pass:
 *                 1. every body record k of a triggered agent that is not DISABLED: SKIPPED when the slot is beyond the capacity, FREE
 *                    or STATIC; else position, rot, linearVelocity and angularVelocity come from the record with jitter, deltaPosition,
 *                    force and torque become +0, every other field is kept, and the body is marked.
 *                 2. jitter of component c (0, 1 position; 2, 3 linear velocity; 4 angular velocity): h = fmix32(seed + 0x9e3779b9 *
 *                    (uint32)(8 * k + c)), h = fmix32(h ^ (uint32)n) (MurmurHash3's finaliser), u = (float)(h >> 8) * 2^-24,
 *                    t = 2 * u - 1 (both exact), value = base + t * jitter: one multiply, one add.  A component whose jitter is 0
 *                    copies the base's bits, so -0 stays -0.
 *                 3. origins[body] = position - rotate(rot, localCenter), in stage 4's operation order.
 *                 4. every live shape of a marked body: the tight box as stage 4 computes it, the fat box = the tight box -+
 *                    S2_AABB_MARGIN unconditionally, enlarged = 1.  No other shape is touched: their flags stand.
 *                 5. every live pair slot whose contact has a marked bodyA or bodyB: pointCount, frictionPersisted, normal and both
 *                    points zero; in the pair state everything but shapeA and shapeB zero.  bodyA, bodyB, friction and constraintIndex
 *                    are kept.  What stage 3 remembers as "touching after the last step" is not written: the next step compares with
 *                    it, so a manifold that touches again is no flip, and a pair the teleport parted is found SEPARATED and destroyed
 *                    by the next stage 3 as always (s2amd_world_separated).
 *                 6. every joint record of a triggered agent that is not DISABLED: SKIPPED for a slot beyond the capacity or FREE; else
 *                    impulse, motorImpulse, lowerImpulse and upperImpulse become +0, and with S2AMD_RESET_JOINT_SETTINGS a revolute
 *                    joint takes enableMotor, enableLimit and motorSpeed, a mouse joint targetA, from the record.  A joint that is not
 *                    listed is not touched, even when its body is marked.
 *                 7. resets[a] += 1 for every triggered agent.  counts = {agents reset, bodies applied, bodies skipped, joints applied,
 *                    joints skipped, shapes moved, contacts emptied, source off}: integers from wave ballots.
 *   Reports       no report is re-based by a reset: each of the ten still compares the world after this step with the world after the
 *                 step before, so a contact that touched and is parted by a reset is `ended` in the next step, a teleported shape may
 *                 enter or leave a view or a sensor, and a body report sees the jump as motion.  The observation ring keeps its frames:
 *                 the first observation of a new episode is the state one step after the reset, and a DIFFERENCE rule across frames
 *                 reads the jump in that step.
 *   Pairs         info.movedCount stays the refit's.  Call s2amd_world_find_pairs when movedCount > 0 or any exported done & 3 was
 *                 set, and after s2amd_world_reset_agents: the query then runs on the flags as they stand, the resets' included.
 *   Validation    on the host, before anything is replaced: 0 <= agents <= S2AMD_MAX_RESET_AGENTS, counts within S2AMD_MAX_RESET_BODIES
 *                 and _JOINTS, records need agents > 0 and a non-NULL list; per record agent in [0, agents), target >= 0, no unknown
 *                 flag bits (JOINT_SETTINGS is a joint record's), reserved == 0, every float finite, jitters >= 0, and no body slot and
 *                 no joint slot named twice -- which is what lets the pass run without an ordering rule.  One bad record refuses the
 *                 call with S2AMD_E_INVALID and the old list stands.  Whether a slot is live is the device's to judge (SKIPPED).  The
 *                 list holds across uploads; the `resets` counters go to zero at an upload and when the list is replaced.
 *                 Device trees (s2amd_world_set_tree) and a refit order (s2amd_world_set_refit_order) are the drop-in binding's, where
 *                 a teleport is a tree remove and insert: s2amd_world_set_resets with a non-empty list returns S2AMD_E_STATE while
 *                 either is set, and those two setters return S2AMD_E_STATE while a reset list is set.
 *   Cost          two launches per pass: one lane per record and per agent, then one lane per shape slot and per contact slot, whose
 *                 waves leave at once when nobody was marked.  No float atomics, no sort, no scratch, no memset and no host wait.
 *                 With no list, or with the flags at 0 and no one-shot call, a step enqueues nothing.
 * Not offered: sharded worlds; reset lists or triggers in the caller's device memory; capturing the start state on the device; rotation
 * jitter (sinf and cosf cannot be stated bit for bit); static bodies; mass or type changes; re-observation after the reset; an episode
 * rule flag that mutes a rule in an episode's first step. */
#define S2AMD_MAX_RESET_AGENTS 16384
#define S2AMD_MAX_RESET_BODIES 65536
#define S2AMD_MAX_RESET_JOINTS 65536
#define S2AMD_RESET_DISABLED 1
#define S2AMD_RESET_JOINT_SETTINGS 2
#define S2AMD_RESET_ON_EPISODE_END 1
#define S2AMD_RESET_REPORT_STATES 2
#define S2AMD_RESET_ALL (-1)
typedef struct s2amdResetBody /* 64 bytes */
{
	int32_t agent;	/* [0, agents) */
	int32_t body;	/* the body slot */
	int32_t flags;	/* S2AMD_RESET_DISABLED */
	float position[2]; /* the centre of mass, as s2amdBody.position */
	float rot[2];	   /* {s, c} */
	float linearVelocity[2];
	float angularVelocity;
	float positionJitter[2], velocityJitter[2], angularJitter; /* >= 0 */
	int32_t reserved; /* 0 */
} s2amdResetBody;
typedef struct s2amdResetJoint /* 32 bytes */
{
	int32_t agent;	/* [0, agents) */
	int32_t joint;	/* the joint slot */
	int32_t flags;	/* S2AMD_RESET_DISABLED | S2AMD_RESET_JOINT_SETTINGS */
	int32_t enableMotor, enableLimit; /* revolute, with JOINT_SETTINGS */
	float motorSpeed;				  /* revolute, with JOINT_SETTINGS */
	float targetA[2];				  /* mouse, with JOINT_SETTINGS */
} s2amdResetJoint;
typedef struct s2amdResetState /* 16 bytes */
{
	int32_t resets;	   /* passes that reset this agent since the list was set and since the last upload */
	int32_t triggered; /* 1: the last pass reset it */
	int32_t pad[2];
} s2amdResetState;
int s2amd_world_set_resets(s2amdSolver* solver, const s2amdResetBody* bodies, int32_t bodyCount, const s2amdResetJoint* joints, int32_t jointCount, int32_t agents, uint32_t seed); /* replaces everything; agents 0 clears */
int s2amd_world_set_reset_report(s2amdSolver* solver, int32_t flags); /* S2AMD_RESET_ON_EPISODE_END | S2AMD_RESET_REPORT_STATES */
int s2amd_world_reset_agents(s2amdSolver* solver, const int32_t* agents, int32_t count); /* the pass between steps; NULL with S2AMD_RESET_ALL: every agent */
int s2amd_world_reset_states(s2amdSolver* solver, s2amdResetState* out, int32_t capacity, int32_t* count); /* one record per agent, with S2AMD_RESET_REPORT_STATES */
int s2amd_world_reset_counts(s2amdSolver* solver, int32_t counts[8]); /* of the last pass, either mode */

/* ---- constraint-graph structure on the device (the reference has neither islands nor colours) ----
 * Islands: connected components over the movable bodies (invMass != 0 or invI != 0) joined by active contacts
 * (pointCount > 0) and revolute joints; every other live non-static body is an island of its own; static and free
 * bodies get -1.  Islands are numbered by their lowest body index.  == solver2d_amd/islands.py: find_islands. */
int s2amd_find_islands(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdContact* contacts, int32_t contactCapacity,
					   const s2amdJoint* joints, int32_t jointCapacity, int32_t* islandOfBody, int32_t* islandCount);
/* A proper colouring of the active contacts: no two contacts of one colour share a movable body, so one colour is one
 * race-free parallel batch of a Gauss-Seidel sweep.  Deterministic: the greedy colouring in descending order of the
 * fixed priority hash fmix32(contact index).  colorOfContact[c] = -1 for inactive slots.  *rounds: Jones-Plassmann
 * rounds the device needed. */
int s2amd_color_constraints(s2amdSolver* solver, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdContact* contacts, int32_t contactCapacity,
							int32_t* colorOfContact, int32_t* colorCount, int32_t* rounds);

/* Multi-GPU exchange: writes one {position.x, position.y, rot.s, rot.c} record per body slot into
 * a DEVICE buffer owned by the caller (e.g. the send buffer of an RCCL all-gather of per-island
 * body arrays).  Returns after the copy has completed on the solver's stream. */
int s2amd_export_poses(s2amdSolver* solver, void* devicePoses, int32_t capacity);
/* The same copy, enqueued behind the steps already enqueued on the solver's stream (see "async") and followed by an event
 * in `slot` (0..3); s2amd_export_wait blocks the host until that event has fired.  Lets a host enqueue step s+1 before it
 * waits for the poses of step s and hands them to the collective: the device never idles between steps. */
int s2amd_export_poses_async(s2amdSolver* solver, void* devicePoses, int32_t capacity, int32_t slot);
/* (API 2) ... the per-island body arrays of a sharded world (28 bytes per body): TWO 16-byte records per body slot,
 * {position.x, position.y, rot.s, rot.c} and {linearVelocity.x, linearVelocity.y, angularVelocity, 0}; capacity in bodies. */
int s2amd_export_bodies_async(s2amdSolver* solver, void* deviceRecords, int32_t capacity, int32_t slot);
int s2amd_export_wait(s2amdSolver* solver, int32_t slot);

/* Device buffers for callers that have no device allocator of their own (a host language behind cgo / JNI / ctypes): the
 * destination of s2amd_export_poses, the source of s2amd_device_read and the destination of s2amd_device_write.  Owned by the caller, freed with
 * s2amd_device_free (or never: s2amd_destroy does not track them). */
int s2amd_device_alloc(s2amdSolver* solver, uint64_t bytes, void** devicePtr);
int s2amd_device_free(s2amdSolver* solver, void* devicePtr);
/* Copies `bytes` from device memory to host memory behind everything enqueued on the solver's stream; returns when done. */
int s2amd_device_read(s2amdSolver* solver, void* hostDst, const void* deviceSrc, uint64_t bytes);
/* (API 5) The mirror: copies `bytes` from host memory to device memory behind everything enqueued on the solver's stream; returns when
 * done, so the caller may reuse hostSrc.  How a caller without a device allocator fills the source of s2amd_world_import_actions. */
int s2amd_device_write(s2amdSolver* solver, void* deviceDst, const void* hostSrc, uint64_t bytes);

/* ---- introspection (tests, bench) ---- */
/* Execution order of the last step: order[k] = contact-array index of the k-th constraint in
 * sweep order; colorOffsets[c]..colorOffsets[c+1] delimit colour batch c.  A sequential
 * Gauss-Seidel sweep in this order is arithmetic-identical to the batched device sweep.  (s2Solve_Jacobi's contact pass
 * writes no body and needs no colours: there only the order -- the order of the per-body sums -- is meaningful.) */
int s2amd_get_contact_order(s2amdSolver* solver, int32_t* order, int32_t orderCapacity, int32_t* colorOffsets,
							int32_t colorCapacity, int32_t* constraintCount, int32_t* colorCount);
int s2amd_get_joint_order(s2amdSolver* solver, int32_t* order, int32_t orderCapacity, int32_t* colorOffsets,
						  int32_t colorCapacity, int32_t* jointCount, int32_t* colorCount);
/* (API 5) writable[b] = 1: the sweeps the contact order above was coloured for write body b -- no two constraints of one colour share
 * such a body (the check a caller can make of an order it is handed).  *solverClass: 0 the velocity sweeps (bodies with mass), 1 the
 * position sweeps of PGS_NGS / PGS_NGS_Block / TGS_NGS, which also rewrite the rotation of immovable bodies (src/solve_common.c:383-392:
 * only a static body whose rotation that normalisation leaves alone is read-only there). */
int s2amd_get_writable_bodies(s2amdSolver* solver, uint8_t* writable, int32_t bodyCapacity, int32_t* solverClass);
int s2amd_get_stats(s2amdSolver* solver, s2amdStepStats* stats);
/* (API 3) Which strip -- which workgroup of the persistent step kernel -- owns each body in the structure in use, and which bodies the
 * seam between strips i and i + 1 carries: ownerStrip[body] = strip or -1 (a static body, a body of an LDS group or of the global part;
 * every entry -1 when the structure has no strips or keeps no picture of them), onSeam[body] = i when the seam i | i + 1 exchanges the
 * body every sweep, else -1.  Either array may be NULL; capacity = entries each can hold (>= the body capacity of the world).
 * *stripCount = number of strips.  Tests use it to build contacts whose place in the structure they know. */
int s2amd_get_strip_owners(s2amdSolver* solver, int32_t* ownerStrip, int32_t* onSeam, int32_t capacity, int32_t* stripCount);
/* (additive, API 5) Which kernel swept the resident islands -- the LDS groups of small islands a soft solver keeps in registers for the
 * whole step -- in the last step, and in which variant: *rounds = 6 or 8, the colour rounds per lane the variant holds (0 with kernel 0).
 * Either pointer may be NULL.  Nothing about the results depends on it: tests use it to know which code they compared. */
#define S2AMD_RESIDENT_NONE 0             /* the last step had no resident islands */
#define S2AMD_RESIDENT_INTERPRETER 1      /* the group interpreter (group_kernel.hip), e.g. beside a persistent strip launch */
#define S2AMD_RESIDENT_ISLAND 2           /* islandStepKernel (strip_kernel.hip): any soft kind; option "wide" = 0 */
#define S2AMD_RESIDENT_WIDE 3             /* the 512-thread island kernel (wide_kernel.hip) between the body prologue and epilogue */
#define S2AMD_RESIDENT_WIDE_ONLY_LAUNCH 4 /* ... as the step's only launch (a world of resident islands only) */
int s2amd_get_resident_kernel(s2amdSolver* solver, int32_t* kernel, int32_t* rounds);
/* (additive, API 5) The variant census.  The register-resident soft kernels exist in many instantiations, kept in one table per kernel
 * family; a step's launcher looks the instantiation for its input up by a key of small integers (the template arguments).  These calls
 * enumerate the tables -- s2amd_variant_family_count() families; per family the kernel template's name, the names of the key's fields
 * (comma separated, in the key's order), the key length and the number of entries; per entry its key -- and report per entry how often a
 * launcher SELECTED it in this process, over all solvers.  That counts what the host enqueued or captured: a step replayed from its
 * captured hipGraph executes the kernel again without selecting it again, and is not counted.  Counters never reset: take differences.
 * The strings live as long as the library.  Any out pointer may be NULL.  No solver is needed, and nothing about a result depends on it:
 * tests use it to know which code they compared.  A launcher that finds NO entry for its key fails the step with S2AMD_E_STATE and
 * names family and key in s2amd_last_error(); it launches nothing. */
int s2amd_variant_family_count(void);
int s2amd_get_variant_family(int32_t family, const char** kernel, const char** keyFields, int32_t* keyLength, int32_t* entryCount);
int s2amd_get_variant_entry(int32_t family, int32_t entry, int32_t* key, int32_t keyCapacity, uint64_t* selections);
/* Live timing of the dominant kernel on the solver's own stream: the first contact solve sweep of
 * the step plan (all its colour-batch launches) is enqueued `repeats` times back to back in one
 * hipGraph and bracketed by a HIP event pair; *usPerLaunch = elapsed / launches, i.e. the time one
 * launch occupies in steady state (kernel + dependent-kernel boundary).  When every constraint lives
 * in an LDS group the whole-step group kernel is timed instead (launchesPerSweep = 1).  The resident
 * world is advanced by the extra sweeps: call it after the timed region. */
int s2amd_measure_dominant(s2amdSolver* solver, const s2amdStepParams* params, int32_t repeats, float* usPerLaunch,
						   int32_t* launchesPerSweep, int32_t* constraintsPerLaunch);
/* option keys: "graph" (0/1 hipGraph replay), "profile" (0/1 per-sweep HIP events),
 * "groups" (0/1 LDS group path for small islands), "message" (0/1 message-passing sweeps), "max_group_bodies", "pack_group_bodies",
 * "strips" (0/1 cut islands that fit no LDS group into strips of BFS levels: two launches per sweep), "strip_bodies" (target
 * bodies per strip, default 8 = strips of two BFS levels), "near_handoff" (0/1, default 1: hand-offs between workgroups the per-launch census finds on one XCD stay in its L2), "strip_retry" (0/1 rebuild the partition with other strip widths when the persistent kernel cannot take this one or it needs more than five interior colour rounds), "strip_min_bodies" (loose bodies below which the colour-batch path is kept), "strip_patience" (steps the constraint graph must
 * stay unchanged before the strip structure is built: its host build costs ~3 ms at 60k constraints, the colour-batch one ~1 ms), "async" (0/1, see s2amd_synchronize), "strip_lean" (0/1 dedicated strip
 * kernel for the soft sweeps), "persist" (0/1 whole step of the strips in one persistent launch), "wide" (0/1 the persistent launch of TGS_Soft, SoftStep and PGS_Soft runs 512 threads per strip, and their resident islands run on the 512-thread island kernel: wide_kernel.hip; 0 = the 256-thread kernels of strip_kernel.hip),
 * "generic" (0/1 every other Gauss-Seidel solver, and any big island with joints, runs its whole step as one launch of the op interpreter over the
 * same strips: generic_kernel.hip; 0 = colour batches for them), "persist_retry" (steps a solver whose persistent launch lost a hand-off stays on the
 * fallback path before the one-launch kernels get another chance -- the wait doubles with every further time-out; default 256, 0 = for ever),
 * "stage_joints" (0/1 the op interpreter keeps a strip's joint records in LDS for the whole step when they fit),
 * "step_readback" (0/1 s2amd_world_step of a world with a refit order brings the poses and the re-inflated boxes along in its own synchronisation: s2amd_world_download_step then
 * costs a host copy),
 * "free_body_groups" (0/1 bodies without any constraint form LDS groups of their own next to groups / strips instead of riding the global path's body launches),
 * "self_contained" (0/1 a world of resident islands only is stepped by their kernel alone: it stages its bodies from the wire records and writes them back),
 * "pair_lanes" (0/1 that launch solves a constraint with two lanes, one per body: pair_kernel.hip; measured no faster, off by default), "body_warm", "incremental" (0/1 created
 * contacts are placed into the existing structure when they fit; 0 = every created contact rebuilds it), "defer" (0/1 a created
 * contact that cannot be placed and has no manifold points yet is only watched until it gets its first points; 0 = it rebuilds the
 * structure when it is created), "island_resident" (0/1 small islands under the soft contact solvers keep their constraints in
 * registers for the whole step: one read of every record per step -- TGS_Soft, PGS_Soft and, up to six colour rounds, SoftStep on the
 * 512-thread island kernel, which is the step's only launch in a world of such islands only; 0 = the group interpreter;
 * s2amd_get_resident_kernel tells which one ran).  None of them changes a result beyond the sweep order the
 * library reports. */
int s2amd_set_option(s2amdSolver* solver, const char* key, int32_t value);

/* ---- (API 4) island-sharded worlds: ONE process, N devices (csrc/sharded.hip) ----
 * A world whose constraint graph falls into islands -- connected components over the movable bodies, as s2amd_find_islands labels them --
 * is partitioned over `deviceCount` shards, one s2amdSolver each on the HIP device named for it (the same ordinal may be named more
 * than once: logical shards on one GPU).  Islands share no movable body, so a step needs no collective: every shard runs the whole
 * s2Solve_* of its islands; the step's ONE exchange carries each shard's owned body records -- {position, rot}, {linearVelocity,
 * angularVelocity, 0}: 28 bytes per body in two 16-byte records -- into every device's copy of the WHOLE world's body records, on a
 * stream of its own per shard (the next step's solve does not wait for it).  How it travels is chosen at s2amd_sharded_create: ONE
 * kernel per shard storing into every copy when the shards share a device; ONE ncclAllGather per device plus a scatter kernel between
 * distinct devices (RCCL over xGMI, single process: librccl.so is looked up at run time and the library loads without it); peer
 * copies otherwise (S2AMD_SHARDED_EXCHANGE=stores|rccl|copies overrides).  The multi-PROCESS form of the same partition (one rank per
 * GPU, torch.distributed over RCCL) is solver2d_amd/distributed.py.
 *   s2amd_sharded_upload    islands found on the device, bin-packed by constraint count (2 per contact constraint + 1 per joint; longest
 *                           processing time first, ties by index: deterministic), every shard's sub-world uploaded -- its islands'
 *                           bodies and constraints in pool order, immovable bodies they touch as read-only replicas;
 *   s2amd_sharded_step      == s2Solve_<solverType> of the whole world, results resident on the shards' devices, + the exchange
 *                           (== s2amd_sharded_step_async + s2amd_sharded_wait);
 *   s2amd_sharded_step_async  (API 5) the same, enqueued only: O(shards) stream operations, no host wait;
 *   s2amd_sharded_wait      (API 5) the one host wait (one stream, which takes every shard's last event).  A shard whose persistent
 *                           launch lost a hand-off is noticed here: with ONE step outstanding its step is repeated and its rows exchanged
 *                           again; with more, the steps behind the failing one were dropped on that shard only, the call fails and the
 *                           world must be uploaded again.  Download, read_bodies, reshard and upload wait by themselves;
 *   s2amd_sharded_download  the world's arrays on the host, every body and constraint from the shard that owns it; constraintIndex as
 *                           the reference's gather loop over the whole pool writes it;
 *   s2amd_sharded_read_bodies  float[bodyCapacity][8] of the world's body records as of the last exchange, read from `shard`'s device;
 *   s2amd_sharded_reshard   the constraint graph changed (contacts / joints: the world's new arrays, pool capacities unchanged, or NULL
 *                           for "unchanged"): solver state comes down, a slot that kept its pair keeps its impulses, islands are found
 *                           again, an island stays on the shard that owned most of its bodies (ties: the lowest shard) -- a contact
 *                           created between two islands moves the smaller one --, islands nobody owned go to the least loaded shard,
 *                           and past 1.75 x the mean load the heaviest shard gives up its lightest islands;
 *   s2amd_sharded_solver    the s2amdSolver of a shard, for the queries of this header (orders, stats, options); owned by the sharded solver. */
typedef struct s2amdShardedSolver s2amdShardedSolver;
int s2amd_sharded_create(const int32_t* devices, int32_t deviceCount, s2amdShardedSolver** out);
void s2amd_sharded_destroy(s2amdShardedSolver* sharded);
int s2amd_sharded_shard_count(const s2amdShardedSolver* sharded);
s2amdSolver* s2amd_sharded_solver(s2amdShardedSolver* sharded, int32_t shard);
int s2amd_sharded_upload(s2amdShardedSolver* sharded, const s2amdBody* bodies, int32_t bodyCapacity, const s2amdContact* contacts, int32_t contactCapacity,
						 const s2amdJoint* joints, int32_t jointCapacity);
int s2amd_sharded_step(s2amdShardedSolver* sharded, const s2amdStepParams* params);
int s2amd_sharded_step_async(s2amdShardedSolver* sharded, const s2amdStepParams* params);
int s2amd_sharded_wait(s2amdShardedSolver* sharded);
/* what the last s2amd_sharded_step_async enqueued, counted where it is enqueued: stream operations (launches, copies, collectives,
 * event records and waits), host waits since (s2amd_sharded_wait: 1), and the form of the exchange (0 stores, 1 rccl, 2 peer copies) */
int s2amd_sharded_get_step_ops(s2amdShardedSolver* sharded, int32_t* streamOps, int32_t* hostWaits, int32_t* exchange);
/* the same count for `shards` shards in the given form, by the code that enqueues a step, enqueueing nothing (no device needed) */
int s2amd_sharded_count_ops(int32_t shards, int32_t exchange, int32_t* streamOps);
int s2amd_sharded_download(s2amdShardedSolver* sharded, s2amdBody* bodies, int32_t bodyCapacity, s2amdContact* contacts, int32_t contactCapacity,
						   s2amdJoint* joints, int32_t jointCapacity);
int s2amd_sharded_read_bodies(s2amdShardedSolver* sharded, int32_t shard, float* records, int32_t bodyCapacity);
int s2amd_sharded_reshard(s2amdShardedSolver* sharded, const s2amdContact* contacts, int32_t contactCapacity, const s2amdJoint* joints, int32_t jointCapacity);
/* shardOfBody[b]: the shard that owns body b (-1: static or free -- replicated, owned by nobody); may be NULL */
int s2amd_sharded_get_partition(s2amdShardedSolver* sharded, int32_t* shardOfBody, int32_t capacity, int32_t* islandCount, int32_t* reshards);

#ifdef __cplusplus
}
#endif

#endif /* SOLVER2D_AMD_H */
