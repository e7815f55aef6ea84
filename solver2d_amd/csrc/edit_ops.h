// The body setters' arithmetic (s2Body_SetLinearVelocity, _SetAngularVelocity, _ApplyForceToCenter, _ApplyLinearImpulse,
// src/body.c:337-370) and the joint setters' (s2MouseJoint_SetTarget, src/mouse_joint.c:18-29; s2RevoluteJoint_EnableLimit, _EnableMotor,
// _SetMotorSpeed, src/revolute_joint.c:890-927) on a wire record whose edited fields a lane keeps in registers: what s2amd_world_edit
// (world_edit.hip), the force fields (force_field.hip) and the actuators (actuators.hip) share, so that a field's or an actuator's term
// IS the edit of the same name.  Everything is in an unnamed namespace: each file holds its own copy.
#pragma once

#include "solver_internal.h"

namespace
{

static_assert(sizeof(s2amdWorldEdit) == 32, "the edit record");
static_assert(sizeof(s2amdBody) == 88, "the wire record");

// which fields of a body record an edit (or a walk) has written
#define S2_EDIT_W_LINEAR 1
#define S2_EDIT_W_ANGULAR 2
#define S2_EDIT_W_FORCE 4

// what the body kinds read and never write ...
struct BodyFixed
{
	int type;
	float invMass, invI, px, py;
};

// ... and what they write
struct BodyFields
{
	float vx, vy, w, fx, fy;
	int written;
};

__device__ inline void loadBody(const s2amdBody* b, BodyFixed& k, BodyFields& f)
{
	k.type = b->type;
	k.invMass = b->invMass, k.invI = b->invI;
	k.px = b->position[0], k.py = b->position[1];
	f.vx = b->linearVelocity[0], f.vy = b->linearVelocity[1];
	f.w = b->angularVelocity;
	f.fx = b->force[0], f.fy = b->force[1];
	f.written = 0;
}

__device__ inline void storeBody(s2amdBody* b, const BodyFields& f)
{
	if ((f.written & S2_EDIT_W_LINEAR) != 0)
	{
		b->linearVelocity[0] = f.vx, b->linearVelocity[1] = f.vy;
	}
	if ((f.written & S2_EDIT_W_ANGULAR) != 0)
	{
		b->angularVelocity = f.w;
	}
	if ((f.written & S2_EDIT_W_FORCE) != 0)
	{
		b->force[0] = f.fx, b->force[1] = f.fy;
	}
}

// one body edit on a live slot (kinds 1-4); the reference's statements, in its order
__device__ inline void applyBodyEdit(const s2amdWorldEdit& e, const BodyFixed& k, BodyFields& f)
{
	if (e.kind == S2AMD_EDIT_BODY_SET_LINEAR_VELOCITY)
	{
		f.vx = e.v[0], f.vy = e.v[1]; // body.c:341
		f.written |= S2_EDIT_W_LINEAR;
	}
	else if (e.kind == S2AMD_EDIT_BODY_SET_ANGULAR_VELOCITY)
	{
		f.w = e.v[0]; // body.c:349
		f.written |= S2_EDIT_W_ANGULAR;
	}
	else if (e.kind == S2AMD_EDIT_BODY_APPLY_FORCE_TO_CENTER)
	{
		f.fx = f.fx + e.v[0], f.fy = f.fy + e.v[1]; // body.c:356: s2Add(body->force, force)
		f.written |= S2_EDIT_W_FORCE;
	}
	else if (k.type == S2AMD_BODY_DYNAMIC) // S2AMD_EDIT_BODY_APPLY_LINEAR_IMPULSE; body.c:363-366: any other type returns
	{
		// body.c:368: s2MulAdd(v, invMass, impulse) = {v.x + invMass * impulse.x, v.y + invMass * impulse.y}
		f.vx = f.vx + k.invMass * e.v[0];
		f.vy = f.vy + k.invMass * e.v[1];
		// body.c:369: w += invI * s2Cross(s2Sub(point, position), impulse)
		const float rx = e.v[2] - k.px, ry = e.v[3] - k.py;
		f.w = f.w + k.invI * (rx * e.v[1] - ry * e.v[0]);
		f.written |= S2_EDIT_W_LINEAR | S2_EDIT_W_ANGULAR;
	}
}

// ---- the joint half: kinds 5-8 ----
static_assert(sizeof(s2amdJoint) == 92, "the wire record");

#define S2_EDIT_FIRST_JOINT_KIND S2AMD_EDIT_MOUSE_SET_TARGET

// which fields of a joint record an edit (or a walk) has written
#define S2_EDIT_W_MOTOR 1
#define S2_EDIT_W_LIMIT 2
#define S2_EDIT_W_SPEED 4
#define S2_EDIT_W_TARGET 8

struct JointFields
{
	int enableMotor, enableLimit;
	float motorSpeed, tx, ty;
	int written;
};

__device__ inline s2amdWorldEdit loadEdit(const s2amdWorldEdit* edits, size_t i)
{
	// (32 bytes, 32-byte aligned: two 16-byte loads)
	const int4 a = ((const int4*)edits)[2 * i];
	const float4 b = ((const float4*)edits)[2 * i + 1];
	s2amdWorldEdit e;
	e.kind = a.x, e.target = a.y, e.flag = a.z, e.reserved = a.w;
	e.v[0] = b.x, e.v[1] = b.y, e.v[2] = b.z, e.v[3] = b.w;
	return e;
}

__device__ inline void loadJoint(const s2amdJoint* j, JointFields& f)
{
	f.enableMotor = j->enableMotor, f.enableLimit = j->enableLimit;
	f.motorSpeed = j->motorSpeed;
	f.tx = j->targetA[0], f.ty = j->targetA[1];
	f.written = 0;
}

__device__ inline void storeJoint(s2amdJoint* j, const JointFields& f)
{
	if ((f.written & S2_EDIT_W_MOTOR) != 0)
	{
		j->enableMotor = f.enableMotor;
	}
	if ((f.written & S2_EDIT_W_LIMIT) != 0)
	{
		j->enableLimit = f.enableLimit;
	}
	if ((f.written & S2_EDIT_W_SPEED) != 0)
	{
		j->motorSpeed = f.motorSpeed;
	}
	if ((f.written & S2_EDIT_W_TARGET) != 0)
	{
		j->targetA[0] = f.tx, j->targetA[1] = f.ty;
	}
}

// one joint edit (kinds 5-8) on a slot of type `type`; false: the joint is free or of the other type, nothing is written
__device__ inline bool applyJointEdit(const s2amdWorldEdit& e, int type, JointFields& f)
{
	if (e.kind == S2AMD_EDIT_MOUSE_SET_TARGET)
	{
		if (type != S2AMD_JOINT_MOUSE)
		{
			return false;
		}
		f.tx = e.v[0], f.ty = e.v[1]; // mouse_joint.c:28
		f.written |= S2_EDIT_W_TARGET;
		return true;
	}
	if (type != S2AMD_JOINT_REVOLUTE)
	{
		return false;
	}
	if (e.kind == S2AMD_EDIT_REVOLUTE_ENABLE_LIMIT)
	{
		f.enableLimit = e.flag != 0 ? 1 : 0; // revolute_joint.c:900
		f.written |= S2_EDIT_W_LIMIT;
	}
	else if (e.kind == S2AMD_EDIT_REVOLUTE_ENABLE_MOTOR)
	{
		f.enableMotor = e.flag != 0 ? 1 : 0; // revolute_joint.c:913
		f.written |= S2_EDIT_W_MOTOR;
	}
	else
	{
		f.motorSpeed = e.v[0]; // revolute_joint.c:926
		f.written |= S2_EDIT_W_SPEED;
	}
	return true;
}

} // namespace
