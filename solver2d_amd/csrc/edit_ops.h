// The body setters' arithmetic (s2Body_SetLinearVelocity, _SetAngularVelocity, _ApplyForceToCenter, _ApplyLinearImpulse,
// src/body.c:337-370) on a wire record whose edited fields a lane keeps in registers: what s2amd_world_edit (world_edit.hip) and the
// force fields (force_field.hip) share, so that a field's term IS the edit of the same name.  Everything is in an unnamed namespace:
// each file holds its own copy.
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

} // namespace
