// What the queries that run s2ShapeDistance against the resident shapes share (proximity_query.hip, shape_cast.hip): the proxy
// s2Shape_MakeDistanceProxy (src/shape.c:75-93) would build of a shape slot, as a lane keeps it, and a proxy whose vertices stay in a
// wire record.  Included after gjk_ops.h (S2_NP_MAX_VERTS, Xf).  Everything is in an unnamed namespace: each file holds its own copy.
#pragma once

#include "gjk_ops.h"
#include "report_common.h"

namespace
{

static_assert(sizeof(s2amdShape) == 196, "the shape record");

// what a lane keeps of its shape slot: the header of s2Shape_MakeDistanceProxy's proxy and the frame
struct LaneProxy
{
	bool live;
	int body, count;
	uint32_t category;
	float radius;
	float fat[4];
	Xf xf;
};

// Slot `slot` (< n).  count: a circle's 1, a capsule's or segment's 2, a polygon's own clamped to 1..8 (s2FindSupport reads vertex 0
// whatever the count); radius: the shape's, a segment's 0.  The vertices stay where they are: vertices[0 .. count) of the wire record.
S2_DEV LaneProxy loadProxy(const s2amdShape* shapes, int slot, const s2amdBody* bodies, const float2* origins, int nb)
{
	LaneProxy s;
	const s2amdShape* w = shapes + slot;
	const int type = w->type;
	s.live = type != S2AMD_SHAPE_FREE;
	s.body = -1, s.count = 1;
	s.category = 0u;
	s.radius = 0.0f;
	s.fat[0] = s.fat[1] = s.fat[2] = s.fat[3] = 0.0f;
	s.xf.p = v2(0.0f, 0.0f);
	s.xf.q.s = 0.0f, s.xf.q.c = 1.0f;
	if (!s.live)
	{
		return s;
	}
	s.body = w->body;
	s.category = w->categoryBits;
	s.radius = type == S2AMD_SHAPE_SEGMENT ? 0.0f : w->radius;
	s.fat[0] = w->fatAABB[0], s.fat[1] = w->fatAABB[1], s.fat[2] = w->fatAABB[2], s.fat[3] = w->fatAABB[3];
	if (type == S2AMD_SHAPE_POLYGON)
	{
		const int count = w->count;
		s.count = count < 1 ? 1 : count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : count;
	}
	else
	{
		s.count = type == S2AMD_SHAPE_CIRCLE ? 1 : 2;
	}
	if (s.body >= 0 && s.body < nb) // (s2amd_world_upload refuses a live shape on a body outside the array)
	{
		const float2 o = origins[s.body];
		s.xf.p = v2(o.x, o.y);
		s.xf.q.s = bodies[s.body].rot[0], s.xf.q.c = bodies[s.body].rot[1];
	}
	return s;
}

// a proxy whose vertices lie in a wire record (4-byte aligned: a shape record is 196 bytes), in LDS or in global memory
struct WireProxy
{
	const float (*verts)[2];
	int count;
	float radius;
	S2_DEV V2 v(int i) const { return v2(verts[i][0], verts[i][1]); }
};

// the proxy of slot `slot` read where the resident array holds it (the finish passes: one lane per answer)
S2_DEV WireProxy slotProxy(const s2amdShape* shapes, int slot, const LaneProxy& s)
{
	WireProxy B;
	B.verts = shapes[slot].vertices, B.count = s.count, B.radius = s.radius;
	return B;
}

} // namespace
