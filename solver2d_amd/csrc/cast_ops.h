// What the calls that sweep a caller's proxy against the resident shapes share (shape_cast.hip, mover_query.hip): the constants of the
// shape casts' statement (include/solver2d_amd.h), the swept box and the conservative advancement C(q, s), every distance of which is
// s2ShapeDistance (gjk_ops.h).  Included after gjk_ops.h and proxy_ops.h (S2_NP_MAX_VERTS, Xf, WireProxy).  Everything is in an unnamed
// namespace: each file holds its own copy.
#pragma once

#include "gjk_ops.h"
#include "proxy_ops.h"

namespace
{

#define S2_CAST_TARGET S2_LINEAR_SLOP
#define S2_CAST_TOLERANCE (0.25f * S2_LINEAR_SLOP)
#define S2_CAST_SPECULATIVE (4.0f * S2_LINEAR_SLOP) // constants.h:8
#define S2_CAST_CAP 20

S2_DEV Rot castRot(const s2amdShapeCast& c)
{
	Rot q;
	q.s = c.rot[0], q.c = c.rot[1];
	return q;
}

// the bounds of the proxy's vertices under xf, folded from vertex 0 in index order
S2_DEV void proxyBounds(const s2amdShapeCast& c, Xf xf, V2* lower, V2* upper)
{
	*lower = xfPoint(xf, v2(c.vertices[0][0], c.vertices[0][1]));
	*upper = *lower;
	for (int i = 1; i < c.count && i < S2_NP_MAX_VERTS; ++i)
	{
		const V2 w = xfPoint(xf, v2(c.vertices[i][0], c.vertices[i][1]));
		*lower = v2(S2_MINF(lower->x, w.x), S2_MINF(lower->y, w.y));
		*upper = v2(S2_MAXF(upper->x, w.x), S2_MAXF(upper->y, w.y));
	}
}

// the swept box (the header's statement): the bounds at fraction 0 and at maxFraction together, grown by radius + s2_speculativeDistance
S2_DEV float4 sweptBox(const s2amdShapeCast& c)
{
	Xf xf;
	xf.q = castRot(c);
	xf.p = v2(c.position[0], c.position[1]);
	V2 lower0, upper0, lower1, upper1;
	proxyBounds(c, xf, &lower0, &upper0);
	xf.p = mulAdd(xf.p, c.maxFraction, v2(c.translation[0], c.translation[1]));
	proxyBounds(c, xf, &lower1, &upper1);
	const V2 lower = v2(S2_MINF(lower0.x, lower1.x), S2_MINF(lower0.y, lower1.y));
	const V2 upper = v2(S2_MAXF(upper0.x, upper1.x), S2_MAXF(upper0.y, upper1.y));
	const float r = c.radius + S2_CAST_SPECULATIVE;
	return make_float4(lower.x - r, lower.y - r, upper.x + r, upper.y + r);
}

// C(q, s) of the header: `hit`, and for a hit t_k, k and D_k
struct CastOutcome
{
	bool hit;
	float fraction;
	int advances;
	ShapeDistanceOutput d;
};

template <class PB>
S2_DEV CastOutcome castAgainst(const s2amdShapeCast* c, const PB& B, Xf xfB)
{
	const float threshold = S2_CAST_TARGET + S2_CAST_TOLERANCE;
	WireProxy A;
	A.verts = c->vertices, A.count = c->count, A.radius = c->radius;
	const V2 position = v2(c->position[0], c->position[1]), translation = v2(c->translation[0], c->translation[1]);
	const float maxFraction = c->maxFraction;
	Xf xfA;
	xfA.q = castRot(*c);
	CastOutcome o;
	o.hit = false;
	o.fraction = 0.0f;
	o.advances = 0;
	for (;;)
	{
		xfA.p = mulAdd(position, o.fraction, translation);
		o.d = shapeDistanceWithRadii(A, xfA, B, xfB);
		if (o.d.distance < threshold || o.advances == S2_CAST_CAP)
		{
			o.hit = true;
			return o;
		}
		const V2 n = normalize(sub(o.d.pointB, o.d.pointA));
		const float approach = dot(translation, n);
		if (approach <= 0.0f)
		{
			return o;
		}
		const float next = o.fraction + (o.d.distance - S2_CAST_TARGET) / approach;
		if (!(next <= maxFraction))
		{
			return o;
		}
		o.fraction = next;
		o.advances += 1;
	}
}

} // namespace
