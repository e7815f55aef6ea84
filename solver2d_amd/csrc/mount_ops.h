// What the lists mounted on bodies of the resident world share on the device (sensor_report.hip, force_field.hip, ray_report.hip,
// grid_report.hip): the mount rule -- whether an entry is active and the world frame it stands in -- and the candidate box of an entry
// that is a proxy.  Device functions only, no kernel: including this adds nothing to a translation unit.  The candidate rules (which
// shapes an entry takes) differ per list and stay in their files.  The including file defines S2_NP_BLOCK and S2_NP_MAX_VERTS first, as
// gjk_ops.h asks (Xf, xfPoint).  What needs no frame -- boxesOverlap, liveBody, clampedAffine -- is in report_common.h, which
// actuators.hip and observers.hip see too.
//
// How the two functions take their arguments is part of "the kernels stay as they were, instruction for instruction": the mount rule
// reads the entry's fields itself, and the box reads radius and reach where it uses them.  Handed over by value, the compiler knows the
// values defined and loads them early, and the pose kernels come out scheduled differently.
#pragma once

#include "gjk_ops.h"
#include "report_common.h"

namespace
{

// no exponent bits all set: neither a NaN nor an infinity
S2_DEV bool finiteBits(float f)
{
	return (asBits(f) & 0x7f800000u) != 0x7f800000u;
}

S2_DEV Xf frameOf(const float* position, const float* rot)
{
	Xf xf;
	xf.p = v2(position[0], position[1]);
	xf.q.s = rot[0], xf.q.c = rot[1];
	return xf;
}

// the frame of an entry that is not active: all zero (not the identity), so that its state says so in every field
S2_DEV Xf noFrame()
{
	Xf xf;
	xf.p = v2(0.0f, 0.0f);
	xf.q.s = 0.0f, xf.q.c = 0.0f;
	return xf;
}

// The mount rule of entry q (a record with position, rot, body and flags).  The entry is active unless its `disabledFlag` is set or it
// is mounted (body >= 0) on what is no live body of the array; xf is {position, rot} for an entry fixed in the world and
// s2MulTransforms(xf(body), {position, rot}) for a mounted one, in the reference's operation order: include/solver2d/math.h:368-374;
// s2MulRot :291-300.  An entry that is not active reports noFrame(): the caller sets it once it knows, as the grids know only after
// their corners.
template <typename Entry> S2_DEV bool mountFrame(const Entry* q, int disabledFlag, const s2amdBody* bodies, const float2* origins, int nb, Xf& xf)
{
	const int body = q->body, flags = q->flags;
	bool active = (flags & disabledFlag) == 0;
	xf.p = v2(q->position[0], q->position[1]);
	xf.q.s = q->rot[0], xf.q.c = q->rot[1];
	if (active && body >= 0)
	{
		active = liveBody(bodies, nb, body);
		if (active)
		{
			const float2 o = origins[body];
			const float bs = bodies[body].rot[0], bc = bodies[body].rot[1];
			const float s = bs * xf.q.c + bc * xf.q.s;
			const float c = bc * xf.q.c - bs * xf.q.s;
			const float px = (bc * xf.p.x - bs * xf.p.y) + o.x;
			const float py = (bs * xf.p.x + bc * xf.p.y) + o.y;
			xf.p = v2(px, py);
			xf.q.s = s, xf.q.c = c;
		}
	}
	return active;
}

// the candidate box of a proxy in frame xf: the proximity queries' query box with maxDistance = *reach, over vertices[0 .. count)
S2_DEV float4 mountBox(Xf xf, const float (*vertices)[2], int count, const float* radius, const float* reach)
{
	V2 lower = xfPoint(xf, v2(vertices[0][0], vertices[0][1]));
	V2 upper = lower;
	for (int k = 1; k < count; ++k)
	{
		const V2 w = xfPoint(xf, v2(vertices[k][0], vertices[k][1]));
		lower = v2(S2_MINF(lower.x, w.x), S2_MINF(lower.y, w.y));
		upper = v2(S2_MAXF(upper.x, w.x), S2_MAXF(upper.y, w.y));
	}
	const float r = *radius + *reach;
	return make_float4(lower.x - r, lower.y - r, upper.x + r, upper.y + r);
}

} // namespace
