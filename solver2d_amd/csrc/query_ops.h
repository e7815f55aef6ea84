// The exact per-shape tests of the scene queries (scene_query.hip), restated operation for operation from the reference's
// src/geometry.c: s2PointInCircle :343-347, s2PointInCapsule :349-374, s2PointInPolygon :376-389 (GJK: gjk_ops.h), s2RayCastCircle
// :393-448, s2RayCastCapsule :450-581, s2RayCastSegment :584-654, s2RayCastPolygon :656-730.  Inputs are in the shape's body frame.
// s2RayCastOutput.point is not computed: the queries report the point on the world-space ray (include/solver2d_amd.h).
// The including file defines S2_NP_BLOCK (the stride of its LDS polygons) first, as gjk_ops.h asks.
#pragma once

#include "gjk_ops.h"

namespace
{

struct RayIn
{
	V2 p1, p2;
	float maxFraction;
};

struct RayOut
{
	V2 normal;
	float fraction;
	bool hit;
};

S2_DEV RayOut rayMiss()
{
	RayOut o;
	o.normal = v2(0.0f, 0.0f);
	o.fraction = 0.0f;
	o.hit = false;
	return o;
}

S2_DEV float distanceSquared(V2 a, V2 b) // math.h:188-192
{
	const float cx = b.x - a.x, cy = b.y - a.y;
	return cx * cx + cy * cy;
}

S2_DEV bool pointInCircle(V2 point, V2 center, float radius) // :343-347
{
	return distanceSquared(point, center) <= radius * radius;
}

S2_DEV bool pointInCapsule(V2 point, V2 p1, V2 p2, float radius) // :349-374
{
	const float rr = radius * radius;
	const V2 d = sub(p2, p1);
	const float dd = dot(d, d);
	if (dd == 0.0f)
	{
		return distanceSquared(point, p1) <= rr;
	}
	float t = dot(sub(point, p1), d) / dd;
	t = S2_CLAMPF(t, 0.0f, 1.0f);
	const V2 c = mulAdd(p1, t, d);
	return distanceSquared(point, c) <= rr;
}

// :376-389: proxy A the polygon's vertices without its radius, proxy B the point, identity transforms, an empty cache
S2_DEV bool pointInPolygon(const PolyRef& polygon, const PolyRef& point)
{
	Cache cache;
	cache.metric = 0.0f;
	cache.count = 0;
	cache.indexA[0] = cache.indexA[1] = cache.indexA[2] = 0;
	cache.indexB[0] = cache.indexB[1] = cache.indexB[2] = 0;
	const DistanceOutput out = shapeDistance(cache, polygon, point);
	return out.distance <= polygon.radius;
}

S2_DEV RayOut rayCastCircle(const RayIn& in, V2 p, float radius) // :393-448
{
	RayOut output = rayMiss();
	const V2 s = sub(in.p1, p);
	float len;
	const V2 d = lengthAndNormalize(&len, sub(in.p2, in.p1));
	if (len == 0.0f)
	{
		return output;
	}
	const float t = -dot(s, d);
	const V2 c = mulAdd(s, t, d);
	const float cc = dot(c, c);
	const float rr = radius * radius;
	if (cc > rr)
	{
		return output;
	}
	const float h = sqrtf(rr - cc);
	const float fraction = t - h;
	if (fraction < 0.0f || in.maxFraction * len < fraction)
	{
		return output;
	}
	const V2 hitPoint = mulAdd(s, fraction, d);
	output.fraction = fraction / len;
	output.normal = normalize(hitPoint);
	output.hit = true;
	return output;
}

S2_DEV RayOut rayCastCapsule(const RayIn& in, V2 v1, V2 vEnd, float radius) // :450-581
{
	RayOut output = rayMiss();
	const V2 e = sub(vEnd, v1);
	float capsuleLength;
	const V2 a = lengthAndNormalize(&capsuleLength, e);
	if (capsuleLength < FLT_EPSILON)
	{
		return rayCastCircle(in, v1, radius);
	}
	const V2 p1 = in.p1, p2 = in.p2;
	const V2 q = sub(p1, v1);
	const float qa = dot(q, a);
	const V2 qp = mulAdd(q, -qa, a);
	if (dot(qp, qp) < radius * radius)
	{
		if (qa < 0.0f)
		{
			return rayCastCircle(in, v1, radius);
		}
		if (qa > 1.0f)
		{
			return rayCastCircle(in, vEnd, radius);
		}
		return output;
	}
	V2 n = v2(a.y, -a.x);
	float rayLength;
	const V2 u = lengthAndNormalize(&rayLength, sub(p2, p1));
	const float den = -a.x * u.y + u.x * a.y;
	if (-FLT_EPSILON < den && den < FLT_EPSILON)
	{
		return output;
	}
	const V2 b1 = mulSub(q, radius, n);
	const V2 bz2 = mulAdd(q, radius, n);
	const float invDen = 1.0f / den;
	const float s21 = (a.x * b1.y - b1.x * a.y) * invDen;
	const float s22 = (a.x * bz2.y - bz2.x * a.y) * invDen;
	float s2;
	V2 b;
	if (s21 < s22)
	{
		s2 = s21;
		b = b1;
	}
	else
	{
		s2 = s22;
		b = bz2;
		n = neg(n);
	}
	if (s2 < 0.0f || in.maxFraction * rayLength < s2)
	{
		return output;
	}
	const float s1 = (-b.x * u.y + u.x * b.y) * invDen;
	if (s1 < 0.0f)
	{
		return rayCastCircle(in, v1, radius);
	}
	else if (capsuleLength < s1)
	{
		return rayCastCircle(in, vEnd, radius);
	}
	output.fraction = s2 / rayLength;
	output.normal = n;
	output.hit = true;
	return output;
}

S2_DEV RayOut rayCastSegment(const RayIn& in, V2 v1, V2 vEnd) // :584-654
{
	RayOut output = rayMiss();
	const V2 p1 = in.p1, p2 = in.p2;
	const V2 d = sub(p2, p1);
	const V2 e = sub(vEnd, v1);
	float len;
	const V2 eUnit = lengthAndNormalize(&len, e);
	if (len == 0.0f)
	{
		return output;
	}
	V2 normal = v2(eUnit.y, -eUnit.x);
	const float numerator = dot(normal, sub(v1, p1));
	const float denominator = dot(normal, d);
	if (denominator == 0.0f)
	{
		return output;
	}
	const float t = numerator / denominator;
	if (t < 0.0f || in.maxFraction < t)
	{
		return output;
	}
	const V2 p = mulAdd(p1, t, d);
	const float s = dot(sub(p, v1), eUnit);
	if (s < 0.0f || len < s)
	{
		return output;
	}
	if (numerator > 0.0f)
	{
		normal = neg(normal);
	}
	output.fraction = t;
	output.normal = normal;
	output.hit = true;
	return output;
}

// :656-730 (the polygon's radius takes no part); polygon.count is the caller's clamp to 0..8
S2_DEV RayOut rayCastPolygon(const RayIn& in, const PolyRef& polygon)
{
	RayOut output = rayMiss();
	const V2 p1 = in.p1, p2 = in.p2;
	const V2 d = sub(p2, p1);
	float lower = 0.0f, upper = in.maxFraction;
	int index = -1;
	for (int i = 0; i < polygon.count; ++i)
	{
		const V2 normal = polygon.n(i);
		const float numerator = dot(normal, sub(polygon.v(i), p1));
		const float denominator = dot(normal, d);
		if (denominator == 0.0f)
		{
			if (numerator < 0.0f)
			{
				return output;
			}
		}
		else
		{
			if (denominator < 0.0f && numerator < lower * denominator)
			{
				lower = numerator / denominator;
				index = i;
			}
			else if (denominator > 0.0f && numerator < upper * denominator)
			{
				upper = numerator / denominator;
			}
		}
		if (upper < lower)
		{
			return output;
		}
	}
	if (index >= 0)
	{
		output.fraction = lower;
		output.normal = polygon.n(index);
		output.hit = true;
	}
	return output;
}

} // namespace
