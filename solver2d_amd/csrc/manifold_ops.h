// The reference's manifold functions (src/manifold.c) as device functions: shared by the narrow phase (narrowphase.hip: stage 3's
// s2UpdateContact) and the contact queries (contact_query.hip: the manifolds of a caller's shape).  Reference map: s2CollideCircles
// :16-49, s2CollideCapsuleAndCircle :51-110, s2CollidePolygonAndCircle :113-222, s2ClipPolygons :248-399, s2FindMaxSeparation :402-438,
// s2PolygonSAT :441-506, s2CollidePolygons :509-650; capsules and segments enter the polygon path through s2MakeCapsule
// (src/geometry.c:100-115) exactly as :224-246 and :652-663 do.  The including file defines S2_NP_BLOCK, S2_NP_MAX_VERTS (gjk_ops.h) and
// S2_NP_SPECULATIVE first.  Everything is in an unnamed namespace: each file holds its own copy.
#pragma once

#include "gjk_ops.h"

#include "solver2d_amd.h"

#include <cfloat>

namespace
{

struct MPoint
{
	V2 localAnchorA, localAnchorB;
	float separation;
	uint32_t id;
};
struct Manifold
{
	MPoint points[2];
	V2 normal;
	int pointCount;
};
S2_DEV Manifold emptyManifold()
{
	Manifold m;
	m.points[0].localAnchorA = m.points[0].localAnchorB = v2(0.0f, 0.0f);
	m.points[1].localAnchorA = m.points[1].localAnchorB = v2(0.0f, 0.0f);
	m.points[0].separation = m.points[1].separation = 0.0f;
	m.points[0].id = m.points[1].id = 0u;
	m.normal = v2(0.0f, 0.0f);
	m.pointCount = 0;
	return m;
}
S2_DEV uint32_t makeId(int a, int b) { return (((uint32_t)a & 0xffu) << 8) | ((uint32_t)b & 0xffu); } // manifold.h:17


// ---- manifold functions (src/manifold.c) ----
S2_DEV Manifold collideCircles(V2 pointA, float radiusA, Xf xfA, V2 pointB0, float radiusB, Xf xfB)
{
	Manifold m = emptyManifold();
	Xf xf = xfInvMul(xfA, xfB);
	V2 pointB = xfPoint(xf, pointB0);
	float dist;
	V2 normal = lengthAndNormalize(&dist, sub(pointB, pointA));
	float separation = dist - radiusA - radiusB;
	if (separation > S2_NP_SPECULATIVE)
	{
		return m;
	}
	V2 cA = mulAdd(pointA, radiusA, normal);
	V2 cB = mulAdd(pointB, -radiusB, normal);
	V2 contactPointA = lerp2(cA, cB, 0.5f);
	m.normal = rotate(xfA.q, normal);
	m.points[0].localAnchorA = contactPointA;
	m.points[0].localAnchorB = xfInvPoint(xf, contactPointA);
	m.points[0].separation = separation;
	m.pointCount = 1;
	return m;
}

S2_DEV Manifold collideCapsuleAndCircle(V2 p1, V2 p2, float radiusA, Xf xfA, V2 pointB0, float radiusB, Xf xfB)
{
	Manifold m = emptyManifold();
	Xf xf = xfInvMul(xfA, xfB);
	V2 pB = xfPoint(xf, pointB0);
	V2 e = sub(p2, p1);
	V2 pA;
	float s1 = dot(sub(pB, p1), e);
	float s2 = dot(sub(p2, pB), e);
	if (s1 < 0.0f)
	{
		pA = p1;
	}
	else if (s2 < 0.0f)
	{
		pA = p2;
	}
	else
	{
		float s = s1 / dot(e, e);
		pA = mulAdd(p1, s, e);
	}
	float dist;
	V2 normal = lengthAndNormalize(&dist, sub(pB, pA));
	float separation = dist - radiusA - radiusB;
	if (separation > S2_NP_SPECULATIVE)
	{
		return m;
	}
	V2 cA = mulAdd(pA, radiusA, normal);
	V2 cB = mulAdd(pB, -radiusB, normal);
	V2 contactPointA = lerp2(cA, cB, 0.5f);
	m.normal = rotate(xfA.q, normal);
	m.points[0].localAnchorA = contactPointA;
	m.points[0].localAnchorB = xfInvPoint(xf, contactPointA);
	m.points[0].separation = separation;
	m.pointCount = 1;
	return m;
}

S2_DEV Manifold collidePolygonAndCircle(const PolyRef& polygonA, Xf xfA, V2 pointB0, float radiusB, Xf xfB)
{
	Manifold m = emptyManifold();
	Xf xf = xfInvMul(xfA, xfB);
	V2 c = xfPoint(xf, pointB0);
	float radiusA = polygonA.radius;
	float radius = radiusA + radiusB;
	int normalIndex = 0;
	float separation = -FLT_MAX;
	int vertexCount = polygonA.count;
	for (int i = 0; i < vertexCount; ++i)
	{
		float s = dot(polygonA.n(i), sub(c, polygonA.v(i)));
		if (s > separation)
		{
			separation = s;
			normalIndex = i;
		}
	}
	if (separation > radius + S2_NP_SPECULATIVE)
	{
		return m;
	}
	int vertIndex1 = normalIndex;
	int vertIndex2 = vertIndex1 + 1 < vertexCount ? vertIndex1 + 1 : 0;
	V2 v1 = polygonA.v(vertIndex1), v2_ = polygonA.v(vertIndex2);
	float u1 = dot(sub(c, v1), sub(v2_, v1));
	float u2 = dot(sub(c, v2_), sub(v1, v2_));
	const bool near1 = u1 < 0.0f && separation > FLT_EPSILON;
	const bool near2 = u2 < 0.0f && separation > FLT_EPSILON;
	if (near1 || near2)
	{
		V2 v = near1 ? v1 : v2_;
		V2 normal = normalize(sub(c, v));
		separation = dot(sub(c, v), normal);
		if (separation > radius + S2_NP_SPECULATIVE)
		{
			return m;
		}
		V2 cA = mulAdd(v, radiusA, normal);
		V2 cB = mulSub(c, radiusB, normal);
		V2 contactPointA = lerp2(cA, cB, 0.5f);
		m.normal = rotate(xfA.q, normal);
		m.points[0].localAnchorA = contactPointA;
		m.points[0].localAnchorB = xfInvPoint(xf, contactPointA);
		m.points[0].separation = dot(sub(cB, cA), normal);
		m.pointCount = 1;
	}
	else
	{
		V2 normal = polygonA.n(normalIndex);
		m.normal = rotate(xfA.q, normal);
		V2 cA = mulAdd(c, radiusA - dot(sub(c, v1), normal), normal);
		V2 cB = mulSub(c, radiusB, normal);
		V2 contactPointA = lerp2(cA, cB, 0.5f);
		m.points[0].localAnchorA = contactPointA;
		m.points[0].localAnchorB = xfInvPoint(xf, contactPointA);
		m.points[0].separation = separation - radius;
		m.pointCount = 1;
	}
	return m;
}

S2_DEV Manifold clipPolygons(const PolyRef& polyA, const PolyRef& polyB, int edgeA, int edgeB, bool flip)
{
	Manifold m = emptyManifold();
	const PolyRef& poly1 = flip ? polyB : polyA;
	const PolyRef& poly2 = flip ? polyA : polyB;
	int i11 = flip ? edgeB : edgeA;
	int i21 = flip ? edgeA : edgeB;
	int i12 = i11 + 1 < poly1.count ? i11 + 1 : 0;
	int i22 = i21 + 1 < poly2.count ? i21 + 1 : 0;
	V2 normal = poly1.n(i11);
	V2 v11 = poly1.v(i11), v12 = poly1.v(i12);
	V2 v21 = poly2.v(i21), v22 = poly2.v(i22);
	V2 tangent = crossSV(1.0f, normal);
	float lower1 = 0.0f;
	float upper1 = dot(sub(v12, v11), tangent);
	float upper2 = dot(sub(v21, v11), tangent);
	float lower2 = dot(sub(v22, v11), tangent);
	V2 vLower = (lower2 < lower1 && upper2 - lower2 > FLT_EPSILON) ? lerp2(v22, v21, (lower1 - lower2) / (upper2 - lower2)) : v22;
	V2 vUpper = (upper2 > upper1 && upper2 - lower2 > FLT_EPSILON) ? lerp2(v22, v21, (upper1 - lower2) / (upper2 - lower2)) : v21;
	float separationLower = dot(sub(vLower, v11), normal);
	float separationUpper = dot(sub(vUpper, v11), normal);
	float r1 = poly1.radius, r2 = poly2.radius;
	vLower = mulAdd(vLower, 0.5f * (r1 - r2 - separationLower), normal);
	vUpper = mulAdd(vUpper, 0.5f * (r1 - r2 - separationUpper), normal);
	float radius = r1 + r2;
	if (!flip)
	{
		m.normal = normal;
		m.points[0].localAnchorA = vLower;
		m.points[0].separation = separationLower - radius;
		m.points[0].id = makeId(i11, i22);
		m.points[1].localAnchorA = vUpper;
		m.points[1].separation = separationUpper - radius;
		m.points[1].id = makeId(i12, i21);
	}
	else
	{
		m.normal = neg(normal);
		m.points[0].localAnchorA = vUpper;
		m.points[0].separation = separationUpper - radius;
		m.points[0].id = makeId(i21, i12);
		m.points[1].localAnchorA = vLower;
		m.points[1].separation = separationLower - radius;
		m.points[1].id = makeId(i22, i11);
	}
	m.pointCount = 2;
	return m;
}

S2_DEV float findMaxSeparation(int* edgeIndex, const PolyRef& poly1, const PolyRef& poly2)
{
	int bestIndex = 0;
	float maxSeparation = -FLT_MAX;
	for (int i = 0; i < poly1.count; ++i)
	{
		V2 n = poly1.n(i), v1 = poly1.v(i);
		float si = FLT_MAX;
		for (int j = 0; j < poly2.count; ++j)
		{
			float sij = dot(n, sub(poly2.v(j), v1));
			if (sij < si)
			{
				si = sij;
			}
		}
		if (si > maxSeparation)
		{
			maxSeparation = si;
			bestIndex = i;
		}
	}
	*edgeIndex = bestIndex;
	return maxSeparation;
}

S2_DEV int minDotEdge(V2 searchDirection, const PolyRef& poly)
{
	int edge = 0;
	float minDot = FLT_MAX;
	for (int i = 0; i < poly.count; ++i)
	{
		float d = dot(searchDirection, poly.n(i));
		if (d < minDot)
		{
			minDot = d;
			edge = i;
		}
	}
	return edge;
}

// polyB must already be in polyA's frame (the caller built it in LDS)
S2_DEV Manifold collidePolygons(const PolyRef& polyA, Xf xfA, const PolyRef& localPolyB, Xf xf, Cache& cache)
{
	Manifold m = emptyManifold();
	float radius = polyA.radius + localPolyB.radius;
	DistanceOutput output = shapeDistance(cache, polyA, localPolyB);
	if (output.distance > radius + S2_NP_SPECULATIVE)
	{
		return m;
	}
	if (output.distance < 0.1f * S2_LINEAR_SLOP)
	{
		// s2PolygonSAT :441-506
		int edgeA = 0, edgeB = 0;
		float separationA = findMaxSeparation(&edgeA, polyA, localPolyB);
		float separationB = findMaxSeparation(&edgeB, localPolyB, polyA);
		bool flip;
		if (separationB > separationA)
		{
			flip = true;
			edgeA = minDotEdge(localPolyB.n(edgeB), polyA);
		}
		else
		{
			flip = false;
			edgeB = minDotEdge(polyA.n(edgeA), localPolyB);
		}
		m = clipPolygons(polyA, localPolyB, edgeA, edgeB, flip);
	}
	else if (cache.count == 1)
	{
		V2 pA = output.pointA, pB = output.pointB;
		float dist = output.distance;
		V2 normal = normalize(sub(pB, pA));
		V2 contactPointA = mulAdd(pB, 0.5f * (polyA.radius - localPolyB.radius - dist), normal);
		m.normal = rotate(xfA.q, normal);
		m.points[0].localAnchorA = contactPointA;
		m.points[0].localAnchorB = xfInvPoint(xf, contactPointA);
		m.points[0].separation = dist - radius;
		m.points[0].id = makeId(cache.indexA[0], cache.indexB[0]);
		m.pointCount = 1;
		return m;
	}
	else
	{
		bool flip;
		int edgeA, edgeB;
		int countA = polyA.count, countB = localPolyB.count;
		int a1 = cache.indexA[0], a2 = cache.indexA[1];
		int b1 = cache.indexB[0], b2 = cache.indexB[1];
		if (a1 == a2)
		{
			V2 axis = sub(output.pointA, output.pointB);
			float dot1 = dot(axis, localPolyB.n(b1));
			float dot2 = dot(axis, localPolyB.n(b2));
			edgeB = dot1 > dot2 ? b1 : b2;
			flip = true;
			axis = localPolyB.n(edgeB);
			int edgeA1 = a1;
			int edgeA2 = edgeA1 == 0 ? countA - 1 : edgeA1 - 1;
			dot1 = dot(axis, polyA.n(edgeA1));
			dot2 = dot(axis, polyA.n(edgeA2));
			edgeA = dot1 < dot2 ? edgeA1 : edgeA2;
		}
		else
		{
			V2 axis = sub(output.pointB, output.pointA);
			float dot1 = dot(axis, polyA.n(a1));
			float dot2 = dot(axis, polyA.n(a2));
			edgeA = dot1 > dot2 ? a1 : a2;
			flip = false;
			axis = polyA.n(edgeA);
			int edgeB1 = b1;
			int edgeB2 = edgeB1 == 0 ? countB - 1 : edgeB1 - 1;
			dot1 = dot(axis, localPolyB.n(edgeB1));
			dot2 = dot(axis, localPolyB.n(edgeB2));
			edgeB = dot1 < dot2 ? edgeB1 : edgeB2;
		}
		m = clipPolygons(polyA, localPolyB, edgeA, edgeB, flip);
	}
	if (m.pointCount > 0)
	{
		m.normal = rotate(xfA.q, m.normal);
		for (int i = 0; i < m.pointCount; ++i)
		{
			m.points[i].localAnchorB = xfInvPoint(xf, m.points[i].localAnchorA);
		}
	}
	return m;
}

// shape -> polygon in LDS; B is transformed into A's frame on the way (src/manifold.c:517-526).  Capsules and
// segments become two-vertex polygons as s2MakeCapsule builds them (src/geometry.c:100-115).
S2_DEV void stagePolygon(const s2amdShape* sh, const PolyRef& out, bool toFrame, Xf xf, float* radius, int* count)
{
	if (sh->type == S2AMD_SHAPE_POLYGON)
	{
		*count = sh->count;
		*radius = sh->radius;
		for (int i = 0; i < sh->count; ++i)
		{
			V2 vert = v2(sh->vertices[i][0], sh->vertices[i][1]);
			V2 norm = v2(sh->normals[i][0], sh->normals[i][1]);
			if (toFrame)
			{
				vert = xfPoint(xf, vert);
				norm = rotate(xf.q, norm);
			}
			out.set(i, vert, norm);
		}
		return;
	}
	V2 p1 = v2(sh->vertices[0][0], sh->vertices[0][1]), p2 = v2(sh->vertices[1][0], sh->vertices[1][1]);
	V2 axis = normalizeChecked(sub(p2, p1));
	V2 normal = rightPerp(axis);
	V2 n0 = normal, n1 = neg(normal);
	if (toFrame)
	{
		p1 = xfPoint(xf, p1), p2 = xfPoint(xf, p2);
		n0 = rotate(xf.q, n0), n1 = rotate(xf.q, n1);
	}
	out.set(0, p1, n0);
	out.set(1, p2, n1);
	*count = 2;
	*radius = sh->type == S2AMD_SHAPE_CAPSULE ? sh->radius : 0.0f;
}

} // namespace
