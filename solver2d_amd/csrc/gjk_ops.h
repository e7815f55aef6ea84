// GJK of the reference (src/distance.c:120-604) in the one form the contact and containment callers use -- identity transforms, no radii
// -- with the small transform and vector helpers and the LDS polygon it addresses by computed index: shared by the narrow phase
// (narrowphase.hip: s2CollidePolygons, src/manifold.c:523-530) and the scene queries (scene_query.hip: s2PointInPolygon,
// src/geometry.c:376-389).  Below it the general form (:485-636: both transforms, radii, iteration count) of the proximity queries
// (proximity_query.hip).  The including file defines S2_NP_BLOCK, the stride of its LDS polygons (its workgroup size), and
// S2_NP_MAX_VERTS first.  Everything is in an unnamed namespace: each file holds its own copy.
#pragma once

#include "s2_device.h"

#include <cfloat>

namespace
{

struct Xf
{
	V2 p;
	Rot q;
};

S2_DEV V2 xfPoint(Xf xf, V2 p) // math.h:350-356
{
	float x = (xf.q.c * p.x - xf.q.s * p.y) + xf.p.x;
	float y = (xf.q.s * p.x + xf.q.c * p.y) + xf.p.y;
	return v2(x, y);
}
S2_DEV V2 xfInvPoint(Xf xf, V2 p) // math.h:359-364
{
	float vx = p.x - xf.p.x, vy = p.y - xf.p.y;
	return v2(xf.q.c * vx + xf.q.s * vy, -xf.q.s * vx + xf.q.c * vy);
}
S2_DEV Xf xfInvMul(Xf A, Xf B) // math.h:378-384, s2InvMulRot :307-317
{
	Xf C;
	C.q.s = A.q.c * B.q.s - A.q.s * B.q.c;
	C.q.c = A.q.c * B.q.c + A.q.s * B.q.s;
	C.p = invRotate(A.q, sub(B.p, A.p));
	return C;
}
S2_DEV V2 lerp2(V2 a, V2 b, float t) { return v2(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y)); } // math.h:103-106
S2_DEV float distance2(V2 a, V2 b)																	 // math.h:180-185
{
	float dx = b.x - a.x, dy = b.y - a.y;
	return sqrtf(dx * dx + dy * dy);
}
S2_DEV V2 normalizeChecked(V2 v) // src/math.c:54-66
{
	float len = length(v);
	if (len < FLT_EPSILON)
	{
		return v2(0.0f, 0.0f);
	}
	float inv = 1.0f / len;
	return v2(inv * v.x, inv * v.y);
}
S2_DEV V2 lengthAndNormalize(float* len, V2 v) // src/math.c:68-80
{
	*len = length(v);
	if (*len < FLT_EPSILON)
	{
		return v2(0.0f, 0.0f);
	}
	float inv = 1.0f / *len;
	return v2(inv * v.x, inv * v.y);
}

// A polygon in LDS: vertices and normals interleaved per workgroup thread (stride = blockDim) so that lanes
// reading "their" vertex i hit distinct banks
struct PolyRef
{
	float2* verts; // [S2_NP_MAX_VERTS] at stride S2_NP_BLOCK
	float2* norms;
	float radius;
	int count;
	S2_DEV V2 v(int i) const
	{
		float2 t = verts[i * S2_NP_BLOCK];
		return v2(t.x, t.y);
	}
	S2_DEV V2 n(int i) const
	{
		float2 t = norms[i * S2_NP_BLOCK];
		return v2(t.x, t.y);
	}
	S2_DEV void set(int i, V2 vert, V2 norm) const
	{
		verts[i * S2_NP_BLOCK] = make_float2(vert.x, vert.y);
		norms[i * S2_NP_BLOCK] = make_float2(norm.x, norm.y);
	}
};

struct Cache
{
	float metric;
	int count;
	int indexA[3], indexB[3];
};

// ---- GJK (src/distance.c) ----
struct SVertex
{
	V2 wA, wB, w;
	float a;
	int indexA, indexB;
};

S2_DEV int findSupport(const PolyRef& p, V2 d) // :120-135
{
	int best = 0;
	float bestValue = dot(p.v(0), d);
	for (int i = 1; i < p.count; ++i)
	{
		float value = dot(p.v(i), d);
		if (value > bestValue)
		{
			best = i;
			bestValue = value;
		}
	}
	return best;
}

S2_DEV V2 weight2(float a1, V2 w1, float a2, V2 w2) { return v2(a1 * w1.x + a2 * w2.x, a1 * w1.y + a2 * w2.y); }
S2_DEV V2 weight3(float a1, V2 w1, float a2, V2 w2, float a3, V2 w3)
{
	return v2(a1 * w1.x + a2 * w2.x + a3 * w3.x, a1 * w1.y + a2 * w2.y + a3 * w3.y);
}

struct DistanceOutput
{
	V2 pointA, pointB;
	float distance;
};

// s2ShapeDistance in the only form the manifold code uses: identity transforms, no radii (src/manifold.c:523-530)
S2_DEV DistanceOutput shapeDistance(Cache& cache, const PolyRef& A, const PolyRef& B)
{
	const Xf identity = {v2(0.0f, 0.0f), {0.0f, 1.0f}};
	SVertex s0, s1, s2;
	s0.a = s1.a = s2.a = 0.0f;
	s0.indexA = s0.indexB = s1.indexA = s1.indexB = s2.indexA = s2.indexB = 0;
	s0.wA = s0.wB = s0.w = s1.wA = s1.wB = s1.w = s2.wA = s2.wB = s2.w = v2(0.0f, 0.0f);
	int count = cache.count;
	// s2MakeSimplexFromCache :172-214
	auto fromCache = [&](SVertex& v, int i) {
		v.indexA = cache.indexA[i];
		v.indexB = cache.indexB[i];
		v.wA = xfPoint(identity, A.v(v.indexA));
		v.wB = xfPoint(identity, B.v(v.indexB));
		v.w = sub(v.wB, v.wA);
		v.a = -1.0f;
	};
	if (count > 0)
	{
		fromCache(s0, 0);
	}
	if (count > 1)
	{
		fromCache(s1, 1);
	}
	if (count > 2)
	{
		fromCache(s2, 2);
	}
	if (count == 0)
	{
		s0.indexA = 0;
		s0.indexB = 0;
		s0.wA = xfPoint(identity, A.v(0));
		s0.wB = xfPoint(identity, B.v(0));
		s0.w = sub(s0.wB, s0.wA);
		s0.a = 1.0f;
		count = 1;
	}

	int saveA[3] = {0, 0, 0}, saveB[3] = {0, 0, 0};
	int iter = 0;
	while (iter < 20)
	{
		int saveCount = count;
		saveA[0] = s0.indexA, saveB[0] = s0.indexB;
		saveA[1] = s1.indexA, saveB[1] = s1.indexB;
		saveA[2] = s2.indexA, saveB[2] = s2.indexB;

		if (count == 2)
		{
			// s2SolveSimplex2 :337-367
			V2 w1 = s0.w, w2 = s1.w;
			V2 e12 = sub(w2, w1);
			float d12_2 = -dot(w1, e12);
			if (d12_2 <= 0.0f)
			{
				s0.a = 1.0f;
				count = 1;
			}
			else
			{
				float d12_1 = dot(w2, e12);
				if (d12_1 <= 0.0f)
				{
					s1.a = 1.0f;
					count = 1;
					s0 = s1;
				}
				else
				{
					float inv_d12 = 1.0f / (d12_1 + d12_2);
					s0.a = d12_1 * inv_d12;
					s1.a = d12_2 * inv_d12;
					count = 2;
				}
			}
		}
		else if (count == 3)
		{
			// s2SolveSimplex3 :369-473
			V2 w1 = s0.w, w2 = s1.w, w3 = s2.w;
			V2 e12 = sub(w2, w1);
			float w1e12 = dot(w1, e12), w2e12 = dot(w2, e12);
			float d12_1 = w2e12, d12_2 = -w1e12;
			V2 e13 = sub(w3, w1);
			float w1e13 = dot(w1, e13), w3e13 = dot(w3, e13);
			float d13_1 = w3e13, d13_2 = -w1e13;
			V2 e23 = sub(w3, w2);
			float w2e23 = dot(w2, e23), w3e23 = dot(w3, e23);
			float d23_1 = w3e23, d23_2 = -w2e23;
			float n123 = cross(e12, e13);
			float d123_1 = n123 * cross(w2, w3);
			float d123_2 = n123 * cross(w3, w1);
			float d123_3 = n123 * cross(w1, w2);
			if (d12_2 <= 0.0f && d13_2 <= 0.0f)
			{
				s0.a = 1.0f;
				count = 1;
			}
			else if (d12_1 > 0.0f && d12_2 > 0.0f && d123_3 <= 0.0f)
			{
				float inv = 1.0f / (d12_1 + d12_2);
				s0.a = d12_1 * inv;
				s1.a = d12_2 * inv;
				count = 2;
			}
			else if (d13_1 > 0.0f && d13_2 > 0.0f && d123_2 <= 0.0f)
			{
				float inv = 1.0f / (d13_1 + d13_2);
				s0.a = d13_1 * inv;
				s2.a = d13_2 * inv;
				count = 2;
				s1 = s2;
			}
			else if (d12_1 <= 0.0f && d23_2 <= 0.0f)
			{
				s1.a = 1.0f;
				count = 1;
				s0 = s1;
			}
			else if (d13_1 <= 0.0f && d23_1 <= 0.0f)
			{
				s2.a = 1.0f;
				count = 1;
				s0 = s2;
			}
			else if (d23_1 > 0.0f && d23_2 > 0.0f && d123_1 <= 0.0f)
			{
				float inv = 1.0f / (d23_1 + d23_2);
				s1.a = d23_1 * inv;
				s2.a = d23_2 * inv;
				count = 2;
				s0 = s2;
			}
			else
			{
				float inv = 1.0f / (d123_1 + d123_2 + d123_3);
				s0.a = d123_1 * inv;
				s1.a = d123_2 * inv;
				s2.a = d123_3 * inv;
				count = 3;
			}
		}
		if (count == 3)
		{
			break;
		}
		// s2ComputeSimplexSearchDirection :228-254
		V2 d;
		if (count == 1)
		{
			d = neg(s0.w);
		}
		else
		{
			V2 e12 = sub(s1.w, s0.w);
			float sgn = cross(e12, neg(s0.w));
			d = sgn > 0.0f ? crossSV(1.0f, e12) : crossVS(e12, 1.0f);
		}
		if (dot(d, d) < FLT_EPSILON * FLT_EPSILON)
		{
			break;
		}
		SVertex nv;
		nv.a = count == 1 ? s1.a : s2.a; // the slot's barycentric coordinate is left as it was (:568-573 touch w*, index* only)
		nv.indexA = findSupport(A, invRotate(identity.q, neg(d)));
		nv.wA = xfPoint(identity, A.v(nv.indexA));
		nv.indexB = findSupport(B, invRotate(identity.q, d));
		nv.wB = xfPoint(identity, B.v(nv.indexB));
		nv.w = sub(nv.wB, nv.wA);
		if (count == 1)
		{
			s1 = nv;
		}
		else
		{
			s2 = nv;
		}
		++iter;
		bool duplicate = false;
		for (int i = 0; i < saveCount; ++i)
		{
			if (nv.indexA == saveA[i] && nv.indexB == saveB[i])
			{
				duplicate = true;
				break;
			}
		}
		if (duplicate)
		{
			break;
		}
		++count;
	}

	DistanceOutput out;
	if (count == 1)
	{
		out.pointA = s0.wA;
		out.pointB = s0.wB;
	}
	else if (count == 2)
	{
		out.pointA = weight2(s0.a, s0.wA, s1.a, s1.wA);
		out.pointB = weight2(s0.a, s0.wB, s1.a, s1.wB);
	}
	else
	{
		out.pointA = weight3(s0.a, s0.wA, s1.a, s1.wA, s2.a, s2.wA);
		out.pointB = out.pointA;
	}
	out.distance = distance2(out.pointA, out.pointB);

	// s2MakeSimplexCache :216-226 with s2Simplex_Metric :149-170 (slots beyond count keep their old indices)
	if (count == 1)
	{
		cache.metric = 0.0f;
	}
	else if (count == 2)
	{
		cache.metric = distance2(s0.w, s1.w);
	}
	else
	{
		cache.metric = cross(sub(s1.w, s0.w), sub(s2.w, s0.w));
	}
	cache.count = count;
	cache.indexA[0] = s0.indexA & 0xff, cache.indexB[0] = s0.indexB & 0xff;
	if (count > 1)
	{
		cache.indexA[1] = s1.indexA & 0xff, cache.indexB[1] = s1.indexB & 0xff;
	}
	if (count > 2)
	{
		cache.indexA[2] = s2.indexA & 0xff, cache.indexB[2] = s2.indexB & 0xff;
	}
	return out;
}

// ---- s2ShapeDistance in its general form (src/distance.c:485-636): both transforms, the radii epilogue, the iteration count ----
// The proximity queries' distance (proximity_query.hip).  A proxy is vertices at a stride, wherever they lie -- a staged query read by
// every lane (stride 1), a lane's LDS column (stride S2_NP_BLOCK), a wire record in global memory (stride 1); the cache is empty
// (count == 0) and is not returned.  The simplex is three named vertices, as above: indexing them would put them in scratch.
template <int STRIDE>
struct ProxyRef
{
	const float2* verts;
	int count;
	float radius;
	S2_DEV V2 v(int i) const
	{
		float2 t = verts[i * STRIDE];
		return v2(t.x, t.y);
	}
};

template <class P>
S2_DEV int findSupportOf(const P& p, V2 d) // :116-131
{
	int best = 0;
	float bestValue = dot(p.v(0), d);
	for (int i = 1; i < p.count; ++i)
	{
		float value = dot(p.v(i), d);
		if (value > bestValue)
		{
			best = i;
			bestValue = value;
		}
	}
	return best;
}

struct Simplex
{
	SVertex v1, v2, v3;
	int count;
};

S2_DEV void solveSimplex2(Simplex& s) // :333-365
{
	V2 w1 = s.v1.w, w2 = s.v2.w;
	V2 e12 = sub(w2, w1);
	float d12_2 = -dot(w1, e12);
	if (d12_2 <= 0.0f)
	{
		s.v1.a = 1.0f;
		s.count = 1;
		return;
	}
	float d12_1 = dot(w2, e12);
	if (d12_1 <= 0.0f)
	{
		s.v2.a = 1.0f;
		s.count = 1;
		s.v1 = s.v2;
		return;
	}
	float inv_d12 = 1.0f / (d12_1 + d12_2);
	s.v1.a = d12_1 * inv_d12;
	s.v2.a = d12_2 * inv_d12;
	s.count = 2;
}

S2_DEV void solveSimplex3(Simplex& s) // :367-474
{
	V2 w1 = s.v1.w, w2 = s.v2.w, w3 = s.v3.w;
	V2 e12 = sub(w2, w1);
	float w1e12 = dot(w1, e12), w2e12 = dot(w2, e12);
	float d12_1 = w2e12, d12_2 = -w1e12;
	V2 e13 = sub(w3, w1);
	float w1e13 = dot(w1, e13), w3e13 = dot(w3, e13);
	float d13_1 = w3e13, d13_2 = -w1e13;
	V2 e23 = sub(w3, w2);
	float w2e23 = dot(w2, e23), w3e23 = dot(w3, e23);
	float d23_1 = w3e23, d23_2 = -w2e23;
	float n123 = cross(e12, e13);
	float d123_1 = n123 * cross(w2, w3);
	float d123_2 = n123 * cross(w3, w1);
	float d123_3 = n123 * cross(w1, w2);
	if (d12_2 <= 0.0f && d13_2 <= 0.0f)
	{
		s.v1.a = 1.0f;
		s.count = 1;
		return;
	}
	if (d12_1 > 0.0f && d12_2 > 0.0f && d123_3 <= 0.0f)
	{
		float inv_d12 = 1.0f / (d12_1 + d12_2);
		s.v1.a = d12_1 * inv_d12;
		s.v2.a = d12_2 * inv_d12;
		s.count = 2;
		return;
	}
	if (d13_1 > 0.0f && d13_2 > 0.0f && d123_2 <= 0.0f)
	{
		float inv_d13 = 1.0f / (d13_1 + d13_2);
		s.v1.a = d13_1 * inv_d13;
		s.v3.a = d13_2 * inv_d13;
		s.count = 2;
		s.v2 = s.v3;
		return;
	}
	if (d12_1 <= 0.0f && d23_2 <= 0.0f)
	{
		s.v2.a = 1.0f;
		s.count = 1;
		s.v1 = s.v2;
		return;
	}
	if (d13_1 <= 0.0f && d23_1 <= 0.0f)
	{
		s.v3.a = 1.0f;
		s.count = 1;
		s.v1 = s.v3;
		return;
	}
	if (d23_1 > 0.0f && d23_2 > 0.0f && d123_1 <= 0.0f)
	{
		float inv_d23 = 1.0f / (d23_1 + d23_2);
		s.v2.a = d23_1 * inv_d23;
		s.v3.a = d23_2 * inv_d23;
		s.count = 2;
		s.v1 = s.v3;
		return;
	}
	float inv_d123 = 1.0f / (d123_1 + d123_2 + d123_3);
	s.v1.a = d123_1 * inv_d123;
	s.v2.a = d123_2 * inv_d123;
	s.v3.a = d123_3 * inv_d123;
	s.count = 3;
}

struct ShapeDistanceOutput // s2DistanceOutput, include/solver2d/distance.h:60-66
{
	V2 pointA, pointB;
	float distance;
	int iterations;
};

// s2ShapeDistance(&emptyCache, {proxyA, proxyB, transformA, transformB, useRadii = true})
template <class PA, class PB>
S2_DEV ShapeDistanceOutput shapeDistanceWithRadii(const PA& A, Xf xfA, const PB& B, Xf xfB)
{
	Simplex s;
	s.v2.a = s.v3.a = 0.0f; // (never read before a solve sets them; the reference leaves them unset)
	s.v2.indexA = s.v2.indexB = s.v3.indexA = s.v3.indexB = 0;
	s.v2.wA = s.v2.wB = s.v2.w = s.v3.wA = s.v3.wB = s.v3.w = v2(0.0f, 0.0f);
	// s2MakeSimplexFromCache with an empty cache :198-210
	s.v1.indexA = 0;
	s.v1.indexB = 0;
	s.v1.wA = xfPoint(xfA, A.v(0));
	s.v1.wB = xfPoint(xfB, B.v(0));
	s.v1.w = sub(s.v1.wB, s.v1.wA);
	s.v1.a = 1.0f;
	s.count = 1;

	int saveA0 = 0, saveB0 = 0, saveA1 = 0, saveB1 = 0, saveA2 = 0, saveB2 = 0;
	int iter = 0;
	while (iter < 20)
	{
		const int saveCount = s.count;
		saveA0 = s.v1.indexA, saveB0 = s.v1.indexB;
		saveA1 = s.v2.indexA, saveB1 = s.v2.indexB;
		saveA2 = s.v3.indexA, saveB2 = s.v3.indexB;
		if (s.count == 2)
		{
			solveSimplex2(s);
		}
		else if (s.count == 3)
		{
			solveSimplex3(s);
		}
		if (s.count == 3)
		{
			break;
		}
		// s2ComputeSimplexSearchDirection :227-254
		V2 d;
		if (s.count == 1)
		{
			d = neg(s.v1.w);
		}
		else
		{
			V2 e12 = sub(s.v2.w, s.v1.w);
			float sgn = cross(e12, neg(s.v1.w));
			d = sgn > 0.0f ? crossSV(1.0f, e12) : crossVS(e12, 1.0f);
		}
		if (dot(d, d) < FLT_EPSILON * FLT_EPSILON)
		{
			break;
		}
		// :562-567: the new vertex's w*, index* are set, its barycentric coordinate stays what the slot held
		SVertex nv;
		nv.a = s.count == 1 ? s.v2.a : s.v3.a;
		nv.indexA = findSupportOf(A, invRotate(xfA.q, neg(d)));
		nv.wA = xfPoint(xfA, A.v(nv.indexA));
		nv.indexB = findSupportOf(B, invRotate(xfB.q, d));
		nv.wB = xfPoint(xfB, B.v(nv.indexB));
		nv.w = sub(nv.wB, nv.wA);
		if (s.count == 1)
		{
			s.v2 = nv;
		}
		else
		{
			s.v3 = nv;
		}
		++iter;
		bool duplicate = nv.indexA == saveA0 && nv.indexB == saveB0; // (saveCount >= 1)
		duplicate = duplicate || (saveCount > 1 && nv.indexA == saveA1 && nv.indexB == saveB1);
		duplicate = duplicate || (saveCount > 2 && nv.indexA == saveA2 && nv.indexB == saveB2);
		if (duplicate)
		{
			break;
		}
		++s.count;
	}

	// s2ComputeSimplexWitnessPoints :279-308
	ShapeDistanceOutput out;
	if (s.count == 1)
	{
		out.pointA = s.v1.wA;
		out.pointB = s.v1.wB;
	}
	else if (s.count == 2)
	{
		out.pointA = weight2(s.v1.a, s.v1.wA, s.v2.a, s.v2.wA);
		out.pointB = weight2(s.v1.a, s.v1.wB, s.v2.a, s.v2.wB);
	}
	else
	{
		out.pointA = weight3(s.v1.a, s.v1.wA, s.v2.a, s.v2.wA, s.v3.a, s.v3.wA);
		out.pointB = out.pointA;
	}
	out.distance = distance2(out.pointA, out.pointB);
	out.iterations = iter;

	// the radii :610-633
	if (out.distance < FLT_EPSILON)
	{
		V2 p = v2(0.5f * (out.pointA.x + out.pointB.x), 0.5f * (out.pointA.y + out.pointB.y));
		out.pointA = p;
		out.pointB = p;
		out.distance = 0.0f;
	}
	else
	{
		float rA = A.radius, rB = B.radius;
		float reduced = out.distance - rA - rB;
		out.distance = S2_MAXF(0.0f, reduced);
		V2 normal = normalize(sub(out.pointB, out.pointA));
		V2 offsetA = v2(rA * normal.x, rA * normal.y);
		V2 offsetB = v2(rB * normal.x, rB * normal.y);
		out.pointA = add(out.pointA, offsetA);
		out.pointB = sub(out.pointB, offsetB);
	}
	return out;
}

} // namespace
