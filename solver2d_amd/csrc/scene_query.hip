// Scene queries on the resident world (include/solver2d_amd.h: s2amd_world_ray_cast, s2amd_world_point_probe, s2amd_world_query_boxes):
// what s2World_QueryAABB (src/world.c:605-615), s2Shape_TestPoint (src/shape.c:110-137) and a closest-hit use of
// s2DynamicTree_RayCast (src/dynamic_tree.c:1213-1290) with s2RayCast<type> (src/geometry.c:393-730) answer, computed from the resident
// shape, body and origin arrays instead of a host copy of the world.  Nothing resident is written; everything is enqueued on the
// solver's stream behind whatever changed the world last.  The results are order-free statements (the header states them), so no
// traversal order -- and none of the optional device trees -- takes part.
//
// The mapping is lane per shape, as the report kernels': a workgroup holds one tile of 256 shape slots -- box, category bits, body
// frame and geometry in registers, a polygon's vertices and normals in the lane's LDS column because the exact tests address them by
// computed index -- and walks one chunk of 256 queries staged in LDS, every query a broadcast read.  The grid is tiles x chunks.
//
//   rayCandidatesKernel   per ray the candidates (live, category & mask, s2AABB_Overlaps(fatAABB, segment box)) run s2RayCast<type> in
//                         the body frame; a hit proposes key = (ordered bits of its fraction, -0 as +0) << 32 | slot by a 64-bit integer
//                         atomic min.  The least key is the least fraction, ties to the lowest slot, whatever the launch geometry.
//   rayFinishKernel       one lane per ray: the winner's exact test again (the same operations, so the same bits) and the 32-byte record.
//   listMaskKernel        box queries and point probes: per (query, tile, wave) the 64-bit ballot of the hits.
//   query_list.h          listTilePrefixKernel, listOffsetsKernel, listWriteKernel: the masks into CSR lists ascending by slot.
//
// The host side is query_host.h's ("The query facility"): the ray cast is a queryBest over rayKind, the two list calls a
// queryLists of plain slot lists with no validator; this file supplies the kinds and the launches of its kernels.
//
// All arithmetic is fp32 in the reference's operation order (query_ops.h, gjk_ops.h); this file is compiled without contraction in
// both libraries (Makefile).
#include "query_list.h"
#include "query_host.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "query_ops.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdRay) == 24 && sizeof(s2amdRayHit) == 32 && sizeof(s2amdPointProbe) == 12 && sizeof(s2amdBoxQuery) == 20, "the query records");
static_assert(sizeof(s2amdShape) == 196, "the shape record");

// what a lane keeps of its shape slot
struct LaneShape
{
	bool live;
	int type, body;
	uint32_t category;
	float radius;
	float fat[4];
	V2 a, b; // vertices[0], vertices[1]: circle, capsule, segment
	Xf xf;
};

S2_DEV LaneShape noShape()
{
	LaneShape s;
	s.live = false;
	s.type = S2AMD_SHAPE_FREE, s.body = -1;
	s.category = 0u;
	s.radius = 0.0f;
	s.fat[0] = s.fat[1] = s.fat[2] = s.fat[3] = 0.0f;
	s.a = s.b = v2(0.0f, 0.0f);
	s.xf.p = v2(0.0f, 0.0f);
	s.xf.q.s = 0.0f, s.xf.q.c = 1.0f;
	return s;
}

// Slot `slot` (< n): its header and frame into registers; a polygon's vertices (and normals, when `polygon.norms` is set) into the
// lane's LDS column.  polygon.count is the wire's count clamped to 0..8 -- the bound of every loop over the vertices.
S2_DEV LaneShape loadShape(const s2amdShape* shapes, int slot, const s2amdBody* bodies, const float2* origins, int nb, PolyRef& polygon)
{
	LaneShape s = noShape();
	const s2amdShape* w = shapes + slot;
	s.type = w->type;
	s.live = s.type != S2AMD_SHAPE_FREE;
	polygon.count = 0;
	polygon.radius = 0.0f;
	if (!s.live)
	{
		return s;
	}
	s.body = w->body;
	s.category = w->categoryBits;
	s.radius = w->radius;
	s.fat[0] = w->fatAABB[0], s.fat[1] = w->fatAABB[1], s.fat[2] = w->fatAABB[2], s.fat[3] = w->fatAABB[3];
	s.a = v2(w->vertices[0][0], w->vertices[0][1]);
	s.b = v2(w->vertices[1][0], w->vertices[1][1]);
	if (s.body >= 0 && s.body < nb) // (s2amd_world_upload refuses a live shape on a body outside the array)
	{
		const float2 o = origins[s.body];
		s.xf.p = v2(o.x, o.y);
		s.xf.q.s = bodies[s.body].rot[0], s.xf.q.c = bodies[s.body].rot[1];
	}
	if (s.type == S2AMD_SHAPE_POLYGON)
	{
		const int count = w->count;
		polygon.count = count < 0 ? 0 : count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : count;
		polygon.radius = s.radius;
		for (int i = 0; i < polygon.count; ++i)
		{
			polygon.verts[i * S2_NP_BLOCK] = make_float2(w->vertices[i][0], w->vertices[i][1]);
			if (polygon.norms != nullptr)
			{
				polygon.norms[i * S2_NP_BLOCK] = make_float2(w->normals[i][0], w->normals[i][1]);
			}
		}
		if (polygon.count == 0)
		{
			polygon.verts[0] = make_float2(0.0f, 0.0f); // (GJK reads vertex 0 of an empty proxy)
		}
	}
	return s;
}

// the ray in the shape's body frame (s2InvTransformPoint on both ends, maxFraction as it is), then s2RayCast<type>
S2_DEV RayOut rayCastShape(const LaneShape& s, const PolyRef& polygon, V2 p1, V2 p2, float maxFraction)
{
	RayIn in;
	in.p1 = xfInvPoint(s.xf, p1);
	in.p2 = xfInvPoint(s.xf, p2);
	in.maxFraction = maxFraction;
	switch (s.type)
	{
		case S2AMD_SHAPE_CAPSULE:
			return rayCastCapsule(in, s.a, s.b, s.radius);
		case S2AMD_SHAPE_CIRCLE:
			return rayCastCircle(in, s.a, s.radius);
		case S2AMD_SHAPE_POLYGON:
			return rayCastPolygon(in, polygon);
		case S2AMD_SHAPE_SEGMENT:
			return rayCastSegment(in, s.a, s.b);
		default:
			return rayMiss();
	}
}

// ascending as unsigned integers == ascending as floats; -0 is +0
S2_DEV uint32_t orderedFractionBits(float f)
{
	const uint32_t bits = f == 0.0f ? 0u : asBits(f);
	return (bits & 0x80000000u) != 0u ? ~bits : bits | 0x80000000u;
}

// one staged ray: 40 bytes
struct StagedRay
{
	float p1x, p1y, p2x, p2y, maxFraction;
	uint32_t mask;
	float lx, ly, ux, uy; // the segment box, src/dynamic_tree.c:1231-1238
};

__global__ __launch_bounds__(S2_BLOCK) void rayCandidatesKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const s2amdRay* rays,
																 int count, unsigned long long* keys)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK], norms[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ StagedRay staged[S2_QUERY_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		const s2amdRay r = rays[first + (int)threadIdx.x];
		StagedRay q;
		q.p1x = r.p1[0], q.p1y = r.p1[1], q.p2x = r.p2[0], q.p2y = r.p2[1], q.maxFraction = r.maxFraction, q.mask = r.maskBits;
		const V2 p1 = v2(r.p1[0], r.p1[1]);
		const V2 t = mulAdd(p1, r.maxFraction, sub(v2(r.p2[0], r.p2[1]), p1));
		q.lx = S2_MINF(p1.x, t.x), q.ly = S2_MINF(p1.y, t.y);
		q.ux = S2_MAXF(p1.x, t.x), q.uy = S2_MAXF(p1.y, t.y);
		staged[threadIdx.x] = q;
	}
	PolyRef polygon;
	polygon.verts = verts + threadIdx.x, polygon.norms = norms + threadIdx.x;
	polygon.count = 0, polygon.radius = 0.0f;
	LaneShape s = noShape();
	if (slot < n)
	{
		s = loadShape(shapes, slot, bodies, origins, nb, polygon);
	}
	__syncthreads();
	if (!s.live)
	{
		return;
	}
	for (int k = 0; k < chunk; ++k)
	{
		const StagedRay q = staged[k];
		if ((s.category & q.mask) == 0u || !boxesOverlap(s.fat, q.lx, q.ly, q.ux, q.uy))
		{
			continue;
		}
		const RayOut o = rayCastShape(s, polygon, v2(q.p1x, q.p1y), v2(q.p2x, q.p2y), q.maxFraction);
		if (o.hit)
		{
			const unsigned long long key = ((unsigned long long)orderedFractionBits(o.fraction) << 32) | (unsigned long long)(uint32_t)slot;
			atomicMin(keys + first + k, key);
		}
	}
}

struct alignas(16) HitRecord
{
	float4 lo, hi;
};
static_assert(sizeof(HitRecord) == sizeof(s2amdRayHit), "the hit record as the finish pass stores it");

__global__ __launch_bounds__(S2_BLOCK) void rayFinishKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const s2amdRay* rays, int count,
															 const unsigned long long* keys, HitRecord* hits)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK], norms[S2_NP_MAX_VERTS * S2_BLOCK];
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const s2amdRay r = rays[i];
	const unsigned long long key = keys[i];
	const int slot = keySlot(key);
	HitRecord rec;
	rec.lo = make_float4(__int_as_float(-1), __int_as_float(-1), r.maxFraction, 0.0f);
	rec.hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (slot >= 0 && slot < n)
	{
		PolyRef polygon;
		polygon.verts = verts + threadIdx.x, polygon.norms = norms + threadIdx.x;
		const LaneShape s = loadShape(shapes, slot, bodies, origins, nb, polygon);
		const V2 p1 = v2(r.p1[0], r.p1[1]), p2 = v2(r.p2[0], r.p2[1]);
		const RayOut o = s.live ? rayCastShape(s, polygon, p1, p2, r.maxFraction) : rayMiss();
		if (o.hit)
		{
			const V2 normal = rotate(s.xf.q, o.normal);
			const V2 point = mulAdd(p1, o.fraction, sub(p2, p1));
			rec.lo = make_float4(__int_as_float(slot), __int_as_float(s.body), o.fraction, point.x);
			rec.hi = make_float4(point.y, normal.x, normal.y, 0.0f);
		}
	}
	hits[i] = rec;
}

// one staged list query: a box, or a probe's point as the box {p, p}
struct StagedBox
{
	float lx, ly, ux, uy;
	uint32_t mask;
};

// masks[((query * tiles) + tile) * 4 + wave]: the wave's hits of the query, bit = lane.  Every word is written.
template <bool POINT>
__global__ __launch_bounds__(S2_BLOCK) void listMaskKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, const float2* origins, int nb, const void* queries,
															int count, unsigned long long* masks)
{
	__shared__ float2 verts[POINT ? S2_NP_MAX_VERTS * S2_BLOCK : 1];
	__shared__ float2 probe[POINT ? S2_BLOCK : 1];
	__shared__ StagedBox staged[S2_QUERY_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		StagedBox q;
		if (POINT)
		{
			const s2amdPointProbe p = ((const s2amdPointProbe*)queries)[first + (int)threadIdx.x];
			q.lx = q.ux = p.p[0], q.ly = q.uy = p.p[1], q.mask = p.maskBits;
		}
		else
		{
			const s2amdBoxQuery b = ((const s2amdBoxQuery*)queries)[first + (int)threadIdx.x];
			q.lx = b.box[0], q.ly = b.box[1], q.ux = b.box[2], q.uy = b.box[3], q.mask = b.maskBits;
		}
		staged[threadIdx.x] = q;
	}
	PolyRef polygon, point;
	polygon.verts = verts + (POINT ? threadIdx.x : 0), polygon.norms = nullptr;
	polygon.count = 0, polygon.radius = 0.0f;
	point.verts = probe + (POINT ? threadIdx.x : 0), point.norms = nullptr;
	point.count = 1, point.radius = 0.0f;
	LaneShape s = noShape();
	if (slot < n)
	{
		if (POINT)
		{
			s = loadShape(shapes, slot, bodies, origins, nb, polygon);
		}
		else
		{
			// the box query reads 24 bytes of the slot
			const s2amdShape* w = shapes + slot;
			s.type = w->type;
			s.live = s.type != S2AMD_SHAPE_FREE;
			if (s.live)
			{
				s.category = w->categoryBits;
				s.fat[0] = w->fatAABB[0], s.fat[1] = w->fatAABB[1], s.fat[2] = w->fatAABB[2], s.fat[3] = w->fatAABB[3];
			}
		}
	}
	__syncthreads();
	for (int k = 0; k < chunk; ++k)
	{
		const StagedBox q = staged[k];
		bool hit = s.live && (s.category & q.mask) != 0u && boxesOverlap(s.fat, q.lx, q.ly, q.ux, q.uy);
		if (POINT && hit)
		{
			// s2Shape_TestPoint, src/shape.c:110-137
			const V2 local = xfInvPoint(s.xf, v2(q.lx, q.ly));
			switch (s.type)
			{
				case S2AMD_SHAPE_CAPSULE:
					hit = pointInCapsule(local, s.a, s.b, s.radius);
					break;
				case S2AMD_SHAPE_CIRCLE:
					hit = pointInCircle(local, s.a, s.radius);
					break;
				case S2AMD_SHAPE_POLYGON:
					point.verts[0] = make_float2(local.x, local.y);
					hit = pointInPolygon(polygon, point);
					break;
				default:
					hit = false;
					break;
			}
		}
		const unsigned long long ballot = __ballot(hit);
		if (lane == 0)
		{
			masks[((size_t)(first + k) * tiles + blockIdx.x) * 4 + wave] = ballot;
		}
	}
}

// s2IsValidRay, src/geometry.c:15-20
bool validRay(const void* record)
{
	const s2amdRay& r = *(const s2amdRay*)record;
	const bool finite = std::isfinite(r.p1[0]) && std::isfinite(r.p1[1]) && std::isfinite(r.p2[0]) && std::isfinite(r.p2[1]) && std::isfinite(r.maxFraction);
	return finite && 0.0f <= r.maxFraction && r.maxFraction < 100000.0f;
}

const QueryKind rayKind = {sizeof(s2amdRay), "rays", validRay, "ray", "fails s2IsValidRay (a NaN or infinite end point, or maxFraction outside [0, 100000))", {0, 0}, nullptr};

// ---- the launches query_host.h's drivers ask for ----
void launchRayCandidates(const QueryCall& c, unsigned long long* keys)
{
	rayCandidatesKernel<<<c.grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdRay*)c.records, c.count, keys);
}

void launchRayFinish(const QueryCall& c, const unsigned long long* keys, void* hits)
{
	rayFinishKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdRay*)c.records, c.count, keys,
																				(HitRecord*)hits);
}

template <bool POINT> void launchMasks(const QueryCall& c, unsigned long long* masks)
{
	listMaskKernel<POINT><<<c.grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.tiles, c.bodies, c.origins, c.nb, c.records, c.count, masks);
}

// box queries and point probes: nothing to validate, the lists are the shape slots as they are
template <bool POINT>
int listQuery(s2amdSolver* s, const void* queries, size_t stride, int32_t count, int32_t* offsets, int32_t* shapes, int32_t capacity, int32_t* total)
{
	const QueryKind kind = {stride, "queries", nullptr, nullptr, nullptr, {0, 0}, nullptr};
	const QueryPayload slots = {0, POINT ? "point-probe hit buffer too small" : "box-query hit buffer too small", nullptr};
	return queryLists(s, kind, queries, count, offsets, shapes, nullptr, capacity, total, slots, launchMasks<POINT>);
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_ray_cast(s2amdSolver* s, const s2amdRay* rays, int32_t count, s2amdRayHit* hits)
{
	return queryBest(s, rayKind, rays, count, hits, sizeof(s2amdRayHit), launchRayCandidates, launchRayFinish);
}

int s2amd_world_point_probe(s2amdSolver* s, const s2amdPointProbe* probes, int32_t count, int32_t* offsets, int32_t* shapes, int32_t capacity, int32_t* total)
{
	return listQuery<true>(s, probes, sizeof(s2amdPointProbe), count, offsets, shapes, capacity, total);
}

int s2amd_world_query_boxes(s2amdSolver* s, const s2amdBoxQuery* boxes, int32_t count, int32_t* offsets, int32_t* shapes, int32_t capacity, int32_t* total)
{
	return listQuery<false>(s, boxes, sizeof(s2amdBoxQuery), count, offsets, shapes, capacity, total);
}

} // extern "C"
#pragma GCC visibility pop
