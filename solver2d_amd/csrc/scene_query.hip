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
//   query_list.h          listTilePrefixKernel, listOffsetsKernel, listWriteKernel: the masks into CSR lists ascending by slot (shared
//                         with proximity_query.hip).
//
// All arithmetic is fp32 in the reference's operation order (query_ops.h, gjk_ops.h); this file is compiled without contraction in
// both libraries (Makefile).
#include "query_list.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "query_ops.h"

#include <cmath>
#include <cstring>

namespace
{

static_assert(sizeof(s2amdRay) == 24 && sizeof(s2amdRayHit) == 32 && sizeof(s2amdPointProbe) == 12 && sizeof(s2amdBoxQuery) == 20, "the query records");
static_assert(sizeof(s2amdShape) == 196, "the shape record");

#define S2_NO_HIT_KEY 0xffffffffffffffffull

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
	const int slot = (int)(uint32_t)(key & 0xffffffffull);
	HitRecord rec;
	rec.lo = make_float4(__int_as_float(-1), __int_as_float(-1), r.maxFraction, 0.0f);
	rec.hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (key != S2_NO_HIT_KEY && slot >= 0 && slot < n)
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
bool validRay(const s2amdRay& r)
{
	const bool finite = std::isfinite(r.p1[0]) && std::isfinite(r.p1[1]) && std::isfinite(r.p2[0]) && std::isfinite(r.p2[1]) && std::isfinite(r.maxFraction);
	return finite && 0.0f <= r.maxFraction && r.maxFraction < 100000.0f;
}

// box queries and point probes: upload, four launches, one copy back of {offsets, entries}
template <bool POINT>
int listQuery(s2amdSolver* s, const void* queries, size_t stride, int32_t count, int32_t* offsets, int32_t* shapes, int32_t capacity, int32_t* total)
{
	if (!s || count < 0 || capacity < 0 || !total || (count > 0 && (!queries || !offsets)) || (capacity > 0 && !shapes))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (int rc = queryState(s))
	{
		return rc;
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	if (count > S2_QUERY_MAX_COUNT)
	{
		return fail(S2AMD_E_INVALID, "more queries than one call takes: split the batch");
	}
	const int ns = s->shapeCapacity;
	if (ns <= 0)
	{
		std::memset(offsets, 0, ((size_t)count + 1) * sizeof(int32_t));
		*total = 0;
		return S2AMD_OK;
	}
	const int tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	const size_t words = (size_t)count * tiles * 4;
	if ((size_t)count * (size_t)ns > (size_t)INT32_MAX)
	{
		return fail(S2AMD_E_INVALID, "queries x shape slots beyond 2^31: split the batch");
	}
	// no list is longer than the shape slots, nor all together than the caller's capacity
	const size_t entries = std::min((size_t)capacity, (size_t)count * (size_t)ns);
	size_t at = 0;
	const size_t inAt = at;
	at += roundUp((size_t)count * stride);
	const size_t masksAt = at;
	at += roundUp(words * sizeof(unsigned long long));
	const size_t prefixAt = at;
	at += roundUp((size_t)count * tiles * sizeof(int));
	const size_t totalsAt = at;
	at += roundUp((size_t)count * sizeof(int));
	const size_t outAt = at; // {offsets[count + 1], entries}
	const size_t outBytes = ((size_t)count + 1 + entries) * sizeof(int32_t);
	at += roundUp(outBytes);
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	HIP_TRY(hipMemcpyAsync(base + inAt, queries, (size_t)count * stride, hipMemcpyHostToDevice, st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	unsigned long long* masks = (unsigned long long*)(base + masksAt);
	int* dOffsets = (int*)(base + outAt);
	listMaskKernel<POINT><<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, tiles, (const s2amdBody*)s->dBodies.p,
																							   (const float2*)s->dOrigins.p, s->bodyCapacity, base + inAt, count, masks);
	listTilePrefixKernel<<<dim3((unsigned)((count + 3) / 4)), dim3(S2_BLOCK), 0, st>>>(masks, count, tiles, (int*)(base + prefixAt), (int*)(base + totalsAt));
	listOffsetsKernel<<<dim3(1), dim3(64), 0, st>>>((const int*)(base + totalsAt), count, dOffsets);
	listWriteKernel<<<gridFor(words), dim3(S2_BLOCK), 0, st>>>(masks, words, tiles, (const int*)(base + prefixAt), dOffsets, dOffsets + count + 1, (int)entries);
	HIP_TRY(hipGetLastError());
	s->hQueryStage.resize((size_t)count + 1 + entries);
	HIP_TRY(hipMemcpyAsync(s->hQueryStage.data(), base + outAt, outBytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	std::memcpy(offsets, s->hQueryStage.data(), ((size_t)count + 1) * sizeof(int32_t));
	*total = offsets[count];
	if (*total > capacity)
	{
		return fail(S2AMD_E_CAPACITY, POINT ? "point-probe hit buffer too small" : "box-query hit buffer too small");
	}
	if (*total > 0)
	{
		std::memcpy(shapes, s->hQueryStage.data() + count + 1, (size_t)*total * sizeof(int32_t));
	}
	return S2AMD_OK;
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_ray_cast(s2amdSolver* s, const s2amdRay* rays, int32_t count, s2amdRayHit* hits)
{
	if (!s || count < 0 || (count > 0 && (!rays || !hits)))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (int rc = queryState(s))
	{
		return rc;
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	if (count > S2_QUERY_MAX_COUNT)
	{
		return fail(S2AMD_E_INVALID, "more rays than one call takes: split the batch");
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validRay(rays[i]))
		{
			return fail(S2AMD_E_INVALID, "ray " + std::to_string(i) + " fails s2IsValidRay (a NaN or infinite end point, or maxFraction outside [0, 100000))");
		}
	}
	const int ns = s->shapeCapacity;
	const int tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	size_t at = 0;
	const size_t inAt = at;
	at += roundUp((size_t)count * sizeof(s2amdRay));
	const size_t keysAt = at;
	at += roundUp((size_t)count * sizeof(unsigned long long));
	const size_t hitsAt = at;
	at += roundUp((size_t)count * sizeof(s2amdRayHit));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	const s2amdRay* dRays = (const s2amdRay*)(base + inAt);
	unsigned long long* keys = (unsigned long long*)(base + keysAt);
	HIP_TRY(hipMemcpyAsync(base + inAt, rays, (size_t)count * sizeof(s2amdRay), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)count * sizeof(unsigned long long), st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	if (tiles > 0)
	{
		rayCandidatesKernel<<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p,
																								 (const float2*)s->dOrigins.p, s->bodyCapacity, dRays, count, keys);
	}
	rayFinishKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p,
																		s->bodyCapacity, dRays, count, keys, (HitRecord*)(base + hitsAt));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hits, base + hitsAt, (size_t)count * sizeof(s2amdRayHit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return S2AMD_OK;
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
