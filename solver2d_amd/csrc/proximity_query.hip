// Proximity queries on the resident world (include/solver2d_amd.h: s2amd_world_closest_shape, s2amd_world_shapes_in_range): what
// s2ShapeDistance (src/distance.c:485-636) over the proxies of s2Shape_MakeDistanceProxy (src/shape.c:75-93) answers between a caller's
// proxy and every shape near it, computed from the resident shape, body and origin arrays instead of a host copy of the world.  Nothing
// resident is written; everything is enqueued on the solver's stream behind whatever changed the world last.  The results are order-free
// statements (the header states them), so no traversal order -- and none of the optional device trees -- takes part.
//
// The mapping is scene_query.hip's: a workgroup holds one tile of 256 shape slots -- box, category bits, body frame, radius and vertex
// count in registers, the up-to-8 proxy vertices in the lane's LDS column because GJK addresses them by computed index -- and walks one
// chunk of 256 queries staged in LDS as they came (96 bytes each, 24 KiB) with their world-space boxes beside them (4 KiB), every query
// a broadcast read.  The grid is tiles x chunks.
//
//   proximityCandidatesKernel<false>  closest shape: a candidate (live, category & mask, s2AABB_Overlaps(fatAABB, query box)) runs the
//                                     distance; one in range proposes key = distance bits << 32 | slot by a 64-bit integer atomic min
//                                     (distances are >= +0: the bits order as the values).  The least key is the least distance, ties to
//                                     the lowest slot, whatever the launch geometry.
//   proximityFinishKernel             one lane per query: the winner's distance again (the same operations, so the same bits) and the record.
//   proximityCandidatesKernel<true>   shapes in range: per (query, tile, wave) the 64-bit ballot of the candidates in range; the lists
//                                     come from query_list.h's listTilePrefixKernel, listOffsetsKernel and listWriteKernel.
//   proximityDistancesKernel          one lane per list entry: its query by bisection of the offsets, the distance again.
//
// The host side is query_host.h's ("The query facility"): closest shape is a queryBest, shapes in range a queryLists of slot
// lists with the distances beside them where asked for; this file supplies proximityKind and the launches of its kernels.
//
// All arithmetic is fp32 in the reference's operation order (gjk_ops.h); this file is compiled without contraction in both libraries
// (Makefile).
#include "query_list.h"
#include "query_host.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "gjk_ops.h"
#include "proxy_ops.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdProximityQuery) == 96 && sizeof(s2amdProximityHit) == 32 && sizeof(s2amdProximityQuery) % 16 == 0, "the query records");

S2_DEV Xf queryFrame(const s2amdProximityQuery& q)
{
	Xf xf;
	xf.p = v2(q.position[0], q.position[1]);
	xf.q.s = q.rot[0], xf.q.c = q.rot[1];
	return xf;
}

// the query box (the header's statement): the bounds of the transformed vertices, folded from vertex 0 in index order, grown by
// radius + maxDistance
S2_DEV float4 queryBox(const s2amdProximityQuery& q)
{
	const Xf xf = queryFrame(q);
	V2 lower = xfPoint(xf, v2(q.vertices[0][0], q.vertices[0][1]));
	V2 upper = lower;
	for (int i = 1; i < q.count && i < S2_NP_MAX_VERTS; ++i)
	{
		const V2 w = xfPoint(xf, v2(q.vertices[i][0], q.vertices[i][1]));
		lower = v2(S2_MINF(lower.x, w.x), S2_MINF(lower.y, w.y));
		upper = v2(S2_MAXF(upper.x, w.x), S2_MAXF(upper.y, w.y));
	}
	const float r = q.radius + q.maxDistance;
	return make_float4(lower.x - r, lower.y - r, upper.x + r, upper.y + r);
}

S2_DEV WireProxy queryProxy(const s2amdProximityQuery* q)
{
	WireProxy A;
	A.verts = q->vertices, A.count = q->count, A.radius = q->radius;
	return A;
}

// D(q, s) of a lane that reads both proxies where the caller's arrays hold them (the finish passes)
S2_DEV ShapeDistanceOutput distanceToSlot(const s2amdProximityQuery* q, const s2amdShape* shapes, int slot, const LaneProxy& s)
{
	return shapeDistanceWithRadii(queryProxy(q), queryFrame(*q), slotProxy(shapes, slot, s), s.xf);
}

// LIST: masks[((query * tiles) + tile) * 4 + wave] = the wave's shapes in range of the query, bit = lane; every word is written.
// Otherwise keys[query] takes the least distance bits << 32 | slot.
template <bool LIST>
__global__ __launch_bounds__(S2_BLOCK) void proximityCandidatesKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, const float2* origins, int nb,
																		 const s2amdProximityQuery* queries, int count, unsigned long long* out)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ alignas(16) s2amdProximityQuery staged[S2_QUERY_CHUNK];
	__shared__ float4 boxes[S2_QUERY_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		// (six 16-byte words straight into LDS: a copy in registers would be indexed by the box's vertex loop, and go to scratch)
		const float4* from = (const float4*)(queries + first + (int)threadIdx.x);
		float4* to = (float4*)(staged + threadIdx.x);
		for (int j = 0; j < (int)(sizeof(s2amdProximityQuery) / sizeof(float4)); ++j)
		{
			to[j] = from[j];
		}
		boxes[threadIdx.x] = queryBox(staged[threadIdx.x]);
	}
	LaneProxy s;
	s.live = false;
	ProxyRef<S2_BLOCK> B;
	B.verts = verts + threadIdx.x, B.count = 1, B.radius = 0.0f;
	if (slot < n)
	{
		s = loadProxy(shapes, slot, bodies, origins, nb);
		if (s.live)
		{
			B.count = s.count, B.radius = s.radius;
			for (int i = 0; i < s.count; ++i)
			{
				verts[i * S2_BLOCK + threadIdx.x] = make_float2(shapes[slot].vertices[i][0], shapes[slot].vertices[i][1]);
			}
		}
	}
	__syncthreads();
	if (!LIST && !s.live)
	{
		return;
	}
	for (int k = 0; k < chunk; ++k)
	{
		const s2amdProximityQuery* q = staged + k;
		const float4 box = boxes[k];
		bool inRange = false;
		float distance = 0.0f;
		if (s.live && (s.category & q->maskBits) != 0u && boxesOverlap(s.fat, box.x, box.y, box.z, box.w))
		{
			distance = shapeDistanceWithRadii(queryProxy(q), queryFrame(*q), B, s.xf).distance;
			inRange = distance <= q->maxDistance;
		}
		if (LIST)
		{
			const unsigned long long ballot = __ballot(inRange);
			if (lane == 0)
			{
				out[((size_t)(first + k) * tiles + blockIdx.x) * 4 + wave] = ballot;
			}
		}
		else if (inRange)
		{
			atomicMin(out + first + k, ((unsigned long long)asBits(distance) << 32) | (unsigned long long)(uint32_t)slot);
		}
	}
}

struct alignas(16) HitRecord
{
	float4 lo, hi;
};
static_assert(sizeof(HitRecord) == sizeof(s2amdProximityHit), "the hit record as the finish pass stores it");

__global__ __launch_bounds__(S2_BLOCK) void proximityFinishKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																   const s2amdProximityQuery* queries, int count, const unsigned long long* keys, HitRecord* hits)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const s2amdProximityQuery* q = queries + i;
	const unsigned long long key = keys[i];
	const int slot = keySlot(key);
	HitRecord rec;
	rec.lo = make_float4(__int_as_float(-1), __int_as_float(-1), q->maxDistance, 0.0f);
	rec.hi = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
	if (slot >= 0 && slot < n)
	{
		const LaneProxy s = loadProxy(shapes, slot, bodies, origins, nb);
		if (s.live)
		{
			const ShapeDistanceOutput o = distanceToSlot(q, shapes, slot, s);
			rec.lo = make_float4(__int_as_float(slot), __int_as_float(s.body), o.distance, o.pointA.x);
			rec.hi = make_float4(o.pointA.y, o.pointB.x, o.pointB.y, __int_as_float(o.iterations));
		}
	}
	hits[i] = rec;
}

// distances[e] for the entries the list holds: e < min(offsets[count], capacity).  The entry's query is the last one whose offset is <= e.
__global__ __launch_bounds__(S2_BLOCK) void proximityDistancesKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																	  const s2amdProximityQuery* queries, int count, const int* offsets, const int32_t* entries, int capacity,
																	  float* distances)
{
	const int e = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (e >= capacity || e >= offsets[count])
	{
		return;
	}
	const int lo = entryQuery(offsets, count, e);
	const int slot = entries[e];
	float distance = 0.0f;
	if (slot >= 0 && slot < n)
	{
		const LaneProxy s = loadProxy(shapes, slot, bodies, origins, nb);
		if (s.live)
		{
			distance = distanceToSlot(queries + lo, shapes, slot, s).distance;
		}
	}
	distances[e] = distance;
}

bool validQuery(const void* record)
{
	const s2amdProximityQuery& q = *(const s2amdProximityQuery*)record;
	if (q.count < 1 || q.count > S2_NP_MAX_VERTS)
	{
		return false;
	}
	bool finite = std::isfinite(q.radius) && std::isfinite(q.maxDistance) && std::isfinite(q.position[0]) && std::isfinite(q.position[1]) &&
				  std::isfinite(q.rot[0]) && std::isfinite(q.rot[1]);
	for (int i = 0; i < q.count; ++i)
	{
		finite = finite && std::isfinite(q.vertices[i][0]) && std::isfinite(q.vertices[i][1]);
	}
	return finite && q.radius >= 0.0f && q.maxDistance >= 0.0f;
}

const QueryKind proximityKind = {sizeof(s2amdProximityQuery), "queries", validQuery, "proximity query",
								 "is invalid (count outside 1..8, a NaN or infinite field, a negative radius or maxDistance)", {0, 0}, nullptr};

// ---- the launches query_host.h's drivers ask for ----
template <bool LIST> void launchCandidates(const QueryCall& c, unsigned long long* out)
{
	proximityCandidatesKernel<LIST>
		<<<c.grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.tiles, c.bodies, c.origins, c.nb, (const s2amdProximityQuery*)c.records, c.count, out);
}

void launchFinish(const QueryCall& c, const unsigned long long* keys, void* hits)
{
	proximityFinishKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdProximityQuery*)c.records, c.count,
																					  keys, (HitRecord*)hits);
}

void launchDistances(const QueryCall& c, const int* offsets, const int32_t* slots, int capacity, void* distances)
{
	proximityDistancesKernel<<<gridFor((size_t)capacity), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdProximityQuery*)c.records,
																						  c.count, offsets, slots, capacity, (float*)distances);
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_closest_shape(s2amdSolver* s, const s2amdProximityQuery* queries, int32_t count, s2amdProximityHit* hits)
{
	return queryBest(s, proximityKind, queries, count, hits, sizeof(s2amdProximityHit), launchCandidates<false>, launchFinish);
}

int s2amd_world_shapes_in_range(s2amdSolver* s, const s2amdProximityQuery* queries, int32_t count, int32_t* offsets, int32_t* shapes, float* distances, int32_t capacity,
								int32_t* total)
{
	const QueryPayload slots = {0, "shapes-in-range buffer too small", launchDistances};
	return queryLists(s, proximityKind, queries, count, offsets, shapes, distances, capacity, total, slots, launchCandidates<true>);
}

} // extern "C"
#pragma GCC visibility pop
