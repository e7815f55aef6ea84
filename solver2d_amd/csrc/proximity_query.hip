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
// All arithmetic is fp32 in the reference's operation order (gjk_ops.h); this file is compiled without contraction in both libraries
// (Makefile).
#include "query_list.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "gjk_ops.h"
#include "proxy_ops.h"

#include <cmath>
#include <cstring>

namespace
{

static_assert(sizeof(s2amdProximityQuery) == 96 && sizeof(s2amdProximityHit) == 32 && sizeof(s2amdProximityQuery) % 16 == 0, "the query records");

#define S2_NO_SHAPE_KEY 0xffffffffffffffffull

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
	const int slot = (int)(uint32_t)(key & 0xffffffffull);
	HitRecord rec;
	rec.lo = make_float4(__int_as_float(-1), __int_as_float(-1), q->maxDistance, 0.0f);
	rec.hi = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
	if (key != S2_NO_SHAPE_KEY && slot >= 0 && slot < n)
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
	int lo = 0, hi = count; // offsets[lo] <= e < offsets[hi]
	while (hi - lo > 1)
	{
		const int mid = lo + (hi - lo) / 2;
		if (offsets[mid] <= e)
		{
			lo = mid;
		}
		else
		{
			hi = mid;
		}
	}
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

bool validQuery(const s2amdProximityQuery& q)
{
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

// what both calls check before anything is enqueued; *proceed is false when the call has already been answered
int openCall(s2amdSolver* s, const s2amdProximityQuery* queries, int32_t count, bool* proceed)
{
	*proceed = false;
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
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validQuery(queries[i]))
		{
			return fail(S2AMD_E_INVALID, "proximity query " + std::to_string(i) +
											 " is invalid (count outside 1..8, a NaN or infinite field, a negative radius or maxDistance)");
		}
	}
	*proceed = true;
	return S2AMD_OK;
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_closest_shape(s2amdSolver* s, const s2amdProximityQuery* queries, int32_t count, s2amdProximityHit* hits)
{
	if (!s || count < 0 || (count > 0 && (!queries || !hits)))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	bool proceed;
	if (int rc = openCall(s, queries, count, &proceed))
	{
		return rc;
	}
	if (!proceed)
	{
		return S2AMD_OK;
	}
	const int ns = s->shapeCapacity;
	const int tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	size_t at = 0;
	const size_t inAt = at;
	at += roundUp((size_t)count * sizeof(s2amdProximityQuery));
	const size_t keysAt = at;
	at += roundUp((size_t)count * sizeof(unsigned long long));
	const size_t hitsAt = at;
	at += roundUp((size_t)count * sizeof(s2amdProximityHit));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	const s2amdProximityQuery* dQueries = (const s2amdProximityQuery*)(base + inAt);
	unsigned long long* keys = (unsigned long long*)(base + keysAt);
	HIP_TRY(hipMemcpyAsync(base + inAt, queries, (size_t)count * sizeof(s2amdProximityQuery), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)count * sizeof(unsigned long long), st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	if (tiles > 0)
	{
		proximityCandidatesKernel<false><<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(
			(const s2amdShape*)s->dShapes.p, ns, tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity, dQueries, count, keys);
	}
	proximityFinishKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p,
																			  s->bodyCapacity, dQueries, count, keys, (HitRecord*)(base + hitsAt));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hits, base + hitsAt, (size_t)count * sizeof(s2amdProximityHit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return S2AMD_OK;
}

// upload, the mask pass, query_list.h's three, the distances where asked for, one copy back of {offsets, entries, distances}
int s2amd_world_shapes_in_range(s2amdSolver* s, const s2amdProximityQuery* queries, int32_t count, int32_t* offsets, int32_t* shapes, float* distances, int32_t capacity,
								int32_t* total)
{
	if (!s || count < 0 || capacity < 0 || !total || (count > 0 && (!queries || !offsets)) || (capacity > 0 && !shapes))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	bool proceed;
	if (int rc = openCall(s, queries, count, &proceed))
	{
		return rc;
	}
	if (!proceed)
	{
		return S2AMD_OK;
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
	at += roundUp((size_t)count * sizeof(s2amdProximityQuery));
	const size_t masksAt = at;
	at += roundUp(words * sizeof(unsigned long long));
	const size_t prefixAt = at;
	at += roundUp((size_t)count * tiles * sizeof(int));
	const size_t totalsAt = at;
	at += roundUp((size_t)count * sizeof(int));
	const size_t outAt = at; // {offsets[count + 1], entries, their distances}
	const size_t outWords = (size_t)count + 1 + entries + (distances ? entries : 0);
	at += roundUp(outWords * sizeof(int32_t));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	const s2amdProximityQuery* dQueries = (const s2amdProximityQuery*)(base + inAt);
	HIP_TRY(hipMemcpyAsync(base + inAt, queries, (size_t)count * sizeof(s2amdProximityQuery), hipMemcpyHostToDevice, st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	unsigned long long* masks = (unsigned long long*)(base + masksAt);
	int* dOffsets = (int*)(base + outAt);
	int32_t* dEntries = dOffsets + count + 1;
	proximityCandidatesKernel<true><<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(
		(const s2amdShape*)s->dShapes.p, ns, tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity, dQueries, count, masks);
	listTilePrefixKernel<<<dim3((unsigned)((count + 3) / 4)), dim3(S2_BLOCK), 0, st>>>(masks, count, tiles, (int*)(base + prefixAt), (int*)(base + totalsAt));
	listOffsetsKernel<<<dim3(1), dim3(64), 0, st>>>((const int*)(base + totalsAt), count, dOffsets);
	listWriteKernel<<<gridFor(words), dim3(S2_BLOCK), 0, st>>>(masks, words, tiles, (const int*)(base + prefixAt), dOffsets, dEntries, (int)entries);
	if (distances && entries > 0)
	{
		proximityDistancesKernel<<<gridFor(entries), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p,
																			   s->bodyCapacity, dQueries, count, dOffsets, dEntries, (int)entries, (float*)(dEntries + entries));
	}
	HIP_TRY(hipGetLastError());
	s->hQueryStage.resize(outWords);
	HIP_TRY(hipMemcpyAsync(s->hQueryStage.data(), base + outAt, outWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	std::memcpy(offsets, s->hQueryStage.data(), ((size_t)count + 1) * sizeof(int32_t));
	*total = offsets[count];
	if (*total > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "shapes-in-range buffer too small");
	}
	if (*total > 0)
	{
		std::memcpy(shapes, s->hQueryStage.data() + count + 1, (size_t)*total * sizeof(int32_t));
		if (distances)
		{
			std::memcpy(distances, s->hQueryStage.data() + count + 1 + entries, (size_t)*total * sizeof(float));
		}
	}
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop
