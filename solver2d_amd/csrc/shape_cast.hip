// Shape casts on the resident world (include/solver2d_amd.h: s2amd_world_cast_shape, s2amd_world_cast_shape_all): a caller's proxy swept
// along a vector against every shape near its path by conservative advancement, every distance of which is s2ShapeDistance
// (src/distance.c:485-636) over the proxies of s2Shape_MakeDistanceProxy (src/shape.c:75-93), computed from the resident shape, body and
// origin arrays.  Nothing resident is written; everything is enqueued on the solver's stream behind whatever changed the world last.  The
// results are order-free statements (the header states them), so no traversal order -- and none of the optional device trees -- takes part.
//
// The mapping is proximity_query.hip's: a workgroup holds one tile of 256 shape slots -- box, category bits, body frame, radius and vertex
// count in registers, the up-to-8 proxy vertices in the lane's LDS column because GJK addresses them by computed index -- and walks one
// chunk of 256 casts staged in LDS as they came (112 bytes each, 28 KiB) with their swept boxes beside them (4 KiB), every cast a
// broadcast read.  The grid is tiles x chunks.
//
//   castCandidatesKernel<false>  first hit: a candidate (live, category & mask, s2AABB_Overlaps(fatAABB, swept box)) runs the advancement;
//                                one that hits proposes key = fraction bits << 32 | slot by a 64-bit integer atomic min (fractions are
//                                >= +0: the bits order as the values).  The least key is the least fraction, ties to the lowest slot,
//                                whatever the launch geometry.
//   castFinishKernel             one lane per cast: the winner's advancement again (the same operations, so the same bits) and the record.
//   castCandidatesKernel<true>   all hits: per (cast, tile, wave) the 64-bit ballot of the candidates that hit; the lists come from
//                                query_list.h's listTilePrefixKernel, listOffsetsKernel and listWriteKernel.
//   castRecordsKernel            one lane per list entry: its cast by bisection of the offsets, the advancement again, the record.
//
// The host side is query_host.h's ("The query facility"): cast shape is a queryBest, cast shape all a queryLists of 48-byte
// records; this file supplies castKind and the launches of its kernels.  The swept box and the advancement are cast_ops.h's, which
// mover_query.hip shares.
//
// All arithmetic is fp32 in the reference's operation order (gjk_ops.h); this file is compiled without contraction in both libraries
// (Makefile).
#include "query_list.h"
#include "query_host.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "gjk_ops.h"
#include "proxy_ops.h"
#include "cast_ops.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdShapeCast) == 112 && sizeof(s2amdShapeCastHit) == 48 && sizeof(s2amdShapeCast) % 16 == 0, "the cast records");

struct alignas(16) HitRecord
{
	float4 a, b, c;
};
static_assert(sizeof(HitRecord) == sizeof(s2amdShapeCastHit), "the hit record as the finish passes store it");

// the record of cast `c` against slot `slot`: the advancement again, one lane, both proxies read where the arrays hold them.  A slot
// that does not hit (-1: no winner) leaves the no-hit record.
S2_DEV HitRecord recordOf(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const s2amdShapeCast* c, int slot)
{
	HitRecord rec;
	rec.a = make_float4(__int_as_float(-1), __int_as_float(-1), c->maxFraction, 0.0f);
	rec.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	rec.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (slot < 0 || slot >= n)
	{
		return rec;
	}
	const LaneProxy s = loadProxy(shapes, slot, bodies, origins, nb);
	if (!s.live)
	{
		return rec;
	}
	const CastOutcome o = castAgainst(c, slotProxy(shapes, slot, s), s.xf);
	if (o.hit)
	{
		const V2 normal = normalize(sub(o.d.pointA, o.d.pointB));
		rec.a = make_float4(__int_as_float(slot), __int_as_float(s.body), o.fraction, o.d.distance);
		rec.b = make_float4(o.d.pointB.x, o.d.pointB.y, normal.x, normal.y);
		rec.c.x = __int_as_float(o.advances);
	}
	return rec;
}

// LIST: masks[((cast * tiles) + tile) * 4 + wave] = the wave's shapes the cast hits, bit = lane; every word is written.
// Otherwise keys[cast] takes the least fraction bits << 32 | slot.
template <bool LIST>
__global__ __launch_bounds__(S2_BLOCK) void castCandidatesKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, const float2* origins, int nb,
																 const s2amdShapeCast* casts, int count, unsigned long long* out)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ alignas(16) s2amdShapeCast staged[S2_QUERY_CHUNK];
	__shared__ float4 boxes[S2_QUERY_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		// (seven 16-byte words straight into LDS: a copy in registers would be indexed by the box's vertex loop, and go to scratch)
		const float4* from = (const float4*)(casts + first + (int)threadIdx.x);
		float4* to = (float4*)(staged + threadIdx.x);
		for (int j = 0; j < (int)(sizeof(s2amdShapeCast) / sizeof(float4)); ++j)
		{
			to[j] = from[j];
		}
		boxes[threadIdx.x] = sweptBox(staged[threadIdx.x]);
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
		const s2amdShapeCast* c = staged + k;
		const float4 box = boxes[k];
		bool hit = false;
		float fraction = 0.0f;
		if (s.live && (s.category & c->maskBits) != 0u && boxesOverlap(s.fat, box.x, box.y, box.z, box.w))
		{
			const CastOutcome o = castAgainst(c, B, s.xf);
			hit = o.hit, fraction = o.fraction;
		}
		if (LIST)
		{
			const unsigned long long ballot = __ballot(hit);
			if (lane == 0)
			{
				out[((size_t)(first + k) * tiles + blockIdx.x) * 4 + wave] = ballot;
			}
		}
		else if (hit)
		{
			atomicMin(out + first + k, ((unsigned long long)asBits(fraction) << 32) | (unsigned long long)(uint32_t)slot);
		}
	}
}

__global__ __launch_bounds__(S2_BLOCK) void castFinishKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
															 const s2amdShapeCast* casts, int count, const unsigned long long* keys, HitRecord* hits)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const unsigned long long key = keys[i];
	const int slot = keySlot(key);
	hits[i] = recordOf(shapes, n, bodies, origins, nb, casts + i, slot);
}

// hits[e] for the entries the list holds: e < min(offsets[count], capacity).  The entry's cast is the last one whose offset is <= e.
__global__ __launch_bounds__(S2_BLOCK) void castRecordsKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
															  const s2amdShapeCast* casts, int count, const int* offsets, const int32_t* entries, int capacity,
															  HitRecord* hits)
{
	const int e = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (e >= capacity || e >= offsets[count])
	{
		return;
	}
	const int lo = entryQuery(offsets, count, e);
	hits[e] = recordOf(shapes, n, bodies, origins, nb, casts + lo, entries[e]);
}

bool validCast(const void* record)
{
	const s2amdShapeCast& c = *(const s2amdShapeCast*)record;
	if (c.count < 1 || c.count > S2_NP_MAX_VERTS)
	{
		return false;
	}
	bool finite = std::isfinite(c.radius) && std::isfinite(c.maxFraction) && std::isfinite(c.position[0]) && std::isfinite(c.position[1]) &&
				  std::isfinite(c.rot[0]) && std::isfinite(c.rot[1]) && std::isfinite(c.translation[0]) && std::isfinite(c.translation[1]);
	for (int i = 0; i < c.count; ++i)
	{
		finite = finite && std::isfinite(c.vertices[i][0]) && std::isfinite(c.vertices[i][1]);
	}
	return finite && c.radius >= 0.0f && c.maxFraction >= 0.0f;
}

const QueryKind castKind = {sizeof(s2amdShapeCast), "casts", validCast, "shape cast", "is invalid (count outside 1..8, a NaN or infinite field, a negative radius or maxFraction)",
							{0, 0}, nullptr};

// ---- the launches query_host.h's drivers ask for ----
template <bool LIST> void launchCandidates(const QueryCall& c, unsigned long long* out)
{
	castCandidatesKernel<LIST><<<c.grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.tiles, c.bodies, c.origins, c.nb, (const s2amdShapeCast*)c.records, c.count, out);
}

void launchFinish(const QueryCall& c, const unsigned long long* keys, void* hits)
{
	castFinishKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdShapeCast*)c.records, c.count, keys,
																				 (HitRecord*)hits);
}

void launchRecords(const QueryCall& c, const int* offsets, const int32_t* slots, int capacity, void* hits)
{
	castRecordsKernel<<<gridFor((size_t)capacity), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdShapeCast*)c.records, c.count, offsets,
																				   slots, capacity, (HitRecord*)hits);
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_cast_shape(s2amdSolver* s, const s2amdShapeCast* casts, int32_t count, s2amdShapeCastHit* hits)
{
	return queryBest(s, castKind, casts, count, hits, sizeof(s2amdShapeCastHit), launchCandidates<false>, launchFinish);
}

int s2amd_world_cast_shape_all(s2amdSolver* s, const s2amdShapeCast* casts, int32_t count, int32_t* offsets, s2amdShapeCastHit* hits, int32_t capacity, int32_t* total)
{
	const QueryPayload records = {sizeof(s2amdShapeCastHit), "cast-shape buffer too small", launchRecords};
	return queryLists(s, castKind, casts, count, offsets, hits, nullptr, capacity, total, records, launchCandidates<true>);
}

} // extern "C"
#pragma GCC visibility pop
