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

static_assert(sizeof(s2amdShapeCast) == 112 && sizeof(s2amdShapeCastHit) == 48 && sizeof(s2amdShapeCast) % 16 == 0, "the cast records");

#define S2_NO_HIT_KEY 0xffffffffffffffffull
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
	const int slot = key == S2_NO_HIT_KEY ? -1 : (int)(uint32_t)(key & 0xffffffffull);
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
	hits[e] = recordOf(shapes, n, bodies, origins, nb, casts + lo, entries[e]);
}

bool validCast(const s2amdShapeCast& c)
{
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

// what both calls check before anything is enqueued; *proceed is false when the call has already been answered
int openCall(s2amdSolver* s, const s2amdShapeCast* casts, int32_t count, bool* proceed)
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
		return fail(S2AMD_E_INVALID, "more casts than one call takes: split the batch");
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validCast(casts[i]))
		{
			return fail(S2AMD_E_INVALID, "shape cast " + std::to_string(i) +
											 " is invalid (count outside 1..8, a NaN or infinite field, a negative radius or maxFraction)");
		}
	}
	*proceed = true;
	return S2AMD_OK;
}

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_cast_shape(s2amdSolver* s, const s2amdShapeCast* casts, int32_t count, s2amdShapeCastHit* hits)
{
	if (!s || count < 0 || (count > 0 && (!casts || !hits)))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	bool proceed;
	if (int rc = openCall(s, casts, count, &proceed))
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
	at += roundUp((size_t)count * sizeof(s2amdShapeCast));
	const size_t keysAt = at;
	at += roundUp((size_t)count * sizeof(unsigned long long));
	const size_t hitsAt = at;
	at += roundUp((size_t)count * sizeof(s2amdShapeCastHit));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	const s2amdShapeCast* dCasts = (const s2amdShapeCast*)(base + inAt);
	unsigned long long* keys = (unsigned long long*)(base + keysAt);
	HIP_TRY(hipMemcpyAsync(base + inAt, casts, (size_t)count * sizeof(s2amdShapeCast), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)count * sizeof(unsigned long long), st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	if (tiles > 0)
	{
		castCandidatesKernel<false><<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(
			(const s2amdShape*)s->dShapes.p, ns, tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity, dCasts, count, keys);
	}
	castFinishKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p,
																		 s->bodyCapacity, dCasts, count, keys, (HitRecord*)(base + hitsAt));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hits, base + hitsAt, (size_t)count * sizeof(s2amdShapeCastHit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return S2AMD_OK;
}

// upload, the mask pass, query_list.h's three, the records; the offsets come back, then the records they count
int s2amd_world_cast_shape_all(s2amdSolver* s, const s2amdShapeCast* casts, int32_t count, int32_t* offsets, s2amdShapeCastHit* hits, int32_t capacity, int32_t* total)
{
	if (!s || count < 0 || capacity < 0 || !total || (count > 0 && (!casts || !offsets)) || (capacity > 0 && !hits))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	bool proceed;
	if (int rc = openCall(s, casts, count, &proceed))
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
		return fail(S2AMD_E_INVALID, "casts x shape slots beyond 2^31: split the batch");
	}
	// no list is longer than the shape slots, nor all together than the caller's capacity
	const size_t entries = std::min((size_t)capacity, (size_t)count * (size_t)ns);
	size_t at = 0;
	const size_t inAt = at;
	at += roundUp((size_t)count * sizeof(s2amdShapeCast));
	const size_t masksAt = at;
	at += roundUp(words * sizeof(unsigned long long));
	const size_t prefixAt = at;
	at += roundUp((size_t)count * tiles * sizeof(int));
	const size_t totalsAt = at;
	at += roundUp((size_t)count * sizeof(int));
	const size_t slotsAt = at;
	at += roundUp(entries * sizeof(int32_t));
	const size_t outAt = at; // {offsets[count + 1], padding to 16 bytes, records}
	const size_t recordsIn = (((size_t)count + 1) * sizeof(int32_t) + 15) & ~size_t(15);
	at += roundUp(recordsIn + entries * sizeof(s2amdShapeCastHit));
	HIP_TRY(hipSetDevice(s->device));
	if (int rc = s->dQuery.ensure(at))
	{
		return rc;
	}
	char* base = (char*)s->dQuery.p;
	hipStream_t st = s->stream;
	const s2amdShapeCast* dCasts = (const s2amdShapeCast*)(base + inAt);
	HIP_TRY(hipMemcpyAsync(base + inAt, casts, (size_t)count * sizeof(s2amdShapeCast), hipMemcpyHostToDevice, st));
	const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	unsigned long long* masks = (unsigned long long*)(base + masksAt);
	int* dOffsets = (int*)(base + outAt);
	int32_t* dSlots = (int32_t*)(base + slotsAt);
	castCandidatesKernel<true><<<dim3((unsigned)tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(
		(const s2amdShape*)s->dShapes.p, ns, tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity, dCasts, count, masks);
	listTilePrefixKernel<<<dim3((unsigned)((count + 3) / 4)), dim3(S2_BLOCK), 0, st>>>(masks, count, tiles, (int*)(base + prefixAt), (int*)(base + totalsAt));
	listOffsetsKernel<<<dim3(1), dim3(64), 0, st>>>((const int*)(base + totalsAt), count, dOffsets);
	listWriteKernel<<<gridFor(words), dim3(S2_BLOCK), 0, st>>>(masks, words, tiles, (const int*)(base + prefixAt), dOffsets, dSlots, (int)entries);
	if (entries > 0)
	{
		castRecordsKernel<<<gridFor(entries), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p,
																		s->bodyCapacity, dCasts, count, dOffsets, dSlots, (int)entries, (HitRecord*)(base + outAt + recordsIn));
	}
	HIP_TRY(hipGetLastError());
	// the offsets first: a record is 48 bytes, and only offsets[count] of the `entries` the caller has room for exist
	HIP_TRY(hipMemcpyAsync(offsets, base + outAt, ((size_t)count + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	*total = offsets[count];
	if (*total > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "cast-shape buffer too small");
	}
	if (*total > 0)
	{
		HIP_TRY(hipMemcpyAsync(hits, base + outAt + recordsIn, (size_t)*total * sizeof(s2amdShapeCastHit), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	return S2AMD_OK;
}

} // extern "C"
#pragma GCC visibility pop
