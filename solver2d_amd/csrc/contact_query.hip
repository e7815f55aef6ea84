// Contact queries on the resident world (include/solver2d_amd.h: s2amd_world_collide_shape, s2amd_world_deepest_contact): the manifolds
// the reference's nine s2Collide* functions (include/solver2d/manifold.h:56-85, dispatched by s_registers, src/contact.c:139-151) give
// between a caller's shape at a caller's transform and every shape near it, computed from the resident shape, body and origin arrays
// instead of a host copy of the world.  Nothing resident is written; everything is enqueued on the solver's stream behind whatever
// changed the world last.  The results are order-free statements (the header states them), so no traversal order -- and none of the
// optional device trees -- takes part.
//
// The mapping is proximity_query.hip's: a workgroup holds one tile of 256 shape slots -- type, box, category bits and body frame in
// registers -- and walks one chunk of 256 queries; the grid is tiles x chunks.  A query is staged once per call, not once per
// workgroup: contactStageKernel turns it into a shape record of the wire format (so that stagePolygon and refitShapeOne read it as they
// read a world shape) with the box stage 4 would give it; a workgroup keeps the 256 boxes, masks and types of its chunk in LDS (6 KiB:
// what decides "candidate", a broadcast read each) and reads the record itself, through a wave-uniform pointer, for a candidate only.
// The two polygons of a pair live in the lane's LDS columns (manifold_ops.h; 4 x 8 x 256 float2 = 64 KiB per workgroup) because GJK
// and the clipping address them by computed index; no lane reads another's column, so the walk itself has no barrier.
//
//   contactStageKernel               one lane per query: the wire shape record, its frame, the query box (refit_ops.h: refitShapeOne).
//   contactCandidatesKernel<true>    collide shape: per (query, tile, wave) the 64-bit ballot of the candidates (live, category & mask,
//                                    s2AABB_Overlaps(fatAABB, query box), a type pair with a manifold function) whose manifold has
//                                    points; the lists come from query_list.h's listTilePrefixKernel, listOffsetsKernel, listWriteKernel.
//   contactRecordsKernel             one lane per list entry: its query by bisection of the offsets, the manifold again (the same
//                                    operations, so the same bits), the 80-byte record.
//   contactCandidatesKernel<false>   deepest contact: a hit proposes key = orderable(least separation + 0.0f) << 32 | slot by a 64-bit
//                                    integer atomic min: the least key is the least separation as floats compare (-0 is +0), ties to
//                                    the lowest slot, whatever the launch geometry.
//   contactDeepestKernel             one lane per query: the winner's manifold again and the record.
//
// The host side is query_host.h's ("The query facility"): deepest contact is a queryBest, collide shape a queryLists of
// 80-byte records; contactKind names what is staged behind the upload -- the shape records and the frames, by contactStageKernel -- and
// this file supplies the launches of its kernels.
//
// All arithmetic is fp32 in the reference's operation order (manifold_ops.h, gjk_ops.h); this file is compiled without contraction in
// both libraries (Makefile).
#include "solver_internal.h"

#include "refit_ops.h" // (before gjk_ops.h: its transform type is the global one, the query files' own lives in their unnamed namespace)

#include "query_list.h"
#include "query_host.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_SPECULATIVE (4.0f * S2_LINEAR_SLOP) // constants.h:8
#define S2_NP_MAX_VERTS 8
#include "manifold_ops.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdContactQuery) == 160 && sizeof(s2amdContactHit) == 80, "the query records");
static_assert(sizeof(s2amdShape) == 196, "the shape record");

#define S2_CQ_LDS (4 * S2_NP_MAX_VERTS * S2_BLOCK) // vertsA, normsA, vertsB, normsB: one column per lane, 64 KiB

// s_registers[query type][shape type].primary (src/contact.c:143-151) as 16 bits, bit = 4 * query type + shape type: capsule x
// {capsule, circle}; circle x {circle}; polygon x {capsule, circle, polygon}; segment x {capsule, circle, polygon}
#define S2_CQ_PRIMARY 0x7723u

// what a lane keeps of its shape slot
struct LaneShape
{
	bool live;
	int body, type;
	uint32_t category;
	float fat[4];
	Xf xf;
};

S2_DEV LaneShape loadLaneShape(const s2amdShape* shapes, int slot, const s2amdBody* bodies, const float2* origins, int nb)
{
	LaneShape s;
	const s2amdShape* w = shapes + slot;
	s.type = w->type;
	// LIVE; a type outside the four has no manifold function, and a polygon of more than 8 vertices -- no s2Polygon holds one -- would
	// leave its LDS column: neither is ever a candidate
	s.live = s.type >= S2AMD_SHAPE_CAPSULE && s.type <= S2AMD_SHAPE_SEGMENT && !(s.type == S2AMD_SHAPE_POLYGON && w->count > S2_NP_MAX_VERTS);
	s.body = -1;
	s.category = 0u;
	s.fat[0] = s.fat[1] = s.fat[2] = s.fat[3] = 0.0f;
	s.xf.p = v2(0.0f, 0.0f);
	s.xf.q.s = 0.0f, s.xf.q.c = 1.0f;
	if (!s.live)
	{
		return s;
	}
	s.body = w->body;
	s.category = w->categoryBits;
	s.fat[0] = w->fatAABB[0], s.fat[1] = w->fatAABB[1], s.fat[2] = w->fatAABB[2], s.fat[3] = w->fatAABB[3];
	if (s.body >= 0 && s.body < nb) // (s2amd_world_upload refuses a live shape on a body outside the array)
	{
		const float2 o = origins[s.body];
		s.xf.p = v2(o.x, o.y);
		s.xf.q.s = bodies[s.body].rot[0], s.xf.q.c = bodies[s.body].rot[1];
	}
	return s;
}

S2_DEV Xf frameOf(float4 f)
{
	Xf xf;
	xf.p = v2(f.x, f.y);
	xf.q.s = f.z, xf.q.c = f.w;
	return xf;
}

// The query as a shape record of the wire format with the box of stage 4 in `aabb` (src/world.c:286-290), and its frame.
__global__ __launch_bounds__(S2_BLOCK) void contactStageKernel(const s2amdContactQuery* queries, int count, s2amdShape* staged, float4* frames)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const s2amdContactQuery* q = queries + i;
	s2amdShape* sh = staged + i;
	const int type = q->type;
	const int reads = type == S2AMD_SHAPE_POLYGON ? q->count : type == S2AMD_SHAPE_CIRCLE ? 1 : 2;
	sh->body = -1;
	sh->type = type;
	sh->categoryBits = 0u;
	sh->maskBits = q->maskBits;
	sh->groupIndex = 0;
	sh->proxyKey = 0;
	sh->enlarged = 0;
	sh->count = type == S2AMD_SHAPE_POLYGON ? q->count : 0;
	sh->radius = type == S2AMD_SHAPE_SEGMENT ? 0.0f : q->radius;
	for (int k = 0; k < 4; ++k)
	{
		sh->aabb[k] = 0.0f;
		sh->fatAABB[k] = 0.0f;
	}
	for (int k = 0; k < S2_NP_MAX_VERTS; ++k)
	{
		const bool read = k < reads;
		const bool normal = read && type == S2AMD_SHAPE_POLYGON;
		sh->vertices[k][0] = read ? q->vertices[k][0] : 0.0f;
		sh->vertices[k][1] = read ? q->vertices[k][1] : 0.0f;
		sh->normals[k][0] = normal ? q->normals[k][0] : 0.0f;
		sh->normals[k][1] = normal ? q->normals[k][1] : 0.0f;
	}
	Rot rot;
	rot.s = q->rot[0], rot.c = q->rot[1];
	(void)refitShapeOne(rot, sh, v2(q->position[0], q->position[1]));
	frames[i] = make_float4(q->position[0], q->position[1], q->rot[0], q->rot[1]);
}

// the manifold function of the ordered type pair (src/contact.c:139-151) with an empty distance cache; lds: the block's S2_CQ_LDS float2
S2_DEV Manifold manifoldOf(const s2amdShape* shapeA, Xf xfA, const s2amdShape* shapeB, Xf xfB, float2* lds)
{
	Cache cache;
	cache.metric = 0.0f;
	cache.count = 0;
	for (int k = 0; k < 3; ++k)
	{
		cache.indexA[k] = 0;
		cache.indexB[k] = 0;
	}
	const int ta = shapeA->type, tb = shapeB->type;
	Manifold m = emptyManifold();
	PolyRef pa, pb;
	pa.verts = lds + threadIdx.x;
	pa.norms = lds + S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	pb.verts = lds + 2 * S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	pb.norms = lds + 3 * S2_NP_MAX_VERTS * S2_NP_BLOCK + threadIdx.x;
	const V2 a0 = v2(shapeA->vertices[0][0], shapeA->vertices[0][1]), a1 = v2(shapeA->vertices[1][0], shapeA->vertices[1][1]);
	const V2 b0 = v2(shapeB->vertices[0][0], shapeB->vertices[0][1]);
	if (tb == S2AMD_SHAPE_CIRCLE)
	{
		if (ta == S2AMD_SHAPE_CIRCLE)
		{
			m = collideCircles(a0, shapeA->radius, xfA, b0, shapeB->radius, xfB);
		}
		else if (ta == S2AMD_SHAPE_CAPSULE || ta == S2AMD_SHAPE_SEGMENT)
		{
			m = collideCapsuleAndCircle(a0, a1, ta == S2AMD_SHAPE_CAPSULE ? shapeA->radius : 0.0f, xfA, b0, shapeB->radius, xfB);
		}
		else if (ta == S2AMD_SHAPE_POLYGON)
		{
			stagePolygon(shapeA, pa, false, xfA, &pa.radius, &pa.count);
			m = collidePolygonAndCircle(pa, xfA, b0, shapeB->radius, xfB);
		}
	}
	else if ((ta == S2AMD_SHAPE_CAPSULE && tb == S2AMD_SHAPE_CAPSULE) || (ta == S2AMD_SHAPE_POLYGON && tb == S2AMD_SHAPE_CAPSULE) ||
			 (ta == S2AMD_SHAPE_POLYGON && tb == S2AMD_SHAPE_POLYGON) || (ta == S2AMD_SHAPE_SEGMENT && tb == S2AMD_SHAPE_CAPSULE) ||
			 (ta == S2AMD_SHAPE_SEGMENT && tb == S2AMD_SHAPE_POLYGON))
	{
		Xf xf = xfInvMul(xfA, xfB);
		stagePolygon(shapeA, pa, false, xf, &pa.radius, &pa.count);
		stagePolygon(shapeB, pb, true, xf, &pb.radius, &pb.count);
		m = collidePolygons(pa, xfA, pb, xf, cache);
	}
	return m;
}

// M(q, s): shape A is the query where the pair's register entry is primary, the world shape otherwise (s2CreateContact's flip)
S2_DEV Manifold queryManifold(const s2amdShape* q, Xf xfQ, const s2amdShape* w, Xf xfW, int worldType, float2* lds, bool* queryIsB)
{
	const bool primary = ((S2_CQ_PRIMARY >> (4 * q->type + worldType)) & 1u) != 0u;
	*queryIsB = !primary;
	return manifoldOf(primary ? q : w, primary ? xfQ : xfW, primary ? w : q, primary ? xfW : xfQ, lds);
}

// live, passing, boxes overlapping, a pair with a manifold function
S2_DEV bool isCandidate(const LaneShape& s, float4 box, uint32_t maskBits, int queryType)
{
	return s.live && (s.category & maskBits) != 0u && boxesOverlap(s.fat, box.x, box.y, box.z, box.w) &&
		   !(queryType == S2AMD_SHAPE_SEGMENT && s.type == S2AMD_SHAPE_SEGMENT);
}

// the monotone map of the float order onto the unsigned order, of f + 0.0f: -0 and +0 give one key
S2_DEV uint32_t orderable(float f)
{
	const uint32_t u = asBits(f + 0.0f);
	return (u & 0x80000000u) != 0u ? ~u : (u | 0x80000000u);
}

struct alignas(16) HitRecord
{
	float4 w[5];
};
static_assert(sizeof(HitRecord) == sizeof(s2amdContactHit), "the hit record as the finish passes store it");

S2_DEV float4 bits4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return make_float4(fromBits(a), fromBits(b), fromBits(c), fromBits(d)); }

S2_DEV void storeHit(HitRecord* out, int slot, int body, const Manifold& m, bool queryIsB)
{
	const MPoint p0 = m.points[0];
	const bool two = m.pointCount > 1;
	const MPoint p1 = m.points[1];
	out->w[0] = bits4((uint32_t)slot, (uint32_t)body, (uint32_t)m.pointCount, queryIsB ? 1u : 0u);
	out->w[1] = make_float4(m.normal.x, m.normal.y, p0.localAnchorA.x, p0.localAnchorA.y);
	out->w[2] = make_float4(p0.localAnchorB.x, p0.localAnchorB.y, p0.separation, fromBits(p0.id));
	out->w[3] = two ? make_float4(p1.localAnchorA.x, p1.localAnchorA.y, p1.localAnchorB.x, p1.localAnchorB.y) : bits4(0u, 0u, 0u, 0u);
	out->w[4] = two ? make_float4(p1.separation, fromBits(p1.id), 0.0f, 0.0f) : bits4(0u, 0u, 0u, 0u);
}

S2_DEV void storeNoHit(HitRecord* out)
{
	out->w[0] = bits4(0xffffffffu, 0xffffffffu, 0u, 0u);
	out->w[1] = out->w[2] = out->w[3] = out->w[4] = bits4(0u, 0u, 0u, 0u);
}

// LIST: masks[((query * tiles) + tile) * 4 + wave] = the wave's hits of the query, bit = lane; every word is written.
// Otherwise keys[query] takes the least orderable(separation) << 32 | slot.
template <bool LIST>
__global__ __launch_bounds__(S2_BLOCK) void contactCandidatesKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, const float2* origins, int nb,
																	 const s2amdShape* staged, const float4* frames, int count, unsigned long long* out)
{
	__shared__ float2 lds[S2_CQ_LDS];
	__shared__ float4 boxes[S2_QUERY_CHUNK]; // what decides "candidate" for all but a few (query, slot) pairs: a broadcast read each
	__shared__ uint2 filters[S2_QUERY_CHUNK]; // {maskBits, type}
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		const s2amdShape* q = staged + first + (int)threadIdx.x;
		boxes[threadIdx.x] = make_float4(q->aabb[0], q->aabb[1], q->aabb[2], q->aabb[3]);
		filters[threadIdx.x] = make_uint2(q->maskBits, (uint32_t)q->type);
	}
	LaneShape s;
	s.live = false;
	s.type = S2AMD_SHAPE_FREE;
	if (slot < n)
	{
		s = loadLaneShape(shapes, slot, bodies, origins, nb);
	}
	__syncthreads();
	if (!LIST && !s.live)
	{
		return;
	}
	const s2amdShape* w = shapes + (s.live ? slot : 0);
	for (int k = 0; k < chunk; ++k)
	{
		const s2amdShape* q = staged + first + k;
		const float4 box = boxes[k];
		const uint2 filter = filters[k];
		bool hit = false;
		float least = 0.0f;
		if (isCandidate(s, box, filter.x, (int)filter.y))
		{
			bool queryIsB;
			const Manifold m = queryManifold(q, frameOf(frames[first + k]), w, s.xf, s.type, lds, &queryIsB);
			hit = m.pointCount > 0;
			least = m.points[0].separation;
			if (m.pointCount > 1 && m.points[1].separation < least)
			{
				least = m.points[1].separation;
			}
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
			atomicMin(out + first + k, ((unsigned long long)orderable(least) << 32) | (unsigned long long)(uint32_t)slot);
		}
	}
}

// one lane's record: M(q, slot) again
S2_DEV void recordOf(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const s2amdShape* q, Xf xfQ, int slot, float2* lds,
					 HitRecord* out)
{
	if (slot >= 0 && slot < n)
	{
		const LaneShape s = loadLaneShape(shapes, slot, bodies, origins, nb);
		if (s.live && !(q->type == S2AMD_SHAPE_SEGMENT && s.type == S2AMD_SHAPE_SEGMENT))
		{
			bool queryIsB;
			const Manifold m = queryManifold(q, xfQ, shapes + slot, s.xf, s.type, lds, &queryIsB);
			if (m.pointCount > 0)
			{
				storeHit(out, slot, s.body, m, queryIsB);
				return;
			}
		}
	}
	storeNoHit(out);
}

__global__ __launch_bounds__(S2_BLOCK) void contactDeepestKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																  const s2amdShape* staged, const float4* frames, int count, const unsigned long long* keys, HitRecord* hits)
{
	__shared__ float2 lds[S2_CQ_LDS];
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const unsigned long long key = keys[i];
	const int slot = keySlot(key);
	recordOf(shapes, n, bodies, origins, nb, staged + i, frameOf(frames[i]), slot, lds, hits + i);
}

// hits[e] for the entries the list holds: e < min(offsets[count], capacity).  The entry's query is the last one whose offset is <= e.
__global__ __launch_bounds__(S2_BLOCK) void contactRecordsKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																  const s2amdShape* staged, const float4* frames, int count, const int* offsets, const int32_t* entries,
																  int capacity, HitRecord* hits)
{
	__shared__ float2 lds[S2_CQ_LDS];
	const int e = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (e >= capacity || e >= offsets[count])
	{
		return;
	}
	const int lo = entryQuery(offsets, count, e);
	recordOf(shapes, n, bodies, origins, nb, staged + lo, frameOf(frames[lo]), entries[e], lds, hits + e);
}

bool finite2(const float* v)
{
	return std::isfinite(v[0]) && std::isfinite(v[1]);
}

bool validQuery(const void* record)
{
	const s2amdContactQuery& q = *(const s2amdContactQuery*)record;
	if (q.type != S2AMD_SHAPE_CAPSULE && q.type != S2AMD_SHAPE_CIRCLE && q.type != S2AMD_SHAPE_POLYGON && q.type != S2AMD_SHAPE_SEGMENT)
	{
		return false;
	}
	if (q.type == S2AMD_SHAPE_POLYGON && (q.count < 3 || q.count > S2_NP_MAX_VERTS))
	{
		return false;
	}
	const int reads = q.type == S2AMD_SHAPE_POLYGON ? q.count : q.type == S2AMD_SHAPE_CIRCLE ? 1 : 2;
	bool ok = finite2(q.position) && finite2(q.rot);
	for (int i = 0; i < reads; ++i)
	{
		ok = ok && finite2(q.vertices[i]) && (q.type != S2AMD_SHAPE_POLYGON || finite2(q.normals[i]));
	}
	if (q.type != S2AMD_SHAPE_SEGMENT)
	{
		ok = ok && std::isfinite(q.radius) && q.radius >= 0.0f;
	}
	return ok;
}

// ---- the launches query_host.h's drivers ask for ----
// staged behind the upload: the queries' shape records (staged[0]) and their frames (staged[1])
void launchStage(const QueryCall& c)
{
	contactStageKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>((const s2amdContactQuery*)c.records, c.count, (s2amdShape*)c.staged[0], (float4*)c.staged[1]);
}

template <bool LIST> void launchCandidates(const QueryCall& c, unsigned long long* out)
{
	contactCandidatesKernel<LIST><<<c.grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.tiles, c.bodies, c.origins, c.nb, (const s2amdShape*)c.staged[0],
																			(const float4*)c.staged[1], c.count, out);
}

void launchDeepest(const QueryCall& c, const unsigned long long* keys, void* hits)
{
	contactDeepestKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdShape*)c.staged[0],
																					 (const float4*)c.staged[1], c.count, keys, (HitRecord*)hits);
}

void launchRecords(const QueryCall& c, const int* offsets, const int32_t* slots, int capacity, void* hits)
{
	contactRecordsKernel<<<gridFor((size_t)capacity), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdShape*)c.staged[0],
																					  (const float4*)c.staged[1], c.count, offsets, slots, capacity, (HitRecord*)hits);
}

const QueryKind contactKind = {sizeof(s2amdContactQuery),
							   "queries",
							   validQuery,
							   "contact query",
							   "is invalid (a type outside the four, a polygon count outside 3..8, a NaN or infinite field, a negative radius)",
							   {sizeof(s2amdShape), sizeof(float4)},
							   launchStage};

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_deepest_contact(s2amdSolver* s, const s2amdContactQuery* queries, int32_t count, s2amdContactHit* hits)
{
	return queryBest(s, contactKind, queries, count, hits, sizeof(s2amdContactHit), launchCandidates<false>, launchDeepest);
}

int s2amd_world_collide_shape(s2amdSolver* s, const s2amdContactQuery* queries, int32_t count, int32_t* offsets, s2amdContactHit* hits, int32_t capacity, int32_t* total)
{
	const QueryPayload records = {sizeof(s2amdContactHit), "collide-shape buffer too small", launchRecords};
	return queryLists(s, contactKind, queries, count, offsets, hits, nullptr, capacity, total, records, launchCandidates<true>);
}

} // extern "C"
#pragma GCC visibility pop
