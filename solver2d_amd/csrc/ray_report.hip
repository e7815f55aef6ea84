// Ray report of the resident world (include/solver2d_amd.h: s2amd_world_set_ray_sensors, s2amd_world_set_ray_report and the four
// getters): a list of up to 16,384 rays, fixed in the world or mounted on bodies, cast behind every s2amd_world_step -- what a caller
// otherwise composes per step from a pose download, the host's own s2TransformPoint on both ends and s2amd_world_ray_cast.  The answer
// of a ray is that call's statement (scene_query.hip) with two further exclusions from the candidates: the shapes of the ray's own
// body, and with SKIP_STATIC the shapes on static bodies.  The passes are enqueued behind stage 4 of s2amd_world_step and behind the
// other six reports, once per step (a repeated step reports once); the report owns its "before" state on the device.
//
//   rayPoseKernel              one lane per ray: active (liveBody, finiteBits), the world ends (xfPoint(xf(body), p) for a mounted ray), the segment box, the
//                              excluded body, staged as one 48-byte record; the ray's key set to the no-hit key.  Per group of 64 rays
//                              (a wave here: one fan of 64) the union of the segment boxes of the group's active rays, reduced by wave
//                              shuffles: the group box.  A group without an active ray is marked empty; one with a box that is not
//                              finite takes every tile (the box test of such a ray is s2AABB_Overlaps's own, which a NaN passes).
//   rayReportCandidatesKernel  scene_query.hip's mapping: a workgroup holds one tile of 256 shape slots, a polygon's vertices and normals
//                              in the lane's LDS column, and walks one group of 64 posed rays staged in LDS (3 KiB), every ray a
//                              broadcast read.  The grid is tiles x groups.  Before anything is staged a lane reads 24 bytes of its
//                              slot and tests its fat box against the group box: a workgroup in which no lane overlaps returns (rays of
//                              one fan are neighbours in space, so most workgroups end here), and of the workgroups that stay, a wave
//                              without an overlapping lane returns behind the one barrier.  Overlapping the union box is necessary for
//                              overlapping a member's box, so this decides no result.  A hit proposes (ordered bits of its fraction)
//                              << 32 | slot by a 64-bit integer atomic min.  (A wave casts the rays it is a candidate of one after the
//                              other, about a microsecond each: with 256 rays to a workgroup that chain, not the number of workgroups,
//                              set the kernel's time -- DESIGN.md section 6a has the three mappings as measured.)
//   rayReportFinishKernel      one lane per ray: the winner's exact test again (the same operations on the same staged ends, so the same
//                              bits), the 64-byte state, the range, shapeNow into the ping-pong "before" array, and per wave the ballot of
//                              the rays whose hit shape changed.  <true>: "before" only -- shapeNow alone.
//   rayReportEventsKernel      one workgroup per chunk: the prefix over the at most 256 ballot words (64 chunks x 4 waves) in LDS, then
//                              each changed ray's record at its rank: ascending by ray, no sort, no atomic.
//
// No float atomics, no scratch.  LaneShape, loadShape, rayCastShape and orderedFractionBits are private copies of scene_query.hip's (its
// kernels stay as they were, instruction for instruction).  All arithmetic is fp32 in the reference's operation order (query_ops.h,
// gjk_ops.h); this file is compiled without contraction in both libraries (Makefile).  All device memory is one block sized by
// rayReportPrepare; a step allocates nothing and waits for nothing -- the getters do.
#include "query_list.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "query_ops.h"
#include "mount_ops.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdRaySensor) == 48 && sizeof(s2amdRayState) == 64 && sizeof(s2amdRayEvent) == 16, "the report's records");
static_assert(sizeof(s2amdShape) == 196, "the shape record");
static_assert(S2AMD_MAX_RAY_SENSORS <= 64 * S2_QUERY_CHUNK, "the events pass holds every ballot word of the list in one workgroup's lanes");

#define S2_RAY_SENSOR_KNOWN_FLAGS (S2AMD_RAY_SENSOR_DISABLED | S2AMD_RAY_SENSOR_SKIP_STATIC)
#define S2_RAY_REPORT_KNOWN (S2AMD_RAY_REPORT_STATES | S2AMD_RAY_REPORT_RANGES | S2AMD_RAY_REPORT_EVENTS)

// a ray as the candidates pass stages it: the world ends, the rule's fields, the segment box (src/dynamic_tree.c:1231-1238)
struct alignas(16) PosedRay
{
	float p1x, p1y, p2x, p2y;
	float maxFraction;
	uint32_t mask;
	int32_t body; // the ray's own (< 0: fixed in the world, nothing excluded)
	int32_t bits; // 1: active, 2: SKIP_STATIC
	float lx, ly, ux, uy;
};
static_assert(sizeof(PosedRay) == 48, "three 16-byte words per staged ray");

// the union of the segment boxes of the active rays of a group of 64 (one wave of the pose pass, one workgroup of the candidates pass:
// one fan of 64); any == 0: no active ray, any == 2: a box that is not finite (no pruning)
#define S2_RAY_GROUP 64
#define S2_RAY_GROUPS (S2_QUERY_CHUNK / S2_RAY_GROUP)
struct alignas(16) GroupBox
{
	float lx, ly, ux, uy;
	int32_t any, pad[3];
};
static_assert(S2_RAY_GROUPS == S2_BLOCK / 64 && sizeof(GroupBox) == 32, "a group is a wave of the pose pass");

struct RayLayout
{
	size_t rays, posed, boxes, keys, states, ranges, shapes[2], words, head, events, total;
	int chunks;
};

// shapes[0], shapes[1]: the hit shape per ray, now / before, ping-pong
RayLayout rayLayout(int count)
{
	RayLayout l{};
	size_t at = 0;
	l.chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
	l.rays = reportTake(at, (size_t)count * sizeof(s2amdRaySensor));
	l.posed = reportTake(at, (size_t)count * sizeof(PosedRay));
	l.boxes = reportTake(at, (size_t)l.chunks * S2_RAY_GROUPS * sizeof(GroupBox));
	l.keys = reportTake(at, (size_t)count * sizeof(unsigned long long));
	l.states = reportTake(at, (size_t)count * sizeof(s2amdRayState));
	l.ranges = reportTake(at, (size_t)count * sizeof(float));
	l.shapes[0] = reportTake(at, (size_t)count * sizeof(int32_t));
	l.shapes[1] = reportTake(at, (size_t)count * sizeof(int32_t));
	l.words = reportTake(at, (size_t)l.chunks * 4 * sizeof(unsigned long long));
	l.head = reportTake(at, 4 * sizeof(int32_t));
	l.events = reportTake(at, (size_t)count * sizeof(s2amdRayEvent));
	l.total = at;
	return l;
}

// posed[i], keys[i] = the no-hit key, and boxes[blockIdx.x * 4 + wave]
__global__ __launch_bounds__(S2_BLOCK) void rayPoseKernel(const s2amdRaySensor* rays, int count, const s2amdBody* bodies, const float2* origins, int nb, PosedRay* posed,
														  unsigned long long* keys, GroupBox* boxes)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	bool active = false;
	float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (i < count)
	{
		const s2amdRaySensor* q = rays + i;
		const int body = q->body, flags = q->flags;
		const float maxFraction = q->maxFraction;
		V2 p1 = v2(q->p1[0], q->p1[1]), p2 = v2(q->p2[0], q->p2[1]);
		active = (flags & S2AMD_RAY_SENSOR_DISABLED) == 0;
		if (active && body >= 0)
		{
			active = liveBody(bodies, nb, body);
			if (active)
			{
				Xf xf;
				const float2 o = origins[body];
				xf.p = v2(o.x, o.y);
				xf.q.s = bodies[body].rot[0], xf.q.c = bodies[body].rot[1];
				p1 = xfPoint(xf, p1);
				p2 = xfPoint(xf, p2);
			}
		}
		// s2IsValidRay on the world ray (maxFraction is the setter's)
		active = active && finiteBits(p1.x) && finiteBits(p1.y) && finiteBits(p2.x) && finiteBits(p2.y);
		if (active)
		{
			const V2 t = mulAdd(p1, maxFraction, sub(p2, p1));
			box = make_float4(S2_MINF(p1.x, t.x), S2_MINF(p1.y, t.y), S2_MAXF(p1.x, t.x), S2_MAXF(p1.y, t.y));
		}
		else
		{
			p1 = p2 = v2(0.0f, 0.0f);
		}
		float4* to = (float4*)(posed + i);
		to[0] = make_float4(p1.x, p1.y, p2.x, p2.y);
		to[1] = make_float4(maxFraction, __uint_as_float(q->maskBits), __int_as_float(body),
							__int_as_float((active ? 1 : 0) | ((flags & S2AMD_RAY_SENSOR_SKIP_STATIC) != 0 ? 2 : 0)));
		to[2] = box;
		keys[i] = S2_QUERY_NO_KEY;
	}
	// the group's box: 1 = an active ray, 2 = one whose box is not finite
	int any = !active ? 0 : finiteBits(box.x) && finiteBits(box.y) && finiteBits(box.z) && finiteBits(box.w) ? 1 : 2;
	if (any != 1)
	{
		box = make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
	}
	for (int d = 32; d > 0; d >>= 1)
	{
		const float lx = __shfl_xor(box.x, d), ly = __shfl_xor(box.y, d), ux = __shfl_xor(box.z, d), uy = __shfl_xor(box.w, d);
		const int other = __shfl_xor(any, d);
		box = make_float4(S2_MINF(box.x, lx), S2_MINF(box.y, ly), S2_MAXF(box.z, ux), S2_MAXF(box.w, uy));
		any = other > any ? other : any;
	}
	if (lane == 0)
	{
		GroupBox out;
		out.lx = box.x, out.ly = box.y, out.ux = box.z, out.uy = box.w;
		out.any = any, out.pad[0] = out.pad[1] = out.pad[2] = 0;
		boxes[blockIdx.x * S2_RAY_GROUPS + wave] = out;
	}
}

// ---- scene_query.hip's lane code, a private copy ----
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

// Slot `slot` (< n): its header and frame into registers; a polygon's vertices and normals into the lane's LDS column.  polygon.count is
// the wire's count clamped to 0..8 -- the bound of every loop over the vertices.
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
			polygon.norms[i * S2_NP_BLOCK] = make_float2(w->normals[i][0], w->normals[i][1]);
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

// whether shape s is a candidate of the posed ray q before the box test: the ray is active, the category passes, the shape is not on the
// ray's own body, and not on a static one under SKIP_STATIC
S2_DEV bool rayTakes(const PosedRay& q, const LaneShape& s, bool onStatic)
{
	if ((q.bits & 1) == 0 || (s.category & q.mask) == 0u)
	{
		return false;
	}
	if (q.body >= 0 && s.body == q.body)
	{
		return false;
	}
	return !((q.bits & 2) != 0 && onStatic);
}

__global__ __launch_bounds__(S2_BLOCK) void rayReportCandidatesKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																	   const PosedRay* posed, int count, const GroupBox* boxes, unsigned long long* keys)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK], norms[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ PosedRay staged[S2_RAY_GROUP];
	__shared__ int stays;
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int first = (int)blockIdx.y * S2_RAY_GROUP;
	const int group = count - first < S2_RAY_GROUP ? count - first : S2_RAY_GROUP;
	// 24 bytes of the slot against the group's box
	const GroupBox gb = boxes[blockIdx.y];
	bool overlaps = false;
	if (gb.any != 0 && slot < n && shapes[slot].type != S2AMD_SHAPE_FREE)
	{
		overlaps = gb.any == 2 || boxesOverlap(shapes[slot].fatAABB, gb.lx, gb.ly, gb.ux, gb.uy);
	}
	if (threadIdx.x == 0)
	{
		stays = 0;
	}
	__syncthreads();
	const bool waveStays = __ballot(overlaps) != 0ull;
	if (waveStays && (threadIdx.x & 63) == 0)
	{
		stays = 1; // (every wave that writes, writes the same value)
	}
	__syncthreads();
	if (stays == 0)
	{
		return;
	}
	if ((int)threadIdx.x < group)
	{
		const float4* from = (const float4*)(posed + first + (int)threadIdx.x);
		float4* to = (float4*)(staged + threadIdx.x);
		to[0] = from[0], to[1] = from[1], to[2] = from[2];
	}
	PolyRef polygon;
	polygon.verts = verts + threadIdx.x, polygon.norms = norms + threadIdx.x;
	polygon.count = 0, polygon.radius = 0.0f;
	LaneShape s = noShape();
	bool onStatic = false;
	if (overlaps)
	{
		s = loadShape(shapes, slot, bodies, origins, nb, polygon);
		onStatic = s.body >= 0 && s.body < nb && bodies[s.body].type == S2AMD_BODY_STATIC;
	}
	__syncthreads();
	if (!overlaps) // (behind the last barrier: a whole wave may go)
	{
		return;
	}
	for (int k = 0; k < group; ++k)
	{
		const PosedRay q = staged[k];
		if (!rayTakes(q, s, onStatic) || !boxesOverlap(s.fat, q.lx, q.ly, q.ux, q.uy))
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

struct alignas(16) StateRecord
{
	int4 a;
	float4 b, c, d;
};
static_assert(sizeof(StateRecord) == sizeof(s2amdRayState), "the state as the finish pass stores it");

// states[i], ranges[i], now[i] and words[chunk * 4 + wave] (bit = lane: now[i] != before[i]); BEFORE: now[i] alone
template <bool BEFORE>
__global__ __launch_bounds__(S2_BLOCK) void rayReportFinishKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, const PosedRay* posed,
																   int count, const unsigned long long* keys, const int32_t* before, int32_t* now, StateRecord* states,
																   float* ranges, unsigned long long* words)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK], norms[S2_NP_MAX_VERTS * S2_BLOCK];
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	bool changed = false;
	if (i < count)
	{
		const PosedRay q = posed[i];
		const int slot = keySlot(keys[i]);
		const bool active = (q.bits & 1) != 0;
		int shape = -1, hitBody = -1;
		float fraction = q.maxFraction;
		V2 point = v2(0.0f, 0.0f), normal = v2(0.0f, 0.0f);
		if (active && slot >= 0 && slot < n)
		{
			PolyRef polygon;
			polygon.verts = verts + threadIdx.x, polygon.norms = norms + threadIdx.x;
			const LaneShape s = loadShape(shapes, slot, bodies, origins, nb, polygon);
			const V2 p1 = v2(q.p1x, q.p1y), p2 = v2(q.p2x, q.p2y);
			const RayOut o = s.live ? rayCastShape(s, polygon, p1, p2, q.maxFraction) : rayMiss();
			if (o.hit)
			{
				shape = slot, hitBody = s.body;
				fraction = o.fraction;
				normal = rotate(s.xf.q, o.normal);
				point = mulAdd(p1, o.fraction, sub(p2, p1));
			}
		}
		now[i] = shape;
		if (!BEFORE)
		{
			const int was = before[i];
			changed = was != shape;
			StateRecord rec;
			rec.a = make_int4(i, q.body, active ? 1 : 0, shape);
			rec.b = make_float4(__int_as_float(hitBody), __int_as_float(was), fraction, q.p1x);
			rec.c = make_float4(q.p1y, q.p2x, q.p2y, point.x);
			rec.d = make_float4(point.y, normal.x, normal.y, 0.0f);
			states[i] = rec;
			ranges[i] = fraction;
		}
	}
	if (!BEFORE)
	{
		const unsigned long long ballot = __ballot(changed);
		if ((threadIdx.x & 63) == 0)
		{
			words[blockIdx.x * 4 + (threadIdx.x >> 6)] = ballot;
		}
	}
}

// events[rank of ray i among the changed rays] for the rays of chunk blockIdx.x; block 0 writes head = {total, 0, 0, 0}
__global__ __launch_bounds__(S2_BLOCK) void rayReportEventsKernel(const unsigned long long* words, int chunks, const s2amdRayState* states, int4* events, int32_t* head)
{
	__shared__ int exclusive[S2_BLOCK];
	__shared__ int waveTotal[S2_BLOCK / 64];
	const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
	const int c = t < chunks * 4 ? __popcll(words[t]) : 0;
	const int inclusive = waveInclusive(c, lane);
	if (lane == 63)
	{
		waveTotal[wave] = inclusive;
	}
	__syncthreads();
	int carry = 0;
	for (int w = 0; w < wave; ++w)
	{
		carry += waveTotal[w];
	}
	exclusive[t] = carry + inclusive - c;
	if (blockIdx.x == 0 && t == S2_BLOCK - 1)
	{
		head[0] = carry + inclusive, head[1] = 0, head[2] = 0, head[3] = 0;
	}
	__syncthreads();
	const int word = (int)blockIdx.x * 4 + wave;
	const unsigned long long m = words[word];
	if (((m >> lane) & 1ull) != 0ull)
	{
		const int at = exclusive[word] + __popcll(m & ((1ull << lane) - 1ull));
		const int i = (int)blockIdx.x * S2_BLOCK + t;
		const s2amdRayState* st = states + i;
		events[at] = make_int4(i, st->shapeBefore, st->shape, st->hitBody);
	}
}

int rayCountOf(const s2amdSolver* s)
{
	return (int)s->hRaySensors.size();
}

RayLayout layoutOf(const s2amdSolver* s)
{
	return rayLayout(rayCountOf(s));
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->rayReport, s->hRayReportHead, sizeof(s->hRayReportHead), "ray-report", "s2amd_world_set_ray_report"} : ReportRef{};
}

// the pose pass, the candidates (none without shape slots) and the finish pass into hit-shape array `nowSet`
template <bool BEFORE> void launchCast(s2amdSolver* s, const RayLayout& l, int count, int nowSet)
{
	char* base = (char*)s->rayReport.block.p;
	hipStream_t st = s->stream;
	const s2amdShape* shapes = (const s2amdShape*)s->dShapes.p;
	const s2amdBody* bodies = (const s2amdBody*)s->dBodies.p;
	const float2* origins = (const float2*)s->dOrigins.p;
	const int ns = std::max(s->shapeCapacity, 0), tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	PosedRay* posed = (PosedRay*)(base + l.posed);
	GroupBox* boxes = (GroupBox*)(base + l.boxes);
	unsigned long long* keys = (unsigned long long*)(base + l.keys);
	rayPoseKernel<<<dim3((unsigned)l.chunks), dim3(S2_BLOCK), 0, st>>>((const s2amdRaySensor*)(base + l.rays), count, bodies, origins, s->bodyCapacity, posed, keys, boxes);
	if (tiles > 0)
	{
		rayReportCandidatesKernel<<<dim3((unsigned)tiles, (unsigned)((count + S2_RAY_GROUP - 1) / S2_RAY_GROUP)), dim3(S2_BLOCK), 0, st>>>(shapes, ns, bodies, origins, s->bodyCapacity, posed, count, boxes, keys);
	}
	rayReportFinishKernel<BEFORE><<<dim3((unsigned)l.chunks), dim3(S2_BLOCK), 0, st>>>(shapes, ns, bodies, origins, s->bodyCapacity, posed, count, keys,
																						   (const int32_t*)(base + l.shapes[nowSet ^ 1]), (int32_t*)(base + l.shapes[nowSet]),
																						   (StateRecord*)(base + l.states), (float*)(base + l.ranges),
																						   (unsigned long long*)(base + l.words));
}

// "before" := the rule as the resident world and the list stand now: the list into the block, then the cast with shapeNow alone
int rayReportRestate(s2amdSolver* s)
{
	const int count = rayCountOf(s);
	const RayLayout l = layoutOf(s);
	if (count <= 0 || s->rayReport.block.p == nullptr || s->rayReport.block.bytes < l.total)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	char* base = (char*)s->rayReport.block.p;
	// (waited for: the caller's next s2amd_world_set_ray_sensors replaces the vector this copy reads)
	HIP_TRY(hipMemcpyAsync(base + l.rays, s->hRaySensors.data(), (size_t)count * sizeof(s2amdRaySensor), hipMemcpyHostToDevice, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	launchCast<true>(s, l, count, s->rayNowSet);
	HIP_TRY(hipGetLastError());
	return S2AMD_OK;
}

// s2IsValidRay, src/geometry.c:15-20, on the local ray; the flags
bool validRaySensor(const s2amdRaySensor& r)
{
	const bool finite = std::isfinite(r.p1[0]) && std::isfinite(r.p1[1]) && std::isfinite(r.p2[0]) && std::isfinite(r.p2[1]) && std::isfinite(r.maxFraction);
	return finite && 0.0f <= r.maxFraction && r.maxFraction < 100000.0f && (r.flags & ~S2_RAY_SENSOR_KNOWN_FLAGS) == 0;
}

} // namespace

int rayReportPrepare(s2amdSolver* s)
{
	if (!reportPrepareBegin(s, s->rayReport))
	{
		return S2AMD_OK;
	}
	const RayLayout l = layoutOf(s);
	const int rc = reportPrepareBlock(s->rayReport, l.total, l.head);
	return rc ? rc : rayReportRestate(s);
}

int rayReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->rayReport;
	const int flags = r.flags;
	const int count = rayCountOf(s);
	const RayLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "ray"))
	{
		return rc;
	}
	if (count > 0)
	{
		char* base = (char*)r.block.p;
		s->rayNowSet ^= 1; // (per reported step: this is enqueued once, behind the attempt that stands)
		launchCast<false>(s, l, count, s->rayNowSet);
		if ((flags & S2AMD_RAY_REPORT_EVENTS) != 0)
		{
			rayReportEventsKernel<<<dim3((unsigned)l.chunks), dim3(S2_BLOCK), 0, s->stream>>>((const unsigned long long*)(base + l.words), l.chunks,
																							   (const s2amdRayState*)(base + l.states), (int4*)(base + l.events),
																							   (int32_t*)(base + l.head));
		}
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (no rays: nothing is launched, and the head is known here)
		s->hRayReportHead[0] = s->hRayReportHead[1] = s->hRayReportHead[2] = s->hRayReportHead[3] = 0;
	}
	r.stepFlags = flags;
	r.headKnown = count <= 0;
	return S2AMD_OK;
}

const float* rayReportRanges(const s2amdSolver* s, int* rayCount)
{
	const ReportState& r = s->rayReport;
	*rayCount = rayCountOf(s);
	if ((r.stepFlags & S2AMD_RAY_REPORT_RANGES) == 0 || *rayCount <= 0 || r.block.p == nullptr)
	{
		return nullptr;
	}
	return (const float*)((const char*)r.block.p + layoutOf(s).ranges);
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_ray_sensors(s2amdSolver* s, const s2amdRaySensor* rays, int32_t count)
{
	if (int rc = listArgs(s, rays, count, S2AMD_MAX_RAY_SENSORS))
	{
		return rc;
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validRaySensor(rays[i]) || (s->worldResident && rays[i].body >= s->bodyCapacity))
		{
			return fail(S2AMD_E_INVALID, "ray sensor " + std::to_string(i) +
											 " is invalid (fails s2IsValidRay: a NaN or infinite end point, or maxFraction outside [0, 100000); unknown flag bits; a body outside the body array)");
		}
	}
	// "before" of the next step is taken under the new list: the change itself is no event; the last step's report is void
	std::vector<s2amdRaySensor> next(rays, rays + count);
	return listSwapIn(s, [&] { next.swap(s->hRaySensors); }, rayReportPrepare);
}

int s2amd_world_set_ray_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2_RAY_REPORT_KNOWN, rayReportPrepare);
}

// (the states and the ranges need no head: one entry per ray)
int s2amd_world_ray_states(s2amdSolver* s, s2amdRayState* out, int32_t capacity, int32_t* count)
{
	const int rc = reportGetPerItem(ref(s), S2AMD_RAY_REPORT_STATES, "s2amd_world_ray_states", "ray state buffer too small", out, capacity, count, s ? rayCountOf(s) : 0);
	return rc ? rc : reportCopyOut(s, out, s->rayReport.block, layoutOf(s).states, *count, sizeof(s2amdRayState), hipMemcpyDeviceToHost);
}

int s2amd_world_ray_ranges(s2amdSolver* s, float* out, int32_t capacity, int32_t* count)
{
	const int rc = reportGetPerItem(ref(s), S2AMD_RAY_REPORT_RANGES, "s2amd_world_ray_ranges", "ray range buffer too small", out, capacity, count, s ? rayCountOf(s) : 0);
	return rc ? rc : reportCopyOut(s, out, s->rayReport.block, layoutOf(s).ranges, *count, sizeof(float), hipMemcpyDeviceToHost);
}

int s2amd_world_export_ray_ranges(s2amdSolver* s, void* deviceRanges, int32_t capacity)
{
	int32_t count = 0;
	const int rc = reportGetPerItem(ref(s), S2AMD_RAY_REPORT_RANGES, "s2amd_world_export_ray_ranges", "device range buffer too small", deviceRanges, capacity, &count,
									s ? rayCountOf(s) : 0);
	return rc ? rc : reportCopyOut(s, deviceRanges, s->rayReport.block, layoutOf(s).ranges, count, sizeof(float), hipMemcpyDeviceToDevice);
}

int s2amd_world_ray_events(s2amdSolver* s, s2amdRayEvent* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_RAY_REPORT_EVENTS, "s2amd_world_ray_events", "ray event buffer too small", 0, s ? layoutOf(s).events : 0, sizeof(s2amdRayEvent), out,
						 capacity, count);
}

} // extern "C"
#pragma GCC visibility pop
