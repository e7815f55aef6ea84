// Move-and-slide on the resident world (include/solver2d_amd.h: s2amd_world_move_shapes): a batch of character movers, each a caller's
// proxy that wants to go by a displacement, casts against the shapes near its path, stops a skin short of the first blocker, clips what is
// left of the displacement to that plane and casts again, up to eight times -- the loop a caller otherwise drives from the host with one
// s2amd_world_cast_shape call, a wait and an upload per bounce.  Here it stays on the device: nothing resident is written, everything is
// enqueued on the solver's stream behind whatever changed the world last, and the host waits once.  Every distance is s2ShapeDistance
// (gjk_ops.h) and every advancement loop the shape casts' C(q, s) (cast_ops.h), unchanged; the header states the loop around them.
//
// In the query block behind the uploaded movers lie, per mover, the cast of the coming round (112 bytes: the mover's proxy, where it
// stands, what is left of its displacement, maxFraction 1) and its state (128 bytes: status, counts, limits, the slots and normals of its
// planes); then the keys, the results and the planes.
//
//   moverInitKernel        one lane per mover: the first cast and the empty state out of the record.
//   moverCandidatesKernel  shape_cast.hip's mapping: a workgroup holds one tile of 256 shape slots -- box, category bits, body frame,
//                          whether the body is static, radius and vertex count in registers, the vertices in the lane's LDS column --
//                          and walks one chunk of 128 movers staged in LDS: cast (14 KiB), swept box (2 KiB) and the first half of the
//                          state (8 KiB).  A mover that has finished costs one broadcast read of its status.  A candidate that is not
//                          excluded (a slot of the plane list, compared in LDS; the ignored body; a moving body under STATIC_ONLY) runs
//                          the advancement; one that blocks proposes key = fraction bits << 32 | slot by a 64-bit integer atomic min.
//   moverAdvanceKernel     one lane per mover: the winner's advancement again (the same operations, so the same bits), steps 5-10 of
//                          the statement, the next cast, and the key back to the no-hit key.  A mover that ends writes its result.
//
// The host side is query_host.h's queryRounds: the upload, the init kernel, max(maxIterations) rounds of the two passes, one copy back,
// one wait.  40 KiB of LDS a workgroup leave the candidates pass four workgroups a CU (DESIGN.md section 6a has the compiler's report).
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

static_assert(sizeof(s2amdMover) == 128 && sizeof(s2amdMoverResult) == 32 && sizeof(s2amdMoverPlane) == 32, "the mover records");
static_assert(offsetof(s2amdMover, maxIterations) == offsetof(s2amdShapeCast, maxFraction) && offsetof(s2amdMover, maskBits) == offsetof(s2amdShapeCast, maskBits) &&
				  offsetof(s2amdMover, translation) == offsetof(s2amdShapeCast, translation),
			  "a mover begins as the cast it makes");

#define S2_MOVER_CHUNK 128 // movers a workgroup stages
#define S2_MOVER_GRAZE 1e-4f
#define S2_MOVER_RUNNING (-1)

// what the rounds keep of one mover besides its cast; the first 64 bytes are what the candidates pass stages
struct alignas(16) MoverState
{
	int32_t status, planeCount, iterations, advances;
	int32_t maxIterations, ignoreBody;
	uint32_t flags;
	int32_t pad;
	int32_t slots[S2AMD_MOVER_MAX_ITERATIONS]; // -1 beyond planeCount
	float normals[S2AMD_MOVER_MAX_ITERATIONS][2];
};
static_assert(sizeof(MoverState) == 128 && offsetof(MoverState, normals) == 64, "the mover state");

struct alignas(16) MoverHead
{
	float4 w[4];
};
static_assert(sizeof(MoverHead) == offsetof(MoverState, normals), "the staged half of the state");

struct alignas(16) MoverOut
{
	float4 a, b;
};
static_assert(sizeof(MoverOut) == sizeof(s2amdMoverResult) && sizeof(MoverOut) == sizeof(s2amdMoverPlane), "the records as the advance pass stores them");

// r grazes n (the header's statement): one multiply and one negation beside s2Dot and s2Length
S2_DEV bool grazes(V2 r, V2 n)
{
	return dot(r, n) >= -(S2_MOVER_GRAZE * length(r));
}

// step 3: a HIT blocks unless the mover touches the shape where it stands (k == 0, a normal) and is leaving it or sliding along
S2_DEV bool blocks(const CastOutcome& o, V2 r, V2* normal)
{
	*normal = normalize(sub(o.d.pointA, o.d.pointB));
	return !(o.advances == 0 && (normal->x != 0.0f || normal->y != 0.0f) && grazes(r, *normal));
}

__global__ __launch_bounds__(S2_BLOCK) void moverInitKernel(const s2amdMover* movers, int count, s2amdShapeCast* casts, MoverState* states)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const float4* from = (const float4*)(movers + i);
	float4* to = (float4*)(casts + i);
	for (int j = 0; j < 6; ++j)
	{
		to[j] = from[j];
	}
	const float4 tail = from[6];
	to[6] = make_float4(1.0f, tail.y, 0.0f, 0.0f); // maxFraction, maskBits, pad
	float4* st = (float4*)(states + i);
	st[0] = make_float4(__int_as_float(S2_MOVER_RUNNING), __int_as_float(0), __int_as_float(0), __int_as_float(0));
	st[1] = make_float4(tail.x, tail.z, tail.w, __int_as_float(0)); // maxIterations, ignoreBody, flags
	const float none = __int_as_float(-1);
	st[2] = make_float4(none, none, none, none);
	st[3] = make_float4(none, none, none, none);
	for (int j = 4; j < 8; ++j)
	{
		st[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	}
}

__global__ __launch_bounds__(S2_BLOCK) void moverCandidatesKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb,
																   const s2amdShapeCast* casts, const MoverState* states, int count, unsigned long long* keys)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ alignas(16) s2amdShapeCast staged[S2_MOVER_CHUNK];
	__shared__ float4 boxes[S2_MOVER_CHUNK];
	__shared__ MoverHead heads[S2_MOVER_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	// (the chunks of the batch limit outnumber a grid's y: they are folded over y and z, and the last z plane may hold chunks beyond the batch)
	const int first = (int)(blockIdx.z * gridDim.y + blockIdx.y) * S2_MOVER_CHUNK;
	if (first >= count)
	{
		return;
	}
	const int chunk = count - first < S2_MOVER_CHUNK ? count - first : S2_MOVER_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		// (straight into LDS, as shape_cast.hip stages its casts: a copy in registers would be indexed by the box's vertex loop)
		const float4* from = (const float4*)(casts + first + (int)threadIdx.x);
		float4* to = (float4*)(staged + threadIdx.x);
		for (int j = 0; j < (int)(sizeof(s2amdShapeCast) / sizeof(float4)); ++j)
		{
			to[j] = from[j];
		}
		const float4* head = (const float4*)(states + first + (int)threadIdx.x);
		for (int j = 0; j < 4; ++j)
		{
			heads[threadIdx.x].w[j] = head[j];
		}
		boxes[threadIdx.x] = sweptBox(staged[threadIdx.x]);
	}
	LaneProxy s;
	s.live = false;
	bool isStatic = false;
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
			isStatic = s.body >= 0 && s.body < nb && bodies[s.body].type == S2AMD_BODY_STATIC;
		}
	}
	__syncthreads();
	if (!s.live)
	{
		return;
	}
	for (int k = 0; k < chunk; ++k)
	{
		const int4 h = *(const int4*)&heads[k].w[0];
		if (h.x != S2_MOVER_RUNNING)
		{
			continue;
		}
		const int4 limits = *(const int4*)&heads[k].w[1]; // maxIterations, ignoreBody, flags
		const s2amdShapeCast* c = staged + k;
		const float4 box = boxes[k];
		if ((s.category & c->maskBits) == 0u || (limits.y >= 0 && s.body == limits.y) || (((uint32_t)limits.z & S2AMD_MOVER_STATIC_ONLY) != 0u && !isStatic) ||
			!boxesOverlap(s.fat, box.x, box.y, box.z, box.w))
		{
			continue;
		}
		const int4 e0 = *(const int4*)&heads[k].w[2], e1 = *(const int4*)&heads[k].w[3];
		if (slot == e0.x || slot == e0.y || slot == e0.z || slot == e0.w || slot == e1.x || slot == e1.y || slot == e1.z || slot == e1.w)
		{
			continue;
		}
		const CastOutcome o = castAgainst(c, B, s.xf);
		V2 normal;
		if (o.hit && blocks(o, v2(c->translation[0], c->translation[1]), &normal))
		{
			atomicMin(keys + first + k, ((unsigned long long)asBits(o.fraction) << 32) | (unsigned long long)(uint32_t)slot);
		}
	}
}

S2_DEV MoverOut resultOf(V2 p, V2 r, int status, int planeCount, int iterations, int advances)
{
	MoverOut out;
	out.a = make_float4(p.x, p.y, r.x, r.y);
	out.b = make_float4(__int_as_float(status), __int_as_float(planeCount), __int_as_float(iterations), __int_as_float(advances));
	return out;
}

__global__ __launch_bounds__(S2_BLOCK) void moverAdvanceKernel(const s2amdShape* shapes, int n, const s2amdBody* bodies, const float2* origins, int nb, s2amdShapeCast* casts,
																MoverState* states, int count, unsigned long long* keys, MoverOut* results, MoverOut* planes)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	MoverState* st = states + i;
	if (st->status != S2_MOVER_RUNNING || st->iterations >= S2AMD_MOVER_MAX_ITERATIONS) // (a ninth plane has no place)
	{
		return;
	}
	s2amdShapeCast* c = casts + i;
	const int slot = keySlot(keys[i]);
	keys[i] = S2_QUERY_NO_KEY;
	V2 p = v2(c->position[0], c->position[1]), r = v2(c->translation[0], c->translation[1]);
	int planeCount = st->planeCount, advances = st->advances;
	const int iterations = st->iterations + 1;
	int status = S2_MOVER_RUNNING;
	LaneProxy s;
	s.live = false;
	if (slot >= 0 && slot < n)
	{
		s = loadProxy(shapes, slot, bodies, origins, nb);
	}
	if (!s.live)
	{
		// step 5: nothing blocks
		p = add(p, r);
		r = v2(0.0f, 0.0f);
		status = S2AMD_MOVER_REACHED;
	}
	else
	{
		const CastOutcome o = castAgainst(c, slotProxy(shapes, slot, s), s.xf);
		V2 normal;
		blocks(o, r, &normal);
		// step 6
		const float t = o.fraction;
		p = mulAdd(p, t, r);
		V2 rem = mulSV(1.0f - t, r);
		advances += o.advances;
		MoverOut plane;
		plane.a = make_float4(__int_as_float(slot), __int_as_float(s.body), t, o.d.distance);
		plane.b = make_float4(o.d.pointB.x, o.d.pointB.y, normal.x, normal.y);
		planes[(size_t)i * S2AMD_MOVER_MAX_ITERATIONS + planeCount] = plane;
		st->slots[planeCount] = slot;
		st->normals[planeCount][0] = normal.x, st->normals[planeCount][1] = normal.y;
		planeCount += 1;
		if (normal.x == 0.0f && normal.y == 0.0f)
		{
			// step 7
			status = S2AMD_MOVER_OVERLAPPED;
		}
		else
		{
			// step 8
			const float into = dot(rem, normal);
			if (into < 0.0f)
			{
				rem = mulSub(rem, into, normal);
			}
			// steps 9 and 10
			for (int j = 0; j + 1 < planeCount; ++j)
			{
				if (!grazes(rem, v2(st->normals[j][0], st->normals[j][1])))
				{
					status = S2AMD_MOVER_CORNERED;
				}
			}
			if (status == S2_MOVER_RUNNING && rem.x == 0.0f && rem.y == 0.0f)
			{
				status = S2AMD_MOVER_BLOCKED;
			}
		}
		r = rem;
	}
	if (status == S2_MOVER_RUNNING && iterations == st->maxIterations)
	{
		status = S2AMD_MOVER_OUT_OF_ITERATIONS;
	}
	c->position[0] = p.x, c->position[1] = p.y;
	c->translation[0] = r.x, c->translation[1] = r.y;
	st->status = status, st->planeCount = planeCount, st->iterations = iterations, st->advances = advances;
	if (status != S2_MOVER_RUNNING)
	{
		results[i] = resultOf(p, r, status, planeCount, iterations, advances);
	}
}

bool validMover(const void* record)
{
	const s2amdMover& m = *(const s2amdMover*)record;
	if (m.count < 1 || m.count > S2_NP_MAX_VERTS)
	{
		return false;
	}
	bool finite = std::isfinite(m.radius) && std::isfinite(m.position[0]) && std::isfinite(m.position[1]) && std::isfinite(m.rot[0]) && std::isfinite(m.rot[1]) &&
				  std::isfinite(m.translation[0]) && std::isfinite(m.translation[1]);
	for (int i = 0; i < m.count; ++i)
	{
		finite = finite && std::isfinite(m.vertices[i][0]) && std::isfinite(m.vertices[i][1]);
	}
	return finite && m.radius >= 0.0f && m.maxIterations >= 1 && m.maxIterations <= S2AMD_MOVER_MAX_ITERATIONS && (m.flags & ~(uint32_t)S2AMD_MOVER_STATIC_ONLY) == 0u &&
		   m.reserved[0] == 0 && m.reserved[1] == 0 && m.reserved[2] == 0 && m.reserved[3] == 0;
}

// the one rule that needs the world: ignoreBody names a body slot, or none
bool moverFits(const s2amdSolver* s, const void* record)
{
	return ((const s2amdMover*)record)->ignoreBody < s->bodyCapacity;
}

int moverRounds(const void* records, int32_t count)
{
	int rounds = 1;
	for (int32_t i = 0; i < count; ++i)
	{
		rounds = std::max(rounds, (int)((const s2amdMover*)records)[i].maxIterations);
	}
	return rounds;
}

// ---- the launches query_host.h's driver asks for ----
void launchInit(const QueryCall& c)
{
	moverInitKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>((const s2amdMover*)c.records, c.count, (s2amdShapeCast*)c.staged[0], (MoverState*)c.staged[1]);
}

void launchCandidates(const QueryCall& c, unsigned long long* keys)
{
	const unsigned chunks = (unsigned)((c.count + S2_MOVER_CHUNK - 1) / S2_MOVER_CHUNK), rows = std::min(chunks, 32768u);
	const dim3 grid((unsigned)c.tiles, rows, (chunks + rows - 1) / rows);
	moverCandidatesKernel<<<grid, dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (const s2amdShapeCast*)c.staged[0], (const MoverState*)c.staged[1],
																  c.count, keys);
}

void launchAdvance(const QueryCall& c, unsigned long long* keys, void* results, void* planes)
{
	moverAdvanceKernel<<<gridFor((size_t)c.count), dim3(S2_BLOCK), 0, c.stream>>>(c.shapes, c.ns, c.bodies, c.origins, c.nb, (s2amdShapeCast*)c.staged[0], (MoverState*)c.staged[1],
																				   c.count, keys, (MoverOut*)results, (MoverOut*)planes);
}

const QueryKind moverKind = {sizeof(s2amdMover), "movers", validMover, "mover",
							 "is invalid (count outside 1..8, a NaN or infinite field, a negative radius, maxIterations outside 1..8, an unknown flag, reserved not 0)",
							 {sizeof(s2amdShapeCast), sizeof(MoverState)}, launchInit};

const QueryRounds moverPasses = {moverFits, "names a body slot beyond the world's (ignoreBody)", moverRounds, sizeof(s2amdMoverResult),
								 S2AMD_MOVER_MAX_ITERATIONS * sizeof(s2amdMoverPlane), launchCandidates, launchAdvance};

} // namespace

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_move_shapes(s2amdSolver* s, const s2amdMover* movers, int32_t count, s2amdMoverResult* results, s2amdMoverPlane* planes)
{
	return queryRounds(s, moverKind, movers, count, results, planes, moverPasses);
}

} // extern "C"
#pragma GCC visibility pop
