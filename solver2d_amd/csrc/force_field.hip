// Force fields on the resident world (include/solver2d_amd.h: s2amd_world_apply_fields, s2amd_world_set_fields,
// s2amd_world_field_states): a write addressed by region.  A field is a sensor's region (mount_ops.h: the frame, the candidate
// box) with a rule that turns every shape of a dynamic body within reach -- the proximity queries' D(q, s).distance <= range
// (proximity_query.hip; s2ShapeDistance, src/distance.c:485-636) -- into one term, and a term is one of s2amd_world_edit's two
// additive setters (edit_ops.h: applyBodyEdit).  The statement is sequential: fields in list order, inside a field the shapes in slot
// order.  A term reads and writes its shape's body only, so only the order of the terms ON ONE BODY matters -- to the bit, because
// force adds and impulse adds are float sums and a DRAG term reads the velocity the terms before it left.
//
//   fieldKeysKernel     the body -> shapes list, once per upload at the first use: key = the body of a live shape (else the body
//                       count), value = the slot; rocPRIM's radix sort by body is STABLE, so a body's slots stay ascending;
//                       report_common.h's reportBodyRangesKernel gives each body its run.
//   fieldPrepareKernel  one lane per field: active, the world transform, the candidate box (mount_ops.h); the staged record of the apply pass and
//                       the field's state with terms = 0, lowestShape = -1.
//   fieldApplyKernel    one lane per body slot.  The prepared fields are staged through LDS in chunks of S2_FIELD_CHUNK (144 bytes
//                       each), every field a broadcast read.  A lane of a dynamic body walks the fields in index order and inside a
//                       field its own shapes in ascending slot order (the first shape's header in registers): the candidate tests,
//                       the distance, the term through applyBodyEdit, with linearVelocity, angularVelocity and force in registers;
//                       it writes its record back only if it applied a term.  A body with hundreds of shapes is walked by one lane: correct, not fast.
//
// The states' counts: per field a wave ballot, and only in a wave with a term a wave sum and one integer atomicAdd, the lowest slot by
// one integer atomicMin.  No float atomics, no host sort, no host wait unless the caller asks for the states.  All arithmetic is fp32
// in the reference's operation order; this file is compiled without contraction in both libraries (Makefile).
#include "query_list.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "gjk_ops.h"
#include "proxy_ops.h"
#include "mount_ops.h"
#include "edit_ops.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstring>

namespace
{

static_assert(sizeof(s2amdField) == 128 && sizeof(s2amdFieldState) == 64, "the fields' records");

#define S2_FIELD_KNOWN_FLAGS (S2AMD_FIELD_DISABLED | S2AMD_FIELD_AS_IMPULSE | S2AMD_FIELD_LINEAR_FALLOFF)
#define S2_FIELD_CHUNK 128

// a field as the apply pass stages it: the proxy in its own frame, the world transform, the rule's fields, the candidate box
struct alignas(16) PreparedField
{
	float vertices[8][2];
	int32_t count;
	float radius;
	float position[2], rot[2];
	float range;
	uint32_t maskBits;
	int32_t body, active, kind, flags;
	float strength, direction[2];
	int32_t pad;
	float box[4];
};
static_assert(sizeof(PreparedField) == 144, "nine 16-byte words per staged field");
#define S2_FIELD_WORDS ((int)(sizeof(PreparedField) / sizeof(float4)))

// one list's device block: {the list, the prepared records, the states}
struct FieldLayout
{
	size_t fields, prepared, states, total;
};

FieldLayout fieldLayout(int count)
{
	FieldLayout l{};
	size_t at = 0;
	l.fields = reportTake(at, (size_t)count * sizeof(s2amdField));
	l.prepared = reportTake(at, (size_t)count * sizeof(PreparedField));
	l.states = reportTake(at, (size_t)count * sizeof(s2amdFieldState));
	l.total = at;
	return l;
}

// the body -> shapes list's block
struct AdjLayout
{
	size_t ranges, keysIn, keysOut, valsIn, valsOut, sortTmp, total;
};

AdjLayout adjLayout(int ns, int nb, size_t tmpBytes)
{
	AdjLayout l{};
	size_t at = 0;
	l.ranges = reportTake(at, (size_t)2 * nb * sizeof(int));
	l.keysIn = reportTake(at, (size_t)ns * sizeof(uint32_t));
	l.keysOut = reportTake(at, (size_t)ns * sizeof(uint32_t));
	l.valsIn = reportTake(at, (size_t)ns * sizeof(int));
	l.valsOut = reportTake(at, (size_t)ns * sizeof(int));
	l.sortTmp = reportTake(at, tmpBytes);
	l.total = at;
	return l;
}

// keys[slot] = the body of a live shape on a body of the array, else nb (an entry of no body); vals[slot] = slot
__global__ __launch_bounds__(S2_BLOCK) void fieldKeysKernel(const s2amdShape* shapes, int ns, int nb, uint32_t* keys, int* vals)
{
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (slot >= ns)
	{
		return;
	}
	const int body = shapes[slot].body;
	const bool owned = shapes[slot].type != S2AMD_SHAPE_FREE && body >= 0 && body < nb;
	keys[slot] = owned ? (uint32_t)body : (uint32_t)nb;
	vals[slot] = slot;
}

// prepared[i] and states[i] (terms and lowestShape as a field without terms has them: the apply pass counts into them)
__global__ __launch_bounds__(S2_BLOCK) void fieldPrepareKernel(const s2amdField* fields, int count, const s2amdBody* bodies, const float2* origins, int nb,
																PreparedField* prepared, s2amdFieldState* states)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const s2amdField* q = fields + i;
	PreparedField* out = prepared + i;
	const int body = q->body, flags = q->flags;
	Xf xf;
	const bool active = mountFrame(q, S2AMD_FIELD_DISABLED, bodies, origins, nb, xf);
	const int count8 = q->count < 1 ? 1 : q->count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : q->count;
	float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (active)
	{
		// the proximity queries' query box with maxDistance = range
		box = mountBox(xf, q->vertices, count8, &q->radius, &q->range);
	}
	else
	{
		xf = noFrame();
	}
	const float4* from = (const float4*)q->vertices;
	float4* to = (float4*)out->vertices;
	to[0] = from[0], to[1] = from[1], to[2] = from[2], to[3] = from[3];
	to[4] = make_float4(__int_as_float(count8), q->radius, xf.p.x, xf.p.y);
	to[5] = make_float4(xf.q.s, xf.q.c, q->range, __uint_as_float(q->maskBits));
	to[6] = make_float4(__int_as_float(body), __int_as_float(active ? 1 : 0), __int_as_float(q->kind), __int_as_float(flags));
	to[7] = make_float4(q->strength, q->direction[0], q->direction[1], __int_as_float(0));
	to[8] = box;
	s2amdFieldState* st = states + i;
	st->field = i, st->body = body, st->active = active ? 1 : 0, st->terms = 0, st->lowestShape = -1;
	st->pad[0] = st->pad[1] = st->pad[2] = 0;
	st->position[0] = xf.p.x, st->position[1] = xf.p.y, st->rot[0] = xf.q.s, st->rot[1] = xf.q.c;
	st->box[0] = box.x, st->box[1] = box.y, st->box[2] = box.z, st->box[3] = box.w;
}

// what the candidate rule reads of a shape slot
struct ShapeHead
{
	int slot, type, body;
	uint32_t category;
	float fat[4];
};

S2_DEV ShapeHead loadHead(const s2amdShape* shapes, int slot)
{
	const s2amdShape* w = shapes + slot;
	ShapeHead h;
	h.slot = slot, h.type = w->type, h.body = w->body;
	h.category = w->categoryBits;
	h.fat[0] = w->fatAABB[0], h.fat[1] = w->fatAABB[1], h.fat[2] = w->fatAABB[2], h.fat[3] = w->fatAABB[3];
	return h;
}

// The term of field q on the shape with head h of the lane's dynamic body, if the shape is a candidate within reach: applied to f
// through applyBodyEdit.  true: a term was applied.
S2_DEV bool fieldTerm(const PreparedField& q, const s2amdShape* shapes, const ShapeHead& h, int body, Xf bodyXf, const BodyFixed& k, BodyFields& f)
{
	const int type = h.type;
	if (type == S2AMD_SHAPE_FREE || h.body != body || (h.category & q.maskBits) == 0u || !boxesOverlap(h.fat, q.box[0], q.box[1], q.box[2], q.box[3]))
	{
		return false;
	}
	const s2amdShape* w = shapes + h.slot;
	// s2Shape_MakeDistanceProxy (proxy_ops.h: loadProxy), the vertices where the wire record holds them
	WireProxy A, B;
	A.verts = q.vertices, A.count = q.count, A.radius = q.radius;
	B.verts = w->vertices;
	B.radius = type == S2AMD_SHAPE_SEGMENT ? 0.0f : w->radius;
	if (type == S2AMD_SHAPE_POLYGON)
	{
		const int count = w->count;
		B.count = count < 1 ? 1 : count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : count;
	}
	else
	{
		B.count = type == S2AMD_SHAPE_CIRCLE ? 1 : 2;
	}
	const ShapeDistanceOutput D = shapeDistanceWithRadii(A, frameOf(q.position, q.rot), B, bodyXf);
	if (!(D.distance <= q.range))
	{
		return false;
	}
	float scale = 1.0f;
	if ((q.flags & S2AMD_FIELD_LINEAR_FALLOFF) != 0 && q.range > 0.0f)
	{
		scale = 1.0f - D.distance / q.range;
	}
	const float m = q.strength * scale;
	V2 g, point = v2(k.px, k.py);
	if (q.kind == S2AMD_FIELD_RADIAL)
	{
		const V2 n = normalize(sub(D.pointB, v2(q.position[0], q.position[1])));
		g = v2(m * n.x, m * n.y);
		point = D.pointB;
	}
	else if (q.kind == S2AMD_FIELD_UNIFORM)
	{
		g = v2(m * q.direction[0], m * q.direction[1]);
	}
	else
	{
		const float nm = -m;
		g = v2(nm * f.vx, nm * f.vy);
	}
	s2amdWorldEdit e;
	e.kind = (q.flags & S2AMD_FIELD_AS_IMPULSE) != 0 ? S2AMD_EDIT_BODY_APPLY_LINEAR_IMPULSE : S2AMD_EDIT_BODY_APPLY_FORCE_TO_CENTER;
	e.target = body, e.flag = 0, e.reserved = 0;
	e.v[0] = g.x, e.v[1] = g.y, e.v[2] = point.x, e.v[3] = point.y;
	applyBodyEdit(e, k, f);
	return true;
}

// One lane per body slot; ranges[2 * body] .. ranges[2 * body + 1] is the body's run in `list`, its shape slots ascending.
__global__ __launch_bounds__(S2_BLOCK) void fieldApplyKernel(const s2amdShape* shapes, int ns, s2amdBody* bodies, const float2* origins, int nb, const PreparedField* prepared,
															  int count, const int* ranges, const int* list, s2amdFieldState* states)
{
	__shared__ PreparedField staged[S2_FIELD_CHUNK];
	const int body = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63);
	BodyFixed k;
	BodyFields f;
	k.type = S2AMD_BODY_FREE, k.invMass = k.invI = k.px = k.py = 0.0f;
	f.vx = f.vy = f.w = f.fx = f.fy = 0.0f, f.written = 0;
	Xf bodyXf;
	bodyXf.p = v2(0.0f, 0.0f);
	bodyXf.q.s = 0.0f, bodyXf.q.c = 1.0f;
	int first = 0, last = 0;
	// (the head of the lane's first shape stays in registers: most bodies have one shape, and the walk over the fields then reads LDS only)
	ShapeHead head;
	head.slot = 0, head.type = S2AMD_SHAPE_FREE, head.body = -1, head.category = 0u;
	head.fat[0] = head.fat[1] = head.fat[2] = head.fat[3] = 0.0f;
	if (body < nb)
	{
		loadBody(bodies + body, k, f);
		if (k.type == S2AMD_BODY_DYNAMIC)
		{
			first = ranges[2 * body], last = ranges[2 * body + 1];
			// (a run never leaves the list; the clamp only keeps a lane inside it whatever the ranges hold)
			first = first < 0 ? 0 : first > ns ? ns : first;
			last = last < first ? first : last > ns ? ns : last;
			const float2 o = origins[body];
			bodyXf.p = v2(o.x, o.y);
			bodyXf.q.s = bodies[body].rot[0], bodyXf.q.c = bodies[body].rot[1];
			if (first < last)
			{
				const int slot = list[first];
				if (slot >= 0 && slot < ns)
				{
					head = loadHead(shapes, slot);
				}
			}
		}
	}
	for (int base = 0; base < count; base += S2_FIELD_CHUNK)
	{
		const int chunk = count - base < S2_FIELD_CHUNK ? count - base : S2_FIELD_CHUNK;
		__syncthreads(); // (every lane is done with the chunk before)
		{
			const float4* from = (const float4*)(prepared + base);
			float4* to = (float4*)staged;
			for (int j = (int)threadIdx.x; j < chunk * S2_FIELD_WORDS; j += S2_BLOCK)
			{
				to[j] = from[j];
			}
		}
		__syncthreads();
		for (int c = 0; c < chunk; ++c)
		{
			const PreparedField& q = staged[c];
			int terms = 0, lowest = -1;
			if (q.active != 0 && q.body != body)
			{
				for (int at = first; at < last; ++at)
				{
					ShapeHead h = head;
					if (at != first)
					{
						const int slot = list[at];
						if (slot < 0 || slot >= ns)
						{
							continue;
						}
						h = loadHead(shapes, slot);
					}
					if (fieldTerm(q, shapes, h, body, bodyXf, k, f))
					{
						lowest = terms == 0 ? h.slot : lowest; // (the run ascends)
						terms += 1;
					}
				}
			}
			if (__ballot(terms != 0) != 0ull)
			{
				// the wave's sum and its lowest slot (as unsigned: -1 is the largest), then one atomic each
				unsigned int low = (unsigned int)lowest;
				for (int d = 32; d > 0; d >>= 1)
				{
					terms += __shfl_xor(terms, d);
					const unsigned int other = (unsigned int)__shfl_xor((int)low, d);
					low = other < low ? other : low;
				}
				if (lane == 0)
				{
					s2amdFieldState* st = states + base + c;
					atomicAdd(&st->terms, terms);
					atomicMin((unsigned int*)&st->lowestShape, low);
				}
			}
		}
	}
	if (f.written != 0)
	{
		storeBody(bodies + body, f);
	}
}

bool validField(const s2amdField& q)
{
	if (q.count < 1 || q.count > S2_NP_MAX_VERTS || (q.flags & ~S2_FIELD_KNOWN_FLAGS) != 0 || q.kind < S2AMD_FIELD_RADIAL || q.kind > S2AMD_FIELD_DRAG || q.reserved != 0)
	{
		return false;
	}
	bool finite = std::isfinite(q.radius) && std::isfinite(q.range) && std::isfinite(q.position[0]) && std::isfinite(q.position[1]) && std::isfinite(q.rot[0]) &&
				  std::isfinite(q.rot[1]) && std::isfinite(q.strength) && std::isfinite(q.direction[0]) && std::isfinite(q.direction[1]);
	for (int i = 0; i < q.count; ++i)
	{
		finite = finite && std::isfinite(q.vertices[i][0]) && std::isfinite(q.vertices[i][1]);
	}
	return finite && q.radius >= 0.0f && q.range >= 0.0f;
}

// the whole list, before anything is enqueued or replaced
int checkList(const s2amdSolver* s, const s2amdField* fields, int32_t count)
{
	if (int rc = listArgs(s, fields, count, S2AMD_MAX_FIELDS))
	{
		return rc;
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validField(fields[i]) || (s->worldResident && fields[i].body >= s->bodyCapacity))
		{
			return fail(S2AMD_E_INVALID, "field " + std::to_string(i) +
											 " is invalid (count outside 1..8, kind outside 1..3, a NaN or infinite field, a negative radius or range, unknown flag bits, "
											 "reserved != 0, a body outside the body array): nothing was applied or replaced");
		}
	}
	return S2AMD_OK;
}

// the body -> shapes list of the resident world, built once per upload
int ensureAdjacency(s2amdSolver* s)
{
	if (s->fieldAdjValid)
	{
		return S2AMD_OK;
	}
	const int ns = s->shapeCapacity, nb = s->bodyCapacity;
	hipStream_t st = s->stream;
	size_t tmp = 0;
	if (ns > 0)
	{
		HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)ns, 0, bodyKeyBits(nb), st));
	}
	const AdjLayout l = adjLayout(ns, nb, tmp);
	if (int rc = s->dFieldAdj.ensure(l.total))
	{
		return rc;
	}
	char* base = (char*)s->dFieldAdj.p;
	HIP_TRY(hipMemsetAsync(base + l.ranges, 0, reportRound((size_t)2 * nb * sizeof(int)), st));
	if (ns > 0)
	{
		fieldKeysKernel<<<gridFor((size_t)ns), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, nb, (uint32_t*)(base + l.keysIn), (int*)(base + l.valsIn));
		HIP_TRY(hipGetLastError());
		HIP_TRY(rocprim::radix_sort_pairs((void*)(base + l.sortTmp), tmp, (uint32_t*)(base + l.keysIn), (uint32_t*)(base + l.keysOut), (int*)(base + l.valsIn),
										  (int*)(base + l.valsOut), (size_t)ns, 0, bodyKeyBits(nb), st));
		if (nb > 0)
		{
			reportBodyRangesKernel<<<gridFor((size_t)ns), dim3(S2_BLOCK), 0, st>>>((const uint32_t*)(base + l.keysOut), ns, nb, (int*)(base + l.ranges));
		}
		HIP_TRY(hipGetLastError());
	}
	s->fieldAdjValid = true;
	s->fieldAdjBuilds += 1;
	return S2AMD_OK;
}

// the two kernels over the list at the head of `block` (laid out by fieldLayout(count)), on the step's stream
int enqueueFields(s2amdSolver* s, const DevBuf& block, int count)
{
	if (int rc = ensureAdjacency(s))
	{
		return rc;
	}
	const int ns = s->shapeCapacity, nb = s->bodyCapacity;
	const FieldLayout l = fieldLayout(count);
	char* base = (char*)block.p;
	const AdjLayout a = adjLayout(ns, nb, 0);
	const char* adj = (const char*)s->dFieldAdj.p;
	hipStream_t st = s->stream;
	fieldPrepareKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const s2amdField*)(base + l.fields), count, (const s2amdBody*)s->dBodies.p,
																		 (const float2*)s->dOrigins.p, nb, (PreparedField*)(base + l.prepared), (s2amdFieldState*)(base + l.states));
	if (nb > 0 && ns > 0)
	{
		fieldApplyKernel<<<gridFor((size_t)nb), dim3(S2_BLOCK), 0, st>>>((const s2amdShape*)s->dShapes.p, ns, (s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, nb,
																		(const PreparedField*)(base + l.prepared), count, (const int*)(adj + a.ranges),
																		(const int*)(adj + a.valsOut), (s2amdFieldState*)(base + l.states));
	}
	HIP_TRY(hipGetLastError());
	return S2AMD_OK;
}

} // namespace

int fieldsStepEnqueue(s2amdSolver* s)
{
	const int count = (int)s->hFields.size();
	if (count == 0)
	{
		return S2AMD_OK;
	}
	if (s->dFieldList.p == nullptr || s->dFieldList.bytes < fieldLayout(count).total)
	{
		return fail(S2AMD_E_STATE, "internal: the field list's device block was not prepared");
	}
	const int rc = enqueueFields(s, s->dFieldList, count);
	s->fieldStatesValid = rc == S2AMD_OK;
	return rc;
}

void fieldsForgetWorld(s2amdSolver* s)
{
	s->fieldAdjValid = false;
	s->fieldStatesValid = false;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_apply_fields(s2amdSolver* s, const s2amdField* fields, int32_t count, s2amdFieldState* states)
{
	if (int rc = checkList(s, fields, count))
	{
		return rc;
	}
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	hipStream_t st = s->stream;
	// the pinned stage, as s2amd_world_edit's: the caller may reuse its list at once and the copy to the device is a true asynchronous
	// one.  The copy of the call before may still be reading the stage: its event is waited for first.
	const size_t listBytes = (size_t)count * sizeof(s2amdField);
	if (int rc = s->fieldStage.begin(listBytes, std::max(reportRound(listBytes + listBytes / 2), (size_t)4096)))
	{
		return rc;
	}
	const FieldLayout l = fieldLayout(count);
	if (int rc = s->dFieldCall.ensure(l.total))
	{
		return rc;
	}
	memcpy(s->fieldStage.buf.p, fields, listBytes);
	char* base = (char*)s->dFieldCall.p;
	HIP_TRY(hipMemcpyAsync(base + l.fields, s->fieldStage.buf.p, listBytes, hipMemcpyHostToDevice, st));
	HIP_TRY(s->fieldStage.record(st));
	if (int rc = enqueueFields(s, s->dFieldCall, count))
	{
		return rc;
	}
	if (states)
	{
		HIP_TRY(hipMemcpyAsync(states, base + l.states, (size_t)count * sizeof(s2amdFieldState), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	return S2AMD_OK;
}

int s2amd_world_set_fields(s2amdSolver* s, const s2amdField* fields, int32_t count)
{
	if (int rc = checkList(s, fields, count))
	{
		return rc;
	}
	if (count > 0)
	{
		// the list goes to its device block now, so that a step only launches: waited for, because the block of the list before may
		// still be read by a step in flight and the copy reads the caller's memory
		const FieldLayout l = fieldLayout(count);
		const int rc = listUpload(s, s->dFieldList, l.total, [&](char* base) {
			HIP_TRY(hipMemcpyAsync(base + l.fields, fields, (size_t)count * sizeof(s2amdField), hipMemcpyHostToDevice, s->stream));
			return (int)S2AMD_OK;
		});
		if (rc)
		{
			return rc; // (the old list stands: its block is as it was or larger)
		}
	}
	s->hFields.assign(fields, fields + count);
	s->fieldStatesValid = false;
	return S2AMD_OK;
}

int s2amd_world_field_states(s2amdSolver* s, s2amdFieldState* out, int32_t capacity, int32_t* count)
{
	if (!s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (!s->worldResident || !s->resident)
	{
		return fail(S2AMD_E_STATE, "no resident world");
	}
	if (s->hFields.empty())
	{
		*count = 0;
		return S2AMD_OK;
	}
	if (!s->fieldStatesValid)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_field_states: no s2amd_world_step has applied the list since it was set (s2amd_world_set_fields, then a step)");
	}
	*count = (int32_t)s->hFields.size();
	if (*count > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "field state buffer too small");
	}
	return reportCopyOut(s, out, s->dFieldList, fieldLayout(*count).states, *count, sizeof(s2amdFieldState), hipMemcpyDeviceToHost);
}

} // extern "C"
#pragma GCC visibility pop
