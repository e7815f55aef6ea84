// Sensor report of the resident world (include/solver2d_amd.h: s2amd_world_set_sensors, s2amd_world_set_sensor_report and the three
// getters): which shapes are inside each of up to 1,024 regions now, which came in during the step and which went out -- what a caller
// otherwise composes per step from a pose download, s2amd_world_shapes_in_range and a host-side set difference.  A region is a proxy
// (s2MakeProxy) fixed in the world or riding on a body; "inside" is the proximity queries' D(q, s).distance <= margin
// (proximity_query.hip; s2ShapeDistance, src/distance.c:485-636).  The passes are enqueued behind stage 4 of s2amd_world_step and behind
// the other five reports, once per step (a repeated step reports once); the report owns its "before" state on the device.
//
//   sensorPoseKernel     one lane per sensor: active, the world transform, the candidate box (mount_ops.h); the staged record of the
//                        mask pass and the fixed fields of the sensor's state.
//   sensorMaskKernel     proximity_query.hip's mapping: a workgroup holds one tile of 256 shape slots -- header in registers, the proxy
//                        vertices in the lane's LDS column -- and walks one chunk of up to 256 posed sensors staged in LDS (128 bytes
//                        each, 32 KiB), every sensor a broadcast read.  The grid is tiles x chunks.  Per (sensor, tile, wave) it reads the
//                        previous 64-bit ballot word and writes three in the same pass: now, now & ~before, before & ~now.  The now /
//                        before masks ping-pong between two sets, swapped per reported step.  <true>: "before" only -- the now word alone.
//   sensorPrefixKernel   one wave per sensor: query_list.h's tile prefix over the three mask sets, and the sensor's state from it (the
//                        three counts, the lowest inside slot).
//   sensorOffsetsKernel  one wave per list: the CSR offsets over the sensors; the totals are the head the getters fetch.
//   sensorWriteKernel    one lane per ballot word and list: query_list.h's write pass; the event lists take 16-byte records.
//
// No sort, no atomic.  All arithmetic is fp32 in the reference's operation order (gjk_ops.h); this file is compiled without contraction
// in both libraries (Makefile).  All device memory is one block sized by sensorReportPrepare; a step allocates nothing and waits for
// nothing -- the getters do, and a getter whose list outgrew listCapacity writes it again from the kept masks into the query scratch.
#include "query_list.h"

#define S2_NP_BLOCK S2_BLOCK
#define S2_NP_MAX_VERTS 8
#include "gjk_ops.h"
#include "proxy_ops.h"
#include "mount_ops.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace
{

static_assert(sizeof(s2amdSensor) == 112 && sizeof(s2amdSensorEvent) == 16 && sizeof(s2amdSensorState) == 64, "the report's records");

#define S2_SENSOR_KNOWN_FLAGS (S2AMD_SENSOR_DISABLED | S2AMD_SENSOR_SKIP_STATIC)
#define S2_SENSOR_REPORT_KNOWN (S2AMD_SENSOR_REPORT_INSIDE | S2AMD_SENSOR_REPORT_EVENTS | S2AMD_SENSOR_REPORT_STATES)

// a sensor as the mask pass stages it: the proxy in its own frame, the world transform, the rule's fields, the candidate box
struct alignas(16) PosedSensor
{
	float vertices[8][2];
	int32_t count;
	float radius;
	float position[2], rot[2];
	float margin;
	uint32_t maskBits;
	int32_t body, active, skipStatic, pad;
	float box[4];
};
static_assert(sizeof(PosedSensor) == 128, "eight 16-byte words per staged sensor");

struct SensorLayout
{
	size_t sensors, posed, states, masks[4], prefix, totals, offsets, head, inside, entered, left, total;
	size_t words; // ballot words per mask set
	int tiles, lists;
};

// masks[0], masks[1]: now / before, ping-pong; masks[2]: entered; masks[3]: left
SensorLayout sensorLayout(int count, int ns, int listCapacity)
{
	SensorLayout l{};
	size_t at = 0;
	l.tiles = (ns + S2_BLOCK - 1) / S2_BLOCK;
	l.words = (size_t)count * l.tiles * 4;
	// (no list is longer than sensors x shape slots)
	l.lists = (int)std::min((size_t)listCapacity, (size_t)count * (size_t)ns);
	l.sensors = reportTake(at, (size_t)count * sizeof(s2amdSensor));
	l.posed = reportTake(at, (size_t)count * sizeof(PosedSensor));
	l.states = reportTake(at, (size_t)count * sizeof(s2amdSensorState));
	for (int k = 0; k < 4; ++k)
	{
		l.masks[k] = reportTake(at, l.words * sizeof(unsigned long long));
	}
	l.prefix = reportTake(at, (size_t)3 * count * l.tiles * sizeof(int));
	l.totals = reportTake(at, (size_t)3 * count * sizeof(int));
	l.offsets = reportTake(at, (size_t)3 * ((size_t)count + 1) * sizeof(int));
	l.head = reportTake(at, 4 * sizeof(int32_t));
	l.inside = reportTake(at, (size_t)l.lists * sizeof(int32_t));
	l.entered = reportTake(at, (size_t)l.lists * sizeof(s2amdSensorEvent));
	l.left = reportTake(at, (size_t)l.lists * sizeof(s2amdSensorEvent));
	l.total = at;
	return l;
}

// states[i]'s fixed fields and posed[i]
__global__ __launch_bounds__(S2_BLOCK) void sensorPoseKernel(const s2amdSensor* sensors, int count, const s2amdBody* bodies, const float2* origins, int nb, PosedSensor* posed,
															 s2amdSensorState* states)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const s2amdSensor* q = sensors + i;
	PosedSensor* out = posed + i;
	const int body = q->body, flags = q->flags;
	Xf xf;
	const bool active = mountFrame(q, S2AMD_SENSOR_DISABLED, bodies, origins, nb, xf);
	const int count8 = q->count < 1 ? 1 : q->count > S2_NP_MAX_VERTS ? S2_NP_MAX_VERTS : q->count;
	float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (active)
	{
		// the proximity queries' query box with maxDistance = margin
		box = mountBox(xf, q->vertices, count8, &q->radius, &q->margin);
	}
	else
	{
		xf = noFrame();
	}
	const float4* from = (const float4*)q->vertices;
	float4* to = (float4*)out->vertices;
	to[0] = from[0], to[1] = from[1], to[2] = from[2], to[3] = from[3];
	to[4] = make_float4(__int_as_float(count8), q->radius, xf.p.x, xf.p.y);
	to[5] = make_float4(xf.q.s, xf.q.c, q->margin, __uint_as_float(q->maskBits));
	to[6] = make_float4(__int_as_float(body), __int_as_float(active ? 1 : 0), __int_as_float((flags & S2AMD_SENSOR_SKIP_STATIC) != 0 ? 1 : 0), __int_as_float(0));
	to[7] = box;
	// (inside, entered, left and lowestShape are the prefix pass's)
	s2amdSensorState* st = states + i;
	st->sensor = i, st->body = body, st->active = active ? 1 : 0, st->pad = 0;
	st->position[0] = xf.p.x, st->position[1] = xf.p.y, st->rot[0] = xf.q.s, st->rot[1] = xf.q.c;
	st->box[0] = box.x, st->box[1] = box.y, st->box[2] = box.z, st->box[3] = box.w;
}

// word = ((sensor * tiles) + tile) * 4 + wave, bit = lane: now[word] = the wave's shapes inside the sensor; unless BEFORE also
// entered[word] = now & ~before[word] and left[word] = before[word] & ~now.  Every word is written.
template <bool BEFORE>
__global__ __launch_bounds__(S2_BLOCK) void sensorMaskKernel(const s2amdShape* shapes, int n, int tiles, const s2amdBody* bodies, const float2* origins, int nb,
															 const PosedSensor* posed, int count, const unsigned long long* before, unsigned long long* now,
															 unsigned long long* entered, unsigned long long* left)
{
	__shared__ float2 verts[S2_NP_MAX_VERTS * S2_BLOCK];
	__shared__ PosedSensor staged[S2_QUERY_CHUNK];
	const int slot = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int first = (int)blockIdx.y * S2_QUERY_CHUNK;
	const int chunk = count - first < S2_QUERY_CHUNK ? count - first : S2_QUERY_CHUNK;
	if ((int)threadIdx.x < chunk)
	{
		const float4* from = (const float4*)(posed + first + (int)threadIdx.x);
		float4* to = (float4*)(staged + threadIdx.x);
		for (int j = 0; j < (int)(sizeof(PosedSensor) / sizeof(float4)); ++j)
		{
			to[j] = from[j];
		}
	}
	LaneProxy s;
	s.live = false;
	s.body = -1;
	s.category = 0u;
	bool onStatic = false;
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
			onStatic = s.body >= 0 && s.body < nb && bodies[s.body].type == S2AMD_BODY_STATIC;
		}
	}
	__syncthreads();
	for (int k = 0; k < chunk; ++k)
	{
		const PosedSensor* q = staged + k;
		bool inside = false;
		if (q->active != 0 && s.live && (s.category & q->maskBits) != 0u && s.body != q->body && !(q->skipStatic != 0 && onStatic) &&
			boxesOverlap(s.fat, q->box[0], q->box[1], q->box[2], q->box[3]))
		{
			WireProxy A;
			A.verts = q->vertices, A.count = q->count, A.radius = q->radius;
			inside = shapeDistanceWithRadii(A, frameOf(q->position, q->rot), B, s.xf).distance <= q->margin;
		}
		const unsigned long long ballot = __ballot(inside);
		if (lane == 0)
		{
			const size_t word = ((size_t)(first + k) * tiles + blockIdx.x) * 4 + wave;
			now[word] = ballot;
			if (!BEFORE)
			{
				const unsigned long long was = before[word];
				entered[word] = ballot & ~was;
				left[word] = was & ~ballot;
			}
		}
	}
}

// tilePrefix[list][sensor * tiles + tile], totals[list][sensor] for the three mask sets (query_list.h: listTilePrefixKernel), and the
// counts and lowestShape of states[sensor]
__global__ __launch_bounds__(S2_BLOCK) void sensorPrefixKernel(const unsigned long long* now, const unsigned long long* entered, const unsigned long long* left, int count,
															   int tiles, int* tilePrefix, int* totals, s2amdSensorState* states)
{
	const int lane = (int)(threadIdx.x & 63);
	const int q = (int)(blockIdx.x * (S2_BLOCK / 64) + (threadIdx.x >> 6));
	if (q >= count) // (whole waves)
	{
		return;
	}
	int sums[3];
	int lowest = INT_MAX;
#pragma unroll
	for (int list = 0; list < 3; ++list)
	{
		const unsigned long long* masks = list == 0 ? now : list == 1 ? entered : left;
		int* prefix = tilePrefix + (size_t)list * count * tiles;
		int carry = 0;
		for (int base = 0; base < tiles; base += 64)
		{
			const int t = base + lane;
			const int c = t < tiles ? tileHits(masks, ((size_t)q * tiles + t) * 4) : 0;
			const int inclusive = waveInclusive(c, lane);
			if (t < tiles)
			{
				prefix[(size_t)q * tiles + t] = carry + inclusive - c;
			}
			carry += __shfl(inclusive, 63);
			if (list == 0 && c > 0 && lowest == INT_MAX)
			{
				// (the lane's tiles ascend: its first tile with a hit holds its lowest slot)
				for (int w = 3; w >= 0; --w)
				{
					const unsigned long long m = masks[((size_t)q * tiles + t) * 4 + w];
					if (m != 0ull)
					{
						lowest = t * S2_BLOCK + w * 64 + (__ffsll((long long)m) - 1);
					}
				}
			}
		}
		sums[list] = carry;
		if (lane == 0)
		{
			totals[(size_t)list * count + q] = carry;
		}
	}
	for (int d = 32; d > 0; d >>= 1)
	{
		const int other = __shfl_xor(lowest, d);
		lowest = other < lowest ? other : lowest;
	}
	if (lane == 0)
	{
		s2amdSensorState* st = states + q;
		st->inside = sums[0], st->entered = sums[1], st->left = sums[2];
		st->lowestShape = lowest == INT_MAX ? -1 : lowest;
	}
}

// block `list`: offsets[list][0 .. count] (query_list.h: listOffsetsKernel) and head[list] = the list's total; block 0 clears head[3]
__global__ __launch_bounds__(64) void sensorOffsetsKernel(const int* totals, int count, int* offsets, int32_t* head)
{
	const int lane = (int)threadIdx.x, list = (int)blockIdx.x;
	const int* in = totals + (size_t)list * count;
	int* out = offsets + (size_t)list * (count + 1);
	int carry = 0;
	for (int base = 0; base < count; base += 64)
	{
		const int q = base + lane;
		const int c = q < count ? in[q] : 0;
		const int inclusive = waveInclusive(c, lane);
		if (q < count)
		{
			out[q] = carry + inclusive - c;
		}
		carry += __shfl(inclusive, 63);
	}
	if (lane == 0)
	{
		out[count] = carry;
		head[list] = carry;
		if (list == 0)
		{
			head[3] = 0;
		}
	}
}

struct SensorLists
{
	const unsigned long long* masks[3];
	void* out[3]; // int32_t entries of list 0, s2amdSensorEvent records of lists 1 and 2
	int capacity[3];
	int wanted; // bit `list`
};

// query_list.h's listWriteKernel over the three lists (blockIdx.y): entries beyond a list's capacity are dropped
__global__ __launch_bounds__(S2_BLOCK) void sensorWriteKernel(SensorLists lists, size_t words, int tiles, int count, const int* tilePrefix, const int* offsets,
															  const s2amdShape* shapes, const PosedSensor* posed)
{
	const int list = (int)blockIdx.y;
	const size_t w = (size_t)blockIdx.x * S2_BLOCK + threadIdx.x;
	if (((lists.wanted >> list) & 1) == 0 || w >= words)
	{
		return;
	}
	const unsigned long long* masks = list == 0 ? lists.masks[0] : list == 1 ? lists.masks[1] : lists.masks[2];
	unsigned long long m = masks[w];
	if (m == 0ull)
	{
		return;
	}
	const int capacity = list == 0 ? lists.capacity[0] : list == 1 ? lists.capacity[1] : lists.capacity[2];
	const int wave = (int)(w & 3);
	const size_t qt = w >> 2;
	const int q = (int)(qt / (size_t)tiles), tile = (int)(qt % (size_t)tiles);
	int at = offsets[(size_t)list * (count + 1) + q] + tilePrefix[(size_t)list * count * tiles + qt];
	for (int v = 0; v < wave; ++v)
	{
		at += __popcll(masks[w - wave + v]);
	}
	const int base = tile * S2_BLOCK + wave * 64;
	int32_t* entries = (int32_t*)lists.out[0];
	int4* events = (int4*)(list == 1 ? lists.out[1] : lists.out[2]);
	const int sensorBody = posed[q].body;
	while (m != 0ull)
	{
		const int bit = __ffsll((long long)m) - 1;
		m &= m - 1ull;
		if (at < capacity)
		{
			const int slot = base + bit;
			if (list == 0)
			{
				entries[at] = slot;
			}
			else
			{
				events[at] = make_int4(q, slot, shapes[slot].body, sensorBody);
			}
		}
		at += 1;
	}
}

int sensorCountOf(const s2amdSolver* s)
{
	return (int)s->hSensors.size();
}

SensorLayout layoutOf(const s2amdSolver* s)
{
	return sensorLayout(sensorCountOf(s), s->shapeCapacity, s->sensorListCapacity);
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->sensorReport, s->hSensorReportHead, sizeof(s->hSensorReportHead), "sensor-report", "s2amd_world_set_sensor_report"} : ReportRef{};
}

void launchPose(s2amdSolver* s, const SensorLayout& l, int count)
{
	char* base = (char*)s->sensorReport.block.p;
	sensorPoseKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, s->stream>>>((const s2amdSensor*)(base + l.sensors), count, (const s2amdBody*)s->dBodies.p,
																			   (const float2*)s->dOrigins.p, s->bodyCapacity, (PosedSensor*)(base + l.posed),
																			   (s2amdSensorState*)(base + l.states));
}

// "before" := the rule as the resident world and the list stand now: the list into the block, the poses, the now word alone
int sensorReportRestate(s2amdSolver* s)
{
	const int count = sensorCountOf(s);
	const SensorLayout l = layoutOf(s);
	if (count <= 0 || s->sensorReport.block.p == nullptr || s->sensorReport.block.bytes < l.total)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	char* base = (char*)s->sensorReport.block.p;
	// (waited for: the caller's next s2amd_world_set_sensors replaces the vector this copy reads)
	HIP_TRY(hipMemcpyAsync(base + l.sensors, s->hSensors.data(), (size_t)count * sizeof(s2amdSensor), hipMemcpyHostToDevice, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	launchPose(s, l, count);
	if (l.tiles > 0)
	{
		const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
		unsigned long long* now = (unsigned long long*)(base + l.masks[s->sensorNowSet]);
		sensorMaskKernel<true><<<dim3((unsigned)l.tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, s->stream>>>(
			(const s2amdShape*)s->dShapes.p, s->shapeCapacity, l.tiles, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity,
			(const PosedSensor*)(base + l.posed), count, nullptr, now, nullptr, nullptr);
	}
	HIP_TRY(hipGetLastError());
	return S2AMD_OK;
}

bool validSensor(const s2amdSensor& q)
{
	if (q.count < 1 || q.count > S2_NP_MAX_VERTS || (q.flags & ~S2_SENSOR_KNOWN_FLAGS) != 0)
	{
		return false;
	}
	bool finite = std::isfinite(q.radius) && std::isfinite(q.margin) && std::isfinite(q.position[0]) && std::isfinite(q.position[1]) && std::isfinite(q.rot[0]) &&
				  std::isfinite(q.rot[1]);
	for (int i = 0; i < q.count; ++i)
	{
		finite = finite && std::isfinite(q.vertices[i][0]) && std::isfinite(q.vertices[i][1]);
	}
	return finite && q.radius >= 0.0f && q.margin >= 0.0f;
}

// one list of the last step for a getter: from the block where the step's list holds it, else written again from the kept masks into
// the query scratch (one more launch); enqueues the copy to `out`, the caller waits
int enqueueListFetch(s2amdSolver* s, int list, int total, void* out)
{
	if (total <= 0)
	{
		return S2AMD_OK;
	}
	const SensorLayout l = layoutOf(s);
	const int count = sensorCountOf(s);
	char* base = (char*)s->sensorReport.block.p;
	const size_t size = list == 0 ? sizeof(int32_t) : sizeof(s2amdSensorEvent);
	const char* from = base + (list == 0 ? l.inside : list == 1 ? l.entered : l.left);
	HIP_TRY(hipSetDevice(s->device));
	if (total > l.lists)
	{
		if (int rc = s->dQuery.ensure((size_t)total * size))
		{
			return rc;
		}
		SensorLists lists{};
		lists.masks[0] = (const unsigned long long*)(base + l.masks[s->sensorNowSet]);
		lists.masks[1] = (const unsigned long long*)(base + l.masks[2]);
		lists.masks[2] = (const unsigned long long*)(base + l.masks[3]);
		lists.out[0] = lists.out[1] = lists.out[2] = s->dQuery.p;
		lists.capacity[0] = lists.capacity[1] = lists.capacity[2] = total;
		lists.wanted = 1 << list;
		sensorWriteKernel<<<dim3(gridFor(l.words).x, 3), dim3(S2_BLOCK), 0, s->stream>>>(lists, l.words, l.tiles, count, (const int*)(base + l.prefix),
																							(const int*)(base + l.offsets), (const s2amdShape*)s->dShapes.p,
																							(const PosedSensor*)(base + l.posed));
		HIP_TRY(hipGetLastError());
		from = (const char*)s->dQuery.p;
	}
	HIP_TRY(hipMemcpyAsync(out, from, (size_t)total * size, hipMemcpyDeviceToHost, s->stream));
	return S2AMD_OK;
}

} // namespace

int sensorReportPrepare(s2amdSolver* s)
{
	if (!reportPrepareBegin(s, s->sensorReport))
	{
		return S2AMD_OK;
	}
	if ((size_t)sensorCountOf(s) * (size_t)std::max(s->shapeCapacity, 0) > (size_t)INT32_MAX)
	{
		return fail(S2AMD_E_INVALID, "sensor report: sensors x shape slots beyond 2^31");
	}
	const SensorLayout l = layoutOf(s);
	const int rc = reportPrepareBlock(s->sensorReport, l.total, l.head);
	return rc ? rc : sensorReportRestate(s);
}

int sensorReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->sensorReport;
	const int flags = r.flags;
	const int count = sensorCountOf(s);
	const SensorLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "sensor"))
	{
		return rc;
	}
	if (count > 0)
	{
		hipStream_t st = s->stream;
		char* base = (char*)r.block.p;
		const s2amdShape* shapes = (const s2amdShape*)s->dShapes.p;
		const PosedSensor* posed = (const PosedSensor*)(base + l.posed);
		unsigned long long* before = (unsigned long long*)(base + l.masks[s->sensorNowSet]);
		unsigned long long* now = (unsigned long long*)(base + l.masks[s->sensorNowSet ^ 1]);
		unsigned long long* entered = (unsigned long long*)(base + l.masks[2]);
		unsigned long long* left = (unsigned long long*)(base + l.masks[3]);
		launchPose(s, l, count);
		if (l.tiles > 0)
		{
			const int chunks = (count + S2_QUERY_CHUNK - 1) / S2_QUERY_CHUNK;
			sensorMaskKernel<false><<<dim3((unsigned)l.tiles, (unsigned)chunks), dim3(S2_BLOCK), 0, st>>>(shapes, s->shapeCapacity, l.tiles, (const s2amdBody*)s->dBodies.p,
																										 (const float2*)s->dOrigins.p, s->bodyCapacity, posed, count, before, now,
																										 entered, left);
			s->sensorNowSet ^= 1; // (per reported step: this is enqueued once, behind the attempt that stands)
		}
		sensorPrefixKernel<<<dim3((unsigned)((count + 3) / 4)), dim3(S2_BLOCK), 0, st>>>(now, entered, left, count, l.tiles, (int*)(base + l.prefix), (int*)(base + l.totals),
																						 (s2amdSensorState*)(base + l.states));
		sensorOffsetsKernel<<<dim3(3), dim3(64), 0, st>>>((const int*)(base + l.totals), count, (int*)(base + l.offsets), (int32_t*)(base + l.head));
		SensorLists lists{};
		lists.masks[0] = now, lists.masks[1] = entered, lists.masks[2] = left;
		lists.out[0] = base + l.inside, lists.out[1] = base + l.entered, lists.out[2] = base + l.left;
		lists.capacity[0] = lists.capacity[1] = lists.capacity[2] = l.lists;
		lists.wanted = ((flags & S2AMD_SENSOR_REPORT_INSIDE) != 0 ? 1 : 0) | ((flags & S2AMD_SENSOR_REPORT_EVENTS) != 0 ? 6 : 0);
		if (lists.wanted != 0 && l.words > 0 && l.lists > 0)
		{
			sensorWriteKernel<<<dim3(gridFor(l.words).x, 3), dim3(S2_BLOCK), 0, st>>>(lists, l.words, l.tiles, count, (const int*)(base + l.prefix), (const int*)(base + l.offsets),
																					  shapes, posed);
		}
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (no sensors: nothing is launched, and the head is known here)
		s->hSensorReportHead[0] = s->hSensorReportHead[1] = s->hSensorReportHead[2] = s->hSensorReportHead[3] = 0;
	}
	r.stepFlags = flags;
	r.headKnown = count <= 0;
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_sensors(s2amdSolver* s, const s2amdSensor* sensors, int32_t count)
{
	if (int rc = listArgs(s, sensors, count, S2AMD_MAX_SENSORS))
	{
		return rc;
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validSensor(sensors[i]) || (s->worldResident && sensors[i].body >= s->bodyCapacity))
		{
			return fail(S2AMD_E_INVALID, "sensor " + std::to_string(i) +
											 " is invalid (count outside 1..8, a NaN or infinite field, a negative radius or margin, unknown flag bits, a body outside the body array)");
		}
	}
	if (s->worldResident && (size_t)count * (size_t)std::max(s->shapeCapacity, 0) > (size_t)INT32_MAX)
	{
		return fail(S2AMD_E_INVALID, "sensor report: sensors x shape slots beyond 2^31");
	}
	// "before" of the next step is taken under the new list: the change itself is no event; the last step's report is void
	std::vector<s2amdSensor> next(sensors, sensors + count);
	return listSwapIn(s, [&] { next.swap(s->hSensors); }, sensorReportPrepare);
}

int s2amd_world_set_sensor_report(s2amdSolver* s, int32_t flags, int32_t listCapacity)
{
	if (!s)
	{
		return fail(S2AMD_E_INVALID, "null solver");
	}
	if ((flags & ~S2_SENSOR_REPORT_KNOWN) != 0)
	{
		return fail(S2AMD_E_INVALID, "unknown sensor-report flag bits");
	}
	if (listCapacity < 0)
	{
		return fail(S2AMD_E_INVALID, "sensor report: listCapacity < 0");
	}
	const bool resized = listCapacity != s->sensorListCapacity;
	const bool wasOn = s->sensorReport.flags != 0;
	s->sensorListCapacity = listCapacity;
	if (resized)
	{
		// lists of another size are another layout of the block: the last step's report, laid out under the old one, is void
		s->sensorReport.stepFlags = 0;
		s->sensorReport.headKnown = false;
	}
	const int rc = reportSet(ref(s), flags, S2_SENSOR_REPORT_KNOWN, sensorReportPrepare);
	// (... and where the report stays on, the block is laid out again now, as if the report were turned on again)
	return rc == S2AMD_OK && resized && wasOn && flags != 0 ? sensorReportPrepare(s) : rc;
}

int s2amd_world_sensor_inside(s2amdSolver* s, int32_t* offsets, int32_t* shapes, int32_t capacity, int32_t* total)
{
	if (!s || !offsets || !total || capacity < 0 || (capacity > 0 && !shapes))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	int rc = reportHeadFor(ref(s), S2AMD_SENSOR_REPORT_INSIDE, "s2amd_world_sensor_inside");
	if (rc)
	{
		return rc;
	}
	const int count = sensorCountOf(s);
	*total = s->hSensorReportHead[0];
	if (count <= 0)
	{
		offsets[0] = 0;
		return S2AMD_OK;
	}
	const SensorLayout l = layoutOf(s);
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipMemcpyAsync(offsets, (const char*)s->sensorReport.block.p + l.offsets, ((size_t)count + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
	if (*total <= capacity && (rc = enqueueListFetch(s, 0, *total, shapes)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return *total > capacity ? fail(S2AMD_E_CAPACITY, "sensor inside buffer too small") : S2AMD_OK;
}

int s2amd_world_sensor_events(s2amdSolver* s, s2amdSensorEvent* entered, int32_t enteredCapacity, int32_t* enteredCount, s2amdSensorEvent* left, int32_t leftCapacity,
							  int32_t* leftCount)
{
	if (!s || !enteredCount || !leftCount || enteredCapacity < 0 || leftCapacity < 0 || (enteredCapacity > 0 && !entered) || (leftCapacity > 0 && !left))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	int rc = reportHeadFor(ref(s), S2AMD_SENSOR_REPORT_EVENTS, "s2amd_world_sensor_events");
	if (rc)
	{
		return rc;
	}
	*enteredCount = s->hSensorReportHead[1];
	*leftCount = s->hSensorReportHead[2];
	if (*enteredCount > enteredCapacity || *leftCount > leftCapacity)
	{
		return fail(S2AMD_E_CAPACITY, "sensor event buffer too small");
	}
	if (*enteredCount + *leftCount == 0)
	{
		return S2AMD_OK;
	}
	// (the two lists share the scratch a rebuilt one lies in: each is waited for before the next is written)
	if ((rc = enqueueListFetch(s, 1, *enteredCount, entered)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	if ((rc = enqueueListFetch(s, 2, *leftCount, left)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

int s2amd_world_sensor_states(s2amdSolver* s, s2amdSensorState* out, int32_t capacity, int32_t* count)
{
	// (the states need no head: their count is the list's)
	const int rc = reportGetPerItem(ref(s), S2AMD_SENSOR_REPORT_STATES, "s2amd_world_sensor_states", "sensor state buffer too small", out, capacity, count, s ? sensorCountOf(s) : 0);
	return rc ? rc : reportCopyOut(s, out, s->sensorReport.block, layoutOf(s).states, *count, sizeof(s2amdSensorState), hipMemcpyDeviceToHost);
}

} // extern "C"
#pragma GCC visibility pop
