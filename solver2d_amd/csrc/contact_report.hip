// Contact report of the resident world (include/solver2d_amd.h: s2amd_world_set_report and its three getters): what s2World_Draw's
// contact pass reads (src/world.c:486-561) -- which contacts touch, where, how hard -- compacted on the device behind stage 4 of
// s2amd_world_step instead of downloaded with the whole world.
//
//   reportCountKernel / reportWriteKernel   one pass over the contact slots in tiles of 256: "touching now" (pair live, manifold with
//                                           points) against the report's own "was touching" byte gives the began / ended / touching
//                                           flags; per-tile counts by wave ballots, then every tile adds up the counts before it and
//                                           writes its entries at their ranks (the shape of movedCountKernel / movedWriteKernel in
//                                           world.hip): three lists in ascending slot order without a sort, and the byte advances.
//   reportBodyKeysKernel -> rocPRIM radix sort -> reportBodyRangesKernel (report_common.h) -> reportBodySumKernel
//                                           the per-body sums: two (body, entry) keys per contact slot (a slot that does not touch sorts
//                                           behind every body), sorted STABLY by body so that a body's entries stay in slot order, then
//                                           one wave per body gathers 64 entries at a time and adds their terms in list order.
//
// The byte array is the report's own (not world.hip's pointBytes, which advance inside the retry loop of s2amd_world_step): the passes
// are enqueued once per step, behind the attempt that stands, so a repeated step reports once.  All device memory is one block sized
// by contactReportPrepare (at upload / set_report); a step allocates nothing and waits for nothing -- the getters do.
#include "report_common.h"

#include <rocprim/device/device_radix_sort.hpp>

#define S2_REPORT_STAGE 128 // terms one wave stages per batch of a body's list: 64 entries, two points each

namespace
{

struct ReportLayout
{
	size_t was, counts, head, began, ended, records, keysIn, keysOut, valsIn, valsOut, ranges, sums, sortTmp, total;
	int tiles;
};

ReportLayout reportLayout(int nc, int nb, size_t sortTmpBytes)
{
	ReportLayout l{};
	size_t at = 0;
	l.tiles = (nc + S2_BLOCK - 1) / S2_BLOCK;
	l.was = reportTake(at, (size_t)nc);
	l.counts = reportTake(at, (size_t)3 * l.tiles * sizeof(int));
	l.head = reportTake(at, 4 * sizeof(int32_t));
	l.began = reportTake(at, (size_t)nc * sizeof(int32_t));
	l.ended = reportTake(at, (size_t)nc * sizeof(int32_t));
	l.records = reportTake(at, (size_t)nc * sizeof(s2amdTouchingContact));
	l.keysIn = reportTake(at, (size_t)2 * nc * sizeof(uint32_t));
	l.keysOut = reportTake(at, (size_t)2 * nc * sizeof(uint32_t));
	l.valsIn = reportTake(at, (size_t)2 * nc * sizeof(int));
	l.valsOut = reportTake(at, (size_t)2 * nc * sizeof(int));
	l.ranges = reportTake(at, (size_t)2 * nb * sizeof(int));
	l.sums = reportTake(at, (size_t)nb * sizeof(s2amdBodyContactSum));
	l.sortTmp = reportTake(at, sortTmpBytes);
	l.total = at;
	return l;
}

__global__ __launch_bounds__(S2_BLOCK) void reportInitKernel(const s2amdContact* contacts, int n, uint8_t* was)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		was[i] = contacts[i].pointCount > 0 ? 1 : 0;
	}
}

__global__ __launch_bounds__(S2_BLOCK) void reportSetKernel(const int32_t* slots, int n, const s2amdContact* newContacts, uint8_t* was)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		was[slots[i]] = newContacts[i].pointCount > 0 ? 1 : 0;
	}
}

// bit 0: touching now, bit 1: was touching before the step
S2_DEV int touchBits(const s2amdContact* contacts, const s2amdPairState* pairs, const uint8_t* was, int n, int i)
{
	if (i >= n)
	{
		return 0;
	}
	const int now = pairs[i].shapeA >= 0 && contacts[i].pointCount > 0 ? 1 : 0;
	return now | (was[i] != 0 ? 2 : 0);
}

// counts[0..tiles) began, [tiles..2 tiles) ended, [2 tiles..3 tiles) touching
__global__ __launch_bounds__(S2_BLOCK) void reportCountKernel(const s2amdContact* contacts, const s2amdPairState* pairs, const uint8_t* was, int n, int tiles,
															  int* counts)
{
	__shared__ int waves[3][S2_BLOCK / 64];
	const int bits = touchBits(contacts, pairs, was, n, (int)(blockIdx.x * blockDim.x + threadIdx.x));
	const unsigned long long began = __ballot(bits == 1), ended = __ballot(bits == 2), touching = __ballot((bits & 1) != 0);
	if ((threadIdx.x & 63) == 0)
	{
		waves[0][threadIdx.x >> 6] = __popcll(began);
		waves[1][threadIdx.x >> 6] = __popcll(ended);
		waves[2][threadIdx.x >> 6] = __popcll(touching);
	}
	__syncthreads();
	if (threadIdx.x < 3)
	{
		int total = 0;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			total += waves[threadIdx.x][w];
		}
		counts[(int)threadIdx.x * tiles + (int)blockIdx.x] = total;
	}
}

// head[0..2] = {began, ended, touching} counts of the step; `flags`: which lists are wanted (the byte advances in any case)
__global__ __launch_bounds__(S2_BLOCK) void reportWriteKernel(const s2amdContact* contacts, const s2amdPairState* pairs, uint8_t* was, int n, int tiles,
															  const int* counts, const s2amdBody* bodies, const float2* origins, int nb, int flags, int32_t* head,
															  int32_t* beganOut, int32_t* endedOut, s2amdTouchingContact* records)
{
	__shared__ int waves[3][S2_BLOCK / 64];
	__shared__ int base[3];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const int bits = touchBits(contacts, pairs, was, n, i);
	const bool isBegan = bits == 1, isEnded = bits == 2, isTouching = (bits & 1) != 0;
	const unsigned long long began = __ballot(isBegan), ended = __ballot(isEnded), touching = __ballot(isTouching);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	if (lane == 0)
	{
		waves[0][wave] = __popcll(began);
		waves[1][wave] = __popcll(ended);
		waves[2][wave] = __popcll(touching);
	}
	if (wave < 3)
	{
		// the tiles before this one: wave w adds up list w's counts
		int partial = tileCountsBefore(counts, tiles, wave, (int)blockIdx.x, lane);
		for (int d = 32; d > 0; d >>= 1)
		{
			partial += __shfl_xor(partial, d);
		}
		if (lane == 0)
		{
			base[wave] = partial;
		}
	}
	__syncthreads();
	int at[3] = {base[0], base[1], base[2]};
	for (int w = 0; w < wave; ++w)
	{
		at[0] += waves[0][w], at[1] += waves[1][w], at[2] += waves[2][w];
	}
	const unsigned long long lower = (1ull << lane) - 1ull;
	at[0] += __popcll(began & lower), at[1] += __popcll(ended & lower), at[2] += __popcll(touching & lower);
	if ((int)blockIdx.x == tiles - 1 && threadIdx.x == blockDim.x - 1)
	{
		head[0] = at[0] + (isBegan ? 1 : 0);
		head[1] = at[1] + (isEnded ? 1 : 0);
		head[2] = at[2] + (isTouching ? 1 : 0);
		head[3] = 0;
	}
	if (i >= n)
	{
		return;
	}
	was[i] = (uint8_t)(bits & 1);
	if ((flags & S2AMD_REPORT_TOUCH) != 0)
	{
		if (isBegan)
		{
			beganOut[at[0]] = i;
		}
		if (isEnded)
		{
			endedOut[at[1]] = i;
		}
	}
	if ((flags & S2AMD_REPORT_CONTACTS) != 0 && isTouching)
	{
		// one 64-byte record per lane: a full line each
		const s2amdContact& c = contacts[i];
		s2amdTouchingContact r{};
		r.slot = i, r.bodyA = c.bodyA, r.bodyB = c.bodyB;
		const int pc = c.pointCount < 2 ? c.pointCount : 2;
		r.pointCount = (uint8_t)pc;
		r.normal[0] = c.normal[0], r.normal[1] = c.normal[1];
		float2 origin = make_float2(0.0f, 0.0f), rot = make_float2(0.0f, 1.0f);
		if (c.bodyA >= 0 && c.bodyA < nb)
		{
			origin = origins[c.bodyA];
			rot = make_float2(bodies[c.bodyA].rot[0], bodies[c.bodyA].rot[1]);
		}
		for (int j = 0; j < 2; ++j)
		{
			if (j < pc)
			{
				const s2amdManifoldPoint& mp = c.points[j];
				const float2 p = transformPoint(origin, rot, make_float2(mp.localAnchorA[0], mp.localAnchorA[1]));
				r.persisted[j] = pairs[i].persisted[j];
				r.point[j][0] = p.x, r.point[j][1] = p.y;
				r.separation[j] = mp.separation;
				r.normalImpulse[j] = mp.normalImpulse;
				r.tangentImpulse[j] = mp.tangentImpulse;
			}
		}
		records[at[2]] = r;
	}
}

// entry e = 2 * slot + side (0: the slot's bodyA, 1: its bodyB); key = that body where the slot touches, else nb
__global__ __launch_bounds__(S2_BLOCK) void reportBodyKeysKernel(const s2amdContact* contacts, const s2amdPairState* pairs, int nc, int nb, uint32_t* keys, int* vals)
{
	const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (e >= 2 * nc)
	{
		return;
	}
	const int slot = e >> 1;
	const bool touching = pairs[slot].shapeA >= 0 && contacts[slot].pointCount > 0;
	const int body = (e & 1) != 0 ? contacts[slot].bodyB : contacts[slot].bodyA;
	keys[e] = touching && body >= 0 && body < nb ? (uint32_t)body : (uint32_t)nb;
	vals[e] = e;
}

// One wave per body slot.  64 entries of the body's run are gathered at once, their points' terms -- {P.x, P.y, normalImpulse}, P negated
// where the body is the contact's bodyA -- compacted into the wave's staging rows in list order (point 0 before point 1), then lanes 0, 1
// and 2 add one row each in that order.  A body with thousands of entries (a drum, the ground) costs one dependent add per term instead
// of one dependent global load.
__global__ __launch_bounds__(S2_BLOCK) void reportBodySumKernel(const s2amdContact* contacts, const int* vals, const int* ranges, int nb, s2amdBodyContactSum* sums)
{
	__shared__ __attribute__((aligned(16))) float stageAll[S2_BLOCK / 64][3 * S2_REPORT_STAGE];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int body = (int)blockIdx.x * (S2_BLOCK / 64) + wave;
	if (body >= nb)
	{
		return; // (the whole wave: the kernel has no block-wide barrier)
	}
	float* stage = stageAll[wave];
	const int start = ranges[2 * body], count = ranges[2 * body + 1] - start;
	const int row = lane < 2 ? lane : 2;
	float acc = 0.0f;
	for (int base = 0; base < count; base += 64)
	{
		const bool in = base + lane < count;
		float2 p0 = make_float2(0.0f, 0.0f), p1 = p0;
		float n0 = 0.0f, n1 = 0.0f;
		int pc = 0;
		if (in)
		{
			const int entry = vals[start + base + lane];
			const s2amdContact& c = contacts[entry >> 1];
			const bool isA = (entry & 1) == 0;
			const float nx = c.normal[0], ny = c.normal[1];
			const float tx = ny, ty = -nx; // s2RightPerp(normal)
			pc = c.pointCount < 2 ? c.pointCount : 2;
			n0 = c.points[0].normalImpulse, n1 = c.points[1].normalImpulse;
			const float t0 = c.points[0].tangentImpulse, t1 = c.points[1].tangentImpulse;
			p0 = make_float2(n0 * nx + t0 * tx, n0 * ny + t0 * ty);
			p1 = make_float2(n1 * nx + t1 * tx, n1 * ny + t1 * ty);
			if (isA)
			{
				p0 = make_float2(-p0.x, -p0.y), p1 = make_float2(-p1.x, -p1.y);
			}
		}
		const bool v0 = in && pc > 0, v1 = in && pc > 1;
		const unsigned long long b0 = __ballot(v0), b1 = __ballot(v1), lower = (1ull << lane) - 1ull;
		const int at0 = __popcll(b0 & lower) + __popcll(b1 & lower), at1 = at0 + (v0 ? 1 : 0);
		if (v0)
		{
			stage[at0] = p0.x, stage[S2_REPORT_STAGE + at0] = p0.y, stage[2 * S2_REPORT_STAGE + at0] = n0;
		}
		if (v1)
		{
			stage[at1] = p1.x, stage[S2_REPORT_STAGE + at1] = p1.y, stage[2 * S2_REPORT_STAGE + at1] = n1;
		}
		const int n = __builtin_amdgcn_readfirstlane(__popcll(b0) + __popcll(b1));
		waveLdsOrder();
		acc = addInOrder(acc, stage + row * S2_REPORT_STAGE, n);
		waveLdsOrder();
	}
	const float ax = laneOf(acc, 0), ay = laneOf(acc, 1), an = laneOf(acc, 2);
	if (lane == 0)
	{
		s2amdBodyContactSum out;
		out.impulse[0] = ax, out.impulse[1] = ay;
		out.normalImpulse = an;
		out.touching = count;
		sums[body] = out;
	}
}

ReportLayout layoutOf(const s2amdSolver* s)
{
	return reportLayout(s->contactCapacity, s->bodyCapacity, s->contactReport.sortTmpBytes);
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->contactReport, s->hReportHead, sizeof(s->hReportHead), "report", "s2amd_world_set_report"} : ReportRef{};
}

// where a piece of the block lies, for a getter (0 for the null solver it will refuse)
size_t at(const s2amdSolver* s, size_t ReportLayout::*piece)
{
	return s ? layoutOf(s).*piece : 0;
}

} // namespace

int contactReportPrepare(s2amdSolver* s)
{
	ReportState& r = s->contactReport;
	if (!reportPrepareBegin(s, r))
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	const int nc = s->contactCapacity, nb = s->bodyCapacity;
	size_t tmp = 0;
	if (nc > 0)
	{
		HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)2 * nc, 0, bodyKeyBits(nb), s->stream));
	}
	r.sortTmpBytes = tmp;
	const ReportLayout l = layoutOf(s);
	int rc = reportPrepareBlock(r, l.total, l.head);
	if (rc)
	{
		return rc;
	}
	if (nc > 0)
	{
		reportInitKernel<<<gridFor((size_t)nc), dim3(S2_BLOCK), 0, s->stream>>>((const s2amdContact*)s->dContacts.p, nc, (uint8_t*)r.block.p + l.was);
		HIP_TRY(hipGetLastError());
	}
	return S2AMD_OK;
}

int reportNoteSetContacts(s2amdSolver* s, const int32_t* dSlots, int count, const s2amdContact* dNewContacts)
{
	if (s->contactReport.flags == 0 || count <= 0 || s->contactReport.block.p == nullptr)
	{
		return S2AMD_OK;
	}
	const ReportLayout l = layoutOf(s);
	reportSetKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, s->stream>>>(dSlots, count, dNewContacts, (uint8_t*)s->contactReport.block.p + l.was);
	HIP_TRY(hipGetLastError());
	return S2AMD_OK;
}

int contactReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->contactReport;
	const int flags = r.flags;
	const int nc = s->contactCapacity, nb = s->bodyCapacity;
	const ReportLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "contact"))
	{
		return rc;
	}
	hipStream_t st = s->stream;
	char* base = (char*)r.block.p;
	const s2amdContact* contacts = (const s2amdContact*)s->dContacts.p;
	const s2amdPairState* pairs = (const s2amdPairState*)s->dPairs.p;
	if (nc > 0)
	{
		reportCountKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(contacts, pairs, (const uint8_t*)(base + l.was), nc, l.tiles, (int*)(base + l.counts));
		reportWriteKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(contacts, pairs, (uint8_t*)(base + l.was), nc, l.tiles, (const int*)(base + l.counts),
																			   (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, nb, flags, (int32_t*)(base + l.head),
																			   (int32_t*)(base + l.began), (int32_t*)(base + l.ended), (s2amdTouchingContact*)(base + l.records));
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (a world without contact slots launches no tile: its head is known here)
		memset(s->hReportHead, 0, sizeof(s->hReportHead));
	}
	if ((flags & S2AMD_REPORT_BODY_SUMS) != 0 && nb > 0)
	{
		if (nc > 0)
		{
			size_t tmp = r.sortTmpBytes;
			reportBodyKeysKernel<<<gridFor((size_t)2 * nc), dim3(S2_BLOCK), 0, st>>>(contacts, pairs, nc, nb, (uint32_t*)(base + l.keysIn), (int*)(base + l.valsIn));
			HIP_TRY(hipGetLastError());
			HIP_TRY(rocprim::radix_sort_pairs((void*)(base + l.sortTmp), tmp, (uint32_t*)(base + l.keysIn), (uint32_t*)(base + l.keysOut), (int*)(base + l.valsIn),
											  (int*)(base + l.valsOut), (size_t)2 * nc, 0, bodyKeyBits(nb), st));
		}
		HIP_TRY(hipMemsetAsync(base + l.ranges, 0, (size_t)2 * nb * sizeof(int), st));
		if (nc > 0)
		{
			reportBodyRangesKernel<<<gridFor((size_t)2 * nc), dim3(S2_BLOCK), 0, st>>>((const uint32_t*)(base + l.keysOut), 2 * nc, nb, (int*)(base + l.ranges));
		}
		reportBodySumKernel<<<dim3((unsigned)((nb + S2_BLOCK / 64 - 1) / (S2_BLOCK / 64))), dim3(S2_BLOCK), 0, st>>>(contacts, (const int*)(base + l.valsOut), (const int*)(base + l.ranges),
																											  nb, (s2amdBodyContactSum*)(base + l.sums));
		HIP_TRY(hipGetLastError());
	}
	r.stepFlags = flags;
	r.headKnown = nc <= 0;
	return S2AMD_OK;
}

const s2amdBodyContactSum* contactReportBodySums(const s2amdSolver* s)
{
	const ReportState& r = s->contactReport;
	if ((r.stepFlags & S2AMD_REPORT_BODY_SUMS) == 0 || s->bodyCapacity <= 0 || r.block.p == nullptr)
	{
		return nullptr;
	}
	return (const s2amdBodyContactSum*)((const char*)r.block.p + layoutOf(s).sums);
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2AMD_REPORT_TOUCH | S2AMD_REPORT_CONTACTS | S2AMD_REPORT_BODY_SUMS, contactReportPrepare);
}

int s2amd_world_touch_events(s2amdSolver* s, int32_t* began, int32_t beganCapacity, int32_t* beganCount, int32_t* ended, int32_t endedCapacity, int32_t* endedCount)
{
	return reportGetEvents(ref(s), S2AMD_REPORT_TOUCH, "s2amd_world_touch_events", "touch event buffer too small", 0, at(s, &ReportLayout::began), at(s, &ReportLayout::ended), began,
						   beganCapacity, beganCount, ended, endedCapacity, endedCount);
}

int s2amd_world_touching(s2amdSolver* s, s2amdTouchingContact* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_REPORT_CONTACTS, "s2amd_world_touching", "touching-contact buffer too small", 2, at(s, &ReportLayout::records), sizeof(*out), out, capacity,
						 count);
}

int s2amd_world_body_sums(s2amdSolver* s, s2amdBodyContactSum* out, int32_t bodyCapacity)
{
	return reportGetBodyArray(ref(s), S2AMD_REPORT_BODY_SUMS, "s2amd_world_body_sums", at(s, &ReportLayout::sums), sizeof(*out), out, bodyCapacity);
}

} // extern "C"
#pragma GCC visibility pop
