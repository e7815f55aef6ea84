// Joint report of the resident world (include/solver2d_amd.h: s2amd_world_set_joint_report and its four getters): what s2World_Draw's
// joint pass (src/joint.c:469-505, src/revolute_joint.c:942-984) and s2RevoluteJoint_GetMotorTorque read -- anchors, angle, speed,
// limit contacts, impulses -- compacted on the device behind stage 4 of s2amd_world_step and behind the contact report, instead of
// derived on the host from a download of the joint and body arrays.  The shape is contact_report.hip's:
//
//   jointCountKernel / jointWriteKernel   one pass each over the joint slots in tiles of 256.  "At its lower / upper limit now" (revolute,
//                                         enableLimit, stored lowerImpulse / upperImpulse > 0) against the report's own state byte gives up
//                                         to two began and two ended codes per slot; `live` gives the record list.  Per-tile counts by wave
//                                         ballots, every tile adds up the counts before it (report_common.h: tileCountsBefore) and writes
//                                         its entries at their ranks: three ascending lists without a sort or an atomic, and the byte
//                                         advances.  The count pass also leaves one summary partial per tile -- revolute / atLower /
//                                         atUpper counts and the tile's largest anchor gap as (g, slot) -- which the fourth wave of the
//                                         write pass's last tile reduces: (g, slot) under "larger g, then lower slot" is a total order, so
//                                         the result does not depend on how the reduction is bracketed.
//   jointBodySumKernel                    one wave per body over the body -> joint adjacency: 64 entries gathered at a time, their terms
//                                         staged in the wave's LDS rows in list order, lanes 0, 1 and 2 add one row each in that order.
//
// The adjacency -- entries 2 * slot + side keyed by body, sorted STABLY by body with rocPRIM's radix sort, then body ranges
// (report_common.h: reportBodyRangesKernel) -- is built by jointReportPrepare, at s2amd_world_upload and when the report is turned on,
// not per step: no resident-world call changes a joint's type, bodyA or bodyB between uploads.  The state bytes are the report's own
// and the passes are enqueued once per step, behind the attempt that stands: a repeated step reports once.  All device memory is one
// block sized by jointReportPrepare; a step allocates nothing and waits for nothing -- the getters do.
#include "report_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace
{

// what one tile of the count pass contributes to s2amdJointSummary
struct JointTilePartial
{
	int32_t revolute, atLower, atUpper, maxGapSlot;
	float maxGap;
	int32_t pad[3];
};

// the head of the report as the getters fetch it (solver_internal.h: hJointReportHead)
struct JointReportHead
{
	int32_t counts[4]; // {live, began, ended, 0}
	s2amdJointSummary summary;
};

struct JointReportLayout
{
	size_t was, counts, partials, head, began, ended, records, keysIn, keysOut, valsIn, valsOut, ranges, sums, sortTmp, total;
	int tiles;
};

JointReportLayout jointReportLayout(int nj, int nb, size_t sortTmpBytes)
{
	JointReportLayout l{};
	size_t at = 0;
	l.tiles = (nj + S2_BLOCK - 1) / S2_BLOCK;
	l.was = reportTake(at, (size_t)nj);
	l.counts = reportTake(at, (size_t)3 * l.tiles * sizeof(int));
	l.partials = reportTake(at, (size_t)l.tiles * sizeof(JointTilePartial));
	l.head = reportTake(at, sizeof(JointReportHead));
	l.began = reportTake(at, (size_t)2 * nj * sizeof(int32_t));
	l.ended = reportTake(at, (size_t)2 * nj * sizeof(int32_t));
	l.records = reportTake(at, (size_t)nj * sizeof(s2amdJointState));
	l.keysIn = reportTake(at, (size_t)2 * nj * sizeof(uint32_t));
	l.keysOut = reportTake(at, (size_t)2 * nj * sizeof(uint32_t));
	l.valsIn = reportTake(at, (size_t)2 * nj * sizeof(int));
	l.valsOut = reportTake(at, (size_t)2 * nj * sizeof(int));
	l.ranges = reportTake(at, (size_t)2 * nb * sizeof(int));
	l.sums = reportTake(at, (size_t)nb * sizeof(s2amdBodyJointSum));
	l.sortTmp = reportTake(at, sortTmpBytes);
	l.total = at;
	return l;
}

// bit 0: at the lower limit, bit 1: at the upper limit -- of what the solver stored
S2_DEV int limitBits(const s2amdJoint& j)
{
	if (j.type != S2AMD_JOINT_REVOLUTE || j.enableLimit == 0)
	{
		return 0;
	}
	return (j.lowerImpulse > 0.0f ? 1 : 0) | (j.upperImpulse > 0.0f ? 2 : 0);
}

struct Pose
{
	float2 origin, rot; // rot = {s, c}
	float w;
};

S2_DEV Pose poseOf(const s2amdBody* bodies, const float2* origins, int nb, int body)
{
	Pose p;
	p.origin = make_float2(0.0f, 0.0f), p.rot = make_float2(0.0f, 1.0f), p.w = 0.0f;
	if (body >= 0 && body < nb)
	{
		p.origin = origins[body];
		p.rot = make_float2(bodies[body].rot[0], bodies[body].rot[1]);
		p.w = bodies[body].angularVelocity;
	}
	return p;
}

// "larger g, then lower slot": a total order, (-1, -1) is below every gap that is a number
S2_DEV void gapMax(float& g, int& slot, float otherG, int otherSlot)
{
	if (otherG > g || (otherG == g && otherSlot < slot))
	{
		g = otherG, slot = otherSlot;
	}
}

S2_DEV void gapMaxOverWave(float& g, int& slot)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const float otherG = __shfl_xor(g, d);
		const int otherSlot = __shfl_xor(slot, d);
		gapMax(g, slot, otherG, otherSlot);
	}
}

__global__ __launch_bounds__(S2_BLOCK) void jointInitKernel(const s2amdJoint* joints, int n, uint8_t* was)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		was[i] = (uint8_t)limitBits(joints[i]);
	}
}

// counts[0..tiles) live, [tiles..2 tiles) began codes, [2 tiles..3 tiles) ended codes; partials[tile]
// Reads per slot: the 92-byte joint record and its state byte; per live revolute joint also origin and rot of its two bodies.
__global__ __launch_bounds__(S2_BLOCK) void jointCountKernel(const s2amdJoint* joints, const uint8_t* was, int n, int tiles, const s2amdBody* bodies,
															 const float2* origins, int nb, int* counts, JointTilePartial* partials)
{
	__shared__ int waves[6][S2_BLOCK / 64];
	__shared__ float waveGap[S2_BLOCK / 64];
	__shared__ int waveGapSlot[S2_BLOCK / 64];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	bool live = false, revolute = false;
	int now = 0, before = 0;
	float g = -1.0f;
	int gSlot = -1;
	if (i < n)
	{
		const s2amdJoint& j = joints[i];
		live = j.type != S2AMD_JOINT_FREE;
		revolute = j.type == S2AMD_JOINT_REVOLUTE;
		now = limitBits(j);
		before = was[i];
		if (revolute)
		{
			const Pose a = poseOf(bodies, origins, nb, j.bodyA), b = poseOf(bodies, origins, nb, j.bodyB);
			const float2 pa = transformPoint(a.origin, a.rot, make_float2(j.localOriginAnchorA[0], j.localOriginAnchorA[1]));
			const float2 pb = transformPoint(b.origin, b.rot, make_float2(j.localOriginAnchorB[0], j.localOriginAnchorB[1]));
			const float dx = pb.x - pa.x, dy = pb.y - pa.y;
			const float gap = dx * dx + dy * dy;
			if (gap >= 0.0f) // (a NaN never wins)
			{
				g = gap, gSlot = i;
			}
		}
	}
	const int began = now & ~before, ended = before & ~now;
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const int nLive = __popcll(__ballot(live));
	const int nBegan = __popcll(__ballot((began & 1) != 0)) + __popcll(__ballot((began & 2) != 0));
	const int nEnded = __popcll(__ballot((ended & 1) != 0)) + __popcll(__ballot((ended & 2) != 0));
	const int nRevolute = __popcll(__ballot(revolute));
	const int nLower = __popcll(__ballot((now & 1) != 0)), nUpper = __popcll(__ballot((now & 2) != 0));
	gapMaxOverWave(g, gSlot);
	if (lane == 0)
	{
		waves[0][wave] = nLive, waves[1][wave] = nBegan, waves[2][wave] = nEnded;
		waves[3][wave] = nRevolute, waves[4][wave] = nLower, waves[5][wave] = nUpper;
		waveGap[wave] = g, waveGapSlot[wave] = gSlot;
	}
	__syncthreads();
	if (threadIdx.x < 6)
	{
		int total = 0;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			total += waves[threadIdx.x][w];
		}
		if (threadIdx.x < 3)
		{
			counts[(int)threadIdx.x * tiles + (int)blockIdx.x] = total;
		}
		else if (threadIdx.x == 3)
		{
			partials[blockIdx.x].revolute = total;
		}
		else if (threadIdx.x == 4)
		{
			partials[blockIdx.x].atLower = total;
		}
		else
		{
			partials[blockIdx.x].atUpper = total;
		}
	}
	if (threadIdx.x == 6)
	{
		float tg = waveGap[0];
		int ts = waveGapSlot[0];
		for (int w = 1; w < S2_BLOCK / 64; ++w)
		{
			gapMax(tg, ts, waveGap[w], waveGapSlot[w]);
		}
		partials[blockIdx.x].maxGap = tg;
		partials[blockIdx.x].maxGapSlot = ts;
	}
}

// head->counts = {live, began, ended} of the step, head->summary; `flags`: which lists are wanted (the state byte advances in any case).
// Reads per slot what the count pass read (under STATES also angularVelocity of the bodies: 100-odd bytes of joint record and state plus
// 2 x 28 bytes of body state per live joint); writes one full 64-byte line per live joint under STATES and 4 bytes per event.
__global__ __launch_bounds__(S2_BLOCK) void jointWriteKernel(const s2amdJoint* joints, uint8_t* was, int n, int tiles, const int* counts,
															 const JointTilePartial* partials, const s2amdBody* bodies, const float2* origins, int nb, int flags,
															 JointReportHead* head, int32_t* beganOut, int32_t* endedOut, s2amdJointState* records)
{
	__shared__ int waves[3][S2_BLOCK / 64];
	__shared__ int base[3];
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	bool live = false;
	int now = 0, before = 0;
	if (i < n)
	{
		live = joints[i].type != S2AMD_JOINT_FREE;
		now = limitBits(joints[i]);
		before = was[i];
	}
	const int beganBits = now & ~before, endedBits = before & ~now;
	const unsigned long long liveMask = __ballot(live);
	const unsigned long long b0 = __ballot((beganBits & 1) != 0), b1 = __ballot((beganBits & 2) != 0);
	const unsigned long long e0 = __ballot((endedBits & 1) != 0), e1 = __ballot((endedBits & 2) != 0);
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	if (lane == 0)
	{
		waves[0][wave] = __popcll(liveMask);
		waves[1][wave] = __popcll(b0) + __popcll(b1);
		waves[2][wave] = __popcll(e0) + __popcll(e1);
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
	else if ((int)blockIdx.x == tiles - 1)
	{
		// the summary: the idle wave of the last tile adds up the tiles' partials
		int nLive = 0, nRevolute = 0, nLower = 0, nUpper = 0, gSlot = -1;
		float g = -1.0f;
		for (int b = lane; b < tiles; b += 64)
		{
			const JointTilePartial p = partials[b];
			nLive += counts[b];
			nRevolute += p.revolute, nLower += p.atLower, nUpper += p.atUpper;
			gapMax(g, gSlot, p.maxGap, p.maxGapSlot);
		}
		for (int d = 32; d > 0; d >>= 1)
		{
			nLive += __shfl_xor(nLive, d), nRevolute += __shfl_xor(nRevolute, d);
			nLower += __shfl_xor(nLower, d), nUpper += __shfl_xor(nUpper, d);
		}
		gapMaxOverWave(g, gSlot);
		if (lane == 0)
		{
			s2amdJointSummary s{};
			s.liveJoints = nLive, s.revoluteJoints = nRevolute, s.atLower = nLower, s.atUpper = nUpper;
			s.maxGapSlot = gSlot, s.maxGapSquared = g;
			head->summary = s;
		}
	}
	__syncthreads();
	int at[3] = {base[0], base[1], base[2]};
	for (int w = 0; w < wave; ++w)
	{
		at[0] += waves[0][w], at[1] += waves[1][w], at[2] += waves[2][w];
	}
	const unsigned long long lower = (1ull << lane) - 1ull;
	at[0] += __popcll(liveMask & lower);
	at[1] += __popcll(b0 & lower) + __popcll(b1 & lower);
	at[2] += __popcll(e0 & lower) + __popcll(e1 & lower);
	if ((int)blockIdx.x == tiles - 1 && threadIdx.x == blockDim.x - 1)
	{
		head->counts[0] = at[0] + (live ? 1 : 0);
		head->counts[1] = at[1] + (beganBits & 1) + (beganBits >> 1);
		head->counts[2] = at[2] + (endedBits & 1) + (endedBits >> 1);
		head->counts[3] = 0;
	}
	if (i >= n)
	{
		return;
	}
	was[i] = (uint8_t)now;
	if ((flags & S2AMD_JOINT_REPORT_LIMITS) != 0)
	{
		// the lower code of a slot before its upper code
		if ((beganBits & 1) != 0)
		{
			beganOut[at[1]] = 2 * i;
		}
		if ((beganBits & 2) != 0)
		{
			beganOut[at[1] + (beganBits & 1)] = 2 * i + 1;
		}
		if ((endedBits & 1) != 0)
		{
			endedOut[at[2]] = 2 * i;
		}
		if ((endedBits & 2) != 0)
		{
			endedOut[at[2] + (endedBits & 1)] = 2 * i + 1;
		}
	}
	if ((flags & S2AMD_JOINT_REPORT_STATES) != 0 && live)
	{
		// one 64-byte record per lane: a full line each
		const s2amdJoint& j = joints[i];
		s2amdJointState r{};
		r.slot = i, r.type = j.type, r.bodyA = j.bodyA, r.bodyB = j.bodyB;
		const Pose b = poseOf(bodies, origins, nb, j.bodyB);
		const float2 pb = transformPoint(b.origin, b.rot, make_float2(j.localOriginAnchorB[0], j.localOriginAnchorB[1]));
		r.anchorB[0] = pb.x, r.anchorB[1] = pb.y;
		r.impulse[0] = j.impulse[0], r.impulse[1] = j.impulse[1];
		r.motorImpulse = j.motorImpulse;
		if (j.type == S2AMD_JOINT_REVOLUTE)
		{
			const Pose a = poseOf(bodies, origins, nb, j.bodyA);
			const float2 pa = transformPoint(a.origin, a.rot, make_float2(j.localOriginAnchorA[0], j.localOriginAnchorA[1]));
			r.anchorA[0] = pa.x, r.anchorA[1] = pa.y;
			Rot qa, qb;
			qa.s = a.rot.x, qa.c = a.rot.y, qb.s = b.rot.x, qb.c = b.rot.y;
			r.angle = relativeAngle(qb, qa) - j.referenceAngle;
			r.angularSpeed = b.w - a.w;
			r.axialImpulse = (j.motorImpulse + j.lowerImpulse) - j.upperImpulse;
			r.lowerImpulse = j.lowerImpulse, r.upperImpulse = j.upperImpulse;
		}
		else
		{
			// (a mouse joint: what src/joint.c:485-492 draws; its angle and limit impulses are not state)
			r.anchorA[0] = j.targetA[0], r.anchorA[1] = j.targetA[1];
			r.angularSpeed = b.w;
			r.axialImpulse = j.motorImpulse;
		}
		records[at[0]] = r;
	}
}

// entry e = 2 * slot + side (0: the joint's bodyA, 1: its bodyB); key = that body where the entry is a term of its sums, else nb:
// a free slot, a body outside the array, the bodyA of a joint that is not revolute (src/mouse_joint.c applies its impulse to bodyB only)
__global__ __launch_bounds__(S2_BLOCK) void jointBodyKeysKernel(const s2amdJoint* joints, int nj, int nb, uint32_t* keys, int* vals)
{
	const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (e >= 2 * nj)
	{
		return;
	}
	const s2amdJoint& j = joints[e >> 1];
	const bool isB = (e & 1) != 0;
	const int body = isB ? j.bodyB : j.bodyA;
	const bool term = j.type != S2AMD_JOINT_FREE && (isB || j.type == S2AMD_JOINT_REVOLUTE) && body >= 0 && body < nb;
	keys[e] = term ? (uint32_t)body : (uint32_t)nb;
	vals[e] = e;
}

// One wave per body slot.  64 entries of the body's run are gathered at once, their terms -- {impulse.x, impulse.y, axial}, negated where
// the body is the joint's bodyA -- staged in the wave's rows in list order, then lanes 0, 1 and 2 add one row each in that order: a hub
// with hundreds of joints costs one dependent add per term instead of one dependent global load.  Reads 4 bytes of adjacency and 28
// bytes of the joint record per term, writes 16 bytes per body.
__global__ __launch_bounds__(S2_BLOCK) void jointBodySumKernel(const s2amdJoint* joints, const int* vals, const int* ranges, int nb, s2amdBodyJointSum* sums)
{
	__shared__ __attribute__((aligned(16))) float stageAll[S2_BLOCK / 64][3 * 64];
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
		if (base + lane < count)
		{
			const int entry = vals[start + base + lane];
			const s2amdJoint& j = joints[entry >> 1];
			float px = j.impulse[0], py = j.impulse[1];
			float axial = j.type == S2AMD_JOINT_REVOLUTE ? (j.motorImpulse + j.lowerImpulse) - j.upperImpulse : j.motorImpulse;
			if ((entry & 1) == 0)
			{
				px = -px, py = -py, axial = -axial;
			}
			stage[lane] = px, stage[64 + lane] = py, stage[128 + lane] = axial;
		}
		const int n = count - base < 64 ? count - base : 64;
		waveLdsOrder();
		acc = addInOrder(acc, stage + row * 64, n);
		waveLdsOrder();
	}
	const float ax = laneOf(acc, 0), ay = laneOf(acc, 1), aa = laneOf(acc, 2);
	if (lane == 0)
	{
		s2amdBodyJointSum out;
		out.impulse[0] = ax, out.impulse[1] = ay;
		out.axialImpulse = aa;
		out.joints = count;
		sums[body] = out;
	}
}

JointReportLayout layoutOf(const s2amdSolver* s)
{
	return jointReportLayout(s->jointCapacity, s->bodyCapacity, s->jointReport.sortTmpBytes);
}

ReportRef ref(s2amdSolver* s)
{
	static_assert(sizeof(s->hJointReportHead) == sizeof(JointReportHead), "the host copy of the report's head");
	return s ? ReportRef{s, &s->jointReport, &s->hJointReportHead, sizeof(s->hJointReportHead), "joint-report", "s2amd_world_set_joint_report"} : ReportRef{};
}

// where a piece of the block lies, for a getter (0 for the null solver it will refuse)
size_t at(const s2amdSolver* s, size_t JointReportLayout::*piece)
{
	return s ? layoutOf(s).*piece : 0;
}

} // namespace

int jointReportPrepare(s2amdSolver* s)
{
	ReportState& r = s->jointReport;
	if (!reportPrepareBegin(s, r))
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	const int nj = s->jointCapacity, nb = s->bodyCapacity;
	size_t tmp = 0;
	if (nj > 0)
	{
		HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)2 * nj, 0, bodyKeyBits(nb), s->stream));
	}
	r.sortTmpBytes = tmp;
	const JointReportLayout l = layoutOf(s);
	int rc = reportPrepareBlock(r, l.total, l.head);
	if (rc)
	{
		return rc;
	}
	hipStream_t st = s->stream;
	char* base = (char*)r.block.p;
	const s2amdJoint* joints = (const s2amdJoint*)s->dJoints.p;
	if (nb > 0)
	{
		HIP_TRY(hipMemsetAsync(base + l.ranges, 0, (size_t)2 * nb * sizeof(int), st));
	}
	if (nj > 0)
	{
		jointInitKernel<<<gridFor((size_t)nj), dim3(S2_BLOCK), 0, st>>>(joints, nj, (uint8_t*)(base + l.was));
		// the body -> joint adjacency: keys -> stable sort by body -> ranges; valsOut and ranges stay until the next prepare
		jointBodyKeysKernel<<<gridFor((size_t)2 * nj), dim3(S2_BLOCK), 0, st>>>(joints, nj, nb, (uint32_t*)(base + l.keysIn), (int*)(base + l.valsIn));
		HIP_TRY(hipGetLastError());
		HIP_TRY(rocprim::radix_sort_pairs((void*)(base + l.sortTmp), tmp, (uint32_t*)(base + l.keysIn), (uint32_t*)(base + l.keysOut), (int*)(base + l.valsIn),
										  (int*)(base + l.valsOut), (size_t)2 * nj, 0, bodyKeyBits(nb), st));
		if (nb > 0)
		{
			reportBodyRangesKernel<<<gridFor((size_t)2 * nj), dim3(S2_BLOCK), 0, st>>>((const uint32_t*)(base + l.keysOut), 2 * nj, nb, (int*)(base + l.ranges));
		}
		HIP_TRY(hipGetLastError());
	}
	return S2AMD_OK;
}

int jointReportEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->jointReport;
	const int flags = r.flags;
	const int nj = s->jointCapacity, nb = s->bodyCapacity;
	const JointReportLayout l = layoutOf(s);
	if (flags == 0)
	{
		return S2AMD_OK;
	}
	if (int rc = reportEnqueueGuard(r, l.total, "joint"))
	{
		return rc;
	}
	hipStream_t st = s->stream;
	char* base = (char*)r.block.p;
	const s2amdJoint* joints = (const s2amdJoint*)s->dJoints.p;
	const s2amdBody* bodies = (const s2amdBody*)s->dBodies.p;
	if (nj > 0)
	{
		jointCountKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(joints, (const uint8_t*)(base + l.was), nj, l.tiles, bodies, (const float2*)s->dOrigins.p, nb,
																			 (int*)(base + l.counts), (JointTilePartial*)(base + l.partials));
		jointWriteKernel<<<dim3((unsigned)l.tiles), dim3(S2_BLOCK), 0, st>>>(joints, (uint8_t*)(base + l.was), nj, l.tiles, (const int*)(base + l.counts),
																			 (const JointTilePartial*)(base + l.partials), bodies, (const float2*)s->dOrigins.p, nb, flags,
																			 (JointReportHead*)(base + l.head), (int32_t*)(base + l.began), (int32_t*)(base + l.ended),
																			 (s2amdJointState*)(base + l.records));
		HIP_TRY(hipGetLastError());
	}
	else
	{
		// (a world without joint slots launches no tile: its head is known here)
		s->hJointReportHead = {};
		s->hJointReportHead.summary.maxGapSlot = -1, s->hJointReportHead.summary.maxGapSquared = -1.0f;
	}
	if ((flags & S2AMD_JOINT_REPORT_BODY_SUMS) != 0 && nb > 0)
	{
		jointBodySumKernel<<<dim3((unsigned)((nb + S2_BLOCK / 64 - 1) / (S2_BLOCK / 64))), dim3(S2_BLOCK), 0, st>>>(joints, (const int*)(base + l.valsOut), (const int*)(base + l.ranges),
																													 nb, (s2amdBodyJointSum*)(base + l.sums));
		HIP_TRY(hipGetLastError());
	}
	r.stepFlags = flags;
	r.headKnown = nj <= 0; // (a world without joint slots: the head is known without asking the device)
	return S2AMD_OK;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_joint_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2AMD_JOINT_REPORT_STATES | S2AMD_JOINT_REPORT_LIMITS | S2AMD_JOINT_REPORT_BODY_SUMS, jointReportPrepare);
}

int s2amd_world_joint_states(s2amdSolver* s, s2amdJointState* out, int32_t capacity, int32_t* count)
{
	return reportGetList(ref(s), S2AMD_JOINT_REPORT_STATES, "s2amd_world_joint_states", "joint-state buffer too small", 0, at(s, &JointReportLayout::records), sizeof(*out), out,
						 capacity, count);
}

int s2amd_world_joint_limit_events(s2amdSolver* s, int32_t* began, int32_t beganCapacity, int32_t* beganCount, int32_t* ended, int32_t endedCapacity, int32_t* endedCount)
{
	return reportGetEvents(ref(s), S2AMD_JOINT_REPORT_LIMITS, "s2amd_world_joint_limit_events", "joint limit event buffer too small", 1, at(s, &JointReportLayout::began),
						   at(s, &JointReportLayout::ended), began, beganCapacity, beganCount, ended, endedCapacity, endedCount);
}

int s2amd_world_body_joint_sums(s2amdSolver* s, s2amdBodyJointSum* out, int32_t bodyCapacity)
{
	return reportGetBodyArray(ref(s), S2AMD_JOINT_REPORT_BODY_SUMS, "s2amd_world_body_joint_sums", at(s, &JointReportLayout::sums), sizeof(*out), out, bodyCapacity);
}

int s2amd_world_joint_summary(s2amdSolver* s, s2amdJointSummary* out)
{
	const int rc = out ? reportHeadFor(ref(s), 0, "s2amd_world_joint_summary") : fail(S2AMD_E_INVALID, "bad argument");
	if (rc == S2AMD_OK)
	{
		*out = s->hJointReportHead.summary;
	}
	return rc;
}

} // extern "C"
#pragma GCC visibility pop
