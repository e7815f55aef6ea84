// Observers on the resident world (include/solver2d_amd.h: s2amd_world_set_observers, s2amd_world_set_observation_report,
// s2amd_world_observations, s2amd_world_export_observations(_async), s2amd_world_observer_states, s2amd_world_observer_counts): a
// persistent list that turns quantities of the resident world, and of the reports in front of it in the step's table, into channels of
// an observation vector in device memory -- the mirror image of actuators.hip.  An observer reads its target (and its frame, its joint's
// two bodies, its source report's record), forms its raw value x, its status and its value y = clamp(gain * x + bias), and writes y into
// its channels of the current row of a ring of `frames` rows.
//
// The setter has checked that no two observers' channel ranges overlap, so the pass is observeKernel alone: one lane per observer, no
// ordering rule.  The lane loads its 64-byte record with four 16-byte loads.  The ring's row, whether the ring is fresh (then grid y =
// frames and workgroup row y writes row y) and the three source pointers are kernel arguments the host decides when it enqueues:
// nothing is read back.  The vector is zeroed once, in the setter: channel ranges are static, and a channel no observer covers never
// changes.  The status counts are the actuators' (two sets of counters, ping-pong).  No float atomics, no sort, no scratch, no
// LDS, no host wait.  The arithmetic is fp32 one operation at a time; this file is compiled without contraction in both libraries
// (Makefile), because the result is stated bit for bit.
//
// The ring: row `head` holds frame 0 and frame k is row (head + k) % frames.  A reporting step moves the head one row BACK and writes
// there, so an export is rows [head, frames) and then rows [0, head): two contiguous copies, one when head is 0.
#include "solver_internal.h"

#include "report_common.h"

#include <cmath>
#include <numeric>

namespace
{

static_assert(sizeof(s2amdObserver) == 64 && sizeof(s2amdObserverState) == 32, "the observers' records");

#define S2_OBSERVATION_KNOWN (S2AMD_OBSERVATION_REPORT_VECTOR | S2AMD_OBSERVATION_REPORT_STATES)

// the device block of a list
struct ObserverLayout
{
	size_t counts, list, states, ring, total;
};

ObserverLayout observerLayout(int count, int channels, int frames)
{
	ObserverLayout l{};
	size_t at = 0;
	l.counts = reportTake(at, 8 * sizeof(int));
	l.list = reportTake(at, (size_t)count * sizeof(s2amdObserver));
	l.states = reportTake(at, (size_t)count * sizeof(s2amdObserverState));
	l.ring = reportTake(at, (size_t)frames * (size_t)channels * sizeof(float));
	l.total = at;
	return l;
}

ObserverLayout layoutOf(const s2amdSolver* s)
{
	return observerLayout((int)s->hObservers.size(), s->observationChannels, s->observationFrames);
}

__host__ __device__ inline int observerWidth(int kind)
{
	return kind == S2AMD_OBSERVER_BODY_POINT || kind == S2AMD_OBSERVER_BODY_ROTATION || kind == S2AMD_OBSERVER_BODY_LINEAR_VELOCITY || kind == S2AMD_OBSERVER_BODY_CONTACT ? 2 : 1;
}

// the joint report's rot of a joint's body: a body outside the array is unrotated (joint_report.hip: poseOf)
__device__ inline Rot jointBodyRot(const s2amdBody* bodies, int nb, int body)
{
	Rot q;
	q.s = 0.0f, q.c = 1.0f;
	if (body >= 0 && body < nb)
	{
		q.s = bodies[body].rot[0], q.c = bodies[body].rot[1];
	}
	return q;
}

// One lane per observer; workgroup row y writes ring row (fresh ? y : row).  The host has checked every record; the comparisons against
// nb, nj, rayCount, actionChannels and channels keep a lane inside the arrays whatever a record holds (a list set before an upload with
// smaller capacities, a ray or actuator list replaced by a shorter one).  sums, ranges, actions: nullptr when the source is off.
__global__ __launch_bounds__(S2_BLOCK) void observeKernel(const s2amdObserver* list, int count, const s2amdBody* bodies, const float2* origins, int nb, const s2amdJoint* joints,
														  int nj, const s2amdBodyContactSum* sums, const float* ranges, int rayCount, const float* actions, int actionChannels,
														  float* ring, int channels, int row, int fresh, s2amdObserverState* states, int* countsNow, int* countsNext)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	const bool first = blockIdx.y == 0;
	if (i == 0 && first)
	{
		// (the set the pass behind this one counts into)
		*(int4*)countsNext = make_int4(0, 0, 0, 0);
	}
	int status = -1;
	if (i < count)
	{
		const int4 head = ((const int4*)list)[4 * (size_t)i];
		const float4 map = ((const float4*)list)[4 * (size_t)i + 1];
		const float4 rule = ((const float4*)list)[4 * (size_t)i + 2];
		// (the rest is `reserved`: zero, checked by the host)
		const int kind = head.x, target = head.y, frame = head.z, channel = head.w;
		const int flags = __float_as_int(map.x);
		const float gain = map.y, bias = map.z, lower = map.w, upper = rule.x;
		const int width = observerWidth(kind);
		float x0 = 0.0f, x1 = 0.0f;
		if ((flags & S2AMD_OBSERVER_DISABLED) != 0)
		{
			status = S2AMD_OBSERVER_STATUS_DISABLED;
		}
		else if (kind <= S2AMD_OBSERVER_BODY_ANGULAR_VELOCITY)
		{
			const bool framed = frame >= 0;
			if (!liveBody(bodies, nb, target) || (framed && !liveBody(bodies, nb, frame)))
			{
				status = S2AMD_OBSERVER_STATUS_SKIPPED;
			}
			else
			{
				status = S2AMD_OBSERVER_STATUS_OBSERVED;
				const s2amdBody* b = bodies + target;
				const s2amdBody* f = bodies + (framed ? frame : target); // (read only where framed)
				const float bs = b->rot[0], bc = b->rot[1], fs = f->rot[0], fc = f->rot[1];
				const bool relative = framed && (flags & S2AMD_OBSERVER_RELATIVE) != 0;
				if (kind == S2AMD_OBSERVER_BODY_POINT)
				{
					// s2TransformPoint(xf(target), local) (math.h:350-356), then s2InvTransformPoint(xf(frame), p) (math.h:359-364)
					const float2 o = origins[target];
					x0 = (bc * rule.y - bs * rule.z) + o.x;
					x1 = (bs * rule.y + bc * rule.z) + o.y;
					if (framed)
					{
						const float2 fo = origins[frame];
						const float vx = x0 - fo.x, vy = x1 - fo.y;
						x0 = fc * vx + fs * vy;
						x1 = -fs * vx + fc * vy;
					}
				}
				else if (kind == S2AMD_OBSERVER_BODY_ROTATION || kind == S2AMD_OBSERVER_BODY_ANGLE)
				{
					// s2InvMulRot(rot(frame), rot(target)) (math.h:307-317)
					float qs = bs, qc = bc;
					if (framed)
					{
						qs = fc * bs - fs * bc;
						qc = fc * bc + fs * bs;
					}
					if (kind == S2AMD_OBSERVER_BODY_ROTATION)
					{
						x0 = qs, x1 = qc;
					}
					else
					{
						x0 = s2_atan2f(qs, qc);
					}
				}
				else if (kind == S2AMD_OBSERVER_BODY_LINEAR_VELOCITY)
				{
					float vx = b->linearVelocity[0], vy = b->linearVelocity[1];
					if (relative)
					{
						vx = vx - f->linearVelocity[0], vy = vy - f->linearVelocity[1]; // s2Sub
					}
					x0 = vx, x1 = vy;
					if (framed)
					{
						// s2InvRotateVector(rot(frame), v) (math.h:344-347)
						x0 = fc * vx + fs * vy;
						x1 = -fs * vx + fc * vy;
					}
				}
				else
				{
					x0 = b->angularVelocity;
					if (relative)
					{
						x0 = x0 - f->angularVelocity;
					}
				}
			}
		}
		else if (kind <= S2AMD_OBSERVER_REVOLUTE_MOTOR_IMPULSE)
		{
			if (target < 0 || target >= nj || joints[target].type != S2AMD_JOINT_REVOLUTE)
			{
				status = S2AMD_OBSERVER_STATUS_SKIPPED;
			}
			else
			{
				status = S2AMD_OBSERVER_STATUS_OBSERVED;
				const s2amdJoint* j = joints + target;
				const int bodyA = j->bodyA, bodyB = j->bodyB;
				if (kind == S2AMD_OBSERVER_REVOLUTE_ANGLE)
				{
					// the joint report's angle (joint_report.hip), the servo actuator's (actuators.hip)
					x0 = relativeAngle(jointBodyRot(bodies, nb, bodyB), jointBodyRot(bodies, nb, bodyA)) - j->referenceAngle;
				}
				else if (kind == S2AMD_OBSERVER_REVOLUTE_SPEED)
				{
					const float wA = bodyA >= 0 && bodyA < nb ? bodies[bodyA].angularVelocity : 0.0f;
					const float wB = bodyB >= 0 && bodyB < nb ? bodies[bodyB].angularVelocity : 0.0f;
					x0 = wB - wA;
				}
				else
				{
					x0 = j->motorImpulse;
				}
			}
		}
		else if (kind == S2AMD_OBSERVER_BODY_CONTACT)
		{
			if (!liveBody(bodies, nb, target))
			{
				status = S2AMD_OBSERVER_STATUS_SKIPPED;
			}
			else if (sums == nullptr)
			{
				status = S2AMD_OBSERVER_STATUS_SOURCE_OFF;
			}
			else
			{
				status = S2AMD_OBSERVER_STATUS_OBSERVED;
				x0 = sums[target].touching > 0 ? 1.0f : 0.0f;
				x1 = sums[target].normalImpulse;
			}
		}
		else
		{
			// a ray range or an action channel: one float of a list whose length the host knows (0: no such list is set)
			const bool ray = kind == S2AMD_OBSERVER_RAY_RANGE;
			const int length = ray ? rayCount : actionChannels;
			const float* source = ray ? ranges : actions;
			if (target < 0 || (length > 0 && target >= length))
			{
				status = S2AMD_OBSERVER_STATUS_SKIPPED;
			}
			else if (source == nullptr || target >= length)
			{
				status = S2AMD_OBSERVER_STATUS_SOURCE_OFF;
			}
			else
			{
				status = S2AMD_OBSERVER_STATUS_OBSERVED;
				x0 = source[target];
			}
		}
		float y0 = 0.0f, y1 = 0.0f;
		if (status == S2AMD_OBSERVER_STATUS_OBSERVED)
		{
			y0 = clampedAffine(x0, gain, bias, lower, upper);
			y1 = width == 2 ? clampedAffine(x1, gain, bias, lower, upper) : 0.0f;
		}
		else
		{
			x0 = 0.0f, x1 = 0.0f;
		}
		if (channel >= 0 && channel + width <= channels)
		{
			float* out = ring + (size_t)(fresh != 0 ? (int)blockIdx.y : row) * (size_t)channels + channel;
			out[0] = y0;
			if (width == 2)
			{
				out[1] = y1;
			}
		}
		if (states != nullptr && first)
		{
			float4* st = (float4*)(states + i);
			st[0] = make_float4(__int_as_float(i), __int_as_float(status), x0, x1);
			st[1] = make_float4(y0, y1, __int_as_float(0), __int_as_float(0));
		}
	}
	if (first)
	{
		for (int code = 0; code < 4; ++code)
		{
			const unsigned long long m = __ballot(status == code);
			if (m != 0ull && (threadIdx.x & 63) == 0)
			{
				atomicAdd(countsNow + code, __popcll(m));
			}
		}
	}
}

bool validObserver(const s2amdObserver& o, int32_t channels)
{
	if (o.kind < S2AMD_OBSERVER_BODY_POINT || o.kind > S2AMD_OBSERVER_ACTION || o.target < 0 || o.frame < -1 || o.channel < 0 ||
		(o.flags & ~(S2AMD_OBSERVER_DISABLED | S2AMD_OBSERVER_RELATIVE)) != 0)
	{
		return false;
	}
	if (o.kind >= S2AMD_OBSERVER_REVOLUTE_ANGLE && o.frame != -1)
	{
		return false;
	}
	if ((int64_t)o.channel + observerWidth(o.kind) > (int64_t)channels)
	{
		return false;
	}
	for (int32_t r : o.reserved)
	{
		if (r != 0)
		{
			return false;
		}
	}
	if (!std::isfinite(o.gain) || !std::isfinite(o.bias) || !std::isfinite(o.local[0]) || !std::isfinite(o.local[1]))
	{
		return false;
	}
	// (a comparison with a NaN is false)
	return o.lower <= o.upper;
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->observationReport, nullptr, 0, "observation-report", "s2amd_world_set_observation_report"} : ReportRef{};
}

// a getter's state (report_host.cpp: reportGetPerItem): *count = `entries`, 0 and S2AMD_OK with no list whatever else holds
int getterState(s2amdSolver* s, int flag, const char* what, const void* out, int32_t capacity, int32_t* count, int entries)
{
	const std::string tooSmall = std::string(what) + ": buffer too small";
	return reportGetPerItem(ref(s), flag, what, tooSmall.c_str(), out, capacity, count, s && !s->hObservers.empty() ? entries : 0, true);
}

// frames 0 .. frames - 1 of the ring to `out` (host or device), enqueued: rows [head, frames), then rows [0, head)
int enqueueVector(s2amdSolver* s, void* out, hipMemcpyKind kind)
{
	const size_t row = (size_t)s->observationChannels * sizeof(float);
	const int head = s->observationHead, frames = s->observationFrames;
	const char* ring = (const char*)s->dObservers.p + layoutOf(s).ring;
	HIP_TRY(hipMemcpyAsync(out, ring + (size_t)head * row, (size_t)(frames - head) * row, kind, s->stream));
	if (head > 0)
	{
		HIP_TRY(hipMemcpyAsync((char*)out + (size_t)(frames - head) * row, ring, (size_t)head * row, kind, s->stream));
	}
	return S2AMD_OK;
}

int vectorOut(s2amdSolver* s, const char* what, void* out, int32_t capacity, int32_t* count, hipMemcpyKind kind)
{
	int rc = getterState(s, S2AMD_OBSERVATION_REPORT_VECTOR, what, out, capacity, count, s ? s->observationFrames * s->observationChannels : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	HIP_TRY(hipSetDevice(s->device));
	if ((rc = enqueueVector(s, out, kind)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

} // namespace

// (at s2amd_world_upload and when the flags go from 0 to non-zero: the history is re-based; the block is the setter's and stays)
int observationPrepare(s2amdSolver* s)
{
	(void)reportPrepareBegin(s, s->observationReport);
	s->observationFresh = true;
	return S2AMD_OK;
}

int observationEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->observationReport;
	const int count = (int)s->hObservers.size();
	if (r.flags == 0)
	{
		return S2AMD_OK;
	}
	if (count > 0)
	{
		const ObserverLayout l = layoutOf(s);
		if (s->dObservers.p == nullptr || s->dObservers.bytes < l.total)
		{
			return fail(S2AMD_E_STATE, "internal: the observer list's device block was not prepared");
		}
		char* base = (char*)s->dObservers.p;
		const int frames = s->observationFrames;
		const bool fresh = s->observationFresh;
		// a fresh ring is written whole and frame 0 is row 0; otherwise the head moves one row back and that row is written
		s->observationHead = fresh ? 0 : (s->observationHead + frames - 1) % frames;
		s->observationFresh = false;
		int* counts = (int*)(base + l.counts);
		int rayCount = 0, actionChannels = 0;
		const float* ranges = rayReportRanges(s, &rayCount);
		const float* actions = actuatorsActionBuffer(s, &actionChannels);
		observeKernel<<<dim3(gridFor((size_t)count).x, fresh ? (unsigned)frames : 1u), dim3(S2_BLOCK), 0, s->stream>>>(
			(const s2amdObserver*)(base + l.list), count, (const s2amdBody*)s->dBodies.p, (const float2*)s->dOrigins.p, s->bodyCapacity, (const s2amdJoint*)s->dJoints.p,
			s->jointCapacity, contactReportBodySums(s), ranges, rayCount, actions, actionChannels, (float*)(base + l.ring), s->observationChannels, s->observationHead,
			fresh ? 1 : 0, (r.flags & S2AMD_OBSERVATION_REPORT_STATES) != 0 ? (s2amdObserverState*)(base + l.states) : nullptr, counts + 4 * (int)(s->observationPasses & 1),
			counts + 4 * (int)((s->observationPasses + 1) & 1));
		HIP_TRY(hipGetLastError());
		s->observationPasses += 1;
	}
	r.stepFlags = r.flags;
	return S2AMD_OK;
}

const float* observationRing(const s2amdSolver* s, int* channels, int* frames, int* head)
{
	*channels = s->observationChannels, *frames = s->observationFrames, *head = s->observationHead;
	if (s->hObservers.empty() || s->observationReport.stepFlags == 0 || s->dObservers.p == nullptr)
	{
		return nullptr;
	}
	return (const float*)((const char*)s->dObservers.p + layoutOf(s).ring);
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_observers(s2amdSolver* s, const s2amdObserver* list, int32_t count, int32_t channels, int32_t frames)
{
	if (int rc = listArgs(s, list, count, S2AMD_MAX_OBSERVERS))
	{
		return rc;
	}
	if (count > 0 && (channels < 1 || channels > S2AMD_MAX_OBSERVATION_CHANNELS || frames < 1 || frames > S2AMD_MAX_OBSERVATION_FRAMES))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validObserver(list[i], channels))
		{
			return fail(S2AMD_E_INVALID, "observer " + std::to_string(i) +
											 " is invalid (kind outside 1..11, a negative target, a frame below -1 or one on kinds 6-11, channels outside the observation "
											 "vector, unknown flag bits, reserved != 0, a NaN or infinite gain, bias or local, lower > upper): nothing was replaced");
		}
	}
	// no two channel ranges overlap: in the order of their first channels, each range ends where the next begins or before
	std::vector<int32_t> order((size_t)count);
	std::iota(order.begin(), order.end(), 0);
	std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return list[a].channel < list[b].channel; });
	for (int32_t k = 1; k < count; ++k)
	{
		const s2amdObserver& before = list[order[(size_t)k - 1]];
		if (before.channel + observerWidth(before.kind) > list[order[(size_t)k]].channel)
		{
			return fail(S2AMD_E_INVALID, "observers " + std::to_string(std::min(order[(size_t)k - 1], order[(size_t)k])) + " and " +
											 std::to_string(std::max(order[(size_t)k - 1], order[(size_t)k])) + " write the same channel: nothing was replaced");
		}
	}
	if (count == 0)
	{
		// (the block stays for the next list; a step in flight still reads it)
		s->hObservers.clear();
		s->observationChannels = s->observationFrames = 0;
		s->observationReport.stepFlags = 0;
		s->observationFresh = true;
		return S2AMD_OK;
	}
	// The list goes to its device block now, so that a step only launches: waited for, because the block of the list before may still be
	// read by a step or an export in flight and the copy reads the caller's memory.
	const ObserverLayout l = observerLayout(count, channels, frames);
	const int rc = listUpload(s, s->dObservers, l.total, [&](char* base) {
		HIP_TRY(hipMemsetAsync(base + l.counts, 0, 8 * sizeof(int), s->stream));
		HIP_TRY(hipMemcpyAsync(base + l.list, list, (size_t)count * sizeof(s2amdObserver), hipMemcpyHostToDevice, s->stream));
		// (once: a channel no observer covers reads +0 from here on)
		HIP_TRY(hipMemsetAsync(base + l.ring, 0, (size_t)frames * (size_t)channels * sizeof(float), s->stream));
		return (int)S2AMD_OK;
	});
	if (rc)
	{
		return rc; // (the old list stands: its block is as it was)
	}
	s->hObservers.assign(list, list + count);
	s->observationChannels = channels, s->observationFrames = frames;
	s->observationHead = 0;
	s->observationFresh = true; // re-based
	s->observationPasses = 0;
	s->observationReport.stepFlags = 0; // the last step's answers were of the list that left
	return S2AMD_OK;
}

int s2amd_world_set_observation_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2_OBSERVATION_KNOWN, observationPrepare);
}

int s2amd_world_observations(s2amdSolver* s, float* out, int32_t capacity, int32_t* count)
{
	return vectorOut(s, "s2amd_world_observations", out, capacity, count, hipMemcpyDeviceToHost);
}

int s2amd_world_export_observations(s2amdSolver* s, void* deviceVector, int32_t capacity)
{
	int32_t count = 0;
	return vectorOut(s, "s2amd_world_export_observations", deviceVector, capacity, &count, hipMemcpyDeviceToDevice);
}

int s2amd_world_export_observations_async(s2amdSolver* s, void* deviceVector, int32_t capacity, int32_t slot)
{
	if (slot < 0 || slot >= 4)
	{
		return fail(S2AMD_E_INVALID, "slot outside 0..3");
	}
	int32_t count = 0;
	int rc = getterState(s, S2AMD_OBSERVATION_REPORT_VECTOR, "s2amd_world_export_observations_async", deviceVector, capacity, &count,
						 s ? s->observationFrames * s->observationChannels : 0);
	if (rc)
	{
		return rc;
	}
	HIP_TRY(hipSetDevice(s->device));
	hipEvent_t exported = nullptr;
	HIP_TRY(exportEvent(s, slot, &exported));
	if (count > 0 && (rc = enqueueVector(s, deviceVector, hipMemcpyDeviceToDevice)) != 0)
	{
		return rc;
	}
	// (recorded with an empty list too: s2amd_export_wait(slot) then returns at once)
	HIP_TRY(hipEventRecord(exported, s->stream));
	return S2AMD_OK;
}

int s2amd_world_observer_states(s2amdSolver* s, s2amdObserverState* out, int32_t capacity, int32_t* count)
{
	const int rc = getterState(s, S2AMD_OBSERVATION_REPORT_STATES, "s2amd_world_observer_states", out, capacity, count, s ? (int)s->hObservers.size() : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	return reportCopyOut(s, out, s->dObservers, layoutOf(s).states, *count, sizeof(s2amdObserverState), hipMemcpyDeviceToHost);
}

int s2amd_world_observer_counts(s2amdSolver* s, int32_t counts[4])
{
	int32_t count = 0;
	const int rc = getterState(s, 0, "s2amd_world_observer_counts", counts, 4, &count, 4);
	if (rc)
	{
		return rc;
	}
	if (count == 0)
	{
		counts[0] = counts[1] = counts[2] = counts[3] = 0;
		return S2AMD_OK;
	}
	return listStatusCounts(s, s->dObservers, s->observationPasses, counts);
}

} // extern "C"
#pragma GCC visibility pop
