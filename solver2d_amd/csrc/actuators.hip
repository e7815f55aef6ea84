// Actuators on the resident world (include/solver2d_amd.h: s2amd_world_set_actuators, s2amd_world_set_actions,
// s2amd_world_import_actions, s2amd_world_actuator_states, s2amd_world_actuator_counts): a persistent list that turns channels of an
// action vector in device memory into s2amd_world_edit's edits, in front of every step.  An actuator reads its channels, forms its
// command u = clamp(gain * a + bias), and its term is one edit through applyBodyEdit / applyJointEdit (edit_ops.h), so a term IS the
// edit of the same name.  The statement is sequential: the terms of the APPLIED actuators in list order.  A term reads and writes its
// own target's record only and changes no pose, so only the order of the terms ON ONE TARGET matters -- to the bit, because force adds
// are float sums and a set hides the sets before it.
//
// The list is static, so the setter groups it once: a stable order of the actuators by (joint?, target, list index), the first entry of
// every target's segment marked, and whether any target occurs twice.  A step then launches
//
//   all targets distinct   actuatorTermsKernel<true>: one lane per actuator.  The lane loads its 64-byte record with four 16-byte loads,
//                          reads its channels and its target (the servo: the joint's two bodies' rot behind that), forms the term,
//                          applies it to the target's edited fields in registers, stores them and writes its state.
//   a target twice         actuatorTermsKernel<false>: the same lane forms the term and the state -- the atan2 of every servo is paid in
//                          parallel -- and writes the term to a term array; actuatorWalkKernel: one lane per entry of the order, the
//                          first lane of a target's segment applies the segment's APPLIED terms in list order with the fields in
//                          registers and stores once.  A list that puts thousands of actuators on one body is walked by one lane:
//                          correct, not fast.
//
// The status counts: one wave ballot per status and one integer atomic per wave that has any, into one of two sets of counters -- a pass
// counts into one set and clears the other for the pass behind it, so a step enqueues no memset.  No float atomics, no sort in the step,
// no scratch, no host wait.  The arithmetic is fp32 one operation at a time; this file is compiled without contraction in both libraries
// (Makefile), because the result is stated bit for bit.
#include "solver_internal.h"

#include "report_common.h"
#include "edit_ops.h"

#include <cmath>
#include <cstring>
#include <numeric>

namespace
{

static_assert(sizeof(s2amdActuator) == 64 && sizeof(s2amdActuatorState) == 48, "the actuators' records");

#define S2_ACT_SEGMENT_START 0x80000000u // in an entry of the order: the first actuator of its target

// the device block of a list
struct ActuatorLayout
{
	size_t counts, list, order, terms, states, actions, total;
};

ActuatorLayout actuatorLayout(int count, int channels, bool repeated)
{
	ActuatorLayout l{};
	size_t at = 0;
	l.counts = reportTake(at, 8 * sizeof(int));
	l.list = reportTake(at, (size_t)count * sizeof(s2amdActuator));
	l.order = reportTake(at, (size_t)count * sizeof(uint32_t));
	l.terms = repeated ? reportTake(at, (size_t)count * sizeof(s2amdWorldEdit)) : at;
	l.states = reportTake(at, (size_t)count * sizeof(s2amdActuatorState));
	l.actions = reportTake(at, (size_t)channels * sizeof(float));
	l.total = at;
	return l;
}

__host__ __device__ inline int actuatorWidth(int kind)
{
	return kind == S2AMD_ACTUATOR_BODY_FORCE || kind == S2AMD_ACTUATOR_BODY_LINEAR_VELOCITY || kind == S2AMD_ACTUATOR_MOUSE_TARGET ? 2 : 1;
}

// all exponent bits set: a NaN or an infinity
__device__ inline bool notFinite(float a)
{
	return (__float_as_uint(a) & 0x7f800000u) == 0x7f800000u;
}

// One lane per actuator: its term and its state.  APPLY: all targets are distinct and the lane applies its own term; otherwise the term
// goes to terms[i] (flag: the actuator is APPLIED) for the walk.  The host has checked every record; the comparisons against nb, nj and
// channels keep a lane inside the arrays whatever a record holds (a list set before an upload with smaller capacities).
template <bool APPLY>
__global__ __launch_bounds__(S2_BLOCK) void actuatorTermsKernel(const s2amdActuator* list, int count, const float* actions, int channels, s2amdBody* bodies, int nb,
																	s2amdJoint* joints, int nj, s2amdWorldEdit* terms, s2amdActuatorState* states, int* countsNow, int* countsNext)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i == 0)
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
		// (the fourth 16 bytes are `reserved`: zero, checked by the host)
		const int kind = head.x, target = head.y, channel = head.z, flags = head.w;
		const int width = actuatorWidth(kind);
		const bool onJoint = kind >= S2AMD_ACTUATOR_REVOLUTE_MOTOR_SPEED;
		float a0 = 0.0f, a1 = 0.0f, u0 = 0.0f, u1 = 0.0f, o0 = 0.0f, o1 = 0.0f, angle = 0.0f;
		s2amdWorldEdit e;
		e.kind = kind == S2AMD_ACTUATOR_BODY_LINEAR_VELOCITY	? S2AMD_EDIT_BODY_SET_LINEAR_VELOCITY
				 : kind == S2AMD_ACTUATOR_BODY_ANGULAR_VELOCITY ? S2AMD_EDIT_BODY_SET_ANGULAR_VELOCITY
				 : kind == S2AMD_ACTUATOR_MOUSE_TARGET			? S2AMD_EDIT_MOUSE_SET_TARGET
				 : onJoint										? S2AMD_EDIT_REVOLUTE_SET_MOTOR_SPEED
																: S2AMD_EDIT_BODY_APPLY_FORCE_TO_CENTER;
		e.target = target, e.flag = 0, e.reserved = 0;
		e.v[0] = e.v[1] = e.v[2] = e.v[3] = 0.0f;
		if ((flags & S2AMD_ACTUATOR_DISABLED) != 0)
		{
			status = S2AMD_ACTUATOR_STATUS_DISABLED;
		}
		else
		{
			if (channel >= 0 && channel + width <= channels)
			{
				a0 = actions[channel];
				a1 = width == 2 ? actions[channel + 1] : 0.0f;
			}
			const bool inside = target >= 0 && target < (onJoint ? nj : nb);
			BodyFixed k;
			BodyFields bf;
			JointFields jf;
			float rs = 0.0f, rc = 1.0f;
			int jointType = S2AMD_JOINT_FREE, bodyA = -1, bodyB = -1;
			float referenceAngle = 0.0f;
			bool live = false;
			if (inside && !onJoint)
			{
				const s2amdBody* b = bodies + target;
				loadBody(b, k, bf);
				rs = b->rot[0], rc = b->rot[1];
				live = k.type != S2AMD_BODY_FREE;
			}
			else if (inside)
			{
				const s2amdJoint* j = joints + target;
				loadJoint(j, jf);
				jointType = j->type, bodyA = j->bodyA, bodyB = j->bodyB;
				referenceAngle = j->referenceAngle;
				live = jointType == (kind == S2AMD_ACTUATOR_MOUSE_TARGET ? S2AMD_JOINT_MOUSE : S2AMD_JOINT_REVOLUTE);
			}
			if (!live)
			{
				status = S2AMD_ACTUATOR_STATUS_SKIPPED;
			}
			else if (notFinite(a0) || (width == 2 && notFinite(a1)))
			{
				status = S2AMD_ACTUATOR_STATUS_NONFINITE;
			}
			else
			{
				status = S2AMD_ACTUATOR_STATUS_APPLIED;
				u0 = clampedAffine(a0, map.x, map.y, map.z, map.w);
				u1 = width == 2 ? clampedAffine(a1, map.x, map.y, map.z, map.w) : 0.0f;
				if (kind == S2AMD_ACTUATOR_BODY_THRUST)
				{
					// s2RotateVector(rot, axis) (math.h:330-341), then s2MulSV
					const float x = rc * rule.x - rs * rule.y;
					const float y = rs * rule.x + rc * rule.y;
					o0 = u0 * x, o1 = u0 * y;
				}
				else if (kind == S2AMD_ACTUATOR_REVOLUTE_SERVO)
				{
					// the joint report's angle (joint_report.hip): a body outside the array is unrotated
					Rot qa, qb;
					qa.s = 0.0f, qa.c = 1.0f, qb.s = 0.0f, qb.c = 1.0f;
					if (bodyA >= 0 && bodyA < nb)
					{
						qa.s = bodies[bodyA].rot[0], qa.c = bodies[bodyA].rot[1];
					}
					if (bodyB >= 0 && bodyB < nb)
					{
						qb.s = bodies[bodyB].rot[0], qb.c = bodies[bodyB].rot[1];
					}
					angle = relativeAngle(qb, qa) - referenceAngle;
					const float v = rule.z * (u0 - angle);
					const float maxSpeed = rule.w, negMax = -rule.w;
					o0 = v < negMax ? negMax : (v > maxSpeed ? maxSpeed : v);
				}
				else
				{
					o0 = u0, o1 = u1;
				}
				e.flag = 1;
				e.v[0] = o0, e.v[1] = o1;
				if (APPLY)
				{
					if (!onJoint)
					{
						applyBodyEdit(e, k, bf);
						storeBody(bodies + target, bf);
					}
					else
					{
						(void)applyJointEdit(e, jointType, jf);
						storeJoint(joints + target, jf);
					}
				}
			}
		}
		if (!APPLY)
		{
			((int4*)terms)[2 * (size_t)i] = make_int4(e.kind, e.target, e.flag, 0);
			((float4*)terms)[2 * (size_t)i + 1] = make_float4(e.v[0], e.v[1], 0.0f, 0.0f);
		}
		float4* st = (float4*)(states + i);
		st[0] = make_float4(__int_as_float(i), __int_as_float(target), __int_as_float(status), __int_as_float(0));
		st[1] = make_float4(a0, a1, u0, u1);
		st[2] = make_float4(o0, o1, angle, __int_as_float(0));
	}
	for (int code = 0; code < 4; ++code)
	{
		const unsigned long long m = __ballot(status == code);
		if (m != 0ull && (threadIdx.x & 63) == 0)
		{
			atomicAdd(countsNow + code, __popcll(m));
		}
	}
}

// Repeated targets: one lane per entry of the order; the first lane of a target's segment walks it.
__global__ __launch_bounds__(S2_BLOCK) void actuatorWalkKernel(const uint32_t* order, int count, const s2amdWorldEdit* terms, s2amdBody* bodies, int nb, s2amdJoint* joints,
															  int nj)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i >= count)
	{
		return;
	}
	const uint32_t entry = order[i];
	if ((entry & S2_ACT_SEGMENT_START) == 0u)
	{
		return;
	}
	const uint32_t firstIndex = entry & ~S2_ACT_SEGMENT_START;
	if (firstIndex >= (uint32_t)count)
	{
		return;
	}
	const s2amdWorldEdit first = loadEdit(terms, firstIndex);
	const bool onJoint = first.kind >= S2_EDIT_FIRST_JOINT_KIND;
	const int target = first.target;
	if (target < 0 || target >= (onJoint ? nj : nb))
	{
		return; // (every actuator of the segment is SKIPPED)
	}
	if (!onJoint)
	{
		s2amdBody* b = bodies + target;
		BodyFixed k;
		BodyFields f;
		loadBody(b, k, f);
		for (int at = i; at < count && (at == i || (order[at] & S2_ACT_SEGMENT_START) == 0u); ++at)
		{
			const uint32_t index = order[at] & ~S2_ACT_SEGMENT_START;
			if (index >= (uint32_t)count)
			{
				continue;
			}
			const s2amdWorldEdit e = loadEdit(terms, index);
			if (e.flag != 0)
			{
				applyBodyEdit(e, k, f);
			}
		}
		storeBody(b, f);
	}
	else
	{
		s2amdJoint* j = joints + target;
		const int type = j->type;
		JointFields f;
		loadJoint(j, f);
		for (int at = i; at < count && (at == i || (order[at] & S2_ACT_SEGMENT_START) == 0u); ++at)
		{
			const uint32_t index = order[at] & ~S2_ACT_SEGMENT_START;
			if (index >= (uint32_t)count)
			{
				continue;
			}
			const s2amdWorldEdit e = loadEdit(terms, index);
			if (e.flag != 0)
			{
				(void)applyJointEdit(e, type, f);
			}
		}
		storeJoint(j, f);
	}
}

bool validActuator(const s2amdSolver* s, const s2amdActuator& a, int32_t channels)
{
	if (a.kind < S2AMD_ACTUATOR_BODY_FORCE || a.kind > S2AMD_ACTUATOR_MOUSE_TARGET || a.target < 0 || a.channel < 0 || (a.flags & ~S2AMD_ACTUATOR_DISABLED) != 0 ||
		a.reserved[0] != 0 || a.reserved[1] != 0 || a.reserved[2] != 0 || a.reserved[3] != 0)
	{
		return false;
	}
	if ((int64_t)a.channel + actuatorWidth(a.kind) > (int64_t)channels)
	{
		return false;
	}
	if (s->worldResident && a.target >= (a.kind >= S2AMD_ACTUATOR_REVOLUTE_MOTOR_SPEED ? s->jointCapacity : s->bodyCapacity))
	{
		return false;
	}
	if (!std::isfinite(a.gain) || !std::isfinite(a.bias) || !std::isfinite(a.axis[0]) || !std::isfinite(a.axis[1]) || !std::isfinite(a.kp))
	{
		return false;
	}
	// (a comparison with a NaN is false)
	return a.lower <= a.upper && a.maxSpeed >= 0.0f;
}

// what the two writers check
int checkActionRange(const s2amdSolver* s, const void* values, int32_t first, int32_t count)
{
	if (!s || first < 0 || count < 0 || (count > 0 && !values))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (s->hActuators.empty())
	{
		return fail(S2AMD_E_STATE, "no actuator list is set (s2amd_world_set_actuators)");
	}
	if ((int64_t)first + count > (int64_t)s->actuatorChannels)
	{
		return fail(S2AMD_E_INVALID, "channels " + std::to_string(first) + " .. " + std::to_string((int64_t)first + count) + " lie outside the action buffer's " +
										 std::to_string(s->actuatorChannels));
	}
	return S2AMD_OK;
}

float* actionBuffer(const s2amdSolver* s)
{
	return (float*)((char*)s->dActuators.p + actuatorLayout((int)s->hActuators.size(), s->actuatorChannels, s->actuatorsRepeated).actions);
}

} // namespace

int actuatorsStepEnqueue(s2amdSolver* s)
{
	const int count = (int)s->hActuators.size();
	if (count == 0)
	{
		return S2AMD_OK;
	}
	const ActuatorLayout l = actuatorLayout(count, s->actuatorChannels, s->actuatorsRepeated);
	if (s->dActuators.p == nullptr || s->dActuators.bytes < l.total)
	{
		return fail(S2AMD_E_STATE, "internal: the actuator list's device block was not prepared");
	}
	char* base = (char*)s->dActuators.p;
	hipStream_t st = s->stream;
	int* counts = (int*)(base + l.counts);
	int* now = counts + 4 * (int)(s->actuatorPasses & 1);
	int* next = counts + 4 * (int)((s->actuatorPasses + 1) & 1);
	const s2amdActuator* list = (const s2amdActuator*)(base + l.list);
	const float* actions = (const float*)(base + l.actions);
	s2amdActuatorState* states = (s2amdActuatorState*)(base + l.states);
	s2amdBody* bodies = (s2amdBody*)s->dBodies.p;
	s2amdJoint* joints = (s2amdJoint*)s->dJoints.p;
	const int nb = s->bodyCapacity, nj = s->jointCapacity;
	if (!s->actuatorsRepeated)
	{
		actuatorTermsKernel<true><<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>(list, count, actions, s->actuatorChannels, bodies, nb, joints, nj, nullptr, states, now, next);
	}
	else
	{
		s2amdWorldEdit* terms = (s2amdWorldEdit*)(base + l.terms);
		actuatorTermsKernel<false><<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>(list, count, actions, s->actuatorChannels, bodies, nb, joints, nj, terms, states, now, next);
		actuatorWalkKernel<<<gridFor((size_t)count), dim3(S2_BLOCK), 0, st>>>((const uint32_t*)(base + l.order), count, terms, bodies, nb, joints, nj);
	}
	HIP_TRY(hipGetLastError());
	s->actuatorPasses += 1;
	s->actuatorStatesValid = true;
	return S2AMD_OK;
}

const float* actuatorsActionBuffer(const s2amdSolver* s, int* channels)
{
	*channels = s->actuatorChannels;
	return s->hActuators.empty() || s->dActuators.p == nullptr ? nullptr : actionBuffer(s);
}

void actuatorsForgetWorld(s2amdSolver* s)
{
	s->actuatorStatesValid = false;
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_actuators(s2amdSolver* s, const s2amdActuator* list, int32_t count, int32_t channels)
{
	if (int rc = listArgs(s, list, count, S2AMD_MAX_ACTUATORS))
	{
		return rc;
	}
	if (count > 0 && (channels < 1 || channels > S2AMD_MAX_ACTION_CHANNELS))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	for (int32_t i = 0; i < count; ++i)
	{
		if (!validActuator(s, list[i], channels))
		{
			return fail(S2AMD_E_INVALID, "actuator " + std::to_string(i) +
											 " is invalid (kind outside 1..7, a target outside the resident capacity, channels outside the action vector, unknown flag "
											 "bits, reserved != 0, a NaN or infinite gain, bias, axis or kp, lower > upper, a negative maxSpeed): nothing was replaced");
		}
	}
	if (count == 0)
	{
		// (the block stays for the next list; a step in flight still reads it)
		s->hActuators.clear();
		s->actuatorChannels = 0;
		s->actuatorsRepeated = false;
		s->actuatorStatesValid = false;
		return S2AMD_OK;
	}
	// the grouping by target, once: a stable order by (joint?, target), the first entry of every segment marked
	std::vector<uint32_t> keys((size_t)count), order((size_t)count);
	for (int32_t i = 0; i < count; ++i)
	{
		keys[(size_t)i] = (list[i].kind >= S2AMD_ACTUATOR_REVOLUTE_MOTOR_SPEED ? 0x80000000u : 0u) | (uint32_t)list[i].target;
	}
	std::iota(order.begin(), order.end(), 0u);
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
	bool repeated = false;
	for (int32_t i = count - 1; i >= 0; --i)
	{
		const bool start = i == 0 || keys[order[(size_t)i]] != keys[order[(size_t)i - 1]];
		repeated = repeated || !start;
		order[(size_t)i] |= start ? S2_ACT_SEGMENT_START : 0u;
	}
	// The list goes to its device block now, so that a step only launches: waited for, because the block of the list before may still be
	// read by a step in flight and the copies read the caller's memory and a local.
	const ActuatorLayout l = actuatorLayout(count, channels, repeated);
	const int rc = listUpload(s, s->dActuators, l.total, [&](char* base) {
		HIP_TRY(hipMemsetAsync(base + l.counts, 0, 8 * sizeof(int), s->stream));
		HIP_TRY(hipMemcpyAsync(base + l.list, list, (size_t)count * sizeof(s2amdActuator), hipMemcpyHostToDevice, s->stream));
		HIP_TRY(hipMemcpyAsync(base + l.order, order.data(), (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
		HIP_TRY(hipMemsetAsync(base + l.actions, 0, (size_t)channels * sizeof(float), s->stream));
		return (int)S2AMD_OK;
	});
	if (rc)
	{
		return rc; // (the old list stands: its block is as it was)
	}
	s->hActuators.assign(list, list + count);
	s->actuatorChannels = channels;
	s->actuatorsRepeated = repeated;
	s->actuatorPasses = 0;
	s->actuatorStatesValid = false;
	return S2AMD_OK;
}

int s2amd_world_set_actions(s2amdSolver* s, const float* hostValues, int32_t first, int32_t count)
{
	if (int rc = checkActionRange(s, hostValues, first, count))
	{
		return rc;
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	// the pinned stage, as s2amd_world_edit's: the caller may reuse its array at once and the copy to the device is a true asynchronous
	// one.  The copy of the call before may still be reading the stage: its event is waited for first.
	const size_t bytes = (size_t)count * sizeof(float);
	if (int rc = s->actionStage.begin(bytes, std::max(reportRound((size_t)s->actuatorChannels * sizeof(float)), (size_t)4096)))
	{
		return rc;
	}
	memcpy(s->actionStage.buf.p, hostValues, bytes);
	HIP_TRY(hipMemcpyAsync(actionBuffer(s) + first, s->actionStage.buf.p, bytes, hipMemcpyHostToDevice, s->stream));
	HIP_TRY(s->actionStage.record(s->stream));
	return S2AMD_OK;
}

int s2amd_world_import_actions(s2amdSolver* s, const void* deviceValues, int32_t first, int32_t count)
{
	if (int rc = checkActionRange(s, deviceValues, first, count))
	{
		return rc;
	}
	if (count == 0)
	{
		return S2AMD_OK;
	}
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipMemcpyAsync(actionBuffer(s) + first, deviceValues, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
	return S2AMD_OK;
}

int s2amd_world_actuator_states(s2amdSolver* s, s2amdActuatorState* out, int32_t capacity, int32_t* count)
{
	if (!s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (s->hActuators.empty())
	{
		*count = 0;
		return S2AMD_OK;
	}
	if (!s->actuatorStatesValid)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_actuator_states: no s2amd_world_step has applied the list since it was set or since the last upload");
	}
	*count = (int32_t)s->hActuators.size();
	if (*count > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "actuator state buffer too small");
	}
	const ActuatorLayout l = actuatorLayout(*count, s->actuatorChannels, s->actuatorsRepeated);
	return reportCopyOut(s, out, s->dActuators, l.states, *count, sizeof(s2amdActuatorState), hipMemcpyDeviceToHost);
}

int s2amd_world_actuator_counts(s2amdSolver* s, int32_t counts[4])
{
	if (!s || !counts)
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	if (s->hActuators.empty())
	{
		counts[0] = counts[1] = counts[2] = counts[3] = 0;
		return S2AMD_OK;
	}
	if (!s->actuatorStatesValid)
	{
		return fail(S2AMD_E_STATE, "s2amd_world_actuator_counts: no s2amd_world_step has applied the list since it was set or since the last upload");
	}
	return listStatusCounts(s, s->dActuators, s->actuatorPasses, counts);
}

} // extern "C"
#pragma GCC visibility pop
