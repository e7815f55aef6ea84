// Episodes on the resident world (include/solver2d_amd.h: s2amd_world_set_episodes, s2amd_world_set_episode_report,
// s2amd_world_episode_rewards, s2amd_world_episode_flags, s2amd_world_export_episode_step(_async), s2amd_world_episode_states,
// s2amd_world_episode_rule_states, s2amd_world_episode_events, s2amd_world_episode_counts): a persistent list of episode rules over
// agents, evaluated behind the observers on the observation vector of this step -- one reward and one flags word per agent, the episode
// accounting (length, return, automatic restart, time limit) kept in device memory, and the short list of agents that finished.
//
// The setter groups the static list once: a stable order by (agent, list index), a copy of the records in that order with the list index
// in reserved[0], and first[agents + 1].  A reporting step is then
//   episodeRulesKernel   one lane per grouped position: the 64-byte record with four 16-byte loads, one or two floats of the ring, the
//                        rule's y and a packed {status, fired, kind, list index} word at its position, the rule state at the list index;
//   episodeAgentsKernel  one lane per agent: walks its contiguous run of y / code in order (the float sum's order is the list's), reads,
//                        modifies and writes its own 32-byte record -- the record IS the accumulator, so there is no race --, rewards[a]
//                        and flags[a];
//   episodeEventsKernel  only with S2AMD_EPISODE_REPORT_EVENTS: one workgroup, at most 64 chunks of 256 agents, ballot + prefix.
// The two first kernels are kept apart: fused, one lane would issue its agent's record loads one behind the other, uncoalesced; apart,
// the rule loads are coalesced and the walk reads two dense arrays.  The ring's head, frames and channels, and whether the pass is fresh
// (then every agent record is taken as zero: no memset), are kernel arguments the host decides when it enqueues: nothing is read back.
// The counts are the actuators' (two sets, ping-pong; one ballot and one integer atomic per wave and code).  No float atomics, no sort
// in the step, no scratch, no LDS beyond the compaction's four wave totals, no host wait.  The arithmetic is fp32 one operation at a
// time; this file is compiled without contraction in both libraries (Makefile), because the result is stated bit for bit.
#include "solver_internal.h"

#include "report_common.h"

#include <cmath>

namespace
{

static_assert(sizeof(s2amdEpisodeRule) == 64 && sizeof(s2amdEpisodeState) == 32 && sizeof(s2amdEpisodeRuleState) == 32 && sizeof(s2amdEpisodeEvent) == 16,
			  "the episodes' records");

#define S2_EPISODE_KNOWN (S2AMD_EPISODE_REPORT_STEP | S2AMD_EPISODE_REPORT_STATES | S2AMD_EPISODE_REPORT_RULE_STATES | S2AMD_EPISODE_REPORT_EVENTS)
#define S2_EPISODE_RULE_FLAGS (S2AMD_EPISODE_RULE_DISABLED | S2AMD_EPISODE_RULE_DIFFERENCE | S2AMD_EPISODE_RULE_OUTSIDE)
// the packed word of a grouped position: status in bits 0-1, fired in bit 2, kind in bits 3-5, the list index from bit 6 (< 65,536)
#define S2_EPISODE_CODE(status, fired, kind, index) ((status) | ((fired) << 2) | ((kind) << 3) | ((index) << 6))

// the device block of a list
struct EpisodeLayout
{
	size_t counts, rules, first, limits, y, codes, states, rewards, flags, ruleStates, events, total;
};

EpisodeLayout episodeLayout(int rules, int agents)
{
	EpisodeLayout l{};
	size_t at = 0;
	l.counts = reportTake(at, 16 * sizeof(int));
	l.rules = reportTake(at, (size_t)rules * sizeof(s2amdEpisodeRule));
	l.first = reportTake(at, ((size_t)agents + 1) * sizeof(int));
	l.limits = reportTake(at, (size_t)agents * sizeof(int));
	l.y = reportTake(at, (size_t)rules * sizeof(float));
	l.codes = reportTake(at, (size_t)rules * sizeof(int));
	l.states = reportTake(at, (size_t)agents * sizeof(s2amdEpisodeState));
	l.rewards = reportTake(at, (size_t)agents * sizeof(float));
	l.flags = reportTake(at, (size_t)agents * sizeof(int));
	l.ruleStates = reportTake(at, (size_t)rules * sizeof(s2amdEpisodeRuleState));
	l.events = reportTake(at, (size_t)agents * sizeof(s2amdEpisodeEvent));
	l.total = at;
	return l;
}

EpisodeLayout layoutOf(const s2amdSolver* s)
{
	return episodeLayout((int)s->hEpisodeRules.size(), s->episodeAgents);
}

// One lane per grouped position.  The host has checked every record; the comparisons against channels and frames keep a lane inside the
// ring whatever a record holds (an observer list replaced by a narrower one).  ring: nullptr when the observation report did not run
// this step; channels and frames: the observer list's, 0 with no list.
__global__ __launch_bounds__(S2_BLOCK) void episodeRulesKernel(const s2amdEpisodeRule* rules, int count, const float* ring, int channels, int frames, int head, float* ys,
																   int* codes, s2amdEpisodeRuleState* ruleStates, int* countsNow, int* countsNext)
{
	const int i = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (i == 0)
	{
		// (the set the pass behind this one counts into; the agents' half is cleared by their kernel)
		*(int4*)countsNext = make_int4(0, 0, 0, 0);
	}
	int status = -1;
	if (i < count)
	{
		const int4 what = ((const int4*)rules)[4 * (size_t)i];
		const int4 more = ((const int4*)rules)[4 * (size_t)i + 1];
		const float4 map = ((const float4*)rules)[4 * (size_t)i + 2];
		const int4 tail = ((const int4*)rules)[4 * (size_t)i + 3];
		const int kind = what.x, channelA = what.z, frameA = what.w, channelB = more.x, frameB = more.y, shape = more.z, flags = more.w;
		const float gain = map.x, bias = map.y, lower = map.z, upper = map.w;
		const int index = tail.x; // the list index (the setter's)
		const bool reads = channelA >= 0, difference = (flags & S2AMD_EPISODE_RULE_DIFFERENCE) != 0;
		if ((flags & S2AMD_EPISODE_RULE_DISABLED) != 0)
		{
			status = S2AMD_EPISODE_STATUS_DISABLED;
		}
		else if (reads && channels > 0 && (channelA >= channels || frameA < 0 || frameA >= frames || (difference && (channelB < 0 || channelB >= channels || frameB < 0 || frameB >= frames))))
		{
			status = S2AMD_EPISODE_STATUS_SKIPPED;
		}
		else if (reads && (ring == nullptr || channels <= 0))
		{
			status = S2AMD_EPISODE_STATUS_SOURCE_OFF;
		}
		else
		{
			status = S2AMD_EPISODE_STATUS_EVALUATED;
		}
		float x = 0.0f, f = 0.0f, y = 0.0f;
		int fired = 0;
		if (status == S2AMD_EPISODE_STATUS_EVALUATED)
		{
			if (reads)
			{
				int row = head + frameA;
				row = row >= frames ? row - frames : row;
				x = ring[(size_t)row * (size_t)channels + channelA];
				if (difference)
				{
					row = head + frameB;
					row = row >= frames ? row - frames : row;
					x = x - ring[(size_t)row * (size_t)channels + channelB];
				}
			}
			f = shape == S2AMD_EPISODE_SHAPE_ABS ? fabsf(x) : (shape == S2AMD_EPISODE_SHAPE_SQUARE ? x * x : x);
			const bool inside = lower <= f && f <= upper;
			const bool test = inside != ((flags & S2AMD_EPISODE_RULE_OUTSIDE) != 0);
			if (kind == S2AMD_EPISODE_REWARD_VALUE)
			{
				y = clampedAffine(f, gain, bias, lower, upper);
			}
			else if (kind == S2AMD_EPISODE_REWARD_TEST)
			{
				y = test ? gain : bias;
			}
			else
			{
				fired = test ? 1 : 0;
				y = test ? gain : 0.0f;
			}
		}
		ys[i] = y;
		codes[i] = S2_EPISODE_CODE(status, fired, kind & 7, index);
		if (ruleStates != nullptr && index >= 0 && index < count)
		{
			float4* st = (float4*)(ruleStates + index);
			st[0] = make_float4(__int_as_float(index), __int_as_float(status), x, f);
			st[1] = make_float4(y, __int_as_float(fired), __int_as_float(0), __int_as_float(0));
		}
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

// One lane per agent: steps 1-5 of the statement over the agent's run [first[a], first[a + 1]) of the grouped positions, in order.
// fresh: the records are taken as zero (a re-base), whatever they hold.
__global__ __launch_bounds__(S2_BLOCK) void episodeAgentsKernel(const int* first, const int* limits, const float* ys, const int* codes, int ruleCount, s2amdEpisodeState* states,
																	float* rewards, int* flagsOut, int agents, int fresh, int* countsNow, int* countsNext)
{
	const int a = (int)(blockIdx.x * S2_BLOCK + threadIdx.x);
	if (a == 0)
	{
		*(int4*)(countsNext + 4) = make_int4(0, 0, 0, 0);
	}
	int flags = 0;
	if (a < agents)
	{
		int4 head = make_int4(0, -1, 0, 0), tail = make_int4(0, 0, 0, 0);
		if (fresh == 0)
		{
			head = ((const int4*)(states + a))[0];
			tail = ((const int4*)(states + a))[1];
		}
		float episodeReturn = __int_as_float(head.w), lastReturn = __int_as_float(tail.z);
		int episodeLength = tail.x, episodes = tail.y, lastLength = tail.w;
		if (fresh != 0 || (head.x & 3) != 0)
		{
			episodeLength = 0, episodeReturn = 0.0f;
		}
		float r = 0.0f;
		int rule = -1;
		const int begin = max(first[a], 0), end = min(first[a + 1], ruleCount);
		for (int p = begin; p < end; ++p)
		{
			const int code = codes[p];
			if ((code & 3) == S2AMD_EPISODE_STATUS_EVALUATED)
			{
				r = r + ys[p];
				if ((code & 4) != 0)
				{
					flags |= ((code >> 3) & 7) == S2AMD_EPISODE_TERMINATE ? S2AMD_EPISODE_TERMINATED : S2AMD_EPISODE_TRUNCATED;
					rule = rule < 0 ? code >> 6 : rule;
				}
			}
		}
		episodeLength += 1;
		const int limit = limits[a];
		if (limit > 0 && episodeLength >= limit)
		{
			flags |= S2AMD_EPISODE_TRUNCATED | S2AMD_EPISODE_TIME_LIMIT;
		}
		episodeReturn = episodeReturn + r;
		if ((flags & 3) != 0)
		{
			episodes += 1, lastReturn = episodeReturn, lastLength = episodeLength;
		}
		int4* st = (int4*)(states + a);
		st[0] = make_int4(flags, rule, __float_as_int(r), __float_as_int(episodeReturn));
		st[1] = make_int4(episodeLength, episodes, __float_as_int(lastReturn), lastLength);
		rewards[a] = r;
		flagsOut[a] = flags;
	}
	// done, terminated, truncated, at the time limit
	for (int code = 0; code < 4; ++code)
	{
		const unsigned long long m = __ballot(code == 0 ? (flags & 3) != 0 : (flags & (1 << (code - 1))) != 0);
		if (m != 0ull && (threadIdx.x & 63) == 0)
		{
			atomicAdd(countsNow + 4 + code, __popcll(m));
		}
	}
}

// One workgroup: the agents with flags & 3, ascending, with the values of step 5 (an ordered compaction: ballot + prefix per wave, the
// four wave totals through LDS, a running base over the chunks of 256 agents).
__global__ __launch_bounds__(S2_BLOCK) void episodeEventsKernel(const int* flagsIn, const s2amdEpisodeState* states, int agents, s2amdEpisodeEvent* events)
{
	__shared__ int waveTotal[S2_BLOCK / 64];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	int base = 0;
	for (int start = 0; start < agents; start += S2_BLOCK)
	{
		const int a = start + (int)threadIdx.x;
		const int flags = a < agents ? flagsIn[a] : 0;
		const bool done = (flags & 3) != 0;
		const unsigned long long m = __ballot(done);
		if (lane == 0)
		{
			waveTotal[wave] = __popcll(m);
		}
		__syncthreads();
		int at = base, total = 0;
		for (int w = 0; w < S2_BLOCK / 64; ++w)
		{
			const int t = waveTotal[w];
			at += w < wave ? t : 0;
			total += t;
		}
		if (done)
		{
			at += __popcll(m & ((1ull << lane) - 1ull));
			const int4 head = ((const int4*)(states + a))[0];
			const int length = states[a].episodeLength;
			if (at < agents)
			{
				*(int4*)(events + at) = make_int4(a, flags, length, head.w);
			}
		}
		base += total;
		__syncthreads();
	}
}

bool validRule(const s2amdEpisodeRule& r, int32_t agents)
{
	if (r.kind < S2AMD_EPISODE_REWARD_VALUE || r.kind > S2AMD_EPISODE_TRUNCATE || r.shape < S2AMD_EPISODE_SHAPE_LINEAR || r.shape > S2AMD_EPISODE_SHAPE_SQUARE || r.agent < 0 ||
		r.agent >= agents || r.channelA < -1 || r.frameA < 0 || (r.flags & ~S2_EPISODE_RULE_FLAGS) != 0)
	{
		return false;
	}
	if ((r.flags & S2AMD_EPISODE_RULE_DIFFERENCE) != 0 ? (r.channelA < 0 || r.channelB < 0 || r.frameB < 0) : (r.channelB != 0 || r.frameB != 0))
	{
		return false;
	}
	for (int32_t v : r.reserved)
	{
		if (v != 0)
		{
			return false;
		}
	}
	if (!std::isfinite(r.gain) || !std::isfinite(r.bias) || (r.kind >= S2AMD_EPISODE_TERMINATE && r.bias != 0.0f))
	{
		return false;
	}
	// (a comparison with a NaN is false)
	return r.lower <= r.upper;
}

ReportRef ref(s2amdSolver* s)
{
	return s ? ReportRef{s, &s->episodeReport, nullptr, 0, "episode-report", "s2amd_world_set_episode_report"} : ReportRef{};
}

// a getter's state (report_host.cpp: reportGetPerItem): *count = `entries`, 0 and S2AMD_OK with no list whatever else holds
int getterState(s2amdSolver* s, int flag, const char* what, const void* out, int32_t capacity, int32_t* count, int entries)
{
	const std::string tooSmall = std::string(what) + ": buffer too small";
	return reportGetPerItem(ref(s), flag, what, tooSmall.c_str(), out, capacity, count, s && s->episodeAgents > 0 ? entries : 0, true);
}

// the eight counts of the last pass, waited for
int fetchCounts(s2amdSolver* s, int32_t counts[8])
{
	HIP_TRY(hipSetDevice(s->device));
	const int* set = (const int*)((const char*)s->dEpisodes.p + layoutOf(s).counts) + 8 * (int)((s->episodePasses - 1) & 1);
	HIP_TRY(hipMemcpyAsync(counts, set, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

// rewards and flags to two device arrays, enqueued
int enqueueStep(s2amdSolver* s, void* deviceRewards, void* deviceFlags)
{
	const EpisodeLayout l = layoutOf(s);
	const char* base = (const char*)s->dEpisodes.p;
	const size_t bytes = (size_t)s->episodeAgents * sizeof(float);
	HIP_TRY(hipMemcpyAsync(deviceRewards, base + l.rewards, bytes, hipMemcpyDeviceToDevice, s->stream));
	HIP_TRY(hipMemcpyAsync(deviceFlags, base + l.flags, bytes, hipMemcpyDeviceToDevice, s->stream));
	return S2AMD_OK;
}

// the arguments and the state of the two exports: *count = agents (0 with no list)
int exportState(s2amdSolver* s, const char* what, const void* deviceRewards, const void* deviceFlags, int32_t capacity, int32_t* count)
{
	if (capacity > 0 && (!deviceRewards || !deviceFlags))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	return getterState(s, S2AMD_EPISODE_REPORT_STEP, what, deviceRewards, capacity, count, s ? s->episodeAgents : 0);
}

} // namespace

// (at s2amd_world_upload and when the flags go from 0 to non-zero: the accounting is re-based; the block is the setter's and stays)
int episodePrepare(s2amdSolver* s)
{
	(void)reportPrepareBegin(s, s->episodeReport);
	s->episodeFresh = true;
	return S2AMD_OK;
}

int episodeEnqueue(s2amdSolver* s, const s2amdStepParams*)
{
	ReportState& r = s->episodeReport;
	const int agents = s->episodeAgents, rules = (int)s->hEpisodeRules.size();
	if (r.flags == 0)
	{
		return S2AMD_OK;
	}
	if (agents > 0)
	{
		const EpisodeLayout l = layoutOf(s);
		if (s->dEpisodes.p == nullptr || s->dEpisodes.bytes < l.total)
		{
			return fail(S2AMD_E_STATE, "internal: the episode list's device block was not prepared");
		}
		char* base = (char*)s->dEpisodes.p;
		int* counts = (int*)(base + l.counts);
		int* now = counts + 8 * (int)(s->episodePasses & 1);
		int* next = counts + 8 * (int)((s->episodePasses + 1) & 1);
		if (rules > 0)
		{
			int channels = 0, frames = 0, head = 0;
			const float* ring = observationRing(s, &channels, &frames, &head);
			episodeRulesKernel<<<gridFor((size_t)rules), dim3(S2_BLOCK), 0, s->stream>>>(
				(const s2amdEpisodeRule*)(base + l.rules), rules, ring, channels, frames, head, (float*)(base + l.y), (int*)(base + l.codes),
				(r.flags & S2AMD_EPISODE_REPORT_RULE_STATES) != 0 ? (s2amdEpisodeRuleState*)(base + l.ruleStates) : nullptr, now, next);
			HIP_TRY(hipGetLastError());
		}
		episodeAgentsKernel<<<gridFor((size_t)agents), dim3(S2_BLOCK), 0, s->stream>>>((const int*)(base + l.first), (const int*)(base + l.limits), (const float*)(base + l.y),
																						(const int*)(base + l.codes), rules, (s2amdEpisodeState*)(base + l.states),
																						(float*)(base + l.rewards), (int*)(base + l.flags), agents, s->episodeFresh ? 1 : 0, now, next);
		HIP_TRY(hipGetLastError());
		if ((r.flags & S2AMD_EPISODE_REPORT_EVENTS) != 0)
		{
			episodeEventsKernel<<<dim3(1), dim3(S2_BLOCK), 0, s->stream>>>((const int*)(base + l.flags), (const s2amdEpisodeState*)(base + l.states), agents,
																			(s2amdEpisodeEvent*)(base + l.events));
			HIP_TRY(hipGetLastError());
		}
		s->episodeFresh = false;
		s->episodePasses += 1;
	}
	r.stepFlags = r.flags;
	return S2AMD_OK;
}

const int* episodeStepFlags(const s2amdSolver* s, int* agents)
{
	*agents = s->episodeAgents;
	if (s->episodeAgents <= 0 || s->episodeReport.stepFlags == 0 || s->dEpisodes.p == nullptr)
	{
		return nullptr;
	}
	return (const int*)((const char*)s->dEpisodes.p + layoutOf(s).flags);
}

#pragma GCC visibility push(default)
extern "C"
{

int s2amd_world_set_episodes(s2amdSolver* s, const s2amdEpisodeRule* rules, int32_t ruleCount, int32_t agents, const int32_t* stepLimits)
{
	if (int rc = listArgs(s, rules, ruleCount, S2AMD_MAX_EPISODE_RULES))
	{
		return rc;
	}
	if (agents < 0 || agents > S2AMD_MAX_EPISODE_AGENTS || (ruleCount > 0 && agents == 0))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	for (int32_t i = 0; i < ruleCount; ++i)
	{
		if (!validRule(rules[i], agents))
		{
			return fail(S2AMD_E_INVALID, "episode rule " + std::to_string(i) +
											 " is invalid (kind outside 1..4, shape outside 0..2, an agent outside the agents, channelA below -1, a negative frame, channelB or frameB "
											 "negative with DIFFERENCE or non-zero without, DIFFERENCE without a channelA, unknown flag bits, reserved != 0, a NaN or infinite gain or "
											 "bias, lower > upper, a bias on kinds 3 and 4): nothing was replaced");
		}
	}
	for (int32_t a = 0; stepLimits != nullptr && a < agents; ++a)
	{
		if (stepLimits[a] < 0)
		{
			return fail(S2AMD_E_INVALID, "step limit " + std::to_string(a) + " is negative: nothing was replaced");
		}
	}
	if (agents == 0)
	{
		// (the block stays for the next list; a step in flight still reads it)
		s->hEpisodeRules.clear();
		s->hEpisodeLimits.clear();
		s->episodeAgents = 0;
		s->episodeReport.stepFlags = 0;
		s->episodeFresh = true;
		return S2AMD_OK;
	}
	// grouped once: a stable order by (agent, list index), the records copied in that order with their list index, and first[agents + 1]
	std::vector<int32_t> first((size_t)agents + 1, 0);
	for (int32_t i = 0; i < ruleCount; ++i)
	{
		first[(size_t)rules[i].agent + 1] += 1;
	}
	for (int32_t a = 0; a < agents; ++a)
	{
		first[(size_t)a + 1] += first[(size_t)a];
	}
	std::vector<s2amdEpisodeRule> grouped((size_t)ruleCount);
	{
		std::vector<int32_t> next(first.begin(), first.end() - 1);
		for (int32_t i = 0; i < ruleCount; ++i)
		{
			s2amdEpisodeRule& g = grouped[(size_t)next[(size_t)rules[i].agent]++];
			g = rules[i];
			g.reserved[0] = i;
		}
	}
	std::vector<int32_t> limits((size_t)agents, 0);
	if (stepLimits != nullptr)
	{
		limits.assign(stepLimits, stepLimits + agents);
	}
	// The list goes to its device block now, so that a step only launches: waited for, because the block of the list before may still be
	// read by a step or an export in flight and the copies read this call's memory.
	const EpisodeLayout l = episodeLayout(ruleCount, agents);
	const int rc = listUpload(s, s->dEpisodes, l.total, [&](char* base) {
		HIP_TRY(hipMemsetAsync(base + l.counts, 0, 16 * sizeof(int), s->stream));
		if (ruleCount > 0)
		{
			HIP_TRY(hipMemcpyAsync(base + l.rules, grouped.data(), (size_t)ruleCount * sizeof(s2amdEpisodeRule), hipMemcpyHostToDevice, s->stream));
		}
		HIP_TRY(hipMemcpyAsync(base + l.first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
		HIP_TRY(hipMemcpyAsync(base + l.limits, limits.data(), limits.size() * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
		// (the agent records: a fresh pass takes them as zero anyway; zeroed so that the block holds nothing of the list that left)
		HIP_TRY(hipMemsetAsync(base + l.states, 0, (size_t)agents * sizeof(s2amdEpisodeState), s->stream));
		return (int)S2AMD_OK;
	});
	if (rc)
	{
		return rc; // (the old list stands: its host state is as it was)
	}
	s->hEpisodeRules.assign(rules, rules + ruleCount);
	s->hEpisodeLimits.swap(limits);
	s->episodeAgents = agents;
	s->episodeFresh = true; // re-based
	s->episodePasses = 0;
	s->episodeReport.stepFlags = 0; // the last step's answers were of the list that left
	return S2AMD_OK;
}

int s2amd_world_set_episode_report(s2amdSolver* s, int32_t flags)
{
	return reportSet(ref(s), flags, S2_EPISODE_KNOWN, episodePrepare);
}

int s2amd_world_episode_rewards(s2amdSolver* s, float* out, int32_t capacity, int32_t* count)
{
	const int rc = getterState(s, S2AMD_EPISODE_REPORT_STEP, "s2amd_world_episode_rewards", out, capacity, count, s ? s->episodeAgents : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	return reportCopyOut(s, out, s->dEpisodes, layoutOf(s).rewards, *count, sizeof(float), hipMemcpyDeviceToHost);
}

int s2amd_world_episode_flags(s2amdSolver* s, int32_t* out, int32_t capacity, int32_t* count)
{
	const int rc = getterState(s, S2AMD_EPISODE_REPORT_STEP, "s2amd_world_episode_flags", out, capacity, count, s ? s->episodeAgents : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	return reportCopyOut(s, out, s->dEpisodes, layoutOf(s).flags, *count, sizeof(int32_t), hipMemcpyDeviceToHost);
}

int s2amd_world_export_episode_step(s2amdSolver* s, void* deviceRewards, void* deviceFlags, int32_t capacity)
{
	int32_t count = 0;
	int rc = exportState(s, "s2amd_world_export_episode_step", deviceRewards, deviceFlags, capacity, &count);
	if (rc || count == 0)
	{
		return rc;
	}
	HIP_TRY(hipSetDevice(s->device));
	if ((rc = enqueueStep(s, deviceRewards, deviceFlags)) != 0)
	{
		return rc;
	}
	HIP_TRY(hipStreamSynchronize(s->stream));
	return S2AMD_OK;
}

int s2amd_world_export_episode_step_async(s2amdSolver* s, void* deviceRewards, void* deviceFlags, int32_t capacity, int32_t slot)
{
	if (slot < 0 || slot >= 4)
	{
		return fail(S2AMD_E_INVALID, "slot outside 0..3");
	}
	int32_t count = 0;
	int rc = exportState(s, "s2amd_world_export_episode_step_async", deviceRewards, deviceFlags, capacity, &count);
	if (rc)
	{
		return rc;
	}
	HIP_TRY(hipSetDevice(s->device));
	hipEvent_t exported = nullptr;
	HIP_TRY(exportEvent(s, slot, &exported));
	if (count > 0 && (rc = enqueueStep(s, deviceRewards, deviceFlags)) != 0)
	{
		return rc;
	}
	// (recorded with no list too: s2amd_export_wait(slot) then returns at once)
	HIP_TRY(hipEventRecord(exported, s->stream));
	return S2AMD_OK;
}

int s2amd_world_episode_states(s2amdSolver* s, s2amdEpisodeState* out, int32_t capacity, int32_t* count)
{
	const int rc = getterState(s, S2AMD_EPISODE_REPORT_STATES, "s2amd_world_episode_states", out, capacity, count, s ? s->episodeAgents : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	return reportCopyOut(s, out, s->dEpisodes, layoutOf(s).states, *count, sizeof(s2amdEpisodeState), hipMemcpyDeviceToHost);
}

int s2amd_world_episode_rule_states(s2amdSolver* s, s2amdEpisodeRuleState* out, int32_t capacity, int32_t* count)
{
	const int rc = getterState(s, S2AMD_EPISODE_REPORT_RULE_STATES, "s2amd_world_episode_rule_states", out, capacity, count, s ? (int)s->hEpisodeRules.size() : 0);
	if (rc || *count == 0)
	{
		return rc;
	}
	return reportCopyOut(s, out, s->dEpisodes, layoutOf(s).ruleStates, *count, sizeof(s2amdEpisodeRuleState), hipMemcpyDeviceToHost);
}

int s2amd_world_episode_events(s2amdSolver* s, s2amdEpisodeEvent* out, int32_t capacity, int32_t* count)
{
	if (!s || !count || capacity < 0 || (capacity > 0 && !out))
	{
		return fail(S2AMD_E_INVALID, "bad argument");
	}
	// (the state alone: how many there are is the device's to say)
	int32_t agents = 0;
	int rc = getterState(s, S2AMD_EPISODE_REPORT_EVENTS, "s2amd_world_episode_events", &agents, S2AMD_MAX_EPISODE_AGENTS, &agents, s->episodeAgents);
	if (rc || agents == 0)
	{
		*count = rc ? *count : 0;
		return rc;
	}
	int32_t counts[8];
	if ((rc = fetchCounts(s, counts)) != 0)
	{
		return rc;
	}
	*count = std::min(std::max(counts[4], 0), agents);
	if (*count > capacity)
	{
		return fail(S2AMD_E_CAPACITY, "s2amd_world_episode_events: buffer too small");
	}
	return reportCopyOut(s, out, s->dEpisodes, layoutOf(s).events, *count, sizeof(s2amdEpisodeEvent), hipMemcpyDeviceToHost);
}

int s2amd_world_episode_counts(s2amdSolver* s, int32_t counts[8])
{
	int32_t count = 0;
	const int rc = getterState(s, 0, "s2amd_world_episode_counts", counts, 8, &count, 8);
	if (rc)
	{
		return rc;
	}
	if (count == 0)
	{
		for (int k = 0; k < 8; ++k)
		{
			counts[k] = 0;
		}
		return S2AMD_OK;
	}
	return fetchCounts(s, counts);
}

} // extern "C"
#pragma GCC visibility pop
