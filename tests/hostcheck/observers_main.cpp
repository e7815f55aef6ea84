// TEST INFRASTRUCTURE.  The host side of the observers (solver2d_amd/csrc/observers.hip: validation with the overlap check, the list's
// device block and its replacement, the ring's head, the one- or two-piece export, the getters' state machine and the ninth entry of
// report_host.cpp's table) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with ASan + UBSan and linked
// against _build/libs2amd_hostcheck.so.  Kernels never run here, so this program plays the kernel's one write: after every step it fills
// the ring row the host chose (every row of a fresh ring) with that step's number, and then checks that the three ways out give the
// history the header states -- for frames = 1, 2, 3 (and more) over more steps than frames, so that every head position is exported,
// across re-bases by upload, by list replacement and by the flags, and across steps with the flags at 0.  Every buffer is a heap block
// of exactly the size passed.  Built and run by tests/test_observers_host.py.
#include "report_main_common.h"

#include <deque>

static int widthOf(int kind)
{
	return kind == 1 || kind == 2 || kind == 4 || kind == 9 ? 2 : 1;
}

// `count` observers, kinds 1..11 in turn, channels packed with a gap of one uncovered channel after every fifth
static std::vector<s2amdObserver> makeList(int count, int targets, int* channels)
{
	std::vector<s2amdObserver> list;
	int at = 0;
	for (int k = 0; k < count; ++k)
	{
		s2amdObserver o = {};
		o.kind = 1 + k % 11;
		o.target = targets > 0 ? k % targets : 0;
		o.frame = o.kind <= 5 && k % 3 == 0 ? (k + 1) % (targets > 0 ? targets : 1) : -1;
		o.channel = at;
		o.flags = (k % 5 == 4 ? S2AMD_OBSERVER_DISABLED : 0) | (k % 2 == 1 ? S2AMD_OBSERVER_RELATIVE : 0);
		o.gain = 1.5f, o.bias = -0.25f, o.lower = k % 2 == 0 ? -INFINITY : -2.0f, o.upper = k % 3 == 0 ? INFINITY : 2.0f;
		o.local[0] = 0.6f, o.local[1] = 0.8f;
		at += widthOf(o.kind) + (k % 5 == 4 ? 1 : 0);
		list.push_back(o);
	}
	*channels = at > 0 ? at : 1;
	return list;
}

static size_t roundUp(size_t bytes)
{
	return ((bytes > 0 ? bytes : 1) + 255) & ~size_t(255);
}

// (observers.hip: observerLayout) where the ring lies in the list's block
static float* ringOf(s2amdSolver* s)
{
	const size_t count = s->hObservers.size();
	return (float*)((char*)s->dObservers.p + roundUp(8 * sizeof(int)) + roundUp(count * sizeof(s2amdObserver)) + roundUp(count * sizeof(s2amdObserverState)));
}

// the statement's history, newest first
struct Model
{
	std::deque<float> frames;
	bool fresh = true;
	void push(float v, int n)
	{
		if (fresh)
		{
			frames.assign((size_t)n, v);
		}
		else
		{
			frames.push_front(v);
			frames.pop_back();
		}
		fresh = false;
	}
};

// one step with the report on, the kernel's write played, the model advanced
static void stepOn(s2amdSolver* s, Model& m, float value)
{
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	const bool wasFresh = s->observationFresh;
	const int headBefore = s->observationHead;
	EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
	const int frames = s->observationFrames, channels = s->observationChannels;
	if (s->hObservers.empty())
	{
		return;
	}
	EXPECT(s->observationFresh ? 1 : 0, 0);
	EXPECT(s->observationHead, wasFresh ? 0 : (headBefore + frames - 1) % frames);
	EXPECT(s->observationHead >= 0 && s->observationHead < frames ? 1 : 0, 1);
	float* ring = ringOf(s);
	for (int row = 0; row < frames; ++row)
	{
		if (wasFresh || row == s->observationHead)
		{
			for (int c = 0; c < channels; ++c)
			{
				ring[(size_t)row * channels + c] = value + 0.001f * (float)c;
			}
		}
	}
	m.push(value, frames);
}

// the three ways out against the model, into blocks of exactly frames * channels floats; then the refusals of a too-small block
static void checkOut(s2amdSolver* s, const Model& m)
{
	const int frames = s->observationFrames, channels = s->observationChannels, n = frames * channels;
	for (int way = 0; way < 3; ++way)
	{
		Exact<float> out(n);
		int32_t count = -7;
		void* device = nullptr;
		EXPECT(s2amd_device_alloc(s, 4u * (uint64_t)n, &device), S2AMD_OK);
		if (way == 0)
		{
			EXPECT(s2amd_world_observations(s, out.p, n, &count), S2AMD_OK);
			EXPECT(count, n);
		}
		else
		{
			EXPECT(way == 1 ? s2amd_world_export_observations(s, device, n) : s2amd_world_export_observations_async(s, device, n, way), S2AMD_OK);
			if (way == 2)
			{
				EXPECT(s2amd_export_wait(s, way), S2AMD_OK);
			}
			EXPECT(s2amd_device_read(s, out.p, device, 4u * (uint64_t)n), S2AMD_OK);
		}
		int wrong = 0;
		for (int f = 0; f < frames; ++f)
		{
			for (int c = 0; c < channels; ++c)
			{
				wrong += out.p[(size_t)f * channels + c] != m.frames[(size_t)f] + 0.001f * (float)c ? 1 : 0;
			}
		}
		EXPECT(wrong, 0);
		EXPECT(s2amd_device_free(s, device), S2AMD_OK);
	}
	Exact<float> small(n - 1);
	int32_t count = -7;
	EXPECT(s2amd_world_observations(s, small.p, n - 1, &count), S2AMD_E_CAPACITY);
	EXPECT(count, n);
	EXPECT(s2amd_world_observations(s, small.p, -1, &count), S2AMD_E_INVALID);
	EXPECT(s2amd_world_observations(s, nullptr, 1, &count), S2AMD_E_INVALID);
	void* device = nullptr;
	EXPECT(s2amd_device_alloc(s, 4u * (uint64_t)n, &device), S2AMD_OK);
	EXPECT(s2amd_world_export_observations(s, device, n - 1), S2AMD_E_CAPACITY);
	EXPECT(s2amd_world_export_observations_async(s, device, n - 1, 0), S2AMD_E_CAPACITY);
	EXPECT(s2amd_world_export_observations_async(s, device, n, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_export_observations_async(s, device, n, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_device_free(s, device), S2AMD_OK);
}

static void askStates(s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<s2amdObserverState> out(capacity);
	int32_t count = -7;
	EXPECT(s2amd_world_observer_states(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
	Exact<int32_t> counts(4);
	EXPECT(s2amd_world_observer_counts(s, counts.p), wantRc == S2AMD_E_CAPACITY || wantRc == S2AMD_E_INVALID ? S2AMD_OK : wantRc);
}

// every refusal; the old list, its sizes and its ring's head stand
static void refusals(s2amdSolver* s)
{
	int channels = 0;
	const std::vector<s2amdObserver> list = makeList(12, 7, &channels);
	const size_t held = s->hObservers.size();
	const int heldChannels = s->observationChannels, heldFrames = s->observationFrames, heldHead = s->observationHead;
	const bool heldFresh = s->observationFresh;
	const int heldStepFlags = s->observationReport.stepFlags;
	EXPECT(s2amd_world_set_observers(s, list.data(), -1, channels, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, nullptr, 3, channels, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(nullptr, list.data(), 3, channels, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, list.data(), 12, 0, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, list.data(), 12, S2AMD_MAX_OBSERVATION_CHANNELS + 1, 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, list.data(), 12, channels, 0), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, list.data(), 12, channels, S2AMD_MAX_OBSERVATION_FRAMES + 1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observers(s, list.data(), 12, channels - 1, 1), S2AMD_E_INVALID); // the last observer's channel
	const std::vector<s2amdObserver> many((size_t)S2AMD_MAX_OBSERVERS + 1, list[2]);
	EXPECT(s2amd_world_set_observers(s, many.data(), S2AMD_MAX_OBSERVERS + 1, channels, 1), S2AMD_E_INVALID);
	for (int bad = 0; bad < 20; ++bad)
	{
		std::vector<s2amdObserver> wrong = list;
		s2amdObserver& o = wrong[(size_t)(bad % 12)];
		switch (bad)
		{
		case 0: o.kind = 0; break;
		case 1: o.kind = 12; break;
		case 2: o.target = -1; break;
		case 3: o.channel = -1; break;
		case 4: o.channel = channels; break;
		case 5: o.flags = 4; break;
		case 6: o.flags = -1; break;
		case 7: o.reserved[4] = 1; break;
		case 8: o.gain = NAN; break;
		case 9: o.bias = INFINITY; break;
		case 10: o.local[1] = NAN; break;
		case 11: o.frame = -2; break;
		case 12: o.lower = NAN; break;
		case 13: o.upper = NAN; break;
		case 14: o.lower = 3.0f, o.upper = 2.0f; break;
		case 15: wrong[5].frame = 0; break;				   // kind 6 with a frame
		case 16: wrong[10].frame = 1; break;			   // kind 11 with a frame
		case 17: wrong[3].channel = wrong[2].channel; break; // two observers on one channel
		case 18: wrong[1].channel = wrong[0].channel + 1; break; // a width-2 range's second channel
		default: o.channel = INT32_MAX; break;			   // (channel + width must not wrap)
		}
		EXPECT(s2amd_world_set_observers(s, wrong.data(), (int32_t)wrong.size(), channels, 2), S2AMD_E_INVALID);
	}
	EXPECT(s2amd_world_set_observation_report(s, 4), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_observation_report(nullptr, 1), S2AMD_E_INVALID);
	EXPECT((int)s->hObservers.size(), (int)held);
	EXPECT(s->observationChannels, heldChannels);
	EXPECT(s->observationFrames, heldFrames);
	EXPECT(s->observationHead, heldHead);
	EXPECT(s->observationFresh ? 1 : 0, heldFresh ? 1 : 0);
	EXPECT(s->observationReport.stepFlags, heldStepFlags);
}

static void drive(const World& first, const World& second, int count, int frames)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	const int both = S2AMD_OBSERVATION_REPORT_VECTOR | S2AMD_OBSERVATION_REPORT_STATES;
	int channels = 0;
	// no list, no world
	refusals(s);
	askStates(s, 4, S2AMD_OK, 0);
	// a list before any world, the report on before any world
	std::vector<s2amdObserver> list = makeList(count, 30, &channels);
	EXPECT(s2amd_world_set_observers(s, list.data(), count, channels, frames), S2AMD_OK);
	EXPECT(s2amd_world_set_observation_report(s, both), S2AMD_OK);
	askStates(s, count, count > 0 ? S2AMD_E_STATE : S2AMD_OK, count > 0 ? -7 : 0);
	float stamp = 1.0f;
	const World* worlds[3] = {&first, &second, &first};
	for (int pass = 0; pass < 3; ++pass)
	{
		EXPECT(upload(s, *worlds[pass]), S2AMD_OK);
		EXPECT((int)s->hObservers.size(), count); // the list holds across uploads
		EXPECT(s->observationFresh ? 1 : 0, 1);	  // ... and the history is re-based
		refusals(s);
		askStates(s, count, count > 0 ? S2AMD_E_STATE : S2AMD_OK, count > 0 ? -7 : 0); // no step since the upload
		Model m;
		for (int step = 0; step < 2 * frames + 3; ++step)
		{
			stepOn(s, m, stamp);
			stamp += 1.0f;
			if (count > 0)
			{
				checkOut(s, m);
				askStates(s, count - 1, S2AMD_E_CAPACITY, count);
			}
			askStates(s, -1, S2AMD_E_INVALID, -7);
			askStates(s, count, S2AMD_OK, count);
			if (step == frames)
			{
				// a step with the flags at 0 is none: the head stays, the getters refuse, and turning them on again re-bases
				const int head = s->observationHead;
				EXPECT(s2amd_world_set_observation_report(s, 0), S2AMD_OK);
				EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
				EXPECT(s->observationHead, head);
				askStates(s, count, count > 0 ? S2AMD_E_STATE : S2AMD_OK, count > 0 ? -7 : 0);
				EXPECT(s2amd_world_set_observation_report(s, S2AMD_OBSERVATION_REPORT_VECTOR), S2AMD_OK);
				EXPECT(s->observationFresh ? 1 : 0, 1);
				m.fresh = true;
				stepOn(s, m, stamp);
				stamp += 1.0f;
				if (count > 0)
				{
					checkOut(s, m);
					Exact<s2amdObserverState> states(count);
					int32_t got = -7;
					EXPECT(s2amd_world_observer_states(s, states.p, count, &got), S2AMD_E_STATE); // (the vector alone was asked for)
				}
				EXPECT(s2amd_world_set_observation_report(s, both), S2AMD_OK); // (non-zero to non-zero: no re-base)
				EXPECT(s->observationFresh ? 1 : 0, count > 0 ? 0 : 1); // (an empty list has no ring to write)
			}
		}
		refusals(s);
		if (count > 0)
		{
			checkOut(s, m); // a refused list leaves the answers in place
		}
		// replaced: re-based, the getters refuse until a step, and the new sizes hold
		int here = 0;
		const int fewer = count > 1 ? count / 2 : count;
		std::vector<s2amdObserver> other = makeList(fewer, 5, &here);
		const int otherFrames = frames % S2AMD_MAX_OBSERVATION_FRAMES + 1;
		EXPECT(s2amd_world_set_observers(s, other.data(), fewer, here + 3, otherFrames), S2AMD_OK);
		EXPECT(s->observationFresh ? 1 : 0, 1);
		askStates(s, fewer, fewer > 0 ? S2AMD_E_STATE : S2AMD_OK, fewer > 0 ? -7 : 0);
		Model n;
		for (int step = 0; step < otherFrames + 2; ++step)
		{
			stepOn(s, n, stamp);
			stamp += 1.0f;
			if (fewer > 0)
			{
				checkOut(s, n);
			}
		}
		// cleared: count 0 at once
		EXPECT(s2amd_world_set_observers(s, nullptr, 0, 0, 0), S2AMD_OK);
		askStates(s, 0, S2AMD_OK, 0);
		int32_t none = -7;
		EXPECT(s2amd_world_observations(s, nullptr, 0, &none), S2AMD_OK);
		EXPECT(none, 0);
		EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
		// the first list again, for the next upload
		EXPECT(s2amd_world_set_observers(s, list.data(), count, channels, frames), S2AMD_OK);
	}
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0), small = makeWorld(40), big = makeWorld(300);
	const int counts[5] = {0, 1, 65, 1000, S2AMD_MAX_OBSERVERS};
	for (int count : counts)
	{
		for (int frames = 1; frames <= (count == 65 ? 5 : 3); ++frames)
		{
			if (count > 1000 && frames != 2)
			{
				continue; // (the largest list once: its ring is 16,384 observers' channels wide)
			}
			drive(small, big, count, frames);
			drive(none, small, count, frames);
		}
	}
	drive(big, none, 257, S2AMD_MAX_OBSERVATION_FRAMES);
	if (failures == 0)
	{
		printf("OBSERVERS MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
