// TEST INFRASTRUCTURE.  What a solver owns and gives back (solver2d_amd/csrc/solver.cpp: s2amd_destroy over solver_internal.h's two
// inventories of device blocks, the pinned stages and blocks, the events and streams) on the stand-in HIP runtime of tests/hostcheck, as
// a stand-alone program compiled with ASan + UBSan and linked against _build/libs2amd_hostcheck.so, run with the leak check on: a
// solver with a world, every list set and every report on, two steps, each staged writer twice in a row (the second call waits for the
// first one's copy and finds the stage too small), one asynchronous export per slot, a world of another size, and the destroy -- after
// which nothing may be left on the heap (a device block, a pinned block, an event and a stream are heap blocks there) and nothing may
// have been given back twice.  The simplest valid item stands for each list: what the lists hold is the business of their own programs.
// The first run of s2amd_world_edit on the stand-in runtime as well.  Built and run by tests/test_teardown_host.py.
#include "report_main_common.h"

static const s2amdStepParams PARAMS = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};

// every mounted list, `count` items each on body slots 0 .. bodies - 1, and all three reports of each
static void setMountedLists(s2amdSolver* s, int count, int bodies)
{
	std::vector<s2amdSensor> sensors((size_t)count, s2amdSensor{});
	std::vector<s2amdRaySensor> rays((size_t)count, s2amdRaySensor{});
	std::vector<s2amdGridSensor> grids((size_t)count, s2amdGridSensor{});
	for (int k = 0; k < count; ++k)
	{
		s2amdSensor& q = sensors[(size_t)k];
		q.count = 1, q.radius = 0.25f, q.rot[1] = 1.0f, q.maskBits = 0xffffffffu, q.body = k % bodies;
		s2amdRaySensor& r = rays[(size_t)k];
		r.p1[1] = 3.0f, r.p2[1] = -1.0f, r.maxFraction = 1.0f, r.maskBits = 0xffffffffu, r.body = k % bodies;
		s2amdGridSensor& g = grids[(size_t)k];
		g.rot[1] = 1.0f, g.cellSize = 0.25f, g.width = 3, g.height = 9, g.maskBits = 0xffffffffu, g.body = k % bodies;
	}
	EXPECT(s2amd_world_set_sensors(s, sensors.data(), count), S2AMD_OK);
	EXPECT(s2amd_world_set_sensor_report(s, S2AMD_SENSOR_REPORT_INSIDE | S2AMD_SENSOR_REPORT_EVENTS | S2AMD_SENSOR_REPORT_STATES, 64), S2AMD_OK);
	EXPECT(s2amd_world_set_ray_sensors(s, rays.data(), count), S2AMD_OK);
	EXPECT(s2amd_world_set_ray_report(s, S2AMD_RAY_REPORT_STATES | S2AMD_RAY_REPORT_RANGES | S2AMD_RAY_REPORT_EVENTS), S2AMD_OK);
	EXPECT(s2amd_world_set_grid_sensors(s, grids.data(), count), S2AMD_OK);
	EXPECT(s2amd_world_set_grid_report(s, S2AMD_GRID_REPORT_CATEGORIES | S2AMD_GRID_REPORT_SHAPES | S2AMD_GRID_REPORT_OCCUPANCY | S2AMD_GRID_REPORT_STATES), S2AMD_OK);
}

static std::vector<s2amdField> makeFields(int count, int bodies)
{
	std::vector<s2amdField> fields((size_t)count, s2amdField{});
	for (int k = 0; k < count; ++k)
	{
		s2amdField& f = fields[(size_t)k];
		f.count = 1, f.radius = 0.25f, f.range = 2.0f, f.rot[1] = 1.0f, f.maskBits = 0xffffffffu, f.body = k % bodies;
		f.kind = S2AMD_FIELD_UNIFORM, f.strength = 1.5f, f.direction[0] = 0.6f, f.direction[1] = -0.8f;
	}
	return fields;
}

// a force on every body slot (two channels each), a point observer on every body slot (two channels each, two frames), one agent per
// body slot with a step limit and one reward rule, and one reset record per body slot under that agent; every report of theirs on
static int setAgentLists(s2amdSolver* s, int bodies)
{
	std::vector<s2amdActuator> actuators((size_t)bodies, s2amdActuator{});
	std::vector<s2amdObserver> observers((size_t)bodies, s2amdObserver{});
	std::vector<s2amdEpisodeRule> rules((size_t)bodies, s2amdEpisodeRule{});
	std::vector<s2amdResetBody> resets((size_t)bodies, s2amdResetBody{});
	const std::vector<int32_t> limits((size_t)bodies, 3);
	for (int k = 0; k < bodies; ++k)
	{
		s2amdActuator& a = actuators[(size_t)k];
		a.kind = S2AMD_ACTUATOR_BODY_FORCE, a.target = k, a.channel = 2 * k, a.gain = 1.5f, a.lower = -2.0f, a.upper = 2.0f;
		s2amdObserver& o = observers[(size_t)k];
		o.kind = S2AMD_OBSERVER_BODY_POINT, o.target = k, o.frame = -1, o.channel = 2 * k, o.gain = 1.5f, o.lower = -2.0f, o.upper = 2.0f;
		s2amdEpisodeRule& r = rules[(size_t)k];
		r.kind = 1, r.agent = k, r.channelA = 2 * k, r.gain = 1.5f, r.lower = -2.0f, r.upper = 2.0f;
		s2amdResetBody& b = resets[(size_t)k];
		b.agent = k, b.body = k, b.rot[1] = 1.0f, b.positionJitter[0] = 0.25f;
	}
	EXPECT(s2amd_world_set_fields(s, makeFields(3, bodies).data(), 3), S2AMD_OK);
	EXPECT(s2amd_world_set_actuators(s, actuators.data(), bodies, 2 * bodies), S2AMD_OK);
	EXPECT(s2amd_world_set_observers(s, observers.data(), bodies, 2 * bodies, 2), S2AMD_OK);
	EXPECT(s2amd_world_set_observation_report(s, S2AMD_OBSERVATION_REPORT_VECTOR | S2AMD_OBSERVATION_REPORT_STATES), S2AMD_OK);
	EXPECT(s2amd_world_set_episodes(s, rules.data(), bodies, bodies, limits.data()), S2AMD_OK);
	EXPECT(s2amd_world_set_episode_report(s, S2AMD_EPISODE_REPORT_STEP | S2AMD_EPISODE_REPORT_STATES | S2AMD_EPISODE_REPORT_RULE_STATES | S2AMD_EPISODE_REPORT_EVENTS), S2AMD_OK);
	EXPECT(s2amd_world_set_resets(s, resets.data(), bodies, nullptr, 0, bodies, 7u), S2AMD_OK);
	EXPECT(s2amd_world_set_reset_report(s, S2AMD_RESET_ON_EPISODE_END | S2AMD_RESET_REPORT_STATES), S2AMD_OK);
	return 2 * bodies; // action and observation channels
}

// each of the four writers through a pinned stage twice in a row, the second list longer than the first one's stage (4,096 bytes at the
// least) wherever the world is large enough for one
static void stagedWriters(s2amdSolver* s, int bodies, int channels)
{
	std::vector<s2amdWorldEdit> edits;
	for (int k = 0; k < 2 * bodies; ++k)
	{
		s2amdWorldEdit e = {};
		e.kind = 1 + k % 4, e.target = k % bodies, e.v[0] = 0.5f;
		edits.push_back(e);
	}
	int32_t skipped = -7;
	EXPECT(s2amd_world_edit(s, edits.data(), bodies, nullptr), S2AMD_OK); // distinct targets
	EXPECT(s2amd_world_edit(s, edits.data(), 2 * bodies, &skipped), S2AMD_OK); // every target twice: the sorted walk
	EXPECT(skipped, 0);

	const std::vector<s2amdField> fields = makeFields(std::min(2 * bodies, S2AMD_MAX_FIELDS), bodies);
	Exact<s2amdFieldState> states((int)fields.size());
	EXPECT(s2amd_world_apply_fields(s, fields.data(), 1, nullptr), S2AMD_OK);
	EXPECT(s2amd_world_apply_fields(s, fields.data(), (int32_t)fields.size(), states.p), S2AMD_OK);

	const std::vector<float> actions((size_t)channels, 0.25f);
	EXPECT(s2amd_world_set_actions(s, actions.data(), channels - 1, 1), S2AMD_OK);
	EXPECT(s2amd_world_set_actions(s, actions.data(), 0, channels), S2AMD_OK);

	const int32_t who[3] = {bodies - 1, 0, bodies - 1};
	EXPECT(s2amd_world_reset_agents(s, who, 3), S2AMD_OK);
	EXPECT(s2amd_world_reset_agents(s, who + 1, 1), S2AMD_OK);
}

// one asynchronous export per slot, each through another entry point, into exact device blocks of the caller's
static void exports(s2amdSolver* s, int bodies, int channels)
{
	void *poses = nullptr, *records = nullptr, *vector = nullptr, *rewards = nullptr, *flags = nullptr;
	EXPECT(s2amd_device_alloc(s, 16u * (uint64_t)bodies, &poses), S2AMD_OK);
	EXPECT(s2amd_device_alloc(s, 32u * (uint64_t)bodies, &records), S2AMD_OK);
	EXPECT(s2amd_device_alloc(s, 4u * 2u * (uint64_t)channels, &vector), S2AMD_OK);
	EXPECT(s2amd_device_alloc(s, 4u * (uint64_t)bodies, &rewards), S2AMD_OK);
	EXPECT(s2amd_device_alloc(s, 4u * (uint64_t)bodies, &flags), S2AMD_OK);
	for (int round = 0; round < 2; ++round) // (the second round finds the four events made)
	{
		EXPECT(s2amd_export_poses_async(s, poses, bodies, 0), S2AMD_OK);
		EXPECT(s2amd_export_bodies_async(s, records, bodies, 1), S2AMD_OK);
		EXPECT(s2amd_world_export_observations_async(s, vector, 2 * channels, 2), S2AMD_OK);
		EXPECT(s2amd_world_export_episode_step_async(s, rewards, flags, bodies, 3), S2AMD_OK);
		for (int slot = 0; slot < 4; ++slot)
		{
			EXPECT(s2amd_export_wait(s, slot), S2AMD_OK);
		}
	}
	for (void* p : {poses, records, vector, rewards, flags})
	{
		EXPECT(s2amd_device_free(s, p), S2AMD_OK);
	}
}

static void drive(const World& first, const World& second)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	EXPECT(upload(s, first), S2AMD_OK);
	const int bodies = (int)first.bodies.size();
	setMountedLists(s, 5, bodies);
	const int channels = setAgentLists(s, bodies);
	EXPECT(s2amd_world_set_report(s, S2AMD_REPORT_TOUCH | S2AMD_REPORT_CONTACTS | S2AMD_REPORT_BODY_SUMS), S2AMD_OK);
	EXPECT(s2amd_world_set_joint_report(s, S2AMD_JOINT_REPORT_STATES | S2AMD_JOINT_REPORT_LIMITS | S2AMD_JOINT_REPORT_BODY_SUMS), S2AMD_OK);
	EXPECT(s2amd_world_set_shape_report(s, S2AMD_SHAPE_REPORT_DRAW | S2AMD_SHAPE_REPORT_VIEW | S2AMD_SHAPE_REPORT_BOUNDS), S2AMD_OK);
	EXPECT(s2amd_world_set_body_report(s, S2AMD_BODY_REPORT_STATES | S2AMD_BODY_REPORT_REST | S2AMD_BODY_REPORT_ISLANDS), S2AMD_OK);
	EXPECT(s2amd_world_set_metrics(s, S2AMD_METRICS_CONTACTS | S2AMD_METRICS_BODIES | S2AMD_METRICS_JOINTS, 8), S2AMD_OK);
	s2amdWorldStepInfo info;
	EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
	EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
	stagedWriters(s, bodies, channels);
	exports(s, bodies, channels);
	// (the resets and the device trees refuse each other: the list goes, and the trees' stream and events are the destroy's to free too)
	EXPECT(s2amd_world_set_resets(s, nullptr, 0, nullptr, 0, 0, 0u), S2AMD_OK);
	EXPECT(s2amd_world_set_tree(s, 0, nullptr, 0, -1), S2AMD_OK);
	EXPECT(upload(s, second), S2AMD_OK);
	EXPECT(s2amd_world_step(s, &PARAMS, &info), S2AMD_OK);
	s2amd_destroy(s);
}

int main()
{
	const World none = makeWorld(0), small = makeWorld(40), big = makeWorld(700);
	drive(none, small);
	drive(small, big);
	drive(big, none);
	if (failures == 0)
	{
		printf("TEARDOWN MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
