// TEST INFRASTRUCTURE.  The host sides of the contact report and the joint report (solver2d_amd/csrc/contact_report.hip, joint_report.hip:
// layout, prepare, enqueue, setters, getters, and report_host.cpp behind them) on the stand-in HIP runtime of tests/hostcheck, as a
// stand-alone program compiled with ASan + UBSan and linked against _build/libs2amd_hostcheck.so: upload -> every flag combination of
// both reports -> every getter with too-small, exact and ample buffers -> uploads with other capacities, worlds without contact slots
// and without joint slots among them -> destroy.  Kernels never run here, so the heads the write passes would leave (counts, and the
// joint summary) are written by this program at the report states' headOffset: what is checked is that the host side touches only
// memory it owns -- every output buffer is a heap block of exactly the size passed.  Built and run by tests/test_report_host.py.
#include "report_main_common.h"

// makeWorld(count) with `contactSlots` free contact slots and `jointSlots` free joint slots: the blocks are sized by the capacities,
// whatever the slots hold
static World worldWith(int count, int contactSlots, int jointSlots)
{
	World w = makeWorld(count);
	w.contacts.assign((size_t)contactSlots, s2amdContact{});
	w.pairs.assign((size_t)contactSlots, s2amdPairState{});
	for (size_t i = 0; i < w.contacts.size(); ++i)
	{
		w.contacts[i].constraintIndex = -1;
		w.pairs[i].shapeA = w.pairs[i].shapeB = -1;
	}
	w.joints.assign((size_t)jointSlots, s2amdJoint{});
	for (s2amdJoint& j : w.joints)
	{
		j.type = S2AMD_JOINT_FREE;
	}
	return w;
}

// in place of the contact report's write pass: {began, ended, touching, 0}
static void writeContactHead(s2amdSolver* s, int began, int ended, int touching)
{
	const int32_t head[4] = {began, ended, touching, 0};
	memcpy((char*)s->contactReport.block.p + s->contactReport.headOffset, head, sizeof(head));
}

// in place of the joint report's write pass: {live, began, ended, 0} and a summary
static void writeJointHead(s2amdSolver* s, int live, int began, int ended)
{
	struct
	{
		int32_t counts[4];
		s2amdJointSummary summary;
	} head = {};
	head.counts[0] = live, head.counts[1] = began, head.counts[2] = ended;
	head.summary.liveJoints = live, head.summary.maxGapSlot = live - 1;
	memcpy((char*)s->jointReport.block.p + s->jointReport.headOffset, &head, sizeof(head));
}

template <typename T, typename Fn> static void askList(Fn fn, s2amdSolver* s, int capacity, int wantRc, int wantCount)
{
	Exact<T> out(capacity);
	int32_t count = -7;
	EXPECT(fn(s, out.p, capacity, &count), wantRc);
	EXPECT(count, wantCount);
}

template <typename Fn> static void askEvents(Fn fn, s2amdSolver* s, int capacityA, int capacityB, int wantRc, int wantA, int wantB)
{
	Exact<int32_t> a(capacityA), b(capacityB);
	int32_t nA = -7, nB = -7;
	EXPECT(fn(s, a.p, capacityA, &nA, b.p, capacityB, &nB), wantRc);
	EXPECT(nA, wantA);
	EXPECT(nB, wantB);
}

template <typename T, typename Fn> static void askBodyArray(Fn fn, s2amdSolver* s, int capacity, int wantRc)
{
	Exact<T> out(capacity);
	EXPECT(fn(s, out.p, capacity), wantRc);
}

// a counted list after a step that ran with its flag set (`on`) or without it
template <typename T, typename Fn> static void listGetter(Fn fn, s2amdSolver* s, bool on, int n)
{
	if (!on)
	{
		askList<T>(fn, s, 4, S2AMD_E_STATE, -7);
		return;
	}
	askList<T>(fn, s, -1, S2AMD_E_INVALID, -7);
	if (n > 0)
	{
		askList<T>(fn, s, n - 1, S2AMD_E_CAPACITY, n);
		askList<T>(fn, s, 0, S2AMD_E_CAPACITY, n);
	}
	askList<T>(fn, s, n, S2AMD_OK, n);
	askList<T>(fn, s, n + 5, S2AMD_OK, n);
}

template <typename Fn> static void eventGetter(Fn fn, s2amdSolver* s, bool on, int a, int b)
{
	if (!on)
	{
		askEvents(fn, s, 4, 4, S2AMD_E_STATE, -7, -7);
		return;
	}
	askEvents(fn, s, -1, b, S2AMD_E_INVALID, -7, -7);
	if (a > 0)
	{
		askEvents(fn, s, a - 1, b, S2AMD_E_CAPACITY, a, b);
	}
	if (b > 0)
	{
		askEvents(fn, s, a, b - 1, S2AMD_E_CAPACITY, a, b);
	}
	askEvents(fn, s, a, b, S2AMD_OK, a, b);
	askEvents(fn, s, a + 3, b + 9, S2AMD_OK, a, b);
}

template <typename T, typename Fn> static void bodyArrayGetter(Fn fn, s2amdSolver* s, bool on, int nb)
{
	if (!on)
	{
		askBodyArray<T>(fn, s, nb + 4, S2AMD_E_STATE);
		return;
	}
	askBodyArray<T>(fn, s, -1, S2AMD_E_INVALID);
	if (nb > 0)
	{
		askBodyArray<T>(fn, s, nb - 1, S2AMD_E_CAPACITY);
		askBodyArray<T>(fn, s, 0, S2AMD_E_CAPACITY);
	}
	askBodyArray<T>(fn, s, nb, S2AMD_OK);
	askBodyArray<T>(fn, s, nb + 5, S2AMD_OK);
}

// `fresh`: the first getters after the step, which fetch the head; later ones answer from the host copy whatever lies in the block
static void contactGettersAfterStep(s2amdSolver* s, int flags, int nc, int nb, bool fresh)
{
	// the largest counts the passes can leave: every slot touching, every slot in one of the lists; a world without contact slots
	// launches no tile, and its counts are zero without a look at the block
	if (fresh && nc > 0)
	{
		writeContactHead(s, nc / 2, nc - nc / 2, nc);
	}
	else
	{
		writeContactHead(s, 1, 1, 1);
	}
	eventGetter(s2amd_world_touch_events, s, (flags & S2AMD_REPORT_TOUCH) != 0, nc / 2, nc - nc / 2);
	listGetter<s2amdTouchingContact>(s2amd_world_touching, s, (flags & S2AMD_REPORT_CONTACTS) != 0, nc);
	bodyArrayGetter<s2amdBodyContactSum>(s2amd_world_body_sums, s, (flags & S2AMD_REPORT_BODY_SUMS) != 0, nb);
}

static void jointGettersAfterStep(s2amdSolver* s, int flags, int nj, int nb)
{
	// every slot live, both codes of every slot in the began list and one in the ended list: each list holds 2 * nj codes
	// (a world without joint slots launches no tile: zero counts and the empty summary without a look at the block)
	if (nj > 0)
	{
		writeJointHead(s, nj, 2 * nj, nj);
	}
	else
	{
		writeJointHead(s, 5, 5, 5);
	}
	s2amdJointSummary summary;
	summary.liveJoints = -7;
	EXPECT(s2amd_world_joint_summary(s, &summary), flags != 0 ? S2AMD_OK : S2AMD_E_STATE);
	EXPECT(summary.liveJoints, flags != 0 ? nj : -7);
	if (flags != 0)
	{
		EXPECT(summary.maxGapSlot, nj - 1); // (nj == 0: the -1 the host leaves without asking the device)
	}
	EXPECT(s2amd_world_joint_summary(s, nullptr), S2AMD_E_INVALID);
	listGetter<s2amdJointState>(s2amd_world_joint_states, s, (flags & S2AMD_JOINT_REPORT_STATES) != 0, nj);
	eventGetter(s2amd_world_joint_limit_events, s, (flags & S2AMD_JOINT_REPORT_LIMITS) != 0, 2 * nj, nj);
	bodyArrayGetter<s2amdBodyJointSum>(s2amd_world_body_joint_sums, s, (flags & S2AMD_JOINT_REPORT_BODY_SUMS) != 0, nb);
}

static void drive(const World& first, const World& second, bool flagsFirst)
{
	s2amdSolver* s = nullptr;
	EXPECT(s2amd_create(0, &s), S2AMD_OK);
	if (!s)
	{
		return;
	}
	s2amdStepParams params = {s2amd_solverTGS_Soft, 1.0f / 60.0f, 4, 2, 1, {0.0f, -10.0f}};
	s2amdWorldStepInfo info;
	s2amdJointSummary summary;
	EXPECT(s2amd_world_set_report(nullptr, 7), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_report(s, 8), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_joint_report(nullptr, 7), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_joint_report(s, 8), S2AMD_E_INVALID);
	EXPECT(s2amd_world_set_joint_report(s, -1), S2AMD_E_INVALID);
	EXPECT(s2amd_world_joint_summary(s, &summary), S2AMD_E_STATE); // no resident world
	EXPECT(s2amd_world_joint_summary(nullptr, &summary), S2AMD_E_INVALID);
	askList<s2amdTouchingContact>(s2amd_world_touching, s, 4, S2AMD_E_STATE, -7);
	askList<s2amdTouchingContact>(s2amd_world_touching, nullptr, 4, S2AMD_E_INVALID, -7);
	askEvents(s2amd_world_touch_events, nullptr, 4, 4, S2AMD_E_INVALID, -7, -7);
	askBodyArray<s2amdBodyContactSum>(s2amd_world_body_sums, nullptr, 4, S2AMD_E_INVALID);
	if (flagsFirst)
	{
		EXPECT(s2amd_world_set_report(s, 7), S2AMD_OK); // before any world: held for the upload
		EXPECT(s2amd_world_set_joint_report(s, 7), S2AMD_OK);
	}
	const World* worlds[3] = {&first, &second, &first};
	for (const World* w : worlds)
	{
		const int nc = (int)w->contacts.size(), nj = (int)w->joints.size(), nb = (int)w->bodies.size();
		EXPECT(upload(s, *w), S2AMD_OK);
		if (!flagsFirst)
		{
			EXPECT(s2amd_world_set_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_report(s, 7), S2AMD_OK); // prepares on the resident world
			EXPECT(s2amd_world_set_joint_report(s, 0), S2AMD_OK);
			EXPECT(s2amd_world_set_joint_report(s, 7), S2AMD_OK);
		}
		EXPECT(s2amd_world_joint_summary(s, &summary), S2AMD_E_STATE); // no step since the upload
		askList<s2amdTouchingContact>(s2amd_world_touching, s, 4, S2AMD_E_STATE, -7);
		for (int flags = 7; flags >= 0; --flags)
		{
			// every combination 0..7 of either report, the two out of step with each other; each is turned on from 0 once
			const int contactFlags = flags, jointFlags = (flags + 3) % 8;
			EXPECT(s2amd_world_set_report(s, contactFlags), S2AMD_OK);
			EXPECT(s2amd_world_set_joint_report(s, jointFlags), S2AMD_OK);
			EXPECT(s2amd_world_step(s, &params, &info), S2AMD_OK);
			contactGettersAfterStep(s, contactFlags, nc, nb, true);
			jointGettersAfterStep(s, jointFlags, nj, nb);
			contactGettersAfterStep(s, contactFlags, nc, nb, false);
		}
	}
	s2amd_destroy(s);
}

int main()
{
	const World small = worldWith(40, 4, 3), big = worldWith(700, 2300, 300); // one tile each; three, nine and two
	const World noContacts = worldWith(40, 0, 5), noJoints = worldWith(40, 6, 0), neither = worldWith(3, 0, 0);
	World empty = worldWith(3, 0, 0);
	empty.bodies.clear(), empty.origins.clear(), empty.shapes.clear(); // no slots at all
	for (int flagsFirst = 0; flagsFirst < 2; ++flagsFirst)
	{
		drive(small, big, flagsFirst != 0);
		drive(big, noContacts, flagsFirst != 0);
		drive(noJoints, small, flagsFirst != 0);
		drive(neither, big, flagsFirst != 0);
		drive(empty, small, flagsFirst != 0);
	}
	if (failures == 0)
	{
		printf("CONTACT JOINT REPORT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
