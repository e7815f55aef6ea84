// TEST INFRASTRUCTURE.  What becomes of created, destroyed and flipped contacts on the host (solver2d_amd/csrc/solver_incremental.cpp and its
// callers in solver_step.cpp and world.hip) on the stand-in HIP runtime of tests/hostcheck, as a stand-alone program compiled with
// ASan + UBSan and linked against _build/libs2amd_hostcheck.so, in the manner of query_main.cpp and mover_main.cpp.  Small box pyramids as
// wire arrays; a scripted churn of contacts between existing bodies -- created without points, given points a round later, destroyed,
// their slots used again -- run once through the host-array route (s2amd_upload + s2amd_step_resident) and once through the world route
// (s2amd_world_upload + s2amd_world_set_contacts + s2amd_world_step), in one scene per placement route: colour batches, a body whose
// colours are all taken, the sequential tail of a hub, a structure built for s2Solve_Jacobi, strips (rounds, adopted bodies, extended
// seams, opened spare rounds) under a soft solver and under the op interpreter.  After every call the program prints the return code,
// the counters of the structure, hashes of the sweep order and of the host shadows (each line only where it differs from what it said
// after the call before), and the call's patch list with every address
// resolved to the block that holds it; it then plays the list into the "device" blocks, which the patch kernel would have done.
// With S2_HOSTCHECK_TRACE_CALLS set hip_stub.cpp prints the launches, copies, memsets and waits of every upload and s2amd_world_set_contacts
// between the lines of this program (not those of the steps: hundreds of launches each).
// tests/hostcheck/placement_transcript.txt is stdout; tests/test_placement_host.py builds and runs the program and compares.
#include "report_main_common.h"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <set>
#include <string>
#include <utility>

static s2amdSolver* solver = nullptr;
static const bool tracing = getenv("S2_HOSTCHECK_TRACE_CALLS") != nullptr;

// the stand-in's call trace covers the calls that change the graph; a step's hundreds of launches are not what this program is about
static bool traced = true; // (off for a whole scene when a worker thread makes calls of its own meanwhile)
static void trace(bool on)
{
	on = on && traced;
	if (tracing)
	{
		on ? setenv("S2_HOSTCHECK_TRACE_CALLS", "1", 1) : unsetenv("S2_HOSTCHECK_TRACE_CALLS");
	}
}

static const char* const bufNames[] = {"dWatched", "dBodyFlags", "soaBodies", "soaContacts", "soaJoints", "dContactIndex", "dJointIndex", "dContactLocal", "dJointLocal",
									   "dAdjOffsets", "dAdjList", "dAdjHeavy", "dPatches", "dJointAdjRange", "dJointAdjList", "dResidentDesc", "dResidentOps", "dStripLean",
									   "dPersist", "dGranules", "dOverflowBodies", "dPersistOps", "dJacobi", "dJacobiGran", "dMsg", "dGroups", "dContactTail",
									   "dJointTail", "dStripA", "dStripB", "dResident"};

struct Scene
{
	std::vector<s2amdBody> bodies;
	std::vector<s2amdContact> contacts;
	std::vector<s2amdPairState> pairs;
	std::vector<s2amdShape> shapes;
	std::vector<float> origins;
	int live = 0;	// contact slots in use as built; the spare ones follow
	int boxes = 0;	// bodies of the pyramid, the ground included; free bodies ("balls") follow
};

static s2amdContact freeContact()
{
	s2amdContact c{};
	c.bodyA = c.bodyB = -1, c.constraintIndex = -1;
	return c;
}

static s2amdContact touching(int a, int b, int points)
{
	s2amdContact c{};
	c.bodyA = a, c.bodyB = b, c.pointCount = points, c.constraintIndex = -1;
	c.normal[0] = 0.0f, c.normal[1] = 1.0f, c.friction = 0.6f;
	for (int i = 0; i < 2; ++i)
	{
		c.points[i].localAnchorA[0] = i == 0 ? 0.5f : -0.5f, c.points[i].localAnchorA[1] = 0.5f;
		c.points[i].localAnchorB[0] = i == 0 ? 0.5f : -0.5f, c.points[i].localAnchorB[1] = -0.5f;
		c.points[i].separation = -0.005f;
	}
	return c;
}

// a pyramid of `base` boxes at the bottom on a static ground (body 0), `balls` free boxes beside it, `spare` free contact slots
static Scene pyramid(int base, int spare, int balls)
{
	Scene w;
	auto body = [&](float x, float y, bool dynamic) {
		s2amdBody b{};
		b.position[0] = x, b.position[1] = y, b.rot[0] = 0.0f, b.rot[1] = 1.0f, b.gravityScale = 1.0f;
		b.type = dynamic ? S2AMD_BODY_DYNAMIC : S2AMD_BODY_STATIC;
		if (dynamic)
		{
			b.mass = 1.0f, b.invMass = 1.0f, b.I = 1.0f / 6.0f, b.invI = 6.0f;
		}
		w.bodies.push_back(b);
		return (int)w.bodies.size() - 1;
	};
	body(0.0f, -1.0f, false);
	std::vector<std::vector<int>> index((size_t)base, std::vector<int>((size_t)base, -1));
	for (int i = 0; i < base; ++i)
	{
		for (int j = i; j < base; ++j)
		{
			const int bi = body(0.5f * (float)(i + 1) + (float)(j - i) - 0.5f * (float)base, (float)i + 0.5f, true);
			index[(size_t)i][(size_t)j] = bi;
			if (i == 0)
			{
				w.contacts.push_back(touching(0, bi, 2));
			}
			else
			{
				w.contacts.push_back(touching(index[(size_t)i - 1][(size_t)j], bi, 2));
				w.contacts.push_back(touching(index[(size_t)i - 1][(size_t)j - 1], bi, 2));
			}
			if (j > i)
			{
				w.contacts.push_back(touching(index[(size_t)i][(size_t)j - 1], bi, 2));
			}
		}
	}
	w.boxes = (int)w.bodies.size();
	for (int i = 0; i < balls; ++i)
	{
		body((float)(base + 40 + 3 * i), 5.0f, true);
	}
	w.live = (int)w.contacts.size();
	w.contacts.resize((size_t)(w.live + spare), freeContact());
	for (const s2amdContact& c : w.contacts)
	{
		s2amdPairState p{};
		p.shapeA = c.bodyA, p.shapeB = c.bodyB; // one shape per body, same index
		w.pairs.push_back(p);
	}
	for (size_t i = 0; i < w.bodies.size(); ++i)
	{
		const s2amdBody& b = w.bodies[i];
		const float hx = i == 0 ? 100.0f : 0.5f, hy = i == 0 ? 1.0f : 0.5f;
		s2amdShape sh{};
		sh.body = (int)i, sh.type = S2AMD_SHAPE_POLYGON, sh.categoryBits = 1, sh.maskBits = 0xffffffffu, sh.proxyKey = ((int)i << 4) | b.type, sh.count = 4;
		const float v[4][2] = {{-hx, -hy}, {hx, -hy}, {hx, hy}, {-hx, hy}}, n[4][2] = {{0.0f, -1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}};
		for (int k = 0; k < 4; ++k)
		{
			sh.vertices[k][0] = v[k][0], sh.vertices[k][1] = v[k][1], sh.normals[k][0] = n[k][0], sh.normals[k][1] = n[k][1];
		}
		sh.aabb[0] = b.position[0] - hx, sh.aabb[1] = b.position[1] - hy, sh.aabb[2] = b.position[0] + hx, sh.aabb[3] = b.position[1] + hy;
		sh.fatAABB[0] = sh.aabb[0] - 0.1f, sh.fatAABB[1] = sh.aabb[1] - 0.1f, sh.fatAABB[2] = sh.aabb[2] + 0.1f, sh.fatAABB[3] = sh.aabb[3] + 0.1f;
		w.shapes.push_back(sh);
		w.origins.push_back(b.position[0]), w.origins.push_back(b.position[1]);
	}
	return w;
}

// `count` contacts of the pile are turned to lean on one box in its middle: a hub (more than S2_HUB_DEGREE potential constraints)
static int makeHub(Scene& w, int count)
{
	const int hub = w.boxes / 2;
	std::vector<int> others;
	for (int i = 0; i < w.live; ++i)
	{
		if (w.contacts[(size_t)i].bodyA != hub && w.contacts[(size_t)i].bodyB != hub && w.contacts[(size_t)i].bodyA != 0)
		{
			others.push_back(i);
		}
	}
	const int stride = std::max(1, (int)others.size() / count);
	std::set<int> leaning;
	for (int n = 0, i = 0; n < count && i < (int)others.size(); i += stride)
	{
		s2amdContact& c = w.contacts[(size_t)others[(size_t)i]];
		if (leaning.insert(c.bodyA).second)
		{
			c.bodyB = hub;
			w.pairs[(size_t)others[(size_t)i]].shapeB = hub;
			n += 1;
		}
	}
	return hub;
}

// ---- the script: per round, the slots that change ----
struct Change
{
	int slot, a, b, points; // a < 0: destroyed
};
enum Kind
{
	NEIGHBOURS, // boxes two hops apart in the contact graph
	HUB,		// a box and the hub
	BALLS,		// a free body and a box, then boxes next to that one
};

struct Rng
{
	uint32_t x;
	int below(int n)
	{
		x = x * 1664525u + 1013904223u;
		return (int)((x >> 8) % (uint32_t)n);
	}
};

static std::vector<std::vector<Change>> script(const Scene& w, Kind kind, int rounds, int hub, uint32_t seed)
{
	Rng rng{seed};
	std::vector<s2amdContact> now = w.contacts;
	std::vector<std::vector<int>> nbrs(w.bodies.size());
	std::set<std::pair<int, int>> joined;
	for (int i = 0; i < w.live; ++i)
	{
		const int a = now[(size_t)i].bodyA, b = now[(size_t)i].bodyB;
		nbrs[(size_t)a].push_back(b), nbrs[(size_t)b].push_back(a);
		joined.insert({std::min(a, b), std::max(a, b)});
	}
	std::vector<int> spare, mine;
	for (int i = (int)now.size() - 1; i >= w.live; --i)
	{
		spare.push_back(i); // (pop_back: the lowest)
	}
	std::vector<int> lastBox(w.bodies.size(), -1); // BALLS: the box a ball touched last
	std::vector<std::vector<Change>> out;
	int nextOriginal = 3;
	for (int r = 0; r < rounds; ++r)
	{
		std::vector<Change> changes;
		std::set<int> touched;
		auto put = [&](int slot, int a, int b, int points) {
			now[(size_t)slot] = a < 0 ? freeContact() : touching(a, b, points);
			changes.push_back(Change{slot, a, b, points});
			touched.insert(slot);
		};
		// what the churn made earlier: manifolds gain and lose their points, contacts are destroyed
		for (size_t m = 0; m < mine.size();)
		{
			const int slot = mine[m], what = rng.below(8);
			const s2amdContact c = now[(size_t)slot];
			if (what < 3)
			{
				put(slot, c.bodyA, c.bodyB, c.pointCount == 0 ? 1 + rng.below(2) : what == 0 ? 0 : 3 - c.pointCount);
			}
			else if (what == 3)
			{
				joined.erase({std::min(c.bodyA, c.bodyB), std::max(c.bodyA, c.bodyB)});
				put(slot, -1, -1, 0);
				spare.push_back(slot);
				std::sort(spare.begin(), spare.end(), std::greater<int>());
				mine.erase(mine.begin() + (long)m);
				continue;
			}
			m += 1;
		}
		// a contact of the pile as built is destroyed every third round: its slot is the lowest free one from then on
		if (r % 3 == 2 && nextOriginal < w.live)
		{
			const s2amdContact c = now[(size_t)nextOriginal];
			if (c.bodyA > 0 && c.bodyB != hub && c.bodyA != hub)
			{
				joined.erase({std::min(c.bodyA, c.bodyB), std::max(c.bodyA, c.bodyB)});
				put(nextOriginal, -1, -1, 0);
				spare.push_back(nextOriginal);
				std::sort(spare.begin(), spare.end(), std::greater<int>());
			}
			nextOriginal += 7;
		}
		const int creations = 1 + rng.below(4);
		for (int n = 0; n < creations && !spare.empty(); ++n)
		{
			int a = -1, b = -1;
			if (kind == NEIGHBOURS)
			{
				a = 1 + rng.below(w.boxes - 1);
				const int mid = nbrs[(size_t)a][(size_t)rng.below((int)nbrs[(size_t)a].size())];
				b = nbrs[(size_t)mid][(size_t)rng.below((int)nbrs[(size_t)mid].size())];
			}
			else if (kind == HUB)
			{
				a = 1 + rng.below(w.boxes - 1), b = hub;
			}
			else
			{
				a = w.boxes + rng.below((int)w.bodies.size() - w.boxes);
				const int last = lastBox[(size_t)a];
				b = last < 0 ? 1 + rng.below(w.boxes - 1) : nbrs[(size_t)last][(size_t)rng.below((int)nbrs[(size_t)last].size())];
			}
			if (a == b || a <= 0 || b <= 0 || joined.count({std::min(a, b), std::max(a, b)}) != 0 || touched.count(spare.back()) != 0)
			{
				continue;
			}
			if (kind == BALLS)
			{
				lastBox[(size_t)a] = b;
			}
			if (rng.below(2) == 1)
			{
				std::swap(a, b);
			}
			joined.insert({std::min(a, b), std::max(a, b)});
			const int slot = spare.back();
			spare.pop_back();
			put(slot, a, b, rng.below(3) == 0 ? 2 : 0);
			mine.push_back(slot);
		}
		out.push_back(changes);
	}
	return out;
}

// ---- the block printed after every call ----
template <typename T> static unsigned hashOf(const std::vector<T>& v)
{
	return (unsigned)fnv(1469598103934665603ull, v.data(), v.size() * sizeof(T)); // (the low half of the FNV hash)
}

static void playPatches()
{
	SolverStructure& t = *solver;
	if (t.dPatches.p == nullptr)
	{
		return;
	}
	const uint4* list = (const uint4*)t.dPatches.p;
	const size_t capacity = t.dPatches.bytes / sizeof(uint4);
	size_t n = 0;
	while (n < capacity && (list[n].x != 0u || list[n].y != 0u))
	{
		n += 1;
	}
	if (n > 0)
	{
		printf("PATCHES %zu\n", n);
	}
	for (size_t i = 0; i < n; ++i)
	{
		const uintptr_t addr = (uintptr_t)(((unsigned long long)list[i].y << 32) | list[i].x);
		const char* name = "?";
		size_t word = 0;
		int at = 0;
		forEachStructureBuf(t, [&](DevBuf& b) {
			if (b.p != nullptr && addr >= (uintptr_t)b.p && addr + 4 <= (uintptr_t)b.p + b.bytes)
			{
				name = bufNames[at], word = (addr - (uintptr_t)b.p) / 4;
			}
			at += 1;
		});
		printf("%s%s[%zu]=%d", i % 6 == 0 ? (i == 0 ? "  " : "\n  ") : " ", name, word, (int)list[i].z); // (six to a line)
		if (name[0] != '?')
		{
			*(uint32_t*)addr = list[i].z; // what patchWordsKernel does
		}
		else
		{
			failures += 1;
		}
	}
	if (n > 0)
	{
		printf("\n");
	}
	memset(t.dPatches.p, 0, t.dPatches.bytes); // (the next call's list ends at the first zero address)
}

// (a line of the block that says what it said after the call before is not printed again; `said` is cleared where a scene begins)
static std::string said[9];
static void say(int line, const char* format, ...)
{
	char text[320];
	va_list args;
	va_start(args, format);
	vsnprintf(text, sizeof text, format, args);
	va_end(args);
	if (said[line] != text)
	{
		said[line] = text;
		printf("%s\n", text);
	}
}

static void answered(const char* call, int rc)
{
	const s2amdSolver* s = solver;
	printf("-- %s\n", call);
	say(0, "RC %d%s%s", rc, rc ? " " : "", rc ? s2amd_last_error() : "");
	say(1, "builds %llu placed %ld dirty %d (%s) layout %llu", (unsigned long long)s->structureGeneration, s->placedTotal, s->structureDirty ? 1 : 0,
		s->structureDirty ? s->dirtyReason : "", (unsigned long long)s->layoutGeneration);
	say(6, "age %d", s->graphAge);
	say(2, "patience strips %d groups %d, tail slack %d, slack shift %d, spare colours %d, builds by a worker: requested %d adopted %d", s->stripPatienceNow,
		s->groupPatienceNow, s->tailSlackShift, s->slackShift, s->spareColours, s->asyncRequested, s->asyncAdopted);
	say(7, "slack positions %d, watched %d", s->slackPositions, s->watchedCount);
	say(3, "inc valid %d inserted %ld removed %ld fallbacks %ld tail %ld", s->inc.valid ? 1 : 0, s->inc.inserted, s->inc.removed, s->inc.fallbacks, s->inc.tailPlaced);
	say(8, "strips valid %d placed %ld rounds %ld adopted %ld seam bodies %ld overflow %d", s->stripInc.valid ? 1 : 0, s->stripInc.placed, s->stripInc.roundsOpened,
		s->stripInc.adopted, s->stripInc.seamBodiesAdded, s->stripInc.overflowUsed);
	say(4, "order %08x local %08x pos %08x strip pos %08x", hashOf(s->contacts.order), hashOf(s->contacts.local), hashOf(s->inc.positionOfSlot),
		hashOf(s->stripInc.positionOfSlot));
	say(5, "A %08x B %08x edge %08x dead %08x watched %08x", hashOf(s->hContactA), hashOf(s->hContactB), hashOf(s->hContactEdge), hashOf(s->hContactDead),
		hashOf(s->hContactWatched));
	playPatches();
	fflush(stdout);
}

static int step(int route, const s2amdStepParams& params)
{
	trace(false);
	const int rc = route == 0 ? s2amd_step_resident(solver, &params) : s2amd_world_step(solver, &params, nullptr);
	trace(true);
	return rc;
}

struct Option
{
	const char* key;
	int value;
};

static void run(const char* name, const Scene& w, Kind kind, int hub, int solverType, int rounds, uint32_t seed, const std::vector<Option>& options, int firstRoute = 0)
{
	const std::vector<std::vector<Change>> rounds_ = script(w, kind, rounds, hub, seed);
	s2amdStepParams params{};
	params.solverType = solverType, params.dt = 1.0f / 60.0f, params.velIters = 4, params.posIters = 2, params.warmStart = 1, params.gravity[1] = -10.0f;
	for (int route = firstRoute; route < 2; ++route)
	{
		printf("== %s, %s: %d bodies, %d contact slots, %d in use\n", name, route == 0 ? "host arrays" : "resident world", (int)w.bodies.size(), (int)w.contacts.size(), w.live);
		for (std::string& line : said)
		{
			line.clear();
		}
		trace(false);
		EXPECT(s2amd_create(0, &solver), S2AMD_OK);
		trace(true);
		if (solver == nullptr)
		{
			return;
		}
		EXPECT(s2amd_set_option(solver, "async_build", 0), S2AMD_OK); // (no worker threads: what is printed must not depend on their timing)
		for (const Option& o : options)
		{
			EXPECT(s2amd_set_option(solver, o.key, o.value), S2AMD_OK);
		}
		std::vector<s2amdContact> contacts = w.contacts;
		std::vector<s2amdPairState> pairs = w.pairs;
		char label[96];
		if (route == 0)
		{
			answered("upload", s2amd_upload(solver, w.bodies.data(), (int32_t)w.bodies.size(), contacts.data(), (int32_t)contacts.size(), nullptr, 0));
			answered("step_resident", step(route, params));
		}
		else
		{
			answered("world_upload", s2amd_world_upload(solver, w.bodies.data(), (int32_t)w.bodies.size(), contacts.data(), (int32_t)contacts.size(), nullptr, 0, w.shapes.data(),
														(int32_t)w.shapes.size(), pairs.data(), w.origins.data()));
			answered("world_step", step(route, params));
		}
		for (size_t r = 0; r < rounds_.size(); ++r)
		{
			std::vector<int32_t> slots;
			std::vector<s2amdContact> cs;
			std::vector<s2amdPairState> ps;
			for (const Change& ch : rounds_[r])
			{
				contacts[(size_t)ch.slot] = ch.a < 0 ? freeContact() : touching(ch.a, ch.b, ch.points);
				s2amdPairState p{};
				p.shapeA = ch.a, p.shapeB = ch.b;
				pairs[(size_t)ch.slot] = p;
				slots.push_back(ch.slot), cs.push_back(contacts[(size_t)ch.slot]), ps.push_back(p);
			}
			if (route == 0)
			{
				snprintf(label, sizeof label, "round %zu: upload, %zu slots changed", r, slots.size());
				answered(label, s2amd_upload(solver, w.bodies.data(), (int32_t)w.bodies.size(), contacts.data(), (int32_t)contacts.size(), nullptr, 0));
				answered("step_resident", step(route, params));
			}
			else
			{
				if (!slots.empty())
				{
					snprintf(label, sizeof label, "round %zu: world_set_contacts, %zu slots", r, slots.size());
					answered(label, s2amd_world_set_contacts(solver, slots.data(), (int32_t)slots.size(), cs.data(), ps.data()));
				}
				answered("world_step", step(route, params));
			}
		}
		trace(false);
		s2amd_destroy(solver);
		trace(true);
		solver = nullptr;
	}
}

int main()
{
	const std::vector<Option> batches{{"groups", 0}, {"strips", 0}, {"incremental", 1}};
	const std::vector<Option> strips{{"max_group_bodies", 48}, {"strip_bodies", 12}, {"strip_min_bodies", 0}, {"strip_patience", 0}};
	// colour batches of the global part (a base of 20: below that the colours are small enough to end up in the tail); the contact that
	// finds no colour free on its bodies rebuilds, and the spare colours of that build take the next one
	run("colour batches", pyramid(20, 24, 0), NEIGHBOURS, -1, s2amd_solverTGS_Soft, 7, 1u, batches);
	// a box inside the pile uses every colour: contact after contact on that one box
	{
		const Scene w = pyramid(20, 24, 0);
		run("no free colour", w, HUB, w.boxes / 2, s2amd_solverTGS_Soft, 5, 2u, batches);
	}
	// a hub: its manifolds are watched, and the ones that gain points take positions of the sequential tail (host arrays: the defer-then-flip
	// path; the world route learns of flips from stage 3's counters, which only the device writes)
	{
		Scene w = pyramid(12, 40, 0);
		const int hub = makeHub(w, 20);
		run("sequential tail", w, HUB, hub, s2amd_solverPGS_Soft, 7, 3u, batches);
	}
	// a structure built for s2Solve_Jacobi: any free position does
	run("jacobi", pyramid(10, 24, 0), NEIGHBOURS, -1, s2amd_solverJacobi, 5, 4u, batches);
	// strips under a soft solver: free positions of strip and seam rounds, seams that come to carry a body, spare rounds that open ...
	run("strips", pyramid(14, 48, 0), NEIGHBOURS, -1, s2amd_solverTGS_Soft, 8, 5u, strips);
	// ... and bodies without constraints that join the pile: adopted by the strip they touch first
	run("strips, joining bodies", pyramid(14, 48, 6), BALLS, -1, s2amd_solverTGS_Soft, 8, 6u, strips);
	// ... and under the op interpreter, which takes free positions of the rounds as built and nothing else
	run("strips, op interpreter", pyramid(14, 48, 0), NEIGHBOURS, -1, s2amd_solverPGS, 7, 7u, strips);
	// ... and built by a worker thread on a copy of the solver, adopted a fixed number of steps after the request (the caller waits for a
	// worker that is not done): the contacts created and destroyed meanwhile are replayed on the copy, the watched ones that gained points
	// take their places there.  No call trace: the worker's calls would fall between the caller's wherever its timing puts them.
	traced = false;
	trace(false);
	run("strips, built by a worker", pyramid(14, 48, 0), NEIGHBOURS, -1, s2amd_solverTGS_Soft, 12, 8u,
		{{"max_group_bodies", 48}, {"strip_bodies", 12}, {"strip_min_bodies", 0}, {"strip_patience", 1}, {"async_build", 2}, {"async_build_delay", 3}}, 1); // (the world route alone has workers)
	if (failures == 0)
	{
		printf("PLACEMENT MAIN OK\n");
	}
	return failures == 0 ? 0 : 1;
}
