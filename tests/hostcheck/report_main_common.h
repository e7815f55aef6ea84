// TEST INFRASTRUCTURE.  What the stand-alone host-check programs of the reports share (shape_report_main.cpp, body_report_main.cpp,
// step_metrics_main.cpp, contact_joint_report_main.cpp): the EXPECT check, a small world and its upload, and exact-size heap buffers.
#pragma once

#include "solver_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;

#define EXPECT(expr, want)                                                                                   \
	do                                                                                                       \
	{                                                                                                        \
		const int got_ = (expr);                                                                             \
		if (got_ != (want))                                                                                  \
		{                                                                                                    \
			printf("line %d: %s = %d, expected %d (%s)\n", __LINE__, #expr, got_, (int)(want), s2amd_last_error()); \
			failures += 1;                                                                                   \
		}                                                                                                    \
	} while (0)

struct World
{
	std::vector<s2amdBody> bodies;
	std::vector<s2amdContact> contacts;
	std::vector<s2amdJoint> joints;
	std::vector<s2amdShape> shapes;
	std::vector<s2amdPairState> pairs;
	std::vector<float> origins;
};

// body 0 static with a ground box; `count` unit-mass bodies above it, one small box each that collides with nothing; every seventh
// shape slot free
static World makeWorld(int count)
{
	World w;
	w.bodies.assign((size_t)count + 1, s2amdBody{});
	w.origins.assign(2 * ((size_t)count + 1), 0.0f);
	for (size_t i = 0; i < w.bodies.size(); ++i)
	{
		s2amdBody& b = w.bodies[i];
		b.rot[0] = 0.0f, b.rot[1] = 1.0f;
		b.gravityScale = 1.0f;
		b.type = i == 0 ? S2AMD_BODY_STATIC : S2AMD_BODY_DYNAMIC;
		if (i > 0)
		{
			b.position[0] = 0.5f * (float)(i % 40), b.position[1] = 1.0f + 0.5f * (float)(i / 40);
			b.mass = 1.0f, b.invMass = 1.0f, b.I = 0.5f, b.invI = 2.0f;
		}
		w.origins[2 * i] = b.position[0], w.origins[2 * i + 1] = b.position[1];
	}
	const int slots = count + 1 + (count + 1) / 6;
	w.shapes.assign((size_t)slots, s2amdShape{});
	int body = 0;
	for (int k = 0; k < slots; ++k)
	{
		s2amdShape& sh = w.shapes[(size_t)k];
		if (k % 7 == 6 || body > count)
		{
			sh.type = S2AMD_SHAPE_FREE, sh.body = -1;
			continue;
		}
		const float h = body == 0 ? 10.0f : 0.125f;
		const float px = w.bodies[(size_t)body].position[0], py = w.bodies[(size_t)body].position[1];
		sh.body = body, sh.type = S2AMD_SHAPE_POLYGON;
		sh.categoryBits = 1, sh.maskBits = 0;
		sh.proxyKey = (k << 4) | w.bodies[(size_t)body].type;
		sh.count = 4;
		const float v[4][2] = {{-h, -0.125f}, {h, -0.125f}, {h, 0.125f}, {-h, 0.125f}};
		const float n[4][2] = {{0.0f, -1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}};
		for (int i = 0; i < 4; ++i)
		{
			sh.vertices[i][0] = v[i][0], sh.vertices[i][1] = v[i][1];
			sh.normals[i][0] = n[i][0], sh.normals[i][1] = n[i][1];
		}
		sh.aabb[0] = px - h, sh.aabb[1] = py - 0.125f, sh.aabb[2] = px + h, sh.aabb[3] = py + 0.125f;
		sh.fatAABB[0] = sh.aabb[0] - 0.1f, sh.fatAABB[1] = sh.aabb[1] - 0.1f, sh.fatAABB[2] = sh.aabb[2] + 0.1f, sh.fatAABB[3] = sh.aabb[3] + 0.1f;
		body += 1;
	}
	w.contacts.assign(4, s2amdContact{});
	w.pairs.assign(4, s2amdPairState{});
	for (size_t i = 0; i < 4; ++i)
	{
		w.contacts[i].constraintIndex = -1;
		w.pairs[i].shapeA = w.pairs[i].shapeB = -1;
	}
	return w;
}

static int upload(s2amdSolver* s, const World& w)
{
	return s2amd_world_upload(s, w.bodies.data(), (int32_t)w.bodies.size(), w.contacts.data(), (int32_t)w.contacts.size(), w.joints.data(), (int32_t)w.joints.size(),
							  w.shapes.data(), (int32_t)w.shapes.size(), w.pairs.data(), w.origins.data());
}

// a heap block of exactly n elements (n == 0: a null pointer)
template <typename T> struct Exact
{
	T* p;
	explicit Exact(int n) : p(n > 0 ? (T*)malloc((size_t)n * sizeof(T)) : nullptr) {}
	~Exact() { free(p); }
};
