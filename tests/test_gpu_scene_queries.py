"""Scene queries on the resident world (s2amd_world_ray_cast / _point_probe / _query_boxes; solver2d_amd/csrc/scene_query.hip) against
their statement (tests/scene_query_ref.py: numpy around the reference's own s2RayCast* and s2PointIn*): every answer equal byte for byte.
The fixture tests read the statement's answers from tests/golden/scene_query/*.npz and need no reference library."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import resident, scene_query_ref as ref, scene_query_world as sq, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, upload

pytestmark = pytest.mark.gpu

STEPS = 12


def ask(s, rays, probes, boxes):
    """The three calls through the hip.py methods -> the five result arrays in sq.RESULT_KEYS order"""
    hits = s.world_ray_cast(rays)
    probe_offsets, probe_shapes = s.world_point_probe(probes)
    box_offsets, box_shapes = s.world_query_boxes(boxes)
    return dict(zip(sq.RESULT_KEYS, (hits, probe_offsets, probe_shapes, box_offsets, box_shapes)))


def raw_list_call(s, fn, queries, capacity):
    """One call through the C ABI -> (rc, offsets, shapes, total); the arrays start as -7 so that what the call wrote shows"""
    offsets = np.full(len(queries) + 1, -7, dtype=np.int32)
    shapes = np.full(max(capacity, 1), -7, dtype=np.int32)
    total = ctypes.c_int32(-7)
    rc = fn(s._h, wire.as_ptr(queries), len(queries), wire.as_ptr(offsets), wire.as_ptr(shapes), capacity, ctypes.byref(total))
    return rc, offsets, shapes, total.value


def ask_raw(s, rays, probes, boxes):
    """... and through the C ABI itself, with exactly the capacity the statement's answer needs"""
    L = s._L
    hits = np.full(len(rays), -7, dtype=np.int32).repeat(8).view(wire.ray_hit_dtype)
    assert L.s2amd_world_ray_cast(s._h, wire.as_ptr(rays), len(rays), wire.as_ptr(hits)) == 0
    out = {"hits": hits}
    for key, fn, queries in (("probe", L.s2amd_world_point_probe, probes), ("box", L.s2amd_world_query_boxes, boxes)):
        rc, offsets, _, total = raw_list_call(s, fn, queries, 0)
        assert rc == (E_CAPACITY if total > 0 else 0) and total == offsets[-1]
        rc, offsets, shapes, total = raw_list_call(s, fn, queries, total)
        assert rc == 0
        out[key + "_offsets"], out[key + "_shapes"] = offsets, shapes[:total]
    return out


def assert_equal_bytes(got, want, what):
    resident.assert_equal_bytes(got, want, what, sq.RESULT_KEYS)


@pytest.mark.parametrize("name", sq.FIXTURES)
def test_fixtures_byte_equal(name):
    fx = sq.load_fixture(name)
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask_raw(s, fx["rays"], fx["probes"], fx["boxes"]), fx, name + " through the C ABI")
        assert_equal_bytes(ask(s, fx["rays"], fx["probes"], fx["boxes"]), fx, name + " through hip.py")


def in_chunks(s, fx, size):
    parts = [ask(s, fx["rays"][i:i + size], fx["probes"][i:i + size], fx["boxes"][i:i + size])
             for i in range(0, max(len(fx["rays"]), len(fx["probes"]), len(fx["boxes"])), size)]
    out = {"hits": np.concatenate([p["hits"] for p in parts])}
    for key in ("probe", "box"):
        out[key + "_shapes"] = np.concatenate([p[key + "_shapes"] for p in parts])
        counts = np.concatenate([np.diff(p[key + "_offsets"]) for p in parts])
        out[key + "_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


@pytest.mark.parametrize("size", [1, 100])
def test_a_batch_in_chunks_answers_as_the_whole(size):
    fx = sq.load_fixture("synthetic")
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(in_chunks(s, fx, size), fx, "chunks of %d" % size)


def test_a_thousand_rays_cross_the_query_chunk():
    """More rays than a workgroup stages at once, on the two-tile world: every copy of a ray answers as the fixture's one"""
    fx = sq.load_fixture("pyramid30")
    order = np.arange(1000) % len(fx["rays"])
    order[500:] = order[500:][::-1].copy()
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        hits = s.world_ray_cast(fx["rays"][order])
        assert hits.tobytes() == fx["hits"][order].tobytes()
        probes = np.tile(fx["probes"], 3)[:700]
        offsets, shapes = s.world_point_probe(probes)
        counts = np.diff(fx["probe_offsets"])
        assert np.array_equal(np.diff(offsets), np.tile(counts, 3)[:700])
        assert shapes.tobytes() == np.concatenate([fx["probe_shapes"]] * 3)[:offsets[-1]].tobytes()


def test_the_fast_library_answers_the_same_bytes():
    fx = sq.load_fixture("zoo")
    with hip.Solver(0, fast=True) as s:
        assert s._L.s2amd_build_flags().decode() == "fp-contract=fast"
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask(s, fx["rays"], fx["probes"], fx["boxes"]), fx, "libs2amd_fast.so")


def stepping_batch(world):
    return sq.make_batch(world, (256, 128, 32), 5, sq.special_cases()[:3])


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
def test_queries_follow_the_world_as_the_device_steps_it():
    """12 steps of the synthetic world on the device; after the 1st, 6th and 12th the queries equal the statement applied to what
    s2amd_world_download returns."""
    world = sq.synthetic_world()
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    rays, probes, boxes = stepping_batch(world)
    with hip.Solver(0) as s:
        upload(s, world)
        for step in range(STEPS):
            s.world_step(params)
            if step in (0, 5, STEPS - 1):
                got = ask(s, rays, probes, boxes)
                now, _ = download(s, world)
                assert_equal_bytes(got, sq.expected(now, rays, probes, boxes), "after step %d" % step)
                if step == 0:  # (the rays were aimed at the shapes where they started)
                    assert 2 * int((got["hits"]["shape"] >= 0).sum()) >= len(rays)
        assert now["bodies"]["position"].tobytes() != world["bodies"]["position"].tobytes()


def test_queries_between_steps_change_nothing():
    """Two solvers in lockstep on the synthetic world, one asked all three queries (twice) between steps: the same world bytes and
    stage-3 status after every step, the shape report still answers, and asking twice answers the same."""
    world = sq.synthetic_world()
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    rays, probes, boxes = stepping_batch(world)
    with hip.Solver(0) as asked, hip.Solver(0) as quiet:
        for s in (asked, quiet):
            s.world_set_shape_report(wire.SHAPE_REPORT_ALL)
            upload(s, world)
        first = ask(asked, rays, probes, boxes)
        for step in range(STEPS):
            asked.world_step(params), quiet.world_step(params)
            a = ask(asked, rays, probes, boxes)
            assert_equal_bytes(ask(asked, rays, probes, boxes), a, "step %d, asked again" % step)
            assert asked.world_shape_summary().tobytes() == quiet.world_shape_summary().tobytes()
            assert asked.world_shape_draws().tobytes() == quiet.world_shape_draws().tobytes()
            (wa, sta), (wb, stb) = download(asked, world), download(quiet, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert a["hits"].tobytes() != first["hits"].tobytes()  # (the world moved under the rays)


def test_errors():
    fx = sq.load_fixture("zoo")
    rays, probes, boxes = fx["rays"][:8].copy(), fx["probes"][:8].copy(), fx["boxes"][:8].copy()
    with hip.Solver(0) as s:
        L = s._L
        lists = ((L.s2amd_world_point_probe, probes, "probe"), (L.s2amd_world_query_boxes, boxes, "box"))
        # no resident world
        hits = np.full(8, -7, dtype=np.int32).repeat(8).view(wire.ray_hit_dtype)
        untouched = hits.tobytes()
        assert L.s2amd_world_ray_cast(s._h, wire.as_ptr(rays), 8, wire.as_ptr(hits)) == E_STATE
        for fn, queries, _ in lists:
            assert raw_list_call(s, fn, queries, 64)[0] == E_STATE
        for method, queries in ((s.world_ray_cast, rays), (s.world_point_probe, probes), (s.world_query_boxes, boxes)):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                method(queries)
        upload(s, sq.fixture_world(fx))
        # a ray that fails s2IsValidRay refuses the whole call before anything is enqueued
        for field, index, value in (("p1", 0, np.nan), ("p2", 1, np.nan), ("p2", 0, np.inf), ("maxFraction", None, -0.5), ("maxFraction", None, np.nan),
                                    ("maxFraction", None, 100000.0)):
            bad = rays.copy()
            if index is None:
                bad[field][5] = value
            else:
                bad[field][5, index] = value
            assert L.s2amd_world_ray_cast(s._h, wire.as_ptr(bad), 8, wire.as_ptr(hits)) == E_INVALID, (field, value)
            assert hits.tobytes() == untouched
        assert L.s2amd_world_ray_cast(s._h, wire.as_ptr(rays), -1, wire.as_ptr(hits)) == E_INVALID
        assert L.s2amd_world_ray_cast(s._h, wire.as_ptr(rays), 8, None) == E_INVALID
        # count == 0 touches nothing
        assert L.s2amd_world_ray_cast(s._h, None, 0, None) == 0 and hits.tobytes() == untouched
        for fn, queries, _ in lists:
            rc, offsets, shapes, total = raw_list_call(s, fn, queries[:0], 4)
            assert rc == 0 and offsets.tolist() == [-7] and shapes.tolist() == [-7] * 4 and total == -7
        # the ask-again round trip: offsets and the total are filled, the hit array is untouched
        for fn, queries, key in lists:
            want_offsets = fx[key + "_offsets"][:9]
            want_shapes = fx[key + "_shapes"][:want_offsets[-1]]
            assert want_offsets[-1] >= 2
            rc, offsets, shapes, total = raw_list_call(s, fn, queries, int(want_offsets[-1]) - 1)
            assert rc == E_CAPACITY and total == want_offsets[-1] and np.array_equal(offsets, want_offsets)
            assert (shapes == -7).all()
            rc, offsets, shapes, total = raw_list_call(s, fn, queries, total)
            assert rc == 0 and np.array_equal(offsets, want_offsets) and np.array_equal(shapes[:total], want_shapes)
            assert raw_list_call(s, fn, queries, -1)[0] == E_INVALID
        # hip.py asks again by itself
        offsets, shapes = s.world_query_boxes(fx["boxes"], expected=1)
        assert offsets.tobytes() == fx["box_offsets"].tobytes() and shapes.tobytes() == fx["box_shapes"].tobytes()
        assert s.world_ray_cast(rays).tobytes() == fx["hits"][:8].tobytes()
