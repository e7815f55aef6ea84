"""Proximity queries on the resident world (s2amd_world_closest_shape / _shapes_in_range; solver2d_amd/csrc/proximity_query.hip) against
their statement (tests/proximity_ref.py: numpy around the reference's own s2ShapeDistance): every answer equal byte for byte.  The
fixture tests read the statement's answers from tests/golden/proximity/*.npz and need no reference library."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import proximity_ref as ref, proximity_world as pw, resident, scene_query_world as sq, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, upload

pytestmark = pytest.mark.gpu

STEPS = 12


def ask(s, queries):
    """Both calls through the hip.py methods -> the four result arrays under pw.RESULT_KEYS; the lists asked with and without distances"""
    offsets, shapes, distances = s.world_shapes_in_range(queries, distances=True)
    plain_offsets, plain_shapes = s.world_shapes_in_range(queries)
    assert plain_offsets.tobytes() == offsets.tobytes() and plain_shapes.tobytes() == shapes.tobytes()
    return dict(zip(pw.RESULT_KEYS, (s.world_closest_shape(queries), offsets, shapes, distances)))


def new_hits(n):
    return np.full(n, -7, dtype=np.int32).repeat(8).view(wire.proximity_hit_dtype)


def raw_range_call(s, queries, capacity, with_distances=True):
    """One s2amd_world_shapes_in_range through the C ABI -> (rc, offsets, shapes, distances, total); the arrays start as -7 so that
    what the call wrote shows"""
    offsets = np.full(len(queries) + 1, -7, dtype=np.int32)
    shapes = np.full(max(capacity, 1), -7, dtype=np.int32)
    distances = np.full(max(capacity, 1), -7, dtype=np.float32)
    total = ctypes.c_int32(-7)
    rc = s._L.s2amd_world_shapes_in_range(s._h, wire.as_ptr(queries), len(queries), wire.as_ptr(offsets), wire.as_ptr(shapes),
                                          wire.as_ptr(distances) if with_distances else None, capacity, ctypes.byref(total))
    return rc, offsets, shapes, distances, total.value


def ask_raw(s, queries):
    """... and through the C ABI itself, with exactly the capacity the answer needs, with and without distances"""
    hits = new_hits(len(queries))
    assert s._L.s2amd_world_closest_shape(s._h, wire.as_ptr(queries), len(queries), wire.as_ptr(hits)) == 0
    rc, offsets, _, _, total = raw_range_call(s, queries, 0)
    assert rc == (E_CAPACITY if total > 0 else 0) and total == offsets[-1]
    rc, offsets, shapes, distances, total = raw_range_call(s, queries, total)
    assert rc == 0
    rc, plain_offsets, plain_shapes, untouched, plain_total = raw_range_call(s, queries, total, with_distances=False)
    assert rc == 0 and plain_total == total and (untouched == -7).all()
    assert plain_offsets.tobytes() == offsets.tobytes() and plain_shapes.tobytes() == shapes.tobytes()
    return dict(zip(pw.RESULT_KEYS, (hits, offsets, shapes[:total], distances[:total])))


def assert_equal_bytes(got, want, what):
    resident.assert_equal_bytes(got, want, what, pw.RESULT_KEYS)


@pytest.mark.parametrize("name", pw.FIXTURES)
def test_fixtures_byte_equal(name):
    fx = pw.load_fixture(name)
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask_raw(s, fx["queries"]), fx, name + " through the C ABI")
        assert_equal_bytes(ask(s, fx["queries"]), fx, name + " through hip.py")


def in_chunks(s, queries, size):
    parts = [ask(s, queries[i:i + size]) for i in range(0, len(queries), size)]
    out = {"hits": np.concatenate([p["hits"] for p in parts])}
    for key in ("range_shapes", "range_distances"):
        out[key] = np.concatenate([p[key] for p in parts])
    counts = np.concatenate([np.diff(p["range_offsets"]) for p in parts])
    out["range_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


@pytest.mark.parametrize("size", [1, 100])
def test_a_batch_in_chunks_answers_as_the_whole(size):
    fx = pw.load_fixture("synthetic")
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(in_chunks(s, fx["queries"], size), fx, "chunks of %d" % size)


def test_a_thousand_queries_cross_the_query_chunk():
    """More queries than a workgroup stages at once, on the two-tile world: every copy of a query answers as the fixture's one"""
    fx = pw.load_fixture("pyramid30")
    order = np.arange(1000) % len(fx["queries"])
    order[500:] = order[500:][::-1].copy()
    o = fx["range_offsets"]
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        queries = fx["queries"][order]
        assert s.world_closest_shape(queries).tobytes() == fx["hits"][order].tobytes()
        offsets, shapes, distances = s.world_shapes_in_range(queries, distances=True)
        assert np.array_equal(np.diff(offsets), np.diff(o)[order])
        assert shapes.tobytes() == np.concatenate([fx["range_shapes"][o[i]:o[i + 1]] for i in order]).tobytes()
        assert distances.tobytes() == np.concatenate([fx["range_distances"][o[i]:o[i + 1]] for i in order]).tobytes()


def test_the_fast_library_answers_the_same_bytes():
    fx = pw.load_fixture("zoo")
    with hip.Solver(0, fast=True) as s:
        assert s._L.s2amd_build_flags().decode() == "fp-contract=fast"
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask(s, fx["queries"]), fx, "libs2amd_fast.so")


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
def test_queries_follow_the_world_as_the_device_steps_it():
    """12 steps of the pyramid30 world on the device; the queries then equal the statement applied to what s2amd_world_download returns"""
    fx = pw.load_fixture("pyramid30")
    world = sq.fixture_world(fx)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    queries = fx["queries"][:128]
    with hip.Solver(0) as s:
        upload(s, world)
        for _ in range(STEPS):
            s.world_step(params)
        got = ask(s, queries)
        now, _ = download(s, world)
    assert now["origins"].tobytes() != world["origins"].tobytes()
    assert_equal_bytes(got, pw.expected(now, queries), "after %d steps" % STEPS)
    assert got["hits"].tobytes() != fx["hits"][:128].tobytes()  # (the world moved under the queries)


def test_queries_are_read_only():
    """Two solvers in lockstep on the synthetic world, one asked both queries before and between steps: a download before and after the
    queries is the same bytes, and after every step both hold the same world and stage-3 status"""
    fx = pw.load_fixture("synthetic")
    world = sq.synthetic_world()
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    queries = fx["queries"]
    with hip.Solver(0) as asked, hip.Solver(0) as quiet:
        upload(asked, world), upload(quiet, world)
        before, _ = download(asked, world)
        assert_equal_bytes(ask(asked, queries), fx, "before the first step")
        after, _ = download(asked, world)
        for k in world_chain.WORLD_KEYS:
            assert np.ascontiguousarray(before[k]).tobytes() == np.ascontiguousarray(after[k]).tobytes(), k
        for step in range(3):
            asked.world_step(params), quiet.world_step(params)
            a = ask(asked, queries)
            assert_equal_bytes(ask(asked, queries), a, "step %d, asked again" % step)
            (wa, sta), (wb, stb) = download(asked, world), download(quiet, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert wa["bodies"]["position"].tobytes() != world["bodies"]["position"].tobytes()


def test_errors():
    fx = pw.load_fixture("zoo")
    queries = fx["queries"][:8].copy()
    with hip.Solver(0) as s:
        L = s._L
        # no resident world
        hits = new_hits(8)
        untouched = hits.tobytes()
        assert L.s2amd_world_closest_shape(s._h, wire.as_ptr(queries), 8, wire.as_ptr(hits)) == E_STATE
        assert raw_range_call(s, queries, 64)[0] == E_STATE
        for method in (s.world_closest_shape, s.world_shapes_in_range):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                method(queries)
        upload(s, sq.fixture_world(fx))
        # one invalid query refuses the whole call before anything is enqueued: every output keeps its fill
        rules = (("count", None, 0), ("count", None, 9), ("radius", None, -0.25), ("vertices", (0, 1), np.nan), ("maxDistance", None, np.inf),
                 ("maxDistance", None, -1.0), ("position", 0, np.inf), ("rot", 1, np.nan), ("radius", None, np.nan))
        for field, index, value in rules:
            bad = queries.copy()
            if index is None:
                bad[field][5] = value
            else:
                bad[field][5][index] = value
            assert L.s2amd_world_closest_shape(s._h, wire.as_ptr(bad), 8, wire.as_ptr(hits)) == E_INVALID, (field, value)
            assert hits.tobytes() == untouched
            rc, offsets, shapes, distances, total = raw_range_call(s, bad, 64)
            assert rc == E_INVALID and total == -7 and (offsets == -7).all() and (shapes == -7).all() and (distances == -7).all(), (field, value)
        assert L.s2amd_world_closest_shape(s._h, wire.as_ptr(queries), -1, wire.as_ptr(hits)) == E_INVALID
        assert L.s2amd_world_closest_shape(s._h, wire.as_ptr(queries), 8, None) == E_INVALID
        assert raw_range_call(s, queries, -1)[0] == E_INVALID
        # count == 0 touches nothing
        assert L.s2amd_world_closest_shape(s._h, None, 0, None) == 0 and hits.tobytes() == untouched
        rc, offsets, shapes, distances, total = raw_range_call(s, queries[:0], 4)
        assert rc == 0 and offsets.tolist() == [-7] and shapes.tolist() == [-7] * 4 and (distances == -7).all() and total == -7
        # the ask-again round trip: offsets and the total are filled, the lists are untouched
        want_offsets = fx["range_offsets"][:9]
        want = int(want_offsets[-1])
        assert want >= 2
        rc, offsets, shapes, distances, total = raw_range_call(s, queries, want - 1)
        assert rc == E_CAPACITY and total == want and np.array_equal(offsets, want_offsets)
        assert (shapes == -7).all() and (distances == -7).all()
        rc, offsets, shapes, distances, total = raw_range_call(s, queries, total)
        assert rc == 0 and np.array_equal(offsets, want_offsets)
        assert shapes[:total].tobytes() == fx["range_shapes"][:want].tobytes() and distances[:total].tobytes() == fx["range_distances"][:want].tobytes()
        # hip.py asks again by itself
        offsets, shapes, distances = s.world_shapes_in_range(fx["queries"], distances=True, expected=1)
        assert offsets.tobytes() == fx["range_offsets"].tobytes() and shapes.tobytes() == fx["range_shapes"].tobytes()
        assert distances.tobytes() == fx["range_distances"].tobytes()
        assert s.world_closest_shape(queries).tobytes() == fx["hits"][:8].tobytes()
