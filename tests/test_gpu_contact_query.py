"""Contact queries on the resident world (s2amd_world_collide_shape / _deepest_contact; solver2d_amd/csrc/contact_query.hip) against their
statement (tests/contact_query_ref.py: numpy around the reference's own s2Collide*): every answer equal byte for byte.  The fixture
tests read the statement's answers from tests/golden/contact_query/*.npz and need no reference library; the moved-world test compares
with the library's own narrow phase (s2amd_update_contacts) and needs none either."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, wire
from tests import contact_query_ref as ref, contact_query_world as cw, resident, scene_query_world as sq, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, upload

pytestmark = pytest.mark.gpu

STEPS = 12


def ask(s, queries):
    """Both calls through the hip.py methods -> the three result arrays under cw.RESULT_KEYS"""
    offsets, hits = s.world_collide_shape(queries)
    return dict(zip(cw.RESULT_KEYS, (offsets, hits, s.world_deepest_contact(queries))))


def new_hits(n):
    return np.full(max(n, 1), -7, dtype=np.int32).repeat(20).view(wire.contact_hit_dtype)


def raw_collide_call(s, queries, capacity):
    """One s2amd_world_collide_shape through the C ABI -> (rc, offsets, hits, total); the arrays start as -7 so that what the call wrote
    shows"""
    offsets = np.full(len(queries) + 1, -7, dtype=np.int32)
    hits = new_hits(capacity)
    total = ctypes.c_int32(-7)
    rc = s._L.s2amd_world_collide_shape(s._h, wire.as_ptr(queries), len(queries), wire.as_ptr(offsets), wire.as_ptr(hits), capacity,
                                        ctypes.byref(total))
    return rc, offsets, hits, total.value


def untouched(hits):
    return (hits.view(np.int32) == -7).all()


def ask_raw(s, queries):
    """... and through the C ABI itself, with exactly the capacity the answer needs"""
    deepest = new_hits(len(queries))
    assert s._L.s2amd_world_deepest_contact(s._h, wire.as_ptr(queries), len(queries), wire.as_ptr(deepest)) == 0
    rc, offsets, hits, total = raw_collide_call(s, queries, 0)
    assert rc == (E_CAPACITY if total > 0 else 0) and total == offsets[-1] and untouched(hits)
    rc, offsets, hits, total = raw_collide_call(s, queries, total)
    assert rc == 0 and total == offsets[-1]
    return dict(zip(cw.RESULT_KEYS, (offsets, hits[:total], deepest)))


def assert_equal_bytes(got, want, what):
    resident.assert_equal_bytes(got, want, what, cw.RESULT_KEYS)


@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_byte_equal(name):
    fx = cw.load_fixture(name)
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask_raw(s, fx["queries"]), fx, name + " through the C ABI")
        assert_equal_bytes(ask(s, fx["queries"]), fx, name + " through hip.py")


def in_chunks(s, queries, size):
    parts = [ask(s, queries[i:i + size]) for i in range(0, len(queries), size)]
    out = {key: np.concatenate([p[key] for p in parts]) for key in ("hits", "deepest")}
    counts = np.concatenate([np.diff(p["offsets"]) for p in parts])
    out["offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


@pytest.mark.parametrize("size", [1, 100])
def test_a_batch_in_chunks_answers_as_the_whole(size):
    fx = cw.load_fixture("synthetic")
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(in_chunks(s, fx["queries"], size), fx, "chunks of %d" % size)


def test_a_thousand_queries_cross_the_query_chunk():
    """More queries than a workgroup walks, on the two-tile world: every copy of a query answers as the fixture's one"""
    fx = cw.load_fixture("pyramid30")
    order = np.arange(1000) % len(fx["queries"])
    order[500:] = order[500:][::-1].copy()
    o = fx["offsets"]
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        queries = fx["queries"][order]
        assert s.world_deepest_contact(queries).tobytes() == fx["deepest"][order].tobytes()
        offsets, hits = s.world_collide_shape(queries)
        assert np.array_equal(np.diff(offsets), np.diff(o)[order])
        assert hits.tobytes() == np.concatenate([fx["hits"][o[i]:o[i + 1]] for i in order]).tobytes()


def test_the_fast_library_answers_the_same_bytes():
    fx = cw.load_fixture("zoo")
    with hip.Solver(0, fast=True) as s:
        assert s._L.s2amd_build_flags().decode() == "fp-contract=fast"
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask(s, fx["queries"]), fx, "libs2amd_fast.so")


def test_capacity_zero_states_the_offsets_and_the_total():
    fx = cw.load_fixture("zoo")
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        rc, offsets, hits, total = raw_collide_call(s, fx["queries"], 0)
        assert rc == E_CAPACITY and total == fx["offsets"][-1] > 0 and offsets.tobytes() == fx["offsets"].tobytes() and untouched(hits)


def moved_world_queries(now):
    """Queries copied from shapes of the moved pyramid -- every seventh brick and the ground's neighbours -- at the shape's own transform
    nudged by a few centimetres, and a few of the three other types laid on bricks (they make the world shape the manifold's A or B)"""
    shapes, bodies, origins = now["shapes"], now["bodies"], now["origins"]
    rng = np.random.RandomState(5)
    queries = []
    for slot in np.nonzero(shapes["type"] == cw.POLYGON)[0][::7]:
        sh, body = shapes[slot], int(shapes["body"][slot])
        q = np.zeros(1, dtype=wire.contact_query_dtype)[0]
        for key in ("vertices", "normals", "type", "count", "radius"):
            q[key] = sh[key]
        q["position"] = origins[body] + (rng.rand(2).astype(np.float32) * 0.06 - 0.03)
        q["rot"], q["maskBits"] = bodies["rot"][body], cw.ALL
        queries.append(q)
        if len(queries) % 8 == 0:
            at = sq._centre(now, int(slot)) + np.array([0.0, 0.3], dtype=np.float32)
            queries.append(cw.make_query(cw.CIRCLE, [(0.0, 0.0)], 0.25, at, 0.0))
            queries.append(cw.make_query(cw.CAPSULE, [(-0.3, 0.0), (0.3, 0.05)], 0.1, at, 0.2))
            queries.append(cw.make_query(cw.SEGMENT, [(-0.4, 0.1), (0.4, -0.1)], 0.0, at, 1.0))
    return np.array(queries, dtype=wire.contact_query_dtype)


def test_the_query_agrees_with_the_library_narrow_phase_on_a_world_that_moved():
    """12 device steps of the pyramid, a download, and the queries' candidates as a host pair list for the pinned stage call
    s2amd_update_contacts: the query an extra shape on an extra body, A and B by the order rule, empty caches, a fat box so wide that
    no pair is separated.  Normal, point count, anchors, separations and ids equal the hits' bytes; a candidate without points is no hit."""
    fx = cw.load_fixture("pyramid30")
    world = sq.fixture_world(fx)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    with hip.Solver(0) as s:
        upload(s, world)
        for _ in range(STEPS):
            s.world_step(params)
        now, _ = download(s, world)
        assert now["origins"].tobytes() != world["origins"].tobytes()
        queries = moved_world_queries(now)
        offsets, hits = s.world_collide_shape(queries)
        deepest = s.world_deepest_contact(queries)
        nb, ns, nq = len(now["bodies"]), len(now["shapes"]), len(queries)
        bodies = np.concatenate([now["bodies"], np.zeros(nq, dtype=wire.body_dtype)])
        bodies["rot"][nb:], bodies["position"][nb:], bodies["type"][nb:] = queries["rot"], queries["position"], wire.BODY_DYNAMIC
        origins = np.concatenate([np.ascontiguousarray(now["origins"], dtype=np.float32).reshape(-1, 2), queries["position"]])
        shapes = np.concatenate([now["shapes"], np.zeros(nq, dtype=wire.shape_dtype)])
        for key in ("vertices", "normals", "type", "count", "radius"):
            shapes[key][ns:] = queries[key]
        shapes["body"][ns:], shapes["categoryBits"][ns:] = nb + np.arange(nq), 1
        shapes["fatAABB"][ns:] = (-1.0e6, -1.0e6, 1.0e6, 1.0e6)
        pair_list = [(i, slot) for i, q in enumerate(queries) for slot in ref.candidates(now, q)]  # (numpy only: no reference library)
        assert len(pair_list) >= 2 * nq
        pairs = np.zeros(len(pair_list), dtype=wire.pair_state_dtype)
        contacts = np.zeros(len(pair_list), dtype=wire.contact_dtype)
        query_is_b = []
        for k, (i, slot) in enumerate(pair_list):
            flipped = (int(queries["type"][i]), int(shapes["type"][slot])) not in ref.REGISTERS
            query_is_b.append(int(flipped))
            pairs["shapeA"][k], pairs["shapeB"][k] = (slot, ns + i) if flipped else (ns + i, slot)
        status = s.update_contacts(bodies, origins, shapes, pairs, contacts)
    assert (status == wire.PAIR_UPDATED).all()
    want = [[] for _ in range(nq)]
    for k, (i, slot) in enumerate(pair_list):
        c = contacts[k]
        if c["pointCount"] == 0:
            continue
        h = np.zeros(1, dtype=wire.contact_hit_dtype)[0]
        h["shape"], h["body"], h["pointCount"], h["queryIsB"], h["normal"] = slot, shapes["body"][slot], c["pointCount"], query_is_b[k], c["normal"]
        for p in range(int(c["pointCount"])):
            for key in ("localAnchorA", "localAnchorB", "separation"):
                h["points"][p][key] = c["points"][p][key]
            h["points"][p]["id"] = pairs["id"][k][p]
        want[i].append(h)
    counts = [len(x) for x in want]
    assert np.array_equal(np.diff(offsets), counts)
    flat = np.array([h for x in want for h in x], dtype=wire.contact_hit_dtype)
    assert_equal_bytes({"offsets": offsets, "hits": hits, "deepest": deepest[:0]}, {"offsets": offsets, "hits": flat, "deepest": deepest[:0]}, "narrow phase")
    assert sum(counts) >= nq and set(flat["queryIsB"].tolist()) == {0, 1} and set(flat["pointCount"].tolist()) == {1, 2}
    for i in range(nq):  # the deepest record is the list's entry of least separation, the first of equal ones
        if not want[i]:
            assert deepest["shape"][i] == -1
            continue
        least = [min(float(x) for x in h["points"]["separation"][:h["pointCount"]]) for h in want[i]]
        assert deepest[i].tobytes() == want[i][int(np.argmin(least))].tobytes(), i


def test_queries_are_read_only():
    """Two solvers in lockstep on the synthetic world, one asked both queries before and between steps: a download before and after the
    queries is the same bytes, and after every step both hold the same world and stage-3 status"""
    fx = cw.load_fixture("synthetic")
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
    fx = cw.load_fixture("zoo")
    queries = fx["queries"][:8].copy()
    queries[5] = cw.make_query(cw.POLYGON, cw.BOX, 0.1, (0.0, 1.0), 0.3)
    with hip.Solver(0) as s:
        L = s._L
        # no resident world
        hits = new_hits(8)
        fill = hits.tobytes()
        assert L.s2amd_world_deepest_contact(s._h, wire.as_ptr(queries), 8, wire.as_ptr(hits)) == E_STATE
        assert raw_collide_call(s, queries, 64)[0] == E_STATE
        for method in (s.world_deepest_contact, s.world_collide_shape):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                method(queries)
        upload(s, sq.fixture_world(fx))
        assert L.s2amd_world_deepest_contact(s._h, wire.as_ptr(queries), 8, wire.as_ptr(hits)) == 0
        hits = new_hits(8)
        # one invalid query refuses the whole call before anything is enqueued: every output keeps its fill
        rules = (("type", None, -1), ("type", None, 4), ("count", None, 2), ("count", None, 9), ("radius", None, -0.25), ("radius", None, np.nan),
                 ("radius", None, np.inf), ("vertices", (3, 1), np.nan), ("normals", (0, 0), np.inf), ("position", 0, np.inf), ("position", 1, np.nan),
                 ("rot", 0, np.inf), ("rot", 1, np.nan))
        for field, index, value in rules:
            bad = queries.copy()
            if index is None:
                bad[field][5] = value
            else:
                bad[field][5][index] = value
            assert not ref.valid_query(bad[5])
            assert L.s2amd_world_deepest_contact(s._h, wire.as_ptr(bad), 8, wire.as_ptr(hits)) == E_INVALID, (field, value)
            assert hits.tobytes() == fill
            rc, offsets, listed, total = raw_collide_call(s, bad, 64)
            assert rc == E_INVALID and total == -7 and (offsets == -7).all() and untouched(listed), (field, value)
        # what a type does not read is not looked at
        ok = queries.copy()
        ok[5] = cw.make_query(cw.SEGMENT, [(-1.0, 0.0), (1.0, 0.0)], 0.0, (0.0, 1.0), 0.3)
        ok["radius"][5], ok["count"][5], ok["vertices"][5][2], ok["normals"][5][0] = np.nan, 77, np.nan, np.nan
        assert ref.valid_query(ok[5]) and L.s2amd_world_deepest_contact(s._h, wire.as_ptr(ok), 8, wire.as_ptr(new_hits(8))) == 0
        assert L.s2amd_world_deepest_contact(s._h, wire.as_ptr(queries), -1, wire.as_ptr(hits)) == E_INVALID
        assert L.s2amd_world_deepest_contact(s._h, wire.as_ptr(queries), 8, None) == E_INVALID
        assert raw_collide_call(s, queries, -1)[0] == E_INVALID
        # count == 0 touches nothing
        assert L.s2amd_world_deepest_contact(s._h, None, 0, None) == 0 and hits.tobytes() == fill
        rc, offsets, listed, total = raw_collide_call(s, queries[:0], 4)
        assert rc == 0 and offsets.tolist() == [-7] and untouched(listed) and total == -7
        # the ask-again round trip: offsets and the total are filled, the hits are untouched
        first = fx["queries"][:8]
        want_offsets = fx["offsets"][:9]
        want = int(want_offsets[-1])
        assert want >= 2
        rc, offsets, listed, total = raw_collide_call(s, first, want - 1)
        assert rc == E_CAPACITY and total == want and np.array_equal(offsets, want_offsets) and untouched(listed)
        rc, offsets, listed, total = raw_collide_call(s, first, total)
        assert rc == 0 and np.array_equal(offsets, want_offsets) and listed[:total].tobytes() == fx["hits"][:want].tobytes()
        # hip.py asks again by itself
        offsets, listed = s.world_collide_shape(fx["queries"], expected=1)
        assert offsets.tobytes() == fx["offsets"].tobytes() and listed.tobytes() == fx["hits"].tobytes()
        assert s.world_deepest_contact(first).tobytes() == fx["deepest"][:8].tobytes()
