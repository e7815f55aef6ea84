"""Shape casts on the resident world (s2amd_world_cast_shape / _cast_shape_all; solver2d_amd/csrc/shape_cast.hip) against their
statement (tests/shape_cast_ref.py: numpy around the reference's own s2ShapeDistance): every answer equal byte for byte.  The fixture
tests read the statement's answers from tests/golden/shape_cast/*.npz and need no reference library."""
import ctypes

import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import resident, scene_query_world as sq, shape_cast_ref as ref, shape_cast_world as cw, world_chain
from tests.resident import E_CAPACITY, E_INVALID, E_STATE, download, upload

pytestmark = pytest.mark.gpu

STEPS = 12
f32 = np.float32


def ask(s, casts):
    """Both calls through the hip.py methods -> the three result arrays under cw.RESULT_KEYS"""
    return dict(zip(cw.RESULT_KEYS, (s.world_cast_shape(casts),) + s.world_cast_shape_all(casts)))


def new_hits(n):
    return np.full(12 * max(n, 1), -7, dtype=np.int32).view(wire.shape_cast_hit_dtype)


def raw_all_call(s, casts, capacity):
    """One s2amd_world_cast_shape_all through the C ABI -> (rc, offsets, hits, total); the arrays start as -7 so that what the call
    wrote shows"""
    offsets = np.full(len(casts) + 1, -7, dtype=np.int32)
    hits = new_hits(capacity)
    total = ctypes.c_int32(-7)
    rc = s._L.s2amd_world_cast_shape_all(s._h, wire.as_ptr(casts), len(casts), wire.as_ptr(offsets), wire.as_ptr(hits), capacity, ctypes.byref(total))
    return rc, offsets, hits, total.value


def ask_raw(s, casts):
    """... and through the C ABI itself, with exactly the capacity the answer needs"""
    first = new_hits(len(casts))
    assert s._L.s2amd_world_cast_shape(s._h, wire.as_ptr(casts), len(casts), wire.as_ptr(first)) == 0
    rc, offsets, _, total = raw_all_call(s, casts, 0)
    assert rc == (E_CAPACITY if total > 0 else 0) and total == offsets[-1]
    rc, offsets, hits, total = raw_all_call(s, casts, total)
    assert rc == 0
    return dict(zip(cw.RESULT_KEYS, (first, offsets, hits[:total])))


def assert_equal_bytes(got, want, what):
    resident.assert_equal_bytes(got, want, what, cw.RESULT_KEYS)


@pytest.mark.parametrize("name", cw.FIXTURES)
def test_fixtures_byte_equal(name):
    fx = cw.load_fixture(name)
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask_raw(s, fx["casts"]), fx, name + " through the C ABI")
        assert_equal_bytes(ask(s, fx["casts"]), fx, name + " through hip.py")


def in_chunks(s, casts, size):
    parts = [ask(s, casts[i:i + size]) for i in range(0, len(casts), size)]
    out = {key: np.concatenate([p[key] for p in parts]) for key in ("first", "all_hits")}
    counts = np.concatenate([np.diff(p["all_offsets"]) for p in parts])
    out["all_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


@pytest.mark.parametrize("size", [1, 100])
def test_a_batch_in_chunks_answers_as_the_whole(size):
    fx = cw.load_fixture("synthetic")
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(in_chunks(s, fx["casts"], size), fx, "chunks of %d" % size)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
def test_a_thousand_casts_cross_the_cast_chunk():
    """More casts than a workgroup stages at once, on the two-tile world: the fixture's casts in another order, every fourth with its
    sweep halved, against the statement"""
    fx = cw.load_fixture("pyramid30")
    world = sq.fixture_world(fx)
    order = np.arange(1000) % len(fx["casts"])
    order[500:] = order[500:][::-1].copy()
    casts = fx["casts"][order]
    casts["maxFraction"][::4] *= f32(0.5)
    with hip.Solver(0) as s:
        upload(s, world)
        got = ask(s, casts)
    assert_equal_bytes(got, cw.expected(world, casts), "1,000 casts")
    same = np.arange(1000) % 4 != 0
    assert got["first"][same].tobytes() == fx["first"][order][same].tobytes()


def test_the_fast_library_answers_the_same_bytes():
    fx = cw.load_fixture("zoo")
    with hip.Solver(0, fast=True) as s:
        assert s._L.s2amd_build_flags().decode() == "fp-contract=fast"
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask(s, fx["casts"]), fx, "libs2amd_fast.so")


@pytest.mark.parametrize("name", ["pyramid30", "synthetic"])
def test_without_translation_a_cast_is_a_proximity_query(name):
    """Owes nothing to the new statement: a cast that does not move hits exactly what is within the threshold where it stands.  Every
    cast of the fixture that names a shape is put where it stopped, the others stay at their starts; s2amd_world_shapes_in_range with
    maxDistance one ulp below the threshold names the same shapes with the same distance bits."""
    fx = cw.load_fixture(name)
    casts = fx["casts"].copy()
    for c, h in zip(casts, fx["first"]):
        if h["shape"] >= 0:
            c["position"] = ref.mul_add(c["position"], h["fraction"], c["translation"])
    casts["translation"] = 0
    queries = np.zeros(len(casts), dtype=wire.proximity_query_dtype)
    for key in ("vertices", "count", "radius", "position", "rot", "maskBits"):
        queries[key] = casts[key]
    queries["maxDistance"] = np.nextafter(ref.THRESHOLD, f32(0.0))
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        offsets, hits = s.world_cast_shape_all(casts)
        want_offsets, want_shapes, want_distances = s.world_shapes_in_range(queries, distances=True)
        first = s.world_cast_shape(casts)
    assert offsets.tobytes() == want_offsets.tobytes() and hits["shape"].tobytes() == want_shapes.tobytes()
    assert hits["distance"].tobytes() == want_distances.tobytes()
    assert (hits["fraction"] == 0).all() and (hits["iterations"] == 0).all()
    named = np.diff(offsets) > 0
    assert np.array_equal(named, fx["first"]["shape"] >= 0) and int(named.sum()) >= 128
    assert np.array_equal(first["shape"][named], hits["shape"][offsets[:-1][named]]) and (first["shape"][~named] == -1).all()  # (all at fraction 0: the lowest slot)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
def test_casts_follow_the_world_as_the_device_steps_it():
    """12 steps of a base-12 pyramid on the device and through the oracle chain of tests/world_chain.py in the device's constraint
    order; before the first step and after the 6th and the 12th the casts equal the statement applied to the oracle's world"""
    world = synthetic.pyramid_world(12)
    oracle = world_chain.copy_world(world)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    casts = cw.make_batch(world, 64, 41)
    answers = []
    with hip.Solver(0) as s:
        upload(s, world)
        for step in range(STEPS + 1):
            if step in (0, 6, STEPS):
                got = ask(s, casts)
                assert_equal_bytes(got, cw.expected(oracle, casts), "after %d steps" % step)
                answers.append(got["first"].tobytes())
            if step < STEPS:
                s.world_step(params)
                world_chain.oracle_world_step(params, oracle, contact_order=s.contact_order()[0])
    assert oracle["origins"].tobytes() != world["origins"].tobytes() and len(set(answers)) == 3  # (the world moved under the casts)
    assert 4 * int((got["first"]["shape"] >= 0).sum()) >= len(casts)


def test_casts_are_read_only():
    """Two solvers in lockstep on the synthetic world, one asked both calls before and between steps: a download before and after the
    casts is the same bytes, and after every step both hold the same world and stage-3 status"""
    fx = cw.load_fixture("synthetic")
    world = sq.synthetic_world()
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    casts = fx["casts"]
    with hip.Solver(0) as asked, hip.Solver(0) as quiet:
        upload(asked, world), upload(quiet, world)
        before, _ = download(asked, world)
        assert_equal_bytes(ask(asked, casts), fx, "before the first step")
        after, _ = download(asked, world)
        for k in world_chain.WORLD_KEYS:
            assert np.ascontiguousarray(before[k]).tobytes() == np.ascontiguousarray(after[k]).tobytes(), k
        for step in range(3):
            asked.world_step(params), quiet.world_step(params)
            a = ask(asked, casts)
            assert_equal_bytes(ask(asked, casts), a, "step %d, asked again" % step)
            (wa, sta), (wb, stb) = download(asked, world), download(quiet, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert wa["bodies"]["position"].tobytes() != world["bodies"]["position"].tobytes()


def test_errors():
    fx = cw.load_fixture("pyramid30")
    casts = fx["casts"][:8].copy()
    with hip.Solver(0) as s:
        L = s._L
        # no resident world
        first = new_hits(8)
        untouched = first.tobytes()
        assert L.s2amd_world_cast_shape(s._h, wire.as_ptr(casts), 8, wire.as_ptr(first)) == E_STATE
        assert raw_all_call(s, casts, 64)[0] == E_STATE
        for method in (s.world_cast_shape, s.world_cast_shape_all):
            with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
                method(casts)
        upload(s, sq.fixture_world(fx))
        # one invalid cast refuses the whole call before anything is enqueued: every output keeps its fill
        rules = (("count", None, 0), ("count", None, 9), ("radius", None, -0.25), ("radius", None, np.nan), ("vertices", (0, 1), np.nan),
                 ("maxFraction", None, np.inf), ("maxFraction", None, -1.0), ("maxFraction", None, np.nan), ("position", 0, np.inf),
                 ("rot", 1, np.nan), ("translation", 0, np.nan), ("translation", 1, -np.inf))
        for field, index, value in rules:
            bad = casts.copy()
            if index is None:
                bad[field][5] = value
            else:
                bad[field][5][index] = value
            assert L.s2amd_world_cast_shape(s._h, wire.as_ptr(bad), 8, wire.as_ptr(first)) == E_INVALID, (field, value)
            assert first.tobytes() == untouched
            rc, offsets, hits, total = raw_all_call(s, bad, 64)
            assert rc == E_INVALID and total == -7 and (offsets == -7).all() and hits.tobytes() == new_hits(64).tobytes(), (field, value)
        assert L.s2amd_world_cast_shape(s._h, wire.as_ptr(casts), -1, wire.as_ptr(first)) == E_INVALID
        assert L.s2amd_world_cast_shape(s._h, wire.as_ptr(casts), 8, None) == E_INVALID
        assert raw_all_call(s, casts, -1)[0] == E_INVALID
        # an unused vertex and the padding are not looked at
        odd = casts.copy()
        odd["vertices"][:, 7, 1][odd["count"] < 8] = np.nan
        odd["pad"] = -1
        assert s.world_cast_shape(odd).tobytes() == fx["first"][:8].tobytes()
        # count == 0 touches nothing
        assert L.s2amd_world_cast_shape(s._h, None, 0, None) == 0 and first.tobytes() == untouched
        rc, offsets, hits, total = raw_all_call(s, casts[:0], 4)
        assert rc == 0 and offsets.tolist() == [-7] and hits.tobytes() == new_hits(4).tobytes() and total == -7
        # the ask-again round trip: offsets and the total are filled, the records are untouched
        want_offsets = fx["all_offsets"][:9]
        want = int(want_offsets[-1])
        assert want >= 2
        rc, offsets, hits, total = raw_all_call(s, casts, want - 1)
        assert rc == E_CAPACITY and total == want and np.array_equal(offsets, want_offsets)
        assert hits.tobytes() == new_hits(want - 1).tobytes()
        rc, offsets, hits, total = raw_all_call(s, casts, total)
        assert rc == 0 and np.array_equal(offsets, want_offsets) and hits[:total].tobytes() == fx["all_hits"][:want].tobytes()
        # hip.py asks again by itself
        offsets, hits = s.world_cast_shape_all(fx["casts"], expected=1)
        assert offsets.tobytes() == fx["all_offsets"].tobytes() and hits.tobytes() == fx["all_hits"].tobytes()
        assert s.world_cast_shape(casts).tobytes() == fx["first"][:8].tobytes()
