"""Move-and-slide on the resident world (s2amd_world_move_shapes; solver2d_amd/csrc/mover_query.hip) against its statement
(tests/mover_ref.py: numpy around the reference's own s2ShapeDistance): every answer equal byte for byte.  The fixture tests read the
statement's answers from tests/golden/mover/*.npz and need no reference library."""
import numpy as np
import pytest

from solver2d_amd import hip, synthetic, wire
from tests import mover_ref as ref, mover_world as mw, scene_query_world as sq, shape_cast_world as cw, world_chain
from tests.resident import E_INVALID, E_STATE, assert_equal_bytes, download, upload

pytestmark = pytest.mark.gpu

STEPS = 12
f32 = np.float32
needs_reference = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")


def new_results(n):
    return np.full(8 * max(n, 1), -7, dtype=np.int32).view(wire.mover_result_dtype)


def new_planes(n):
    return np.full(8 * 8 * max(n, 1), -7, dtype=np.int32).view(wire.mover_plane_dtype)


def ask(s, movers):
    return dict(zip(mw.RESULT_KEYS, s.world_move_shapes(movers)))


def ask_raw(s, movers, planes=True):
    """Through the C ABI itself, into arrays of exactly the size the answer needs that start as -7"""
    results, out = new_results(len(movers)), new_planes(len(movers)) if planes else None
    assert s._L.s2amd_world_move_shapes(s._h, wire.as_ptr(movers), len(movers), wire.as_ptr(results), wire.as_ptr(out) if planes else None) == 0
    return {"results": results, "planes": out.reshape(len(movers), 8)} if planes else {"results": results}


@pytest.mark.parametrize("name", mw.FIXTURES)
def test_fixtures_byte_equal(name):
    fx = mw.load_fixture(name)
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask_raw(s, fx["movers"]), fx, name + " through the C ABI")
        assert_equal_bytes(ask_raw(s, fx["movers"], planes=False), fx, name + " through the C ABI without planes")
        assert_equal_bytes(ask(s, fx["movers"]), fx, name + " through hip.py")
        assert s.world_move_shapes(fx["movers"], planes=False).tobytes() == fx["results"].tobytes()


@pytest.mark.parametrize("size", [1, 100])
def test_a_batch_in_chunks_answers_as_the_whole(size):
    fx = mw.load_fixture("synthetic")
    movers = fx["movers"]
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        parts = [ask(s, movers[i:i + size]) for i in range(0, len(movers), size)]
    assert_equal_bytes({k: np.concatenate([p[k] for p in parts]) for k in mw.RESULT_KEYS}, fx, "chunks of %d" % size)


@needs_reference
def test_a_thousand_movers_cross_the_staged_chunk():
    """More movers than a workgroup stages at once, on the two-tile world: the fixture's movers in another order, every fourth with
    its displacement halved and every fifth with another iteration limit, against the statement"""
    fx = mw.load_fixture("pyramid30")
    world = sq.fixture_world(fx)
    order = np.arange(1000) % len(fx["movers"])
    order[500:] = order[500:][::-1].copy()
    movers = fx["movers"][order]
    movers["translation"][::4] *= f32(0.5)
    movers["maxIterations"][::5] = 1 + np.arange(len(movers["maxIterations"][::5])) % 8
    with hip.Solver(0) as s:
        upload(s, world)
        got = ask(s, movers)
    assert_equal_bytes(got, mw.expected(world, movers), "1,000 movers")
    same = (np.arange(1000) % 4 != 0) & (np.arange(1000) % 5 != 0)
    assert got["results"][same].tobytes() == fx["results"][order][same].tobytes()


def test_the_fast_library_answers_the_same_bytes():
    fx = mw.load_fixture("zoo")
    with hip.Solver(0, fast=True) as s:
        assert s._L.s2amd_build_flags().decode() == "fp-contract=fast"
        upload(s, sq.fixture_world(fx))
        assert_equal_bytes(ask(s, fx["movers"]), fx, "libs2amd_fast.so")


@pytest.mark.parametrize("name", mw.FIXTURES)
def test_plane_0_is_the_first_hit_of_the_same_cast(name):
    """Owes nothing to the new statement: for the movers the fixture marks, plane 0 is the record s2amd_world_cast_shape answers on
    the device for the mover's first cast"""
    fx = mw.load_fixture(name)
    marked = fx["first"]
    assert len(marked) >= 64
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        hits = s.world_cast_shape(mw.to_casts(fx["movers"][marked]))
        results, planes = s.world_move_shapes(fx["movers"][marked])
    assert (results["planeCount"] >= 1).all()
    for key in ("shape", "body", "fraction", "distance", "point", "normal"):
        assert hits[key].tobytes() == np.ascontiguousarray(planes[key][:, 0]).tobytes(), key
    assert np.array_equal(results["advances"][results["planeCount"] == 1], hits["iterations"][results["planeCount"] == 1])


def test_the_prefix_property_holds_on_the_device():
    """With maxIterations = m the planes are the first planes of the maxIterations = 8 answer, and the mover stands where that one
    stood after m casts"""
    fx = mw.load_fixture("pyramid30")
    base = fx["movers"][::2].copy()
    with hip.Solver(0) as s:
        upload(s, sq.fixture_world(fx))
        base["maxIterations"] = 8
        full_results, full_planes = s.world_move_shapes(base)
        seen = 0
        for m in range(1, 8):
            base["maxIterations"] = m
            results, planes = s.world_move_shapes(base)
            n = results["planeCount"]
            assert (n <= full_results["planeCount"]).all() and (results["iterations"] == np.minimum(full_results["iterations"], m)).all()
            for i in range(len(base)):
                assert planes[i, :n[i]].tobytes() == full_planes[i, :n[i]].tobytes(), (m, i)
                assert not planes[i, n[i]:].tobytes().strip(b"\0"), (m, i)
            cut = full_results["iterations"] > m
            assert (results["status"][cut] == wire.MOVER_OUT_OF_ITERATIONS).all() and results[~cut].tobytes() == full_results[~cut].tobytes()
            seen += int(cut.sum())
    assert seen >= 16


def test_the_walk_frame_by_frame():
    """The walk fixture's 300 frames fed back frame by frame: every frame's answer byte-equal, three worlds, two movers"""
    fx = mw.load_walk_fixture()
    for kind in mw.WALKS:
        with hip.Solver(0) as s:
            upload(s, mw.walk_world(kind))
            for which in mw.WALKERS:
                results, planes = mw.walk(None, which, s.world_move_shapes)
                assert_equal_bytes({"results": results, "planes": planes},
                                   {"results": fx["%s_%s_results" % (kind, which)], "planes": fx["%s_%s_planes" % (kind, which)]}, "%s %s" % (kind, which))


@needs_reference
def test_movers_follow_the_world_as_the_device_steps_it():
    """12 steps of a base-12 pyramid on the device and through the oracle chain of tests/world_chain.py in the device's constraint
    order; before the first step and after the 6th and the 12th the movers equal the statement applied to the oracle's world"""
    world = synthetic.pyramid_world(12)
    oracle = world_chain.copy_world(world)
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    movers = mw.from_casts(cw.make_batch(world, 64, 41))
    movers["flags"][::7] = wire.MOVER_STATIC_ONLY
    movers["ignoreBody"][::5] = 3
    answers = []
    with hip.Solver(0) as s:
        upload(s, world)
        for step in range(STEPS + 1):
            if step in (0, 6, STEPS):
                got = ask(s, movers)
                assert_equal_bytes(got, mw.expected(oracle, movers), "after %d steps" % step)
                answers.append(got["results"].tobytes())
            if step < STEPS:
                s.world_step(params)
                world_chain.oracle_world_step(params, oracle, contact_order=s.contact_order()[0])
    assert oracle["origins"].tobytes() != world["origins"].tobytes() and len(set(answers)) == 3  # (the world moved under the movers)
    assert 4 * int((got["results"]["planeCount"] >= 1).sum()) >= len(movers)


def test_movers_are_read_only():
    """Two solvers in lockstep on the synthetic world, one asked before and between steps: a download before and after the call is
    the same bytes, and after every step both hold the same world and stage-3 status -- a step after a call equals the step alone"""
    fx = mw.load_fixture("synthetic")
    world = sq.synthetic_world()
    params = wire.StepParams.make("TGS_Soft", 1.0 / 60.0, 4, 2, True)
    movers = fx["movers"]
    with hip.Solver(0) as asked, hip.Solver(0) as quiet:
        upload(asked, world), upload(quiet, world)
        before, _ = download(asked, world)
        assert_equal_bytes(ask(asked, movers), fx, "before the first step")
        after, _ = download(asked, world)
        for k in world_chain.WORLD_KEYS:
            assert np.ascontiguousarray(before[k]).tobytes() == np.ascontiguousarray(after[k]).tobytes(), k
        for step in range(3):
            asked.world_step(params), quiet.world_step(params)
            a = ask(asked, movers)
            assert_equal_bytes(ask(asked, movers), a, "step %d, asked again" % step)
            (wa, sta), (wb, stb) = download(asked, world), download(quiet, world)
            assert np.array_equal(sta, stb), "step %d: status" % step
            for k in world_chain.WORLD_KEYS:
                assert np.ascontiguousarray(wa[k]).tobytes() == np.ascontiguousarray(wb[k]).tobytes(), "step %d: %s" % (step, k)
        assert wa["bodies"]["position"].tobytes() != world["bodies"]["position"].tobytes()


def test_errors():
    fx = mw.load_fixture("pyramid30")
    movers = fx["movers"][:8].copy()
    with hip.Solver(0) as s:
        L = s._L
        results, planes = new_results(8), new_planes(8)
        untouched = results.tobytes(), planes.tobytes()

        def call(m, count=8, res=results, pl=planes):
            return L.s2amd_world_move_shapes(s._h, wire.as_ptr(m), count, wire.as_ptr(res), wire.as_ptr(pl))

        # no resident world
        assert call(movers) == E_STATE and (results.tobytes(), planes.tobytes()) == untouched
        with pytest.raises(hip.S2AmdError, match="error %d" % E_STATE):
            s.world_move_shapes(movers)
        world = sq.fixture_world(fx)
        upload(s, world)
        # one invalid mover refuses the whole call before anything is enqueued: every output keeps its fill
        rules = (("count", None, 0), ("count", None, 9), ("radius", None, -0.25), ("radius", None, np.nan), ("vertices", (0, 1), np.nan),
                 ("position", 0, np.inf), ("rot", 1, np.nan), ("translation", 0, np.nan), ("translation", 1, -np.inf),
                 ("maxIterations", None, 0), ("maxIterations", None, 9), ("maxIterations", None, -3), ("flags", None, 2), ("flags", None, 0x80000001),
                 ("reserved", 0, 1), ("reserved", 3, -1), ("ignoreBody", None, len(world["bodies"])), ("ignoreBody", None, 2 ** 31 - 1))
        for field, index, value in rules:
            bad = movers.copy()
            if index is None:
                bad[field][5] = value
            else:
                bad[field][5][index] = value
            assert not ref.valid_mover(bad[5], len(world["bodies"])), (field, value)
            assert call(bad) == E_INVALID, (field, value)
            assert (results.tobytes(), planes.tobytes()) == untouched, (field, value)
            assert L.s2amd_world_move_shapes(s._h, wire.as_ptr(bad), 8, wire.as_ptr(results), None) == E_INVALID and results.tobytes() == untouched[0]
        assert call(movers, -1) == E_INVALID
        assert L.s2amd_world_move_shapes(s._h, wire.as_ptr(movers), 8, None, wire.as_ptr(planes)) == E_INVALID
        assert L.s2amd_world_move_shapes(s._h, None, 8, wire.as_ptr(results), wire.as_ptr(planes)) == E_INVALID
        assert (results.tobytes(), planes.tobytes()) == untouched
        # an unused vertex is not looked at; any negative ignoreBody is none; the last body slot is one
        odd = movers.copy()
        odd["vertices"][:, 7, 1][odd["count"] < 8] = np.nan
        odd["ignoreBody"] = -12345
        assert s.world_move_shapes(odd)[0].tobytes() == fx["results"][:8].tobytes()
        odd["ignoreBody"] = len(world["bodies"]) - 1
        s.world_move_shapes(odd)
        # count == 0 touches nothing
        assert L.s2amd_world_move_shapes(s._h, None, 0, None, None) == 0 and (results.tobytes(), planes.tobytes()) == untouched
        assert call(movers) == 0
        assert results.tobytes() == fx["results"][:8].tobytes() and planes.tobytes() == fx["planes"][:8].tobytes()
