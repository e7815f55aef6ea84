"""The narrow-chain fixtures (tests/golden/narrow_chain/*.npz), the part that needs no GPU: the conditions the fixtures must meet, read
from the fixtures alone; the oracle (oracle/narrow_oracle.c) carried through every pose equals them byte for byte; and, where the
compiled reference is there, the fixtures are what the statement (tests/narrow_chain_ref.py: the reference's own s2Collide* with the
carried cache, then the id matching) says today."""
import glob
import os

import numpy as np
import pytest

from solver2d_amd import wire
from tests import contact_query_ref as cq, narrow_chain_world as nw, oraclebind

FIXTURES = ("chains", "directed")


@pytest.fixture(scope="module")
def chains():
    return nw.load_fixture("chains")


@pytest.fixture(scope="module")
def directed():
    return nw.load_fixture("directed")


def test_fixture_covers_what_it_claims(chains):
    """Conditions, not measurements: the generator was tuned until the reference alone meets them (the achieved counts are what
    python -m tests.narrow_chain_world prints)."""
    largest_capture = max(os.path.getsize(p) for p in glob.glob(os.path.join(os.path.dirname(nw.GOLDEN), "*_step*.npz")))
    for name in FIXTURES:
        for part in range(nw.parts_of(name)):
            assert os.path.getsize(nw.fixture_path(name, part)) <= largest_capture, (name, part)
    n, poses = chains["status"].shape
    assert (n, poses) == (nw.PAIRS, nw.POSES) == (288, 12)
    for key, new in zip(("pairs_pre", "contacts_pre"), nw.fresh(n)):  # every chain starts as a new contact
        assert np.ascontiguousarray(chains[key][:, 0]).tobytes() == new.tobytes(), key
    shapes = chains["shapes"]
    assert (shapes["count"][shapes["type"] == nw.POLYGON] <= 8).all() and (shapes["count"][shapes["type"] == nw.POLYGON] >= 3).all()
    assert set(shapes["count"][shapes["type"] == nw.POLYGON].tolist()) == set(range(3, 9))
    assert (shapes["radius"][shapes["type"] == nw.POLYGON] > 0).any() and (shapes["radius"][shapes["type"] == nw.POLYGON] == 0).any()
    got = nw.coverage(chains)
    print(got)
    assert got["finite"]
    assert 4 * got["separated"] <= got["pair-poses"]
    assert len(got["updated per type pair"]) == 9 and min(got["updated per type pair"].values()) >= 100, got["updated per type pair"]
    for fn in sorted(cq.TAKES_CACHE):
        assert min(got["entering cache counts"][fn]) >= 5, (fn, got["entering cache counts"][fn])  # caches of 0, 1, 2 and 3 vertices
        assert min(got["point counts"][fn]) >= 1, (fn, got["point counts"][fn])                    # manifolds of 0, 1 and 2 points
    assert len(got["count changes"]) == 6 and min(got["count changes"].values()) >= 5, got["count changes"]
    assert got["persisted points with their stamped impulses"] >= 200
    assert got["same count, an id lost"] >= 10
    assert got["one point persisted beside one that is not"] >= 10
    assert got["born mid-chain"] >= 20
    # a cache index names a vertex of the pair's own shapes (the kernel reads its staged polygons at it), in every pre-state
    for key in ("pairs_pre", "pairs_post"):
        p = chains[key]
        for side, first in (("cacheIndexA", 0), ("cacheIndexB", 1)):
            counts = np.where(shapes["type"][first::2] == nw.POLYGON, shapes["count"][first::2], 2)
            for k in range(3):
                used = p["cacheCount"] > k
                assert (p[side][..., k][used] < np.broadcast_to(counts[:, None], used.shape)[used]).all(), (key, side, k)


def test_directed_fixture_holds_the_stated_cases(directed):
    cases = nw.directed_cases()
    status, contacts = directed["status"][:, 0], directed["contacts_post"][:, 0]
    assert len(cases) == len(status) and nw.coverage(directed)["finite"]
    for i, (what, _, _, _, _, want_status, want_points, _) in enumerate(cases):
        assert status[i] == want_status, (what, status[i])
        if want_points is not None:
            assert contacts["pointCount"][i] == want_points, (what, contacts["pointCount"][i])
    # the two rows with a made-up old manifold: the first old point with the id wins; exchanged ids exchange the impulses
    pairs = directed["pairs_post"][:, 0]
    same, swapped = ([i for i, c in enumerate(cases) if c[7] == mode][0] for mode in ("same ids", "swapped ids"))
    impulses = contacts["points"]["normalImpulse"]
    assert pairs["persisted"][same].tolist() == [1, 0] and contacts["frictionPersisted"][same] == 0
    assert impulses[same].tolist() == [nw.stamp_value(0, same, 0, 0), 0.0]
    assert pairs["persisted"][swapped].tolist() == [1, 1] and contacts["frictionPersisted"][swapped] == 1
    assert impulses[swapped].tolist() == [nw.stamp_value(0, swapped, 1, 0), nw.stamp_value(0, swapped, 0, 0)]
    assert all(directed["pairs_pre"]["cacheCount"][i, 0] > 0 for i in (same, swapped))  # ... and they enter GJK with a warm cache
    # the fat-box rows: exactly touching is UPDATED, one ulp apart is SEPARATED
    fat_rows = range(len(cases) - nw.BAND_ROWS - nw.FAT_BOX_ROWS, len(cases) - nw.BAND_ROWS)
    assert [int(status[i]) for i in fat_rows] == [wire.PAIR_UPDATED, wire.PAIR_UPDATED, wire.PAIR_SEPARATED, wire.PAIR_SEPARATED]
    for i, (axis, side) in zip(fat_rows, ((0, 1), (1, -1), (1, 1), (0, -1))):
        fa, fb = directed["fat"][i, 0]
        d = fb[axis] - fa[axis + 2] if side > 0 else fa[axis] - fb[axis + 2]
        upper = fa[axis + 2] if side > 0 else fb[axis + 2]  # the box edge the other box's lower edge is compared with
        assert d == (0 if status[i] == wire.PAIR_UPDATED else np.spacing(upper)), (i, d)
    # the band rows, from both sides: two points down to just inside 4 * linearSlop, none just outside
    band = contacts[len(cases) - nw.BAND_ROWS:]
    assert band["pointCount"].tolist() == [2, 2, 2, 2, 0] * 2
    sep = band["points"]["separation"]
    assert (sep[[0, 5]] < 0).all() and (sep[[1, 6]] == 0).all() and (sep[[2, 3, 7, 8]] > 0).all() and (sep[[3, 8]] < nw.SPECULATIVE).all()
    assert band["normal"][:5, 1].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0] and band["normal"][5:, 1].tolist() == [-1.0, -1.0, -1.0, -1.0, 0.0]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_fixture(name):
    """oraclebind.update_contacts, its own output carried through every pose: updated slots equal the fixture on every byte of pair
    state and contact, separated slots are untouched; the first failure names the pose, the pair and the type pair."""
    assert nw.run_chain(oraclebind.update_contacts, nw.load_fixture(name)) == 0


@pytest.mark.ref
@pytest.mark.skipif(not cq.available(), reason="oracle/_ref/libs2ref.so (the compiled reference) is absent")
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_what_the_reference_says(name):
    fx, again = nw.load_fixture(name), nw.build_fixture(name)
    assert sorted(fx) == sorted(again)
    for key in sorted(fx):
        assert again[key].dtype == fx[key].dtype and again[key].shape == fx[key].shape, key
        assert again[key].tobytes() == fx[key].tobytes(), key
