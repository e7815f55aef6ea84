"""The script of the sharded-world tests (tests/test_islands_dist.py over gloo with the oracle, tests/test_gpu_sharded.py and
tests/test_gpu_reshard.py with the device): four pyramids with one spare contact slot, a contact that joins two of them after step 1
and is destroyed after step 3 -- the same on every rank and in the single process.  Test infrastructure only."""
import socket

import numpy as np

from solver2d_amd import wire


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _joining_contact(world, islands_of, a_island, b_island):
    """A two-point manifold between the top boxes of two pyramids (made-up geometry: a solver input, not a scene)."""
    bodies, contacts, _ = world
    a = int(np.flatnonzero(islands_of == a_island)[-1])
    b = int(np.flatnonzero(islands_of == b_island)[-1])
    c = contacts[int(np.flatnonzero(contacts["pointCount"] == 2)[0])].copy()
    c["bodyA"], c["bodyB"] = a, b
    c["normal"] = (1.0, 0.0)
    for p in range(2):
        c["points"][p]["localAnchorA"] = (0.5, 0.25 - 0.5 * p)
        c["points"][p]["localAnchorB"] = (-0.5, 0.25 - 0.5 * p)
        c["points"][p]["separation"] = -0.004
        c["points"][p]["normalImpulse"] = 0.0
        c["points"][p]["tangentImpulse"] = 0.0
    return c


def _merging_script(world, step):
    """The collision phase of the test, the same on every rank and in the single process: after step 1 a contact appears between
    island 0 and island 1 (different ranks under the first partition), after step 3 it is destroyed again."""
    from solver2d_amd import islands as isl
    bodies, contacts, joints = world
    slot = len(contacts) - 1
    if step == 1:
        island, _n = isl.find_islands(bodies, contacts, joints)
        new = contacts.copy()
        new[slot] = _joining_contact(world, island, 0, 1)
        return new
    if step == 3:
        new = contacts.copy()
        new[slot]["bodyA"], new[slot]["bodyB"], new[slot]["pointCount"] = -1, -1, 0
        return new
    return None


def _spare(world, n):
    b, c, j = world
    free = np.zeros(n, dtype=wire.contact_dtype)
    free["bodyA"], free["bodyB"], free["constraintIndex"] = -1, -1, -1
    return b, np.concatenate([c, free]), j
