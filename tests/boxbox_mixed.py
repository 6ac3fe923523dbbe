"""One wave whose 64 lanes interleave every case of the block<->torso generator (brs_core.hpp: collide_coupled (i)), shared by
tests/test_boxbox_mixed_cpu.py and tests/test_boxbox_mixed_wave_gpu.py.  The generator's cases exclude each other per lane,
but a wave walks every arm that one of its lanes takes; since the arms share one tail (patch_begin and the insertion loop)
and one pair of fp64 poses, a lane's result must still not depend on which arms its neighbours walk.

The states are rows of block_robot_states, edge_edge_states and pinned_states (tests/constructed_states.py); the far lanes
are block_robot rows with the block moved 0.5 m along x, out of the generator's reach.  kind() says which case a state is,
from the ORACLE's generator alone (oracle.box_box_points: code 0-2 = a torso face is the reference, 3-5 = a block face,
>= 6 = the edge pair) and, where the oracle emits nothing, from the brute-force separations of tests/ref_boxbox.py.

How the reference-face role of a constructed pose is known, by geometry: the reference face belongs to the box whose face
axis has the largest separation, and that is the box the OTHER one touches with a vertex.  A block pushed corner-first into
a torso face (block_robot: random orientation, centre 0.7-1.3 block half sizes off the face) has its deepest feature in a
block vertex: the torso face is the reference ("faceT").  Where a torso corner pokes into a block face, the block face is
the reference ("faceB"): block_robot row 12, and those pinned rows -- the block flat on the floor, face to face with the
torso's broad side within 0.03 rad of pitch and yaw -- in which the tilt makes a torso corner lead.  In the
face-to-face rows the two face separations are level within that tilt, so the role is not guessed from the construction:
kind() reads it off the oracle, and the tests assert it for every row.  Test infrastructure."""
import numpy as np

from tests import constructed_states as cs, ref_boxbox as rb

MARGIN = 0.002
KINDS = ("edge_in", "edge_out", "faceT", "faceB", "sep", "far")
# rows per kind: (scenario, row).  edge_in / edge_out: the edge pair has the largest separation, inside / outside the
# margin; sep: within reach, a face axis separates by more than the margin
ROWS = {
    "edge_in": [("edge_edge", r) for r in (0, 1, 2, 4, 5)] + [("pinned", r) for r in (1, 10, 13)] + [("block_robot", r) for r in (5, 17, 24)],
    "edge_out": [("edge_edge", r) for r in (3, 8, 15, 18, 20, 22, 24, 26)] + [("block_robot", r) for r in (7, 23)],
    "faceT": [("block_robot", r) for r in (0, 2, 3, 6, 9, 13)] + [("pinned", r) for r in (4, 5, 11, 16, 17, 20)],
    "faceB": [("block_robot", 12)] + [("pinned", r) for r in (2, 7, 8, 50, 52, 85, 88, 94)],
    "sep": [("block_robot", r) for r in (1, 4, 8, 26, 32, 38)] + [("pinned", r) for r in (0, 3, 6, 9, 12, 15)],
    "far": [("block_robot", r) for r in (10, 11, 14, 20, 22, 25, 27, 35, 41, 46)],
}
FAR_SHIFT = np.array([0.5, 0.0, 0.0])


def geometry(q):
    """qpos row -> (block centre in the torso frame, the same relative to the torso geom centre, RTB)"""
    RT, RB = cs.quat_to_mat(q[3:7]), cs.quat_to_mat(q[12:16])
    cB = RT.T @ (q[9:12] - q[0:3])
    return cB, cB - cs.TC, RT.T @ RB


def kind(q):
    """the generator's case of one qpos row (KINDS), or "none" where the boxes overlap within the margin and the clip leaves no point"""
    from oracle import oracle as O
    cB, cg, RTB = geometry(q)
    reach = np.linalg.norm(cs.TS) + cs.TC[2] + cs.BS * np.sqrt(3.0) + MARGIN   # collide_coupled's first test
    if cB @ cB > reach * reach:
        return "far"
    code = O.box_box_points(cs.TS, cs.BS, cg, RTB, MARGIN)[3]
    if code >= 0:
        return "edge_in" if code >= 6 else "faceB" if code >= 3 else "faceT"
    VT, VB = rb.box_vertices(cs.TS, cs.BS, cg, RTB)
    seps = [(k, rb.separation(L, VT, VB)) for k, _, L in rb.axes15(RTB)]
    if max(s for _, s in seps) <= MARGIN:
        return "none"
    return "edge_out" if max(s for k, s in seps if k != "E") <= MARGIN else "sep"


def population():
    """-> (qpos [64,16], qvel [64,14], ctrl [64,2], kinds [64], source scenario [64]); the kinds go round the lanes in turn"""
    inputs = {name: cs.scenario_inputs(name) for name in ("block_robot", "edge_edge", "pinned")}
    todo = {k: list(v) for k, v in ROWS.items()}
    rows = []
    while any(todo.values()):
        rows += [(k, *todo[k].pop(0)) for k in KINDS if todo[k]]
    qpos = np.array([inputs[name][0][r] for _, name, r in rows]); qvel = np.array([inputs[name][1][r] for _, name, r in rows])
    ctrl = np.array([inputs[name][2][r] for _, name, r in rows])
    kinds, source = np.array([k for k, _, _ in rows]), np.array([name for _, name, _ in rows])
    qpos[kinds == "far", 9:12] += FAR_SHIFT
    assert len(rows) == 64
    return qpos, qvel, ctrl, kinds, source


def scenario(env_id="Env03-v2"):
    """the population as an entry of cs.SCENARIOS, for cs.run_scenario_steps_on (a test registers it for its own duration)"""
    qpos, qvel, ctrl, _, _ = population()
    return dict(env=env_id, states=lambda: (qpos.copy(), qvel.copy()), ctrl=lambda n: ctrl.copy(), nsub=5,
                covered=lambda probes, vt: None, probe=lambda teacher, qpos: None)
