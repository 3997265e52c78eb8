"""Batched full bundle adjustment (ba_batch_*): the parts that need no GPU — exports,
bindings, the result record, host-side validation (which runs before anything touches a
device) and the per-problem planner (stable landmark-major grouping, pair lists,
last-writer marks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ba_batch_create", "ba_batch_destroy", "ba_batch_solve", "ba_batch_update_values",
       "ba_batch_get_poses", "ba_batch_get_points", "ba_batch_info", "ba_batch_scratch_bytes",
       "ba_batch_plan_problem"]


def test_symbols_declared_exported_bound(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.SIGNATURES, name
    # the declared parameter counts are the bound ones
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
        assert m, name
        n_decl = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_decl == len(_lib.SIGNATURES[name][1]), name


def test_result_record_layout(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    m = re.search(r"typedef struct \{\s*int ([^;]*);[^}]*\}\s*ba_batch_result;", src, re.S)
    assert m
    assert [f.strip() for f in m.group(1).split(",")] == \
        ["n_iter", "converged", "n_rows", "status", "dropped_pivots"]
    assert [f for f, _ in _lib.BaBatchResult._fields_] == \
        ["n_iter", "converged", "n_rows", "status", "dropped_pivots"]
    assert C.sizeof(_lib.BaBatchResult) == 20


def _create(lib, h, B, cam_off, pose_off, pt_off, obs_off, obs=None):
    """ba_batch_create on a two-camera, well-formed set of arrays sized for the
    LARGEST offsets used by the tests; returns (rc, batch pointer)."""
    i32 = lambda a: np.asarray(a, np.int32)
    n_cam, n_pose, n_pt, n_obs = 4, 8, 8, 8
    intr = np.ones((n_cam, 4))
    camT = np.tile(np.r_[np.eye(3).ravel(), 0, 0, 0], (n_cam, 1))
    poseT = np.tile(np.r_[np.eye(3).ravel(), 0, 0, 0], (n_pose, 1))
    X = np.ones((n_pt, 3))
    pf = np.zeros(n_pose, np.uint8)
    qf = np.zeros(n_pt, np.uint8)
    oc, op, oq = (i32(np.zeros(n_obs)) for _ in range(3)) if obs is None else map(i32, obs)
    uv = np.zeros((n_obs, 2))
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    i = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    co, po, qo = i32(cam_off), i32(pose_off), i32(pt_off)
    oo = np.asarray(obs_off, np.int64)
    b = C.c_void_p()
    rc = lib.ba_batch_create(C.byref(b), h, B, i(co), i(po), i(qo),
                             oo.ctypes.data_as(C.POINTER(C.c_int64)), d(intr), d(camT), d(poseT),
                             u(pf), d(X), u(qf), i(oc), i(op), i(oq), d(uv))
    return rc, b


def test_host_validation_rejects_without_a_gpu(built):
    """No handle exists in this test (there is no GPU to create one on).  The array
    checks come first — B, offsets, indices inside their problem — and the handle is
    looked at last, so every malformed batch is refused for its own reason and a
    well-formed one for the NULL handle; nothing touches a device."""
    lib = _lib.load()
    err = lambda: lib.ba_last_error().decode()
    h = C.c_void_p(0)
    ok = dict(cam_off=[0, 2, 4], pose_off=[0, 4, 8], pt_off=[0, 4, 8], obs_off=[0, 4, 8])
    rc, b = _create(lib, h, 2, **ok)
    assert rc == -1 and not b.value and "null handle" in err()
    rc, b = _create(lib, h, 0, [0], [0], [0], [0])
    assert rc == -1 and "B must be >= 1" in err()
    rc, b = _create(lib, h, -3, [0], [0], [0], [0])
    assert rc == -1 and "B must be >= 1" in err()
    for key in ok:
        bad = dict(ok)
        bad[key] = [1] + ok[key][1:]
        rc, b = _create(lib, h, 2, **bad)
        assert rc == -1 and key in err() and "must be 0" in err(), (key, err())
        bad[key] = [0, ok[key][2], ok[key][1]]
        rc, b = _create(lib, h, 2, **bad)
        assert rc == -1 and key in err() and "not decrease" in err(), (key, err())
    # indices are problem-local: pose 4 does not exist in a 4-pose problem, camera 2
    # not in a 2-camera one, and a negative point never
    for which, val in ((0, 2), (1, 4), (2, 4), (2, -1)):
        obs = [np.zeros(8), np.zeros(8), np.zeros(8)]
        obs[which][5] = val
        rc, b = _create(lib, h, 2, obs=obs, **ok)
        assert rc == -1 and "observation 1 of problem 1" in err(), (which, val, err())
    # the other entry points refuse a NULL batch
    assert lib.ba_batch_solve(None, C.byref(_lib.make_options()), None, 0, None) == -1
    assert lib.ba_batch_update_values(None, None, None) == -1
    assert lib.ba_batch_get_poses(None, None) == -1 and lib.ba_batch_info(None, None) == -1
    assert lib.ba_batch_scratch_bytes(None, None) == -1
    lib.ba_batch_destroy(None)


def _plan(lib, pose_fixed, pt_fixed, obs_pose, obs_pt):
    n = len(obs_pose)
    pf, qf = np.asarray(pose_fixed, np.uint8), np.asarray(pt_fixed, np.uint8)
    op, oq = np.asarray(obs_pose, np.int32), np.asarray(obs_pt, np.int32)
    order, pair = np.zeros(n, np.int32), np.zeros(n, np.int32)
    last = np.zeros(n, np.uint8)
    plm, ppose = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    i = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    P = lib.ba_batch_plan_problem(len(pf), u(pf), len(qf), u(qf), n, i(op), i(oq), i(order),
                                  i(pair), u(last), i(plm), i(ppose))
    return P, order, pair, last, plm[:max(P, 0)], ppose[:max(P, 0)]


def test_planner_three_observations_by_hand(built):
    """Two poses (both optimisable), two points; input order: (pose 1, point 1),
    (pose 0, point 0), (pose 1, point 1) again.  Landmark-major and stable: point 0's
    observation first, then the two of point 1 in input order; point 1's pair with
    pose 1 is written by the LATER of its two observations (reference :826)."""
    lib = _lib.load()
    P, order, pair, last, plm, ppose = _plan(lib, [0, 0], [0, 0], [1, 0, 1], [1, 0, 1])
    assert P == 2
    assert order.tolist() == [1, 0, 2]
    assert pair.tolist() == [0, 1, 1]
    assert last.tolist() == [1, 0, 1]
    assert plm.tolist() == [0, 1] and ppose.tolist() == [0, 1]


def test_planner_fixed_members_and_pair_order(built):
    """Pairs exist only between optimisable poses and optimisable points, are numbered
    landmark by landmark with ascending pose inside a landmark, and the optimisable
    indices follow input order of the non-fixed entries."""
    lib = _lib.load()
    # poses: 0 fixed, 1, 2 optimisable (j = 0, 1); points: 0 optimisable (i = 0), 1 fixed,
    # 2 optimisable (i = 1)
    obs_pose = [2, 1, 0, 2, 1, 2, 0]
    obs_pt = [2, 2, 2, 0, 1, 2, 0]
    P, order, pair, last, plm, ppose = _plan(lib, [1, 0, 0], [0, 1, 0], obs_pose, obs_pt)
    assert order.tolist() == [3, 6, 4, 0, 1, 2, 5]
    # point 0: (pose 2) -> pair 0; point 2: poses 1, 2 -> pairs 1, 2
    assert P == 3 and plm.tolist() == [0, 1, 1] and ppose.tolist() == [1, 0, 1]
    assert pair.tolist() == [0, -1, -1, 2, 1, -1, 2]
    assert last.tolist() == [1, 0, 0, 0, 1, 0, 1]
    assert lib.ba_batch_plan_problem(2, None, 2, None, 1,
                                     np.array([2], np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                     np.array([0], np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                     None, None, None, None, None) == -1


def test_planner_matches_the_oracles_pair_list(built):
    """On a cut of the reference scene the planner's pairs are the oracle's: the same
    (landmark, pose) list in the same order."""
    from oracle import oracle_py as O
    sc = scenes.pose_window_subscene(scenes.test_ba_scene(), 50, 60, n_fixed=2)
    pr = scenes.scaled_problem(sc)
    lib = _lib.load()
    P, order, pair, last, plm, ppose = _plan(lib, pr["pose_fixed"], pr["pt_fixed"], pr["obs_pose"],
                                             pr["obs_pt"])
    o = O.Oracle(pr)
    oi, oj, _ = o.get_pairs()
    assert P == len(oi) == 390 and plm.tolist() == list(oi) and ppose.tolist() == list(oj)
    # every pair has exactly one writer, and it is the pair's last observation in input order
    assert np.bincount(pair[pair >= 0], weights=last[pair >= 0], minlength=P).tolist() == [1.0] * P
    pos_in_input = order
    for p in range(0, P, 97):
        members = np.nonzero(pair == p)[0]
        assert last[members].argmax() == pos_in_input[members].argmax()


def test_batch_scene_shapes():
    win = scenes.ba_batch_scene(3, n_pose=6, n_pt=40, seed=5)
    assert len(win) == 3
    for sc in win:
        assert sc["T_wc_init"].shape[0] == 6 and sc["X_init"].shape[0] == 40
        assert sc["pose_fixed"].sum() == 2
        assert sc["obs_pt"].size == 40 * 6 * 2 and sc["obs_pose"].max() == 5
    assert not np.array_equal(win[0]["X_true"], win[1]["X_true"])


def test_python_solve_batch_refuses_a_sharded_solver():
    """As the C++ facade: a solver with a shard or an all-reduce configured cannot join a
    batch; refused before any array is built or a device is touched."""
    from bundle_adjustment_solver_amd.solver import FullBundleAdjustmentSolver, Options
    plain, sharded, hooked = (FullBundleAdjustmentSolver(0) for _ in range(3))
    sharded.SetShard(0, 2)
    hooked.SetShard(0, 1, allreduce=lambda which, ptr, n, stream: 0)
    for bad in (sharded, hooked):
        with pytest.raises(RuntimeError, match="shard or an all-reduce"):
            FullBundleAdjustmentSolver.SolveBatch([plain, bad], Options())
