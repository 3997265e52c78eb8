"""GPU tests of ba_batch_marginalize (BaBatch.marginalize, MarginalizeBatch): the
marginalisation prior of every problem of a batch in one launch (k_ba_batch_marg:
linearisation over the landmarks of the marked poses, Schur complement into a permuted LDS
image, partial Cholesky whose trailing update is the prior).

Reference, independent of the code under test: marg_ref.reference — the CPU oracle
linearises the sub-problem of the landmarks in L, the full normal matrix is assembled on
the host and {marked poses} U L eliminated two ways; their difference is the reference's
own noise.

Tolerance: the project's rule of test_gpu_covariance.py — the noise must be <= 1e-8 (else
the scene is unfit) and the GPU result lies within 10 x max(noise, 1e-12) of route (i), in
the matrix-wide relative measure max|x - ref| / max|ref|, for H and for b.

Windows (marg_ref.SCENES): the smallest that reach every path — 32, 64, 96 and 112 image
columns; 1, 2, 3 and 8 marked poses (4, 14 and no padding columns, a marked block that
straddles a tile); mono and stereo; with and without fixed poses (gauge-singular H).
"""
import copy

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib, scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, Camera, FullBundleAdjustmentSolver,
                                                 marginal_to_user_units)

import marg_ref

pytestmark = pytest.mark.gpu

HUBER = 1.0
ROW_FIELDS = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
              "damping_term", "iteration_status", "rho", "model_change", "trial_cost")


def row_bits(rows):
    return np.array([[getattr(r, f) for f in ROW_FIELDS] for r in rows], float).reshape(-1, len(ROW_FIELDS))


_cache = {}


def scene(name):
    """(problem dict, marking, far pose, H, b, noise, kept, L) — computed once"""
    if name not in _cache:
        pr, mk, far = marg_ref.build_scene(name)
        _cache[name] = (pr, mk, far) + marg_ref.reference(pr, mk, HUBER)
    return _cache[name]


WIDTH = {n: marg_ref.image_columns(*marg_ref.build_scene(n)[:2]) for n in marg_ref.SCENES}
BY_WIDTH = {w: [n for n in marg_ref.SCENES if WIDTH[n] == w] for w in (32, 64, 96, 112)}


def plan_abi(pr, mk):
    """ba_batch_marg_plan_problem of one problem -> (kept, L)"""
    lib = _lib.load()
    n_pose, n_pt = len(pr["pose_fixed"]), len(pr["pt_fixed"])
    kept, mq = np.zeros(n_pose, np.int32), np.zeros(n_pt, np.uint8)
    u8 = lambda a: np.ascontiguousarray(a, np.uint8).ctypes.data_as(_lib._U8)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib._I32)
    K = lib.ba_batch_marg_plan_problem(n_pose, u8(pr["pose_fixed"]), u8(mk), n_pt, u8(pr["pt_fixed"]),
                                       len(pr["obs_pt"]), i32(pr["obs_pose"]), i32(pr["obs_pt"]),
                                       kept.ctypes.data_as(_lib._I32), mq.ctypes.data_as(_lib._U8))
    assert K >= 0
    return kept[:K], mq != 0


def run(items, huber=HUBER, calls=1):
    """BaBatch.marginalize of [(problem, marking)] -> per problem (H, b, kept, L, result);
    with calls > 1 every call must return the bits of the first"""
    b = BaBatch([pr for pr, _ in items])
    mk = np.concatenate([m for _, m in items])
    Hl, bl, kl, res = b.marginalize(mk, huber)
    Hl, bl, mq = [h.copy() for h in Hl], [v.copy() for v in bl], b.marg_pt.copy()
    for _ in range(calls - 1):
        H2, b2, k2, res2 = b.marginalize(mk, huber)
        assert all(np.array_equal(x, y) for x, y in zip(Hl + bl, H2 + b2))
        assert np.array_equal(mq, b.marg_pt)
        assert [tuple(getattr(r, f) for f, _ in r._fields_) for r in res] == \
            [tuple(getattr(r, f) for f, _ in r._fields_) for r in res2]
    out = [(Hl[p], bl[p], kl[p], b.points_of(p, mq) != 0, res[p]) for p in range(len(items))]
    b.close()
    return out


def check(label, pr, mk, got, ref, far=None):
    H, bv, kept, in_l, res = got
    rH, rb, noise, rkept, rl = ref
    eH, eb = marg_ref.rel_diff(H, rH), marg_ref.rel_diff(bv, rb)
    print("%s: reference noise %.3e  gpu error H %.3e b %.3e" % (label, noise, eH, eb))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert res.status == 0 and res.dropped_pivots == 0
    tol = 10.0 * max(noise, 1e-12)
    assert eH <= tol and eb <= tol, (label, eH, eb, tol)
    assert np.array_equal(H, H.T)
    pk, pl = plan_abi(pr, mk)
    assert np.array_equal(kept, rkept) and np.array_equal(pk, rkept)
    assert np.array_equal(in_l, rl) and np.array_equal(pl, rl)
    opt = np.asarray(pr["pose_fixed"]) == 0
    assert (res.n_kept, res.n_marg_pose, res.n_marg_pt) == \
        (len(rkept), int((opt & (np.asarray(mk) != 0)).sum()), int(rl.sum()))
    assert np.abs(H).max() > 0 and np.abs(bv).max() > 0
    if far is not None:
        i = 6 * list(kept).index(far)
        assert not H[i:i + 6].any() and not H[:, i:i + 6].any() and not bv[i:i + 6].any()
        assert not rH[i:i + 6].any() and not rb[i:i + 6].any()


@pytest.fixture(scope="module")
def by_width(built):
    """the four batches of test 1, one per image width, each run twice"""
    out = {}
    for w, names in BY_WIDTH.items():
        assert names, w
        out.update(zip(names, run([scene(n)[:2] for n in names], calls=2)))
    return out


@pytest.mark.parametrize("width", [32, 64, 96, 112])
def test_prior_matches_the_host_elimination(by_width, width):
    for n in BY_WIDTH[width]:
        pr, mk, far = scene(n)[:3]
        check("%s (image %d)" % (n, width), pr, mk, by_width[n], scene(n)[3:], far)


def test_position_and_width_independence(by_width):
    names = list(marg_ref.SCENES)
    mixed = run([scene(n)[:2] for n in names])
    for n, m in zip(names, mixed):
        (alone,) = run([scene(n)[:2]])
        for g in (alone, by_width[n]):
            assert np.array_equal(m[0], g[0]) and np.array_equal(m[1], g[1]), n
            assert np.array_equal(m[3], g[3])
            assert (g[4].status, g[4].dropped_pivots, g[4].n_marg_pt) == (0, 0, m[4].n_marg_pt)


def test_marking_a_fixed_pose_adds_its_landmarks(by_width):
    for n in ("mono5_m1", "stereo12_m3"):
        pr, mk = scene(n)[:2]
        mk2 = mk.copy()
        mk2[0] = 1
        assert pr["pose_fixed"][0] and not mk[0]
        ref = marg_ref.reference(pr, mk2, HUBER)
        (got,) = run([(pr, mk2)])
        check("%s + fixed pose 0" % n, pr, mk2, got, ref)
        assert np.array_equal(got[2], by_width[n][2])            # the kept set is the same
        assert got[3].sum() > by_width[n][3].sum()               # L grew
        assert got[4].n_marg_pose == by_width[n][4].n_marg_pose  # a fixed pose owns no column


def test_edge_markings(built):
    pr = scene("mono8_m2")[0]
    n_pose = len(pr["pose_fixed"])
    (none,) = run([(pr, np.zeros(n_pose, np.uint8))])
    assert none[4].status == 0 and none[4].dropped_pivots == 0
    assert (none[4].n_kept, none[4].n_marg_pose, none[4].n_marg_pt) == (6, 0, 0)
    assert none[0].shape == (36, 36) and not none[0].any() and not none[1].any() and not none[3].any()
    # every optimisable pose marked: K = 0, no output, NULL H and bvec accepted
    every = (np.asarray(pr["pose_fixed"]) == 0).astype(np.uint8)
    b = BaBatch([pr])
    res = (_lib.BaBatchMargResult * 1)()
    rc = b.lib.ba_batch_marginalize(b.b, HUBER, every.ctypes.data_as(_lib._U8), None, None, None, res)
    assert rc == 0 and res[0].status == 0 and res[0].dropped_pivots == 0
    assert (res[0].n_kept, res[0].n_marg_pose) == (0, 6) and res[0].n_marg_pt > 0
    Hl, bl, kl, r2 = b.marginalize(every, HUBER)
    assert Hl[0].shape == (0, 0) and bl[0].shape == (0,) and len(kl[0]) == 0 and r2[0].status == 0
    # H is required as soon as a pose is kept
    rc = b.lib.ba_batch_marginalize(b.b, HUBER, np.zeros(n_pose, np.uint8).ctypes.data_as(_lib._U8),
                                    None, None, None, res)
    assert rc == -1 and "null H" in b.lib.ba_last_error().decode()
    b.close()


def test_more_problems_than_cus(built):
    pr, mk = scene("mono5_m1")[:2]
    got = run([(pr, mk)] * 300)
    assert len(got) == 300
    for g in got:
        assert g[4].status == 0 and g[4].dropped_pivots == 0
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1])
    assert np.abs(got[0][0]).max() > 0 and np.abs(got[0][1]).max() > 0


def test_status_codes(built):
    good, gmk = scene("stereo18_m1")[:2]
    over = scenes.scaled_problem(scenes.ba_batch_scene(1, 19, 30, True, 21, n_fixed=2)[0])
    assert int((over["pose_fixed"] == 0).sum()) == 17
    omk = np.zeros(19, np.uint8)
    omk[2] = 1
    nan, nmk = scene("mono5_m1")[:2]
    nan = copy.copy(nan)
    nan["pt_X"] = nan["pt_X"].copy()
    nan["pt_X"][3, 1] = np.nan
    got = run([(good, gmk), (over, omk), (nan, nmk)])
    assert [g[4].status for g in got] == [0, 2, 1]
    assert got[1][0].shape == (96, 96) and got[2][0].shape == (12, 12)
    for g in got[1:]:
        assert not g[0].any() and not g[1].any() and not g[3].any()
    (alone,) = run([(good, gmk)])
    assert np.array_equal(got[0][0], alone[0]) and np.array_equal(got[0][1], alone[1])
    assert np.abs(alone[0]).max() > 0


def test_nothing_visible_changes(built):
    names = ["stereo12_m3", "mono8_m2", "stereo4_m1"]
    probs = [scene(n)[0] for n in names]
    mk = np.concatenate([scene(n)[1] for n in names])
    opt = make_options(max_iter=5, thr_step=0.0, thr_cost=0.0)
    a, b = BaBatch(probs), BaBatch(probs)
    T0, X0 = a.get_poses(), a.get_points()
    a.marginalize(mk, 0.37)                     # (another Huber threshold than the solve's)
    assert np.array_equal(a.get_poses(), T0) and np.array_equal(a.get_points(), X0)
    ra, sa = a.solve(opt)
    rb, sb = b.solve(opt)
    for p in range(len(probs)):
        assert np.array_equal(row_bits(ra[p]), row_bits(rb[p])) and len(ra[p]) == 5
        assert (sa[p].n_iter, sa[p].converged, sa[p].status, sa[p].dropped_pivots) == \
            (sb[p].n_iter, sb[p].converged, sb[p].status, sb[p].dropped_pivots)
    T1, X1 = a.get_poses(), a.get_points()
    assert np.array_equal(T1, b.get_poses()) and np.array_equal(X1, b.get_points())
    # after a solve: the prior at the solution, the values left alone, the covariance intact
    Hl, bl, kl, res = a.marginalize(mk, HUBER)
    assert np.array_equal(a.get_poses(), T1) and np.array_equal(a.get_points(), X1)
    ca, cb = a.covariance(HUBER), b.covariance(HUBER)
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])
    assert [(r.status, r.dropped_pivots) for r in ca[2]] == [(r.status, r.dropped_pivots) for r in cb[2]]
    for p, n in enumerate(names):
        pr = copy.copy(probs[p])
        pr["pose_T"], pr["pt_X"] = a.poses_of(p, T1).copy(), a.points_of(p, X1).copy()
        ref = marg_ref.reference(pr, scene(n)[1], HUBER)
        check("%s at the solved values" % n, pr, scene(n)[1],
              (Hl[p], bl[p], kl[p], a.points_of(p, a.marg_pt) != 0, res[p]), ref, scene(n)[2])
    a.close()
    b.close()


def _facade_solver(sc):
    s = FullBundleAdjustmentSolver(0)
    for c in range(sc["intr"].shape[0]):
        s.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    hp, hq = s.AddPoseArray(sc["T_wc_init"].copy()), s.AddPointArray(sc["X_init"].copy())
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    return s, hp, hq


def test_facade_returns_user_units_of_the_raw_call(built):
    scs = [scenes.ba_batch_scene(1, 5, 37, True, 31)[0], scenes.ba_batch_scene(1, 7, 41, False, 32)[0]]
    for sc in scs:  # the marked pose sees the first 20 landmarks only
        drop = (sc["obs_pose"] == 2) & (sc["obs_pt"] >= 20)
        for k in marg_ref.OBS_KEYS:
            sc[k] = sc[k][~drop]
    built_ = [_facade_solver(sc) for sc in scs]
    solvers = [t[0] for t in built_]
    out = FullBundleAdjustmentSolver.MarginalizeBatch(solvers, [[int(t[1][2])] for t in built_],
                                                      sigma_pixel=0.7)
    items = []
    for sv in solvers:
        intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
        mk = np.zeros(len(pf), np.uint8)
        mk[2] = 1
        items.append((dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X, pt_fixed=qf,
                           obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv), mk))
    raw = run(items, huber=1.0)
    assert len(out) == 2
    for (sv, hp, hq), sc, (Hu, bu, kept, mpts, res), (rH, rb, rk, rl, _) in zip(built_, scs, out, raw):
        eH, eb = marginal_to_user_units(rH, rb, 0.7)
        assert res.status == 0 and res.dropped_pivots == 0
        assert np.array_equal(Hu, eH) and np.array_equal(bu, eb) and np.abs(Hu).max() > 0
        n_pose = len(sc["pose_fixed"])
        assert kept == [int(hp[j]) for j in range(3, n_pose)] and Hu.shape == (6 * len(kept),) * 2
        assert mpts == [int(hq[i]) for i in range(20)] and res.n_marg_pt == 20
