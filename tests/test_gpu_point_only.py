"""GPU tests of the point-only solve (ba_point_only: every pose fixed, a team of lanes per
landmark, the whole LM loop of every landmark in one launch) against the CPU reference of
tests/point_only_ref.py — a loop of one-landmark oracle problems — with the project's
tolerances (assert_same_trajectory of test_gpu_full_batch.py): identical status per row,
lambda within 1e-12, cost and trial cost within 1e-7 relative, final points within 1e-8
absolute in scaled units.  Every test runs at both team widths (8 and 16 lanes)."""
import numpy as np
import pytest

import point_only_ref as R
from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaProblem, Camera, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, Options,
                                                 SolverType, point_only, point_only_team)
from test_gpu_full_batch import assert_same_trajectory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(built):
    p = BaProblem(0)
    yield p
    p.close()


@pytest.fixture(params=[8, 16], ids=["team8", "team16"])
def team(request):
    default = point_only_team(0)
    assert point_only_team(request.param) == request.param
    yield request.param
    point_only_team(default)


def run(handle, pr, opt_kw=R.DEFAULT, X=None, tri=None, cap=None, sel=None):
    """point_only on the landmarks `sel` (default all) of a scaled problem"""
    n_pt = pr["pt_X"].shape[0]
    X = pr["pt_X"] if X is None else X
    cam, pose, pt, uv = pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"]
    if sel is not None:
        sel = np.asarray(sel)
        new_of = np.full(n_pt, -1, np.int64)
        new_of[sel] = np.arange(sel.size)
        # the observations of a landmark keep their order; the landmarks take the order of sel
        keep = np.nonzero(new_of[pt] >= 0)[0]
        cam, pose, pt, uv = cam[keep], pose[keep], new_of[pt[keep]], uv[keep]
        X = X[sel]
        tri = None if tri is None else np.asarray(tri)[sel]
    return point_only(handle, pr["cam_intr"], pr["cam_T"], pr["pose_T"], X, cam, pose, pt, uv,
                      make_options(**opt_kw), triangulate=tri, cap=cap)


def check_landmark(X, res, rows, k, want):
    """landmark k of a call against its reference `want`"""
    assert res[k].status == 0
    assert res[k].n_iter == want["n_iter"] == res[k].n_rows == len(rows[k]), (k, res[k].n_iter, want["n_iter"])
    assert bool(res[k].converged) == want["converged"], k
    assert_same_trajectory(rows[k], want["rows"])
    assert np.abs(X[k] - want["X"]).max() < 1e-8, k
    last = [r for r in want["rows"] if r.iteration_status != 2]
    if last:
        assert abs(res[k].cost - last[-1].trial_cost) <= 1e-7 * abs(last[-1].trial_cost)
    assert res[k].dropped_pivots == 0


def bits(X, res, rows=None):
    out = [np.asarray(X).view(np.uint64).ravel(),
           np.array([[r.n_iter, r.converged, r.n_rows, r.status, r.n_behind, r.dropped_pivots] for r in res]).ravel(),
           np.array([[r.cost0, r.cost] for r in res]).view(np.uint64).ravel()]
    if rows is not None:
        out.append(np.array([[getattr(r, f) for f in R.ROW_FIELDS] for rr in rows for r in rr],
                            float).view(np.uint64).ravel())
    return np.concatenate([o.astype(np.uint64) for o in out])


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("gn", [False, True], ids=["lm", "gauss_newton"])
def test_trajectory_of_every_landmark(handle, team, stereo, gn):
    pr, ref = R.cached(stereo, gauss_newton=gn)
    X, res, rows = run(handle, pr, dict(R.DEFAULT, gauss_newton=gn))
    assert len(ref) == 40
    for i in range(40):
        check_landmark(X, res, rows, i, ref[i])
    if not gn:
        assert len({int(r.n_iter) for r in res}) >= 5     # the teams of a wave stop at different iterations
        assert sum(any(r.iteration_status == 2 for r in rr) for rr in rows) * 3 >= 40


def test_team_edges(handle, team):
    """2, 3, w-1, w, w+1, 2w, 2w+1 observations for both widths in one call, and calls of 1, 3
    and one more / one less than the landmarks a wave holds."""
    pr, ref = R.cached_edges()
    n = len(R.EDGE_COUNTS)
    assert np.bincount(pr["obs_pt"]).tolist() == list(R.EDGE_COUNTS)
    per_wave = 64 // team
    for n_pt in sorted({n, 1, 3, per_wave + 1, per_wave - 1}):
        sel = np.roll(np.arange(n), -n_pt)[:n_pt]
        X, res, rows = run(handle, pr, sel=sel)
        for k, i in enumerate(sel):
            check_landmark(X, res, rows, k, ref[int(i)])
    for i in range(n):                                   # every landmark alone
        X, res, rows = run(handle, pr, sel=[i])
        check_landmark(X, res, rows, 0, ref[i])


def test_empty_landmark_between_two_regular_ones(handle, team):
    pr, _ = R.cached(True)
    odd = np.array([1.5, -0.0, 1e-310])
    X3 = np.stack([pr["pt_X"][4], odd, pr["pt_X"][9]])
    m4, m9 = pr["obs_pt"] == 4, pr["obs_pt"] == 9
    keep = m4 | m9
    pt = np.where(pr["obs_pt"][keep] == 4, 0, 2)
    args = (pr["cam_intr"], pr["cam_T"], pr["pose_T"])
    obs = (pr["obs_cam"][keep], pr["obs_pose"][keep])
    X, res, rows = point_only(handle, *args, X3, *obs, pt, pr["obs_uv"][keep], make_options(**R.DEFAULT))
    assert [int(r.status) for r in res] == [0, 2, 0]
    assert np.array_equal(X[1].view(np.uint64), odd.view(np.uint64))
    assert res[1].n_iter == 0 and res[1].n_rows == 0 and rows[1] == []
    Xw, resw, rowsw = point_only(handle, *args, X3[[0, 2]], *obs, np.where(pt == 0, 0, 1), pr["obs_uv"][keep],
                                 make_options(**R.DEFAULT))
    assert np.array_equal(bits(X[[0, 2]], [res[0], res[2]], [rows[0], rows[2]]), bits(Xw, resw, rowsw))
    # the empty landmark wins over a non-finite value and over a triangulation request
    X3[1, 0] = np.nan
    _, res, _ = point_only(handle, *args, X3, *obs, pt, pr["obs_uv"][keep], make_options(**R.DEFAULT),
                           triangulate=[0, 1, 0])
    assert [int(r.status) for r in res] == [0, 2, 0]


def test_one_observation_landmark(handle, team):
    pr, _ = R.cached(False)
    k = np.nonzero(pr["obs_pt"] == 3)[0][:1]
    X, res, _ = point_only(handle, pr["cam_intr"], pr["cam_T"], pr["pose_T"], pr["pt_X"][[3]], pr["obs_cam"][k],
                           pr["obs_pose"][k], [0], pr["obs_uv"][k], make_options(**R.DEFAULT))
    assert res[0].status == 0 and np.isfinite(X).all()
    assert np.isfinite([res[0].cost0, res[0].cost]).all() and res[0].cost <= res[0].cost0


def test_same_bits_alone_twice_and_permuted(handle, team):
    pr, _ = R.cached(True)
    X, res, rows = run(handle, pr)
    X2, res2, rows2 = run(handle, pr)
    assert np.array_equal(bits(X, res, rows), bits(X2, res2, rows2))
    for i in (0, 7, 22, 39):
        Xa, ra, rwa = run(handle, pr, sel=[i])
        assert np.array_equal(bits(Xa, ra, rwa), bits(X[[i]], [res[i]], [rows[i]])), i
    perm = np.random.default_rng(5).permutation(40)
    Xp, rp, rwp = run(handle, pr, sel=perm)
    assert np.array_equal(bits(Xp, rp, rwp), bits(X[perm], [res[i] for i in perm], [rows[i] for i in perm]))


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_triangulation_and_the_refinement_after_it(handle, team, stereo):
    pr, ref = R.cached(stereo, triangulated=True)
    want = R.triangulate_reference(pr)
    nan = np.full_like(pr["pt_X"], np.nan)
    X, res, rows = run(handle, pr, dict(R.DEFAULT, max_iter=0), X=nan, tri=np.ones(40, np.uint8))
    assert all(r.status == 0 and r.n_iter == 0 and r.n_behind == 0 for r in res)
    assert np.abs(X - want).max() <= 1e-9 * np.abs(want).max()
    assert (np.abs(X - want) <= 1e-9 * np.linalg.norm(want, axis=1)[:, None]).all()
    X, res, rows = run(handle, pr, X=nan, tri=np.ones(40, np.uint8))
    for i in range(40):
        check_landmark(X, res, rows, i, ref[i])


def test_mixed_flags_degenerate_and_behind(handle, team):
    pr, _ = R.cached(True)
    X0, res0, rows0 = run(handle, pr)
    flags = (np.arange(40) % 3 == 0).astype(np.uint8)
    X1, res1, rows1 = run(handle, pr, tri=flags)
    u = np.nonzero(flags == 0)[0]
    assert np.array_equal(bits(X1[u], [res1[i] for i in u], [rows1[i] for i in u]),
                          bits(X0[u], [res0[i] for i in u], [rows0[i] for i in u]))
    assert all(res1[i].status == 0 for i in range(40))
    # one pose through one camera: a single observation, and the same observation twice
    # (exactly rank deficient); both keep their X
    k = np.nonzero(pr["obs_pt"] == 6)[0][:1]
    odd = np.array([[0.25, np.nan, -3.0]])
    for idx in (k, np.concatenate([k, k])):
        X, res, _ = point_only(handle, pr["cam_intr"], pr["cam_T"], pr["pose_T"], odd, pr["obs_cam"][idx],
                               pr["obs_pose"][idx], np.zeros(idx.size, int), pr["obs_uv"][idx],
                               make_options(**R.DEFAULT), triangulate=[1])
        assert res[0].status == 3 and res[0].n_iter == 0
        assert np.array_equal(X.view(np.uint64), odd.view(np.uint64))
    # a point mirrored behind the cameras that see it
    idx = np.nonzero(pr["obs_pt"] == 6)[0]
    T = pr["pose_T"][pr["obs_pose"][idx[0]]]
    Rj, tj = T[:9].reshape(3, 3), T[9:]
    Xb = Rj @ pr["pt_X"][6] + tj
    Xb[2] = -Xb[2]
    Xw = (Rj.T @ (Xb - tj)).reshape(1, 3)
    X, res, _ = point_only(handle, pr["cam_intr"], pr["cam_T"], pr["pose_T"], Xw, pr["obs_cam"][idx],
                           pr["obs_pose"][idx], np.zeros(idx.size, int), pr["obs_uv"][idx],
                           make_options(max_iter=0))
    assert res[0].status == 0 and res[0].n_behind > 0
    assert np.array_equal(X, Xw)


def test_status_1_leaves_the_others_untouched(handle, team):
    pr, _ = R.cached(True)
    X0, res0, rows0 = run(handle, pr)
    bad = dict(pr)
    bad["pose_T"] = np.concatenate([pr["pose_T"], pr["pose_T"][:1]])
    bad["pose_T"][-1, 4] = np.inf                  # a ninth pose, used by landmark 5 only
    bad["obs_pose"] = pr["obs_pose"].copy()
    bad["obs_pose"][np.nonzero(pr["obs_pt"] == 5)[0][2]] = 8
    X1, res1, rows1 = run(handle, bad)
    assert res1[5].status == 1 and res1[5].n_iter == 0 and rows1[5] == []
    assert np.array_equal(X1[5], pr["pt_X"][5])
    u = [i for i in range(40) if i != 5]
    assert np.array_equal(bits(X1[u], [res1[i] for i in u], [rows1[i] for i in u]),
                          bits(X0[u], [res0[i] for i in u], [rows0[i] for i in u]))
    # a non-finite point is status 1 as well, unless it is triangulated
    Xn = pr["pt_X"].copy()
    Xn[11, 1] = np.nan
    _, res2, _ = run(handle, pr, X=Xn)
    assert [int(r.status) for r in res2] == [1 if i == 11 else 0 for i in range(40)]
    _, res3, _ = run(handle, pr, X=Xn, tri=(np.arange(40) == 11).astype(np.uint8))
    assert all(r.status == 0 for r in res3)


def test_zero_iterations_change_nothing(handle, team):
    pr, _ = R.cached(True)
    X, res, rows = run(handle, pr, dict(max_iter=0))
    assert np.array_equal(X.view(np.uint64), pr["pt_X"].view(np.uint64))
    assert all(r.status == 0 and r.n_iter == 0 and r.converged == 1 and r.n_rows == 0 for r in res)
    assert rows is None
    assert all(r.cost0 == r.cost > 0 for r in res)


def _solver_for(cls, sc):
    s = cls(0)
    for c in range(sc["intr"].shape[0]):
        add = s.RegisterCamera if cls is FullBundleAdjustmentSolverRefactor else s.AddCamera
        add(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    poses, pts = sc["T_wc_init"].copy(), sc["X_init"].copy()
    hp, hq = s.AddPoseArray(poses), s.AddPointArray(pts)
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for q in np.nonzero(sc["pt_fixed"])[0]:
        s.MakePointFixed(int(hq[q]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    return s, poses, pts, hq


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor],
                         ids=["solver", "refactor"])
def test_facades_equal_the_raw_call_and_a_solve_follows(handle, cls):
    sc = scenes.synthetic_ba_scene(8, 40, 5, True, seed=11, pixel_sigma=0.5)
    sc["pt_fixed"] = sc["pt_fixed"].copy()
    sc["pt_fixed"][[3, 30]] = True
    sc["X_init"] = sc["X_init"].copy()
    sc["X_init"][17] = np.nan                          # triangulated below
    opt = Options()
    opt.iteration_handle.max_num_iterations = 12
    opt.solver_type = SolverType.LEVENBERG_MARQUARDT
    s, poses, pts, hq = _solver_for(cls, sc)
    poses_before = poses.copy()
    res = s.SolvePointsOnly(opt, triangulate=[int(hq[17])])
    # the raw call on the arrays the facade converts (its own host arrays, cameras by group)
    s2, _, _, _ = _solver_for(cls, sc)
    intr, camT, T_jw, X, pf, qf, ocam, opose, opt_pt, ouv = s2._host_arrays()
    sel = np.nonzero(qf == 0)[0]
    new_of = np.full(40, -1)
    new_of[sel] = np.arange(sel.size)
    keep = new_of[opt_pt] >= 0
    Xr, rr, _ = point_only(handle, intr, camT, T_jw, X[sel], ocam[keep], opose[keep], new_of[opt_pt[keep]],
                           ouv[keep], opt.to_c(), triangulate=(sel == 17).astype(np.uint8), cap=0)
    assert len(res) == len(rr) == 38 and all(r.status == 0 for r in res)
    assert np.array_equal(bits(np.zeros(3), res), bits(np.zeros(3), rr))
    assert np.array_equal(pts[sel], Xr * 100.0)
    assert np.array_equal(pts[[3, 30]], sc["X_init"][[3, 30]])       # fixed points stay
    assert np.array_equal(poses, poses_before)                        # and every pose
    # a Solve after it equals the Solve of a fresh solver given the same values
    sc3 = dict(sc, X_init=pts.copy())
    s3, poses3, pts3, _ = _solver_for(cls, sc3)
    opt.iteration_handle.max_num_iterations = 4
    s.Solve(opt)
    s3.Solve(opt)
    assert np.array_equal(poses, poses3) and np.array_equal(pts, pts3)
    assert not np.array_equal(poses, poses_before)
