"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle
on the same seeded inputs, stage by stage and over the whole LM loop.

Tolerances (fp64): the GPU and the oracle differ only in floating-point
summation order, so per-block results must agree to ~1e-11 relative; the
north-star acceptance bound for final poses / points is 1e-4 relative.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import BaProblem
from oracle import oracle_py as O
from split_cases import ragged_duplicate_scene

pytestmark = pytest.mark.gpu

RTOL_BLOCK = 1e-10     # per-block relative tolerance (max-norm of the block)
RTOL_FINAL = 1e-4      # north_star: final poses / points within 1e-4 rel


def make_gpu(pr, rank=0, world=1):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"],
                       pr["obs_uv"])
    if world > 1:
        p.set_shard(rank, world)
    p.finalize()
    return p


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() / den


def pose_errors(P, Q):
    """SURVEY §8(d) acceptance metrics for (n,12) pose arrays {R row-major, t}:
    max rotation angle between the two rotations [rad], max |dt| / |t|."""
    P, Q = np.asarray(P).reshape(-1, 12), np.asarray(Q).reshape(-1, 12)
    Ra, Rb = P[:, :9].reshape(-1, 3, 3), Q[:, :9].reshape(-1, 3, 3)
    D = Ra @ np.transpose(Rb, (0, 2, 1))
    # angle from the skew part (accurate near zero, where arccos is not)
    w = np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0],
                  D[:, 1, 0] - D[:, 0, 1]], axis=1) * 0.5
    ang = np.arcsin(np.clip(np.linalg.norm(w, axis=1), 0.0, 1.0))
    dt = np.linalg.norm(P[:, 9:] - Q[:, 9:], axis=1)
    tn = np.maximum(np.linalg.norm(Q[:, 9:], axis=1), 1e-300)
    return ang.max(), (dt / tn).max()


def blockwise_relerr(a, b):
    """max over leading index of |a-b|_max / |b|_max (blocks with b == 0 must
    be exactly 0 in a)."""
    a = np.asarray(a).reshape(a.shape[0], -1)
    b = np.asarray(b).reshape(b.shape[0], -1)
    den = np.abs(b).max(axis=1)
    num = np.abs(a - b).max(axis=1)
    z = den == 0
    assert (num[z] == 0).all()
    return (num[~z] / den[~z]).max() if (~z).any() else 0.0


def small_scene(kind):
    if kind == "c1":
        return scenes.test_ba_scene()
    if kind == "mono":
        return scenes.synthetic_ba_scene(24, 1500, 10, False, seed=11)
    if kind == "stereo":
        return scenes.synthetic_ba_scene(40, 3000, 5, True, seed=12)
    raise ValueError(kind)


@pytest.fixture(scope="module", params=["c1", "mono", "stereo"])
def pair(request, built):
    sc = small_scene(request.param)
    pr = scenes.scaled_problem(sc)
    return pr, make_gpu(pr), O.Oracle(pr)


def test_cost(pair):
    pr, g, o = pair
    assert relerr(g.stage_cost(), o.cost()) < 1e-12


def test_linearize_blocks(pair):
    pr, g, o = pair
    lam, hub = 3.7, 1.0
    o.linearize(hub)
    o.damp_invert(lam)
    g.stage_linearize(lam, hub)
    A, a = g.get_A()
    oA, oa = o.get_A()
    assert blockwise_relerr(A, oA) < RTOL_BLOCK
    assert blockwise_relerr(a, oa) < RTOL_BLOCK
    Cm, b = g.get_C()
    oC, ob = o.get_C()
    assert blockwise_relerr(Cm, oC) < RTOL_BLOCK
    assert blockwise_relerr(b, ob) < RTOL_BLOCK
    Ci, cb = g.get_Cinv()
    oCi, ocb = o.get_Cinv()
    # inverse of a 3x3 block: relative to the block's own scale, conditioning
    # of C_i enters (well below 1e6 here)
    assert blockwise_relerr(Ci, oCi) < 1e-7
    assert blockwise_relerr(cb, ocb) < 1e-7
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    assert len(pi) == len(opi)
    key = np.lexsort((pj, pi))
    okey = np.lexsort((opj, opi))
    assert (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    assert blockwise_relerr(W[key], oW[okey]) < RTOL_BLOCK


def test_schur_solve_backsub(pair):
    pr, g, o = pair
    lam, hub = 0.5, 1.0
    o.linearize(hub)
    o.damp_invert(lam)
    o.schur()
    g.stage_linearize(lam, hub)
    g.stage_schur()
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9
    assert relerr(rhs, orhs) < 1e-9
    o.solve_reduced()
    o.backsub()
    g.stage_solve_reduced()
    g.stage_backsub_update()
    x, y = g.get_xy()
    ox, oy = o.get_xy()
    # x solves S x = rhs: compare through the residual and directly
    n6 = S.shape[0]
    res = np.abs(oS @ x.reshape(-1) - orhs).max() / np.abs(orhs).max()
    assert res < 1e-8
    assert relerr(x, ox) < 1e-6
    assert relerr(y, oy) < 1e-6
    # trial parameters, model change, step norms
    o.backup()
    o.update()
    ocost = o.cost()
    omodel = o.model_change()
    osp, osq = o.step_norms()
    cost, model, sp, sq = g.stage_scalars()
    assert relerr(cost, ocost) < 1e-9
    assert relerr(model, omodel) < 1e-6
    assert relerr(sp, osp) < 1e-6 and relerr(sq, osq) < 1e-6
    g.stage_commit(False)
    o.revert()
    assert relerr(g.stage_cost(), o.cost()) < 1e-12


@pytest.mark.parametrize("kind", ["c1", "mono", "stereo"])
def test_lm_trajectory(kind, built):
    """Whole LM loop: same accept/reject sequence, same lambda sequence,
    costs to 1e-8, final parameters far inside the 1e-4 acceptance bound."""
    sc = small_scene(kind)
    pr = scenes.scaled_problem(sc)
    n_it = 25
    g = make_gpu(pr)
    o = O.Oracle(pr)
    rows, conv = g.solve(make_options(max_iter=n_it, thr_step=1e-7,
                                        thr_cost=1e-7))
    orows, oconv = o.solve(O.make_options(max_iter=n_it, thr_step=1e-7,
                                          thr_cost=1e-7))
    assert len(rows) == len(orows) and conv == oconv
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, k
        assert relerr(a.damping_term, b.damping_term) < 1e-12, k
        assert relerr(a.trial_cost, b.trial_cost) < 1e-7, k
        assert relerr(a.cost, b.cost) < 1e-7, k
        assert relerr(a.abs_step, b.abs_step) < 1e-5, k
    P, oP = g.get_poses(), o.get_poses()
    X, oX = g.get_points()[0], o.get_points()
    assert relerr(P, oP) < RTOL_FINAL * 1e-2
    assert relerr(X, oX) < RTOL_FINAL * 1e-2
    # the north-star metrics proper: rotation angle [rad], |dt|/|t|, |dX|/|X|
    ang, dt = pose_errors(P, oP)
    dX = (np.linalg.norm(X - oX, axis=1) / np.maximum(np.linalg.norm(oX, axis=1), 1e-300)).max()
    assert ang < RTOL_FINAL * 1e-2 and dt < RTOL_FINAL * 1e-2 and dX < RTOL_FINAL * 1e-2


def test_converges_to_truth(built):
    """Noise-free scene: the HIP solver must reach the ground truth."""
    sc = scenes.synthetic_ba_scene(20, 800, 5, True, seed=3)
    pr = scenes.scaled_problem(sc)
    g = make_gpu(pr)
    rows, conv = g.solve(make_options(max_iter=60, thr_step=1e-9,
                                        thr_cost=1e-9))
    X = g.get_points()[0] / 0.01
    err = np.linalg.norm(X - sc["X_true"], axis=1)
    err0 = np.linalg.norm(sc["X_init"] - sc["X_true"], axis=1)
    # the reference's LM (multiplicative damping, sum-of-norms rho) converges
    # slowly; 60 iterations take the cost down by > 100x and the median
    # landmark error from 0.49 m to 0.04 m (the oracle does exactly the same)
    assert rows[-1].cost < 1e-2 * rows[0].cost
    assert np.median(err) < 0.1 * np.median(err0)


def test_edge_cases(built):
    """Never-observed landmark (C_i = 0 -> Cinv = 0), fixed
    landmark, landmark seen by fixed poses only, pose without observations."""
    sc = scenes.synthetic_ba_scene(12, 60, 5, False, seed=5)
    # landmark 0: unobserved; landmark 1: fixed; pose 11: no observations
    keep = (sc["obs_pt"] != 0) & (sc["obs_pose"] != 11)
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][keep]
    sc["pt_fixed"][1] = True
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    lam = 2.0
    o.linearize(1.0); o.damp_invert(lam); o.schur()
    o.solve_reduced(); o.backsub()
    g.stage_linearize(lam, 1.0); g.stage_schur()
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9
    g.stage_solve_reduced(); g.stage_backsub_update()
    Ci, _ = g.get_Cinv()
    assert (Ci[0] == 0).all()            # pseudo-inverse, not NaN
    x, y = g.get_xy()
    ox, oy = o.get_xy()
    assert np.isfinite(x).all() and np.isfinite(y).all()
    assert relerr(x, ox) < 1e-6 and relerr(y, oy) < 1e-6
    jlast = o.N - 1                      # pose 11 -> zero row/col -> x = 0
    assert (x[jlast] == 0).all() and np.abs(ox[jlast]).max() == 0
    rows, _ = g.solve(make_options(max_iter=10, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=10, thr_step=0, thr_cost=0))
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert relerr(a.trial_cost, b.trial_cost) < 1e-7
    assert relerr(g.get_points()[0], o.get_points()) < 1e-6


def test_last_writer_quirk(built):
    """Stereo: B_ji keeps only the LAST-inserted camera's cross term
    (reference :826): reversing the insertion order of the two
    cameras changes W but neither A, C, a nor b."""
    sc = scenes.synthetic_ba_scene(10, 80, 5, True, seed=9)
    pr = scenes.scaled_problem(sc)
    g1 = make_gpu(pr)
    g1.stage_linearize(1.0, 1.0)
    pr2 = dict(pr)
    order = np.lexsort((pr["obs_pt"], -pr["obs_cam"], pr["obs_pose"]))
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        pr2[k] = np.ascontiguousarray(pr[k][order])
    g2, o2 = make_gpu(pr2), O.Oracle(pr2)
    g2.stage_linearize(1.0, 1.0)
    o2.linearize(1.0); o2.damp_invert(1.0)
    A1, a1 = g1.get_A(); A2, a2 = g2.get_A()
    assert relerr(A1, A2) < 1e-12 and relerr(a1, a2) < 1e-12
    _, _, W1 = g1.get_pairs(); pi2, pj2, W2 = g2.get_pairs()
    assert relerr(W1, W2) > 1e-3          # different camera survived
    opi, opj, oW = o2.get_pairs()
    k1, k2 = np.lexsort((pj2, pi2)), np.lexsort((opj, opi))
    assert blockwise_relerr(W2[k1], oW[k2]) < RTOL_BLOCK


def test_dense_spd_solve(built):
    """The MFMA Cholesky alone, incl. non-multiple-of-64 sizes."""
    rng = np.random.default_rng(0)
    g = BaProblem(0)
    for n in (6, 64, 100, 330, 1000):
        Q = rng.standard_normal((n, n))
        A = Q @ Q.T + n * np.eye(n)
        b = rng.standard_normal(n)
        x, ms = g.dense_spd_solve(A, b)
        ref = np.linalg.solve(A, b)
        assert relerr(x, ref) < 1e-10, n


def test_reproducible_bits(built):
    """No floating-point atomics: two runs give bit-identical results."""
    for kind in ("stereo", "c1"):
        pr = scenes.scaled_problem(small_scene(kind))
        outs = []
        for _ in range(3):
            g = make_gpu(pr)
            rows, _ = g.solve(make_options(max_iter=14, thr_step=0,
                                             thr_cost=0))
            outs.append((g.get_poses().copy(), g.get_points()[0].copy(),
                         [r.trial_cost for r in rows]))
        for o in outs[1:]:
            assert (outs[0][0] == o[0]).all()
            assert (outs[0][1] == o[1]).all()
            assert outs[0][2] == o[2]


def test_cost_kernel_record_variants(built):
    """k_cost on the 8-byte {camera|pose, point} records (default) and on the
    16-byte records it falls back to for >= 65 536 cameras / poses
    (BA_COST_WIDE=1 forces them): same cost, equal to the oracle's."""
    import os
    sc = scenes.synthetic_ba_scene(30, 1200, 5, True, seed=23)
    pr = scenes.scaled_problem(sc)
    ref = O.Oracle(pr).cost()
    costs = []
    for flag in ("0", "1"):
        os.environ["BA_COST_WIDE"] = flag
        try:
            costs.append(make_gpu(pr).stage_cost())
        finally:
            os.environ.pop("BA_COST_WIDE", None)
    assert costs[0] == costs[1]
    assert relerr(costs[0], ref) < 1e-12


def test_tail_workgroup_matches_the_level_path(built):
    """k_chol_tail (last levels of the dense solve in one workgroup, default)
    against BA_DENSE_TAIL=0 (every level by its own launches): same x on a
    chain scene (tail of 2 + 1 tiles), on a 7-pose scene whose whole reduced
    system is the tail, and for a dense SPD system."""
    import os
    for sc in (scenes.synthetic_ba_scene(60, 2500, 5, True, seed=21),
               scenes.synthetic_ba_scene(12, 300, 5, False, seed=22)):
        pr = scenes.scaled_problem(sc)
        xs = []
        for flag in ("0", "1"):
            os.environ["BA_DENSE_TAIL"] = flag
            try:
                p = make_gpu(pr)
                p.stage_linearize(10.0, 1.0)
                p.stage_schur()
                p.stage_solve_reduced()
                xs.append(p.get_xy()[0].copy())
            finally:
                os.environ.pop("BA_DENSE_TAIL", None)
        assert np.abs(xs[0]).max() > 0
        assert np.abs(xs[0] - xs[1]).max() <= 1e-9 * np.abs(xs[0]).max()
    rng = np.random.default_rng(4)
    n = 150
    Q = rng.standard_normal((n, 40))
    A = Q @ Q.T + n * np.eye(n)
    b = rng.standard_normal(n)
    g = BaProblem(0)
    x, _ = g.dense_spd_solve(A, b)
    assert np.abs(A @ x - b).max() < 1e-10 * np.abs(b).max() * n


def test_one_stream_iteration_and_dataflow_sweep_equal_their_fallbacks(built):
    """The LM loop of a grouped scene runs on ONE stream (tile reset as a role of
    k_backsub_update, pose-side sums as workgroups of k_scalars); the forward sweep of
    its reduced solve is ONE dataflow launch per level (k_chol_level_flow) and the
    backward sweep ONE dataflow launch (per-tile flags; roles from the block index when
    the grid is resident, from tickets otherwise: BA_DENSE_TICKET=1 forces tickets);
    BA_GRAPH=1 replays the iteration as a captured hipGraph (per-level launches: the
    generation number of the dataflow launches is a kernel argument);
    BA_FORCE_SIDE=1 (side stream with fork / join) and BA_DENSE_FLOW=0 (separate
    diag_trsm / update launches, one backward launch per level) are the paths every
    other problem takes.  Same arithmetic in the same order, so the trajectories must
    agree bit for bit, iteration by iteration."""
    import os
    pr = scenes.scaled_problem(scenes.synthetic_ba_scene(150, 9000, 5, True, seed=33, pixel_sigma=0.3))
    runs = []
    for env in ({}, {"BA_FORCE_SIDE": "1"}, {"BA_DENSE_FLOW": "0"}, {"BA_FORCE_SIDE": "1", "BA_DENSE_FLOW": "0"},
                {"BA_DENSE_TICKET": "1"}, {"BA_GRAPH": "1"}):
        for k, v in env.items():
            os.environ[k] = v
        try:
            g = make_gpu(pr)
            rows, _ = g.solve(make_options(max_iter=10, thr_step=0, thr_cost=0))
        finally:
            for k in env:
                os.environ.pop(k, None)
        runs.append(([(r.iteration_status, r.trial_cost, r.damping_term) for r in rows], g.get_poses().copy(),
                     g.get_points()[0].copy()))
        if not env:
            assert g.get_lin_info()["pose_major_observations"] == 0 and g.get_lin_info()["chunks"] == 0
        assert g.get_dropped_pivots() == 0
    assert len(runs[0][0]) == 10
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert (other[1] == runs[0][1]).all() and (other[2] == runs[0][2]).all()
    # BA_FORCE_SIDE=1 reached its handles (every handle reads the environment at its own
    # ba_create, so a setting does not depend on what ran earlier in the process): the launch
    # counts of timing mode, which covers the kernels of enqueue_iteration.  On one stream an
    # iteration never calls launch_lin_poses (k_scalars sums the pose side) and calls
    # launch_dense_init only while no k_backsub_update has reset the tiles yet, i.e. in the
    # first iteration after lm_begin.  With the knob every iteration calls both once: one
    # k_pose_finalize (and no k_lin_poses: the scene has no pose-major list) and one
    # k_dense_init.  So from the second iteration on the counts stand still without the knob
    # and grow by one per iteration with it.  (Timing mode serialises the streams: these
    # handles are for the counts only.)
    growth = {}
    for env in ({}, {"BA_FORCE_SIDE": "1"}):
        for k, v in env.items():
            os.environ[k] = v
        try:
            g = make_gpu(pr)
        finally:
            for k in env:
                os.environ.pop(k, None)
        g.enable_stage_timing(True)
        g.lm_begin(make_options(max_iter=10, thr_step=0, thr_cost=0))
        seen, done = [], 0
        for n in (1, 2):
            g.lm_iterate(n)
            done += n
            assert g.lm_sync()[1] == done
            km = g.get_kernel_ms(reset=False)
            seen.append({k: km[k][1] for k in ("k_pose_finalize", "k_dense_init", "k_lin_poses")})
        print("launches after 1 and 3 iterations", env, seen)
        assert seen[1]["k_lin_poses"] == 0
        growth[bool(env)] = {k: seen[1][k] - seen[0][k] for k in ("k_pose_finalize", "k_dense_init")}
    later_iterations = 2
    assert growth[False] == {"k_pose_finalize": 0, "k_dense_init": 0}
    assert growth[True] == {"k_pose_finalize": later_iterations, "k_dense_init": later_iterations}


def _compare_solve(pr, iters=6, tol_cost=1e-7, tol_par=1e-6):
    g, o = make_gpu(pr), O.Oracle(pr)
    lam = 3.0
    o.linearize(1.0); o.damp_invert(lam); o.schur()
    g.stage_linearize(lam, 1.0); g.stage_schur()
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9 and relerr(rhs, orhs) < 1e-9
    rows, _ = g.solve(make_options(max_iter=iters, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=iters, thr_step=0, thr_cost=0))
    assert len(rows) == len(orows) == iters
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert relerr(a.trial_cost, b.trial_cost) < tol_cost
    assert relerr(g.get_poses(), o.get_poses()) < tol_par
    assert relerr(g.get_points()[0], o.get_points()) < tol_par
    return g, o


def test_landmarks_seen_by_more_than_128_poses(built):
    """Landmarks with more than kSchurPairs (128) pose pairs leave the LDS
    super-run path: W goes straight to HBM in k_lin_landmarks and their Schur
    triples are summed by k_schur_partial."""
    sc = scenes.hover_scene(150, 12, 1, seed=21)
    # plus a few ordinary landmarks seen by a handful of poses
    pr = scenes.scaled_problem(sc)
    assert np.bincount(pr["obs_pt"]).max() == 150
    _compare_solve(pr, iters=5)


def test_rig_with_more_than_eight_cameras(built):
    """More cameras than the LDS camera table holds (kCamLds = 8): the kernels
    switch to their global-memory camera path."""
    sc = scenes.hover_scene(14, 300, 9, seed=22, visible_frac=0.7)
    _compare_solve(scenes.scaled_problem(sc), iters=5)


def test_ragged_and_duplicate_observations(built):
    """Landmarks with one observation, several observations of one
    (camera, pose, landmark) triple, three cameras: the last-writer rule picks
    the W block, everything else sums."""
    sc = ragged_duplicate_scene()
    pr = scenes.scaled_problem(sc)
    cnt = np.bincount(pr["obs_pt"], minlength=200)
    assert (cnt[:10] == 1).all() and cnt[10] == 0
    _compare_solve(pr, iters=5, tol_par=1e-5)


def test_all_points_fixed_and_single_free_pose(built):
    """No optimisable landmark (structure-less pose refinement through the
    full solver) and the smallest reduced system (one free pose)."""
    sc = scenes.hover_scene(6, 80, 2, seed=24)
    sc["pt_fixed"][:] = True
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    rows, _ = g.solve(make_options(max_iter=5, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=5, thr_step=0, thr_cost=0))
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert relerr(a.trial_cost, b.trial_cost) < 1e-7
    assert relerr(g.get_poses(), o.get_poses()) < 1e-6
    sc = scenes.hover_scene(3, 50, 1, seed=25, n_fixed=2)
    _compare_solve(scenes.scaled_problem(sc), iters=5)


def test_all_poses_fixed_and_no_observations(built):
    """Degenerate sizes: no optimisable pose (the reduced system is empty, only
    the landmarks move) and no observation at all (nothing moves; the control
    step sees a 0/0 gain ratio exactly like the oracle)."""
    sc = scenes.hover_scene(5, 60, 2, seed=26)
    sc["pose_fixed"][:] = True
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    rows, _ = g.solve(make_options(max_iter=5, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=5, thr_step=0, thr_cost=0))
    assert len(rows) == len(orows)
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert relerr(a.trial_cost, b.trial_cost) < 1e-7
    assert relerr(g.get_points()[0], o.get_points()) < 1e-6
    assert np.array_equal(g.get_poses(), pr["pose_T"])
    sc = scenes.hover_scene(4, 20, 1, seed=27)
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][:0]
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    rows, _ = g.solve(make_options(max_iter=3, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=3, thr_step=0, thr_cost=0))
    assert [r.iteration_status for r in rows] == [r.iteration_status for r in orows]
    assert np.array_equal(g.get_points()[0], pr["pt_X"])
    assert np.array_equal(g.get_poses(), pr["pose_T"])


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_structures(seed, built):
    """Randomised visibility graphs (dense to very sparse), pose / landmark
    counts, camera counts, fixed poses and fixed landmarks: the reduced system,
    three LM iterations and the final parameters must match the oracle."""
    rng = np.random.default_rng(1000 + seed)
    n_pose = int(rng.integers(3, 70))
    n_pt = int(rng.integers(20, 400))
    n_cam = int(rng.integers(1, 4))
    frac = float(rng.choice([0.05, 0.15, 0.4, 0.9]))
    sc = scenes.hover_scene(n_pose, n_pt, n_cam, seed=2000 + seed,
                            n_fixed=int(rng.integers(1, max(2, n_pose // 3))),
                            visible_frac=frac)
    sc["pt_fixed"][rng.uniform(size=n_pt) < 0.1] = True
    if sc["obs_pt"].size == 0:
        pytest.skip("empty draw")
    _compare_solve(scenes.scaled_problem(sc), iters=3, tol_par=1e-5)


@pytest.mark.parametrize("stereo", [False, True])
def test_minimiser_matches_an_independent_least_squares_solver(stereo, built):
    """INDEPENDENT (non-restatement) check of the full bundle-adjustment path: with the robust
    weight off (Huber threshold far above every residual) the solver's fixed point is the
    minimiser of the sum of squared reprojection errors.  scipy.optimize.least_squares
    (trust-region reflective, finite-difference Jacobian of a plain numpy projection written
    here, its own pose parametrisation) started from the same values must end in the same
    minimum: squared-error sums equal to 1e-6 relative, poses and points to 1e-4 of the scene
    scale (the LM loop with its thresholds off ends in an accept / reject cycle at its noise
    floor: 5e-8 / 6e-5 on the mono scene, 1e-10 / 1e-6 on the stereo scene).
    Neither the oracle nor any analytic Jacobian of this repository takes part."""
    from scipy.optimize import least_squares
    sc = scenes.synthetic_ba_scene(8, 70, 5, stereo, seed=91, pixel_sigma=0.5, pose_noise=0.01, point_noise=0.03)
    pr = scenes.scaled_problem(sc)
    intr, camT = pr["cam_intr"], pr["cam_T"]
    T0, X0 = pr["pose_T"].copy(), pr["pt_X"].copy()
    pf, xf = pr["pose_fixed"].astype(bool), pr["pt_fixed"].astype(bool)
    oc, op, ox, uv = pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"]
    free_p, free_x = np.flatnonzero(~pf), np.flatnonzero(~xf)

    def rodrigues(w):
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        if th < 1e-12:
            return np.eye(3) + K
        return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)

    def unpack(z):
        T, X = T0.copy(), X0.copy()
        for a, j in enumerate(free_p):   # T_j = [exp(w) R0 | t0 + v]: any smooth chart has the same minimiser
            w, v = z[6 * a:6 * a + 3], z[6 * a + 3:6 * a + 6]
            T[j, :9] = (rodrigues(w) @ T0[j, :9].reshape(3, 3)).reshape(9)
            T[j, 9:] = T0[j, 9:] + v
        X[free_x] = X0[free_x] + z[6 * len(free_p):].reshape(-1, 3)
        return T, X

    def residuals(z):
        T, X = unpack(z)
        R = T[op, :9].reshape(-1, 3, 3)
        Xj = np.einsum("kab,kb->ka", R, X[ox]) + T[op, 9:]
        Rc = camT[oc, :9].reshape(-1, 3, 3)
        Xc = np.einsum("kab,kb->ka", Rc, Xj) + camT[oc, 9:]
        u = intr[oc, 0] * Xc[:, 0] / Xc[:, 2] + intr[oc, 2]
        v = intr[oc, 1] * Xc[:, 1] / Xc[:, 2] + intr[oc, 3]
        return np.concatenate([u - uv[:, 0], v - uv[:, 1]])

    z0 = np.zeros(6 * len(free_p) + 3 * len(free_x))
    ls = least_squares(residuals, z0, method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    T_ls, X_ls = unpack(ls.x)
    g = make_gpu(pr)
    g.solve(make_options(max_iter=80, thr_step=0, thr_cost=0, huber=1e9))
    Tg, Xg = g.get_poses(), g.get_points()[0]
    # squared-error sum at the solver's result, evaluated by the numpy projection above
    def sse(T, X):
        R = T[op, :9].reshape(-1, 3, 3)
        Xj = np.einsum("kab,kb->ka", R, X[ox]) + T[op, 9:]
        Xc = np.einsum("kab,kb->ka", camT[oc, :9].reshape(-1, 3, 3), Xj) + camT[oc, 9:]
        u = intr[oc, 0] * Xc[:, 0] / Xc[:, 2] + intr[oc, 2]
        v = intr[oc, 1] * Xc[:, 1] / Xc[:, 2] + intr[oc, 3]
        return float(((u - uv[:, 0]) ** 2 + (v - uv[:, 1]) ** 2).sum())
    s_gpu, s_ls, s_0 = sse(Tg, Xg), sse(T_ls, X_ls), sse(T0, X0)
    assert s_ls < 0.5 * s_0 and s_gpu < 0.5 * s_0            # both moved well away from the start
    assert abs(s_gpu - s_ls) <= 1e-6 * s_ls, (s_gpu, s_ls)
    scale = np.abs(X0).max()
    assert np.abs(Tg - T_ls).max() <= 1e-4 * scale, np.abs(Tg - T_ls).max()
    assert np.abs(Xg - X_ls).max() <= 1e-4 * scale, np.abs(Xg - X_ls).max()


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_wide_window_scenes(seed, built):
    """Randomised scenes on the round-3 paths: windows of 11..20 poses (mono) or 11..16
    (stereo), 0-30 % of the observations dropped, some landmarks fixed, group sizes around
    the 24-landmark threshold (so that wide groups, masked wide groups, pose-group classes and
    the triple list all occur in one problem): reduced system, four LM iterations and the
    final parameters against the oracle."""
    rng = np.random.default_rng(5000 + seed)
    stereo = bool(rng.integers(0, 2))
    window = int(rng.integers(11, 17 if stereo else 21))
    n_pose = int(rng.integers(window + 8, 70))
    n_pt = int(rng.integers(600, 4000))
    sc = scenes.synthetic_ba_scene(n_pose, n_pt, window, stereo, seed=6000 + seed,
                                   pixel_sigma=float(rng.choice([0.0, 0.3])),
                                   dropout=float(rng.choice([0.0, 0.1, 0.3])))
    sc["pt_fixed"][rng.uniform(size=sc["pt_fixed"].shape[0]) < 0.05] = True
    _compare_solve(scenes.scaled_problem(sc), iters=4, tol_par=1e-5)


def test_stereo_windows_beyond_the_slot_limit_of_the_groups(built):
    """20 stereo views per landmark = 40 observations: more than the 32 pattern slots of a
    covisibility group (one lane per slot in k_lin_grp), so nothing is grouped although the
    20 poses would fit: pose-group classes / chunk kernels, against the oracle."""
    sc = scenes.synthetic_ba_scene(44, 1800, 20, True, seed=71, pixel_sigma=0.2)
    pr = scenes.scaled_problem(sc)
    g, o = _compare_solve(pr, iters=5, tol_par=1e-5)
    assert g.get_schur_info()["grouped_landmarks"] < 0.2 * g.M_global


@pytest.mark.parametrize("window", [15, 16, 20])
def test_wide_windows_around_the_slot_limit(window, built):
    """A landmark seen by d poses touches d(d+1)/2 blocks of S: d = 15 (120
    blocks) still fits the 128 register-resident slots of a super-run, d = 16
    (136) and d = 20 (210) go through the global triple list."""
    sc = scenes.synthetic_ba_scene(48, 700, window, False, seed=30 + window)
    _compare_solve(scenes.scaled_problem(sc), iters=4, tol_par=1e-5)


def test_gauss_newton_mode_of_the_refactored_solver(built):
    """ba_options.gauss_newton (reference ..._refactor.cpp:976-982): every step
    is accepted with lambda fixed at initial_lambda; the Python
    FullBundleAdjustmentSolverRefactor facade selects it from
    options.solver_type."""
    from bundle_adjustment_solver_amd import (FullBundleAdjustmentSolverRefactor,
                                              Options, SolverType, Summary)
    sc = scenes.synthetic_ba_scene(16, 400, 5, True, seed=77, pose_noise=0.02,
                                   point_noise=0.05)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    kw = dict(max_iter=6, thr_step=0, thr_cost=0, lambda0=1e-3, gauss_newton=True)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert len(rows) == len(orows) == 6
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status == 0
        assert a.damping_term == b.damping_term == pytest.approx(1e-3)
        assert relerr(a.cost, b.cost) < 1e-7
    assert relerr(g.get_poses(), o.get_poses()) < 1e-6
    assert relerr(g.get_points()[0], o.get_points()) < 1e-6
    assert rows[-1].cost < 0.5 * rows[0].cost       # GN makes progress on this scene
    # facade: GAUSS_NEWTON (default of Options) vs LEVENBERG_MARQUARDT
    from bundle_adjustment_solver_amd import Camera
    outs = {}
    for st in (SolverType.GAUSS_NEWTON, SolverType.LEVENBERG_MARQUARDT):
        s = FullBundleAdjustmentSolverRefactor()
        for c in range(sc["intr"].shape[0]):
            s.RegisterCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
        poses = [sc["T_wc_init"][k].copy() for k in range(16)]
        pts = [sc["X_init"][k].copy() for k in range(400)]
        for T in poses:
            s.RegisterWorldToBodyPose(T)
        for X in pts:
            s.RegisterWorldPoint(X)
        for k in range(5):
            s.MakePoseFixed(poses[k])
        for c, j, i, uv in zip(sc["obs_cam"], sc["obs_pose"], sc["obs_pt"], sc["obs_uv"]):
            s.AddObservation(int(c), poses[j], pts[i], uv)
        opt = Options()
        opt.solver_type = st
        opt.iteration_handle.max_num_iterations = 5
        opt.trust_region_handle.initial_lambda = 1e-3
        summ = Summary()
        assert s.Solve(opt, summ)
        outs[st] = [i.iteration_status for i in summ.optimization_info_list_]
    assert all(int(v) == 0 for v in outs[SolverType.GAUSS_NEWTON])
    assert any(int(v) == 1 for v in outs[SolverType.LEVENBERG_MARQUARDT])


def test_full_size_configs_properties(built):
    """BASELINE.json sizes, through size-independent properties (the oracle
    needs ~20 s per iteration at C4): C2 converges towards the ground truth of
    its noise-free scene; C4 is bitwise reproducible run to run, accepted steps
    never increase the cost, and one handle re-solved from the same start
    repeats its trajectory."""
    opts = dict(thr_step=0, thr_cost=0)
    # ---- C2: 200 poses / 50 k landmarks / 500 k observations (mono) ----
    sc = scenes.config_scene("C2")
    pr = scenes.scaled_problem(sc)
    g = make_gpu(pr)
    rows, _ = g.solve(make_options(max_iter=40, **opts))
    X0 = pr["pt_X"]
    Xt = sc["X_true"] * 0.01
    e0 = np.linalg.norm(X0 - Xt, axis=1)
    e1 = np.linalg.norm(g.get_points()[0] - Xt, axis=1)
    assert np.median(e1) < 0.1 * np.median(e0)
    assert rows[-1].cost < 1e-2 * rows[0].cost
    for r in rows:
        if r.iteration_status != 2:       # accepted step: rho > 0.25 > 0
            assert r.rho > 0.25
    del g
    # ---- C4: 1000 poses / 500 k landmarks / 5 M observations (stereo) ----
    sc = scenes.config_scene("C4")
    pr = scenes.scaled_problem(sc)
    logs = []
    for _ in range(2):
        g = make_gpu(pr)
        rows, _ = g.solve(make_options(max_iter=6, **opts))
        logs.append([(r.cost, r.damping_term, r.iteration_status, r.trial_cost)
                     for r in rows])
        P, X = g.get_poses().copy(), g.get_points()[0].copy()
        if len(logs) == 1:
            P0, X0 = P, X
        del g
    assert logs[0] == logs[1]                          # bitwise, run to run
    assert np.array_equal(P0, P) and np.array_equal(X0, X)
    costs = [c for c, _, st, _ in logs[0] if st != 2]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


def test_handles_release_their_device_memory(built):
    """create -> finalize -> solve -> destroy cycles must not leak device
    memory (handles own every buffer, incl. the side stream, events, graph)."""
    torch = pytest.importorskip("torch")   # same HIP runtime as libba_hip.so (see _lib)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    sc = scenes.synthetic_ba_scene(30, 4000, 5, True, seed=3)
    pr = scenes.scaled_problem(sc)
    opt = make_options(max_iter=4, thr_step=0, thr_cost=0)
    def cycle():
        g = make_gpu(pr)
        g.solve(opt)
        g.pose_only_mono6(np.random.rand(100, 3).astype(np.float32) + [0, 0, 2],
                          np.random.rand(100, 2).astype(np.float32) * 100, 300, 300,
                          320, 240,
                          np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32),
                          np.ones(100, np.uint8), opt)
        g.close()

    # one-time runtime reservations (code objects, the kernel scratch pool of the
    # HIP queues: ~100 MB once, then constant) happen in the first cycles
    for _ in range(10):
        cycle()
    before = free_bytes()
    for _ in range(25):
        cycle()
    after = free_bytes()
    assert before - after < 16 << 20, (before, after)


def north_star_errors(g, o):
    """SURVEY.md §8(d) acceptance metrics of north_star, per pose / per point:
    max rotation angle [rad], max |dt|/|t|, max |dX|/|X| between the HIP
    solver's and the oracle's CURRENT parameters."""
    P, oP = g.get_poses(), o.get_poses()
    X, oX = g.get_points()[0], o.get_points()
    ang, dt = pose_errors(P, oP)
    dX = (np.linalg.norm(X - oX, axis=1) /
          np.maximum(np.linalg.norm(oX, axis=1), 1e-300)).max()
    return ang, dt, dX


def north_star_errors_with_runaways(g, o, far=1e2):
    """The same metrics with the landmarks that the ALGORITHM drives to infinity set
    apart.  Under the reference's multiplicative damping a few weakly constrained
    landmarks of the large window scenes leave the scene geometrically once lambda
    has fallen (|X| x13 per accepted step; C4: landmark 140739 reaches 1e36 by
    iteration 45 — in the oracle and on the GPU alike,
    test_thresholds_off_runaway_regime_matches_oracle).  Their coordinates are the
    product of dozens of amplifications of roundoff: a relative comparison of THEM
    is meaningless.  `far`: |X| in scaled units (the scenes span < 3).  Returns
    (angle, |dt|/|t|, max |dX|/|X| over the regular landmarks, indices of the
    oracle's run-aways, indices of the GPU's, max |log10 ratio| of their norms)."""
    P, oP = g.get_poses(), o.get_poses()
    X, oX = g.get_points()[0], o.get_points()
    ang, dt = pose_errors(P, oP)
    n, on = np.linalg.norm(X, axis=1), np.linalg.norm(oX, axis=1)
    away_o = np.nonzero(~(on < far))[0]
    away_g = np.nonzero(~(n < far))[0]
    reg = on < far
    dX = (np.linalg.norm(X[reg] - oX[reg], axis=1) / np.maximum(on[reg], 1e-300)).max()
    both = np.intersect1d(away_o, away_g)
    mag = float(np.abs(np.log10(n[both]) - np.log10(on[both])).max()) if both.size else 0.0
    return ang, dt, dX, away_o, away_g, mag


def assert_same_trajectory(rows, orows, rtol_cost=1e-7):
    """Identical accept / reject decisions and lambda sequence, trial costs to
    rtol_cost (relative; floored at 1e-12 of the starting cost, the roundoff
    level a noise-free scene converges to)."""
    assert len(rows) == len(orows)
    floor = 1e-12 * abs(orows[0].cost)
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, k
        assert relerr(a.damping_term, b.damping_term) < 1e-12, k
        assert abs(a.trial_cost - b.trial_cost) <= rtol_cost * abs(b.trial_cost) + floor, k
        assert abs(a.cost - b.cost) <= rtol_cost * abs(b.cost) + floor, k


def test_config_c2_to_convergence_matches_faithful_oracle(built):
    """BASELINE config C2 (mono 200 / 50 k / 500 k) run until the solver's own
    convergence test fires (reference :971-975), against the FAITHFUL oracle
    (restated Eigen pivoted LDLT): same number of iterations, same status and
    lambda sequence, and the north-star metrics per pose / point <= 1e-4."""
    sc = scenes.config_scene("C2")
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    kw = dict(max_iter=80, thr_step=1e-9, thr_cost=1e-9)
    rows, conv = g.solve(make_options(**kw))
    orows, oconv = o.solve(O.make_options(**kw))
    assert conv and oconv and len(rows) >= 25
    assert_same_trajectory(rows, orows)
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    # and the fixed point is the ground truth of the noise-free scene
    Xt = sc["X_true"] * 0.01
    assert np.median(np.linalg.norm(g.get_points()[0] - Xt, axis=1)) < 1e-6


@pytest.mark.parametrize("name,iters", [("C3", 16), ("C4", 14)])
def test_config_c3_c4_trajectories_match_fast_oracle(name, iters, built):
    """BASELINE configs C3 (stereo 500 / 200 k / 2 M) and C4 (stereo 1000 /
    500 k / 5 M, the headline): >= 12 LM iterations against the oracle in
    fast-solve mode (envelope LDL^T, cross-checked against the faithful
    pivoted LDLT in tests/test_oracle_pins.py; the faithful dense factorisation
    needs 17 s per C4 iteration).  Status / lambda sequences identical,
    north-star metrics per pose / point <= 1e-4 after every batch."""
    sc = scenes.config_scene(name)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    o.set_fast_solve(True)
    kw = dict(max_iter=iters, thr_step=0, thr_cost=0)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert len(rows) == iters
    assert_same_trajectory(rows, orows)
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    assert rows[-1].cost < 0.02 * rows[0].cost     # well past the first steps


@pytest.mark.parametrize("name,thr_cost", [("C3", 1e-6), ("C4", 1e-7)])
def test_config_c3_c4_to_the_solvers_own_stop_match_fast_oracle(name, thr_cost, built):
    """BASELINE configs C3 and C4 (the headline) run with the options SURVEY.md
    §8(d) names for them — lambda0 100, ratios 0.33f / 3.0f, Huber 1.0, thresholds
    1e-6f, at most 50 iterations — until the solver's OWN stopping rule ends the
    loop (reference :971-979: average step or cost change below the threshold, or
    the iteration cap), GPU and fast-solve oracle alike: same number of iterations,
    same convergence flag, identical status / lambda sequences, trial costs to 1e-7,
    and the three north-star metrics per pose / per point <= 1e-4 at the end.
    (C4 with threshold_cost_change 1e-7: at 1e-6 the stop is not determined by the
    arithmetic — the cost changes of the C4 trajectory bottom out at 2e-6 around
    iteration 38, i.e. within 2x of the threshold and at a relative 5e-10 of the cost,
    far below the 1e-7 to which any two summation orders of the reduced solve agree;
    the GPU stopped at iteration 40 or ran to the cap of 50 depending on the rounding
    of the 16x16 tile factorisation, the oracle ran to 50.)"""
    sc = scenes.config_scene(name)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    o.set_fast_solve(True)
    kw = dict(max_iter=50, thr_step=1e-6, thr_cost=thr_cost)
    rows, conv = g.solve(make_options(**kw))
    orows, oconv = o.solve(O.make_options(**kw))
    assert len(rows) == len(orows) and conv == oconv, (len(rows), len(orows), conv, oconv)
    assert len(rows) >= 20
    assert_same_trajectory(rows, orows)
    # poses and the regular landmarks: the north-star metrics; the handful of
    # landmarks the algorithm itself sends to infinity (see the helper): the SAME
    # landmarks on both sides, at the same order of magnitude
    ang, dt, dX, away_o, away_g, mag = north_star_errors_with_runaways(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    assert np.array_equal(away_o, away_g), (away_o, away_g)
    assert away_o.size <= 5e-4 * g.M_global and mag < 0.5, (away_o.size, mag)   # C4: 63 of 500 000
    assert g.get_dropped_pivots() == 0


def test_config_c3_pixel_noise_half_px_huber_to_the_solvers_own_stop(built):
    """SURVEY.md §8(d)'s second run at size: C3 with pixel noise sigma = 0.5 px and
    threshold_huber_loss = 0.005 (0.5 px in the solver's 0.01-px units: the robust
    branch of reference :763-768 is taken by most observations at the start and by
    about half of them at the optimum), to the solver's own stop, against the
    fast-solve oracle."""
    sc = scenes.config_scene("C3", pixel_sigma=0.5)
    pr = scenes.scaled_problem(sc)
    huber = 0.005
    w0 = weighted_fraction(pr, huber)
    assert w0 > 0.9
    g, o = make_gpu(pr), O.Oracle(pr)
    o.set_fast_solve(True)
    kw = dict(max_iter=50, thr_step=1e-6, thr_cost=1e-6, huber=huber)
    rows, conv = g.solve(make_options(**kw))
    orows, oconv = o.solve(O.make_options(**kw))
    assert len(rows) == len(orows) and conv == oconv
    assert_same_trajectory(rows, orows)
    ang, dt, dX, away_o, away_g, mag = north_star_errors_with_runaways(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    assert np.array_equal(away_o, away_g) and away_o.size <= 5e-4 * g.M_global and mag < 0.5
    w1 = weighted_fraction(pr, huber, g.get_poses(), g.get_points()[0])
    assert 0.3 < w1 < 0.8, (w0, w1)       # still on the weighted branch at the optimum
    assert rows[-1].cost < 0.2 * rows[0].cost


def test_thresholds_off_runaway_regime_matches_oracle(built):
    """bench.py times with the convergence thresholds off.  Past convergence the
    reference's multiplicative damping (lambda -> 1e-10) lets a weakly constrained
    landmark run away geometrically (landmark 140739 of config C4, seen by poses
    991-995 close to the image row v = cy: |X| grows about 13-fold per accepted step, from
    iteration ~15 on).  The oracle shows exactly this; this test pins the GPU to it on
    the 16-pose tail of C4 that contains the landmark, 320 iterations:
    * while the run-away is representable — until the oracle's average step passes
      1e130, iteration ~120, |X| ~ 1e135 — identical status and lambda sequences, the
      step within half a decade, trial costs to 1e-7 for 40 iterations and 1e-5 after
      (with lambda at its 1e-10 floor the slow modes amplify roundoff: the oracle's OWN
      two solve modes, pivoted LDLT / envelope LDL^T, are 1e-7 apart by iteration 64);
    * beyond (|X| ~ 1e147: the landmark's C_i ~ 1e-293 with a last pivot in the
      denormal range, where Eigen's `|d| <= DBL_MIN -> 0` rule decides between "the
      landmark stops" and "the inverse overflows" on the last bits of a chaotic
      trajectory) no correspondence is meaningful; asserted is what must hold
      anyway: every row is either finite or a SKIPPED step with lambda unchanged
      (the rho = NaN branch of reference :939-953, pinned row for row by
      test_nan_cost_branch_of_the_control_step_matches_oracle), and no pivot of the
      reduced system is dropped before."""
    sc = scenes.pose_window_subscene(scenes.config_scene("C4"), 984, 1000)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    n_it = 320
    kw = dict(max_iter=n_it, thr_step=-1.0, thr_cost=-1.0)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert len(rows) == len(orows) == n_it
    assert max(r.abs_step for r in orows if np.isfinite(r.abs_step)) > 1e100   # the regime is reached
    floor = 1e-12 * abs(orows[0].cost)
    worst = 0.0
    edge = next(k for k, r in enumerate(orows) if r.abs_step > 1e130)
    assert edge > 100
    for k, a in enumerate(rows[edge:], edge):
        if not np.isfinite(a.trial_cost):
            assert a.iteration_status == 2 and a.damping_term == rows[k - 1].damping_term, k
    for k, (a, b) in enumerate(zip(rows[:edge], orows[:edge])):
        assert a.iteration_status == b.iteration_status, k
        assert np.isfinite(a.trial_cost) == np.isfinite(b.trial_cost), k
        assert np.isfinite(a.abs_step) == np.isfinite(b.abs_step), k
        assert a.damping_term == b.damping_term or relerr(a.damping_term, b.damping_term) < 1e-12, k
        if np.isfinite(b.trial_cost):
            assert abs(a.trial_cost - b.trial_cost) <= (1e-7 if k < 40 else 1e-5) * abs(b.trial_cost) + floor, k
            worst = max(worst, abs(a.trial_cost - b.trial_cost) / abs(b.trial_cost))
        if np.isfinite(b.abs_step) and b.abs_step > 0:
            # the run-away step itself: the same order of magnitude (its value is the
            # product of ~100 amplifications of one landmark's roundoff)
            assert abs(np.log10(a.abs_step) - np.log10(b.abs_step)) < 0.5, (k, a.abs_step, b.abs_step)
    print("largest relative trial-cost difference over the first %d iterations: %.2e; largest step "
          "%.2e; first non-finite GPU row: %s"
          % (edge, worst, max(r.abs_step for r in rows if np.isfinite(r.abs_step)),
             next((k for k, r in enumerate(rows) if not np.isfinite(r.trial_cost)), None)))


def nan_observation_problem():
    sc = scenes.synthetic_ba_scene(12, 300, 5, True, seed=7)
    pr = scenes.scaled_problem(sc)
    pr["obs_uv"] = pr["obs_uv"].copy()
    pr["obs_uv"][1234, 0] = np.nan
    return pr


def test_nan_cost_branch_of_the_control_step_matches_oracle(built):
    """rho = NaN fails `rho > 0.25`, `rho > 0.5` and `rho <= 0.25` alike (reference
    :939-953): the step is reverted (SKIPPED), lambda stays, previous_cost advances to
    the NaN trial cost (:1005).  One NaN pixel makes every cost NaN from the start:
    GPU and oracle must log the same rows."""
    pr = nan_observation_problem()
    g, o = make_gpu(pr), O.Oracle(pr)
    kw = dict(max_iter=6, thr_step=-1.0, thr_cost=-1.0)
    rows, conv = g.solve(make_options(**kw))
    orows, oconv = o.solve(O.make_options(**kw))
    assert len(rows) == len(orows) == 6 and conv == oconv
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status == 2
        assert a.damping_term == b.damping_term == 100.0
        assert np.isnan(a.trial_cost) and np.isnan(b.trial_cost)
        assert np.isnan(a.cost) == np.isnan(b.cost)
        assert np.isnan(a.rho) and np.isnan(b.rho)


def weighted_fraction(pr, huber, P=None, X=None):
    """Share of observations on the weighted branch of reference :763-766
    (|r_x| + |r_y| > threshold_huber_loss) at the given parameters (numpy)."""
    P = pr["pose_T"] if P is None else P
    X = pr["pt_X"] if X is None else X
    T = P[pr["obs_pose"]]
    Xij = np.einsum("nij,nj->ni", T[:, :9].reshape(-1, 3, 3), X[pr["obs_pt"]]) + T[:, 9:]
    cT = pr["cam_T"][pr["obs_cam"]]
    Xc = np.einsum("nij,nj->ni", cT[:, :9].reshape(-1, 3, 3), Xij) + cT[:, 9:]
    K = pr["cam_intr"][pr["obs_cam"]]
    r0 = K[:, 0] * Xc[:, 0] / Xc[:, 2] + K[:, 2] - pr["obs_uv"][:, 0]
    r1 = K[:, 1] * Xc[:, 1] / Xc[:, 2] + K[:, 3] - pr["obs_uv"][:, 1]
    return float((np.abs(r0) + np.abs(r1) > huber).mean())


@pytest.mark.parametrize("huber", [0.05, 0.005])
@pytest.mark.parametrize("kind", ["stereo", "mono"])
def test_robust_branch_with_pixel_noise(kind, huber, built):
    """The Huber-like weight w = thr / (|r_x| + |r_y|) (reference :763-768) under
    pixel noise sigma = 0.5 px (SURVEY.md §8d second run): thresholds of 5 px
    (0.05 in the solver's 0.01-px units: every observation weighted at the start,
    none at the end) and 0.5 px (about 60 % still weighted at the optimum).
    Stage blocks, reduced system and an LM trajectory with rejected steps."""
    stereo = kind == "stereo"
    sc = scenes.synthetic_ba_scene(40, 3000, 5 if stereo else 10, stereo,
                                   seed=12 if stereo else 11, pixel_sigma=0.5)
    pr = scenes.scaled_problem(sc)
    assert weighted_fraction(pr, huber) > 0.9
    g, o = make_gpu(pr), O.Oracle(pr)
    lam = 0.7
    o.linearize(huber); o.damp_invert(lam); o.schur()
    g.stage_linearize(lam, huber); g.stage_schur()
    for (a, b) in zip(g.get_A() + g.get_C(), o.get_A() + o.get_C()):
        assert blockwise_relerr(a, b) < RTOL_BLOCK
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    assert blockwise_relerr(W[np.lexsort((pj, pi))], oW[np.lexsort((opj, opi))]) < RTOL_BLOCK
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9 and relerr(rhs, orhs) < 1e-9
    # the weight matters: the unweighted blocks are different
    o.linearize(1.0); o.damp_invert(lam)
    assert relerr(g.get_A()[0], o.get_A()[0]) > 1e-2
    # trajectory from the start
    g, o = make_gpu(pr), O.Oracle(pr)
    kw = dict(max_iter=18, thr_step=0, thr_cost=0, huber=huber)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert_same_trajectory(rows, orows)
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    f_end = weighted_fraction(pr, huber, g.get_poses(), g.get_points()[0])
    if huber < 0.01:
        assert f_end > 0.3          # the weighted branch is live at the optimum
    else:
        assert f_end < 0.05


def test_config_c4_first_iteration_matches_oracle(built):
    """The headline configuration (stereo 1000 / 500 k / 5 M) against the
    FAITHFUL oracle: one LM iteration (about 20 s, nearly all of it in the
    reference-style dense LDLT of the 5970 x 5970 reduced system); the longer
    C4 trajectory is in test_config_c3_c4_trajectories_match_fast_oracle."""
    sc = scenes.config_scene("C4")
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    rows, _ = g.solve(make_options(max_iter=1, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=1, thr_step=0, thr_cost=0))
    assert rows[0].iteration_status == orows[0].iteration_status
    assert relerr(rows[0].trial_cost, orows[0].trial_cost) < 1e-8
    assert relerr(rows[0].model_change, orows[0].model_change) < 1e-7
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)


def test_dropped_pivots_are_reported(built):
    """The reduced system is factorised by Cholesky without pivoting (the
    reference: Eigen's pivoted LDLT with pseudo-inverted D).  Where the two can
    differ — a non-positive pivot — the library counts it: 0 on a regular
    problem, 6 per factorisation for a pose without observations (zero row and
    column of S; both solvers then return x_j = 0, test_edge_cases)."""
    sc = scenes.synthetic_ba_scene(12, 60, 5, False, seed=5)
    pr = scenes.scaled_problem(sc)
    g = make_gpu(pr)
    g.solve(make_options(max_iter=4, thr_step=0, thr_cost=0))
    assert g.get_dropped_pivots() == 0
    keep = sc["obs_pose"] != 11
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][keep]
    pr = scenes.scaled_problem(sc)
    g = make_gpu(pr)
    g.solve(make_options(max_iter=4, thr_step=0, thr_cost=0))
    assert g.get_dropped_pivots() == 6 * 4
    assert g.get_dropped_pivots(reset=True) == 24 and g.get_dropped_pivots() == 0


@pytest.mark.parametrize("stereo", [True, False])
def test_gauge_free_problem_at_the_lambda_floor(stereo, built):
    """No fixed pose and lambda at its floor of 1e-10 (reference :949): the
    reduced system keeps the gauge freedom of the scene (mono: cond(S) ~ 1e13).
    Un-pivoted Cholesky (HIP) and the reference-style pivoted LDLT (oracle) must
    still agree: no dropped pivot, both residuals at roundoff, same trial cost."""
    sc = scenes.synthetic_ba_scene(20, 600, 5 if stereo else 10, stereo, seed=31,
                                   n_fixed=0, pose_noise=0.02, point_noise=0.05)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    lam = 1e-10
    o.linearize(1.0); o.damp_invert(lam); o.schur(); o.solve_reduced(); o.backsub()
    g.stage_linearize(lam, 1.0); g.stage_schur()
    g.get_dropped_pivots(reset=True)
    g.stage_solve_reduced(); g.stage_backsub_update()
    assert g.get_dropped_pivots() == 0
    S, rhs = o.get_S()
    x, _ = g.get_xy()
    ox, _ = o.get_xy()
    assert np.abs(S @ x.reshape(-1) - rhs).max() < 1e-12 * np.abs(rhs).max()
    assert np.abs(S @ ox.reshape(-1) - rhs).max() < 1e-12 * np.abs(rhs).max()
    o.backup(); o.update()
    assert relerr(g.stage_scalars()[0], o.cost()) < 1e-5


@pytest.mark.parametrize("kind", ["stereo", "mono", "c1"])
def test_covisibility_groups_equal_the_super_run_path(kind, built):
    """k_schur_grp (landmarks with identical pose sets as one dense product on
    the matrix cores) against the super-run kernel alone (BA_NO_GROUPS=1): same
    reduced system to roundoff, and the window scenes really take the group path
    (32-wide tiles for the stereo windows of 5 poses, 64-wide for the mono windows
    of 10); the wall scene C1 (pose sets of up to 55 poses) has no group."""
    import os
    pr = scenes.scaled_problem(small_scene(kind))
    out = []
    for flag in ("0", "1"):
        os.environ["BA_NO_GROUPS"] = flag
        try:
            g = make_gpu(pr)
        finally:
            os.environ.pop("BA_NO_GROUPS", None)
        info = g.get_schur_info()
        g.stage_linearize(2.5, 1.0)
        g.stage_schur()
        out.append((info,) + g.get_S())
    (ia, Sa, ra), (ib, Sb, rb) = out
    assert ib["grouped_landmarks"] == 0 and ib["groups32"] == ib["groups64"] == 0
    if kind == "stereo":
        assert ia["groups32"] > 10 and ia["grouped_landmarks"] > 0.8 * g.M
    elif kind == "mono":
        assert ia["groups64"] > 5 and ia["grouped_landmarks"] > 0.8 * g.M
    else:
        assert ia["grouped_landmarks"] < 0.2 * g.M
    assert relerr(Sa, Sb) < 1e-12 and relerr(ra, rb) < 1e-12


@pytest.mark.parametrize("shape,env", [
    ((40, 3000, 5, True), {}),                          # stereo windows of 5: 10 slots, 6 landmarks per wave step
    ((40, 3000, 5, True), {"BA_LIN_STEPS": "2"}),        # several pieces per group, partial last steps
    ((40, 3000, 5, True), {"BA_NO_LINGRP": "1"}),        # the chunk / pose-major kernels on the same plan
    ((30, 2500, 3, True), {"BA_LIN_STEPS": "3"}),        # 6 slots: the 7-landmark cap, 42 of 64 lanes
    ((30, 2500, 2, False), {}),                         # mono pairs: 2 slots, 14 of 64 lanes
    ((24, 1500, 10, False), {"BA_LIN_STEPS": "1"}),      # mono windows of 10 (64-wide Schur tiles), one step per piece
    ((30, 4000, 7, True), {}),                          # 14 slots, 4 landmarks per wave step
    (("hover", 3, 500, 9), {}),                         # one free pose, nine cameras (global camera path), 27 slots
    (("hover", 6, 400, 3), {"BA_LIN_STEPS": "5"}),       # 18 slots, d = 4, two fixed poses inside every pattern
    (("hover", 12, 300, 2), {}),                        # d = 10 (64-wide Schur tiles), 24 slots
    (("hover", 10, 300, 3), {}),                        # d = 8, 30 slots: 2 landmarks per wave step
])
def test_group_linearisation_matches_oracle(shape, env, built):
    """k_lin_grp (landmark and pose side of the covisibility groups in one pass,
    lane = (landmark, pattern slot)) against the oracle's blocks: A_j, a_j, C_i,
    b_i, B_ji per pair and the cost (reference core/full_bundle_adjustment_solver.
    cpp:716-856), for pattern lengths that fill the wave differently, pieces of
    one to many wave steps, fixed poses inside the patterns (the first five poses
    are fixed), Huber weights active; BA_NO_LINGRP=1 runs the chunk and pose-major
    kernels on the same grouped plan."""
    import os
    if shape[0] == "hover":  # every camera of every pose sees every point: ONE group
        pr = scenes.scaled_problem(scenes.hover_scene(shape[1], shape[2], shape[3], seed=31))
    else:
        n_pose, n_pt, window, stereo = shape
        pr = scenes.scaled_problem(scenes.synthetic_ba_scene(n_pose, n_pt, window, stereo, seed=21, pixel_sigma=1.0))
    for k, v in env.items():
        os.environ[k] = v
    try:
        g = make_gpu(pr)
    finally:
        for k in env:
            os.environ.pop(k, None)
    info = g.get_schur_info()
    assert info["grouped_landmarks"] > 0.7 * g.M
    o = O.Oracle(pr)
    lam, hub = 1.3, 0.7
    o.linearize(hub)
    o.damp_invert(lam)
    g.stage_linearize(lam, hub)
    assert relerr(g.stage_cost(), o.cost()) < 1e-12
    A, a = g.get_A()
    oA, oa = o.get_A()
    assert blockwise_relerr(A, oA) < RTOL_BLOCK and blockwise_relerr(a, oa) < RTOL_BLOCK
    Cm, b = g.get_C()
    oC, ob = o.get_C()
    assert blockwise_relerr(Cm, oC) < RTOL_BLOCK and blockwise_relerr(b, ob) < RTOL_BLOCK
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    key, okey = np.lexsort((pj, pi)), np.lexsort((opj, opi))
    assert (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    assert blockwise_relerr(W[key], oW[okey]) < RTOL_BLOCK
    # the LM path (cost as the by-product of the trial-point linearisation)
    rows, _ = g.solve(make_options(max_iter=3, thr_step=0, thr_cost=0))
    orows, _ = o.solve(O.make_options(max_iter=3, thr_step=0, thr_cost=0))
    for ra, rb in zip(rows, orows):
        assert ra.iteration_status == rb.iteration_status
        assert relerr(ra.trial_cost, rb.trial_cost) < 1e-7
    assert relerr(g.get_poses(), o.get_poses()) < 1e-6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_observation_patterns_match_oracle(seed, built):
    """Covisibility groups with IRREGULAR patterns: every landmark takes one of a few
    random patterns — a random subset of (pose, camera) pairs of a three-camera rig,
    poses not contiguous, cameras in any combination, fixed poses inside, one to nine
    free poses, up to 27 slots — plus a tail of landmarks with unique patterns (chunk
    kernels).  Blocks, reduced system and a short LM trajectory against the oracle."""
    rng = np.random.default_rng(100 + seed)
    n_pose, n_cam, n_pt = 14, 3, 900
    sc = scenes.hover_scene(n_pose, n_pt, n_cam, seed=40 + seed)
    # pattern table: subsets of the (pose, camera) pairs
    pats = []
    for _ in range(6):
        poses = rng.choice(n_pose, size=int(rng.integers(2, 10)), replace=False)
        pat = [(int(j), int(c)) for j in poses for c in range(n_cam) if rng.uniform() < 0.7]
        pats.append(pat if pat else [(int(poses[0]), 0)])
    which = rng.integers(0, len(pats), n_pt)
    keep = np.zeros(sc["obs_pt"].size, bool)
    key = sc["obs_pose"].astype(np.int64) * n_cam + sc["obs_cam"]
    for k, pat in enumerate(pats):
        allowed = np.zeros(n_pose * n_cam, bool)
        for j, c in pat:
            allowed[j * n_cam + c] = True
        keep |= (which[sc["obs_pt"]] == k) & allowed[key]
    # the last 60 landmarks: individual random patterns (no group)
    tail = sc["obs_pt"] >= n_pt - 60
    keep = np.where(tail, rng.uniform(size=keep.size) < 0.4, keep)
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][keep]
    pr = scenes.scaled_problem(sc)
    g, o = _compare_solve(pr, iters=4, tol_par=1e-5)
    info, li = g.get_schur_info(), g.get_lin_info()
    assert info["grouped_landmarks"] > 0.5 * g.M and li["group_pieces"] >= 3 and li["chunks"] >= 1
    lam, hub = 0.8, 0.9
    o.linearize(hub)
    o.damp_invert(lam)
    g.stage_linearize(lam, hub)
    A, a = g.get_A()
    oA, oa = o.get_A()
    assert blockwise_relerr(A, oA) < RTOL_BLOCK and blockwise_relerr(a, oa) < RTOL_BLOCK
    Cm, b = g.get_C()
    oC, ob = o.get_C()
    assert blockwise_relerr(Cm, oC) < RTOL_BLOCK and blockwise_relerr(b, ob) < RTOL_BLOCK
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    key, okey = np.lexsort((pj, pi)), np.lexsort((opj, opi))
    assert (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    assert blockwise_relerr(W[key], oW[okey]) < RTOL_BLOCK


@pytest.mark.parametrize("name,scale", [("W20", 0.1), ("DENSE1K", 0.06), ("C4R", 0.04)])
def test_off_path_configs_match_oracle(name, scale, built):
    """The two configurations bench.py measures OFF the headline's happy path,
    at a size the faithful oracle follows: 20-pose windows (every landmark goes
    through k_schur_partial's global triple list) and random 8-view covisibility
    (dense reduced system, no covisibility group, natural dense sweep)."""
    pr = scenes.scaled_problem(scenes.config_scene(name, scale))
    g, o = _compare_solve(pr, iters=8, tol_par=1e-5)
    info = g.get_schur_info()
    if name == "C4R":
        assert g.get_mask_info()["masked_landmarks"] > 0.5 * g.M_global
    elif name == "W20":   # 20-pose windows: covisibility groups with the 128-wide image (k_schur_grp_wide)
        assert info["grouped_landmarks"] > 0.8 * g.M_global and info["groups64"] > 0
    else:
        assert g.get_dense_info()["fill"] > 0.9


@pytest.mark.parametrize("kind", ["stereo", "mono", "stereo_noise"])
def test_masked_superset_groups_match_oracle(kind, built, monkeypatch):
    """Real visibility breaks the exact repetition of observation patterns: with 15-25 %
    of the observations dropped at random the landmarks of a pose window share the
    UNION of their patterns in a masked covisibility group (padded slots: uv = NaN,
    weight 0; padded pairs: W = 0; the pair's last writer is its last VALID slot).
    Blocks (A, a, C, b, W pair by pair — padded pairs are not shown), the reduced
    system and the LM trajectory against the oracle; and against the library's own
    exact-groups-only plan (BA_NO_SUPERSET=1) to 1e-11."""
    stereo = kind != "mono"
    sc = scenes.synthetic_ba_scene(40, 6000, 5 if stereo else 9, stereo, seed=41,
                                   pixel_sigma=0.4 if kind == "stereo_noise" else 0.0,
                                   dropout=0.15 if stereo else 0.25)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    mi = g.get_mask_info()
    assert mi["masked_landmarks"] > 0.5 * g.M_global and mi["padded_observation_slots"] > 0
    assert g.get_schur_info()["grouped_landmarks"] > 0.9 * g.M_global
    if stereo:
        assert mi["padded_pairs"] > 0
    lam, hub = 2.0, 1.0 if kind != "stereo_noise" else 0.004
    o.linearize(hub); o.damp_invert(lam); o.schur()
    g.stage_linearize(lam, hub); g.stage_schur()
    for (a, b) in zip(g.get_A() + g.get_C(), o.get_A() + o.get_C()):
        assert blockwise_relerr(a, b) < RTOL_BLOCK
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    key, okey = np.lexsort((pj, pi)), np.lexsort((opj, opi))
    assert pi.shape == opi.shape and (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    assert blockwise_relerr(W[key], oW[okey]) < RTOL_BLOCK
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9 and relerr(rhs, orhs) < 1e-9
    assert relerr(g.stage_cost(), o.cost()) < 1e-12
    kw = dict(max_iter=12, thr_step=0, thr_cost=0, huber=hub)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert_same_trajectory(rows, orows)
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    monkeypatch.setenv("BA_NO_SUPERSET", "1")
    e = make_gpu(pr)
    assert e.get_mask_info()["masked_landmarks"] == 0
    erows, _ = e.solve(make_options(**kw))
    for a, b in zip(rows, erows):
        assert a.iteration_status == b.iteration_status
        assert abs(a.trial_cost - b.trial_cost) <= 1e-11 * abs(b.trial_cost)


@pytest.mark.parametrize("kind", ["mono20", "mono13", "stereo16", "mono20_dropout", "stereo14_dropout"])
def test_wide_covisibility_groups_match_oracle(kind, built, monkeypatch):
    """Pose sets of 11..20 poses (windows of 13 / 20 mono views, 14 / 16 stereo views:
    up to 32 pattern slots): k_lin_grp with up to 20 poses per group, k_schur_grp_wide
    (128-wide image, the four waves own nine of the 36 tiles each) and the group role
    of k_backsub_update.  Blocks, reduced system and trajectory against the oracle, and
    against the library's own plan without groups (BA_NO_GROUPS=1: super-runs / pose-
    group classes / global triple list) to 1e-10."""
    window = {"mono20": 20, "mono13": 13, "stereo16": 16, "mono20_dropout": 20, "stereo14_dropout": 14}[kind]
    stereo = kind.startswith("stereo")
    sc = scenes.synthetic_ba_scene(56, 5000, window, stereo, seed=61 + window, pixel_sigma=0.2,
                                   dropout=0.15 if kind.endswith("dropout") else 0.0)
    pr = scenes.scaled_problem(sc)
    g, o = make_gpu(pr), O.Oracle(pr)
    info = g.get_schur_info()
    assert info["grouped_landmarks"] > 0.8 * g.M_global and info["groups64"] > 0, info
    if kind.endswith("dropout"):
        assert g.get_mask_info()["masked_landmarks"] > 0.3 * g.M_global
    lam, hub = 1.5, 0.01
    o.linearize(hub); o.damp_invert(lam); o.schur()
    g.stage_linearize(lam, hub); g.stage_schur()
    for (a, b) in zip(g.get_A() + g.get_C(), o.get_A() + o.get_C()):
        assert blockwise_relerr(a, b) < RTOL_BLOCK
    pi, pj, W = g.get_pairs()
    opi, opj, oW = o.get_pairs()
    key, okey = np.lexsort((pj, pi)), np.lexsort((opj, opi))
    assert pi.shape == opi.shape and (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    assert blockwise_relerr(W[key], oW[okey]) < RTOL_BLOCK
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    assert relerr(S, oS) < 1e-9 and relerr(rhs, orhs) < 1e-9
    assert relerr(g.stage_cost(), o.cost()) < 1e-12
    kw = dict(max_iter=10, thr_step=0, thr_cost=0, huber=hub)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = o.solve(O.make_options(**kw))
    assert_same_trajectory(rows, orows)
    ang, dt, dX = north_star_errors(g, o)
    assert ang <= RTOL_FINAL and dt <= RTOL_FINAL and dX <= RTOL_FINAL, (ang, dt, dX)
    monkeypatch.setenv("BA_NO_GROUPS", "1")
    e = make_gpu(pr)
    assert e.get_schur_info()["grouped_landmarks"] == 0
    erows, _ = e.solve(make_options(**kw))
    for a, b in zip(rows, erows):
        assert a.iteration_status == b.iteration_status
        assert abs(a.trial_cost - b.trial_cost) <= 1e-10 * abs(b.trial_cost)


def test_dense_pattern_ordered_backward_sweep(built, monkeypatch):
    """A dense reduced system with more than 12 row tiles per column (170 poses, every
    landmark seen from 8 random poses: 16 tiles of 64 columns, all coupled) takes the
    ORDERED dataflow backward sweep (k_chol_back_flow<true>: the row tiles of a column are
    consumed one by one as their flags come up).  Against the oracle, and against the
    per-level launches (BA_DENSE_FLOW=0; the summation order of the gather differs:
    1e-10, not bit-identical)."""
    sc = scenes.dense_covisibility_scene(170, 5000, 8, seed=51)
    pr = scenes.scaled_problem(sc)
    g, o = _compare_solve(pr, iters=6, tol_par=1e-5)
    assert g.get_dense_info()["fill"] > 0.9 and g.get_dense_info()["levels"] >= 14
    assert g.get_dropped_pivots() == 0
    rows, _ = g.solve(make_options(max_iter=4, thr_step=0, thr_cost=0))
    monkeypatch.setenv("BA_DENSE_FLOW", "0")
    e = make_gpu(pr)
    e.solve(make_options(max_iter=6, thr_step=0, thr_cost=0))
    erows, _ = e.solve(make_options(max_iter=4, thr_step=0, thr_cost=0))
    for a, b in zip(rows, erows):
        assert a.iteration_status == b.iteration_status
        assert abs(a.trial_cost - b.trial_cost) <= 1e-9 * abs(b.trial_cost)


@pytest.mark.parametrize("scene", ["dense170", "window20", "c1"])
def test_dag_forward_sweep_equals_the_three_launches_per_level(scene, built, monkeypatch):
    """Patterns with many row tiles per column take the three-kernel path (k_chol_diag /
    k_chol_trsm / k_chol_update).  Its forward sweep runs as ONE dataflow launch over all
    levels with lookahead (k_chol_dag: tiles, TRSM items and update targets as tickets; the
    next level's tiles ahead of the bulk of this level's update); BA_DENSE_DAG=0 keeps the
    three launches per level: same arithmetic in the same order, so the trajectories agree
    bit for bit; with forced re-use of the handle (second solve: counters and flags of the
    first are reset / superseded by the generation number)."""
    if scene == "dense170":
        sc = scenes.dense_covisibility_scene(170, 5000, 8, seed=51)
    elif scene == "window20":
        sc = scenes.synthetic_ba_scene(120, 9000, 20, False, seed=52, pixel_sigma=0.2)
    else:
        sc = scenes.config_scene("C1")
    pr = scenes.scaled_problem(sc)
    opt = dict(max_iter=6, thr_step=0, thr_cost=0)
    runs = []
    # (DAG=1: also beyond the item limit of the default; LOOK2=1: the in-launch lookahead that
    #  dense patterns beyond that limit take — k_chol_look: the next level's tiles and TRSM
    #  items beside the bulk of this level's update, two launches per level)
    for env in ({"BA_DENSE_DAG": "1"}, {"BA_DENSE_LOOK2": "1"}, {"BA_DENSE_DAG": "0", "BA_DENSE_LOOK2": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = make_gpu(pr)
        rows, _ = g.solve(make_options(**opt))
        assert g.get_dropped_pivots() == 0
        P1 = g.get_poses().copy()
        g.update_values(pr["pose_T"], pr["pt_X"])
        rows2, _ = g.solve(make_options(**opt))
        assert [(r.iteration_status, r.trial_cost) for r in rows] == [(r.iteration_status, r.trial_cost) for r in rows2]
        assert (g.get_poses() == P1).all()
        runs.append(([(r.iteration_status, r.trial_cost, r.damping_term) for r in rows], P1, g.get_points()[0].copy()))
        for k in env:
            monkeypatch.delenv(k)
    for other in runs[1:]:
        assert runs[0][0] == other[0]
        assert (runs[0][1] == other[1]).all() and (runs[0][2] == other[2]).all()
    if scene == "dense170":
        o = O.Oracle(pr)
        orows, _ = o.solve(O.make_options(**opt))
        for a, b in zip(runs[0][0], orows):
            assert a[0] == b.iteration_status and relerr(a[1], b.trial_cost) < 1e-7


def test_update_values_resolves_without_replanning(built):
    """ba_update_values (new values, same structure): after a solve the problem is
    re-seeded with its ORIGINAL values and solved again — the second trajectory and
    result are bit-identical to the first, with no second ba_finalize; re-seeding with
    other values follows the oracle started from those values."""
    sc = scenes.synthetic_ba_scene(30, 2000, 5, True, seed=31, pixel_sigma=0.2)
    pr = scenes.scaled_problem(sc)
    g = make_gpu(pr)
    opt = dict(max_iter=10, thr_step=0, thr_cost=0)
    rows1, _ = g.solve(make_options(**opt))
    P1, X1 = g.get_poses(), g.get_points()[0]
    g.update_values(pr["pose_T"], pr["pt_X"])
    rows2, _ = g.solve(make_options(**opt))
    assert [(r.iteration_status, r.trial_cost, r.damping_term) for r in rows1] == \
        [(r.iteration_status, r.trial_cost, r.damping_term) for r in rows2]
    assert np.array_equal(P1, g.get_poses()) and np.array_equal(X1, g.get_points()[0])
    # other values (points only): the oracle built from them agrees
    rng = np.random.default_rng(5)
    pr2 = dict(pr)
    pr2["pt_X"] = pr["pt_X"] + rng.uniform(-1e-3, 1e-3, pr["pt_X"].shape)
    g.update_values(None, pr2["pt_X"])
    pr2["pose_T"] = g.get_poses()          # (the poses stayed where the last solve left them)
    rows3, _ = g.solve(make_options(**opt))
    o = O.Oracle(pr2)
    orows, _ = o.solve(O.make_options(**opt))
    assert_same_trajectory(rows3, orows)
    with pytest.raises(ValueError):
        g.update_values(pr["pose_T"][:-1], None)


def test_facade_reload_parameter_values(built):
    """FullBundleAdjustmentSolver.ReloadParameterValues (new): the registered objects
    are read again into the finalized problem; Solve then starts from them.  Without
    the call a second Solve continues from the internal state, as the reference does."""
    from bundle_adjustment_solver_amd.solver import (Camera, FullBundleAdjustmentSolver, Options,
                                                      Summary)
    sc = scenes.synthetic_ba_scene(20, 600, 5, True, seed=33)

    def build():
        ba = FullBundleAdjustmentSolver(0)
        for c in range(sc["intr"].shape[0]):
            ba.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
        poses = sc["T_wc_init"].copy()
        pts = sc["X_init"].copy()
        hp = ba.AddPoseArray(poses)
        hq = ba.AddPointArray(pts)
        for j in np.nonzero(sc["pose_fixed"])[0]:
            ba.MakePoseFixed(int(hp[j]))
        for c in range(sc["intr"].shape[0]):
            m = sc["obs_cam"] == c
            ba.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
        return ba, poses, pts

    opt = Options()
    opt.iteration_handle.max_num_iterations = 8
    opt.convergence_handle.threshold_cost_change = 0.0
    opt.convergence_handle.threshold_step_size = 0.0
    ba, poses, pts = build()
    s1 = Summary()
    ba.Solve(opt, s1)
    first = [(i.iteration_status, i.cost) for i in s1.optimization_info_list_]
    solved_pts = pts.copy()
    # put the initial values back into the caller's arrays and reload them
    poses[...] = sc["T_wc_init"]
    pts[...] = sc["X_init"]
    ba.ReloadParameterValues()
    s2 = Summary()
    ba.Solve(opt, s2)
    assert [(i.iteration_status, i.cost) for i in s2.optimization_info_list_] == first
    assert np.array_equal(pts, solved_pts)
    # without a reload the next Solve continues: its first cost is the last one's
    s3 = Summary()
    ba.Solve(opt, s3)
    assert s3.optimization_info_list_[0].cost < first[0][1] * 0.5
