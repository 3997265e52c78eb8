"""GPU tests of ba_covariance (BaProblem.covariance, csrc/ba_cov.hip and its driver in
csrc/ba_api.hip) at the shapes that tests/test_gpu_covariance.py does not reach: tile
order 64 with several tiles (the left-looking loop of k_cov_solve<64>, four 16-wide panels
per diagonal tile), schedules with fill-in, landmarks with more than 64 pairs (the second
trip of k_cov_rhs's pair loop), handles that hold 64-byte and 96-byte pair records at
once, BA_PAIR_SLIM=0, the call's factorisation at order 64 (no schedule has a tail there:
the launch plan is the LM loop's, not the per-level one of order 32), and selections whose
sweep starts late in the schedule.

Reference, independent of the code under test (test_gpu_batch_covariance.reference): the
CPU oracle linearises (lambda = 0, the same Huber threshold), H = [[A, W], [W^T, C]] is
assembled from its blocks and inverted twice on the host (cov_ref.blocks_two_ways: numpy
inv, and scipy's Cholesky on identity columns); the largest relative block difference
between the two inverses is the reference's own noise.

Tolerance: the rule of test_gpu_covariance.test_blocks_match_the_host_inverse — the
noise must be <= 1e-8 (else the scene is unfit) and the GPU blocks lie within
10 x max(noise, 1e-12) by cov_ref.rel_block_diff.  Everywhere: no dropped pivot, blocks
symmetric to the bit, positive diagonals.

Scenes: the smallest that take the path they are there for.  The numbers of optimisable
poses are chosen so that the image sizes of the two tile orders differ and the order can
be read off the handle: a tile of 32 columns holds 5 poses, one of 64 holds 10, so
npad = ceil(N / 5) * 32 or ceil(N / 10) * 64, and for N = 23, 34, 35, 43 and 65 this is
also ceil(6 N / nb) * nb.

The elimination position of a tile is not visible from outside.  The late-start
selections therefore take every tile of the image in turn — one of them is the last
position — and the points seen by poses of one tile only, for every tile that has any:
the one tile without such points is the short last tile of a chain of tiles, which has
the lowest degree, leaves in the first level of the minimum-degree order and so is never
the last position.
"""
import copy
import os
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import BaBatch, BaProblem
from oracle import oracle_py as O

import cov_ref

pytestmark = pytest.mark.gpu

HUBER = 1.0
ROW_FIELDS = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
              "damping_term", "iteration_status", "rho", "model_change", "trial_cost")

SCENES = {
    # banded, mono; at 64: three tiles (the scene of test_gpu_covariance.py)
    "mono28": lambda: scenes.synthetic_ba_scene(28, 150, 5, False, seed=11, n_fixed=5),
    # banded, stereo (last-writer rule of the cross block); 43 optimisable poses: five tiles of 64
    "stereo44": lambda: scenes.synthetic_ba_scene(44, 300, 5, True, seed=13, n_fixed=1),
    # every landmark seen from four random poses: fill-in, several contributors per row tile
    "loops36": lambda: scenes.dense_covisibility_scene(36, 300, 4, seed=14, n_fixed=2),
    # every landmark seen by all 65 optimisable poses: more than 64 pairs; fully dense image
    "hover70": lambda: scenes.hover_scene(72, 40, 1, seed=15, n_fixed=7),
    # windows of 16 stereo poses: wide covisibility groups feeding k_cov_rhs.  (A group needs 24
    # landmarks of one observation pattern: of the 400 landmarks here 77 are in three groups.)
    "wide40": lambda: scenes.synthetic_ba_scene(40, 400, 16, True, seed=75, n_fixed=5, pixel_sigma=0.2),
    # per-observation dropout: two masked groups (49 landmarks); grouped and ungrouped pairs in
    # one handle
    "dropout40": lambda: scenes.synthetic_ba_scene(40, 500, 5, True, seed=42, pixel_sigma=0.4,
                                                   dropout=0.15, n_fixed=5),
    # the stereo scene of test_gpu_covariance.py (handle path against batch path)
    "stereo12": lambda: scenes.synthetic_ba_scene(n_pose=12, n_pt=150, window=5, stereo=True, seed=12, n_fixed=5),
}
FREE_POSES = {"mono28": 23, "stereo44": 43, "loops36": 34, "hover70": 65, "wide40": 35, "dropout40": 35,
              "stereo12": 7}


class environment:
    """The BA_* variables of a handle: every handle reads them once, at its creation."""

    def __init__(self, **env):
        self.env = {k: v for k, v in env.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_gpu(pr, **env):
    with environment(**env):
        p = BaProblem(0)
        p.set_cameras(pr["cam_intr"], pr["cam_T"])
        p.set_poses(pr["pose_T"], pr["pose_fixed"])
        p.set_points(pr["pt_X"], pr["pt_fixed"])
        p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
        p.finalize()
    return p


def knobs(nb=None, slim=None, batch=None):
    return dict(BA_DENSE_NB=None if nb is None else str(nb), BA_PAIR_SLIM=slim,
                BA_COV_BATCH=None if batch is None else str(batch))


def reference(pr, huber=HUBER):
    """(cov_pose [n_pose, 6, 6], cov_pt [n_pt, 3, 3], noise) of a problem dict from the CPU
    oracle and the two host inverses; blocks of fixed members and of never-observed
    landmarks are zero (test_gpu_batch_covariance.reference)."""
    o = O.Oracle(pr)
    o.linearize(huber)
    o.damp_invert(0.0)
    A, _ = o.get_A()
    Cm, _ = o.get_C()
    pi, pj, W = o.get_pairs()
    o.close()
    ps = np.nonzero(np.asarray(pr["pose_fixed"]) == 0)[0]
    qs = np.nonzero(np.asarray(pr["pt_fixed"]) == 0)[0]
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_fixed"]))[qs] > 0
    remap = np.cumsum(seen) - 1
    assert seen[pi].all()
    H = cov_ref.full_normal_matrix(A, Cm[seen], remap[pi], pj, W)
    cp, cq, noise = cov_ref.blocks_two_ways(H, len(ps), int(seen.sum()))
    full_p = np.zeros((len(pr["pose_fixed"]), 6, 6))
    full_q = np.zeros((len(pr["pt_fixed"]), 3, 3))
    full_p[ps] = cp
    full_q[qs[seen]] = cq
    return full_p, full_q, noise


_problems, _runs = {}, {}


def problem(name):
    """(problem dict, user indices of the optimisable poses / points, reference pose and
    point blocks of these, reference noise) — computed once and left unchanged"""
    if name not in _problems:
        pr = scenes.scaled_problem(SCENES[name]())
        ps = np.nonzero(pr["pose_fixed"] == 0)[0]
        qs = np.nonzero(pr["pt_fixed"] == 0)[0]
        assert ps.size == FREE_POSES[name]
        full_p, full_q, noise = reference(pr)
        _problems[name] = (pr, ps, qs, full_p[ps], full_q[qs], noise)
    return _problems[name]


def select_all(name, nb=None, slim=None, batch=None):
    """The select-all call of a scene on a handle created under the given knobs -> dict of
    the blocks and of what the handle says about itself — computed once per combination."""
    key = (name, nb, slim, batch)
    if key not in _runs:
        pr, ps, qs = problem(name)[:3]
        p = make_gpu(pr, **knobs(nb, slim, batch))
        assert p.N == ps.size
        gp, gq, dropped = p.covariance(ps, qs, HUBER)
        _runs[key] = dict(gp=gp, gq=gq, dropped=dropped, dense=p.get_dense_info(), rec=p.get_pair_record_info(),
                          cov=p.covariance_info(), mask=p.get_mask_info())
        p.close()
    return _runs[key]


def tile_order(npad, N):
    """The tile order an image of npad columns for N optimisable poses was built at."""
    by_order = {nb: -(-N // ppt) * nb for nb, ppt in ((32, 5), (64, 10))}
    assert by_order[32] != by_order[64], "this number of poses does not tell the orders apart"
    assert npad in by_order.values()
    return 32 if npad == by_order[32] else 64


def check_blocks(label, pr, qs, gp, gq, dropped, ref_p, ref_q, noise):
    """prints the figures, then the rule of test_blocks_match_the_host_inverse"""
    err_p, err_q = cov_ref.rel_block_diff(gp, ref_p), cov_ref.rel_block_diff(gq, ref_q)
    print("%s: reference noise %.3e  gpu error pose %.3e point %.3e" % (label, noise, err_p, err_q))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert dropped == 0
    assert gp.shape == ref_p.shape and gq.shape == ref_q.shape
    tol = 10.0 * max(noise, 1e-12)
    assert err_p <= tol and err_q <= tol, (label, err_p, err_q, tol)
    assert np.array_equal(gp, gp.transpose(0, 2, 1)) and np.array_equal(gq, gq.transpose(0, 2, 1))
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_fixed"]))[qs] > 0
    assert (np.einsum("nii->ni", gp) > 0).all() and (np.einsum("nii->ni", gq[seen]) > 0).all()
    assert not gq[~seen].any()
    return err_p, err_q


def check_run(label, name, r):
    pr, ps, qs, ref_p, ref_q, noise = problem(name)
    d = r["dense"]
    label = "%s: npad %d levels %d fill %.3f" % (label, d["npad"], d["levels"], d["fill"])
    return check_blocks(label, pr, qs, r["gp"], r["gq"], r["dropped"], ref_p, ref_q, noise)


# ---------------------------------------------------------------------------------------
# 1. both tile orders

@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["mono28", "stereo44", "loops36", "dropout40"])
def test_blocks_match_the_host_inverse_at_both_tile_orders(built, name, nb):
    """All poses and all points under BA_DENSE_NB=32 and =64.  The order is read off the
    handle: npad is ceil(6 N / nb) * nb, which differs between the two orders for every
    scene here; at 64 the image has at least three tiles, so the left-looking loop of
    k_cov_solve<64> runs.  The call's factorisation hands no level to k_chol_tail: at 32
    these schedules have a tail, the uploaded lists do not fit and the levels take the
    per-level kernels; at 64 no schedule has a tail (two levels of 64 columns exceed its 96)
    and the plan is the LM loop's own."""
    N = FREE_POSES[name]
    r = select_all(name, nb=nb)
    npad = r["dense"]["npad"]
    assert npad == -(-6 * N // nb) * nb
    assert -(-6 * N // 32) * 32 != -(-6 * N // 64) * 64
    assert tile_order(npad, N) == nb
    if nb == 64:
        assert npad // 64 >= 3
    check_run("%s at %d" % (name, nb), name, r)


@pytest.mark.parametrize("nb", [32, 64])
def test_the_random_covisibility_scene_has_fill(built, capfd, nb):
    """loops36 is there for row tiles with several contributing columns in permuted
    order.  Its schedule holds more of the lower triangle than the banded scenes' at the
    same order (fill of get_dense_info), and the BA_PLAN_STATS line of the handle's
    creation shows a column with at least three row tiles below it (max_rows counts the
    rhs block too): the lowest of them lies three positions or more from its column, a
    contributor that is no neighbour.  The launch-plan line of the same handle shows what
    the solves hand to k_chol_tail and the covariance call does not: 96 columns at order
    32 (the last three of seven one-tile levels), nothing at 64."""
    fill = select_all("loops36", nb=nb)["dense"]["fill"]
    banded = [select_all(k, nb=nb)["dense"]["fill"] for k in ("mono28", "stereo44")]
    capfd.readouterr()
    make_gpu(problem("loops36")[0], BA_PLAN_STATS="1", BA_DENSE_NB=str(nb)).close()
    said = capfd.readouterr().err.splitlines()
    lines = [l for l in said if l.startswith("dense schedules:")]
    plans = [l for l in said if l.startswith("dense launch plan: nb%d " % nb)]
    assert len(lines) == 1 and len(plans) == 1, said
    assert ("tail %d columns" % (96 if nb == 32 else 0)) in plans[0], plans
    m = re.search(r"nb%d (\d+) tiles (\d+) levels max_rows (\d+) fill ([0-9.]+)" % nb, lines[0])
    tiles, levels, max_rows, said_fill = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4))
    print("loops36 at %d: %d tiles, %d levels, max_rows %d, fill %.3f; banded scenes' fill %s"
          % (nb, tiles, levels, max_rows, fill, banded))
    assert tiles * nb == select_all("loops36", nb=nb)["dense"]["npad"] and abs(said_fill - fill) < 1e-3
    assert fill > max(banded)
    assert max_rows - 1 >= 3


@pytest.mark.parametrize("name", ["hover70", "wide40"])
def test_blocks_match_the_host_inverse_at_the_planners_order(built, name):
    """The dense and the wide pattern at the order dense_pick_tile_order takes for them,
    read off npad.  hover70 is fully dense: 64 (seven tiles).  wide40's windows of 16 poses
    still make a narrow band of 32-column tiles (at most three row tiles below a column),
    and five levels of 32 are a shorter chain than three of 64: 32.  hover70: every
    landmark has 65 pairs, one more than a trip of k_cov_rhs's loop over a landmark's pairs
    covers."""
    pr, ps, qs = problem(name)[:3]
    N = FREE_POSES[name]
    r = select_all(name)
    nb = {"hover70": 64, "wide40": 32}[name]
    assert tile_order(r["dense"]["npad"], N) == nb and r["dense"]["npad"] // nb >= 3
    if name == "hover70":
        free = pr["pose_fixed"][pr["obs_pose"]] == 0
        pairs = np.bincount(pr["obs_pt"][free], minlength=len(pr["pt_fixed"]))
        assert (pairs == N).all() and N > 64       # (one camera: a pair per observation)
        assert r["dense"]["fill"] == 1.0
    if name == "wide40":
        assert r["rec"]["slim_pairs"] > 0
    check_run(name, name, r)


def test_long_landmarks_across_column_batches(built):
    """hover70 under BA_COV_BATCH=64: four waves per batch, so the 33 pose groups and the
    8 groups of landmarks with 65 pairs each take 11 batches: the bits of the one-batch
    call."""
    one = select_all("hover70")
    many = select_all("hover70", batch=64)
    assert one["cov"]["last_batches"] == 1
    assert many["cov"]["batch_cols"] == 64 and many["cov"]["last_batches"] == 11
    assert many["dropped"] == 0
    assert np.array_equal(many["gp"], one["gp"]) and np.array_equal(many["gq"], one["gq"])


# ---------------------------------------------------------------------------------------
# 2. record forms

@pytest.mark.parametrize("name", ["dropout40", "wide40"])
def test_both_pair_record_forms(built, name):
    """Default handle and BA_PAIR_SLIM=0, each against the reference.  On dropout40 the
    default handle holds 64-byte {G, w} records and 96-byte records at once, so both
    branches of k_cov_rhs run in one call; with the knob off no pair is slim.  pair_from_G
    is written to rebuild {K, X_ij} with the roundings of the writer of the 96-byte record
    (csrc/ba_device_fn.h), and on the MI355X the two forms gave the same bits on both
    scenes: asserted."""
    slim, full = select_all(name), select_all(name, slim="0")
    print(name, "default", slim["rec"], slim["mask"], "BA_PAIR_SLIM=0", full["rec"])
    assert slim["rec"]["pairs"] == full["rec"]["pairs"] > 0
    if name == "dropout40":
        assert 0 < slim["rec"]["slim_pairs"] < slim["rec"]["pairs"]
        assert slim["mask"]["masked_landmarks"] > 0 and slim["mask"]["padded_pairs"] > 0
    else:
        assert slim["rec"]["slim_pairs"] > 0
    assert full["rec"]["slim_pairs"] == 0
    check_run("%s, default records" % name, name, slim)
    check_run("%s, BA_PAIR_SLIM=0" % name, name, full)
    print("%s: the two record forms against each other, largest relative block difference pose %.3e point %.3e"
          % (name, cov_ref.rel_block_diff(slim["gp"], full["gp"]), cov_ref.rel_block_diff(slim["gq"], full["gq"])))
    assert np.array_equal(slim["gp"], full["gp"]) and np.array_equal(slim["gq"], full["gq"])


# ---------------------------------------------------------------------------------------
# 3. late and mixed starts

def tiles_of(name, nb):
    """Per tile of the image (in pose order: the elimination position is not visible):
    positions in the select-all result of its poses, and of the points whose pairs all
    lie in it."""
    pr, ps, qs = problem(name)[:3]
    ppt = 5 if nb == 32 else 10
    jopt = np.cumsum(pr["pose_fixed"] == 0) - 1
    free = pr["pose_fixed"][pr["obs_pose"]] == 0
    t = jopt[pr["obs_pose"][free]] // ppt
    lo, hi = np.full(len(pr["pt_fixed"]), 1 << 30), np.full(len(pr["pt_fixed"]), -1)
    np.minimum.at(lo, pr["obs_pt"][free], t)
    np.maximum.at(hi, pr["obs_pt"][free], t)
    ntile = -(-ps.size // ppt)
    poses = [np.arange(ps.size)[np.arange(ps.size) // ppt == k] for k in range(ntile)]
    points = [np.nonzero((lo[qs] == k) & (hi[qs] == k))[0] for k in range(ntile)]
    return poses, points


@pytest.mark.parametrize("name,nb", [("stereo44", 64), ("mono28", 32)])
def test_late_and_mixed_starts_give_the_bits_of_select_all(built, name, nb):
    """Selections whose sweep starts below the top of the schedule, each bit for bit the
    same blocks as in the select-all call: the poses of one tile only and the points seen
    only by poses of one tile, for every tile (one of them is the last position, where the
    sweep is a single step); one pose alone; three poses of three tiles (groups of 2 and
    1); six points of two tiles (groups of 5 and 1, the first holding landmarks whose
    right-hand sides start in different tiles)."""
    pr, ps, qs = problem(name)[:3]
    full = select_all(name, nb=nb)
    assert tile_order(full["dense"]["npad"], ps.size) == nb
    poses, points = tiles_of(name, nb)
    assert len(poses) == full["dense"]["npad"] // nb >= 5
    # every tile but the short last one of the chain has points of its own
    assert all(q.size >= 3 for q in points[:-1]) and len(poses[-1]) < (5 if nb == 32 else 10)
    p = make_gpu(pr, **knobs(nb=nb))
    assert p.get_dense_info() == full["dense"]

    def same(kp, kq, what):
        gp, gq, dropped = p.covariance(ps[kp], qs[kq], HUBER)
        assert dropped == 0, what
        assert np.array_equal(gp, full["gp"][kp]) and np.array_equal(gq, full["gq"][kq]), what

    none = np.zeros(0, int)
    for k in range(len(poses)):
        same(poses[k], none, "poses of tile %d" % k)
        if points[k].size:
            same(none, points[k], "points of tile %d" % k)
        same(poses[k], points[k], "poses and points of tile %d" % k)
        same(poses[k][-1:], none, "last pose of tile %d alone" % k)
    same(np.array([poses[0][1], poses[2][0], poses[4][0]]), none, "three poses of three tiles")
    same(np.array([poses[3][2], poses[1][0], poses[1][1]]), none, "three poses of two tiles")
    for a, b in ((1, 3), (3, 0), (2, 1)):
        six = np.r_[points[a][:3], points[b][:3]]
        assert six.size == 6
        same(none, six, "six points of tiles %d and %d" % (a, b))
        same(poses[a][:1], six[::-1], "the same with a pose, reversed")
    p.close()


# ---------------------------------------------------------------------------------------
# 4. after a solve

def _rows(rows):
    return [tuple(getattr(r, k) for k in ROW_FIELDS) for r in rows]


def test_after_a_solve_at_order_64_with_fill(built):
    """loops36 under BA_DENSE_NB=64: three LM iterations (huber 1.0), then the covariance
    of the solved values against the reference at exactly those values (the GPU's poses
    and points are the oracle's input, so only the covariance is under test; the oracle's
    own three iterations, same options, end at the same values to the 1e-8 of smoke()).
    A second solve on that handle then gives the rows and values of a handle that never
    called covariance, bit for bit (the rule of
    test_solve_after_covariance_is_the_solve_without_it, here at 64 and with fill)."""
    pr, ps, qs = problem("loops36")[:3]
    kw = dict(max_iter=3, thr_step=0.0, thr_cost=0.0, huber=HUBER)
    a, b = make_gpu(pr, **knobs(nb=64)), make_gpu(pr, **knobs(nb=64))
    assert tile_order(a.get_dense_info()["npad"], ps.size) == 64
    ra, _ = a.solve(make_options(**kw))
    rb, _ = b.solve(make_options(**kw))
    assert len(ra) == 3 and _rows(ra) == _rows(rb)
    T1, X1 = a.get_poses(), a.get_points()[0]
    o = O.Oracle(pr)
    orows, _ = o.solve(O.make_options(**kw))
    dT, dX = np.abs(o.get_poses() - T1).max(), np.abs(o.get_points() - X1).max()
    o.close()
    print("after three iterations: GPU against oracle, poses %.2e points %.2e" % (dT, dX))
    assert [r.iteration_status for r in ra] == [r.iteration_status for r in orows]
    assert dT < 1e-8 and dX < 1e-8
    assert np.abs(T1 - pr["pose_T"]).max() > 1e-6        # the solve moved the values
    gp, gq, dropped = a.covariance(ps, qs, HUBER)
    assert np.array_equal(a.get_poses(), T1) and np.array_equal(a.get_points()[0], X1)
    solved = copy.copy(pr)
    solved["pose_T"], solved["pt_X"] = T1.copy(), X1.copy()
    full_p, full_q, noise = reference(solved)
    check_blocks("loops36 at 64, at the solved values", pr, qs, gp, gq, dropped, full_p[ps], full_q[qs], noise)
    opt2 = make_options(max_iter=4, thr_step=0.0, thr_cost=0.0, huber=HUBER)
    ra2, ca = a.solve(opt2)
    rb2, cb = b.solve(opt2)
    assert len(ra2) == len(rb2) == 4 and ca == cb and _rows(ra2) == _rows(rb2)
    assert np.array_equal(a.get_poses(), b.get_poses())
    assert np.array_equal(a.get_points()[0], b.get_points()[0])
    assert a.get_dropped_pivots() == b.get_dropped_pivots() == 0
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------
# 5. handle path against batch path

def test_handle_path_against_batch_path(built):
    """stereo12 of test_gpu_covariance.py through BaProblem.covariance (tile Cholesky in
    the dense image, k_cov_solve) and through BaBatch([pr]).covariance (k_ba_batch_cov:
    Cholesky and S^-1 in LDS): both match the one reference, and each other within the
    same bound — two independent kernels that agree rule out an error shared with the
    reference's construction of H."""
    pr, ps, qs, ref_p, ref_q, noise = problem("stereo12")
    r = select_all("stereo12")
    check_run("stereo12, handle path", "stereo12", r)
    b = BaBatch([pr])
    cp, cq, res = b.covariance(HUBER)
    b.close()
    assert res[0].status == 0
    bp, bq = cp[ps], cq[qs]
    check_blocks("stereo12, batch path", pr, qs, bp, bq, res[0].dropped_pivots, ref_p, ref_q, noise)
    fixed_p, fixed_q = np.asarray(pr["pose_fixed"]) != 0, np.asarray(pr["pt_fixed"]) != 0
    assert not cp[fixed_p].any() and not cq[fixed_q].any()
    d_p, d_q = cov_ref.rel_block_diff(r["gp"], bp), cov_ref.rel_block_diff(r["gq"], bq)
    print("stereo12: handle path against batch path, pose %.3e point %.3e" % (d_p, d_q))
    tol = 10.0 * max(noise, 1e-12)
    assert d_p <= tol and d_q <= tol, (d_p, d_q, tol)
