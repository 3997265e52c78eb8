"""GPU tests of the observation report, the observation mask and the outlier cull of the
batched full bundle adjustment (BaBatch.obs_report / set_obs_mask / cull / solve_culled;
k_ba_batch_obs_report, k_ba_batch_mask_apply, k_ba_batch_cull).

The contract of the mask: every result of a masked batch agrees with the same call on a fresh
batch created from the same arrays with the off observations removed (`filtered`), and so with
the CPU oracle on those arrays.  Tolerances are the project's: trajectories by
assert_same_trajectory of test_gpu_full_batch.py (equal statuses, damping to 1e-12, costs to
1e-7 relative, final values to 1e-6); covariance and marginalisation by the noise rule of
test_gpu_batch_covariance.py / test_gpu_batch_marginalize.py against cov_ref / marg_ref.

Windows: A stereo 4 poses (2 fixed) / 12 landmarks; B mono 5 poses / 37 landmarks; C stereo
10 poses / 60 landmarks = 1 200 observations, more than four workgroup widths, so every
chunked loop of the mask kernels wraps, with its observation arrays shuffled by a seeded
permutation (user order != planned order).
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import BaError, make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, CullOptions, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, Options)
from oracle import oracle_py as O

import marg_ref
import prior_ref
import rel_ref
from test_gpu_batch_covariance import check_blocks, reference as cov_reference
from test_gpu_batch_marginalize import check as marg_check
from test_gpu_full_batch import FIXED, assert_same_trajectory, relerr, row_bits, window

pytestmark = pytest.mark.gpu

OBS_KEYS = ("obs_cam", "obs_pose", "obs_pt", "obs_uv")
HUBER = 1.0


def shuffled(sc, seed):
    perm = np.random.default_rng(seed).permutation(sc["obs_pt"].size)
    for k in OBS_KEYS:
        sc[k] = sc[k][perm]
    return sc


def filtered(pr, on):
    out = dict(pr)
    for k in OBS_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(pr[k])[np.asarray(on, bool)])
    return out


def project_np(pr, T=None, X=None):
    """fp64 numpy projection of every observation of a problem dict: (r (n, 2), depth)"""
    T = np.asarray(pr["pose_T"] if T is None else T, np.float64).reshape(-1, 12)
    X = np.asarray(pr["pt_X"] if X is None else X, np.float64).reshape(-1, 3)
    oc, op, oq = pr["obs_cam"], pr["obs_pose"], pr["obs_pt"]
    P, Cm, intr = T[op], np.asarray(pr["cam_T"])[oc], np.asarray(pr["cam_intr"])[oc]
    Xij = np.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), X[oq]) + P[:, 9:]
    Xc = np.einsum("nij,nj->ni", Cm[:, :9].reshape(-1, 3, 3), Xij) + Cm[:, 9:]
    r0 = intr[:, 0] * (Xc[:, 0] / Xc[:, 2]) + intr[:, 2] - pr["obs_uv"][:, 0]
    r1 = intr[:, 1] * (Xc[:, 1] / Xc[:, 2]) + intr[:, 3] - pr["obs_uv"][:, 1]
    return np.stack([r0, r1], 1), Xc[:, 2]


def ulp_diff(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.fixture(scope="module")
def abc(built):
    A = scenes.scaled_problem(window(4, 12, True, 41))
    Bm = scenes.scaled_problem(window(5, 37, False, 11))
    Cs = scenes.scaled_problem(shuffled(window(10, 60, True, 43), 7))
    assert [len(p["obs_pt"]) for p in (A, Bm, Cs)] == [96, 185, 1200]
    return [A, Bm, Cs]


# ---- the five mask cases --------------------------------------------------------------------
def pair_key(pr):
    return pr["obs_pt"].astype(np.int64) * 1000 + pr["obs_pose"]


def some_pairs(pr, seed, n):
    """n (landmark, optimisable pose) pairs of the problem, seeded"""
    keys = np.unique(pair_key(pr)[pr["pose_fixed"][pr["obs_pose"]] == 0])
    return np.random.default_rng(seed).choice(keys, n, replace=False)


def mask_of(pr, case, seed):
    n = len(pr["obs_pt"])
    on = np.ones(n, bool)
    stereo = len(pr["cam_intr"]) > 1
    if case == "right":          # (a) the right-camera observation, the last writer, of several pairs
        if stereo:
            on[np.isin(pair_key(pr), some_pairs(pr, seed, 7)) & (pr["obs_cam"] == 1)] = False
    elif case == "pairs":        # (b) every observation of several pairs
        on[np.isin(pair_key(pr), some_pairs(pr, seed, 7))] = False
    elif case == "landmarks":    # (c) every observation of two landmarks
        on[np.isin(pr["obs_pt"], [1, len(pr["pt_fixed"]) - 2])] = False
    elif case == "random":       # (d) a seeded 20 %
        on[np.random.default_rng(seed).choice(n, n // 5, replace=False)] = False
    return on


CASES = ("right", "pairs", "landmarks", "random", "one_all_on")


def masks_of(probs, case):
    if case == "one_all_on":     # (e) B all on between two masked problems
        return [mask_of(probs[0], "random", 90), mask_of(probs[1], "none", 0), mask_of(probs[2], "pairs", 92)]
    return [mask_of(pr, case, 80 + k) for k, pr in enumerate(probs)]


def oldest_marked(probs):
    mk = [np.zeros(len(p["pose_fixed"]), np.uint8) for p in probs]
    for m, p in zip(mk, probs):
        m[np.flatnonzero(p["pose_fixed"] == 0)[0]] = 1
    return mk


def solved(b, opt):
    rows, res = b.solve(opt)
    T, X = b.get_poses(), b.get_points()
    return [(rows[p], res[p], b.poses_of(p, T).copy(), b.points_of(p, X).copy()) for p in range(b.B)]


def assert_close_solve(got, ref):
    rows, res, T, X = got
    rrows, rres, rT, rX = ref
    assert res.status == rres.status == 0 and res.n_iter == rres.n_iter == len(rrows)
    assert_same_trajectory(rows, rrows)
    assert relerr(T, rT) < 1e-6 and relerr(X, rX) < 1e-6


def assert_same_bits(got, ref):
    assert np.array_equal(row_bits(got[0]), row_bits(ref[0]))
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert (got[1].n_iter, got[1].status, got[1].dropped_pivots) == (ref[1].n_iter, ref[1].status, ref[1].dropped_pivots)


@pytest.fixture(scope="module")
def unmasked(abc):
    b = BaBatch(abc)
    out = solved(b, make_options(**FIXED))
    b.close()
    return out


# ---- 1. report ---------------------------------------------------------------------------------
def check_report(b, probs, huber):
    rep = b.obs_report(huber)
    T, X = b.get_poses(), b.get_points()
    for p, pr in enumerate(probs):
        r, depth = project_np(pr, b.poses_of(p, T), b.points_of(p, X))
        g = rep[p]
        err_r, err_d = np.abs(g["r2"] - r).max(), np.abs(g["depth"] - depth).max()
        print("report problem %d: |dr| %.2e |ddepth| %.2e" % (p, err_r, err_d))
        assert err_r <= 1e-12 and err_d <= 1e-12
        e2 = g["r2"][:, 0] ** 2 + g["r2"][:, 1] ** 2
        absr = np.abs(g["r2"]).sum(1)
        w = np.where(absr > huber, huber / np.where(absr > 0, absr, 1.0), 1.0)
        assert ulp_diff(g["e2"], e2).max() <= 4 and ulp_diff(g["w"], w).max() <= 4
    return rep


def test_report_matches_a_numpy_projection(abc):
    b = BaBatch(abc)
    rep0 = check_report(b, abc, 0.02)
    b.solve(make_options(**FIXED))
    rep1 = check_report(b, abc, 0.02)
    assert all(r1["e2"].sum() < r0["e2"].sum() for r0, r1 in zip(rep0, rep1))
    assert all((r["w"] < 1).any() for r in rep0) and any((r["w"] == 1).any() for r in rep1)   # both Huber branches
    # with a mask: off observations are still reported, and the values are those of before
    b.set_obs_mask(masks_of(abc, "random"))
    rep2 = check_report(b, abc, 0.02)
    for r1, r2 in zip(rep1, rep2):
        assert all(np.array_equal(r1[k], r2[k]) for k in r1)
    with pytest.raises(BaError, match="every output is null"):
        from bundle_adjustment_solver_amd._lib import check
        check(b.lib.ba_batch_obs_report(b.b, 1.0, None, None, None, None), "ba_batch_obs_report")
    b.close()


# ---- 2. the mask contract ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_masked_batch_is_the_fresh_filtered_batch(abc, unmasked, case):
    masks = masks_of(abc, case)
    assert any(not m.all() for m in masks)
    fl = [filtered(pr, m) for pr, m in zip(abc, masks)]
    opt = make_options(**FIXED)
    mk = oldest_marked(abc)

    def run(b):
        cp, cq, cres = b.covariance(HUBER)
        cov = [(b.cov_poses_of(p, cp).copy(), b.cov_points_of(p, cq).copy(), cres[p]) for p in range(b.B)]
        Hl, bl, kl, mres = b.marginalize(np.concatenate(mk), HUBER)
        mq = b.marg_pt.copy()
        mg = [(Hl[p].copy(), bl[p].copy(), kl[p], b.points_of(p, mq) != 0, mres[p]) for p in range(b.B)]
        return cov, mg, solved(b, opt)

    b = BaBatch(abc)
    b.set_obs_mask(masks)
    assert all(np.array_equal(g, m) for g, m in zip(b.get_obs_mask(), masks))
    cov, mg, got = run(b)
    b.close()
    f = BaBatch(fl)
    fcov, fmg, fresh = run(f)
    f.close()
    for p, pr in enumerate(fl):
        label = "%s/%d" % (case, p)
        assert_close_solve(got[p], fresh[p])
        o = O.Oracle(pr)
        orows, _ = o.solve(O.make_options(**FIXED))
        assert_same_trajectory(got[p][0], orows)
        assert relerr(got[p][2], o.get_poses()) < 1e-6 and relerr(got[p][3], o.get_points()) < 1e-6
        o.close()
        if masks[p].all():       # an all-on problem beside masked ones: the bits of the batch without a mask
            assert_same_bits(got[p], unmasked[p])
        else:
            assert not np.array_equal(got[p][2], unmasked[p][2])
        ref_p, ref_q, noise = cov_reference(pr, HUBER)
        check_blocks(label, pr, cov[p], ref_p, ref_q, noise)
        marg_check(label, pr, mk[p], mg[p], marg_ref.reference(pr, mk[p], HUBER))
        assert np.array_equal(mg[p][3], fmg[p][3])          # the L set is decided from the on observations


# ---- 3. state ----------------------------------------------------------------------------------
def test_mask_state(abc, unmasked):
    big = scenes.scaled_problem(window(19, 20, True, 13))            # 17 optimisable poses: status 2
    probs = [abc[0], big, abc[1]]
    masks = [mask_of(probs[0], "random", 3), mask_of(big, "random", 4), mask_of(probs[2], "pairs", 5)]
    opt = make_options(**FIXED)
    b = BaBatch(probs)
    T0, X0 = b.get_poses(), b.get_points()
    never = solved(b, opt)
    assert [r[1].status for r in never] == [0, 2, 0]
    assert_same_bits(never[0], unmasked[0])
    assert_same_bits(never[2], unmasked[1])
    b.update_values(T0, X0)
    b.set_obs_mask(masks)
    first = solved(b, opt)
    assert first[1][1].status == 2
    assert np.array_equal(first[1][2], never[1][2]) and np.array_equal(first[1][3], never[1][3])
    assert not np.array_equal(first[0][2], never[0][2])
    # the neighbours of the problem over the limit are what they are without it
    alone = BaBatch([probs[0], probs[2]])
    alone.set_obs_mask([masks[0], masks[2]])
    al = solved(alone, opt)
    alone.close()
    assert_same_bits(first[0], al[0])
    assert_same_bits(first[2], al[1])
    # update_values keeps the mask; the same mask twice gives the same bits
    b.update_values(T0, X0)
    assert_same_bits(solved(b, opt)[0], first[0])
    b.update_values(T0, X0)
    b.set_obs_mask(np.concatenate(masks))
    assert all(np.array_equal(g, m) for g, m in zip(b.get_obs_mask(), masks))
    again = solved(b, opt)
    assert_same_bits(again[0], first[0])
    assert_same_bits(again[2], first[2])
    # None restores the never-masked bits
    b.update_values(T0, X0)
    b.set_obs_mask(None)
    assert all(g.all() for g in b.get_obs_mask())
    back = solved(b, opt)
    assert_same_bits(back[0], never[0])
    assert_same_bits(back[2], never[2])
    with pytest.raises(ValueError, match="problem 1"):
        b.set_obs_mask([masks[0], masks[1][:-1], masks[2]])
    b.close()


# ---- 4. with a prior and with relative-pose factors -------------------------------------------
def test_mask_with_prior_and_relative_factors(abc):
    probs = [abc[1], abc[2]]
    masks = [mask_of(probs[0], "random", 21), mask_of(probs[1], "pairs", 22)]
    free = [np.flatnonzero(p["pose_fixed"] == 0) for p in probs]
    priors = [prior_ref.random_prior(p, f[:2], seed=60 + k) for k, (p, f) in enumerate(zip(probs, free))]
    rels = [rel_ref.random_relatives(p, [(int(f[1]), int(f[0])), (int(f[2]), int(f[1])), (int(f[2]), 0)],
                                     seed=70 + k) for k, (p, f) in enumerate(zip(probs, free))]
    opt = make_options(**FIXED)

    def run(ps, ms):
        b = BaBatch(ps)
        b.set_prior(priors)
        b.set_relative(rels)
        if ms is not None:
            b.set_obs_mask(ms)
        out = solved(b, opt)
        b.close()
        return out

    got = run(probs, masks)
    fresh = run([filtered(p, m) for p, m in zip(probs, masks)], None)
    full = run(probs, None)
    for p in range(2):
        assert_close_solve(got[p], fresh[p])
        assert relerr(got[p][0][0].trial_cost, full[p][0][0].trial_cost) > 1e-6    # the mask is felt


# ---- 5. cull -----------------------------------------------------------------------------------
CULL_SCENES = ((101, True, 6, 40), (102, False, 5, 37), (103, True, 10, 60))
CULL_OPT = dict(huber=0.02, lambda0=1e-3, thr_step=0.0, thr_cost=0.0)
E2_MAX = 25e-4            # 25 px^2 in the library's units (pixels x 0.01)


def displaced(sc, seed, idx=None):
    """the scene with a seeded 5-6 % of its observations (or idx) moved by 30-80 px in a random
    direction: (scene, bool per observation: displaced)"""
    rng = np.random.default_rng(seed)
    n = sc["obs_pt"].size
    if idx is None:
        idx = rng.choice(n, int(np.ceil(0.055 * n)), replace=False)
    ang, mag = rng.uniform(0, 2 * np.pi, len(idx)), rng.uniform(30.0, 80.0, len(idx))
    sc["obs_uv"] = sc["obs_uv"].copy()
    sc["obs_uv"][idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    out = np.zeros(n, bool)
    out[idx] = True
    return sc, out


@pytest.fixture(scope="module")
def cull_scenes(built):
    probs, bad = [], []
    for seed, stereo, n_pose, n_pt in CULL_SCENES:
        sc, out = displaced(window(n_pose, n_pt, stereo, seed, pixel_sigma=0.3), seed + 3000)
        assert 0.05 <= out.mean() <= 0.06
        probs.append(scenes.scaled_problem(sc))
        bad.append(out)
    # the condition of the test, from the oracle alone: after its stage 1 no observation lies
    # within a factor 2 of the threshold (on the CPU: inlier maxima 1.3, 1.7 and 1.6 px^2, outlier
    # minima 1011, 860 and 954 px^2; the displacement seeds are those of the scenes + 3000: with
    # + 1000 or + 2000 the mono scene 102 keeps an inlier at 35 px^2 after five iterations and
    # does not separate)
    for pr, out in zip(probs, bad):
        o = O.Oracle(pr)
        o.solve(O.make_options(max_iter=5, **CULL_OPT))
        r, depth = project_np(pr, o.get_poses(), o.get_points())
        o.close()
        e2 = (r ** 2).sum(1)
        print("oracle stage 1: inlier max %.2f px^2, outlier min %.1f px^2" % (e2[~out].max() * 1e4, e2[out].min() * 1e4))
        assert e2[~out].max() < E2_MAX / 2 and e2[out].min() > 2 * E2_MAX and (depth > 0).all()
    return probs, bad


def full_state(b):
    return b.get_poses(), b.get_points(), np.concatenate(b.get_obs_mask())


def test_cull_finds_the_displaced_observations(cull_scenes):
    probs, bad = cull_scenes
    first, second = make_options(max_iter=5, **CULL_OPT), make_options(max_iter=6, **CULL_OPT)
    # the three separate calls
    b = BaBatch(probs)
    rows1, res1 = b.solve(first)
    T1, X1 = b.get_poses(), b.get_points()
    cres = b.cull(E2_MAX)
    mask = b.get_obs_mask()
    for p, out in enumerate(bad):
        assert np.array_equal(mask[p], ~out)
        assert (cres[p].n_on_before, cres[p].n_culled, cres[p].starved, cres[p].status) == (out.size, int(out.sum()), 0, 0)
    rows2, res2 = b.solve(second)
    T2, X2, m2 = full_state(b)
    # stage 2 is the oracle on the filtered arrays from the values after stage 1
    for p, (pr, out) in enumerate(zip(probs, bad)):
        fp = filtered(pr, ~out)
        fp["pose_T"], fp["pt_X"] = b.poses_of(p, T1).copy(), b.points_of(p, X1).copy()
        o = O.Oracle(fp)
        orows, _ = o.solve(O.make_options(max_iter=6, **CULL_OPT))
        assert res2[p].status == 0 and res2[p].n_iter == 6
        assert_same_trajectory(rows2[p], orows)
        assert relerr(b.poses_of(p, T2), o.get_poses()) < 1e-6 and relerr(b.points_of(p, X2), o.get_points()) < 1e-6
        o.close()
    # a second cull finds nothing more and re-admits nothing
    again = b.cull(E2_MAX)
    assert [(c.n_on_before, c.n_culled) for c in again] == [(int((~o).sum()), 0) for o in bad]
    b.close()
    # solve_culled: the same bits in rows, results, values and mask
    c = BaBatch(probs)
    crows1, cres1, crows2, cres2, ccull = c.solve_culled(first, second, E2_MAX)
    Tc, Xc, mc = full_state(c)
    c.close()
    assert np.array_equal(Tc, T2) and np.array_equal(Xc, X2) and np.array_equal(mc, m2)
    for p in range(len(probs)):
        assert np.array_equal(row_bits(crows1[p]), row_bits(rows1[p])) and len(crows1[p]) == 5
        assert np.array_equal(row_bits(crows2[p]), row_bits(rows2[p])) and len(crows2[p]) == 6
        for x, y in ((cres1[p], res1[p]), (cres2[p], res2[p])):
            assert (x.n_iter, x.converged, x.n_rows, x.status, x.dropped_pivots) == \
                (y.n_iter, y.converged, y.n_rows, y.status, y.dropped_pivots)
        assert (ccull[p].n_on_before, ccull[p].n_culled, ccull[p].starved, ccull[p].status) == \
            (cres[p].n_on_before, cres[p].n_culled, cres[p].starved, cres[p].status)
    # the host route: solve, report, the rule in numpy, set_obs_mask, solve (the mask is applied
    # by compaction either way: bit for bit)
    h = BaBatch(probs)
    hrows1, _ = h.solve(first)
    rep = h.obs_report(first.threshold_huber_loss)
    h.set_obs_mask([(r["e2"] <= E2_MAX) & (r["depth"] > 0) for r in rep])
    hrows2, _ = h.solve(second)
    Th, Xh, mh = full_state(h)
    h.close()
    assert np.array_equal(mh, m2) and np.array_equal(Th, T2) and np.array_equal(Xh, X2)
    for p in range(len(probs)):
        assert np.array_equal(row_bits(hrows1[p]), row_bits(rows1[p]))
        assert np.array_equal(row_bits(hrows2[p]), row_bits(rows2[p]))


def test_solve_culled_rows_and_refusals(cull_scenes):
    probs, _ = cull_scenes
    from bundle_adjustment_solver_amd import _lib
    import ctypes as C
    b = BaBatch(probs[:1])
    first, second = make_options(max_iter=2, **CULL_OPT), make_options(max_iter=3, **CULL_OPT)
    T0, X0 = b.get_poses(), b.get_points()
    cap = 8                                 # rows 5..7 belong to neither stage: untouched
    rows = (_lib.BaIterInfo * cap)()
    for r in rows:
        r.cost = -7.0
    r1, r2 = (_lib.BaBatchResult * 1)(), (_lib.BaBatchResult * 1)()
    cres = (_lib.BaBatchCullResult * 1)()
    c = _lib.BaCullOptions(E2_MAX, 1)
    call = lambda f, s, cc, rw, cp, rr, cr: b.lib.ba_batch_solve_culled(
        b.b, f, s, cc, rw, cp, r1, rr, cr)
    assert call(C.byref(first), C.byref(second), C.byref(c), rows, cap, r2, cres) == 0
    assert (r1[0].n_rows, r2[0].n_rows) == (2, 3)
    assert [rows[i].cost == -7.0 for i in range(cap)] == [False] * 5 + [True] * 3
    state = full_state(b)
    bad_c = _lib.BaCullOptions(float("nan"), 1)
    zero = make_options(max_iter=0, **CULL_OPT)
    for args, msg in (((None, C.byref(second), C.byref(c), rows, cap, r2, cres), "null options"),
                      ((C.byref(first), C.byref(second), None, rows, cap, r2, cres), "null cull options"),
                      ((C.byref(first), C.byref(second), C.byref(bad_c), rows, cap, r2, cres), "e2_max"),
                      ((C.byref(first), C.byref(second), C.byref(c), rows, 4, r2, cres), "cap = 4"),
                      ((C.byref(first), C.byref(zero), C.byref(c), rows, cap, r2, cres), "max_num_iterations"),
                      ((C.byref(first), C.byref(second), C.byref(c), rows, cap, None, cres), "null result"),
                      ((C.byref(first), C.byref(second), C.byref(c), rows, cap, r2, None), "null cres")):
        assert call(*args) == -1
        assert msg in b.lib.ba_last_error().decode()
    assert b.lib.ba_batch_cull(b.b, C.byref(bad_c), cres) == -1 and b.lib.ba_batch_cull(b.b, C.byref(c), None) == -1
    assert all(np.array_equal(x, y) for x, y in zip(state, full_state(b)))   # a refusal changes nothing
    b.close()


# ---- 6. starvation and cheirality ---------------------------------------------------------------
def at_truth(sc):
    sc["T_wc_init"], sc["X_init"] = sc["T_wc_true"].copy(), sc["X_true"].copy()
    return sc


def test_starved_problem_keeps_its_mask(built):
    # pose 4 of the middle window keeps three landmarks only, all of them displaced
    st = at_truth(window(5, 37, False, 111))
    keep = (st["obs_pose"] != 4) | (st["obs_pt"] < 3)
    for k in OBS_KEYS:
        st[k] = st[k][keep]
    lone = np.flatnonzero(st["obs_pose"] == 4)
    assert lone.size == 3
    others = np.random.default_rng(5).choice(np.flatnonzero(st["obs_pose"] != 4), 6, replace=False)
    st, out_st = displaced(st, 7, np.concatenate([lone, others]))
    a, out_a = displaced(at_truth(window(6, 40, True, 112)), 8)
    c, out_c = displaced(at_truth(window(4, 12, True, 113)), 9)
    probs = [scenes.scaled_problem(s) for s in (a, st, c)]
    b = BaBatch(probs)
    pre = mask_of(probs[1], "random", 6)
    pre[lone] = True
    b.set_obs_mask([np.ones(out_a.size, bool), pre, np.ones(out_c.size, bool)])
    cres = b.cull(E2_MAX)
    mask = b.get_obs_mask()
    assert (cres[1].starved, cres[1].n_culled, cres[1].n_on_before, cres[1].status) == (1, 0, int(pre.sum()), 0)
    assert np.array_equal(mask[1], pre)
    for p, out in ((0, out_a), (2, out_c)):
        assert np.array_equal(mask[p], ~out)
        assert (cres[p].starved, cres[p].n_culled, cres[p].n_on_before) == (0, int(out.sum()), out.size)
    b.close()


def test_cheirality(built):
    sc = at_truth(window(5, 37, True, 114))
    q = 9
    sc["pt_fixed"] = sc["pt_fixed"].copy()
    sc["pt_fixed"][q] = True
    T0 = sc["T_wc_true"][0]
    sc["X_true"][q] = sc["X_init"][q] = T0[:3, 3] - 5.0 * T0[:3, 2]      # behind the first camera
    pr = scenes.scaled_problem(sc)
    _, depth = project_np(pr)
    behind = pr["obs_pt"] == q
    assert (depth[behind] < 0).all() and (depth[~behind] > 0).all()
    probs = [pr, scenes.scaled_problem(at_truth(window(4, 12, True, 115)))]
    b = BaBatch(probs)
    cres = b.cull(1e30, cull_behind=False)
    assert [c.n_culled for c in cres] == [0, 0] and all(m.all() for m in b.get_obs_mask())
    cres = b.cull(1e30, cull_behind=True)
    mask = b.get_obs_mask()
    assert [c.n_culled for c in cres] == [int(behind.sum()), 0]
    assert np.array_equal(mask[0], ~behind) and mask[1].all()
    b.close()


# ---- 7. facades --------------------------------------------------------------------------------
def facade_options(max_iter):
    o = Options()
    o.iteration_handle.max_num_iterations = max_iter
    o.convergence_handle.threshold_step_size = 0.0
    o.convergence_handle.threshold_cost_change = 0.0
    o.outlier_handle.threshold_huber_loss = CULL_OPT["huber"]
    o.trust_region_handle.initial_lambda = CULL_OPT["lambda0"]
    return o


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_cull_and_masks_are_the_raw_calls(built, cls):
    from bundle_adjustment_solver_amd.solver import covariance_to_user_units, marginal_to_user_units
    from test_batch_obs_abi import _facade_solver
    from test_gpu_batch_prior import _probs_of
    sigma = 0.7
    scs = [displaced(window(n_pose, n_pt, stereo, seed, pixel_sigma=0.3), seed + 3000)[0]
           for seed, stereo, n_pose, n_pt in CULL_SCENES[:2]]
    made = [_facade_solver(cls, sc) for sc in scs]
    solvers = [s for s, _ in made]
    probs = _probs_of(solvers)                   # registration order: camera by camera
    first, second = facade_options(5), facade_options(6)
    if cls is FullBundleAdjustmentSolverRefactor:
        from bundle_adjustment_solver_amd.solver import SolverType
        first.solver_type = second.solver_type = SolverType.LEVENBERG_MARQUARDT
    cull = CullOptions(first=first, chi2=25.0 / sigma ** 2)
    assert cull.e2_max_scaled(sigma) == pytest.approx(E2_MAX, rel=1e-15)
    # the raw calls, scaled units
    b = BaBatch(probs)
    _, res1, _, res2, cres = b.solve_culled(first.to_c(), second.to_c(), cull.e2_max_scaled(sigma))
    T, X, inl = b.get_poses(), b.get_points(), b.get_obs_mask()
    b.close()
    mk = oldest_marked(probs)
    r = BaBatch(probs)
    r.set_obs_mask(inl)
    cp, cq, _ = r.covariance(HUBER)
    Hl, bl, kl, _ = r.marginalize(np.concatenate(mk), HUBER)
    r.close()
    # covariance and marginalisation first (they read the registered values), then the solve
    cov = cls.ComputeCovarianceBatch(solvers, sigma_pixel=sigma, obs_masks=inl)
    marg = cls.MarginalizeBatch(solvers, [[made[k][1][int(np.flatnonzero(mk[k])[0])]] for k in range(2)],
                                sigma_pixel=sigma, obs_masks=inl)
    res, reports = cls.SolveBatch(solvers, second, sigma_pixel=sigma, cull=cull)
    for k, sv in enumerate(solvers):
        rep = reports[k]
        assert np.array_equal(rep["inliers"], inl[k]) and not rep["inliers"].all()
        assert (rep["n_culled"], rep["starved"], rep["n_iter_first"]) == (cres[k].n_culled, 0, res1[k].n_iter)
        assert rep["n_culled"] == int((~inl[k]).sum()) and res[k].n_iter == res2[k].n_iter == 6
        Tk, Xk = sv._host_arrays()[2], sv._host_arrays()[3]
        sl_p, sl_q = slice(b.pose_off[k], b.pose_off[k + 1]), slice(b.pt_off[k], b.pt_off[k + 1])
        assert np.array_equal(Tk, T[sl_p]) and np.array_equal(Xk, X[sl_q])
        up, uq = covariance_to_user_units(cp[sl_p], cq[sl_q], sigma)
        assert np.array_equal(cov[k][0], up) and np.array_equal(cov[k][1], uq)
        Hu, bu = marginal_to_user_units(Hl[k], bl[k], sigma)
        assert np.array_equal(marg[k][0], Hu) and np.array_equal(marg[k][1], bu)
    # without the keywords the calls return what they returned before: a plain result list
    plain = cls.SolveBatch(solvers, second)
    assert len(plain) == 2 and not isinstance(plain, tuple)


def test_cpp_facade_masks_and_cull_match_the_direct_calls(built):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "cpp", "build", "test_batch_obs")
    assert os.path.exists(exe), "cpp/build/test_batch_obs is not built (build() makes it)"
    r = subprocess.run([exe], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH OBS FACADE TEST PASSED" in r.stdout, r.stdout
