"""The bounds of test_gpu_batch_rounding.py earned on the CPU: on every window of
batch_rounding_cases.py the CPU oracle, a second and independent fp64 implementation, meets in long
double what the batched kernels are asked for ("what the oracle achieves, a kernel can be asked for"):
  the step of a one-iteration solve solves the full damped normal equations of the problem
      (xp_ref.full_system_units): e <= 8 max(e64, 1) on pose rows and on landmark rows, e64 the same
      figure of xp_ref's own float64 step;
  S and rhs at lambda 0 over the observed landmarks (xp_ref.reduced_system): the same rule, and
      e <= n_terms + 8.
A case that failed here would be unfit, not the bound too narrow.  Also pinned: xp_ref.se3_log, the
status of the rejected-step case, and the property each edge case is there for.  Every figure is
printed ("ROUNDING batch ...")."""
import numpy as np
import pytest

import batch_rounding_cases as BC
import xp_ref as X
from oracle import oracle_py as O

if not X.LD_OK:
    pytest.skip(X.LD_REASON, allow_module_level=True)

EPS_LD = float(np.finfo(X.LD).eps)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def print_step(tag, fig, e64):
    print("ROUNDING batch %s pose rows: e %.3f, e64 %.3f; landmark rows: e %.3f, e64 %.3f"
          % (tag, fig[0], e64[0], fig[1], e64[1]))


def step_failures(fig, e64):
    return ["%s rows: e = %.3g > 8 max(e64 = %.3g, 1)" % (k, e, y)
            for k, e, y in zip(("pose", "landmark"), fig, e64) if not X.within(e, y)]


def print_reduced(tag, fig):
    for k in ("S", "rhs"):
        print("ROUNDING batch %s %s: e %.3f, e64 %.3f, max(e - n_terms) %.3f (<= %g)"
              % ((tag, k) + fig[k] + fig[k + " cap"]))


# ---- se3_log ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0.0, 1e-12, 1e-9, 3e-8, 5e-7, 2e-6, 1e-4, 1e-2, 0.3, 0.97])
def test_se3_log_inverts_se3_exp(size):
    """se3_exp(se3_log(dR, dt)) gives (dR, dt) back to 4 eps_ld of the magnitudes se3_exp carries for
    every element (its VS scale: 1 on the diagonal of dR, about |w| beside it, about |v| for dt), on
    both sides of se3_exp's branch at 1e-7 and of se3_log's at 1e-6 and up to nearly 1 rad."""
    rng = np.random.default_rng(int(size * 1e13) % 9973)
    w = rng.standard_normal((40, 3))
    w *= size / np.linalg.norm(w, axis=1, keepdims=True)
    x = np.concatenate([rng.standard_normal((40, 3)) * max(size, 1e-3), w], 1)
    dR, dt = X.se3_exp(x, X.LD)
    v, ww = X.se3_log(dR.v, dt.v)
    th = np.sqrt((ww * ww).sum(axis=1))
    assert (th < 1e-6).all() == (size < 1e-6)                     # the branch the case is there for
    back_R, back_t = X.se3_exp(np.concatenate([v, ww], 1), X.LD)
    eR = float((np.abs(back_R.v - dR.v) / dR.s).max()) / EPS_LD if size > 0 else float(np.abs(back_R.v - dR.v).max())
    et = float((np.abs(back_t.v - dt.v) / dt.s).max()) / EPS_LD
    print("ROUNDING batch se3_log |w| = %g: dR %.2f eps_ld, dt %.2f eps_ld" % (size, eR, et))
    assert eR <= 4 and et <= 4


def test_recover_step_returns_the_step_of_an_update():
    """recover_step of update(x, y) in long double is (x, y), although the stored rotations are
    orthogonal to fp64 rounding only: to 4 eps_ld of 1 + |x| for the poses (the composition with a
    pose of unit size) and of |X| + |y| for the points."""
    pr = BC.cases()["stereo"]
    st = X.Structure(pr)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((st.N, 6)) * np.array([1e-3, 1e-9, 1e-5, 0.1])[:, None]
    y = rng.standard_normal((st.M, 3)) * 1e-4
    P, Q = X.update(pr, st, x, y, X.LD)
    xr, yr = X.recover_step(pr, st, P.v, Q.v)
    ex = float((np.abs(xr - x) / (1 + np.abs(x))).max()) / EPS_LD
    ey = float((np.abs(yr - y) / (np.abs(pr["pt_X"][st.pt_of_i]) + np.abs(y))).max()) / EPS_LD
    print("ROUNDING batch recover_step: x %.2f eps_ld, y %.2f eps_ld" % (ex, ey))
    assert ex <= 4 and ey <= 4


# ---- the cases are what they are named for ------------------------------------------------------
def test_cases_have_the_edges_they_are_named_for():
    cs = BC.cases()
    assert list(cs) == BC.CASE_NAMES
    for n in (1, 4, 5, 6, 10, 11, 15, 16):
        assert BC.free_poses(cs["N%d" % n]) == n
    for m in (255, 256, 257):
        pr = cs["M%d" % m]
        assert BC.free_poses(pr) == 5 and int(BC.observed_landmarks(pr).sum()) == m and len(pr["cam_intr"]) == 1
    for k in (63, 64, 65):
        pr = cs["obs%d" % k]
        per_pose = np.bincount(pr["obs_pose"], minlength=5)
        assert per_pose.tolist() == [65, 65, k, k, k] and len(pr["cam_intr"]) == 1
    assert len(cs["mono"]["cam_intr"]) == 1 and len(cs["stereo"]["cam_intr"]) == 2
    pr = cs["last writer"]
    key = pr["obs_pt"].astype(np.int64) * 64 + pr["obs_pose"]
    assert np.unique(key).size * 2 == key.size
    last_cam = {k: c for k, c in zip(key, pr["obs_cam"])}
    assert 0 < sum(last_cam.values()) < len(last_cam)              # both cameras win somewhere
    pr = cs["huber"]
    absr = np.abs(X.project(pr, pr["pose_T"], pr["pt_X"], np.float64, False)[-1].v).sum(axis=1)
    assert (absr > BC.huber_of("huber")).mean() > 0.2              # the robust branch is active
    assert BC.huber_of("huber") != 0.005 and abs(BC.huber_of("huber") - 0.005) < 1e-9
    pr = cs["fixed only"]
    assert pr["pt_fixed"].sum() == 3
    lone = np.arange(0, 41, 5)
    assert (pr["pose_fixed"][pr["obs_pose"][np.isin(pr["obs_pt"], lone)]] != 0).all()
    pr = cs["unobserved"]
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_X"]))
    assert (seen == 0).sum() == 1 and not pr["pt_fixed"].any()
    for name, pr in cs.items():
        # every observed optimisable landmark is seen by the fixed pose 0: marking it selects them all
        assert pr["pose_fixed"][0] and BC.free_poses(pr) <= 16
        by0 = np.zeros(len(pr["pt_X"]), bool)
        by0[pr["obs_pt"][pr["obs_pose"] == 0]] = True
        assert np.array_equal(by0 & (pr["pt_fixed"] == 0), BC.observed_landmarks(pr)), name


# ---- 1. the one-step solve ----------------------------------------------------------------------
@pytest.mark.parametrize("name,lam", BC.passes(), ids=lambda v: str(v))
def test_oracle_step_solves_the_damped_normal_equations(name, lam):
    rows, T, Xp = BC.oracle_solve(name, lam)
    assert len(rows) == 1 and rows[0].iteration_status in (BC.UPDATE, BC.UPDATE_TRUST_MORE)
    fig, e64 = BC.step_figures(name, BC.lambda_of(lam), T, Xp)
    tag = "oracle %s lambda=%g" % (name, lam)
    print_step(tag, fig, e64)
    bad = step_failures(fig, e64)
    for what, (e, y) in (("trial cost", BC.cost_figures(name, rows[0].trial_cost, T, Xp)),
                         ("cost change", BC.cost_change_figures(name, rows[0].cost_change, T, Xp))):
        print("ROUNDING batch %s %s: e %.3f, e64 %.3f" % (tag, what, e, y))
        if not X.within(e, y):
            bad.append("%s: e = %.3g > 8 max(e64 = %.3g, 1)" % (what, e, y))
    assert rows[0].cost == rows[0].trial_cost                      # an accepted row logs the trial cost twice
    assert not bad, "\n".join(bad)
    if name == "small":
        x = X.recover_step(BC.cases()[name], X.Structure(BC.cases()[name]), T, Xp)[0]
        w = np.sqrt((x[:, 3:] ** 2).sum(axis=1))
        assert (w < 1e-7).all() and (w > 0).all()


# ---- 2. rejected, then accepted -----------------------------------------------------------------
def test_rejected_case_is_skipped_then_accepted():
    rows, T, Xp = BC.oracle_solve(BC.REJECTED, BC.REJECTED_LAMBDA, max_iter=2)
    print("ROUNDING batch oracle rejected: status %s rho %s lambda %s" % (
        [r.iteration_status for r in rows], [r.rho for r in rows], [r.damping_term for r in rows]))
    assert rows[0].iteration_status == BC.SKIPPED and np.isfinite(rows[0].trial_cost)
    assert rows[1].iteration_status in (BC.UPDATE, BC.UPDATE_TRUST_MORE)
    assert rows[0].rho < 0.25 - 1 and rows[1].rho > 0.5 + 1         # far from both thresholds
    # the lambda of the second step is the one row 0 holds (a row logs lambda after its update)
    lam1 = rows[0].damping_term
    assert lam1 == pytest.approx(3 * BC.REJECTED_LAMBDA, rel=1e-6)
    fig, e64 = BC.step_figures(BC.REJECTED, lam1, T, Xp)
    print_step("oracle rejected lambda=%g" % lam1, fig, e64)
    bad = step_failures(fig, e64)
    pr = BC.cases()[BC.REJECTED]
    e, y = BC.cost_figures(BC.REJECTED, rows[0].cost, pr["pose_T"], pr["pt_X"])   # a SKIPPED row keeps the cost before
    print("ROUNDING batch oracle rejected lambda=%g cost at the inputs: e %.3f, e64 %.3f" % (lam1, e, y))
    assert X.within(e, y) and not bad, "\n".join(bad)
    e, y = BC.cost_figures(BC.REJECTED, rows[1].trial_cost, T, Xp)
    print("ROUNDING batch oracle rejected lambda=%g trial cost: e %.3f, e64 %.3f" % (lam1, e, y))
    assert X.within(e, y) and rows[1].cost == rows[1].trial_cost
    # and the step that was refused is not the one returned: at lambda 0.1 the returned values miss
    fig0 = BC.step_figures(BC.REJECTED, BC.lambda_of(BC.REJECTED_LAMBDA), T, Xp)[0]
    assert min(fig0) > 1e6


# ---- 3. the reduced system ----------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.CASE_NAMES)
def test_oracle_reduced_system_is_within_the_bounds(name):
    pr, hub = BC.cases()[name], BC.huber_of(name)
    L = BC.observed_landmarks(pr)
    o = O.Oracle(X.only_landmarks(pr, L))          # (the oracle keeps observations of fixed points: given none)
    o.linearize(hub)
    o.damp_invert(0.0)
    o.schur()
    S, rhs = o.get_S()
    o.close()
    fig = X.reduced_figures(S, rhs, BC.reduced_reference(name))
    print_reduced("oracle %s" % name, fig)
    bad = X.reduced_failures(fig)
    assert not bad, "\n".join(bad)


def test_reduced_system_leaves_out_observations_of_fixed_points():
    pr = BC.cases()["fixed only"]
    st, L = X.Structure(pr), BC.observed_landmarks(pr)
    fixed_obs = (pr["pt_fixed"][pr["obs_pt"]] != 0) & (pr["pose_fixed"][pr["obs_pose"]] == 0)
    assert fixed_obs.sum() > 0
    S = X.reduced_system(pr, st, 1.0, np.float64, L)[0].v
    lin = X.linearize(pr, st, 1.0, 0.0, np.float64)            # every observation
    full = X.schur(lin["A"].v, lin["a"].v, lin["B"].v, st.pair_i, st.pair_j, X.pinv3(lin["C"].v, np.float64)[0],
                   lin["b"].v, np.float64)[0].v
    assert np.abs(S - full).max() > 1e-3 * np.abs(full).max()
