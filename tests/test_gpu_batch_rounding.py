"""The batched full bundle adjustment (k_ba_batch<NPt>, k_ba_batch_marg<NPt>,
k_ba_batch_obs_report) held to ROUNDING level against the long-double restatement of
tests/xp_ref.py, in units of u * (the expression evaluated on magnitudes), u = 2^-53.  The
batched path has no stage getters, so it is judged on what it returns:

 1. The step of a one-iteration solve (max_iter = 1, thresholds 0) solves the FULL damped normal
    equations of the problem, linearised in long double at its own parameters
    (xp_ref.full_system_units): e <= 8 max(e64, 1) on pose rows and on landmark rows apart, e64
    the same figure of xp_ref's float64 step.  A landmark nobody observes, fixed poses and fixed
    points keep their bits.  The row: trial_cost against xp_ref.cost at the RETURNED values in the
    same rule; an accepted row logs the trial cost as its cost too (asserted bit for bit), so the cost
    at the inputs is held through cost_change = |trial cost - cost at the inputs| in units of both
    costs' scales, and directly on the SKIPPED row of test 2; damping_term to 1e-12 of the oracle's.
 2. A first step that is SKIPPED and a second that is accepted (max_iter = 2): the returned values
    solve the equations of the ORIGINAL inputs at the second step's damping (what row 0 logs: a row
    holds lambda after its update), from blocks the kernel only damped again.
 3. ba_batch_marginalize with the fixed pose 0 as the only mark eliminates nothing: H, bvec are the
    reduced camera system S, rhs at lambda 0 over the observed landmarks (xp_ref.reduced_system):
    e <= 8 max(e64, 1) and e <= n_terms + 8 on the lower triangle, H symmetric to the bit,
    elements without a term exactly 0.
 4. The observation report against xp_ref.project in the LINEARISATION form fx (x invz) + cx,
    which is what k_ba_batch_obs_report evaluates (ba_device_fn.h: project).

All windows of batch_rounding_cases.py of one lambda are ONE BaBatch (the 96-column instances);
those with at most 5 and at most 10 optimisable poses also form batches of their own, so that the
32- and 64-column instances are judged (the width is asserted through BaBatch.info).  The bounds
are earned by the CPU oracle in test_batch_rounding_ref.py.  Every figure is printed ("ROUNDING
batch ...") before it is asserted; the table of DESIGN.md is made of these lines.
"""
import numpy as np
import pytest

import batch_rounding_cases as BC
import xp_ref as X
from test_batch_rounding_ref import print_reduced, print_step, step_failures

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not X.LD_OK, reason=X.LD_REASON)]

WIDTHS = (32, 64, 96)
ACCEPTED = (BC.UPDATE, BC.UPDATE_TRUST_MORE)
REPORT_CASES = ("mono", "stereo", "huber", "unobserved")


def members(width):
    """the cases of the batch judged at this image width"""
    limit = {32: 5, 64: 10, 96: 16}[width]
    return [n for n in BC.CASE_NAMES if BC.free_poses(BC.cases()[n]) <= limit]


def one_step_params():
    return [(w, n, lam) for w in WIDTHS for n, lam in BC.passes() if n in members(w)]


class Batches:
    """One BaBatch per width, made on first use; one solve per (width, lambda, Huber threshold)."""

    def __init__(self):
        self.made, self.steps, self.margs = {}, {}, {}

    def batch(self, width):
        from bundle_adjustment_solver_amd.solver import BaBatch
        if width not in self.made:
            names = members(width)
            assert max(BC.free_poses(BC.cases()[n]) for n in names) > {32: 0, 64: 5, 96: 10}[width]
            b = BaBatch([BC.cases()[n] for n in names])
            assert b.info()["image_columns"] == width
            self.made[width] = (b, names, b.get_poses(), b.get_points())
        return self.made[width]

    def one_step(self, width, name, lam):
        """(rows, result, poses, points) of `name` after one iteration from the inputs"""
        from bundle_adjustment_solver_amd._lib import make_options
        key = (width, lam, BC.huber_of(name))
        if key not in self.steps:
            b, names, T0, X0 = self.batch(width)
            b.update_values(T0, X0)
            rows, res = b.solve(make_options(max_iter=1, thr_step=0.0, thr_cost=0.0, lambda0=lam, huber=key[2]))
            T, Xp = b.get_poses(), b.get_points()
            self.steps[key] = {n: (rows[p], res[p], b.poses_of(p, T).copy(), b.points_of(p, Xp).copy())
                               for p, n in enumerate(names)}
            b.update_values(T0, X0)
        return self.steps[key][name]

    def marginalized(self, width, name):
        """(H, bvec, kept, L, result) of `name` with the fixed pose 0 of every problem marked"""
        key = (width, BC.huber_of(name))
        if key not in self.margs:
            b, names, T0, X0 = self.batch(width)
            b.update_values(T0, X0)
            mark = np.zeros(b.n_pose, np.uint8)
            mark[b.pose_off[:-1]] = 1
            assert (b.pose_fixed[mark != 0] != 0).all()
            Hl, bl, kl, res = b.marginalize(mark, key[1])
            L = b.marg_pt.copy()
            self.margs[key] = {n: (Hl[p].copy(), bl[p].copy(), kl[p], b.points_of(p, L) != 0, res[p])
                               for p, n in enumerate(names)}
        return self.margs[key][name]

    def close(self):
        for b, _, _, _ in self.made.values():
            b.close()


@pytest.fixture(scope="module")
def batches(built):
    bs = Batches()
    yield bs
    bs.close()


def row_failures(tag, name, row, T, Xp):
    """trial cost at the returned values, cost change from the inputs"""
    bad = []
    for what, (e, y) in (("trial cost", BC.cost_figures(name, row.trial_cost, T, Xp)),
                         ("cost change", BC.cost_change_figures(name, row.cost_change, T, Xp))):
        print("ROUNDING batch %s %s: e %.3f, e64 %.3f" % (tag, what, e, y))
        if not X.within(e, y):
            bad.append("%s: e = %.3g > 8 max(e64 = %.3g, 1)" % (what, e, y))
    return bad


# ---- 1. the one-step solve ----------------------------------------------------------------------
@pytest.mark.parametrize("width,name,lam", one_step_params(), ids=lambda v: str(v))
def test_one_step_solves_the_damped_normal_equations(width, name, lam, batches):
    rows, res, T, Xp = batches.one_step(width, name, lam)
    assert res.status == 0 and res.dropped_pivots == 0 and res.n_rows == len(rows) == 1
    assert rows[0].iteration_status in ACCEPTED
    fig, e64 = BC.step_figures(name, BC.lambda_of(lam), T, Xp)
    tag = "%d columns %s lambda=%g" % (width, name, lam)
    print_step(tag, fig, e64)
    bad = step_failures(fig, e64) + row_failures(tag, name, rows[0], T, Xp)
    assert rows[0].cost == rows[0].trial_cost
    orow = BC.oracle_solve(name, lam)[0][0]
    assert orow.iteration_status == rows[0].iteration_status
    assert abs(rows[0].damping_term - orow.damping_term) <= 1e-12 * orow.damping_term
    pr = BC.cases()[name]
    if name == "small":
        x = X.recover_step(pr, X.Structure(pr), T, Xp)[0]
        w = np.sqrt((x[:, 3:] ** 2).sum(axis=1))
        assert (w < 1e-7).all() and (w > 0).all()               # se3_exp's small-angle branch, every pose
    if name == "unobserved":
        lone = np.bincount(pr["obs_pt"], minlength=len(pr["pt_X"])) == 0
        assert lone.sum() == 1 and np.array_equal(Xp[lone], pr["pt_X"][lone])
        assert not np.array_equal(Xp[~lone], pr["pt_X"][~lone])
    if name == "fixed only":
        assert not np.array_equal(Xp[[0, 5]], pr["pt_X"][[0, 5]])    # seen by fixed poses only: they move
    assert not bad, "\n".join(bad)


# ---- 2. rejected, then accepted -----------------------------------------------------------------
def test_step_after_a_rejected_one_solves_the_equations_of_the_inputs(built):
    from bundle_adjustment_solver_amd._lib import make_options
    from bundle_adjustment_solver_amd.solver import BaBatch
    name, pr = BC.REJECTED, BC.cases()[BC.REJECTED]
    b = BaBatch([pr])
    rows, res = b.solve(make_options(max_iter=2, thr_step=0.0, thr_cost=0.0, lambda0=BC.REJECTED_LAMBDA,
                                     huber=BC.huber_of(name)))
    T, Xp = b.get_poses(), b.get_points()
    b.close()
    rows, res = rows[0], res[0]
    orows = BC.oracle_solve(name, BC.REJECTED_LAMBDA, max_iter=2)[0]
    assert res.status == 0 and res.dropped_pivots == 0 and res.n_rows == len(rows) == 2
    assert rows[0].iteration_status == BC.SKIPPED and rows[1].iteration_status in ACCEPTED
    for a, o in zip(rows, orows):
        assert a.iteration_status == o.iteration_status
        assert abs(a.damping_term - o.damping_term) <= 1e-12 * o.damping_term
    lam1 = rows[0].damping_term                     # the damping of the second step
    assert lam1 > 2 * BC.REJECTED_LAMBDA
    fig, e64 = BC.step_figures(name, lam1, T, Xp)
    tag = "32 columns rejected lambda=%g" % lam1
    print_step(tag, fig, e64)
    bad = step_failures(fig, e64)
    e, y = BC.cost_figures(name, rows[0].cost, pr["pose_T"], pr["pt_X"])       # a SKIPPED row keeps the cost before
    print("ROUNDING batch %s cost at the inputs: e %.3f, e64 %.3f" % (tag, e, y))
    if not X.within(e, y):
        bad.append("cost at the inputs: e = %.3g > 8 max(e64 = %.3g, 1)" % (e, y))
    e, y = BC.cost_figures(name, rows[1].trial_cost, T, Xp)
    print("ROUNDING batch %s trial cost: e %.3f, e64 %.3f" % (tag, e, y))
    if not X.within(e, y):
        bad.append("trial cost: e = %.3g > 8 max(e64 = %.3g, 1)" % (e, y))
    assert rows[1].cost == rows[1].trial_cost
    assert not bad, "\n".join(bad)


# ---- 3. the reduced system through a marginalisation that eliminates nothing --------------------
def marg_params():
    return [(w, n) for w in WIDTHS for n in members(w)]


@pytest.mark.parametrize("width,name", marg_params(), ids=lambda v: str(v))
def test_marginalising_a_fixed_pose_returns_the_reduced_system(width, name, batches):
    pr = BC.cases()[name]
    H, bvec, kept, L, res = batches.marginalized(width, name)
    N = BC.free_poses(pr)
    assert res.status == 0 and res.dropped_pivots == 0 and res.n_marg_pose == 0 and res.n_kept == N
    assert np.array_equal(kept, np.flatnonzero(pr["pose_fixed"] == 0))
    assert np.array_equal(L, BC.observed_landmarks(pr)) and res.n_marg_pt == int(L.sum())
    assert H.shape == (6 * N, 6 * N) and np.array_equal(H, H.T)
    fig = X.reduced_figures(H, bvec, BC.reduced_reference(name))
    print_reduced("%d columns %s" % (width, name), fig)
    bad = X.reduced_failures(fig)
    assert not bad, "\n".join(bad)


# ---- 4. the observation report ------------------------------------------------------------------
def report_reference(pr, huber, dt):
    """(r2 (n, 2), e2, w, depth) as VS, user order, from xp_ref.project in its linearisation form"""
    Xc, r = X.project(pr, pr["pose_T"], pr["pt_X"], dt, False)[3::3]
    n = r.v.shape[0]
    absr = X.VS(np.abs(r.v).sum(axis=1), r.s.sum(axis=1))
    hub, one = X.vs(np.full(n, np.float64(huber)), dt), X.vs(np.ones(n), dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = X.where(absr.v > hub.v, hub * X.recip(absr), one)
    return dict(r2=r, e2=(r * r).sum(axis=1), w=w, depth=Xc[:, 2])


@pytest.fixture(scope="module")
def reports(built):
    from bundle_adjustment_solver_amd.solver import BaBatch
    b = BaBatch([BC.cases()[n] for n in REPORT_CASES])
    out = {}
    for hub in sorted({BC.huber_of(n) for n in REPORT_CASES}):
        rep = b.obs_report(hub)
        out.update({n: {k: v.copy() for k, v in rep[p].items()} for p, n in enumerate(REPORT_CASES)
                    if BC.huber_of(n) == hub})
    b.close()
    return out


@pytest.mark.parametrize("name", REPORT_CASES)
def test_observation_report_is_within_rounding(name, reports):
    pr, hub = BC.cases()[name], BC.huber_of(name)
    ref, yard = report_reference(pr, hub, X.LD), report_reference(pr, hub, np.float64)
    bad = []
    for k in ("r2", "e2", "w", "depth"):
        e, e64 = X.rounding_units(reports[name][k], ref[k]), X.rounding_units(yard[k].v, ref[k])
        print("ROUNDING batch report %s %s: e %.3f, e64 %.3f" % (name, k, e, e64))
        if not X.within(e, e64):
            bad.append("%s: e = %.3g > 8 max(e64 = %.3g, 1)" % (k, e, e64))
    w = reports[name]["w"]
    assert np.array_equal(w < 1, ref["w"].v < 1)                 # the same branch of the weight everywhere
    if name == "huber":
        assert (w < 1).mean() > 0.2
    assert not bad, "\n".join(bad)
