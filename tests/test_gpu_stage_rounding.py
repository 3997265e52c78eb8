"""Every stage of one LM iteration on the handle path, and the dense solve alone, held to
ROUNDING level: the device against the long-double restatement of tests/xp_ref.py, in
units of u * (the stage's expression evaluated on magnitudes), u = 2^-53.

Each stage is judged from what the previous stage left on the device (read back with the
getters), so an error is charged to the kernel that made it:
  A a C b B_ji, y, model change, step norms, committed poses and points, trial cost:
      e <= 8 max(e64, 1), e64 the same figure of xp_ref's float64 run on the same inputs;
  S, rhs: the same, and e <= n_terms + 8 (n_terms: landmarks that contribute to the element);
  Cinv_i, Cinv_i b_i: <= 8 u kappa_inf(C_i) max|Cinv_i| against the exact inverse of the device's
      damped C_i, asserted apart for kappa <= 1e6 and above; C_i = 0 gives exact zeros;
  x: backward error eta(S_dev, rhs_dev, x_dev) <= 4 max(eta of LAPACK's Cholesky, u), no dropped pivot.
Elements whose expression has no term at all (scale 0) must be exactly 0; nothing else is
left out of a maximum.  Every figure is printed ("ROUNDING ...") before it is asserted; the
table of DESIGN.md ("Rounding-level figures") is made of these lines.
"""
import os

import numpy as np
import pytest

import xp_ref as X
from test_gpu_dense_cone import block_tridiagonal_spd, environment

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not X.LD_OK, reason=X.LD_REASON)]

# scene -> (scene of xp_ref.scene_problem, BA_* knobs of the handle)
HANDLES = {name: (name, {}) for name in X.SPLIT_SCENES + (X.SMALL,)}
HANDLES["A slim"] = ("A", {"BA_PAIR_OBS": "0"})       # the 64-byte record {G, w}
HANDLES["A full"] = ("A", {"BA_PAIR_SLIM": "0"})      # the 96-byte record {K, X_ij}
PASSES = X.passes() + [("A slim", X.LAMBDA), ("A full", X.LAMBDA)]


@pytest.fixture(scope="module")
def handles(built):
    """One finalized handle per scene, made on first use, closed with the module."""
    import split_cases as sc
    from bundle_adjustment_solver_amd.solver import BaProblem
    made = {}

    def get(name):
        if name not in made:
            scene, env = HANDLES[name]
            with environment(**env):
                made[name] = sc.load(BaProblem(0), X.scene_problem(scene))
        return made[name]
    yield get
    for g in made.values():
        g.close()


def check_paths(name, g, pr):
    """The path a scene is there for is really taken (the assertions the tests of these
    scenes make in test_gpu_split_parity.py, test_gpu_pair_slim.py and test_gpu_pair_obs.py)."""
    schur, lin, mask = g.get_schur_info(), g.get_lin_info(), g.get_mask_info()
    print("ROUNDING %s paths: form %d %s %s %s" % (name, g.get_pair_form(), schur, lin, mask))
    if name in ("A", "A slim", "A full", "B", "C", X.SMALL):
        assert schur["grouped_landmarks"] > 0
    if name in ("A", "A slim", "A full"):
        assert schur["groups32"] > 0 and schur["groups64"] == 0
        assert g.get_pair_form() == {"A": 2, "A slim": 1, "A full": 0}[name]
        rec = g.get_pair_record_info()
        if name == "A full":
            assert rec["slim_pairs"] == 0
        else:
            assert rec["slim_pairs"] > 0.7 * rec["pairs"]
    if name == "B":
        assert schur["groups64"] > 0
    if name == "C":
        assert pr["pt_fixed"][5] and not (pr["obs_pt"] == 17).any()
    if name == "H":
        # (the triple list is what get_schur_info shows; that its triples go through k_schur_partial
        # is implied by the plan, not observed here)
        assert schur["list_triples"] > 0
    if name == "W":
        assert mask["masked_landmarks"] > 0 and schur["super_runs"] > 0
        assert schur["groups64"] > 0 and schur["grouped_pairs"] > 10 * schur["grouped_landmarks"]
    if name == "T":
        assert schur["grouped_landmarks"] < 0.2 * g.M
        assert lin["chunks"] > 0 or lin["pose_major_observations"] > 0
    if name == "G":
        assert pr["cam_intr"].shape[0] > 8
    if name == "R":
        key = pr["obs_cam"].astype(np.int64) * 10**6 + pr["obs_pose"] * 10**3 + pr["obs_pt"]
        assert np.unique(key).size < key.size


def device_pass(g, pr, lam, huber):
    """One pass through the stages from the scene's own parameters; the step is committed, read
    back, and the handle is given its parameters again."""
    g.update_values(pr["pose_T"], pr["pt_X"])
    assert np.array_equal(g.get_poses(), pr["pose_T"]) and np.array_equal(g.get_points()[0], pr["pt_X"])
    g.get_dropped_pivots(reset=True)
    D = {}
    g.stage_linearize(lam, huber)
    D["A"], D["a"] = g.get_A()
    D["C"], D["b"] = g.get_C()
    D["Cinv"], D["Cinvb"] = g.get_Cinv()
    D["pairs"] = g.get_pairs()
    g.stage_schur()
    D["S"], D["rhs"] = g.get_S()
    g.stage_solve_reduced()
    g.stage_backsub_update()
    D["x"], D["y"] = g.get_xy()
    D["cost"], D["model"], D["sp"], D["sq"] = g.stage_scalars()
    g.stage_commit(True)
    D["poses"], D["points"] = g.get_poses(), g.get_points()[0]
    D["dropped"] = g.get_dropped_pivots()
    g.update_values(pr["pose_T"], pr["pt_X"])
    return D


@pytest.mark.parametrize("name,lam", PASSES, ids=lambda v: str(v))
def test_every_stage_is_within_rounding_of_the_long_double_reference(name, lam, handles):
    pr = X.scene_problem(HANDLES[name][0])
    huber = X.huber_of(HANDLES[name][0])
    g = handles(name)
    check_paths(name, g, pr)
    st = X.Structure(pr)
    assert (g.N, g.M, g.P) == (st.N, st.M, st.P)
    D = device_pass(g, pr, lam, huber)
    fig = X.measure_stages(pr, st, lam, huber, D)
    tag = "%s lambda=%g" % (name, lam)
    X.report(tag, fig)
    print("ROUNDING %s dropped pivots: %d" % (tag, D["dropped"]))
    if name == "C":
        absr = np.abs(X.project(pr, pr["pose_T"], pr["pt_X"], np.float64, False)[-1].v).sum(axis=1)
        assert (absr > huber).mean() > 0.2                      # the robust branch is active
        assert fig["kappa"][1] == 1                             # the unobserved landmark: C = 0
    if name == "R":
        assert fig["kappa"][1] == 1
        if lam == X.LAMBDA_FLOOR:
            assert fig["kappa"][0] >= 8                         # spd3_inverse's pivoted fallback
    if name == X.SMALL:
        assert (np.linalg.norm(D["x"][:, 3:], axis=1) < 1e-7).all() and np.abs(D["x"]).max() > 0
    bad = X.failures(fig)
    assert not bad, "\n".join(bad)
    assert D["dropped"] == 0


# ---------------------------------------------------------------------------------------
# the dense solve alone
# ---------------------------------------------------------------------------------------
def _orthogonal(n, rng):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def wishart(n, rng):
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T + n * np.eye(n)
    return 0.5 * (A + A.T)


def graded(n, rng):
    """D (Q Q^T / n + I) D with D spanning four decades, randomly permuted: condition ~ 1e8."""
    Q = rng.standard_normal((n, n))
    d = rng.permutation(10.0 ** np.linspace(-2, 2, n))
    A = (Q @ Q.T / n + np.eye(n)) * np.outer(d, d)
    return 0.5 * (A + A.T)


def spectrum(cond):
    def make(n, rng):
        V = _orthogonal(n, rng)
        A = (V * 10.0 ** np.linspace(0, -np.log10(cond), n)) @ V.T
        return 0.5 * (A + A.T)
    return make


def block_tridiagonal(tiles, nb, rng, cond=1e8):
    """The generator of test_gpu_dense_cone.py with its diagonal shift lowered until the
    condition is `cond`: A0 + s I has the spectrum of the unshifted A0 moved by s."""
    A, b = block_tridiagonal_spd(tiles, nb, rng, shift=0.0)
    ev = np.linalg.eigvalsh(A)
    return A + (ev[-1] - cond * ev[0]) / (cond - 1) * np.eye(A.shape[0]), b


FAMILIES = {"wishart": wishart, "graded": graded, "spectrum 1e6": spectrum(1e6), "spectrum 1e10": spectrum(1e10)}
DENSE_N = (17, 100, 330)


@pytest.fixture(scope="module")
def dense_handles(built):
    from bundle_adjustment_solver_amd.solver import BaProblem
    made = {}
    for nb in (32, 64):
        with environment(BA_DENSE_NB=str(nb)):     # no other BA_DENSE_* knob: the default launch path
            made[nb] = BaProblem(0)
    yield made
    for g in made.values():
        g.close()


@pytest.mark.parametrize("family", list(FAMILIES) + ["block tridiagonal"])
@pytest.mark.parametrize("nb", [32, 64])
def test_dense_solve_backward_error_is_within_four_times_lapacks(nb, family, dense_handles):
    assert not [k for k in os.environ if k.startswith("BA_DENSE_")]
    rng = np.random.default_rng(1000 + nb + 7 * (list(FAMILIES) + ["block tridiagonal"]).index(family))
    if family == "block tridiagonal":
        systems = [block_tridiagonal(9, nb, rng)]
    else:
        systems = [(A, rng.standard_normal(A.shape[0])) for A in (FAMILIES[family](n, rng) for n in DENSE_N)]
    bad = []
    for A, b in systems:
        n = A.shape[0]
        x, _ = dense_handles[nb].dense_spd_solve(A, b)
        assert np.isfinite(x).all()
        x_lapack = X.lapack_solve(A, b)
        eta, eta_lapack = X.backward_error(A, b, x), X.backward_error(A, b, x_lapack)
        print("ROUNDING dense nb=%d %s n=%d cond %.1e: eta %.3f u, LAPACK %.3f u"
              % (nb, family, n, np.linalg.cond(A), eta / X.U, eta_lapack / X.U))
        if eta > 4 * max(eta_lapack, X.U):
            bad.append((n, eta / X.U, eta_lapack / X.U))
        if family == "graded":
            # the rows span four decades and the normwise eta above sees the largest only (1e-5 u for
            # any solver): the same criterion once more on the symmetrically equilibrated system,
            # which a Cholesky factorisation solves as well (it commutes with a diagonal scaling)
            eq, eq_lapack = (X.backward_error(*X.equilibrated(A, b, v)) for v in (x, x_lapack))
            print("ROUNDING dense nb=%d %s n=%d equilibrated: eta %.3f u, LAPACK %.3f u"
                  % (nb, family, n, eq / X.U, eq_lapack / X.U))
            if eq > 4 * max(eq_lapack, X.U):
                bad.append((n, "equilibrated", eq / X.U, eq_lapack / X.U))
    assert not bad, bad
