"""CPU pins of the point-only reference (tests/point_only_ref.py): what makes the GPU
comparison of test_gpu_point_only.py meaningful.  On the 40-landmark scene the one-landmark
oracle solves take different numbers of iterations, reject steps on many landmarks, and stay
far from every decision boundary (gain ratio against 0.25 / 0.5, the stopping quantities
against their thresholds), so a GPU trajectory that differs by rounding takes the same
decisions.  The scene is fixed; if a change of it breaks a pin, another seed is chosen —
the comparison is not loosened."""
import numpy as np
import pytest

import point_only_ref as R
from bundle_adjustment_solver_amd import scenes

THR = 1e-5   # default threshold_step_size and threshold_cost_change


@pytest.fixture(scope="module", params=[False, True], ids=["mono", "stereo"])
def solved(request, built):
    return R.cached(request.param)


def test_every_landmark_is_solved_and_the_counts_differ(solved):
    pr, ref = solved
    assert sorted(ref) == list(range(40))
    its = [ref[i]["n_iter"] for i in range(40)]
    assert all(1 <= n <= 30 for n in its)
    assert len(set(its)) >= 5, its                      # landmarks of one wave stop at different iterations
    assert min(its) < 15 and max(its) > 20, its
    for i in range(40):
        assert np.isfinite(ref[i]["X"]).all()
        rows = ref[i]["rows"]
        assert rows[-1].cost < rows[0].trial_cost or rows[-1].cost <= rows[0].cost


def test_a_third_of_the_landmarks_reject_a_step(solved):
    _, ref = solved
    skipped = sum(any(r.iteration_status == 2 for r in v["rows"]) for v in ref.values())
    assert 3 * skipped >= 40, skipped


def test_no_gain_ratio_is_near_a_decision_boundary(solved):
    _, ref = solved
    worst = min(abs(r.rho - edge) / edge for v in ref.values() for r in v["rows"] for edge in (0.25, 0.5))
    assert worst > 0.5, worst


def test_no_last_row_is_near_a_stopping_threshold(solved):
    """The stop is decided on the last row (an earlier row did not stop: both quantities were
    above their thresholds there, and the first that is below ends the loop)."""
    _, ref = solved
    worst = np.inf
    for v in ref.values():
        rows = v["rows"]
        last = rows[-1]
        prev_cost = rows[-2].trial_cost if len(rows) > 1 else None
        if prev_cost is None:
            continue
        cost_change = abs(last.trial_cost - prev_cost)
        for q in (last.abs_step, cost_change):
            worst = min(worst, abs(q - THR) / THR)
    assert worst > 1e-3, worst


def test_earlier_rows_are_clear_of_the_thresholds_too(solved):
    _, ref = solved
    worst = np.inf
    for v in ref.values():
        rows = v["rows"]
        for k in range(1, len(rows) - 1):
            cost_change = abs(rows[k].trial_cost - rows[k - 1].trial_cost)
            worst = min(worst, (rows[k].abs_step - THR) / THR, (cost_change - THR) / THR)
    assert worst > 1e-3, worst      # every earlier row was above both thresholds, by a margin


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_triangulation_of_noise_free_pixels_returns_the_true_point(stereo):
    sc = scenes.synthetic_ba_scene(8, 40, 5, stereo, seed=11, pixel_sigma=0.0)
    sc["T_wc_init"] = sc["T_wc_true"]
    pr = scenes.scaled_problem(sc)
    X = R.triangulate_reference(pr)
    assert np.abs(X - sc["X_true"] * 0.01).max() < 1e-9


def test_the_triangulated_start_is_solved_as_well(built):
    for stereo in (False, True):
        pr, ref = R.cached(stereo, triangulated=True)
        assert sorted(ref) == list(range(40))
        assert all(np.isfinite(v["X"]).all() for v in ref.values())


def test_the_team_edge_scene_is_clear_of_the_boundaries_too(built):
    pr, ref = R.cached_edges()
    assert np.bincount(pr["obs_pt"]).tolist() == list(R.EDGE_COUNTS) and sorted(ref) == list(range(10))
    rho, stop = R.margins(ref, THR)
    assert rho > 0.5 and stop > 1e-3, (rho, stop)
    for gn in (False, True):
        for stereo in (False, True):
            rho, stop = R.margins(R.cached(stereo, gauss_newton=gn)[1], THR)
            assert rho > 0.5 and stop > 1e-3, (gn, stereo, rho, stop)
