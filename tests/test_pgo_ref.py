"""Host tests of the pose-graph reference (pgo_ref.py) and of the scenes the GPU tests compare
trajectories on (pgo_cases.py).  No GPU.

(a) fitness: on every scene and option set of pgo_cases.TRAJECTORY every gain ratio of the
    reference is at least 0.1 relative away from 0.25 and from 0.5 and every iteration changes
    chi-square by at least 1e-6 relative, so that no status rests on rounding; statuses 0, 1
    and 2 all occur, also decisively inside one scene (g60, g330: rejections followed by
    accepted steps).
(b) on two noise-free scenes the reference reaches the truth to 1e-8.
(c) the full solver's control restated without observations rejects every step on the 60-pose
    scene: the reason the pose graph has a solver of its own.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import make_options

import pgo_cases as cases
import pgo_ref


@pytest.mark.parametrize("name", cases.TRAJECTORY)
def test_trajectory_scene_is_fit(name):
    g = cases.scene(name)
    rows, conv, _ = cases.reference(name)
    assert len(rows) == cases.SCENES[name][2] and not conv
    prev = pgo_ref.chi2(g["pose_T"], g["rels"])
    gn = bool(cases.SCENES[name][1].get("gauss_newton"))
    for it, r in enumerate(rows):
        change = abs(prev - r.trial_cost) / prev
        margin = np.inf if gn else min(abs(r.rho - 0.25) / 0.25, abs(r.rho - 0.5) / 0.5)
        print("%s it %d status %d rho %.4f margin %.3f relative change %.3e"
              % (name, it, r.iteration_status, r.rho, margin, change))
        assert margin >= 0.1 and change >= 1e-6
        prev = r.cost


def test_every_status_occurs():
    seen = set()
    for name in cases.TRAJECTORY:
        seen |= {r.iteration_status for r in cases.reference(name)[0]}
    assert seen == {0, 1, 2}
    for name in ("g60", "g330"):   # a rejection, later an accepted step: the records are reused, then rebuilt
        st = [r.iteration_status for r in cases.reference(name)[0]]
        assert 2 in st and any(s != 2 for s in st[st.index(2):]), st
        assert {0, 1, 2} <= set(st), st


def test_factor_counts_straddle_one_linearisation_workgroup():
    counts = [len(cases.scene(n)["rels"]["j"]) for n in ("g60_63", "g60", "g60_65")]
    assert counts == [63, 64, 65]
    sizes = {n: int((cases.scene(n)["pose_fixed"] == 0).sum()) for n in ("g2", "n5", "n6", "n10", "g12")}
    assert sizes == dict(g2=1, n5=5, n6=6, n10=10, g12=11)


def test_scenes_hold_both_orientations_a_twin_and_fixed_ends():
    g = cases.scene("g60")
    j, k, fx = g["rels"]["j"], g["rels"]["k"], g["pose_fixed"]
    assert (j > k).any() and (j < k).any()
    pairs = list(zip(j.tolist(), k.tolist()))
    assert any((b, a) in pairs for a, b in pairs)
    assert any(fx[a] and not fx[b] for a, b in pairs) and any(fx[b] and not fx[a] for a, b in pairs)


@pytest.mark.parametrize("name", sorted(cases.EXACT))
def test_reference_reaches_the_truth_without_noise(name):
    g = cases.scene(name)
    assert pgo_ref.pose_distance(g["pose_T"], g["truth"]) > 1e-4
    rows, _, T = pgo_ref.lm(g, make_options(max_iter=8, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4))
    err = pgo_ref.pose_distance(T, g["truth"])
    print(name, "distance to the truth", err, "chi2", rows[-1].cost)
    assert err <= 1e-8


def test_full_solver_control_rejects_every_step():
    """sum of norms against the quadratic model, times 100: the gain ratio is far below 0.25 at
    chi-square of 1e8, and after a rejection the trial cost is kept as `previous`"""
    g = cases.scene("g60")
    assert pgo_ref.chi2(g["pose_T"], g["rels"]) > 1e5
    rows = pgo_ref.lm_full_control(g, make_options(max_iter=8, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4))
    print([(r.iteration_status, r.rho) for r in rows])
    assert [r.iteration_status for r in rows] == [2] * 8
    assert all(abs(r.rho) < 0.1 for r in rows)
    # the chi-square control makes progress on the same scene
    ref = cases.reference("g60")[0]
    assert ref[-1].cost < 0.1 * pgo_ref.chi2(g["pose_T"], g["rels"])
