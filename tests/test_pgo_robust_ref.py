"""Host tests of the robust pose-graph reference (pgo_robust_ref.py) and of the scenes the GPU
tests compare on (pgo_robust_cases.py).  No GPU.

(a) w = rho' by central differences for each kind, on both sides of the Huber knee; s = 0 gives
    w = 1 and rho = 0 for every kind.
(b) the two outlier scenes: without a kernel the false closures bend the trajectory (distance to
    the clean solution >= 1.0); Geman-McClure comes back to <= 0.02 and Cauchy to <= 0.3, every
    false closure ends with w < 1e-2 and every true closure with w > 0.8.  Measured (40 / 70
    poses): none 6.2 / 4.9, Cauchy 0.057 / 0.19, Geman-McClure 0.0033 / 0.0024, largest outlier
    weight 2.2e-4 / 4.2e-4 (Cauchy), smallest inlier weight 0.93: a factor of at least 5 on each.
(c) fitness of the trajectory scenes: every gain ratio at least 0.1 relative away from 0.25 and
    0.5, every iteration moves the cost by at least 1e-6 relative; statuses 0, 1 and 2 all occur,
    and r60_huber, r60_cauchy and r60_gm hold a decisive rejection followed by an accepted step.
"""
import numpy as np
import pytest

import pgo_cases
import pgo_ref
import pgo_robust_cases as cases
import pgo_robust_ref as ref


@pytest.mark.parametrize("kind", [ref.NONE, ref.HUBER, ref.CAUCHY, ref.GM])
def test_weight_is_the_derivative_of_rho(kind):
    c = 3.0
    for s in (1e-3, 0.5, 4.0, 8.9, 9.1, 30.0, 1e3, 1e6):   # the Huber knee is at c^2 = 9
        h = 1e-5 * s
        fd = (ref.rho(kind, c, s + h) - ref.rho(kind, c, s - h)) / (2.0 * h)
        w = ref.weight(kind, c, s)
        print(kind, s, float(w), float(fd))
        assert abs(fd - w) <= 1e-6 * max(w, 1e-12) + 1e-9


def test_huber_is_continuous_at_the_knee():
    c = 3.0
    assert ref.rho(ref.HUBER, c, 9.0) == 9.0 and ref.weight(ref.HUBER, c, 9.0) == 1.0
    up = np.nextafter(9.0, 10.0)
    assert abs(ref.rho(ref.HUBER, c, up) - 9.0) < 1e-14 * 9 * 4 and abs(ref.weight(ref.HUBER, c, up) - 1.0) < 1e-15 * 4


@pytest.mark.parametrize("kind", [ref.NONE, ref.HUBER, ref.CAUCHY, ref.GM])
def test_zero_s_gives_unit_weight(kind):
    with np.errstate(all="raise"):
        assert ref.weight(kind, 30.0, 0.0) == 1.0 and ref.rho(kind, 30.0, 0.0) == 0.0


def test_kind_zero_is_the_plain_reference():
    g = pgo_cases.scene("g12")
    opt = pgo_cases.options("g12")
    a = pgo_ref.lm(g, opt)
    b = ref.lm(dict(g, kind=np.zeros(len(g["rels"]["j"]), np.int32), scale=np.zeros(len(g["rels"]["j"]))), opt)
    for x, y in zip(a[0], b[0]):
        assert x.iteration_status == y.iteration_status and x.damping_term == y.damping_term
        assert abs(x.trial_cost - y.trial_cost) <= 1e-12 * abs(x.trial_cost)
    assert pgo_ref.pose_distance(a[2], b[2]) < 1e-9


@pytest.mark.parametrize("name", sorted(cases.OUTLIERS))
def test_outlier_scene_needs_and_rewards_a_kernel(name):
    g, bad, good = cases.outlier_scene(name)
    truth_s = ref.factor_s(g["truth"], g["rels"])
    print(name, "s at the truth: outliers >= %.3g, inlier closures <= %.3g" % (truth_s[bad].min(), truth_s[good].max()))
    assert truth_s[bad].min() > 1e3 * cases.SCALE ** 2 and truth_s[good].max() < cases.SCALE ** 2
    clean = cases.outlier_clean(name)
    assert pgo_ref.pose_distance(clean, g["truth"]) < 0.2   # the measurement noise
    dist, wout, win = {}, {}, {}
    for kind in (ref.NONE, ref.CAUCHY, ref.GM):
        T = cases.outlier_reference(name, kind)[2]
        gk = cases.with_kernels(g, kind, "closures") if kind else g
        _, w = ref.report(T, gk)
        dist[kind], wout[kind], win[kind] = pgo_ref.pose_distance(T, clean), w[bad].max(), w[good].min()
        print("%s kind %d: distance to the clean solution %.4g, largest outlier weight %.3g, smallest inlier-closure "
              "weight %.3g" % (name, kind, dist[kind], wout[kind], win[kind]))
    assert dist[ref.NONE] >= 1.0
    assert dist[ref.GM] <= 0.02 and dist[ref.CAUCHY] <= 0.3
    for kind in (ref.CAUCHY, ref.GM):
        assert wout[kind] < 1e-2 and win[kind] > 0.8


@pytest.mark.parametrize("name", cases.TRAJECTORY)
def test_trajectory_scene_is_fit(name):
    g = cases.scene(name)
    rows, conv, _ = cases.reference(name)
    assert len(rows) == cases.SCENES[name][4] and not conv
    prev = ref.cost(g["pose_T"], g)
    for it, r in enumerate(rows):
        change = abs(prev - r.trial_cost) / prev
        margin = min(abs(r.rho - 0.25) / 0.25, abs(r.rho - 0.5) / 0.5)
        print("%s it %d status %d rho %.4f margin %.3f relative change %.3e"
              % (name, it, r.iteration_status, r.rho, margin, change))
        assert margin >= 0.1 and change >= 1e-6
        prev = r.cost


def test_robust_scenes_hold_every_status_and_every_kind():
    seen = set()
    for name in cases.TRAJECTORY:
        seen |= {r.iteration_status for r in cases.reference(name)[0]}
    assert seen == {0, 1, 2}
    for name in ("r60_huber", "r60_cauchy", "r60_gm"):   # a rejection, later an accepted step
        st = [r.iteration_status for r in cases.reference(name)[0]]
        assert 2 in st and 0 in st and any(s != 2 for s in st[st.index(2):]), st
    counts = {name: len(cases.scene(name)["rels"]["j"]) for name in ("r60_huber", "r60_mixed", "r60_cauchy")}
    assert counts == dict(r60_huber=63, r60_mixed=64, r60_cauchy=65)
    kd = cases.scene("r60_mixed")["kind"]
    assert set(kd[:64].tolist()) == {0, 1, 2, 3}   # all four kinds inside one linearisation workgroup
    # the kernels bite: on every scene some weight is far from 1 at the start
    for name in cases.TRAJECTORY:
        g = cases.scene(name)
        _, w = ref.report(g["pose_T"], g)
        assert w.min() < 0.5, name
