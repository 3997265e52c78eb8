"""The case table of tests/split_cases.py, checked without a GPU: what every case
of test_gpu_split_parity.py is named for must hold on the CPU oracle and on the
host-only landmark partition, so that a changed scene or option cannot silently
turn a case into one more all-accepted five-view solve."""
import time

import numpy as np
import pytest

import split_cases as sc
from bundle_adjustment_solver_amd.sharding import partition_points
from oracle import oracle_py as O


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def part_sizes(pr, parts):
    """(points, optimisable points, observations) owned by every part."""
    owner = partition_points(pr, parts)
    assert owner.min() >= 0 and owner.max() < parts
    return (np.bincount(owner, minlength=parts), np.bincount(owner[pr["pt_fixed"] == 0], minlength=parts),
            np.bincount(owner[pr["obs_pt"]], minlength=parts))


@pytest.mark.parametrize("cid", list(sc.CASES))
def test_oracle_run_is_finite_small_and_as_recorded(cid):
    case, pr = sc.CASES[cid], sc.problem(cid)
    assert pr["obs_pt"].size <= 75_000
    o = O.Oracle(pr)
    t0 = time.perf_counter()
    o.solve(O.make_options(**case.opt()))
    seconds = time.perf_counter() - t0
    o.close()
    assert seconds < 5.0, seconds          # (T, the largest: 0.25 s; H: 0.5 s)
    first, second, cost0 = sc.oracle_run(cid)
    assert len(first.rows) >= 5 and np.isfinite(cost0)
    for res in (first, second):
        assert np.isfinite(res.poses).all() and np.isfinite(res.points).all()
        assert all(np.isfinite([r.trial_cost, r.cost, r.damping_term]).all() for r in res.rows)
    if case.status is not None:
        assert sc.status_string(first.rows) == case.status
    assert len(second.rows) == sc.CONTINUE_ITERS or second.converged
    # the second solve really continued: it did not start from the inputs again
    assert abs(second.rows[0].trial_cost - first.rows[0].trial_cost) > 1e-3 * first.rows[0].trial_cost


def test_every_listed_split_is_in_the_table():
    got = sc.splits()
    assert len(got) == len(set(got)) == 47
    want = {"A": ((1, 2, 3, 5), (2, 3, 8)), "B": ((1, 2, 3, 5), (2, 3, 8)), "H": ((2, 3), (2, 3, 8)),
            "E1": ((4,), (4,)), "E2": ((5,), (5,))}
    for cid, case in sc.CASES.items():
        assert (case.streamed, case.sharded) == want.get(cid, ((2, 3), (2, 3))), cid
    assert list(sc.CASES) == ["A", "B", "C", "S", "H", "W", "T", "G", "R", "E1", "E2"]


@pytest.mark.parametrize("cid", ["A", "B"])
def test_rejected_steps_in_mid_run_with_decisions_far_from_their_thresholds(cid):
    # over 12 iterations the recorded strings; the case is their prefix (see split_cases.py)
    o = O.Oracle(sc.problem(cid))
    rows12 = sc.to_rows(o.solve(O.make_options(**sc.CASES[cid].opt(max_iter=12)))[0])
    o.close()
    assert sc.status_string(rows12) == sc.AB_STATUS_12[cid]
    assert min(min(abs(r.rho - 0.25), abs(r.rho - 0.5)) for r in rows12) >= 0.04
    rows = sc.oracle_run(cid)[0].rows
    s = sc.status_string(rows)
    assert sc.AB_STATUS_12[cid].startswith(s)
    assert any(a == "2" and b != "2" for a, b in zip(s, s[1:])), s     # a revert, then the loop goes on
    assert "2" in s[:-1] and s[0] != "2"
    margin = min(min(abs(r.rho - 0.25), abs(r.rho - 0.5)) for r in rows)
    assert margin >= 0.04, margin
    if cid == "B":
        assert "222" in s                                              # lambda raised three times in a row


def test_case_c_takes_the_robust_branch_with_a_fixed_and_an_unobserved_landmark():
    pr = sc.problem("C")
    assert pr["pt_fixed"][5] and not (pr["obs_pt"] == 17).any()
    # robust branch: the cost at Huber 0.005 differs from the squared-error cost
    o = O.Oracle(pr)
    o.linearize(0.005)
    C_rob = o.get_C()[0].copy()
    o.linearize(1.0)
    C_sq = o.get_C()[0]
    changed = np.abs(C_rob - C_sq).reshape(C_sq.shape[0], -1).max(axis=1) > 0
    assert changed.mean() > 0.5, changed.mean()     # most landmarks have a down-weighted observation
    first = sc.oracle_run("C")[0]
    assert np.array_equal(first.points[17], pr["pt_X"][17]) and np.array_equal(first.points[5], pr["pt_X"][5])


def test_case_s_stops_by_the_solvers_own_rule_with_a_margin_on_both_sides():
    case = sc.CASES["S"]
    first, _, cost0 = sc.oracle_run("S")
    assert first.converged and len(first.rows) == 16 < case.options["max_iter"]
    thr = case.options["thr_step"]
    assert thr == case.options["thr_cost"] == 1e-6
    q = sc.stop_quantities(first.rows, cost0)
    assert q[-1] * 2 <= thr, q[-1]
    assert min(q[:-1]) >= 2 * thr, min(q[:-1])


def test_partition_facts_of_the_table():
    # H at W = 8: every shard has a landmark, each of them on the triple list (150 poses > 128 pairs)
    pr = sc.problem("H")
    npt, nopt, nobs = part_sizes(pr, 8)
    assert nopt.min() >= 1 and nopt.tolist() == [2, 1, 2, 1, 2, 1, 2, 1]
    assert np.bincount(pr["obs_pt"]).min() > 128
    # E1: part 2 has observations and points, none of them optimisable; fixing them kept the partition
    pr = sc.problem("E1")
    npt, nopt, nobs = part_sizes(pr, sc.E1_PARTS)
    assert npt[sc.E1_EMPTY] == 100 and nobs[sc.E1_EMPTY] == 1000 and nopt[sc.E1_EMPTY] == 0
    assert (np.delete(nopt, sc.E1_EMPTY) > 0).all()
    free = dict(pr)
    free["pt_fixed"] = np.zeros_like(pr["pt_fixed"])
    assert np.array_equal(partition_points(free, sc.E1_PARTS), partition_points(pr, sc.E1_PARTS))
    assert sc.status_string(sc.oracle_run("E1")[0].rows)[-1] == "2"
    # E2: part 4 owns 280 points, all never observed; the oracle leaves the appended points alone
    pr = sc.problem("E2")
    npt, nopt, nobs = part_sizes(pr, sc.E2_PARTS)
    assert npt[sc.E2_EMPTY] == nopt[sc.E2_EMPTY] == 280 and nobs[sc.E2_EMPTY] == 0
    assert (np.delete(nobs, sc.E2_EMPTY) > 0).all()
    assert pr["obs_pt"].max() < pr["pt_X"].shape[0] - sc.E2_APPENDED
    for res in sc.oracle_run("E2")[:2]:
        assert np.array_equal(res.points[-sc.E2_APPENDED:], pr["pt_X"][-sc.E2_APPENDED:])
    # the other cases: no part is empty, so their splits exercise kernels, not guards
    for cid in ("A", "B", "C", "S", "W", "T", "G", "R"):
        case, pr = sc.CASES[cid], sc.problem(cid)
        for parts in sorted(set(case.streamed + case.sharded) - {1}):
            npt, nopt, nobs = part_sizes(pr, parts)
            assert nopt.min() > 0 and nobs.min() > 0, (cid, parts)


def test_scene_properties_the_cases_are_named_for():
    assert sc.problem("G")["cam_intr"].shape[0] > 8
    assert sc.problem("B")["cam_intr"].shape[0] == 1 and sc.problem("A")["cam_intr"].shape[0] == 2
    pr = sc.problem("T")
    assert np.bincount(pr["obs_pt"]).min() == 40                      # more than the 32 slots of a group
    pr = sc.problem("W")
    per_lm = np.bincount(pr["obs_pt"])
    assert per_lm.max() <= 20 and np.median(per_lm) > 10 and len(set(per_lm.tolist())) > 3
    pr = sc.problem("R")
    cnt = np.bincount(pr["obs_pt"], minlength=200)
    assert (cnt[:10] == 1).all() and cnt[10] == 0
    key = pr["obs_cam"].astype(np.int64) * 10**6 + pr["obs_pose"] * 10**3 + pr["obs_pt"]
    assert np.unique(key).size < key.size                             # duplicate observations are there
