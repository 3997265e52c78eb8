"""The landmark-split paths — K chunks through the arenas of a BaStream, W shard
handles with a summed exchange — against the CPU ORACLE, on every case of
tests/split_cases.py (rejected steps, the solver's own stop, every linearisation /
Schur path a part can take, empty parts), and against the resident handle.

What a split run must reproduce (split_cases.check_against_oracle /
check_against_resident): the oracle's status sequence and converged flag, lambda
to 1e-12, trial cost and cost to 1e-7, final poses and points to 1e-6 (1e-5: cases
H, W, R); the resident handle's trajectory to 1e-11 (case A: 1.2e-10, see its table
entry) and parameters to 1e-9.  Each test prints the figures it measured
("SPLIT-FIGURE ...") before it asserts them.
"""
import numpy as np
import pytest

import split_cases as sc

pytestmark = pytest.mark.gpu

_resident = {}


def resident(cid):
    """(Result of the case's solve on the resident handle, Result of CONTINUE_ITERS
    more iterations for the cases that continue), computed once per case."""
    if cid not in _resident:
        from bundle_adjustment_solver_amd._lib import make_options
        from bundle_adjustment_solver_amd.solver import BaProblem
        case, pr = sc.CASES[cid], sc.problem(cid)
        p = sc.load(BaProblem(0), pr)
        rows, conv = p.solve(make_options(**case.opt()))
        first = sc.Result(sc.to_rows(rows), conv, p.get_poses(), p.get_points()[0])
        second = None
        if cid in sc.CONTINUED:
            rows, conv = p.solve(make_options(**case.opt(max_iter=sc.CONTINUE_ITERS)))
            second = sc.Result(sc.to_rows(rows), conv, p.get_poses(), p.get_points()[0])
        assert p.get_dropped_pivots() == 0
        p.close()
        _resident[cid] = (first, second)
    return _resident[cid]


def static_points(pr):
    """Points no solve may move: fixed ones and those without an observation."""
    return (pr["pt_fixed"] != 0) | (np.bincount(pr["obs_pt"], minlength=pr["pt_X"].shape[0]) == 0)


def check_paths(cid, infos):
    """The path a case is named for is really taken by its parts."""
    print("SPLIT-PATHS %s %d parts: %s" % (cid, len(infos), infos))
    schur = [i["schur"] for i in infos]
    if cid in ("A", "B", "C", "S"):
        assert all(s["grouped_landmarks"] > 0 for s in schur)
    if cid == "H":
        assert any(s["list_triples"] > 0 for s in schur)
        assert all(i["M"] >= 1 for i in infos)
    if cid == "W":
        assert any(i["mask"]["masked_landmarks"] > 0 for i in infos)
        # a group of more than 10 poses: the mean over the grouped landmarks exceeds 10
        assert any(s["groups64"] > 0 and s["grouped_pairs"] > 10 * s["grouped_landmarks"] for s in schur)
    if cid == "T":
        assert any(s["grouped_landmarks"] < 0.2 * i["M"] for s, i in zip(schur, infos))
        assert any(i["lin"]["chunks"] > 0 or i["lin"]["pose_major_observations"] > 0 for i in infos)
    if cid == "E1":
        assert infos[sc.E1_EMPTY]["M"] == 0
        assert all(i["M"] > 0 for k, i in enumerate(infos) if k != sc.E1_EMPTY)
    if cid == "E2":
        assert infos[sc.E2_EMPTY]["M"] == 280


def check_split_result(cid, kind, parts, res, label=""):
    """A split run against the oracle and against the resident handle."""
    case, pr = sc.CASES[cid], sc.problem(cid)
    ref = sc.oracle_run(cid)[0]
    full = resident(cid)[0]
    fo = sc.check_against_oracle(full, ref, case.tol_par)
    static = static_points(pr)
    assert np.array_equal(full.points[static], pr["pt_X"][static])
    eo = er = (float("nan"), float("nan"))
    try:
        eo = sc.check_against_oracle(res, ref, case.tol_par)
        er = sc.check_against_resident(res, full, case)
    finally:
        print("SPLIT-FIGURE %s %s %d%s: resident-vs-oracle traj %.2e par %.2e | split-vs-oracle traj %.2e par %.2e"
              " | split-vs-resident traj %.2e par %.2e" % ((cid, kind, parts, label) + fo + eo + er))
    assert np.array_equal(res.points[static], pr["pt_X"][static])
    if case.status is not None:
        assert sc.status_string(res.rows) == case.status


@pytest.mark.parametrize("cid,kind,parts", [s for s in sc.splits() if s[1] == "stream"],
                         ids=lambda v: str(v))
def test_streamed_split_matches_oracle_and_resident(cid, kind, parts, built):
    case, pr = sc.CASES[cid], sc.problem(cid)
    res, st = sc.run_streamed(pr, parts, case.opt(), keep=True)
    try:
        assert st.info()["n_chunks"] == parts
        check_split_result(cid, kind, parts, res)
        if cid in sc.CONTINUED:
            # a second solve continues from the streamed state, like the oracle's and the handle's
            from bundle_adjustment_solver_amd._lib import make_options
            rows, conv = st.solve(make_options(**case.opt(max_iter=sc.CONTINUE_ITERS)))
            res2 = sc.Result(sc.to_rows(rows), conv, st.get_poses(), st.get_points())
            ref2, full2 = sc.oracle_run(cid)[1], resident(cid)[1]
            eo = sc.check_against_oracle(res2, ref2, case.tol_par)
            worst = sc.same_rows(res2.rows, full2.rows, 1e-10)
            print("SPLIT-FIGURE %s stream %d continued: split-vs-oracle traj %.2e par %.2e | split-vs-resident"
                  " traj %.2e" % ((cid, parts) + eo + (worst,)))
            assert sc.relerr(res2.poses, full2.poses) < case.par_vs_resident
            assert sc.relerr(res2.points, full2.points) < case.par_vs_resident
    finally:
        st.close()
    check_paths(cid, sc.shard_infos(pr, parts))


@pytest.mark.parametrize("cid,kind,parts", [s for s in sc.splits() if s[1] == "shard"],
                         ids=lambda v: str(v))
def test_sharded_split_matches_oracle_and_resident(cid, kind, parts, built):
    case, pr = sc.CASES[cid], sc.problem(cid)
    run = sc.run_sharded(pr, parts, case.opt())
    n_pt = pr["pt_X"].shape[0]
    # owned masks partition the point set
    count = np.zeros(n_pt, int)
    for m in run.owned:
        count += m
    assert (count == 1).all()
    n_it = len(run.results[0].rows)
    assert len(set(run.calls)) == 1 and run.calls[0] >= 2 * n_it + 2, run.calls
    assert run.dropped == [0] * parts
    for r in range(parts):
        # replicated poses: the same bits on every shard
        assert np.array_equal(run.results[r].poses, run.results[0].poses), r
        # after gather_points every shard holds every point, bit-equal to its owner's values
        assert run.gathered_mask[r].all()
        assert np.array_equal(run.gathered[r], run.gathered[0]), r
        m = run.owned[r]
        assert np.array_equal(run.gathered[0][m], run.results[r].points[m]), r
    for r in range(parts):
        res = run.results[r]._replace(points=run.gathered[r])
        check_split_result(cid, kind, parts, res, label=" rank %d" % r)
    check_paths(cid, run.infos)


def test_own_stop_through_the_stepwise_stream_api(built):
    """Case S through ba_stream_lm_begin / lm_iterate / lm_sync in batches of five:
    20 iterations requested, 16 performed; the four past convergence are device-side
    no-ops, and so are four more."""
    from bundle_adjustment_solver_amd._lib import make_options
    case, pr = sc.CASES["S"], sc.problem("S")
    ref = sc.oracle_run("S")[0]
    cap = case.options["max_iter"]
    st = sc.open_stream(pr, 3)
    st.lm_begin(make_options(**case.opt()))
    seen = []
    for _ in range(4):
        st.lm_iterate(5)
        rows, n, conv, done = st.lm_sync(cap)
        seen.append((n, conv, done))
    assert seen == [(5, False, False), (10, False, False), (15, False, False), (16, True, True)], seen
    res = sc.Result(sc.to_rows(rows), conv, st.get_poses(), st.get_points())
    eo = sc.check_against_oracle(res, ref, case.tol_par)
    print("SPLIT-FIGURE S stream 3 stepwise: split-vs-oracle traj %.2e par %.2e" % eo)
    fresh = sc.run_streamed(pr, 3, case.opt())
    assert fresh.converged and [tuple(r) for r in fresh.rows] == [tuple(r) for r in res.rows]
    assert np.array_equal(fresh.poses, res.poses) and np.array_equal(fresh.points, res.points)
    st.lm_iterate(4)
    rows2, n2, conv2, done2 = st.lm_sync(cap)
    assert (n2, conv2, done2) == (16, True, True)
    assert [tuple(r) for r in sc.to_rows(rows2)] == [tuple(r) for r in res.rows]
    assert np.array_equal(st.get_poses(), res.poses) and np.array_equal(st.get_points(), res.points)
    st.close()


def test_zero_iterations_return_the_inputs(built):
    """Case A through three chunks with max_iter = 0: no rows, the inputs come back
    bit for bit (the point read-back takes pts[cur] out of every chunk's host image)."""
    from bundle_adjustment_solver_amd._lib import make_options
    case, pr = sc.CASES["A"], sc.problem("A")
    st = sc.open_stream(pr, 3)
    rows, conv = st.solve(make_options(**case.opt(max_iter=0)))
    assert rows == [] and not conv
    assert np.array_equal(st.get_poses(), pr["pose_T"])
    assert np.array_equal(st.get_points(), pr["pt_X"])
    st.close()


def test_unobserved_points_come_back_unchanged_from_every_split(built):
    """Case E2: the 300 appended, never-observed points (280 of them the whole of
    part 4) through five chunks and through five shards."""
    case, pr = sc.CASES["E2"], sc.problem("E2")
    tail = pr["pt_X"][-sc.E2_APPENDED:]
    res = sc.run_streamed(pr, sc.E2_PARTS, case.opt())
    assert np.array_equal(res.points[-sc.E2_APPENDED:], tail)
    assert not np.array_equal(res.points[:100], pr["pt_X"][:100])       # the observed ones moved
    run = sc.run_sharded(pr, sc.E2_PARTS, case.opt())
    assert int(run.owned[sc.E2_EMPTY].sum()) == 280
    for r in range(sc.E2_PARTS):
        assert np.array_equal(run.gathered[r][-sc.E2_APPENDED:], tail), r
        assert not np.array_equal(run.gathered[r][:100], pr["pt_X"][:100])
