"""The 64-byte pair record {G, w} of the covisibility groups (ba_device.h kWSlim):
k_lin_grp writes it, k_schur_grp / k_schur_grp_wide, the group role of
k_backsub_update, ba_covariance and the host's block getter rebuild {K, X_ij} from it,
the lane's pose and the landmark's point.  Blocks, reduced system and LM trajectories
against the CPU oracle at the tolerances of test_gpu_parity.py, on the smallest
shapes that take each kernel form; the 96-byte record (BA_PAIR_SLIM=0, BA_NO_LINGRP=1)
as the other side of a comparison; streamed, sharded and covariance paths."""
import threading

import numpy as np
import pytest

import cov_ref
from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import BaProblem, BaStream
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

RTOL_BLOCK = 1e-10   # B_ji, C_i, b_i, A_j, a_j (test_gpu_parity.RTOL_BLOCK)
RTOL_S = 1e-9        # S and rhs (test_gpu_parity.test_schur_solve_backsub)


def load(p, pr, rank=0, world=1):
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    if world > 1:
        p.set_shard(rank, world)
    p.finalize()
    return p


def make_gpu(pr, env=None, monkeypatch=None):
    """A finalized handle; the BA_* knobs are read once, when the handle is created."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return load(BaProblem(0), pr)
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def blockwise_relerr(a, b):
    """max over blocks of |a - b|_max / |b|_max; a block that is zero in b is zero in a."""
    a = np.asarray(a).reshape(a.shape[0], -1)
    b = np.asarray(b).reshape(b.shape[0], -1)
    den = np.abs(b).max(axis=1)
    num = np.abs(a - b).max(axis=1)
    z = den == 0
    assert (num[z] == 0).all()
    return (num[~z] / den[~z]).max() if (~z).any() else 0.0


SHAPES = {
    # name: (scene, knobs, kernel form it is there for)
    "stereo5": (lambda: scenes.synthetic_ba_scene(40, 3000, 5, True, seed=21, pixel_sigma=1.0), {}),
    "stereo5_steps2": (lambda: scenes.synthetic_ba_scene(40, 3000, 5, True, seed=21, pixel_sigma=1.0),
                       {"BA_LIN_STEPS": "2"}),      # pieces cut a group, partial last steps
    "mono10": (lambda: scenes.synthetic_ba_scene(24, 1500, 10, False, seed=21, pixel_sigma=1.0), {}),  # 64-wide image
    "stereo16": (lambda: scenes.synthetic_ba_scene(56, 5000, 16, True, seed=77, pixel_sigma=0.2), {}),  # k_schur_grp_wide
    "dropout": (lambda: scenes.synthetic_ba_scene(40, 6000, 5, True, seed=41, pixel_sigma=0.4, dropout=0.15), {}),
    "hover": (lambda: scenes.hover_scene(6, 400, 3, seed=31), {}),   # d = 4, two fixed poses inside every pattern
}
_problems = {}


def problem(name):
    """The scaled problem of a shape and the oracle's blocks at (lambda, huber): computed once."""
    if name not in _problems:
        pr = scenes.scaled_problem(SHAPES[name][0]())
        lam, hub = 1.3, 0.7
        o = O.Oracle(pr)
        o.linearize(hub)
        o.damp_invert(lam)
        o.schur()
        ref = dict(lam=lam, hub=hub, cost=o.cost(), A=o.get_A(), C=o.get_C(), pairs=o.get_pairs(), S=o.get_S())
        _problems[name] = (pr, ref)
    return _problems[name]


def check_blocks(g, ref):
    """Blocks of the handle (already linearised at ref's lambda / huber, Schur done) against
    the oracle's: every figure is printed before it is asserted."""
    A, a = g.get_A()
    Cm, b = g.get_C()
    pi, pj, W = g.get_pairs()
    opi, opj, oW = ref["pairs"]
    key, okey = np.lexsort((pj, pi)), np.lexsort((opj, opi))
    assert pi.shape == opi.shape and (pi[key] == opi[okey]).all() and (pj[key] == opj[okey]).all()
    S, rhs = g.get_S()
    errs = dict(A=blockwise_relerr(A, ref["A"][0]), a=blockwise_relerr(a, ref["A"][1]),
                C=blockwise_relerr(Cm, ref["C"][0]), b=blockwise_relerr(b, ref["C"][1]),
                B=blockwise_relerr(W[key], oW[okey]), S=relerr(S, ref["S"][0]), rhs=relerr(rhs, ref["S"][1]))
    print("block errors:", {k: "%.2e" % v for k, v in errs.items()})
    for k in ("A", "a", "C", "b", "B"):
        assert errs[k] <= RTOL_BLOCK, (k, errs[k])
    assert errs["S"] <= RTOL_S and errs["rhs"] <= RTOL_S, errs


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_blocks_and_reduced_system_match_oracle(name, built, monkeypatch):
    pr, ref = problem(name)
    g = make_gpu(pr, SHAPES[name][1], monkeypatch)
    rec, info = g.get_pair_record_info(), g.get_schur_info()
    print(name, rec, info)
    # the slim path really is the one under test, in the kernel form the shape is there for
    assert rec["slim_pairs"] > 0.7 * rec["pairs"]
    if name == "mono10":
        assert info["groups64"] > 0
    if name == "dropout":
        mi = g.get_mask_info()
        assert mi["masked_landmarks"] > 0 and mi["padded_pairs"] > 0
    if name == "stereo5_steps2":
        assert g.get_lin_info()["group_pieces"] > info["groups32"]
    g.stage_linearize(ref["lam"], ref["hub"])
    g.stage_schur()
    assert relerr(g.stage_cost(), ref["cost"]) < 1e-12
    check_blocks(g, ref)


@pytest.mark.parametrize("name", ["stereo5", "stereo16", "dropout"])
def test_lm_trajectory_matches_oracle(name, built, monkeypatch):
    """Status and lambda sequences identical to the oracle's, trial costs to 1e-7."""
    pr, _ = problem(name)
    g = make_gpu(pr, SHAPES[name][1], monkeypatch)
    assert g.get_pair_record_info()["slim_pairs"] > 0
    kw = dict(max_iter=8, thr_step=0, thr_cost=0, huber=0.7)
    rows, _ = g.solve(make_options(**kw))
    orows, _ = O.Oracle(pr).solve(O.make_options(**kw))
    assert len(rows) == len(orows) == 8
    for k, (a, b) in enumerate(zip(rows, orows)):
        print(k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
              "%.3e" % (abs(a.trial_cost - b.trial_cost) / abs(b.trial_cost)))
        assert a.iteration_status == b.iteration_status, k
        assert a.damping_term == b.damping_term, k
        assert abs(a.trial_cost - b.trial_cost) <= 1e-7 * abs(b.trial_cost), k


def test_the_96_byte_record_gives_the_same_reduced_system(built, monkeypatch):
    """BA_PAIR_SLIM=0 keeps {K, X_ij} for the grouped pairs: S and rhs of the two record
    forms agree to 1e-12 (the tolerance of test_covisibility_groups_equal_the_super_run_path)."""
    pr, ref = problem("stereo5")
    out = []
    for env in ({}, {"BA_PAIR_SLIM": "0"}):
        g = make_gpu(pr, env, monkeypatch)
        rec = g.get_pair_record_info()
        g.stage_linearize(ref["lam"], ref["hub"])
        g.stage_schur()
        out.append((rec,) + g.get_S() + (g.get_pairs()[2],))
    (ra, Sa, rhsa, Wa), (rb, Sb, rhsb, Wb) = out
    assert ra["slim_pairs"] > 0 and rb["slim_pairs"] == 0 and ra["pairs"] == rb["pairs"]
    print("S %.2e rhs %.2e B %.2e" % (relerr(Sa, Sb), relerr(rhsa, rhsb), blockwise_relerr(Wa, Wb)))
    assert relerr(Sa, Sb) <= 1e-12 and relerr(rhsa, rhsb) <= 1e-12
    assert blockwise_relerr(Wa, Wb) <= 1e-12


def test_chunk_linearisation_of_a_grouped_plan_keeps_the_96_byte_record(built, monkeypatch):
    """BA_NO_LINGRP=1: the groups feed k_schur_grp, but k_lin_landmarks writes every pair:
    no slim pair, and the result equals the oracle's as above."""
    pr, ref = problem("stereo5")
    g = make_gpu(pr, {"BA_NO_LINGRP": "1"}, monkeypatch)
    assert g.get_pair_record_info()["slim_pairs"] == 0
    assert g.get_schur_info()["grouped_landmarks"] > 0.7 * g.M and g.get_lin_info()["group_pieces"] == 0
    g.stage_linearize(ref["lam"], ref["hub"])
    g.stage_schur()
    check_blocks(g, ref)


def same_rows(rows, frows, rtol=1e-11):
    assert len(rows) == len(frows)
    for k, (a, b) in enumerate(zip(rows, frows)):
        assert a.iteration_status == b.iteration_status, k
        assert abs(a.damping_term - b.damping_term) <= 1e-12 * b.damping_term, k
        assert abs(a.trial_cost - b.trial_cost) <= rtol * abs(b.trial_cost), k
        assert abs(a.cost - b.cost) <= rtol * abs(b.cost), k


_resident = {}


def resident_run():
    """The resident solve of the stereo-5 scene: the reference of the streamed and the sharded run."""
    if not _resident:
        pr, _ = problem("stereo5")
        opt = make_options(max_iter=8, thr_step=0, thr_cost=0)
        full = load(BaProblem(0), pr)
        assert full.get_pair_record_info()["slim_pairs"] > 0
        rows, _ = full.solve(opt)
        _resident.update(pr=pr, opt=opt, rows=rows, P=full.get_poses(), X=full.get_points()[0])
    return _resident


def test_streamed_run_equals_the_resident_run(built):
    """Three chunks through the arena: the chunk handles run the same group kernels on the
    same record form; trajectory to 1e-11 as in test_gpu_streaming.py."""
    r = resident_run()
    st = load(BaStream(0, 3, 64 << 20), r["pr"])
    rows, _ = st.solve(r["opt"])
    same_rows(rows, r["rows"])
    assert relerr(st.get_poses(), r["P"]) < 1e-9
    assert relerr(st.get_points(), r["X"]) < 1e-9


def test_two_shards_in_one_process_equal_the_resident_run(built):
    """Two shard handles on the one card, each on its own thread, the all-reduce hook
    summing the bound buffers at a barrier (test_gpu_sharded.py): per iteration status,
    lambda and trial cost to 1e-11 of the resident run, owned points to 1e-9."""
    import torch
    r = resident_run()
    pr, opt, world = r["pr"], r["opt"], 2
    sh = [load(BaProblem(0), pr, k, world) for k in range(world)]
    assert all(s.get_pair_record_info()["slim_pairs"] > 0 for s in sh)
    bufs = []
    for s in sh:
        per = []
        for which in (0, 1, 2):
            n = s.reduce_buffer_size(which)
            t = torch.zeros(n, dtype=torch.float64, device="cuda")
            s.bind_reduce_buffer(which, t.data_ptr(), n)
            per.append(t)
        bufs.append(per)
    barrier = threading.Barrier(world)

    def make_hook(rank):
        def hook(which, ptr, n, stream):
            torch.cuda.ExternalStream(stream).synchronize()
            barrier.wait()
            if rank == 0:
                tot = bufs[0][which] + bufs[1][which]
                bufs[0][which].copy_(tot)
                bufs[1][which].copy_(tot)
                torch.cuda.synchronize()
            barrier.wait()
            return 0
        return hook

    for k in range(world):
        sh[k].set_allreduce(make_hook(k))
    out, owned, errs = [None] * world, [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            out[rank] = sh[rank].solve(opt)
            owned[rank] = sh[rank].get_points()
        except Exception as e:  # noqa
            errs.append((rank, repr(e)))
            barrier.abort()

    th = [threading.Thread(target=run, args=(k,)) for k in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    seen = np.zeros(r["X"].shape[0], bool)
    for k in range(world):
        same_rows(out[k][0], r["rows"])
        X, m = owned[k]
        assert relerr(X[m], r["X"][m]) < 1e-9
        seen |= m
    assert seen.all()
    assert np.array_equal(sh[0].get_poses(), sh[1].get_poses())
    assert relerr(sh[0].get_poses(), r["P"]) < 1e-9


def test_covariance_after_a_solve_matches_the_host_inverse(built):
    """ba_covariance places W_ji Cinv_i from the slim records: pose and point blocks
    against the dense host inverse of the full normal matrix (tests/cov_ref.py), after a
    solve has moved the accepted buffers."""
    huber = 1.0
    pr = scenes.scaled_problem(scenes.synthetic_ba_scene(n_pose=12, n_pt=150, window=5, stereo=True, seed=12, n_fixed=5))
    p = load(BaProblem(0), pr)
    assert p.get_pair_record_info()["slim_pairs"] > 0
    p.solve(make_options(max_iter=3, thr_step=0, thr_cost=0, huber=huber))
    p.stage_linearize(0.0, huber)
    A, _ = p.get_A()
    Cm, _ = p.get_C()
    pi, pj, W = p.get_pairs()
    H = cov_ref.full_normal_matrix(A, Cm, pi, pj, W)
    cp, cq, noise = cov_ref.blocks_two_ways(H, p.N, p.M_global)
    ps = np.nonzero(pr["pose_fixed"] == 0)[0]
    qs = np.nonzero(pr["pt_fixed"] == 0)[0]
    gp, gq, dropped = p.covariance(ps, qs, huber)
    err_p, err_q = cov_ref.rel_block_diff(gp, cp), cov_ref.rel_block_diff(gq, cq)
    print("reference noise %.3e  pose %.3e  point %.3e" % (noise, err_p, err_q))
    assert noise <= 1e-8 and dropped == 0
    tol = 10.0 * max(noise, 1e-12)   # the bound of test_gpu_covariance.test_blocks_match_the_host_inverse
    assert err_p <= tol and err_q <= tol, (err_p, err_q, tol)
