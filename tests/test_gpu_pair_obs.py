"""The "from the observation" form of the grouped pairs (ba_device.h PairObs): a slim handle
whose covisibility groups are all 32 wide and unmasked keeps no pair record in the iteration
— k_lin_grp writes none, k_schur_grp<2> and the group role of k_backsub_update rebuild {G, w}
from the uv of the pair's last writer (pair_G_from_obs), k_pair_records fills the slim records
for ba_get_pairs and ba_covariance on demand.  On the smallest shapes that take each code
form: the handle reports the form, blocks and reduced system against the CPU oracle at the
tolerances of test_gpu_pair_slim.py, and EQUAL BITS against the slim form (BA_PAIR_OBS=0) for
the reduced system, LM trajectories (a run-away one included), the pair getter and the
covariance.  Shapes outside the form keep the slim one."""
import numpy as np
import pytest

import test_gpu_pair_slim as S
from bundle_adjustment_solver_amd import _lib, scenes
from bundle_adjustment_solver_amd._lib import make_options
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

# name: (scene or the name of a shape of test_gpu_pair_slim, knobs, huber of the staged linearisation)
SHAPES = {
    "stereo5": ("stereo5", {}, 0.7),                  # stereo windows of 5: d = 5, 10 slots
    "stereo5_steps2": ("stereo5_steps2", {"BA_LIN_STEPS": "2"}, 0.7),  # pieces cut a group, partial last steps and chunks
    "slots6": (lambda: scenes.synthetic_ba_scene(30, 2500, 3, True, seed=23, pixel_sigma=1.0), {}, 0.7),   # 6 slots
    "mono2": (lambda: scenes.synthetic_ba_scene(30, 2500, 2, False, seed=24, pixel_sigma=1.0), {}, 0.7),   # the only slot is the last
    "hover": ("hover", {}, 0.7),                      # fixed poses inside the pattern, d = 4
    "hover9": (lambda: scenes.hover_scene(3, 500, 9, seed=32), {}, 0.7),   # nine cameras: the global camera path, last writer = ninth slot
    "huber05": (lambda: scenes.synthetic_ba_scene(40, 3000, 5, True, seed=25, pixel_sigma=1.5), {}, 0.5),  # w < 1 on a good share
}
OUTSIDE = ["mono10", "stereo16", "dropout"]   # 64-wide, wide, masked: the slim form stays
_problems = {}


def problem(name):
    """The scaled problem of a shape and the oracle's blocks at (lambda, huber): computed once
    (shared with test_gpu_pair_slim.py where the shape is one of its)."""
    src, _, hub = SHAPES[name]
    if isinstance(src, str):
        return S.problem(src)
    if name not in _problems:
        pr = scenes.scaled_problem(src())
        lam = 1.3
        o = O.Oracle(pr)
        o.linearize(hub)
        o.damp_invert(lam)
        o.schur()
        _problems[name] = (pr, dict(lam=lam, hub=hub, cost=o.cost(), A=o.get_A(), C=o.get_C(), pairs=o.get_pairs(),
                                    S=o.get_S()))
    return _problems[name]


def rows_array(rows):
    return np.array([[r.iteration_status, r.cost, r.trial_cost, r.damping_term, r.abs_step, r.abs_gradient,
                      r.rho, r.model_change] for r in rows])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_both_forms(name, monkeypatch, check_oracle):
    """Everything one handle of each form gives, in the order of a real session: staged
    linearisation and Schur complement, the pair getter, 8 LM iterations, the pair getter and the
    covariance after them (the records of the new form are rebuilt for the moved buffers)."""
    pr, ref = problem(name)
    hub = SHAPES[name][2]
    ps = np.nonzero(pr["pose_fixed"] == 0)[0][:3]
    qs = np.nonzero(pr["pt_fixed"] == 0)[0][:6]
    out = []
    for extra in ({}, {"BA_PAIR_OBS": "0"}):
        g = S.make_gpu(pr, dict(SHAPES[name][1], **extra), monkeypatch)
        form, rec = g.get_pair_form(), g.get_pair_record_info()
        g.stage_linearize(ref["lam"], hub)
        g.stage_schur()
        if check_oracle:
            assert S.relerr(g.stage_cost(), ref["cost"]) < 1e-12
            S.check_blocks(g, ref)
        r = dict(form=form, rec=rec, S=g.get_S(), W0=g.get_pairs()[2], slim0=g.get_slim_records()["rec"])
        rows, _ = g.solve(make_options(max_iter=8, thr_step=0, thr_cost=0, huber=hub))
        r.update(rows=rows_array(rows), P=g.get_poses(), X=g.get_points()[0], W1=g.get_pairs()[2])
        r["cov"] = g.covariance(ps, qs, hub)
        r["W2"] = g.get_pairs()[2]   # once more: the covariance call linearised into the same buffer
        out.append(r)
    return out


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_form_is_taken_matches_oracle_and_equals_the_slim_form_bit_for_bit(name, built, monkeypatch):
    new, slim = run_both_forms(name, monkeypatch, check_oracle=True)
    print(name, new["form"], slim["form"], new["rec"])
    # (a) the form under test really is the one taken; BA_PAIR_OBS=0 is today's slim form
    assert new["form"] == 2 and slim["form"] == 1
    assert new["rec"] == slim["rec"] and new["rec"]["slim_pairs"] > 0.7 * new["rec"]["pairs"]
    if name == "huber05":
        share = (slim["slim0"][:, 6] < 1.0).mean()
        print("share of pairs with w < 1: %.2f" % share)
        assert share > 0.2
    # (c) reduced system and trajectory
    assert same_bits(new["S"][0], slim["S"][0]) and same_bits(new["S"][1], slim["S"][1])
    assert len(new["rows"]) == 8 and same_bits(new["rows"], slim["rows"])
    assert same_bits(new["P"], slim["P"]) and same_bits(new["X"], slim["X"])
    # (d) the readers off the hot path: k_pair_records gives the records k_lin_grp's slim form
    # holds, before and after further iterations
    assert same_bits(new["slim0"], slim["slim0"])
    for k in ("W0", "W1", "W2"):
        assert same_bits(new[k], slim[k]), k
    assert not same_bits(new["W0"], new["W1"])   # (the iterations did move the linearisation point)
    assert same_bits(new["cov"][0], slim["cov"][0]) and same_bits(new["cov"][1], slim["cov"][1])
    assert new["cov"][2] == slim["cov"][2]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_runaway_trajectory_has_equal_bits(name, built, monkeypatch):
    """(e) thresholds off, 25 iterations (the regime bench.py times): rows, poses and points
    of the two forms are the same bits, NaN rows included."""
    pr, _ = problem(name)
    res = []
    for extra in ({}, {"BA_PAIR_OBS": "0"}):
        g = S.make_gpu(pr, dict(SHAPES[name][1], **extra), monkeypatch)
        rows, _ = g.solve(make_options(max_iter=25, thr_step=-1.0, thr_cost=-1.0, huber=SHAPES[name][2]))
        res.append((g.get_pair_form(), rows_array(rows), g.get_poses(), g.get_points()[0]))
    (fa, ra, Pa, Xa), (fb, rb, Pb, Xb) = res
    assert fa == 2 and fb == 1 and len(ra) == 25
    print(name, "non-finite rows:", int((~np.isfinite(ra).all(axis=1)).sum()))
    assert same_bits(ra, rb) and same_bits(Pa, Pb) and same_bits(Xa, Xb)


@pytest.mark.parametrize("name", OUTSIDE)
def test_shapes_outside_the_form_keep_the_slim_record(name, built, monkeypatch):
    pr, ref = S.problem(name)
    g = S.make_gpu(pr, S.SHAPES[name][1], monkeypatch)
    assert g.get_pair_form() == 1 and g.get_pair_record_info()["slim_pairs"] > 0
    g.stage_linearize(ref["lam"], ref["hub"])
    g.stage_schur()
    S.check_blocks(g, ref)


def test_host_helper_reproduces_every_slim_record(built, monkeypatch):
    """pair_G_from_obs compiled for the host (ba_pair_G_from_obs) against the records k_lin_grp
    wrote in a slim-form run of the stereo-5 scene: every pair, bit for bit."""
    import ctypes as C
    pr, ref = problem("stereo5")
    g = S.make_gpu(pr, {"BA_PAIR_OBS": "0"}, monkeypatch)
    assert g.get_pair_form() == 1
    g.stage_linearize(ref["lam"], ref["hub"])
    r = g.get_slim_records()
    n = r["rec"].shape[0]
    assert n > 10000
    lib = _lib.load()
    # the records were made from the parameters the handle was loaded with
    T = np.ascontiguousarray(pr["pose_T"][r["pose"]], np.float64)
    X = np.ascontiguousarray(pr["pt_X"][r["lm"]], np.float64)
    cams = np.ascontiguousarray(np.concatenate([pr["cam_intr"], pr["cam_T"]], axis=1), np.float64)
    assert cams.shape[1] == 16
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros((n, 8))
    uv = np.ascontiguousarray(r["uv"])
    for p in range(n):
        lib.ba_pair_G_from_obs(dp(cams[r["cam"][p]]), dp(T[p]), dp(X[p]), dp(uv[p]), ref["hub"], dp(out[p]))
    bad = np.nonzero((out.view(np.uint64) != r["rec"].view(np.uint64)).any(axis=1))[0]
    print("pairs %d, differing %d" % (n, bad.size))
    assert bad.size == 0, (bad[:5], out[bad[:2]], r["rec"][bad[:2]])
