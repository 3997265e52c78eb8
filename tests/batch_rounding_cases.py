"""The windows of test_batch_rounding_ref.py (CPU oracle) and test_gpu_batch_rounding.py (device):
tiny problems of scenes.ba_batch_scene, each named for the edge of the batched kernels
(ba_batch_kernels.h) it is there for.

  N1 N4 N5 N6 N10 N11 N15 N16   optimisable poses: the pose pass runs one wave per pose on a 4-wave
                                workgroup (4 fills it, 5 wraps round); 5 / 10 / 16 are the last
                                counts of the 32- / 64- / 96-column image, 6 / 11 the first of the
                                next; the Schur pass has 240 half blocks at 15 (fits 256 threads) and
                                272 at 16 (the thread loop wraps)
  M255 M256 M257                optimisable landmarks at N = 5: one thread per landmark, 256 threads
  obs63 obs64 obs65             observations per optimisable pose: the pose pass strides over 64 lanes
  mono stereo                   one window of each kind
  last writer                   both cameras see every pair, observation order shuffled
  huber                         pixel noise 0.5 px, threshold 0.005: the robust branch
  fixed only                    landmarks seen by fixed poses only, three fixed points
  unobserved                    an optimisable landmark nobody observes (C_i = 0)
  small                         points displaced by 1e-9, poses exact: se3_exp's small-angle branch
  rejected                      first step SKIPPED, second accepted (REJECTED_LAMBDA)

Every observed optimisable landmark of every window is seen by the fixed pose 0, so that a
marginalisation that marks pose 0 alone selects all of them.
"""
import numpy as np

import xp_ref as X
from bundle_adjustment_solver_amd import scenes

OBS_KEYS = ("obs_cam", "obs_pose", "obs_pt", "obs_uv")
LAMBDA_MAX = 100.0
LAMBDAS = (LAMBDA_MAX, X.LAMBDA, X.LAMBDA_FLOOR)
MORE_LAMBDAS = ("N1", "N5", "N16", "M257")      # also at 1e-3 and 1e-10
HUBER = {"huber": 0.005}
REJECTED = "rejected"
REJECTED_LAMBDA = 0.1
UPDATE, UPDATE_TRUST_MORE, SKIPPED = 0, 1, 2
WIDTH_OF = lambda n: 32 if n <= 5 else 64 if n <= 10 else 96


def window(n_pose, n_pt, stereo, seed, n_fixed=2, **kw):
    """window of test_gpu_full_batch.py"""
    return scenes.ba_batch_scene(1, n_pose=n_pose, n_pt=n_pt, stereo=stereo, seed=seed, n_fixed=n_fixed, **kw)[0]


def _without(sc, drop):
    for k in OBS_KEYS:
        sc[k] = sc[k][~drop]
    return sc


def _trimmed(n_obs):
    """mono, 3 optimisable poses of 65 landmarks: every optimisable pose keeps n_obs observations
    (each loses other landmarks), the fixed poses keep all"""
    sc = window(5, 65, False, 170)
    drop = np.zeros(sc["obs_pt"].size, bool)
    for j in (2, 3, 4):
        gone = (np.arange(65 - n_obs) * 23 + 7 * j) % 65
        drop |= (sc["obs_pose"] == j) & np.isin(sc["obs_pt"], gone)
    return _without(sc, drop)


def _unobserved():
    sc = window(6, 23, True, 180)
    return _without(sc, sc["obs_pt"] == 9)


def _build():
    import test_gpu_full_batch as F
    sp = scenes.scaled_problem
    out = {}
    for n, n_pt, stereo in ((1, 14, False), (4, 13, True), (5, 15, False), (6, 13, True), (10, 11, False),
                            (11, 11, True), (15, 9, False), (16, 10, True)):
        out["N%d" % n] = sp(window(n + 2, n_pt, stereo, 100 + n))
    for m in (255, 256, 257):
        out["M%d" % m] = sp(window(7, m, False, 140 + m))
    for n_obs in (63, 64, 65):
        out["obs%d" % n_obs] = sp(_trimmed(n_obs))
    out["mono"] = sp(window(5, 37, False, 11))
    out["stereo"] = sp(window(6, 21, True, 61))
    out["last writer"] = F.quirk_problems()[0]
    out["huber"] = sp(window(6, 33, True, 22, pixel_sigma=0.5))
    out["fixed only"] = F.five_problems()[4]
    out["unobserved"] = sp(_unobserved())
    out["small"] = sp(window(6, 25, True, 190, pose_noise=0.0, point_noise=1e-9))
    out[REJECTED] = sp(window(*REJECTED_SCENE[0], **REJECTED_SCENE[1]))
    for pr in out.values():
        for v in pr.values():
            v.setflags(write=False)
    return out


# Found by a search with the CPU oracle over seeds 1..8, pose / point noise (0.05, 0.2), (0.3, 1), (1, 2) m,
# pixel noise 5 / 20 / 50 px, mono and stereo, initial lambda 0.1 .. 30: the one window of 864 whose first
# step is SKIPPED and whose second is accepted.  The cost is the sum of the UNSQUARED residual norms, the
# step minimises the squared ones: with 50 px of pixel noise the step at lambda 0.1 raises the cost
# (rho = -91), the step at lambda 0.3 lowers it (rho = 160): neither decision is near its threshold 0.25.
REJECTED_SCENE = ((6, 25, False, 7), dict(pose_noise=0.05, point_noise=0.2, pixel_sigma=50.0))

_cases, _oracle = {}, {}


def cases():
    """name -> problem (scaled units), built once, read-only"""
    if not _cases:
        _cases.update(_build())
    return _cases


def huber_of(name):
    """the threshold the solvers really use: their options hold a float (0.005 is none)"""
    return float(np.float32(HUBER.get(name, 1.0)))


def free_poses(pr):
    return int((pr["pose_fixed"] == 0).sum())


def passes():
    """every (case, lambda0) of the one-step tests"""
    names = [n for n in CASE_NAMES if n != REJECTED]
    return [(n, LAMBDA_MAX) for n in names] + [(n, lam) for lam in LAMBDAS[1:] for n in MORE_LAMBDAS]


CASE_NAMES = (["N%d" % n for n in (1, 4, 5, 6, 10, 11, 15, 16)] + ["M255", "M256", "M257", "obs63", "obs64", "obs65",
              "mono", "stereo", "last writer", "huber", "fixed only", "unobserved", "small", REJECTED])


def lambda_of(lam):
    """the damping the solvers really start from: their options hold a float"""
    return float(np.float32(lam))


def observed_landmarks(pr):
    """one flag per point: optimisable and observed"""
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_fixed"])) > 0
    return seen & (pr["pt_fixed"] == 0)


def oracle_solve(name, lam, max_iter=1):
    """(rows, poses, points) of the CPU oracle on a case, thresholds 0 (computed once)"""
    key = (name, lam, max_iter)
    if key not in _oracle:
        from oracle import oracle_py as O
        o = O.Oracle(cases()[name])
        rows, _ = o.solve(O.make_options(max_iter=max_iter, thr_step=0.0, thr_cost=0.0, lambda0=lam,
                                         huber=huber_of(name)))
        _oracle[key] = (rows, o.get_poses(), o.get_points())
        o.close()
    return _oracle[key]


_refs = {}


def reference(name, lam):
    """what both test files need of a (case, damping): the structure, the long-double linearisation
    and e64 = full_system_units of xp_ref's own float64 step (computed once)"""
    key = (name, lam)
    if key not in _refs:
        pr, hub = cases()[name], huber_of(name)
        st = X.Structure(pr)
        lin = X.linearize(pr, st, hub, lam, X.LD)
        e64 = X.full_system_units(pr, st, lam, hub, *X.yardstick_step(pr, st, lam, hub), lin=lin)
        _refs[key] = (st, lin, e64)
    return _refs[key]


def step_figures(name, lam, poses, points):
    """((pose rows, landmark rows), e64 of the same) of a one-step result"""
    st, lin, e64 = reference(name, lam)
    return X.full_system_units(cases()[name], st, lam, huber_of(name), poses, points, lin=lin), e64


def cost_figures(name, value, poses, points):
    """(e, e64) of a cost value against xp_ref.cost in long double at the given parameters"""
    pr = cases()[name]
    r = X.cost(pr, poses, points, X.LD)
    return X.rounding_units(value, r), X.rounding_units(X.cost(pr, poses, points, np.float64).v, r)


def cost_change_figures(name, value, poses, points):
    """(e, e64) of a row's cost_change |trial cost - cost at the inputs| at the given trial parameters"""
    pr = cases()[name]
    ch = lambda dt: X.cost(pr, poses, points, dt) - X.cost(pr, pr["pose_T"], pr["pt_X"], dt)
    r, y = ch(X.LD), ch(np.float64)
    r, y = X.VS(np.abs(r.v), r.s), X.VS(np.abs(y.v), y.s)
    return X.rounding_units(value, r), X.rounding_units(y.v, r)


_reduced = {}


def reduced_reference(name):
    """xp_ref.reduced_reference of a case over its observed landmarks (computed once)"""
    if name not in _reduced:
        pr = cases()[name]
        _reduced[name] = X.reduced_reference(pr, X.Structure(pr), huber_of(name), observed_landmarks(pr))
    return _reduced[name]
