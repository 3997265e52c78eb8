"""ba_covariance: the parts that need no GPU — exports and bindings, the argument
checks (they run before anything touches a device; ba_covariance_check is the same code
on plain values, since no handle exists without a GPU) and the unit conversion
covariance_to_user_units, checked against finite differences in real units."""
import ctypes as C
import os
import re

import numpy as np

from bundle_adjustment_solver_amd import _lib, scene_io, scenes
from bundle_adjustment_solver_amd.solver import covariance_to_user_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ba_covariance", "ba_covariance_info", "ba_covariance_check"]


def test_symbols_declared_exported_bound(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
        assert m, name
        assert hasattr(lib, name), "missing export: " + name
        n_decl = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_decl == len(_lib.SIGNATURES[name][1]), name


def _check(lib, finalized=1, sharded=0, streamed=0, pose_fixed=(1, 0, 0), pt_fixed=(0, 0, 1, 0),
           pose_sel=(1, 2), cov_pose=True, pt_sel=(0, 1, 3), cov_pt=True):
    pf, qf = np.asarray(pose_fixed, np.uint8), np.asarray(pt_fixed, np.uint8)
    ps, qs = np.asarray(pose_sel, np.int32), np.asarray(pt_sel, np.int32)
    cp, cq = np.zeros((max(ps.size, 1), 36)), np.zeros((max(qs.size, 1), 9))
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    i = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.ba_covariance_check(finalized, sharded, streamed, pf.size, u(pf), qf.size, u(qf),
                                 ps.size, i(ps) if ps.size else None, d(cp) if cov_pose else None,
                                 qs.size, i(qs) if qs.size else None, d(cq) if cov_pt else None)
    return rc, lib.ba_last_error().decode()


def test_host_validation_rejects_without_a_gpu(built):
    lib = _lib.load()
    assert _check(lib)[0] == 0
    # either selection may be empty, and its output pointer then NULL; repeats, any order
    assert _check(lib, pose_sel=(), cov_pose=False)[0] == 0
    assert _check(lib, pt_sel=(), cov_pt=False)[0] == 0
    assert _check(lib, pose_sel=(2, 1, 2), pt_sel=(3, 3, 0))[0] == 0
    for kw, word in ((dict(finalized=0), "not finalized"),
                     (dict(sharded=1), "sharded"),
                     (dict(streamed=1), "streamed"),
                     (dict(pose_sel=(1, 3)), "pose_sel[1] = 3 is out of range"),
                     (dict(pose_sel=(-1,)), "pose_sel[0] = -1 is out of range"),
                     (dict(pose_sel=(2, 0)), "pose_sel[1] = 0 is a fixed pose"),
                     (dict(pt_sel=(0, 4)), "pt_sel[1] = 4 is out of range"),
                     (dict(pt_sel=(-2,)), "pt_sel[0] = -2 is out of range"),
                     (dict(pt_sel=(2,)), "pt_sel[0] = 2 is a fixed point"),
                     (dict(cov_pose=False), "cov_pose36 is NULL"),
                     (dict(cov_pt=False), "cov_pt9 is NULL")):
        rc, msg = _check(lib, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    # the entry points themselves refuse a NULL handle before anything else
    assert lib.ba_covariance(None, 1.0, 0, None, None, 0, None, None, None) == -1
    assert "null handle" in lib.ba_last_error().decode()
    assert lib.ba_covariance_info(None, None) == -1


# ---- unit conversion -----------------------------------------------------------------
def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def _exp_se3(xi):
    """exp of xi = [v; omega] as a 4x4 matrix (closed form)."""
    v, w = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    K = _hat(w)
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + 0.5 * K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


def _jacobian(sc, h_len, h_rot):
    """d residuals / d [xi of the free poses; delta of the free points] by central
    differences, T_jw <- exp(xi) T_jw (T_jw = inverse of the scene's pose) and X += delta."""
    free_p = np.nonzero(~sc["pose_fixed"])[0]
    free_q = np.nonzero(~sc["pt_fixed"])[0]
    cols = []

    def res(T_wc, X):
        return scene_io.reprojection_residuals(dict(sc, T_wc_init=T_wc, X_init=X)).ravel()
    for j in free_p:
        for k in range(6):
            h = h_len if k < 3 else h_rot
            r = []
            for sgn in (1.0, -1.0):
                xi = np.zeros(6)
                xi[k] = sgn * h
                T = sc["T_wc_init"].copy()
                T[j] = np.linalg.inv(_exp_se3(xi) @ np.linalg.inv(T[j]))
                r.append(res(T, sc["X_init"]))
            cols.append((r[0] - r[1]) / (2 * h))
    for i in free_q:
        for k in range(3):
            r = []
            for sgn in (1.0, -1.0):
                X = sc["X_init"].copy()
                X[i, k] += sgn * h_len
                r.append(res(sc["T_wc_init"], X))
            cols.append((r[0] - r[1]) / (2 * h_len))
    return np.stack(cols, axis=1), free_p.size, free_q.size


def _blocks(Hi, N, M):
    cp = np.stack([Hi[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(N)])
    cq = np.stack([Hi[6 * N + 3 * i:6 * N + 3 * i + 3, 6 * N + 3 * i:6 * N + 3 * i + 3] for i in range(M)])
    return cp, cq


def test_unit_conversion_against_real_unit_finite_differences():
    """Tiny mono scene: 3 poses (1 fixed), 12 free landmarks — plus 2 fixed landmarks,
    without which a monocular problem with one fixed pose keeps its scale gauge and
    J^T J has no inverse.

    Real side: J in pixels per metre / radian by central differences of
    scene_io.reprojection_residuals, Cov = sigma^2 (J^T J)^-1.  Scaled side: the same
    differences on scaled_problem(scene) (lengths and pixels x 0.01), Sigma_s =
    (J_s^T J_s)^-1, then covariance_to_user_units(Sigma_s, sigma).

    Step and tolerance.  A central difference is off by h^2 |f'''| / 6 (truncation) plus
    about 4 eps |u| / h (rounding of a pixel coordinate |u| <= 640 computed in a few
    operations).  With |f'| ~ f / z ~ 100 px/m and |f'''| ~ 6 f / z^3 ~ 25 px/m^3 (f = 500
    px, depth z >= 4 m) the two meet near h = (12 eps |u| / |f'''|)^(1/3) ~ 1e-5: h = 1e-5
    m and rad on the real side, 1e-7 scaled length (the same point, so the truncation
    terms of the two sides are the same numbers scaled) and 1e-5 rad on the scaled side.
    Per entry of J that leaves a relative error of delta <= 4 eps 640 / (1e-5 * 100) +
    1e-10 * 25 / (6 * 100) ~ 3e-10.  (J + dJ)^T (J + dJ) is off by 2 delta relative,
    and a block of the inverse by at most kappa times that, kappa the condition number of
    the diagonally equilibrated J^T J (the equilibration takes the units out, so kappa is
    the same on both sides).  Both sides carry the error: tol = 2 * 2 * delta * kappa."""
    sc = scenes.synthetic_ba_scene(n_pose=3, n_pt=14, window=3, stereo=False, seed=7, n_fixed=1)
    sc["pt_fixed"] = np.arange(14) >= 12
    sc["X_init"][12:] = sc["X_true"][12:]
    sigma = 0.7
    J, N, M = _jacobian(sc, 1e-5, 1e-5)
    H = J.T @ J
    cov_p, cov_q = _blocks(sigma ** 2 * np.linalg.inv(H), N, M)
    # the scaled problem as a scene of its own
    pr = scenes.scaled_problem(sc)
    to44 = lambda T12: np.concatenate(
        [np.concatenate([T12[:, :9].reshape(-1, 3, 3), T12[:, 9:, None]], axis=2),
         np.tile([[[0, 0, 0, 1.0]]], (T12.shape[0], 1, 1))], axis=1)
    ss = dict(intr=pr["cam_intr"], T_cj=to44(pr["cam_T"]), T_wc_init=np.linalg.inv(to44(pr["pose_T"])),
              X_init=pr["pt_X"], obs_uv=pr["obs_uv"], obs_pose=sc["obs_pose"], obs_cam=sc["obs_cam"],
              obs_pt=sc["obs_pt"], pose_fixed=sc["pose_fixed"], pt_fixed=sc["pt_fixed"])
    Js, _, _ = _jacobian(ss, 1e-7, 1e-5)
    sp, sq = _blocks(np.linalg.inv(Js.T @ Js), N, M)
    got_p, got_q = covariance_to_user_units(sp, sq, sigma)
    dg = 1.0 / np.sqrt(np.diag(H))
    kappa = np.linalg.cond(H * dg[:, None] * dg[None, :])
    tol = 2 * 2 * 3e-10 * kappa
    rel = lambda a, b: max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a, b))
    print("kappa %.3e tol %.3e  pose %.3e point %.3e" % (kappa, tol, rel(got_p, cov_p), rel(got_q, cov_q)))
    assert kappa < 1e8
    assert rel(got_p, cov_p) <= tol and rel(got_q, cov_q) <= tol
    # the conversion is not a no-op: the raw blocks are off by the unit factors
    assert rel(sp, cov_p) > 1.0 and abs(rel(sq, cov_q) - abs(1 - 1 / sigma ** 2)) < 1e-3
