"""Host side of the "from the observation" form of the grouped pairs (include/ba_hip.h
ba_pair_G_from_obs, csrc/ba_device_fn.h pair_G_from_obs): {G, w} of one observation from
its camera, pose, point and uv.  No GPU: the entry point is plain host code of the library;
the bit-for-bit comparison with k_lin_grp's records is in test_gpu_pair_obs.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from bundle_adjustment_solver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc")


def rot(a):
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def helper(lib, cam, T, X, uv, huber):
    rec = (C.c_double * 8)()
    lib.ba_pair_G_from_obs((C.c_double * 16)(*cam), (C.c_double * 12)(*T), (C.c_double * 3)(*X),
                           (C.c_double * 2)(*uv), huber, rec)
    return np.array(rec[:])


def reference(cam, T, X, uv, huber):
    """Projection, Huber-like weight and G = dpi/dXc R_cj (reference :743-787) in longdouble."""
    ld = np.longdouble
    cam, T, X, uv = (np.array(v, ld) for v in (cam, T, X, uv))
    xij = T[:9].reshape(3, 3) @ X + T[9:]
    Rc = cam[4:13].reshape(3, 3)
    xc = Rc @ xij + cam[13:]
    iz = 1 / xc[2]
    r = np.array([cam[0] * xc[0] * iz + cam[2] - uv[0], cam[1] * xc[1] * iz + cam[3] - uv[1]])
    absr = np.abs(r).sum()
    w = ld(huber) / absr if absr > huber else ld(1)
    J = np.array([[cam[0] * iz, 0, -cam[0] * xc[0] * iz * iz], [0, cam[1] * iz, -cam[1] * xc[1] * iz * iz]], ld)
    return J @ Rc, w, r


def test_G_and_w_of_an_observation(built):
    lib = _lib.load()
    rng = np.random.default_rng(9)
    seen_w = set()
    for k in range(40):
        cam = [420.0 + k, 415.0, 320.0, 240.0] + list(rot(rng.normal(size=3) * 0.05).reshape(-1)) + list(rng.normal(size=3) * 0.1)
        T = list(rot(rng.normal(size=3) * 0.3).reshape(-1)) + list(rng.normal(size=3) * 0.5)
        X = list(rng.normal(size=3) * 0.8 + np.array([0.0, 0.0, 5.0]))
        Gr, _, r0 = reference(cam, T, X, [0.0, 0.0], 1.0)
        # the observation a pixel or so beside the projection: both branches of the weight
        uv = list(np.asarray(r0, np.float64) + rng.normal(size=2) * (0.2 if k % 2 else 2.0))
        huber = 0.7
        Gr, wr, r = reference(cam, T, X, uv, huber)
        rec = helper(lib, cam, T, X, uv, huber)
        assert rec[7] == 0.0
        # G: sums of two or three products of O(f / z) terms, a few roundings each; 64 ulp of
        # the row's largest entry is far above that.  w: the residual is a difference of
        # pixel coordinates of magnitude ~300, so its error is ~1e-13 / |r| relative.
        tol = 64 * np.finfo(np.float64).eps
        G = rec[:6].reshape(2, 3)
        assert np.abs(G - np.asarray(Gr, np.float64)).max() <= tol * np.abs(np.asarray(Gr, np.float64)).max()
        absr = float(np.abs(r).sum())
        assert abs(rec[6] - float(wr)) <= 1e-11 / absr
        seen_w.add(rec[6] == 1.0)
    assert seen_w == {True, False}


def test_obs_knob_follows_the_environment(tmp_path):
    """BA_PAIR_OBS is read by Knobs::from_env like every other knob (tests/cpp/
    pair_obs_knob_check.cpp): only "0" turns the form off, nothing is cached."""
    exe = str(tmp_path / "pair_obs_knob_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "pair_obs_knob_check.cpp"),
                    os.path.join(CSRC, "ba_dense_sched.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "PAIR OBS KNOB CHECK OK" in r.stdout, r.stdout[-2000:]
