"""Host side of the 64-byte pair record (include/ba_hip.h ba_expand_pair_slim): {G, w}
with the pose and the point gives the compact {K, X_ij} that ba_get_pairs expands for
every other pair.  No GPU: the entry point is plain host code of the library."""
import ctypes as C
import os
import subprocess

import numpy as np

from bundle_adjustment_solver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc")

# recorded inputs: G (2x3 row-major), w, pose {R_jw row-major, t_jw}, point
RECORDED = [
    # a camera looking down +z at a point two metres ahead, Huber weight active
    dict(G=[262.5, 0.0, -13.125, 0.0, 262.5, 9.84375], w=0.37,
         T=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.1, -0.075, 2.0], X=[0.0, 0.0, 0.0]),
    # rotated pose (30 degrees about y, 10 about x), full weight
    dict(G=[181.02, -3.7, 55.91, 12.25, 240.6, -31.08], w=1.0,
         T=[0.8660254037844387, 0.0, 0.5, 0.08682408883346517, 0.984807753012208, -0.1503837331804353,
            -0.492403876506104, 0.17364817766693033, 0.8528685319524433, -0.3, 0.25, 1.7],
         X=[0.42, -0.17, 3.1]),
    # the zero record of a masked pair without an observation
    dict(G=[0.0] * 6, w=0.0,
         T=[0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0, 5.0, 6.0], X=[1.0, 2.0, 3.0]),
]


def expand_slim(lib, G, w, T, X):
    rec = (C.c_double * 8)(*G, w, 0.0)
    k12 = (C.c_double * 12)()
    lib.ba_expand_pair_slim(rec, (C.c_double * 12)(*T), (C.c_double * 3)(*X), k12)
    return np.array(k12[:])


def block_from_compact(k12):
    """The 96-byte expansion of ba_get_pairs: rows 0..2 = K, row 3 + a = (X_ij x K[:, c])[a]."""
    K, x = k12[:9].reshape(3, 3), k12[9:]
    return np.vstack([K, np.cross(x[None, :], K.T).T])


def reference_block(G, w, T, X):
    """B_ji = w Q^T (G R_jw), Q = [G, G (-[X_ij]x)] (reference :797-826), in longdouble."""
    ld = np.longdouble
    G, T, X = np.array(G, ld).reshape(2, 3), np.array(T, ld), np.array(X, ld)
    R, t = T[:9].reshape(3, 3), T[9:]
    x = R @ X + t
    skew = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]], ld)
    Q = np.hstack([G, -G @ skew])
    return ld(w) * Q.T @ (G @ R), x


def test_expansion_of_the_slim_record_gives_the_block(built):
    lib = _lib.load()
    rng = np.random.default_rng(5)
    cases = list(RECORDED)
    for _ in range(20):   # poses near the identity, points a few metres away, pixel-scale G
        a = rng.normal(size=3) * 0.3
        th = np.linalg.norm(a)
        k = a / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        cases.append(dict(G=list(rng.normal(size=6) * 200.0), w=float(rng.uniform(0.05, 1.0)),
                          T=list(R.reshape(-1)) + list(rng.normal(size=3)), X=list(rng.normal(size=3) * 3.0)))
    for c in cases:
        k12 = expand_slim(lib, c["G"], c["w"], c["T"], c["X"])
        B = block_from_compact(k12)
        ref, x = reference_block(c["G"], c["w"], c["T"], c["X"])
        ref, x = np.asarray(ref, np.float64), np.asarray(x, np.float64)
        if c["w"] == 0.0:
            assert not k12[:9].any() and not B.any()
            continue
        # K is a sum of 2 x 3 products of O(1) factors, X_ij a sum of four terms: a few
        # roundings each; rows 3..5 add one product and one difference.  64 ulp of the
        # block's largest entry is far above that and far below the 1e-10 of the GPU tests.
        tol = 64 * np.finfo(np.float64).eps
        assert np.abs(k12[9:] - x).max() <= tol * np.abs(x).max()
        assert np.abs(B - ref).max() <= tol * np.abs(ref).max()


def test_slim_and_compact_records_of_one_pair_expand_alike(built):
    """The 96-byte record of a pair is {K, X_ij} of the same G, w, pose and point: what the
    getter returns for a slim pair is what it returns for that compact record."""
    lib = _lib.load()
    for c in RECORDED[:2]:
        k12 = expand_slim(lib, c["G"], c["w"], c["T"], c["X"])
        G, T, X = np.array(c["G"]).reshape(2, 3), np.array(c["T"]), np.array(c["X"])
        R, t = T[:9].reshape(3, 3), T[9:]
        K = G.T @ (c["w"] * (G @ R))
        compact = np.concatenate([K.reshape(-1), R @ X + t])
        a, b = block_from_compact(k12), block_from_compact(compact)
        assert np.abs(a - b).max() <= 64 * np.finfo(np.float64).eps * np.abs(b).max()


def test_layout_knob_follows_the_environment(tmp_path):
    """BA_PAIR_SLIM is read by Knobs::from_env like every other knob (tests/cpp/
    pair_knob_check.cpp): only "0" turns the slim record off, nothing is cached."""
    exe = str(tmp_path / "pair_knob_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "pair_knob_check.cpp"),
                    os.path.join(CSRC, "ba_dense_sched.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "PAIR KNOB CHECK OK" in r.stdout, r.stdout[-2000:]
