"""Scenes, cases, references and tolerances of the pose-only one-step tests
(test_pose_only_onestep_ref.py on the CPU, test_gpu_pose_only_onestep.py on the
GPU).  Test infrastructure only.

Scene.  The residuals of the first iteration are evaluated at the initial pose,
so the pixels are built as the float64 projection at that pose (from the
float32 inputs the kernel gets) minus a designed offset: every edge's residual
is its offset to ~1e-4 px and every point's class is known by construction.
Inliers get offsets uniform in +-0.4 px (L1 <= 0.8).  The PROBE indices, every
index next to a structural edge of the kernel's work split, carry the other
classes, alternating along the sorted probe list:

  option set A (huber 1.0, outlier 2.5): "outlier" |du|, |dv| in [2.5, 20],
      "Huber" |du|, |dv| in [0.65, 1.1] (L1 in [1.3, 2.2]);
  option set B (both thresholds 1e9, the pure quadratic branch): every probe
      |du|, |dv| in [100, 200], so every probe dominates the cost.

Stereo: half of the probes, always n - 1 and 1024, have no right match (one
negative right coordinate, u and v in turn); the others carry their class in
the right image through offsets of their own.  One inlier is placed so that its
right u is exactly 0.0 (a match).

Tolerances.  Nothing here is tuned on the GPU.  MEASURED holds, per size class
and quantity, the largest deviation of the project's fp32 CPU restatements
(oracle.oracle_py.pose_only_{mono,stereo}6, planar_pose_ref at float32) from
the float64 references over all cases of the class; the CPU test asserts that
it is not exceeded.  TOL = K * MEASURED with K = 4: the GPU adds the same fp32
terms in another order (DPP rows, 16 waves, workgroups), which at large n is
more accurate than the sequential restatement, and uses another sinf / cosf."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script: print the MEASURED table)
    sys.path.insert(0, ROOT)

import planar_pose_ref as R3
import pose_only6_ref as R6
from bundle_adjustment_solver_amd import scenes

D = np.float64
VARIANTS = ("mono6", "stereo6", "mono3", "stereo3")
OPTS = {"A": dict(huber=1.0, outlier=2.5), "B": dict(huber=1e9, outlier=1e9)}
MARGIN_PX = 0.05

# n -> the edge of the work split it exists for ("pose-only one-step tests")
SIZES = (3, 6,                  # tiny systems, partial first wave
         63, 64, 65,            # wave edges
         1023, 1024, 1025,      # workgroup edge, first use of unroll slot 1
         2048, 2049,            # one workgroup -> two: grid barrier and `partial`
         4097,                  # three workgroups
         131072, 131073,        # 64-workgroup cap, unroll slots 2, 3, 2nd trip of stereo3
         262145)                # second trip of the kU = 4 variants
SIZES_3ITER = (1025, 2049, 4097, 131073)
BATCH_SIZES = (3, 65, 1025, 2049, 0, 3073, 4096, 4097, 8193)   # 0: the empty problem
LARGE_N = 131072


def sizes(variant):
    return ((2,) if variant.endswith("3") else ()) + SIZES


def size_class(n):
    """The classes of the tolerance table.  The fp32 yardsticks lose accuracy
    with n (the C++ oracle adds sequentially), and a system of 2 to 6 points
    takes a step of order 1 under set B (pose error 1e-4 in fp32), so one class
    would hold every size to the worst one's figure."""
    return "tiny" if n <= 6 else "small" if n <= 1025 else "mid" if n <= 8193 else "large"


K = 4.0
# MEASURED[class][quantity]: largest |fp32 restatement - float64 reference| over
# the cases of the class (both restatements, every variant), as deviations()
# defines the quantities.  Asserted by the CPU test; `python
# tests/onestep_cases.py` prints the table again when a scene or a case changes.
MEASURED = {
    "tiny": dict(cost=4.5e-06, change=5.2e-08, step=2.0e-05, T12=1.4e-04),
    "small": dict(cost=5.0e-06, change=2.5e-06, step=3.8e-04, T12=3.2e-06),
    "mid": dict(cost=4.9e-05, change=5.2e-06, step=2.4e-03, T12=1.7e-06),
    "large": dict(cost=None, change=3.8e-05, step=6.5e-03, T12=2.2e-06),
}
# The cost of the large class.  The C++ oracle adds its 131 072+ terms one after
# the other in fp32 and is itself off by up to 1.7e-3 there, so K times that
# (6.5e-3) is more than a probe's whole share of the cost (~1e-2) / 8 and could
# not see a dropped point.  The constant is instead the a-priori bound of the
# kernel's OWN sum, for the non-negative terms of set B: at most
# 4 + 6 + 16 + 64 additions on the way of a term through a thread, the DPP
# rows, the 16 waves and the 64 workgroups, 3 roundings of the normalisation
# (93 x 2^-24 = 5.6e-6), and 2e-6 for the terms that carry the cost (|rv| >=
# 100 px known to 1e-4 px in fp32).  Not multiplied by K.  The CPU test holds
# the pairwise-summing planar restatement to it.
COST_LARGE = 1e-5
TOL = {c: {q: (COST_LARGE if v is None else K * v) for q, v in m.items()}
       for c, m in MEASURED.items()}


def tol(sc):
    return TOL[size_class(sc["n"])]


def sequential_yardstick(sc):
    """The 6-DoF restatement is the C++ oracle's sequential fp32 loop."""
    return "T12" in sc


def cost_compared(opt, n):
    """Where every probe's share of the cost is at least 8x the cost tolerance
    (the CPU test asserts it).  Set A: up to 1025 points; beyond, a Huber
    probe's ~0.3 drowns among the inliers, set A checks masks, step and pose
    only and set B carries the cost check."""
    return opt == "B" or n <= 1025


# ---- probes -------------------------------------------------------------------
_EDGES = (0, 1, 62, 63, 64, 65, 1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049, 3071, 3072,
          4095, 4096, 65535, 65536, 65537, 131071, 131072)


def probe_indices(n):
    idx = set(i for i in _EDGES if i < n)
    idx.update(i for i in (n - 2, n - 1) if i >= 0)
    if n > 131072:   # each unroll slot's first and last thread of workgroup 0
        idx.update(i for u in range(1, 5) for i in (u * 65536, u * 65536 + 1023) if i < n)
    return np.array(sorted(idx))


def _offsets(rng, n, probes, opt):
    """(n, 2) designed residuals: inliers, and the probes' classes."""
    d = rng.uniform(-0.4, 0.4, (n, 2))
    for k, p in enumerate(probes):
        if opt == "B":
            mag = rng.uniform(100.0, 200.0, 2)
        elif k % 2 == 0:
            mag = rng.uniform(2.5, 20.0, 2)      # outlier
        else:
            mag = rng.uniform(0.65, 1.1, 2)      # Huber
        d[p] = mag * rng.choice([-1.0, 1.0], 2)
    return d


def _pixels(proj, d):
    """pixel = projection - residual, the residual's sign turned where the
    pixel would go negative (a negative right pixel means no match)."""
    d = np.where(proj - d < 0, -d, d)
    return (proj - d).astype(np.float32)


def _no_right(n, probes):
    sel = np.array([(k // 2) % 2 == 1 for k in range(len(probes))])
    sel |= np.isin(probes, [n - 1, 1024])
    return probes[sel]


def _camera_points(rng, n):
    return np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n),
                     rng.uniform(4.0, 10.0, n)], 1)


def _zero_u_point(probes, n, Kr, baseline):
    """(index, left-camera point) of the inlier whose right pixel u is 0.0: its
    right projection lies at u = 0.2.  None where every index is a probe."""
    free = np.setdiff1d(np.arange(min(n, 8)), probes)
    if free.size == 0:
        return None, None
    z = 6.0
    return int(free[0]), np.array([(0.2 - Kr[2]) / Kr[0] * z + baseline, 0.3, z])


def _stereo_pixels(rng, sc, proj_r, n, probes, opt, zero_idx):
    d = _offsets(rng, n, probes, opt)
    if zero_idx is not None:
        d[zero_idx, 0] = proj_r[zero_idx, 0]          # pixel u = 0.0, residual ~0.2
    uvr = _pixels(proj_r, d)
    if zero_idx is not None:
        uvr[zero_idx, 0] = 0.0
    miss = _no_right(n, probes)
    for k, p in enumerate(miss):
        uvr[p, k % 2] = -1.0
    sc.update(uv_right=uvr, no_right=miss, zero_idx=zero_idx)


def t12(T):
    T = np.asarray(T)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float32)


def scene6(n, seed, stereo, opt, intr=None, baseline=scenes.BASELINE):
    """6-DoF scene: points in the camera frame, X = T12 * points."""
    rng = np.random.default_rng(seed)
    Kf = np.asarray([338.0, 338.0, 320.0, 240.0] if intr is None else intr, np.float32)
    probes = probe_indices(n)
    Lc = _camera_points(rng, n)
    zero_idx = None
    if stereo:
        zero_idx, pt = _zero_u_point(probes, n, Kf.astype(D), baseline)
        if zero_idx is not None:
            Lc[zero_idx] = pt
    a = rng.uniform(-0.2, 0.2, 3)
    Rm = scenes._rot("x", a[0]) @ scenes._rot("y", a[1]) @ scenes._rot("z", a[2])
    tv = rng.uniform(-0.5, 0.5, 3)
    T12 = np.concatenate([Rm.reshape(9), tv]).astype(np.float32)
    X = (Lc @ Rm.T + tv).astype(np.float32)
    Ri, ti = R6.inv12(T12)
    L = X.astype(D) @ Ri.T + ti
    sc = dict(n=n, X=X, K=Kf, T12=T12, probes=probes, stereo=stereo, opt=opt,
              uv=_pixels(R6.project(L, Kf.astype(D)), _offsets(rng, n, probes, opt)))
    if stereo:
        T_lr12 = np.concatenate([np.eye(3).reshape(9), [baseline, 0, 0]]).astype(np.float32)
        Rrl, trl = R6.inv12(T_lr12)
        sc["T_lr12"] = T_lr12
        _stereo_pixels(rng, sc, R6.project(L @ Rrl.T + trl, Kf.astype(D)), n, probes, opt,
                       zero_idx)
    return sc


def scene3(n, seed, stereo, opt, intr=None, height=0.3, baseline=scenes.BASELINE):
    """Planar scene in the conventions of scenes.planar_pose_only_scene: points
    in the current camera at theta_init, X their base-1 coordinates."""
    rng = np.random.default_rng(seed)
    Kf = np.asarray([scenes.FX, scenes.FY, scenes.CX, scenes.CY] if intr is None else intr,
                    np.float32)
    probes = probe_indices(n)
    Xc = _camera_points(rng, n)
    zero_idx = None
    if stereo:
        zero_idx, pt = _zero_u_point(probes, n, Kf.astype(D), baseline)
        if zero_idx is not None:
            Xc[zero_idx] = pt
    T_bc = np.eye(4)
    T_bc[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    T_bc[:3, 3] = [0.0, 0.0, height]
    theta = np.array([rng.uniform(0.05, 0.25), rng.uniform(-0.15, 0.15),
                      rng.uniform(-0.2, 0.2)])
    Pi = scenes._inv(scenes.planar_T(theta))
    X = ((Xc @ T_bc[:3, :3].T + T_bc[:3, 3]) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
    W_b1 = scenes.planar_T([2.0, -1.0, 0.3])
    f32 = lambda a: np.asarray(a, np.float32)
    sc = dict(n=n, X=X, K=Kf, T_bc=f32(T_bc), T_wl=f32(W_b1 @ T_bc),
              T_wc=f32(W_b1 @ Pi @ T_bc), probes=probes, stereo=stereo, opt=opt)
    # the float64 reference's own linearisation point, from the float32 inputs
    th0 = R3.prior_theta(sc["T_bc"], sc["T_wl"], sc["T_wc"], D)
    Pl = R3.iso_mul(R3.iso_inv(R3.iso(sc["T_bc"], D)), R3.planar_iso(*th0, dtype=D))
    K64 = Kf.astype(D)
    sc["uv"] = _pixels(R6.project(R3.warp(Pl, X.astype(D)), K64),
                       _offsets(rng, n, probes, opt))
    if stereo:
        T_lr = np.eye(4)
        T_lr[0, 3] = baseline
        sc["T_lr"] = f32(T_lr)
        Pr = R3.iso_mul(R3.iso_inv(R3.iso(sc["T_lr"], D)), Pl)
        _stereo_pixels(rng, sc, R6.project(R3.warp(Pr, X.astype(D)), K64), n, probes, opt,
                       zero_idx)
    return sc


COND_MAX = 1e4
# A system of 2 to 6 points is often ill-conditioned (median cond(H) 5e4 for 3
# points in 6-DoF, against ~7e2 from 63 points on) and then measures the fp32
# solve, not the sums: for those cases the seed is the first of 9000, 9001, ...
# at which the float64 reference's cond(H) is below 5e3.  (variant, n, opt,
# batch problem + 1 or 0) -> seed.
TINY_SEEDS = {
    ("mono6", 3, "A", 0): 9004, ("mono6", 6, "A", 0): 9000, ("mono6", 3, "A", 1): 9004,
    ("mono6", 3, "B", 0): 9004, ("mono6", 6, "B", 0): 9000, ("mono6", 3, "B", 1): 9004,
    ("stereo6", 3, "A", 0): 9007, ("stereo6", 6, "A", 0): 9008, ("stereo6", 3, "A", 1): 9007,
    ("stereo6", 3, "B", 0): 9004, ("stereo6", 6, "B", 0): 9000, ("stereo6", 3, "B", 1): 9004,
    ("mono3", 2, "A", 0): 9004, ("mono3", 3, "A", 0): 9001, ("mono3", 6, "A", 0): 9000,
    ("mono3", 2, "A", 1): 9004, ("mono3", 2, "B", 0): 9004, ("mono3", 3, "B", 0): 9001,
    ("mono3", 6, "B", 0): 9000, ("mono3", 2, "B", 1): 9004,
    ("stereo3", 2, "A", 0): 9004, ("stereo3", 3, "A", 0): 9001, ("stereo3", 6, "A", 0): 9000,
    ("stereo3", 2, "A", 1): 9004, ("stereo3", 2, "B", 0): 9004, ("stereo3", 3, "B", 0): 9001,
    ("stereo3", 6, "B", 0): 9000, ("stereo3", 2, "B", 1): 9004,
}


def _seed(variant, n, opt, b=0):
    if (variant, n, opt, b) in TINY_SEEDS:
        return TINY_SEEDS[variant, n, opt, b]
    return 100003 * VARIANTS.index(variant) + 17 * n + 7 * (opt == "B") + 1009 * b + 5


def _build(variant, n, seed, opt, **kw):
    build = scene6 if variant.endswith("6") else scene3
    return build(n, seed, variant.startswith("stereo"), opt, **kw)


@functools.lru_cache(maxsize=None)
def scene(variant, n, opt):
    """The scene of one single-call case (cached: read, never written)."""
    return _build(variant, n, _seed(variant, n, opt), opt)


def _batch_kw(variant, opt):
    """(n, scene arguments) of the problems of a batch: own intrinsics, stereo
    baseline and (planar) camera height each."""
    rng = np.random.default_rng(100003 * VARIANTS.index(variant) + 7 * (opt == "B") + 99)
    out = []
    for n in BATCH_SIZES:
        if variant.endswith("3") and n == 3:
            n = 2
        fx = rng.uniform(300.0, 600.0)
        kw = dict(intr=[fx, fx * rng.uniform(0.98, 1.02), rng.uniform(300.0, 340.0),
                        rng.uniform(220.0, 260.0)], baseline=rng.uniform(0.10, 0.15))
        if variant.endswith("3"):
            kw["height"] = rng.uniform(0.2, 0.5)
        out.append((n, kw))
    return out


@functools.lru_cache(maxsize=None)
def batch(variant, opt):
    """The problems of one batch case: a list of scenes (None for the empty
    problem), each with its own pose and intrinsics."""
    return [None if n == 0 else _build(variant, n, _seed(variant, n, opt, b + 1), opt, **kw)
            for b, (n, kw) in enumerate(_batch_kw(variant, opt))]


# ---- references -----------------------------------------------------------------
def _ref64(sc, max_iter):
    kw = dict(OPTS[sc["opt"]], max_iter=max_iter, thr_step=0.0, thr_cost=0.0)
    n = sc["n"]
    K = sc["K"]
    if "T12" in sc:
        if sc["stereo"]:
            kw.update(uv_right=sc["uv_right"], intr_r=K, T_lr12=sc["T_lr12"],
                      mask_r=np.ones(n, bool))
        return R6.solve(sc["X"], sc["uv"], K[0], K[1], K[2], K[3], sc["T12"], np.ones(n, bool),
                        **kw)
    if sc["stereo"]:
        kw.update(uv_right=sc["uv_right"], intr_r=K, T_lr=sc["T_lr"], mask_r=np.ones(n, bool))
    return R3.solve(sc["X"], sc["uv"], K[0], K[1], K[2], K[3], sc["T_bc"], sc["T_wl"],
                    sc["T_wc"], np.ones(n, bool), dtype=D, **kw)


_REF = {}


def ref64(sc, max_iter=1):
    """The float64 reference of a scene (computed once, shared, read-only)."""
    key = (id(sc), max_iter)
    if key not in _REF:
        _REF[key] = (sc, _ref64(sc, max_iter))     # (holds sc: its id stays taken)
    return _REF[key][1]


def ref32(sc, max_iter=1):
    """The project's fp32 CPU restatement on the same inputs."""
    from oracle import oracle_py as O
    kw = dict(OPTS[sc["opt"]], max_iter=max_iter, thr_step=0.0, thr_cost=0.0)
    n = sc["n"]
    K = sc["K"]
    if "T12" in sc:
        T44 = np.eye(4, dtype=np.float32)
        T44[:3, :3], T44[:3, 3] = sc["T12"][:9].reshape(3, 3), sc["T12"][9:]
        ones = np.ones(n, np.uint8)
        if sc["stereo"]:
            Tlr = np.eye(4, dtype=np.float32)
            Tlr[:3, 3] = sc["T_lr12"][9:]
            return O.pose_only_stereo6(sc["X"], sc["uv"], sc["uv_right"], K, K, Tlr, T44, ones,
                                       ones, O.make_options(**kw))
        return O.pose_only_mono6(sc["X"], sc["uv"], K[0], K[1], K[2], K[3], T44, ones,
                                 O.make_options(**kw))
    if sc["stereo"]:
        kw.update(uv_right=sc["uv_right"], intr_r=K, T_lr=sc["T_lr"], mask_r=np.ones(n, bool))
    return R3.solve(sc["X"], sc["uv"], K[0], K[1], K[2], K[3], sc["T_bc"], sc["T_wl"],
                    sc["T_wc"], np.ones(n, bool), **kw)


# ---- checks shared by the CPU and the GPU test ------------------------------------
def mask_keys(sc):
    return ("mask_l", "mask_r") if sc["stereo"] else ("mask",)


def deviations(res, ref):
    """Largest deviation of a result from the float64 reference over the rows.
    cost: relative.  cost_change = |cost - previous| (previous = 1e10 in the
    first row): relative to the larger of the two, which is what bounds its
    error; relative to itself it is noise once the costs agree.  step: relative
    to the FIRST row's step: the later steps of a converging solve go to zero
    while their error stays that of the same sums (H^-1 times the rounding of
    g), so the first step is the scale.  T12: absolute."""
    assert len(res["rows"]) == len(ref["rows"]) >= 1
    a, b = np.array(res["rows"], D), np.array(ref["rows"], D)
    prev = np.concatenate([[1e10], b[:-1, 0]])
    return dict(cost=(np.abs(a[:, 0] - b[:, 0]) / np.abs(b[:, 0])).max(),
                change=(np.abs(a[:, 1] - b[:, 1]) / np.maximum(prev, b[:, 0])).max(),
                step=(np.abs(a[:, 2] - b[:, 2]) / b[0, 2]).max(),
                T12=np.abs(np.asarray(res["T12"], D) - ref["T12"]).max())


def check_preconditions(sc, ref, cost_tol):
    """From the float64 reference alone: every edge at least MARGIN_PX from both
    thresholds, (cost_tol not None) every probe edge's share of the total cost
    at least 8x the cost tolerance, and cond(H) at most COND_MAX.  Returns (margin, smallest share)."""
    o = OPTS[sc["opt"]]
    e = ref["edges"]
    ars = [e["ars_l"]] + ([e["ars_r"]] if sc["stereo"] else [])
    margin = min(min(np.abs(a - np.float32(t)).min() for t in (o["huber"], o["outlier"]))
                 for a in ars if a.size)
    assert margin >= MARGIN_PX, margin
    total = e["err_l"].sum() + (e["err_r"].sum() if sc["stereo"] else 0.0)
    share = e["err_l"][sc["probes"]].min() / total
    if sc["stereo"]:
        pos = np.cumsum(e["has_r"]) - 1          # index into the right edges
        pr = [p for p in sc["probes"] if e["has_r"][p]]
        assert not e["has_r"][sc["no_right"]].any() and len(pr) >= 1
        if pr:
            share = min(share, e["err_r"][pos[pr]].min() / total)
    if cost_tol is not None:
        assert share >= 8.0 * cost_tol, (share, cost_tol)
    assert ref["cond"] <= COND_MAX, ref["cond"]
    return margin, share


def expected_classes(sc):
    """The masks the construction implies under set A: probes at even positions
    of the probe list are outliers (left, and right where matched)."""
    n = sc["n"]
    out = np.zeros(n, bool)
    if sc["opt"] == "A":
        out[sc["probes"][0::2]] = True
    left = ~out
    if not sc["stereo"]:
        return dict(mask=left)
    right = ~out
    right[sc["no_right"]] = True
    return dict(mask_l=left, mask_r=right)


def all_cases():
    """(scene, max_iter, cost compared) of every case of the GPU module."""
    for v in VARIANTS:
        for o in "AB":
            for n in sizes(v):
                yield scene(v, n, o), 1, cost_compared(o, n)
        for n in SIZES_3ITER:
            yield scene(v, n, "B"), 3, True
        for o in "AB":
            for sc in batch(v, o):
                if sc is not None:
                    yield sc, 1, cost_compared(o, sc["n"])


if __name__ == "__main__":     # print the MEASURED table
    import math
    worst = {}
    for sc, it, cc in all_cases():
        dev = deviations(ref32(sc, it), ref64(sc, it))
        w = worst.setdefault(size_class(sc["n"]), {})
        for q, x in dev.items():
            if q != "cost" or (cc and size_class(sc["n"]) != "large"):
                w[q] = max(w.get(q, 0.0), x)
    def up(x):                 # two significant digits, rounded up
        e = 10.0 ** (math.floor(math.log10(x)) - 1)
        return math.ceil(x / e) * e
    for c in ("tiny", "small", "mid", "large"):
        print('    "%s": dict(%s),' % (c, ", ".join(
            "%s=%.1e" % (q, up(worst[c][q])) for q in ("cost", "change", "step", "T12")
            if q in worst[c])))
