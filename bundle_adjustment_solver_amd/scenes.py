"""Seeded synthetic scenes for the BA hot path.

* test_ba_scene        — the stereo wall scene of reference test/test_ba.cpp:
                         53-232 (60 poses, 660 landmarks, 34 019 observations),
                         seeded instead of std::random_device.
* synthetic_ba_scene   — configs C2..C4: the same camera rig and trajectory
                         law extended to N poses; every landmark is seen by a
                         window of consecutive poses.
* pose_only_scene      — config C5: reference
                         test/test_compare_ceres_vs_native.cpp:20-95.
* planar_pose_only_scene — planar 3-DoF pose-only (wheeled base, forward
                         camera), mono or stereo.
All quantities are in USER units (metres, pixels, world->camera 4x4 poses);
the solver facade applies the reference's 0.01 scaling.
"""
import numpy as np

SEED_BASE = 20240600
FX = FY = 525.0
CX, CY = 320.0, 240.0
WIDTH, HEIGHT = 640, 480
BASELINE = 0.12


def _rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], float)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], float)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], float)


def stereo_cameras(stereo=True):
    """reference test/test_ba.cpp:79-98: (intr [n,4], T_cj [n,4,4])."""
    intr = [[FX, FY, CX, CY]]
    T = [np.eye(4)]
    if stereo:
        intr.append([FX, FY, CX, CY])
        Tr = np.eye(4)
        Tr[0, 3] = -BASELINE  # inverse of left->right translate(+0.12, 0, 0)
        T.append(Tr)
    return np.array(intr), np.stack(T)


def trajectory(n_pose):
    """World->camera poses T_wc, reference test/test_ba.cpp:132-171."""
    base_to_cam = np.eye(4)
    base_to_cam[:3, :3] = _rot("y", np.pi / 2) @ _rot("z", -np.pi / 2)
    x_step = float(np.float32(0.005))
    y_step = float(np.float32(0.2))
    yaw_step = float(np.float32(0.005))
    w2b = np.eye(4)
    w2b[:3, :3] = _rot("z", -0.1)
    w2b[:3, 3] = [-4.0, -2.5, 0.0]
    Rz = _rot("z", yaw_step)
    out = np.zeros((n_pose, 4, 4))
    for k in range(n_pose):
        w2b[:3, :3] = w2b[:3, :3] @ Rz
        w2b[0, 3] += x_step
        w2b[1, 3] += y_step
        out[k] = w2b @ base_to_cam
    return out


def _inv(T):
    R = T[..., :3, :3]
    t = T[..., :3, 3]
    out = np.zeros_like(T)
    Rt = np.swapaxes(R, -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, t)
    out[..., 3, 3] = 1.0
    return out


def _wall_points():
    """reference test/test_ba.cpp:53-77 (float loop counters)."""
    pts = []
    z = np.float32(1.7)
    while z <= np.float32(5.7):
        y = np.float32(0.0)
        while y <= np.float32(26.0):
            pts.append([8.5, float(y), float(z)])
            y = np.float32(y + np.float32(0.4))
        z = np.float32(z + np.float32(0.4))
    return np.array(pts, float)


def test_ba_scene(seed=SEED_BASE + 1, pixel_sigma=0.0):
    """Scene of reference test/test_ba.cpp (config C1)."""
    rng = np.random.default_rng(seed)
    n_pose, n_fixed = 60, 5
    intr, T_cj = stereo_cameras(True)
    T_wc_true = trajectory(n_pose)
    X_true = _wall_points()
    n_pt = X_true.shape[0]
    T_wc_init = T_wc_true.copy()
    T_wc_init[n_fixed:, :3, 3] += rng.uniform(-0.1, 0.1, (n_pose - n_fixed, 3)) \
        .astype(np.float32)
    X_init = X_true + rng.uniform(-0.5, 0.5, (n_pt, 3)).astype(np.float32)
    T_cw = _inv(T_wc_true)
    cams, poses, pts, pix = [], [], [], []
    for j in range(n_pose):
        local = X_true @ T_cw[j, :3, :3].T + T_cw[j, :3, 3]
        for c in range(2):
            Xc = local @ T_cj[c, :3, :3].T + T_cj[c, :3, 3]
            inv_z = (1.0 / Xc[:, 2]).astype(np.float32).astype(np.float64)
            u = intr[c, 0] * Xc[:, 0] * inv_z + intr[c, 2]
            v = intr[c, 1] * Xc[:, 1] * inv_z + intr[c, 3]
            if pixel_sigma > 0:
                u = u + rng.normal(0, pixel_sigma, n_pt)
                v = v + rng.normal(0, pixel_sigma, n_pt)
            seen = (u < WIDTH) & (u > 0) & (v < HEIGHT) & (v > 0)
            idx = np.nonzero(seen)[0]
            cams.append(np.full(idx.size, c, np.int32))
            poses.append(np.full(idx.size, j, np.int32))
            pts.append(idx.astype(np.int32))
            pix.append(np.stack([u[idx], v[idx]], axis=1))
    return dict(
        intr=intr, T_cj=T_cj, T_wc_true=T_wc_true, T_wc_init=T_wc_init,
        X_true=X_true, X_init=X_init,
        pose_fixed=np.arange(n_pose) < n_fixed,
        pt_fixed=np.zeros(n_pt, bool),
        obs_cam=np.concatenate(cams), obs_pose=np.concatenate(poses),
        obs_pt=np.concatenate(pts), obs_uv=np.concatenate(pix, axis=0))


def synthetic_ba_scene(n_pose, n_pt, window, stereo, seed, n_fixed=5,
                       pixel_sigma=0.0, pose_noise=0.1, point_noise=0.5, dropout=0.0):
    """Configs C2..C4: every landmark is seen by `window`
    consecutive poses in every camera -> n_obs = n_pt * window * n_cam.
    dropout > 0 (config C4R): every observation is dropped independently with that
    probability (occlusion / track loss), a landmark keeps at least two — the
    observation patterns then differ from landmark to landmark."""
    rng = np.random.default_rng(seed)
    intr, T_cj = stereo_cameras(stereo)
    n_cam = intr.shape[0]
    T_wc_true = trajectory(n_pose)
    T_cw = _inv(T_wc_true)
    T_cam_w = np.einsum("cij,pjk->pcik", T_cj, T_cw)   # [pose, cam] world->cam
    half = window // 2
    X_true = np.zeros((n_pt, 3))
    first = np.zeros(n_pt, np.int64)
    uv_all = np.zeros((n_pt, window, n_cam, 2))
    done = 0
    while done < n_pt:
        m = int((n_pt - done) * 1.3) + 64
        center = rng.integers(half, n_pose - (window - half) + 1, m)
        depth = rng.uniform(4.0, 12.0, m)
        pu = rng.uniform(0, WIDTH, m)
        pv = rng.uniform(0, HEIGHT, m)
        Xc = np.stack([(pu - CX) / FX * depth, (pv - CY) / FY * depth, depth], 1)
        Tw = T_wc_true[center]
        Xw = np.einsum("mij,mj->mi", Tw[:, :3, :3], Xc) + Tw[:, :3, 3]
        f0 = center - half
        ok = np.ones(m, bool)
        uvw = np.zeros((m, window, n_cam, 2))
        for w in range(window):
            T = T_cam_w[f0 + w]                      # [m, cam, 4, 4]
            Xl = np.einsum("mcij,mj->mci", T[:, :, :3, :3], Xw) + T[:, :, :3, 3]
            z = Xl[..., 2]
            u = intr[None, :, 0] * Xl[..., 0] / z + intr[None, :, 2]
            v = intr[None, :, 1] * Xl[..., 1] / z + intr[None, :, 3]
            good = (z > 0) & (u > 0) & (u < WIDTH) & (v > 0) & (v < HEIGHT)
            ok &= good.all(axis=1)
            uvw[:, w, :, 0] = u
            uvw[:, w, :, 1] = v
        idx = np.nonzero(ok)[0][:n_pt - done]
        k = idx.size
        X_true[done:done + k] = Xw[idx]
        first[done:done + k] = f0[idx]
        uv_all[done:done + k] = uvw[idx]
        done += k
    # observation list, insertion order pose-major, left then right, landmark
    lm = np.repeat(np.arange(n_pt), window * n_cam)
    wi = np.tile(np.repeat(np.arange(window), n_cam), n_pt)
    ci = np.tile(np.arange(n_cam), n_pt * window)
    pose = first[lm] + wi
    uv = uv_all.reshape(-1, 2)
    if pixel_sigma > 0:
        uv = uv + rng.normal(0, pixel_sigma, uv.shape)
    if dropout > 0:
        keep = rng.uniform(size=lm.size) >= dropout
        # (a landmark keeps its first two observations whatever the draw)
        first_two = np.tile(np.arange(window * n_cam) < 2, n_pt)
        keep |= first_two
        lm, ci, pose, uv = lm[keep], ci[keep], pose[keep], uv[keep]
    order = np.lexsort((lm, ci, pose))
    T_wc_init = T_wc_true.copy()
    T_wc_init[n_fixed:, :3, 3] += rng.uniform(-pose_noise, pose_noise,
                                              (n_pose - n_fixed, 3))
    X_init = X_true + rng.uniform(-point_noise, point_noise, (n_pt, 3))
    return dict(
        intr=intr, T_cj=T_cj, T_wc_true=T_wc_true, T_wc_init=T_wc_init,
        X_true=X_true, X_init=X_init,
        pose_fixed=np.arange(n_pose) < n_fixed,
        pt_fixed=np.zeros(n_pt, bool),
        obs_cam=ci[order].astype(np.int32),
        obs_pose=pose[order].astype(np.int32),
        obs_pt=lm[order].astype(np.int32), obs_uv=uv[order])


# name -> (n_pose, n_pt, window, stereo, seed)   (BASELINE.json configs)
CONFIGS = {
    "C2": (200, 50_000, 10, False, SEED_BASE + 2),
    "C3": (500, 200_000, 5, True, SEED_BASE + 3),
    "C4": (1000, 500_000, 5, True, SEED_BASE + 4),
}


def dense_covisibility_scene(n_pose, n_pt, views, seed, n_fixed=5, pose_noise=0.02,
                            point_noise=0.1, pixel_sigma=0.0):
    """Off-the-happy-path scene: the rig circles a cloud of points and every
    landmark is seen from `views` RANDOM poses (loop closures everywhere), so
    that with enough landmarks every pair of poses shares some: the reduced
    camera system has no zero block and the structure-aware solve degenerates
    to the plain dense sweep.  One camera."""
    rng = np.random.default_rng(seed)
    intr = np.array([[FX, FY, CX, CY]])
    T_cj = np.eye(4)[None]
    ang = 2 * np.pi * np.arange(n_pose) / n_pose
    T_wc_true = np.tile(np.eye(4), (n_pose, 1, 1))
    radius = 12.0
    for k in range(n_pose):
        # camera on a circle of radius 12 m, looking at the centre
        c = np.array([radius * np.cos(ang[k]), radius * np.sin(ang[k]), 0.3 * np.sin(3 * ang[k])])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        T_wc_true[k, :3, :3] = np.stack([x, y, z], axis=1)
        T_wc_true[k, :3, 3] = c
    X_true = rng.uniform(-2.0, 2.0, (n_pt, 3))
    T_cw = _inv(T_wc_true)
    pose = np.stack([rng.choice(n_pose, views, replace=False) for _ in range(n_pt)])
    pose.sort(axis=1)
    lm = np.repeat(np.arange(n_pt), views)
    pj = pose.reshape(-1)
    Xl = np.einsum("nij,nj->ni", T_cw[pj, :3, :3], X_true[lm]) + T_cw[pj, :3, 3]
    uv = np.stack([FX * Xl[:, 0] / Xl[:, 2] + CX, FY * Xl[:, 1] / Xl[:, 2] + CY], 1)
    assert (Xl[:, 2] > 0).all()
    if pixel_sigma > 0:
        uv = uv + rng.normal(0, pixel_sigma, uv.shape)
    order = np.lexsort((lm, pj))
    T_wc_init = T_wc_true.copy()
    T_wc_init[n_fixed:, :3, 3] += rng.uniform(-pose_noise, pose_noise, (n_pose - n_fixed, 3))
    return dict(
        intr=intr, T_cj=T_cj, T_wc_true=T_wc_true, T_wc_init=T_wc_init,
        X_true=X_true, X_init=X_true + rng.uniform(-point_noise, point_noise, (n_pt, 3)),
        pose_fixed=np.arange(n_pose) < n_fixed, pt_fixed=np.zeros(n_pt, bool),
        obs_cam=np.zeros(lm.size, np.int32), obs_pose=pj[order].astype(np.int32),
        obs_pt=lm[order].astype(np.int32), obs_uv=uv[order])


# configurations OFF the headline's happy path (bench.py --config ...)
OFFPATH = {
    # C4 with per-observation dropout (p = 0.15): real visibility — occlusion, image
    # borders, track loss — breaks the exact repetition of observation patterns that the
    # covisibility groups of the headline scene rely on
    "C4R": ("window_dropout", (1000, 500_000, 5, True, SEED_BASE + 4, 0.15)),
    # mono, windows of 20 poses: a landmark's 210 block pairs exceed the 128 register
    # slots of a super-run and its pose set the 10 poses of a covisibility group ->
    # everything goes through k_schur_partial's global triple list
    "W20": ("window", (500, 100_000, 20, False, SEED_BASE + 7)),
    # 1000 poses, every landmark seen from 8 random poses: S is fully dense
    "DENSE1K": ("dense", (1000, 60_000, 8, SEED_BASE + 8)),
}


def config_scene(name, scale=1.0, pixel_sigma=0.0, landmark_factor=1):
    """Scene of a BASELINE.json config; scale<1 shrinks poses and landmarks
    proportionally (parity-test sizes); pixel_sigma is the measurement noise in
    pixels (0, and a second run at 0.5); landmark_factor multiplies
    landmarks and observations at FIXED poses (bench.py --weak: the per-GPU share
    of the sharded work stays that of the one-GPU problem)."""
    if name == "C1":
        if landmark_factor != 1:
            raise ValueError("C1 is the fixed scene of test_ba.cpp: no landmark_factor")
        return test_ba_scene(pixel_sigma=pixel_sigma)
    if name in OFFPATH:
        kind, par = OFFPATH[name]
        if kind == "dense":
            n_pose, n_pt, views, seed = par
            return dense_covisibility_scene(max(20, int(round(n_pose * scale))),
                                            max(200, int(round(n_pt * scale))) * landmark_factor,
                                            views, seed, pixel_sigma=pixel_sigma)
        if kind == "window_dropout":
            n_pose, n_pt, window, stereo, seed, drop = par
            return synthetic_ba_scene(max(window + 6, int(round(n_pose * scale))),
                                      max(16, int(round(n_pt * scale))) * landmark_factor, window,
                                      stereo, seed, pixel_sigma=pixel_sigma, dropout=drop)
        n_pose, n_pt, window, stereo, seed = par
        return synthetic_ba_scene(max(window + 6, int(round(n_pose * scale))),
                                  max(16, int(round(n_pt * scale))) * landmark_factor, window,
                                  stereo, seed, pixel_sigma=pixel_sigma)
    n_pose, n_pt, window, stereo, seed = CONFIGS[name]
    n_pose = max(window + 6, int(round(n_pose * scale)))
    n_pt = max(16, int(round(n_pt * scale))) * landmark_factor
    return synthetic_ba_scene(n_pose, n_pt, window, stereo, seed,
                              pixel_sigma=pixel_sigma)


def pose_window_subscene(scene, p0, p1, n_fixed=5):
    """The part of a window scene that lives on poses [p0, p1): those poses (the
    first n_fixed of them fixed at their true values) and every landmark all of
    whose observations fall inside; indices re-based.  Used to cut small test
    problems out of a BASELINE config that keep a specific landmark's geometry."""
    n_pt = scene["X_true"].shape[0]
    first = np.full(n_pt, np.iinfo(np.int64).max)
    last = np.full(n_pt, -1)
    np.minimum.at(first, scene["obs_pt"], scene["obs_pose"])
    np.maximum.at(last, scene["obs_pt"], scene["obs_pose"])
    keep_pt = (first >= p0) & (last < p1)
    new_index = np.cumsum(keep_pt) - 1
    keep_obs = keep_pt[scene["obs_pt"]]
    out = dict(
        intr=scene["intr"], T_cj=scene["T_cj"],
        T_wc_true=scene["T_wc_true"][p0:p1].copy(),
        T_wc_init=scene["T_wc_init"][p0:p1].copy(),
        X_true=scene["X_true"][keep_pt], X_init=scene["X_init"][keep_pt],
        pose_fixed=np.arange(p1 - p0) < n_fixed,
        pt_fixed=np.zeros(int(keep_pt.sum()), bool),
        obs_cam=scene["obs_cam"][keep_obs],
        obs_pose=(scene["obs_pose"][keep_obs] - p0).astype(np.int32),
        obs_pt=new_index[scene["obs_pt"][keep_obs]].astype(np.int32),
        obs_uv=scene["obs_uv"][keep_obs])
    out["T_wc_init"][:n_fixed] = out["T_wc_true"][:n_fixed]
    return out


def ba_batch_scene(B, n_pose=10, n_pt=300, stereo=True, seed=SEED_BASE + 9, pixel_sigma=0.0,
                   n_fixed=2, pose_noise=0.05, point_noise=0.2):
    """B independent window problems for the batched full-BA solver (ba_batch_*):
    problem b is a synthetic scene of its own (synthetic_ba_scene, seed + 7919 * b) of
    n_pose poses — the first n_fixed of them fixed at their true values — and n_pt
    landmarks, every one seen by every pose in every camera, taken whole through
    pose_window_subscene.  Returns a list of B scene dicts."""
    out = []
    for b in range(B):
        big = synthetic_ba_scene(n_pose, n_pt, n_pose, stereo, seed + 7919 * b, n_fixed=n_fixed,
                                 pixel_sigma=pixel_sigma, pose_noise=pose_noise,
                                 point_noise=point_noise)
        out.append(pose_window_subscene(big, 0, n_pose, n_fixed=n_fixed))
    return out


def scaled_problem(scene):
    """Apply the facade's host preprocessing (reference
    core/full_bundle_adjustment_solver.cpp:72-117,155-180): 0.01 scaling,
    T_jw = pose^-1; returns the C-ABI level arrays."""
    s = 0.01
    intr = scene["intr"] * s
    T_cj = scene["T_cj"].copy()
    T_cj[:, :3, 3] *= s
    T_jw = _inv(scene["T_wc_init"])
    T_jw[:, :3, 3] *= s
    to12 = lambda T: np.concatenate(
        [T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], axis=1)
    return dict(
        cam_intr=np.ascontiguousarray(intr), cam_T=to12(T_cj),
        pose_T=to12(T_jw), pose_fixed=scene["pose_fixed"].astype(np.uint8),
        pt_X=np.ascontiguousarray(scene["X_init"] * s),
        pt_fixed=scene["pt_fixed"].astype(np.uint8),
        obs_cam=scene["obs_cam"].astype(np.int32),
        obs_pose=scene["obs_pose"].astype(np.int32),
        obs_pt=scene["obs_pt"].astype(np.int32),
        obs_uv=np.ascontiguousarray(scene["obs_uv"] * s))


def pose_only_scene(n=10_000, seed=SEED_BASE + 5, pixel_sigma=0.0):
    """Config C5, reference test/test_compare_ceres_vs_native.cpp:20-95."""
    rng = np.random.default_rng(seed)
    fx = fy = 338.0
    cx, cy = 320.0, 240.0
    T_true = np.eye(4, dtype=np.float32)
    T_true[:3, :3] = _rot("y", -0.5).astype(np.float32)
    T_true[:3, 3] = [0.2, 0.3, -1.9]
    X = np.stack([rng.uniform(-1.7, 1.7, n), rng.uniform(-1.3, 1.3, n),
                  rng.uniform(0, 5.0, n) + 1.2], axis=1).astype(np.float32)
    Ti = _inv(T_true.astype(np.float64)).astype(np.float32)
    L = X @ Ti[:3, :3].T + Ti[:3, 3]
    inv_z = (np.float32(1.0) / L[:, 2]).astype(np.float32)
    uv = np.stack([fx * L[:, 0] * inv_z + cx, fy * L[:, 1] * inv_z + cy],
                  axis=1).astype(np.float32)
    if pixel_sigma > 0:
        uv = (uv + rng.normal(0, pixel_sigma, uv.shape)).astype(np.float32)
    return dict(X=X, uv=uv, fx=fx, fy=fy, cx=cx, cy=cy, T_true=T_true,
                T_init=np.eye(4, dtype=np.float32))


def hover_scene(n_pose, n_pt, n_cam, seed, n_fixed=2, visible_frac=1.0,
                pose_noise=0.02, point_noise=0.1):
    """Test scene with arbitrary camera count and dense visibility: the rig
    hovers around the origin looking down +z at a cloud of points, every camera
    of every pose sees every point (or a random `visible_frac` of them).  Used
    for the structure edge cases the window scenes cannot produce: landmarks
    seen by more than 128 poses, rigs with more than 8 cameras, ragged
    landmarks."""
    rng = np.random.default_rng(seed)
    intr = np.tile(np.array([[FX, FY, CX, CY]]), (n_cam, 1))
    T_cj = np.tile(np.eye(4), (n_cam, 1, 1))
    T_cj[:, 0, 3] = -0.05 * np.arange(n_cam)           # cameras side by side
    T_wc_true = np.tile(np.eye(4), (n_pose, 1, 1))
    for k in range(n_pose):
        ang = rng.uniform(-0.03, 0.03, 3)
        T_wc_true[k, :3, :3] = _rot("x", ang[0]) @ _rot("y", ang[1]) @ _rot("z", ang[2])
        T_wc_true[k, :3, 3] = rng.uniform(-0.3, 0.3, 3)
    X_true = np.stack([rng.uniform(-1.5, 1.5, n_pt), rng.uniform(-1.0, 1.0, n_pt),
                       rng.uniform(6.0, 10.0, n_pt)], 1)
    T_cw = _inv(T_wc_true)
    oc, op, oq, uv = [], [], [], []
    for j in range(n_pose):
        for c in range(n_cam):
            T = T_cj[c] @ T_cw[j]
            Xl = X_true @ T[:3, :3].T + T[:3, 3]
            u = intr[c, 0] * Xl[:, 0] / Xl[:, 2] + intr[c, 2]
            v = intr[c, 1] * Xl[:, 1] / Xl[:, 2] + intr[c, 3]
            sel = np.nonzero(rng.uniform(size=n_pt) < visible_frac)[0]
            oc.append(np.full(sel.size, c)); op.append(np.full(sel.size, j))
            oq.append(sel); uv.append(np.stack([u[sel], v[sel]], 1))
    T_wc_init = T_wc_true.copy()
    T_wc_init[n_fixed:, :3, 3] += rng.uniform(-pose_noise, pose_noise,
                                              (n_pose - n_fixed, 3))
    return dict(
        intr=intr, T_cj=T_cj, T_wc_true=T_wc_true, T_wc_init=T_wc_init,
        X_true=X_true, X_init=X_true + rng.uniform(-point_noise, point_noise, (n_pt, 3)),
        pose_fixed=np.arange(n_pose) < n_fixed, pt_fixed=np.zeros(n_pt, bool),
        obs_cam=np.concatenate(oc).astype(np.int32),
        obs_pose=np.concatenate(op).astype(np.int32),
        obs_pt=np.concatenate(oq).astype(np.int32), obs_uv=np.concatenate(uv))


def pose_only_stereo_scene(n=10_000, seed=SEED_BASE + 6, pixel_sigma=0.0,
                           right_missing_frac=0.2):
    """Stereo variant of the pose-only scene (reference
    core/pose_only_bundle_adjustment_solver.cpp:172-399 conventions): the right
    camera sees X_r = left_to_right^-1 * X_l with left_to_right = translate(+0.12,
    0, 0) (reference test/test_ba.cpp:88-97); a fraction of the points has no
    right match, marked by a negative right pixel (:298)."""
    sc = pose_only_scene(n, seed=seed, pixel_sigma=pixel_sigma)
    rng = np.random.default_rng(seed + 1000)
    T_lr = np.eye(4, dtype=np.float32)
    T_lr[0, 3] = BASELINE
    Ti = _inv(sc["T_true"].astype(np.float64)).astype(np.float32)
    L = sc["X"] @ Ti[:3, :3].T + Ti[:3, 3]
    Tr = _inv(T_lr.astype(np.float64)).astype(np.float32)
    Lr = L @ Tr[:3, :3].T + Tr[:3, 3]
    inv_z = (np.float32(1.0) / Lr[:, 2]).astype(np.float32)
    uvr = np.stack([sc["fx"] * Lr[:, 0] * inv_z + sc["cx"],
                    sc["fy"] * Lr[:, 1] * inv_z + sc["cy"]], axis=1).astype(np.float32)
    if pixel_sigma > 0:
        uvr = (uvr + rng.normal(0, pixel_sigma, uvr.shape)).astype(np.float32)
    miss = rng.uniform(size=n) < right_missing_frac
    uvr[miss] = -1.0
    sc.update(uv_right=uvr, T_lr=T_lr, right_missing=miss)
    return sc


def pose_only_batch_scene(B, n_min, n_max, seed, stereo=False, pixel_sigma=0.0,
                          right_missing_frac=0.0, outlier_frac=0.0):
    """B independent 6-DoF pose-only problems for the batched solvers
    (ba_pose_only_{mono,stereo}6_batch), concatenated: problem b owns rows
    [offsets[b], offsets[b+1]) of X / uv (/ uv_right, right_missing).  Each has
    n_min..n_max points drawn by pose_only_scene / pose_only_stereo_scene, its
    own intrinsics (fx 300..600), a true pose near the scene's (+-0.05 rad,
    +-0.1 m), a start pose near the true one (+-0.03 rad, +-0.05 m), and, in
    stereo, its own baseline (0.10..0.15 m); pixels get `pixel_sigma` noise and
    an `outlier_frac` of the points a gross error of 20..60 px.  Seeded."""
    rng = np.random.default_rng(seed)
    ns = rng.integers(n_min, n_max + 1, B)
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum(ns)

    def perturb(T, ang, lin):
        a = rng.uniform(-ang, ang, 3)
        P = np.eye(4)
        P[:3, :3] = _rot("x", a[0]) @ _rot("y", a[1]) @ _rot("z", a[2])
        P[:3, 3] = rng.uniform(-lin, lin, 3)
        return (T.astype(np.float64) @ P).astype(np.float32)

    def project(L, k):
        inv_z = (np.float32(1.0) / L[:, 2]).astype(np.float32)
        return np.stack([k[0] * L[:, 0] * inv_z + k[2], k[1] * L[:, 1] * inv_z + k[3]],
                        axis=1).astype(np.float32)

    Xs, uvs, uvrs, miss = [], [], [], []
    intr = np.zeros((B, 4), np.float32)
    T_lr = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T_true = np.zeros((B, 4, 4), np.float32)
    T_init = np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        n = int(ns[b])
        sub = int(rng.integers(1 << 30))
        sc = (pose_only_stereo_scene(n, seed=sub, right_missing_frac=right_missing_frac)
              if stereo else pose_only_scene(n, seed=sub))
        fx = rng.uniform(300.0, 600.0)
        intr[b] = [fx, fx * rng.uniform(0.98, 1.02), rng.uniform(300.0, 340.0),
                   rng.uniform(220.0, 260.0)]
        T_true[b] = perturb(sc["T_true"], 0.05, 0.1)
        T_init[b] = perturb(T_true[b], 0.03, 0.05)
        Ti = _inv(T_true[b].astype(np.float64)).astype(np.float32)
        L = sc["X"] @ Ti[:3, :3].T + Ti[:3, 3]
        uv = project(L, intr[b])
        bad = rng.uniform(size=n) < outlier_frac
        err = rng.uniform(20.0, 60.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        if pixel_sigma > 0:
            uv = uv + rng.normal(0, pixel_sigma, uv.shape)
        uvs.append((uv + bad[:, None] * err).astype(np.float32))
        Xs.append(sc["X"])
        if stereo:
            T_lr[b, 0, 3] = rng.uniform(0.10, 0.15)
            Tr = _inv(T_lr[b].astype(np.float64)).astype(np.float32)
            uvr = project(L @ Tr[:3, :3].T + Tr[:3, 3], intr[b])
            if pixel_sigma > 0:
                uvr = uvr + rng.normal(0, pixel_sigma, uvr.shape)
            uvr = (uvr + bad[:, None] * err[:, ::-1]).astype(np.float32)
            uvr[sc["right_missing"]] = -1.0
            uvrs.append(uvr)
            miss.append(sc["right_missing"])
    out = dict(B=B, offsets=offsets, n=ns.astype(np.int32), X=np.concatenate(Xs),
               uv=np.concatenate(uvs), intr=intr, T_true=T_true, T_init=T_init)
    if stereo:
        out.update(uv_right=np.concatenate(uvrs), intr_r=intr.copy(), T_lr=T_lr,
                   right_missing=np.concatenate(miss))
    return out


def planar_T(theta):
    """4x4 pose_b2b1 of the planar parameters (x, y, psi): rotation psi about
    the base z axis, translation (x, y, 0) (reference
    core/pose_only_bundle_adjustment_solver.cpp:484-489)."""
    T = np.eye(4)
    T[:3, :3] = _rot("z", theta[2])
    T[:2, 3] = theta[:2]
    return T


def planar_pose_only_scene(n=10_000, seed=SEED_BASE + 7, pixel_sigma=0.0,
                           stereo=False, right_missing_frac=0.2, intr=None,
                           height=0.3, baseline=BASELINE):
    """Planar 3-DoF pose-only scene (reference
    core/pose_only_bundle_adjustment_solver.cpp:401-900 conventions): a wheeled
    base carries a forward-looking camera (optical axis along base x, image x
    along -base y, image y along -base z, 0.3 m above the base origin); between
    the last and the current frame the base moves by theta = (x, y, psi),
    |t| <= 0.3 m, |psi| <= 0.2 rad.  The points X are base-1 coordinates in
    front of the camera.  world_to_last (T_wl) is the camera of a base at a
    planar world pose W_b1; world_to_current (T_wc_init) is chosen so that the
    reference's prior, T_bc * (T_wc^-1 * T_wl) * T_bc^-1, is pose_b2b1 of the
    perturbed theta_init.  T_out_true is what the reference writes back at the
    true theta: pose_b2b1^-1 * T_bc (:549-551).  Stereo: the right camera sees
    left_to_right^-1 * X_left with left_to_right = translate(+0.12, 0, 0); a
    fraction of the points has no right match (pixel -1).  intr = (fx, fy, cx,
    cy), the camera height and the stereo baseline default to FX..CY, 0.3 m and
    BASELINE; they draw nothing from the generator."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (FX, FY, CX, CY) if intr is None else (float(v) for v in intr)
    T_bc = np.eye(4)
    T_bc[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    T_bc[:3, 3] = [0.0, 0.0, height]
    theta_true = np.array([rng.uniform(0.05, 0.25), rng.uniform(-0.15, 0.15),
                           rng.uniform(-0.2, 0.2)])
    theta_init = theta_true + np.array([rng.uniform(-0.01, 0.01),      # odometry prior
                                        rng.uniform(-0.01, 0.01),
                                        rng.uniform(-0.003, 0.003)])
    z = rng.uniform(1.5, 12.0, n)
    Xc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.35, 0.35, n) * z,
                   z], axis=1)                        # current camera
    Xb2 = Xc @ T_bc[:3, :3].T + T_bc[:3, 3]
    Pi = _inv(planar_T(theta_true))
    X = (Xb2 @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    if pixel_sigma > 0:
        uv = uv + rng.normal(0, pixel_sigma, uv.shape)
    W_b1 = planar_T([2.0, -1.0, 0.3])
    T_wl = W_b1 @ T_bc
    T_wc_init = W_b1 @ _inv(planar_T(theta_init)) @ T_bc
    T_out_true = _inv(planar_T(theta_true)) @ T_bc
    f32 = lambda a: np.asarray(a, np.float32)
    sc = dict(X=X, uv=f32(uv), fx=fx, fy=fy, cx=cx, cy=cy, T_bc=f32(T_bc),
              T_wl=f32(T_wl), T_wc_init=f32(T_wc_init), theta_true=theta_true,
              theta_init=theta_init, T_out_true=f32(T_out_true))
    if stereo:
        T_lr = np.eye(4)
        T_lr[0, 3] = baseline
        Xr = Xc - T_lr[:3, 3]
        uvr = np.stack([fx * Xr[:, 0] / Xr[:, 2] + cx, fy * Xr[:, 1] / Xr[:, 2] + cy], 1)
        if pixel_sigma > 0:
            uvr = uvr + rng.normal(0, pixel_sigma, uvr.shape)
        miss = rng.uniform(size=n) < right_missing_frac
        uvr[miss] = -1.0
        sc.update(uv_right=f32(uvr), T_lr=f32(T_lr), right_missing=miss)
    return sc


def planar_pose_only_batch_scene(B, n_min, n_max, seed, stereo=False, pixel_sigma=0.0,
                                 right_missing_frac=0.0, outlier_frac=0.0):
    """B independent planar 3-DoF problems for the batched planar solvers
    (ba_pose_only_{mono,stereo}3_batch), concatenated: problem b owns rows
    [offsets[b], offsets[b+1]) of X / uv (/ uv_right, right_missing).  Each is a
    planar_pose_only_scene of n_min..n_max points with its own theta_true and
    theta_init (drawn by that scene), intrinsics (fx 300..600), camera height
    (0.2..0.5 m) and, in stereo, baseline (0.10..0.15 m); pixels get
    `pixel_sigma` noise and an `outlier_frac` of the points a gross error of
    20..60 px (a missing right pixel stays -1).  Per-problem arrays: intr,
    T_bc, T_wl, T_wc_init, T_out_true, theta_true, theta_init (and intr_r,
    T_lr).  Seeded."""
    rng = np.random.default_rng(seed)
    ns = rng.integers(n_min, n_max + 1, B)
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum(ns)
    keys = ("T_bc", "T_wl", "T_wc_init", "T_out_true", "theta_true", "theta_init")
    per = {k: [] for k in keys}
    Xs, uvs, uvrs, miss, intr, T_lr = [], [], [], [], [], []
    for b in range(B):
        n = int(ns[b])
        sub = int(rng.integers(1 << 30))
        fx = rng.uniform(300.0, 600.0)
        K = [fx, fx * rng.uniform(0.98, 1.02), rng.uniform(300.0, 340.0),
             rng.uniform(220.0, 260.0)]
        height = rng.uniform(0.2, 0.5)
        baseline = rng.uniform(0.10, 0.15)
        sc = planar_pose_only_scene(n, seed=sub, pixel_sigma=pixel_sigma, stereo=stereo,
                                    right_missing_frac=right_missing_frac, intr=K,
                                    height=height, baseline=baseline)
        bad = rng.uniform(size=n) < outlier_frac
        err = rng.uniform(20.0, 60.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        Xs.append(sc["X"])
        uvs.append((sc["uv"] + bad[:, None] * err).astype(np.float32))
        intr.append(K)
        for k in keys:
            per[k].append(sc[k])
        if stereo:
            uvr = (sc["uv_right"] + bad[:, None] * err[:, ::-1]).astype(np.float32)
            uvr[sc["right_missing"]] = -1.0
            uvrs.append(uvr)
            miss.append(sc["right_missing"])
            T_lr.append(sc["T_lr"])
    out = dict(B=B, offsets=offsets, n=ns.astype(np.int32), X=np.concatenate(Xs),
               uv=np.concatenate(uvs), intr=np.asarray(intr, np.float32))
    out.update({k: np.stack(v) for k, v in per.items()})
    if stereo:
        out.update(uv_right=np.concatenate(uvrs), intr_r=out["intr"].copy(),
                   T_lr=np.stack(T_lr), right_missing=np.concatenate(miss))
    return out
