"""CPU restatement (numpy float64) of the 6-DoF pose-only Gauss-Newton loop of
k_pose_only6 (csrc/ba_pose_only.hip), monocular and stereo; the same loop is
stated in fp32 by oracle/ba_oracle.cpp (pose_only_core).

Test infrastructure only: the product path never imports it.  It takes the
float32 inputs the kernel gets, widens them exactly and computes everything in
float64, vectorised over the points, so it is a higher-precision reference of
ONE linearisation, ONE solve and ONE update (and of a few of them in a row),
not a second fp32 opinion.  Kept as the kernel has them:

* pose = inverse of the given T12 (R^T, -R^T t); the output is its inverse;
* the two Jacobian rows per edge;
* the L1 Huber weight thr / (|ru| + |rv|) where |ru| + |rv| >= thr;
* the cost quirk: a Huber edge adds w * ru * ru, any other edge rv * rv;
* the outlier flag on |ru| + |rv| >= thr_out, sticky false (the input mask is
  never read, only cleared);
* stereo: the right camera sees X_r = left_to_right^-1 * X_l, its edge exists
  only where neither right coordinate is negative, and the cost is normalised
  by (n + count_right) * 0.5; mono by 2 n;
* the diagonal scaled by 1 + 1e-5, the solve, the se3 exponential, the left
  composition."""
import numpy as np

D = np.float64


def _w(a):
    """float32 input -> float64, exactly."""
    return np.asarray(a, np.float32).astype(D)


def inv12(T12):
    """(R, t) of the inverse of the rigid transform T12 = R (9, row-major), t (3)."""
    T12 = _w(T12).reshape(12)
    R = T12[:9].reshape(3, 3).T.copy()
    return R, -(R @ T12[9:])


def to12(R, t):
    """T12 of the inverse of (R, t)."""
    Rt = R.T
    return np.concatenate([Rt.reshape(9), -(Rt @ t)])


def project(L, K):
    iz = 1.0 / L[:, 2]
    return np.stack([K[0] * (L[:, 0] * iz) + K[2], K[1] * (L[:, 1] * iz) + K[3]], 1)


def edge_terms(L, uv, K, thr_huber):
    """One camera's terms for the points L (in that camera): H (6, 6), g (6) =
    -J^T W r, the per-edge cost terms and the per-edge |ru| + |rv|."""
    fx, fy = K[0], K[1]
    iz = 1.0 / L[:, 2]
    xiz, yiz = L[:, 0] * iz, L[:, 1] * iz
    r = project(L, K) - uv
    ru, rv = r[:, 0], r[:, 1]
    z = np.zeros_like(iz)
    Ju = np.stack([fx * iz, z, -fx * xiz * iz, -fx * xiz * yiz, fx * (1.0 + xiz * xiz),
                   -fx * yiz], 1)
    Jv = np.stack([z, fy * iz, -fy * yiz * iz, -fy * (1.0 + yiz * yiz), fy * yiz * xiz,
                   fy * xiz], 1)
    ars = np.abs(ru) + np.abs(rv)
    hub = ars >= thr_huber
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(hub, thr_huber / ars, 1.0)
    H = (w[:, None] * Ju).T @ Ju + (w[:, None] * Jv).T @ Jv
    g = -(Ju.T @ (w * ru) + Jv.T @ (w * rv))
    err = np.where(hub, w * ru * ru, rv * rv)
    return H, g, err, ars


def se3_exp(d):
    """(dR, dt) of the twist d = (v, w)."""
    v, w = d[:3], d[3:]
    theta = np.sqrt(w @ w)
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], D)
    wx2 = wx @ wx
    if theta < 1e-7:
        ca, cb, va, vb = 1.0, 0.5, 0.5, 1.0 / 3.0
    else:
        st, ct = np.sin(theta), np.cos(theta)
        ca = st / theta
        cb = (1.0 - ct) / (theta * theta)
        va = cb
        vb = (theta - st) / (theta ** 3)
    I = np.eye(3)
    return I + ca * wx + cb * wx2, (I + va * wx + vb * wx2) @ v


def solve(X, uv, fx, fy, cx, cy, T12, mask, max_iter=1, thr_step=0.0, thr_cost=0.0,
          huber=1.0, outlier=2.5, uv_right=None, intr_r=None, T_lr12=None, mask_r=None):
    """k_pose_only6<STEREO = uv_right is not None> in float64.  Returns the dict
    the GPU path returns (T12, n_iter, converged, success, rows = (cost,
    cost_change, abs_step) per logged iteration, debug, mask or mask_l / mask_r)
    plus "edges": the first iteration's per-edge |ru| + |rv| and cost terms
    (ars_l, err_l, and for the points with a right match has_r, ars_r, err_r)
    and "cond", the condition number of its damped H."""
    stereo = uv_right is not None
    X = _w(X).reshape(-1, 3)
    uv = _w(uv).reshape(-1, 2)
    n = X.shape[0]
    K = _w([fx, fy, cx, cy])
    huber, outlier, thr_step, thr_cost = (float(np.float32(v)) for v in
                                          (huber, outlier, thr_step, thr_cost))
    mask = np.asarray(mask, bool).copy()
    R, t = inv12(T12)
    if stereo:
        uvr = _w(uv_right).reshape(-1, 2)
        Kr = _w(intr_r).reshape(4)
        Rrl, trl = inv12(T_lr12)
        mask_r = np.asarray(mask_r, bool).copy()
        has_r = ~((uvr[:, 0] < 0) | (uvr[:, 1] < 0))
        idx_r = np.nonzero(has_r)[0]
    err_prev = float(np.float32(1e10))
    converged, rows, debug = True, [], []
    edges = cond = None
    n_iter = 0
    for it in range(max_iter):
        L = X @ R.T + t
        H, g, err, ars = edge_terms(L, uv, K, huber)
        mask[ars >= outlier] = False
        cost = err.sum()
        if stereo:
            Lr = L[has_r] @ Rrl.T + trl
            Hr, gr, er, arr = edge_terms(Lr, uvr[has_r], Kr, huber)
            mask_r[idx_r[arr >= outlier]] = False
            H, g, cost = H + Hr, g + gr, cost + er.sum()
        if edges is None:
            edges = dict(ars_l=ars, err_l=err)
            if stereo:
                edges.update(has_r=has_r, ars_r=arr, err_r=er)
        H = H.copy()
        H[np.diag_indices(6)] *= 1.0 + 1e-5
        if cond is None:
            cond = float(np.linalg.cond(H))
        d = np.linalg.solve(H, g)
        dR, dt = se3_exp(d)
        R, t = dR @ R, dR @ t + dt
        debug.append(to12(R, t))
        cost = cost / ((n + idx_r.size) * 0.5) if stereo else cost * (1.0 / n * 0.5)
        change = abs(cost - err_prev)
        step = float(np.sqrt(d @ d))
        n_iter = it + 1
        if step < thr_step or change < thr_cost:
            converged = True
            break
        if it == max_iter - 1:
            converged = False
        rows.append((float(cost), float(change), step))
        err_prev = cost
    success = bool(np.isfinite(R).all())
    out = dict(T12=to12(R, t) if success and n_iter else _w(T12).reshape(12), n_iter=n_iter,
               converged=converged, success=success, rows=rows,
               debug=np.array(debug, D).reshape(-1, 12), edges=edges, cond=cond)
    if stereo:
        out.update(mask_l=mask, mask_r=mask_r)
    else:
        out.update(mask=mask)
    return out
