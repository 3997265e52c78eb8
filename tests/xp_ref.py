"""The stages of one LM iteration of the full-BA solver, restated in numpy for any
floating dtype: numpy.longdouble (80-bit on x86) is the reference of
test_gpu_stage_rounding.py, the same functions at numpy.float64 are its yardstick.

The expressions and quirks are those of the stage functions of oracle/ba_oracle.cpp
(cited as "oracle:<function>"): the projection written as fx * (x * invz) + cx in the
linearisation and (fx * x) * invz + cx in the cost, the weight from |r0| + |r1|, the
upper triangles of A_j and C_i mirrored, B_ji ASSIGNED by the last observation of a
(pose, landmark) pair in input order, the diagonals damped by fl64(1 + lambda), an
all-zero C_i inverted to 0, the upper blocks of B Cinv B^T mirrored, the se3
exponential with its theta < 1e-7 branch, the model change with the damped blocks.
Sums over observations, poses and landmarks run one term after the other in input order, as the
oracle's loops do (numpy.add.at, numpy.cumsum); short sums inside a block are numpy's.

Every quantity is a VS: the value and its SCALE, the same expression evaluated on
magnitudes, carried through every operation:
    scale(input) = |input|,  scale(a + b) = scale(a - b) = scale(a) + scale(b),
    scale(a * b) = scale(a) * scale(b),  scale(1 / z) = scale(z) / z^2,
    scale(sqrt(q)) = sqrt(scale(q))      (q a sum of squares: the norm of the scales).
A sum of products so has the scale |B||Cinv||B^T|, a residual |projection| + |c| +
|measurement|, a composed pose |dR||R| and |dR||t| + |dt|.  u * scale is the size of
the rounding error any fp64 evaluation of the expression, in any order of its sums and
with or without fused multiply-adds, commits per operation; errors are quoted in that
unit (rounding_units) with u = 2^-53.

Each stage takes its inputs as plain arrays (what the previous stage left on the
device), so an error is charged to the stage that made it.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
LD_OK = bool(np.finfo(LD).eps <= 2e-19)
LD_REASON = "numpy.longdouble is not an extended format here (eps %.3g > 2e-19)" % float(np.finfo(LD).eps)


class VS:
    """A value and its scale (see the module docstring)."""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = v
        self.s = np.abs(v) if s is None else s

    def __add__(self, o):
        return VS(self.v + o.v, self.s + o.s)

    def __sub__(self, o):
        return VS(self.v - o.v, self.s + o.s)

    def __mul__(self, o):
        return VS(self.v * o.v, self.s * o.s)

    def __neg__(self):
        return VS(-self.v, self.s)

    def __getitem__(self, k):
        return VS(self.v[k], self.s[k])

    def sum(self, axis=None):
        return VS(self.v.sum(axis=axis), self.s.sum(axis=axis))

    def total(self):
        """Sum of all elements one after the other, in their order (the oracle's loops)."""
        if self.v.size == 0:
            return VS(self.v.dtype.type(0), self.v.dtype.type(0))
        return VS(np.cumsum(self.v.reshape(-1))[-1], np.cumsum(self.s.reshape(-1))[-1])

    def reshape(self, *shape):
        return VS(self.v.reshape(*shape), self.s.reshape(*shape))


def vs(a, dt):
    return VS(np.asarray(a, dtype=dt))


def ein(expr, *ops):
    """einsum of the values and of the scales."""
    return VS(np.einsum(expr, *[o.v for o in ops]), np.einsum(expr, *[o.s for o in ops]))


def recip(z):
    return VS(1 / z.v, z.s / (z.v * z.v))


def root(q):
    return VS(np.sqrt(q.v), np.sqrt(q.s))


def where(c, a, b):
    return VS(np.where(c, a.v, b.v), np.where(c, a.s, b.s))


def stack(parts, axis):
    return VS(np.stack([p.v for p in parts], axis), np.stack([p.s for p in parts], axis))


def scatter(x, idx, n):
    """Rows of x added up by idx into n rows (numpy's order: the input order)."""
    out = VS(np.zeros((n,) + x.v.shape[1:], x.v.dtype), np.zeros((n,) + x.v.shape[1:], x.v.dtype))
    np.add.at(out.v, idx, x.v)
    np.add.at(out.s, idx, x.s)
    return out


def rounding_units(dev, ref):
    """max |dev - ref.v| / (u ref.s) over the elements with a scale; where the scale is 0
    the expression has no term at all and dev must be exactly 0."""
    dev = np.atleast_1d(np.asarray(dev, np.float64))
    v, s = np.broadcast_to(ref.v, dev.shape), np.broadcast_to(ref.s, dev.shape)
    assert np.isfinite(dev).all()
    z = s == 0
    assert (dev[z] == 0).all(), "%d element(s) without a term are not 0" % int((dev[z] != 0).sum())
    if z.all():
        return 0.0
    return float((np.abs(dev[~z].astype(LD) - v[~z].astype(LD)) / (LD(U) * s[~z].astype(LD))).max())


# ---------------------------------------------------------------------------------------
# structure (oracle:build_structure): optimisation indices in input order, the distinct
# (landmark, pose) pairs sorted by (i, j), the last observation of every pair
# ---------------------------------------------------------------------------------------
class Structure:
    def __init__(self, pr):
        self.j_opt = np.where(pr["pose_fixed"] == 0, np.cumsum(pr["pose_fixed"] == 0) - 1, -1)
        self.i_opt = np.where(pr["pt_fixed"] == 0, np.cumsum(pr["pt_fixed"] == 0) - 1, -1)
        self.N, self.M = int((pr["pose_fixed"] == 0).sum()), int((pr["pt_fixed"] == 0).sum())
        self.pose_of_j = np.nonzero(pr["pose_fixed"] == 0)[0]
        self.pt_of_i = np.nonzero(pr["pt_fixed"] == 0)[0]
        self.oi, self.oj = self.i_opt[pr["obs_pt"]], self.j_opt[pr["obs_pose"]]
        both = np.nonzero((self.oi >= 0) & (self.oj >= 0))[0]
        key = self.oi[both].astype(np.int64) * max(self.N, 1) + self.oj[both]
        uniq, inv = np.unique(key, return_inverse=True)
        self.pair_i, self.pair_j = uniq // max(self.N, 1), uniq % max(self.N, 1)
        self.P = uniq.size
        _, first_of_reversed = np.unique(inv[::-1], return_index=True)
        self.last_obs = both[::-1][first_of_reversed]       # the pair's last writer


def pair_order(pi, pj):
    """Permutation of a (pair_i, pair_j) list into the (i, j)-sorted order of Structure."""
    return np.lexsort((pj, pi))


# ---------------------------------------------------------------------------------------
# projection and cost (oracle:project, oracle:ba_oracle_cost)
# ---------------------------------------------------------------------------------------
def project(pr, poses, points, dt, cost_form):
    oc, op, oq = pr["obs_cam"], pr["obs_pose"], pr["obs_pt"]
    T, Tc = vs(poses, dt)[op], vs(pr["cam_T"], dt)[oc]
    intr, uv = vs(pr["cam_intr"], dt)[oc], vs(pr["obs_uv"], dt)
    R, Rc = T[:, :9].reshape(-1, 3, 3), Tc[:, :9].reshape(-1, 3, 3)
    Xij = ein("nij,nj->ni", R, vs(points, dt)[oq]) + T[:, 9:]
    Xc = ein("nij,nj->ni", Rc, Xij) + Tc[:, 9:]
    invz = recip(Xc[:, 2])
    f, c = intr[:, 0:2], intr[:, 2:4]
    if cost_form:
        r = (f * Xc[:, 0:2]) * invz[:, None] + c - uv
    else:
        r = f * (Xc[:, 0:2] * invz[:, None]) + c - uv
    return R, Rc, Xij, Xc, invz, f, r


def cost(pr, poses, points, dt):
    """Sum of the unsquared residual norms at the given parameters."""
    r = project(pr, poses, points, dt, True)[-1]
    return root((r * r).sum(axis=1)).total()


# ---------------------------------------------------------------------------------------
# linearisation and damping (oracle:ba_oracle_linearize, the damping of ba_oracle_damp_invert)
# ---------------------------------------------------------------------------------------
def linearize(pr, st, huber, lam, dt):
    """dict of VS: A (N, 6, 6) and C (M, 3, 3) full and damped, a (N, 6), b (M, 3),
    B (P, 6, 3) in the pair order of `st`."""
    R, Rc, Xij, Xc, invz, f, r = project(pr, pr["pose_T"], pr["pt_X"], dt, False)
    n = r.v.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):          # (huber / 0 in the branch not taken)
        return _linearize(st, huber, lam, dt, R, Rc, Xij, Xc, invz, f, r, n)


def _linearize(st, huber, lam, dt, R, Rc, Xij, Xc, invz, f, r, n):
    finvz = f * invz[:, None]                                   # fx invz, fy invz
    f_xinvz2 = finvz * (Xc[:, 0:2] * invz[:, None])             # fx invz (x invz), ...
    absr = VS(np.abs(r.v).sum(axis=1), r.s.sum(axis=1))
    hub = vs(np.full(n, np.float64(huber)), dt)
    one = vs(np.ones(n), dt)
    w = where(absr.v > hub.v, hub * recip(absr), one)
    wr = r * w[:, None]
    # G (n, 2, 3): row m is f_m invz Rc[m, :] + (-f_m m invz^2) Rc[2, :]
    G = finvz[:, :, None] * Rc[:, 0:2, :] + (-f_xinvz2)[:, :, None] * Rc[:, 2:3, :]
    zero = vs(np.zeros(n), dt)
    Sk = stack([stack([zero, Xij[:, 2], -Xij[:, 1]], 1), stack([-Xij[:, 2], zero, Xij[:, 0]], 1),
                stack([Xij[:, 1], -Xij[:, 0], zero], 1)], 1)   # -[Xij]x
    GS = ein("nrk,nkc->nrc", G, Sk)
    Q = VS(np.concatenate([G.v, GS.v], 2), np.concatenate([G.s, GS.s], 2))   # (n, 2, 6)
    Rm = ein("nrk,nkc->nrc", G, R)                                          # (n, 2, 3)
    wQ = Q * w[:, None, None]
    Aobs = ein("nri,nrj->nij", wQ, Q)
    aobs = -ein("nrc,nr->nc", Q, wr)
    Cobs = ein("nri,nrj->nij", Rm, Rm) * w[:, None, None]
    bobs = -ein("nrc,nr->nc", Rm, wr)
    Bobs = ein("nri,nrc->nic", Q, Rm) * w[:, None, None]
    kj, ki = np.nonzero(st.oj >= 0)[0], np.nonzero(st.oi >= 0)[0]
    A, a = scatter(Aobs[kj], st.oj[kj], st.N), scatter(aobs[kj], st.oj[kj], st.N)
    C, b = scatter(Cobs[ki], st.oi[ki], st.M), scatter(bobs[ki], st.oi[ki], st.M)
    lp1 = dt(np.float64(1.0) + np.float64(lam))
    for blk, k in ((A, 6), (C, 3)):
        up = np.triu(np.ones((k, k), bool))
        for part in ("v", "s"):
            x = getattr(blk, part)
            x[...] = np.where(up, x, np.swapaxes(x, 1, 2))       # upper triangle mirrored
            x[:, np.arange(k), np.arange(k)] *= lp1
    return dict(A=A, a=a, C=C, b=b, B=Bobs[st.last_obs])


# ---------------------------------------------------------------------------------------
# the 3 x 3 inverse (oracle:ldlt3_inverse: C.ldlt().solve(I), an all-zero C gives 0)
# ---------------------------------------------------------------------------------------
def pinv3(C, dt, newton=2):
    """(inverse of every C[i] (M, 3, 3) by cofactors and `newton` steps X += X (I - C X);
    kappa_inf(C[i]), 0 for an all-zero C[i]).  In long double the inverse is exact to about
    eps_ld kappa: 2^-11 of the unit u kappa max|Cinv| the device is held to."""
    C = np.asarray(C, dtype=dt)
    zero = (C == 0).all(axis=(1, 2))
    Cs = np.where(zero[:, None, None], np.eye(3, dtype=dt), C)
    cof = np.empty_like(Cs)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            cof[:, c, r] = Cs[:, r1, c1] * Cs[:, r2, c2] - Cs[:, r1, c2] * Cs[:, r2, c1]
    det = (Cs[:, 0, :] * cof[:, :, 0]).sum(axis=1)
    if (det == 0).any():
        raise ValueError("pinv3: a singular, non-zero C_i is outside this restatement")
    X = cof / det[:, None, None]
    eye = np.eye(3, dtype=dt)
    for _ in range(newton):
        X = X + X @ (eye - Cs @ X)
    kappa = np.abs(Cs).sum(axis=2).max(axis=1) * np.abs(X).sum(axis=2).max(axis=1)
    X[zero] = 0
    return X, np.where(zero, 0, kappa)


def inverse_units(dev_Cinv, dev_Cinvb, C, b):
    """The device's Cinv_i and Cinv_i b_i against the exact inverse of C (the device's damped
    blocks), per landmark, in units of u kappa_inf(C_i) max|Cinv_i| (times max|b_i| for the
    product).  Returns (units of Cinv (M,), units of Cinv b (M,), kappa (M,)); landmarks with
    C_i = 0 must hold exact zeros and report 0."""
    X, kappa = pinv3(C, LD)
    b = np.asarray(b, LD)
    zero = kappa == 0
    assert (np.asarray(dev_Cinv)[zero] == 0).all() and (np.asarray(dev_Cinvb)[zero] == 0).all()
    unit = LD(U) * kappa * np.abs(X).max(axis=(1, 2))
    unit_b = unit * np.abs(b).max(axis=1)
    eC = np.abs(np.asarray(dev_Cinv, LD) - X).max(axis=(1, 2))
    eb = np.abs(np.asarray(dev_Cinvb, LD) - np.einsum("nij,nj->ni", X, b)).max(axis=1)
    ok, okb = unit > 0, unit_b > 0
    assert (eb[~okb] == 0).all()
    return (np.where(ok, eC / np.where(ok, unit, 1), 0).astype(float),
            np.where(okb, eb / np.where(okb, unit_b, 1), 0).astype(float), kappa.astype(float))


# ---------------------------------------------------------------------------------------
# Schur complement (oracle:ba_oracle_schur)
# ---------------------------------------------------------------------------------------
def schur(A, a, B, pair_i, pair_j, Cinv, b, dt):
    """(S (6N, 6N) VS, rhs (6N,) VS, n_terms (6N, 6N), n_terms_rhs (6N,)) from the damped A,
    a, B in (i, j)-sorted pair order, Cinv and b.  n_terms counts the landmarks that
    contribute to an element."""
    A, a, B, Cinv, b = (vs(x, dt) for x in (A, a, B, Cinv, b))
    N, M = A.v.shape[0], Cinv.v.shape[0]
    n6 = 6 * N
    acc = VS(np.zeros((n6, n6), dt), np.zeros((n6, n6), dt))
    accb = VS(np.zeros(n6, dt), np.zeros(n6, dt))
    cnt, cntb = np.zeros((N, N), np.int64), np.zeros(N, np.int64)
    ptr = np.searchsorted(pair_i, np.arange(M + 1))
    six = np.arange(6)
    for i in range(M):
        p0, p1 = ptr[i], ptr[i + 1]
        if p0 == p1:
            continue
        js = pair_j[p0:p1]
        idx = (6 * js[:, None] + six).ravel()
        Bi = B[p0:p1]
        V = ein("pkc,cd->pkd", Bi, Cinv[i])                      # B_ji Cinv_i
        Vf, Bf = V.reshape(-1, 3), Bi.reshape(-1, 3)
        ix = np.ix_(idx, idx)
        acc.v[ix] += Vf.v @ Bf.v.T
        acc.s[ix] += Vf.s @ Bf.s.T
        accb.v[idx] += Vf.v @ b.v[i]
        accb.s[idx] += Vf.s @ b.s[i]
        cnt[np.ix_(js, js)] += 1
        cntb[js] += 1
    upper = (np.arange(n6)[:, None] // 6) <= (np.arange(n6)[None, :] // 6)    # blocks k >= j, mirrored
    S = VS(np.zeros((n6, n6), dt), np.zeros((n6, n6), dt))
    for j in range(N):
        S.v[6 * j:6 * j + 6, 6 * j:6 * j + 6] = A.v[j]
        S.s[6 * j:6 * j + 6, 6 * j:6 * j + 6] = A.s[j]
    S = S - VS(np.where(upper, acc.v, acc.v.T), np.where(upper, acc.s, acc.s.T))
    rhs = a.reshape(-1) - accb
    return S, rhs, np.kron(cnt, np.ones((6, 6), np.int64)), np.repeat(cntb, 6)


def backward_error(S, rhs, x):
    """Normwise backward error |rhs - S x|_inf / (|S|_inf |x|_inf + |rhs|_inf), in long double."""
    S, rhs, x = np.asarray(S, LD), np.asarray(rhs, LD).reshape(-1), np.asarray(x, LD).reshape(-1)
    den = np.abs(S).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()
    return float(np.abs(rhs - S @ x).max() / den)


def equilibrated(S, rhs, x):
    """(D^-1 S D^-1, D^-1 rhs, D x) with D = sqrt(diag S) rounded to powers of two (so that the
    scaling is exact): the system a Cholesky factorisation is really judged on when the rows of S
    span decades, where the normwise backward error sees the largest rows only."""
    d = 2.0 ** np.round(0.5 * np.log2(np.diag(S)))
    return S / np.outer(d, d), np.asarray(rhs).reshape(-1) / d, np.asarray(x).reshape(-1) * d


# ---------------------------------------------------------------------------------------
# back substitution, quadratic model, step norms (oracle:ba_oracle_backsub, _model_change,
# _step_norms)
# ---------------------------------------------------------------------------------------
def _Btx(B, pair_i, pair_j, x, M):
    """sum_j B_ji^T x_j per landmark (M, 3)."""
    return scatter(ein("pkc,pk->pc", B, x[pair_j]), pair_i, M)


def backsub(Cinv, b, B, pair_i, pair_j, x, dt):
    """y_i = Cinv_i b_i - Cinv_i sum_j B_ji^T x_j."""
    Cinv, b, B, x = (vs(v, dt) for v in (Cinv, b, B, x))
    t = _Btx(B, pair_i, pair_j, x, Cinv.v.shape[0])
    return ein("nij,nj->ni", Cinv, b) - ein("nij,nj->ni", Cinv, t)


def model_change(A, a, C, b, B, pair_i, pair_j, x, y, dt):
    """-(a.x + x^T A x + b.y + y^T C y + 2 y.(B^T x)) with the damped A and C."""
    A, a, C, b, B, x, y = (vs(v, dt) for v in (A, a, C, b, B, x, y))
    two = vs(2.0, dt)
    per_pose = stack([(a * x).sum(axis=1), ein("nr,nrc,nc->n", x, A, x)], 1)
    per_point = stack([(b * y).sum(axis=1), ein("nr,nrc,nc->n", y, C, y),
                       (y * _Btx(B, pair_i, pair_j, x, C.v.shape[0])).sum(axis=1) * two], 1)
    return -(per_pose.total() + per_point.total())


def step_norms(x, y, dt):
    """(sum of |x_j|, sum of |y_i|)."""
    x, y = vs(x, dt), vs(y, dt)
    return root((x * x).sum(axis=1)).total(), root((y * y).sum(axis=1)).total()


# ---------------------------------------------------------------------------------------
# parameter update (oracle:se3_exp, rigid_compose, ba_oracle_update)
# ---------------------------------------------------------------------------------------
def se3_exp(x, dt):
    """(dR (N, 3, 3), dt (N, 3)) of x = (v, w) per row."""
    x = vs(x, dt)
    n = x.v.shape[0]
    v, w = x[:, 0:3], x[:, 3:6]
    th = root((w * w).sum(axis=1))
    zero = vs(np.zeros(n), dt)
    wx = stack([stack([zero, -w[:, 2], w[:, 1]], 1), stack([w[:, 2], zero, -w[:, 0]], 1),
                stack([-w[:, 1], w[:, 0], zero], 1)], 1)
    wx2 = ein("nrk,nkc->nrc", wx, wx)
    small = th.v < dt(1e-7)
    ths = VS(np.where(small, dt(1), th.v), np.where(small, dt(1), th.s))   # (no 0 / 0 in the unused branch)
    sn, cs = VS(np.sin(ths.v), np.abs(np.sin(ths.v))), VS(np.cos(ths.v), np.abs(np.cos(ths.v)))
    one = vs(np.ones(n), dt)
    rt = recip(ths)
    const = lambda c: vs(np.full(n, c), dt)
    ca = where(small, one, sn * rt)
    cb = where(small, const(0.5), (one - cs) * (rt * rt))
    vb = where(small, const(np.float64(0.33333333333333333333333333)), (ths - sn) * (rt * rt * rt))
    eye = VS(np.broadcast_to(np.eye(3, dtype=dt), (n, 3, 3)))
    dR = eye + wx * ca[:, None, None] + wx2 * cb[:, None, None]
    V = eye + wx * cb[:, None, None] + wx2 * vb[:, None, None]
    return dR, ein("nij,nj->ni", V, v)


def update(pr, st, x, y, dt):
    """(poses (n_pose, 12) VS, points (n_pt, 3) VS) after T_j <- exp(x_j) T_j, X_i <- X_i + y_i;
    fixed poses and points keep their value (and their scale |value|)."""
    dR, dtr = se3_exp(x, dt)
    T = vs(pr["pose_T"], dt)
    To = T[st.pose_of_j]
    Rn = ein("nij,njk->nik", dR, To[:, :9].reshape(-1, 3, 3))
    tn = ein("nij,nj->ni", dR, To[:, 9:]) + dtr
    new = VS(np.concatenate([Rn.v.reshape(-1, 9), tn.v], 1), np.concatenate([Rn.s.reshape(-1, 9), tn.s], 1))
    poses = VS(T.v.copy(), T.s.copy())
    poses.v[st.pose_of_j], poses.s[st.pose_of_j] = new.v, new.s
    X = vs(pr["pt_X"], dt)
    Xn = X[st.pt_of_i] + vs(y, dt)
    points = VS(X.v.copy(), X.s.copy())
    points.v[st.pt_of_i], points.s[st.pt_of_i] = Xn.v, Xn.s
    return poses, points


# ---------------------------------------------------------------------------------------
# one pass through the stages, every stage judged from what the previous one produced
# ---------------------------------------------------------------------------------------
# e <= 8 max(e64, 1); Cinv within 8 u kappa max|Cinv|.  Three bits of margin keep an fp32 intermediate
# (1e6 units and more) far outside, but they are a LIMIT of these tests as well: rcp_newton with one
# Newton step instead of two raises Cinv from 0.35 to 2.9 of the 8 units on case A (v_rcp_f64 is good
# to about 2^-26 on the MI355X, one step already reaches 2^-52) and passes.
BOUND_FACTOR = 8.0
SUM_CAP = 8             # S, rhs: e <= n_terms + 8 as well
KAPPA_SPLIT = 1e6       # Cinv is asserted apart for kappa <= 1e6 and above


def units_array(dev, ref):
    """rounding_units per element (0 where the scale is 0, after the same equality check)."""
    dev = np.asarray(dev, np.float64)
    z = ref.s == 0
    assert np.isfinite(dev).all() and (dev[z] == 0).all()
    return (np.abs(dev.astype(LD) - ref.v) / (LD(U) * np.where(z, 1, ref.s))).astype(np.float64) * ~z


def within(e, e64):
    return e <= BOUND_FACTOR * max(e64, 1.0)


def lapack_solve(S, rhs):
    from scipy.linalg import cho_factor, cho_solve
    return cho_solve(cho_factor(np.asarray(S, np.float64), lower=True), np.asarray(rhs).reshape(-1))


def lapack_backward_error(S, rhs):
    """backward_error of scipy.linalg.cho_solve on the same system."""
    return backward_error(S, rhs, lapack_solve(S, rhs))


def measure_stages(pr, st, lam, huber, D):
    """The figures of one pass: D holds what an implementation (the device, or the CPU oracle)
    produced: A a C b (damped), pairs = (pair_i, pair_j, B), Cinv Cinvb, S rhs, x y, model sp sq
    cost (the trial cost), poses points (after the step is committed).  Returns an ordered
    dict: stage -> (e, e64) in rounding units, and
      "S cap", "rhs cap": (max over elements of e - n_terms, SUM_CAP),
      "Cinv", "Cinvb": (e for kappa <= KAPPA_SPLIT, e above it), in units of u kappa max|Cinv|,
      "... of the yardstick": the same caps and inverse bounds for xp_ref's own float64 run,
      "x": (eta, eta of LAPACK), "kappa": (landmarks above KAPPA_SPLIT, landmarks with C = 0).
    Nothing is asserted here but exact zeros where an expression has no term."""
    import collections
    out = collections.OrderedDict()
    f64 = np.float64
    perm = pair_order(D["pairs"][0], D["pairs"][1])
    pi, pj, B = D["pairs"][0][perm], D["pairs"][1][perm], D["pairs"][2][perm]
    assert np.array_equal(pi, st.pair_i) and np.array_equal(pj, st.pair_j)
    ref, yard = linearize(pr, st, huber, lam, LD), linearize(pr, st, huber, lam, f64)
    for k, dev in (("A", D["A"]), ("a", D["a"]), ("C", D["C"]), ("b", D["b"]), ("B", B)):
        out[k] = (rounding_units(dev, ref[k]), rounding_units(yard[k].v, ref[k]))
    eC, eb, kappa = inverse_units(D["Cinv"], D["Cinvb"], D["C"], D["b"])
    lo, hi = (kappa <= KAPPA_SPLIT), (kappa > KAPPA_SPLIT)
    mx = lambda e, m: float(e[m].max()) if m.any() else 0.0
    out["Cinv"], out["Cinvb"] = (mx(eC, lo), mx(eC, hi)), (mx(eb, lo), mx(eb, hi))
    out["kappa"] = (int(hi.sum()), int((kappa == 0).sum()))
    X64 = pinv3(D["C"], f64)[0]
    yC, yb = inverse_units(X64, np.einsum("nij,nj->ni", X64, D["b"]), D["C"], D["b"])[:2]
    out["Cinv of the yardstick"], out["Cinvb of the yardstick"] = (mx(yC, lo), mx(yC, hi)), (mx(yb, lo), mx(yb, hi))
    args = (D["A"], D["a"], B, pi, pj, D["Cinv"], D["b"])
    S, rhs, nS, nr = schur(*args, LD)
    S64, rhs64 = schur(*args, f64)[:2]
    for k, dev, r, y64, nt in (("S", D["S"], S, S64, nS), ("rhs", D["rhs"], rhs, rhs64, nr)):
        e = units_array(dev, r)
        out[k] = (float(e.max()), rounding_units(y64.v, r))
        out[k + " cap"] = (float((e - nt).max()), float(SUM_CAP))
        out[k + " cap of the yardstick"] = (float((units_array(y64.v, r) - nt).max()), float(SUM_CAP))
    out["x"] = (backward_error(D["S"], D["rhs"], D["x"]), lapack_backward_error(D["S"], D["rhs"]))
    args = (D["Cinv"], D["b"], B, pi, pj, D["x"])
    r = backsub(*args, LD)
    out["y"] = (rounding_units(D["y"], r), rounding_units(backsub(*args, f64).v, r))
    args = (D["A"], D["a"], D["C"], D["b"], B, pi, pj, D["x"], D["y"])
    r = model_change(*args, LD)
    out["model"] = (rounding_units(D["model"], r), rounding_units(model_change(*args, f64).v, r))
    rp, rq = step_norms(D["x"], D["y"], LD)
    yp, yq = step_norms(D["x"], D["y"], f64)
    out["step poses"] = (rounding_units(D["sp"], rp), rounding_units(yp.v, rp))
    out["step points"] = (rounding_units(D["sq"], rq), rounding_units(yq.v, rq))
    rP, rX = update(pr, st, D["x"], D["y"], LD)
    yP, yX = update(pr, st, D["x"], D["y"], f64)
    out["poses"] = (rounding_units(D["poses"], rP), rounding_units(yP.v, rP))
    out["points"] = (rounding_units(D["points"], rX), rounding_units(yX.v, rX))
    r = cost(pr, D["poses"], D["points"], LD)
    out["cost"] = (rounding_units(D["cost"], r), rounding_units(cost(pr, D["poses"], D["points"], f64).v, r))
    return out


YARDSTICK_STAGES = ("A", "a", "C", "b", "B", "S", "rhs", "y", "model", "step poses", "step points", "poses",
                    "points", "cost")


def failures(fig, eta_factor=4.0):
    """The bounds a set of figures misses, as a list of strings (empty: all hold)."""
    bad = []
    for k in YARDSTICK_STAGES:
        if not within(*fig[k]):
            bad.append("%s: e = %.3g > 8 max(e64 = %.3g, 1)" % ((k,) + fig[k]))
    for k in ("S cap", "rhs cap", "S cap of the yardstick", "rhs cap of the yardstick"):
        if fig[k][0] > fig[k][1]:
            bad.append("%s: e - n_terms = %.3g > %g" % ((k,) + fig[k]))
    for k in ("Cinv", "Cinvb", "Cinv of the yardstick", "Cinvb of the yardstick"):
        for which, e in zip(("kappa <= 1e6", "kappa > 1e6"), fig[k]):
            if e > BOUND_FACTOR:
                bad.append("%s (%s): %.3g > 8 u kappa max|Cinv|" % (k, which, e))
    eta, eta_lapack = fig["x"]
    if eta > eta_factor * max(eta_lapack, U):
        bad.append("x: eta = %.3g u > 4 max(eta_LAPACK = %.3g u, u)" % (eta / U, eta_lapack / U))
    return bad


def report(tag, fig):
    """One printed line per stage."""
    for k, v in fig.items():
        if k == "x":
            print("ROUNDING %s x: eta %.3f u, LAPACK %.3f u" % (tag, v[0] / U, v[1] / U))
        elif k == "kappa":
            print("ROUNDING %s landmarks with kappa > 1e6: %d, with C = 0: %d" % ((tag,) + v))
        elif k.startswith("Cinv"):
            print("ROUNDING %s %s: %.3f (kappa <= 1e6) %.3f (kappa > 1e6) of u kappa max|Cinv|" % ((tag, k) + v))
        elif " cap" in k:
            print("ROUNDING %s %s: max(e - n_terms) %.3f (<= %g)" % ((tag, k) + v))
        else:
            print("ROUNDING %s %s: e %.3f, e64 %.3f" % ((tag, k) + v))


# ---------------------------------------------------------------------------------------
# the passes of test_xp_ref.py (CPU oracle) and test_gpu_stage_rounding.py (device)
# ---------------------------------------------------------------------------------------
LAMBDA, LAMBDA_FLOOR = 1e-3, 1e-10
SPLIT_SCENES = ("A", "B", "C", "H", "W", "T", "G", "R")
FLOOR_SCENES = ("B", "H", "R")          # also at the damping floor: an ill-conditioned S
SMALL = "small"                         # noise-free: every pose step takes se3_exp's small-angle branch
HUBER = {"C": 0.005}                    # every other scene: 1.0


def scene_problem(name):
    import split_cases as sc
    if name != SMALL:
        return sc.problem(name)
    return _small_step_problem()


_small = []


def _small_step_problem():
    if not _small:
        from bundle_adjustment_solver_amd import scenes
        pr = scenes.scaled_problem(scenes.synthetic_ba_scene(12, 300, 5, True, seed=7, pixel_sigma=0, pose_noise=0,
                                                             point_noise=1e-9))
        for v in pr.values():
            v.setflags(write=False)
        _small.append(pr)
    return _small[0]


def passes():
    """Every (scene, lambda) both test files run."""
    return ([(s, LAMBDA) for s in SPLIT_SCENES + (SMALL,)] + [(s, LAMBDA_FLOOR) for s in FLOOR_SCENES])


def huber_of(name):
    return HUBER.get(name, 1.0)


# ---------------------------------------------------------------------------------------
# the batched path (test_batch_rounding_ref.py, test_gpu_batch_rounding.py): it has no stage
# getters, so it is judged on what it returns: the step of a one-iteration solve must solve
# the full damped normal equations, the output of a marginalisation that eliminates nothing
# is the reduced camera system.  The bounds are those above (BOUND_FACTOR, SUM_CAP) and so is their
# LIMIT: with one Newton step taken out of rcp_newton every batched test still passes (largest rises
# on the MI355X: landmark rows of M257 at lambda 1e-3 from 8.0 to 11.9 units, bound 56; S of N5 from
# 1.2 to 3.0, bound 43).  An intermediate of the landmark pass through float (S at 1e6 .. 5e7 units)
# and a wave-sum term of the pose pass dropped for lane 63 (pose rows at 4e6 units and more, wherever
# a pose has 64 observations) are far outside.
# ---------------------------------------------------------------------------------------
def se3_log(dR, dt):
    """(v (n, 3), w (n, 3)) in long double with se3_exp((v, w)) = (dR (n, 3, 3), dt (n, 3)).
    theta = atan2(|vee(dR - dR^T)| / 2, (tr dR - 1) / 2), w = theta / (2 sin theta) vee(dR - dR^T),
    v = (I - wx / 2 + k wx^2) dt, k = (1 - (theta / 2) cot(theta / 2)) / theta^2; below
    theta = 1e-6 the series theta / (2 sin theta) = (1 + theta^2 / 6) / 2, k = 1 / 12 + theta^2 / 720
    (their next terms are below 1e-25 there).  Below 1e-7 it inverts what se3_exp's small-angle
    branch really applies, dR = I + wx + wx^2 / 2 and V = I + wx / 2 + fl64(1 / 3) wx^2 (the
    reference's coefficient; the limit of the closed form is 1 / 6): w = vee(dR - dR^T) / 2 and
    k = 1 / 4 - fl64(1 / 3), next term theta^3 |dt|."""
    dR, dt = np.asarray(dR, LD), np.asarray(dt, LD)
    a = np.stack([dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]], 1)
    sn = np.sqrt((a * a).sum(axis=1)) / 2
    cs = (dR[:, 0, 0] + dR[:, 1, 1] + dR[:, 2, 2] - 1) / 2
    th = np.arctan2(sn, cs)
    small = th < LD(1e-6)
    ths = np.where(small, LD(1), th)
    sns = np.where(small, LD(1), sn)
    hf = ths / 2
    f = np.where(small, (1 + th * th / 6) / 2, ths / (2 * sns))
    k = np.where(small, LD(1) / 12 + th * th / 720, (1 - hf * np.cos(hf) / np.sin(hf)) / (ths * ths))
    tiny = th < LD(1e-7)
    f = np.where(tiny, LD(1) / 2, f)
    k = np.where(tiny, LD(1) / 4 - LD(np.float64(0.33333333333333333333333333)), k)
    w = a * f[:, None]
    c = np.cross(w, dt)
    e = np.cross(w, c)
    return dt - c / 2 + e * k[:, None], w


def recover_step(pr, st, poses, points):
    """(x (N, 6), y (M, 3)) in long double: the step that takes the problem's own parameters to
    `poses`, `points`: x_j = se3_log(T'_j T_j^-1) (T_j^-1 the inverse of the stored matrix, which
    is orthogonal to rounding only), y_i = X'_i - X_i."""
    T0 = np.asarray(pr["pose_T"], LD)[st.pose_of_j]
    T1 = np.asarray(poses, LD)[st.pose_of_j]
    R0i = pinv3(T0[:, :9].reshape(-1, 3, 3), LD, newton=3)[0]
    dR = T1[:, :9].reshape(-1, 3, 3) @ R0i
    dt = T1[:, 9:] - np.einsum("nij,nj->ni", dR, T0[:, 9:])
    v, w = se3_log(dR, dt)
    y = np.asarray(points, LD)[st.pt_of_i] - np.asarray(pr["pt_X"], LD)[st.pt_of_i]
    return np.concatenate([v, w], 1), y


def _units_max(res):
    z = res.s == 0
    if z.all():
        return 0.0
    return float((np.abs(res.v[~z]) / (LD(U) * res.s[~z])).max())


def full_system_units(pr, st, lam, huber, poses, points, lin=None):
    """(pose rows, landmark rows): how well the step from the problem's parameters to `poses`,
    `points` solves the damped normal equations of the problem, linearised in long double at its
    own parameters: max |a_j - A_j x_j - sum_i B_ji y_i| / (u (|a| + |A||x| + |B||y|)) and
    max |b_i - sum_j B_ji^T x_j - C_i y_i| / (u (|b| + |B^T||x| + |C||y|)), A and C damped by
    fl64(1 + lam), the magnitudes carried by VS.  A row whose scale is 0 (a landmark nobody
    observes, C_i = 0) has no equation: its parameters must be bit-equal to the input, as those
    of fixed poses and fixed points must.  `lin`: linearize(pr, st, huber, lam, LD), if at hand."""
    poses, points = np.asarray(poses, np.float64), np.asarray(points, np.float64)
    assert np.isfinite(poses).all() and np.isfinite(points).all()
    fp, fq = pr["pose_fixed"] != 0, pr["pt_fixed"] != 0
    assert np.array_equal(poses[fp], pr["pose_T"][fp]) and np.array_equal(points[fq], pr["pt_X"][fq])
    lin = linearize(pr, st, huber, lam, LD) if lin is None else lin
    xv, yv = recover_step(pr, st, poses, points)
    x, y, B = VS(xv), VS(yv), lin["B"]
    By = scatter(ein("pkc,pc->pk", B, y[st.pair_i]), st.pair_j, st.N)
    rp = lin["a"] - ein("nrc,nc->nr", lin["A"], x) - By
    rl = lin["b"] - _Btx(B, st.pair_i, st.pair_j, x, st.M) - ein("nrc,nc->nr", lin["C"], y)
    for res, idx, new, old in ((rp, st.pose_of_j, poses, pr["pose_T"]), (rl, st.pt_of_i, points, pr["pt_X"])):
        none = (res.s == 0).all(axis=1)
        assert np.array_equal(new[idx[none]], old[idx[none]]), "a parameter block without an equation moved"
    return _units_max(rp), _units_max(rl)


def yardstick_step(pr, st, lam, huber):
    """(poses, points) after one step of xp_ref's own float64 chain: linearize -> pinv3 -> schur
    -> LAPACK -> backsub -> update."""
    f64 = np.float64
    lin = linearize(pr, st, huber, lam, f64)
    Cinv = pinv3(lin["C"].v, f64)[0]
    S, rhs = schur(lin["A"].v, lin["a"].v, lin["B"].v, st.pair_i, st.pair_j, Cinv, lin["b"].v, f64)[:2]
    x = lapack_solve(S.v, rhs.v).reshape(-1, 6)
    y = backsub(Cinv, lin["b"].v, lin["B"].v, st.pair_i, st.pair_j, x, f64).v
    P, Xn = update(pr, st, x, y, f64)
    return P.v, Xn.v


def only_landmarks(pr, landmarks):
    """The problem with the observations of the points in the boolean mask `landmarks` only."""
    keep = np.asarray(landmarks, bool)[pr["obs_pt"]]
    out = dict(pr)
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        out[k] = np.ascontiguousarray(np.asarray(pr[k])[keep])
    return out


def reduced_system(pr, st, huber, dt, landmarks):
    """(S (6N, 6N) VS, rhs (6N,) VS, n_terms, n_terms_rhs) of the reduced camera system at lambda 0
    over the observations of the landmarks in the boolean mask `landmarks` (one flag per point:
    the set L ba_batch_marginalize reports; observations of fixed points, which are never in L, are
    left out, as its header says): linearize -> pinv3 -> schur, all in `dt`.  The scale of an
    element of S is |A| + |B||Cinv||B^T| of the values of that chain.  That of rhs is
    s(a) + |B||Cinv| s(b) with the scales s(a), s(b) the linearisation carries: a and b are sums of
    J^T w r, and r = projection + c - measurement cancels (to 1e-9 of its terms on the small-step
    scene), so |a| and |b| are no measure of the rounding error any evaluation of them commits; A, B
    and C hold no residual."""
    assert not (np.asarray(landmarks, bool) & (pr["pt_fixed"] != 0)).any()
    sub = only_landmarks(pr, landmarks)
    ss = Structure(sub)
    assert (ss.N, ss.M) == (st.N, st.M)
    lin = linearize(sub, ss, huber, 0.0, dt)
    Cinv = pinv3(lin["C"].v, dt)[0]
    args = (lin["B"].v, ss.pair_i, ss.pair_j, Cinv)
    S, rhs, nS, nr = schur(lin["A"].v, lin["a"].v, *args, lin["b"].v, dt)
    rhs_scale = schur(lin["A"].v, lin["a"].s, *args, lin["b"].s, dt)[1].s
    return S, VS(rhs.v, rhs_scale), nS, nr


def reduced_reference(pr, st, huber, landmarks):
    """reduced_system in long double and in float64 (its yardstick), for reduced_figures."""
    return reduced_system(pr, st, huber, LD, landmarks) + reduced_system(pr, st, huber, np.float64, landmarks)[:2]


def reduced_figures(H, bvec, ref):
    """The lower triangle of H and bvec against `ref` = reduced_reference(...): dict of
    "S", "rhs": (e, e64) in rounding units, "S cap", "rhs cap": (max(e - n_terms), SUM_CAP);
    elements without a term must be exactly 0 (units_array)."""
    S, rhs, nS, nr, S64, rhs64 = ref
    low = np.tril(np.ones(S.v.shape, bool))
    out = {}
    for k, dev, r, y64, nt in (("S", np.asarray(H)[low], S[low], S64.v[low], nS[low]),
                               ("rhs", np.asarray(bvec), rhs, rhs64.v, nr)):
        e = units_array(dev, r)
        out[k] = (float(e.max()), rounding_units(y64, r))
        out[k + " cap"] = (float((e - nt).max()), float(SUM_CAP))
    return out


def reduced_failures(fig):
    bad = []
    for k in ("S", "rhs"):
        if not within(*fig[k]):
            bad.append("%s: e = %.3g > 8 max(e64 = %.3g, 1)" % ((k,) + fig[k]))
        if fig[k + " cap"][0] > fig[k + " cap"][1]:
            bad.append("%s: e - n_terms = %.3g > %g" % ((k,) + fig[k + " cap"]))
    return bad
