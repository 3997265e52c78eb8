"""Host references for the covariance tests (numpy / scipy fp64, no GPU).

full_normal_matrix: H = [[A, W], [W^T, C]] from the stage readers of a problem object
(BaProblem on the GPU, oracle_py.Oracle on the CPU: the same three calls).
blocks_two_ways: the pose and point diagonal blocks of H^-1 once by numpy.linalg.inv
and once by scipy's Cholesky on identity columns, and the largest relative block
difference between the two — the reference's own noise.
"""
import numpy as np
import scipy.linalg


def full_normal_matrix(A, Cm, pair_i, pair_j, W):
    N, M = A.shape[0], Cm.shape[0]
    n = 6 * N + 3 * M
    H = np.zeros((n, n))
    for j in range(N):
        H[6 * j:6 * j + 6, 6 * j:6 * j + 6] = A[j]
    for i in range(M):
        o = 6 * N + 3 * i
        H[o:o + 3, o:o + 3] = Cm[i]
    for i, j, w in zip(pair_i, pair_j, W):
        o = 6 * N + 3 * int(i)
        H[6 * j:6 * j + 6, o:o + 3] = w
        H[o:o + 3, 6 * j:6 * j + 6] = w.T
    return H


def diag_blocks(Hi, N, M):
    cp = np.stack([Hi[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(N)]) if N else np.zeros((0, 6, 6))
    o = 6 * N
    cq = np.stack([Hi[o + 3 * i:o + 3 * i + 3, o + 3 * i:o + 3 * i + 3] for i in range(M)]) \
        if M else np.zeros((0, 3, 3))
    return cp, cq


def rel_block_diff(a, b):
    """Largest over the blocks of max|a - b| / max|b| (0 for a pair of zero blocks)."""
    worst = 0.0
    for x, y in zip(a, b):
        s = np.abs(y).max()
        d = np.abs(x - y).max()
        worst = max(worst, d / s if s > 0 else (0.0 if d == 0 else np.inf))
    return worst


def blocks_two_ways(H, N, M):
    """(pose blocks, point blocks) of inv(H), and the reference's own noise."""
    cp, cq = diag_blocks(np.linalg.inv(H), N, M)
    cf = scipy.linalg.cho_factor(H, lower=True)
    cp2, cq2 = diag_blocks(scipy.linalg.cho_solve(cf, np.eye(H.shape[0])), N, M)
    noise = max(rel_block_diff(cp2, cp), rel_block_diff(cq2, cq))
    return cp, cq, noise
