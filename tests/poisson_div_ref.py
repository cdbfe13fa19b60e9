"""numpy fp64 restatement of the divergence-form operator div(theta grad u) and of its sine-preconditioned CG.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

Grid: all n^2 nodes unknown, a zero ghost ring one h outside, h = 1 / (n - 1).  Face coefficient between node a and
its neighbour b: 0.5 * (ta + tb) ("arithmetic") or (2.0 * (ta * tb)) / (ta + tb) ("harmonic"); towards the ghost ring
c = ta and u_b = 0.  Then, every operation rounded once (numpy contracts nothing),

    y = ((cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))) * inv_h2
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import spsolve

MEANS = ("arithmetic", "harmonic")


def face(ta, tb, mean):
    if mean == "arithmetic":
        return 0.5 * (ta + tb)
    if mean == "harmonic":
        return (2.0 * (ta * tb)) / (ta + tb)
    raise ValueError(mean)


def _faces(theta, mean):
    """cE, cW, cS, cN [..., n, n]: E is x + 1 (the last axis), S is y + 1."""
    t = theta
    cE, cW, cS, cN = t.copy(), t.copy(), t.copy(), t.copy()
    cE[..., :, :-1] = face(t[..., :, :-1], t[..., :, 1:], mean)
    cW[..., :, 1:] = face(t[..., :, 1:], t[..., :, :-1], mean)
    cS[..., :-1, :] = face(t[..., :-1, :], t[..., 1:, :], mean)
    cN[..., 1:, :] = face(t[..., 1:, :], t[..., :-1, :], mean)
    return cE, cW, cS, cN


def apply(u, theta, mean="harmonic", inv_h2=None):
    """y = D_theta u in the rounding order of the module docstring; u, theta [..., n, n] (theta broadcasts)."""
    u = np.asarray(u, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape)
    n = u.shape[-1]
    if inv_h2 is None:
        inv_h2 = float((n - 1) ** 2)
    cE, cW, cS, cN = _faces(theta, mean)
    p = np.pad(u, [(0, 0)] * (u.ndim - 2) + [(1, 1), (1, 1)])
    uE, uW = p[..., 1:-1, 2:], p[..., 1:-1, :-2]
    uS, uN = p[..., 2:, 1:-1], p[..., :-2, 1:-1]
    return ((cE * (uE - u) + cW * (uW - u)) + (cS * (uS - u) + cN * (uN - u))) * inv_h2


def dense(theta, mean="harmonic"):
    """The n^2 x n^2 matrix of D_theta, column j = apply(e_j)."""
    n = theta.shape[-1]
    eye = np.eye(n * n).reshape(n * n, n, n)
    return apply(eye, theta, mean).reshape(n * n, n * n).T.copy()


def sparse(theta, mean="harmonic"):
    """D_theta as CSR, entries formed as the operator forms them (for grids too large for ``dense``)."""
    n = theta.shape[-1]
    inv_h2 = float((n - 1) ** 2)
    cE, cW, cS, cN = _faces(theta, mean)
    idx = np.arange(n * n).reshape(n, n)
    diag = (((cE * -1.0 + cW * -1.0) + (cS * -1.0 + cN * -1.0)) * inv_h2).reshape(-1)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [diag]
    for c, a, b in ((cE, idx[:, :-1], idx[:, 1:]), (cW, idx[:, 1:], idx[:, :-1]),
                    (cS, idx[:-1, :], idx[1:, :]), (cN, idx[1:, :], idx[:-1, :])):
        rows.append(a.reshape(-1))
        cols.append(b.reshape(-1))
        vals.append((c.reshape(-1)[a.reshape(-1)]) * inv_h2)
    return csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n))


def solve_dense(f, theta, mean="harmonic"):
    n = f.shape[-1]
    return np.linalg.solve(dense(theta, mean), f.reshape(-1)).reshape(n, n)


def solve_sparse(f, theta, mean="harmonic"):
    n = f.shape[-1]
    return spsolve(sparse(theta, mean).tocsc(), f.reshape(-1)).reshape(n, n)


@functools.lru_cache(maxsize=None)
def sine_plan(n):
    """S (symmetric, orthogonal) and the eigenvalues of tridiag(1, -2, 1)."""
    j = np.arange(1, n + 1)
    S = np.sqrt(2.0 / (n + 1)) * np.sin(np.pi * np.outer(j, j) / (n + 1))
    lam = -4.0 * np.sin(np.pi * j / (2.0 * (n + 1))) ** 2
    return S, lam


def precondition(r):
    """z = L^-1 r, L the 5-point Laplacian (theta = 1) on the same grid."""
    n = r.shape[-1]
    S, lam = sine_plan(n)
    h2 = (1.0 / (n - 1)) ** 2
    return S @ ((S @ r @ S) * (h2 / (lam[:, None] + lam[None, :]))) @ S


def pcg(f, theta, mean="harmonic", rtol=1e-12, maxit=None):
    """The iteration the device runs, for one problem: -> (u, iterations, |r| / |f|)."""
    n = f.shape[-1]
    if maxit is None:
        maxit = 20 * n * n
    x = np.zeros_like(f)
    nf = np.sqrt(np.sum(f * f))
    if nf == 0.0:
        return x, 0, 0.0
    r = f.copy()
    z = precondition(r)
    p = z.copy()
    rz = np.sum(r * z)
    k, resid = 0, 1.0
    while k < maxit:
        q = apply(p, theta, mean)
        alpha = rz / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        nr = np.sqrt(np.sum(r * r))
        resid = nr / nf
        if nr <= rtol * nf:
            break
        z = precondition(r)
        rz_new = np.sum(r * z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k, resid


# ---- seeded inputs ------------------------------------------------------------------------------------------
def rng(seed):
    return np.random.default_rng(seed)


def field_u(n, seed, B=None):
    """Unsymmetric standard-normal u."""
    return rng(1000 + seed).standard_normal((n, n) if B is None else (B, n, n))


def field_theta(n, seed, lo, hi, B=None):
    """theta ~ U(lo, hi) per pixel."""
    return rng(2000 + seed).uniform(lo, hi, (n, n) if B is None else (B, n, n))


def forcing(n, k1=3.3, k2=1.7):
    """The project's forcing sin(2 pi k1 X) sin(2 pi k2 Y) on linspace(0, 1, n)^2, non-integer k."""
    x = np.linspace(0.0, 1.0, n)
    X, Y = np.meshgrid(x, x)
    return np.sin(2.0 * np.pi * k1 * X) * np.sin(2.0 * np.pi * k2 * Y)


# the (n, seed, lo, hi, mean) of every solve the GPU tests compare with ``pcg``
SOLVE_NS = (5, 20, 33, 97, 129)
SOLVE_CASES = [(n, s, 0.5, 2.0, m) for n in SOLVE_NS for s in (0, 1) for m in MEANS]
FREEZE_CASES = [(20, 3, 0.5, 2.0, "harmonic"), (20, 4, 0.1, 10.0, "harmonic")]


def chebyshev_iterations(lo, hi, tol=1e-12):
    """Smallest k with 2 ((sqrt(c) - 1) / (sqrt(c) + 1))^k <= tol for c = hi / lo: CG's bound for a condition number
    c, which theta_max / theta_min bounds for the sine-preconditioned operator."""
    s = np.sqrt(hi / lo)
    rho = (s - 1.0) / (s + 1.0)
    k = 0
    while 2.0 * rho ** k > tol:
        k += 1
    return k
