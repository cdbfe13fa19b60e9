"""numpy fp64 restatement of the divergence-form operator with zero-flux (Neumann) sides, of the separable solve of its
constant-coefficient counterpart, and of the CG the device runs with it (ABI 22).

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

A pattern is a 4-string of "d" (the zero ghost ring) / "n" (zero flux) for (row 0 side, row n - 1 side, column 0 side,
column n - 1 side); the C entries' mask has bit i set for an "n" at place i.  A zero-flux side's ghost faces have
coefficient 0 (derivative 0 in the pair gradient) where tests/poisson_div_ref.py and tests/div_adjoint_ref.py have
theta_a (1); every other operation and its place are theirs, so "dddd" gives their bits.
"""
from __future__ import annotations

import functools

import numpy as np

import diffuse_ref as R
import div_adjoint_ref as A
import poisson_div_ref as D

PATTERNS = tuple("".join("dn"[m >> i & 1] for i in range(4)) for m in range(16))


def mask(bc):
    assert len(bc) == 4 and set(bc) <= set("dn"), bc
    return sum(1 << i for i, c in enumerate(bc) if c == "n")


def _cut(cE, cW, cS, cN, bc):
    """The ghost faces of the "n" sides set to 0, in place."""
    if bc[0] == "n":
        cN[..., 0, :] = 0.0
    if bc[1] == "n":
        cS[..., -1, :] = 0.0
    if bc[2] == "n":
        cW[..., :, 0] = 0.0
    if bc[3] == "n":
        cE[..., :, -1] = 0.0
    return cE, cW, cS, cN


# ---- the 1-D eigen-decompositions -----------------------------------------------------------------------------------
def tridiag(n, lo, hi):
    """T: 1 off the diagonal, -2 on it, -1 at a Neumann end (lo: node 0, hi: node n - 1; "d" or "n")."""
    T = -2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
    if lo == "n":
        T[0, 0] = -1.0
    if hi == "n":
        T[-1, -1] = -1.0
    return T


@functools.lru_cache(maxsize=None)
def eig1d(n, lo, hi):
    """(Q, lam) in closed form, the trigonometric arguments reduced in integers first: column k of Q is the unit
    eigenvector of tridiag(n, lo, hi) for lam[k]."""
    j = np.arange(n)[:, None]
    k = np.arange(n)[None, :]
    if lo == "d" and hi == "d":
        m = ((j + 1) * (k + 1)) % (2 * (n + 1))
        Q = np.sqrt(2.0 / (n + 1)) * np.sin(np.pi * (m / (n + 1)))
        s = np.sin(np.pi * ((k[0] + 1) / (2.0 * (n + 1))))
    elif lo == "n" and hi == "n":
        m = ((2 * j + 1) * k) % (4 * n)
        Q = np.sqrt(np.where(k > 0, 2.0, 1.0) / n) * np.cos(np.pi * (m / (2 * n)))
        s = np.sin(np.pi * (k[0] / (2.0 * n)))
    else:
        jj = n - 1 - j if lo == "n" else j
        m = ((jj + 1) * (2 * k + 1)) % (2 * (2 * n + 1))
        Q = (2.0 / np.sqrt(2 * n + 1)) * np.sin(np.pi * (m / (2 * n + 1)))
        s = np.sin(np.pi * ((2 * k[0] + 1) / (2.0 * (2 * n + 1))))
    return Q, -4.0 * s * s


def plan(n, bc):
    """(Qy, lam_y, Qx, lam_x): T_y acts along the row index (sides bc[0], bc[1]), T_x along the column index."""
    return eig1d(n, bc[0], bc[1]) + eig1d(n, bc[2], bc[3])


# ---- the operator ---------------------------------------------------------------------------------------------------
def apply(u, theta, mean="harmonic", bc="dddd", sigma=0.0, inv_h2=None):
    """y = D_theta u (- sigma u when sigma != 0: the product, then one subtraction) in the device's rounding order."""
    u = np.asarray(u, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape)
    n = u.shape[-1]
    if inv_h2 is None:
        inv_h2 = float((n - 1) ** 2)
    cE, cW, cS, cN = _cut(*D._faces(theta, mean), bc)
    p = np.pad(u, [(0, 0)] * (u.ndim - 2) + [(1, 1), (1, 1)])
    uE, uW = p[..., 1:-1, 2:], p[..., 1:-1, :-2]
    uS, uN = p[..., 2:, 1:-1], p[..., :-2, 1:-1]
    y = ((cE * (uE - u) + cW * (uW - u)) + (cS * (uS - u) + cN * (uN - u))) * inv_h2
    return y - sigma * u if sigma != 0.0 else y


def dense(theta, mean="harmonic", bc="dddd", sigma=0.0):
    """The n^2 x n^2 matrix of D_theta - sigma I with the sides bc, column j = apply(e_j)."""
    n = theta.shape[-1]
    eye = np.eye(n * n).reshape(n * n, n, n)
    M = apply(eye, theta, mean, bc).reshape(n * n, n * n).T.copy()
    M[np.diag_indices_from(M)] -= sigma
    return M


def theta_grad(u, lam, theta, mean="harmonic", bc="dddd", inv_h2=None, scale=1.0):
    """scale * G(u, lam; theta) in the rounding order of tests/div_adjoint_ref.py, d = 0 towards an "n" side."""
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    theta = np.ascontiguousarray(np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape))
    n = u.shape[-1]
    if inv_h2 is None:
        inv_h2 = float((n - 1) ** 2)
    dE, dW, dS, dN = _cut(*A._dfaces(theta, mean), bc)
    uE, uW, uS, uN = A._neighbours(u)
    lE, lW, lS, lN = A._neighbours(lam)
    tE, tW = (dE * (uE - u)) * (lE - lam), (dW * (uW - u)) * (lW - lam)
    tS, tN = (dS * (uS - u)) * (lS - lam), (dN * (uN - u)) * (lN - lam)
    return (((tE + tW) + (tS + tN)) * inv_h2) * scale


def step_rhs(u, f, theta, mean, sigma, scheme, bc="dddd"):
    f = np.zeros_like(u) if f is None else f
    if scheme == "be":
        return f - sigma * u
    return (2.0 * f - sigma * u) - apply(u, theta, mean, bc)


# ---- the separable solve and the CG -----------------------------------------------------------------------------------
def sep_solve(r, bc, sigma_p=0.0):
    """z = (L_bc - sigma_p I)^-1 r, the eigenvalue scaling in the stated order."""
    n = r.shape[-1]
    Qy, ly, Qx, lx = plan(n, bc)
    inv_h2 = float((n - 1) ** 2)
    scale = 1.0 / ((ly[:, None] + lx[None, :]) * inv_h2 - sigma_p)
    return Qy @ ((Qy.T @ r @ Qx) * scale) @ Qx.T


def pcg(f, theta, mean="harmonic", bc="dddd", sigma=0.0, sigma_p=None, rtol=1e-12, maxit=None, u0=None):
    """The iteration the device runs on (D_theta - sigma I) u = f with the sides bc, for one problem, with its
    per-problem stopping rule: -> (u, iterations, |r| / |f|)."""
    n = f.shape[-1]
    if sigma_p is None:
        sigma_p = R.precond_shift(theta, sigma)
    assert bc != "nnnn" or (sigma > 0.0 and sigma_p > 0.0)
    if maxit is None:
        maxit = 20 * n * n
    nf = np.sqrt(np.sum(f * f))
    if nf == 0.0:
        return np.zeros_like(f), 0, 0.0
    if u0 is None:
        x, r = np.zeros_like(f), f.copy()
    else:
        x = u0.copy()
        r = f - apply(u0, theta, mean, bc, sigma)
    nr = np.sqrt(np.sum(r * r))
    k, resid = 0, nr / nf
    if u0 is not None and nr <= rtol * nf:
        return x, 0, resid
    z = sep_solve(r, bc, sigma_p)
    p = z.copy()
    rz = np.sum(r * z)
    while k < maxit:
        q = apply(p, theta, mean, bc, sigma)
        alpha = rz / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        nr = np.sqrt(np.sum(r * r))
        resid = nr / nf
        if nr <= rtol * nf:
            break
        z = sep_solve(r, bc, sigma_p)
        rz_new = np.sum(r * z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k, resid


def diffuse_dense(u0, theta, f=None, dt=1.0, steps=1, scheme="be", mean="harmonic", bc="dddd"):
    """``steps`` dense steps of u_t = D_theta u - f with the sides bc, the matrix inverted once."""
    n = u0.shape[-1]
    sigma = R.step_sigma(dt, scheme)
    Ainv = np.linalg.inv(dense(theta, mean, bc, sigma))
    u = u0.copy()
    for _ in range(steps):
        u = (Ainv @ step_rhs(u, f, theta, mean, sigma, scheme, bc).reshape(-1)).reshape(n, n)
    return u


def eigenmode(n, bc, i, j):
    """The (i, j) eigenvector of L_bc (0-based) and mu_ij = (lam_y,i + lam_x,j) * inv_h2 <= 0."""
    Qy, ly, Qx, lx = plan(n, bc)
    return np.outer(Qy[:, i], Qx[:, j]), (ly[i] + lx[j]) * float((n - 1) ** 2)


# ---- the insulated box both suites run --------------------------------------------------------------------------------
BOX_N, BOX_DT, BOX_STEPS, BOX_RTOL = 33, 1e-3, 10, 1e-12


def box_case():
    """(u0, theta) of the insulated-box test: u0 standard normal, theta ~ U(0.5, 2)."""
    return D.field_u(BOX_N, 21), D.field_theta(BOX_N, 21, 0.5, 2.0)


def conservation_bound(n, rtol, rhs, sigma, u_prev):
    """|sum u+ - sum u| <= n rtol |rhs|_2 / sigma + 64 n^2 eps max|u|.  1^T (D_theta - sigma I) u+ = -sigma sum u+ for
    four zero-flux sides and 1^T rhs = -sigma sum u, so sigma |sum u+ - sum u| = |1^T r| <= |1|_2 |r|_2 <= n rtol
    |rhs|_2; the second term caps the rounding of the two n^2-term sums compared (64 spare over the sqrt(n^2) expected)."""
    return n * rtol * np.sqrt(np.sum(rhs * rhs)) / sigma + 64.0 * n * n * np.finfo(np.float64).eps * np.abs(u_prev).max()
