"""numpy fp64 restatement of the shifted divergence-form operator D_theta - sigma I, of its shifted sine solve and
sine-preconditioned CG, and of one implicit time step of u_t = div(theta grad u) - f.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

Rounding orders (include/srpde.h, ABI 21; numpy contracts nothing):
    apply_shift     y = (face sum * inv_h2) - (sigma * u)
    shift scale     1 / ((lam_i + lam_j) * inv_h2 - sigma_p)
    step_rhs        be: f - sigma * u                  cn: (2 f - sigma * u) - D_theta u
"""
from __future__ import annotations

import numpy as np

import poisson_div_ref as D


def apply_shift(u, theta, mean="harmonic", sigma=0.0, inv_h2=None):
    """y = D_theta u - sigma u in the device's rounding order."""
    u = np.asarray(u, dtype=np.float64)
    return D.apply(u, theta, mean, inv_h2) - sigma * u


def dense_shift(theta, mean="harmonic", sigma=0.0):
    """The n^2 x n^2 matrix of D_theta - sigma I from poisson_div_ref.dense: only the diagonal changes."""
    A = D.dense(theta, mean)
    A[np.diag_indices_from(A)] -= sigma
    return A


def laplacian_dense(n):
    """L, the 5-point Laplacian of the project's grid: D_theta for theta = 1."""
    return D.dense(np.ones((n, n)), "arithmetic")


def sine_solve_shift(r, sigma_p=0.0):
    """z = (L - sigma_p I)^-1 r by the sine transform, the eigenvalue scaling in the stated order."""
    n = r.shape[-1]
    S, lam = D.sine_plan(n)
    inv_h2 = float((n - 1) ** 2)
    scale = 1.0 / ((lam[:, None] + lam[None, :]) * inv_h2 - sigma_p)
    return S @ ((S @ r @ S) * scale) @ S


def precondition(r, sigma_p):
    """What the device applies: the unshifted code for sigma_p = 0, the shifted scaling otherwise."""
    return D.precondition(r) if sigma_p == 0.0 else sine_solve_shift(r, sigma_p)


def precond_shift(theta, sigma):
    """The default sigma_p = sigma / sqrt(theta_min theta_max)."""
    return sigma / float(np.sqrt(theta.min() * theta.max()))


def pcg_shift(f, theta, mean="harmonic", sigma=0.0, sigma_p=None, rtol=1e-12, maxit=None, u0=None):
    """The iteration the device runs on (D_theta - sigma I) u = f, for one problem: -> (u, iterations, |r| / |f|)."""
    n = f.shape[-1]
    if sigma_p is None:
        sigma_p = precond_shift(theta, sigma)
    if maxit is None:
        maxit = 20 * n * n
    nf = np.sqrt(np.sum(f * f))
    if nf == 0.0:
        return np.zeros_like(f), 0, 0.0
    if u0 is None:
        x, r = np.zeros_like(f), f.copy()
    else:
        x = u0.copy()
        r = f - apply_shift(u0, theta, mean, sigma)
    nr = np.sqrt(np.sum(r * r))
    k, resid = 0, nr / nf
    if u0 is not None and nr <= rtol * nf:
        return x, 0, resid
    z = precondition(r, sigma_p)
    p = z.copy()
    rz = np.sum(r * z)
    while k < maxit:
        q = apply_shift(p, theta, mean, sigma)
        alpha = rz / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        nr = np.sqrt(np.sum(r * r))
        resid = nr / nf
        if nr <= rtol * nf:
            break
        z = precondition(r, sigma_p)
        rz_new = np.sum(r * z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k, resid


def step_sigma(dt, scheme):
    return {"be": 1.0, "cn": 2.0}[scheme] / dt


def step_rhs(u, f, theta, mean, sigma, scheme):
    f = np.zeros_like(u) if f is None else f
    if scheme == "be":
        return f - sigma * u
    return (2.0 * f - sigma * u) - D.apply(u, theta, mean)


def step_dense(u, f, theta, dt, scheme="be", mean="harmonic"):
    """One backward-Euler or Crank-Nicolson step of u_t = D_theta u - f as a dense solve (one [n, n] problem)."""
    n = u.shape[-1]
    sigma = step_sigma(dt, scheme)
    rhs = step_rhs(u, f, theta, mean, sigma, scheme)
    return np.linalg.solve(dense_shift(theta, mean, sigma), rhs.reshape(-1)).reshape(n, n)


def diffuse_dense(u0, theta, f=None, dt=1.0, steps=1, scheme="be", mean="harmonic"):
    """``steps`` dense steps with the matrix factored once (theta and dt fixed)."""
    n = u0.shape[-1]
    sigma = step_sigma(dt, scheme)
    Ainv = np.linalg.inv(dense_shift(theta, mean, sigma))
    u = u0.copy()
    for _ in range(steps):
        u = (Ainv @ step_rhs(u, f, theta, mean, sigma, scheme).reshape(-1)).reshape(n, n)
    return u


def eigenmode(n, i, j):
    """The (i, j) sine eigenvector of L (0-based) and mu_ij = (lam_i + lam_j) * inv_h2 <= 0."""
    S, lam = D.sine_plan(n)
    return np.outer(S[:, i], S[:, j]), (lam[i] + lam[j]) * float((n - 1) ** 2)


def decay_factor(dt, c, mu, scheme):
    """The factor one step multiplies an eigenmode by, theta = c constant and f = 0."""
    if scheme == "be":
        return 1.0 / (1.0 - dt * c * mu)
    return (1.0 + dt * c * mu / 2.0) / (1.0 - dt * c * mu / 2.0)


def lambda_min_neg_laplacian(n):
    """The smallest eigenvalue of -L: -2 lam_0 (n - 1)^2."""
    _, lam = D.sine_plan(n)
    return -2.0 * lam[0] * float((n - 1) ** 2)
