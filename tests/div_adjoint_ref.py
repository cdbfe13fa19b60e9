"""numpy fp64 restatement of the pair gradient of the divergence-form operator and of its warm-started PCG.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

With the face coefficient c_ab of tests/poisson_div_ref.py and d_ab = dc_ab / dtheta_a,

    arithmetic:  d = 0.5
    harmonic:    d = (2.0 * (tb * tb)) / ((ta + tb) * (ta + tb))
    ghost face:  d = 1, u_b = lam_b = 0

the pair gradient is, every operation rounded once (numpy contracts nothing),

    t_b = (d_ab * (u_b - u_a)) * (lam_b - lam_a)
    G_a = ((t_E + t_W) + (t_S + t_N)) * inv_h2            g = G * scale

d<lam, D_theta u>/dtheta = -G: for y = D_theta u, grad_theta = -G(u, grad_y); for u = D_theta^-1 f,
grad_theta = +G(u, lam) with lam = D_theta^-1 grad_u.
"""
from __future__ import annotations

import numpy as np

import poisson_div_ref as D


def dface(ta, tb, mean):
    if mean == "arithmetic":
        return np.full_like(ta, 0.5)
    if mean == "harmonic":
        return (2.0 * (tb * tb)) / ((ta + tb) * (ta + tb))
    raise ValueError(mean)


def _dfaces(theta, mean):
    """dE, dW, dS, dN [..., n, n]: E is x + 1 (the last axis), S is y + 1; 1 towards the ghost ring."""
    t = theta
    dE, dW, dS, dN = (np.ones_like(t) for _ in range(4))
    dE[..., :, :-1] = dface(t[..., :, :-1], t[..., :, 1:], mean)
    dW[..., :, 1:] = dface(t[..., :, 1:], t[..., :, :-1], mean)
    dS[..., :-1, :] = dface(t[..., :-1, :], t[..., 1:, :], mean)
    dN[..., 1:, :] = dface(t[..., 1:, :], t[..., :-1, :], mean)
    return dE, dW, dS, dN


def _neighbours(a):
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)])
    return p[..., 1:-1, 2:], p[..., 1:-1, :-2], p[..., 2:, 1:-1], p[..., :-2, 1:-1]     # E, W, S, N


def theta_grad(u, lam, theta, mean="harmonic", inv_h2=None, scale=1.0):
    """scale * G(u, lam; theta) in the rounding order of the module docstring; [..., n, n], theta broadcasts."""
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    theta = np.ascontiguousarray(np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape))
    n = u.shape[-1]
    if inv_h2 is None:
        inv_h2 = float((n - 1) ** 2)
    dE, dW, dS, dN = _dfaces(theta, mean)
    uE, uW, uS, uN = _neighbours(u)
    lE, lW, lS, lN = _neighbours(lam)
    tE, tW = (dE * (uE - u)) * (lE - lam), (dW * (uW - u)) * (lW - lam)
    tS, tN = (dS * (uS - u)) * (lS - lam), (dN * (uN - u)) * (lN - lam)
    return (((tE + tW) + (tS + tN)) * inv_h2) * scale


def pcg_from(f, theta, mean="harmonic", rtol=1e-12, maxit=None, x0=None):
    """poisson_div_ref.pcg from the initial guess x0 (None or zeros: the same operations as pcg), for one problem:
    -> (u, iterations, |r| / |f|).  r0 = f - D x0, |f| and |r0| kept apart; done before the first iteration if
    |r0| <= rtol |f|."""
    n = f.shape[-1]
    if maxit is None:
        maxit = 20 * n * n
    nf = np.sqrt(np.sum(f * f))
    if nf == 0.0:
        return np.zeros_like(f), 0, 0.0
    x = np.zeros_like(f) if x0 is None else np.array(x0, dtype=np.float64)
    r = f - D.apply(x, theta, mean)
    nr = np.sqrt(np.sum(r * r))
    k, resid = 0, nr / nf
    if x0 is not None and nr <= rtol * nf:
        return x, 0, resid
    z = D.precondition(r)
    p = z.copy()
    rz = np.sum(r * z)
    while k < maxit:
        q = D.apply(p, theta, mean)
        alpha = rz / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        nr = np.sqrt(np.sum(r * r))
        resid = nr / nf
        if nr <= rtol * nf:
            break
        z = D.precondition(r)
        rz_new = np.sum(r * z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k, resid


# ---- the warm-start case the host test fixes and the GPU test reuses ----------------------------------------
WARM_N, WARM_SEEDS, WARM_LO, WARM_HI = 40, (7, 8, 9, 10), 0.5, 2.0
WARM_RTOL = 1e-10
WARM_PERTURB = 0.01


def warm_case(seed, n=WARM_N):
    """(f, theta, theta_near) of one problem: theta ~ U(0.5, 2), theta_near = theta * (1 + 0.01 * U(-1, 1)) per
    pixel, f the project's forcing with a wavenumber of its own."""
    th = D.field_theta(n, seed, WARM_LO, WARM_HI)
    near = th * (1.0 + WARM_PERTURB * D.rng(3000 + seed).uniform(-1.0, 1.0, th.shape))
    return D.forcing(n, 3.3 + 0.5 * (seed - WARM_SEEDS[0]), 1.7), th, near


def lambda_min_neg_laplacian(n):
    """The smallest eigenvalue of -L on the project's grid: 8 (n - 1)^2 sin^2(pi / (2 (n + 1)))."""
    return 8.0 * (n - 1) ** 2 * np.sin(np.pi / (2.0 * (n + 1))) ** 2
