"""numpy fp64 restatement of the plain (pointwise-form) CG solver of csrc/poisson.hip: the Chronopoulos-Gear recurrence
of the LDS kernels (cg_lds_kernel, cg_lds_n_kernel) and of the cooperative kernel (gcg_coop_kernel).

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

The system is (-L) u = -f / theta on the project's grid (all n^2 nodes unknown, a zero ghost ring one h outside,
h = 1 / (n - 1)), A = -L the 5-point stencil in the kernels' order,

    A v = ((((4 v - vW) - vE) - vN) - vS) * (n - 1)^2

and the recurrence, one pair of inner products (gamma, delta) = (<r, r>, <A r, r>) per iteration:

    r = -f / theta;  w = A r;  gamma0, delta0;  stop = rtol^2 gamma0;  alpha = gamma0 / delta0;  beta = 0
    while gamma > stop and it < maxit:
        p = r + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  it += 1
        w = A r;  gamma_new, delta_new
        beta = gamma_new / gamma;  alpha = gamma_new / (delta_new - beta * gamma_new / alpha);  gamma = gamma_new

The kernels form beta and alpha from one division (cg_scalars); here they are the three plain divisions that it
replaces, so the two agree to rounding, not bit for bit (the kernels also contract a * b + c into one rounding, and sum
in another order).  Every operation above scales exactly under a power of two, so cg_cg(2^k f) == 2^k cg_cg(f) bit for
bit while nothing leaves fp64's range: numpy's pairwise sums scale exactly too.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import poisson_ref as R


def apply_a(v):
    """A v = -L v for v [n, n], in the kernels' order of operations."""
    n = v.shape[-1]
    p = np.pad(v, 1)
    west, east, north, south = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    return ((((4.0 * v - west) - east) - north) - south) * float((n - 1) * (n - 1))


def cg_cg(f, theta, rtol=1e-12, maxit=None):
    """-> (u, iters, resid, history): the recurrence of the module docstring on one problem f, theta [n, n].
    resid = sqrt(gamma / gamma0) (gamma0 -> 1 when it is 0), the kernels' resid word; history = gamma after 0, 1, ...
    iterations (for messages).  maxit None: 20 n^2, solve_batched's default."""
    f = np.asarray(f, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    n = f.shape[-1]
    if maxit is None:
        maxit = 20 * n * n
    r = -f / theta
    w = apply_a(r)
    gamma, delta = float(np.sum(r * r)), float(np.sum(w * r))
    g0 = gamma
    stop = rtol * rtol * gamma
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.float64(gamma) / np.float64(delta)       # 0 / 0 for f = 0: never used, the loop does not run
    beta = 0.0
    x, p, s = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    it = 0
    history = [gamma]
    while gamma > stop and it < maxit:
        p = r + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        it += 1
        w = apply_a(r)
        gn, dn = float(np.sum(r * r)), float(np.sum(w * r))
        beta = gn / gamma
        alpha = gn / (dn - beta * gn / alpha)
        gamma = gn
        history.append(gamma)
    return x, it, float(np.sqrt(gamma / (g0 if g0 > 0.0 else 1.0))), history


def true_resid(u, f, theta):
    """|-f / theta - A u| / |f / theta| from the oracle's matrix-free operator (another statement of the stencil)."""
    b = -np.asarray(f, dtype=np.float64) / theta
    au = -R.apply_operator(np.asarray(u, dtype=np.float64), np.ones_like(b))
    return float(np.linalg.norm(b - au) / np.linalg.norm(b))


def kappa(n):
    """The condition-number allowance 4 (n - 1)^2 / (2 pi^2) that test_grid_cg_at_the_cooperative_size_bound uses:
    lambda_max -> 8 / h^2 over lambda_min -> 2 pi^2."""
    return 4.0 * (n - 1) ** 2 / (2.0 * np.pi ** 2)


def iters_close(a, b):
    """The bar of test_cooperative_grid_cg_matches_polled for two roundings of one Krylov iteration: 2 % + 2."""
    return abs(int(a) - int(b)) <= 0.02 * int(b) + 2


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def fields(n, count=3, seed=0, wide_theta=False):
    """Deterministic (f, theta) [count, n, n], read-only: theta ~ U(0.5, 2) (``wide_theta``: 2^U(-6, 6)); f[0] the
    project's forcing sin(2 pi k1 X) sin(2 pi k2 Y) with seeded (k1, k2) in (0.5, 8), the others standard normal."""
    rng = np.random.default_rng(1000 * n + seed)
    theta = 2.0 ** rng.uniform(-6.0, 6.0, (count, n, n)) if wide_theta else rng.uniform(0.5, 2.0, (count, n, n))
    k1, k2 = rng.uniform(0.5, 8.0, 2)
    f = rng.standard_normal((count, n, n))
    f[0] = R.forcing(k1, k2, n)
    f.setflags(write=False)
    theta.setflags(write=False)
    return f, theta


@functools.lru_cache(maxsize=None)
def reference(n, b, count=3, seed=0, wide_theta=False, rtol=1e-12, maxit=None):
    """cg_cg of problem b of fields(n, count, seed, wide_theta), computed once per session."""
    f, theta = fields(n, count, seed, wide_theta)
    u, it, resid, hist = cg_cg(f[b], theta[b], rtol, maxit)
    u.setflags(write=False)
    return u, it, resid, tuple(hist)


@functools.lru_cache(maxsize=None)
def direct(n, b, count=3, seed=0):
    """oracle.poisson_ref.solve (SuperLU) of problem b of fields(n, count, seed), computed once per session."""
    f, theta = fields(n, count, seed)
    u = R.solve(f[b], theta[b])
    u.setflags(write=False)
    return u
