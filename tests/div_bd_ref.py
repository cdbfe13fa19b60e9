"""numpy fp64 restatement of the divergence-form operator with boundary values and prescribed fluxes (ABI 23, extended): the
operator A_bd, its affine part b, Crank-Nicolson's right-hand side, both gradients, the smoother's sweep and the CG with
the stop rule on |f - b|.  Built on tests/div_bc_ref.py.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

Boundary data is [..., 4, n]: the sides in the pattern's order (row 0, row n - 1, column 0, column n - 1), entry k of a
row side at column k, of a column side at row k.  On a "d" side it is the ghost value g, on an "n" side the outward
flux q.  The order of operations is the header's: the face sum of div_bc_ref.apply on a field padded with g beyond "d"
sides (0 beyond "n" sides and in the corners), * inv_h2, + ((qE + qW) + (qS + qN)) * inv_h at nodes with a flux-side
ghost face only, then the shift.
"""
from __future__ import annotations

import numpy as np

import diffuse_ref as R
import div_adjoint_ref as A
import div_bc_ref as BC
import poisson_div_ref as D

ASYM = "dnnd"                                              # the asymmetric pattern of the suites
PATTERNS = (None, "ddnn", "ndnd", "nnnn", ASYM)


def pattern(bc):
    return "dddd" if bc is None else bc


def data(n, seed, B=None):
    """Random boundary data [4, n] or [B, 4, n], standard normal."""
    return D.rng(1000 + seed).standard_normal((4, n) if B is None else (B, 4, n))


def _like(bd, u):
    return np.broadcast_to(np.asarray(bd, dtype=np.float64), u.shape[:-2] + (4, u.shape[-1]))


def pad(u, bd, bc):
    """u with its ring: g beyond the "d" sides, 0 beyond the "n" sides and in the four corners."""
    bd = _like(bd, u)
    p = np.pad(u, [(0, 0)] * (u.ndim - 2) + [(1, 1), (1, 1)])
    if bc[0] == "d":
        p[..., 0, 1:-1] = bd[..., 0, :]
    if bc[1] == "d":
        p[..., -1, 1:-1] = bd[..., 1, :]
    if bc[2] == "d":
        p[..., 1:-1, 0] = bd[..., 2, :]
    if bc[3] == "d":
        p[..., 1:-1, -1] = bd[..., 3, :]
    return p


def flux(u, bd, bc):
    """((qE + qW) + (qS + qN), the mask of the nodes with a flux-side ghost face), both of u's shape."""
    bd = _like(bd, u)
    qE, qW, qS, qN = (np.zeros(u.shape) for _ in range(4))
    on = np.zeros(u.shape, dtype=bool)
    if bc[0] == "n":
        qN[..., 0, :] = bd[..., 0, :]
        on[..., 0, :] = True
    if bc[1] == "n":
        qS[..., -1, :] = bd[..., 1, :]
        on[..., -1, :] = True
    if bc[2] == "n":
        qW[..., :, 0] = bd[..., 2, :]
        on[..., :, 0] = True
    if bc[3] == "n":
        qE[..., :, -1] = bd[..., 3, :]
        on[..., :, -1] = True
    return (qE + qW) + (qS + qN), on


def _neighbours(p):
    return p[..., 1:-1, 2:], p[..., 1:-1, :-2], p[..., 2:, 1:-1], p[..., :-2, 1:-1]     # E, W, S, N


def apply(u, theta, bd, mean="harmonic", bc="dddd", sigma=0.0, inv_h2=None):
    """y = A_bd u in the device's rounding order."""
    u = np.asarray(u, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape)
    n = u.shape[-1]
    inv_h2 = np.float64((n - 1) ** 2 if inv_h2 is None else inv_h2)
    inv_h = np.sqrt(inv_h2)
    cE, cW, cS, cN = BC._cut(*D._faces(theta, mean), bc)
    uE, uW, uS, uN = _neighbours(pad(u, bd, bc))
    y = ((cE * (uE - u) + cW * (uW - u)) + (cS * (uS - u) + cN * (uN - u))) * inv_h2
    q, on = flux(u, bd, bc)
    y = np.where(on, y + q * inv_h, y)
    return y - sigma * u if sigma != 0.0 else y


def affine(theta, bd, mean="harmonic", bc="dddd", inv_h2=None, shape=None):
    """b = A_bd 0 at sigma = 0."""
    theta = np.asarray(theta, dtype=np.float64)
    return apply(np.zeros(theta.shape if shape is None else shape), theta, bd, mean, bc, 0.0, inv_h2)


def step_rhs(u, f, theta, bd, mean, sigma, scheme, bc="dddd"):
    f = np.zeros_like(u) if f is None else f
    if scheme == "be":
        return f - sigma * u
    return (2.0 * f - sigma * u) - apply(u, theta, bd, mean, bc)


def theta_grad(u, lam, theta, bd, mean="harmonic", bc="dddd", inv_h2=None, scale=1.0):
    """scale * G(u, lam; theta) with g in u's ring and 0 in lam's."""
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    theta = np.ascontiguousarray(np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape))
    n = u.shape[-1]
    if inv_h2 is None:
        inv_h2 = float((n - 1) ** 2)
    dE, dW, dS, dN = BC._cut(*A._dfaces(theta, mean), bc)
    uE, uW, uS, uN = _neighbours(pad(u, bd, bc))
    lE, lW, lS, lN = _neighbours(pad(lam, np.zeros((4, n)), bc))
    tE, tW = (dE * (uE - u)) * (lE - lam), (dW * (uW - u)) * (lW - lam)
    tS, tN = (dS * (uS - u)) * (lS - lam), (dN * (uN - u)) * (lN - lam)
    return (((tE + tW) + (tS + tN)) * inv_h2) * scale


def bd_grad(lam, theta, bc="dddd", inv_h2=None):
    """[..., 4, n] = d<lam, A_bd u>/d bd: (inv_h2 * theta_a) * lam_a on a "d" side, inv_h * lam_a on an "n" side."""
    lam = np.asarray(lam, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), lam.shape)
    n = lam.shape[-1]
    inv_h2 = np.float64((n - 1) ** 2 if inv_h2 is None else inv_h2)
    inv_h = np.sqrt(inv_h2)
    edges = ((Ellipsis, 0, slice(None)), (Ellipsis, -1, slice(None)), (Ellipsis, slice(None), 0),
             (Ellipsis, slice(None), -1))
    out = np.empty(lam.shape[:-2] + (4, n))
    for s, e in enumerate(edges):
        out[..., s, :] = inv_h * lam[e] if bc[s] == "n" else (inv_h2 * theta[e]) * lam[e]
    return out


def relax(u, f, theta, bd, mean, bc, inv_h2, sweeps, omega=0.8):
    """srpde_div_relax_bd restated: one plain pass per sweep, Jacobi, the ring held at g."""
    u = np.array(u, dtype=np.float64)
    f, theta = np.asarray(f, np.float64), np.asarray(theta, np.float64)
    inv_h2 = np.float64(inv_h2)
    inv_h = np.sqrt(inv_h2)
    cE, cW, cS, cN = BC._cut(*D._faces(theta, mean), bc)
    q, on = flux(u, bd, bc)
    g = np.where(on, f - q * inv_h, f) / inv_h2
    w = np.float64(omega) / ((cE + cW) + (cS + cN))
    for _ in range(sweeps):
        uE, uW, uS, uN = _neighbours(pad(u, bd, bc))
        a = (cE * (uE - u) + cW * (uW - u)) + (cS * (uS - u) + cN * (uN - u))
        u = u + w * (a - g)
    return u


def precondition(r, bc, sigma_p):
    return R.precondition(r, sigma_p) if bc == "dddd" else BC.sep_solve(r, bc, sigma_p)


def pcg(f, theta, bd, mean="harmonic", bc="dddd", sigma=0.0, sigma_p=None, rtol=1e-12, maxit=None, u0=None):
    """The iteration the device runs on A_bd u = f, one problem: -> (u, iterations, |r| / |f - b|).  The start is
    r = f - A_bd u0 (u0 = None: zeros) and the k = 0 test at rtol; the iteration itself is homogeneous."""
    n = f.shape[-1]
    if sigma_p is None:
        sigma_p = R.precond_shift(theta, sigma)
    assert bc != "nnnn" or (sigma > 0.0 and sigma_p > 0.0)
    if maxit is None:
        maxit = 20 * n * n
    ref = f - affine(theta, bd, mean, bc)
    nf = np.sqrt(np.sum(ref * ref))
    if nf == 0.0:
        return np.zeros_like(f), 0, 0.0
    x = np.zeros_like(f) if u0 is None else u0.copy()
    r = f - apply(x, theta, bd, mean, bc, sigma)
    nr = np.sqrt(np.sum(r * r))
    k, resid = 0, nr / nf
    if nr <= rtol * nf:
        return x, 0, resid
    z = precondition(r, bc, sigma_p)
    p = z.copy()
    rz = np.sum(r * z)
    while k < maxit:
        q = BC.apply(p, theta, mean, bc, sigma)
        alpha = rz / np.sum(p * q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        nr = np.sqrt(np.sum(r * r))
        resid = nr / nf
        if nr <= rtol * nf:
            break
        z = precondition(r, bc, sigma_p)
        rz_new = np.sum(r * z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, k, resid


def solve_dense(f, theta, bd, mean="harmonic", bc="dddd", sigma=0.0):
    """(D_bc - sigma I)^-1 (f - b) by a dense solve, and the matrix's smallest eigenvalue of -(D_bc - sigma I)."""
    n = f.shape[-1]
    M = BC.dense(theta, mean, bc, sigma)
    rhs = f - affine(theta, bd, mean, bc)
    return np.linalg.solve(M, rhs.reshape(-1)).reshape(n, n), float(np.linalg.eigvalsh(-M)[0])


def diffuse_dense(u0, theta, bd, f=None, dt=1.0, steps=1, scheme="be", mean="harmonic", bc="dddd"):
    """``steps`` dense steps of u_t = A_bd u - f: (D_bc - sigma I) u+ = rhs - b."""
    n = u0.shape[-1]
    sigma = R.step_sigma(dt, scheme)
    Ainv = np.linalg.inv(BC.dense(theta, mean, bc, sigma))
    b = affine(theta, bd, mean, bc)
    u = u0.copy()
    for _ in range(steps):
        u = (Ainv @ (step_rhs(u, f, theta, bd, mean, sigma, scheme, bc) - b).reshape(-1)).reshape(n, n)
    return u
