"""numpy fp64 restatement of the face fluxes of the divergence-form operator, their wall totals, both adjoints and the
effective coefficient (ABI 23, extended: srpde_div_face_flux, srpde_div_face_flux_grad, srpde_div_wall_flux,
srpde_div_wall_flux_grad; poisson.face_flux, poisson.wall_flux, poisson.effective_coefficient).  Built on
tests/div_bd_ref.py.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

Fx [..., n, n + 1]: entry (i, j) is the face between nodes (i, j - 1) and (i, j); Fy [..., n + 1, n]: entry (i, j) is the
face between nodes (i - 1, j) and (i, j).  The order of operations is the header's: a face between two nodes is
(c * (u_hi - u_lo)) * inv_h, a "d" side's wall face (theta_a * (u_a - g)) * inv_h (low) or (theta_a * (g - u_a)) * inv_h
(high), an "n" side's -q (low) or +q (high).  Wall totals are summed with math.fsum: the exactly rounded sum, which
any order of summation is compared with.
"""
from __future__ import annotations

import math

import numpy as np

import div_adjoint_ref as A
import div_bc_ref as BC
import div_bd_ref as BD
import poisson_div_ref as D

PATTERNS = BC.PATTERNS                                   # all 16, PATTERNS[mask]
AXIS_PATTERNS = ("ddnn", "nndd")                         # effective_coefficient's sides for axis 0 / 1


def _prepare(u, theta, bd, inv_h2):
    u = np.asarray(u, dtype=np.float64)
    theta = np.ascontiguousarray(np.broadcast_to(np.asarray(theta, dtype=np.float64), u.shape))
    n = u.shape[-1]
    bd = BD._like(np.zeros((4, n)) if bd is None else bd, u)
    inv_h2 = np.float64((n - 1) ** 2 if inv_h2 is None else inv_h2)
    return u, theta, bd, n, np.sqrt(inv_h2)


def face_flux(u, theta, bd=None, mean="harmonic", bc="dddd", inv_h2=None):
    """(Fx, Fy) in the device's rounding order; bd None is data of zeros."""
    u, t, bd, n, inv_h = _prepare(u, theta, bd, inv_h2)
    p = BD.pad(u, bd, bc)
    Fx = np.empty(u.shape[:-2] + (n, n + 1))
    Fy = np.empty(u.shape[:-2] + (n + 1, n))
    Fx[..., :, 1:n] = (D.face(t[..., :, :-1], t[..., :, 1:], mean) * (u[..., :, 1:] - u[..., :, :-1])) * inv_h
    Fy[..., 1:n, :] = (D.face(t[..., :-1, :], t[..., 1:, :], mean) * (u[..., 1:, :] - u[..., :-1, :])) * inv_h
    Fy[..., 0, :] = -bd[..., 0, :] if bc[0] == "n" else (t[..., 0, :] * (u[..., 0, :] - p[..., 0, 1:-1])) * inv_h
    Fy[..., n, :] = bd[..., 1, :] if bc[1] == "n" else (t[..., -1, :] * (p[..., -1, 1:-1] - u[..., -1, :])) * inv_h
    Fx[..., :, 0] = -bd[..., 2, :] if bc[2] == "n" else (t[..., :, 0] * (u[..., :, 0] - p[..., 1:-1, 0])) * inv_h
    Fx[..., :, n] = bd[..., 3, :] if bc[3] == "n" else (t[..., :, -1] * (p[..., 1:-1, -1] - u[..., :, -1])) * inv_h
    return Fx, Fy


def divergence(Fx, Fy, inv_h):
    """((Fx[i][j+1] - Fx[i][j]) + (Fy[i+1][j] - Fy[i][j])) * inv_h, and the sum of the four faces' absolute values
    * inv_h: what a rounding bound of the difference scales with."""
    d = ((Fx[..., :, 1:] - Fx[..., :, :-1]) + (Fy[..., 1:, :] - Fy[..., :-1, :])) * inv_h
    m = ((np.abs(Fx[..., :, 1:]) + np.abs(Fx[..., :, :-1])) + (np.abs(Fy[..., 1:, :]) + np.abs(Fy[..., :-1, :]))) * inv_h
    return d, m


def wall_terms(u, theta, bd=None, bc="dddd", inv_h2=None):
    """[..., 4, n]: the outward flux through every wall face, the sides in the mask's order: -Fy[0], +Fy[n], -Fx[:, 0],
    +Fx[:, n] (wall faces do not depend on the face mean)."""
    Fx, Fy = face_flux(u, theta, bd, "arithmetic", bc, inv_h2)
    n = Fx.shape[-2]
    return np.stack([-Fy[..., 0, :], Fy[..., n, :], -Fx[..., :, 0], Fx[..., :, n]], axis=-2)


def wall_flux(u, theta, bd=None, bc="dddd", inv_h2=None, with_abs=False):
    """W [..., 4] = h * fsum(the side's terms); with_abs: also h * fsum(|terms|)."""
    t = wall_terms(u, theta, bd, bc, inv_h2)
    n = t.shape[-1]
    h = 1.0 / np.sqrt(np.float64((n - 1) ** 2 if inv_h2 is None else inv_h2))
    flat = t.reshape(-1, n)
    W = np.array([h * math.fsum(r) for r in flat]).reshape(t.shape[:-1])
    if not with_abs:
        return W
    return W, np.array([h * math.fsum(np.abs(r)) for r in flat]).reshape(t.shape[:-1])


def _edges(n):
    """The index of a field's edge row per side, in the mask's order."""
    return ((Ellipsis, 0, slice(None)), (Ellipsis, n - 1, slice(None)), (Ellipsis, slice(None), 0),
            (Ellipsis, slice(None), n - 1))


def face_flux_adjoint(u, theta, gFx, gFy, bd=None, mean="harmonic", bc="dddd", inv_h2=None, with_abs=False):
    """(gu, gtheta, gbd) of <gFx, Fx> + <gFy, Fy> in the header's order; with_abs: the same sums of the terms'
    absolute values as a second triple."""
    u, t, bd, n, inv_h = _prepare(u, theta, bd, inv_h2)
    cE, cW, cS, cN = BC._cut(*D._faces(t, mean), bc)
    dE, dW, dS, dN = BC._cut(*A._dfaces(t, mean), bc)
    uE, uW, uS, uN = BD._neighbours(BD.pad(u, bd, bc))
    gW, gE, gN, gS = gFx[..., :, :n], gFx[..., :, 1:], gFy[..., :n, :], gFy[..., 1:, :]
    gu = ((cW * gW - cE * gE) + (cN * gN - cS * gS)) * inv_h
    tW, tE = (dW * (u - uW)) * gW, (dE * (uE - u)) * gE
    tN, tS = (dN * (u - uN)) * gN, (dS * (uS - u)) * gS
    gth = ((tW + tE) + (tN + tS)) * inv_h
    edges = _edges(n)
    walls = ((gFy[..., 0, :], -1.0), (gFy[..., n, :], 1.0), (gFx[..., :, 0], -1.0), (gFx[..., :, n], 1.0))
    gbd = np.empty(u.shape[:-2] + (4, n))
    for s, (gF, sign) in enumerate(walls):
        gbd[..., s, :] = sign * gF if bc[s] == "n" else sign * ((t[edges[s]] * inv_h) * gF)
    if not with_abs:
        return gu, gth, gbd
    mu = ((np.abs(cW * gW) + np.abs(cE * gE)) + (np.abs(cN * gN) + np.abs(cS * gS))) * inv_h
    mth = ((np.abs(tW) + np.abs(tE)) + (np.abs(tN) + np.abs(tS))) * inv_h
    return (gu, gth, gbd), (mu, mth, np.abs(gbd))


def _scatter(e, shape):
    """The four edge rows [..., 4, n] added into a zero field in the sides' order."""
    n = shape[-1]
    g = np.zeros(shape)
    g[..., 0, :] += e[..., 0, :]
    g[..., n - 1, :] += e[..., 1, :]
    g[..., :, 0] += e[..., 2, :]
    g[..., :, n - 1] += e[..., 3, :]
    return g


def wall_flux_adjoint(gW, u, theta, bd=None, bc="dddd", inv_h2=None, with_abs=False):
    """(gu [..., n, n], gtheta [..., n, n], gbd [..., 4, n]) of <gW, W> in the header's order: w = gW * h, then per
    edge entry -((theta_a * inv_h) * w), ((g - u_a) * inv_h) * w and (theta_a * inv_h) * w on a "d" side, 0, 0 and w on
    an "n" side; the edge rows added into zero fields in the sides' order."""
    u, t, bd, n, inv_h = _prepare(u, theta, bd, inv_h2)
    h = 1.0 / inv_h
    gW = np.asarray(gW, dtype=np.float64)
    eu, et, eb = (np.zeros(u.shape[:-2] + (4, n)) for _ in range(3))
    for s, e in enumerate(_edges(n)):
        w = (gW[..., s] * h)[..., None]
        if bc[s] == "n":
            eb[..., s, :] = w
        else:
            tw = t[e] * inv_h
            eu[..., s, :] = -(tw * w)
            et[..., s, :] = ((bd[..., s, :] - u[e]) * inv_h) * w
            eb[..., s, :] = tw * w
    out = _scatter(eu, u.shape), _scatter(et, u.shape), eb
    if not with_abs:
        return out
    return out, (_scatter(np.abs(eu), u.shape), _scatter(np.abs(et), u.shape), np.abs(eb))


def unit_gradient_data(n, axis):
    """(pattern, bd [4, n]): g = 1 beyond the first wall of the axis, 0 beyond the second, the other sides insulated."""
    bd = np.zeros((4, n))
    bd[2 * axis] = 1.0
    return AXIS_PATTERNS[axis], bd


def _solve(f, theta, bd, mean, bc, solver, rtol):
    if solver == "dense":
        return BD.solve_dense(f, theta, bd, mean, bc)[0]
    return BD.pcg(f, theta, bd, mean, bc, rtol=rtol)[0]


def effective_coefficient(theta, axis=0, mean="harmonic", solver="dense", rtol=1e-12):
    """theta_eff of one [n, n] field: 0.5 (W_first - W_second) (n + 1) / n of the solution of A_bd u = 0 with the unit
    gradient's data, by a dense solve or by div_bd_ref.pcg (the device's iteration) at rtol."""
    theta = np.asarray(theta, dtype=np.float64)
    n = theta.shape[-1]
    bc, bd = unit_gradient_data(n, axis)
    u = _solve(np.zeros((n, n)), theta, bd, mean, bc, solver, rtol)
    W = wall_flux(u, theta, bd, bc)
    return 0.5 * (W[2 * axis] - W[2 * axis + 1]) * (n + 1) / n


def effective_coefficient_grad(theta, axis=0, mean="harmonic", solver="dense", rtol=1e-12):
    """d theta_eff / d theta [n, n] by the adjoint: the wall totals' direct gradient in theta plus the solve's,
    +G(u, lam; theta) with lam = (D_bc)^-1 gu (the operator is symmetric); both solves dense, or both by
    div_bd_ref.pcg at rtol."""
    theta = np.asarray(theta, dtype=np.float64)
    n = theta.shape[-1]
    bc, bd = unit_gradient_data(n, axis)
    u = _solve(np.zeros((n, n)), theta, bd, mean, bc, solver, rtol)
    gW = np.zeros(4)
    gW[2 * axis], gW[2 * axis + 1] = 0.5 * (n + 1) / n, -0.5 * (n + 1) / n
    gu, gth, _ = wall_flux_adjoint(gW, u, theta, bd, bc)
    lam = _solve(gu, theta, np.zeros((4, n)), mean, bc, solver, rtol)
    return gth + BD.theta_grad(u, lam, theta, bd, mean, bc)


def effective_cases(n, axis):
    """(theta [3, n, n], {mean: the three closed forms, None where there is none}): uniform 1.7, layers parallel to the
    flow along ``axis``, layers across it; the layers ~ U(0.5, 2)."""
    layers = D.rng(3000 + n).uniform(0.5, 2.0, n)
    rows, cols = np.broadcast_to(layers[:, None], (n, n)), np.broadcast_to(layers[None, :], (n, n))
    parallel, across = (cols, rows) if axis == 0 else (rows, cols)
    theta = np.ascontiguousarray(np.stack([np.full((n, n), 1.7), parallel, across]))
    par = layered_parallel(layers)
    return theta, {"arithmetic": [1.7, par, None], "harmonic": [1.7, par, layered_series(layers)]}


def layered_parallel(layers):
    """Layers parallel to the flow: the mean of theta across the layers (each layer is a strip of uniform theta from
    wall to wall, carrying theta_layer * the uniform gradient; both face means see uniform theta along the flow)."""
    return float(np.mean(layers))


def layered_series(layers):
    """Layers across the flow, harmonic mean: n - 1 interior faces of resistance (1/ta + 1/tb) / 2 and two wall faces of
    resistance 1 / theta_a in series over n + 1 cells: (n + 1) / (sum_a 1/theta_a + (1/theta_0 + 1/theta_{n-1}) / 2)."""
    t = np.asarray(layers, dtype=np.float64)
    return float((len(t) + 1) / (np.sum(1.0 / t) + 0.5 * (1.0 / t[0] + 1.0 / t[-1])))
