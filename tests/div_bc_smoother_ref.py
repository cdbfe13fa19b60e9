"""numpy / torch restatements of the divergence-form smoother and loss term with zero-flux (Neumann) sides (ABI 23:
srpde_div_relax_bc, srpde_physics_loss_div_fwd_bc).

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

A pattern is tests/div_bc_ref.py's 4-string.  A zero-flux side's ghost faces have coefficient 0.0 where
tests/test_div_smoother_host.py's restatements have theta_a; the zero is multiplied in like any coefficient, never
skipped, so the signs of zeros agree with the device too, and "dddd" gives the bc-less restatements' bits.
"""
from __future__ import annotations

import numpy as np
import torch

import div_bc_ref as B
import poisson_div_ref as D

INV_H2 = (39.0 ** 2, 79.0 ** 2)


def relax_div_bc_np(u, f, theta, mean, bc, inv_h2, sweeps, omega=0.8):
    """srpde_div_relax_bc restated: fields [E, n, n] fp64, one plain pass per sweep, every operation one rounded numpy
    pass in the header's order, Jacobi (each sweep reads the previous one's u throughout)."""
    u = np.array(u, dtype=np.float64)
    f, theta = np.asarray(f, np.float64), np.asarray(theta, np.float64)
    cE, cW, cS, cN = B._cut(*D._faces(theta, mean), bc)
    g = f / np.float64(inv_h2)
    w = np.float64(omega) / ((cE + cW) + (cS + cN))
    for _ in range(sweeps):
        p = np.pad(u, ((0, 0), (1, 1), (1, 1)))                       # a node outside the grid is 0
        uE, uW, uS, uN = p[:, 1:-1, 2:], p[:, 1:-1, :-2], p[:, 2:, 1:-1], p[:, :-2, 1:-1]
        a = (cE * (uE - u) + cW * (uW - u)) + (cS * (uS - u) + cN * (uN - u))
        u = u + w * (a - g)
    return u


def dirichlet_ghost_count(n, bc, dtype=torch.float64):
    """k_d [n, n]: the number of each node's ghost faces on "d" sides (D_theta 1 = -k_d theta)."""
    k = torch.zeros(n, n, dtype=dtype)
    if bc[0] == "d":
        k[0, :] += 1
    if bc[1] == "d":
        k[-1, :] += 1
    if bc[2] == "d":
        k[:, 0] += 1
    if bc[3] == "d":
        k[:, -1] += 1
    return k


def restatement_div_bc(y, t, x, kind, stats, weight, inv_h2=INV_H2, mean="harmonic", bc="dddd", dtype=torch.float64):
    """The loss of srpde_physics_loss_div_fwd_bc.  y, t [B, 1, n, n], x [B, 3, n, n], kind [B], stats 6 values ->
    dict(total, mse, pde, r, m, theta, q, M) in ``dtype`` throughout; differentiable in y.  The pattern applies to the
    kind-0 samples; a kind-1 sample has the faces and the ghost count of "dddd" (its ring is never counted)."""
    y, t, x = y.to(dtype), t.to(dtype), x.to(dtype)
    mu_u, sg_u, mu_f, sg_f, mu_t, sg_t = [float(torch.as_tensor(v).to(dtype)) for v in stats]
    n = y.shape[-1]
    theta = sg_t * x[:, 1:2] + mu_t
    f = sg_f * x[:, 2:3] + mu_f
    kinds = [int(v) for v in torch.as_tensor(kind).reshape(-1)]
    sub = torch.tensor(kinds).reshape(-1, 1, 1, 1) != 0
    ih2 = torch.where(sub, torch.tensor(float(inv_h2[1]), dtype=dtype), torch.tensor(float(inv_h2[0]), dtype=dtype))
    inner = torch.zeros(1, 1, n, n, dtype=torch.bool)
    inner[..., 1:-1, 1:-1] = True
    m = (~sub | inner).to(dtype)                      # kind 0: every node; kind 1: the interior
    th_np = theta.detach().numpy()
    faces = [B._cut(*D._faces(th_np[b], mean), "dddd" if kinds[b] else bc) for b in range(len(kinds))]
    cE, cW, cS, cN = (torch.from_numpy(np.stack([fc[i] for fc in faces])) for i in range(4))
    assert cE.dtype == dtype
    k_d = torch.stack([dirichlet_ghost_count(n, "dddd" if kd else bc, dtype) for kd in kinds]).reshape(-1, 1, n, n)
    p = torch.nn.functional.pad(y, (1, 1, 1, 1))
    a = (cE * (p[..., 1:-1, 2:] - y) + cW * (p[..., 1:-1, :-2] - y)) + \
        (cS * (p[..., 2:, 1:-1] - y) + cN * (p[..., :-2, 1:-1] - y))
    r = ((sg_u * a + mu_u * (-k_d * theta)) * ih2 - f) / sg_f
    M = m.sum()
    pde = (m * r * r).sum() / M
    mse = ((y - t) ** 2).mean()
    return {"total": mse + weight * pde, "mse": mse, "pde": pde, "r": r, "m": m, "theta": theta, "q": m * r,
            "M": float(M)}
