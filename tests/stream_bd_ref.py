"""numpy / torch restatements of boundary data in the sample stream and the physics loss (ABI 23, extended:
srpde_stream_walls, srpde_physics_loss_div_fwd_bd).  Built on tests/div_bd_ref.py, tests/div_bc_ref.py and
tests/div_bc_smoother_ref.py.

TEST INFRASTRUCTURE ONLY: nothing here is imported from the product, and the product imports nothing from here.

Walls.  ``words`` are the raw Philox words of field 2, [B, 8, 4] uint32 (srpde_stream_raw, or test_online_host's numpy
Philox): element e belongs to side e >> 1 and gives the coefficients of the cosine modes m = 2 (e & 1) (words 0, 1) and
m + 1 (words 2, 3), c = (amp * (2 u - 1)) / (m + 1) -- every operation one rounded numpy pass, so ``wall_coefficients``
is the device's bits.  ``wall_values`` evaluates the four modes in extended precision (the cosine's argument reduced in
integers first): the value the device's fp64 result is compared with.

Loss.  ``restatement_div_bd`` is div_bc_smoother_ref.restatement_div_bc with the affine term of div_bd_ref.apply on the
kind-0 samples, in the header's order:
    r = ((((u_std a(y) + u_mean (-k_d theta)) + beta) ih2 - f) + Q inv_h) / f_std
"""
from __future__ import annotations

import numpy as np
import torch

import div_bc_ref as BC
import div_bd_ref as BD
import poisson_div_ref as D
from div_bc_smoother_ref import INV_H2, dirichlet_ghost_count

FIELD_WALLS = 2
MODES = 4


def uniform53(a, b):
    """The header's [0, 1) double of an ordered pair of words."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (((a << np.uint64(32)) | b) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def wall_coefficients(words, bc, amps):
    """[B, 4 sides, 4 modes] fp64 from words [B, 8, 4] uint32; ``bc`` a 4-string, ``amps`` = (g_amp, q_amp)."""
    words = np.asarray(words, dtype=np.uint32)
    assert words.shape[1:] == (8, 4), words.shape
    c = np.empty((words.shape[0], 4, MODES))
    for e in range(8):
        side, m = e >> 1, 2 * (e & 1)
        amp = np.float64(amps[1] if bc[side] == "n" else amps[0])
        for j, (a, b) in enumerate(((0, 1), (2, 3))):
            u = uniform53(words[:, e, a], words[:, e, b])
            c[:, side, m + j] = (amp * (2.0 * u - 1.0)) / np.float64(m + j + 1)
    return c


def mode_table(n, dtype=np.longdouble):
    """[4 modes, n]: cos(pi m k / (n - 1)), the argument reduced in integers, evaluated in ``dtype``."""
    m = np.arange(MODES)[:, None]
    k = np.arange(n)[None, :]
    r = (m * k) % (2 * (n - 1))
    return np.cos(_pi(dtype) * r.astype(dtype) / dtype(n - 1))


def _pi(dtype):
    """pi in ``dtype`` (np.pi is a double: for the extended type it is taken from 4 atan(1) in that type)."""
    return dtype(4) * np.arctan(dtype(1))


def wall_values(coef, n):
    """(values [B, 4, n] in extended precision, sum |c| [B, 4, 1]): (c0 cos0 + c1 cos1) + (c2 cos2 + c3 cos3)."""
    tab = mode_table(n)
    c = coef.astype(np.longdouble)[..., None]                      # [B, 4, 4, 1]
    t = c * tab[None, None]
    return (t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3]), np.abs(coef).sum(-1, keepdims=True)


def wall_values_exact_grid(coef):
    """n = 3: the cosines are exactly 1, 0 and -1, so every operation of the device's sum is reproduced bit for bit in
    fp64: [B, 4, 3]."""
    tab = np.array([[1.0, 1.0, 1.0], [1.0, 0.0, -1.0], [1.0, -1.0, 1.0], [1.0, 0.0, -1.0]])    # cos(pi m k / 2) [m, k]
    t = coef[..., None] * tab[None, None]
    return (t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3])


# ---- the loss -----------------------------------------------------------------------------------------------------
def _affine_parts(theta, bd, mean, bc):
    """(beta, Q, on) [n, n] fp64 of one problem: the ghost faces' terms theta_a * g summed (E + W) + (S + N), the flux
    sum (qE + qW) + (qS + qN) and the mask of the nodes with a flux-side ghost face."""
    n = theta.shape[-1]
    cE, cW, cS, cN = BC._cut(*D._faces(theta, mean), bc)
    p = BD.pad(np.zeros((n, n)), bd, bc)
    gE, gW, gS, gN = BD._neighbours(p)
    inside = np.zeros((n + 2, n + 2), dtype=bool)
    inside[1:-1, 1:-1] = True
    iE, iW, iS, iN = BD._neighbours(inside)
    beta = (np.where(iE, 0.0, cE * gE) + np.where(iW, 0.0, cW * gW)) + \
           (np.where(iS, 0.0, cS * gS) + np.where(iN, 0.0, cN * gN))
    q, on = BD.flux(np.zeros((n, n)), bd, bc)
    return beta, q, on


def restatement_div_bd(y, t, x, kind, stats, weight, inv_h2=INV_H2, mean="harmonic", bc="dddd", bd=None,
                       dtype=torch.float64):
    """The loss of srpde_physics_loss_div_fwd_bd.  y, t [B, 1, n, n], x [B, 3, n, n], kind [B], stats 6 values, bd
    [B, 4, n] or [4, n] in raw units (None: zeros) -> dict(total, mse, pde, r, m, theta, q, M, beta, flux) in ``dtype``;
    differentiable in y.  Pattern and data apply to the kind-0 samples; a kind-1 sample's row of bd is never read."""
    y, t, x = y.to(dtype), t.to(dtype), x.to(dtype)
    mu_u, sg_u, mu_f, sg_f, mu_t, sg_t = [float(torch.as_tensor(v).to(dtype)) for v in stats]
    B, n = y.shape[0], y.shape[-1]
    pat = BD.pattern(bc)
    theta = sg_t * x[:, 1:2] + mu_t
    f = sg_f * x[:, 2:3] + mu_f
    kinds = [int(v) for v in torch.as_tensor(kind).reshape(-1)]
    sub = torch.tensor(kinds).reshape(-1, 1, 1, 1) != 0
    ih2 = torch.where(sub, torch.tensor(float(inv_h2[1]), dtype=dtype), torch.tensor(float(inv_h2[0]), dtype=dtype))
    inv_h = float(np.float32(np.sqrt(np.float64(np.float32(inv_h2[0])))))
    inner = torch.zeros(1, 1, n, n, dtype=torch.bool)
    inner[..., 1:-1, 1:-1] = True
    m = (~sub | inner).to(dtype)
    th_np = theta.detach().numpy()
    faces = [BC._cut(*D._faces(th_np[b], mean), "dddd" if kinds[b] else pat) for b in range(B)]
    cE, cW, cS, cN = (torch.from_numpy(np.stack([fc[i] for fc in faces])) for i in range(4))
    k_d = torch.stack([dirichlet_ghost_count(n, "dddd" if kd else pat, dtype) for kd in kinds]).reshape(-1, 1, n, n)
    beta, flux = np.zeros((B, 1, n, n)), np.zeros((B, 1, n, n))
    if bd is not None:
        bd_np = np.asarray(torch.as_tensor(bd).detach().double())
        bd_np = np.broadcast_to(bd_np if bd_np.ndim == 3 else bd_np[None], (B, 4, n))
        for b in range(B):
            if not kinds[b]:
                bt, q, on = _affine_parts(th_np[b, 0], bd_np[b], mean, pat)
                beta[b, 0], flux[b, 0] = bt, np.where(on, q * inv_h, 0.0)
    beta, flux = torch.from_numpy(beta).to(dtype), torch.from_numpy(flux).to(dtype)
    p = torch.nn.functional.pad(y, (1, 1, 1, 1))
    a = (cE * (p[..., 1:-1, 2:] - y) + cW * (p[..., 1:-1, :-2] - y)) + \
        (cS * (p[..., 2:, 1:-1] - y) + cN * (p[..., :-2, 1:-1] - y))
    r = ((((sg_u * a + mu_u * (-k_d * theta)) + beta) * ih2 - f) + flux) / sg_f
    M = m.sum()
    pde = (m * r * r).sum() / M
    mse = ((y - t) ** 2).mean()
    return {"total": mse + weight * pde, "mse": mse, "pde": pde, "r": r, "m": m, "theta": theta, "q": m * r,
            "M": float(M), "beta": beta, "flux": flux}


def dense_loss(y, t, x, kind, stats, weight, inv_h2, mean, bc, bd):
    """The same loss from the dense matrices: on a kind-0 sample r = (A_bd u - f) / f_std with A_bd u = D_bc u + b from
    div_bc_ref.dense and div_bd_ref.affine and u = u_std y + u_mean -- no split form, no face sums on y -- and on a
    kind-1 sample the "dddd" matrix on the interior nodes.  torch fp64, differentiable in y: (total, mse, pde)."""
    y, t, x = y.double(), t.double(), x.double()
    mu_u, sg_u, mu_f, sg_f, mu_t, sg_t = [float(v) for v in torch.as_tensor(stats).double()]
    B, n = y.shape[0], y.shape[-1]
    pat = BD.pattern(bc)
    base = float((n - 1) ** 2)                                      # the inv_h2 that dense() and affine() are built with
    bd_np = np.zeros((B, 4, n)) if bd is None else np.asarray(torch.as_tensor(bd).double())
    bd_np = np.broadcast_to(bd_np if bd_np.ndim == 3 else bd_np[None], (B, 4, n))
    num, cnt = 0.0, 0
    for b in range(B):
        th = (sg_t * x[b, 1] + mu_t).numpy()
        f = sg_f * x[b, 2] + mu_f
        u = (sg_u * y[b, 0] + mu_u).reshape(-1)
        if int(kind[b]):
            A = torch.from_numpy(BC.dense(th, mean, "dddd") * (inv_h2[1] / base))
            r = ((A @ u).reshape(n, n) - f)[1:-1, 1:-1] / sg_f
        else:
            A = torch.from_numpy(BC.dense(th, mean, pat) * (inv_h2[0] / base))
            aff = torch.from_numpy(BD.affine(th, bd_np[b], mean, pat, inv_h2=inv_h2[0]))
            r = ((A @ u).reshape(n, n) + aff - f) / sg_f
        num = num + (r * r).sum()
        cnt += r.numel()
    pde = num / cnt
    mse = ((y - t) ** 2).mean()
    return mse + weight * pde, mse, pde
