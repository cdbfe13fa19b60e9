"""HIP MSE loss (reference ``nn.MSELoss()``, src/train_enhanced.py:70, :307).

``mse_loss`` keeps the loss scalar on the device (no host sync); its backward is the
HIP kernel dy = 2 (y - t) / numel * grad_out.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hipops as H
from .poisson import check_bc, face_mean_arg


def _bc_arg(form, bc):
    """The side mask of ``bc`` (poisson.check_bc) for the divergence form's loss, None for none."""
    mask = check_bc(bc)
    if mask is not None and form != "divergence":
        raise ValueError('bc belongs to form="divergence": the pointwise residual has the zero ghost ring')
    return mask


def _bd_arg(form, data, B, n):
    """``bc_data`` of the loss as the kernel takes it: None, or the data checked (ValueErrors that need no device) and
    brought to [B or 1, 4, n] fp32, contiguous -- cast once, here."""
    if data is None:
        return None
    if form != "divergence":
        raise ValueError('bc_data belongs to form="divergence": the pointwise residual has the zero ghost ring')
    if not isinstance(data, torch.Tensor) or data.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"bc_data must be a float32 or float64 tensor, got "
                         f"{data.dtype if isinstance(data, torch.Tensor) else type(data).__name__}")
    if data.dim() not in (2, 3) or tuple(data.shape[-2:]) != (4, n) or (data.dim() == 3 and data.shape[0] not in (1, B)):
        raise ValueError(f"bc_data must be [4, n], [1, 4, n] or [B, 4, n] with n={n} B={B}, got {tuple(data.shape)}")
    data = data.detach()
    if data.dim() == 2:
        data = data.unsqueeze(0)
    return data.float().contiguous()


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, t):
        y = y.contiguous()
        t = t.contiguous()
        ctx.save_for_backward(y, t)
        return H.mse_fwd(y, t)

    @staticmethod
    def backward(ctx, gout):
        y, t = ctx.saved_tensors
        dy = H.mse_bwd(y, t, gout.contiguous())
        return dy, None


def mse_loss(y: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    if y.shape != t.shape:
        raise ValueError(f"mse_loss: shape mismatch {tuple(y.shape)} vs {tuple(t.shape)}")
    if not y.is_cuda or y.dtype != torch.float32:
        raise RuntimeError("mse_loss: HIP path needs float32 ROCm tensors (no CPU fallback)")
    return _MSEFn.apply(y, t)


class MSELoss(nn.Module):
    """Drop-in for nn.MSELoss() with reduction='mean'."""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:  # noqa: A002
        return mse_loss(input, target)


# 1 / h^2 of the training samples: a whole-domain solve on 40^2 nodes, a 40^2 crop of a solve on 80^2 nodes
DEFAULT_INV_H2 = (39.0 ** 2, 79.0 ** 2)


class _PhysicsMSEFn(torch.autograd.Function):
    """(terms [3] = (total, mse, pde)) of srpde_physics_loss_fwd; only terms[0] carries a gradient.  The forward
    pass emits the gradient for grad_out = 1 (when one is wanted), the backward pass scales it."""

    @staticmethod
    def forward(ctx, y, t, x, kind, stats, weight, inv_h2, want_grad, face_mean=None, bc=None, bd=None):
        terms, unit = H.physics_loss_fwd(y, t, x, kind, stats, weight, inv_h2, want_grad, face_mean, bc, bd)
        ctx.unit = unit
        return terms

    @staticmethod
    def backward(ctx, gterms):
        if ctx.unit is None:
            raise RuntimeError("physics_mse_loss: backward through a loss evaluated without a gradient")
        dy = H.physics_loss_bwd(ctx.unit, gterms.contiguous())   # reads gterms[0], the total's grad_out
        return dy, None, None, None, None, None, None, None, None, None, None


def physics_loss_terms(y, t, x, kind, stats, weight, inv_h2=DEFAULT_INV_H2, form="pointwise", face_mean="harmonic",
                       bc=None, bc_data=None):
    """The device tensor (mse + weight * pde, mse, pde) behind ``physics_mse_loss``; differentiable through its
    first element only (the other two are reports of the same pass; ``bc_data`` gets no gradient)."""
    mean = face_mean_arg(form, face_mean)
    mask = _bc_arg(form, bc)
    if y.shape != t.shape:
        raise ValueError(f"physics_mse_loss: shape mismatch {tuple(y.shape)} vs {tuple(t.shape)}")
    if y.dim() != 4 or y.shape[1] != 1 or y.shape[2] != y.shape[3]:
        raise ValueError(f"physics_mse_loss: fields must be [B, 1, n, n], got {tuple(y.shape)}")
    B, _, n, _ = y.shape
    bd = _bd_arg(form, bc_data, B, n)
    if tuple(x.shape) != (B, 3, n, n):
        raise ValueError(f"physics_mse_loss: the model input must be [{B}, 3, {n}, {n}], got {tuple(x.shape)}")
    if tuple(kind.shape) != (B,) or kind.dtype != torch.int32:
        raise ValueError(f"physics_mse_loss: kind must be [{B}] int32, got {tuple(kind.shape)} {kind.dtype}")
    if stats.numel() != 6:
        raise ValueError("physics_mse_loss: stats = (u_mean, u_std, f_mean, f_std, theta_mean, theta_std)")
    if not 3 <= n <= 64:
        raise ValueError(f"physics_mse_loss: 3 <= n <= 64, got n={n}")
    if len(inv_h2) != 2:
        raise ValueError("physics_mse_loss: inv_h2 = (1 / h^2 of kind 0, 1 / h^2 of kind 1)")
    for v in (y, t, x, kind, stats):
        if not v.is_cuda:
            raise RuntimeError("physics_mse_loss: HIP path needs ROCm tensors (no CPU fallback)")
    if not all(v.dtype == torch.float32 for v in (y, t, x, stats)):
        raise RuntimeError("physics_mse_loss: HIP path needs float32 ROCm tensors (no CPU fallback)")
    if bd is not None and bd.device != y.device:
        raise RuntimeError("physics_mse_loss: bc_data must be on the fields' device (no CPU fallback)")
    want_grad = torch.is_grad_enabled() and y.requires_grad
    return _PhysicsMSEFn.apply(y.contiguous(), t.contiguous(), x.contiguous(), kind.contiguous(),
                               stats.contiguous(), float(weight), (float(inv_h2[0]), float(inv_h2[1])), want_grad,
                               mean, mask, *(() if bd is None else (bd,)))


def physics_mse_loss(y, t, x, kind, stats, weight, inv_h2=DEFAULT_INV_H2, form="pointwise",
                     face_mean="harmonic", bc=None, bc_data=None) -> torch.Tensor:
    """mean((y - t)^2) + weight * L_pde: the MSE plus the mean squared residual of the discrete equation
    theta * L u = f that the samples solve, evaluated from the normalised fields (include/srpde.h,
    srpde_physics_loss_fwd).  x: the model input (theta and f are its channels 1 and 2), kind [B] int32: 0 for a
    whole-domain sample, 1 for a crop; stats: the dataset's six statistics on the device.
    ``form="divergence"``: the residual of div(theta grad u) = f with ``face_mean`` on the faces instead
    (srpde_physics_loss_div_fwd), for samples that solve the conservative problem.  ``bc`` (poisson.check_bc, e.g.
    ``"ddnn"``), with that form: the whole-domain (kind 0) samples solve the problem with those zero-flux sides
    (srpde_physics_loss_div_fwd_bc); crops count interior nodes only and are scored as without it.  ``bc_data``, with
    that form: the whole-domain samples' boundary data in RAW units (poisson.bc_data's layout: [B, 4, n], or [1, 4, n] /
    [4, n] shared by the batch; fp32, or fp64 cast to fp32 once) -- the ghost value g beyond a "d" side (every side
    without ``bc``), the outward flux q through an "n" side, what ``solve_div(bc_data=)`` solved with -- so that the
    residual is that of A u = f with those walls (srpde_physics_loss_div_fwd_bd).  A crop's row is never read.  The
    data gets no gradient.  None (default) makes the calls above."""
    return physics_loss_terms(y, t, x, kind, stats, weight, inv_h2, form, face_mean, bc, bc_data)[0]


class PhysicsMSELoss(nn.Module):
    """``criterion(outputs, targets, inputs, kind)``: MSE + weight * PDE residual.  ``needs_inputs`` tells
    train_model to pass the batch's inputs and kinds; ``last_terms`` holds the last call's (total, mse, pde) as a
    device tensor (no host sync).  ``bc_data=True`` (with ``form="divergence"``): the samples' walls carry data,
    ``needs_bd`` tells train_model to pass the batch's boundary data as a fifth argument, and a call without it is
    refused -- scoring such samples against zero walls would report a residual for the exact solution."""

    needs_inputs = True
    needs_bd = False

    def __init__(self, weight: float, stats: torch.Tensor, inv_h2=DEFAULT_INV_H2, form: str = "pointwise",
                 face_mean: str = "harmonic", bc=None, bc_data: bool = False):
        super().__init__()
        if bc_data and form != "divergence":
            raise ValueError('bc_data belongs to form="divergence": the pointwise residual has the zero ghost ring')
        self.needs_bd = bool(bc_data)
        if weight < 0:
            raise ValueError("PhysicsMSELoss: weight >= 0")
        face_mean_arg(form, face_mean)
        _bc_arg(form, bc)
        self.form, self.face_mean, self.bc = form, face_mean, bc
        self.weight = float(weight)
        self.inv_h2 = (float(inv_h2[0]), float(inv_h2[1]))
        self.register_buffer("stats", stats.detach().float().contiguous().clone(), persistent=False)
        self.last_terms = None

    def forward(self, input, target, x, kind, bd=None):  # noqa: A002
        if self.needs_bd and bd is None:
            raise ValueError("PhysicsMSELoss(bc_data=True) needs the batch's boundary data: criterion(outputs, targets, "
                             "inputs, kind, bd)")
        terms = physics_loss_terms(input, target, x, kind, self.stats, self.weight, self.inv_h2, self.form,
                                   self.face_mean, self.bc, bd)
        self.last_terms = terms.detach()
        return terms[0]
