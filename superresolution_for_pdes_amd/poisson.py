"""Batched on-device Poisson solve: the HIP replacement of scipy spsolve on the 5-point
operator (reference src/data_generation.py:35-104, src/enhanced_data_generation.py:47-68).

``solve_batched(f, theta)`` solves theta * Lap_h(u) = f for B problems of size n x n
(h = 1/(n-1), all n^2 nodes unknown, zero ghost ring -- exactly diag(theta) @ L of the
reference) as the SPD system (-L) u = -f/theta by matrix-free CG in fp64:
  * n <= 128 : one workgroup per problem, direction vector in LDS (one launch);
  * n  > 128 : grid CG as cooperative launches (srpde_poisson_coop_problems(n) problems each):
               two grid barriers per iteration instead of two launches, convergence decided on
               the device -- stream-ordered, no host sync.
Both go through the single C entry ``srpde_poisson_cg_batched`` (include/srpde.h), which a
non-Python caller binds the same way.

``solve_direct(f, theta)`` / ``solve_batched(..., method="dst")`` solve the same system exactly by the
2-D sine transform (csrc/poisson_dst.hip): L = (T (x) I + I (x) T) / h^2 is diagonalised by the symmetric
orthogonal sine matrix S, so u = S ((S (f / theta) S) o h^2 / (lam_i + lam_j)) S -- four dense fp64 MFMA
products per problem, no iteration, any n.  Opt-in: every default stays CG.

All of the above solve the POINTWISE form diag(theta) L u = f, which is L u = f / theta.  ``apply_div`` /
``solve_div`` / ``solve_batched(..., form="divergence")`` are the DIVERGENCE form div(theta grad u) = f
(csrc/poisson_div.hip): the conservative variable-coefficient operator with arithmetic or harmonic face means, solved
by CG preconditioned with the sine-transform solve of L, whose iteration count is bounded by theta_max / theta_min and
does not grow with n.  Opt-in as well: every default stays pointwise.  ``apply_div`` and ``solve_div`` are
differentiable in their fields and in theta (the operator is symmetric, so the solve's adjoint is the same solve;
``div_theta_grad`` is the one local pass the theta gradient needs), and ``solve_div(..., u0=)`` starts the iteration
from a guess.  ``shift=`` on both makes the operator div(theta grad u) - sigma u, preconditioned with the
sine-transform solve of L - sigma_p I at the same condition bound, and ``diffuse`` steps u_t = div(theta grad u) - f
implicitly with it (backward Euler or Crank-Nicolson), each solve warm-started from the previous state.  ``bc=`` on
all of these makes chosen sides of the grid zero-flux (insulated, du/dn = 0) instead of the zero ghost ring: a 4-string
of "d" / "n" for (row 0, row n - 1, column 0, column n - 1), preconditioned with the separable solve of the
constant-coefficient operator with the same sides at the same condition bound; None (default) and "dddd" are today's
calls.  ``bc_data=`` (``bc_data()``) gives the sides values: u = g on a "d" side (the ghost ring holds g instead of 0),
a prescribed outward flux q = theta du/dn through an "n" side -- an affine extension A u = D u - sigma u + b(data,
theta) with the same iteration, preconditioner and bound, a stop rule on |f - b| (so Laplace's equation, f = 0 with
g != 0, iterates) and a gradient in the data; None (default) makes exactly today's calls.  ``face_flux`` returns the
fluxes theta du/dx and theta du/dy of that discretisation on the faces, ``wall_flux`` their integral over each of the
four walls (the discrete divergence theorem: the four sum to h^2 sum(apply_div)), and ``effective_coefficient`` the
homogenised coefficient of a theta field from a unit-gradient solve and its wall fluxes; all three are differentiable.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, query, stream_ptr

DEFAULT_RTOL = 1e-12


def _dev_f64(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def forcing_batched(k12, n: int, device="cuda"):
    """f[b] = sin(2 pi k1_b X) sin(2 pi k2_b Y) on linspace(0,1,n)^2 (data_generation.py:60-77)."""
    k = _dev_f64(k12, device).reshape(-1, 2).contiguous()
    out = torch.empty(k.shape[0], n, n, dtype=torch.float64, device=device)
    if k.shape[0] == 0:      # an empty rank shard (shard_range with n < world): nothing to launch
        return out
    call("srpde_forcing_batched", k.data_ptr(), k.shape[0], n, out.data_ptr(), stream_ptr())
    return out


class GridBarrierAbort(RuntimeError):
    """A cooperative grid-CG launch gave up at a grid barrier (iters = -1): its u is not a solution."""


SOLVERS = ("cg", "dst")
_dst_plans = {}   # (n, device) -> the plan buffer of srpde_poisson_dst_plan (S [n][n], lam [n])


def check_solver(solver: str) -> str:
    if solver not in SOLVERS:
        raise ValueError(f"unknown Poisson solver {solver!r}: one of {SOLVERS}")
    return solver


def dst_plan(n: int, device="cuda"):
    """The sine matrix and eigenvalues for n on ``device``, built on first use (one launch) and kept."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    key = (int(n), dev)
    plan = _dst_plans.get(key)
    if plan is None:
        nbytes = int(query("srpde_poisson_dst_plan_size", int(n)))
        if nbytes == 0:
            raise ValueError(f"no sine-transform plan for n={n}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"the sine-transform plan for n={n} must exist before stream capture: call "
                               "poisson.dst_plan(n) first")
        plan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("srpde_poisson_dst_plan", int(n), plan.data_ptr(), nbytes, stream_ptr(dev))
        _dst_plans[key] = plan
    return plan


def _dst_ws(B, n, device):
    ws_bytes = int(query("srpde_poisson_dst_workspace_size", B, n))
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device), ws_bytes


def solve_direct(f, theta, device="cuda"):
    """u[B, n, n] (float64, on device) with theta*Lap(u) = f per problem, by the sine transform: exact up to
    rounding, cost fixed by the shape, stream-ordered with no host sync (capturable once dst_plan(n) exists)."""
    f = _dev_f64(f, device)
    theta = _dev_f64(theta, device)
    if f.dim() == 2:
        f, theta = f.unsqueeze(0), theta.unsqueeze(0)
    if theta.shape != f.shape:
        theta = theta.expand_as(f).contiguous()
    B, n, n2 = f.shape
    if n != n2:
        raise ValueError("square grids only")
    u = torch.empty_like(f)
    if B == 0:
        return u
    plan = dst_plan(n, f.device)
    ws, ws_bytes = _dst_ws(B, n, f.device)
    call("srpde_poisson_dst_batched", f.data_ptr(), theta.data_ptr(), u.data_ptr(), B, n, plan.data_ptr(),
         plan.numel(), ws.data_ptr(), ws_bytes, stream_ptr(f.device))
    return u


def dst2(x, device="cuda"):
    """y = S x S per field: the orthonormal 2-D DST-I of x [B, n, n] (or [n, n]); its own inverse."""
    x = _dev_f64(x, device)
    single = x.dim() == 2
    if single:
        x = x.unsqueeze(0)
    B, n, n2 = x.shape
    if n != n2:
        raise ValueError("square grids only")
    y = torch.empty_like(x)
    if B:
        plan = dst_plan(n, x.device)
        ws, ws_bytes = _dst_ws(B, n, x.device)
        call("srpde_poisson_dst_apply", x.data_ptr(), y.data_ptr(), B, n, plan.data_ptr(), plan.numel(),
             ws.data_ptr(), ws_bytes, stream_ptr(x.device))
    return y[0] if single else y


FORMS = ("pointwise", "divergence")
FACE_MEANS = ("arithmetic", "harmonic")


def check_form(form: str) -> str:
    if form not in FORMS:
        raise ValueError(f"unknown operator form {form!r}: one of {FORMS}")
    return form


def check_face_mean(face_mean: str) -> int:
    """The C entries' face_mean argument: 0 arithmetic, 1 harmonic."""
    if face_mean not in FACE_MEANS:
        raise ValueError(f"unknown face mean {face_mean!r}: one of {FACE_MEANS}")
    return FACE_MEANS.index(face_mean)


def face_mean_arg(form: str, face_mean: str):
    """The face_mean argument of hipops.pde_relax / hipops.physics_loss_fwd: None for the pointwise form (which takes
    no mean: anything but the default is refused), 0 / 1 for the divergence form's arithmetic / harmonic mean."""
    mean = check_face_mean(face_mean)
    if check_form(form) == "divergence":
        return mean
    if face_mean != "harmonic":
        raise ValueError('face_mean belongs to form="divergence"')
    return None


def check_bc(bc):
    """The side mask of the C entries' bc argument from a pattern such as "ddnn": one of "d" (the zero ghost ring) or
    "n" (zero flux) for (row 0 side, row n - 1 side, column 0 side, column n - 1 side), bit i set for an "n" at place
    i.  None and "dddd" give None: the entries without a mask, today's calls."""
    if bc is None:
        return None
    if not isinstance(bc, str) or len(bc) != 4 or any(c not in "dn" for c in bc):
        raise ValueError(f'bc must be None or four of "d" / "n" for (row 0, row n-1, column 0, column n-1), got {bc!r}')
    mask = sum(1 << i for i, c in enumerate(bc) if c == "n")
    return mask or None


_sep_plans = {}   # (n, mask, device) -> the plan buffer of srpde_poisson_sep_plan


def sep_plan(n: int, bc, device="cuda"):
    """The eigenvector matrices and eigenvalues of the separable solve for n and the pattern ``bc`` (a 4-string or a
    mask) on ``device``, built on first use (two launches) and kept, like ``dst_plan``."""
    mask = int(bc) if isinstance(bc, int) else (check_bc(bc) or 0)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    key = (int(n), mask, dev)
    plan = _sep_plans.get(key)
    if plan is None:
        nbytes = int(query("srpde_poisson_sep_plan_size", int(n), mask))
        if nbytes == 0:
            raise ValueError(f"no separable plan for n={n}, bc={bc!r}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"the separable plan for n={n}, bc={bc!r} must exist before stream capture: call "
                               "poisson.sep_plan(n, bc) first")
        plan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("srpde_poisson_sep_plan", int(n), mask, plan.data_ptr(), nbytes, stream_ptr(dev))
        _sep_plans[key] = plan
    return plan


SIDES = ("row0", "row1", "col0", "col1")   # the order of the mask's bits and of boundary data's second axis


def bc_data(n: int, bc=None, row0=0.0, row1=0.0, col0=0.0, col1=0.0, B: int = 1, device="cuda"):
    """Boundary data for ``bc_data=``: a [B, 4, n] fp64 tensor on ``device`` from one scalar, [n] or [B, n] per side,
    the sides in the pattern's order (row 0, row n - 1, column 0, column n - 1).  Entry k of a row side belongs to
    column k, entry k of a column side to row k; a corner node receives data from both of its sides.  On a "d" side of
    ``bc`` (every side for None) the entry is the value g of the ghost node one h beyond the edge node, on an "n" side
    the outward flux q = theta du/dn through the face half a cell beyond it.  The layout does not depend on ``bc``,
    which is only checked.  Built with torch operations, so a side given as a tensor that requires grad receives
    one."""
    check_bc(bc)
    n, B = int(n), int(B)
    if n < 2 or B < 1:
        raise ValueError(f"bc_data: n >= 2 and B >= 1, got n={n} B={B}")
    rows = []
    for name, v in zip(SIDES, (row0, row1, col0, col1)):
        if not isinstance(v, torch.Tensor):
            a = np.asarray(v, dtype=np.float64)
            if not np.isfinite(a).all():
                raise ValueError(f"bc_data: {name} is not finite")
            v = torch.from_numpy(np.array(a))           # (ascontiguousarray would make a scalar 1-d)
        if v.dim() > 2 or (v.dim() >= 1 and v.shape[-1] != n) or (v.dim() == 2 and v.shape[0] not in (1, B)):
            raise ValueError(f"bc_data: {name} must be a scalar, [n] or [B, n] with n={n} B={B}, got {tuple(v.shape)}")
        rows.append(v.to(device=device, dtype=torch.float64).expand(B, n))
    return torch.stack(rows, dim=1).contiguous()


def _bd_check(data, field):
    """The refusals of ``bc_data=`` against the field it goes with ([n, n] or [B, n, n], anything with a shape), as
    ValueErrors before anything touches a device: shape, dtype, non-finite values.  Data that already lives on a device
    is not read back (that would be a host sync): its values are the caller's."""
    if data is None:
        return
    shape = tuple(field.shape) if hasattr(field, "shape") else np.shape(field)
    n, B = int(shape[-1]), int(shape[0]) if len(shape) == 3 else 1
    if not isinstance(data, (torch.Tensor, np.ndarray)):
        raise ValueError(f"bc_data must be a tensor or an array (poisson.bc_data), got {type(data).__name__}")
    if tuple(data.shape)[-2:] != (4, n) or len(data.shape) not in (2, 3) or (len(data.shape) == 3 and
                                                                             data.shape[0] not in (1, B)):
        raise ValueError(f"bc_data must be [4, n], [1, 4, n] or [B, 4, n] with n={n} B={B}, got {tuple(data.shape)}")
    if data.dtype not in (torch.float64, np.float64):
        raise ValueError(f"bc_data must be float64, got {data.dtype}")
    if isinstance(data, np.ndarray):
        if not np.isfinite(data).all():
            raise ValueError("bc_data is not finite")
    elif data.device.type == "cpu" and not bool(torch.isfinite(data).all()):
        raise ValueError("bc_data is not finite")


def _bd_fields(data, field, device):
    """``bc_data=`` as the C entries take it: a contiguous [Bd, 4, n] fp64 tensor on ``device``, Bd in (1, B), checked
    against the prepared ``field`` [B, n, n] (``_bd_check``); None stays None."""
    if data is None:
        return None
    _bd_check(data, field)
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(np.ascontiguousarray(data))
    data = data.to(device)
    if data.dim() == 2:
        data = data.unsqueeze(0)
    return data.contiguous()


def _bd_stride(bd, B: int) -> int:
    """The C entries' bd_stride: 4 n doubles between problems, 0 for one [4][n] shared by all."""
    return 4 * bd.shape[-1] if bd.shape[0] == B else 0


def _bd_grad(lam, theta, inv_h2: float, bc, bd, scale: float = 1.0):
    """scale * srpde_div_bd_grad(lam), summed over the batch for shared data: the gradient in ``bd``'s shape."""
    B, n = lam.shape[0], lam.shape[-1]
    out = torch.empty(B, 4, n, dtype=torch.float64, device=lam.device)
    if B:
        call("srpde_div_bd_grad", lam.data_ptr(), theta.data_ptr(), out.data_ptr(), B, n, inv_h2, bc or 0,
             stream_ptr(lam.device))
    if bd.shape[0] != B:
        out = out.sum(0, keepdim=True)
    return out if scale == 1.0 else out * scale


class NotConverged(RuntimeError):
    """solve_div left problems above their tolerance (maxit reached)."""


def _div_fields(a, theta, device):
    a, theta = _dev_f64(a, device), _dev_f64(theta, device)
    if a.dim() == 2:
        a = a.unsqueeze(0)
        if theta.dim() == 2:
            theta = theta.unsqueeze(0)
    if theta.shape != a.shape:
        theta = theta.expand_as(a).contiguous()
    B, n, n2 = a.shape
    if n != n2:
        raise ValueError("square grids only")
    return a, theta, B, n


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def check_shift(shift, what: str = "shift") -> float:
    """A shift sigma of D_theta - sigma I (or of the preconditioner L - sigma_p I): finite and >= 0."""
    shift = float(shift)
    if not (shift >= 0.0 and np.isfinite(shift)):
        raise ValueError(f"{what} must be finite and >= 0, got {shift}")
    return shift


def pcg_iterations(theta_lo: float, theta_hi: float, tol: float = 1e-12) -> int:
    """The smallest k with 2 ((sqrt(c) - 1) / (sqrt(c) + 1))^k <= tol for c = theta_hi / theta_lo: CG's bound at the
    condition number that theta_max / theta_min bounds for the sine-preconditioned operator -- D_theta, and
    D_theta - sigma I with the preconditioner L - (sigma / theta_g) I for any sigma >= 0.  A fixed
    iteration count for ``solve_div(check_every=0)`` and ``diffuse(pcg_iters=)``; add a margin of a few."""
    lo, hi = float(theta_lo), float(theta_hi)
    if not 0.0 < lo <= hi:
        raise ValueError(f"theta range ({theta_lo}, {theta_hi}): 0 < lo <= hi")
    s = (hi / lo) ** 0.5
    rho = (s - 1.0) / (s + 1.0)
    k = 0
    while 2.0 * rho ** k > tol:
        k += 1
    return k


def precond_shift_for(theta, shift: float) -> float:
    """sigma_p = shift / theta_g with theta_g = sqrt(theta_min theta_max) over the whole batch: the default shift of
    the preconditioner L - sigma_p I.  ONE HOST READ of two device scalars, so not under stream capture."""
    if shift == 0.0:
        return 0.0
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("precond_shift=None reads theta's range back (a host sync): give precond_shift under "
                           "stream capture")
    lo, hi = torch.stack(torch.aminmax(theta.detach())).tolist()       # the one read
    if not 0.0 < lo <= hi:
        raise ValueError(f"theta must be positive (range {lo:g} .. {hi:g})")
    return shift / float(np.sqrt(lo * hi))


def _apply_div(u, theta, mean: int, inv_h2: float, shift: float = 0.0, bc=None, bd=None):
    """srpde_div_apply (shift 0: today's call) or srpde_div_apply_shift on prepared fields (_div_fields); with a side
    mask ``bc`` srpde_div_apply_bc; with boundary data ``bd`` (_bd_fields) srpde_div_apply_bd."""
    y = torch.empty_like(u)
    if u.shape[0] and bd is not None:
        call("srpde_div_apply_bd", u.data_ptr(), theta.data_ptr(), y.data_ptr(), u.shape[0], u.shape[-1], mean,
             inv_h2, shift, bc or 0, bd.data_ptr(), _bd_stride(bd, u.shape[0]), stream_ptr(u.device))
    elif u.shape[0] and bc is not None:
        call("srpde_div_apply_bc", u.data_ptr(), theta.data_ptr(), y.data_ptr(), u.shape[0], u.shape[-1], mean,
             inv_h2, shift, bc, stream_ptr(u.device))
    elif u.shape[0] and shift == 0.0:
        call("srpde_div_apply", u.data_ptr(), theta.data_ptr(), y.data_ptr(), u.shape[0], u.shape[-1], mean,
             inv_h2, stream_ptr(u.device))
    elif u.shape[0]:
        call("srpde_div_apply_shift", u.data_ptr(), theta.data_ptr(), y.data_ptr(), u.shape[0], u.shape[-1], mean,
             inv_h2, shift, stream_ptr(u.device))
    return y


def _div_theta_grad(u, lam, theta, mean: int, inv_h2: float, scale: float, bc=None, bd=None):
    """srpde_div_theta_grad on prepared fields; with a side mask ``bc`` srpde_div_theta_grad_bc; with boundary data
    ``bd`` (u's) srpde_div_theta_grad_bd."""
    g = torch.empty_like(u)
    if u.shape[0] and bd is not None:
        call("srpde_div_theta_grad_bd", u.data_ptr(), lam.data_ptr(), theta.data_ptr(), g.data_ptr(), u.shape[0],
             u.shape[-1], mean, inv_h2, scale, bc or 0, bd.data_ptr(), _bd_stride(bd, u.shape[0]),
             stream_ptr(u.device))
    elif u.shape[0] and bc is not None:
        call("srpde_div_theta_grad_bc", u.data_ptr(), lam.data_ptr(), theta.data_ptr(), g.data_ptr(), u.shape[0],
             u.shape[-1], mean, inv_h2, scale, bc, stream_ptr(u.device))
    elif u.shape[0]:
        call("srpde_div_theta_grad", u.data_ptr(), lam.data_ptr(), theta.data_ptr(), g.data_ptr(), u.shape[0],
             u.shape[-1], mean, inv_h2, scale, stream_ptr(u.device))
    return g


def div_theta_grad(u, lam, theta, face_mean: str = "harmonic", inv_h2: float = None, scale: float = 1.0,
                   device="cuda", bc=None, bc_data=None):
    """scale * G(u, lam; theta), the pair gradient of the divergence-form operator: a new [B, n, n] fp64 device tensor
    with G_a = inv_h2 * (sum over the four faces of node a of dc_ab/dtheta_a (u_b - u_a) (lam_b - lam_a)), where
    dc/dtheta_a is 0.5 (``"arithmetic"``), 2 tb^2 / (ta + tb)^2 (``"harmonic"``) and 1 towards the ghost ring (u and
    lam are 0 there).  d<lam, D_theta u>/dtheta = -G: the theta gradient of apply_div is -G(u, grad_y), that of
    solve_div +G(u, lam) with lam the adjoint solve.  u, lam [n, n] or [B, n, n]; theta is broadcast; ``inv_h2``
    defaults to (n - 1)^2.  One launch, stream-ordered, no host sync, not itself differentiable
    (srpde_div_theta_grad; include/srpde.h states the rounding order).  ``bc`` (``check_bc``): dc/dtheta_a is 0
    towards a zero-flux side (srpde_div_theta_grad_bc).  ``bc_data``: the boundary data of ``u`` -- beyond a "d" side u
    is g, lam stays 0 -- so that d<lam, A u>/dtheta = -G still (srpde_div_theta_grad_bd); fluxes do not enter."""
    mean = check_face_mean(face_mean)
    bc = check_bc(bc)
    _bd_check(bc_data, u)
    with torch.no_grad():
        u, theta, B, n = _div_fields(u, theta, device)
        bd = _bd_fields(bc_data, u, u.device)
        lam = _dev_f64(lam, device).reshape(u.shape)
        return _div_theta_grad(u, lam, theta, mean, float((n - 1) ** 2 if inv_h2 is None else inv_h2), float(scale),
                               bc, bd)


class _ApplyDiv(torch.autograd.Function):
    """y = D_theta u - shift u.  The operator is symmetric: grad_u = (D_theta - shift) grad_y; the shift does not
    depend on theta, so grad_theta = -G(u, grad_y; theta) as without it."""

    @staticmethod
    def forward(ctx, u, theta, mean, inv_h2, shift=0.0, bc=None, bd=None):
        u, theta = u.detach().contiguous(), theta.detach().contiguous()
        bd = None if bd is None else bd.detach()
        ctx.save_for_backward(u, theta, bd)
        ctx.mean, ctx.inv_h2, ctx.shift, ctx.bc = mean, inv_h2, shift, bc
        return _apply_div(u, theta, mean, inv_h2, shift, bc, bd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        # with boundary data y = (D - shift) u + b(bd, theta): the gradient in u is the homogeneous operator's, the
        # one in theta sees g through u's halo, the one in bd is srpde_div_bd_grad of grad_y
        u, theta, bd = ctx.saved_tensors
        gy = gy.contiguous()
        gu = _apply_div(gy, theta, ctx.mean, ctx.inv_h2, ctx.shift, ctx.bc) if ctx.needs_input_grad[0] else None
        gth = None
        if ctx.needs_input_grad[1]:
            gth = _div_theta_grad(u, gy, theta, ctx.mean, ctx.inv_h2, -1.0, ctx.bc, bd)
        gbd = _bd_grad(gy, theta, ctx.inv_h2, ctx.bc, bd) if bd is not None and ctx.needs_input_grad[6] else None
        return gu, gth, None, None, None, None, gbd


class _SolveDiv(torch.autograd.Function):
    """u = (D_theta - shift)^-1 f.  The adjoint solve is the same solve: lam = (D_theta - shift)^-1 grad_u with the
    forward's face mean, tolerance, limits, shift and preconditioner shift, from a zero start; grad_f = lam;
    grad_theta = +G(u, lam; theta), the shift not depending on theta.  Nothing depends on u0."""

    @staticmethod
    def forward(ctx, f, theta, u0, mean, rtol, maxit, check_every, check, shift=0.0, pshift=0.0, bc=None, bd=None):
        f, theta = f.detach().contiguous(), theta.detach().contiguous()
        bd = None if bd is None else bd.detach()
        u, iters, resid = _solve_div(f, theta, u0, mean, rtol, maxit, check_every, check, shift, pshift, bc=bc, bd=bd)
        ctx.save_for_backward(u, theta, bd)
        ctx.args, ctx.bc = (mean, rtol, maxit, check_every, check, shift, pshift), bc
        ctx.mark_non_differentiable(iters, resid)
        return u, iters, resid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gu, _giters, _gresid):
        # with boundary data u = (D - shift)^-1 (f - b(bd, theta)): the adjoint solve stays homogeneous, the theta
        # gradient sees g through u's halo, and grad_bd = -srpde_div_bd_grad(lam)
        u, theta, bd = ctx.saved_tensors
        mean = ctx.args[0]
        lam = _solve_div(gu.contiguous(), theta, None, *ctx.args, bc=ctx.bc)[0]     # NotConverged propagates
        inv_h2 = float((u.shape[-1] - 1) ** 2)
        gth = None
        if ctx.needs_input_grad[1]:
            gth = _div_theta_grad(u, lam, theta, mean, inv_h2, 1.0, ctx.bc, bd)
        gbd = _bd_grad(lam, theta, inv_h2, ctx.bc, bd, -1.0) if bd is not None and ctx.needs_input_grad[11] else None
        return ((lam if ctx.needs_input_grad[0] else None), gth, None, None, None, None, None, None, None, None, None,
                gbd)


def apply_div(u, theta, face_mean: str = "harmonic", inv_h2: float = None, device="cuda", shift: float = 0.0,
              bc=None, bc_data=None):
    """y = div(theta grad u) on the project's grid (zero ghost ring, h = 1 / (n - 1)): a new [B, n, n] fp64 device
    tensor.  The face coefficient between nodes a and b is 0.5 (ta + tb) (``"arithmetic"``) or 2 ta tb / (ta + tb)
    (``"harmonic"``), theta_a towards the ghost ring; ``inv_h2`` defaults to (n - 1)^2.  One launch, stream-ordered,
    no host sync (srpde_div_apply; include/srpde.h states the rounding order).

    Differentiable in u and theta when grad mode is on and one of them requires grad (one more srpde_div_apply for
    u, one srpde_div_theta_grad for theta; once differentiable); otherwise exactly the call above.

    ``shift`` (sigma >= 0, finite): y = div(theta grad u) - sigma u, the operator of an implicit time step, in the
    same launch (srpde_div_apply_shift: the product sigma * u, then one subtraction).  The gradient in u carries the
    shift, the one in theta does not change, the shift itself gets none.  0.0 (default) is exactly today's call.

    ``bc`` (``check_bc``, e.g. ``"ddnn"``): an "n" side is zero-flux -- its ghost faces have coefficient 0 instead of
    theta_a -- in the same launch (srpde_div_apply_bc); both gradients carry the pattern.  None (default) and
    ``"dddd"`` are exactly today's calls.

    ``bc_data`` (``bc_data()``; [4, n], [1, 4, n] shared by the batch, or [B, 4, n], fp64): the sides carry values, in
    the same launch (srpde_div_apply_bd): beyond a "d" side of ``bc`` (all four for ``bc=None``) the ghost node holds
    g instead of 0, through an "n" side flows the outward flux q, which adds q * sqrt(inv_h2) to the edge node:
    y = D u - sigma u + b(data, theta).  The gradient in u is the homogeneous operator's, the one in theta sees g, and
    the data gets one (srpde_div_bd_grad; summed over the batch when shared).  Wrong shape or dtype and, for data on
    the host, non-finite values are ValueErrors.  None (default) is exactly today's call."""
    mean = check_face_mean(face_mean)
    shift = check_shift(shift)
    bc = check_bc(bc)
    _bd_check(bc_data, u)
    u, theta, B, n = _div_fields(u, theta, device)
    bd = _bd_fields(bc_data, u, u.device)
    inv_h2 = float((n - 1) ** 2 if inv_h2 is None else inv_h2)
    if _wants_grad(u, theta, *(() if bd is None else (bd,))):
        return _ApplyDiv.apply(u, theta, mean, inv_h2, shift, bc, bd)
    return _apply_div(u, theta, mean, inv_h2, shift, bc, bd)


def solve_div(f, theta, face_mean: str = "harmonic", rtol: float = DEFAULT_RTOL, maxit: int = None,
              check_every: int = 8, check: bool = True, return_info: bool = False, device="cuda", u0=None,
              shift: float = 0.0, precond_shift: float = None, bc=None, bc_data=None):
    """u[B, n, n] (float64, on device) with div(theta grad u) = f per problem, by CG preconditioned with the
    sine-transform solve of the constant-coefficient operator (srpde_div_cg_*).  Convergence, |r| <= rtol |f|, is
    decided per problem on the device, and a converged problem is frozen, so a problem's u / iters / resid are the
    same bits whatever else is in the batch and however many further iterations run.

    ``check_every`` > 0 (default): iterations run in chunks of that many and the done flags are read between chunks
    (one small host sync each), until every problem is done or ``maxit`` (default 20 n^2) is reached.
    ``check_every=0``: exactly ``maxit`` iterations and no host sync at all -- capturable in a graph once
    ``dst_plan(n)`` exists.
    ``check`` (not under stream capture): problems with resid > rtol raise NotConverged (one host sync).
    ``return_info``: (u, iters [B] int32, resid [B] fp64 = |r| / |f|, 0 for f = 0).
    ``u0`` ([B, n, n] or [n, n], broadcast like f): the iteration starts from it instead of from 0
    (srpde_div_cg_init_from): a u0 with |f - D u0| <= rtol |f| is returned after 0 iterations, a nearby one (the last
    step of an optimisation loop, a cascade output) saves the iterations that its residual is already below |f|;
    zeros give the bits of ``u0=None``, which is today's call sequence.

    Differentiable in f and theta when grad mode is on and one of them requires grad (once differentiable): the
    backward is one more solve with the same theta, face_mean, rtol, maxit and check_every from a zero start (the
    operator is symmetric), which raises NotConverged like the forward, and, if theta needs a gradient, one
    srpde_div_theta_grad.  u0 gets no gradient (the solution does not depend on it); iters and resid are not
    differentiable.  Without a tensor that requires grad, or under no_grad, exactly the calls above.

    ``shift`` (sigma >= 0, finite): solves div(theta grad u) - sigma u = f, one implicit time step or the screened
    problem (srpde_div_cg_*_shift), preconditioned with the sine-transform solve of L - sigma_p I.  ``precond_shift``
    is sigma_p; None takes sigma / sqrt(theta_min theta_max) over the batch, which is one host read of theta's range:
    in fixed-iteration mode (``check_every=0``) and under stream capture it must be given.  Any sigma_p = sigma /
    theta_g with theta_g in theta's range keeps cond <= theta_max / theta_min, so the iteration count is at most the
    unshifted one's bound (``pcg_iterations``) for every sigma.  The adjoint solve uses the same two shifts; the shift
    gets no gradient.  ``shift=0.0`` (default; ``precond_shift`` must then be None or 0) makes exactly today's calls.

    ``bc`` (``check_bc``, e.g. ``"ddnn"``): "n" sides are zero-flux (srpde_div_cg_*_bc), and the preconditioner is the
    separable solve of the constant-coefficient operator with the same sides (``sep_plan(n, bc)``, four launches at
    every n), so the bound theta_max / theta_min and ``pcg_iterations`` hold for every pattern.  ``"nnnn"`` is singular
    without a shift and refused (ValueError); with one it is the insulated box.  u0, shift, precond_shift, both modes,
    capture (once ``sep_plan(n, bc)`` exists) and the gradients work as without.  None (default) and ``"dddd"`` make
    exactly today's calls.

    ``bc_data`` (as for ``apply_div``): u = g on the "d" sides, the outward flux q through the "n" sides; the problem
    solved is (D - sigma) u = f - b(data, theta), started by srpde_div_cg_init_from_bd (also without ``u0``) and
    iterated by today's entries: the iteration, the preconditioner (the sine plan for four "d" sides, the separable
    one otherwise) and the bound are the homogeneous ones.  The stop rule is |r| <= rtol |f - b| and ``resid`` is
    |r| / |f - b|: Laplace's equation, f = 0 with g != 0, has |f| = 0 but is not solved by u = 0.  The data gets a
    gradient, minus srpde_div_bd_grad of the (homogeneous) adjoint solution.  ``"nnnn"`` without a shift stays
    refused; whether its fluxes balance the forcing is the caller's business.  None (default) makes today's calls."""
    mean = check_face_mean(face_mean)
    shift = check_shift(shift)
    bc = check_bc(bc)
    if bc == 15 and shift == 0.0:
        raise ValueError('solve_div: bc="nnnn" with shift=0 is singular (the constants): it needs a shift > 0')
    if bc == 15 and precond_shift is not None and float(precond_shift) == 0.0:
        raise ValueError('solve_div: bc="nnnn" needs a precond_shift > 0 (the unshifted preconditioner is singular)')
    if precond_shift is not None:
        precond_shift = check_shift(precond_shift, "precond_shift")
        if shift == 0.0 and precond_shift != 0.0:
            raise ValueError("solve_div: precond_shift belongs to a shifted solve (shift > 0)")
    elif shift != 0.0 and (int(check_every) == 0 or torch.cuda.is_current_stream_capturing()):
        raise ValueError("solve_div: precond_shift=None reads theta's range back (a host sync): give precond_shift "
                         "in fixed-iteration mode (check_every=0) and under stream capture")
    _bd_check(bc_data, f)
    f, theta, B, n = _div_fields(f, theta, device)
    bd = _bd_fields(bc_data, f, f.device)
    if u0 is not None:
        u0 = _dev_f64(u0, device).detach()
        if u0.dim() == 2:
            u0 = u0.unsqueeze(0)
        if u0.shape != f.shape:
            u0 = u0.expand_as(f)
        u0 = u0.contiguous()
    if maxit is None:
        maxit = 20 * n * n
    maxit, check_every = int(maxit), int(check_every)
    if maxit < 0 or check_every < 0:
        raise ValueError("solve_div: maxit and check_every must be >= 0")
    if shift == 0.0:
        pshift = 0.0
    else:
        pshift = precond_shift_for(theta, shift) if precond_shift is None else precond_shift
    if _wants_grad(f, theta, *(() if bd is None else (bd,))):
        out = _SolveDiv.apply(f, theta, u0, mean, float(rtol), maxit, check_every, bool(check), shift, pshift, bc, bd)
    else:
        out = _solve_div(f, theta, u0, mean, float(rtol), maxit, check_every, bool(check), shift, pshift, bc=bc,
                         bd=bd)
    return out if return_info else out[0]


def _solve_div(f, theta, u0, mean: int, rtol: float, maxit: int, check_every: int, check: bool, shift: float = 0.0,
               pshift: float = 0.0, ws=None, out=None, bc=None, bd=None):
    """The srpde_div_cg_* call sequence on prepared fields -> (u, iters, resid); shift 0 is the unshifted entries'
    sequence, call for call; a side mask ``bc`` the *_bc entries' with the separable plan.  ``ws`` / ``out`` = (u,
    iters, resid): the caller's buffers (diffuse reuses them).  Boundary data ``bd``: srpde_div_cg_init_from_bd starts
    (u0 or not), on the plan and workspace that ``bc`` selects, and the same iterate / finish calls follow."""
    B, n = f.shape[0], f.shape[-1]
    if out is None:
        u = torch.empty_like(f)
        iters = torch.empty(B, dtype=torch.int32, device=f.device)
        resid = torch.empty(B, dtype=torch.float64, device=f.device)
    else:
        u, iters, resid = out
    if B == 0:
        return u, iters, resid
    capturing = torch.cuda.is_current_stream_capturing()
    if check_every and capturing:
        raise RuntimeError("solve_div: reading the done flags synchronises the host; capture with check_every=0")
    plan = dst_plan(n, f.device) if bc is None else sep_plan(n, bc, f.device)
    ws_bytes = int(query("srpde_div_cg_workspace_size" if bc is None else "srpde_div_cg_workspace_size_bc", B, n))
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=f.device)
    sp = stream_ptr(f.device)
    if bd is not None:
        call("srpde_div_cg_init_from_bd", f.data_ptr(), 0 if u0 is None else u0.data_ptr(), theta.data_ptr(), B, n,
             mean, bc or 0, shift, pshift, rtol, bd.data_ptr(), _bd_stride(bd, B), plan.data_ptr(), plan.numel(),
             ws.data_ptr(), ws_bytes, sp)
    elif bc is not None:
        if u0 is None:
            call("srpde_div_cg_init_bc", f.data_ptr(), B, n, bc, pshift, plan.data_ptr(), plan.numel(), ws.data_ptr(),
                 ws_bytes, sp)
        else:
            call("srpde_div_cg_init_from_bc", f.data_ptr(), u0.data_ptr(), theta.data_ptr(), B, n, mean, bc, shift,
                 pshift, rtol, plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
    elif shift != 0.0:
        if u0 is None:
            call("srpde_div_cg_init_shift", f.data_ptr(), B, n, pshift, plan.data_ptr(), plan.numel(), ws.data_ptr(),
                 ws_bytes, sp)
        else:
            call("srpde_div_cg_init_from_shift", f.data_ptr(), u0.data_ptr(), theta.data_ptr(), B, n, mean, shift,
                 pshift, rtol, plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
    elif u0 is None:
        call("srpde_div_cg_init", f.data_ptr(), B, n, plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
    else:
        call("srpde_div_cg_init_from", f.data_ptr(), u0.data_ptr(), theta.data_ptr(), B, n, mean, rtol,
             plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
    done_at = int(query("srpde_div_cg_done_offset", B, n))
    done = ws[done_at:done_at + 4 * B].view(torch.int32)
    k = 0
    if (u0 is not None or bd is not None) and check_every and bool(done.all()):   # rtol already met: no chunk at all
        k = maxit
    while k < maxit:
        count = min(check_every, maxit - k) if check_every else maxit
        if bc is not None:
            call("srpde_div_cg_iterate_bc", theta.data_ptr(), B, n, mean, bc, shift, pshift, rtol, k + 1, count,
                 plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
        elif shift != 0.0:
            call("srpde_div_cg_iterate_shift", theta.data_ptr(), B, n, mean, shift, pshift, rtol, k + 1, count,
                 plan.data_ptr(), plan.numel(), ws.data_ptr(), ws_bytes, sp)
        else:
            call("srpde_div_cg_iterate", theta.data_ptr(), B, n, mean, rtol, k + 1, count, plan.data_ptr(),
                 plan.numel(), ws.data_ptr(), ws_bytes, sp)
        k += count
        if check_every and k < maxit and bool(done.all()):
            break
    call("srpde_div_cg_finish", u.data_ptr(), iters.data_ptr(), resid.data_ptr(), B, n, ws.data_ptr(), ws_bytes, sp)
    if check and not capturing:
        bad = resid > rtol
        nbad = int(bad.sum())
        if nbad:
            raise NotConverged(f"solve_div: {nbad} of {B} problems (n={n}) above rtol={rtol:g} after {maxit} "
                               f"iterations; worst residual {float(resid.max()):.3e}")
    return u, iters, resid


SCHEMES = ("be", "cn")


def diffuse(u0, theta, f=None, dt: float = None, steps: int = 1, scheme: str = "be", face_mean: str = "harmonic",
            rtol: float = DEFAULT_RTOL, maxit: int = None, pcg_iters: int = None, precond_shift: float = None,
            save_every: int = None, check: bool = False, check_every: int = 8, device="cuda", bc=None, bc_data=None):
    """``steps`` implicit time steps of u_t = div(theta grad u) - f from u0, the forcing constant in time (None: 0),
    on the project's grid (zero ghost ring).  Each step solves (D_theta - sigma I) u+ = rhs by the shifted
    sine-preconditioned CG, warm-started from the current state:
        ``scheme="be"``  backward Euler,  sigma = 1 / dt,  rhs = f - sigma u              (first order, L-stable)
        ``scheme="cn"``  Crank-Nicolson,  sigma = 2 / dt,  rhs = 2 f - sigma u - D_theta u (second order)
    u0, f [n, n] or [B, n, n]; theta is broadcast.  -> the final u [B, n, n] fp64; with ``save_every`` = s also the
    frames after steps s, 2 s, ... as [T, B, n, n]; with ``check`` also the per-step iteration counts [steps, B]
    int32 -- in that order, as a tuple when there is more than u.

    One step is srpde_div_step_rhs, srpde_div_cg_init_from_shift with u0 = the current state, srpde_div_cg_iterate_
    shift, srpde_div_cg_finish; the plan, the workspace and sigma_p are made once, outside the loop.
    ``pcg_iters`` = k selects fixed mode: exactly k iterations per step (converged problems freeze), no host read
    anywhere in the loop, so the whole loop is capturable in one graph once ``dst_plan(n)`` exists; it needs a
    ``precond_shift`` (the default, sigma / sqrt(theta_min theta_max), is a host read).  ``pcg_iterations(theta_lo,
    theta_hi, tol)`` bounds k for every dt.  Without ``pcg_iters`` a step iterates to ``rtol`` in chunks of
    ``check_every`` (one small host read each, ``maxit`` at most, default 20 n^2) and raises NotConverged above it.

    Differentiable in theta, u0 and f when grad mode is on and one of them requires grad: the steps are then composed
    from the autograd ``solve_div(shift=, u0=)`` and ``apply_div`` plus torch arithmetic for rhs (same solves, a few
    more launches and one adjoint solve per step in the backward; once differentiable).  dt and the shift get no
    gradient.  Otherwise the direct ABI path above.

    ``bc`` (``check_bc``, e.g. ``"nnnn"``, the insulated box: with f = None the sum of u is conserved up to the solves'
    tolerance): "n" sides are zero-flux in the operator, in Crank-Nicolson's right-hand side (srpde_div_step_rhs_bc)
    and in every solve (``solve_div(bc=)``); capture needs ``sep_plan(n, bc)`` first.  None (default) and ``"dddd"``
    make exactly today's calls.

    ``bc_data`` (as for ``apply_div``), constant in time: u_t = D u + b(data, theta) - f.  Crank-Nicolson's right-hand
    side carries the data (srpde_div_step_rhs_bd: 2 f - sigma u - (D u + b)), backward Euler's does not change, and
    every solve is ``solve_div(bc_data=)``'s; differentiable in the data by the same composition.  None (default)
    makes today's calls."""
    pattern, bc = bc, check_bc(bc)
    _bd_check(bc_data, u0)
    if scheme not in SCHEMES:
        raise ValueError(f"unknown time scheme {scheme!r}: one of {SCHEMES}")
    mean = check_face_mean(face_mean)
    if dt is None or not (float(dt) > 0.0 and np.isfinite(float(dt))):
        raise ValueError(f"diffuse: dt must be positive and finite, got {dt}")
    steps = int(steps)
    if steps < 0:
        raise ValueError("diffuse: steps must be >= 0")
    if save_every is not None and int(save_every) < 1:
        raise ValueError("diffuse: save_every must be >= 1")
    cn = SCHEMES.index(scheme)
    sigma = check_shift((2.0 if cn else 1.0) / float(dt), "1 / dt")
    fixed = pcg_iters is not None
    if fixed and int(pcg_iters) < 1:
        raise ValueError("diffuse: pcg_iters must be >= 1")
    if precond_shift is not None:
        precond_shift = check_shift(precond_shift, "precond_shift")
        if bc == 15 and precond_shift == 0.0:
            raise ValueError('diffuse: bc="nnnn" needs a precond_shift > 0 (the unshifted preconditioner is singular)')
    elif fixed or torch.cuda.is_current_stream_capturing():
        raise ValueError("diffuse: precond_shift=None reads theta's range back (a host sync): give precond_shift "
                         "in fixed mode (pcg_iters) and under stream capture")
    u, theta, B, n = _div_fields(u0, theta, device)
    bd = _bd_fields(bc_data, u, u.device)
    if f is not None:
        f = _dev_f64(f, device)
        if f.dim() == 2:
            f = f.unsqueeze(0)
        if f.shape != u.shape:
            f = f.expand_as(u)
        f = f.contiguous()
    pshift = precond_shift_for(theta, sigma) if precond_shift is None else precond_shift
    if maxit is None:
        maxit = 20 * n * n
    it_max, chunk = (int(pcg_iters), 0) if fixed else (int(maxit), int(check_every))
    if not fixed and chunk < 1:
        raise ValueError("diffuse: check_every must be >= 1 (pcg_iters selects the mode without host reads)")
    frames = []
    counts = torch.zeros(steps, B, dtype=torch.int32, device=u.device)

    if _wants_grad(u, theta, *(() if f is None else (f,)), *(() if bd is None else (bd,))):
        for s in range(steps):
            rhs = -sigma * u if f is None else (2.0 * f if cn else f) - sigma * u
            if cn:
                rhs = rhs - apply_div(u, theta, face_mean, device=device, bc=pattern, bc_data=bd)
            u, it, _ = solve_div(rhs, theta, face_mean=face_mean, rtol=rtol, maxit=it_max, check_every=chunk,
                                 check=not fixed, return_info=True, device=device, u0=u.detach(), shift=sigma,
                                 precond_shift=pshift, bc=pattern, bc_data=bd)
            counts[s] = it
            if save_every and (s + 1) % int(save_every) == 0:
                frames.append(u)
    else:
        u = u.detach().clone()           # the state, advanced in place: u0 is left as it was
        theta = theta.detach()
        if B and steps:
            ws_query = "srpde_div_cg_workspace_size" if bc is None else "srpde_div_cg_workspace_size_bc"
            ws = torch.empty(int(query(ws_query, B, n)), dtype=torch.uint8, device=u.device)
            rhs = torch.empty_like(u)
            resid = torch.empty(B, dtype=torch.float64, device=u.device)
            fp = 0 if f is None else f.data_ptr()
        for s in range(steps if B else 0):
            if bd is not None:
                call("srpde_div_step_rhs_bd", u.data_ptr(), fp, theta.data_ptr(), rhs.data_ptr(), B, n, mean, sigma,
                     cn, bc or 0, bd.data_ptr(), _bd_stride(bd, B), stream_ptr(u.device))
            elif bc is None:
                call("srpde_div_step_rhs", u.data_ptr(), fp, theta.data_ptr(), rhs.data_ptr(), B, n, mean, sigma, cn,
                     stream_ptr(u.device))
            else:
                call("srpde_div_step_rhs_bc", u.data_ptr(), fp, theta.data_ptr(), rhs.data_ptr(), B, n, mean, sigma,
                     cn, bc, stream_ptr(u.device))
            # init_from copies the state into the workspace before finish overwrites it with the new one
            _solve_div(rhs, theta, u, mean, float(rtol), it_max, chunk, not fixed, sigma, pshift, ws=ws,
                       out=(u, counts[s], resid), bc=bc, bd=bd)
            if save_every and (s + 1) % int(save_every) == 0:
                frames.append(u.clone())
    out = (u,)
    if save_every:
        out += (torch.stack(frames) if frames else u.new_empty((0,) + tuple(u.shape)),)
    if check:
        out += (counts,)
    return out if len(out) > 1 else out[0]


def _flux_args(mean: int, inv_h2: float, bc, bd, B: int):
    """The tail (face_mean, inv_h2, bc, bd, bd_stride) of the flux entries' arguments; bd None is their NULL."""
    return (mean, inv_h2, bc or 0, 0 if bd is None else bd.data_ptr(), 0 if bd is None else _bd_stride(bd, B))


def _face_flux(u, theta, mean: int, inv_h2: float, bc, bd):
    """srpde_div_face_flux on prepared fields -> (Fx [B, n, n + 1], Fy [B, n + 1, n])."""
    B, n = u.shape[0], u.shape[-1]
    Fx = torch.empty(B, n, n + 1, dtype=torch.float64, device=u.device)
    Fy = torch.empty(B, n + 1, n, dtype=torch.float64, device=u.device)
    if B:
        call("srpde_div_face_flux", u.data_ptr(), theta.data_ptr(), Fx.data_ptr(), Fy.data_ptr(), B, n,
             *_flux_args(mean, inv_h2, bc, bd, B), stream_ptr(u.device))
    return Fx, Fy


def _wall_flux(u, theta, mean: int, inv_h2: float, bc, bd):
    """srpde_div_wall_flux on prepared fields -> W [B, 4]."""
    B, n = u.shape[0], u.shape[-1]
    W = torch.empty(B, 4, dtype=torch.float64, device=u.device)
    if B:
        call("srpde_div_wall_flux", u.data_ptr(), theta.data_ptr(), W.data_ptr(), B, n,
             *_flux_args(mean, inv_h2, bc, bd, B), stream_ptr(u.device))
    return W


def _side_is_flux(bc, side: int) -> bool:
    return bool(((bc or 0) >> side) & 1)


class _FaceFlux(torch.autograd.Function):
    """(Fx, Fy) = srpde_div_face_flux.  grad_u and grad_theta are one srpde_div_face_flux_grad; the data enters wall
    faces only, so its gradient is four slice expressions: -+ theta_a inv_h gF on a "d" side's low / high wall, -+ gF
    on an "n" side's."""

    @staticmethod
    def forward(ctx, u, theta, mean, inv_h2, bc, bd):
        u, theta = u.detach().contiguous(), theta.detach().contiguous()
        bd = None if bd is None else bd.detach()
        ctx.save_for_backward(u, theta, bd)
        ctx.mean, ctx.inv_h2, ctx.bc = mean, inv_h2, bc
        return _face_flux(u, theta, mean, inv_h2, bc, bd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gFx, gFy):
        u, theta, bd = ctx.saved_tensors
        B, n = u.shape[0], u.shape[-1]
        gFx, gFy = gFx.contiguous(), gFy.contiguous()
        gu = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        gth = torch.empty_like(u) if ctx.needs_input_grad[1] else None
        if B and (gu is not None or gth is not None):
            call("srpde_div_face_flux_grad", u.data_ptr(), theta.data_ptr(), gFx.data_ptr(), gFy.data_ptr(),
                 0 if gu is None else gu.data_ptr(), 0 if gth is None else gth.data_ptr(), B, n,
                 *_flux_args(ctx.mean, ctx.inv_h2, ctx.bc, bd, B), stream_ptr(u.device))
        gbd = None
        if bd is not None and ctx.needs_input_grad[5]:
            inv_h = float(np.sqrt(ctx.inv_h2))
            walls = ((gFy[:, 0, :], theta[:, 0, :], -1.0), (gFy[:, n, :], theta[:, n - 1, :], 1.0),
                     (gFx[:, :, 0], theta[:, :, 0], -1.0), (gFx[:, :, n], theta[:, :, n - 1], 1.0))
            gbd = torch.stack([sign * gF if _side_is_flux(ctx.bc, s) else sign * ((ta * inv_h) * gF)
                               for s, (gF, ta, sign) in enumerate(walls)], dim=1)
            if bd.shape[0] != B:
                gbd = gbd.sum(0, keepdim=True)
        return gu, gth, None, None, None, gbd


class _WallFlux(torch.autograd.Function):
    """W = srpde_div_wall_flux.  One srpde_div_wall_flux_grad gives the three gradients on the edges, [B, 4, n] each;
    the edge rows of u and theta are added into zero fields in the sides' order (a corner node receives from both of
    its sides), the data's is summed over the batch when shared."""

    @staticmethod
    def forward(ctx, u, theta, mean, inv_h2, bc, bd):
        u, theta = u.detach().contiguous(), theta.detach().contiguous()
        bd = None if bd is None else bd.detach()
        ctx.save_for_backward(u, theta, bd)
        ctx.inv_h2, ctx.bc = inv_h2, bc
        return _wall_flux(u, theta, mean, inv_h2, bc, bd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gW):
        u, theta, bd = ctx.saved_tensors
        B, n = u.shape[0], u.shape[-1]
        need_u, need_th = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_bd = bd is not None and ctx.needs_input_grad[5]
        gW = gW.contiguous()
        edges = [torch.empty(B, 4, n, dtype=torch.float64, device=u.device) if need else None
                 for need in (need_u, need_th, need_bd)]
        if B and any(e is not None for e in edges):
            call("srpde_div_wall_flux_grad", gW.data_ptr(), u.data_ptr(), theta.data_ptr(),
                 *(0 if e is None else e.data_ptr() for e in edges), B, n, ctx.inv_h2, ctx.bc or 0,
                 0 if bd is None else bd.data_ptr(), 0 if bd is None else _bd_stride(bd, B), stream_ptr(u.device))

        def field(e):
            if e is None:
                return None
            g = torch.zeros_like(u)
            g[:, 0, :] += e[:, 0]
            g[:, n - 1, :] += e[:, 1]
            g[:, :, 0] += e[:, 2]
            g[:, :, n - 1] += e[:, 3]
            return g

        gbd = edges[2]
        if gbd is not None and bd.shape[0] != B:
            gbd = gbd.sum(0, keepdim=True)
        return field(edges[0]), field(edges[1]), None, None, None, gbd


def _flux_prepare(u, theta, face_mean, inv_h2, device, bc, bc_data):
    mean = check_face_mean(face_mean)
    bc = check_bc(bc)
    _bd_check(bc_data, u)
    u, theta, B, n = _div_fields(u, theta, device)
    bd = _bd_fields(bc_data, u, u.device)
    return u, theta, mean, float((n - 1) ** 2 if inv_h2 is None else inv_h2), bc, bd


def face_flux(u, theta, face_mean: str = "harmonic", inv_h2: float = None, device="cuda", bc=None, bc_data=None):
    """(Fx, Fy): the fluxes theta du/dx and theta du/dy of ``apply_div``'s discretisation on the faces, new fp64 device
    tensors.  Fx [B, n, n + 1]: entry (i, j) is the face between nodes (i, j - 1) and (i, j), j = 0 and j = n the wall
    faces of column 0 and column n - 1; Fy [B, n + 1, n]: entry (i, j) is the face between nodes (i - 1, j) and (i, j),
    i = 0 and i = n the wall faces of row 0 and row n - 1.  A face between two nodes is c (u_hi - u_lo) sqrt(inv_h2)
    with ``apply_div``'s face coefficient c; a wall face of a "d" side has c = theta_a and the ghost value g of
    ``bc_data`` (0 without); a wall face of an "n" side carries the prescribed outward flux, -q on a low wall and +q on
    a high one (0 without data).  So ((Fx[i, j+1] - Fx[i, j]) + (Fy[i+1, j] - Fy[i, j])) sqrt(inv_h2) is
    ``apply_div(u, theta, ..., bc=, bc_data=)`` up to rounding.  u [n, n] or [B, n, n]; theta is broadcast; ``inv_h2``
    defaults to (n - 1)^2; ``bc`` and ``bc_data`` are ``apply_div``'s.  One launch, stream-ordered, no host sync
    (srpde_div_face_flux; include/srpde.h states the rounding order).

    Differentiable in u, theta and ``bc_data`` when grad mode is on and one of them requires grad (one
    srpde_div_face_flux_grad, a few slices for the data; once differentiable); otherwise exactly the call above."""
    u, theta, mean, inv_h2, bc, bd = _flux_prepare(u, theta, face_mean, inv_h2, device, bc, bc_data)
    if _wants_grad(u, theta, *(() if bd is None else (bd,))):
        return _FaceFlux.apply(u, theta, mean, inv_h2, bc, bd)
    return _face_flux(u, theta, mean, inv_h2, bc, bd)


def wall_flux(u, theta, face_mean: str = "harmonic", inv_h2: float = None, device="cuda", bc=None, bc_data=None):
    """W [B, 4] (fp64, on device): the integral of the outward flux theta du/dn over each wall, the sides in the
    pattern's order (row 0, row n - 1, column 0, column n - 1): W_s = h * sum over the side's n wall faces of
    -Fy[0, k], +Fy[n, k], -Fx[k, 0], +Fx[k, n] of ``face_flux``, h = 1 / sqrt(inv_h2).  The sum of the four is
    h^2 * sum(apply_div(u, theta, ..., bc=, bc_data=)) up to rounding -- the discrete divergence theorem: for a solution
    of div(theta grad u) = f the walls pass h^2 sum(f).  Reads the 4 n edge nodes of a problem only, sums in fp64 in
    one fixed order that depends on n alone (a problem's W does not depend on the batch), one launch, no host sync
    (srpde_div_wall_flux).  ``face_mean`` is checked and changes nothing: a wall face has c = theta_a.

    Differentiable in u, theta and ``bc_data`` (one srpde_div_wall_flux_grad and slice adds; a shared [1, 4, n] or
    [4, n] data gradient is summed over the batch; once differentiable)."""
    u, theta, mean, inv_h2, bc, bd = _flux_prepare(u, theta, face_mean, inv_h2, device, bc, bc_data)
    if _wants_grad(u, theta, *(() if bd is None else (bd,))):
        return _WallFlux.apply(u, theta, mean, inv_h2, bc, bd)
    return _wall_flux(u, theta, mean, inv_h2, bc, bd)


EFFECTIVE_PATTERNS = ("ddnn", "nndd")   # effective_coefficient's sides for axis 0 (flow across the rows) and axis 1


def effective_coefficient(theta, axis: int = 0, face_mean: str = "harmonic", rtol: float = DEFAULT_RTOL,
                          maxit: int = None, pcg_iters: int = None, device="cuda"):
    """theta_eff [B] (fp64, on device): the homogenised coefficient of each theta field [n, n] or [B, n, n] along
    ``axis`` (0: across the rows, 1: across the columns).  Solves div(theta grad u) = 0 with u = 1 on the ghost nodes
    beyond the first wall of the axis, u = 0 beyond the second and the other two sides insulated (``"ddnn"`` /
    ``"nndd"`` with ``bc_data()``), and returns
        theta_eff = 0.5 (W_first - W_second) (n + 1) / n
    from ``wall_flux``: the flux per unit wall length over the mean gradient.  The ghost nodes are n + 1 cells apart
    and a wall is n cells wide, so a uniform theta gives theta exactly and h cancels.  Layers parallel to the flow give
    the mean of theta across them; layers across the flow with the harmonic mean give
    (n + 1) / (sum_a 1 / theta_a + 0.5 (1 / theta_0 + 1 / theta_{n-1})).

    Differentiable in theta by composition of the autograd ``solve_div`` with ``wall_flux``.  ``rtol`` and ``maxit``
    are ``solve_div``'s; ``pcg_iters`` = k selects its fixed-iteration mode (exactly k iterations, no host read, so the
    call is capturable once ``sep_plan(n, pattern)`` exists; ``pcg_iterations`` bounds k).  theta must be positive
    (checked where the host can see it: arrays and CPU tensors)."""
    if axis not in (0, 1):
        raise ValueError(f"effective_coefficient: axis must be 0 or 1, got {axis!r}")
    mean_name = FACE_MEANS[check_face_mean(face_mean)]
    if pcg_iters is not None and int(pcg_iters) < 1:
        raise ValueError("effective_coefficient: pcg_iters must be >= 1")
    if not isinstance(theta, torch.Tensor):
        theta = np.asarray(theta, dtype=np.float64)
    if len(theta.shape) not in (2, 3) or theta.shape[-1] != theta.shape[-2] or theta.shape[-1] < 2:
        raise ValueError(f"effective_coefficient: theta must be [n, n] or [B, n, n] with n >= 2, got "
                         f"{tuple(theta.shape)}")
    if isinstance(theta, np.ndarray):
        if not (theta > 0.0).all():
            raise ValueError("effective_coefficient: theta must be positive")
    elif theta.device.type == "cpu" and not bool((theta.detach() > 0).all()):
        raise ValueError("effective_coefficient: theta must be positive")
    theta = _dev_f64(theta, device)
    if theta.dim() == 2:
        theta = theta.unsqueeze(0)
    n = theta.shape[-1]
    pattern = EFFECTIVE_PATTERNS[axis]
    # the sides as device scalars: bc_data then copies nothing from the host, which a stream capture would refuse
    sides = {name: torch.full((), 1.0 if s == 2 * axis else 0.0, dtype=torch.float64, device=theta.device)
             for s, name in enumerate(SIDES)}
    data = bc_data(n, pattern, device=theta.device, **sides)
    fixed = pcg_iters is not None
    u = solve_div(torch.zeros_like(theta), theta, face_mean=mean_name, rtol=rtol,
                  maxit=int(pcg_iters) if fixed else maxit, check_every=0 if fixed else 8, check=not fixed,
                  device=device, bc=pattern, bc_data=data)
    W = wall_flux(u, theta, face_mean=mean_name, device=device, bc=pattern, bc_data=data)
    return (0.5 * (n + 1) / n) * (W[:, 2 * axis] - W[:, 2 * axis + 1])


def residual_metrics(u, f, theta, interior_only: bool = False, inv_h2: float = None, device="cuda",
                     form: str = "pointwise", face_mean: str = "harmonic", bc=None, bc_data=None):
    """How well raw fields satisfy the discrete equation: [E, 2] fp64 device tensor of (RMS, max abs) of
    theta * A u / h^2 - f per example (A the 5-point stencil with a zero ghost ring).  u [E, n, n] fp32 or fp64
    (a tensor keeps its precision), f and theta fp64.  ``inv_h2`` defaults to (n - 1)^2, the whole-domain operator
    solve_batched / solve_multi_resolution solve; ``interior_only`` leaves the boundary nodes out (a crop of a
    larger solve, whose ring is not zero).  Stream-ordered, no host sync (srpde_pde_residual_metrics).
    ``form="divergence"``: (RMS, max abs) of div(theta grad u) - f with ``face_mean`` instead, through apply_div, in
    fp64 whatever u's precision -- and, through apply_div, differentiable in u, f and theta when one of them requires
    grad (the pointwise metric is not); ``bc`` is apply_div's side pattern and belongs to that form, and so does
    ``bc_data``, apply_div's boundary data (the residual of A u = f with values on the sides); with ``interior_only``
    the data is refused: the ring is left out and no ghost face counts."""
    if bc_data is not None and check_form(form) != "divergence":
        raise ValueError('bc_data belongs to form="divergence" (apply_div): the pointwise operator has the zero ghost '
                         "ring")
    if bc_data is not None and interior_only:
        raise ValueError("residual_metrics: bc_data with interior_only: the ring is left out and no ghost face counts")
    if check_form(form) == "divergence":
        check_bc(bc)
        _bd_check(bc_data, f)
        f, theta, E, n = _div_fields(f, theta, device)
        u = _dev_f64(u, device).reshape(f.shape)
        res = apply_div(u, theta, face_mean, inv_h2, device, bc=bc, bc_data=bc_data) - f
        if interior_only:
            res = res[:, 1:-1, 1:-1]
        res = res.reshape(E, -1)
        return torch.stack([res.pow(2).mean(1).sqrt(), res.abs().amax(1)], dim=1)
    if bc is not None:
        raise ValueError('bc belongs to form="divergence" (apply_div): the pointwise operator has the zero ghost ring')
    from . import hipops as H
    if isinstance(u, torch.Tensor) and u.dtype == torch.float32:
        u = u.to(device).contiguous()
    else:
        u = _dev_f64(u, device)
    f, theta = _dev_f64(f, device), _dev_f64(theta, device)
    if u.dim() == 2:
        u, f, theta = u.unsqueeze(0), f.unsqueeze(0), theta.unsqueeze(0)
    if theta.shape != f.shape:
        theta = theta.expand_as(f).contiguous()
    n = u.shape[-1]
    return H.pde_residual_metrics(u, f, theta, float((n - 1) ** 2 if inv_h2 is None else inv_h2), interior_only)


def relax(u, f, theta, sweeps: int, omega: float = 0.8, interior_only: bool = False, inv_h2: float = None,
          device="cuda", form: str = "pointwise", face_mean: str = "harmonic", bc=None, bc_data=None):
    """``sweeps`` weighted-Jacobi sweeps of theta * A u / h^2 = f (A the 5-point stencil with a zero ghost ring):
    u <- u + (omega / 4) (A u - h^2 f / theta), each from the previous sweep's u.  It damps the error at the grid
    scale (for omega = 0.8 every component with a wavenumber >= pi / 2 shrinks by at least 0.6 per sweep) and, for
    0 < omega <= 1, grows none, so it polishes a field that is right at low frequencies: a cascade level's output.
    u, f [n, n] or [E, n, n], numpy or tensors; theta is broadcast.  ``inv_h2`` defaults to (n - 1)^2, the whole-domain
    operator that solve_batched solves and residual_metrics scores; ``interior_only`` holds the boundary nodes at
    their values (a crop of a larger solve, whose ring is not zero).  -> a new [E, n, n] fp64 device tensor.
    Stream-ordered, no host sync (srpde_pde_relax).
    ``form="divergence"``: the sweeps of div(theta grad u) = f with ``face_mean`` on the faces instead,
    u <- u + omega (D_theta u - f) / sum of the node's four face coefficients (srpde_div_relax; include/srpde.h states
    the rounding order); the same guarantee for 0 < omega <= 1.  ``face_mean`` belongs to that form.
    ``bc`` (``check_bc``, e.g. ``"ddnn"``), with that form: an "n" side is zero-flux -- its ghost faces have coefficient
    0, in the sum that divides as well (srpde_div_relax_bc) -- so a solve_div(bc=) solution is a fixed point of its own
    smoother.  ``"nnnn"`` is allowed (a sweep inverts nothing); ``interior_only`` and n < 2 are refused with a pattern.
    None (default) and ``"dddd"`` make today's call.
    ``bc_data`` (as for ``apply_div``), with that form: the sweeps of A u = f with values on the sides
    (srpde_div_relax_bd): the ghost nodes beyond "d" sides are held at g, a node on an "n" side sweeps with
    f - q * sqrt(inv_h2) in place of f, so a ``solve_div(bc_data=)`` solution is a fixed point -- a crop of a larger
    solution can be smoothed on its own with the ring around it as g.  Refused with ``interior_only`` and n < 2."""
    from . import hipops as H
    mean = face_mean_arg(form, face_mean)
    bc = check_bc(bc)
    if bc_data is not None:
        if mean is None:
            raise ValueError('bc_data belongs to form="divergence": the pointwise operator has the zero ghost ring')
        if interior_only:
            raise ValueError("relax: bc_data with interior_only: the ring is held and no ghost face is read")
        _bd_check(bc_data, u)
    if bc is not None:
        if mean is None:
            raise ValueError('bc belongs to form="divergence": the pointwise operator has the zero ghost ring')
        if interior_only:
            raise ValueError("relax: bc with interior_only: the ring is held and no ghost face is read")
        if (u.shape if hasattr(u, "shape") else np.shape(u))[-1] < 2:
            raise ValueError("relax: bc needs n >= 2 (a lone node's face coefficients can all be 0)")
    if int(sweeps) < 0:
        raise ValueError(f"relax: sweeps must be >= 0, got {sweeps}")
    if not 0.0 < float(omega) <= 1.0:
        raise ValueError(f"relax: omega must be in (0, 1], got {omega}")
    u, f, theta = _dev_f64(u, device), _dev_f64(f, device), _dev_f64(theta, device)
    if u.dim() == 2:
        u, f = u.unsqueeze(0), f.unsqueeze(0)
    if theta.shape != f.shape:
        theta = theta.expand_as(f).contiguous()
    n = u.shape[-1]
    inv_h2 = float((n - 1) ** 2 if inv_h2 is None else inv_h2)
    if bc_data is not None:
        bd = _bd_fields(bc_data, u, u.device).detach()
        return H.pde_relax(u, f, theta, inv_h2, int(sweeps), float(omega), False, mean, bc, bd)
    return H.pde_relax(u, f, theta, inv_h2, int(sweeps), float(omega), interior_only, mean, bc)


def solve_batched(f, theta, rtol: float = DEFAULT_RTOL, maxit: int = None, device="cuda",
                  return_iters: bool = False, check: bool = True, _start_aborted: bool = False,
                  method: str = "cg", form: str = "pointwise", face_mean: str = "harmonic", u0=None,
                  shift: float = 0.0, precond_shift: float = None, bc=None):
    """u[B, n, n] (float64, on device) with theta*Lap(u) = f per problem.

    ``form="divergence"`` solves div(theta grad u) = f instead (solve_div, which has one solver: ``method`` and
    ``_start_aborted`` are refused; ``return_iters`` gives its iteration counts; ``u0`` is its initial guess, which
    the pointwise form and ``method="dst"`` refuse; ``shift`` / ``precond_shift`` solve div(theta grad u) - shift u
    = f, as solve_div does -- the pointwise forms refuse them too: theta * L - shift is not diagonalised by the sine
    transform and their CG kernels have no shift; ``bc`` is solve_div's side pattern, refused likewise).

    ``method="dst"`` solves directly (solve_direct): there is nothing to iterate, so ``return_iters`` gives
    zeros and non-default ``rtol`` / ``maxit`` / ``check`` / ``_start_aborted`` are refused.

    For n above the LDS solver's limit the solve runs as cooperative launches whose grid barriers
    abort after ~1 s of waiting (srpde_poisson_cg_batched marks those problems iters = -1 and
    leaves u unconverged).  ``check`` (default) reads the iteration counts back -- one host sync,
    only on that path, not under stream capture -- and raises GridBarrierAbort instead of returning
    such a u (every data-generation caller otherwise consumed it silently)."""
    if face_mean_arg(form, face_mean) is not None:
        if method != "cg" or _start_aborted:
            raise ValueError('form="divergence" has one solver (solve_div): method and _start_aborted do not apply')
        u, iters, _ = solve_div(f, theta, face_mean=face_mean, rtol=rtol, maxit=maxit, check=check, return_info=True,
                                device=device, u0=u0, shift=shift, precond_shift=precond_shift, bc=bc)
        return (u, iters) if return_iters else u
    if bc is not None:
        raise ValueError('bc belongs to form="divergence" (solve_div): the pointwise solvers have the zero ghost ring')
    if check_shift(shift) != 0.0 or precond_shift is not None:
        raise ValueError('shift and precond_shift belong to form="divergence" (solve_div): the pointwise solvers '
                         "have no shifted operator")
    if u0 is not None:
        raise ValueError('u0 belongs to form="divergence" (solve_div): the pointwise solvers start from zero')
    if check_solver(method) == "dst":
        if rtol != DEFAULT_RTOL or maxit is not None or check is not True or _start_aborted:
            raise ValueError('method="dst" is a direct solve: rtol, maxit, check and _start_aborted do not apply')
        u = solve_direct(f, theta, device=device)
        return (u, torch.zeros(u.shape[0], dtype=torch.int32, device=u.device)) if return_iters else u
    f = _dev_f64(f, device)
    theta = _dev_f64(theta, device)
    if f.dim() == 2:
        f, theta = f.unsqueeze(0), theta.unsqueeze(0)
    if theta.shape != f.shape:
        theta = theta.expand_as(f).contiguous()
    B, n, n2 = f.shape
    if n != n2:
        raise ValueError("square grids only")
    if maxit is None:
        maxit = 20 * n * n
    u = torch.empty_like(f)
    iters = torch.empty(B, dtype=torch.int32, device=device)
    if B == 0:               # an empty rank shard: the C entry rejects B = 0, there is nothing to solve
        return (u, iters) if return_iters else u
    ws_bytes = int(query("srpde_poisson_workspace_size", B, n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
    # (_start_aborted, a test hook: the C entry's negative rtol -- every grid-CG launch starts aborted)
    call("srpde_poisson_cg_batched", f.data_ptr(), theta.data_ptr(), u.data_ptr(), B, n,
         -float(rtol) if _start_aborted else float(rtol), int(maxit),
         iters.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr())
    if check and n > int(query("srpde_poisson_lds_max_n")) and not torch.cuda.is_current_stream_capturing():
        bad = int((iters < 0).sum())
        if bad:
            raise GridBarrierAbort(f"srpde_poisson_cg_batched: {bad} of {B} problems (n={n}) aborted at a grid "
                                   "barrier; their u is not a solution")
    return (u, iters) if return_iters else u


def solve_rows_sharded(f, theta, rtol: float = DEFAULT_RTOL, maxit: int = None, device="cuda", group=None,
                       check_every: int = 64, return_iters: bool = False):
    """ONE n x n problem (theta*Lap(u) = f) with its rows sharded over the ranks of ``group``
    (the ground-truth solve of solve_multi_resolution, resolution_comparison.py:62-73):
    every rank passes the whole f / theta (the seeded draws are replicated), solves the rows
    shard_range(n, rank, world) with the srpde_poisson_rows_* kernels -- per iteration two launches
    and two all-gathers (one scalar, then the rank's <r,r> partial with its first / last rows of r and
    p, which is what the neighbours' stencils need) -- and all ranks return the full u[n, n].  At
    world 1 (no process group) it runs the same kernels without collectives."""
    import torch.distributed as dist

    from .data_generation import shard_range
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    f = _dev_f64(f, device)
    theta = _dev_f64(theta, device)
    if theta.shape != f.shape:
        theta = theta.expand_as(f).contiguous()
    n = f.shape[-1]
    if f.dim() != 2 or f.shape[0] != n:
        raise ValueError("one square problem [n, n]")
    if world > n:
        raise ValueError(f"more ranks ({world}) than grid rows ({n})")
    if maxit is None:
        maxit = 20 * n * n
    lo, hi = shard_range(n, rank, world)
    nloc = hi - lo
    fl, tl = f[lo:hi].contiguous(), theta[lo:hi].contiguous()
    ws_bytes = int(query("srpde_poisson_rows_workspace_size", n, nloc))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=device)
    done_at = int(query("srpde_poisson_rows_done_offset", n, nloc))
    done = ws[done_at:done_at + 4].view(torch.int32)
    send = torch.zeros(4 * n + 1, dtype=torch.float64, device=device)
    spq = torch.zeros(1, dtype=torch.float64, device=device)
    if world > 1:
        gath = torch.zeros(world, 4 * n + 1, dtype=torch.float64, device=device)
        gpq = torch.zeros(world, 1, dtype=torch.float64, device=device)
        gath_parts, gpq_parts = list(gath.unbind(0)), list(gpq.unbind(0))

        def gather_send():
            dist.all_gather(gath_parts, send, group=group)

        def gather_pq():
            dist.all_gather(gpq_parts, spq, group=group)
    else:
        gath, gpq = send, spq
        gather_send = gather_pq = (lambda: None)
    sp = stream_ptr()
    call("srpde_poisson_rows_init", fl.data_ptr(), tl.data_ptr(), n, nloc, ws.data_ptr(), ws_bytes,
         send.data_ptr(), sp)
    gather_send()
    for k in range(maxit + 1):
        call("srpde_poisson_rows_iter_a", n, nloc, lo, rank, world, gath.data_ptr(), k, int(maxit), float(rtol),
             ws.data_ptr(), ws_bytes, spq.data_ptr(), sp)
        gather_pq()
        call("srpde_poisson_rows_iter_b", n, nloc, world, gath.data_ptr(), gpq.data_ptr(), k, ws.data_ptr(),
             ws_bytes, send.data_ptr(), sp)
        gather_send()
        # every rank decides convergence from the same gathered values, so all leave together
        if (k + 1) % check_every == 0 and int(done.item()):
            break
    ul = torch.empty(nloc, n, dtype=torch.float64, device=device)
    it = torch.zeros(1, dtype=torch.int32, device=device)
    call("srpde_poisson_rows_finish", ul.data_ptr(), it.data_ptr(), n, nloc, int(maxit), ws.data_ptr(), ws_bytes, sp)
    if world > 1:
        counts = [shard_range(n, r, world) for r in range(world)]
        cmax = max(b - a for a, b in counts)
        pad = torch.zeros(cmax, n, dtype=torch.float64, device=device)
        pad[:nloc] = ul
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad, group=group)
        u = torch.cat([parts[r][:b - a] for r, (a, b) in enumerate(counts)])
    else:
        u = ul
    return (u, int(it.item())) if return_iters else u
