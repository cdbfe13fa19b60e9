"""Cascade inference on a user's own fields: overlapping windows, no ground truth (csrc/tiled.hip, ABI 16).

``resolution_comparison_statistical.ml_multi_level_upscale_batched`` reproduces the reference's study: it
normalises every level with the statistics of that level's ground-truth solution, cuts the domain into disjoint
20^2 tiles (so the field size must be a multiple of 20) and pastes the 40^2 outputs side by side.  This module is
the path for someone who has a coarse solution plus f and theta on the fine grids and nothing else:

  * ``stats="input"``: u statistics from the coarse field the level is given, f / theta statistics from the fine
    fields (hipops.tiled_level_stats); ``"truth"`` keeps the reference's behaviour and needs the solution;
    a tensor passes fixed statistics in (e.g. the frozen ones a model was trained with);
  * windows of ``tile``^2 coarse points every ``stride`` points, the last one clamped to the edge, so any
    S >= tile works; their outputs are blended with a partition of unity (``window="linear"``: a separable
    triangle weight that is smallest at a window's border; ``"flat"``: the plain mean of the covering windows).

With ``stride == tile``, ``stats="truth"``, S a multiple of the tile and the same ``max_batch`` the result is bit-equal
to ml_multi_level_upscale_batched.  A level is four passes (statistics, assemble, the U-Net, blend), all stream-ordered,
with no host synchronisation.

``polish=k`` (default 0: nothing changes, no extra launch) ends a level with k weighted-Jacobi sweeps of the level's own
equation, poisson.relax(blend, f_next, theta_next, k, polish_omega, inv_h2=(2S - 1)^2): the U-Net is the prolongation,
this the post-smoother that takes out the grid-scale error the network leaves, also before the next level reads it.
``polish_form="divergence"`` (with ``polish_face_mean``) polishes with the sweeps of div(theta grad u) = f instead, for
fields that solve the conservative problem; the defaults keep the pointwise sweep.
"""
from __future__ import annotations

import numbers
from typing import Dict, List

import numpy as np
import torch

from . import hipops as H
from . import poisson as P
from .resolution_comparison import eval_forward


# Windows per U-Net call.  srpde_conv_fwd_h3 addresses an activation tensor with 32-bit byte offsets and refuses a
# larger one ("tensor too large"): 4096 windows of 40^2 are refused, the 2560 of the disjoint cascade (E = 10 at
# 320 -> 640) pass.  Overlapping windows exceed that easily (stride 10: 9610), so the default chunk is 2048.
MAX_BATCH = 2048


def tile_starts(S: int, tile: int = 20, stride: int = 10) -> List[int]:
    """The window origins on one axis of an S-point grid: min(k stride, S - tile) for k = 0 .. m - 1,
    m = ceil((S - tile) / stride) + 1 (srpde_tiled_tiles_per_side).  Pure Python."""
    if not 1 <= stride <= tile <= S:
        raise ValueError(f"tile_starts: need 1 <= stride <= tile <= S, got S={S} tile={tile} stride={stride}")
    m = -(-(S - tile) // stride) + 1
    return [min(k * stride, S - tile) for k in range(m)]


def _f64(a, device) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.to(device=device, dtype=torch.float64)
    return (t[None] if t.dim() == 2 else t).contiguous()


def _check_polish(name, polish, polish_omega, polish_form="pointwise", polish_face_mean="harmonic", polish_bc=None):
    if not isinstance(polish, numbers.Integral) or polish < 0:
        raise ValueError(f"{name}: polish must be an integer >= 0, got {polish!r}")
    if not 0.0 < float(polish_omega) <= 1.0:
        raise ValueError(f"{name}: polish_omega must be in (0, 1], got {polish_omega!r}")
    P.check_face_mean(polish_face_mean)
    if P.check_form(polish_form) == "pointwise" and polish_face_mean != "harmonic":
        raise ValueError(f'{name}: polish_face_mean belongs to polish_form="divergence"')
    if P.check_bc(polish_bc) is not None and polish_form != "divergence":
        raise ValueError(f'{name}: polish_bc belongs to polish_form="divergence"')


def _level_stats(stats, u_cur, f_next, theta_next, u_next):
    E = u_cur.shape[0]
    if isinstance(stats, torch.Tensor):
        s = stats.to(device=u_cur.device, dtype=torch.float32)
        if s.shape == (6,):
            s = s[None].expand(E, 6)
        if s.shape != (E, 6):
            raise ValueError(f"upscale_level: a stats tensor must be [6] or [E, 6], got {tuple(stats.shape)}")
        return s.contiguous()
    if stats == "input":
        return H.tiled_level_stats(u_cur, f_next, theta_next)[0]
    if stats == "truth":
        if u_next is None:
            raise ValueError("upscale_level: stats='truth' needs the next level's solution (u_next=)")
        return H.cascade_level_stats(_f64(u_next, u_cur.device), f_next, theta_next)[0]
    raise ValueError(f"upscale_level: stats must be 'input', 'truth' or a tensor, got {stats!r}")


@torch.no_grad()
def upscale_level(model, u_cur, f_next, theta_next, *, tile: int = 20, stride: int = 10, window: str = "linear",
                  stats="input", max_batch: int = MAX_BATCH, graphs: bool = True, u_next=None, polish: int = 0,
                  polish_omega: float = 0.8, polish_form: str = "pointwise",
                  polish_face_mean: str = "harmonic", polish_bc=None) -> torch.Tensor:
    """One level: u_cur [E, S, S] with f_next / theta_next [E, 2S, 2S] -> [E, 2S, 2S] fp64 on the model's device.

    ``stats``: "input" (no ground truth), "truth" (needs ``u_next``: cascade_level_stats of the next level's
    solution, as the reference) or an [E, 6] / [6] fp32 tensor {u_mean, u_std, f_mean, f_std, theta_mean, theta_std}.
    The U-Net runs through eval_forward in chunks of ``max_batch`` windows.  ``polish`` > 0: that many
    weighted-Jacobi sweeps (``polish_omega`` in (0, 1]) of the whole-domain equation on the blended field:
    theta * L u = f, or div(theta grad u) = f with ``polish_form="divergence"`` and ``polish_face_mean``;
    ``polish_bc`` (poisson.check_bc, e.g. ``"ddnn"``) gives that form's sweeps zero-flux sides."""
    _check_polish("upscale_level", polish, polish_omega, polish_form, polish_face_mean, polish_bc)
    model.eval()
    device = next(model.parameters()).device
    u_cur, f_next, theta_next = (_f64(a, device) for a in (u_cur, f_next, theta_next))
    E, S = u_cur.shape[0], u_cur.shape[-1]
    if window not in H.TILED_WINDOWS:
        raise ValueError(f"upscale_level: window must be one of {sorted(H.TILED_WINDOWS)}")
    H.tiled_tiles_per_side(S, tile, stride)     # a bad geometry fails before any launch
    st = _level_stats(stats, u_cur, f_next, theta_next, u_next)
    x = H.tiled_assemble(u_cur, f_next, theta_next, st, tile, stride)
    outs = [eval_forward(model, x[s:s + max_batch], graphs) for s in range(0, x.shape[0], max_batch)]
    y = outs[0] if len(outs) == 1 else torch.cat(outs)
    u = H.tiled_blend_denorm(y.contiguous(), st, E, S, tile, stride, window)
    if polish > 0:
        u = P.relax(u, f_next, theta_next, polish, polish_omega, inv_h2=float((2 * S - 1) ** 2), device=device,
                    form=polish_form, face_mean=polish_face_mean, bc=polish_bc)
    return u


@torch.no_grad()
def upscale_cascade(model, u_start, f: Dict[int, object], theta: Dict[int, object], target_resolution: int, *,
                    tile: int = 20, stride: int = 10, window: str = "linear", stats="input", max_batch: int = MAX_BATCH,
                    graphs: bool = True, u_truth: Dict[int, object] = None, polish: int = 0,
                    polish_omega: float = 0.8, polish_form: str = "pointwise",
                    polish_face_mean: str = "harmonic", polish_bc=None) -> torch.Tensor:
    """The level loop: from u_start [E, S0, S0] by doublings to ``target_resolution``; ``f`` and ``theta`` are
    {res: [E, res, res]} for every resolution above S0 on the way.  ``u_truth`` {res: [E, res, res]} is needed for
    stats="truth" only.  ``polish`` / ``polish_omega`` / ``polish_form`` / ``polish_face_mean`` / ``polish_bc``: as
    upscale_level, at every level, so the next level reads the polished field.  -> [E, target, target] fp64 (device
    tensor)."""
    _check_polish("upscale_cascade", polish, polish_omega, polish_form, polish_face_mean, polish_bc)
    device = next(model.parameters()).device
    cur = _f64(u_start, device)
    res = cur.shape[-1]
    ratio = target_resolution // res
    if target_resolution <= res or target_resolution % res or ratio & (ratio - 1):
        raise ValueError(f"upscale_cascade: target {target_resolution} is not {res} times a power of two")
    if isinstance(stats, str) and stats == "truth" and u_truth is None:
        raise ValueError("upscale_cascade: stats='truth' needs u_truth")
    while res < target_resolution:
        nxt = res * 2
        cur = upscale_level(model, cur, f[nxt], theta[nxt], tile=tile, stride=stride, window=window, stats=stats,
                            max_batch=max_batch, graphs=graphs, u_next=None if u_truth is None else u_truth[nxt],
                            polish=polish, polish_omega=polish_omega, polish_form=polish_form,
                            polish_face_mean=polish_face_mean, polish_bc=polish_bc)
        res = nxt
    return cur
