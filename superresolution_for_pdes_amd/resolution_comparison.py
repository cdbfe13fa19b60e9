"""Multi-level cascade inference + multi-resolution ground truth (config #5) on MI355X.

Reference: src/resolution_comparison.py:13-229.  Semantics kept:
  * ``solve_multi_resolution``: one (f, theta ~ U(0.5, 2)) field on the finest grid, strided
    to every resolution, each solved with h = 1/(res-1) (the reference's quirk, :56-73) --
    here by the batched HIP CG instead of SuperLU;
  * ``ml_multi_level_upscale``: per level, GROUND-TRUTH statistics at the next resolution
    normalise the inputs (:196-201, a label leak the reference has, reproduced for parity),
    20^2 tiles -> normalise -> bilinear to 40^2 -> U-Net (eval) -> denormalise -> stitch.
Difference: every level runs as ONE batched forward of all its tiles (1, 4, 16, 64, 256
tiles for 20 -> 640) instead of the reference's batch-1 Python loop (:211-223), and the
start resolution is a parameter (config #5 starts at 20).
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import poisson as P
from .models import upsample_bilinear


def _world() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def solve_multi_resolution(n_coarse: int = 40, resolutions: List[int] = (80, 160, 320, 640), device="cuda",
                           verbose: bool = False, shard_gt: bool = False, solver: str = "cg"):
    """resolution_comparison.py:13-78 with the GT solves on device (returns numpy fields).

    ``solver``: "cg" or "dst" (poisson.solve_batched's method); the row-sharded solve of ``shard_gt`` is CG.

    ``shard_gt``: under a process group of world > 1, the finest level's solve runs row-sharded
    over the ranks (poisson.solve_rows_sharded); every rank still returns every
    field.  Off by default: at 640^2 the solve is latency-bound (two collectives per CG
    iteration), and the replicated single-GPU solve is the faster one."""
    resolutions = list(resolutions)
    P.check_solver(solver)
    k1 = np.random.uniform(10.0, 11.0)
    k2 = np.random.uniform(10.0, 11.0)
    n_finest = max(resolutions)
    x = np.linspace(0, 1, n_finest)
    X, Y = np.meshgrid(x, x)
    f_finest = np.sin(k1 * 2 * np.pi * X) * np.sin(k2 * 2 * np.pi * Y)   # host, as the reference (:36)
    theta_finest = np.random.uniform(0.5, 2.0, size=(n_finest, n_finest))
    data = {"k1": k1, "k2": k2, "f": {}, "theta": {}, "u": {}}
    for res in [n_coarse] + resolutions:
        step = n_finest // res
        data["f"][res] = f_finest if res == n_finest else f_finest[::step, ::step]
        data["theta"][res] = theta_finest if res == n_finest else theta_finest[::step, ::step]
        if shard_gt and res == n_finest and _world() > 1:
            data["u"][res] = P.solve_rows_sharded(data["f"][res], data["theta"][res], device=device).cpu().numpy()
        else:
            data["u"][res] = P.solve_batched(data["f"][res], data["theta"][res], device=device,
                                             method=solver)[0].cpu().numpy()
        if verbose:
            print(f"u_{res} - min: {data['u'][res].min():.6f}, max: {data['u'][res].max():.6f}")
    return data


class GlobalNormalization:
    """resolution_comparison.py:160-181 (fp32 statistics, unbiased std)."""

    def __init__(self, u_fine, u_coarse, f_fine, theta_fine, device="cuda", theta_is_constant=None):
        """``theta_is_constant``: the reference's std < 1e-6 test, if already known (the test is
        a host sync; a graph-captured cascade takes it from its capture)."""
        t = lambda a: _field(a, device, torch.float32)  # noqa: E731
        u_fine, f_fine, theta_fine = t(u_fine), t(f_fine), t(theta_fine)
        self.u_mean, self.u_std = u_fine.mean(), u_fine.std()
        self.f_mean, self.f_std = f_fine.mean(), f_fine.std()
        self.theta_is_constant = (bool(theta_fine.std() < 1e-6) if theta_is_constant is None
                                  else bool(theta_is_constant))
        if self.theta_is_constant:
            self.theta_mean, self.theta_std = 0, 1
        else:
            self.theta_mean, self.theta_std = theta_fine.mean(), theta_fine.std()


def _tiles(a: torch.Tensor, s: int) -> torch.Tensor:
    """[R, R] -> [(R/s)^2, s, s] row-major tile order (split_into_subdomains, :123-139)."""
    m = a.shape[0] // s
    return a.reshape(m, s, m, s).permute(0, 2, 1, 3).reshape(m * m, s, s)


def _stitch(t: torch.Tensor) -> torch.Tensor:
    """inverse of _tiles (stitch_subdomains, :141-158)."""
    T, s, _ = t.shape
    m = int(round(T ** 0.5))
    return t.reshape(m, m, s, s).permute(0, 2, 1, 3).reshape(m * s, m * s)


def split_into_subdomains(array: np.ndarray, subdomain_size: int) -> list:
    m = array.shape[0] // subdomain_size
    return [[array[i * subdomain_size:(i + 1) * subdomain_size, j * subdomain_size:(j + 1) * subdomain_size]
             for j in range(m)] for i in range(m)]


def stitch_subdomains(subdomains: list) -> np.ndarray:
    s = subdomains[0][0].shape[0]
    out = np.zeros((len(subdomains) * s, len(subdomains[0]) * s))
    for i, row in enumerate(subdomains):
        for j, t in enumerate(row):
            out[i * s:(i + 1) * s, j * s:(j + 1) * s] = t
    return out


def _blocks_to_tiles(b: torch.Tensor, s: int) -> torch.Tensor:
    """[nb, S, S] -> [nb * (S/s)^2, s, s]: block-major, row-major tiles inside each block."""
    nb, S, _ = b.shape
    m = S // s
    return b.reshape(nb, m, s, m, s).permute(0, 1, 3, 2, 4).reshape(nb * m * m, s, s)


def _tiles_to_blocks(t: torch.Tensor, nb: int) -> torch.Tensor:
    """inverse of _blocks_to_tiles: [nb * m^2, s, s] -> [nb, m*s, m*s]."""
    T, s, _ = t.shape
    m = int(round((T // nb) ** 0.5))
    return t.reshape(nb, m, m, s, s).permute(0, 1, 3, 2, 4).reshape(nb, m * s, m * s)


def _level_inputs(u_cur, f_next, th_next, norm, tile=20):
    """Normalised model inputs for every tile of one level: [T, 3, 2*tile, 2*tile].

    Fields are [S, S] (whole domain) or [nb, S, S] blocks (a rank's subtrees)."""
    if u_cur.dim() == 2:
        u_cur, f_next, th_next = u_cur[None], f_next[None], th_next[None]
    uc = _blocks_to_tiles(u_cur.float(), tile)
    ft = _blocks_to_tiles(f_next.float(), 2 * tile)
    tt = _blocks_to_tiles(th_next.float(), 2 * tile)
    ucn = (uc - norm.u_mean) / norm.u_std
    fn = (ft - norm.f_mean) / norm.f_std
    tn = tt if norm.theta_is_constant else (tt - norm.theta_mean) / norm.theta_std
    up = upsample_bilinear(ucn.unsqueeze(1).contiguous(), 2 * tile, 2 * tile)
    return torch.cat([up, tn.unsqueeze(1), fn.unsqueeze(1)], dim=1).contiguous()


def upscale_subdomain(model, u_coarse, f_fine, theta_fine, global_norm, device="cuda") -> np.ndarray:
    """Single-tile API of the reference (:80-121)."""
    dev = lambda a: torch.as_tensor(np.asarray(a)).to(device=device, dtype=torch.float64)  # noqa: E731
    x = _level_inputs(dev(u_coarse), dev(f_fine), dev(theta_fine), global_norm, tile=u_coarse.shape[0])
    with torch.no_grad():
        y = model(x) * global_norm.u_std + global_norm.u_mean
    return y.squeeze().double().cpu().numpy()


def _field(a, device, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device=device, dtype=dtype or t.dtype)


def _shard(shard):
    if shard is not None:
        return shard
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


@torch.no_grad()
def eval_forward(model, x: torch.Tensor, graphs: bool = True) -> torch.Tensor:
    """Eval-mode U-Net forward.  On the GPU with ``graphs`` the forward of each input shape is
    captured once into a HIP graph (torch.cuda.CUDAGraph) and replayed: a cascade level is then
    one copy and one graph launch instead of ~100 kernel launches from Python (the small levels
    are launch-bound).  Replays run the same kernels on the same buffers, so the output is
    bit-identical to the eager forward.  A graph is keyed on the weight split's cache key
    (unet_exec.prepare_h3_weights): a weight change re-captures."""
    if not (graphs and x.is_cuda):
        with torch.no_grad():
            return model(x)
    from . import unet_exec as X
    with torch.no_grad():
        model.flatten_parameters_()
        X.prepare_h3_weights(model)          # eval: a no-op unless a weight changed
    key = (tuple(x.shape), x.device, getattr(model, "_srpde_h3w_key", None))
    cache = model.__dict__.setdefault("_srpde_graphs", {})
    ent = cache.get(key)
    if ent is None or key[2] is None:
        for k in [k for k in cache if k[2] != key[2]]:   # graphs of older weights
            del cache[k]
        xs = x.clone()
        with torch.no_grad():
            model(xs)                        # warm-up: lazily created scratch exists before capture
            torch.cuda.current_stream(x.device).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ys = model(xs)
        ent = cache[key] = (g, xs, ys)
    g, xs, ys = ent
    xs.copy_(x)
    g.replay()
    return ys.clone()


def ml_multi_level_upscale(model, data: dict, target_resolution: int, device: str = "cuda",
                           start_resolution: int = 40, tile: int = 20, return_tensor: bool = False,
                           max_batch: int = 4096, shard=None, graphs: bool = True):
    """resolution_comparison.py:183-229 with one batched U-Net forward per level.

    Multi-GPU: a level-(L+1) tile depends on one quadrant of one level-L
    tile only, so the cascade is a forest.  Levels with fewer tiles than ranks run on every
    rank (1 and 4 tiles for 20 -> 640); at the first level with >= world tiles each rank
    takes a contiguous share of them as subtree roots and carries only its own blocks down
    to the target resolution; one all-gather assembles the field.  The per-level
    normalisation statistics come from the (replicated) ground truth, so the subtrees need
    no other exchange.  ``shard`` = (rank, world); default: the torch.distributed world."""
    model.eval()
    rank, world = _shard(shard)
    levels = []
    r = start_resolution
    while r < target_resolution:
        r *= 2
        levels.append(r)
    if graphs and world == 1 and torch.device(device).type == "cuda" and all(
            isinstance(data[k][r], torch.Tensor) and data[k][r].is_cuda
            for k in ("u", "f", "theta") for r in levels + [start_resolution] if k == "u" or r != start_resolution):
        out = _cascade_graphed(model, data, target_resolution, start_resolution, tile, max_batch, levels, device)
    else:
        out = _cascade(model, data, target_resolution, start_resolution, tile, max_batch, rank, world, device,
                       graphs)
    return out if return_tensor else out.cpu().numpy()


def _cascade_graphed(model, data, target_resolution, start_resolution, tile, max_batch, levels, device):
    """The whole cascade (statistics, tiling, five U-Net forwards, stitching) captured once into
    one HIP graph per (data tensors, geometry, weights) and replayed; the theta-constant tests
    (host syncs) run once, at capture.  Bit-identical to the eager cascade."""
    from . import unet_exec as X
    with torch.no_grad():
        model.flatten_parameters_()
        X.prepare_h3_weights(model)
    wkey = getattr(model, "_srpde_h3w_key", None)
    sig = tuple((k, r, data[k][r].data_ptr(), data[k][r]._version) for k in ("u", "f", "theta")
                for r in sorted(data[k]) if r in levels or (k == "u" and r == start_resolution))
    key = ("cascade", target_resolution, start_resolution, tile, max_batch, sig, wkey)
    cache = model.__dict__.setdefault("_srpde_graphs", {})
    ent = cache.get(key) if wkey is not None else None
    if ent is None:
        for k in [k for k in cache if k[0] == "cascade"]:   # one cascade graph at a time
            del cache[k]
        flags = {r: bool(_field(data["theta"][r], device, torch.float32).std() < 1e-6) for r in levels}

        def run():
            return _cascade(model, data, target_resolution, start_resolution, tile, max_batch, 0, 1, device,
                            False, flags)
        with torch.no_grad():
            run()                               # warm-up (lazily created buffers exist before capture)
            torch.cuda.current_stream(torch.device(device)).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = run()
        ent = (g, out)
        if wkey is not None:
            cache[key] = ent
    g, out = ent
    g.replay()
    return out.clone()


def _cascade(model, data, target_resolution, start_resolution, tile, max_batch, rank, world, device, graphs,
             flags=None):
    """The level loop of ml_multi_level_upscale (eager launches; per-level graphs if ``graphs``)."""
    cur_res = start_resolution
    cur = _field(data["u"][cur_res], device, torch.float64)[None]   # [nb, S, S] blocks
    roots, m_split = None, None     # owned root-tile indices, tiles per side at the split level
    # every level's statistics up front: their host syncs (the theta-constant test) then come
    # before the level loop, which the host can queue ahead of the GPU
    norms, r = {}, cur_res
    while r < target_resolution:
        r *= 2
        norms[r] = GlobalNormalization(data["u"][r], None, data["f"][r], data["theta"][r], device=device,
                                       theta_is_constant=None if flags is None else flags[r])
    while cur_res < target_resolution:
        nxt = cur_res * 2
        if roots is None and world > 1 and (cur_res // tile) ** 2 >= world:
            m_split = cur_res // tile
            roots = np.array_split(np.arange(m_split * m_split), world)[rank]
            cur = _blocks_to_tiles(cur, tile)[torch.as_tensor(roots, device=cur.device)]
        norm = norms[nxt]
        f_next = _field(data["f"][nxt], device)[None]
        th_next = _field(data["theta"][nxt], device)[None]
        if roots is not None:  # this rank's regions of the next-level forcing / coefficient
            s2 = nxt // m_split
            idx = torch.as_tensor(roots, device=f_next.device)
            f_next = _blocks_to_tiles(f_next, s2)[idx]
            th_next = _blocks_to_tiles(th_next, s2)[idx]
        x = _level_inputs(cur, f_next, th_next, norm, tile)
        outs = [eval_forward(model, x[s:s + max_batch], graphs) for s in range(0, x.shape[0], max_batch)]
        y = torch.cat(outs) * norm.u_std + norm.u_mean
        cur = _tiles_to_blocks(y[:, 0].double(), cur.shape[0])
        cur_res = nxt
    if roots is not None:
        cur = _gather_blocks(cur, m_split, world)
    return cur[0] if cur.shape[0] == 1 else _tiles_to_blocks(cur, 1)[0]


def _gather_blocks(blocks: torch.Tensor, m_split: int, world: int) -> torch.Tensor:
    """All ranks' subtree blocks -> [m_split^2, S, S] in root order (one all-gather)."""
    import torch.distributed as dist
    counts = [len(a) for a in np.array_split(np.arange(m_split * m_split), world)]
    cmax = max(counts)
    S = blocks.shape[-1]
    pad = blocks.new_zeros(cmax, S, S)
    pad[:blocks.shape[0]] = blocks
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat([parts[r][:counts[r]] for r in range(world)])


def cascade_metrics(pred: np.ndarray, gt: np.ndarray) -> dict:
    d = np.asarray(pred, np.float64) - np.asarray(gt, np.float64)
    return {"mae": float(np.mean(np.abs(d))), "rmse": float(np.sqrt(np.mean(d * d))),
            "max_error": float(np.max(np.abs(d)))}
