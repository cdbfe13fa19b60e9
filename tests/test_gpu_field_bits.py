"""The fp64 field kernels (csrc/cascade.hip, tiled.hip, physics.hip, poisson_div.hip) against bits recorded before
their reductions, statistics and assemble kernels were merged (csrc/field_reduce.h, cascade_level.h): every output
here must equal tests/golden/field_bits*.npz bit for bit.  The other tests of these files compare the kernels with
each other and with numpy; only this one can tell "the same bits as before" from "self-consistent".

    python tests/test_gpu_field_bits.py --record [DIR]     # rewrites the fixture from the library as built

Inputs come from numpy generators with fixed seeds (no libm call on the way, so they are the same bits anywhere);
the fixture holds the outputs' int32 / int64 views.  If an array differs, a kernel's arithmetic changed: that is a
bug in the kernel, not a reason to record again.

Shapes: the smallest that take each path.  Statistics: n = 40 is one workgroup per field, n = 94 five; tiled S = 47
has 2 workgroups for u beside 5 for f and theta.  Example 1's theta is constant, the last example's within 17 ulp of 1.
Windows (S, tile, stride): (47, 20, 10) overlapping with a clamped last window, (40, 20, 20) disjoint.  Physics loss
B = 3, n = 20: a workgroup with two samples beside one with one.  solve_div n = 70: 2 x 3 tiles, so every scalar is a
re-sum of 6 partials; 6 iterations in fixed mode."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = np.array([[2e-4, 1e-4, 0.1, 0.5, 1.2, 0.4], [-3.1e-4, 2.3e-4, 0.1, 0.5, 0, 1], [1.7e-4, 0.9e-4, -0.2, 0.7, 1.1, 0.3]],
                 np.float32)
GEOMETRIES = [(47, 20, 10), (40, 20, 20)]


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.float32, torch.float64):
        t = t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return t.cpu().numpy()


def _level_fields(E, S, n, seed):
    """u [E, S, S] ~ N(2e-4, 1e-4), f ~ U(-0.9, 1.1) and theta ~ U(0.5, 2) on [E, n, n]; example 1: theta = 1.3
    everywhere; the last example, E >= 3: half the thetas 1, half 1 + 17 * 2^-23."""
    rng = np.random.default_rng(seed)
    u = rng.normal(2e-4, 1e-4, (E, S, S))
    f = rng.uniform(-0.9, 1.1, (E, n, n))
    th = rng.uniform(0.5, 2.0, (E, n, n))
    th[1] = 1.3
    if E >= 3:
        th[E - 1] = np.where(rng.permutation(n * n) < n * n // 2, 1.0, 1.0 + 17 * 2.0 ** -23).reshape(n, n)
    return _dev(u), _dev(f), _dev(th)


def g_cascade_stats(H):
    out = {}
    for n in (40, 94):
        stats, flags = H.cascade_level_stats(*_level_fields(3, n, n, 100 + n))
        assert flags.tolist() == [0, 1, 0]
        out[f"stats{n}"], out[f"flags{n}"] = _bits(stats), _bits(flags)
    return out


def g_tiled_stats(H):
    out = {}
    for S in (20, 47):
        stats, flags = H.tiled_level_stats(*_level_fields(2, S, 2 * S, 200 + S))
        assert flags.tolist() == [0, 1]
        out[f"stats{S}"], out[f"flags{S}"] = _bits(stats), _bits(flags)
    return out


def g_cascade_assemble(H):
    u, f, th = _level_fields(3, 40, 80, 300)
    return {"x": _bits(H.cascade_level_assemble(u, f, th, _dev(STATS, torch.float32), 20))}


def g_tiled_assemble(H):
    out = {}
    for S, tile, stride in GEOMETRIES:
        u, f, th = _level_fields(2, S, 2 * S, 400 + S)
        out[f"x{S}"] = _bits(H.tiled_assemble(u, f, th, _dev(STATS[:2], torch.float32), tile, stride))
    return out


def g_denorm(H):
    rng = np.random.default_rng(500)
    y = _dev(rng.normal(0, 1, (3 * 4, 1, 40, 40)), torch.float32)
    out = {"stitch": _bits(H.cascade_stitch_denorm(y, _dev(STATS, torch.float32), 3, 40, 20))}
    for S, tile, stride in GEOMETRIES:
        m = H.tiled_tiles_per_side(S, tile, stride)
        y = _dev(rng.normal(0, 1, (2 * m * m, 1, 2 * tile, 2 * tile)), torch.float32)
        for window in ("linear", "flat"):
            out[f"blend{S}_{window}"] = _bits(H.tiled_blend_denorm(y, _dev(STATS[:2], torch.float32), 2, S, tile, stride,
                                                                 window))
    return out


def g_metrics(H):
    rng = np.random.default_rng(600)
    E, n = 2, 47
    gt = rng.normal(2e-4, 1e-4, (E, n, n))
    pred = gt + rng.normal(0, 3e-6, gt.shape)
    f, th = rng.uniform(-0.9, 1.1, (E, n, n)), rng.uniform(0.5, 2.0, (E, n, n))
    out = {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        out[f"field_{name}"] = _bits(H.field_metrics(_dev(pred, dtype), _dev(gt)))
        for interior in (0, 1):
            out[f"residual_{name}_{interior}"] = _bits(H.pde_residual_metrics(_dev(pred, dtype), _dev(f), _dev(th),
                                                                            float((n - 1) ** 2), bool(interior)))
    return out


def g_physics(H):
    rng = np.random.default_rng(700)
    B, n = 3, 20
    t = rng.normal(0, 1, (B, 1, n, n))
    y = t + 0.05 * rng.normal(0, 1, t.shape)
    x = rng.normal(0, 1, (B, 3, n, n))
    kind = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    loss, unit = H.physics_loss_fwd(_dev(y, torch.float32), _dev(t, torch.float32), _dev(x, torch.float32), kind,
                                    _dev(STATS[0], torch.float32), 0.01, (float((n - 1) ** 2), float((2 * n - 1) ** 2)))
    dy = H.physics_loss_bwd(unit, _dev(np.array(0.75), torch.float32))
    return {"loss": _bits(loss), "unit": _bits(unit), "dy": _bits(dy)}


def g_solve_div(H):
    from superresolution_for_pdes_amd import poisson as P
    rng = np.random.default_rng(800)
    B, n = 2, 70
    f, th = rng.normal(0, 1, (B, n, n)), rng.uniform(0.5, 2.0, (B, n, n))
    out = {}
    for mean in ("arithmetic", "harmonic"):
        x, iters, resid = P.solve_div(_dev(f), _dev(th), face_mean=mean, maxit=6, check_every=0, check=False,
                                      return_info=True)
        assert iters.tolist() == [6, 6]
        out[f"x_{mean}"], out[f"iters_{mean}"], out[f"resid_{mean}"] = _bits(x), _bits(iters), _bits(resid)
    return out


GROUPS = {g.__name__[2:]: g for g in (g_cascade_stats, g_tiled_stats, g_cascade_assemble, g_tiled_assemble, g_denorm,
                                      g_metrics, g_physics, g_solve_div)}


def compute(group):
    from superresolution_for_pdes_amd import hipops as H
    return {f"{group}.{k}": v for k, v in GROUPS[group](H).items()}


@pytest.fixture(scope="module")
def recorded():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "field_bits*.npz"))):
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    return out


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_bits_equal_the_recorded_ones(recorded, group):
    got = compute(group)
    assert sorted(got) == sorted(k for k in recorded if k.startswith(group + "."))
    for k, v in got.items():
        want = recorded[k]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        print(f"{k}: {int((v != want).sum())} of {v.size} values differ")
        assert np.array_equal(v, want), k


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    arrays = {}
    for name in GROUPS:
        arrays.update(compute(name))
    # two files: the assemble outputs (incompressible fp32 mantissas) alone come near the size limit of a committed file
    for dest, keep in (("field_bits.npz", lambda k: "assemble" not in k), ("field_bits_assemble.npz", lambda k: "assemble" in k)):
        dest = os.path.join(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, dest)
        np.savez_compressed(dest, **{k: v for k, v in arrays.items() if keep(k)})
        print(f"{dest}: {os.path.getsize(dest)} bytes")
