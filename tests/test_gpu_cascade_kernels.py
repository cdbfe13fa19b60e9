"""The batched cascade kernels (csrc/cascade.hip, ABI 12) against the per-example torch path they replace
(resolution_comparison.GlobalNormalization / _level_inputs / _tiles_to_blocks) and numpy.

Shapes are the smallest at which tile indexing (4 and 16 tiles per example), example indexing (E = 2, 3, 5) and the
reductions' paths (20^2 = 400 elements: less than one workgroup pass; 40^2: one workgroup; 160^2: 13 workgroups, the
last pass partly filled) can go wrong.  Example 1 of every set has a constant theta, example 0 (E >= 3: example 2)
a theta whose std (1.014e-6) is just above the 1e-6 threshold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 20


def _fields(E, n, seed):
    """u ~ N(2e-4, 1e-4) (a solution's scale), f in [-0.9, 1.1], theta ~ U(0.5, 2); example 1: theta = 1.3 everywhere;
    the last example (E >= 3) or example 0 (E = 2): half the thetas 1, half 1 + 17 * 2^-23 (std 1.014e-6 in fp32)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(2e-4, 1e-4, (E, n, n))
    x = np.linspace(0, 1, n)
    X, Y = np.meshgrid(x, x)
    f = np.stack([np.sin(2 * np.pi * (8.3 + e) * X) * np.sin(2 * np.pi * (11.1 - e) * Y) + 0.1 for e in range(E)])
    th = rng.uniform(0.5, 2.0, (E, n, n))
    th[1] = 1.3
    near = np.where(rng.permutation(n * n) < n * n // 2, 1.0, 1.0 + 17 * 2.0 ** -23).reshape(n, n)
    th[E - 1 if E >= 3 else 0] = near
    return u, f, th


def _np_stats(x):
    """mean, unbiased std in fp64 of the fp32-cast values."""
    x32 = x.astype(np.float32).astype(np.float64)
    return x32.mean(), x32.std(ddof=1)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


@pytest.mark.parametrize("E,n", [(3, 40), (2, 160), (5, 20)])
def test_level_stats(E, n):
    """Mean and unbiased std of the fp32-cast values within 1e-6 relative of numpy's fp64 statistics (the kernel
    accumulates in fp64 and rounds once: 6e-8), the theta-constant flags exact, the flagged rows (0, 1), and equal
    bits from two calls.

    torch's own CPU .float().mean() / .std() of these inputs are checked against the same numpy values here: they
    stay inside 1e-6 (measured <= 1.9e-7) on every field but one, the nearly constant theta, whose fp32 std torch
    gives 1.73e-3 off (its fp32-rounded running mean sits up to 6e-8 from the true one, (6e-8 / 1e-6)^2 / 2 of the
    variance).  The issue's rule would widen the kernel's bound there to twice that; the kernel does not need it,
    so it keeps 1e-6 on every field, and for that field torch is only required to reach the same flag."""
    from superresolution_for_pdes_amd import hipops as H
    u, f, th = _fields(E, n, 10 + n)
    du, df, dth = _dev(u), _dev(f), _dev(th)
    stats, flags = H.cascade_level_stats(du, df, dth)
    stats2, flags2 = H.cascade_level_stats(du, df, dth)
    assert stats.shape == (E, 6) and stats.dtype == torch.float32 and flags.dtype == torch.int32
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32)) and torch.equal(flags, flags2)
    s, fl = stats.cpu().numpy().astype(np.float64), flags.cpu().numpy()
    bound = 1e-6
    for e in range(E):
        want_flag = 0
        for k, x in enumerate((u[e], f[e], th[e])):
            mean, std = _np_stats(x)
            t = torch.from_numpy(x).float()
            tm, ts = float(t.mean()), float(t.std())
            assert abs(tm - mean) <= bound * abs(mean), ("torch mean", e, k, tm, mean)
            if k == 2 and np.float32(std) < np.float32(1e-6):
                want_flag = 1
                assert fl[e] == 1 and s[e, 4] == 0.0 and s[e, 5] == 1.0, (e, s[e])
                continue
            if not (k == 2 and std < 1e-5):
                assert abs(ts - std) <= bound * std, ("torch std", e, k, ts, std)
            else:   # the nearly constant theta (docstring): the same decision, 3.5e-3 = twice its measured deviation
                assert not ts < 1e-6 and abs(ts - std) <= 3.5e-3 * std, ("torch std", e, k, ts, std)
            print(f"E={E} n={n} e={e} field={k}: mean rel {abs(s[e, 2 * k] - mean) / abs(mean):.2e} "
                  f"std rel {abs(s[e, 2 * k + 1] - std) / std:.2e}")
            assert abs(s[e, 2 * k] - mean) <= bound * abs(mean), (e, k, s[e, 2 * k], mean)
            assert abs(s[e, 2 * k + 1] - std) <= bound * std, (e, k, s[e, 2 * k + 1], std)
        assert fl[e] == want_flag, (e, fl[e])
    near = E - 1 if E >= 3 else 0
    assert fl[1] == 1 and fl[near] == 0 and 1.0e-6 < s[near, 5] < 1.03e-6, s[near]   # just above the threshold


def _norm_from_row(u_next, f_next, th_next, row, flag):
    """A GlobalNormalization of one example whose six values are the kernel's statistics row (0-dim device
    tensors, as its own)."""
    from superresolution_for_pdes_amd.resolution_comparison import GlobalNormalization
    norm = GlobalNormalization(u_next, None, f_next, th_next, device="cuda", theta_is_constant=bool(flag))
    norm.u_mean, norm.u_std, norm.f_mean, norm.f_std, norm.theta_mean, norm.theta_std = (row[i] for i in range(6))
    return norm


def _level(E, S, seed):
    from superresolution_for_pdes_amd import hipops as H
    u_next, f_next, th_next = (_dev(a) for a in _fields(E, 2 * S, seed))
    u_cur = _dev(np.random.default_rng(seed + 1).normal(2e-4, 1e-4, (E, S, S)))
    stats, flags = H.cascade_level_stats(u_next, f_next, th_next)
    return u_cur, u_next, f_next, th_next, stats, flags.cpu().numpy()


@pytest.mark.parametrize("S", [40, 80])
def test_level_assemble_equals_per_example_torch_path(S):
    """x == cat_e _level_inputs(u[e], f[e], theta[e], norm_e), bit for bit (E = 3; 4 and 16 tiles per example; example
    1's theta is constant and passes through the (0, 1) row unchanged)."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.resolution_comparison import _level_inputs
    E = 3
    u_cur, u_next, f_next, th_next, stats, flags = _level(E, S, 100 + S)
    assert list(flags) == [0, 1, 0]
    x = H.cascade_level_assemble(u_cur, f_next, th_next, stats, TILE)
    want = torch.cat([_level_inputs(u_cur[e], f_next[e], th_next[e],
                                    _norm_from_row(u_next[e], f_next[e], th_next[e], stats[e], flags[e]), TILE)
                      for e in range(E)])
    assert x.shape == want.shape == (E * (S // TILE) ** 2, 3, 2 * TILE, 2 * TILE) and x.dtype == torch.float32
    for c in range(3):
        assert torch.equal(x[:, c].contiguous().view(torch.int32), want[:, c].contiguous().view(torch.int32)), c


@pytest.mark.parametrize("S", [40, 80])
def test_stitch_denorm_equals_torch_expression(S):
    """u_next[e] == _tiles_to_blocks((y_e * std_e + mean_e)[:, 0].double(), 1), bit for bit."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.resolution_comparison import _tiles_to_blocks
    E, m2 = 3, (S // TILE) ** 2
    _, _, _, _, stats, _ = _level(E, S, 200 + S)
    g = torch.Generator().manual_seed(S)
    y = torch.randn(E * m2, 1, 2 * TILE, 2 * TILE, generator=g).cuda()
    out = H.cascade_stitch_denorm(y, stats, E, S, TILE)
    assert out.shape == (E, 2 * S, 2 * S) and out.dtype == torch.float64
    for e in range(E):
        ye = y[e * m2:(e + 1) * m2]
        want = _tiles_to_blocks((ye * stats[e, 1] + stats[e, 0])[:, 0].double(), 1)[0]
        assert torch.equal(out[e], want), e


@pytest.mark.parametrize("S", [40, 80])
def test_assemble_identity_stitch_round_trip(S):
    """assemble -> an identity "model" (channel 0) -> stitch puts the bilinear resize of every normalised tile,
    denormalised, at that tile's place: the two tile orders are inverse to each other.  The expectation is built
    tile by tile with explicit slices, not with the tiling helpers."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.models import upsample_bilinear
    E = 3
    u_cur, _, f_next, th_next, stats, _ = _level(E, S, 300 + S)
    x = H.cascade_level_assemble(u_cur, f_next, th_next, stats, TILE)
    out = H.cascade_stitch_denorm(x[:, 0:1].contiguous(), stats, E, S, TILE)
    want = torch.empty_like(out)
    for e in range(E):
        mean, std = stats[e, 0], stats[e, 1]
        for ti in range(S // TILE):
            for tj in range(S // TILE):
                t = u_cur[e, ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE].float()
                up = upsample_bilinear(((t - mean) / std)[None, None].contiguous(), 2 * TILE, 2 * TILE)[0, 0]
                want[e, ti * 2 * TILE:(ti + 1) * 2 * TILE, tj * 2 * TILE:(tj + 1) * 2 * TILE] = (up * std + mean).double()
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_field_metrics(dtype):
    """MAE and RMSE within 1e-12 relative of numpy's fp64 values, the maximum exact (E = 3 at 160^2: 13 workgroups
    per example)."""
    from superresolution_for_pdes_amd import hipops as H
    rng = np.random.default_rng(5)
    gt = rng.normal(2e-4, 1e-4, (3, 160, 160))
    pred = (gt + rng.normal(0, 3e-6, gt.shape)).astype(np.float32 if dtype == torch.float32 else np.float64)
    pred[2, 17, 150] += 1e-3     # one outlier decides example 2's maximum
    out = H.field_metrics(_dev(pred, dtype), _dev(gt))
    out2 = H.field_metrics(_dev(pred, dtype), _dev(gt))
    assert out.shape == (3, 3) and out.dtype == torch.float64 and torch.equal(out, out2)
    got = out.cpu().numpy()
    for e in range(3):
        d = pred[e].astype(np.float64) - gt[e]
        mae, rmse, mx = np.mean(np.abs(d)), np.sqrt(np.mean(d * d)), np.max(np.abs(d))
        assert abs(got[e, 0] - mae) <= 1e-12 * mae and abs(got[e, 1] - rmse) <= 1e-12 * rmse, (e, got[e], mae, rmse)
        assert got[e, 2] == mx, (e, got[e, 2], mx)


def test_argument_errors_launch_nothing():
    """A null pointer, an S that is no multiple of the tile and E = 0 each return a negative code with a message,
    before any launch: the output buffers keep their sentinel."""
    from superresolution_for_pdes_amd import _lib
    cd, sp = _lib.lib(), _lib.stream_ptr()
    E, S = 2, 40
    u = torch.zeros(E, 2 * S, 2 * S, dtype=torch.float64, device="cuda")
    uc = torch.zeros(E, S, S, dtype=torch.float64, device="cuda")
    stats = torch.full((E, 6), 7.0, device="cuda")
    flags = torch.full((E,), 7, dtype=torch.int32, device="cuda")
    x = torch.full((E * 4, 3, 40, 40), 7.0, device="cuda")
    y = torch.zeros(E * 4, 1, 40, 40, device="cuda")
    un = torch.full((E, 2 * S, 2 * S), 7.0, dtype=torch.float64, device="cuda")
    mt = torch.full((E, 3), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    wsb = ws.numel() * 8
    cases = [
        ("srpde_cascade_level_stats", (0, p(u), p(u), E, 2 * S, p(stats), p(flags), p(ws), wsb, sp), "null"),
        ("srpde_cascade_level_stats", (p(u), p(u), p(u), 0, 2 * S, p(stats), p(flags), p(ws), wsb, sp), "shape"),
        ("srpde_cascade_level_stats", (p(u), p(u), p(u), E, 2 * S, p(stats), p(flags), p(ws), 8, sp), "workspace"),
        ("srpde_cascade_level_assemble", (p(uc), 0, p(u), p(stats), E, S, TILE, p(x), sp), "null"),
        ("srpde_cascade_level_assemble", (p(uc), p(u), p(u), p(stats), E, 50, TILE, p(x), sp), "multiple of tile"),
        ("srpde_cascade_level_assemble", (p(uc), p(u), p(u), p(stats), 0, S, TILE, p(x), sp), "shape"),
        ("srpde_cascade_stitch_denorm", (p(y), p(stats), E, S, TILE, 0, sp), "null"),
        ("srpde_cascade_stitch_denorm", (p(y), p(stats), E, 50, TILE, p(un), sp), "multiple of tile"),
        ("srpde_cascade_stitch_denorm", (p(y), p(stats), 0, S, TILE, p(un), sp), "shape"),
        ("srpde_field_metrics", (p(u), 0, 0, E, 2 * S, p(mt), p(ws), wsb, sp), "null"),
        ("srpde_field_metrics", (p(u), 0, p(u), 0, 2 * S, p(mt), p(ws), wsb, sp), "shape"),
    ]
    for name, args, word in cases:
        rc = getattr(cd, name)(*args)
        assert rc < 0 and name in _lib.last_error() and word in _lib.last_error(), (name, rc, _lib.last_error())
    torch.cuda.synchronize()
    for t in (stats, flags, x, un, mt):
        assert bool((t == 7).all())
    with pytest.raises(RuntimeError, match="srpde_cascade_level_assemble"):
        _lib.call("srpde_cascade_level_assemble", p(uc), p(u), p(u), p(stats), E, 50, TILE, p(x), sp)
