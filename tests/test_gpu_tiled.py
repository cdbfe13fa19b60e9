"""The overlapping-tile cascade level on the GPU (csrc/tiled.hip, ABI 16; tiled_inference) against the kernels of the
disjoint-tile cascade it extends and the numpy restatement of the blend in test_tiled_host.py.  Everything is compared
by equality of bits.

E = 2 throughout.  Geometries (S, tile, stride): (47, 20, 10) a clamped last window and up to 3 x 3 windows over a
pixel; (30, 20, 10) two windows; (21, 20, 7) a clamped window one point from its neighbour; (40, 20, 20) disjoint
tiles, where the path must reduce to the existing one."""
import numpy as np
import pytest
import torch

from test_tiled_host import blend_denorm_np, crops, starts

pytestmark = pytest.mark.gpu

E = 2
GEOMETRIES = [(47, 20, 10), (30, 20, 10), (21, 20, 7), (40, 20, 20)]
WINDOWS = ["linear", "flat"]


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _fields(S, seed, const_theta=False):
    """u_cur [E, S, S] ~ N(2e-4, 1e-4) (a solution's scale), f_next in [-0.9, 1.1] and theta_next ~ U(0.5, 2) on
    [E, 2S, 2S]; ``const_theta``: example 1's theta is 1.3 everywhere."""
    rng = np.random.default_rng(seed)
    u = rng.normal(2e-4, 1e-4, (E, S, S))
    x = np.linspace(0, 1, 2 * S)
    X, Y = np.meshgrid(x, x)
    f = np.stack([np.sin(2 * np.pi * (3.3 + e) * X) * np.sin(2 * np.pi * (2.1 - e) * Y) + 0.1 for e in range(E)])
    th = rng.uniform(0.5, 2.0, (E, 2 * S, 2 * S))
    if const_theta:
        th[1] = 1.3
    return _dev(u), _dev(f), _dev(th)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_assemble_equals_cascade_assemble_on_every_window(geom):
    """Tile (e, i, j) == srpde_cascade_level_assemble of the fields cropped to window (i, j) with the same stats, bit
    for bit: the existing kernel is the reference."""
    from superresolution_for_pdes_amd import hipops as H
    S, tile, stride = geom
    u, f, th = _fields(S, 10 + S, const_theta=True)
    stats, flags = H.tiled_level_stats(u, f, th)
    assert flags.tolist() == [0, 1]
    st = starts(S, tile, stride)
    m = len(st)
    assert H.tiled_tiles_per_side(S, tile, stride) == m
    x = H.tiled_assemble(u, f, th, stats, tile, stride)
    assert x.shape == (E * m * m, 3, 2 * tile, 2 * tile) and x.dtype == torch.float32
    x = x.view(E, m, m, 3, 2 * tile, 2 * tile)
    for i, si in enumerate(st):
        for j, sj in enumerate(st):
            want = H.cascade_level_assemble(u[:, si:si + tile, sj:sj + tile].contiguous(),
                                            f[:, 2 * si:2 * si + 2 * tile, 2 * sj:2 * sj + 2 * tile].contiguous(),
                                            th[:, 2 * si:2 * si + 2 * tile, 2 * sj:2 * sj + 2 * tile].contiguous(),
                                            stats, tile)
            assert torch.equal(_bits(x[:, i, j]), _bits(want)), (i, j)


@pytest.mark.parametrize("S", [20, 47])
def test_stats_equal_cascade_stats_of_each_field(S):
    """The u columns are srpde_cascade_level_stats' of u_cur, the f / theta columns and the flag its of the fine
    fields, bit for bit (S = 20: one workgroup per field; S = 47: 2 for u, 5 for f and theta, so three of the five
    workgroups of the u plane leave at once).  Example 1's theta is constant."""
    from superresolution_for_pdes_amd import hipops as H
    u, f, th = _fields(S, 20 + S, const_theta=True)
    stats, flags = H.tiled_level_stats(u, f, th)
    stats2, flags2 = H.tiled_level_stats(u, f, th)
    assert stats.shape == (E, 6) and stats.dtype == torch.float32 and flags.dtype == torch.int32
    assert torch.equal(_bits(stats), _bits(stats2)) and torch.equal(flags, flags2)
    su, _ = H.cascade_level_stats(u, u, u)
    sf, ff = H.cascade_level_stats(f, f, th)
    assert torch.equal(_bits(stats[:, 0:2]), _bits(su[:, 0:2]))
    assert torch.equal(_bits(stats[:, 2:6]), _bits(sf[:, 2:6]))
    assert torch.equal(flags, ff) and flags.tolist() == [0, 1]
    assert stats[1, 4:6].tolist() == [0.0, 1.0]
    u64 = u.cpu().numpy().astype(np.float32).astype(np.float64)   # and they are the statistics they claim to be
    for e in range(E):
        assert abs(float(stats[e, 0]) - u64[e].mean()) <= 1e-6 * abs(u64[e].mean())
        assert abs(float(stats[e, 1]) - u64[e].std(ddof=1)) <= 1e-6 * u64[e].std(ddof=1)


def _y_and_stats(S, tile, stride, seed):
    m = len(starts(S, tile, stride))
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1, (E * m * m, 1, 2 * tile, 2 * tile)).astype(np.float32)
    stats = np.array([[2e-4, 1e-4, 0.1, 0.5, 1.2, 0.4], [-3.1e-4, 2.3e-4, 0.1, 0.5, 0, 1]], np.float32)
    return y, stats


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_blend_equals_numpy_restatement(geom, window):
    """fp64 sums in tile order, one rounding to fp32, a float32 multiply and add: equal, not close (every w * y is
    exact in fp64, so a fused multiply-add cannot change a sum).  Two calls give the same bits."""
    from superresolution_for_pdes_amd import hipops as H
    S, tile, stride = geom
    y, stats = _y_and_stats(S, tile, stride, 30 + S)
    out = H.tiled_blend_denorm(_dev(y, torch.float32), _dev(stats, torch.float32), E, S, tile, stride, window)
    out2 = H.tiled_blend_denorm(_dev(y, torch.float32), _dev(stats, torch.float32), E, S, tile, stride, window)
    assert out.shape == (E, 2 * S, 2 * S) and out.dtype == torch.float64 and torch.equal(_bits(out), _bits(out2))
    want = blend_denorm_np(y, stats, E, S, tile, stride, window)
    got = out.cpu().numpy()
    print(f"{geom} {window}: max |got - want| = {np.abs(got - want).max():.3e}")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("window", WINDOWS)
def test_blend_with_disjoint_tiles_is_stitch_denorm(window):
    from superresolution_for_pdes_amd import hipops as H
    S, tile = 40, 20
    y, stats = _y_and_stats(S, tile, tile, 40)
    dy, ds = _dev(y, torch.float32), _dev(stats, torch.float32)
    out = H.tiled_blend_denorm(dy, ds, E, S, tile, tile, window)
    assert torch.equal(_bits(out), _bits(H.cascade_stitch_denorm(dy, ds, E, S, tile)))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_blend_of_crops_of_one_field_is_that_field(geom, window):
    """Partition of unity on the device: windows cropped from a global field, stats (0, 1) -> the field exactly."""
    from superresolution_for_pdes_amd import hipops as H
    S, tile, stride = geom
    G = np.random.default_rng(50 + S).normal(0, 1, (E, 2 * S, 2 * S)).astype(np.float32)
    ident = np.tile(np.array([0, 1, 0, 1, 0, 1], np.float32), (E, 1))
    out = H.tiled_blend_denorm(_dev(crops(G, S, tile, stride), torch.float32), _dev(ident, torch.float32), E, S, tile,
                               stride, window)
    assert np.array_equal(out.cpu().numpy(), G.astype(np.float64))


def test_wrapper_argument_checks():
    from superresolution_for_pdes_amd import hipops as H
    u, f, th = _fields(30, 60)
    stats, _ = H.tiled_level_stats(u, f, th)
    with pytest.raises(ValueError, match="tiled_tiles_per_side"):
        H.tiled_assemble(u, f, th, stats, 20, 0)
    with pytest.raises(ValueError, match="tiled_assemble"):
        H.tiled_assemble(u, f[:, :40, :40].contiguous(), th, stats, 20, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.tiled_level_stats(u.cpu(), f, th)
    with pytest.raises(ValueError, match="window"):
        H.tiled_blend_denorm(torch.zeros(E * 4, 1, 40, 40, device="cuda"), stats, E, 30, 20, 10, "hann")
    with pytest.raises(ValueError, match="E m\\^2"):
        H.tiled_blend_denorm(torch.zeros(E * 4, 1, 40, 40, device="cuda"), stats, E, 47, 20, 10)


@pytest.fixture(scope="module")
def model_and_data():
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.resolution_comparison_statistical import solve_multi_resolution
    torch.manual_seed(7)
    model = UNet().to("cuda")
    model.apply(init_weights)
    model.eval()
    np.random.seed(7)
    data = solve_multi_resolution(n_examples=E, resolutions=(80,), solver="dst")
    return model, data


def test_cascade_with_disjoint_tiles_and_truth_stats_is_the_batched_cascade(model_and_data):
    """stride = tile, stats = "truth": bit for bit ml_multi_level_upscale_batched, for both windows (one window per
    pixel: its value comes back unchanged)."""
    from superresolution_for_pdes_amd.resolution_comparison_statistical import ml_multi_level_upscale_batched
    from superresolution_for_pdes_amd.tiled_inference import upscale_cascade
    model, data = model_and_data
    want = ml_multi_level_upscale_batched(model, data, 80, 40)
    for window in WINDOWS:
        got = upscale_cascade(model, data["u"][40], data["f"], data["theta"], 80, stride=20, stats="truth",
                              window=window, u_truth=data["u"])
        assert got.shape == want.shape == (E, 80, 80) and got.dtype == torch.float64
        assert torch.equal(_bits(got), _bits(want)), window
    with pytest.raises(ValueError, match="u_truth"):
        upscale_cascade(model, data["u"][40], data["f"], data["theta"], 80, stats="truth")


@pytest.mark.parametrize("S", [40, 50])
def test_cascade_without_ground_truth(model_and_data, S):
    """stride 10, stats = "input": 40 -> 80, and 50 -> 100 (no multiple of the tile; crops of the same fields) run,
    give finite [E, 2S, 2S] fields, and two calls give the same bits.  Fixed statistics as a tensor run too."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.tiled_inference import upscale_cascade, upscale_level
    model, data = model_and_data
    if S == 40:
        u, f, th = data["u"][40], data["f"], data["theta"]
    else:   # a 50^2 coarse field and 100^2 fine ones: smooth stand-ins, the model only has to run on them
        u = torch.nn.functional.interpolate(data["u"][40][:, None], size=(50, 50), mode="bilinear")[:, 0].contiguous()
        f = {100: torch.nn.functional.interpolate(data["f"][80][:, None], size=(100, 100), mode="bilinear")[:, 0]}
        th = {100: torch.nn.functional.interpolate(data["theta"][80][:, None], size=(100, 100), mode="nearest")[:, 0]}
    a = upscale_cascade(model, u, f, th, 2 * S, stride=10, stats="input")
    b = upscale_cascade(model, u, f, th, 2 * S, stride=10, stats="input")
    assert a.shape == (E, 2 * S, 2 * S) and a.dtype == torch.float64 and bool(torch.isfinite(a).all())
    assert torch.equal(_bits(a), _bits(b))
    row, _ = H.tiled_level_stats(u.contiguous(), f[2 * S].contiguous(), th[2 * S].contiguous())
    c = upscale_level(model, u, f[2 * S], th[2 * S], stride=10, stats=row)
    assert torch.equal(_bits(c), _bits(a))
    d = upscale_level(model, u, f[2 * S], th[2 * S], stride=10, stats=row[0])     # [6]: one row for every example
    assert d.shape == a.shape and bool(torch.isfinite(d).all())
    g = upscale_level(model, u, f[2 * S], th[2 * S], stride=10, max_batch=7)      # E m^2 = 18 or 32 windows in chunks
    assert g.shape == a.shape and bool(torch.isfinite(g).all())
