"""CPU: the host side of the overlapping-tile cascade level (csrc/tiled.hip, ABI 16; tiled_inference.tile_starts):
the window geometry, the argument checks of every new entry (no GPU is touched: each fails before its launch), and
the partition of unity of the blend, shown on a numpy restatement of srpde_tiled_blend_denorm."""
import numpy as np
import pytest

GEOMETRIES = [((20, 20, 10), [0]), ((30, 20, 10), [0, 10]), ((47, 20, 10), [0, 10, 20, 27]), ((40, 20, 20), [0, 20]),
              ((21, 20, 7), [0, 1])]


@pytest.fixture(scope="module")
def lib():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import _lib
    return _lib


def starts(S, tile, stride):
    m = -(-(S - tile) // stride) + 1
    return [min(k * stride, S - tile) for k in range(m)]


def w1(n, window):
    """the 1-D weight over the n = 2 tile positions of a window"""
    i = np.arange(n)
    return np.minimum(i + 1, n - i).astype(np.float64) if window == "linear" else np.ones(n)


def blend_denorm_np(y, stats, E, S, tile, stride, window):
    """srpde_tiled_blend_denorm restated: fp64 sums of w * y over the covering windows in tile order, the integer
    weight sum, one rounding to fp32, then a float32 multiply and a float32 add, widened."""
    st, t2 = starts(S, tile, stride), 2 * tile
    m = len(st)
    y = np.asarray(y, np.float32).reshape(E, m, m, t2, t2)
    w = np.outer(w1(t2, window), w1(t2, window))
    num = np.zeros((E, 2 * S, 2 * S))
    den = np.zeros((2 * S, 2 * S), np.int64)
    for i, si in enumerate(st):
        for j, sj in enumerate(st):
            num[:, 2 * si:2 * si + t2, 2 * sj:2 * sj + t2] += w * y[:, i, j].astype(np.float64)
            den[2 * si:2 * si + t2, 2 * sj:2 * sj + t2] += w.astype(np.int64)
    assert den.min() >= 1
    v = (num / den.astype(np.float64)).astype(np.float32)
    stats = np.asarray(stats, np.float32)
    r = v * stats[:, 1].reshape(E, 1, 1)
    r = r + stats[:, 0].reshape(E, 1, 1)
    assert r.dtype == np.float32
    return r.astype(np.float64)


def crops(G, S, tile, stride):
    """every window's crop of the global fine fields G [E, 2S, 2S], in tile order: [E m^2, 1, 2 tile, 2 tile]"""
    st, t2 = starts(S, tile, stride), 2 * tile
    return np.stack([G[e, 2 * si:2 * si + t2, 2 * sj:2 * sj + t2] for e in range(G.shape[0]) for si in st
                     for sj in st])[:, None]


@pytest.mark.parametrize("geom,want", GEOMETRIES)
def test_tiles_per_side_and_tile_starts(lib, geom, want):
    from superresolution_for_pdes_amd.tiled_inference import tile_starts
    assert tile_starts(*geom) == want == starts(*geom)
    assert lib.query("srpde_tiled_tiles_per_side", *geom) == len(want)


def test_default_geometry_is_tile_20_stride_10():
    from superresolution_for_pdes_amd.tiled_inference import tile_starts
    assert tile_starts(50) == [0, 10, 20, 30]
    for bad in ((19, 20, 10), (40, 20, 0), (40, 20, 21)):
        with pytest.raises(ValueError, match="tile_starts"):
            tile_starts(*bad)


def test_bad_arguments_fail_before_any_launch(lib):
    """stride = 0, stride > tile, S < tile, a null pointer and an undersized workspace: each a negative code and a
    message that names the entry.  The pointers are made-up (aligned, never dereferenced on the host); that this runs
    on a machine without a GPU is the proof that nothing was launched."""
    cd = lib.lib()
    P, E, S, T = 4096, 2, 40, 20     # P: any non-null, 8-byte aligned value
    for geom in ((S, T, 0), (S, T, T + 1), (T - 1, T, 10), (16385, T, 10), (S, 0, 0)):
        rc = cd.srpde_tiled_tiles_per_side(*geom)
        assert rc < 0 and "srpde_tiled_tiles_per_side" in lib.last_error(), (geom, rc, lib.last_error())
    cases = [
        ("srpde_tiled_assemble", (P, P, P, P, E, S, T, 0, P, 0), "shape"),
        ("srpde_tiled_assemble", (P, P, P, P, E, S, T, T + 1, P, 0), "shape"),
        ("srpde_tiled_assemble", (P, P, P, P, E, T - 1, T, 10, P, 0), "shape"),
        ("srpde_tiled_assemble", (P, P, P, P, 0, S, T, 10, P, 0), "shape"),
        ("srpde_tiled_assemble", (P, P, P, P, 1 << 20, 16384, 4, 1, P, 0), "shape"),   # E m^2 beyond an int
        ("srpde_tiled_assemble", (P, 0, P, P, E, S, T, 10, P, 0), "null"),
        ("srpde_tiled_assemble", (P, P, P, P, E, S, T, 10, 0, 0), "null"),
        ("srpde_tiled_blend_denorm", (P, P, E, S, T, 0, 0, P, 0), "shape"),
        ("srpde_tiled_blend_denorm", (P, P, E, S, T, T + 1, 0, P, 0), "shape"),
        ("srpde_tiled_blend_denorm", (P, P, E, T - 1, T, 10, 0, P, 0), "shape"),
        ("srpde_tiled_blend_denorm", (P, P, E, S, T, 10, 2, P, 0), "window"),
        ("srpde_tiled_blend_denorm", (0, P, E, S, T, 10, 0, P, 0), "null"),
        ("srpde_tiled_blend_denorm", (P, P, E, S, T, 10, 0, 0, 0), "null"),
        ("srpde_tiled_level_stats", (0, P, P, E, S, P, P, P, 1 << 20, 0), "null"),
        ("srpde_tiled_level_stats", (P, P, P, E, S, P, P, 0, 1 << 20, 0), "null"),
        ("srpde_tiled_level_stats", (P, P, P, 0, S, P, P, P, 1 << 20, 0), "shape"),
        ("srpde_tiled_level_stats", (P, P, P, E, 0, P, P, P, 1 << 20, 0), "shape"),
        ("srpde_tiled_level_stats", (P, P, P, E, S, P, P, P + 4, 1 << 20, 0), "aligned"),
        ("srpde_tiled_level_stats", (P, P, P, E, S, P, P, P, 8, 0), "workspace too small"),
    ]
    for name, args, word in cases:
        rc = getattr(cd, name)(*args)
        assert rc < 0 and name in lib.last_error() and word in lib.last_error(), (name, args, rc, lib.last_error())
    with pytest.raises(RuntimeError, match="srpde_tiled_assemble"):
        lib.call("srpde_tiled_assemble", P, P, P, P, E, S, T, 0, P, 0)


def test_stats_workspace_size(lib):
    """E x 3 fields x red_blocks((2S)^2) partial pairs of doubles: the fine fields' partition holds the coarse one's."""
    q = lib.query
    assert q("srpde_tiled_level_stats_workspace_size", 2, 20) == 2 * 3 * 1 * 16          # 40^2 = 1600 -> 1 workgroup
    assert q("srpde_tiled_level_stats_workspace_size", 2, 47) == 2 * 3 * 5 * 16          # 94^2 = 8836 -> 5
    assert q("srpde_tiled_level_stats_workspace_size", 1, 320) == 3 * 200 * 16           # 640^2 -> 200
    assert q("srpde_tiled_level_stats_workspace_size", 1, 640) == 3 * 256 * 16           # capped at 256
    assert q("srpde_tiled_level_stats_workspace_size", 0, 20) == 0
    assert q("srpde_tiled_level_stats_workspace_size", 2, 47) == q("srpde_cascade_level_stats_workspace_size", 2, 94)


@pytest.mark.parametrize("window", ["linear", "flat"])
@pytest.mark.parametrize("geom", [g for g, _ in GEOMETRIES] + [(11, 4, 3), (9, 4, 1), (8, 4, 4)])
def test_blend_is_a_partition_of_unity(geom, window):
    """Windows that are crops of one global field blend back to that field exactly: every w * v is exact in fp64, the
    sum is (sum w) * v up to an fp64 rounding, and the one rounding to fp32 returns the fp32 value v."""
    S, tile, stride = geom
    E = 2
    G = np.random.default_rng(S * 100 + stride).normal(0, 1, (E, 2 * S, 2 * S)).astype(np.float32)
    y = crops(G, S, tile, stride)
    ident = np.tile(np.array([0, 1, 0, 1, 0, 1], np.float32), (E, 1))
    out = blend_denorm_np(y, ident, E, S, tile, stride, window)
    assert out.dtype == np.float64 and np.array_equal(out, G.astype(np.float64))
    stats = np.array([[2e-4, 1e-4, 0, 1, 0, 1], [-3.0, 0.5, 0, 1, 0, 1]], np.float32)
    want = ((G * stats[:, 1].reshape(E, 1, 1)) + stats[:, 0].reshape(E, 1, 1)).astype(np.float64)
    assert np.array_equal(blend_denorm_np(y, stats, E, S, tile, stride, window), want)


def test_linear_window_downweights_window_borders():
    """One window disagreeing by 1 moves a pixel by its weight share: at a border row of that window the linear
    weight is 1 against the neighbour's 20 where the flat mean gives one half."""
    S, tile, stride, E = 30, 20, 10, 1
    y = np.zeros((4, 1, 40, 40), np.float32)
    y[0] = 1.0                                         # the window at (0, 0) alone predicts 1
    ident = np.array([[0, 1, 0, 1, 0, 1]], np.float32)
    lin = blend_denorm_np(y, ident, E, S, tile, stride, "linear")
    flat = blend_denorm_np(y, ident, E, S, tile, stride, "flat")
    # fine pixel (39, 0): the last row of window (0, 0) (w1 = 1), row 19 of window (1, 0) (w1 = 20); column 0: 1 each
    assert lin[0, 39, 0] == np.float32(1 / 21) and flat[0, 39, 0] == 0.5
    assert lin[0, 0, 0] == 1.0 and lin[0, 59, 59] == 0.0
