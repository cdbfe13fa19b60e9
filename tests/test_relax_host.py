"""CPU: the weighted-Jacobi smoother (csrc/relax.hip, ABI 17; poisson.relax, tiled_inference's ``polish``).

``relax_np`` restates srpde_pde_relax with one numpy pass per sweep, in the header's order of operations; the GPU tests
compare the kernel with it by equality of bits.  Here it is established as a reference on its own: the sine modes of
the grid are its eigenvectors with the eigenvalues the theory gives, and the reference solver's solutions
(tests/golden/poisson_fixture.npz) are its fixed points.  Then the host side of the library: the two queries, every
argument check of srpde_pde_relax (no GPU is touched: each fails before a launch) and the keyword checks of the
cascade."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relax_np(u, f, theta, inv_h2, sweeps, omega=0.8, interior_only=False):
    """srpde_pde_relax restated: fields [E, n, n] fp64, every operation one rounded numpy pass, Jacobi (each sweep
    reads the previous one's u throughout)."""
    u = np.array(u, dtype=np.float64)
    f, theta = np.asarray(f, np.float64), np.asarray(theta, np.float64)
    g = f / (theta * np.float64(inv_h2))
    c = 0.25 * np.float64(omega)
    for _ in range(sweeps):
        p = np.pad(u, ((0, 0), (1, 1), (1, 1)))                       # a neighbour outside the grid is 0
        s = (p[:, :-2, 1:-1] + p[:, 2:, 1:-1]) + (p[:, 1:-1, :-2] + p[:, 1:-1, 2:])
        r = (s - 4.0 * u) - g
        new = u + c * r
        if interior_only:                                             # the ring keeps its value in every sweep
            new[:, 0, :], new[:, -1, :], new[:, :, 0], new[:, :, -1] = u[:, 0, :], u[:, -1, :], u[:, :, 0], u[:, :, -1]
        u = new
    return u


def sine_mode(n, p, q):
    i = np.arange(1, n + 1)
    return np.outer(np.sin(p * np.pi * i / (n + 1)), np.sin(q * np.pi * i / (n + 1)))


def mode_factor(n, p, q, omega):
    """the eigenvalue of one sweep's error operator I + (omega / 4) A on sine mode (p, q)"""
    return 1.0 - omega * (np.sin(p * np.pi / (2 * (n + 1))) ** 2 + np.sin(q * np.pi / (2 * (n + 1))) ** 2)


@pytest.fixture(scope="module")
def lib():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import _lib
    return _lib


@pytest.mark.parametrize("omega", [0.8, 1.0])
@pytest.mark.parametrize("n", [7, 33])
def test_sine_modes_are_eigenvectors(n, omega):
    """theta = 1, f = 0: eight sweeps multiply mode (p, q) by lambda^8, for the smoothest mode, the roughest one and a
    mixed one.  |lambda| <= 1 and the mode is at most 1, so 1e-14 is an absolute bound some 50 roundings wide."""
    one, zero = np.ones((1, n, n)), np.zeros((1, n, n))
    for p, q in ((1, 1), (n, n), (n // 2 + 1, 2)):
        v = sine_mode(n, p, q)
        lam = mode_factor(n, p, q, omega)
        assert abs(lam) <= 1.0
        got = relax_np(v[None], zero, one, (n - 1) ** 2, 8, omega)[0]
        err = np.abs(got - lam ** 8 * v).max()
        print(f"n={n} omega={omega} mode=({p},{q}) lambda={lam:.6f} err={err:.2e}")
        assert err <= 1e-14


def test_high_frequencies_shrink_by_0p6_at_omega_0p8():
    """omega = 0.8: every mode with a wavenumber of at least pi / 2 in one direction has |lambda| <= 0.6."""
    n = 33
    k = np.arange(1, n + 1)
    s2 = np.sin(k * np.pi / (2 * (n + 1))) ** 2
    lam = 1.0 - 0.8 * (s2[:, None] + s2[None, :])
    rough = (k[:, None] >= (n + 1) / 2) | (k[None, :] >= (n + 1) / 2)
    assert np.abs(lam[rough]).max() <= 0.6 + 1e-12 and np.abs(lam).max() < 1.0


@pytest.mark.parametrize("n", [20, 40, 80, 160])
def test_reference_solutions_are_fixed_points(n):
    """The reference's spsolve solution with variable theta moves by at most 1e-14 max|u| in eight sweeps."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "poisson_fixture.npz"))
    u, f, th = z[f"uv_{n}"][None], z[f"f{n}"][None], z[f"thv{n}"][None]
    moved = np.abs(relax_np(u, f, th, (n - 1) ** 2, 8) - u).max() / np.abs(u).max()
    print(f"n={n} moved {moved:.2e} of max|u|")
    assert moved <= 1e-14


def test_interior_only_holds_the_ring_and_noise_is_damped():
    z = np.load(os.path.join(ROOT, "tests", "golden", "poisson_fixture.npz"))
    n = 40
    u, f, th = z[f"uv_{n}"][None], z[f"f{n}"][None], z[f"thv{n}"][None]
    rng = np.random.default_rng(0)
    noisy = u + rng.normal(0, 1e-5, u.shape)
    out = relax_np(noisy, f, th, (n - 1) ** 2, 8)
    # every eigenvalue of the symmetric error operator lies inside (-1, 1): the error's 2-norm strictly falls
    print("rmse", np.sqrt(np.mean((noisy - u) ** 2)), "->", np.sqrt(np.mean((out - u) ** 2)))
    assert np.sqrt(np.mean((out - u) ** 2)) < np.sqrt(np.mean((noisy - u) ** 2))
    held = relax_np(noisy, f, th, (n - 1) ** 2, 3, interior_only=True)
    ring = np.ones((n, n), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(held[0][ring], noisy[0][ring]) and not np.array_equal(held[0][~ring], noisy[0][~ring])


def test_queries(lib):
    q = lib.query
    K = q("srpde_pde_relax_sweeps_per_launch")
    assert K >= 2
    from superresolution_for_pdes_amd import hipops as H
    assert H.pde_relax_sweeps_per_launch() == K and H.RELAX_TILE >= 1
    for sweeps in (0, 1, K):
        assert q("srpde_pde_relax_workspace_size", 3, 100, sweeps) == 0
    for sweeps in (K + 1, 2 * K, 5 * K + 1):
        assert q("srpde_pde_relax_workspace_size", 3, 100, sweeps) >= 3 * 100 * 100 * 8
    assert q("srpde_pde_relax_workspace_size", 10, 16384, K + 1) >= 10 * 16384 * 16384 * 8   # beyond 2^32 bytes
    assert q("srpde_pde_relax_workspace_size", 0, 100, K + 1) == 0
    assert q("srpde_pde_relax_workspace_size", -1, 100, K + 1) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    """Every argument error of srpde_pde_relax: a negative code and a message that names the entry.  The pointers
    are made-up (never dereferenced on the host); that this runs on a machine without a GPU is the proof that nothing
    was launched."""
    cd = lib.lib()
    K = lib.query("srpde_pde_relax_sweeps_per_launch")
    E, n = 2, 40
    B = E * n * n * 8                       # bytes of one field
    U, F, TH, O, W = (1 << 20) + 0 * B, (1 << 20) + 1 * B, (1 << 20) + 2 * B, (1 << 20) + 3 * B, (1 << 20) + 4 * B
    ih2 = float((n - 1) ** 2)

    def args(u=U, f=F, th=TH, o=O, E=E, n=n, ih2=ih2, sweeps=K + 1, omega=0.8, interior=0, ws=W, ws_bytes=B):
        return (u, f, th, o, E, n, ih2, sweeps, omega, interior, ws, ws_bytes, 0)

    cases = [
        (args(u=0), "null"), (args(f=0), "null"), (args(th=0), "null"), (args(o=0), "null"),
        (args(E=0), "shape"), (args(E=-3), "shape"),
        (args(n=0), "shape"), (args(n=2, interior=1), "shape"), (args(n=1, interior=1), "shape"),
        (args(n=16385, E=1), "shape"),
        (args(sweeps=-1), "sweeps"),
        (args(omega=0.0), "omega"), (args(omega=-0.5), "omega"), (args(omega=1.0000001), "omega"),
        (args(omega=float("nan")), "omega"),
        (args(ih2=0.0), "inv_h2"), (args(ih2=-1.0), "inv_h2"), (args(ih2=float("inf")), "inv_h2"),
        (args(ih2=float("nan")), "inv_h2"),
        (args(u=U + 4), "aligned"), (args(f=F + 4), "aligned"), (args(th=TH + 4), "aligned"), (args(o=O + 4), "aligned"),
        (args(ws=W + 4, ws_bytes=B + 8), "aligned"),
        (args(o=U), "overlaps"), (args(o=U + B - 8), "overlaps"), (args(o=F), "overlaps"), (args(o=TH - 8), "overlaps"),
        (args(ws=O), "overlaps"), (args(ws=O + B - 8, ws_bytes=2 * B), "overlaps"),
        (args(ws_bytes=B - 8), "workspace too small"), (args(ws=0, ws_bytes=0), "workspace too small"),
    ]
    for a, word in cases:
        rc = cd.srpde_pde_relax(*a)
        assert rc < 0 and "srpde_pde_relax" in lib.last_error() and word in lib.last_error(), (a, rc, lib.last_error())
    with pytest.raises(RuntimeError, match="srpde_pde_relax"):
        lib.call("srpde_pde_relax", *args(omega=2.0))


def test_polish_keywords_are_checked_before_the_model_is_touched():
    """model=None: anything past the keyword check would raise AttributeError."""
    from superresolution_for_pdes_amd.tiled_inference import upscale_cascade, upscale_level
    z = np.zeros((1, 20, 20))
    for kw in ({"polish": -1}, {"polish": 1.5}, {"polish": 2, "polish_omega": 0.0}, {"polish": 2, "polish_omega": 1.01},
               {"polish_omega": -0.8}):
        with pytest.raises(ValueError, match="upscale_level: polish"):
            upscale_level(None, z, np.zeros((1, 40, 40)), np.ones((1, 40, 40)), **kw)
        with pytest.raises(ValueError, match="upscale_cascade: polish"):
            upscale_cascade(None, z, {}, {}, 40, **kw)
    with pytest.raises(AttributeError):      # valid keywords reach the model
        upscale_level(None, z, np.zeros((1, 40, 40)), np.ones((1, 40, 40)), polish=3, polish_omega=1.0)


def test_poisson_relax_checks_its_arguments_before_the_device():
    from superresolution_for_pdes_amd import poisson as P
    z = np.zeros((4, 4))
    with pytest.raises(ValueError, match="relax: sweeps"):
        P.relax(z, z, z + 1, -1)
    for omega in (0.0, 1.5):
        with pytest.raises(ValueError, match="relax: omega"):
            P.relax(z, z, z + 1, 2, omega=omega)
