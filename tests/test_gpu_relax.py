"""The weighted-Jacobi smoother on the GPU (relax_kernel<PointwiseOp> of csrc/relax.hip, ABI 17; hipops.pde_relax,
poisson.relax, the cascade's ``polish``) against relax_np, the one-pass-per-sweep numpy restatement established in
test_relax_host.py.  The kernel rounds every operation once in the header's order, so the comparison is by equality of
bits, whatever the tiling.

E = 3.  Sizes n: 1, 2, 3, 5 (grids smaller than the halo, the smallest with an interior), T - 1, T, T + 1 (one tile
with and without a ragged edge, the first two-tile grid) and 2T + K + 3 (three tiles per axis: a tile with neighbours
on every side).  Sweeps: 0 (a copy), 1, K - 1, K (one launch, short and full), K + 1 (two launches, through the
workspace, a short last one) and 2K + 1 (three launches: the other ping-pong parity)."""
import numpy as np
import pytest
import torch

from test_relax_host import mode_factor, relax_np, sine_mode

pytestmark = pytest.mark.gpu

E = 3


def _KT():
    """(sweeps per launch, from the library; output tile, hipops' constant)"""
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import hipops as H
    return H.pde_relax_sweeps_per_launch(), H.RELAX_TILE


def _sizes():
    K, T = _KT()
    return [1, 2, 3, 5, T - 1, T, T + 1, 2 * T + K + 3]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


def _fields(n, seed):
    """u ~ N(2e-4, 1e-4) (a solution's scale), f a sine product + 0.1, theta ~ U(0.5, 2): numpy [E, n, n]"""
    rng = np.random.default_rng(seed)
    u = rng.normal(2e-4, 1e-4, (E, n, n))
    x = np.linspace(0, 1, n)
    X, Y = np.meshgrid(x, x)
    f = np.stack([np.sin(2 * np.pi * (3.3 + e) * X) * np.sin(2 * np.pi * (2.1 - e) * Y) + 0.1 for e in range(E)])
    th = rng.uniform(0.5, 2.0, (E, n, n))
    return u, f, th


def _same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64))


@pytest.mark.parametrize("interior_only", [False, True])
@pytest.mark.parametrize("n", _sizes())
def test_bit_equal_to_the_numpy_restatement(n, interior_only):
    from superresolution_for_pdes_amd import hipops as H
    if interior_only and n < 3:
        with pytest.raises(RuntimeError, match="srpde_pde_relax"):     # refused, not computed
            H.pde_relax(*(_dev(a) for a in _fields(n, n)), 1.0, 1, 0.8, True)
        return
    K, _ = _KT()
    u, f, th = _fields(n, 100 + n)
    ud, fd, td = _dev(u), _dev(f), _dev(th)
    inv_h2 = float(max(n - 1, 1) ** 2)
    ring = np.ones((n, n), bool)
    ring[1:-1, 1:-1] = False
    for omega in (0.8, 1.0):
        for sweeps in (0, 1, K - 1, K, K + 1, 2 * K + 1):
            got = H.pde_relax(ud, fd, td, inv_h2, sweeps, omega, interior_only)
            want = relax_np(u, f, th, inv_h2, sweeps, omega, interior_only)
            assert got.shape == (E, n, n) and got.dtype == torch.float64
            assert _same_bits(got, want), (n, interior_only, omega, sweeps,
                                           float(np.abs(got.cpu().numpy() - want).max()))
            if interior_only:
                assert np.array_equal(got.cpu().numpy()[:, ring].view(np.int64), u[:, ring].view(np.int64))
            if sweeps == 0:
                assert _same_bits(got, u)
    assert _same_bits(ud, u) and _same_bits(fd, f) and _same_bits(td, th)       # the inputs are untouched


def test_sine_mode_decays_by_its_eigenvalue():
    """n = 33, theta = 1, f = 0, mode (17, 5), 2K + 1 sweeps: lambda^(2K + 1) times the mode, within 1e-13."""
    from superresolution_for_pdes_amd import poisson as P
    K, _ = _KT()
    n, omega = 33, 0.8
    v = sine_mode(n, 17, 5)
    lam = mode_factor(n, 17, 5, omega)
    got = P.relax(v, np.zeros((n, n)), np.ones((n, n)), 2 * K + 1, omega).cpu().numpy()
    err = np.abs(got[0] - lam ** (2 * K + 1) * v).max()
    print(f"lambda={lam:.6f} err={err:.2e}")
    assert got.shape == (1, n, n) and err <= 1e-13


def test_residual_falls_on_a_noisy_solution():
    """theta = 1, a sine f: 8 sweeps on solution + 1e-5 noise lower the residual RMS of every example (the residual
    is A e / h^2 and the sweep's error operator commutes with A and has every eigenvalue inside (-1, 1))."""
    from superresolution_for_pdes_amd import poisson as P
    n = 40
    _, f, _ = _fields(n, 5)
    f = _dev(f - 0.1)
    u = P.solve_batched(f, torch.ones_like(f), method="dst")
    g = torch.Generator(device="cpu").manual_seed(3)
    noisy = u + (1e-5 * torch.randn(E, n, n, generator=g, dtype=torch.float64)).to("cuda")
    before = P.residual_metrics(noisy, f, torch.ones(n, n, dtype=torch.float64))
    after = P.residual_metrics(P.relax(noisy, f, torch.ones(n, n, dtype=torch.float64), 8), f,
                               torch.ones(n, n, dtype=torch.float64))
    print("residual rms", before[:, 0].tolist(), "->", after[:, 0].tolist())
    assert bool((after[:, 0] < before[:, 0]).all())
    rm0 = (noisy - u).pow(2).mean().sqrt()
    rm1 = (P.relax(noisy, f, torch.ones_like(f), 8) - u).pow(2).mean().sqrt()
    assert float(rm1) < float(rm0)


@pytest.fixture(scope="module")
def model():
    from superresolution_for_pdes_amd.models import UNet, init_weights
    torch.manual_seed(11)
    m = UNet().to("cuda")
    m.apply(init_weights)
    return m.eval()


def _level_fields(S, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(2e-4, 1e-4, (2, S, S))
    x = np.linspace(0, 1, 2 * S)
    X, Y = np.meshgrid(x, x)
    f = np.stack([np.sin(2 * np.pi * (3.3 + e) * X) * np.sin(2 * np.pi * (2.1 - e) * Y) + 0.1 for e in range(2)])
    th = rng.uniform(0.5, 2.0, (2, 2 * S, 2 * S))
    return _dev(u), _dev(f), _dev(th)


def test_level_polish(model):
    """polish = 0 is the call without the keyword; polish = K + 1 is poisson.relax of that result with the level's
    own 1 / h^2 = (2S - 1)^2."""
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd.tiled_inference import upscale_level
    K, _ = _KT()
    S = 30
    u, f, th = _level_fields(S, 30)
    plain = upscale_level(model, u, f, th)
    assert torch.equal(upscale_level(model, u, f, th, polish=0), plain)
    got = upscale_level(model, u, f, th, polish=K + 1)
    want = P.relax(plain, f, th, K + 1, inv_h2=float((2 * S - 1) ** 2))
    assert got.shape == (2, 2 * S, 2 * S) and got.dtype == torch.float64
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)) and not torch.equal(got, plain)
    half = upscale_level(model, u, f, th, polish=2, polish_omega=0.5)
    assert torch.equal(half.view(torch.int64), P.relax(plain, f, th, 2, 0.5, inv_h2=float(59 ** 2)).view(torch.int64))


def test_cascade_polish_feeds_the_next_level(model):
    """20 -> 80 with polish = 3 equals the two levels chained by hand: the second level reads the polished field."""
    from superresolution_for_pdes_amd.tiled_inference import upscale_cascade, upscale_level
    u, f40, th40 = _level_fields(20, 20)
    _, f80, th80 = _level_fields(40, 40)
    got = upscale_cascade(model, u, {40: f40, 80: f80}, {40: th40, 80: th80}, 80, polish=3)
    mid = upscale_level(model, u, f40, th40, polish=3)
    want = upscale_level(model, mid, f80, th80, polish=3)
    assert got.shape == (2, 80, 80) and torch.equal(got.view(torch.int64), want.view(torch.int64))
    unpolished_mid = upscale_level(model, u, f40, th40)
    assert not torch.equal(upscale_level(model, unpolished_mid, f80, th80, polish=3), want)
