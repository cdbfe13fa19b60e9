"""The divergence-form weighted-Jacobi smoother on the GPU (relax_kernel<DivOp> of csrc/relax.hip, ABI 19;
hipops.pde_relax(face_mean=...), poisson.relax(form="divergence"), the cascade's ``polish_form``) against
relax_div_np, the one-pass-per-sweep numpy restatement established in test_div_smoother_host.py.  The kernel rounds
every operation once in the header's order, so the comparison is by equality of bits, whatever the tiling.

E = 3.  Sizes n: 1, 2, 3, 5 (grids smaller than the halo, the smallest with an interior), T - 1, T, T + 1 (one tile
with and without a ragged edge, the first two-tile grid: a seam inside the halo) and 2T + K + 3 (three tiles per axis,
a ragged last one).  Sweeps: 0 (a copy), 1, K - 1, K (one launch, short and full), K + 1 (two launches, through the
workspace) and 2K + 1 (three launches: the other ping-pong parity)."""
import numpy as np
import pytest
import torch

import poisson_div_ref as D
from test_div_smoother_host import relax_div_np
from test_relax_host import mode_factor, sine_mode

pytestmark = pytest.mark.gpu

E = 3


def _KT():
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
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", _sizes())
def test_bit_equal_to_the_numpy_restatement(n, mean, interior_only):
    from superresolution_for_pdes_amd import hipops as H
    code = D.MEANS.index(mean)
    if interior_only and n < 3:
        with pytest.raises(RuntimeError, match="srpde_div_relax"):      # refused, not computed
            H.pde_relax(*(_dev(a) for a in _fields(n, n)), 1.0, 1, 0.8, True, face_mean=code)
        return
    K, _ = _KT()
    u, f, th = _fields(n, 100 + n)
    ud, fd, td = _dev(u), _dev(f), _dev(th)
    inv_h2 = float(max(n - 1, 1) ** 2)
    ring = np.ones((n, n), bool)
    ring[1:-1, 1:-1] = False
    for omega in (0.8, 1.0):
        for sweeps in (0, 1, K - 1, K, K + 1, 2 * K + 1):
            got = H.pde_relax(ud, fd, td, inv_h2, sweeps, omega, interior_only, face_mean=code)
            want = relax_div_np(u, f, th, mean, inv_h2, sweeps, omega, interior_only)
            assert got.shape == (E, n, n) and got.dtype == torch.float64
            assert _same_bits(got, want), (n, mean, interior_only, omega, sweeps,
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
    for mean in D.MEANS:
        got = P.relax(v, np.zeros((n, n)), np.ones((n, n)), 2 * K + 1, omega, form="divergence",
                      face_mean=mean).cpu().numpy()
        err = np.abs(got[0] - lam ** (2 * K + 1) * v).max()
        print(f"{mean}: lambda={lam:.6f} err={err:.2e}")
        assert got.shape == (1, n, n) and err <= 1e-13


@pytest.mark.parametrize("mean", D.MEANS)
def test_residual_and_error_fall_on_a_noisy_solution(mean):
    """n = 40, theta ~ U(0.5, 2): 8 sweeps on solve_div solutions + 1e-5 noise lower the divergence residual RMS and
    the RMS error of every example (0.083 -> 0.0012 and 1.0e-5 -> 1.5e-6 in the numpy prototype)."""
    from superresolution_for_pdes_amd import poisson as P
    n = 40
    _, f, th = _fields(n, 5)
    f, th = _dev(f - 0.1), _dev(th)
    u = P.solve_div(f, th, face_mean=mean)
    g = torch.Generator(device="cpu").manual_seed(3)
    noisy = u + (1e-5 * torch.randn(E, n, n, generator=g, dtype=torch.float64)).to("cuda")
    smooth = P.relax(noisy, f, th, 8, form="divergence", face_mean=mean)
    before = P.residual_metrics(noisy, f, th, form="divergence", face_mean=mean)
    after = P.residual_metrics(smooth, f, th, form="divergence", face_mean=mean)
    e0 = (noisy - u).pow(2).mean((1, 2)).sqrt()
    e1 = (smooth - u).pow(2).mean((1, 2)).sqrt()
    print(f"{mean}: residual rms", before[:, 0].tolist(), "->", after[:, 0].tolist())
    print(f"{mean}: rms error", e0.tolist(), "->", e1.tolist())
    assert bool((after[:, 0] < before[:, 0]).all()) and bool((e1 < e0).all())


@pytest.fixture(scope="module")
def model():
    from superresolution_for_pdes_amd.models import UNet, init_weights
    torch.manual_seed(11)
    m = UNet().to("cuda")
    m.apply(init_weights)
    return m.eval()


def test_level_polish(model):
    """polish_form="divergence" with polish = K + 1 is poisson.relax(form="divergence") of the unpolished output with
    the level's own 1 / h^2 = (2S - 1)^2, bit for bit; the default keywords change nothing."""
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd.tiled_inference import upscale_level
    K, _ = _KT()
    S = 30
    rng = np.random.default_rng(30)
    u = _dev(rng.normal(2e-4, 1e-4, (2, S, S)))
    x = np.linspace(0, 1, 2 * S)
    X, Y = np.meshgrid(x, x)
    f = _dev(np.stack([np.sin(2 * np.pi * (3.3 + e) * X) * np.sin(2 * np.pi * (2.1 - e) * Y) + 0.1 for e in range(2)]))
    th = _dev(rng.uniform(0.5, 2.0, (2, 2 * S, 2 * S)))
    plain = upscale_level(model, u, f, th)
    assert torch.equal(upscale_level(model, u, f, th, polish=0, polish_form="divergence"), plain)
    inv_h2 = float((2 * S - 1) ** 2)
    for mean in D.MEANS:
        got = upscale_level(model, u, f, th, polish=K + 1, polish_form="divergence", polish_face_mean=mean)
        want = P.relax(plain, f, th, K + 1, inv_h2=inv_h2, form="divergence", face_mean=mean)
        assert got.shape == (2, 2 * S, 2 * S) and got.dtype == torch.float64
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)) and not torch.equal(got, plain)
    # the pointwise path: the default keywords, spelled out or not
    a = upscale_level(model, u, f, th, polish=K + 1)
    b = upscale_level(model, u, f, th, polish=K + 1, polish_form="pointwise", polish_face_mean="harmonic")
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(a.view(torch.int64), P.relax(plain, f, th, K + 1, inv_h2=inv_h2).view(torch.int64))
    assert not torch.equal(a, got)
