"""The divergence-form smoother with zero-flux (Neumann) sides on the GPU (relax_kernel<DivOp<HARM, true>> of
csrc/relax.hip, ABI 23: srpde_div_relax_bc; hipops.pde_relax(bc=), poisson.relax(bc=), the cascade's ``polish_bc``)
against relax_div_bc_np, the one-pass-per-sweep numpy restatement established in test_div_bc_smoother_host.py.  The
kernel rounds every operation once in the header's order and multiplies the zero coefficient of a missing face in, so
the comparison is by equality of bits -- the signs of zeros included -- whatever the tiling.

E = 3.  Sizes n: 2 (the smallest a pattern takes), 3, 5 (grids inside one halo), T - 1, T, T + 1 (one tile with and
without a ragged edge, the first two-tile grid) and 2T + K + 3 (three tiles per axis: tiles whose halo crosses each
side, tiles that touch none).  Sweeps: 0 (a copy), 1, K (one full launch), K + 1 (two launches, through the workspace)
and 2K + 1 (three: the other ping-pong parity).  Patterns: the four single zero-flux sides (a swapped side or axis
fails one of them), "ddnn" and "nnnn"."""
import numpy as np
import pytest
import torch

import div_bc_ref as B
import poisson_div_ref as D
from div_bc_smoother_ref import relax_div_bc_np

pytestmark = pytest.mark.gpu

E = 3
PATTERNS = ("nddd", "dndd", "ddnd", "dddn", "ddnn", "nnnn")


def _KT():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import hipops as H
    return H.pde_relax_sweeps_per_launch(), H.RELAX_TILE


def _sizes():
    K, T = _KT()
    return [2, 3, 5, T - 1, T, T + 1, 2 * T + K + 3]


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


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", _sizes())
def test_bit_equal_to_the_numpy_restatement(n, mean):
    from superresolution_for_pdes_amd import hipops as H
    code = D.MEANS.index(mean)
    K, _ = _KT()
    u, f, th = _fields(n, 300 + n)
    ud, fd, td = _dev(u), _dev(f), _dev(th)
    inv_h2 = float((n - 1) ** 2)
    for bc in PATTERNS:
        for omega in (0.8, 1.0):
            for sweeps in (0, 1, K, K + 1, 2 * K + 1):
                got = H.pde_relax(ud, fd, td, inv_h2, sweeps, omega, face_mean=code, bc=B.mask(bc))
                want = relax_div_bc_np(u, f, th, mean, bc, inv_h2, sweeps, omega)
                assert got.shape == (E, n, n) and got.dtype == torch.float64
                assert _same_bits(got, want), (n, mean, bc, omega, sweeps,
                                               float(np.abs(got.cpu().numpy() - want).max()))
    assert _same_bits(ud, u) and _same_bits(fd, f) and _same_bits(td, th)       # the inputs are untouched


@pytest.mark.parametrize("mean", D.MEANS)
def test_four_dirichlet_sides_are_the_existing_call(mean):
    """bc = 0 / None / "dddd" give the bits of the call without the keyword, through hipops and through poisson."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd import poisson as P
    K, T = _KT()
    n = T + 1
    code = D.MEANS.index(mean)
    u, f, th = (_dev(a) for a in _fields(n, 7))
    inv_h2 = float((n - 1) ** 2)
    for sweeps in (1, K + 1):
        base = H.pde_relax(u, f, th, inv_h2, sweeps, 0.8, face_mean=code)
        for bc in (0, None):
            assert torch.equal(H.pde_relax(u, f, th, inv_h2, sweeps, 0.8, face_mean=code, bc=bc).view(torch.int64),
                               base.view(torch.int64))
        for bc in (None, "dddd"):
            got = P.relax(u, f, th, sweeps, form="divergence", face_mean=mean, bc=bc)
            assert torch.equal(got.view(torch.int64), base.view(torch.int64))
        held = H.pde_relax(u, f, th, inv_h2, sweeps, 0.8, True, face_mean=code)
        assert torch.equal(H.pde_relax(u, f, th, inv_h2, sweeps, 0.8, True, face_mean=code, bc=0).view(torch.int64),
                           held.view(torch.int64))
        assert not torch.equal(P.relax(u, f, th, sweeps, form="divergence", face_mean=mean, bc="ddnn"), base)


@pytest.mark.parametrize("mean", D.MEANS)
def test_constants_are_a_fixed_point_of_the_insulated_box(mean):
    """n = T + 1 (two tiles per axis), four zero-flux sides, f = 0: a constant field comes back bit for bit."""
    from superresolution_for_pdes_amd import poisson as P
    K, T = _KT()
    n = T + 1
    th = _dev(np.random.default_rng(9).uniform(0.5, 2.0, (E, n, n)))
    u = torch.full((E, n, n), 0.7310585786300049, dtype=torch.float64, device="cuda")
    z = torch.zeros_like(u)
    for sweeps in (1, K, 2 * K + 1):
        for omega in (0.8, 1.0):
            got = P.relax(u, z, th, sweeps, omega, form="divergence", face_mean=mean, bc="nnnn")
            assert torch.equal(got.view(torch.int64), u.view(torch.int64)), (sweeps, omega)
    moved = P.relax(u, z, th, 1, form="divergence", face_mean=mean)
    assert float((moved - u).abs().max()) > 0.1


@pytest.mark.parametrize("mean", D.MEANS)
def test_residual_and_error_fall_on_a_noisy_solution(mean):
    """n = 40, theta ~ U(0.5, 2), "ddnn": 16 sweeps with the pattern on solve_div(bc="ddnn") solutions + noise of
    1e-2 std(u) lower the pattern's residual RMS and the RMS error of every example.  16 sweeps without the pattern
    pull the two zero-flux boundary lines (columns 0 and n - 1) towards the ghost ring's 0: the pattern's residual RMS
    on those lines ends above where it started."""
    from superresolution_for_pdes_amd import poisson as P
    n, bc = 40, "ddnn"
    _, f, th = _fields(n, 5)
    f, th = _dev(f - 0.1), _dev(th)
    u = P.solve_div(f, th, face_mean=mean, bc=bc)
    g = torch.Generator(device="cpu").manual_seed(3)
    noise = torch.randn(E, n, n, generator=g, dtype=torch.float64).to("cuda")
    noisy = u + 1e-2 * u.std(dim=(1, 2), keepdim=True) * noise
    smooth = P.relax(noisy, f, th, 16, form="divergence", face_mean=mean, bc=bc)
    plain = P.relax(noisy, f, th, 16, form="divergence", face_mean=mean)
    before = P.residual_metrics(noisy, f, th, form="divergence", face_mean=mean, bc=bc)
    after = P.residual_metrics(smooth, f, th, form="divergence", face_mean=mean, bc=bc)
    e0 = (noisy - u).pow(2).mean((1, 2)).sqrt()
    e1 = (smooth - u).pow(2).mean((1, 2)).sqrt()
    print(f"{mean}: residual rms", before[:, 0].tolist(), "->", after[:, 0].tolist())
    print(f"{mean}: rms error", e0.tolist(), "->", e1.tolist())
    assert bool((after[:, 0] < before[:, 0]).all()) and bool((e1 < e0).all())

    def lines(v):
        r = P.apply_div(v, th, face_mean=mean, bc=bc) - f
        return torch.cat([r[:, :, 0], r[:, :, -1]], dim=1).pow(2).mean(1).sqrt()
    l0, l_bc, l_plain = lines(noisy), lines(smooth), lines(plain)
    print(f"{mean}: zero-flux lines' residual rms", l0.tolist(), "-> with bc", l_bc.tolist(), ", without",
          l_plain.tolist())
    assert bool((l_plain > l0).all()) and bool((l_bc < l0).all())


def test_argument_errors_of_the_raw_entry():
    """srpde_div_relax_bc refuses a bad mask, a mask with interior_only and a mask at n = 1, on real device buffers;
    the mask-less combinations run."""
    from superresolution_for_pdes_amd import _lib
    from superresolution_for_pdes_amd.hipops import stream_ptr
    _KT()

    def run(n, bc, interior):
        u = torch.ones(1, n, n, dtype=torch.float64, device="cuda")
        out = torch.empty_like(u)
        th = torch.ones_like(u)
        f = torch.zeros_like(u)
        return _lib.call("srpde_div_relax_bc", u.data_ptr(), f.data_ptr(), th.data_ptr(), out.data_ptr(), 1, n, 1, bc,
                         float(max(n - 1, 1) ** 2), 1, 0.8, interior, 0, 0, stream_ptr())
    for bc in (-1, 16):
        with pytest.raises(RuntimeError, match="side mask"):
            run(8, bc, 0)
    with pytest.raises(RuntimeError, match="interior_only"):
        run(8, 3, 1)
    with pytest.raises(RuntimeError, match="n >= 2"):
        run(1, 3, 0)
    assert run(8, 3, 0) == 0 and run(8, 0, 1) == 0 and run(1, 0, 0) == 0 and run(2, 15, 0) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def model():
    from superresolution_for_pdes_amd.models import UNet, init_weights
    torch.manual_seed(11)
    m = UNet().to("cuda")
    m.apply(init_weights)
    return m.eval()


def test_level_polish(model):
    """polish_bc="ddnn" with polish = 8 is poisson.relax(bc="ddnn") of the unpolished output with the level's own
    1 / h^2 = (2S - 1)^2, bit for bit; polish_bc=None / "dddd" is the call without the keyword."""
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd.tiled_inference import upscale_level
    S = 30
    rng = np.random.default_rng(30)
    u = _dev(rng.normal(2e-4, 1e-4, (2, S, S)))
    x = np.linspace(0, 1, 2 * S)
    X, Y = np.meshgrid(x, x)
    f = _dev(np.stack([np.sin(2 * np.pi * (3.3 + e) * X) * np.sin(2 * np.pi * (2.1 - e) * Y) + 0.1 for e in range(2)]))
    th = _dev(rng.uniform(0.5, 2.0, (2, 2 * S, 2 * S)))
    plain = upscale_level(model, u, f, th)
    inv_h2 = float((2 * S - 1) ** 2)
    got = upscale_level(model, u, f, th, polish=8, polish_form="divergence", polish_bc="ddnn")
    want = P.relax(plain, f, th, 8, inv_h2=inv_h2, form="divergence", bc="ddnn")
    assert got.shape == (2, 2 * S, 2 * S) and got.dtype == torch.float64
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    base = upscale_level(model, u, f, th, polish=8, polish_form="divergence")
    assert not torch.equal(got, base)
    for bc in (None, "dddd"):
        again = upscale_level(model, u, f, th, polish=8, polish_form="divergence", polish_bc=bc)
        assert torch.equal(again.view(torch.int64), base.view(torch.int64))
