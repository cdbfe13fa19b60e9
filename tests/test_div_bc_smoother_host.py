"""CPU: zero-flux (Neumann) sides in the divergence-form smoother and loss term (ABI 23: srpde_div_relax_bc,
srpde_physics_loss_div_fwd_bc; poisson.relax(bc=), functional.PhysicsMSELoss(bc=), tiled_inference's ``polish_bc``,
online.SampleStream(bc=), train_enhanced --bc).

The restatements of tests/div_bc_smoother_ref.py, which the GPU tests compare the kernels with, are established here on
their own: against the bc-less restatements, against the dense operator of tests/div_bc_ref.py, and against autograd.
Then every refusal of the Python layers and of the command line, none of which needs a device, and the argument checks
of the two C entries, each of which fails before a launch."""
import numpy as np
import pytest
import torch

import div_bc_ref as B
import div_bc_smoother_ref as S
import poisson_div_ref as D
from test_div_smoother_host import normalised, relax_div_np, restatement_div

INV_H2 = S.INV_H2
MIXED = ("ddnn", "ndnd", "nddd")


@pytest.fixture(scope="module")
def lib():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import _lib
    return _lib


# ---- the smoother's restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_four_dirichlet_sides_are_the_plain_restatement(mean):
    n, E = 13, 3
    u, f, th = D.field_u(n, 1, E), D.field_u(n, 2, E), D.field_theta(n, 3, 0.5, 2.0, E)
    for sweeps, omega in ((0, 0.8), (1, 0.8), (5, 1.0)):
        got = S.relax_div_bc_np(u, f, th, mean, "dddd", (n - 1) ** 2, sweeps, omega)
        want = relax_div_np(u, f, th, mean, (n - 1) ** 2, sweeps, omega)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("mean", D.MEANS)
def test_constants_are_a_fixed_point_of_the_insulated_box(mean):
    """Four zero-flux sides, f = 0: every face term is c * (v - v) = 0 or 0 * (0 - v) = -0, so a constant field comes
    back bit for bit after any number of sweeps.  With the ghost ring it does not."""
    n = 11
    th = D.field_theta(n, 4, 0.5, 2.0, 2)
    u = np.full((2, n, n), 0.7310585786300049)
    z = np.zeros_like(u)
    for sweeps in (1, 3, 17):
        for omega in (0.8, 1.0):
            got = S.relax_div_bc_np(u, z, th, mean, "nnnn", (n - 1) ** 2, sweeps, omega)
            assert got.tobytes() == u.tobytes()
    moved = S.relax_div_bc_np(u, z, th, mean, "dddd", (n - 1) ** 2, 1)
    assert np.abs(moved - u).max() > 0.1


@pytest.mark.parametrize("bc", MIXED)
@pytest.mark.parametrize("mean", D.MEANS)
def test_dense_solutions_are_fixed_points(mean, bc):
    """n = 9, theta ~ U(0.5, 2): the dense solution of D_theta,bc u = f moves by <= 1e-13 max|u| in one sweep and in
    eight (the bound tests/test_div_smoother_host.py sets for the bc-less smoother); the bc-less sweep moves it."""
    n = 9
    th, f = D.field_theta(n, 5, 0.5, 2.0), D.forcing(n)
    u = np.linalg.solve(B.dense(th, mean, bc), f.reshape(-1)).reshape(n, n)
    for sweeps in (1, 8):
        got = S.relax_div_bc_np(u[None], f[None], th[None], mean, bc, (n - 1) ** 2, sweeps)[0]
        moved = np.abs(got - u).max() / np.abs(u).max()
        print(f"{mean} {bc} sweeps={sweeps}: moved {moved:.2e} of max|u|")
        assert moved <= 1e-13
    plain = relax_div_np(u[None], f[None], th[None], mean, (n - 1) ** 2, 1)[0]
    assert np.abs(plain - u).max() / np.abs(u).max() > 1e-3


@pytest.mark.parametrize("omega", [0.8, 1.0])
@pytest.mark.parametrize("bc", MIXED + ("nnnn",))
@pytest.mark.parametrize("mean", D.MEANS)
def test_error_operator_spectrum(mean, bc, omega):
    """n = 7: the dense error operator, column j = one sweep of e_j with f = 0, is I + omega diag(-D)^-1 D with D the
    dense operator of tests/div_bc_ref.py.  Its eigenvalues are real and lie in (-1, 1]; 1 is reached only by the
    constants of "nnnn".
    One case cannot meet the open end: "nnnn" with omega = 1.  The grid is bipartite, so plain Jacobi's spectrum is
    symmetric about 0, and since the constants give +1 the checkerboard-weighted vector gives exactly -1 (measured:
    -1 to 2e-16).  There the test asserts that -1 is attained and nothing lies below it: the mode neither grows nor
    decays, as the header states ("no error component grows")."""
    n = 7
    theta = D.field_theta(n, 6, 0.5, 2.0)
    eye = np.eye(n * n).reshape(n * n, n, n)
    G = S.relax_div_bc_np(eye, np.zeros_like(eye), np.broadcast_to(theta, eye.shape), mean, bc, (n - 1) ** 2, 1,
                          omega).reshape(n * n, n * n).T
    Dm = B.dense(theta, mean, bc)
    want = np.eye(n * n) + omega * (Dm / -np.diag(Dm)[:, None])
    assert np.abs(G - want).max() <= 1e-14
    ev = np.linalg.eigvals(G)
    print(f"{mean} {bc} omega={omega}: eigenvalues in [{ev.real.min():.6f}, {ev.real.max():.6f}], "
          f"max |imag| {np.abs(ev.imag).max():.1e}")
    assert np.abs(ev.imag).max() <= 1e-9
    assert ev.real.max() <= 1.0 + 1e-12
    if bc == "nnnn":
        assert abs(ev.real.max() - 1.0) <= 1e-12
    else:
        assert ev.real.max() < 1.0 - 1e-6
    if bc == "nnnn" and omega == 1.0:
        assert abs(ev.real.min() + 1.0) <= 1e-12
    else:
        assert ev.real.min() > -1.0 + 1e-6


# ---- the loss restatement --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields():
    """(u, f, theta) [2, 24, 24]: sample 0 is scored as a whole-domain sample, sample 1 as a crop."""
    n = 24
    return D.field_u(n, 11, 2), np.stack([D.forcing(n), D.forcing(n, 2.3, 4.1)]), D.field_theta(n, 12, 0.5, 2.0, 2)


def batch(fields, noise=1e-2, seed=0):
    t, x, stats = normalised(*fields)
    g = torch.Generator().manual_seed(seed)
    y = t + noise * torch.randn(t.shape, generator=g, dtype=torch.float64)
    return y, t, x, torch.tensor([0, 1], dtype=torch.int32), stats


@pytest.mark.parametrize("bc", MIXED + ("nnnn",))
@pytest.mark.parametrize("mean", D.MEANS)
def test_loss_restatement_is_the_operator_residual(fields, mean, bc):
    """fp64: on the whole-domain sample r = (D_theta,bc u - f) / f_std with tests/div_bc_ref.py's operator on the
    denormalised field, to 1e-12 of max|r|, and pde is its mean square over the counted nodes; on the crop r is the
    bc-less operator's on the interior."""
    y, t, x, kind, stats = batch(fields)
    out = S.restatement_div_bc(y, t, x, kind, stats, 1.0, mean=mean, bc=bc)
    mu_u, sg_u, mu_f, sg_f, mu_t, sg_t = [float(v) for v in stats]
    u = (sg_u * y[:, 0] + mu_u).numpy()
    theta = (sg_t * x[:, 1] + mu_t).numpy()
    f = (sg_f * x[:, 2] + mu_f).numpy()
    n = u.shape[-1]
    want0 = (B.apply(u[0], theta[0], mean, bc, inv_h2=INV_H2[0]) - f[0]) / sg_f
    want1 = (D.apply(u[1], theta[1], mean, INV_H2[1]) - f[1]) / sg_f
    got = out["r"][:, 0].numpy()
    assert np.abs(got[0] - want0).max() <= 1e-12 * np.abs(want0).max()
    assert np.abs(got[1] - want1)[1:-1, 1:-1].max() <= 1e-12 * np.abs(want1[1:-1, 1:-1]).max()
    M = n * n + (n - 2) ** 2
    assert out["M"] == M
    pde = (np.sum(want0 ** 2) + np.sum(want1[1:-1, 1:-1] ** 2)) / M
    assert abs(float(out["pde"]) - pde) <= 1e-12 * pde
    # the pattern matters: the bc-less residual of the same field differs on the zero-flux lines
    plain = restatement_div(y, t, x, kind, stats, 1.0, mean=mean)
    assert abs(float(plain["pde"]) - pde) > 1e-3 * pde


@pytest.mark.parametrize("bc", MIXED + ("nnnn",))
def test_loss_gradient_is_autograd_and_the_symmetric_operator(fields, bc):
    """The closed form of include/srpde.h -- 2 (y - t) / N + weight (2 sigma_u / (M sigma_f)) ih2 Dt(m r), Dt the same
    face sum with the sides bc (the pattern's operator is symmetric) -- equals torch's fp64 autograd of the
    restatement, to 1e-12."""
    mean, weight = "harmonic", 0.3
    y, t, x, kind, stats = batch(fields)
    yd = y.clone().requires_grad_(True)
    out = S.restatement_div_bc(yd, t, x, kind, stats, weight, mean=mean, bc=bc)
    out["total"].backward()
    sg_u, sg_f = float(stats[1]), float(stats[3])
    q = out["q"].detach()[:, 0].numpy()
    theta = out["theta"].detach()[:, 0].numpy()
    for b in range(2):
        adj = B.apply(q[b], theta[b], mean, bc if b == 0 else "dddd", inv_h2=INV_H2[b])
        want = 2.0 * (y - t)[b, 0].numpy() / y.numel() + weight * (2.0 * sg_u / (out["M"] * sg_f)) * adj
        got = yd.grad[b, 0].numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("mean", D.MEANS)
def test_crops_do_not_see_the_pattern(fields, mean):
    """A kind-1 sample counts interior nodes only: its loss terms and its gradient are the same bits for all 16 masks,
    and they are the bc-less restatement's."""
    y, t, x, _, stats = batch(fields)
    kind = torch.tensor([1, 1], dtype=torch.int32)
    yd = y.clone().requires_grad_(True)
    ref = restatement_div(yd, t, x, kind, stats, 0.3, mean=mean)
    ref["total"].backward()
    for bc in B.PATTERNS:
        yb = y.clone().requires_grad_(True)
        out = S.restatement_div_bc(yb, t, x, kind, stats, 0.3, mean=mean, bc=bc)
        out["total"].backward()
        assert torch.equal(out["pde"].detach(), ref["pde"].detach())
        assert torch.equal(out["total"].detach(), ref["total"].detach())
        assert torch.equal(yb.grad, yd.grad)


def test_four_zero_flux_sides_do_not_see_the_mean(fields):
    """ "nnnn": D_theta 1 = 0, so the residual does not depend on u_mean."""
    y, t, x, _, stats = batch(fields)
    kind = torch.tensor([0, 0], dtype=torch.int32)
    other = stats.clone()
    other[0] += 5.0
    a = S.restatement_div_bc(y, t, x, kind, stats, 1.0, bc="nnnn")
    b = S.restatement_div_bc(y, t, x, kind, other, 1.0, bc="nnnn")
    assert torch.equal(a["r"], b["r"])
    c = S.restatement_div_bc(y, t, x, kind, other, 1.0, bc="ddnn")
    assert not torch.equal(c["r"], S.restatement_div_bc(y, t, x, kind, stats, 1.0, bc="ddnn")["r"])


# ---- the C entries ---------------------------------------------------------------------------------------------
def test_abi_version(lib):
    assert lib.query("srpde_version") == 23


def test_div_relax_bc_argument_checks(lib):
    """The refusals srpde_div_relax_bc adds to srpde_div_relax's come before a launch (the pointers are never
    dereferenced on the host)."""
    cd = lib.lib()
    n, E = 40, 2
    field = E * n * n * 8
    A, F, C, O = ((1 << 20) + k * 2 * field for k in range(4))

    def run(E=E, n=n, mean=1, bc=3, sweeps=8, omega=0.8, interior=0, u=A):
        return cd.srpde_div_relax_bc(u, F, C, O, E, n, mean, bc, 1521.0, sweeps, omega, interior, 0, 0, 0)
    for bc in (-1, 16, 255):
        assert run(bc=bc) < 0 and "side mask" in lib.last_error()
    assert run(interior=1) < 0 and "interior_only" in lib.last_error()
    assert run(n=1) < 0 and "n >= 2" in lib.last_error()
    assert run(u=0) < 0 and "null" in lib.last_error()
    assert run(mean=2) < 0 and "face_mean" in lib.last_error()
    assert run(omega=1.5) < 0 and "omega" in lib.last_error()
    assert run(sweeps=9) < 0 and "workspace too small" in lib.last_error()


def test_physics_div_bc_argument_checks(lib):
    cd = lib.lib()

    def fwd(B=2, n=40, mean=1, bc=3, y=16, ws_bytes=1 << 20):
        return cd.srpde_physics_loss_div_fwd_bc(y, 16, 16, 16, 16, B, n, mean, bc, 0.1, INV_H2[0], INV_H2[1], 16, 0, 16,
                                                ws_bytes, 0)
    for bc in (-1, 16):
        assert fwd(bc=bc) < 0 and "side mask" in lib.last_error()
    assert fwd(y=0) < 0 and "null" in lib.last_error()
    assert fwd(n=2) < 0 and "n=2" in lib.last_error()
    assert fwd(mean=2) < 0 and "face_mean" in lib.last_error()
    need = lib.query("srpde_physics_loss_div_workspace_size", 2, 40)
    assert fwd(ws_bytes=need - 1) < 0 and "workspace too small" in lib.last_error()


# ---- Python keywords and the command line ------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    from superresolution_for_pdes_amd import functional as F
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd.online import SampleStream
    from superresolution_for_pdes_amd.tiled_inference import upscale_cascade, upscale_level
    z = np.zeros((4, 4))
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        P.relax(z, z, z, 1, bc="ddnn")
    with pytest.raises(ValueError, match="bc must be None or four"):
        P.relax(z, z, z, 1, form="divergence", bc="ddn")
    with pytest.raises(ValueError, match="interior_only"):
        P.relax(z, z, z, 1, interior_only=True, form="divergence", bc="ddnn")
    with pytest.raises(ValueError, match="n >= 2"):
        P.relax(np.zeros((1, 1)), np.zeros((1, 1)), np.ones((1, 1)), 1, form="divergence", bc="nddd")
    zt = torch.zeros(1, 4, 4, dtype=torch.float64)
    for bad in (-1, 16, "ddnn", 1.0, True):
        with pytest.raises(ValueError, match="side mask"):
            H.pde_relax(zt, zt, zt, 9.0, 1, face_mean=1, bc=bad)
    with pytest.raises(ValueError, match="divergence form"):
        H.pde_relax(zt, zt, zt, 9.0, 1, bc=3)
    with pytest.raises(ValueError, match="interior_only"):
        H.pde_relax(zt, zt, zt, 9.0, 1, interior_only=True, face_mean=1, bc=3)
    with pytest.raises(ValueError, match="n >= 2"):
        H.pde_relax(zt[:, :1, :1], zt[:, :1, :1], zt[:, :1, :1], 9.0, 1, face_mean=1, bc=3)
    y, x = torch.zeros(1, 1, 4, 4), torch.zeros(1, 3, 4, 4)
    kind, stats = torch.zeros(1, dtype=torch.int32), torch.ones(6)
    with pytest.raises(ValueError, match="side mask"):
        H.physics_loss_fwd(y, y, x, kind, stats, 0.1, INV_H2, face_mean=1, bc=16)
    with pytest.raises(ValueError, match="divergence form"):
        H.physics_loss_fwd(y, y, x, kind, stats, 0.1, INV_H2, bc=3)
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        F.physics_loss_terms(y, y, x, kind, stats, 0.1, bc="ddnn")
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        F.physics_mse_loss(y, y, x, kind, stats, 0.1, bc="nnnn")
    with pytest.raises(ValueError, match="bc must be None or four"):
        F.PhysicsMSELoss(0.1, stats, form="divergence", bc="xxxx")
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        F.PhysicsMSELoss(0.1, stats, bc="ddnn")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # an accepted pattern reaches the device check
        F.physics_loss_terms(y, y, x, kind, stats, 0.1, form="divergence", bc="nnnn")
    crit = F.PhysicsMSELoss(0.1, stats, form="divergence", bc="ddnn")
    assert crit.bc == "ddnn" and F.PhysicsMSELoss(0.1, stats).bc is None
    for fn in (upscale_level, upscale_cascade):
        args = (None, z, z, z) if fn is upscale_level else (None, z, {}, {}, 8)
        with pytest.raises(ValueError, match="polish_bc belongs"):
            fn(*args, polish=1, polish_bc="ddnn")
        with pytest.raises(ValueError, match="bc must be None or four"):
            fn(*args, polish=1, polish_form="divergence", polish_bc="dn")
    kw = dict(theta_range=(0.5, 2.0), device="cpu")     # an accepted pattern reaches the device check
    with pytest.raises(ValueError, match="singular"):
        SampleStream(1, 8, form="divergence", bc="nnnn", **kw)
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        SampleStream(1, 8, bc="ddnn", **kw)
    with pytest.raises(ValueError, match="bc must be None or four"):
        SampleStream(1, 8, form="divergence", bc="dd", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SampleStream(1, 8, form="divergence", bc="ddnn", **kw)


DIV = ["--operator", "divergence", "--online", "2", "--online-theta", "0.5", "2.0"]


@pytest.mark.parametrize("argv,word", [
    (["--bc", "ddnn"], "--online and --operator divergence"),
    (["--online", "2", "--bc", "ddnn"], "--online and --operator divergence"),
    (["--online", "2", "--online-theta", "0.5", "2.0", "--bc", "ddnn"], "--online and --operator divergence"),
    (DIV + ["--bc", "nnnn"], "singular"),
    (DIV + ["--bc", "ddn"], "--bc"),
    (DIV + ["--bc", "ddxx", "--pde-div-weight", "0.01"], "--bc"),
])
def test_cli_refusals_need_no_device(argv, word, monkeypatch):
    from superresolution_for_pdes_amd import train_enhanced as TE

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(torch.cuda, "manual_seed", no_device)
    with pytest.raises(SystemExit) as e:
        TE.main(argv)
    assert word in str(e.value)


def test_cli_accepts_a_pattern():
    from superresolution_for_pdes_amd import train_enhanced as TE
    assert TE.arg_parser().parse_args([]).bc is None
    for bc in ("ddnn", "dddd", "nddd"):
        args = TE.arg_parser().parse_args(DIV + ["--bc", bc, "--pde-div-weight", "0.01"])
        assert args.bc == bc
        TE.check_operator_args(args)
