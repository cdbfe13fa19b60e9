"""CPU: the mathematics that boundary values and prescribed fluxes rest on (ABI 23, extended), checked in numpy before any kernel
relies on it -- the affine split A_bd u = D_bc u - sigma u + b for all 16 patterns, zero data against tests/div_bc_ref.py,
manufactured and Laplace problems through dense solves and the numpy PCG with the stop rule on |f - b|, a window cut
from a larger solution, a refinement study, both gradients against fp64 autograd and finite differences, the smoother's
fixed point, and every refusal of the Python surface (none needs a device)."""
import numpy as np
import pytest
import torch

import div_bc_ref as BC
import div_bd_ref as BD
import poisson_div_ref as D

EPS = np.finfo(np.float64).eps


def _case(n, seed, lo=0.5, hi=2.0):
    return D.field_u(n, seed), D.field_theta(n, seed, lo, hi), BD.data(n, seed)


# ---- the operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_affine_split_for_every_pattern(mean):
    """A_bd u = D_bc u - sigma u + b with the dense matrix of D_bc, to rounding: every entry of the three terms is below
    4 theta_max inv_h2 max(|u|, |g|, |q|), and a handful of roundings separate the two orders of summation."""
    n = 6
    u, th, bd = _case(n, 0)
    for bc in BC.PATTERNS:
        for sigma in (0.0, 7.5):
            M = BC.dense(th, mean, bc, sigma)
            b = BD.affine(th, bd, mean, bc)
            want = (M @ u.reshape(-1)).reshape(n, n) + b
            got = BD.apply(u, th, bd, mean, bc, sigma)
            scale = 4.0 * th.max() * (n - 1) ** 2 * max(np.abs(u).max(), np.abs(bd).max())
            assert np.abs(got - want).max() <= 32 * EPS * scale, (bc, sigma)
            interior = b[1:-1, 1:-1]
            assert not interior.any(), bc                        # b lives on edge nodes only


@pytest.mark.parametrize("mean", D.MEANS)
def test_zero_data_reproduces_the_homogeneous_restatement(mean):
    n, B = 7, 2
    u, lam, f = D.field_u(n, 0, B), D.field_u(n, 1, B), D.field_u(n, 2, B)
    th = D.field_theta(n, 0, 0.1, 10.0, B)
    zero = np.zeros((4, n))
    for bc in BC.PATTERNS:
        for sigma in (0.0, 7.5):
            assert np.array_equal(BD.apply(u, th, zero, mean, bc, sigma), BC.apply(u, th, mean, bc, sigma)), bc
        assert np.array_equal(BD.step_rhs(u, f, th, zero, mean, 7.5, "cn", bc), BC.step_rhs(u, f, th, mean, 7.5, "cn", bc))
        assert np.array_equal(BD.theta_grad(u, lam, th, zero, mean, bc), BC.theta_grad(u, lam, th, mean, bc)), bc
        assert not BD.affine(th, zero, mean, bc).any()
        if bc != "nnnn":
            got = BD.pcg(f[0], th[0], zero, mean, bc, rtol=1e-10)
            want = BC.pcg(f[0], th[0], mean, bc, rtol=1e-10) if bc != "dddd" else None
            if want is not None:
                assert got[1] == want[1] and np.array_equal(got[0], want[0]), bc


# ---- solves ------------------------------------------------------------------------------------------------------------
SOLVE_RTOL = 1e-10


def _bound(rhs, lam_min, rtol=SOLVE_RTOL):
    """|u - u_dense| <= 2 rtol |f - b| / lam_min(-A + sigma I): tests/test_gpu_div_bc.py's bound with the new norm."""
    return 2.0 * rtol * np.linalg.norm(rhs) / lam_min


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 12])
def test_manufactured_solutions(n, mean):
    """Random u*, g, q and f := A_bd u*: the dense solve returns u* to rounding, the numpy PCG within the bound and
    within pcg_iterations."""
    from superresolution_for_pdes_amd import poisson as P
    ustar, th, bd = _case(n, 3)
    for bc in BC.PATTERNS:
        for sigma in (0.0, 50.0):
            if bc == "nnnn" and sigma == 0.0:
                continue
            f = BD.apply(ustar, th, bd, mean, bc, sigma)
            dense, lam_min = BD.solve_dense(f, th, bd, mean, bc, sigma)
            rhs = f - BD.affine(th, bd, mean, bc)
            cond = np.abs(np.linalg.eigvalsh(BC.dense(th, mean, bc, sigma))).max() / lam_min
            assert np.linalg.norm(dense - ustar) <= 64 * EPS * cond * np.linalg.norm(ustar), (bc, sigma)
            u, k, resid = BD.pcg(f, th, bd, mean, bc, sigma, rtol=SOLVE_RTOL)
            assert resid <= SOLVE_RTOL and 1 <= k <= P.pcg_iterations(0.5, 2.0, SOLVE_RTOL), (bc, sigma, k)
            assert np.linalg.norm(u - dense) <= _bound(rhs, lam_min), (bc, sigma)


@pytest.mark.parametrize("bc", ["dddd", "ddnn", "dnnd"])
def test_laplace_with_boundary_values_iterates(bc):
    """f = 0 with g != 0: |f| = 0, but the reference norm |f - b| is not, so the iteration runs and finds the dense
    solution (the homogeneous stop rule would return u = 0 after no iteration)."""
    n = 12
    _, th, bd = _case(n, 4)
    f = np.zeros((n, n))
    dense, lam_min = BD.solve_dense(f, th, bd, "harmonic", bc)
    u, k, resid = BD.pcg(f, th, bd, "harmonic", bc, rtol=SOLVE_RTOL)
    assert k >= 1 and resid <= SOLVE_RTOL
    assert np.linalg.norm(dense) > 0.1
    assert np.linalg.norm(u - dense) <= _bound(-BD.affine(th, bd, "harmonic", bc), lam_min)
    assert BC.pcg(f, th, "harmonic", bc, rtol=SOLVE_RTOL)[1:] == (0, 0.0)        # today's rule: nothing happens


def test_window_of_a_larger_solution_is_recovered():
    """A window of a constant-theta homogeneous solution, with the ring around it as g and the forcing rescaled to the
    window's own h, solves the window's problem: the two stencils are the same equation."""
    N, n, i0, j0, c = 33, 9, 7, 15, 1.7
    F = D.forcing(N)
    U = np.linalg.solve(D.dense(np.full((N, N), c), "harmonic"), F.reshape(-1)).reshape(N, N)
    win = U[i0:i0 + n, j0:j0 + n]
    bd = np.stack([U[i0 - 1, j0:j0 + n], U[i0 + n, j0:j0 + n], U[i0:i0 + n, j0 - 1], U[i0:i0 + n, j0 + n]])
    f = F[i0:i0 + n, j0:j0 + n] * (float(n - 1) / float(N - 1)) ** 2
    th = np.full((n, n), c)
    dense, lam_min = BD.solve_dense(f, th, bd)
    assert np.linalg.norm(dense - win) <= 1e-10 * np.linalg.norm(win)
    u, k, _ = BD.pcg(f, th, bd, rtol=SOLVE_RTOL)
    assert k >= 1 and np.linalg.norm(u - dense) <= _bound(f - BD.affine(th, bd), lam_min)
    # the window is a fixed point of its own smoother, to the rounding of one sweep
    swept = BD.relax(win[None], f[None], th[None], bd, "harmonic", "dddd", float((n - 1) ** 2), 1)[0]
    assert np.abs(swept - win).max() <= 1e-12 * np.abs(win).max()


# ---- refinement --------------------------------------------------------------------------------------------------------
def _analytic(n):
    """A smooth u*, theta and f = div(theta grad u*) on the project's grid, with the ghost values one h outside and the
    flux half a cell outside the column n - 1 side; x runs along the last axis."""
    h = 1.0 / (n - 1)
    t = np.linspace(0.0, 1.0, n)

    def u(x, y):
        return np.sin(1.3 * x + 0.4) * np.cosh(0.9 * y) + x * y

    def ux(x, y):
        return 1.3 * np.cos(1.3 * x + 0.4) * np.cosh(0.9 * y) + y

    def th(x, y):
        return 1.0 + 0.5 * np.sin(2.0 * x) * np.cos(y)

    X, Y = np.meshgrid(t, t)
    uxx = -1.69 * np.sin(1.3 * X + 0.4) * np.cosh(0.9 * Y)
    uyy = 0.81 * np.sin(1.3 * X + 0.4) * np.cosh(0.9 * Y)
    uy = 0.9 * np.sin(1.3 * X + 0.4) * np.sinh(0.9 * Y) + X
    thx, thy = np.cos(2.0 * X) * np.cos(Y), -0.5 * np.sin(2.0 * X) * np.sin(Y)
    f = th(X, Y) * (uxx + uyy) + thx * ux(X, Y) + thy * uy
    bd = np.stack([u(t, -h), u(t, 1.0 + h), u(-h, t), th(1.0 + 0.5 * h, t) * ux(1.0 + 0.5 * h, t)])
    return u(X, Y), th(X, Y), f, bd


def refinement_errors(mean="harmonic", sizes=(9, 17, 33, 65)):
    errs = []
    for n in sizes:
        ustar, th, f, bd = _analytic(n)
        u = BD.pcg(f, th, bd, mean, "dddn", rtol=1e-12)[0]
        errs.append(np.abs(u - ustar).max())
    return errs


@pytest.mark.parametrize("mean", D.MEANS)
def test_refinement_study(mean):
    """Values on three sides (the exact ghost values one h outside) and the exact flux, half a cell outside, through the
    column n - 1 side, with a smooth varying theta.  The scheme is second order: the numpy reference shows max-norm
    errors 9.6e-3, 2.7e-3, 7.4e-4, 1.9e-4 at n = 9, 17, 33, 65 and ratios 3.51, 3.72, 3.85 (arithmetic) / 3.55, 3.74,
    3.86 (harmonic) per halving of h, rising towards 4 (printed).  The floor 3.3 leaves that reference
    its own margin of 0.2 below its smallest ratio."""
    errs = refinement_errors(mean)
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    print(mean, ["%.3e" % e for e in errs], ["%.2f" % r for r in ratios])
    assert all(r >= 3.3 for r in ratios), ratios
    assert errs[-1] <= 2e-2 * np.abs(_analytic(65)[0]).max()


# ---- gradients ---------------------------------------------------------------------------------------------------------
def _apply_torch(u, th, bd, mean, bc, sigma):
    """A_bd u in torch fp64 (any order: it is differentiated, not compared bit for bit)."""
    n = u.shape[-1]
    inv_h2, inv_h = float((n - 1) ** 2), float(n - 1)
    p = torch.zeros(n + 2, n + 2, dtype=torch.float64)
    tp = torch.zeros(n + 2, n + 2, dtype=torch.float64)
    p[1:-1, 1:-1], tp[1:-1, 1:-1] = u, th
    ring = ((0, slice(1, -1)), (-1, slice(1, -1)), (slice(1, -1), 0), (slice(1, -1), -1))
    inner = ((1, slice(1, -1)), (-2, slice(1, -1)), (slice(1, -1), 1), (slice(1, -1), -2))
    y = torch.zeros(n, n, dtype=torch.float64)
    edge = ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1))
    for s in range(4):
        if bc[s] == "d":
            p[ring[s]] = bd[s]
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        tb = tp[1 + dy:n + 1 + dy, 1 + dx:n + 1 + dx]
        ub = p[1 + dy:n + 1 + dy, 1 + dx:n + 1 + dx]
        inside = tb > 0
        tb_safe = torch.where(inside, tb, th)
        c = (2.0 * th * tb_safe / (th + tb_safe)) if mean == "harmonic" else 0.5 * (th + tb_safe)
        c = torch.where(inside, c, th)
        y = y + c * (ub - u)
    # the ghost faces of the "n" sides carry nothing; their flux enters instead
    corr = torch.zeros(n, n, dtype=torch.float64)
    for s in range(4):
        if bc[s] == "n":
            m = torch.zeros(n, n, dtype=torch.float64)
            m[edge[s]] = 1.0
            corr = corr + m * (th * u * inv_h2)                     # cancel theta_a * (0 - u_a) * inv_h2
            q = torch.zeros(n, n, dtype=torch.float64)
            q[edge[s]] = bd[s]
            corr = corr + q * inv_h
    return y * inv_h2 + corr - sigma * u


@pytest.mark.parametrize("bc", ["dddd", "ddnn", "dnnd", "nnnn"])
@pytest.mark.parametrize("mean", D.MEANS)
def test_gradients_against_autograd_and_finite_differences(mean, bc):
    n, sigma = 5, 7.5
    un, thn, bdn = _case(n, 6)
    lamn = D.field_u(n, 7)
    assert np.abs(_apply_torch(torch.from_numpy(un), torch.from_numpy(thn), torch.from_numpy(bdn), mean, bc,
                               sigma).numpy() - BD.apply(un, thn, bdn, mean, bc, sigma)).max() <= 1e-11
    th = torch.from_numpy(thn).requires_grad_(True)
    bd = torch.from_numpy(bdn).requires_grad_(True)
    (torch.from_numpy(lamn) * _apply_torch(torch.from_numpy(un), th, bd, mean, bc, sigma)).sum().backward()
    g_th = BD.theta_grad(un, lamn, thn, bdn, mean, bc, scale=-1.0)      # d<lam, A u>/dtheta = -G
    g_bd = BD.bd_grad(lamn, thn, bc)
    assert np.abs(g_th - th.grad.numpy()).max() <= 1e-11 * np.abs(g_th).max()
    assert np.abs(g_bd - bd.grad.numpy()).max() <= 1e-11 * np.abs(g_bd).max()
    # finite differences of <lam, A_bd u>, central, in a few entries of each
    eps = 1e-6

    def pair(t, b):
        return np.sum(lamn * BD.apply(un, t, b, mean, bc, sigma))
    for i, j in ((0, 0), (2, 3), (4, 1), (4, 4)):
        d = np.zeros((n, n))
        d[i, j] = eps
        fd = (pair(thn + d, bdn) - pair(thn - d, bdn)) / (2 * eps)
        assert abs(fd - g_th[i, j]) <= 1e-6 * np.abs(g_th).max(), (i, j)
    for s in range(4):
        for k in (0, 2, 4):
            d = np.zeros((4, n))
            d[s, k] = eps
            fd = (pair(thn, bdn + d) - pair(thn, bdn - d)) / (2 * eps)
            assert abs(fd - g_bd[s, k]) <= 1e-6 * np.abs(g_bd).max(), (s, k)


def test_solve_gradients_by_the_adjoint():
    """u = A^-1 (f - b): with lam = A^-T w = A^-1 w, d(w.u)/dbd = -bd_grad(lam) and d(w.u)/dtheta = +G_bd(u, lam),
    against central differences of dense solves."""
    n, bc, mean, sigma = 5, "dnnd", "harmonic", 3.0
    f, th, bd = _case(n, 8)
    w = D.field_u(n, 9)
    u = BD.solve_dense(f, th, bd, mean, bc, sigma)[0]
    lam = np.linalg.solve(BC.dense(th, mean, bc, sigma), w.reshape(-1)).reshape(n, n)
    g_bd, g_th = -BD.bd_grad(lam, th, bc), BD.theta_grad(u, lam, th, bd, mean, bc)
    eps = 1e-6

    def loss(t, b):
        return np.sum(w * BD.solve_dense(f, t, b, mean, bc, sigma)[0])
    for s in range(4):
        for k in range(n):
            d = np.zeros((4, n))
            d[s, k] = eps
            assert abs((loss(th, bd + d) - loss(th, bd - d)) / (2 * eps) - g_bd[s, k]) <= 1e-6 * np.abs(g_bd).max()
    for i, j in ((0, 0), (0, 3), (2, 2), (4, 0), (3, 4)):
        d = np.zeros((n, n))
        d[i, j] = eps
        assert abs((loss(th + d, bd) - loss(th - d, bd)) / (2 * eps) - g_th[i, j]) <= 1e-6 * np.abs(g_th).max()


# ---- the smoother ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["dddd", "ddnn", "nnnn"])
def test_a_solution_is_a_fixed_point_of_the_sweep(bc):
    n, sigma = 8, 0.0
    ustar, th, bd = _case(n, 10)
    f = BD.apply(ustar, th, bd, "harmonic", bc, sigma)
    swept = BD.relax(ustar[None], f[None], th[None], bd, "harmonic", bc, float((n - 1) ** 2), 3)[0]
    assert np.abs(swept - ustar).max() <= 64 * EPS * np.abs(ustar).max() * 3
    # constants with g equal to the constant on "d" sides and q = 0 stay fixed exactly
    c = 2.5
    const = BD.relax(np.full((1, n, n), c), np.zeros((1, n, n)), th[None], np.where(
        np.array([s == "d" for s in bc])[:, None], c, 0.0) * np.ones((4, n)), "harmonic", bc, float((n - 1) ** 2), 4)
    assert np.array_equal(const, np.full((1, n, n), c))


# ---- the Python surface: every refusal, without a device -----------------------------------------------------------------
def test_bc_data_builder_refusals():
    from superresolution_for_pdes_amd import poisson as P
    with pytest.raises(ValueError, match="bc"):
        P.bc_data(5, bc="ddx", device="cpu")
    with pytest.raises(ValueError, match="n >= 2"):
        P.bc_data(1, device="cpu")
    with pytest.raises(ValueError, match="row1"):
        P.bc_data(5, row1=np.zeros(4), device="cpu")
    with pytest.raises(ValueError, match="col0"):
        P.bc_data(5, col0=np.zeros((3, 5)), B=2, device="cpu")
    with pytest.raises(ValueError, match="finite"):
        P.bc_data(5, col1=float("nan"), device="cpu")
    d = P.bc_data(5, "ddnn", row0=1.5, row1=np.arange(5.0), col0=torch.ones(2, 5, dtype=torch.float64), B=2, device="cpu")
    assert d.shape == (2, 4, 5) and d.dtype == torch.float64 and d.is_contiguous()
    assert torch.equal(d[1, 0], torch.full((5,), 1.5, dtype=torch.float64))
    assert torch.equal(d[0, 1], torch.arange(5.0, dtype=torch.float64)) and not d[:, 3].any()
    side = torch.ones(5, dtype=torch.float64, requires_grad=True)
    assert P.bc_data(5, row0=side, device="cpu").requires_grad


def test_python_refusals_need_no_device():
    from superresolution_for_pdes_amd import poisson as P
    n = 6
    u, th = D.field_u(n, 0, 2), D.field_theta(n, 0, 0.5, 2.0, 2)
    good = np.zeros((2, 4, n))
    calls = {
        "apply_div": lambda d, **kw: P.apply_div(u, th, bc_data=d, **kw),
        "solve_div": lambda d, **kw: P.solve_div(u, th, bc_data=d, **kw),
        "diffuse": lambda d, **kw: P.diffuse(u, th, dt=1e-2, bc_data=d, **kw),
        "div_theta_grad": lambda d, **kw: P.div_theta_grad(u, u, th, bc_data=d, **kw),
        "residual_metrics": lambda d, **kw: P.residual_metrics(u, u, th, form="divergence", bc_data=d, **kw),
        "relax": lambda d, **kw: P.relax(u, u, th, 2, form="divergence", bc_data=d, **kw),
    }
    bad_shape = [np.zeros((2, 4, n + 1)), np.zeros((3, 4, n)), np.zeros((2, 3, n)), np.zeros(n), np.zeros((1, 2, 4, n))]
    for name, fn in calls.items():
        for d in bad_shape:
            with pytest.raises(ValueError, match="bc_data must be"):
                fn(d)
        with pytest.raises(ValueError, match="float64"):
            fn(good.astype(np.float32))
        with pytest.raises(ValueError, match="float64"):
            fn(torch.zeros(2, 4, n, dtype=torch.float32))
        with pytest.raises(ValueError, match="tensor or an array"):
            fn([[0.0] * n] * 4)
        for v in (np.nan, np.inf):
            d = good.copy()
            d[1, 2, 3] = v
            with pytest.raises(ValueError, match="finite"):
                fn(d)
            with pytest.raises(ValueError, match="finite"):
                fn(torch.from_numpy(d))
        with pytest.raises(ValueError, match="bc"):
            fn(good, bc="ddx")
    # data with the pointwise form, data with interior_only
    with pytest.raises(ValueError, match="divergence"):
        P.relax(u, u, th, 2, bc_data=good)
    with pytest.raises(ValueError, match="divergence"):
        P.residual_metrics(u, u, th, bc_data=good)
    with pytest.raises(ValueError, match="interior_only"):
        P.relax(u, u, th, 2, form="divergence", bc_data=good, interior_only=True)
    with pytest.raises(ValueError, match="interior_only"):
        P.residual_metrics(u, u, th, form="divergence", bc_data=good, interior_only=True)
    # the singular box stays refused with data
    with pytest.raises(ValueError, match="singular"):
        P.solve_div(u, th, bc="nnnn", bc_data=good)


def test_header_declares_the_entries():
    from superresolution_for_pdes_amd import _lib
    protos = _lib.parse_header()
    for name in ("srpde_div_apply_bd", "srpde_div_step_rhs_bd", "srpde_div_cg_init_from_bd", "srpde_div_theta_grad_bd",
                 "srpde_div_bd_grad", "srpde_div_relax_bd"):
        assert name in protos, name
    cdll = _lib.lib()                                            # the built library exports them
    assert all(hasattr(cdll, name) for name in protos)
