"""CPU: the mathematics the zero-flux sides rest on (ABI 22), checked in numpy before any kernel relies on it -- the
closed-form 1-D eigen-decompositions, the symmetry and definiteness of the operator for all 16 patterns, the separable
solve, the condition bound theta_max / theta_min and CG's iteration bound, the insulated box's conservation bound, and
the "dddd" restatement against the existing ones bit for bit."""
import numpy as np
import pytest

import diffuse_ref as R
import div_adjoint_ref as A
import div_bc_ref as BC
import poisson_div_ref as D

SIDES = [("d", "d"), ("d", "n"), ("n", "d"), ("n", "n")]


@pytest.mark.parametrize("lo,hi", SIDES)
@pytest.mark.parametrize("n", [2, 3, 5, 16, 33])
def test_closed_form_eigen_decompositions(n, lo, hi):
    T = BC.tridiag(n, lo, hi)
    Q, lam = BC.eig1d(n, lo, hi)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-13
    assert np.abs(T @ Q - Q * lam[None, :]).max() <= 1e-13
    want = np.linalg.eigh(T)[0]
    assert np.abs(np.sort(lam) - want).max() <= 1e-13
    if (lo, hi) == ("n", "n"):
        assert lam[0] == 0.0 and np.abs(Q[:, 0] - 1.0 / np.sqrt(n)).max() <= 1e-15      # the constant mode
    else:
        assert lam.max() < 0.0


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 12])
def test_operator_is_symmetric_and_definite_for_every_pattern(n, mean):
    th = D.field_theta(n, 0, 0.5, 2.0)
    for bc in BC.PATTERNS:
        M = BC.dense(th, mean, bc)
        assert np.array_equal(M, M.T), bc
        w = np.linalg.eigvalsh(M)
        scale = np.abs(w).max()
        if bc == "nnnn":
            assert w[-2] < -1e-10 * scale and abs(w[-1]) <= 1e-12 * scale      # exactly one null vector ...
            assert np.abs(M @ np.ones(n * n)).max() <= 1e-12 * scale           # ... the constants
        else:
            assert w[-1] < -1e-10 * scale, bc


@pytest.mark.parametrize("n", [5, 12])
def test_separable_solve_matches_a_dense_solve(n):
    r = D.field_u(n, 3)
    ones = np.ones((n, n))
    for bc in BC.PATTERNS:
        for sigma_p in (0.0, 10.0, 1e4):
            if bc == "nnnn" and sigma_p == 0.0:
                continue
            want = np.linalg.solve(BC.dense(ones, "arithmetic", bc, sigma_p), r.reshape(-1)).reshape(n, n)
            got = BC.sep_solve(r, bc, sigma_p)
            assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want), (bc, sigma_p)


@pytest.mark.parametrize("lo,hi", [(0.5, 2.0), (0.1, 10.0)])
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 12])
def test_generalised_eigenvalues_lie_in_thetas_range(n, mean, lo, hi):
    """A = -D_theta + sigma I and M = -L_bc + sigma_p I, sigma_p = sigma / theta_g: eig(M^-1 A) in [theta_min,
    theta_max], so cond <= theta_max / theta_min for every n, sigma and pattern."""
    from scipy.linalg import eigh
    th = D.field_theta(n, 1, lo, hi)
    ones = np.ones((n, n))
    for bc in BC.PATTERNS:
        for sigma in (0.0, 10.0, 1e4):
            if bc == "nnnn" and sigma == 0.0:
                continue
            Am = -BC.dense(th, mean, bc, sigma)
            Mm = -BC.dense(ones, "arithmetic", bc, R.precond_shift(th, sigma))
            w = eigh(Am, Mm, eigvals_only=True)
            assert w[0] >= th.min() * (1.0 - 1e-9) and w[-1] <= th.max() * (1.0 + 1e-9), (bc, sigma, w[0], w[-1])


@pytest.mark.parametrize("lo,hi", [(0.5, 2.0), (0.1, 10.0)])
@pytest.mark.parametrize("mean", D.MEANS)
def test_pcg_count_stays_within_the_bound(mean, lo, hi):
    n, tol = 12, 1e-12
    th, f = D.field_theta(n, 2, lo, hi), D.forcing(n)
    bound = D.chebyshev_iterations(lo, hi, tol)
    for bc in ("nddd", "ddnd", "dnnd", "ddnn", "ndnn", "nnnn"):
        for sigma in (0.0, 10.0, 1e4):
            if bc == "nnnn" and sigma == 0.0:
                continue
            u, k, resid = BC.pcg(f, th, mean, bc, sigma, rtol=tol)
            assert resid <= tol and k <= bound, (bc, sigma, k, bound)
            want = np.linalg.solve(BC.dense(th, mean, bc, sigma), f.reshape(-1)).reshape(n, n)
            assert np.linalg.norm(u - want) <= 1e-8 * np.linalg.norm(want)


@pytest.mark.parametrize("mean", D.MEANS)
def test_dddd_restatement_is_the_existing_one_bit_for_bit(mean):
    n, B = 13, 2
    u, lam, f = D.field_u(n, 0, B), D.field_u(n, 1, B), D.field_u(n, 2, B)
    th = D.field_theta(n, 0, 0.1, 10.0, B)
    assert np.array_equal(BC.apply(u, th, mean, "dddd"), D.apply(u, th, mean))
    assert np.array_equal(BC.apply(u, th, mean, "dddd", inv_h2=77.5), D.apply(u, th, mean, 77.5))
    for sigma in (7.5, 1e6):
        assert np.array_equal(BC.apply(u, th, mean, "dddd", sigma), R.apply_shift(u, th, mean, sigma))
        for scheme in ("be", "cn"):
            assert np.array_equal(BC.step_rhs(u, f, th, mean, sigma, scheme, "dddd"),
                                  R.step_rhs(u, f, th, mean, sigma, scheme))
    assert np.array_equal(BC.theta_grad(u, lam, th, mean, "dddd", scale=-1.0), A.theta_grad(u, lam, th, mean, scale=-1.0))
    assert np.array_equal(BC.dense(th[0], mean, "dddd", 7.5), R.dense_shift(th[0], mean, 7.5))
    # the d-d axis is the existing sine plan; the solve agrees to rounding (the products run in another order)
    S, lam1 = D.sine_plan(n)
    Q, lq = BC.eig1d(n, "d", "d")
    # (sine_plan does not reduce its argument, up to pi n: an argument rounding of pi n eps / 2 on each of its two
    # operations, and the two sines' own half-ulps, stay under 2 pi n eps)
    eps = np.finfo(np.float64).eps
    assert np.abs(Q - S).max() <= 2.0 * np.pi * n * eps and np.abs(lq - lam1).max() <= 8.0 * eps
    got, want = BC.sep_solve(f[0], "dddd", 10.0), R.sine_solve_shift(f[0], 10.0)
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)


def test_every_pattern_differs_from_dddd_only_at_its_sides():
    n = 9
    u, th = D.field_u(n, 4), D.field_theta(n, 4, 0.5, 2.0)
    base = D.apply(u, th, "harmonic")
    for bc in BC.PATTERNS:
        diff = BC.apply(u, th, "harmonic", bc) != base
        edge = np.zeros((n, n), dtype=bool)
        for side, sl in zip(bc, ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1))):
            if side == "n":
                edge[sl] = True
        assert not (diff & ~edge).any() and diff[edge].all(), bc


def test_insulated_box_reference_conserves_within_the_bound():
    """The numpy PCG alone stays inside the conservation bound the GPU test asserts, and the range of u shrinks."""
    n, dt, rtol = BC.BOX_N, BC.BOX_DT, BC.BOX_RTOL
    u, th = BC.box_case()
    sigma = 1.0 / dt
    sigma_p = R.precond_shift(th, sigma)
    for _ in range(BC.BOX_STEPS):
        rhs = BC.step_rhs(u, None, th, "harmonic", sigma, "be", "nnnn")
        new, k, resid = BC.pcg(rhs, th, "harmonic", "nnnn", sigma, sigma_p, rtol=rtol, u0=u)
        assert resid <= rtol
        assert abs(new.sum() - u.sum()) <= BC.conservation_bound(n, rtol, rhs, sigma, u)
        assert new.max() - new.min() < u.max() - u.min()
        u = new


def test_mixed_wall_mode_decay_reference():
    n, dt = 17, 1e-3
    v, mu = BC.eigenmode(n, "ddnn", 1, 2)
    assert mu < 0.0
    got = BC.diffuse_dense(v, np.ones((n, n)), None, dt, 3, "be", "arithmetic", "ddnn")
    assert np.abs(got - v / (1.0 - dt * mu) ** 3).max() <= 1e-12 * np.abs(v).max()


def test_host_queries_and_mask_order():
    """The size queries of ABI 22 answer without a GPU; a plan's size names its n and its mask."""
    from superresolution_for_pdes_amd import _lib, poisson as P
    q = _lib.query
    assert q("srpde_version") >= 22
    sizes = {(n, m): q("srpde_poisson_sep_plan_size", n, m) for n in (2, 5, 64, 65) for m in range(16)}
    assert all(v >= (4 * n * n + 2 * n + 1) * 8 for (n, m), v in sizes.items())
    assert len(set(sizes.values())) == len(sizes)
    for bad in ((1, 0), (5, -1), (5, 16), (16385, 0)):
        assert q("srpde_poisson_sep_plan_size", *bad) == 0
    assert q("srpde_poisson_sep_workspace_size", 3, 40) == 3 * 40 * 40 * 8
    assert q("srpde_poisson_sep_workspace_size", 0, 40) == 0
    lds_max = q("srpde_poisson_dst_lds_max_n")
    for n in (40, lds_max, lds_max + 1):
        base = q("srpde_div_cg_workspace_size", 3, n)
        extra = 3 * n * n * 8 if n <= lds_max else 0
        assert q("srpde_div_cg_workspace_size_bc", 3, n) == base + extra
    assert q("srpde_div_cg_workspace_size_bc", 3, 1) == 0
    assert P.check_bc(None) is None and P.check_bc("dddd") is None
    for bc in BC.PATTERNS[1:]:
        assert P.check_bc(bc) == BC.mask(bc)
    assert P.check_bc("nddd") == 1 and P.check_bc("dddn") == 8
    for bad in ("", "ddd", "ddddd", "ddxd", "DDNN", 5, ("d", "d", "n", "n")):
        with pytest.raises(ValueError, match="bc"):
            P.check_bc(bad)
