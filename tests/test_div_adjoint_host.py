"""CPU: the numpy restatement of the pair gradient G and of the warm-started PCG (tests/div_adjoint_ref.py), the
references of tests/test_gpu_div_adjoint.py, checked against finite differences and against poisson_div_ref.pcg."""
import numpy as np
import pytest

import div_adjoint_ref as A
import poisson_div_ref as D

FD_STEP = 1e-6
# Central differences at a step of 1e-6 deviated from G by 6e-10 (operator) and 2e-9 (solve) when the derivation was
# checked at n = 7; 1e-7 leaves a factor of 50.
FD_RTOL = 1e-7


def _central(fun, theta):
    g = np.zeros_like(theta)
    for i in range(theta.shape[0]):
        for j in range(theta.shape[1]):
            tp, tm = theta.copy(), theta.copy()
            tp[i, j] += FD_STEP
            tm[i, j] -= FD_STEP
            g[i, j] = (fun(tp) - fun(tm)) / (2.0 * FD_STEP)
    return g


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 7])
def test_pair_gradient_against_finite_differences_of_the_operator(n, mean):
    u, w = D.field_u(n, 0), D.field_u(n, 1)
    th = D.field_theta(n, 0, 0.5, 2.0)
    fd = _central(lambda t: np.sum(w * D.apply(u, t, mean)), th)
    dev = _rel(-A.theta_grad(u, w, th, mean), fd)
    print(f"operator n={n} {mean}: relative deviation {dev:.2e}")
    assert dev <= FD_RTOL
    # scale and inv_h2 are plain factors, the sign flip is exact
    assert np.array_equal(A.theta_grad(u, w, th, mean, scale=-1.0), -A.theta_grad(u, w, th, mean))
    assert _rel(A.theta_grad(u, w, th, mean, inv_h2=3.0), A.theta_grad(u, w, th, mean) * (3.0 / (n - 1) ** 2)) < 1e-15
    # and grad_u = D w (symmetry)
    assert abs(np.sum(w * D.apply(u, th, mean)) - np.sum(u * D.apply(w, th, mean))) <= 1e-12 * (n - 1) ** 2 * n * n


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 7])
def test_pair_gradient_against_finite_differences_of_the_solve(n, mean):
    f, w = D.forcing(n), D.field_u(n, 2)
    th = D.field_theta(n, 1, 0.5, 2.0)
    u, lam = D.solve_dense(f, th, mean), D.solve_dense(w, th, mean)
    fd = _central(lambda t: np.sum(w * D.solve_dense(f, t, mean)), th)
    dev = _rel(A.theta_grad(u, lam, th, mean), fd)
    print(f"solve n={n} {mean}: relative deviation {dev:.2e}")
    assert dev <= FD_RTOL
    # grad_f = lam: the solve is linear in f
    g = D.field_u(n, 3)
    assert abs(np.sum(w * D.solve_dense(g, th, mean)) - np.sum(lam * g)) <= 1e-12 * np.linalg.norm(lam) * np.linalg.norm(g)


def test_ghost_faces_and_batching():
    """n = 2: every node has two ghost faces (d = 1, the value beyond is 0); a batch is its problems."""
    u, lam = D.field_u(2, 0, 3), D.field_u(2, 1, 3)
    th = D.field_theta(2, 0, 0.5, 2.0, 3)
    for mean in D.MEANS:
        g = A.theta_grad(u, lam, th, mean)
        for b in range(3):
            assert np.array_equal(g[b], A.theta_grad(u[b], lam[b], th[b], mean))
        d = A.dface(th[0, 0, 0], th[0, 0, 1], mean)
        tE = (d * (u[0, 0, 1] - u[0, 0, 0])) * (lam[0, 0, 1] - lam[0, 0, 0])
        tW = (1.0 * (0.0 - u[0, 0, 0])) * (0.0 - lam[0, 0, 0])
        d = A.dface(th[0, 0, 0], th[0, 1, 0], mean)
        tS = (d * (u[0, 1, 0] - u[0, 0, 0])) * (lam[0, 1, 0] - lam[0, 0, 0])
        assert g[0, 0, 0] == ((tE + tW) + (tS + tW)) * 1.0


# ---- the warm-started PCG -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_zero_start_reproduces_pcg(mean):
    n = 20
    f, th = D.forcing(n), D.field_theta(n, 0, 0.5, 2.0)
    want = D.pcg(f, th, mean)
    for x0 in (None, np.zeros((n, n))):
        got = A.pcg_from(f, th, mean, x0=x0)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    assert A.pcg_from(np.zeros((n, n)), th, mean, x0=D.field_u(n, 0))[1:] == (0, 0.0)


@pytest.mark.parametrize("mean", D.MEANS)
def test_exact_start_costs_no_iteration(mean):
    n = 20
    f, th = D.forcing(n), D.field_theta(n, 0, 0.5, 2.0)
    x0 = D.solve_dense(f, th, mean)
    u, k, resid = A.pcg_from(f, th, mean, rtol=1e-10, x0=x0)
    assert k == 0 and resid <= 1e-10 and np.array_equal(u, x0)


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("seed", A.WARM_SEEDS)
def test_nearby_start_saves_iterations(seed, mean):
    f, th, near = A.warm_case(seed)
    x0, _, _ = D.pcg(f, near, mean, rtol=A.WARM_RTOL)
    _, k_zero, _ = D.pcg(f, th, mean, rtol=A.WARM_RTOL)
    u, k_warm, resid = A.pcg_from(f, th, mean, rtol=A.WARM_RTOL, x0=x0)
    print(f"{mean}: zero start {k_zero} iterations, warm start {k_warm}")
    assert 0 < k_warm < k_zero and resid <= A.WARM_RTOL
