"""tests/poisson_cg_ref.py, the host restatement of the plain CG solver's Chronopoulos-Gear recurrence, held to the
project's references before tests/test_gpu_poisson_cg.py leans on it (CPU only):

* against oracle.poisson_ref.solve (SuperLU on diag(theta) @ L) to 1e-10 relative, the project's bar for a solve;
* its iteration count against oracle.poisson_ref.cg (textbook CG, the same Krylov iterates in exact arithmetic) within
  2 % + 2, the bar test_cooperative_grid_cg_matches_polled uses for the two recurrences;
* exact equivariance under a power-of-two scaling of f, 2^+-100: gamma0 ~ n^2 2^+-200 and every product of the three
  plain divisions stay far inside fp64's range, so not one bit may move.

n = 5 is a grid with one interior ring, 24 | 25 the first selection edge of the LDS kernels, 33 an odd size."""
import numpy as np
import pytest

import poisson_cg_ref as C
from oracle import poisson_ref as R

SIZES = [5, 24, 25, 33]


@pytest.mark.parametrize("n", SIZES)
def test_cg_cg_matches_the_direct_solve_and_textbook_cg(n):
    f, theta = C.fields(n)
    for b in range(f.shape[0]):
        u, it, resid, hist = C.reference(n, b)
        err = C.rel(u, C.direct(n, b))
        _, it_ref = R.cg(f[b], theta[b], rtol=1e-12)
        true = C.true_resid(u, f[b], theta[b])
        print(f"n={n} b={b}: rel err vs spsolve {err:.2e} (bar 1e-10), iters {it} vs textbook {it_ref} "
              f"(bar 2% + 2), resid {resid:.2e}, true resid {true:.2e}")
        assert err <= 1e-10
        assert C.iters_close(it, it_ref), (it, it_ref)
        assert 0 < it < 10 * n and len(hist) == it + 1
        assert resid <= 1e-12 and resid == np.sqrt(hist[-1] / hist[0])
        assert true <= 2e-12 + np.finfo(np.float64).eps * C.kappa(n)


@pytest.mark.parametrize("n", SIZES)
def test_cg_cg_stops_at_maxit_and_at_zero_forcing(n):
    f, theta = C.fields(n)
    full = C.reference(n, 1)[1]
    for maxit in (0, 1, 2, 3):
        u, it, resid, hist = C.cg_cg(f[1], theta[1], 1e-12, maxit)
        assert it == maxit < full and len(hist) == maxit + 1
        assert (maxit == 0) == (not u.any())
        if maxit == 0:
            assert resid == 1.0
    u, it, resid, hist = C.cg_cg(np.zeros((n, n)), theta[0])
    assert it == 0 and resid == 0.0 and not u.any() and hist == [0.0]


@pytest.mark.parametrize("k", [-100, 100])
@pytest.mark.parametrize("n", SIZES)
def test_cg_cg_is_equivariant_under_powers_of_two(n, k):
    f, theta = C.fields(n)
    for b in (0, 1):
        u, it, resid, hist = C.reference(n, b)
        us, its, resids, hists = C.cg_cg(np.ldexp(f[b], k), theta[b])
        assert its == it and resids == resid
        assert np.array_equal(us, np.ldexp(u, k))
        assert hists == [float(np.ldexp(g, 2 * k)) for g in hist]
