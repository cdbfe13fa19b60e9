"""The plain CG solver (csrc/poisson.hip, srpde_poisson_cg_batched / srpde_poisson_cg_lds) at its selection edges, stop
rules, resid word, batch independence, tolerances and magnitude range, against tests/poisson_cg_ref.py (the host
restatement of its Chronopoulos-Gear recurrence, itself held to the oracle by tests/test_poisson_cg_host.py) and
oracle.poisson_ref.solve (SuperLU).

The solver is six kernels chosen by n: cg_lds_kernel<4> (n <= 24), <7> (25 .. 84 but 80), cg_lds_n_kernel<80, 960>
(n = 80, a compile-time slab layout with a ragged last slab), cg_lds_kernel<16> (85 .. 128), gcg_coop_kernel<npt>
(129 .. 1024, npt from B) and the polled gcg_* kernels above.  n = 84 is the one NPT = 7 size whose block rounds up to
1024 threads, so all 16 wave slots of the block reduction are in use.  Both LDS kernels run two iterations per loop trip
with a break between them, so maxit = 0, 1, an even and an odd count leave the loop at different places.

Bars: 1e-10 relative against a direct solve (the project's bar); 2 % + 2 on iteration counts and 1e-9 on u after equal
iterations for two roundings of one recurrence (test_cooperative_grid_cg_matches_polled's bars); bit equality wherever
the arithmetic is the same operations on the same or exactly scaled numbers.

Magnitude range: the kernels form alpha and beta from one division, 1 / (gamma D) with D ~ gamma^2, so they need
gamma^3 inside fp64's range.  cg_scalars takes the three inner products scaled by the power of two of gamma0's exponent
(exactly: alpha and beta are ratios), so the range is that of gamma itself and the solver is equivariant under power-of-
two scalings of f: 2^-200 and 2^180, where the unscaled product underflowed to 0 or overflowed (measured before the
scaling went in: NaN scalars either way, so the LDS kernels returned an all-NaN u with iters = 2 and the cooperative
kernel, whose NaN gamma never compares <= stop, an all-NaN u after all 20 n^2 iterations, neither with an error), are
solved to the bits of 2^0.  The split polled
entries (srpde_poisson_cg_grid_*, n > 1024 through the batched entry) run textbook CG with three plain divisions,
alpha = <r, r> / <p, A p> and beta = <r, r> / <r, r>_old: ratios of like quantities, no product of inner products, so
they never shared the problem and n = 1030 is not run here."""
import numpy as np
import pytest
import torch

import poisson_cg_ref as C

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
RTOL = 1e-12


def _dev(a):
    if isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()      # (a copy: the fields are read-only)


def _solve(f, theta, **kw):
    from superresolution_for_pdes_amd import poisson as P
    u, it = P.solve_batched(_dev(f), _dev(theta), return_iters=True, **kw)
    return u.cpu().numpy(), it.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _with_zero(n):
    """fields(n) with problem 1's forcing zeroed: (f, theta) [3, n, n]."""
    f, theta = C.fields(n)
    f = f.copy()
    f[1] = 0.0
    return f, theta


@pytest.mark.parametrize("n", [24, 25, 79, 80, 81, 84, 85, 127])
def test_selection_edges(n):
    """Both sides of 24 | 25 and 84 | 85, the generic kernel beside n = 80, n = 84 (16 full wave slots) and 127: B = 3
    with three theta fields, the project's forcing, a zero forcing and a standard normal one.  At n = 80 also the
    problem rotated by 180 degrees, whose ragged last slab (rows 72 .. 79) carries what the first slab carried."""
    f, theta = _with_zero(n)
    u, it = _solve(f, theta)
    assert it[1] == 0 and not u[1].any()
    for b in (0, 2):
        err, want = C.rel(u[b], C.direct(n, b)), C.reference(n, b)[1]
        print(f"n={n} b={b}: rel err vs spsolve {err:.2e} (bar 1e-10), iters {it[b]} vs host {want} (bar 2% + 2, "
              f"< {10 * n})")
        assert err <= 1e-10
        assert C.iters_close(it[b], want) and it[b] < 10 * n
    if n == 80:
        ur, itr = _solve(f[:, ::-1, ::-1], theta[:, ::-1, ::-1])
        assert itr[1] == 0 and not ur[1].any()
        for b in (0, 2):
            err = C.rel(ur[b, ::-1, ::-1], u[b])
            print(f"n=80 b={b}: rotated problem, rotated back, vs the unrotated u {err:.2e} (bar 1e-10), iters {itr[b]}")
            assert err <= 1e-10
            assert C.iters_close(itr[b], it[b])


@pytest.mark.parametrize("n", [20, 40, 80, 100])
def test_maxit_on_the_lds_path(n):
    """One size per LDS kernel; maxit = 0 (the loop is not entered), 1 (out at the break), 2 (out at the loop
    condition), 3 and 37 (an odd count after full trips): exactly maxit iterations, and the host recurrence's u after
    as many."""
    f, theta = C.fields(n)
    for b in (0, 2):
        full = C.reference(n, b)[1]
        assert full > 37, (n, b, full)        # not vacuous: nothing here converges within 37 iterations
    for maxit in (0, 1, 2, 3, 37):
        u, it = _solve(f, theta, maxit=maxit)
        assert it.tolist() == [maxit] * 3, (maxit, it)
        if maxit == 0:
            assert not u.any()
            continue
        for b in (0, 2):
            want, itw, _, _ = C.reference(n, b, maxit=maxit)
            assert itw == maxit
            err = C.rel(u[b], want)
            print(f"n={n} b={b} maxit={maxit}: iters {it[b]}, u vs host after as many {err:.2e} (bar 1e-9)")
            assert err <= 1e-9


def _cg_lds(f, theta, rtol, maxit):
    """srpde_poisson_cg_lds with iters and resid buffers -> (u, iters, resid) as numpy."""
    from superresolution_for_pdes_amd._lib import call, stream_ptr
    f, theta = _dev(f), _dev(theta)
    B, n, _ = f.shape
    u = torch.empty_like(f)
    iters = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    resid = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    call("srpde_poisson_cg_lds", f.data_ptr(), theta.data_ptr(), u.data_ptr(), B, n, float(rtol), int(maxit),
         iters.data_ptr(), resid.data_ptr(), stream_ptr())
    return u.cpu().numpy(), iters.cpu().numpy(), resid.cpu().numpy()


@pytest.mark.parametrize("n", [20, 40, 80, 100])
def test_resid_word(n):
    """resid = sqrt(gamma / gamma0) of the recurrence's residual.  Stopped at 37 iterations it is the true residual of
    the returned u to 1e-6 relative (the two drift apart by about k eps kappa = 37 x 2e-16 x 4e3, against a residual
    of 1e-4 or more there); converged, it is <= rtol and the true residual <= 2 rtol + eps kappa, kappa =
    4 (n - 1)^2 / (2 pi^2); zero forcing gives resid 0 after 0 iterations."""
    f, theta = _with_zero(n)
    u, it, resid = _cg_lds(f, theta, RTOL, 37)
    assert it.tolist() == [37, 0, 37] and resid[1] == 0.0 and not u[1].any()
    for b in (0, 2):
        true = C.true_resid(u[b], f[b], theta[b])
        print(f"n={n} b={b} maxit=37: resid {resid[b]:.6e}, true {true:.6e}, rel diff {abs(resid[b] - true) / true:.2e} "
              f"(bar 1e-6), host {C.reference(n, b, maxit=37)[2]:.6e}")
        assert 1e-5 < true < 1.0
        assert abs(resid[b] - true) <= 1e-6 * true
    u, it, resid = _cg_lds(f, theta, RTOL, 20 * n * n)
    assert it[1] == 0 and resid[1] == 0.0 and not u[1].any()
    bar = 2 * RTOL + EPS * C.kappa(n)
    for b in (0, 2):
        true = C.true_resid(u[b], f[b], theta[b])
        print(f"n={n} b={b} converged: iters {it[b]}, resid {resid[b]:.3e} (bar {RTOL:g}), true {true:.3e} "
              f"(bar {bar:.3e}, kappa {C.kappa(n):.0f})")
        assert 0 < it[b] < 10 * n
        assert 0.0 < resid[b] <= RTOL
        assert true <= bar


def test_cg_lds_refuses_bad_arguments():
    """Null pointers, n = 1, n = 129 (above srpde_poisson_lds_max_n) and B = 0: a negative code, _lib.call raises, and
    u keeps its bytes."""
    from superresolution_for_pdes_amd._lib import call, query, stream_ptr
    assert int(query("srpde_poisson_lds_max_n")) == 128
    B, n = 2, 20
    f = torch.ones(B, 129, 129, dtype=torch.float64, device="cuda")
    theta = torch.ones_like(f)
    u = torch.full_like(f, -12345.678)
    before = u.clone()
    iters = torch.zeros(B, dtype=torch.int32, device="cuda")
    resid = torch.zeros(B, dtype=torch.float64, device="cuda")
    good = [f.data_ptr(), theta.data_ptr(), u.data_ptr(), B, n, RTOL, 100, iters.data_ptr(), resid.data_ptr(),
            stream_ptr()]
    bad = {"f null": {0: None}, "theta null": {1: None}, "u null": {2: None}, "B = 0": {3: 0}, "n = 1": {4: 1},
           "n = 129": {4: 129}}
    for name, change in bad.items():
        args = [change.get(i, a) for i, a in enumerate(good)]
        rc = query("srpde_poisson_cg_lds", *args)
        print(f"{name}: rc {rc}")
        assert rc < 0, name
        with pytest.raises(RuntimeError, match="srpde_poisson_cg_lds"):
            call("srpde_poisson_cg_lds", *args)
    torch.cuda.synchronize()
    assert torch.equal(u.view(torch.int64), before.view(torch.int64))
    assert query("srpde_poisson_cg_lds", *good) == 0      # the same buffers, unchanged arguments: accepted
    torch.cuda.synchronize()
    assert not torch.equal(u[:, :n, :n], before[:, :n, :n])


@pytest.mark.parametrize("n", [25, 80, 85])
def test_lds_batch_independence_and_determinism(n):
    """One workgroup per problem and nothing shared: a problem solved alone, as member 0 and as the last member of
    B = 5, and in a second identical call, gives the same bits of u and the same iteration count."""
    f, theta = C.fields(n, 5)
    order = {"alone": [3], "first of 5": [3, 0, 1, 2, 4], "last of 5": [0, 1, 2, 4, 3], "last of 5 again": [0, 1, 2, 4, 3]}
    got = {}
    for name, idx in order.items():
        u, it = _solve(f[idx], theta[idx])
        at = idx.index(3)
        got[name] = (_bits(u[at]), int(it[at]), _bits(u), it)
    want_u, want_it = got["alone"][:2]
    for name, (ub, it, _, _) in got.items():
        print(f"n={n} {name}: iters {it}, {int((ub != want_u).sum())} of {ub.size} values differ from alone")
        assert it == want_it and np.array_equal(ub, want_u), name
    assert np.array_equal(got["last of 5"][2], got["last of 5 again"][2])
    assert np.array_equal(got["last of 5"][3], got["last of 5 again"][3])
    assert C.iters_close(want_it, C.reference(n, 3, 5)[1])


def test_cooperative_batch_independence_and_determinism():
    """n = 129, the smallest cooperative size.  The block size depends on B by design, so bits may differ between batch
    sizes: the same problem alone, last of 3 and last of srpde_poisson_coop_problems(129) + 1 (in the second launch
    group) agrees to 1e-10 with iteration counts within 2 % + 2, and two identical calls agree bit for bit."""
    from superresolution_for_pdes_amd._lib import query
    n = 129
    per = int(query("srpde_poisson_coop_problems", n))
    assert per >= 1
    f, theta = C.fields(n, 5)
    got = {}
    for B in (1, 3, per + 1):
        idx = [b % 3 for b in range(B - 1)] + [3]
        fb, tb = _dev(f[idx]), _dev(theta[idx])
        u, it = _solve(fb, tb)
        u2, it2 = _solve(fb, tb)
        same = np.array_equal(_bits(u), _bits(u2)) and np.array_equal(it, it2)
        print(f"n={n} B={B}: iters of the problem {it[-1]}, a second call equal bit for bit: {same}")
        assert same
        got[B] = (u[-1], int(it[-1]))
    want_u, want_it = got[1]
    err = C.rel(want_u, C.direct(n, 3, 5))
    print(f"n={n} alone: rel err vs spsolve {err:.2e} (bar 1e-10), iters {want_it} vs host {C.reference(n, 3, 5)[1]}")
    assert err <= 1e-10 and C.iters_close(want_it, C.reference(n, 3, 5)[1])
    for B in (3, per + 1):
        err = C.rel(got[B][0], want_u)
        print(f"n={n} B={B} vs alone: {err:.2e} (bar 1e-10), iters {got[B][1]} vs {want_it} (bar 2% + 2)")
        assert err <= 1e-10 and C.iters_close(got[B][1], want_it)


def test_tolerance_and_wide_theta():
    """n = 40 with theta = 2^U(-6, 6): theta enters only through r = -f / theta, and over twelve binary orders a mean
    or a reciprocal taken once per problem would show.  rtol = 1e-4, 1e-8, 1e-12: the true residual is within 2 rtol,
    the count grows with every tightening and stays within 2 % + 2 of the host recurrence's."""
    n = 40
    f, theta = C.fields(n, 3, 0, True)
    assert theta.min() < 2.0 ** -5 and theta.max() > 2.0 ** 5
    counts = []
    for rtol in (1e-4, 1e-8, 1e-12):
        u, it = _solve(f, theta, rtol=rtol)
        counts.append(it)
        for b in range(3):
            true, want = C.true_resid(u[b], f[b], theta[b]), C.reference(n, b, 3, 0, True, rtol)[1]
            print(f"n={n} b={b} rtol={rtol:g}: true resid {true:.3e} (bar {2 * rtol:g}), iters {it[b]} vs host {want} "
                  f"(bar 2% + 2)")
            assert true <= 2 * rtol
            assert C.iters_close(it[b], want)
    assert (counts[0] < counts[1]).all() and (counts[1] < counts[2]).all(), counts


_unscaled = {}


def _scale_case(n):
    """(f, theta) [2, n, n] (the project's forcing and a standard normal one) and their k = 0 solve, once per n."""
    f, theta = C.fields(n)
    f, theta = f[[0, 2]], theta[[0, 2]]
    if n not in _unscaled:
        _unscaled[n] = _solve(f, theta)
    return (f, theta) + _unscaled[n]


SCALE_SIZES = [25, 80, 100, 129]     # cg_lds_kernel<7>, cg_lds_n_kernel, cg_lds_kernel<16>, gcg_coop_kernel


@pytest.mark.parametrize("n", SCALE_SIZES)
def test_power_of_two_scaling_in_range(n):
    """solve(2^k f) == 2^k solve(f) bit for bit with equal iteration counts for k = +-30, +-100: every operation of the
    recurrence scales exactly under a power of two while nothing leaves range.  With |f| = O(1), gamma runs from about
    2^(2k + 30) down to 2^(2k + 30 - 80), and the extreme cubes, 2^690 and 2^-750, are inside 2^+-1022 even
    unscaled."""
    f, theta, u0, it0 = _scale_case(n)
    for k in (-100, -30, 30, 100):
        u, it = _solve(np.ldexp(f, k), theta)
        differ = int((_bits(u) != _bits(np.ldexp(u0, k))).sum())
        print(f"n={n} k={k}: iters {it.tolist()} vs {it0.tolist()}, {differ} of {u.size} values differ from 2^k u")
        assert np.array_equal(it, it0)
        assert differ == 0


@pytest.mark.parametrize("k", [-200, 180])
@pytest.mark.parametrize("n", SCALE_SIZES)
def test_power_of_two_scaling_past_the_cube_range(n, k):
    """k = -200: gamma ~ 2^-370 and gamma D ~ 2^-1110 underflows unscaled; k = 180: gamma ~ 2^390 and gamma D ~ 2^1170
    overflows.  gamma, delta and u themselves are far inside the range, so the solve must either return a finite u that
    is 2^k times the k = 0 solution to 1e-10 or raise; never NaN / inf or an unconverged u."""
    f, theta, u0, it0 = _scale_case(n)
    try:
        u, it = _solve(np.ldexp(f, k), theta)
    except (RuntimeError, ValueError) as e:
        print(f"n={n} k={k}: refused: {e}")
        assert "solve_batched" in str(e) or "srpde_poisson" in str(e)
        return
    finite = bool(np.isfinite(u).all())
    back = np.ldexp(u, -k)
    err = [C.rel(back[b], u0[b]) if finite else float("nan") for b in range(2)]
    differ = int((_bits(back) != _bits(u0)).sum())
    print(f"n={n} k={k}: finite {finite}, iters {it.tolist()} vs {it0.tolist()}, 2^-k u vs the k = 0 solve {err} "
          f"(bar 1e-10), {differ} of {u.size} values differ")
    assert finite
    assert max(err) <= 1e-10
    assert all(C.iters_close(a, b) for a, b in zip(it, it0))
