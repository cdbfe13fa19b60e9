"""GPU: boundary values and prescribed fluxes for the divergence-form operator and its solver (csrc/poisson_div.hip,
ABI 23, extended): apply, shifted apply, Crank-Nicolson's right-hand side, the pair gradient and the data gradient against the
numpy restatement of tests/div_bd_ref.py bit for bit; the CG with the stop rule on |f - b| against sparse direct solves
and numpy's iteration counts, Laplace's equation, batch independence, the warm start, graph capture; poisson.diffuse
towards its stationary state and its balance of sums; autograd; and the raw entries' argument checks.  bc_data=None must
give today's bits everywhere."""
import functools

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import eigsh, splu

import diffuse_ref as R
import div_bc_ref as BC
import div_bd_ref as BD
import poisson_div_ref as D

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forcings(n, B):
    return np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)])


# ---- 1. the operator, the step's right-hand side and both gradients, bit for bit ---------------------------------------
# 2: every node a corner; 5: one tile; 63 / 64 / 65: the 64-column tile edge (and two 32-row tiles); 70: ragged last tiles
# in both directions.  Data shows at edge nodes only, so whole fields are compared exactly.
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [2, 5, 63, 64, 65, 70])
def test_fields_are_bit_equal_to_the_host_restatement(n, mean):
    from superresolution_for_pdes_amd import _lib, poisson as P
    B, code = 2, D.MEANS.index(mean)
    un, ln, fn = D.field_u(n, 0, B), D.field_u(n, 1, B), D.field_u(n, 2, B)
    thn = D.field_theta(n, 0, 0.1, 10.0, B)
    u, f, th, lam = _dev(un), _dev(fn), _dev(thn), _dev(ln)
    for bc in BD.PATTERNS:
        pat, mask = BD.pattern(bc), BC.mask(BD.pattern(bc))
        for bdn in (BD.data(n, 3, B), BD.data(n, 4)[None]):              # Bd = B and Bd = 1
            bd = _dev(bdn)
            stride = 4 * n if bdn.shape[0] == B else 0
            got = P.apply_div(u, th, face_mean=mean, bc=bc, bc_data=bd)
            assert got.dtype == torch.float64 and got.shape == (B, n, n)
            assert np.array_equal(got.cpu().numpy(), BD.apply(un, thn, bdn, mean, pat)), bc
            got = P.apply_div(u, th, face_mean=mean, shift=7.5, bc=bc, bc_data=bd)
            assert np.array_equal(got.cpu().numpy(), BD.apply(un, thn, bdn, mean, pat, 7.5)), bc
            got = P.apply_div(u, th[1], face_mean=mean, inv_h2=1234.5, shift=1e6, bc=bc, bc_data=bd)
            assert np.array_equal(got.cpu().numpy(), BD.apply(un, thn[1], bdn, mean, pat, 1e6, inv_h2=1234.5)), bc
            for cn, scheme in enumerate(("be", "cn")):
                for fp, fh in ((f.data_ptr(), fn), (0, None)):
                    rhs = torch.empty_like(u)
                    _lib.call("srpde_div_step_rhs_bd", u.data_ptr(), fp, th.data_ptr(), rhs.data_ptr(), B, n, code, 7.5,
                              cn, mask, bd.data_ptr(), stride, _lib.stream_ptr())
                    want = BD.step_rhs(un, fh, thn, bdn, mean, 7.5, scheme, pat)
                    assert np.array_equal(rhs.cpu().numpy(), want), (bc, scheme)
            got = P.div_theta_grad(u, ln, th, face_mean=mean, scale=-1.0, bc=bc, bc_data=bd)
            assert np.array_equal(got.cpu().numpy(), BD.theta_grad(un, ln, thn, bdn, mean, pat, scale=-1.0)), bc
        out = torch.empty(B, 4, n, dtype=torch.float64, device="cuda")
        for inv_h2 in (float((n - 1) ** 2), 1234.5):
            _lib.call("srpde_div_bd_grad", lam.data_ptr(), th.data_ptr(), out.data_ptr(), B, n, inv_h2, mask,
                      _lib.stream_ptr())
            assert np.array_equal(out.cpu().numpy(), BD.bd_grad(ln, thn, pat, inv_h2)), bc


# ---- 2. zero data is the homogeneous operator; no data is today's call -------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_zero_data_and_no_data(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 70, 2
    u, lam, f = _dev(D.field_u(n, 0, B)), _dev(D.field_u(n, 1, B)), _dev(_forcings(n, B))
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B))
    zero = P.bc_data(n, B=1)
    assert zero.shape == (1, 4, n) and not bool(zero.any())
    for bc in BD.PATTERNS:
        for kw in ({}, {"shift": 7.5}):
            # equal as numbers: an all-zero sum may differ in the sign of its zero
            assert torch.equal(P.apply_div(u, th, face_mean=mean, bc=bc, bc_data=zero, **kw),
                               P.apply_div(u, th, face_mean=mean, bc=bc, **kw)), bc
            assert torch.equal(P.apply_div(u, th, face_mean=mean, bc=bc, bc_data=None, **kw),
                               P.apply_div(u, th, face_mean=mean, bc=bc, **kw))
        assert torch.equal(P.div_theta_grad(u, lam, th, face_mean=mean, bc=bc, bc_data=zero),
                           P.div_theta_grad(u, lam, th, face_mean=mean, bc=bc))
        kw = {"shift": 1e3} if bc == "nnnn" else {}
        want = P.solve_div(f, th, face_mean=mean, return_info=True, bc=bc, **kw)
        got = P.solve_div(f, th, face_mean=mean, return_info=True, bc=bc, bc_data=None, **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        # with zero data the start is the warm start's from zeros: the bits of u0 = 0, which are the zero start's
        got = P.solve_div(f, th, face_mean=mean, return_info=True, bc=bc, bc_data=zero, **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), bc
        for scheme in ("be", "cn"):
            kw = dict(dt=1e-3, steps=2, scheme=scheme, face_mean=mean, check=True, bc=bc)
            want, got = P.diffuse(u, th, f, **kw), P.diffuse(u, th, f, bc_data=zero, **kw)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (bc, scheme)


# ---- 3. the solve ------------------------------------------------------------------------------------------------------
# rtol 1e-10 and the factor 2 as tests/test_gpu_div_bc.py; the smallest eigenvalue is the matrix's own (shift-invert
# Lanczos on the sparse matrix, which test_sparse_matrix_is_the_dense_one ties to the dense restatement).
SOLVE_RTOL = 1e-10


def _sparse(th, mean, bc, sigma=0.0):
    """D_bc - sigma I as a sparse matrix, assembled from the restatement's face coefficients."""
    n = th.shape[-1]
    cE, cW, cS, cN = BC._cut(*D._faces(th, mean), bc)
    inv_h2 = float((n - 1) ** 2)
    idx = np.arange(n * n).reshape(n, n)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [(-((cE + cW) + (cS + cN)) * inv_h2 - sigma).reshape(-1)]
    for c, a, b in ((cE, idx[:, :-1], idx[:, 1:]), (cW, idx[:, 1:], idx[:, :-1]), (cS, idx[:-1, :], idx[1:, :]),
                    (cN, idx[1:, :], idx[:-1, :])):
        rows.append(a.reshape(-1))
        cols.append(b.reshape(-1))
        vals.append((c.reshape(-1)[a.reshape(-1)] * inv_h2))
    return csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n))


def test_sparse_matrix_is_the_dense_one():
    th = D.field_theta(6, 0, 0.5, 2.0)
    for bc in ("dddd", "ddnn", "nnnn"):
        M = BC.dense(th, "harmonic", bc, 3.0)
        assert np.abs(_sparse(th, "harmonic", bc, 3.0).toarray() - M).max() <= 8 * EPS * np.abs(M).max()


@functools.lru_cache(maxsize=None)
def _direct(n, mean, bc, sigma, b):
    """(the LU of D_bc - sigma I, lam_min(-(D_bc - sigma I))) of problem b's theta."""
    th = D.field_theta(n, 0, 0.5, 2.0, 2)[b]
    M = _sparse(th, mean, bc, sigma).tocsc()
    if n <= 12:
        lam_min = float(np.linalg.eigvalsh(-M.toarray())[0])
    else:
        lam_min = float(eigsh(-M, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    return splu(M), lam_min


def _check_solve(n, mean, bc, sigma, fn, thn, bdn, got, counts=True):
    from superresolution_for_pdes_amd import poisson as P
    u, iters, resid = got
    pat = BD.pattern(bc)
    sigma_p = R.precond_shift(thn, sigma)
    assert bool((resid <= SOLVE_RTOL).all())
    for b in range(fn.shape[0]):
        lu, lam_min = _direct(n, mean, pat, sigma, b)
        bd_b = bdn[b] if bdn.shape[0] > 1 else bdn[0]
        rhs = fn[b] - BD.affine(thn[b], bd_b, mean, pat)
        want = lu.solve(rhs.reshape(-1)).reshape(n, n)
        err, bound = np.linalg.norm(u[b].cpu().numpy() - want), 2.0 * SOLVE_RTOL * np.linalg.norm(rhs) / lam_min
        k_ref = BD.pcg(fn[b], thn[b], bd_b, mean, pat, sigma, sigma_p, rtol=SOLVE_RTOL)[1] if counts else None
        print(f"n={n} {mean} {bc} sigma={sigma:g} b={b}: err {err:.3e} bound {bound:.3e} iters {int(iters[b])} "
              f"ref {k_ref} resid {float(resid[b]):.3e}")
        assert err <= bound
        if counts:
            assert int(iters[b]) == k_ref
        assert 1 <= int(iters[b]) <= P.pcg_iterations(0.5, 2.0, SOLVE_RTOL)


# 5: one tile; 65: two tiles a side, the one-launch sine transform (bc None) / the separable products; 97: past the sine
# transform's LDS limit, so its multi-launch path preconditions
@pytest.mark.parametrize("bc", [None, "ddnn", "nnnn"])
@pytest.mark.parametrize("n", [5, 65, 97])
def test_solve_against_direct_solves(n, bc):
    from superresolution_for_pdes_amd import poisson as P
    B = 2
    fn, thn = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    for mean, sigma, bdn in (("harmonic", 0.0, BD.data(n, 5, B)), ("arithmetic", 1e3, BD.data(n, 6)[None])):
        if bc == "nnnn" and sigma == 0.0:
            sigma = 10.0
        got = P.solve_div(fn, thn, face_mean=mean, rtol=SOLVE_RTOL, return_info=True, shift=sigma, bc=bc, bc_data=bdn)
        _check_solve(n, mean, bc, sigma, fn, thn, bdn, got)
        res = P.residual_metrics(got[0], fn + sigma * got[0].cpu().numpy(), thn, form="divergence", face_mean=mean,
                                 bc=bc, bc_data=bdn)
        for b in range(B):
            bd_b = bdn[b] if bdn.shape[0] > 1 else bdn[0]
            nf = np.linalg.norm(fn[b] - BD.affine(thn[b], bd_b, mean, BD.pattern(bc)))
            assert float(res[b, 0]) <= 2.0 * SOLVE_RTOL * nf / n


@pytest.mark.parametrize("bc", [None, "ddnn"])
@pytest.mark.parametrize("n", [5, 65, 97])
def test_laplace_with_boundary_values(n, bc):
    """f = 0 with g != 0.  The homogeneous stop rule |r| <= rtol |f| is met by u = 0 at once; with data the reference
    norm is |f - b|, the iteration runs and the direct solution comes back."""
    from superresolution_for_pdes_amd import poisson as P
    B = 2
    fn, thn, bdn = np.zeros((B, n, n)), D.field_theta(n, 0, 0.5, 2.0, B), BD.data(n, 7, B)
    got = P.solve_div(fn, thn, rtol=SOLVE_RTOL, return_info=True, bc=bc, bc_data=bdn)
    assert int(got[1].min()) >= 1 and float(got[0].abs().max()) > 1e-3
    _check_solve(n, "harmonic", bc, 0.0, fn, thn, bdn, got)
    plain = P.solve_div(fn, thn, rtol=SOLVE_RTOL, return_info=True, bc=bc)
    assert not bool(plain[0].any()) and plain[1].tolist() == [0, 0]


@pytest.mark.parametrize("bc", [None, "dnnd"])
def test_solve_does_not_depend_on_the_batch(bc):
    from superresolution_for_pdes_amd import poisson as P
    n, B, sigma = 70, 3, 1e3
    f, th, bd = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B), BD.data(n, 8, B)
    sigma_p = R.precond_shift(th, sigma)
    whole = P.solve_div(f, th, return_info=True, shift=sigma, precond_shift=sigma_p, bc=bc, bc_data=bd)
    one = P.solve_div(f[1], th[1], return_info=True, shift=sigma, precond_shift=sigma_p, bc=bc, bc_data=bd[1])
    assert torch.equal(one[0][0], whole[0][1])
    assert int(one[1][0]) == int(whole[1][1]) and float(one[2][0]) == float(whole[2][1])
    shared = P.solve_div(f, th, return_info=True, shift=sigma, precond_shift=sigma_p, bc=bc, bc_data=bd[1:2])
    assert torch.equal(shared[0][1], whole[0][1])


@pytest.mark.parametrize("bc,sigma", [(None, 0.0), ("ddnn", 0.0), ("nnnn", 1e3)])
def test_warm_start(bc, sigma):
    from superresolution_for_pdes_amd import poisson as P
    n, B, rtol = 40, 3, 1e-10
    f, th, bd = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B), BD.data(n, 9, B)
    zero = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc, bc_data=bd)
    got = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc, bc_data=bd, u0=np.zeros((n, n)))
    assert all(torch.equal(g, w) for g, w in zip(got, zero))           # a null u0 gives the bits of a zero field
    assert int(zero[1].min()) >= 1
    tight = P.solve_div(f, th, rtol=1e-13, shift=sigma, bc=bc, bc_data=bd)
    u, iters, resid = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc, bc_data=bd, u0=tight)
    assert iters.tolist() == [0, 0, 0] and torch.equal(u, tight) and bool((resid <= rtol).all())


@pytest.mark.parametrize("bc", [None, "ddnn"])
def test_fixed_mode_under_graph_capture(bc):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 20, 3
    th, f, bd = _dev(D.field_theta(n, 0, 0.5, 2.0, B)), _dev(_forcings(n, B)), _dev(BD.data(n, 10, B))
    k = P.pcg_iterations(0.5, 2.0) + 4
    kw = dict(maxit=k, check_every=0, return_info=True, bc=bc, bc_data=bd)
    P.dst_plan(n) if bc is None else P.sep_plan(n, bc)
    eager = P.solve_div(f, th, **kw)
    assert int(eager[1].max()) < k                           # every problem froze before the count ran out
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # every launch goes to the one capturing stream: a linear chain, no branches
        out = P.solve_div(f, th, **kw)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


# ---- 4. diffuse ----------------------------------------------------------------------------------------------------------
def test_diffuse_converges_to_the_stationary_solution():
    """Backward Euler from 0 with constant g on two sides and constant fluxes through the others.  With e_s the error
    against the stationary solution, e_s+1 = sigma (sigma I - D)^-1 e_s + (the step's solve error), so
    |e_T| <= rho^T |u_stat| + sum_s 2 rtol |rhs_s - b| / (lam_min + sigma) + (the stationary solve's own bound),
    rho = sigma / (sigma + lam_min): the transient plus the solves' tolerance bounds."""
    from superresolution_for_pdes_amd import poisson as P
    n, bc, dt, steps, rtol = 17, "ddnn", 5.0, 12, 1e-12
    th, fn = D.field_theta(n, 3, 0.5, 2.0), D.forcing(n)
    bd = P.bc_data(n, bc, row0=1.5, row1=-0.5, col0=0.25, col1=-0.75).cpu().numpy()
    sigma = 1.0 / dt
    stat = P.solve_div(fn, th, rtol=rtol, bc=bc, bc_data=bd)[0].cpu().numpy()
    u, frames = P.diffuse(np.zeros((n, n)), th, fn, dt=dt, steps=steps, rtol=rtol, bc=bc, bc_data=bd, save_every=1)
    lam_min = float(np.linalg.eigvalsh(-BC.dense(th, "harmonic", bc))[0])
    b = BD.affine(th, bd[0], "harmonic", bc)
    bound = 2.0 * rtol * np.linalg.norm(fn - b) / lam_min + (sigma / (sigma + lam_min)) ** steps * np.linalg.norm(stat)
    prev = np.zeros((n, n))
    for s in range(steps):
        rhs = BD.step_rhs(prev, fn, th, bd[0], "harmonic", sigma, "be", bc)
        bound += 2.0 * rtol * np.linalg.norm(rhs - b) / (lam_min + sigma)
        prev = frames[s, 0].cpu().numpy()
    err = np.linalg.norm(u[0].cpu().numpy() - stat)
    print(f"err {err:.3e} bound {bound:.3e} |stat| {np.linalg.norm(stat):.3e}")
    assert err <= bound
    assert np.linalg.norm(stat - BD.solve_dense(fn, th, bd[0], "harmonic", bc)[0]) <= 2.0 * rtol * np.linalg.norm(fn - b) / lam_min


def test_insulated_box_balances_flux_and_forcing():
    """Four flux sides: 1^T (D - sigma I) u+ = -sigma sum u+ and 1^T (rhs - b) = sum f - sigma sum u - sum q / h, so a
    backward-Euler step changes sum u by dt (sum q / h - sum f) up to 1^T r, |1^T r| <= n rtol |rhs - b|: the
    conservation bound of tests/div_bc_ref.py with the new reference norm."""
    from superresolution_for_pdes_amd import poisson as P
    n, dt, rtol, steps = BC.BOX_N, BC.BOX_DT, BC.BOX_RTOL, 5
    u0, th = BC.box_case()
    fn, bd = D.forcing(n), BD.data(n, 11)
    sigma, inv_h = 1.0 / dt, float(n - 1)
    u, frames = P.diffuse(u0, th, fn, dt=dt, steps=steps, rtol=rtol, bc="nnnn", bc_data=bd, save_every=1)
    b = BD.affine(th, bd, "harmonic", "nnnn")
    want = dt * (bd.sum() * inv_h - fn.sum())
    assert abs(b.sum() - bd.sum() * inv_h) <= 64 * n * EPS * np.abs(bd).max() * inv_h
    prev = u0
    for s in range(steps):
        new = frames[s, 0].cpu().numpy()
        rhs = BD.step_rhs(prev, fn, th, bd, "harmonic", sigma, "be", "nnnn")
        drift = abs((new.sum() - prev.sum()) - want)
        bound = BC.conservation_bound(n, rtol, rhs - b, sigma, prev)
        print(f"step {s}: change {new.sum() - prev.sum():.6e} expected {want:.6e} drift {drift:.3e} bound {bound:.3e}")
        assert drift <= bound
        prev = new


# ---- 5. autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc,sigma", [(None, 0.0), ("ddnn", 0.0), ("nnnn", 7.5)])
@pytest.mark.parametrize("mean", D.MEANS)
def test_gradcheck(mean, bc, sigma):
    """Tolerances as tests/test_gpu_div_adjoint.py: rtol=1e-13 keeps the solve's noise under gradcheck's atol."""
    from superresolution_for_pdes_amd import poisson as P
    n, B = 5, 2
    u = _dev(D.field_u(n, 0, B)).requires_grad_(True)
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B)).requires_grad_(True)
    for bdn in (BD.data(n, 12, B), BD.data(n, 13)[None]):              # per problem, and shared: summed over the batch
        bd = _dev(bdn).requires_grad_(True)
        assert torch.autograd.gradcheck(
            lambda a, t, d: P.apply_div(a, t, face_mean=mean, shift=sigma, bc=bc, bc_data=d), (u, th, bd))
        f = _dev(np.stack([D.forcing(n), D.field_u(n, 4)])).requires_grad_(True)
        pshift = 7.0 if sigma else None
        assert torch.autograd.gradcheck(
            lambda a, t, d: P.solve_div(a, t, face_mean=mean, rtol=1e-13, shift=sigma, precond_shift=pshift, bc=bc,
                                        bc_data=d), (f, th, bd))
    # the builder passes gradients to its sides
    side = torch.full((n,), 0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    P.apply_div(u.detach(), th.detach(), face_mean=mean, bc=bc, bc_data=P.bc_data(n, bc, col1=side, B=B)).sum().backward()
    assert side.grad is not None and bool(side.grad.abs().min() > 0)


@pytest.mark.parametrize("scheme", ["be", "cn"])
def test_gradients_through_two_steps(scheme):
    """As tests/test_gpu_div_bc.py::test_theta_gradient_through_two_steps, in theta and in the data."""
    from superresolution_for_pdes_amd import poisson as P
    n, dt, bc, mean = 5, 5e-2, "dnnd", "harmonic"
    u0, fn, thn, w, bdn = D.field_u(n, 9), D.forcing(n), D.field_theta(n, 5, 0.5, 2.0), D.field_u(n, 10), BD.data(n, 14)
    th, bd = _dev(thn).requires_grad_(True), _dev(bdn).requires_grad_(True)
    u = P.diffuse(u0, th, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13, bc=bc, bc_data=bd)
    assert u.grad_fn is not None
    ((u[0] * _dev(w)).sum()).backward()
    eps = 1e-6

    def loss(t, d):
        return np.sum(w * BD.diffuse_dense(u0, t, d, fn, dt, 2, scheme, mean, bc))
    want_th, want_bd = np.zeros((n, n)), np.zeros((4, n))
    for i in range(n):
        for j in range(n):
            d = np.zeros((n, n))
            d[i, j] = eps
            want_th[i, j] = (loss(thn + d, bdn) - loss(thn - d, bdn)) / (2.0 * eps)
    for s in range(4):
        for k in range(n):
            d = np.zeros((4, n))
            d[s, k] = eps
            want_bd[s, k] = (loss(thn, bdn + d) - loss(thn, bdn - d)) / (2.0 * eps)
    for name, got, want in (("theta", th.grad, want_th), ("data", bd.grad, want_bd)):
        err = np.linalg.norm(got.cpu().numpy().reshape(want.shape) - want) / np.linalg.norm(want)
        print(f"{scheme} {name}: relative error {err:.3e}")
        assert err <= 1e-6
    plain = P.diffuse(u0, thn, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13, bc=bc, bc_data=bdn)
    assert plain.grad_fn is None and float((plain - u.detach()).norm() / plain.norm()) <= 1e-12


# ---- 6. the raw entries' refusals ------------------------------------------------------------------------------------------
def test_library_argument_errors():
    """Each bad argument returns the error before any launch: the outputs and the workspace keep their bytes."""
    from superresolution_for_pdes_amd import _lib, poisson as P
    n, B = 8, 2
    N = B * n * n
    buf = torch.randn(5, N + 1, dtype=torch.float64, device="cuda")
    u, f, th, y, bd = (buf[i, :N] for i in range(5))
    th.abs_().add_(0.5)
    y.fill_(-7.0)
    off = [buf.view(torch.float32)[i, 1:].data_ptr() for i in range(5)]       # offset by 4 bytes
    sp = _lib.stream_ptr()
    m = BC.mask("ddnn")
    plan, other, box, sine = P.sep_plan(n, "ddnn"), P.sep_plan(n, "nddd"), P.sep_plan(n, "nnnn"), P.dst_plan(n)
    nbytes = int(_lib.query("srpde_div_cg_workspace_size_bc", B, n))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def refuse(name, ok, cases):
        for i, v, match in cases:
            args = list(ok)
            if isinstance(i, tuple):
                for ii, vv in zip(i, v):
                    args[ii] = vv
            else:
                args[i] = v
            rc = getattr(_lib.lib(), name)(*args)
            assert rc < 0, (name, i, v)
            with pytest.raises(RuntimeError, match=match):
                _lib.call(name, *args)

    def data_cases(at, bd_at=None):                              # the indices of bc and of bd; bd_stride follows bd
        bd_at = at + 1 if bd_at is None else bd_at
        return [(at, -1, "bc"), (at, 16, "bc"), (bd_at, 0, "boundary data"), (bd_at, off[4], "aligned"),
                (bd_at + 1, n, "bd_stride"), (bd_at + 1, -4 * n, "bd_stride")]

    ok = (u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, float((n - 1) ** 2), 7.5, m, bd.data_ptr(), 4 * n, sp)
    refuse("srpde_div_apply_bd", ok,
           [(i, 0, "null") for i in range(3)] + [(i, off[i], "aligned") for i in range(3)] +
           [(2, ok[0], "alias"), (2, ok[9], "alias"), (5, 2, "face_mean"), (6, 0.0, "inv_h2"), (3, 0, "shape"),
            (7, -1.0, "sigma")] + data_cases(8))
    ok = (u.data_ptr(), f.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, 7.5, 1, m, bd.data_ptr(), 0, sp)
    refuse("srpde_div_step_rhs_bd", ok,
           [(i, 0, "null") for i in (0, 2, 3)] + [(3, ok[0], "alias"), (8, 2, "cn"), (7, float("nan"), "sigma")] +
           data_cases(9))
    ok = (u.data_ptr(), f.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, float((n - 1) ** 2), 1.0, m, bd.data_ptr(),
          4 * n, sp)
    refuse("srpde_div_theta_grad_bd", ok,
           [(i, 0, "null") for i in range(4)] + [(3, ok[2], "alias"), (8, float("inf"), "scale")] + data_cases(9))
    ok = (u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, float((n - 1) ** 2), m, sp)
    refuse("srpde_div_bd_grad", ok,
           [(i, 0, "null") for i in range(3)] + [(2, ok[0], "alias"), (5, -1.0, "inv_h2"), (4, 1, "shape"), (6, 16, "bc"),
                                                 (6, -1, "bc")])
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())

    tail = (plan.data_ptr(), plan.numel(), ws.data_ptr(), nbytes, sp)
    ok = (f.data_ptr(), u.data_ptr(), th.data_ptr(), B, n, 1, m, 7.5, 7.0, 1e-10, bd.data_ptr(), 4 * n) + tail
    refuse("srpde_div_cg_init_from_bd", ok,
           [(0, 0, "null"), (2, 0, "null"), (5, 2, "face_mean"), (9, -1e-10, "rtol"), (15, nbytes - 16, "workspace"),
            ((12, 13), (other.data_ptr(), other.numel()), "plan"),
            ((12, 13), (sine.data_ptr(), sine.numel()), "plan"),                  # the sine plan goes with mask 0 only
            ((6, 12, 13), (0, plan.data_ptr(), plan.numel()), "plan"),            # and mask 0 with no other
            ((6, 7, 12, 13), (15, 0.0, box.data_ptr(), box.numel()), "singular"),
            ((6, 8, 12, 13), (15, 0.0, box.data_ptr(), box.numel()), "singular")] + data_cases(6, 10))
    torch.cuda.synchronize()
    assert not bool(ws.any())                               # nothing was launched on the workspace
