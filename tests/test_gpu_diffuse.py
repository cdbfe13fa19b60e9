"""GPU: the shifted operator D_theta - sigma I and implicit time stepping (csrc/poisson_div.hip, csrc/poisson_dst.hip,
ABI 21): srpde_div_apply_shift and srpde_div_step_rhs against the numpy restatement of tests/diffuse_ref.py bit for
bit, the shifted sine solve and the shifted CG against numpy and dense solves, poisson.diffuse, graph capture,
autograd, and the argument checks.  shift = 0 must give today's bits everywhere."""
import numpy as np
import pytest
import torch

import diffuse_ref as R
import poisson_div_ref as D

pytestmark = pytest.mark.gpu

SIGMAS = (0.0, 7.5, 1e6)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forcings(n, B):
    return np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)])


# ---- 1. the shifted apply -----------------------------------------------------------------------------------
# n = 2: ghost and single faces only; 3: one interior node; 33 crosses a tile edge in y (32 rows), 65 one in x (64
# columns), 70 both with ragged last tiles
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [2, 3, 33, 65, 70])
def test_apply_shift_is_bit_equal_to_the_host_restatement(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    B = 3
    u, th = D.field_u(n, 0, B), D.field_theta(n, 0, 0.1, 10.0, B)
    for sigma in SIGMAS:
        got = P.apply_div(u, th, face_mean=mean, shift=sigma)
        assert got.dtype == torch.float64 and got.shape == (B, n, n)
        assert np.array_equal(got.cpu().numpy(), R.apply_shift(u, th, mean, sigma)), sigma
    assert torch.equal(P.apply_div(u, th, face_mean=mean, shift=0.0), P.apply_div(u, th, face_mean=mean))
    # another inv_h2 and a broadcast theta
    got = P.apply_div(u, th[1], face_mean=mean, inv_h2=1234.5, shift=7.5)
    assert np.array_equal(got.cpu().numpy(), R.apply_shift(u, th[1], mean, 7.5, inv_h2=1234.5))


def test_apply_shift_entry_at_sigma_zero_is_the_unshifted_entry():
    """The C entry itself (poisson.apply_div never calls it with 0): the bits of srpde_div_apply."""
    from superresolution_for_pdes_amd import _lib, poisson as P
    n, B = 70, 3
    u, th = _dev(D.field_u(n, 0, B)), _dev(D.field_theta(n, 0, 0.1, 10.0, B))
    for mean in (0, 1):
        y = torch.empty_like(u)
        _lib.call("srpde_div_apply_shift", u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, mean, float((n - 1) ** 2),
                  0.0, _lib.stream_ptr())
        assert torch.equal(y, P.apply_div(u, th, face_mean=D.MEANS[mean]))


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [2, 33, 70])
def test_step_rhs_is_bit_equal_to_the_host_restatement(n, mean):
    from superresolution_for_pdes_amd import _lib
    B = 3
    un, fn, thn = D.field_u(n, 2, B), D.field_u(n, 3, B), D.field_theta(n, 1, 0.1, 10.0, B)
    u, f, th = _dev(un), _dev(fn), _dev(thn)
    for cn, scheme in enumerate(("be", "cn")):
        for sigma in (7.5, 1e6):
            for fp, fh in ((f.data_ptr(), fn), (0, None)):
                rhs = torch.empty_like(u)
                _lib.call("srpde_div_step_rhs", u.data_ptr(), fp, th.data_ptr(), rhs.data_ptr(), B, n,
                          D.MEANS.index(mean), sigma, cn, _lib.stream_ptr())
                assert np.array_equal(rhs.cpu().numpy(), R.step_rhs(un, fh, thn, mean, sigma, scheme))


# ---- 2. the shifted sine solve ------------------------------------------------------------------------------
def _dst_shift(f, sigma_p):
    from superresolution_for_pdes_amd import _lib, poisson as P
    B, n = f.shape[0], f.shape[-1]
    u = torch.empty_like(f)
    plan = P.dst_plan(n)
    ws, ws_bytes = P._dst_ws(B, n, f.device)
    _lib.call("srpde_poisson_dst_shift_batched", f.data_ptr(), u.data_ptr(), B, n, float(sigma_p), plan.data_ptr(),
              plan.numel(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    return u


# 97 and the first n above the library's LDS limit (the four-launch path), the limit itself (the LDS kernel's largest)
@pytest.mark.parametrize("n", [5, 40, 97, "lds_max", "lds_max+1"])
def test_shifted_sine_solve(n):
    from superresolution_for_pdes_amd import _lib, poisson as P
    lds_max = int(_lib.query("srpde_poisson_dst_lds_max_n"))
    n = {"lds_max": lds_max, "lds_max+1": lds_max + 1}.get(n, n)
    B = 2
    fn = D.field_u(n, 5, B)
    f = _dev(fn)
    for sigma_p in (10.0, 1e3, 1e7):
        got = _dst_shift(f, sigma_p).cpu().numpy()
        for b in range(B):
            want = R.sine_solve_shift(fn[b], sigma_p)
            err = np.linalg.norm(got[b] - want) / np.linalg.norm(want)
            assert err <= 1e-11, (n, sigma_p, err)
    # sigma_p = 0: the unshifted kernels, the bits of the theta = 1 solve
    assert torch.equal(_dst_shift(f, 0.0), P.solve_direct(f, torch.ones_like(f)))


# ---- 3. the shifted solve -----------------------------------------------------------------------------------
# rtol 1e-10: the dense LU solve's own residual (~n^2 eps |f|, 1e-13) and the drift of CG's recurrence residual
# from the true one are both far below it, so of the bound's 2 rtol one covers the device and one is spare.
SOLVE_RTOL = 1e-10


def _solve_bound(f, th, n, sigma, rtol=SOLVE_RTOL):
    return 2.0 * rtol * np.linalg.norm(f) / (th.min() * R.lambda_min_neg_laplacian(n) + sigma)


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [9, 33])
def test_shifted_solve_against_the_dense_reference(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    B = 2
    fn, thn = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    for sigma in (10.0, 1e4):
        sigma_p = R.precond_shift(thn, sigma)              # over the batch, as precond_shift=None takes it
        u, iters, resid = P.solve_div(fn, thn, face_mean=mean, rtol=SOLVE_RTOL, return_info=True, shift=sigma)
        same = P.solve_div(fn, thn, face_mean=mean, rtol=SOLVE_RTOL, return_info=True, shift=sigma,
                           precond_shift=sigma_p)
        assert all(torch.equal(a, b) for a, b in zip((u, iters, resid), same))
        routed = P.solve_batched(fn, thn, rtol=SOLVE_RTOL, form="divergence", face_mean=mean, shift=sigma,
                                 return_iters=True)
        assert torch.equal(routed[0], u) and torch.equal(routed[1], iters)
        assert bool((resid <= SOLVE_RTOL).all())
        for b in range(B):
            want = np.linalg.solve(R.dense_shift(thn[b], mean, sigma), fn[b].reshape(-1)).reshape(n, n)
            err, bound = np.linalg.norm(u[b].cpu().numpy() - want), _solve_bound(fn[b], thn[b], n, sigma)
            k_ref = R.pcg_shift(fn[b], thn[b], mean, sigma, sigma_p, rtol=SOLVE_RTOL)[1]
            print(f"n={n} {mean} sigma={sigma:g} b={b}: err {err:.3e} bound {bound:.3e} iters {int(iters[b])} ref {k_ref}")
            assert err <= bound
            assert int(iters[b]) == k_ref


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [40, 70])
def test_zero_shift_gives_todays_solve(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    B = 3
    f, th = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    want = P.solve_div(f, th, face_mean=mean, return_info=True)
    for kw in ({"shift": 0.0}, {"shift": 0.0, "precond_shift": 0.0}):
        got = P.solve_div(f, th, face_mean=mean, return_info=True, **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    u0 = D.field_u(n, 1, B)
    want = P.solve_div(f, th, face_mean=mean, return_info=True, u0=u0)
    got = P.solve_div(f, th, face_mean=mean, return_info=True, u0=u0, shift=0.0)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


# ---- 4. batch independence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_shifted_solve_does_not_depend_on_the_batch(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B, sigma = 70, 5, 1e3
    f, th = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    sigma_p = R.precond_shift(th, sigma)                   # one sigma_p for both calls: it is an input
    whole = P.solve_div(f, th, face_mean=mean, return_info=True, shift=sigma, precond_shift=sigma_p)
    one = P.solve_div(f[2], th[2], face_mean=mean, return_info=True, shift=sigma, precond_shift=sigma_p)
    assert torch.equal(one[0][0], whole[0][2])
    assert int(one[1][0]) == int(whole[1][2]) and float(one[2][0]) == float(whole[2][2])


# ---- 5. the warm start with a shift -------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_warm_start_with_a_shift(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B, sigma, rtol = 40, 3, 1e3, 1e-10
    f, th = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    f[2] = 0.0
    zero = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, shift=sigma)
    got = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, shift=sigma, u0=np.zeros((n, n)))
    assert all(torch.equal(g, w) for g, w in zip(got, zero))
    assert int(zero[1][2]) == 0 and int(zero[1][:2].min()) >= 1
    # a tighter solve is a u0 that already satisfies rtol: no iteration, u = u0
    tight = P.solve_div(f, th, face_mean=mean, rtol=1e-13, shift=sigma)
    u, iters, resid = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, shift=sigma, u0=tight)
    assert iters.tolist() == [0, 0, 0] and torch.equal(u, tight) and bool((resid <= rtol).all())


# ---- 6. diffuse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("scheme", ["be", "cn"])
def test_one_step_against_the_dense_step(scheme, mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B, dt = 17, 2, 2e-3
    u0, fn, thn = D.field_u(n, 7, B), _forcings(n, B), D.field_theta(n, 3, 0.5, 2.0, B)
    sigma = R.step_sigma(dt, scheme)
    u, counts = P.diffuse(u0, thn, fn, dt=dt, steps=1, scheme=scheme, face_mean=mean, rtol=SOLVE_RTOL, check=True)
    assert u.shape == (B, n, n) and counts.shape == (1, B) and counts.dtype == torch.int32
    for b in range(B):
        want = R.step_dense(u0[b], fn[b], thn[b], dt, scheme, mean)
        rhs = R.step_rhs(u0[b], fn[b], thn[b], mean, sigma, scheme)
        err, bound = np.linalg.norm(u[b].cpu().numpy() - want), _solve_bound(rhs, thn[b], n, sigma)
        print(f"{scheme} {mean} b={b}: err {err:.3e} bound {bound:.3e} iters {int(counts[0, b])}")
        assert err <= bound
    # no forcing, a 2-D call, and u0 is left as it was
    u0d = _dev(u0[0])
    keep = u0d.clone()
    got = P.diffuse(u0d, thn[0], dt=dt, scheme=scheme, face_mean=mean, rtol=SOLVE_RTOL)
    want = R.step_dense(u0[0], None, thn[0], dt, scheme, mean)
    rhs = R.step_rhs(u0[0], None, thn[0], mean, sigma, scheme)
    assert np.linalg.norm(got[0].cpu().numpy() - want) <= _solve_bound(rhs, thn[0], n, sigma)
    assert torch.equal(u0d, keep)


@pytest.mark.parametrize("scheme", ["be", "cn"])
def test_eigenmode_decay_on_the_device(scheme):
    from superresolution_for_pdes_amd import poisson as P
    n, c, dt, steps = 33, 1.7, 3e-3, 5
    v0, mu0 = R.eigenmode(n, 0, 0)
    v1, mu1 = R.eigenmode(n, 2, 5)
    u, frames = P.diffuse(np.stack([v0, v1]), np.full((n, n), c), dt=dt, steps=steps, scheme=scheme, save_every=1)
    assert frames.shape == (steps, 2, n, n) and torch.equal(frames[-1], u)
    for b, (v, mu) in enumerate(((v0, mu0), (v1, mu1))):
        g = R.decay_factor(dt, c, mu, scheme)
        for s in range(steps):
            err = np.abs(frames[s, b].cpu().numpy() - g ** (s + 1) * v).max()
            assert err <= 1e-10 * np.abs(v).max(), (b, s, err)


@pytest.mark.parametrize("mean", D.MEANS)
def test_backward_euler_reaches_the_steady_state(mean):
    from superresolution_for_pdes_amd import poisson as P
    n = 33
    f, th = D.forcing(n), D.field_theta(n, 2, 0.5, 2.0)
    u = P.diffuse(np.zeros((n, n)), th, f, dt=1.0, steps=200, scheme="be", face_mean=mean)
    want = P.solve_div(f, th, face_mean=mean)
    assert float((u - want).norm() / want.norm()) <= 1e-8


@pytest.mark.parametrize("mean", D.MEANS)
def test_warm_start_never_costs_iterations(mean):
    """A smooth forcing switched on at t = 0: every step's solve from the previous state takes at most the iterations
    of the same solve from zero."""
    from superresolution_for_pdes_amd import poisson as P
    n, B, dt, steps = 33, 2, 1e-2, 8
    f = np.stack([D.forcing(n, 1.0, 0.5), D.forcing(n, 1.5, 1.0)])
    th = D.field_theta(n, 4, 0.5, 2.0, B)
    sigma = 1.0 / dt
    sigma_p = R.precond_shift(th, sigma)
    u, frames, warm = P.diffuse(np.zeros((B, n, n)), th, f, dt=dt, steps=steps, face_mean=mean, save_every=1,
                                check=True)
    state = torch.zeros(B, n, n, dtype=torch.float64, device="cuda")
    fd = _dev(f)
    for s in range(steps):
        rhs = fd - sigma * state
        sol, zero, _ = P.solve_div(rhs, th, face_mean=mean, return_info=True, shift=sigma, precond_shift=sigma_p,
                                   u0=np.zeros((n, n)))
        print(f"{mean} step {s}: warm {warm[s].tolist()} zero {zero.tolist()}")
        assert bool((warm[s] <= zero).all()), (s, warm[s].tolist(), zero.tolist())
        state = frames[s]
    assert int(warm[0].min()) >= 1


# ---- 7. graph capture ---------------------------------------------------------------------------------------
def test_fixed_mode_under_graph_capture():
    from superresolution_for_pdes_amd import poisson as P
    n, B, dt, steps = 20, 4, 1e-3, 10
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B))
    f, u0 = _dev(_forcings(n, B)), _dev(D.field_u(n, 8, B))
    k = P.pcg_iterations(0.5, 2.0) + 4
    sigma_p = (1.0 / dt) / float(np.sqrt(0.5 * 2.0))
    kw = dict(dt=dt, steps=steps, pcg_iters=k, precond_shift=sigma_p, save_every=5, check=True)
    P.dst_plan(n)
    eager = P.diffuse(u0, th, f, **kw)
    tol = P.diffuse(u0, th, f, dt=dt, steps=steps)           # the fixed count reaches what the tolerance mode does
    assert float((eager[0] - tol).norm() / tol.norm()) <= 1e-10
    assert int(eager[2].max()) < k                           # every problem froze before the count ran out
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # every launch goes to the one capturing stream: a linear chain, no branches
        out = P.diffuse(u0, th, f, **kw)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


def test_auto_precond_shift_is_refused_in_fixed_mode():
    from superresolution_for_pdes_amd import poisson as P
    n = 8
    f, th = _dev(D.forcing(n)), _dev(D.field_theta(n, 0, 0.5, 2.0))
    with pytest.raises(ValueError, match="precond_shift"):
        P.diffuse(f, th, dt=1e-2, pcg_iters=10)
    with pytest.raises(ValueError, match="precond_shift"):
        P.solve_div(f, th, shift=10.0, maxit=10, check_every=0)
    with pytest.raises(ValueError, match="precond_shift"):
        P.solve_div(f, th, precond_shift=3.0)                # a preconditioner shift without a shift


# ---- 8. autograd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_gradcheck_with_a_shift(mean):
    """Tolerances as tests/test_gpu_div_adjoint.py: rtol=1e-13 keeps the solve's noise under gradcheck's atol."""
    from superresolution_for_pdes_amd import poisson as P
    n, B, sigma = 4, 2, 7.5
    u = _dev(D.field_u(n, 0, B)).requires_grad_(True)
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, t: P.apply_div(a, t, face_mean=mean, shift=sigma), (u, th))
    f = _dev(np.stack([D.forcing(n), D.field_u(n, 4)])).requires_grad_(True)
    # sigma_p is an input of the solve: fixed, so the perturbed solves share it
    assert torch.autograd.gradcheck(
        lambda a, t: P.solve_div(a, t, face_mean=mean, rtol=1e-13, shift=sigma, precond_shift=7.0), (f, th))
    assert torch.autograd.gradcheck(lambda a, t: P.solve_div(a, t, face_mean=mean, rtol=1e-13, shift=sigma), (f, th))


@pytest.mark.parametrize("scheme", ["be", "cn"])
@pytest.mark.parametrize("mean", D.MEANS)
def test_theta_gradient_through_two_steps(mean, scheme):
    from superresolution_for_pdes_amd import poisson as P
    n, dt = 5, 5e-2
    u0, fn, thn, w = D.field_u(n, 9), D.forcing(n), D.field_theta(n, 5, 0.5, 2.0), D.field_u(n, 10)
    th = _dev(thn).requires_grad_(True)
    u0d = _dev(u0).requires_grad_(True)
    u = P.diffuse(u0d, th, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13)
    assert u.grad_fn is not None
    ((u[0] * _dev(w)).sum()).backward()

    def loss(t, v):
        return float(np.sum(w * R.diffuse_dense(v, t, fn, dt, 2, scheme, mean)))

    eps = 1e-6
    for leaf, x in ((th, thn), (u0d, u0)):
        want = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                d = np.zeros((n, n))
                d[i, j] = eps
                args_p, args_m = ((x + d, u0), (x - d, u0)) if leaf is th else ((thn, x + d), (thn, x - d))
                want[i, j] = (loss(*args_p) - loss(*args_m)) / (2.0 * eps)
        got = leaf.grad.cpu().numpy()
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"{scheme} {mean} {'theta' if leaf is th else 'u0'}: relative error {err:.3e}")
        assert err <= 1e-6
    # without grad the direct path gives the same step
    plain = P.diffuse(u0, thn, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13)
    assert plain.grad_fn is None and float((plain - u.detach()).norm() / plain.norm()) <= 1e-12


# ---- 9. argument errors -------------------------------------------------------------------------------------
def test_python_argument_errors():
    from superresolution_for_pdes_amd import poisson as P
    n = 8
    f, th = _dev(D.forcing(n)), _dev(D.field_theta(n, 0, 0.5, 2.0))
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="shift"):
            P.apply_div(f, th, shift=bad)
        with pytest.raises(ValueError, match="shift"):
            P.solve_div(f, th, shift=bad)
        with pytest.raises(ValueError, match="precond_shift"):
            P.solve_div(f, th, shift=1.0, precond_shift=bad)
    for kw in ({"shift": 10.0}, {"precond_shift": 1.0}, {"shift": 10.0, "method": "dst"}):
        with pytest.raises(ValueError, match="divergence"):
            P.solve_batched(f, th, **kw)
    with pytest.raises(ValueError, match="scheme"):
        P.diffuse(f, th, dt=1e-2, scheme="fe")
    for dt in (0.0, -1e-2, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="dt"):
            P.diffuse(f, th, dt=dt)
    with pytest.raises(ValueError, match="pcg_iters"):
        P.diffuse(f, th, dt=1e-2, pcg_iters=0, precond_shift=1.0)
    with pytest.raises(ValueError, match="face mean"):
        P.diffuse(f, th, dt=1e-2, face_mean="geometric")


def test_library_argument_errors():
    """Each bad argument returns the error before any launch: the outputs keep their bytes."""
    from superresolution_for_pdes_amd import _lib, poisson as P
    n, B = 8, 2
    N = B * n * n
    buf = torch.randn(4, N + 1, dtype=torch.float64, device="cuda")
    u, f, th, y = (buf[i, :N] for i in range(4))
    th.abs_().add_(0.5)
    y.fill_(-7.0)
    off = [buf.view(torch.float32)[i, 1:].data_ptr() for i in range(4)]       # offset by 4 bytes
    sp = _lib.stream_ptr()
    plan = P.dst_plan(n)
    nbytes = int(_lib.query("srpde_div_cg_workspace_size", B, n))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    tail = (plan.data_ptr(), plan.numel(), ws.data_ptr(), nbytes, sp)
    bad_sigmas = (-1.0, float("inf"), float("nan"))

    def refuse(name, ok, cases):
        for i, v, match in cases:
            args = list(ok)
            args[i] = v
            with pytest.raises(RuntimeError, match=match):
                _lib.call(name, *args)

    ok = (u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, float((n - 1) ** 2), 7.5, sp)
    refuse("srpde_div_apply_shift", ok,
           [(i, 0, "null") for i in range(3)] + [(i, off[i], "aligned") for i in range(3)] +
           [(2, ok[0], "alias"), (2, ok[1], "alias"), (5, 2, "face_mean"), (6, 0.0, "inv_h2"), (3, 0, "shape"),
            (4, 1, "shape")] + [(7, s, "sigma") for s in bad_sigmas])
    ok = (u.data_ptr(), f.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, 7.5, 1, sp)
    refuse("srpde_div_step_rhs", ok,
           [(i, 0, "null") for i in (0, 2, 3)] + [(i, off[i], "aligned") for i in range(4)] +
           [(3, ok[i], "alias") for i in range(3)] + [(6, -1, "face_mean"), (8, 2, "cn"), (4, 0, "shape")] +
           [(7, s, "sigma") for s in bad_sigmas])
    ok = (f.data_ptr(), y.data_ptr(), B, n, 7.5, plan.data_ptr(), plan.numel(), 0, 0, sp)
    refuse("srpde_poisson_dst_shift_batched", ok,
           [(0, 0, "null"), (1, 0, "null"), (0, off[1], "aligned"), (1, off[3], "aligned"), (3, 1, "shape"),
            (6, plan.numel() - 8, "plan")] + [(4, s, "sigma_p") for s in bad_sigmas])
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())

    ok = (f.data_ptr(), B, n, 7.5) + tail
    refuse("srpde_div_cg_init_shift", ok,
           [(0, 0, "null"), (0, off[1], "aligned"), (7, nbytes - 16, "workspace")] +
           [(3, s, "sigma_p") for s in bad_sigmas])
    ok = (f.data_ptr(), u.data_ptr(), th.data_ptr(), B, n, 1, 7.5, 7.0, 1e-10) + tail
    refuse("srpde_div_cg_init_from_shift", ok,
           [(i, 0, "null") for i in range(3)] + [(1, off[0], "aligned"), (5, 2, "face_mean"), (8, -1e-10, "rtol"),
                                                 (12, nbytes - 16, "workspace")] +
           [(6, s, "sigma") for s in bad_sigmas] + [(7, s, "sigma_p") for s in bad_sigmas])
    ok = (th.data_ptr(), B, n, 1, 7.5, 7.0, 1e-10, 1, 2) + tail
    refuse("srpde_div_cg_iterate_shift", ok,
           [(0, 0, "null"), (0, off[2], "aligned"), (3, 2, "face_mean"), (6, float("nan"), "rtol"), (7, 0, "k_begin"),
            (12, nbytes - 16, "workspace")] +
           [(4, s, "sigma") for s in bad_sigmas] + [(5, s, "sigma_p") for s in bad_sigmas])
    torch.cuda.synchronize()
    assert not bool(ws.any())                               # nothing was launched on the workspace
