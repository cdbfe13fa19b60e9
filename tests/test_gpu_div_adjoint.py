"""GPU: the adjoint of the divergence-form operator and the warm-started CG (csrc/poisson_div.hip, ABI 20):
srpde_div_theta_grad against the numpy restatement of tests/div_adjoint_ref.py bit for bit, autograd through
poisson.apply_div / solve_div, and srpde_div_cg_init_from through solve_div(u0=...)."""
import numpy as np
import pytest
import torch

import div_adjoint_ref as A
import poisson_div_ref as D

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the kernel ------------------------------------------------------------------------------------------
# n = 2: ghost and single faces only; 3: one interior node; 33 crosses a tile edge in y (32 rows), 65 one in x (64
# columns), 70 both with ragged last tiles
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [2, 3, 33, 65, 70])
def test_theta_grad_is_bit_equal_to_the_host_restatement(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    B = 3
    u, lam = D.field_u(n, 0, B), D.field_u(n, 1, B)
    th = D.field_theta(n, 0, 0.1, 10.0, B)
    for scale in (1.0, -1.0):
        got = P.div_theta_grad(u, lam, th, face_mean=mean, scale=scale)
        assert got.dtype == torch.float64 and got.shape == (B, n, n) and got.grad_fn is None
        assert np.array_equal(got.cpu().numpy(), A.theta_grad(u, lam, th, mean, scale=scale))
    # another inv_h2, a 2-D call and a broadcast theta
    got = P.div_theta_grad(u[0], lam[0], th[0], face_mean=mean, inv_h2=1234.5, scale=0.25)
    assert np.array_equal(got.cpu().numpy()[0], A.theta_grad(u[0], lam[0], th[0], mean, inv_h2=1234.5, scale=0.25))
    got = P.div_theta_grad(u, lam, th[1], face_mean=mean)
    assert np.array_equal(got.cpu().numpy(), A.theta_grad(u, lam, th[1], mean))


@pytest.mark.parametrize("mean", D.MEANS)
def test_theta_grad_does_not_depend_on_the_batch(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 70, 5
    u, lam, th = D.field_u(n, 2, B), D.field_u(n, 3, B), D.field_theta(n, 1, 0.1, 10.0, B)
    whole = P.div_theta_grad(u, lam, th, face_mean=mean)
    for b in range(B):
        assert torch.equal(P.div_theta_grad(u[b], lam[b], th[b], face_mean=mean)[0], whole[b]), b


def test_theta_grad_argument_errors():
    """Each bad argument returns the error before any launch: g_out keeps its bytes."""
    from superresolution_for_pdes_amd import _lib
    n, B = 8, 2
    buf = torch.randn(4, B * n * n + 1, dtype=torch.float64, device="cuda")
    u, lam, th, g = (buf[i, :B * n * n] for i in range(4))
    th.abs_().add_(0.5)
    g.fill_(-7.0)
    sp = _lib.stream_ptr()
    ok = (u.data_ptr(), lam.data_ptr(), th.data_ptr(), g.data_ptr(), B, n, 1, float((n - 1) ** 2), 1.0, sp)

    def bad(match, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=match):
            _lib.call("srpde_div_theta_grad", *args)

    for i in range(4):
        bad("null", **{f"a{i}": 0})
    for i in range(3):
        bad("alias", a3=ok[i])
    off4 = buf.view(torch.float32)                       # a view offset by 4 bytes
    for i in range(4):
        bad("aligned", **{f"a{i}": off4[i, 1:].data_ptr()})
    for fm in (-1, 2):
        bad("face_mean", a6=fm)
    for v in (0.0, -1.0, float("inf"), float("nan")):
        bad("inv_h2", a7=v)
    bad("scale", a8=float("nan"))
    bad("shape", a4=0)
    bad("shape", a5=1)
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())
    _lib.call("srpde_div_theta_grad", *ok)
    assert np.array_equal(g.reshape(B, n, n).cpu().numpy(),
                          A.theta_grad(u.reshape(B, n, n).cpu().numpy(), lam.reshape(B, n, n).cpu().numpy(),
                                       th.reshape(B, n, n).cpu().numpy(), "harmonic"))


def test_init_from_argument_errors():
    from superresolution_for_pdes_amd import _lib, poisson as P
    n, B = 8, 2
    f = torch.randn(B, n, n, dtype=torch.float64, device="cuda")
    plan = P.dst_plan(n)
    nbytes = int(_lib.query("srpde_div_cg_workspace_size", B, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ok = (f.data_ptr(), f.data_ptr(), f.data_ptr(), B, n, 1, 1e-10, plan.data_ptr(), plan.numel(), ws.data_ptr(),
          nbytes, _lib.stream_ptr())
    for i, v, match in ((1, 0, "null"), (2, 0, "null"), (1, f.data_ptr() + 4, "aligned"),
                        (2, f.data_ptr() + 4, "aligned"), (6, -1e-10, "rtol"), (6, float("nan"), "rtol"),
                        (5, 2, "face_mean"), (10, nbytes - 16, "workspace")):
        args = list(ok)
        args[i] = v
        with pytest.raises(RuntimeError, match=match):
            _lib.call("srpde_div_cg_init_from", *args)


# ---- 2. autograd --------------------------------------------------------------------------------------------
def _leaves(n, B, seed, f_like):
    a = _dev(f_like).requires_grad_(True)
    th = _dev(D.field_theta(n, seed, 0.5, 2.0, B)).requires_grad_(True)
    return a, th


@pytest.mark.parametrize("mean", D.MEANS)
def test_gradcheck_apply_div(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 5, 2
    u, th = _leaves(n, B, 0, D.field_u(n, 0, B))
    assert torch.autograd.gradcheck(lambda a, t: P.apply_div(a, t, face_mean=mean), (u, th))
    assert torch.autograd.gradcheck(lambda a, t: P.apply_div(a, t, face_mean=mean, inv_h2=3.5), (u, th))


@pytest.mark.parametrize("mean", D.MEANS)
def test_gradcheck_solve_div(mean):
    """Default tolerances (atol 1e-5, rtol 1e-3, step 1e-6).  A solution good to ~1e-12 under a finite-difference
    step of 1e-6 puts ~1e-6 of noise into the numerical Jacobian, against the atol of 1e-5: hence rtol=1e-13 here."""
    from superresolution_for_pdes_amd import poisson as P
    n, B = 5, 2
    f, th = _leaves(n, B, 1, np.stack([D.forcing(n), D.field_u(n, 4)]))
    assert torch.autograd.gradcheck(lambda a, t: P.solve_div(a, t, face_mean=mean, rtol=1e-13), (f, th))
    # with return_info only u is differentiable, and a warm start changes no gradient
    u, iters, resid = P.solve_div(f, th, face_mean=mean, rtol=1e-13, return_info=True)
    assert u.requires_grad and not iters.requires_grad and not resid.requires_grad
    u0 = u.detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, t: P.solve_div(a, t, face_mean=mean, rtol=1e-13, u0=u0 * 0.99), (f, th))
    P.solve_div(f, th, face_mean=mean, u0=u0).sum().backward()
    assert u0.grad is None


@pytest.mark.parametrize("mean", D.MEANS)
def test_gradients_against_the_host_restatement(mean):
    """The same gradients at a size with more than one tile, against numpy: grad_u = D w and grad_theta = -G(u, w)
    bit for bit; the solve's against G of the dense adjoint solve."""
    from superresolution_for_pdes_amd import poisson as P
    n, B = 33, 2
    un, wn, thn = D.field_u(n, 0, B), D.field_u(n, 1, B), D.field_theta(n, 0, 0.5, 2.0, B)
    u, th, w = _dev(un).requires_grad_(True), _dev(thn).requires_grad_(True), _dev(wn)
    gu, gth = torch.autograd.grad(P.apply_div(u, th, face_mean=mean), (u, th), w)
    assert np.array_equal(gu.cpu().numpy(), D.apply(wn, thn, mean))
    assert np.array_equal(gth.cpu().numpy(), A.theta_grad(un, wn, thn, mean, scale=-1.0))
    fn = np.stack([D.forcing(n), D.forcing(n, 2.3, 1.1)])
    f = _dev(fn).requires_grad_(True)
    gf, gth = torch.autograd.grad(P.solve_div(f, th, face_mean=mean), (f, th), w)
    # the CG solutions are held to 1e-10 of the dense ones (tests/test_gpu_poisson_div.py; measured ~1e-12): 1e-9
    # for lam leaves a factor of 10, and G, bilinear in the differences of u and lam, another 10
    for b in range(B):
        lam, sol = D.solve_dense(wn[b], thn[b], mean), D.solve_dense(fn[b], thn[b], mean)
        want = A.theta_grad(sol, lam, thn[b], mean)
        assert np.linalg.norm(gf[b].cpu().numpy() - lam) <= 1e-9 * np.linalg.norm(lam)
        assert np.linalg.norm(gth[b].cpu().numpy() - want) <= 1e-8 * np.linalg.norm(want)


def test_broadcast_theta_and_float32_leaves():
    from superresolution_for_pdes_amd import poisson as P
    n, B = 9, 3
    f = _dev(np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)]))
    w = _dev(D.field_u(n, 5, B))
    th2 = _dev(D.field_theta(n, 2, 0.5, 2.0)).requires_grad_(True)
    th3 = th2.detach().expand(B, n, n).clone().requires_grad_(True)
    for fun in (P.solve_div, P.apply_div):
        (g2,) = torch.autograd.grad(fun(f, th2), th2, w)
        (g3,) = torch.autograd.grad(fun(f, th3), th3, w)
        assert g2.shape == (n, n) and g3.shape == (B, n, n)
        # the same per-problem bits, summed over B by autograd in one case and here in the other
        assert float((g2 - g3.sum(0)).norm() / g2.norm()) < 1e-14
    # a float32 leaf gets a float32 gradient, a 2-D field a 2-D one
    f32 = f[0].float().requires_grad_(True)
    t32 = th2.detach().float().requires_grad_(True)
    out = P.solve_div(f32, t32)
    assert out.dtype == torch.float64 and out.shape == (1, n, n)
    out.sum().backward()
    assert f32.grad.dtype == torch.float32 and f32.grad.shape == (n, n)
    assert t32.grad.dtype == torch.float32 and t32.grad.shape == (n, n)
    # residual_metrics(form="divergence") goes through apply_div
    u = P.solve_div(f, th3.detach()).mul(1.01).requires_grad_(True)
    P.residual_metrics(u, f, th3.detach(), form="divergence")[:, 0].sum().backward()
    assert u.grad is not None and bool(torch.isfinite(u.grad).all()) and float(u.grad.abs().max()) > 0.0


@pytest.mark.parametrize("mean", D.MEANS)
def test_without_grad_nothing_changes(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 33, 2
    f = _dev(np.stack([D.forcing(n), D.forcing(n, 2.3, 1.1)]))
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B))
    fg, tg = f.clone().requires_grad_(True), th.clone().requires_grad_(True)
    y, sol = P.apply_div(fg, tg, face_mean=mean), P.solve_div(fg, tg, face_mean=mean, return_info=True)
    assert y.grad_fn is not None and sol[0].grad_fn is not None
    plain = P.apply_div(f, th, face_mean=mean), P.solve_div(f, th, face_mean=mean, return_info=True)
    with torch.no_grad():
        quiet = P.apply_div(fg, tg, face_mean=mean), P.solve_div(fg, tg, face_mean=mean, return_info=True)
    for ya, sa in (plain, quiet):
        assert ya.grad_fn is None and all(t.grad_fn is None and not t.requires_grad for t in sa)
        assert torch.equal(ya, y.detach())
        assert all(torch.equal(a, b.detach()) for a, b in zip(sa, sol))


def test_not_converged_in_the_backward():
    from superresolution_for_pdes_amd import poisson as P
    n = 20
    f = torch.zeros(n, n, dtype=torch.float64, device="cuda", requires_grad=True)
    th = _dev(D.field_theta(n, 4, 0.1, 10.0))
    u = P.solve_div(f, th, maxit=1)                      # f = 0 is done at once; one iteration cannot solve for grad_u
    assert u.grad_fn is not None and not bool(u.any())
    with pytest.raises(P.NotConverged):
        u.backward(_dev(D.field_u(n, 6)).unsqueeze(0))


# ---- 3. the warm start --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [40, 70])
def test_zero_u0_gives_the_zero_start_bits(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    B = 4
    f = np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)])
    f[3] = 0.0
    th = D.field_theta(n, 0, 0.5, 2.0, B)
    want = P.solve_div(f, th, face_mean=mean, return_info=True)
    got = P.solve_div(f, th, face_mean=mean, return_info=True, u0=np.zeros((n, n)))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert int(want[1][3]) == 0 and int(want[1][:3].min()) >= 1
    # |f| = 0 gives u = 0 whatever u0 is
    got = P.solve_div(f, th, face_mean=mean, return_info=True, u0=D.field_u(n, 0, B))
    assert not bool(got[0][3].any()) and int(got[1][3]) == 0 and float(got[2][3]) == 0.0


@pytest.fixture(scope="module")
def warm():
    cases = [A.warm_case(s) for s in A.WARM_SEEDS]
    return tuple(np.stack([c[i] for c in cases]) for i in range(3))


@pytest.mark.parametrize("mean", D.MEANS)
def test_warm_start_saves_iterations_within_the_bound(warm, mean):
    from superresolution_for_pdes_amd import poisson as P
    f, th, near = warm
    n, rtol = A.WARM_N, A.WARM_RTOL
    # an exact start costs nothing
    tight = P.solve_div(f, th, face_mean=mean, rtol=1e-13)
    u, iters, resid = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, u0=tight)
    assert iters.tolist() == [0] * len(f) and bool((resid <= rtol).all()) and torch.equal(u, tight)
    u, iters, _ = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, u0=tight, check_every=0, maxit=5)
    assert iters.tolist() == [0] * len(f) and torch.equal(u, tight)
    # a nearby start (theta off by 1 %) costs less than a zero start, on every problem
    u_near = P.solve_div(f, near, face_mean=mean, rtol=rtol)
    u_zero, it_zero, _ = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True)
    u_warm, it_warm, r_warm = P.solve_batched(f, th, rtol=rtol, form="divergence", face_mean=mean, u0=u_near,
                                              return_iters=True) + (None,)
    u_ws, it_ws, r_ws = P.solve_div(f, th, face_mean=mean, rtol=rtol, return_info=True, u0=u_near)
    assert torch.equal(u_warm, u_ws) and torch.equal(it_warm, it_ws)
    print(f"{mean}: zero start {it_zero.tolist()}, warm start {it_ws.tolist()}")
    assert bool((it_ws < it_zero).all()) and bool((it_ws > 0).all()) and bool((r_ws <= rtol).all())
    # both residuals are <= rtol |f| and lambda_min(-D_theta) >= theta_min lambda_min(-L)
    diff = (u_ws - u_zero).flatten(1).norm(dim=1).cpu().numpy()
    bound = 2.0 * rtol * np.linalg.norm(f.reshape(len(f), -1), axis=1) / (
        th.reshape(len(f), -1).min(axis=1) * A.lambda_min_neg_laplacian(n))
    print(f"{mean}: |u_ws - u_0| {diff}, bound {bound}")
    assert np.all(diff <= bound)
    # a problem's warm-started result does not depend on the batch
    one = P.solve_div(f[2], th[2], face_mean=mean, rtol=rtol, return_info=True, u0=u_near[2])
    assert torch.equal(one[0][0], u_ws[2]) and int(one[1][0]) == int(it_ws[2]) and float(one[2][0]) == float(r_ws[2])


def test_warm_start_under_graph_capture():
    from superresolution_for_pdes_amd import poisson as P
    n, B = 20, 4
    thn = D.field_theta(n, 0, 0.5, 2.0, B)
    th = _dev(thn)
    f = _dev(np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)]))
    u0 = P.solve_div(f, _dev(thn * 1.01 + 0.01 * D.field_theta(n, 1, 0.0, 1.0, B)), rtol=1e-10)
    P.dst_plan(n)
    eager = P.solve_div(f, th, maxit=30, check_every=0, return_info=True, u0=u0)
    assert bool((eager[2] <= 1e-12).all())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # every launch goes to the one capturing stream: a linear chain, no branches
        out = P.solve_div(f, th, maxit=30, check_every=0, check=False, return_info=True, u0=u0)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


def test_u0_is_refused_where_it_means_nothing():
    from superresolution_for_pdes_amd import poisson as P
    n = 8
    f, th = D.forcing(n), D.field_theta(n, 0, 0.5, 2.0)
    u0 = np.zeros((n, n))
    with pytest.raises(ValueError, match="u0"):
        P.solve_batched(f, th, u0=u0)
    with pytest.raises(ValueError, match="u0"):
        P.solve_batched(f, th, method="dst", u0=u0)
    with pytest.raises(ValueError):
        P.solve_batched(f, th, form="divergence", method="dst", u0=u0)
