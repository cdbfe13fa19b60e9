"""GPU: zero-flux (Neumann) sides for the divergence-form operator and its solver (csrc/poisson_div.hip,
csrc/poisson_dst.hip, ABI 22): the boundary-aware apply, step right-hand side and pair gradient against the numpy
restatement of tests/div_bc_ref.py bit for bit, the separable solve and the CG against numpy and dense solves,
poisson.diffuse in the insulated box and with a mixed wall, graph capture, autograd, and the argument checks.
bc=None and bc="dddd" must give today's bits everywhere."""
import functools

import numpy as np
import pytest
import torch

import diffuse_ref as R
import div_bc_ref as BC
import poisson_div_ref as D

pytestmark = pytest.mark.gpu

EDGE_PATTERNS = ("nnnn", "dnnd", "nddd", "ddnd")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forcings(n, B):
    return np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)])


# ---- 1. the operator, the step's right-hand side and the pair gradient, bit for bit ----------------------------------
# 5: one tile; 63 / 64 / 65: the 64-column tile edge (and two 32-row tiles); 70: ragged last tiles in both directions.
# A wrong side shows at edge nodes only, so whole fields are compared exactly.
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 63, 64, 65, 70])
def test_fields_are_bit_equal_to_the_host_restatement(n, mean):
    from superresolution_for_pdes_amd import _lib, poisson as P
    B = 2
    un, ln, fn = D.field_u(n, 0, B), D.field_u(n, 1, B), D.field_u(n, 2, B)
    thn = D.field_theta(n, 0, 0.1, 10.0, B)
    u, f, th = _dev(un), _dev(fn), _dev(thn)
    for bc in EDGE_PATTERNS:
        got = P.apply_div(u, th, face_mean=mean, bc=bc)
        assert got.dtype == torch.float64 and got.shape == (B, n, n)
        assert np.array_equal(got.cpu().numpy(), BC.apply(un, thn, mean, bc)), bc
        got = P.apply_div(u, th, face_mean=mean, shift=7.5, bc=bc)
        assert np.array_equal(got.cpu().numpy(), BC.apply(un, thn, mean, bc, 7.5)), bc
        got = P.apply_div(u, th[1], face_mean=mean, inv_h2=1234.5, shift=1e6, bc=bc)
        assert np.array_equal(got.cpu().numpy(), BC.apply(un, thn[1], mean, bc, 1e6, inv_h2=1234.5)), bc
        for cn, scheme in enumerate(("be", "cn")):
            for fp, fh in ((f.data_ptr(), fn), (0, None)):
                rhs = torch.empty_like(u)
                _lib.call("srpde_div_step_rhs_bc", u.data_ptr(), fp, th.data_ptr(), rhs.data_ptr(), B, n,
                          D.MEANS.index(mean), 7.5, cn, BC.mask(bc), _lib.stream_ptr())
                assert np.array_equal(rhs.cpu().numpy(), BC.step_rhs(un, fh, thn, mean, 7.5, scheme, bc)), (bc, scheme)
        got = P.div_theta_grad(u, ln, th, face_mean=mean, scale=-1.0, bc=bc)
        assert np.array_equal(got.cpu().numpy(), BC.theta_grad(un, ln, thn, mean, bc, scale=-1.0)), bc
    # the masked entries themselves at mask 0 (poisson routes "dddd" away from them): the unmasked entries' bits
    y = torch.empty_like(u)
    _lib.call("srpde_div_apply_bc", u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, D.MEANS.index(mean),
              float((n - 1) ** 2), 7.5, 0, _lib.stream_ptr())
    assert torch.equal(y, P.apply_div(u, th, face_mean=mean, shift=7.5))
    _lib.call("srpde_div_theta_grad_bc", u.data_ptr(), _dev(ln).data_ptr(), th.data_ptr(), y.data_ptr(), B, n,
              D.MEANS.index(mean), float((n - 1) ** 2), 1.0, 0, _lib.stream_ptr())
    assert torch.equal(y, P.div_theta_grad(u, ln, th, face_mean=mean))


# ---- 2. "dddd" is None -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_dddd_and_none_give_equal_tensors(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 40, 3
    f, th, u = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B), D.field_u(n, 0, B)
    for kw in ({}, {"shift": 7.5}):
        assert torch.equal(P.apply_div(u, th, face_mean=mean, bc="dddd", **kw), P.apply_div(u, th, face_mean=mean, **kw))
    for kw in ({}, {"shift": 1e3}, {"u0": u}):
        want = P.solve_div(f, th, face_mean=mean, return_info=True, **kw)
        got = P.solve_div(f, th, face_mean=mean, return_info=True, bc="dddd", **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    for scheme in ("be", "cn"):
        kw = dict(dt=1e-3, steps=3, scheme=scheme, face_mean=mean, check=True)
        want, got = P.diffuse(u, th, f, **kw), P.diffuse(u, th, f, bc="dddd", **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(P.div_theta_grad(u, f, th, face_mean=mean, bc="dddd"), P.div_theta_grad(u, f, th, face_mean=mean))


# ---- 3. the separable solve ------------------------------------------------------------------------------------------
def _sep_shift(f, bc, sigma_p):
    from superresolution_for_pdes_amd import _lib, poisson as P
    B, n = f.shape[0], f.shape[-1]
    u = torch.empty_like(f)
    plan = P.sep_plan(n, bc)
    nbytes = int(_lib.query("srpde_poisson_sep_workspace_size", B, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
    _lib.call("srpde_poisson_sep_shift_batched", f.data_ptr(), u.data_ptr(), B, n, BC.mask(bc), float(sigma_p),
              plan.data_ptr(), plan.numel(), ws.data_ptr(), nbytes, _lib.stream_ptr())
    return u


# 64 / 65 straddle the 64-wide product tile, the last two the LDS limit of the all-Dirichlet path (one path here).
# The bar is test_gpu_diffuse.py::test_shifted_sine_solve's: the same four products and the same scaling.
@pytest.mark.parametrize("n", [5, 40, 64, 65, "lds_max", "lds_max+1"])
def test_separable_solve(n):
    from superresolution_for_pdes_amd import _lib
    lds_max = int(_lib.query("srpde_poisson_dst_lds_max_n"))
    n = {"lds_max": lds_max, "lds_max+1": lds_max + 1}.get(n, n)
    B = 2
    fn = D.field_u(n, 5, B)
    f = _dev(fn)
    for bc in ("nnnn", "dnnd", "ndnn"):
        for sigma_p in (10.0, 1e3, 1e7):
            got = _sep_shift(f, bc, sigma_p).cpu().numpy()
            for b in range(B):
                want = BC.sep_solve(fn[b], bc, sigma_p)
                err = np.linalg.norm(got[b] - want) / np.linalg.norm(want)
                print(f"n={n} {bc} sigma_p={sigma_p:g} b={b}: relative error {err:.3e}")
                assert err <= 1e-11, (n, bc, sigma_p, err)


def test_plan_holds_the_closed_forms():
    """The device reduces its arguments exactly and calls sinpi / cospi; numpy multiplies the reduced argument, up to
    2, by a rounded pi first: an argument error of up to 2 pi * 1.5 eps, so 2.5e-15 on an entry (its scale is below
    1) and, for lam = -4 s^2 with an argument up to pi / 2, 8 * (pi / 2 * 1.5 eps + eps) < 6e-15."""
    from superresolution_for_pdes_amd import poisson as P
    for n in (5, 65):
        for bc in ("dnnd", "ndnn", "nnnn"):
            plan = P.sep_plan(n, bc).view(torch.float64).cpu().numpy()
            Qy, ly, Qx, lx = BC.plan(n, bc)
            nn = n * n
            for k, want in enumerate((Qx, Qx.T, Qy, Qy.T)):
                assert np.abs(plan[k * nn:(k + 1) * nn].reshape(n, n) - want).max() <= 2.5e-15, (n, bc, k)
            assert np.abs(plan[4 * nn:4 * nn + n] - ly).max() <= 6e-15
            assert np.abs(plan[4 * nn + n:4 * nn + 2 * n] - lx).max() <= 6e-15
            assert plan[4 * nn + 2 * n] == BC.mask(bc)
            assert P.sep_plan(n, bc) is P.sep_plan(n, BC.mask(bc))          # cached, by pattern or mask


# ---- 4. the solve against dense solves --------------------------------------------------------------------------------
# rtol 1e-10 and the factor 2 as tests/test_gpu_diffuse.py; the smallest eigenvalue is the dense matrix's own.
SOLVE_RTOL = 1e-10


@functools.lru_cache(maxsize=None)
def _dense_case(n, mean, bc, b):
    th = D.field_theta(n, 0, 0.5, 2.0, 2)[b]
    M = BC.dense(th, mean, bc)
    return M, float(np.linalg.eigvalsh(-M)[0])


@pytest.mark.parametrize("bc", ["nddd", "dnnd", "nnnn"])
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [9, 33])
def test_solve_against_the_dense_reference(n, mean, bc):
    from superresolution_for_pdes_amd import poisson as P
    B = 2
    fn, thn = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    for sigma in (0.0, 10.0, 1e4):
        if bc == "nnnn" and sigma == 0.0:
            continue
        sigma_p = R.precond_shift(thn, sigma)              # over the batch, as precond_shift=None takes it
        u, iters, resid = P.solve_div(fn, thn, face_mean=mean, rtol=SOLVE_RTOL, return_info=True, shift=sigma, bc=bc)
        routed = P.solve_batched(fn, thn, rtol=SOLVE_RTOL, form="divergence", face_mean=mean, shift=sigma, bc=bc,
                                 return_iters=True)
        assert torch.equal(routed[0], u) and torch.equal(routed[1], iters)
        assert bool((resid <= SOLVE_RTOL).all())
        for b in range(B):
            M, lam_min = _dense_case(n, mean, bc, b)
            A = M.copy()
            A[np.diag_indices_from(A)] -= sigma
            want = np.linalg.solve(A, fn[b].reshape(-1)).reshape(n, n)
            err = np.linalg.norm(u[b].cpu().numpy() - want)
            bound = 2.0 * SOLVE_RTOL * np.linalg.norm(fn[b]) / (max(lam_min, 0.0) + sigma)
            k_ref = BC.pcg(fn[b], thn[b], mean, bc, sigma, sigma_p, rtol=SOLVE_RTOL)[1]
            print(f"n={n} {mean} {bc} sigma={sigma:g} b={b}: err {err:.3e} bound {bound:.3e} iters {int(iters[b])} "
                  f"ref {k_ref}")
            assert err <= bound
            assert int(iters[b]) == k_ref
            assert int(iters[b]) <= P.pcg_iterations(0.5, 2.0, SOLVE_RTOL)
        # the true residual through residual_metrics(bc=): D u - (f + sigma u), RMS = |r| / n, one rtol spare as above
        res = P.residual_metrics(u, fn + sigma * u.cpu().numpy(), thn, form="divergence", face_mean=mean, bc=bc)
        for b in range(B):
            assert float(res[b, 0]) <= 2.0 * SOLVE_RTOL * np.linalg.norm(fn[b]) / n


# ---- 5. batch independence and the warm start ---------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["dnnd", "nnnn"])
def test_solve_does_not_depend_on_the_batch(bc):
    from superresolution_for_pdes_amd import poisson as P
    n, B, sigma = 70, 3, 1e3
    f, th = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    sigma_p = R.precond_shift(th, sigma)                   # one sigma_p for both calls: it is an input
    whole = P.solve_div(f, th, return_info=True, shift=sigma, precond_shift=sigma_p, bc=bc)
    one = P.solve_div(f[1], th[1], return_info=True, shift=sigma, precond_shift=sigma_p, bc=bc)
    assert torch.equal(one[0][0], whole[0][1])
    assert int(one[1][0]) == int(whole[1][1]) and float(one[2][0]) == float(whole[2][1])


@pytest.mark.parametrize("bc,sigma", [("nddd", 0.0), ("nnnn", 1e3)])
def test_warm_start(bc, sigma):
    from superresolution_for_pdes_amd import poisson as P
    n, B, rtol = 40, 3, 1e-10
    f, th = _forcings(n, B), D.field_theta(n, 0, 0.5, 2.0, B)
    zero = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc)
    got = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc, u0=np.zeros((n, n)))
    assert all(torch.equal(g, w) for g, w in zip(got, zero))
    assert int(zero[1].min()) >= 1
    tight = P.solve_div(f, th, rtol=1e-13, shift=sigma, bc=bc)
    u, iters, resid = P.solve_div(f, th, rtol=rtol, return_info=True, shift=sigma, bc=bc, u0=tight)
    assert iters.tolist() == [0, 0, 0] and torch.equal(u, tight) and bool((resid <= rtol).all())


# ---- 6. the insulated box and a mixed wall -----------------------------------------------------------------------------
def test_insulated_box_conserves_and_flattens():
    """10 backward-Euler steps with four zero-flux sides and no forcing: the sum of u is conserved within the bound
    of div_bc_ref.conservation_bound (which tests/test_div_bc_host.py holds the numpy reference to), and the range of
    u shrinks at every step."""
    from superresolution_for_pdes_amd import poisson as P
    n, dt, rtol, steps = BC.BOX_N, BC.BOX_DT, BC.BOX_RTOL, BC.BOX_STEPS
    u0, th = BC.box_case()
    sigma = 1.0 / dt
    u, frames, counts = P.diffuse(u0, th, dt=dt, steps=steps, rtol=rtol, bc="nnnn", save_every=1, check=True)
    assert frames.shape == (steps, 1, n, n) and torch.equal(frames[-1], u)
    prev = u0
    for s in range(steps):
        new = frames[s, 0].cpu().numpy()
        rhs = BC.step_rhs(prev, None, th, "harmonic", sigma, "be", "nnnn")
        drift, bound = abs(new.sum() - prev.sum()), BC.conservation_bound(n, rtol, rhs, sigma, prev)
        print(f"step {s}: drift {drift:.3e} bound {bound:.3e} range {new.max() - new.min():.6f} "
              f"iters {int(counts[s, 0])}")
        assert drift <= bound
        assert new.max() - new.min() < prev.max() - prev.min()
        prev = new
    # the all-Dirichlet box loses mass through its walls instead: the pattern really reached the solve
    lost = P.diffuse(u0 + 1.0, th, dt=dt, steps=steps, rtol=rtol)
    assert (u0 + 1.0).sum() - float(lost.sum()) > 1.0


@pytest.mark.parametrize("scheme", ["be", "cn"])
def test_mixed_wall_eigenmode_decay(scheme):
    from superresolution_for_pdes_amd import poisson as P
    n, dt, steps, bc = 33, 1e-3, 5, "ddnn"
    v0, mu0 = BC.eigenmode(n, bc, 0, 0)                    # constant along the rows' direction, half a sine across
    v1, mu1 = BC.eigenmode(n, bc, 2, 5)
    u, frames = P.diffuse(np.stack([v0, v1]), np.ones((n, n)), dt=dt, steps=steps, scheme=scheme, bc=bc, save_every=1)
    for b, (v, mu) in enumerate(((v0, mu0), (v1, mu1))):
        g = R.decay_factor(dt, 1.0, mu, scheme)
        for s in range(steps):
            err = np.abs(frames[s, b].cpu().numpy() - g ** (s + 1) * v).max()
            assert err <= 1e-10 * np.abs(v).max(), (b, s, err)


# ---- 7. graph capture --------------------------------------------------------------------------------------------------
def test_fixed_mode_under_graph_capture():
    from superresolution_for_pdes_amd import poisson as P
    n, B, dt, steps, bc = 20, 3, 1e-3, 5, "nnnn"
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B))
    f, u0 = _dev(_forcings(n, B)), _dev(D.field_u(n, 8, B))
    k = P.pcg_iterations(0.5, 2.0) + 4
    sigma_p = (1.0 / dt) / float(np.sqrt(0.5 * 2.0))
    kw = dict(dt=dt, steps=steps, pcg_iters=k, precond_shift=sigma_p, save_every=5, check=True, bc=bc)
    P.sep_plan(n, bc)
    eager = P.diffuse(u0, th, f, **kw)
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


# ---- 8. autograd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc,sigma", [("nddd", 0.0), ("nnnn", 7.5)])
@pytest.mark.parametrize("mean", D.MEANS)
def test_gradcheck(mean, bc, sigma):
    """Tolerances as tests/test_gpu_div_adjoint.py: rtol=1e-13 keeps the solve's noise under gradcheck's atol."""
    from superresolution_for_pdes_amd import poisson as P
    n, B = 6, 2
    u = _dev(D.field_u(n, 0, B)).requires_grad_(True)
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, t: P.apply_div(a, t, face_mean=mean, shift=sigma, bc=bc), (u, th))
    f = _dev(np.stack([D.forcing(n), D.field_u(n, 4)])).requires_grad_(True)
    # sigma_p is an input of the solve: fixed, so the perturbed solves share it
    pshift = 7.0 if sigma else None
    assert torch.autograd.gradcheck(
        lambda a, t: P.solve_div(a, t, face_mean=mean, rtol=1e-13, shift=sigma, precond_shift=pshift, bc=bc), (f, th))


@pytest.mark.parametrize("scheme", ["be", "cn"])
@pytest.mark.parametrize("mean", D.MEANS)
def test_theta_gradient_through_two_steps(mean, scheme):
    """As tests/test_gpu_diffuse.py::test_theta_gradient_through_two_steps, in the insulated box."""
    from superresolution_for_pdes_amd import poisson as P
    n, dt, bc = 5, 5e-2, "nnnn"
    u0, fn, thn, w = D.field_u(n, 9), D.forcing(n), D.field_theta(n, 5, 0.5, 2.0), D.field_u(n, 10)
    th = _dev(thn).requires_grad_(True)
    u = P.diffuse(u0, th, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13, bc=bc)
    assert u.grad_fn is not None
    ((u[0] * _dev(w)).sum()).backward()
    eps = 1e-6
    want = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            d = np.zeros((n, n))
            d[i, j] = eps
            lp = np.sum(w * BC.diffuse_dense(u0, thn + d, fn, dt, 2, scheme, mean, bc))
            lm = np.sum(w * BC.diffuse_dense(u0, thn - d, fn, dt, 2, scheme, mean, bc))
            want[i, j] = (lp - lm) / (2.0 * eps)
    err = np.linalg.norm(th.grad.cpu().numpy() - want) / np.linalg.norm(want)
    print(f"{scheme} {mean}: relative error {err:.3e}")
    assert err <= 1e-6
    plain = P.diffuse(u0, thn, fn, dt=dt, steps=2, scheme=scheme, face_mean=mean, rtol=1e-13, bc=bc)
    assert plain.grad_fn is None and float((plain - u.detach()).norm() / plain.norm()) <= 1e-12


# ---- 9. argument errors ------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    from superresolution_for_pdes_amd import poisson as P
    n = 8
    f, th = _dev(D.forcing(n)), _dev(D.field_theta(n, 0, 0.5, 2.0))
    for bad in ("ddn", "dxnd", "NNNN", 3):
        for fn in (P.apply_div, P.solve_div):
            with pytest.raises(ValueError, match="bc"):
                fn(f, th, bc=bad)
        with pytest.raises(ValueError, match="bc"):
            P.diffuse(f, th, dt=1e-2, bc=bad)
        with pytest.raises(ValueError, match="bc"):
            P.div_theta_grad(f, f, th, bc=bad)
    with pytest.raises(ValueError, match="singular"):
        P.solve_div(f, th, bc="nnnn")
    with pytest.raises(ValueError, match="singular"):
        P.solve_batched(f, th, form="divergence", bc="nnnn")
    with pytest.raises(ValueError, match="precond_shift"):
        P.solve_div(f, th, bc="nnnn", shift=10.0, precond_shift=0.0)
    with pytest.raises(ValueError, match="divergence"):
        P.solve_batched(f, th, bc="ddnn")
    with pytest.raises(ValueError, match="divergence"):
        P.solve_batched(f, th, bc="ddnn", method="dst")
    with pytest.raises(ValueError, match="divergence"):
        P.residual_metrics(f, f, th, bc="ddnn")
    with pytest.raises(ValueError, match="precond_shift"):
        P.solve_div(f, th, shift=10.0, maxit=10, check_every=0, bc="ddnn")
    with pytest.raises(ValueError, match="precond_shift"):
        P.diffuse(f, th, dt=1e-2, pcg_iters=10, bc="nnnn")


def test_library_argument_errors():
    """Each bad argument returns the error before any launch: the outputs and the workspace keep their bytes."""
    from superresolution_for_pdes_amd import _lib, poisson as P
    n, B = 8, 2
    N = B * n * n
    buf = torch.randn(4, N + 1, dtype=torch.float64, device="cuda")
    u, f, th, y = (buf[i, :N] for i in range(4))
    th.abs_().add_(0.5)
    y.fill_(-7.0)
    off = [buf.view(torch.float32)[i, 1:].data_ptr() for i in range(4)]       # offset by 4 bytes
    sp = _lib.stream_ptr()
    plan, other, box = P.sep_plan(n, "ddnn"), P.sep_plan(n, "nddd"), P.sep_plan(n, "nnnn")
    nbytes = int(_lib.query("srpde_div_cg_workspace_size_bc", B, n))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    m = BC.mask("ddnn")
    tail = (plan.data_ptr(), plan.numel(), ws.data_ptr(), nbytes, sp)

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

    masks = [(-1, "bc"), (16, "bc")]
    ok = (u.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, float((n - 1) ** 2), 7.5, m, sp)
    refuse("srpde_div_apply_bc", ok,
           [(i, 0, "null") for i in range(3)] + [(i, off[i], "aligned") for i in range(3)] +
           [(2, ok[0], "alias"), (5, 2, "face_mean"), (6, 0.0, "inv_h2"), (3, 0, "shape"), (7, -1.0, "sigma")] +
           [(8, v, mt) for v, mt in masks])
    ok = (u.data_ptr(), f.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, 7.5, 1, m, sp)
    refuse("srpde_div_step_rhs_bc", ok,
           [(i, 0, "null") for i in (0, 2, 3)] + [(3, ok[0], "alias"), (8, 2, "cn"), (7, float("nan"), "sigma")] +
           [(9, v, mt) for v, mt in masks])
    ok = (u.data_ptr(), f.data_ptr(), th.data_ptr(), y.data_ptr(), B, n, 1, float((n - 1) ** 2), 1.0, m, sp)
    refuse("srpde_div_theta_grad_bc", ok,
           [(i, 0, "null") for i in range(4)] + [(3, ok[2], "alias"), (8, float("inf"), "scale")] +
           [(9, v, mt) for v, mt in masks])
    sws = torch.zeros(N * 8, dtype=torch.uint8, device="cuda")
    ok = (f.data_ptr(), y.data_ptr(), B, n, m, 7.5, plan.data_ptr(), plan.numel(), sws.data_ptr(), N * 8, sp)
    refuse("srpde_poisson_sep_shift_batched", ok,
           [(0, 0, "null"), (1, 0, "null"), (6, 0, "null"), (8, 0, "null"), (1, ok[0], "alias"), (3, 1, "shape"),
            (5, -1.0, "sigma_p"), (9, N * 8 - 16, "workspace"),
            ((6, 7), (other.data_ptr(), other.numel()), "plan"),                  # a plan built for another mask
            ((4, 5, 6, 7), (15, 0.0, box.data_ptr(), box.numel()), "singular")] +
           [(4, v, mt) for v, mt in masks])
    refuse("srpde_poisson_sep_plan", (n, m, plan.data_ptr(), plan.numel(), sp),
           [(2, 0, "null"), (0, 1, "shape"), (3, plan.numel() - 8, "plan"), (1, 16, "bc"), (1, -1, "bc")])
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and not bool(sws.any())

    ok = (f.data_ptr(), B, n, m, 7.5) + tail
    refuse("srpde_div_cg_init_bc", ok,
           [(0, 0, "null"), (0, off[1], "aligned"), (8, nbytes - 16, "workspace"), (4, -1.0, "sigma_p"),
            ((5, 6), (other.data_ptr(), other.numel()), "plan"),
            ((3, 4, 5, 6), (15, 0.0, box.data_ptr(), box.numel()), "singular")] + [(3, v, mt) for v, mt in masks])
    ok = (f.data_ptr(), u.data_ptr(), th.data_ptr(), B, n, 1, m, 7.5, 7.0, 1e-10) + tail
    refuse("srpde_div_cg_init_from_bc", ok,
           [(i, 0, "null") for i in range(3)] + [(5, 2, "face_mean"), (9, -1e-10, "rtol"),
                                                 (13, nbytes - 16, "workspace"),
                                                 ((10, 11), (other.data_ptr(), other.numel()), "plan"),
                                                 ((6, 7, 10, 11), (15, 0.0, box.data_ptr(), box.numel()), "singular"),
                                                 ((6, 8, 10, 11), (15, 0.0, box.data_ptr(), box.numel()), "singular")] +
           [(6, v, mt) for v, mt in masks])
    ok = (th.data_ptr(), B, n, 1, m, 7.5, 7.0, 1e-10, 1, 2) + tail
    refuse("srpde_div_cg_iterate_bc", ok,
           [(0, 0, "null"), (3, 2, "face_mean"), (7, float("nan"), "rtol"), (8, 0, "k_begin"),
            (13, nbytes - 16, "workspace"), ((10, 11), (other.data_ptr(), other.numel()), "plan"),
            ((4, 5, 10, 11), (15, 0.0, box.data_ptr(), box.numel()), "singular")] + [(4, v, mt) for v, mt in masks])
    torch.cuda.synchronize()
    assert not bool(ws.any())                               # nothing was launched on the workspace
