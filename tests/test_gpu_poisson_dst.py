"""The direct sine-transform Poisson solver (csrc/poisson_dst.hip, ABI 13; poisson.solve_direct / dst2 /
solve_batched(method="dst")) against numpy, the spsolve fixtures of test_gpu_poisson.py, the oracle and the CG.

Bars: the project's own (relative L2 vs spsolve < 1e-10, 640^2 row / column < 1e-9, residual < 1e-9); for the
plan 4e-15 absolute (entries below 1, a few ulp on each side); for the transform 1e-13 relative (n eps is
3e-14 at n = 129; a wrong MFMA lane map gives O(1)).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def sine_matrix(n):
    """S and lam on the host with the kernel's integer argument reduction, m = (j + 1)(k + 1) mod 2 (n + 1),
    folded on to [0, (n + 1) / 2] (sin(pi (1 + x)) = -sin(pi x), sin(pi (1 - x)) = sin(pi x)) so that the
    argument of np.sin stays below pi / 2."""
    j = np.arange(1, n + 1, dtype=np.int64)
    m = (j[:, None] * j[None, :]) % (2 * (n + 1))
    sign = np.where(m >= n + 1, -1.0, 1.0)
    m = np.where(m >= n + 1, m - (n + 1), m)
    m = np.where(2 * m > n + 1, (n + 1) - m, m)
    S = np.sqrt(2.0 / (n + 1)) * sign * np.sin(np.pi * (m / (n + 1)))
    lam = -4.0 * np.sin(np.pi * (j / (2.0 * (n + 1)))) ** 2
    return S, lam


def plan_arrays(n):
    from superresolution_for_pdes_amd import poisson as P
    p = P.dst_plan(n).view(torch.float64).cpu().numpy()
    assert p.size == n * n + n
    return p[:n * n].reshape(n, n), p[n * n:]


@pytest.mark.parametrize("n", [5, 20, 33, 640])
def test_plan_matches_numpy(n):
    S, lam = plan_arrays(n)
    S0, lam0 = sine_matrix(n)
    es, el = float(np.max(np.abs(S - S0))), float(np.max(np.abs(lam - lam0)))
    print(f"n={n}: max|S - S0| = {es:.3e}, max|lam - lam0| = {el:.3e}")
    assert es <= 4e-15 and el <= 4e-15
    eo = float(np.max(np.abs(S @ S - np.eye(n))))
    print(f"n={n}: max|S S - I| = {eo:.3e}")
    assert eo <= 1e-14


@pytest.mark.parametrize("B,n", [(1, 5), (3, 17), (2, 33), (2, 129)])
def test_dst2_matches_numpy(B, n):
    """(an unsymmetric x: a transposed store or a swapped operand does not pass)"""
    from superresolution_for_pdes_amd import poisson as P
    x = np.random.default_rng(100 * B + n).standard_normal((B, n, n))
    S0, _ = sine_matrix(n)
    y = P.dst2(x)
    e1 = rel(y.cpu().numpy(), S0 @ x @ S0)
    e2 = rel(P.dst2(y).cpu().numpy(), x)
    print(f"B={B} n={n}: dst2 {e1:.3e}, dst2(dst2) {e2:.3e}")
    assert e1 <= 1e-13 and e2 <= 1e-13
    assert P.dst2(x[0]).shape == (n, n)


@pytest.mark.parametrize("n", [20, 40, 80, 160])
def test_matches_spsolve_fixture(golden, n):
    from superresolution_for_pdes_amd import poisson as P
    z = golden["poisson"]
    f = z[f"f{n}"]
    th = np.stack([np.ones((n, n)), z[f"thv{n}"]])
    u = P.solve_direct(np.stack([f, f]), th).cpu().numpy()
    e1, ev = rel(u[0], z[f"u1_{n}"]), rel(u[1], z[f"uv_{n}"])
    print(f"n={n}: theta=1 {e1:.3e}, theta variable {ev:.3e}")
    assert e1 < 1e-10 and ev < 1e-10


def test_640_matches_spsolve_stats(golden):
    from superresolution_for_pdes_amd import poisson as P
    z = golden["poisson"]
    n = 640
    f = P.forcing_batched(np.array([[10.25, 10.75]]), n)
    thv = np.random.default_rng(640).uniform(0.5, 2.0, (n, n))
    u = P.solve_batched(f, thv, method="dst")[0].cpu().numpy()
    en = abs(np.linalg.norm(u) - float(z["u640_norm"])) / float(z["u640_norm"])
    er, ec = rel(u[320], z["u640_row320"]), rel(u[:, 100], z["u640_col100"])
    print(f"640: norm {en:.3e}, row 320 {er:.3e}, column 100 {ec:.3e}")
    assert en < 1e-10 and er < 1e-9 and ec < 1e-9


def _shapes():
    return [(1, 5), (3, 17), (5, 200), (2, 345), (2, "lds_max"), (2, "lds_max+1")]


@pytest.mark.parametrize("B,n", _shapes())
def test_odd_shapes_against_oracle(B, n):
    """Sizes that are no multiple of 16 or 4 on both paths, and the two sizes either side of the path switch."""
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd._lib import query
    from oracle import poisson_ref as R
    if isinstance(n, str):
        n = int(query("srpde_poisson_dst_lds_max_n")) + (1 if n.endswith("+1") else 0)
    rng = np.random.default_rng(7 * n + B)
    f = rng.standard_normal((B, n, n))
    th = rng.uniform(0.5, 2.0, (B, n, n))
    u = P.solve_direct(f, th).cpu().numpy()
    for b in range(B):
        e = rel(u[b], R.solve(f[b], th[b]))
        print(f"B={B} n={n} b={b}: {e:.3e}")
        assert e < 1e-10


def test_beyond_the_cooperative_limit():
    """n = 1030: srpde_poisson_coop_problems is 0 there; the bar is test_batched_large_against_oracle's."""
    from superresolution_for_pdes_amd import poisson as P
    from oracle import poisson_ref as R
    n = 1030
    f = P.forcing_batched(np.array([[3.25, 5.5]]), n)
    th = torch.from_numpy(np.random.default_rng(n).uniform(0.5, 2.0, (1, n, n))).cuda()
    u = P.solve_direct(f, th)
    fn, tn, un = f.cpu().numpy()[0], th.cpu().numpy()[0], u.cpu().numpy()[0]
    res = np.linalg.norm(R.apply_operator(un, tn) - fn) / np.linalg.norm(fn)
    print(f"n=1030 residual {res:.3e}")
    assert res < 1e-9


def test_agrees_with_cg():
    """B = 1024 at n = 40, the draws of test_batched_large_against_oracle."""
    from superresolution_for_pdes_amd import poisson as P
    rng = np.random.default_rng(3)
    B, n = 1024, 40
    k = rng.uniform(0.5, 12.0, (B, 2))
    f = P.forcing_batched(k, n)
    th = torch.from_numpy(rng.uniform(0.5, 2.0, (B, n, n))).cuda()
    ud = P.solve_batched(f, th, method="dst")
    uc = P.solve_batched(f, th, method="cg")
    d = ((ud - uc).flatten(1).norm(dim=1) / uc.flatten(1).norm(dim=1)).max().item()
    print(f"dst vs cg, worst of {B}: {d:.3e}")
    assert d < 1e-9


@pytest.mark.parametrize("n", [33, 129])
def test_deterministic_and_batch_independent(n):
    from superresolution_for_pdes_amd import poisson as P
    rng = np.random.default_rng(n)
    f = torch.from_numpy(rng.standard_normal((3, n, n))).cuda()
    th = torch.from_numpy(rng.uniform(0.5, 2.0, (3, n, n))).cuda()
    f[1] = 0.0
    u = P.solve_direct(f, th)
    assert torch.equal(u, P.solve_direct(f, th))
    for b in range(3):
        assert torch.equal(P.solve_direct(f[b:b + 1], th[b:b + 1])[0], u[b]), b
    assert float(u[1].abs().max()) == 0.0 and float(u[0].abs().max()) > 0.0
    x = f.clone()
    assert torch.equal(P.dst2(x), P.dst2(x)) and torch.equal(P.dst2(x[2:3])[0], P.dst2(x)[2])


def test_argument_errors():
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd._lib import call, query
    n, B = 129, 2                                   # above the LDS limit: the workspace is checked
    assert n > int(query("srpde_poisson_dst_lds_max_n"))
    f = torch.ones(B, n, n, dtype=torch.float64, device="cuda")
    u = torch.full_like(f, 7.0)
    plan = P.dst_plan(n)
    other = P.dst_plan(33)
    wsb = int(query("srpde_poisson_dst_workspace_size", B, n))
    assert wsb >= B * n * n * 8 and int(query("srpde_poisson_dst_plan_size", n)) == plan.numel()
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device="cuda")
    fp, up, pp, wp = f.data_ptr(), u.data_ptr(), plan.data_ptr(), ws.data_ptr()

    def solve(*a):
        call("srpde_poisson_dst_batched", *a, 0)

    def apply(*a):
        call("srpde_poisson_dst_apply", *a, 0)

    good = (fp, fp, up, B, n, pp, plan.numel(), wp, wsb)
    bad = {
        "null f": (0,) + good[1:],
        "null u": good[:2] + (0,) + good[3:],
        "null plan": good[:5] + (0,) + good[6:],
        "n = 0": good[:4] + (0,) + good[5:],
        "n < 0": good[:4] + (-3,) + good[5:],
        "B = 0": good[:3] + (0,) + good[4:],
        "short plan": good[:6] + (plan.numel() - 8,) + good[7:],
        "plan of another n": good[:5] + (other.data_ptr(), other.numel()) + good[7:],
        "null workspace": good[:7] + (0, wsb),
        "short workspace": good[:8] + (wsb - 8,),
        "misaligned workspace": good[:7] + (wp + 8, wsb),
    }
    for what, a in bad.items():
        with pytest.raises(RuntimeError, match="srpde_poisson_dst_batched"):
            solve(*a)
        b = (a[0], a[2]) + a[3:]                    # the same fault in srpde_poisson_dst_apply's arguments
        with pytest.raises(RuntimeError, match="srpde_poisson_dst_apply"):
            apply(*b)
    torch.cuda.synchronize()
    assert float((u - 7.0).abs().max()) == 0.0      # nothing was launched
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_plan"):
        call("srpde_poisson_dst_plan", n, 0, plan.numel(), 0)
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_plan"):
        call("srpde_poisson_dst_plan", 0, pp, plan.numel(), 0)
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_plan"):
        call("srpde_poisson_dst_plan", n, pp, plan.numel() - 8, 0)
    solve(*good)                                    # and the good call goes through
    torch.cuda.synchronize()


def test_method_argument():
    from superresolution_for_pdes_amd import poisson as P
    f, th = np.ones((2, 20, 20)), np.ones((2, 20, 20))
    for kw in ({"maxit": 5}, {"rtol": 1e-6}, {"check": False}, {"_start_aborted": True}):
        with pytest.raises(ValueError):
            P.solve_batched(f, th, method="dst", **kw)
    with pytest.raises(ValueError):
        P.solve_batched(f, th, method="lu")
    u, it = P.solve_batched(f, th, method="dst", return_iters=True)
    assert it.dtype == torch.int32 and it.tolist() == [0, 0]
    assert torch.equal(u, P.solve_direct(f, th))
    e, it = P.solve_batched(np.zeros((0, 20, 20)), np.zeros((0, 20, 20)), method="dst", return_iters=True)
    assert e.shape == (0, 20, 20) and it.shape == (0,)


def test_capturable_once_the_plan_exists():
    from superresolution_for_pdes_amd import poisson as P
    n = 129
    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.standard_normal((2, n, n))).cuda()
    th = torch.from_numpy(rng.uniform(0.5, 2.0, (2, n, n))).cuda()
    want = P.solve_direct(f, th)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        u = P.solve_direct(f, th)
    u.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(u, want)


def _same_inputs_close_fields(a, b, exact, fields):
    for k in exact:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in fields:
        e = rel(a[k], b[k])
        print(f"{k}: {e:.3e}")
        assert e < 1e-9, k


def test_plumbing_data_generators():
    from superresolution_for_pdes_amd.data_generation import PoissonSolver
    from superresolution_for_pdes_amd.enhanced_data_generation import EnhancedPoissonSolver
    out = {}
    for solver in ("dst", None):
        kw = {} if solver is None else {"solver": solver}
        np.random.seed(11)
        d = PoissonSolver(20, 40, **kw).generate_dataset(4)
        np.random.seed(12)
        s = EnhancedPoissonSolver(20, 40, 80, **kw)
        assert s.solver == (solver or "cg")
        e = s.generate_subdomain_dataset(3)
        out[solver] = (d, e)
    exact = ("k1", "k2", "f_coarse", "f_fine", "theta_coarse", "theta_fine")
    _same_inputs_close_fields(out["dst"][0], out[None][0], exact, ("u_coarse", "u_fine"))
    _same_inputs_close_fields(out["dst"][1], out[None][1], exact, ("u_coarse", "u_fine"))
    assert not np.array_equal(out["dst"][0]["u_fine"], out[None][0]["u_fine"])   # the other solver really ran


def test_plumbing_multi_resolution():
    from superresolution_for_pdes_amd import resolution_comparison as RC
    from superresolution_for_pdes_amd import resolution_comparison_statistical as RS
    out = {}
    for solver in ("dst", None):
        kw = {} if solver is None else {"solver": solver}
        np.random.seed(21)
        a = RC.solve_multi_resolution(40, [80, 160], **kw)
        np.random.seed(22)
        b = RS.solve_multi_resolution(2, 40, (80, 160), **kw)
        out[solver] = (a, b)
    for i in (0, 1):
        d, c = out["dst"][i], out[None][i]
        assert np.array_equal(d["k1"], c["k1"]) and np.array_equal(d["k2"], c["k2"])
        for res in (40, 80, 160):
            for k in ("f", "theta"):
                x, y = d[k][res], c[k][res]
                assert torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y), (k, res)
            x, y = d["u"][res], c["u"][res]
            if isinstance(x, torch.Tensor):
                x, y = x.cpu().numpy(), y.cpu().numpy()
            e = rel(x, y)
            print(f"solve_multi_resolution[{i}] u {res}: {e:.3e}")
            assert e < 1e-9 and not np.array_equal(x, y)
