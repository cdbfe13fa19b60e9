"""CPU: the divergence-form operator's host restatement (tests/poisson_div_ref.py) has the properties the GPU tests
lean on, and the refusals of the new options are reached before any device work."""
import numpy as np
import pytest

import poisson_div_ref as D
from oracle import poisson_ref as R


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", [5, 12])
def test_dense_matrix_is_exactly_symmetric_and_negative_definite(n, mean):
    a = D.dense(D.field_theta(n, 7, 0.1, 10.0), mean)
    assert np.array_equal(a, a.T)
    assert np.linalg.eigvalsh(a).max() < 0.0
    # the sparse assembly (the spsolve reference of the larger grids) is the same matrix
    assert np.array_equal(D.sparse(D.field_theta(n, 7, 0.1, 10.0), mean).toarray(), a)


def test_dense_matrix_is_the_operator():
    n = 6
    th, u = D.field_theta(n, 1, 0.1, 10.0), D.field_u(n, 1)
    for mean in D.MEANS:
        y = D.apply(u, th, mean)
        assert np.allclose(D.dense(th, mean) @ u.reshape(-1), y.reshape(-1), rtol=1e-13, atol=1e-10)


@pytest.mark.parametrize("n", [5, 9, 17, 12])
def test_constant_theta_is_theta_times_the_laplacian(n):
    """theta * L of the oracle.  At n = 5, 9, 17 h is a power of two, so the oracle's 1 / (h * h) is (n - 1)^2
    exactly and the arithmetic mean (0.5 * (t + t) = t) must agree bit for bit; at n = 12 the oracle's own rounding
    of 1 / (h * h) allows 1e-15.  The harmonic mean rounds t * t: 1e-15 relative everywhere."""
    t = 1.7
    want = R.laplacian(n).toarray() * t
    arith = D.dense(np.full((n, n), t), "arithmetic")
    harm = D.dense(np.full((n, n), t), "harmonic")
    if n != 12:
        assert np.array_equal(arith, want)
    assert np.abs(arith - want).max() <= 1e-15 * np.abs(want).max()
    assert np.abs(harm - want).max() <= 1e-15 * np.abs(want).max()


@pytest.mark.parametrize("mean", D.MEANS)
def test_second_order_consistency(mean):
    """On smooth theta and u the interior truncation error falls 4x per halving of h."""
    errs = []
    for n in (21, 41, 81):
        x = np.linspace(0.0, 1.0, n)
        X, Y = np.meshgrid(x, x)
        th = 1.0 + 0.5 * np.sin(2.0 * X + Y)
        thx, thy = np.cos(2.0 * X + Y), 0.5 * np.cos(2.0 * X + Y)
        u = np.sin(1.3 * X + 0.4) * np.cos(0.9 * Y + 0.2)
        ux = 1.3 * np.cos(1.3 * X + 0.4) * np.cos(0.9 * Y + 0.2)
        uy = -0.9 * np.sin(1.3 * X + 0.4) * np.sin(0.9 * Y + 0.2)
        lap = -(1.3 ** 2 + 0.9 ** 2) * u
        exact = thx * ux + thy * uy + th * lap
        errs.append(np.abs(D.apply(u, th, mean) - exact)[1:-1, 1:-1].max())
    for a, b in zip(errs, errs[1:]):
        assert 3.8 <= a / b <= 4.2, errs


@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n,lo,hi", [(5, 0.5, 2.0), (20, 0.5, 2.0), (20, 0.1, 10.0), (33, 0.5, 2.0)])
def test_host_pcg_matches_the_dense_solve(n, lo, hi, mean):
    th, f = D.field_theta(n, 0, lo, hi), D.forcing(n)
    u, k, resid = D.pcg(f, th, mean)
    ref = D.solve_dense(f, th, mean)
    assert resid <= 1e-12
    assert np.linalg.norm(u - ref) / np.linalg.norm(ref) < 1e-10


def test_host_pcg_constant_theta_and_zero_forcing():
    n = 20
    u, k, resid = D.pcg(D.forcing(n), np.full((n, n), 1.7), "harmonic")
    assert k <= 2 and resid <= 1e-12
    u, k, resid = D.pcg(np.zeros((n, n)), D.field_theta(n, 0, 0.5, 2.0))
    assert k == 0 and resid == 0.0 and not u.any()


@pytest.mark.parametrize("n,seed,lo,hi,mean", D.SOLVE_CASES + D.FREEZE_CASES)
def test_host_pcg_iterations_within_the_yardstick(n, seed, lo, hi, mean):
    """The GPU tests allow the device the host count + 2.  The host count itself stays within the Chebyshev bound at
    the condition number theta_hi / theta_lo, plus the 4 spare iterations SampleStream's fixed count carries."""
    _, k, resid = D.pcg(D.forcing(n), D.field_theta(n, seed, lo, hi), mean)
    assert resid <= 1e-12
    assert k <= D.chebyshev_iterations(lo, hi) + 4, (k, D.chebyshev_iterations(lo, hi))


def test_pcg_iters_default():
    from superresolution_for_pdes_amd.online import default_pcg_iters
    assert default_pcg_iters((0.5, 2.0)) == 30
    assert default_pcg_iters((0.5, 2.0)) == D.chebyshev_iterations(0.5, 2.0) + 4
    assert default_pcg_iters((0.1, 10.0)) == D.chebyshev_iterations(0.1, 10.0) + 4
    assert default_pcg_iters((1.0, 1.0)) == 5      # 2 * 0^0 = 2 > tol: k = 1, plus 4
    with pytest.raises(ValueError):
        default_pcg_iters((0.0, 1.0))


@pytest.mark.parametrize("argv,word", [
    (["--operator", "divergence"], "--online"),
    (["--operator", "divergence", "--online", "2"], "--online-theta"),
    (["--operator", "divergence", "--online", "2", "--online-theta", "0.5", "2.0", "--pde-weight", "0.1"],
     "pointwise residual"),
    (["--face-mean", "arithmetic"], "--operator divergence"),
])
def test_cli_refusals_need_no_device(argv, word, monkeypatch):
    import torch

    from superresolution_for_pdes_amd import train_enhanced as TE

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(torch.cuda, "manual_seed", no_device)
    with pytest.raises(SystemExit) as e:
        TE.main(argv)
    assert word in str(e.value)


def test_cli_accepts_the_operator_and_keeps_the_default():
    from superresolution_for_pdes_amd import train_enhanced as TE
    args = TE.arg_parser().parse_args([])
    assert args.operator == "pointwise" and args.face_mean == "harmonic"
    TE.check_operator_args(args)
    args = TE.arg_parser().parse_args(["--operator", "divergence", "--face-mean", "arithmetic", "--online", "2",
                                       "--online-theta", "0.5", "2.0"])
    TE.check_operator_args(args)
    with pytest.raises(SystemExit):
        TE.arg_parser().parse_args(["--operator", "conservative"])


def test_stream_and_solver_refusals_need_no_device():
    from superresolution_for_pdes_amd import online as O
    from superresolution_for_pdes_amd import poisson as P
    with pytest.raises(ValueError, match="theta_range"):
        O.SampleStream(0, 8, form="divergence")
    with pytest.raises(ValueError, match="form"):
        O.SampleStream(0, 8, form="conservative")
    with pytest.raises(ValueError, match="divergence"):
        O.SampleStream(0, 8, theta_range=(0.5, 2.0), pcg_iters=10)
    with pytest.raises(ValueError, match="face mean"):
        P.check_face_mean("geometric")
    with pytest.raises(ValueError, match="form"):
        P.check_form("conservative")
    assert P.check_face_mean("arithmetic") == 0 and P.check_face_mean("harmonic") == 1
    assert issubclass(P.NotConverged, RuntimeError)


def test_library_queries_without_gpu():
    """ABI 18: the size queries answer on the host; bad arguments fail before any launch."""
    from superresolution_for_pdes_amd import _lib, build
    build.build()
    q = _lib.query
    assert q("srpde_version") >= 18
    small, large = q("srpde_div_cg_workspace_size", 4, 80), q("srpde_div_cg_workspace_size", 4, 129)
    assert small >= 6 * 4 * 80 * 80 * 8
    assert large >= 7 * 4 * 129 * 129 * 8     # above the sine transform's LDS limit: its workspace too
    assert 0 < q("srpde_div_cg_done_offset", 4, 80) <= small - 16
    assert q("srpde_div_cg_done_offset", 4, 80) % 16 == 0
    assert q("srpde_div_cg_workspace_size", 0, 80) == 0 and q("srpde_div_cg_workspace_size", 4, 1) == 0
    assert q("srpde_div_cg_workspace_size", 65536, 8) == 0
    with pytest.raises(RuntimeError, match="srpde_div_apply"):
        _lib.call("srpde_div_apply", 0, 0, 0, 1, 8, 1, 49.0, 0)
    with pytest.raises(RuntimeError, match="face_mean"):
        _lib.call("srpde_div_apply", 16, 32, 48, 1, 8, 2, 49.0, 0)
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("srpde_div_apply", 16, 32, 48, 1, 1, 1, 49.0, 0)
    with pytest.raises(RuntimeError, match="plan"):
        _lib.call("srpde_div_cg_init", 16, 1, 8, 32, 5, 64, 1 << 20, 0)
    with pytest.raises(RuntimeError, match="k_begin"):
        _lib.call("srpde_div_cg_iterate", 16, 1, 8, 1, 1e-12, 0, 1, 32, (64 + 8) * 8, 64, 1 << 20, 0)
