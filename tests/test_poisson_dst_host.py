"""CPU: the sine-transform solver's host-side surface -- size queries without a GPU, the opt-in defaults
(every caller stays on CG unless told otherwise) and the --solver switch of the two CLIs."""
import inspect

import pytest


@pytest.fixture(scope="module")
def lib():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import _lib
    return _lib


def test_size_queries_without_gpu(lib):
    q = lib.query
    for n in (1, 5, 80, 640, 1030):
        assert q("srpde_poisson_dst_plan_size", n) >= (n * n + n) * 8
    assert q("srpde_poisson_dst_plan_size", 0) == 0 and q("srpde_poisson_dst_plan_size", -4) == 0
    lim = q("srpde_poisson_dst_lds_max_n")
    assert lim >= 80
    assert q("srpde_poisson_dst_workspace_size", 0, 640) == 0
    assert q("srpde_poisson_dst_workspace_size", -1, 640) == 0
    assert q("srpde_poisson_dst_workspace_size", 4, lim) == 0           # the fused path needs none
    assert q("srpde_poisson_dst_workspace_size", 4, lim + 1) >= 4 * (lim + 1) ** 2 * 8
    assert q("srpde_poisson_dst_workspace_size", 4, 640) >= 4 * 640 * 640 * 8


def test_argument_errors_need_no_gpu(lib):
    """Bad arguments are refused on the host, before any launch, with the entry's name in the message."""
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_batched"):
        lib.call("srpde_poisson_dst_batched", 0, 0, 0, 1, 20, 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_batched"):
        lib.call("srpde_poisson_dst_batched", 16, 16, 16, 1, 20, 16, 8, 0, 0, 0)   # 8 bytes: no plan for n = 20
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_apply"):
        lib.call("srpde_poisson_dst_apply", 16, 16, 1, 0, 16, 8, 0, 0, 0)
    with pytest.raises(RuntimeError, match="srpde_poisson_dst_plan"):
        lib.call("srpde_poisson_dst_plan", 20, 16, 8, 0)


def _default(fn, name):
    return inspect.signature(fn).parameters[name].default


def test_every_default_is_cg():
    from superresolution_for_pdes_amd import compare_test_cases as CT
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd import resolution_comparison as RC
    from superresolution_for_pdes_amd import resolution_comparison_statistical as RS
    from superresolution_for_pdes_amd import train_enhanced as TE
    from superresolution_for_pdes_amd.data_generation import PoissonSolver
    from superresolution_for_pdes_amd.enhanced_data_generation import EnhancedPoissonSolver
    assert _default(P.solve_batched, "method") == "cg"
    for fn in (PoissonSolver.__init__, EnhancedPoissonSolver.__init__, RC.solve_multi_resolution,
               RS.solve_multi_resolution, RS.run_examples, CT.generate_test_data, TE.generate_on_device):
        assert _default(fn, "solver") == "cg", fn
    assert "solver" not in TE.default_config()
    assert callable(P.solve_direct) and callable(P.dst2)
    with pytest.raises(ValueError):
        PoissonSolver(solver="lu")


def test_solver_switch_parses_on_both_clis():
    from superresolution_for_pdes_amd import resolution_comparison_statistical as RS
    from superresolution_for_pdes_amd import train_enhanced as TE
    assert RS.arg_parser().parse_args(["--model_path", "m.pth"]).solver == "cg"
    assert RS.arg_parser().parse_args(["--model_path", "m.pth", "--solver", "dst"]).solver == "dst"
    assert TE.arg_parser().parse_args([]).solver == "cg"
    assert TE.arg_parser().parse_args(["--generate", "8", "8", "--solver", "dst"]).solver == "dst"
    with pytest.raises(SystemExit):
        TE.arg_parser().parse_args(["--solver", "lu"])
