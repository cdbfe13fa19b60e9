"""Boundary data in the physics loss, the sample stream and training, without a GPU (ABI 23, extended:
srpde_physics_loss_div_fwd_bd, srpde_stream_walls; functional.physics_mse_loss(bc_data=), online.SampleStream(boundary=),
train_enhanced --bc-data): the restatements of tests/stream_bd_ref.py against independent formulations, and every
refusal that needs no device."""
import numpy as np
import pytest
import torch

import div_bd_ref as BD
import poisson_div_ref as D
import stream_bd_ref as S
from div_bc_smoother_ref import restatement_div_bc
from test_div_smoother_host import normalised
from test_online_host import stream_words

PATTERNS = (None, "ddnn", "dnnd")
SIZES = (5, 12)
KINDS = (0, 0, 1, 1)


def _batch(n, seed):
    """Random normalised fields [4, ., n, n] of kinds (0, 0, 1, 1), theta in [0.5, 2], and random data [4, 4, n]."""
    g = torch.Generator().manual_seed(seed)
    B = len(KINDS)
    t = torch.randn(B, 1, n, n, generator=g, dtype=torch.float64)
    y = t + 0.05 * torch.randn(B, 1, n, n, generator=g, dtype=torch.float64)
    x = torch.randn(B, 3, n, n, generator=g, dtype=torch.float64)
    x[:, 1] = (0.5 + 1.5 * torch.rand(B, n, n, generator=g, dtype=torch.float64) - 1.25) / 0.43
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], dtype=torch.float64)
    inv_h2 = (float((n - 1) ** 2), float((2 * n - 1) ** 2))
    bd = torch.from_numpy(BD.data(n, seed, B))
    return y, t, x, torch.tensor(KINDS, dtype=torch.int32), stats, inv_h2, bd


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", SIZES)
def test_restatement_against_autograd_on_the_dense_formulation(n, mean, bc):
    """Loss and gradient of the split-form restatement against the dense matrices of div_bc_ref / div_bd_ref acting on
    u = u_std y + u_mean, differentiated by autograd: 1e-12 of the largest value."""
    y, t, x, kind, stats, inv_h2, bd = _batch(n, n)
    ya = y.clone().requires_grad_(True)
    out = S.restatement_div_bd(ya, t, x, kind, stats, 0.01, inv_h2, mean, bc, bd)
    out["total"].backward()
    yb = y.clone().requires_grad_(True)
    total, mse, pde = S.dense_loss(yb, t, x, kind, stats, 0.01, inv_h2, mean, bc, bd)
    total.backward()
    out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    total, mse, pde = total.detach(), mse.detach(), pde.detach()
    assert float(pde) > 1e-3
    assert abs(float(out["pde"]) - float(pde)) <= 1e-12 * float(pde)
    assert abs(float(out["mse"]) - float(mse)) <= 1e-12 * float(mse)
    assert abs(float(out["total"]) - float(total)) <= 1e-12 * float(total)
    assert float((ya.grad - yb.grad).abs().max()) <= 1e-12 * float(yb.grad.abs().max())
    # the data reaches the kind-0 samples and only them
    base = S.restatement_div_bd(y, t, x, kind, stats, 0.01, inv_h2, mean, bc, None)
    assert not torch.equal(out["r"][:2], base["r"][:2]) and torch.equal(out["r"][2:], base["r"][2:])
    poisoned = bd.clone()
    poisoned[2:] = float("nan")
    again = S.restatement_div_bd(y, t, x, kind, stats, 0.01, inv_h2, mean, bc, poisoned)
    assert torch.equal(again["r"], out["r"])


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_zero_data_is_the_bc_restatement(n, bc):
    y, t, x, kind, stats, inv_h2, bd = _batch(n, 3)
    for mean in D.MEANS:
        want = restatement_div_bc(y, t, x, kind, stats, 0.01, inv_h2, mean, BD.pattern(bc))
        for data in (None, torch.zeros_like(bd), torch.zeros(4, n, dtype=torch.float64)):
            got = S.restatement_div_bd(y, t, x, kind, stats, 0.01, inv_h2, mean, bc, data)
            for key in ("total", "mse", "pde", "r", "q"):
                assert torch.equal(got[key], want[key]), (mean, key)


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_term_vanishes_on_dense_solutions_and_not_without_the_data(n, bc):
    """u = A_bd^-1 f by div_bd_ref.solve_dense, normalised with its own statistics: the term is <= 1e-20 with the data
    and > 1e-3 with the data dropped from the loss."""
    Bn = 2
    th = D.field_theta(n, 4, 0.5, 2.0, B=Bn)
    f = np.stack([D.forcing(n), D.forcing(n, 1.4, 4.6)])
    bd = BD.data(n, 8, Bn)
    for mean in D.MEANS:
        u = np.stack([BD.solve_dense(f[b], th[b], bd[b], mean, BD.pattern(bc))[0] for b in range(Bn)])
        t, x, stats = normalised(u, f, th)
        kind = torch.zeros(Bn, dtype=torch.int32)
        inv_h2 = (float((n - 1) ** 2), float((2 * n - 1) ** 2))
        got = S.restatement_div_bd(t, t, x, kind, stats, 1.0, inv_h2, mean, bc, torch.from_numpy(bd))
        dropped = S.restatement_div_bd(t, t, x, kind, stats, 1.0, inv_h2, mean, bc, None)
        print(f"n={n} {mean} {bc}: pde with the data {float(got['pde']):.3e}, without {float(dropped['pde']):.3e}")
        assert float(got["pde"]) <= 1e-20
        assert float(dropped["pde"]) > 1e-3


def test_wall_synthesis_restatement():
    """The coefficients' range and decay, the pattern's amplitudes, the exact n = 3 grid against the extended-precision
    evaluation, and the bound (25 / 12) amp."""
    words = stream_words(7, range(5, 5 + 64), S.FIELD_WALLS, np.arange(8))
    amps = (0.05, 0.1)
    c = S.wall_coefficients(words, "ddnn", amps)
    assert c.shape == (64, 4, 4)
    for side in range(4):
        amp = amps[1] if side >= 2 else amps[0]
        for m in range(4):
            assert np.abs(c[:, side, m]).max() <= amp / (m + 1)
            assert np.abs(c[:, side, m]).max() > 0.8 * amp / (m + 1)          # 64 draws reach the range's ends
    assert len(np.unique(c)) == c.size
    same = S.wall_coefficients(words, "dddd", (0.05, 7.0))                    # no flux side: q_amp is not read
    assert np.array_equal(same[:, :2], c[:, :2]) and np.array_equal(same[:, 2:] * 2.0, c[:, 2:])
    v3, tot = S.wall_values(c, 3)
    assert np.abs(S.wall_values_exact_grid(c) - v3).max() <= 4 * np.finfo(np.float64).eps * tot.max()
    v40, tot = S.wall_values(c, 40)
    assert np.abs(v40).max() <= 25.0 / 12.0 * 0.1 and np.all(np.abs(v40) <= tot * (1 + 1e-15))
    tab = S.mode_table(40)
    assert np.all(tab[0] == 1) and tab[1, 0] == 1 and tab[1, -1] == -1 and tab[2, -1] == 1 and tab[3, -1] == -1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    from superresolution_for_pdes_amd import functional as F
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.online import FrozenSet, OnlineBatchLoader, SampleStream
    from superresolution_for_pdes_amd.train_enhanced import _criterion_call
    n = 4
    y, x = torch.zeros(2, 1, n, n), torch.zeros(2, 3, n, n)
    kind, stats = torch.zeros(2, dtype=torch.int32), torch.ones(6)
    good = torch.zeros(2, 4, n)
    div = dict(form="divergence")
    # data with the pointwise form
    with pytest.raises(ValueError, match='bc_data belongs to form="divergence"'):
        F.physics_loss_terms(y, y, x, kind, stats, 0.1, bc_data=good)
    with pytest.raises(ValueError, match='bc_data belongs to form="divergence"'):
        F.physics_mse_loss(y, y, x, kind, stats, 0.1, bc_data=good)
    with pytest.raises(ValueError, match='bc_data belongs to form="divergence"'):
        F.PhysicsMSELoss(0.1, stats, bc_data=True)
    with pytest.raises(ValueError, match="divergence form"):
        H.physics_loss_fwd(y, y, x, kind, stats, 0.1, (9.0, 49.0), bd=good)
    # shape and dtype
    for bad in (torch.zeros(2, 4, n + 1), torch.zeros(3, 4, n), torch.zeros(2, 3, n), torch.zeros(4 * n),
                torch.zeros(1, 2, 4, n)):
        with pytest.raises(ValueError, match="bc_data must be"):
            F.physics_loss_terms(y, y, x, kind, stats, 0.1, bc="ddnn", bc_data=bad, **div)
    for bad in (torch.zeros(2, 4, n, dtype=torch.float16), torch.zeros(2, 4, n, dtype=torch.int32),
                np.zeros((2, 4, n)), [[0.0] * n] * 4):
        with pytest.raises(ValueError, match="float32 or float64 tensor"):
            F.physics_mse_loss(y, y, x, kind, stats, 0.1, bc_data=bad, **div)
    # accepted data reaches the device check: [B, 4, n], [1, 4, n], [4, n], both dtypes
    for ok in (good, good[:1], good[0], good.double()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F.physics_loss_terms(y, y, x, kind, stats, 0.1, bc_data=ok, **div)
    # a module that needs data and gets none
    crit = F.PhysicsMSELoss(0.1, stats, bc="ddnn", bc_data=True, **div)
    assert crit.needs_bd and crit.needs_inputs and not F.PhysicsMSELoss.needs_bd
    assert not F.PhysicsMSELoss(0.1, stats, **div).needs_bd
    with pytest.raises(ValueError, match="needs the batch's boundary data"):
        crit(y, y, x, kind)
    with pytest.raises(ValueError, match="with_bd=True"):
        _criterion_call(crit, y, y, x, kind)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _criterion_call(crit, y, y, x, kind, good)
    # the stream
    kw = dict(theta_range=(0.5, 2.0), device="cpu")
    with pytest.raises(ValueError, match='boundary belongs to form="divergence"'):
        SampleStream(1, 8, boundary=(0.05, 0.1), **kw)
    for bad in (0.05, (0.05,), (0.05, 0.1, 0.2), ("a", "b"), (float("nan"), 0.1), (0.05, float("inf"))):
        with pytest.raises(ValueError, match="boundary"):
            SampleStream(1, 8, boundary=bad, **div, **kw)
    with pytest.raises(ValueError, match="singular"):
        SampleStream(1, 8, bc="nnnn", boundary=(0.05, 0.1), **div, **kw)
    for bc in (None, "ddnn"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SampleStream(1, 8, bc=bc, boundary=(0.05, 0.1), **div, **kw)

    class Plain:
        boundary = None
    with pytest.raises(ValueError, match="with_bd needs a stream"):
        OnlineBatchLoader(Plain(), 2, with_kind=True, with_bd=True)
    from superresolution_for_pdes_amd.train_enhanced import DeviceBatchLoader

    class Walls:
        boundary = (0.05, 0.1)
    with pytest.raises(ValueError, match="with_bd goes with with_kind"):      # train_model reads batches by position
        OnlineBatchLoader(Walls(), 2, with_bd=True)
    with pytest.raises(ValueError, match="with_bd goes with with_kind"):
        DeviceBatchLoader(FrozenSet(x, y, stats, kind, good), 2, with_bd=True)
    fs = FrozenSet(x, y, stats, kind)
    with pytest.raises(ValueError, match="boundary data was asked for"):
        fs.batch(torch.tensor([0]), with_kind=True, with_bd=True)
    got = FrozenSet(x, y, stats, kind, good + 1).batch(torch.tensor([1]), with_kind=True, with_bd=True)
    assert len(got) == 4 and tuple(got[3].shape) == (1, 4, n) and tuple(got[2].shape) == (1,)
    assert len(FrozenSet(x, y, stats, kind, good).batch(torch.tensor([1]), with_bd=True)) == 3


DIV = ["--operator", "divergence", "--online", "2", "--online-theta", "0.5", "2.0"]


@pytest.mark.parametrize("argv,word", [
    (["--bc-data", "0.05", "0.1"], "--online and --operator divergence"),
    (["--online", "2", "--bc-data", "0.05", "0.1"], "--online and --operator divergence"),
    (["--online", "2", "--online-theta", "0.5", "2.0", "--bc-data", "0.05", "0.1"], "--online and --operator divergence"),
    (DIV + ["--bc-data", "nan", "0.1"], "finite"),
    (DIV + ["--bc", "nnnn", "--bc-data", "0.05", "0.1"], "singular"),
])
def test_cli_refusals_need_no_device(argv, word, monkeypatch):
    from superresolution_for_pdes_amd import train_enhanced as TE

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(torch.cuda, "manual_seed", no_device)
    with pytest.raises(SystemExit) as e:
        TE.main(argv)
    assert word in str(e.value)


def test_cli_accepts_the_amplitudes():
    from superresolution_for_pdes_amd import train_enhanced as TE
    assert TE.arg_parser().parse_args([]).bc_data is None
    for extra in ([], ["--bc", "ddnn"], ["--bc", "ddnn", "--pde-div-weight", "0.01"]):
        args = TE.arg_parser().parse_args(DIV + extra + ["--bc-data", "0.05", "0.1"])
        assert args.bc_data == [0.05, 0.1]
        TE.check_operator_args(args)
    with pytest.raises(SystemExit):
        TE.arg_parser().parse_args(DIV + ["--bc-data", "0.05"])


# ---- the library's own checks -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from superresolution_for_pdes_amd import build
    build.build()
    from superresolution_for_pdes_amd import _lib
    return _lib


def test_header_declares_the_entries(lib):
    protos = lib.parse_header()
    assert len(protos["srpde_physics_loss_div_fwd_bd"][1]) == len(protos["srpde_physics_loss_div_fwd_bc"][1]) + 2
    assert len(protos["srpde_stream_walls"][1]) == 11
    assert lib.query("srpde_version") == 23


def test_loss_entry_argument_checks(lib):
    cd = lib.lib()

    def fwd(B=2, n=40, mean=1, bc=3, y=16, bd=16, stride=160, ws_bytes=1 << 20):
        return cd.srpde_physics_loss_div_fwd_bd(y, 16, 16, 16, 16, B, n, mean, bc, 0.1, 39.0 ** 2, 79.0 ** 2, bd, stride,
                                                16, 0, 16, ws_bytes, 0)
    for stride in (1, 40, 159, -160, 320):
        assert fwd(stride=stride) < 0 and "bd_stride" in lib.last_error()
    for bc in (-1, 16):
        assert fwd(bc=bc) < 0 and "side mask" in lib.last_error()
    assert fwd(y=0) < 0 and "null" in lib.last_error()
    assert fwd(n=2) < 0 and "n=2" in lib.last_error()
    assert fwd(n=65, stride=260) < 0 and "n=65" in lib.last_error()
    assert fwd(mean=2) < 0 and "face_mean" in lib.last_error()
    need = lib.query("srpde_physics_loss_div_workspace_size", 2, 40)
    assert fwd(ws_bytes=need - 1) < 0 and "workspace too small" in lib.last_error()
    # without data the call is the _bc entry's, refusals included
    assert fwd(bd=0, bc=16) < 0 and "srpde_physics_loss_div_fwd_bc" in lib.last_error()


def test_walls_entry_argument_checks(lib):
    cd = lib.lib()

    def walls(B=2, n=40, bc=3, g=0.05, q=0.1, bd=16):
        return cd.srpde_stream_walls(1, 0, B, n, bc, g, q, bd, 0, 0, 0)
    assert walls(bd=0) < 0 and "null" in lib.last_error()
    assert walls(B=0) < 0 and "bad shape" in lib.last_error()
    assert walls(n=1) < 0 and "n >= 2" in lib.last_error()
    for bc in (-1, 16):
        assert walls(bc=bc) < 0 and "side mask" in lib.last_error()
    for g, q in ((float("nan"), 0.1), (0.05, float("inf"))):
        assert walls(g=g, q=q) < 0 and "finite" in lib.last_error()
