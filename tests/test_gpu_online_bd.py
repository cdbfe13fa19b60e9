"""Boundary data in the sample stream and the training command line on the GPU (ABI 23 extended: srpde_stream_walls,
online.SampleStream(boundary=), train_enhanced --bc-data) against tests/stream_bd_ref.py: the wall synthesis from the
raw Philox words, sample identity across batch sizes and ranks, the streamed fields against tolerance-mode solves with
the same data, the stream's records, graph capture and one command-line run."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import div_bd_ref as BD
import stream_bd_ref as S

pytestmark = pytest.mark.gpu

BC = "ddnn"
AMPS = (0.05, 0.1)
EPS = np.finfo(np.float64).eps


def _stream(**kw):
    from superresolution_for_pdes_amd.online import SampleStream
    kw.setdefault("n_calib", 64)
    kw.setdefault("theta_range", (0.5, 2.0))
    kw.setdefault("form", "divergence")
    return SampleStream(**kw)


@pytest.mark.parametrize("bc", (None, BC, "nddn"))
def test_walls_from_the_raw_words(bc):
    """The coefficients come from field 2's words by the header's formula: on the n = 3 grid, where the cosines are
    exactly 1, 0 and -1, the device's values are the restated coefficients' exact fp64 combinations bit for bit.  The
    comparison of the coefficients is therefore indirect -- the kernel writes no coefficient, only (c0 + c1) + (c2 + c3),
    c0 - c2 and (c0 - c1) + (c2 - c3) of each side, for 37 samples and both amplitudes -- and the check on the other
    grids, against the same restated coefficients, closes what three combinations of four numbers leave open.  On
    other grids the values lie within 8 eps sum|c| of the extended-precision evaluation: two roundings per term, three
    sums, cospi to two ulp."""
    from superresolution_for_pdes_amd import hipops as H
    seed, first, Bn = 11, (1 << 40) + 3, 37
    pat = BD.pattern(bc)
    mask = sum(1 << i for i, c in enumerate(pat) if c == "n")
    words = H.stream_raw(seed, first, Bn, S.FIELD_WALLS, 0, 8).cpu().numpy().view(np.uint32)
    coef = S.wall_coefficients(words, pat, AMPS)
    bd3, half3, f3 = H.stream_walls(seed, first, Bn, 3, mask, AMPS, half=True, f32=True)
    assert bd3.dtype == torch.float64 and f3.dtype == torch.float32
    assert np.array_equal(bd3.cpu().numpy(), S.wall_values_exact_grid(coef))
    assert torch.equal(half3, bd3[..., ::2]) and torch.equal(f3, bd3.float())
    for n in (2, 7, 40, 80, 257):                # 257 * 4 * 37 entries: more than one pass of the grid-stride loop's block
        bd, half, f32 = H.stream_walls(seed, first, Bn, n, mask, AMPS, half=True, f32=True)
        want, tot = S.wall_values(coef, n)
        err = np.abs(bd.cpu().numpy().astype(np.longdouble) - want)
        print(f"bc={bc} n={n}: max error / (eps sum|c|) = {float((err / (EPS * tot)).max()):.3f}")
        assert np.all(err <= 8 * EPS * tot)
        assert tuple(half.shape) == (Bn, 4, (n + 1) // 2) and torch.equal(half, bd[..., ::2])
        assert torch.equal(f32, bd.float())
        assert float(bd.abs().max()) <= 25.0 / 12.0 * max(AMPS)
    # a pure function of (seed, sample, pattern, amplitudes, n): not of the batch a sample is drawn in
    bd, _, _ = H.stream_walls(seed, first, Bn, 40, mask, AMPS)
    part, _, _ = H.stream_walls(seed, first + 5, 9, 40, mask, AMPS)
    assert torch.equal(part, bd[5:14])
    assert not torch.equal(H.stream_walls(seed + 1, first, Bn, 40, mask, AMPS)[0], bd)
    into = torch.full((Bn + 2, 4, 40), 7.0, dtype=torch.float32, device="cuda")
    H.stream_walls(seed, first, Bn, 40, mask, AMPS, f32=into[1:Bn + 1])
    assert torch.equal(into[1:Bn + 1], bd.float()) and bool((into[0] == 7.0).all()) and bool((into[-1] == 7.0).all())
    # fields 0 and 1 keep their draws: the wall data is a field of its own
    k, _, th, _ = H.stream_draw(seed, first, 4, (0.5, 5.0), (0.5, 2.0), n=8)
    H.stream_walls(seed, first, 4, 8, mask, AMPS)
    k2, _, th2, _ = H.stream_draw(seed, first, 4, (0.5, 5.0), (0.5, 2.0), n=8)
    assert torch.equal(k, k2) and torch.equal(th, th2)


def test_sample_identity_across_batch_sizes_and_ranks():
    """A sample's fields and data are the same bits at batch sizes 4 and 8 and at world 1 and 2."""
    for sub in (0.0, 1.0):
        whole = _stream(seed=3, batch_size=8, sub_fraction=sub, bc=BC, boundary=AMPS)
        ranks = [_stream(seed=3, batch_size=4, sub_fraction=sub, bc=BC, boundary=AMPS, rank=r, world=2) for r in range(2)]
        small = _stream(seed=3, batch_size=4, sub_fraction=sub, bc=BC, boundary=AMPS)
        assert all(torch.equal(whole.stats, r.stats) for r in ranks + [small])
        x, y, kind, bd = whole.next_batch(with_kind=True, with_bd=True)
        assert tuple(bd.shape) == (8, 4, 40) and bd.dtype == torch.float32 and tuple(kind.shape) == (8,)
        parts = [r.next_batch(with_bd=True) for r in ranks]
        steps = [small.next_batch(with_bd=True) for _ in range(2)]
        for group in (parts, steps):
            assert all(len(p) == 3 for p in group)
            for i, full in enumerate((x, y, bd)):
                assert torch.equal(full, torch.cat([p[i] for p in group])), (sub, i)
        assert bool(bd.any()) == (sub == 0.0)              # a subdomain sample's row is zero


@pytest.mark.parametrize("grids", [(6, 12, 20), (20, 40, 80)])
@pytest.mark.parametrize("bc", (None, BC))
def test_streamed_fields_solve_the_problem_with_their_walls(grids, bc):
    """Every kept fp64 field against solve_div(rtol=1e-12, bc_data=) of the same forcing, coefficient and data: within
    2 rtol |f - b| / lam_min, the bound tests/test_gpu_div_bd.py holds a solve to against the direct solution, lam_min
    the matrix's own smallest eigenvalue."""
    from scipy.sparse.linalg import eigsh
    from superresolution_for_pdes_amd import poisson as P
    from test_gpu_div_bd import _sparse
    nc, nf, nsf = grids
    s = _stream(seed=5, batch_size=4, bc=bc, boundary=AMPS, n_coarse=nc, n_fine=nf, n_superfine=nsf)
    x, y, bd32 = s.next_batch(keep_fields=True, with_bd=True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    b = s.last_fields["fp64"]
    std, sub = b["standard"], b["subdomain"]
    assert torch.equal(bd32[:2], std["bd"].float()) and not bool(bd32[2:].any())
    assert torch.equal(std["bd_half"], std["bd"][..., ::2])
    cases = [(std["u_fine"], std["f_fine"], std["theta_fine"], std["bd"]),
             (std["u_coarse"], std["f_coarse"], std["theta_coarse"], std["bd_half"]),
             (sub["u"], sub["f"], sub["theta"], sub["bd"])]
    assert [c[0].shape[-1] for c in cases] == [nf, nc, nsf]
    pat, rtol = BD.pattern(bc), 1e-12
    for u, f, th, bd in cases:
        n = u.shape[-1]
        want = P.solve_div(f, th, face_mean="harmonic", rtol=rtol, bc=bc, bc_data=bd)
        plain = P.solve_div(f, th, face_mean="harmonic", rtol=rtol, bc=bc)
        fn, thn, bdn = f.cpu().numpy(), th.cpu().numpy(), bd.cpu().numpy()
        for i in range(u.shape[0]):
            M = _sparse(thn[i], "harmonic", pat)
            lam_min = float(np.linalg.eigvalsh(-M.toarray())[0]) if n <= 12 else \
                float(eigsh(-M.tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
            rhs = np.linalg.norm(fn[i] - BD.affine(thn[i], bdn[i], "harmonic", pat))
            err = float((u[i] - want[i]).norm())
            bound = 2.0 * rtol * rhs / lam_min
            print(f"{grids} bc={bc} n={n} sample {i}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
            assert float((u[i] - plain[i]).norm()) > 1e6 * bound         # the data-less problem is another one


def test_records_and_resuming():
    s = _stream(seed=3, batch_size=8, bc=BC, boundary=AMPS)
    d = s.describe()
    assert d["boundary"] == list(AMPS) and d["bc"] == BC
    assert s.state_dict() == {"seed": 3, "step": 0, "bc": BC, "boundary": list(AMPS)}
    json.dumps(d), json.dumps(s.state_dict())
    s.next_batch()
    t = _stream(seed=3, batch_size=8, bc=BC, boundary=AMPS)
    t.load_state_dict(s.state_dict())
    assert t.step == 1
    t.load_state_dict({"seed": 3, "step": 2, "bc": BC, "boundary": AMPS})          # a tuple is the same state
    plain = _stream(seed=3, batch_size=8, bc=BC)
    assert plain.describe()["boundary"] is None and plain.state_dict() == {"seed": 3, "step": 0, "bc": BC}
    for a, b in ((plain, s), (s, plain), (s, _stream(seed=3, batch_size=8, bc=BC, boundary=(0.05, 0.2)))):
        with pytest.raises(ValueError, match="boundary"):
            a.load_state_dict(b.state_dict())
    four = _stream(seed=3, batch_size=8, boundary=AMPS)           # no pattern: four "d" sides with values
    assert four.bc is None and four.state_dict() == {"seed": 3, "step": 0, "boundary": list(AMPS)}
    # the fixed sets and the loaders carry the data
    fs = s.frozen_set(12)
    assert tuple(fs.bd.shape) == (12, 4, 40) and bool(fs.bd[:6].any()) and not bool(fs.bd[6:].any())
    assert tuple(s.fixed_set(4, 1 << 62)["bd"].shape) == (4, 4, 40)
    batches = list(s.validation_loader(12, 8, with_kind=True, with_bd=True))
    assert [len(bt) for bt in batches] == [4, 4] and tuple(batches[1][3].shape) == (4, 4, 40)
    assert torch.equal(torch.cat([bt[3] for bt in batches]), fs.bd)
    from superresolution_for_pdes_amd.online import OnlineBatchLoader
    (only,) = list(OnlineBatchLoader(t, 1, with_kind=True, with_bd=True))
    assert len(only) == 4 and tuple(only[3].shape) == (8, 4, 40) and torch.equal(only[2], t.kind)


def test_a_stream_without_boundary_is_unchanged():
    """boundary=None makes the calls it always made: the bits of the stream built without the keyword, no "bd" in its
    sets, and a request for data is refused.  With it, other targets come out."""
    for bc in (None, BC):
        base = _stream(seed=3, batch_size=8, bc=bc)
        named = _stream(seed=3, batch_size=8, bc=bc, boundary=None)
        assert torch.equal(base.stats, named.stats)
        (bx, by), (nx, ny) = base.next_batch(), named.next_batch(keep_fields=True)
        assert torch.equal(bx, nx) and torch.equal(by, ny)
        assert "bd" not in named.last_fields and "bd" not in named.last_fields["fp64"]["standard"]
        assert named.frozen_set(4).bd is None
        with pytest.raises(ValueError, match="with_bd needs a stream"):
            named.next_batch(with_bd=True)
        walls = _stream(seed=3, batch_size=8, bc=bc, boundary=AMPS)
        assert not torch.equal(walls.next_batch()[1], by) and not torch.equal(walls.stats, base.stats)


def test_next_batch_under_graph_capture():
    """next_batch(with_bd=True) makes no host read: captured, it replays to the eager bits."""
    eager = _stream(seed=3, batch_size=8, bc=BC, boundary=AMPS).next_batch(with_kind=True, with_bd=True)
    s = _stream(seed=3, batch_size=8, bc=BC, boundary=AMPS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.next_batch(with_bd=True)                      # every buffer size seen once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.step = 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = s.next_batch(with_kind=True, with_bd=True)
    for _ in range(2):
        for t in (out[0], out[1], out[3]):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


def test_command_line_online_bc_data(tmp_path):
    """Two epochs of two batches of 8 with walls at (0.05, 0.1) and the term at weight 0.01.  The history's train_pde is
    finite and below what the run's first batch scores with the data withheld from the loss: the run's first step is
    rebuilt here -- main's seeds, its stream, its freshly initialised model in training mode -- and its output on the
    first batch is scored without ``bc_data``.  The same batch's exact solutions (y = targets) are scored both ways too:
    with the data withheld the term is at least 1e6 times the term with it."""
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.online import SampleStream
    from superresolution_for_pdes_amd.train_enhanced import main
    hist = main(["--online", "2", "--operator", "divergence", "--online-theta", "0.5", "2.0", "--bc", BC,
                 "--bc-data", str(AMPS[0]), str(AMPS[1]), "--pde-div-weight", "0.01", "--epochs", "2", "--batch-size", "8",
                 "--results", str(tmp_path)])
    for k in ("train_loss", "val_loss", "train_mse", "train_pde", "val_mse", "val_pde"):
        assert len(hist[k]) == 2 and np.isfinite(hist[k]).all(), (k, hist[k])
    torch.manual_seed(42)
    np.random.seed(42)
    torch.cuda.manual_seed(42)
    device = f"cuda:{torch.cuda.current_device()}"
    stream = SampleStream(42, 8, theta_range=(0.5, 2.0), solver="cg", device=device, form="divergence",
                          face_mean="harmonic", bc=BC, boundary=AMPS)
    model = UNet().to(device)
    model.apply(init_weights)
    model.train()
    x, y, kind, bd = stream.next_batch(with_kind=True, with_bd=True)
    kw = dict(form="divergence", bc=BC)
    with torch.no_grad():
        out = model(x)
        first_withheld = float(physics_loss_terms(out, y, x, kind, stream.stats, 0.01, **kw)[2])
        first_informed = float(physics_loss_terms(out, y, x, kind, stream.stats, 0.01, bc_data=bd, **kw)[2])
        withheld = float(physics_loss_terms(y, y, x, kind, stream.stats, 0.01, **kw)[2])
        informed = float(physics_loss_terms(y, y, x, kind, stream.stats, 0.01, bc_data=bd, **kw)[2])
    print(f"train_pde {hist['train_pde']}; the first batch at the first step with the data withheld {first_withheld:.6e}, "
          f"with the data {first_informed:.6e}; its exact solutions with the data withheld {withheld:.4e}, with the data "
          f"{informed:.4e}")
    assert informed * 1e6 <= withheld
    assert max(hist["train_pde"]) < first_withheld
    (run,) = glob.glob(os.path.join(str(tmp_path), "enhanced_run_*"))
    rec = json.load(open(os.path.join(run, "physics_loss.json")))
    assert rec["bc_data"] == list(AMPS) and rec["bc"] == BC and rec["form"] == "divergence"
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["bc_data"] == list(AMPS) and cfg["bc"] == BC
