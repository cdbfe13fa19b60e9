"""GPU: the divergence-form operator div(theta grad u) (csrc/poisson_div.hip), its sine-preconditioned CG and their
way up through poisson.apply_div / solve_div / solve_batched / residual_metrics, online.SampleStream and the training
command line, against the numpy restatement of tests/poisson_div_ref.py."""
import json

import numpy as np
import pytest
import torch

import poisson_div_ref as D

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the operator ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("B,n", [(1, 2), (3, 5), (2, 17), (2, 33), (1, 129)])
def test_apply_div_is_bit_equal_to_the_host_restatement(B, n, mean):
    from superresolution_for_pdes_amd import poisson as P
    u, v = D.field_u(n, 0, B), D.field_u(n, 1, B)
    th = D.field_theta(n, 0, 0.1, 10.0, B)
    got = P.apply_div(u, th, face_mean=mean)
    assert got.dtype == torch.float64 and got.shape == (B, n, n)
    want = D.apply(u, th, mean)
    assert np.array_equal(got.cpu().numpy(), want)
    # another inv_h2 (a crop of a larger grid), and a 2-D call
    got2 = P.apply_div(u[0], th[0], face_mean=mean, inv_h2=1234.5)
    assert np.array_equal(got2.cpu().numpy()[0], D.apply(u[0], th[0], mean, inv_h2=1234.5))
    # symmetry: <v, D u> = <u, D v>
    dv = P.apply_div(v, th, face_mean=mean).cpu().numpy()
    a, b = np.sum(v * got.cpu().numpy()), np.sum(u * dv)
    scale = np.sqrt(np.sum(v * v) * np.sum(want * want))
    assert abs(a - b) <= 1e-13 * scale, (a, b)


# ---- 2. the solve against the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
@pytest.mark.parametrize("n", D.SOLVE_NS)
def test_solve_div_against_the_reference(n, mean):
    from superresolution_for_pdes_amd import poisson as P
    th = np.stack([D.field_theta(n, s, 0.5, 2.0) for s in (0, 1)])
    f = D.forcing(n)
    u, iters, resid = P.solve_div(np.stack([f, f]), th, face_mean=mean, return_info=True)
    u, iters, resid = u.cpu().numpy(), iters.cpu().numpy(), resid.cpu().numpy()
    ref_solve = D.solve_dense if n <= 33 else D.solve_sparse
    for b in range(2):
        ref = ref_solve(f, th[b], mean)
        _, host_iters, _ = D.pcg(f, th[b], mean, rtol=RTOL)
        err = np.linalg.norm(u[b] - ref) / np.linalg.norm(ref)
        print(f"n={n} {mean} problem {b}: GPU iters {iters[b]} (host {host_iters}), resid {resid[b]:.3e}, "
              f"rel L2 {err:.3e}")
        assert err < 1e-10
        assert resid[b] <= RTOL
        assert 1 <= iters[b] <= host_iters + 2


# ---- 3. constant theta --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_constant_theta_converges_at_once(mean):
    from superresolution_for_pdes_amd import poisson as P
    n = 20
    f = D.forcing(n)
    th = np.full((n, n), 1.7)
    u, iters, resid = P.solve_div(f, th, face_mean=mean, return_info=True)
    want = P.solve_direct(f, th)
    assert int(iters[0]) <= 2 and float(resid[0]) <= RTOL
    assert float((u - want).norm() / want.norm()) < 1e-12


# ---- 4. freeze and batch independence -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch():
    n = 20
    f = D.forcing(n)
    (_, s1, lo1, hi1, _), (_, s2, lo2, hi2, _) = D.FREEZE_CASES
    th = np.stack([np.full((n, n), 1.7), D.field_theta(n, s1, lo1, hi1), D.field_theta(n, s2, lo2, hi2),
                   D.field_theta(n, 5, 0.5, 2.0)])
    fs = np.stack([f, f, f, np.zeros((n, n))])
    host = [D.pcg(fs[b], th[b], "harmonic", rtol=RTOL)[1] for b in range(4)]
    return fs, th, host


def test_freeze_and_batch_independence(mixed_batch):
    from superresolution_for_pdes_amd import poisson as P
    fs, th, host = mixed_batch
    u, iters, resid = P.solve_div(fs, th, return_info=True)
    print(f"GPU iters {iters.tolist()} host {host} resid {resid.tolist()}")
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(resid).all())
    assert int(iters[3]) == 0 and float(resid[3]) == 0.0 and not bool(u[3].any())
    assert int(iters[0]) <= 2 and int(iters[0]) < int(iters[1]) < int(iters[2])
    assert bool((resid <= RTOL).all())
    for b in range(4):
        ub, ib, rb = P.solve_div(fs[b], th[b], return_info=True)
        assert torch.equal(ub[0], u[b]) and int(ib[0]) == int(iters[b]) and float(rb[0]) == float(resid[b]), b
    # fixed mode: exactly maxit iterations, no host read; the frozen problems sit through the extra ones unchanged
    uf, itf, rf = P.solve_div(fs, th, maxit=max(host) + 10, check_every=0, return_info=True)
    assert torch.equal(uf, u) and torch.equal(itf, iters) and torch.equal(rf, resid)
    # and the chunk length of the default mode changes nothing
    u3, it3, r3 = P.solve_div(fs, th, check_every=3, return_info=True)
    assert torch.equal(u3, u) and torch.equal(it3, iters) and torch.equal(r3, resid)


# ---- 5. non-convergence -------------------------------------------------------------------------------------
def test_not_converged(mixed_batch):
    from superresolution_for_pdes_amd import poisson as P
    fs, th, _ = mixed_batch
    with pytest.raises(P.NotConverged, match="1 of 1"):
        P.solve_div(fs[2], th[2], maxit=3)
    u, iters, resid = P.solve_div(fs[2], th[2], maxit=3, check=False, return_info=True)
    assert bool(torch.isfinite(u).all()) and int(iters[0]) == 3 and float(resid[0]) > RTOL
    with pytest.raises(P.NotConverged, match="2 of 4"):
        P.solve_div(fs, th, maxit=3)


# ---- 6. fixed mode in a graph -------------------------------------------------------------------------------
def test_fixed_mode_under_graph_capture():
    from superresolution_for_pdes_amd import poisson as P
    n, B = 20, 4
    th = _dev(D.field_theta(n, 0, 0.5, 2.0, B))
    f = _dev(np.stack([D.forcing(n, 3.3 + b, 1.7) for b in range(B)]))
    P.dst_plan(n)
    eager = P.solve_div(f, th, maxit=30, check_every=0, return_info=True)
    assert bool((eager[2] <= RTOL).all())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # every launch goes to the one capturing stream: a linear chain, no branches
        out = P.solve_div(f, th, maxit=30, check_every=0, check=False, return_info=True)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


# ---- 7. residual metric and routing -------------------------------------------------------------------------
@pytest.mark.parametrize("mean", D.MEANS)
def test_residual_metrics_and_solve_batched_route(mean):
    from superresolution_for_pdes_amd import poisson as P
    n, B = 33, 3
    u, th = D.field_u(n, 2, B), D.field_theta(n, 2, 0.5, 2.0, B)
    f = np.stack([D.forcing(n, 2.3 + b, 1.1) for b in range(B)])
    for interior in (False, True):
        got = P.residual_metrics(u, f, th, interior_only=interior, form="divergence", face_mean=mean).cpu().numpy()
        r = D.apply(u, th, mean) - f
        if interior:
            r = r[:, 1:-1, 1:-1]
        r = r.reshape(B, -1)
        want = np.stack([np.sqrt(np.mean(r * r, axis=1)), np.abs(r).max(axis=1)], axis=1)
        assert got.shape == (B, 2) and np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    sol = P.solve_div(f, th, face_mean=mean)
    routed, iters = P.solve_batched(f, th, form="divergence", face_mean=mean, return_iters=True)
    assert torch.equal(routed, sol) and iters.dtype == torch.int32 and int(iters.min()) >= 1
    m = P.residual_metrics(sol, f, th, form="divergence", face_mean=mean).cpu().numpy()
    rms_f = np.sqrt(np.mean(f.reshape(B, -1) ** 2, axis=1))
    print(f"{mean}: residual rms / rms(f) {m[:, 0] / rms_f}")
    assert np.all(m[:, 0] <= 1e-9 * rms_f)
    # the pointwise metric is what it was, named or not
    assert torch.equal(P.residual_metrics(u, f, th), P.residual_metrics(u, f, th, form="pointwise"))
    with pytest.raises(ValueError):
        P.solve_batched(f, th, form="divergence", method="dst")
    with pytest.raises(ValueError):
        P.solve_batched(f, th, face_mean="arithmetic")


# ---- 8. the stream ------------------------------------------------------------------------------------------
def _stream(**kw):
    from superresolution_for_pdes_amd.online import SampleStream
    kw.setdefault("n_calib", 64)
    return SampleStream(**kw)


def test_stream_solves_the_divergence_equation():
    from superresolution_for_pdes_amd import poisson as P
    s = _stream(seed=3, batch_size=8, theta_range=(0.5, 2.0), form="divergence")
    d = s.describe()
    assert d["form"] == "divergence" and d["face_mean"] == "harmonic" and d["pcg_iters"] == 30
    x, y = s.next_batch(keep_fields=True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    b = s.last_fields["fp64"]
    grids = [tuple(b["standard"][k] for k in ("u_fine", "f_fine", "theta_fine")),
             tuple(b["standard"][k] for k in ("u_coarse", "f_coarse", "theta_coarse")),
             tuple(b["subdomain"][k] for k in ("u", "f", "theta"))]
    for u, f, th in grids:
        rms_f = f.flatten(1).pow(2).mean(1).sqrt()
        div = P.residual_metrics(u, f, th, form="divergence")[:, 0]
        pw = P.residual_metrics(u, f, th)[:, 0]
        print(f"n={u.shape[-1]}: divergence {float((div / rms_f).max()):.3e}, pointwise {float((pw / rms_f).min()):.3e}")
        assert bool((div <= 1e-9 * rms_f).all())
        assert bool((pw > 1e-3 * rms_f).all())
    # the crops of the super-fine solves: the interior of a window satisfies the super-fine grid's equation
    u, f, th = b["subdomain"]["u"], b["subdomain"]["f"], b["subdomain"]["theta"]
    nf, nsf = s.n_fine, s.n_superfine
    starts = b["subdomain"]["starts"].cpu().numpy()
    crop = lambda a: torch.stack([a[i, sy:sy + nf, sx:sx + nf] for i, (sx, sy) in enumerate(starts)]).contiguous()
    cu, cf, cth = crop(u), crop(f), crop(th)
    rms_f = cf[:, 1:-1, 1:-1].flatten(1).pow(2).mean(1).sqrt()
    inv_h2 = float((nsf - 1) ** 2)
    div = P.residual_metrics(cu, cf, cth, interior_only=True, inv_h2=inv_h2, form="divergence")[:, 0]
    pw = P.residual_metrics(cu, cf, cth, interior_only=True, inv_h2=inv_h2)[:, 0]
    assert bool((div <= 1e-9 * rms_f).all()) and bool((pw > 1e-3 * rms_f).all())
    # the fp32 training fields are those windows
    n_std = 4
    assert torch.equal(s.last_fields["u_fine"][n_std:], cu.float())
    assert torch.equal(s.last_fields["u_fine"][:n_std], b["standard"]["u_fine"].float())


def test_stream_sample_identity_and_default_form():
    kw = dict(seed=3, theta_range=(0.5, 2.0), form="divergence", sub_fraction=0.0)
    whole = _stream(batch_size=8, **kw)
    halves = _stream(batch_size=4, **kw)
    assert torch.equal(whole.stats, halves.stats)
    x, y = whole.next_batch()
    parts = [halves.next_batch() for _ in range(2)]
    assert torch.equal(x, torch.cat([p[0] for p in parts])) and torch.equal(y, torch.cat([p[1] for p in parts]))
    # with subdomain slots: sample s of the 8-batch's subdomain half is the same sample drawn in a 4-batch
    a = _stream(seed=3, batch_size=8, theta_range=(0.5, 2.0), form="divergence", sub_fraction=1.0)
    c = _stream(seed=3, batch_size=4, theta_range=(0.5, 2.0), form="divergence", sub_fraction=1.0)
    xa, ya = a.next_batch()
    pc = [c.next_batch() for _ in range(2)]
    assert torch.equal(xa, torch.cat([p[0] for p in pc])) and torch.equal(ya, torch.cat([p[1] for p in pc]))
    # the default is the pointwise stream, bit for bit
    plain = _stream(seed=3, batch_size=8, theta_range=(0.5, 2.0))
    named = _stream(seed=3, batch_size=8, theta_range=(0.5, 2.0), form="pointwise")
    assert plain.describe()["form"] == "pointwise" and plain.describe()["pcg_iters"] is None
    assert torch.equal(plain.stats, named.stats)
    (px, py), (nx, ny) = plain.next_batch(), named.next_batch()
    assert torch.equal(px, nx) and torch.equal(py, ny)
    assert not torch.equal(py, _stream(seed=3, batch_size=8, theta_range=(0.5, 2.0), form="divergence").next_batch()[1])


# ---- 9. the training command line ---------------------------------------------------------------------------
def test_training_command_line(tmp_path):
    from superresolution_for_pdes_amd.train_enhanced import main
    hist = main(["--online", "2", "--epochs", "1", "--batch-size", "8", "--operator", "divergence", "--online-theta",
                 "0.5", "2.0", "--solver", "dst", "--results", str(tmp_path)])
    assert hist["num_epochs"] == 1 and np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["val_loss"][0])
    cfg = json.load(open(next(tmp_path.glob("enhanced_run_*/config.json"))))
    assert cfg["operator"] == "divergence" and cfg["face_mean"] == "harmonic"
