"""The divergence-form residual as a loss term on the GPU (csrc/physics.hip physics_loss_kernel<DivLoss>, ABI 19)
against restatement_div of tests/test_div_smoother_host.py in fp64, evaluated on the CPU from the kernel's own fp32
inputs (gradient: torch autograd in fp64).

Tolerances are computed from the inputs, as in tests/test_gpu_physics.py.  With c = u_std * inv_h2 / f_std (the largest
inv_h2 in the batch) and eps = 2^-23, the residual of one node is off by at most
    delta = 64 eps c max|theta| max|y| + 4 eps max|r|
-- the pointwise bound with four times its first term.  A face coefficient (at most max|theta|) carries up to three
roundings, the difference it multiplies (at most 2 max|y|) one and the product one: 10 eps max|theta| max|y| per face,
40 for the four; the two pair sums (at most 4 max|theta| max|y| each) and the sum of the pairs (at most 8) add 16:
56 <= 64.  The second term is the handful of roundings of a value of the size of r, as there.  Then
    |pde - pde64|  <= 2 sqrt(pde64) delta + delta^2            (triangle inequality on the RMS norm)
    |mse - mse64|  <= 4 eps mse64
    |dy - dy64|    <= weight (2 c / M) (8 max|theta| delta + 64 eps max|theta| max|q|) + (2 / N) 4 eps max|y - t|
(elementwise; q = m r: the face sum on q has four faces of at most max|theta| on differences of values off by delta,
and its own roundings are those of the first term above with q for y).
On exact solutions the term is <= 5e-11 (1.2e-13 .. 1.65e-12 for this formulation in fp32 on the CPU).
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

import poisson_div_ref as D
from test_div_smoother_host import CROP, INV_H2, normalised, restatement_div

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
WEIGHT = 0.01
KINDS = (0, 1, 0, 1, 1)


def gpu_loss(y, t, x, kind, stats, weight, mean, inv_h2=INV_H2, grad=True):
    """The kernel on fp32 copies of the inputs -> (terms [3] float64 numpy of the fp32 results, dy fp32 cpu or None)."""
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    yd = y.float().cuda().requires_grad_(grad)
    terms = physics_loss_terms(yd, t.float().cuda(), x.float().cuda(), kind.to(torch.int32).cuda(),
                               stats.float().cuda(), weight, inv_h2, form="divergence", face_mean=mean)
    if grad:
        terms[0].backward()
    return terms.detach().cpu().double().numpy(), (yd.grad.cpu() if grad else None)


def reference(y, t, x, kind, stats, weight, mean, inv_h2=INV_H2):
    """The restatement on the same fp32 values, with its autograd gradient and the bounds of the module docstring."""
    y32, t32, x32, s32 = y.float(), t.float(), x.float(), stats.float()
    yd = y32.double().requires_grad_(True)
    out = restatement_div(yd, t32, x32, kind, s32, weight, inv_h2, mean)
    out["total"].backward()
    sg_u, sg_f = float(s32[1]), float(s32[3])
    c = sg_u * max(inv_h2[int(k != 0)] for k in kind.tolist()) / sg_f
    th_max = float(out["theta"].abs().max())
    r_max = float((out["m"] * out["r"]).detach().abs().max())
    q_max = float(out["q"].detach().abs().max())
    delta = 64 * EPS * c * th_max * float(y32.abs().max()) + 4 * EPS * r_max
    pde, mse = float(out["pde"].detach()), float(out["mse"].detach())
    N = y32.numel()
    return {"pde": pde, "mse": mse, "total": float(out["total"].detach()), "dy": yd.grad, "out": out, "delta": delta,
            "pde_bound": 2 * np.sqrt(pde) * delta + delta * delta, "mse_bound": 4 * EPS * mse,
            "dy_bound": weight * (2 * c / out["M"]) * (8 * th_max * delta + 64 * EPS * th_max * q_max)
            + (2.0 / N) * 4 * EPS * float((y32 - t32).abs().max())}


def check(name, got, dy, ref):
    e_pde, e_mse = abs(got[2] - ref["pde"]), abs(got[1] - ref["mse"])
    e_dy = float((dy.double() - ref["dy"]).abs().max())
    print(f"{name}: pde {got[2]:.6e} err {e_pde:.3e} (bound {ref['pde_bound']:.3e})  mse err {e_mse:.3e} "
          f"(bound {ref['mse_bound']:.3e})  dy err {e_dy:.3e} (bound {ref['dy_bound']:.3e})")
    assert e_pde <= ref["pde_bound"], (name, e_pde, ref["pde_bound"])
    assert e_mse <= ref["mse_bound"], (name, e_mse, ref["mse_bound"])
    assert e_dy <= ref["dy_bound"], (name, e_dy, ref["dy_bound"])


@pytest.fixture(scope="module")
def truth():
    """{mean: (t, x, kind, stats)} fp64 on the CPU: B = 5 samples of kinds (0, 1, 0, 1, 1) at n = 40, theta ~
    U(0.5, 2): solve_div solutions of 40^2 problems and 40^2 crops of 80^2 ones, normalised with their own statistics.
    Solved once per mean and shared (never modified) by the tests below."""
    from superresolution_for_pdes_amd import poisson as P
    out = {}
    for mean in D.MEANS:
        th40, th80 = D.field_theta(40, 11, 0.5, 2.0, B=2), D.field_theta(80, 12, 0.5, 2.0, B=3)
        f40 = np.stack([D.forcing(40), D.forcing(40, 1.4, 4.6)])
        f80 = np.stack([D.forcing(80, 2.3, 4.1), D.forcing(80), D.forcing(80, 4.9, 0.7)])
        u40 = P.solve_div(f40, th40, face_mean=mean).cpu().numpy()
        u80 = P.solve_div(f80, th80, face_mean=mean).cpu().numpy()
        i, j = CROP
        crop = [tuple(a[b, i + 3 * b:i + 3 * b + 40, j - 5 * b:j - 5 * b + 40] for a in (u80, f80, th80))
                for b in range(3)]
        whole = [(u40[b], f40[b], th40[b]) for b in range(2)]
        rows = [whole[0], crop[0], whole[1], crop[1], crop[2]]
        t, x, stats = normalised(*(np.stack([r[k] for r in rows]) for k in range(3)))
        out[mean] = (t, x, torch.tensor(KINDS, dtype=torch.int32), stats)
    return out


def noisy(t, seed=0, noise=1e-2):
    g = torch.Generator().manual_seed(seed)
    return t + noise * torch.randn(t.shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("mean", D.MEANS)
def test_term_vanishes_on_solutions(truth, mean):
    t, x, kind, stats = truth[mean]
    for b in range(len(KINDS)):
        s = slice(b, b + 1)
        got, _ = gpu_loss(t[s], t[s], x[s], kind[s], stats, 1.0, mean)
        print(f"{mean} sample {b} kind {KINDS[b]}: pde on the truth, fp32 kernel: {got[2]:.3e}")
        assert got[2] <= 5e-11, (mean, b, got[2])
        assert got[1] == 0.0 and got[0] == got[2]
    got, _ = gpu_loss(t, t, x, kind, stats, 1.0, mean)
    assert got[2] <= 5e-11


@pytest.mark.parametrize("mean", D.MEANS)
def test_perturbed_against_the_restatement(truth, mean):
    """B = 5 (odd: the last workgroup holds one sample), both kinds, 1e-2 noise on y."""
    t, x, kind, stats = truth[mean]
    y = noisy(t)
    got, dy = gpu_loss(y, t, x, kind, stats, WEIGHT, mean)
    ref = reference(y, t, x, kind, stats, WEIGHT, mean)
    assert ref["pde"] > 1e-3                    # many orders above the truth's 1e-12: a real signal to compare
    check(f"{mean} {KINDS}", got, dy, ref)
    assert abs(got[0] - (got[1] + WEIGHT * got[2])) <= 2 * EPS * got[0]
    # the other mean's faces give another value: the argument reaches the kernel
    other, _ = gpu_loss(y, t, x, kind, stats, WEIGHT, D.MEANS[1 - D.MEANS.index(mean)], grad=False)
    assert abs(other[2] - got[2]) > 10 * ref["pde_bound"]


def _support(v, thr):
    return {tuple(i) for i in (v.abs() > thr).nonzero().tolist()}


@pytest.mark.parametrize("mean", D.MEANS)
def test_impulses(truth, mean):
    """One node off the truth.  With t = y the MSE part of the gradient vanishes, so dy = weight * scale * Dt(q) shows
    where q = m r is non-zero: the impulse's node and its in-grid neighbours, and Dt(q) on those and their
    neighbours."""
    t, x, kind, stats = truth[mean]

    def run(b, i, j):
        y = t[b:b + 1].clone()
        y[0, 0, i, j] += 1.0
        a = (y, y, x[b:b + 1], kind[b:b + 1], stats)
        got, dy = gpu_loss(*a, 1.0, mean)
        ref = reference(*a, 1.0, mean)
        check(f"{mean} impulse ({i},{j}) kind {KINDS[b]}", got, dy, ref)
        q = ref["out"]["q"].detach()
        thr = 1e-3 * float(ref["dy"].abs().max())
        assert thr > 2 * ref["dy_bound"]          # the threshold is above anything rounding can produce
        want = _support(ref["dy"][0, 0], thr)
        assert _support(dy[0, 0], thr) == want
        return _support(q[0, 0], 1e-6 * float(q.abs().max())), want
    q_sup, dy_sup = run(0, 0, 0)                  # kind 0, a corner
    assert q_sup == {(0, 0), (0, 1), (1, 0)}
    assert dy_sup == {(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)}
    q_sup, dy_sup = run(0, 0, 7)                  # kind 0, an edge
    assert q_sup == {(0, 6), (0, 7), (0, 8), (1, 7)}
    assert dy_sup == {(0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (1, 6), (1, 7), (1, 8), (2, 7)}
    q_sup, dy_sup = run(2, 20, 9)                 # kind 0, an interior node
    assert q_sup == {(20, 9), (19, 9), (21, 9), (20, 8), (20, 10)}
    assert len(dy_sup) == 13 and (18, 9) in dy_sup and (20, 11) in dy_sup and (19, 10) in dy_sup
    q_sup, dy_sup = run(1, 0, 5)                  # kind 1, a ring node: its own residual is masked
    assert q_sup == {(1, 5)}
    assert dy_sup == {(0, 5), (1, 4), (1, 5), (1, 6), (2, 5)}


@pytest.mark.parametrize("n", [3, 4, 17, 64])
def test_other_grids_through_the_raw_entry(n):
    """n = 3: one interior node; 4; 17: odd, two samples per workgroup; 64: the largest, one sample per workgroup and
    51 KiB of LDS.  Random fields with theta in [0.5, 2], kinds [0, 1, 1], both means."""
    from superresolution_for_pdes_amd import hipops as H
    g = torch.Generator().manual_seed(n)
    B = 3
    t = torch.randn(B, 1, n, n, generator=g, dtype=torch.float64)
    y = t + 0.05 * torch.randn(B, 1, n, n, generator=g, dtype=torch.float64)
    x = torch.randn(B, 3, n, n, generator=g, dtype=torch.float64)
    x[:, 1] = (0.5 + 1.5 * torch.rand(B, n, n, generator=g, dtype=torch.float64) - 1.25) / 0.43
    kind = torch.tensor([0, 1, 1], dtype=torch.int32)
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], dtype=torch.float64)
    inv_h2 = (float((n - 1) ** 2), float((2 * n - 1) ** 2))
    for code, mean in enumerate(D.MEANS):
        terms, unit = H.physics_loss_fwd(y.float().cuda(), t.float().cuda(), x.float().cuda(), kind.cuda(),
                                         stats.float().cuda(), WEIGHT, inv_h2, face_mean=code)
        dy = H.physics_loss_bwd(unit, None)
        ref = reference(y, t, x, kind, stats, WEIGHT, mean, inv_h2)
        assert ref["out"]["M"] == n * n + 2 * (n - 2) ** 2
        check(f"n={n} {mean}", terms.cpu().double().numpy(), dy.cpu(), ref)


def test_weight_zero_is_the_mse(truth):
    from superresolution_for_pdes_amd.functional import mse_loss
    t, x, kind, stats = truth["harmonic"]
    y = noisy(t, 1)
    got, dy = gpu_loss(y, t, x, kind, stats, 0.0, "harmonic")
    assert got[0] == got[1]
    y32, t32 = y.float().cuda().requires_grad_(True), t.float().cuda()
    plain = mse_loss(y32, t32)
    plain.backward()
    ulp = float(np.spacing(np.float32(plain.item())))
    assert abs(got[0] - float(plain)) <= 2 * ulp
    assert float((dy - y32.grad.cpu()).abs().max()) <= 4 * EPS * float(y32.grad.abs().max())


def test_determinism_grad_out_and_graph(truth):
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.functional import PhysicsMSELoss
    t, x, kind, stats = truth["arithmetic"]
    yp = noisy(t, 2).float().cuda()
    td, xd, kd, sd = t.float().cuda(), x.float().cuda(), kind.cuda(), stats.float().cuda()
    crit = PhysicsMSELoss(WEIGHT, sd, form="divergence", face_mean="arithmetic")

    def run(scale):
        yd = yp.clone().requires_grad_(True)
        loss = crit(yd, td, xd, kd)
        (scale * loss).backward()
        return loss.detach().clone(), yd.grad.clone(), crit.last_terms.clone()
    l1, g1, terms = run(1.0)
    l1b, g1b, _ = run(1.0)
    l3, g3, _ = run(3.0)
    assert torch.equal(l1, l1b) and torch.equal(g1, g1b)                  # bit-reproducible
    assert torch.equal(l3, l1) and torch.equal(g3, 3.0 * g1)              # grad_out scales the unit gradient
    assert terms.shape == (3,) and torch.equal(terms[0], l1)
    eager, eunit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0)
    assert torch.equal(eager, terms) and torch.equal(eunit, g1)
    quiet, unit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, want_grad=False, face_mean=0)
    assert unit is None and torch.equal(quiet, terms)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gt, gu = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0)
        dy = H.physics_loss_bwd(gu, gt[1:2])
    gt.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gt, eager) and torch.equal(gu, eunit) and torch.equal(dy, eunit * eager[1])


def test_pointwise_default_is_untouched(truth):
    """form="pointwise" spelled out is the call without the keywords, bit for bit, and differs from the divergence
    term on a variable theta."""
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    t, x, kind, stats = truth["harmonic"]
    args = (noisy(t, 3).float().cuda(), t.float().cuda(), x.float().cuda(), kind.cuda(), stats.float().cuda(), WEIGHT)
    a = physics_loss_terms(*args)
    b = physics_loss_terms(*args, form="pointwise", face_mean="harmonic")
    c = physics_loss_terms(*args, form="divergence")
    assert torch.equal(a, b) and not torch.equal(a[2], c[2]) and torch.equal(a[1], c[1])


def test_command_line_online_divergence(tmp_path):
    from superresolution_for_pdes_amd.train_enhanced import main
    hist = main(["--operator", "divergence", "--online", "2", "--online-theta", "0.5", "2.0", "--pde-div-weight",
                 "0.01", "--epochs", "2", "--batch-size", "8", "--results", str(tmp_path)])
    for k in ("train_loss", "val_loss", "train_mse", "train_pde", "val_mse", "val_pde"):
        assert len(hist[k]) == 2 and np.isfinite(hist[k]).all(), (k, hist[k])
    for loss, mse, pde in zip(hist["val_loss"], hist["val_mse"], hist["val_pde"]):
        assert abs(loss - (mse + 0.01 * pde)) <= 1e-6 * loss, (loss, mse, pde)
    (run,) = glob.glob(os.path.join(str(tmp_path), "enhanced_run_*"))
    rec = json.load(open(os.path.join(run, "physics_loss.json")))
    assert rec["weight"] == 0.01 and rec["form"] == "divergence" and rec["face_mean"] == "harmonic"
    assert rec["inv_h2"] == list(INV_H2) and len(rec["stats"]) == 6
