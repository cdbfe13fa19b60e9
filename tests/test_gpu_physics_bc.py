"""The divergence-form loss term with zero-flux (Neumann) sides on the GPU (csrc/physics.hip
physics_loss_kernel<DivLoss<HARM, true>>, ABI 23: srpde_physics_loss_div_fwd_bc) against restatement_div_bc of
tests/div_bc_smoother_ref.py in fp64, evaluated on the CPU from the kernel's own fp32 inputs (gradient: torch autograd
in fp64).

The tolerances are those of tests/test_gpu_physics_div.py, formula for formula (its module docstring derives them): a
missing face replaces a coefficient of at most max|theta| by an exact 0 and a ghost count of at most 2 by a smaller
one, so every term of that derivation bounds its counterpart here.  ``check``, EPS and WEIGHT are imported from there;
``reference`` below is its ``reference`` with the restatement exchanged."""
import numpy as np
import pytest
import torch

import div_bc_ref as B
import poisson_div_ref as D
from div_bc_smoother_ref import INV_H2, restatement_div_bc
from test_div_smoother_host import CROP, normalised
from test_gpu_physics_div import EPS, WEIGHT, check

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 0, 1)
PATTERNS = ("ddnn", "nddd", "nnnn")


def gpu_loss(y, t, x, kind, stats, weight, mean, bc, inv_h2=INV_H2, grad=True):
    """The kernel on fp32 copies of the inputs -> (terms [3] float64 numpy of the fp32 results, dy fp32 cpu or None)."""
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    yd = y.float().cuda().requires_grad_(grad)
    terms = physics_loss_terms(yd, t.float().cuda(), x.float().cuda(), kind.to(torch.int32).cuda(),
                               stats.float().cuda(), weight, inv_h2, form="divergence", face_mean=mean, bc=bc)
    if grad:
        terms[0].backward()
    return terms.detach().cpu().double().numpy(), (yd.grad.cpu() if grad else None)


def reference(y, t, x, kind, stats, weight, mean, bc, inv_h2=INV_H2):
    """The restatement on the same fp32 values, with its autograd gradient and the bounds of
    tests/test_gpu_physics_div.py's ``reference``."""
    y32, t32, x32, s32 = y.float(), t.float(), x.float(), stats.float()
    yd = y32.double().requires_grad_(True)
    out = restatement_div_bc(yd, t32, x32, kind, s32, weight, inv_h2, mean, bc)
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


@pytest.fixture(scope="module")
def truth():
    """{(mean, bc): (t, x, kind, stats)} fp64 on the CPU for bc in ("ddnn", "nddd"): B = 4 samples of kinds
    (0, 1, 0, 1) at n = 40, theta ~ U(0.5, 2): solve_div(bc=bc) solutions of 40^2 problems and 40^2 crops of 80^2
    ones, normalised with their own statistics.  Solved once and shared (never modified) by the tests below."""
    from superresolution_for_pdes_amd import poisson as P
    out = {}
    th40, th80 = D.field_theta(40, 11, 0.5, 2.0, B=2), D.field_theta(80, 12, 0.5, 2.0, B=2)
    f40 = np.stack([D.forcing(40), D.forcing(40, 1.4, 4.6)])
    f80 = np.stack([D.forcing(80, 2.3, 4.1), D.forcing(80)])
    i, j = CROP
    for mean in D.MEANS:
        for bc in ("ddnn", "nddd"):
            u40 = P.solve_div(f40, th40, face_mean=mean, bc=bc).cpu().numpy()
            u80 = P.solve_div(f80, th80, face_mean=mean, bc=bc).cpu().numpy()
            crop = [tuple(a[b, i + 3 * b:i + 3 * b + 40, j - 5 * b:j - 5 * b + 40] for a in (u80, f80, th80))
                    for b in range(2)]
            whole = [(u40[b], f40[b], th40[b]) for b in range(2)]
            rows = [whole[0], crop[0], whole[1], crop[1]]
            t, x, stats = normalised(*(np.stack([r[k] for r in rows]) for k in range(3)))
            out[mean, bc] = (t, x, torch.tensor(KINDS, dtype=torch.int32), stats)
    return out


def fields_for(truth, mean, bc):
    """The batch a pattern is compared on: its own solutions, or "ddnn"'s for "nnnn" (singular: nothing to solve)."""
    return truth[mean, "ddnn" if bc == "nnnn" else bc]


def noisy(t, seed=0, noise=1e-2):
    g = torch.Generator().manual_seed(seed)
    return t + noise * torch.randn(t.shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("mean", D.MEANS)
def test_perturbed_against_the_restatement(truth, mean, bc):
    """B = 4, two whole-domain samples and two crops, 1e-2 noise on y."""
    t, x, kind, stats = fields_for(truth, mean, bc)
    y = noisy(t)
    got, dy = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc)
    ref = reference(y, t, x, kind, stats, WEIGHT, mean, bc)
    assert ref["pde"] > 1e-3
    check(f"{mean} {bc} {KINDS}", got, dy, ref)
    assert abs(got[0] - (got[1] + WEIGHT * got[2])) <= 2 * EPS * got[0]
    # another pattern gives another value: the argument reaches the kernel
    other, _ = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, None, grad=False)
    assert abs(other[2] - got[2]) > 10 * ref["pde_bound"]


@pytest.mark.parametrize("bc", ("ddnn", "nddd"))
@pytest.mark.parametrize("mean", D.MEANS)
def test_term_vanishes_on_solutions(truth, mean, bc):
    """<= 5e-11 on the pattern's own solutions (the size tests/test_gpu_physics_div.py accepts); the bc-less term on
    the same whole-domain fields is at least 1e6 times larger."""
    t, x, kind, stats = truth[mean, bc]
    for b in range(len(KINDS)):
        s = slice(b, b + 1)
        got, _ = gpu_loss(t[s], t[s], x[s], kind[s], stats, 1.0, mean, bc, grad=False)
        plain, _ = gpu_loss(t[s], t[s], x[s], kind[s], stats, 1.0, mean, None, grad=False)
        print(f"{mean} {bc} sample {b} kind {KINDS[b]}: pde on the truth {got[2]:.3e}, without the pattern "
              f"{plain[2]:.3e}")
        assert got[2] <= 5e-11, (mean, bc, b, got[2])
        assert got[1] == 0.0 and got[0] == got[2]
        if KINDS[b] == 0:
            assert plain[2] >= 1e6 * max(got[2], 1e-30) and plain[2] > 1e-3
        else:
            assert plain[2] == got[2]               # a crop never sees the pattern
    got, _ = gpu_loss(t, t, x, kind, stats, 1.0, mean, bc, grad=False)
    assert got[2] <= 5e-11


@pytest.mark.parametrize("bc", ("ddnn", "nddd"))
@pytest.mark.parametrize("mean", D.MEANS)
def test_impulses(truth, mean, bc):
    """One node of a whole-domain sample off the truth -- on each side, in each corner, in the interior -- with t = y,
    so that dy is the adjoint alone: the face sum with missing faces applied to q = r.  It equals the autograd
    gradient of the restatement, which only a symmetric adjoint can."""
    t, x, kind, stats = truth[mean, bc]
    n = t.shape[-1]
    for i, j in ((0, 7), (n - 1, 7), (7, 0), (7, n - 1), (0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (20, 9)):
        y = t[0:1].clone()
        y[0, 0, i, j] += 1.0
        a = (y, y, x[0:1], kind[0:1], stats)
        got, dy = gpu_loss(*a, 1.0, mean, bc)
        ref = reference(*a, 1.0, mean, bc)
        check(f"{mean} {bc} impulse ({i},{j})", got, dy, ref)
        thr = 1e-3 * float(ref["dy"].abs().max())
        assert thr > 2 * ref["dy_bound"]            # the gradient is far above anything rounding can produce
        want = {tuple(k) for k in (ref["dy"][0, 0].abs() > thr).nonzero().tolist()}
        assert {tuple(k) for k in (dy[0, 0].abs() > thr).nonzero().tolist()} == want and (i, j) in want


@pytest.mark.parametrize("n", [3, 4, 17, 64])
def test_other_grids_through_the_raw_entry(n):
    """n = 3: one interior node; 4; 17: odd, two samples per workgroup; 64: the largest, one sample per workgroup.
    Random fields with theta in [0.5, 2], kinds [0, 1, 1], both means, "dnnd"."""
    from superresolution_for_pdes_amd import hipops as H
    bc = "dnnd"
    g = torch.Generator().manual_seed(n)
    Bn = 3
    t = torch.randn(Bn, 1, n, n, generator=g, dtype=torch.float64)
    y = t + 0.05 * torch.randn(Bn, 1, n, n, generator=g, dtype=torch.float64)
    x = torch.randn(Bn, 3, n, n, generator=g, dtype=torch.float64)
    x[:, 1] = (0.5 + 1.5 * torch.rand(Bn, n, n, generator=g, dtype=torch.float64) - 1.25) / 0.43
    kind = torch.tensor([0, 1, 1], dtype=torch.int32)
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], dtype=torch.float64)
    inv_h2 = (float((n - 1) ** 2), float((2 * n - 1) ** 2))
    for code, mean in enumerate(D.MEANS):
        terms, unit = H.physics_loss_fwd(y.float().cuda(), t.float().cuda(), x.float().cuda(), kind.cuda(),
                                         stats.float().cuda(), WEIGHT, inv_h2, face_mean=code, bc=B.mask(bc))
        dy = H.physics_loss_bwd(unit, None)
        ref = reference(y, t, x, kind, stats, WEIGHT, mean, bc, inv_h2)
        assert ref["out"]["M"] == n * n + 2 * (n - 2) ** 2
        check(f"n={n} {mean} {bc}", terms.cpu().double().numpy(), dy.cpu(), ref)


def test_weight_zero_is_the_mse(truth):
    from superresolution_for_pdes_amd.functional import mse_loss
    t, x, kind, stats = truth["harmonic", "ddnn"]
    y = noisy(t, 1)
    got, dy = gpu_loss(y, t, x, kind, stats, 0.0, "harmonic", "ddnn")
    assert got[0] == got[1]
    y32, t32 = y.float().cuda().requires_grad_(True), t.float().cuda()
    plain = mse_loss(y32, t32)
    plain.backward()
    ulp = float(np.spacing(np.float32(plain.item())))
    assert abs(got[0] - plain.item()) <= 2 * ulp
    assert float((dy - y32.grad.cpu()).abs().max()) <= 4 * EPS * float(y32.grad.abs().max())


def test_determinism_grad_out_and_graph(truth):
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.functional import PhysicsMSELoss
    t, x, kind, stats = truth["arithmetic", "ddnn"]
    mask = B.mask("ddnn")
    yp = noisy(t, 2).float().cuda()
    td, xd, kd, sd = t.float().cuda(), x.float().cuda(), kind.cuda(), stats.float().cuda()
    crit = PhysicsMSELoss(WEIGHT, sd, form="divergence", face_mean="arithmetic", bc="ddnn")

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
    eager, eunit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0, bc=mask)
    assert torch.equal(eager, terms) and torch.equal(eunit, g1)
    quiet, unit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, want_grad=False, face_mean=0, bc=mask)
    assert unit is None and torch.equal(quiet, terms)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0, bc=mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gt, gu = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, INV_H2, face_mean=0, bc=mask)
        dy = H.physics_loss_bwd(gu, gt[1:2])
    gt.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gt, eager) and torch.equal(gu, eunit) and torch.equal(dy, eunit * eager[1])


@pytest.mark.parametrize("mean", D.MEANS)
def test_no_pattern_is_the_existing_entry(truth, mean):
    """bc = None / "dddd" (and the raw mask 0) reproduce the bits of the call without the keyword, loss and gradient."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    t, x, kind, stats = truth[mean, "ddnn"]
    y = noisy(t, 3)
    args = (t.float().cuda(), x.float().cuda(), kind.cuda(), stats.float().cuda(), WEIGHT)

    def run(**kw):
        yd = y.float().cuda().requires_grad_(True)
        terms = physics_loss_terms(yd, *args, form="divergence", face_mean=mean, **kw)
        terms[0].backward()
        return terms.detach(), yd.grad
    base, gbase = run()
    for bc in (None, "dddd"):
        terms, grad = run(bc=bc)
        assert torch.equal(terms, base) and torch.equal(grad, gbase)
    code = D.MEANS.index(mean)
    raw0, unit0 = H.physics_loss_fwd(y.float().cuda(), *args[:4], WEIGHT, INV_H2, face_mean=code, bc=0)
    assert torch.equal(raw0, base) and torch.equal(unit0, gbase)
    terms, grad = run(bc="ddnn")
    assert not torch.equal(terms[2], base[2]) and torch.equal(terms[1], base[1]) and not torch.equal(grad, gbase)
