"""The divergence-form loss term with boundary data on the GPU (csrc/physics.hip
physics_loss_kernel<DivLoss<HARM, true, true>>, ABI 23 extended: srpde_physics_loss_div_fwd_bd) against
restatement_div_bd of tests/stream_bd_ref.py in fp64, evaluated on the CPU from the kernel's own fp32 inputs (gradient:
torch autograd in fp64).

The tolerances are the formulas of tests/test_gpu_physics_div.py (its module docstring derives them): there the
residual's error delta scales with c max|theta| max|y|, the size of the face sum's terms after the factor
c = u_std inv_h2 / f_std.  The affine term adds terms of the size max|beta| inv_h2 / f_std (a product theta_a g, up to
two per node, one pair sum, one sum with the face term) and max|Q| inv_h / f_std (up to two q, their sum, one product,
one sum): a handful of roundings each, far inside the factor 64 that the four faces' 56 roundings left, so the same
factor multiplies the enlarged magnitude
    delta = 64 eps (c max|theta| max|y| + (max|beta| inv_h2 + max|Q| inv_h) / f_std) + 4 eps max|r|
and the bounds on pde, mse and dy follow from delta as there.  ``check``, EPS and WEIGHT are imported from there."""
import numpy as np
import pytest
import torch

import div_bc_ref as B
import div_bd_ref as BD
import poisson_div_ref as D
import stream_bd_ref as S
from test_div_smoother_host import normalised
from test_gpu_physics_div import EPS, WEIGHT, check

pytestmark = pytest.mark.gpu

KINDS = (0, 0, 1, 1)
PATTERNS = (None, "ddnn", "ndnd", "nnnn")
SIZES = (3, 5, 33, 64)      # 3: every node an edge node, corners take two sides; 5; 33: odd, two samples per workgroup;
#                             64: the LDS limit, one sample per workgroup


def _inv_h2(n):
    return (float((n - 1) ** 2), float((2 * n - 1) ** 2))


def batch(n, seed=0):
    """Random fp64 fields of kinds (0, 0, 1, 1) on the CPU, theta in [0.5, 2], data [4, 4, n] of unit size."""
    g = torch.Generator().manual_seed(100 * n + seed)
    Bn = len(KINDS)
    t = torch.randn(Bn, 1, n, n, generator=g, dtype=torch.float64)
    y = t + 0.05 * torch.randn(Bn, 1, n, n, generator=g, dtype=torch.float64)
    x = torch.randn(Bn, 3, n, n, generator=g, dtype=torch.float64)
    x[:, 1] = (0.5 + 1.5 * torch.rand(Bn, n, n, generator=g, dtype=torch.float64) - 1.25) / 0.43
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], dtype=torch.float64)
    bd = torch.randn(Bn, 4, n, generator=g, dtype=torch.float64)
    return y, t, x, torch.tensor(KINDS, dtype=torch.int32), stats, bd


def gpu_loss(y, t, x, kind, stats, weight, mean, bc, bd, inv_h2, grad=True):
    """The kernel on fp32 copies of the inputs -> (terms [3] fp32 on the device, dy fp32 on the device or None)."""
    from superresolution_for_pdes_amd.functional import physics_loss_terms
    yd = y.float().cuda().requires_grad_(grad)
    terms = physics_loss_terms(yd, t.float().cuda(), x.float().cuda(), kind.to(torch.int32).cuda(),
                               stats.float().cuda(), weight, inv_h2, form="divergence", face_mean=mean, bc=bc,
                               bc_data=None if bd is None else bd.cuda())
    if grad:
        terms[0].backward()
    return terms.detach(), (yd.grad if grad else None)


def reference(y, t, x, kind, stats, weight, mean, bc, bd, inv_h2):
    """The restatement on the same fp32 values (the data cast to fp32 as the wrapper casts it), with its autograd
    gradient and the bounds of the module docstring."""
    y32, t32, x32, s32 = y.float(), t.float(), x.float(), stats.float()
    bd32 = None if bd is None else bd.float()
    yd = y32.double().requires_grad_(True)
    out = S.restatement_div_bd(yd, t32, x32, kind, s32, weight, inv_h2, mean, bc, bd32)
    out["total"].backward()
    sg_u, sg_f = float(s32[1]), float(s32[3])
    c = sg_u * max(inv_h2[int(k != 0)] for k in kind.tolist()) / sg_f
    th_max = float(out["theta"].abs().max())
    r_max = float((out["m"] * out["r"]).detach().abs().max())
    q_max = float(out["q"].detach().abs().max())
    affine = (float(out["beta"].abs().max()) * inv_h2[0] + float(out["flux"].abs().max())) / sg_f
    delta = 64 * EPS * (c * th_max * float(y32.abs().max()) + affine) + 4 * EPS * r_max
    pde, mse = float(out["pde"].detach()), float(out["mse"].detach())
    N = y32.numel()
    return {"pde": pde, "mse": mse, "total": float(out["total"].detach()), "dy": yd.grad, "out": out, "delta": delta,
            "pde_bound": 2 * np.sqrt(pde) * delta + delta * delta, "mse_bound": 4 * EPS * mse,
            "dy_bound": weight * (2 * c / out["M"]) * (8 * th_max * delta + 64 * EPS * th_max * q_max)
            + (2.0 / N) * 4 * EPS * float((y32 - t32).abs().max())}


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_terms_and_gradient_against_the_restatement(n, bc):
    y, t, x, kind, stats, bd = batch(n)
    inv_h2 = _inv_h2(n)
    for mean in D.MEANS:
        terms, dy = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, bd, inv_h2)
        ref = reference(y, t, x, kind, stats, WEIGHT, mean, bc, bd, inv_h2)
        assert ref["out"]["M"] == 2 * n * n + 2 * (n - 2) ** 2
        got = terms.cpu().double().numpy()
        check(f"n={n} {mean} {bc}", got, dy.cpu(), ref)
        assert abs(got[0] - (got[1] + WEIGHT * got[2])) <= 2 * EPS * got[0]
        # the data reaches the kernel: without it the term and the gradient are other numbers
        plain, gplain = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, None, inv_h2)
        assert not torch.equal(plain[2], terms[2]) and not torch.equal(gplain[:2], dy[:2])
        assert torch.equal(gplain[2:], dy[2:])                # a crop never sees the data


@pytest.mark.parametrize("bc", PATTERNS)
@pytest.mark.parametrize("n", (3, 33, 64))
def test_zero_data_gives_the_bits_of_the_pattern_call(n, bc):
    """Terms and dy are torch.equal to the bc= call's (signed zeros compare equal), per sample and shared; NaN in the
    kind-1 rows changes nothing, since those rows are never read; shared [4, n] data equals the same data repeated."""
    y, t, x, kind, stats, bd = batch(n, 1)
    inv_h2 = _inv_h2(n)
    for mean in D.MEANS:
        base, gbase = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, None, inv_h2)
        for zero in (torch.zeros_like(bd), torch.zeros(4, n, dtype=torch.float64), torch.zeros(1, 4, n)):
            terms, dy = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, zero, inv_h2)
            assert torch.equal(terms, base) and torch.equal(dy, gbase), (mean, tuple(zero.shape))
        want, gwant = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, bd, inv_h2)
        assert not torch.equal(want[2], base[2])
        poisoned = bd.clone()
        poisoned[2:] = float("nan")
        terms, dy = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, poisoned, inv_h2)
        assert bool(torch.isfinite(terms).all()) and bool(torch.isfinite(dy).all())
        assert torch.equal(terms, want) and torch.equal(dy, gwant)
        one = bd[0]
        shared, gshared = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, one, inv_h2)
        again, gagain = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, one[None], inv_h2)
        repeated, grepeated = gpu_loss(y, t, x, kind, stats, WEIGHT, mean, bc, one.expand(len(KINDS), 4, n).contiguous(),
                                       inv_h2)
        assert torch.equal(shared, repeated) and torch.equal(gshared, grepeated)
        assert torch.equal(again, repeated) and torch.equal(gagain, grepeated)
        assert not torch.equal(shared[2], want[2])


@pytest.fixture(scope="module")
def truth():
    """{(mean, bc): (t, x, kind, stats, bd)} for bc in (None, "ddnn"): two solve_div(bc_data=) solutions on 40^2 with
    theta ~ U(0.5, 2) and unit-size data, normalised with their own statistics.  Solved once, shared, never modified."""
    from superresolution_for_pdes_amd import poisson as P
    out = {}
    th = D.field_theta(40, 11, 0.5, 2.0, B=2)
    f = np.stack([D.forcing(40), D.forcing(40, 1.4, 4.6)])
    bd = BD.data(40, 3, 2)
    for mean in D.MEANS:
        for bc in (None, "ddnn"):
            u = P.solve_div(f, th, face_mean=mean, bc=bc, bc_data=bd).cpu().numpy()
            t, x, stats = normalised(u, f, th)
            out[mean, bc] = (t, x, torch.zeros(2, dtype=torch.int32), stats, torch.from_numpy(bd))
    return out


@pytest.mark.parametrize("bc", (None, "ddnn"))
@pytest.mark.parametrize("mean", D.MEANS)
def test_term_vanishes_on_solutions(truth, mean, bc):
    """On solve_div(bc_data=) solutions cast to fp32 the data-less loss of the same fields is at least 1e6 times the
    loss with the data -- the criterion of tests/test_gpu_physics_bc.py."""
    t, x, kind, stats, bd = truth[mean, bc]
    inv_h2 = _inv_h2(40)
    for b in range(2):
        s = slice(b, b + 1)
        got, _ = gpu_loss(t[s], t[s], x[s], kind[s], stats, 1.0, mean, bc, bd[s], inv_h2, grad=False)
        plain, _ = gpu_loss(t[s], t[s], x[s], kind[s], stats, 1.0, mean, bc, None, inv_h2, grad=False)
        got, plain = got.cpu().double().numpy(), plain.cpu().double().numpy()
        print(f"{mean} {bc} sample {b}: pde on the truth {got[2]:.3e}, with the data withheld {plain[2]:.3e}")
        assert got[1] == 0.0 and got[0] == got[2]
        assert plain[2] >= 1e6 * max(got[2], 1e-30) and plain[2] > 1e-3


def test_determinism_grad_out_and_graph(truth):
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.functional import PhysicsMSELoss
    t, x, kind, stats, bd = truth["arithmetic", "ddnn"]
    mask, inv_h2 = B.mask("ddnn"), _inv_h2(40)
    g = torch.Generator().manual_seed(2)
    yp = (t + 1e-2 * torch.randn(t.shape, generator=g, dtype=torch.float64)).float().cuda()
    td, xd, kd, sd, bdd = t.float().cuda(), x.float().cuda(), kind.cuda(), stats.float().cuda(), bd.float().cuda()
    crit = PhysicsMSELoss(WEIGHT, sd, inv_h2, form="divergence", face_mean="arithmetic", bc="ddnn", bc_data=True)

    def run(scale):
        yd = yp.clone().requires_grad_(True)
        loss = crit(yd, td, xd, kd, bdd)
        (scale * loss).backward()
        return loss.detach().clone(), yd.grad.clone(), crit.last_terms.clone()
    l1, g1, terms = run(1.0)
    l1b, g1b, _ = run(1.0)
    l3, g3, _ = run(3.0)
    assert torch.equal(l1, l1b) and torch.equal(g1, g1b)                  # bit-reproducible
    assert torch.equal(l3, l1) and torch.equal(g3, 3.0 * g1)              # grad_out scales the unit gradient
    assert terms.shape == (3,) and torch.equal(terms[0], l1)
    with pytest.raises(ValueError, match="needs the batch's boundary data"):
        crit(yp, td, xd, kd)
    eager, eunit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, inv_h2, face_mean=0, bc=mask, bd=bdd)
    assert torch.equal(eager, terms) and torch.equal(eunit, g1)
    quiet, unit = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, inv_h2, want_grad=False, face_mean=0, bc=mask, bd=bdd)
    assert unit is None and torch.equal(quiet, terms)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, inv_h2, face_mean=0, bc=mask, bd=bdd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gt, gu = H.physics_loss_fwd(yp, td, xd, kd, sd, WEIGHT, inv_h2, face_mean=0, bc=mask, bd=bdd)
        dy = H.physics_loss_bwd(gu, gt[1:2])
    gt.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gt, eager) and torch.equal(gu, eunit) and torch.equal(dy, eunit * eager[1])
