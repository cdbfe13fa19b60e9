"""The fp64 references of tests/fused_bwd_ref.py against torch autograd in fp64 (no GPU): the BN + ReLU backward
with the convolution's input and weight gradients, the max-pool routing with ties, the gate-input gradient and the
inference head -- agreement to 1e-12 relative.  And the GPU tests' input recipe on every shape and seed they use:
nothing inside the ReLU-mask margin, 20 % .. 80 % of the elements masked, a negative gamma in every channel octet."""
import pytest
import torch
import torch.nn.functional as F

import fused_bwd_ref as R

F64 = torch.float64
TOL = 1e-12


def rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _conv_bn_relu_case(n, cin, cout, h, w, dil, seed, gamma_sign=None, beta_scale=0.2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g, dtype=F64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64) * (2.0 / (9 * cin)) ** 0.5
    gamma = torch.rand(cout, generator=g, dtype=F64) + 0.5
    if gamma_sign is not None:
        gamma = gamma * gamma_sign(cout)
    beta = torch.randn(cout, generator=g, dtype=F64) * beta_scale
    da = torch.randn(n, cout, h, w, generator=g, dtype=F64)
    return x, wt, gamma, beta, da


@pytest.mark.parametrize("n,cin,cout,h,w,dil,kind", [
    (2, 8, 16, 6, 6, 1, "plain"),
    (3, 4, 8, 7, 5, 1, "negative_gamma"),        # every second channel's gamma negative
    (2, 8, 8, 5, 9, 2, "large_beta"),            # |beta| ~ 1: the mask is not the sign of xhat * gamma
    (1, 3, 4, 4, 4, 1, "negative_gamma"),
])
def test_bn_relu_conv_backward_matches_autograd(n, cin, cout, h, w, dil, kind):
    sign = (lambda c: torch.tensor([(-1.0) ** k for k in range(c)], dtype=F64)) if kind == "negative_gamma" else None
    x, wt, gamma, beta, da = _conv_bn_relu_case(n, cin, cout, h, w, dil, 100 + n + cout + h, sign)
    if kind == "large_beta":
        beta = torch.where(torch.arange(cout) % 2 == 0, 1.0, -1.0).to(F64) * (0.9 + 0.2 * torch.rand(cout, dtype=F64))
    xv, wv, gv, bv = (t.clone().requires_grad_(True) for t in (x, wt, gamma, beta))
    yv = F.conv2d(xv, wv, None, padding=dil, dilation=dil)
    yv.retain_grad()
    a = F.relu(F.batch_norm(yv, None, None, gv, bv, True, 0.1, R.BN_EPS))
    a.backward(da)
    y = yv.detach()
    mean = y.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.var(dim=(0, 2, 3), unbiased=False) + R.BN_EPS)
    yr, dar = R.to_rows(y), R.to_rows(da)
    dy, m1, m2, dgamma, dbeta = R.bn_relu_bwd_ref(yr, dar, mean, invstd, gamma, beta)
    P = yr.shape[0]
    assert rel(R.to_nchw(dy, n, h, w), yv.grad) < TOL
    assert rel(dgamma, gv.grad) < TOL and rel(dbeta, bv.grad) < TOL
    assert torch.equal(m1, dbeta / P) and torch.equal(m2, dgamma / P)
    assert rel(R.to_nchw(R.conv_dgrad_ref(dy, wt, n, h, w, dil), n, h, w), xv.grad) < TOL
    assert rel(R.conv_wgrad_ref(dy, R.to_rows(x), n, h, w, dil), wv.grad) < TOL
    # the mask really depends on beta and on gamma's sign in these cases
    xhat = (yr - mean) * invstd
    if kind != "plain":
        assert bool(((xhat * gamma + beta > 0) != (xhat > 0)).any())
    # m1 / m2 handed in replace the sums' in the apply only
    dy2, r1, r2, _, _ = R.bn_relu_bwd_ref(yr, dar, mean, invstd, gamma, beta, m1=m1 * 0, m2=m2 * 0)
    dy_eval = R.bn_relu_bwd_ref(yr, dar, mean, invstd, gamma, beta, eval_mode=True)[0]
    assert torch.equal(r1, m1) and torch.equal(r2, m2) and torch.equal(dy2, dy_eval)


def test_bn_backward_eval_mode_and_no_relu_match_autograd():
    g = torch.Generator().manual_seed(5)
    P, C = 60, 12
    y = torch.randn(P, C, generator=g, dtype=F64) * 2 + 0.5
    da = torch.randn(P, C, generator=g, dtype=F64)
    gamma = torch.randn(C, generator=g, dtype=F64)
    beta = torch.randn(C, generator=g, dtype=F64)
    rm = torch.randn(C, generator=g, dtype=F64)
    rv = torch.rand(C, generator=g, dtype=F64) + 0.3
    invstd = 1.0 / torch.sqrt(rv + R.BN_EPS)
    for relu in (True, False):
        yv, gv, bv = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
        a = F.batch_norm(yv, rm, rv, gv, bv, False, 0.1, R.BN_EPS)
        (F.relu(a) if relu else a).backward(da)
        dy, m1, m2, dgamma, dbeta = R.bn_relu_bwd_ref(y, da, rm, invstd, gamma, beta, relu=relu, eval_mode=True)
        assert not bool(m1.any()) and not bool(m2.any())
        assert rel(dy, yv.grad) < TOL and rel(dgamma, gv.grad) < TOL and rel(dbeta, bv.grad) < TOL
    # train mode without the ReLU
    yv, gv, bv = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    F.batch_norm(yv, None, None, gv, bv, True, 0.1, R.BN_EPS).backward(da)
    mean, invstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + R.BN_EPS)
    dy, _, _, dgamma, dbeta = R.bn_relu_bwd_ref(y, da, mean, invstd, gamma, beta, relu=False)
    assert rel(dy, yv.grad) < TOL and rel(dgamma, gv.grad) < TOL and rel(dbeta, bv.grad) < TOL


@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 4, 6, 8), (3, 6, 10, 16)])
def test_att_pool_backward_matches_autograd_with_ties(shape):
    n, h, w, c = shape
    case = R.att_pool_case(n, h, w, c, 40 + h)
    a64 = R.d(case["a"])
    ev = R.to_nchw(a64, n, h, w).requires_grad_(True)
    dout, dp = R.to_nchw(R.d(case["dout"]), n, h, w), R.to_nchw(R.d(case["dp"]), n, h // 2, w // 2)
    ca, dm = R.d(case["ca"]).view(n, c, 1, 1), R.d(case["dm"]).view(n, c, 1, 1)
    sa = R.d(case["sa"]).view(n, 1, h, w)
    loss = (ev * ca * sa * dout).sum() + (ev * dm).sum() + (F.max_pool2d(ev, 2) * dp).sum()
    loss.backward()
    de, mag = R.att_pool_bwd_ref(case["dout"], case["ca"], case["sa"], case["dm"], case["a"], case["dp"], n, h, w,
                                 parts=True)
    assert rel(R.to_nchw(de, n, h, w), ev.grad) < TOL
    assert bool((mag >= de.abs() - 1e-15).all())
    # the forced ties are there: an all-zero window, and windows whose maximum is attained more than once
    v = a64.reshape(n, h // 2, 2, w // 2, 2, c)
    top = v.amax(dim=(2, 4), keepdim=True)
    assert bool((top == 0).any())
    if n * (h // 2) * (w // 2) >= 4:
        hits = (v == top).sum(dim=(2, 4))
        assert bool((hits == 2).any()) and bool((hits == 4).any())
        idx = R.first_max_2x2(case["a"], n, h, w)
        assert bool((idx == 1).any()) and bool((idx == 0).any())
    zeros = float((a64 == 0).double().mean())
    assert 0.2 < zeros < 0.6 or n * h * w == 4, zeros


def test_first_max_order_is_row_major_with_strict_greater():
    a = torch.tensor([[1.0], [3.0], [3.0], [2.0]])          # window (0,0)=1 (0,1)=3 (1,0)=3 (1,1)=2
    assert int(R.first_max_2x2(a, 1, 2, 2)) == 1
    assert int(R.first_max_2x2(torch.zeros(4, 1), 1, 2, 2)) == 0
    assert int(R.first_max_2x2(torch.tensor([[0.0], [0.0], [0.0], [1.0]]), 1, 2, 2)) == 3
    assert int(R.first_max_2x2(torch.tensor([[0.0], [0.0], [2.0], [2.0]]), 1, 2, 2)) == 2


@pytest.mark.parametrize("n,h,w,bias", [(2, 6, 6, True), (1, 7, 5, True), (3, 4, 9, False)])
def test_head_eval_matches_conv2d_chain(n, h, w, bias):
    g = torch.Generator().manual_seed(n + h + w)
    z = torch.relu(torch.randn(n, 32, h, w, generator=g, dtype=F64))
    wt = torch.randn(16, 32, 3, 3, generator=g, dtype=F64) * (2.0 / 288) ** 0.5
    b = torch.randn(16, generator=g, dtype=F64) * 0.1 if bias else None
    gamma, beta, rm, _ = (t.double() for t in R.bn_params(16, g))
    rv = torch.rand(16, generator=g, dtype=F64) + 0.2
    wf = torch.randn(1, 16, 1, 1, generator=g, dtype=F64)
    bf = torch.randn(1, generator=g, dtype=F64)
    xin = torch.randn(n, 3, h, w, generator=g, dtype=F64)
    o = F.relu(F.batch_norm(F.conv2d(z, wt, b, padding=1), rm, rv, gamma, beta, False, 0.1, R.BN_EPS))
    want = F.conv2d(o, wf, bf) + xin[:, :1]
    got = R.head_eval_ref(R.to_rows(z), wt, b, rm, 1.0 / torch.sqrt(rv + R.BN_EPS), gamma, beta, wf, bf, xin)
    assert rel(got, want.reshape(-1)) < TOL
    assert bool((gamma < 0).any())


def _recipe_cases():
    for P, C in R.PREPARE_SHAPES:
        for batch in (False, True):
            yield f"prepare P={P} C={C} batch={batch}", R.case_prepare(P, C, batch), batch
    for s in R.DGRAD_SHAPES:
        top, below = R.case_dgrad(s)
        yield f"dgrad {s}", top, False
        yield f"dgrad below {s}", below, False
    for s in R.WGRAD_SHAPES:
        yield f"wgrad {s}", R.case_wgrad(s), False
    for s in R.ATT_POOL_SHAPES:
        yield f"att_pool {s}", R.case_att_pool(s), False


def test_input_recipe_meets_its_conditions_for_every_gpu_case():
    for name, case, batch in _recipe_cases():
        try:
            R.check_bn_case(case)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
        if batch:   # the statistics are the batch's (to their fp32 rounding) after the margin moves
            mean, invstd = R.batch_stats(case["y"])
            assert torch.equal(mean, case["mean"]) and torch.equal(invstd, case["invstd"]), name
        for t in case.values():
            assert t.dtype == torch.float32
    # the recipe is deterministic: the GPU tests and this check see the same tensors
    a, b = R.case_prepare(87, 48, True), R.case_prepare(87, 48, True)
    assert all(torch.equal(a[k], b[k]) for k in a)
