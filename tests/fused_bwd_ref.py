"""fp64 references (torch CPU, no GPU) of the operations behind the fused BN-backward and eval-head kernels, and
the seeded input recipe their GPU tests share (tests/test_gpu_fused_bwd_kernels.py).

Activations are NHWC row tensors [P, C] (P = n * h * w), as the kernels take them; everything is computed in
float64 whatever the inputs' type.  tests/test_fused_bwd_ref_host.py validates these functions against torch
autograd in fp64 and checks the recipe's conditions for every shape and seed the GPU tests use.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
U32 = 2.0 ** -24          # fp32 unit roundoff


def d(t):
    return t.detach().to("cpu", F64)


def to_nchw(r, n, h, w):
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def to_rows(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


# ------------------------------------------ references ------------------------------------------
def bn_relu_bwd_ref(y, da, mean, invstd, gamma, beta, relu=True, eval_mode=False, m1=None, m2=None):
    """Backward of a = relu(bn(y)) for given (mean, invstd) -> dy, m1, m2, dgamma, dbeta.
    xhat = (y - mean) * invstd; dz = da where xhat * gamma + beta > 0 (everywhere without the ReLU);
    m1 = sum(dz) / P, m2 = sum(dz * xhat) / P (both 0 in eval mode: the statistics are constants);
    dy = gamma * invstd * (dz - m1 - xhat * m2); dgamma = sum(dz * xhat), dbeta = sum(dz).
    ``m1`` / ``m2`` given: the apply uses them (a kernel's own fp32 values) instead of the sums' -- the
    returned m1 / m2 are still the sums'."""
    y, da, mean, invstd, gamma, beta = (d(t) for t in (y, da, mean, invstd, gamma, beta))
    P = y.shape[0]
    xhat = (y - mean) * invstd
    dz = torch.where(xhat * gamma + beta > 0, da, torch.zeros_like(da)) if relu else da.clone()
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    r1 = torch.zeros_like(dbeta) if eval_mode else dbeta / P
    r2 = torch.zeros_like(dgamma) if eval_mode else dgamma / P
    a1 = r1 if m1 is None else d(m1)
    a2 = r2 if m2 is None else d(m2)
    dy = gamma * invstd * (dz - a1 - xhat * a2)
    return dy, r1, r2, dgamma, dbeta


def bn_bwd_terms(y, da, mean, invstd, gamma, beta, relu=True):
    """sum|dz| and sum|dz * xhat| per channel: the magnitudes an fp32 summation's error bound scales with."""
    y, da, mean, invstd, gamma, beta = (d(t) for t in (y, da, mean, invstd, gamma, beta))
    xhat = (y - mean) * invstd
    dz = torch.where(xhat * gamma + beta > 0, da, torch.zeros_like(da)) if relu else da
    return dz.abs().sum(0), (dz * xhat).abs().sum(0)


def bn_bwd_apply_terms(y, da, mean, invstd, gamma, beta, m1, m2, relu=True):
    """|gamma invstd| (|dz| + |m1| + |xhat m2|) per element: what the fp32 rounding of the apply scales with."""
    y, da, mean, invstd, gamma, beta, m1, m2 = (d(t) for t in (y, da, mean, invstd, gamma, beta, m1, m2))
    xhat = (y - mean) * invstd
    dz = torch.where(xhat * gamma + beta > 0, da, torch.zeros_like(da)) if relu else da
    return (gamma * invstd).abs() * (dz.abs() + m1.abs() + (xhat * m2).abs())


def conv_dgrad_ref(dy, w, n, h, wd, dil):
    """Input gradient of conv3x3(padding = dilation = dil): dy [P, Cout] rows, w [Cout, Cin, 3, 3] -> dx [P, Cin]."""
    w = d(w)
    dyn = to_nchw(d(dy), n, h, wd)
    dx = torch.nn.grad.conv2d_input((n, w.shape[1], h, wd), w, dyn, padding=dil, dilation=dil)
    return to_rows(dx)


def conv_wgrad_ref(dy, x, n, h, wd, dil, ksize=3):
    """Weight gradient of the same convolution: dy [P, Cout], x [P, Cin] rows -> dw [Cout, Cin, k, k]."""
    dyn = to_nchw(d(dy), n, h, wd)
    xn = to_nchw(d(x), n, h, wd)
    pad = dil * (ksize // 2)
    return torch.nn.grad.conv2d_weight(xn, (dyn.shape[1], xn.shape[1], ksize, ksize), dyn, padding=pad, dilation=dil)


def first_max_2x2(a, n, h, w):
    """Index 0..3 of the first maximum of every 2x2 window of a [P, c], windows in (n, oy, ox) order -> [P/4, c].
    The order compared is maxpool2_bwd_px_kernel's: (0,0), (0,1), (1,0), (1,1), a strict > replacing the maximum."""
    c = a.shape[1]
    v = d(a).reshape(n, h // 2, 2, w // 2, 2, c)
    cand = [v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1]]
    best = cand[0].clone()
    idx = torch.zeros(best.shape, dtype=torch.int64)
    for k in (1, 2, 3):
        m = cand[k] > best
        idx = torch.where(m, torch.full_like(idx, k), idx)
        best = torch.where(m, cand[k], best)
    return idx.reshape(-1, c)


def att_pool_bwd_ref(dout, ca, sa, dm, a, dp, n, h, w, parts=False):
    """Gradient of an encoder output that feeds an AttentionGate and a 2x2 max-pool: dout * sa * ca + dm[n]
    (dout [P, c], sa [P], ca / dm [n, c]) plus dp [P/4, c] routed to the first maximum of each window of a.
    ``parts``: also |dout sa ca| + |dm| + |dp routed|, the magnitudes of the three summands."""
    c = a.shape[1]
    dout, ca, sa, dm, dp = (d(t) for t in (dout, ca, sa, dm, dp))
    hw = h * w
    gate = dout * sa.reshape(-1, 1) * ca.repeat_interleave(hw, 0)
    dmr = dm.repeat_interleave(hw, 0)
    idx = first_max_2x2(a, n, h, w).reshape(n, h // 2, w // 2, c)
    routed = torch.zeros(n, h // 2, 2, w // 2, 2, c, dtype=F64)
    dpv = dp.reshape(n, h // 2, w // 2, c)
    for k, (dy_, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        routed[:, :, dy_, :, dx_] = torch.where(idx == k, dpv, torch.zeros_like(dpv))
    routed = routed.reshape(n * hw, c)
    de = gate + dmr + routed
    if parts:
        return de, gate.abs() + dmr.abs() + routed.abs()
    return de


def head_eval_ref(z, w, bias, mean, invstd, gamma, beta, wf, bf, xin):
    """The U-Net's inference head: conv3x3(32 -> 16, padding 1) -> BN with the given statistics -> ReLU -> 1x1
    (16 -> 1) -> + xin[:, 0].  z [P, 32] rows, w [16, 32, 3, 3], wf 16 weights, bf 1, xin [n, C, h, w] -> [P]."""
    n, _, h, wd = xin.shape
    zn = to_nchw(d(z), n, h, wd)
    o = F.conv2d(zn, d(w), None if bias is None else d(bias), padding=1)
    o = (o - d(mean).view(1, -1, 1, 1)) * d(invstd).view(1, -1, 1, 1) * d(gamma).view(1, -1, 1, 1) \
        + d(beta).view(1, -1, 1, 1)
    o = torch.relu(o)
    out = F.conv2d(o, d(wf).reshape(1, -1, 1, 1), d(bf).reshape(1)) + d(xin)[:, :1]
    return out.reshape(-1)


# ----------------------------------------- input recipe -----------------------------------------
MARGIN = 1e-3     # no |xhat * gamma + beta| below this: the fp32 and fp64 ReLU masks then agree
BN_EPS = 1e-5


def bn_params(C, g):
    """gamma = +-(0.5 + rand) with random signs and at least one negative channel in every group of 8,
    beta ~ N(0, 0.5), mean ~ N(0.5, 1), invstd ~ 0.3 + rand -- fp32."""
    gamma = 0.5 + torch.rand(C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    for c0 in range(0, C, 8):
        if not bool((sign[c0:c0 + 8] < 0).any()):
            sign[c0 + int(torch.randint(0, min(8, C - c0), (1,), generator=g))] = -1.0
    gamma = gamma * sign
    beta = torch.randn(C, generator=g) * 0.5
    mean = torch.randn(C, generator=g) + 0.5
    invstd = 0.3 + torch.rand(C, generator=g)
    return gamma, beta, mean, invstd


def _bn_out(y, mean, invstd, gamma, beta):
    return (d(y) - d(mean)) * d(invstd) * d(gamma) + d(beta)


def _push_out_of_margin(y, mean, invstd, gamma, beta):
    """every element with |bn| < MARGIN moves by 4 * MARGIN / (|gamma| invstd) in y, away from the mask's edge"""
    bn = _bn_out(y, mean, invstd, gamma, beta)
    near = bn.abs() < MARGIN
    if bool(near.any()):
        s = torch.where(bn >= 0, 1.0, -1.0).to(F64) * torch.sign(d(gamma))
        step = 4 * MARGIN * s / (d(gamma).abs() * d(invstd))
        y = torch.where(near, d(y) + step, d(y)).float()
    return y


def batch_stats(y):
    yd = d(y)
    return yd.mean(0).float(), (1.0 / torch.sqrt(yd.var(0, unbiased=False) + BN_EPS)).float()


def bn_case(P, C, seed, batch=False):
    """-> dict(y, da, mean, invstd, gamma, beta) of fp32 CPU tensors, y ~ 2 randn + 0.5, da ~ randn, satisfying
    the mask margin.  ``batch``: mean / invstd are y's batch statistics (biased variance, eps 1e-5), re-taken
    after the margin moves until both hold."""
    g = torch.Generator().manual_seed(seed)
    gamma, beta, mean, invstd = bn_params(C, g)
    y = torch.randn(P, C, generator=g) * 2 + 0.5
    da = torch.randn(P, C, generator=g)
    for _ in range(8):
        if batch:
            mean, invstd = batch_stats(y)
        if not bool((_bn_out(y, mean, invstd, gamma, beta).abs() < MARGIN).any()):
            break
        y = _push_out_of_margin(y, mean, invstd, gamma, beta)
    return dict(y=y, da=da, mean=mean, invstd=invstd, gamma=gamma, beta=beta)


def check_bn_case(case):
    """The recipe's two conditions: nothing inside the margin, and the ReLU mask kills 20 % .. 80 %."""
    bn = _bn_out(case["y"], case["mean"], case["invstd"], case["gamma"], case["beta"])
    assert not bool((bn.abs() < MARGIN).any()), "an element is inside the mask margin"
    killed = float((bn <= 0).double().mean())
    assert 0.2 <= killed <= 0.8, killed
    C = case["gamma"].numel()
    for c0 in range(0, C, 8):
        assert bool((case["gamma"][c0:c0 + 8] < 0).any()), "a group of 8 channels has no negative gamma"
    return killed


def att_pool_case(n, h, w, c, seed):
    """Inputs of att_pool_bn_bwd: a = relu(.) with ~30 % exact zeros and forced ties inside windows (window
    q % 7 == 0: all zero; 1: (0,1) and (1,0) tie at the maximum; 2: (0,0) and (1,1) tie; 3: all four equal),
    sa in (0, 1) per pixel, ca in (0, 1) and dm per (n, c), dout / dp ~ randn, and a BN case for y."""
    g = torch.Generator().manual_seed(seed)
    P, hw = n * h * w, h * w
    a = torch.relu(torch.randn(P, c, generator=g) + 0.52)
    v = a.reshape(n, h // 2, 2, w // 2, 2, c).clone()
    q = torch.arange(n * (h // 2) * (w // 2)).reshape(n, h // 2, w // 2) % 7
    top = v.amax(dim=(2, 4)) + 1.0
    for kind, cells in ((0, ((0, 0), (0, 1), (1, 0), (1, 1))), (1, ((0, 1), (1, 0))), (2, ((0, 0), (1, 1))),
                        (3, ((0, 0), (0, 1), (1, 0), (1, 1)))):
        m = (q == kind)[..., None].expand(-1, -1, -1, c)
        val = torch.zeros_like(top) if kind == 0 else top
        for (i, j) in cells:
            v[:, :, i, :, j] = torch.where(m, val, v[:, :, i, :, j])
    a = v.reshape(P, c).contiguous()
    case = bn_case(P, c, seed + 1)
    case.update(a=a, sa=torch.sigmoid(torch.randn(P, generator=g)), ca=torch.sigmoid(torch.randn(n, c, generator=g)),
                dm=torch.randn(n, c, generator=g) * 0.1, dout=torch.randn(P, c, generator=g),
                dp=torch.randn(P // 4, c, generator=g))
    del case["da"]
    return case


# the shapes and seeds of the GPU tests (the host test checks the recipe on each of them)
PREPARE_SHAPES = [(777, 32), (2 * 35 + 5, 16), (4800, 64), (1600 * 3, 256), (87, 48)]            # (P, C)
DGRAD_SHAPES = [(2, 40, 40, 64, 64, 1), (3, 20, 20, 128, 64, 1), (1, 7, 5, 64, 32, 1), (3, 13, 9, 96, 64, 1),
                (2, 10, 10, 64, 64, 2)]                                      # (n, h, w, cout_dy, cin_dx, dil)
WGRAD_SHAPES = [(2, 40, 40, 4, 3, 64), (1, 7, 5, 4, 3, 64), (3, 13, 9, 8, 8, 32), (5, 6, 6, 4, 3, 16)]
ATT_POOL_SHAPES = [(1, 2, 2, 4), (3, 6, 10, 64), (2, 40, 40, 64), (2, 20, 20, 128), (11, 40, 40, 256)]
HEAD_SHAPES = [(3, 40, 40), (1, 7, 5), (2, 13, 63), (5, 9, 11)]


def seed_of(*shape):
    s = 17
    for v in shape:
        s = (s * 131 + int(v)) % 1000003
    return s


def case_prepare(P, C, batch):
    return bn_case(P, C, seed_of(1, P, C, int(batch)), batch)


def case_dgrad(shape):
    """-> (the layer's BN case [P, cout_dy], the case of the BN below the dgrad's output [P, cin_dx])"""
    n, h, w, cout_dy, cin_dx, _ = shape
    return bn_case(n * h * w, cout_dy, seed_of(2, *shape)), bn_case(n * h * w, cin_dx, seed_of(3, *shape))


def case_wgrad(shape):
    n, h, w, _, _, cout = shape
    return bn_case(n * h * w, cout, seed_of(4, *shape))


def case_att_pool(shape):
    return att_pool_case(*shape, seed_of(5, *shape))
