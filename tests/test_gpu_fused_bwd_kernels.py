"""The fused BN-backward and eval-head kernels called on their own against the fp64 references of
tests/fused_bwd_ref.py: srpde_bn_bwd_prepare, srpde_conv_dgrad_h3_bnb, srpde_conv_wgrad_bnb, srpde_att_pool_bn_bwd,
srpde_conv_head_eval, and the small eval entries (bn_eval_prepare, bn_affine, nhwc_to_nchw, resize_bicubic).

The whole-model A/B tests load gamma ~ 1, beta ~ 0 and compare HIP with HIP at the model's square shapes.  Here
gamma takes both signs inside every channel octet, |beta| ~ 0.5, (mean, invstd) are given numbers, the shapes are
ragged and rectangular, and the errors are taken per channel and per image row.  Inputs are seeded on the CPU; every
|xhat gamma + beta| stays 1e-3 away from 0 (checked by tests/test_fused_bwd_ref_host.py), so the fp32 and fp64
ReLU masks agree.  Bars: fp32 summation bounds for sums, roundings counted from the kernel's expression for
elementwise outputs, and for the MFMA kernels the error of the already tested unfused path on the same inputs
(err_fused <= 3 err_unfused + 1e-7, the rule of test_conv_split_kernels_are_fp32_accurate).

SRPDE_FUSED_BWD_ERRORS=<file>: the measured (fused, unfused) error pairs are also written there as JSON."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U32
F64 = torch.float64
_RECORDS = {}


def dev(t):
    return t.to(DEV)


def cpu64(t):
    return t.detach().to("cpu", F64)


def _record(kind, shape, **errs):
    path = os.environ.get("SRPDE_FUSED_BWD_ERRORS")
    print(f"{kind} {shape}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    if not path:
        return
    _RECORDS[f"{kind} {tuple(shape)}"] = dict(kind=kind, shape=list(shape), **errs)
    with open(path, "w") as f:
        json.dump(sorted(_RECORDS.values(), key=lambda r: (r["kind"], r["shape"])), f, indent=1)


def wide(t, pad=8, off=4):
    """the same values as a column slice of a wider buffer: row stride ld = C + pad, 16-byte aligned start"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[:, off:off + t.shape[1]]
    v.copy_(t)
    return v


def sliced_errors(x, ref, rows_per_slice=None):
    """-> (whole-tensor relative L2, per-column relative L2[, per-row-group relative L2]) of x [P, C] against ref;
    a slice's denominator is floored at 1e-3 of the tensor's RMS (times the slice's element count ** 0.5)."""
    x, ref = cpu64(x), cpu64(ref)
    if x.dim() == 1:
        x, ref = x[:, None], ref[:, None]
    diff = x - ref
    rms = float(ref.pow(2).mean().sqrt())
    out = [float(diff.norm() / ref.norm())]
    out.append(diff.norm(dim=0) / torch.clamp(ref.norm(dim=0), min=1e-3 * rms * ref.shape[0] ** 0.5))
    if rows_per_slice is not None:
        dg, rg = diff.reshape(-1, rows_per_slice * x.shape[1]), ref.reshape(-1, rows_per_slice * x.shape[1])
        out.append(dg.norm(dim=1) / torch.clamp(rg.norm(dim=1), min=1e-3 * rms * rg.shape[1] ** 0.5))
    return out


def assert_within_unfused(ef, eu, what):
    """err_fused <= 3 err_unfused + 1e-7, for a number or slice by slice"""
    ef, eu = torch.as_tensor(ef, dtype=F64), torch.as_tensor(eu, dtype=F64)
    bad = ef > 3.0 * eu + 1e-7
    if bool(bad.any()):
        k = int(torch.argmax((ef - 3.0 * eu).reshape(-1)))
        raise AssertionError(f"{what}: fused {float(ef.reshape(-1)[k]):.3e} against unfused "
                             f"{float(eu.reshape(-1)[k]):.3e} at slice {k} ({int(bad.sum())} slices over the bar)")


def word_value(word):
    return float(word.view(torch.float32))


def bn_dev(case):
    return tuple(dev(case[k]) for k in ("y", "mean", "invstd", "gamma", "beta"))


# --------------------------------------- (a) bn_bwd_prepare ---------------------------------------
def _check_prepare(case, relu, eval_mode, use_wide):
    from superresolution_for_pdes_amd import hipops as H
    P, C = case["y"].shape
    y, mean, invstd, gamma, beta = bn_dev(case)
    da = dev(case["da"])
    if use_wide:
        y, da = wide(y), wide(da, pad=12, off=8)
        assert y.stride(0) > C and da.stride(0) > C
    dg, db, dbias = (torch.full((C,), float("nan"), device=DEV) for _ in range(3))
    m1, m2, word = H.bn_bwd_prepare(y, da, mean, invstd, gamma, beta, dg, db, dbias, relu=relu, eval_mode=eval_mode)
    torch.cuda.synchronize()
    ref = [case[k] for k in ("y", "da", "mean", "invstd", "gamma", "beta")]
    dy_ref, r1, r2, dgamma, dbeta = R.bn_relu_bwd_ref(*ref, relu=relu, eval_mode=eval_mode)
    t1, t2 = R.bn_bwd_terms(*ref, relu=relu)
    b1, b2 = (P + 8) * U * t1, (P + 8) * U * t2          # fp32 recursive summation of P terms, each rounded
    assert bool(((cpu64(db) - dbeta).abs() <= b1).all()), float(((cpu64(db) - dbeta).abs() - b1).max())
    assert bool(((cpu64(dg) - dgamma).abs() <= b2).all()), float(((cpu64(dg) - dgamma).abs() - b2).max())
    if eval_mode:
        assert not bool(m1.any()) and not bool(m2.any())
    else:
        assert bool(((cpu64(m1) - r1).abs() <= b1 / P).all()), float(((cpu64(m1) - r1).abs() - b1 / P).max())
        assert bool(((cpu64(m2) - r2).abs() <= b2 / P).all()), float(((cpu64(m2) - r2).abs() - b2 / P).max())
    # the conv bias gradient sum(dy) = k (sum dz - P m1 - m2 sum xhat): k times a sum of the same terms, and in
    # train mode sum xhat = P (mean64 - mean32) invstd, P 2^-24 |mean invstd m2| at most
    k = cpu64(gamma) * cpu64(invstd)
    slack = k.abs() * (b1 + P * U * (cpu64(mean) * cpu64(invstd) * r2).abs())
    assert bool(((cpu64(dbias) - dy_ref.sum(0)).abs() <= slack).all())
    # the bound word: rigorous from below, its own formula (evaluated in fp64) from above
    bound = word_value(word)
    assert bound >= float(dy_ref.abs().max()), (bound, float(dy_ref.abs().max()))
    xmax = 0.0 if eval_mode else (P - 1) ** 0.5
    formula = float((k.abs() * (float(cpu64(case["da"]).abs().max()) + r1.abs() + xmax * r2.abs())).max())
    assert bound <= 1.001 * formula, (bound, formula)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("eval_mode", [False, True])
@pytest.mark.parametrize("P,C", R.PREPARE_SHAPES)
def test_bn_bwd_prepare_matches_fp64(P, C, eval_mode, relu):
    """m1, m2, dgamma, dbeta within the fp32 summation bound of the fp64 sums (train mode: the batch's own mean and
    invstd; eval mode: given ones, m1 == m2 == 0), and the dy bound word between max|dy| and 1.001 x its formula."""
    _check_prepare(R.case_prepare(P, C, batch=not eval_mode), relu, eval_mode, False)


@pytest.mark.parametrize("relu", [True, False])
def test_bn_bwd_prepare_bound_word_covers_a_gradient_correlated_with_xhat(relu):
    """With random da, m2 ~ P^-1/2 and the xhat m2 term of the bound is never needed.  Here da = clamp(xhat, -1, 1)
    (m2 ~ 0.7 without the ReLU) except -+1 on each channel's largest and smallest xhat (~ +-3): there
    |dy| ~ k (1 + |xhat| m2) exceeds k (max|da| + |m1| + |m2|), so the word holds only with the max|xhat| factor
    of its formula."""
    case = R.case_prepare(777, 32, batch=True)
    xhat = (case["y"].double() - case["mean"].double()) * case["invstd"].double()
    da = xhat.clamp(-1.0, 1.0)
    da[xhat.argmax(0), torch.arange(32)] = -1.0
    da[xhat.argmin(0), torch.arange(32)] = 1.0
    case = dict(case, da=da.float())
    dy, r1, r2 = R.bn_relu_bwd_ref(*(case[k] for k in ("y", "da", "mean", "invstd", "gamma", "beta")), relu=relu)[:3]
    k = (case["gamma"].double() * case["invstd"].double()).abs()
    # the case does what it says: a bound without the max|xhat| factor would not hold
    assert float(dy.abs().max()) > 1.1 * float((k * (1.0 + r1.abs() + r2.abs())).max())
    _check_prepare(case, relu, False, False)


@pytest.mark.parametrize("eval_mode", [False, True])
def test_bn_bwd_prepare_reads_column_slices(eval_mode):
    """the same with y and da as column slices of wider buffers (ld > C, two different strides)"""
    _check_prepare(R.case_prepare(777, 32, batch=not eval_mode), True, eval_mode, True)


# --------------------------------------- (b) conv_dgrad_bnb ---------------------------------------
@pytest.mark.parametrize("shape,relu", [(s, True) for s in R.DGRAD_SHAPES] + [((3, 13, 9, 96, 64, 1), False)])
def test_conv_dgrad_bnb_matches_fp64(shape, relu, conv_math):
    """dx of the fused BN-backward dgrad against conv^T(dy) in fp64 (dy from the kernel's own fp32 m1 / m2), held to
    the unfused path's error whole, per output channel and per image row; dy's split planes, the partial sums for
    the BatchNorm below and the max|dx| slots of the same launch."""
    from superresolution_for_pdes_amd import hipops as H
    H.set_conv_math("h3")
    n, h, w, cout_dy, cin_dx, dil = shape
    assert H.bnb_capable(cout_dy, cin_dx, w, dil), shape
    P = n * h * w
    top, below = R.case_dgrad(shape)
    g = torch.Generator().manual_seed(R.seed_of(6, *shape))
    wt = torch.randn(cout_dy, cin_dx, 3, 3, generator=g) * (2.0 / (9 * cin_dx)) ** 0.5
    wd = H.pack_conv_weights(dev(wt), cin_dx, want_fwd=False, want_dgrad=True)[1]
    assert getattr(wd, "h3", None) is not None
    y, mean, invstd, gamma, beta = bn_dev(top)
    da = dev(top["da"])
    yb, meanb, invstdb, gammab, betab = bn_dev(below)
    scratch = [torch.empty(cout_dy, device=DEV) for _ in range(6)]
    m1, m2, word = H.bn_bwd_prepare(y, da, mean, invstd, gamma, beta, *scratch[:3], relu=relu)
    dx = torch.full((P, cin_dx), float("nan"), device=DEV)
    dysplit = H.split_planes_buffer(P, cout_dy, DEV).fill_(float("nan"))
    part = H.bn_bwd_partials(n, h, w, cin_dx, DEV)
    part.fill_(float("nan"))
    dx_max = H.dx_max_slots(n, h, w, cin_dx, DEV).fill_(-1.0)
    H.conv_dgrad_bnb(da, y, mean, invstd, gamma, beta, m1, m2, word, wd, dx, n, h, w, cout_dy, cin_dx, dil, dysplit,
                     relu=relu, bn_bwd=(yb, meanb, invstdb, gammab, betab, part), dx_max=dx_max)
    # the unfused path on the same inputs: the fp32 apply, then the h3 dgrad
    dy_u = torch.empty(P, cout_dy, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    H.bn_relu_bwd(y, da, mean, invstd, gamma, beta, dy_u, *scratch[3:], relu=relu, amax=slot)
    dx_u = torch.full((P, cin_dx), float("nan"), device=DEV)
    H.conv_fwd(dy_u, None, wd, None, dx_u, n, h, w, cin_dx, 3, dil, -1)
    torch.cuda.synchronize()

    ref_in = [top[k] for k in ("y", "da", "mean", "invstd", "gamma", "beta")]
    dy_ref = R.bn_relu_bwd_ref(*ref_in, relu=relu, m1=m1, m2=m2)[0]
    dx64 = R.conv_dgrad_ref(dy_ref, wt, n, h, w, dil)
    ef, efc, efr = sliced_errors(dx, dx64, w)
    eu, euc, eur = sliced_errors(dx_u, dx64, w)
    _record("conv_dgrad_bnb" + ("" if relu else " no-relu"), shape, err_fused=ef, err_unfused=eu,
            worst_channel_fused=float(efc.max()), worst_channel_unfused=float(euc.max()),
            worst_row_fused=float(efr.max()), worst_row_unfused=float(eur.max()))
    assert ef < 1e-6, ef
    assert_within_unfused(ef, eu, "dx")
    assert_within_unfused(efc, euc, "dx per output channel")
    assert_within_unfused(efr, eur, "dx per image row")

    # dy's split: (hi + lo) / s, s = 2^(15 - e) from the bound word, holds dy to the split's representation error
    # plus the fp32 rounding of the apply
    bound = word_value(word)
    assert bound >= float(dy_ref.abs().max()), (bound, float(dy_ref.abs().max()))
    e = int(np.floor(np.log2(bound))) + 1
    s = 2.0 ** (15 - e)
    deq = (cpu64(dysplit[0]) + cpu64(dysplit[1])) / s
    bar = 2.0 ** -22 * (2.0 ** 15 / s) + 4 * U * R.bn_bwd_apply_terms(*ref_in, m1, m2, relu=relu)
    over = (deq - dy_ref).abs() - bar
    assert bool((over <= 0).all()), float(over.max())      # (a NaN left in the planes fails here too)

    # the reduction for the BatchNorm below, over the kernel's own fp32 dx
    _, _, _, sdzx, sdz = R.bn_relu_bwd_ref(below["y"], dx, *(below[k] for k in ("mean", "invstd", "gamma", "beta")))
    t1, t2 = R.bn_bwd_terms(below["y"], dx, *(below[k] for k in ("mean", "invstd", "gamma", "beta")))
    got = cpu64(part).sum(0)
    assert bool(((got[:, 0] - sdz).abs() <= (P + 8) * U * t1).all()), float((got[:, 0] - sdz).abs().max())
    assert bool(((got[:, 1] - sdzx).abs() <= (P + 8) * U * t2).all()), float((got[:, 1] - sdzx).abs().max())
    assert float(dx_max.min()) >= 0.0
    assert float(dx_max.max()) == float(dx.abs().max())


# --------------------------------------- (c) conv_wgrad_bnb ---------------------------------------
@pytest.mark.parametrize("shape", R.WGRAD_SHAPES)
def test_conv_wgrad_bnb_matches_fp64(shape, conv_math):
    """The fp32 weight gradient with the BN backward on its dY loads against fp64, held to the error of
    bn_relu_bwd + conv_wgrad (fp32 kernels) on the same inputs, whole and per output channel."""
    from superresolution_for_pdes_amd import hipops as H
    H.set_conv_math("f32")
    n, h, w, cin_pad, cin_real, cout = shape
    P = n * h * w
    case = R.case_wgrad(shape)
    g = torch.Generator().manual_seed(R.seed_of(7, *shape))
    x = torch.randn(P, cin_pad, generator=g)       # the padding channels hold numbers too: dw must not see them
    y, mean, invstd, gamma, beta = bn_dev(case)
    da, xd = dev(case["da"]), dev(x)
    scratch = [torch.empty(cout, device=DEV) for _ in range(6)]
    m1, m2, _ = H.bn_bwd_prepare(y, da, mean, invstd, gamma, beta, *scratch[:3])
    dw_f = torch.full((cout, cin_real, 3, 3), float("nan"), device=DEV)
    H.conv_wgrad_bnb(da, y, mean, invstd, gamma, beta, m1, m2, xd, dw_f, n, h, w, 3, 1)
    dy_u = torch.empty(P, cout, device=DEV)
    H.bn_relu_bwd(y, da, mean, invstd, gamma, beta, dy_u, *scratch[3:])
    dw_u = torch.full((cout, cin_real, 3, 3), float("nan"), device=DEV)
    H.conv_wgrad(dy_u, xd, None, dw_u, n, h, w, 3, 1)
    torch.cuda.synchronize()
    ref_in = [case[k] for k in ("y", "da", "mean", "invstd", "gamma", "beta")]
    dy_ref = R.bn_relu_bwd_ref(*ref_in, m1=m1, m2=m2)[0]
    dw64 = R.conv_wgrad_ref(dy_ref, x[:, :cin_real], n, h, w, 1)
    # [cout, cin * 9] -> columns = output channels
    ef, efc = sliced_errors(dw_f.reshape(cout, -1).t(), dw64.reshape(cout, -1).t())
    eu, euc = sliced_errors(dw_u.reshape(cout, -1).t(), dw64.reshape(cout, -1).t())
    _record("conv_wgrad_bnb", shape, err_fused=ef, err_unfused=eu, worst_channel_fused=float(efc.max()),
            worst_channel_unfused=float(euc.max()))
    assert_within_unfused(ef, eu, "dw")
    assert_within_unfused(efc, euc, "dw per output channel")


# --------------------------------------- (d) att_pool_bn_bwd ---------------------------------------
@pytest.mark.parametrize("shape,use_wide", [(s, s == (3, 6, 10, 64)) for s in R.ATT_POOL_SHAPES])
def test_att_pool_bn_bwd_matches_fp64(shape, use_wide):
    """de elementwise within the roundings of (dout sa) ca + dm + dp, the BN partials against fp64 sums over the
    kernel's own de, the max|de| slots, the block count.  (11, 40, 40, 256): more windows than 1024 blocks x 4."""
    from superresolution_for_pdes_amd import hipops as H
    n, h, w, c = shape
    P = n * h * w
    case = R.case_att_pool(shape)
    y, mean, invstd, gamma, beta = bn_dev(case)
    dout, a, dp = dev(case["dout"]), dev(case["a"]), dev(case["dp"])
    ca, sa, dm = dev(case["ca"]), dev(case["sa"]), dev(case["dm"])
    de = torch.full((P, c), float("nan"), device=DEV)
    if use_wide:
        dout, y, de = wide(dout), wide(y, pad=12, off=8), wide(de, pad=4, off=4)
        assert min(dout.stride(0), y.stride(0), de.stride(0)) > c
    nb = int(H.query("srpde_att_pool_bn_bwd_blocks", n, h, w, c))
    if shape == (11, 40, 40, 256):
        assert n * (h // 2) * (w // 2) > nb * (256 // (c // 4))      # the grid-stride loop runs
    part, da_max = H.att_pool_bn_bwd(dout, ca, sa, dm, a, dp, de, y, mean, invstd, gamma, beta, n, h, w)
    torch.cuda.synchronize()
    assert part.shape == (nb, c, 2) and da_max.shape == (nb,)
    ref, mag = R.att_pool_bwd_ref(case["dout"], case["ca"], case["sa"], case["dm"], case["a"], case["dp"], n, h, w,
                                  parts=True)
    over = (cpu64(de) - ref).abs() - 4 * U * mag
    assert bool((over <= 0).all()), float(over.max())
    bn = [case[k] for k in ("mean", "invstd", "gamma", "beta")]
    _, _, _, sdzx, sdz = R.bn_relu_bwd_ref(case["y"], de, *bn)
    t1, t2 = R.bn_bwd_terms(case["y"], de, *bn)
    got = cpu64(part).sum(0)
    assert bool(((got[:, 0] - sdz).abs() <= (P + 8) * U * t1).all()), float((got[:, 0] - sdz).abs().max())
    assert bool(((got[:, 1] - sdzx).abs() <= (P + 8) * U * t2).all()), float((got[:, 1] - sdzx).abs().max())
    assert float(da_max.max()) == float(de.abs().max())


@pytest.mark.parametrize("n,h,w,c", [(1, 3, 4, 64), (1, 4, 4, 12)])
def test_att_pool_bn_bwd_rejects_odd_height_and_non_power_of_two_quads(n, h, w, c):
    from superresolution_for_pdes_amd import hipops as H
    P = n * h * w
    g = torch.Generator().manual_seed(h + c)
    t = lambda *s: dev(torch.randn(*s, generator=g))   # noqa: E731
    de = torch.full((P, c), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="srpde_att_pool_bn_bwd"):
        H.att_pool_bn_bwd(t(P, c), t(n, c), t(P), t(n, c), t(P, c), t(max(P // 4, 1), c), de, t(P, c), t(c), t(c), t(c),
                          t(c), n, h, w)
    torch.cuda.synchronize()
    assert bool((de == 7.0).all())     # nothing was launched


# --------------------------------------- (e) conv_head_eval ---------------------------------------
@pytest.mark.parametrize("shape,ldz", [(s, 32) for s in R.HEAD_SHAPES] + [((5, 9, 11), 64)])
def test_conv_head_eval_matches_fp64(shape, ldz, conv_math):
    """out_conv2 -> BN (eval) -> ReLU -> final -> + residual in one kernel against fp64, held to the error of the
    separate passes (h3 conv with bias, bn_relu_fwd on bn_eval_prepare's outputs, head_fwd), whole and per image row."""
    from superresolution_for_pdes_amd import hipops as H
    H.set_conv_math("h3")
    n, h, w = shape
    P = n * h * w
    assert H.query("srpde_conv_head_eval_supported", w) and H.h3_capable(32, 0, 16, w, 1)
    g = torch.Generator().manual_seed(R.seed_of(8, *shape, ldz))
    z = torch.relu(torch.randn(P, 32, generator=g))
    wt = torch.randn(16, 32, 3, 3, generator=g) * (2.0 / 288) ** 0.5
    bias = torch.randn(16, generator=g) * 0.1
    gamma, beta, rmean, invstd0 = R.bn_params(16, g)
    rvar = (1.0 / invstd0.double() ** 2 - R.BN_EPS).float()
    wf = torch.randn(1, 16, 1, 1, generator=g) * 0.25
    bf = torch.randn(1, generator=g)
    xin = torch.randn(n, 3, h, w, generator=g)
    zd = dev(z)
    if ldz != 32:
        zd = wide(zd, pad=ldz - 32, off=16)
        assert zd.stride(0) == ldz
    wpack = H.pack_conv_weights(dev(wt), 32)[0]
    assert getattr(wpack, "h3", None) is not None
    mean, invstd = H.bn_eval_prepare(dev(rmean), dev(rvar), R.BN_EPS)
    gd, bd, biasd, wfd, bfd, xd = (dev(t) for t in (gamma, beta, bias, wf, bf, xin))
    out_f = H.conv_head_eval(zd, wpack, biasd, mean, invstd, gd, bd, wfd, bfd, xd, n, h, w)
    o2, act = H.empty(P, 16, device=DEV), H.empty(P, 16, device=DEV)
    H.conv_fwd(zd, None, wpack, biasd, o2, n, h, w, 16)
    H.bn_relu_fwd(o2, mean, invstd, gd, bd, act)
    out_s = H.head_fwd(act, wfd, bfd, xd, n, h * w)
    torch.cuda.synchronize()
    assert out_f.shape == (P,)
    ref = R.head_eval_ref(z, wt, bias, mean, invstd, gamma, beta, wf, bf, xin)
    ef, _, efr = sliced_errors(out_f, ref, w)
    eu, _, eur = sliced_errors(out_s, ref, w)
    _record("conv_head_eval" + ("" if ldz == 32 else f" ldz={ldz}"), shape, err_fused=ef, err_unfused=eu,
            worst_row_fused=float(efr.max()), worst_row_unfused=float(eur.max()))
    assert_within_unfused(ef, eu, "head output")
    assert_within_unfused(efr, eur, "head output per image row")


def test_conv_head_eval_reports_wide_rows_unsupported():
    from superresolution_for_pdes_amd import hipops as H
    assert H.query("srpde_conv_head_eval_supported", 63) == 1
    assert H.query("srpde_conv_head_eval_supported", 64) == 0


# --------------------------------------- (f) small eval entries ---------------------------------------
def ulps(x, ref64):
    """|x - ref| in units of the fp32 spacing at ref"""
    x = x.detach().cpu().numpy().astype(np.float64)
    r = ref64.numpy()
    return np.abs(x - r) / np.spacing(np.abs(r.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("C", [4, 16, 300])
def test_bn_eval_prepare_and_affine(C):
    from superresolution_for_pdes_amd import hipops as H
    g = torch.Generator().manual_seed(C)
    rm = torch.randn(C, generator=g)
    rv = torch.logspace(-8, 4, C)[torch.randperm(C, generator=g)]
    mean, invstd = H.bn_eval_prepare(dev(rm), dev(rv), R.BN_EPS)
    torch.cuda.synchronize()
    assert torch.equal(mean.cpu(), rm)
    want = 1.0 / torch.sqrt(rv.double() + float(np.float32(R.BN_EPS)))
    assert float(ulps(invstd, want).max()) <= 2.0, float(ulps(invstd, want).max())
    gamma, beta, _, _ = R.bn_params(C, g)
    scale, shift = H.bn_affine(mean, invstd, dev(gamma), dev(beta), 1600)
    torch.cuda.synchronize()
    sc64 = gamma.double() * cpu64(invstd)
    assert float(ulps(scale, sc64).max()) <= 2.0
    sh64 = beta.double() - rm.double() * sc64
    bar = 4 * U * (beta.double().abs() + (rm.double() * sc64).abs())
    assert bool(((cpu64(shift) - sh64).abs() <= bar).all()), float(((cpu64(shift) - sh64).abs() - bar).max())


@pytest.mark.parametrize("n,c,h,w,ld", [(2, 3, 7, 5, 4), (1, 16, 4, 4, 16)])
def test_nhwc_to_nchw_equals_permute(n, c, h, w, ld):
    from superresolution_for_pdes_amd import hipops as H
    g = torch.Generator().manual_seed(n + c)
    buf = torch.randn(n * h * w, ld, generator=g)
    out = H.nhwc_to_nchw(dev(buf)[:, :c], n, c, h, w)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), buf[:, :c].reshape(n, h, w, c).permute(0, 3, 1, 2))


def _cubic_abs_weights(n_in, n_out):
    """[n_out, n_in] sums of |Keys coefficient| (A = -0.75, align_corners, taps clamped to the border) per source index;
    the source coordinate is the fp32 product the kernel and aten both form."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    A = -0.75
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        r = np.float32(scale * np.float32(o))
        i = int(np.floor(r))
        t = float(r) - i
        x1, x2 = t + 1.0, 1.0 - t
        x3 = x2 + 1.0
        cs = (((A * x1 - 5 * A) * x1 + 8 * A) * x1 - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
              ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A)
        for k, cf in enumerate(cs):
            m[o, min(max(i - 1 + k, 0), n_in - 1)] += abs(cf)
    return torch.from_numpy(m)


@pytest.mark.parametrize("h,w,ho,wo", [(40, 40, 80, 80), (7, 5, 13, 17), (10, 10, 10, 10), (4, 6, 1, 1)])
def test_resize_bicubic_matches_interpolate(h, w, ho, wo):
    """against F.interpolate(mode='bicubic', align_corners=True) in fp32 on the CPU (the kernel claims aten's
    operation order): elementwise within 4 x 2^-24 x sum |tap cx cy|; the identity resize to 1 ulp.

    This test found the kernel leaving the rounding points of Keys' coefficient polynomials to the compiler's
    contraction: 40x40 -> 80x80 then sat at 24.0 x the bar (median element 0.33 x; plane 2, last row, column 77:
    -3.09284e-3 against aten's -3.09270e-3), because the outer polynomial passes through values near 4 on its way
    to |c| < 0.07.  With aten's rounding points stated in the kernel (csrc/resize.hip) the same case measures 0.91
    of the bar and 7x5 -> 13x17 0.48; the identity and the 1x1 resize are exact."""
    from superresolution_for_pdes_amd import hipops as H
    g = torch.Generator().manual_seed(h * 100 + wo)
    x = torch.randn(3, h, w, generator=g)
    out = H.resize_bicubic(dev(x), ho, wo)
    torch.cuda.synchronize()
    want = F.interpolate(x[None], size=(ho, wo), mode="bicubic", align_corners=True)[0]
    mag = _cubic_abs_weights(h, ho) @ x.double().abs() @ _cubic_abs_weights(w, wo).t()
    diff = (out.cpu().double() - want.double()).abs()
    print(f"resize_bicubic {h}x{w} -> {ho}x{wo}: max |diff| / bar {float((diff / (4 * U * mag)).max()):.3f}")
    assert out.shape == (3, ho, wo)
    assert bool((diff <= 4 * U * mag).all()), float((diff / (4 * U * mag)).max())
    if (h, w) == (ho, wo):
        assert float(ulps(out, x.double()).max()) <= 1.0
