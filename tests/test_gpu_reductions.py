"""The reductions, the head, the MSE and the optimizer at sizes where their production loops run.

Part 1 is exact: every operand is a small nonzero integer stored as fp32 (values in +-{1, 2, 3}, weights +-1), so
every product and every partial sum is an integer below 2^24, every summation order gives the same fp32 / fp64
result, and the kernel's output must EQUAL the int64 reference -- one dropped, doubled or misplaced row changes it by
a nonzero integer.  The reference side asserts sum |terms| < 2^24 per output element, so that guarantee is checked.
The shapes enter weighted_colsum_kernel's four-rows-in-flight loop and its tail, partsum_kernel's strided loop,
outer_sum_kernel's eight-sample loop and its tail, and a second (uneven) trip of every grid-stride loop.

Part 2 compares with fp64: the AdamW update against the same formula in numpy fp64 with elementwise bars that follow
from the count of fp32 roundings, and the attention gate (every backward path: the per-sample kernel at C/4 = 16, 32,
64 and the pixel + channel kernels at the other channel counts) against fp64 autograd with test_attention's bars.

Part 3: the channel counts colsum_blocks would divide by zero on are rejected before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7.0                      # fills columns c..ld-1 of a wide buffer
VALS = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)
SIGNS = (-1.0, 1.0)
U = 2.0 ** -24                  # fp32 unit roundoff
N_FLAT = 2 * 2 ** 20 + 2 ** 19 + 3   # 2.5 trips of the 1024 x 256 (float4) and 4096 x 256 grids, n & 3 == 3


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, vals, g):
    """A device fp32 tensor of the given shape drawn from `vals` (small nonzero integers)."""
    t = torch.tensor(vals, dtype=torch.float32, device=DEV)
    return t[torch.randint(0, len(vals), tuple(shape), device=DEV, generator=g)]


def _wsum(v, w):
    """int64 sum over rows of v[p, ...] * w[p, ...] (broadcast), asserting sum |terms| < 2^24 per output element."""
    vi, wi = v.long(), w.long()
    assert int((vi.abs() * wi.abs()).sum(0).max()) < 2 ** 24
    return (vi * wi).sum(0)


def _same(got, want):
    """fp32 kernel output == int64 reference, exactly (fp64 holds both)."""
    return got.shape == want.shape and torch.equal(got.double(), want.double())


def _view(t, wide, fill=None):
    """t (or `fill` in its shape) as a device [P, C] view: contiguous, or the first C columns of a [P, 2C] buffer."""
    if not wide:
        return t.clone() if fill is None else torch.full_like(t, fill)
    b = torch.full((t.shape[0], 2 * t.shape[1]), PAD, device=DEV)
    b[:, :t.shape[1]] = t if fill is None else fill
    return b[:, :t.shape[1]]


def _pad_untouched(v):
    b = v._base
    return b is None or bool((b[:, v.shape[1]:] == PAD).all())


def rows(x):  # NCHW -> [P, C] NHWC rows
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def unrows(r, n, h, w):
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2)


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / max(b.norm(), 1e-30))


# ------------------------------------------ 1. exact integers ------------------------------------------
# P = 2,098,911, C = 16: rows_per_blk = 2112 = 33 rows per thread (eight unrolled trips and one tail trip), 994
# blocks (partsum_kernel's strided loop, the last block partial), P > 8192 * 256 (head_fwd's second trip);
# P = 37: fewer rows than the 64 row slots of a block
HEAD_SHAPES = [(1311, 1601), (1, 37)]


@pytest.fixture(scope="module", params=HEAD_SHAPES, ids=lambda s: f"n{s[0]}hw{s[1]}")
def head_case(request):
    n, hw = request.param
    P, C = n * hw, 16
    g = _gen(P)
    z, dout = _ints((P, C), VALS, g), _ints((P,), SIGNS, g)
    wf, bf = _ints((C,), VALS, g), _ints((1,), VALS, g)
    xin = torch.full((n, 3, hw), 1000.0, device=DEV)     # a wrong plane index reads the sentinel
    xin[:, 0] = _ints((n, hw), VALS, g)
    ref = {
        "out": (z.long() * wf.long()).sum(1) + bf.long() + xin[:, 0].reshape(-1).long(),
        "dz": dout.long()[:, None] * wf.long()[None, :],
        "dwf": _wsum(z, dout[:, None]),
        "dbf": _wsum(dout[:, None], torch.ones(1, 1, device=DEV)),
    }
    return n, hw, z, dout, wf, bf, xin, ref


@pytest.mark.parametrize("wide", [False, True], ids=["ld16", "ld32"])
def test_head_bwd_exact(head_case, wide):
    from superresolution_for_pdes_amd import hipops as H
    n, hw, z, dout, wf, _, _, ref = head_case
    zv, dz = _view(z, wide), _view(z, wide, 0.5)
    dwf, dbf = torch.full((16,), 0.5, device=DEV), torch.full((1,), 0.5, device=DEV)
    H.head_bwd(dout, zv, wf, n, hw, dz, dwf, dbf)
    torch.cuda.synchronize()
    assert _same(dz, ref["dz"])
    assert _same(dwf, ref["dwf"]), (dwf.long() - ref["dwf"]).tolist()
    assert _same(dbf, ref["dbf"]), (dbf.long() - ref["dbf"]).tolist()
    assert _pad_untouched(dz) and _pad_untouched(zv)


@pytest.mark.parametrize("wide", [False, True], ids=["ld16", "ld32"])
def test_head_fwd_exact(head_case, wide):
    from superresolution_for_pdes_amd import hipops as H
    n, hw, z, _, wf, bf, xin, ref = head_case
    zv = _view(z, wide)
    out = H.head_fwd(zv, wf, bf, xin, n, hw)
    torch.cuda.synchronize()
    assert _same(out, ref["out"])
    assert _pad_untouched(zv)


@pytest.fixture(scope="module")
def mse_case():
    n = 1311 * 1601      # 1024 x 256 threads: 8 trips and a 9th for the first 1759 of them
    g = _gen(n)
    y, t = _ints((n,), VALS, g), _ints((n,), SIGNS, g)
    S = int(((y.long() - t.long()) ** 2).sum())
    assert S < 2 ** 24   # the squares are fp32, their sum fp64: exact either way
    return n, y, t, S


def test_mse_fwd_exact(mse_case):
    from superresolution_for_pdes_amd import hipops as H
    n, y, t, S = mse_case
    loss = H.mse_fwd(y, t)
    torch.cuda.synchronize()
    assert np.float32(float(loss)) == np.float32(S / n), (float(loss), S / n)


@pytest.mark.parametrize("gout", [None, 2.0])
def test_mse_bwd_exact(mse_case, gout):
    """dy = ((2 / n) * (y - t)) * gout, the fp32 products in the kernel's order."""
    from superresolution_for_pdes_amd import hipops as H
    n, y, t, _ = mse_case
    norm = torch.tensor(np.float32(2) / np.float32(n), device=DEV)
    assert norm.dtype == torch.float32
    gt = None if gout is None else torch.tensor([gout], device=DEV)
    dy = H.mse_bwd(y, t, gt)
    want = (norm * (y - t)) * (1.0 if gout is None else gt)
    torch.cuda.synchronize()
    assert dy.dtype == want.dtype == torch.float32 and torch.equal(dy, want)


def _att_ws(n, hw, c, gc):
    """srpde_att_bwd's workspace as fp32 words, NaN-filled, and its documented regions
    [dsa P | dm n*c | dw1 rows n*cr*c | dw2 rows n*cr*c | db1 rows n*cr | db2 rows n*c | partials]."""
    from superresolution_for_pdes_amd import _lib
    ws_bytes = int(_lib.query("srpde_att_bwd_workspace_size", n, hw, c, gc))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
    cr, P = c // 8, n * hw
    o1 = P + n * c + 2 * n * cr * c
    o2 = o1 + n * cr
    return ws, ws_bytes, ws[:P], ws[o1:o2].view(n, cr), ws[o2:o2 + n * c].view(n, c)


@pytest.mark.parametrize("c,gc,hw,n", [
    (256, 512, 100, 130),   # colsum: 7 rows per thread, 929 blocks; outer sums: an unrolled trip + a tail (groups 0, 1)
    (64, 128, 1600, 23),    # colsum: 5 rows per thread
    (32, 36, 49, 3),        # gc / 4 = 9 is no power of two: 252 active lanes
])
def test_att_bwd_params_exact(c, gc, hw, n):
    """srpde_att_bwd_params alone, on a workspace prefilled with integer dsa and per-sample bias rows."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd import _lib
    g = _gen(c + gc + n)
    cr, P = c // 8, n * hw
    ws, ws_bytes, dsa, db1r, db2r = _att_ws(n, hw, c, gc)
    dsa.copy_(_ints((P,), SIGNS, g))
    db1r.copy_(_ints((n, cr), VALS, g))
    db2r.copy_(_ints((n, c), VALS, g))
    gt, m, hb = _ints((P, gc), VALS, g), _ints((n, c), VALS, g), _ints((n, cr), VALS, g)
    out = {k: torch.full(s, 0.5, device=DEV) for k, s in
           dict(dw1=(cr, c), db1=(cr,), dw2=(c, cr), db2=(c,), dwg=(gc,), dbg=(1,)).items()}
    want = {
        "dw1": _wsum(db1r[:, :, None], m[:, None, :]), "dw2": _wsum(db2r[:, :, None], hb[:, None, :]),
        "db1": _wsum(db1r, torch.ones(1, 1, device=DEV)), "db2": _wsum(db2r, torch.ones(1, 1, device=DEV)),
        "dwg": _wsum(gt, dsa[:, None]), "dbg": _wsum(dsa[:, None], torch.ones(1, 1, device=DEV)),
    }
    H.call("srpde_att_bwd_params", gt.data_ptr(), gc, n, hw, c, gc, m.data_ptr(), hb.data_ptr(),
           *(out[k].data_ptr() for k in ("dw1", "db1", "dw2", "db2", "dwg", "dbg")), ws.data_ptr(), ws_bytes,
           _lib.stream_ptr())
    torch.cuda.synchronize()
    for k in want:
        assert _same(out[k], want[k]), (k, int((out[k].double() - want[k].double()).abs().max()))


def _ulps(got, want):
    return abs(float(got) - float(want)) / float(np.spacing(np.float32(want)))


@pytest.fixture(scope="module")
def flat_ints():
    g = _ints((N_FLAT,), VALS, _gen(3))
    g[-3:] = 3.0        # the n & 3 tail: 27 of the sum
    s2 = int((g.long() ** 2).sum())
    assert s2 < 2 ** 24
    return g, s2


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("max_norm", [1.0, 1e6, 0.0], ids=["clipped", "unclipped", "off"])
def test_clip_coef_exact(flat_ints, grad_scale, max_norm):
    """The squared norm is exact in the kernel's fp64 (integers times a power of two), so coef[1] is float32(sqrt(S))
    to 1 ulp and coef[0] the kernel's fp32 expression min(1, max_norm / (total + 1e-6)) to 2 ulp."""
    from superresolution_for_pdes_amd import hipops as H
    g, s2 = flat_ints
    coef = torch.full((2,), 0.5, device=DEV)
    H.clip_coef(g, grad_scale, max_norm, coef)
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    total = np.float32(np.sqrt(np.float64(grad_scale * grad_scale * s2)))
    assert _ulps(got[1], total) <= 1, (got[1], total)
    if max_norm > float(total) or max_norm <= 0:
        assert got[0] == np.float32(1)
    else:
        c = np.float32(max_norm) / (total + np.float32(1e-6))
        assert c.dtype == np.float32 and c < 1
        assert _ulps(got[0], c) <= 2, (got[0], c)


# ------------------------------------------ 2. fp64 references ------------------------------------------
@pytest.fixture(scope="module")
def adamw_inputs():
    gen = _gen(7)
    g = torch.randn(N_FLAT, device=DEV, generator=gen) * 3
    p = torch.randn(N_FLAT, device=DEV, generator=gen)
    p[::2] = 0.0        # p_new is the bare update there
    r1 = torch.rand(N_FLAT, device=DEV, generator=gen)
    r2 = torch.rand(N_FLAT, device=DEV, generator=gen)
    return g, p, r1, r2


@pytest.mark.parametrize("step,use_coef,grad_scale,wd", [
    (1, False, 1.0, 1e-4), (1, True, 0.25, 0.0), (2, True, 0.25, 1e-4), (2, False, 0.25, 0.0),
    (10000, True, 1.0, 1e-4), (10000, False, 0.25, 0.0)])
def test_adamw_step_against_fp64(adamw_inputs, step, use_coef, grad_scale, wd):
    """One srpde_adamw_step against the same formula in numpy fp64 from the same fp32 inputs (the hyper-parameters as
    the fp32 values the kernel receives).  Each quantity is a chain of at most 8 fp32 operations, each within 2^-24
    relative, so with u = 2^-24:  |m - m64| <= 4u (|m64| + |g gs|),  |v - v64| <= 4u (v64 + (g gs)^2),
    |p - p64| <= 3u |p_old| + 10u |update64|.
    The bar on p is relative to the update, so it holds where the update's numerator m has no cancellation: the
    moments are zero at step 1 and otherwise a state that one-signed gradients leave (m = r1 g gs with r1 in [0, 1),
    v = (0.5 + r2) (g gs)^2), as after a run of like gradients."""
    from superresolution_for_pdes_amd import hipops as H
    g, p0, r1, r2 = adamw_inputs
    lr, b1, b2, eps = 2e-4, 0.9, 0.999, 1e-8
    coef = torch.tensor([0.37, 123.0], device=DEV) if use_coef else None
    gs32 = np.float32(grad_scale) * np.float32(0.37) if use_coef else np.float32(grad_scale)
    if step == 1:
        m0, v0 = torch.zeros_like(g), torch.zeros_like(g)
    else:
        gi = g * float(gs32)
        m0, v0 = r1 * gi, (0.5 + r2) * gi * gi
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    H.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, coef, grad_scale)
    torch.cuda.synchronize()
    f64 = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    lr_, b1_, b2_, eps_, wd_ = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    gs_ = float(np.float32(grad_scale)) * (float(np.float32(0.37)) if use_coef else 1.0)
    g64, p64, m64, v64 = f64(g) * gs_, f64(p0), f64(m0), f64(v0)
    m64 = m64 + (1.0 - b1_) * (g64 - m64)
    v64 = v64 * b2_ + (1.0 - b2_) * g64 * g64
    bc1, bc2 = 1.0 - b1_ ** step, 1.0 - b2_ ** step
    upd = -(lr_ / bc1) * (m64 / (np.sqrt(v64) / np.sqrt(bc2) + eps_))
    pn64 = p64 * (1.0 - lr_ * wd_) + upd
    em = np.abs(f64(m) - m64) / (np.abs(m64) + np.abs(g64))
    ev = np.abs(f64(v) - v64) / (v64 + g64 * g64)
    ep = np.abs(f64(p) - pn64) / (3.0 * np.abs(p64) + 10.0 * np.abs(upd))
    print(f"adamw step {step}: max err / bar  m {em.max() / (4 * U):.3f}  v {ev.max() / (4 * U):.3f}  "
          f"p {ep.max() / U:.3f}  (bare update: {ep[::2].max() / U:.3f})")
    assert np.all(np.isfinite(f64(p))) and float(np.abs(upd).min()) > 0
    assert em.max() <= 4 * U and ev.max() <= 4 * U
    assert ep.max() <= U


def att_reference(c, gc, h, n, seed):
    """The AttentionGate (channel MLP on the spatial mean, 1x1 spatial gate on g, out = x ca sa) and its backward in
    fp64 autograd, as test_attention builds it: (fp32 inputs, out64, (dx, dg, dw1, db1, dw2, db2, dwg, dbg) in fp64)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, h, generator=g)
    gt = torch.randn(n, gc, h, h, generator=g)
    w1 = torch.randn(c // 8, c, generator=g) * 0.2
    b1 = torch.randn(c // 8, generator=g) * 0.1
    w2 = torch.randn(c, c // 8, generator=g) * 0.2
    b2 = torch.randn(c, generator=g) * 0.1
    wg = torch.randn(1, gc, generator=g) * 0.1
    bg = torch.randn(1, generator=g) * 0.1
    ts = [t.double().requires_grad_(True) for t in (x, gt, w1, b1, w2, b2, wg, bg)]
    xv, gv, w1v, b1v, w2v, b2v, wgv, bgv = ts
    m = xv.mean(dim=(2, 3), keepdim=True)
    hh = F.relu(F.conv2d(m, w1v[:, :, None, None], b1v))
    ca = torch.sigmoid(F.conv2d(hh, w2v[:, :, None, None], b2v))
    sa = torch.sigmoid(F.conv2d(gv, wgv[:, :, None, None], bgv))
    ref = xv * ca * sa
    dout = torch.randn(ref.shape, generator=g)
    ref.backward(dout.double())
    inputs = dict(x=x, g=gt, w1=w1, b1=b1, w2=w2, b2=b2, wg=wg, bg=bg, dout=dout)
    return inputs, ref.detach(), tuple(t.grad for t in ts)


@pytest.mark.parametrize("c,gc,h,n", [
    (128, 256, 20, 3),      # the per-sample kernel at C/4 = 32
    (32, 64, 7, 5),         # the pixel + channel kernels; hw = 49 is no multiple of the 32 row slots
    (96, 64, 6, 4),         # C/4 = 24: 240 active lanes; hw = 36 is no multiple of the 10 row slots
    (512, 64, 5, 3),        # C/4 = 128: two row slots
    (256, 512, 10, 130),    # the unrolled parameter loops on real data
])
def test_attention_against_fp64(c, gc, h, n):
    from superresolution_for_pdes_amd import hipops as H
    inp, ref, grads64 = att_reference(c, gc, h, n, c + gc + h)
    d = {k: inp[k].to(DEV) for k in ("w1", "b1", "w2", "b2", "wg", "bg")}
    xr, gr = rows(inp["x"]).to(DEV), rows(inp["g"]).to(DEV)
    out, saved = H.att_fwd(xr, gr, n, h * h, d["w1"], d["b1"], d["w2"], d["b2"], d["wg"], d["bg"])
    assert rel(unrows(out, n, h, h), ref) < 2e-6
    dx = H.empty(n * h * h, c, device=DEV)
    dg = torch.ones(n * h * h, gc, device=DEV)
    grads = [torch.empty_like(d[k]) for k in ("w1", "b1", "w2", "b2", "wg", "bg")]
    H.att_bwd(rows(inp["dout"]).to(DEV), xr, gr, n, h * h, d["w1"], d["w2"], d["wg"], saved, dx, False, dg, True,
              *grads)
    torch.cuda.synchronize()
    errs = {"dx": rel(unrows(dx, n, h, h), grads64[0]), "dg": rel(unrows(dg, n, h, h) - 1.0, grads64[1])}
    errs.update({k: rel(got, want) for k, got, want in zip(("dw1", "db1", "dw2", "db2", "dwg", "dbg"), grads,
                                                            grads64[2:])})
    print({k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-5, (k, v)


def test_gate_weight_gradient_from_low_res_past_the_unroll_threshold():
    """att_bwd(g_lowres=...) for att3's shapes at n = 300 (c = 256, gc = 512, g = up(d) from 5x5 to 10x10): the
    low-res column sum runs over 7500 rows, past the 6144 at which its unrolled loop starts.  The spatial conv's
    weight and bias gradients against the sum over the upsampled g (test_gate_weight_gradient_from_low_res's
    comparison and bar, 2e-5) and against the same sum in fp64; the channel MLP's, which the two entries form alike,
    bit for bit."""
    from superresolution_for_pdes_amd import hipops as H
    n, c, gc, h, ho = 300, 256, 512, 5, 10
    gen = _gen(n)
    d = torch.randn(n * h * h, gc, device=DEV, generator=gen)
    x = torch.randn(n * ho * ho, c, device=DEV, generator=gen)
    dout = torch.randn(n * ho * ho, c, device=DEV, generator=gen)
    prm = {k: torch.randn(*s, device=DEV, generator=gen) * f for k, s, f in (
        ("w1", (c // 8, c), 0.2), ("b1", (c // 8,), 0.1), ("w2", (c, c // 8), 0.2), ("b2", (c,), 0.1),
        ("wg", (1, gc), 0.1), ("bg", (1,), 0.1))}
    gup = H.upsample_fwd(d, n, h, h, ho, ho)
    _, saved = H.att_fwd(x, gup, n, ho * ho, *(prm[k] for k in ("w1", "b1", "w2", "b2", "wg", "bg")))
    res = []
    for low in (None, (d, h, h, ho, ho)):
        dx, dg = H.empty(n * ho * ho, c, device=DEV), H.empty(n * ho * ho, gc, device=DEV)
        grads = [torch.empty_like(prm[k]) for k in ("w1", "b1", "w2", "b2", "wg", "bg")]
        dsa, _ = H.att_bwd(dout, x, gup, n, ho * ho, prm["w1"], prm["w2"], prm["wg"], saved, dx, False, dg, False,
                           *grads, want_dsa=True, g_lowres=low)
        torch.cuda.synchronize()
        res.append((grads, dsa.double()))
    (gu, _), (gl, dsa) = res
    g64 = rows(F.interpolate(unrows(d.double(), n, h, h), size=(ho, ho), mode="bilinear", align_corners=True))
    dwg64, dbg64 = (g64 * dsa[:, None]).sum(0), dsa.sum()
    for k in range(4):
        assert torch.equal(gl[k], gu[k]), k
    errs = (rel(gl[4], gu[4]), rel(gl[5], gu[5]), rel(gl[4].view(-1), dwg64), rel(gl[5].view(-1), dbg64.view(1)))
    print("low-res dwg / dbg vs upsampled, vs fp64:", [f"{e:.1e}" for e in errs])
    assert max(errs) < 2e-5, errs


# ------------------------------------------ 3. rejected channel counts ------------------------------------------
def test_channel_counts_outside_the_column_sum_are_rejected():
    """A channel count below 4, above 1024 or no multiple of 4 (the gating input's gc, the head's c), or an attention
    c that is no multiple of 32 in 32..1024: the size queries return 0 and the entries return a negative code with a
    message before any launch -- the buffers keep their sentinel."""
    from superresolution_for_pdes_amd import _lib
    cd, sp = _lib.lib(), _lib.stream_ptr()
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    b, nb = buf.data_ptr(), buf.numel() * 4
    for c in (0, 2, 6, 1028, -4):
        assert _lib.query("srpde_head_bwd_workspace_size", 1, 37, c) == 0, c
    for c, gc in ((256, 0), (256, 2), (256, 6), (256, 1028), (0, 64), (16, 64), (48, 64), (1056, 64)):
        assert _lib.query("srpde_att_bwd_workspace_size", 2, 25, c, gc) == 0, (c, gc)
    assert _lib.query("srpde_head_bwd_workspace_size", 1, 37, 16) > 0
    assert _lib.query("srpde_att_bwd_workspace_size", 2, 25, 256, 1024) > 0
    cases = []
    for c in (0, 2, 6, 1028):
        cases.append(("srpde_head_bwd", (b, b, c, c, b, 1, 37, b, c, b, b, b, nb, sp), "channel count"))
    for c, gc in ((256, 2), (256, 1028), (16, 64), (1056, 64)):
        cases.append(("srpde_att_bwd", (b, c, b, c, b, gc, 2, 25, c, gc, b, b, b, b, b, b, b, b, c, 0, b, gc, 0,
                                        b, b, b, b, b, b, b, nb, sp), "channel counts"))
        cases.append(("srpde_att_bwd_params", (b, gc, 2, 25, c, gc, b, b, b, b, b, b, b, b, b, nb, sp),
                      "channel counts"))
        cases.append(("srpde_att_bwd_params_lowres",
                      (b, 1032, 2, 5, 5, 10, 10, c, gc, b, b, b, b, b, b, b, b, b, nb, sp), "channel counts"))
    for name, args, word in cases:
        rc = getattr(cd, name)(*args)
        assert rc < 0 and name in _lib.last_error() and word in _lib.last_error(), (name, args[2:10], rc,
                                                                                    _lib.last_error())
    torch.cuda.synchronize()
    assert bool((buf == 7).all())
    with pytest.raises(RuntimeError, match="srpde_head_bwd: channel count"):
        _lib.call("srpde_head_bwd", b, b, 2, 2, b, 1, 37, b, 2, b, b, b, nb, sp)
