"""The streamed-sample generator on the GPU (csrc/datastream.hip, ABI 14; online.SampleStream / OnlineBatchLoader;
train_enhanced --online) against the numpy Philox and draw formulas of tests/test_online_host.py.

Every comparison is exact, except: the discrete residual ||theta L_h u - f|| / ||f|| < 1e-9 (test_gpu_poisson_dst's
residual bar) and the CG stream against the sine-transform stream on the fp64 fields, relative L2 < 1e-10 (the
project's solver bar).
"""
import numpy as np
import pytest
import torch

from test_online_host import KNOWN, MASK, draws, stream_words

pytestmark = pytest.mark.gpu

GRIDS = (20, 40, 80)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_raw_words_known_answers():
    from superresolution_for_pdes_amd import hipops as H
    for ctr, key, want in KNOWN:
        seed, sample = key[0] | key[1] << 32, ctr[2] | ctr[3] << 32
        if seed >= 1 << 63:      # the entry takes signed 64-bit values: the same bits
            seed -= 1 << 64
        if sample >= 1 << 63:
            sample -= 1 << 64
        got = _u32(H.stream_raw(seed, sample, 1, ctr[1], ctr[0], 1))
        assert [int(v) for v in got[0, 0]] == list(want), (ctr, [hex(int(v)) for v in got[0, 0]])


def test_raw_words_across_the_32_bit_sample_boundary():
    """4,096 consecutive counters: 64 samples around 2^32 x 64 elements, field 1."""
    from superresolution_for_pdes_amd import hipops as H
    first, ns, e0, ne = (1 << 32) - 32, 64, 5, 64
    got = _u32(H.stream_raw(12345678901234567, first, ns, 1, e0, ne))
    want = stream_words(12345678901234567, range(first, first + ns), 1, np.arange(e0, e0 + ne))
    assert got.shape == want.shape == (64, 64, 4) and np.array_equal(got, want)
    assert not np.array_equal(got[31], got[32])
    # the last element a 32-bit counter word holds
    got = _u32(H.stream_raw(-5, 7, 2, 0, MASK - 2, 3))
    assert np.array_equal(got, stream_words(-5, [7, 8], 0, np.arange(MASK - 2, MASK + 1)))


@pytest.mark.parametrize("first", [0, (1 << 40) + 7])
def test_draws_equal_the_numpy_formulas(first):
    from superresolution_for_pdes_amd import hipops as H
    B, n, seed, ms = 5, 8, 3, 4
    wk, ws, wt = draws(seed, first, B, (0.5, 12.0), (0.5, 2.0), n=n, max_start=ms)
    k, s, t, th = H.stream_draw(seed, first, B, (0.5, 12.0), (0.5, 2.0), n=n, max_start=ms, theta_half=True)
    assert s.dtype == torch.int32 and k.dtype == t.dtype == torch.float64
    assert np.array_equal(k.cpu().numpy(), wk) and np.array_equal(s.cpu().numpy(), ws)
    assert np.array_equal(t.cpu().numpy(), wt) and np.array_equal(th.cpu().numpy(), wt[:, ::2, ::2])
    assert 0 <= ws.min() and ws.max() < ms and len(np.unique(wt)) == wt.size
    # ones mode: the same k and starts, theta exactly 1
    k1, s1, t1, th1 = H.stream_draw(seed, first, B, (0.5, 12.0), None, n=n, max_start=ms, theta_half=True)
    assert torch.equal(k1, k) and torch.equal(s1, s)
    assert bool((t1 == 1.0).all()) and bool((th1 == 1.0).all()) and t1.shape == (B, n, n) and th1.shape == (B, 4, 4)
    # a sample's values do not depend on the batch it is drawn in
    k2, s2, t2, _ = H.stream_draw(seed, first + 2, 3, (0.5, 12.0), (0.5, 2.0), n=n, max_start=ms)
    assert torch.equal(k2, k[2:]) and torch.equal(s2, s[2:]) and torch.equal(t2, t[2:])
    # an odd grid: the last element holds one pixel; no theta, no starts: k alone
    k3, s3, t3, th3 = H.stream_draw(seed, first, B, (0.5, 5.0), (0.5, 2.0), n=7, theta_half=True)
    w3 = draws(seed, first, B, (0.5, 5.0), (0.5, 2.0), n=7)
    assert s3 is None and np.array_equal(k3.cpu().numpy(), w3[0]) and np.array_equal(t3.cpu().numpy(), w3[2])
    assert np.array_equal(th3.cpu().numpy(), w3[2][:, ::2, ::2])
    k4, s4, t4, _ = H.stream_draw(seed, first, B, (0.5, 5.0))
    assert s4 is None and t4 is None and torch.equal(k4, k3)


def test_window_equals_numpy_slicing():
    from superresolution_for_pdes_amd import hipops as H
    B, ns, nf = 3, 12, 6
    ms = ns - nf
    rng = np.random.default_rng(0)
    u, f, th = (rng.standard_normal((B, ns, ns)) for _ in range(3))
    starts = np.array([[0, 0], [ms - 1, ms - 1], [2, 5]], dtype=np.int32)     # (x, y)
    dev = [torch.from_numpy(a).cuda() for a in (u, f, th)]
    got = [t.cpu().numpy() for t in H.stream_window(*dev, torch.from_numpy(starts).cuda(), nf)]
    assert [g.dtype for g in got] == [np.float32] * 4

    def crop(a):
        return np.stack([a[b, y:y + nf, x:x + nf] for b, (x, y) in enumerate(starts)]).astype(np.float32)
    for g, a in zip(got[:3], (u, f, th)):
        assert np.array_equal(g, crop(a))
    assert got[3].shape == (B, 3, 3) and np.array_equal(got[3], crop(u)[:, ::2, ::2])
    # pass-through: the window is the field, the coarse field a solve of its own
    uf, ff, tf = (a[:, :nf, :nf].copy() for a in (u, f, th))
    uc = rng.standard_normal((B, 3, 3))
    dev = [torch.from_numpy(a).cuda() for a in (uf, ff, tf)]
    got = [t.cpu().numpy() for t in H.stream_window(*dev, None, nf, u_coarse_in=torch.from_numpy(uc).cuda())]
    for g, a in zip(got, (uf, ff, tf, uc)):
        assert np.array_equal(g, a.astype(np.float32))
    got = H.stream_window(*dev, None, nf)[3].cpu().numpy()
    assert np.array_equal(got, uf.astype(np.float32)[:, ::2, ::2])
    # into row slices of a larger buffer, an odd window, more than one workgroup
    B2, ns2, nf2 = 7, 23, 11
    a = rng.standard_normal((3, B2, ns2, ns2))
    st = rng.integers(0, ns2 - nf2, (B2, 2)).astype(np.int32)
    bufs = tuple(torch.full((B2 + 2, m, m), 7.0, dtype=torch.float32, device="cuda") for m in (nf2, nf2, nf2, 6))
    H.stream_window(*[torch.from_numpy(x).cuda() for x in a], torch.from_numpy(st).cuda(), nf2,
                    out=tuple(b[1:B2 + 1] for b in bufs))
    for i, b in enumerate(bufs):
        src = a[min(i, 2) if i < 3 else 0]
        want = np.stack([src[s, y:y + nf2, x:x + nf2] for s, (x, y) in enumerate(st)]).astype(np.float32)
        want = want[:, ::2, ::2] if i == 3 else want
        got = b.cpu().numpy()
        assert np.array_equal(got[1:B2 + 1], want) and np.all(got[0] == 7.0) and np.all(got[-1] == 7.0)


def _stream(**kw):
    from superresolution_for_pdes_amd.online import SampleStream
    kw.setdefault("n_calib", 64)
    return SampleStream(**kw)


def _apply_operator(u, theta):
    """theta * L_h u on the n x n grid, h = 1 / (n - 1), zero ghost ring (the reference's diag(theta) @ L)."""
    n = u.shape[-1]
    p = np.pad(u, ((0, 0), (1, 1), (1, 1)))
    lap = (p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:] - 4.0 * u) * float((n - 1) ** 2)
    return theta * lap


def _rebuild(stream, first, B):
    """Batch `first .. first + B - 1` from the numpy draws, the project's forcing / sine-transform solve, numpy crop and
    stride, and pde_dataset_assemble with the stream's frozen statistics -> (inputs, targets, fp64 (u, f, theta) list)."""
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd import poisson as P
    from superresolution_for_pdes_amd.online import n_standard
    nc, nf, nsf = GRIDS
    n_std = n_standard(B, stream.sub_fraction)
    tr = stream.theta_range
    k, _, th_f = draws(stream.seed, first, n_std, stream.k_std, tr, n=nf)
    f_f, f_c = P.forcing_batched(k, nf), P.forcing_batched(k, nc)
    th_c = np.ascontiguousarray(th_f[:, ::2, ::2])
    u_f = P.solve_batched(f_f, th_f, method="dst").cpu().numpy()
    u_c = P.solve_batched(f_c, th_c, method="dst").cpu().numpy()
    f_f, f_c = f_f.cpu().numpy(), f_c.cpu().numpy()
    k, starts, th = draws(stream.seed, first + n_std, B - n_std, stream.k_sub, tr, n=nsf, max_start=nsf - nf)
    f = P.forcing_batched(k, nsf)
    u = P.solve_batched(f, th, method="dst").cpu().numpy()
    f = f.cpu().numpy()

    def crop(a):
        return np.stack([a[b, y:y + nf, x:x + nf] for b, (x, y) in enumerate(starts)])
    cu = crop(u)
    fields = {"u_fine": np.concatenate([u_f, cu]), "f_fine": np.concatenate([f_f, crop(f)]),
              "theta_fine": np.concatenate([th_f, crop(th)]), "u_coarse": np.concatenate([u_c, cu[:, ::2, ::2]])}
    dev = {key: torch.from_numpy(v.astype(np.float32)).cuda() for key, v in fields.items()}
    x, y = H.pde_dataset_assemble(dev["u_coarse"], dev["u_fine"], dev["theta_fine"], dev["f_fine"], stream.stats,
                                  stream.theta_is_constant)
    return x, y, [(u_f, f_f, th_f), (u_c, f_c, th_c), (u, f, th)], fields


@pytest.fixture(scope="module", params=[None, (0.5, 2.0)], ids=["theta1", "theta_uniform"])
def whole_batch(request):
    """One stream per theta mode, its first batch with the fields kept, and the batch rebuilt in the test."""
    s = _stream(seed=1, batch_size=6, sub_fraction=0.5, theta_range=request.param)
    x, y = s.next_batch(keep_fields=True)
    return s, x, y, s.last_fields, _rebuild(s, 0, 6)


def test_whole_batch_is_bit_equal_to_its_rebuild(whole_batch):
    s, x, y, fields, (wx, wy, _, wfields) = whole_batch
    assert x.shape == (6, 3, 40, 40) and y.shape == (6, 1, 40, 40) and x.dtype == y.dtype == torch.float32
    assert list(fields["is_subdomain"]) == [False] * 3 + [True] * 3
    for key, want in wfields.items():
        assert np.array_equal(fields[key].cpu().numpy(), want.astype(np.float32)), key
    assert torch.equal(x, wx) and torch.equal(y, wy)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    if s.theta_range is None:
        assert s.theta_is_constant and bool((x[:, 1] == 1.0).all())
    else:
        assert not s.theta_is_constant and float(x[:, 1].std()) > 0.5


def test_whole_batch_solves_the_discrete_equation(whole_batch):
    s, _, _, fields, (_, _, rebuilt, _) = whole_batch
    b = fields["fp64"]
    mine = [(b["standard"][k] for k in ("u_fine", "f_fine", "theta_fine")),
            (b["standard"][k] for k in ("u_coarse", "f_coarse", "theta_coarse")),
            (b["subdomain"][k] for k in ("u", "f", "theta"))]
    for grid, want in zip(mine, rebuilt):
        u, f, th = (t.cpu().numpy() for t in grid)
        assert np.array_equal(u, want[0]) and np.array_equal(f, want[1]) and np.array_equal(th, want[2])
        r = _apply_operator(u, th) - f
        res = np.linalg.norm(r.reshape(len(u), -1), axis=1) / np.linalg.norm(f.reshape(len(u), -1), axis=1)
        print(f"n={u.shape[-1]}: residual {res.max():.3e}")
        assert res.max() < 1e-9


def test_cg_stream_gives_the_same_batch(whole_batch):
    s, _, _, fields, _ = whole_batch
    c = _stream(seed=1, batch_size=6, sub_fraction=0.5, theta_range=s.theta_range, solver="cg")
    c.next_batch(keep_fields=True)
    a, b = fields["fp64"], c.last_fields["fp64"]
    for kind, keys in (("standard", ("u_fine", "u_coarse")), ("subdomain", ("u",))):
        for key in a[kind]:
            if key in keys:
                d = (a[kind][key] - b[kind][key]).flatten(1).norm(dim=1) / a[kind][key].flatten(1).norm(dim=1)
                print(f"{kind} {key}: cg vs dst {float(d.max()):.3e}")
                assert float(d.max()) < 1e-10
            else:
                assert torch.equal(a[kind][key], b[kind][key]), (kind, key)


def test_determinism_sharding_and_resume():
    a, b = (_stream(seed=5, batch_size=4) for _ in range(2))
    assert torch.equal(a.stats, b.stats)
    steps = [a.next_batch() for _ in range(6)]
    for t in range(2):
        x, y = b.next_batch()
        assert torch.equal(x, steps[t][0]) and torch.equal(y, steps[t][1])
    assert not torch.equal(steps[0][0], steps[1][0]) and not torch.equal(steps[0][1], steps[1][1])
    other = _stream(seed=6, batch_size=4).next_batch()
    assert not torch.equal(other[0], steps[0][0])
    # world 2: rank r at step t is the single-process step 2 t + r (the statistics do not depend on the rank)
    ranks = [_stream(seed=5, batch_size=4, rank=r, world=2) for r in range(2)]
    for t in range(3):
        for r in range(2):
            assert list(ranks[r].indices()) == list(range((2 * t + r) * 4, (2 * t + r + 1) * 4))
            x, y = ranks[r].next_batch()
            assert torch.equal(x, steps[2 * t + r][0]) and torch.equal(y, steps[2 * t + r][1])
    # resuming after three steps reproduces step 3
    b.next_batch()
    state = b.state_dict()
    assert state == {"seed": 5, "step": 3}
    c = _stream(seed=5, batch_size=4)
    c.load_state_dict(state)
    x, y = c.next_batch()
    assert torch.equal(x, steps[3][0]) and torch.equal(y, steps[3][1])
    with pytest.raises(ValueError):
        _stream(seed=6, batch_size=4).load_state_dict(state)


@pytest.mark.parametrize("theta_range", [None, (0.5, 2.0)], ids=["theta1", "theta_uniform"])
def test_frozen_statistics_are_pde_dataset_statistics(theta_range):
    from superresolution_for_pdes_amd import online as O
    from superresolution_for_pdes_amd.models import PDEDataset
    s = _stream(seed=2, batch_size=4, theta_range=theta_range)
    cal = s.fixed_set(64, O.CALIB_FIRST)
    assert int(cal["is_subdomain"].sum()) == 32 and cal["u_fine"].shape == (64, 40, 40)
    ds = PDEDataset(cal)
    want = torch.stack([torch.as_tensor(v, dtype=torch.float32, device="cuda") for v in
                        (ds.u_mean, ds.u_std, ds.f_mean, ds.f_std, ds.theta_mean, ds.theta_std)])
    assert s.stats.dtype == torch.float32 and torch.equal(s.stats, want)
    assert s.theta_is_constant == ds.theta_is_constant == (theta_range is None)
    # the calibration set normalised with its own statistics is the PDEDataset
    fz = s.frozen_set(64, O.CALIB_FIRST)
    assert torch.equal(fz.inputs, ds.inputs) and torch.equal(fz.targets, ds.targets)
    assert torch.equal(fz.denormalize(fz.targets), ds.denormalize(ds.targets))
    # held-out sets are fixed, distinct, and refused outside their ranges
    v1, v2 = s.fixed_set(8, O.VALID_FIRST), s.fixed_set(8, O.VALID_FIRST)
    assert all(torch.equal(v1[k], v2[k]) for k in ("u_fine", "f_fine", "theta_fine", "u_coarse"))
    assert not torch.equal(v1["u_fine"], cal["u_fine"][:8])
    for n, first in ((8, 0), (8, O.CALIB_END - 4), (8, O.VALID_END - 4), (0, O.VALID_FIRST)):
        with pytest.raises(ValueError):
            s.fixed_set(n, first)


def _train_once(tmp_path, tag):
    from superresolution_for_pdes_amd.functional import MSELoss
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.online import OnlineBatchLoader
    from superresolution_for_pdes_amd.optim import FusedAdamW
    from superresolution_for_pdes_amd.train_enhanced import train_model
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    s = _stream(seed=11, batch_size=8)
    train, val = OnlineBatchLoader(s, 3), s.validation_loader(16)
    assert len(train) == 3 and len(val) == 2
    model = UNet().to("cuda")
    model.apply(init_weights)
    opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=10, min_lr=1e-6)
    out = tmp_path / tag
    out.mkdir()
    hist = train_model(model, train, val, MSELoss(), opt, sched, 2, "cuda", out, None)
    assert s.step == 6 and (out / "best_model.pth").exists()
    assert torch.equal(train.denormalize(torch.ones((), device="cuda")), s.stats[1] + s.stats[0])
    return hist


def test_train_model_on_the_stream(tmp_path):
    h1, h2 = _train_once(tmp_path, "a"), _train_once(tmp_path, "b")
    assert h1["num_epochs"] == 2 and len(h1["train_loss"]) == len(h1["val_loss"]) == 2
    assert np.all(np.isfinite(h1["train_loss"] + h1["val_loss"]))
    assert h1 == h2


def test_command_line(tmp_path):
    from superresolution_for_pdes_amd.train_enhanced import main
    hist = main(["--online", "2", "--epochs", "1", "--batch-size", "8", "--results", str(tmp_path)])
    assert hist["num_epochs"] == 1 and np.isfinite(hist["train_loss"][0])
    assert len(list(tmp_path.glob("enhanced_run_*/best_model.pth"))) == 1
    with pytest.raises(SystemExit):
        main(["--online-theta", "0.5", "2.0", "--results", str(tmp_path)])
