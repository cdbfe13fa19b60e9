"""The sample stream and the training command line with zero-flux (Neumann) sides on the GPU (ABI 23:
online.SampleStream(form="divergence", bc=), train_enhanced --bc): the streamed fields solve the problem with those
sides, a sample does not depend on the batch size or the rank that draws it, and a run with the pattern in its loss
trains and records it."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BC = "ddnn"


def _stream(**kw):
    from superresolution_for_pdes_amd.online import SampleStream
    kw.setdefault("n_calib", 64)
    kw.setdefault("theta_range", (0.5, 2.0))
    kw.setdefault("form", "divergence")
    return SampleStream(**kw)


def test_stream_solves_the_problem_with_its_sides():
    """Default sizes 20 / 40 / 80.  The kept fp64 fields satisfy the pattern's equation to 1e-9 rms(f), the bar
    tests/test_gpu_poisson_div.py sets for the stream without a pattern; scored without the pattern they miss it."""
    from superresolution_for_pdes_amd import poisson as P
    s = _stream(seed=3, batch_size=8, bc=BC)
    d = s.describe()
    assert d["bc"] == BC and d["form"] == "divergence" and d["pcg_iters"] == 30
    assert s.state_dict() == {"seed": 3, "step": 0, "bc": BC}
    x, y = s.next_batch(keep_fields=True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    b = s.last_fields["fp64"]
    grids = [tuple(b["standard"][k] for k in ("u_fine", "f_fine", "theta_fine")),
             tuple(b["standard"][k] for k in ("u_coarse", "f_coarse", "theta_coarse")),
             tuple(b["subdomain"][k] for k in ("u", "f", "theta"))]
    assert [g[0].shape[-1] for g in grids] == [40, 20, 80]
    for u, f, th in grids:
        rms_f = f.flatten(1).pow(2).mean(1).sqrt()
        with_bc = P.residual_metrics(u, f, th, form="divergence", bc=BC)[:, 0]
        without = P.residual_metrics(u, f, th, form="divergence")[:, 0]
        print(f"n={u.shape[-1]}: residual / rms(f) with the pattern {float((with_bc / rms_f).max()):.3e}, without "
              f"{float((without / rms_f).min()):.3e}")
        assert bool((with_bc <= 1e-9 * rms_f).all())
        assert bool((without > 1e-9 * rms_f).all())
    # another stream state is refused; the pattern-less stream draws other targets
    with pytest.raises(ValueError):
        _stream(seed=3, batch_size=8).load_state_dict(s.state_dict())
    assert not torch.equal(y, _stream(seed=3, batch_size=8).next_batch()[1])
    plain = _stream(seed=3, batch_size=8)
    assert plain.describe()["bc"] is None and plain.state_dict() == {"seed": 3, "step": 0}
    same = _stream(seed=3, batch_size=8, bc="dddd")            # four ghost-ring sides: the stream without a pattern
    (px, py), (sx, sy) = plain.next_batch(), same.next_batch()
    assert same.bc is None and torch.equal(px, sx) and torch.equal(py, sy)


def test_stream_sample_identity():
    """The same samples come out for a batch of 8 and for two ranks of 4, with the same frozen statistics."""
    whole = _stream(seed=3, batch_size=8, sub_fraction=0.0, bc=BC)
    ranks = [_stream(seed=3, batch_size=4, sub_fraction=0.0, bc=BC, rank=r, world=2) for r in range(2)]
    assert all(torch.equal(whole.stats, r.stats) for r in ranks)
    x, y = whole.next_batch()
    parts = [r.next_batch() for r in ranks]
    assert torch.equal(x, torch.cat([p[0] for p in parts])) and torch.equal(y, torch.cat([p[1] for p in parts]))
    a = _stream(seed=3, batch_size=8, sub_fraction=1.0, bc=BC)
    c = [_stream(seed=3, batch_size=4, sub_fraction=1.0, bc=BC, rank=r, world=2) for r in range(2)]
    xa, ya = a.next_batch()
    pc = [r.next_batch() for r in c]
    assert torch.equal(xa, torch.cat([p[0] for p in pc])) and torch.equal(ya, torch.cat([p[1] for p in pc]))


def test_the_insulated_box_is_refused():
    with pytest.raises(ValueError, match="singular"):
        _stream(seed=3, batch_size=8, bc="nnnn")
    with pytest.raises(ValueError, match='bc belongs to form="divergence"'):
        _stream(seed=3, batch_size=8, form="pointwise", bc=BC)


def test_command_line_online_bc(tmp_path):
    from superresolution_for_pdes_amd.train_enhanced import main
    hist = main(["--online", "2", "--operator", "divergence", "--online-theta", "0.5", "2.0", "--bc", BC,
                 "--pde-div-weight", "0.01", "--epochs", "1", "--batch-size", "8", "--results", str(tmp_path)])
    for k in ("train_loss", "val_loss", "train_mse", "train_pde", "val_mse", "val_pde"):
        assert len(hist[k]) == 1 and np.isfinite(hist[k]).all(), (k, hist[k])
    (run,) = glob.glob(os.path.join(str(tmp_path), "enhanced_run_*"))
    rec = json.load(open(os.path.join(run, "physics_loss.json")))
    assert rec["bc"] == BC and rec["weight"] == 0.01 and rec["form"] == "divergence"
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["bc"] == BC and cfg["operator"] == "divergence"
