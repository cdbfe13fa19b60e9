"""Which kernel every conv entry call runs, in order, over one training step and one eval() forward of the
seeded U-Net at n = 2, 40 x 40: the network's three widths (40, 20, 10) are what select h5 / h4 / h3r / h3 /
h3h / h3g / h3p, so the list pins the entries' dispatch rules and the executor's backward paths.  The names are
srpde_last_kernel's, recorded through hipops.LAUNCH_TAP; tests/golden/conv_dispatch_n2.json is that record of the
code as it stood before the entries' setup and dispatch were shared.  Names and order only: no timings."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_n2.json")


def record_dispatch():
    from oracle import unet_ref as U   # (test infrastructure: the seeded reference initialisation)
    from superresolution_for_pdes_amd import hipops as H
    from superresolution_for_pdes_amd.functional import mse_loss
    from superresolution_for_pdes_amd.models import UNet
    model = UNet()
    model.load_state_dict(U.kaiming_init_state(0))
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 40, 40, generator=g)
    x[:, 1] = 1.0
    t = torch.randn(2, 1, 40, 40, generator=g).to(DEV)
    x = x.to(DEV)
    out = {}
    assert H.LAUNCH_TAP is None
    try:
        H.LAUNCH_TAP = []
        mse_loss(model(x), t).backward()
        torch.cuda.synchronize()
        out["train_step"] = [rec[0] for rec in H.LAUNCH_TAP]
        model.eval()
        H.LAUNCH_TAP = []
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
        out["eval_forward"] = [rec[0] for rec in H.LAUNCH_TAP]
    finally:
        H.LAUNCH_TAP = None
    return out


def test_conv_kernel_dispatch_matches_recorded_order():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record_dispatch()
    assert set(got) == set(want)
    for phase in ("train_step", "eval_forward"):
        assert len(want[phase]) > 0
        assert got[phase] == want[phase], phase
