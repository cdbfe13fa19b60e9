"""Generate the fixture of the repeated-example study by running the REAL reference (read-only import).

Run where the reference checkout is present (it is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_statistical.py

Like make_golden.py, this imports the reference from ``/root/reference/src`` and stubs the plot / log-only modules
that are absent (``seaborn``, ``torch.utils.tensorboard``; ``pandas`` too where it is not installed -- the numeric
procedure does not touch it).  Everything written is data: inputs' draws and the reference's outputs.

statistical_fixture*.npz: np.random.seed(7), then E = 3 examples from the reference's own
resolution_comparison_statistical.solve_multi_resolution(40, [80, 160]) called three times in sequence; per example
its ml_multi_level_upscale and bilinear_multi_level_upscale and the direct F.interpolate (bilinear as
run_single_example :162-167, bicubic beside it, and resolution_comparison_enhanced.cubic_multi_level_upscale) to
80^2 and 160^2, with the fixture weights and final.weight x CASCADE20_FINAL_SCALE (make_golden.cascade20_fixture:
every level stays in the physical range).  Stored: k1, k2 [3]; per resolution the ground truth's (mean, std, norm,
min, max) [3, 5] and row res // 3 [3, res] (theta's statistics too); the 40^2 start fields; the ML and baseline
fields as fp32 [3, res, res]; their (MAE, RMSE) [3, 2].  The 160^2 fields are stored beside the main file
(state.save_fixture), so no file passes 1 MiB.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
REF = "/root/reference/src"
sys.path.insert(0, REF)

# --- stubs for plot / log-only dependencies that may be absent --------------------------------
tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None,
                                              "add_scalar": lambda self, *a, **k: None,
                                              "close": lambda self: None})
sys.modules["torch.utils.tensorboard"] = tb
for name in ("seaborn", "pandas"):
    if importlib.util.find_spec(name) is None:
        sys.modules[name] = types.ModuleType(name)

import models as ref_models  # noqa: E402  (reference)
import resolution_comparison_enhanced as ref_rce  # noqa: E402
import resolution_comparison_statistical as ref_rcs  # noqa: E402

from state import fixture_state_torch, save_fixture  # noqa: E402

CASCADE20_FINAL_SCALE = 1e-3   # as make_golden.cascade20_fixture
SEED, E, N_COARSE, RESOLUTIONS = 7, 3, 40, [80, 160]


def _stats(a):
    return np.array([a.mean(), a.std(), np.linalg.norm(a), a.min(), a.max()])


def statistical_fixture():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    m = ref_models.UNet()
    m.load_state_dict(fixture_state_torch(dtype=torch.float32))
    m = m.float().eval()
    with torch.no_grad():
        m.final.weight.mul_(CASCADE20_FINAL_SCALE)
    np.random.seed(SEED)
    datas = [ref_rcs.solve_multi_resolution(N_COARSE, RESOLUTIONS) for _ in range(E)]
    out = {"k1": np.array([d["k1"] for d in datas]), "k2": np.array([d["k2"] for d in datas]),
           "final_scale": np.array(CASCADE20_FINAL_SCALE), "seed": np.array(SEED),
           "u40": np.stack([d["u"][N_COARSE] for d in datas])}
    for r in [N_COARSE] + RESOLUTIONS:
        out[f"u{r}_stats"] = np.stack([_stats(d["u"][r]) for d in datas])
        out[f"u{r}_row"] = np.stack([d["u"][r][r // 3].copy() for d in datas])
        out[f"theta{r}_stats"] = np.stack([_stats(d["theta"][r]) for d in datas])
    for tgt in RESOLUTIONS:
        sols = {k: [] for k in ("ml", "blm", "bld", "cbm", "cbd")}
        for d in datas:
            u40 = torch.from_numpy(d["u"][N_COARSE]).float().unsqueeze(0).unsqueeze(0)
            sols["ml"].append(ref_rcs.ml_multi_level_upscale(m, d, tgt, "cpu"))
            sols["blm"].append(ref_rcs.bilinear_multi_level_upscale(d, tgt))
            sols["cbm"].append(ref_rce.cubic_multi_level_upscale(d, tgt))
            sols["bld"].append(torch.nn.functional.interpolate(u40, size=(tgt, tgt), mode="bilinear",
                                                               align_corners=True).squeeze().numpy())
            sols["cbd"].append(torch.nn.functional.interpolate(u40, size=(tgt, tgt), mode="bicubic",
                                                               align_corners=True).squeeze().numpy())
        for k, fields in sols.items():
            errs = [np.asarray(v, np.float64) - d["u"][tgt] for v, d in zip(fields, datas)]
            out[f"{k}{tgt}_metrics"] = np.array([[np.mean(np.abs(e)), np.sqrt(np.mean(e ** 2))] for e in errs])
            out[f"{k}{tgt}"] = np.stack(fields).astype(np.float32)
    big = max(RESOLUTIONS)
    save_fixture("statistical", out, parts={f"{k}{big}": 1 for k in ("ml", "blm", "bld", "cbm", "cbd")})


if __name__ == "__main__":
    statistical_fixture()
    for f in sorted(os.listdir(HERE)):
        if f.startswith("statistical_fixture"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
