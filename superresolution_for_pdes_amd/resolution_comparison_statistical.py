"""Repeated-example statistics of the cascade against its interpolation baselines on MI355X.

Reference: src/resolution_comparison_statistical.py -- ``solve_multi_resolution`` :25-96 (k1, k2 ~ U(8, 12), theta ~
U(0.5, 2) on the finest grid, strided to every resolution, solve times kept), ``run_single_example`` :98-205 (ML
cascade, multi-level and direct bilinear to every resolution, MAE / RMSE and timings) and the tables of
``plot_statistical_analysis`` :475-499 (mean / std / min / max per resolution and method).  The reference runs its
examples one after the other and stops at its plotting call; the numeric procedure before that call is
what is kept, the plots are out of scope.

Difference: the E examples run side by side.  The ground truth is one batched CG solve per resolution, a cascade
level is one statistics pass, one assembly pass, the batched U-Net forward and one stitch pass for all examples
(hipops.cascade_level_stats / _assemble / _stitch_denorm, csrc/cascade.hip) with no host synchronisation in the level
loop, the baselines are one resize call per step, and every metric comes from srpde_field_metrics.  Times are HIP-event
times of the batched call divided by E.  The bicubic baselines of resolution_comparison_enhanced are tabulated beside
the reference's three methods.  Tables are computed with numpy (sample std, ddof = 1, as pandas' ``.std()``).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
from datetime import datetime
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import hipops as H
from . import poisson as P
from .resolution_comparison import eval_forward

# (metrics key prefix, label of the reference's tables); the first three are the reference's methods
METHODS = (("ml", "ML Multi-level"), ("bilinear_multi", "Bilinear Multi-level"), ("bilinear_direct", "Direct Bilinear"),
           ("cubic_multi", "Cubic Multi-level"), ("cubic_direct", "Direct Cubic"))


def draw_fields(n_examples: int, n_coarse: int = 40, resolutions: Sequence[int] = (80, 160, 320, 640),
                k_range=(8.0, 12.0)) -> dict:
    """The random draws and host-side fields of ``n_examples`` test cases (:39-72): per example k1, k2, then theta
    on the finest grid -- the np.random calls, in the order, of calling the reference's solve_multi_resolution once
    per example, so a seed reproduces its fields.  f = sin(2 pi k1 X) sin(2 pi k2 Y) on the finest grid in numpy;
    both strided to every resolution.  Returns k1, k2 [E] and f / theta {res: [E, res, res]} (fp64 numpy)."""
    resolutions = list(resolutions)
    n_finest = max(resolutions)
    x = np.linspace(0, 1, n_finest)
    X, Y = np.meshgrid(x, x)
    k1s, k2s, fs, ths = [], [], [], []
    for _ in range(n_examples):
        k1 = np.random.uniform(k_range[0], k_range[1])
        k2 = np.random.uniform(k_range[0], k_range[1])
        fs.append(np.sin(k1 * 2 * np.pi * X) * np.sin(k2 * 2 * np.pi * Y))
        ths.append(np.random.uniform(0.5, 2.0, size=(n_finest, n_finest)))
        k1s.append(k1)
        k2s.append(k2)
    f_finest = np.stack(fs) if fs else np.zeros((0, n_finest, n_finest))
    th_finest = np.stack(ths) if ths else np.zeros((0, n_finest, n_finest))
    out = {"k1": np.array(k1s), "k2": np.array(k2s), "f": {}, "theta": {}}
    for res in [n_coarse] + resolutions:
        step = n_finest // res
        out["f"][res] = np.ascontiguousarray(f_finest[:, ::step, ::step])
        out["theta"][res] = np.ascontiguousarray(th_finest[:, ::step, ::step])
    return out


def _timed(fn, n_examples: int, device):
    """(fn(), HIP-event seconds of the call / n_examples)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream(device)
    start.record(stream)
    out = fn()
    end.record(stream)
    end.synchronize()
    return out, start.elapsed_time(end) * 1e-3 / max(n_examples, 1)


def solve_multi_resolution(n_examples: int = 1, n_coarse: int = 40, resolutions: Sequence[int] = (80, 160, 320, 640),
                           k_range=(8.0, 12.0), device="cuda", solver: str = "cg") -> dict:
    """:25-96 for ``n_examples`` fields at once: draw_fields, then ONE batched solve per resolution (``solver``: "cg"
    or "dst", poisson.solve_batched's method) on the [E, res, res] stack.  data['u' | 'f' | 'theta'][res] are [E, res, res] fp64 device tensors, data['k1'], ['k2']
    length-E arrays, data['solve_times'][res] the HIP-event time of the batched solve divided by E."""
    device = torch.device(device)
    P.check_solver(solver)
    drawn = draw_fields(n_examples, n_coarse, resolutions, k_range)
    data = {"k1": drawn["k1"], "k2": drawn["k2"], "f": {}, "theta": {}, "u": {}, "solve_times": {}}
    for res in [n_coarse] + list(resolutions):
        data["f"][res] = torch.from_numpy(drawn["f"][res]).to(device)
        data["theta"][res] = torch.from_numpy(drawn["theta"][res]).to(device)
        data["u"][res], data["solve_times"][res] = _timed(
            lambda: P.solve_batched(data["f"][res], data["theta"][res], device=device, method=solver), n_examples,
            device)
    return data


def _stack(a, device) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.to(device=device, dtype=torch.float64)
    return (t[None] if t.dim() == 2 else t).contiguous()


@torch.no_grad()
def ml_multi_level_upscale_batched(model, data: dict, target_resolution: int, start_resolution: int = 40,
                                   tile: int = 20, max_batch: int = 4096, graphs: bool = True,
                                   return_tensor: bool = True):
    """ml_multi_level_upscale (resolution_comparison.py:183-229) for every example of ``data`` at once: per level
    the ground-truth statistics of the next resolution per example (the reference's label leak, kept), the
    normalised tiles of all examples as one batch, the U-Net in chunks of ``max_batch`` tiles (eval_forward, its
    per-shape graphs), denormalise and stitch.  No host synchronisation inside the level loop (the theta-constant
    test stays on the device).  -> [E, target, target] fp64 (device tensor, or numpy)."""
    model.eval()
    device = next(model.parameters()).device
    cur = _stack(data["u"][start_resolution], device)
    E, res = cur.shape[0], start_resolution
    while res < target_resolution:
        nxt = res * 2
        u_n, f_n, th_n = (_stack(data[k][nxt], device) for k in ("u", "f", "theta"))
        stats, _ = H.cascade_level_stats(u_n, f_n, th_n)
        x = H.cascade_level_assemble(cur, f_n, th_n, stats, tile)
        outs = [eval_forward(model, x[s:s + max_batch], graphs) for s in range(0, x.shape[0], max_batch)]
        y = outs[0] if len(outs) == 1 else torch.cat(outs)
        cur = H.cascade_stitch_denorm(y.contiguous(), stats, E, res, tile)
        res = nxt
    return cur if return_tensor else cur.cpu().numpy()


def _resize(u: torch.Tensor, size: int, mode: str) -> torch.Tensor:
    """[E, h, w] fp32 device fields -> [E, size, size] (align_corners=True), one kernel call for all examples."""
    E, h, w = u.shape
    if mode == "bilinear":
        return H.upsample_fwd(u.contiguous().view(E * h * w, 1), E, h, w, size, size).view(E, size, size)
    if mode == "bicubic":
        return H.resize_bicubic(u.contiguous(), size, size)
    raise ValueError(mode)


def interpolate_batched(u_start: torch.Tensor, target_resolution: int, mode: str, multi_level: bool) -> torch.Tensor:
    """The interpolation baselines (resolution_comparison_enhanced.py:19-65 repeated 2x steps, :371-392 one resize)
    of the fp32-cast start fields [E, n, n], all examples per call."""
    cur = u_start.float()
    if not multi_level:
        return _resize(cur, target_resolution, mode)
    res = cur.shape[-1]
    while res < target_resolution:
        res *= 2
        cur = _resize(cur, res, mode)
    return cur


def run_examples(model, n_examples: int = 10, resolutions: Sequence[int] = (80, 160, 320, 640), seed=None,
                 device="cuda", solver: str = "cg") -> List[Dict]:
    """run_single_example (:98-205) for ``n_examples`` fields side by side: the list of per-example metric dicts with
    the reference's keys (example, k1, k2, resolutions, {ml, bilinear_multi, bilinear_direct}_{mae, rmse},
    {ml, bilinear_multi, bilinear_direct}_times, solve_times) plus cubic_multi_* / cubic_direct_*.  Every time is
    the HIP-event time of the batched call divided by E (the ML cascade's after one untimed call, so that graph
    capture is not in it); every metric comes from srpde_field_metrics."""
    if seed is not None:
        np.random.seed(seed)
    device = torch.device(device)
    resolutions = list(resolutions)
    data = solve_multi_resolution(n_examples, 40, resolutions, device=device, solver=solver)
    E = n_examples
    start = data["u"][40]
    cols = {f"{k}_{m}": [] for k, _ in METHODS for m in ("mae", "rmse", "times")}
    for res in resolutions:
        ml_multi_level_upscale_batched(model, data, res)
        sols = {}
        sols["ml"] = _timed(lambda: ml_multi_level_upscale_batched(model, data, res), E, device)
        for key, mode, multi in (("bilinear_multi", "bilinear", True), ("bilinear_direct", "bilinear", False),
                                 ("cubic_multi", "bicubic", True), ("cubic_direct", "bicubic", False)):
            sols[key] = _timed(lambda: interpolate_batched(start, res, mode, multi), E, device)
        for key, (pred, secs) in sols.items():
            mt = H.field_metrics(pred.contiguous(), data["u"][res]).cpu().numpy()
            cols[f"{key}_mae"].append(mt[:, 0])
            cols[f"{key}_rmse"].append(mt[:, 1])
            cols[f"{key}_times"].append(secs)
    all_metrics = []
    for e in range(E):
        m = {"example": e + 1, "k1": float(data["k1"][e]), "k2": float(data["k2"][e]), "resolutions": list(resolutions)}
        for key, _ in METHODS:
            m[f"{key}_mae"] = [float(v[e]) for v in cols[f"{key}_mae"]]
            m[f"{key}_rmse"] = [float(v[e]) for v in cols[f"{key}_rmse"]]
            m[f"{key}_times"] = [float(t) for t in cols[f"{key}_times"]]
        m["solve_times"] = [float(data["solve_times"][res]) for res in resolutions]
        all_metrics.append(m)
    return all_metrics


def summarize(all_metrics: List[Dict]) -> Dict:
    """The table of :475-479: {resolution: {method label: {'MAE' | 'RMSE': {mean, std, min, max}}}} over the
    examples; std is the sample standard deviation (ddof = 1, NaN for one example, as pandas' ``.std()``).
    Methods whose keys are absent from the metric dicts are left out."""
    out: Dict = {}
    for key, label in METHODS:
        if not all_metrics or f"{key}_mae" not in all_metrics[0]:
            continue
        for name, suffix in (("MAE", "mae"), ("RMSE", "rmse")):
            per_res: Dict = {}
            for m in all_metrics:
                for i, res in enumerate(m["resolutions"]):
                    per_res.setdefault(res, []).append(m[f"{key}_{suffix}"][i])
            for res, vals in per_res.items():
                v = np.asarray(vals, np.float64)
                out.setdefault(res, {}).setdefault(label, {})[name] = {
                    "mean": float(v.mean()), "std": float(v.std(ddof=1)) if v.size > 1 else float("nan"),
                    "min": float(v.min()), "max": float(v.max())}
    return out


def write_summary(all_metrics: List[Dict], save_dir) -> Dict:
    """statistical_summary.csv (the layout of the reference's grouped table: Resolution, Method, then mean / std /
    min / max of MAE and RMSE, six decimals), .json (the same table unrounded, with the per-example metrics) and
    .txt (the reference's text summary, :484-499, line for line)."""
    save_dir = str(save_dir)
    os.makedirs(save_dir, exist_ok=True)
    table = summarize(all_metrics)
    agg = ("mean", "std", "min", "max")
    with open(os.path.join(save_dir, "statistical_summary.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", ""] + ["MAE"] * 4 + ["RMSE"] * 4)
        w.writerow(["", ""] + list(agg) * 2)
        w.writerow(["Resolution", "Method"] + [""] * 8)
        for res in sorted(table):
            for label in sorted(table[res]):
                row = table[res][label]
                w.writerow([res, label] + [round(row[n][a], 6) for n in ("MAE", "RMSE") for a in agg])
    with open(os.path.join(save_dir, "statistical_summary.json"), "w") as f:
        json.dump({"n_examples": len(all_metrics), "summary": {str(r): v for r, v in table.items()},
                   "examples": all_metrics}, f, indent=2)
    with open(os.path.join(save_dir, "statistical_summary.txt"), "w") as f:
        f.write(f"Statistical Summary of {len(all_metrics)} Examples\n")
        f.write("=" * 50 + "\n\n")
        for res in table:
            f.write(f"\nResults for {res}x{res} Resolution:\n")
            f.write("-" * 40 + "\n")
            for _, label in METHODS:
                if label not in table[res]:
                    continue
                mae, rmse = table[res][label]["MAE"], table[res][label]["RMSE"]
                f.write(f"\n{label}:\n")
                f.write(f"  MAE:  mean = {mae['mean']:.6f} ± {mae['std']:.6f}\n")
                f.write(f"        min = {mae['min']:.6f}, max = {mae['max']:.6f}\n")
                f.write(f"  RMSE: mean = {rmse['mean']:.6f} ± {rmse['std']:.6f}\n")
                f.write(f"        min = {rmse['min']:.6f}, max = {rmse['max']:.6f}\n")
    return table


def arg_parser():
    ap = argparse.ArgumentParser(description="Statistical analysis of upscaling methods")
    ap.add_argument("--model_path", type=str, required=True, help="Path to the model file")
    ap.add_argument("--n_examples", type=int, default=10, help="Number of examples to run")
    ap.add_argument("--seed", type=int, default=None, help="np.random seed of the test fields (reference: unseeded)")
    ap.add_argument("--resolutions", type=int, nargs="+", default=[80, 160, 320, 640],
                    help="Target resolutions (reference: 80 160 320 640)")
    ap.add_argument("--solver", choices=("cg", "dst"), default="cg",
                    help="Ground-truth Poisson solver: conjugate gradients (default) or the direct sine transform")
    return ap


def main(argv=None):
    """CLI of the reference (:501-540) plus ``--seed``, ``--resolutions`` and ``--solver``: the summary files go into
    ``resolution_comparison_statistical_<timestamp>/`` next to the checkpoint.  Returns that directory."""
    from .compare_methods import load_model
    args = arg_parser().parse_args(argv)
    if not os.path.exists(args.model_path):
        raise FileNotFoundError(f"Model not found at path: {args.model_path}")
    model = load_model(args.model_path, "cuda")
    model.eval()
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    results_dir = os.path.join(os.path.dirname(os.path.abspath(args.model_path)),
                               f"resolution_comparison_statistical_{stamp}")
    all_metrics = run_examples(model, args.n_examples, args.resolutions, seed=args.seed, solver=args.solver)
    write_summary(all_metrics, results_dir)
    print(f"\nResults saved in: {results_dir}")
    return results_dir


if __name__ == "__main__":
    main()
