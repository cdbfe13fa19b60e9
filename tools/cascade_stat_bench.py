"""The 40 -> 640 cascade for E examples, batched against sequential, in one process on one GPU.

  batched      one ml_multi_level_upscale_batched call on the [E, n, n] device stacks
  seq_host     E calls of ml_multi_level_upscale (graphs on) on one example's numpy fields each -- what a loop over
               resolution_comparison.solve_multi_resolution's output runs today (per-shape graphs, per-level host
               syncs and field uploads)
  seq_device   the same E calls on device-resident fields: the whole-cascade graph path, which keeps one graph and
               so re-captures it for every other example

Every variant is warmed up (all shapes captured), then the variants are timed alternately `--reps` times with device
events and the medians reported; the batched output is compared with the sequential one.  The batched path is also
run stage by stage (statistics, assembly, forward, stitch per level) with events around each stage.  One JSON line
on stdout (and in --out).

usage: python tools/cascade_stat_bench.py [--examples 10] [--reps 7] [--seed 0] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from superresolution_for_pdes_amd import hipops as H  # noqa: E402
from superresolution_for_pdes_amd import resolution_comparison_statistical as S  # noqa: E402
from superresolution_for_pdes_amd.models import UNet, init_weights  # noqa: E402
from superresolution_for_pdes_amd.resolution_comparison import eval_forward, ml_multi_level_upscale  # noqa: E402

LEVELS = (80, 160, 320, 640)
TILE = 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def staged(model, data, E):
    """One batched cascade with events around every stage -> ({level: {stage: ms}}, result)."""
    marks, cur, res = [], data["u"][40], 40

    def mark():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)
    for nxt in LEVELS:
        u_n, f_n, th_n = data["u"][nxt], data["f"][nxt], data["theta"][nxt]
        mark()
        stats, _ = H.cascade_level_stats(u_n, f_n, th_n)
        mark()
        x = H.cascade_level_assemble(cur, f_n, th_n, stats, TILE)
        mark()
        y = torch.cat([eval_forward(model, x[s:s + 4096], True) for s in range(0, x.shape[0], 4096)])
        mark()
        cur = H.cascade_stitch_denorm(y, stats, E, res, TILE)
        mark()
        res = nxt
    torch.cuda.synchronize()
    out = {}
    for i, nxt in enumerate(LEVELS):
        m = marks[5 * i:5 * i + 5]
        out[nxt] = {k: m[j].elapsed_time(m[j + 1]) for j, k in enumerate(("stats", "assemble", "forward", "stitch"))}
    return out, cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--examples", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cascade_stat_bench: no GPU (a timing needs one)")
    E = a.examples
    torch.manual_seed(a.seed)
    model = UNet().apply(init_weights)
    with torch.no_grad():
        model.final.weight.mul_(1e-3)      # the residual dominates: every level stays in the physical range
    model = model.cuda().eval()
    np.random.seed(a.seed)
    data = S.solve_multi_resolution(E, 40, list(LEVELS))
    per_dev = [{k: {r: v[e].contiguous() for r, v in data[k].items()} for k in ("u", "f", "theta")} for e in range(E)]
    per_host = [{k: {r: v.cpu().numpy() for r, v in d[k].items()} for k in d} for d in per_dev]

    def batched():
        return S.ml_multi_level_upscale_batched(model, data, 640)

    def seq(fields):
        return torch.stack([ml_multi_level_upscale(model, d, 640, "cuda", return_tensor=True) for d in fields])

    variants = {"batched": batched, "seq_host": lambda: seq(per_host), "seq_device": lambda: seq(per_dev)}
    outs = {}
    for name, fn in variants.items():       # warm-up: code objects, every shape's graph
        fn()
        outs[name] = fn()
    scale = float(outs["seq_host"].abs().max())
    diff = {k: float((outs["batched"] - outs[k]).abs().max()) / scale for k in ("seq_host", "seq_device")}
    times = {k: [] for k in variants}
    stages = []
    for _ in range(a.reps):                 # alternate the variants: drift hits all of them alike
        for name, fn in variants.items():
            times[name].append(timed(fn)[1])
        stages.append(staged(model, data, E)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    split = {str(r): {k: statistics.median(s[r][k] for s in stages) for k in ("stats", "assemble", "forward", "stitch")}
             for r in LEVELS}
    result = {
        "tool": "cascade_stat_bench", "device": torch.cuda.get_device_name(0), "examples": E, "reps": a.reps,
        "cascade": "40 -> 640, tile 20, 4 levels", "ms_median": med,
        "ms_min": {k: min(v) for k, v in times.items()}, "ms_max": {k: max(v) for k, v in times.items()},
        "ms_per_example_batched": med["batched"] / E,
        "speedup_vs_seq_host": med["seq_host"] / med["batched"],
        "speedup_vs_seq_device": med["seq_device"] / med["batched"],
        "batched_not_slower": bool(med["batched"] <= min(med["seq_host"], med["seq_device"])),
        "max_abs_diff_over_max_field": diff,
        "batched_level_split_ms_median": split,
        "batched_stage_totals_ms": {k: sum(split[str(r)][k] for r in LEVELS)
                                    for k in ("stats", "assemble", "forward", "stitch")},
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
