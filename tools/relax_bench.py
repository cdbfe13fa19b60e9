"""What polishing a cascade level with weighted-Jacobi sweeps does and costs (poisson.relax,
relax_kernel<PointwiseOp> of csrc/relax.hip).

    python tools/relax_bench.py [--model_path best_model.pth] [--out profiles/relax_bench.json]

1. Cascade quality and cost.  E seeded fields of solve_multi_resolution, 40 -> 640, through
   tiled_inference.upscale_cascade for two variants -- stride 10 / linear window / input statistics (no ground truth) and
   stride 20 / truth statistics (the reference's disjoint tiles) -- at polish = 0, 2, 4, 8, 16 sweeps per level.  Per row:
   RMSE against the 640^2 solution, the residual RMS of the discrete equation (poisson.residual_metrics), the seam
   figure of tools/tiled_inference_bench.py, and ms per call (HIP events, median of ``--reps`` repeats in which all rows
   take turns).  The polish = 0 time stands beside the figure the same variant has in
   profiles/tiled_inference_bench.json (the commit before the smoother).
2. The kernel alone.  E fields of 640^2, sweeps = K and 2K (one and two launches): ms per call (``calls`` back to back
   between two events, median of the repeats) beside the traffic floor of a launch -- u, f, theta read and u written
   once, 32 bytes per node, at the 8.0 TB/s HBM peak of the MI355X -- and the fraction floor / measured.

The model comes as in tools/tiled_inference_bench.py: --model_path, or a seeded short online run here (same seed and
steps as that tool's record, so the polish = 0 rows repeat its rows).  A recorded observation, not a pass criterion.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tiled_inference_bench as TB  # noqa: E402
from superresolution_for_pdes_amd import hipops as H  # noqa: E402
from superresolution_for_pdes_amd import poisson as P  # noqa: E402
from superresolution_for_pdes_amd import resolution_comparison_statistical as S  # noqa: E402
from superresolution_for_pdes_amd import tiled_inference as T  # noqa: E402

VARIANTS = ({"stride": 10, "window": "linear", "stats": "input"}, {"stride": 20, "window": "linear", "stats": "truth"})
POLISH = (0, 2, 4, 8, 16)
HBM_PEAK = 8.0e12          # bytes / s, the MI355X's specified HBM3E peak
BYTES_PER_NODE = 32        # a launch reads u, f, theta and writes u, fp64


def parent_ms(variant, start, target):
    """ms per call of the same variant in profiles/tiled_inference_bench.json (recorded before polish existed)"""
    path = os.path.join(ROOT, "profiles", "tiled_inference_bench.json")
    if not os.path.exists(path):
        return None
    rec = json.load(open(path))["cascade"]
    if (rec["from"], rec["to"]) != (start, target):
        return None
    for r in rec["rows"]:
        if all(r[k] == variant[k] for k in variant):
            return r["ms"]
    return None


def cascade(model, data, start, target, reps, omega):
    def run(v, k):
        return T.upscale_cascade(model, data["u"][start], data["f"], data["theta"], target, tile=TB.TILE,
                                 u_truth=data["u"], polish=k, polish_omega=omega, **v)
    combos = [(i, k) for i in range(len(VARIANTS)) for k in POLISH]
    rows = {}
    for i, k in combos:
        run(VARIANTS[i], k)                      # warm-up: code objects, every shape's forward graph
        rows[i, k] = TB.quality(run(VARIANTS[i], k), data, target)
    times = {c: [] for c in combos}
    for _ in range(reps):                        # all rows take turns: drift hits them alike
        for i, k in combos:
            times[i, k].append(TB.timed_ms(lambda: run(VARIANTS[i], k))[1])
    out = []
    for i, k in combos:
        ms = times[i, k]
        row = {**VARIANTS[i], "polish": k, **rows[i, k], "ms": statistics.median(ms), "ms_min": min(ms),
               "ms_max": max(ms)}
        base = statistics.median(times[i, 0])
        row["ms_over_polish_0"] = row["ms"] / base
        if k == 0:
            row["ms_parent_commit"] = parent_ms(VARIANTS[i], start, target)
        out.append(row)
    bil = S.interpolate_batched(data["u"][start], target, "bilinear", True)
    return {"from": start, "to": target, "omega": omega, "rows": out,
            "bilinear_multi_level": TB.quality(bil, data, target)}


def kernel_alone(data, n, reps, E, omega, calls=20):
    K = H.pde_relax_sweeps_per_launch()
    u, f, th = data["u"][n].contiguous(), data["f"][n].contiguous(), data["theta"][n].contiguous()
    floor_ms = E * n * n * BYTES_PER_NODE / HBM_PEAK * 1e3
    rows = []
    cases = [K, 2 * K]
    for sweeps in cases:
        P.relax(u, f, th, sweeps, omega)
    times = {s: [] for s in cases}
    for _ in range(reps):
        for sweeps in cases:
            times[sweeps].append(TB.timed_ms(lambda: [P.relax(u, f, th, sweeps, omega) for _ in range(calls)])[1]
                                 / calls)
    for sweeps in cases:
        ms = times[sweeps]
        med = statistics.median(ms)
        launches = -(-sweeps // K)
        rows.append({"E": E, "n": n, "sweeps": sweeps, "launches": launches, "ms": med, "ms_min": min(ms),
                     "ms_max": max(ms), "traffic_floor_ms_per_launch": floor_ms,
                     "floor_over_measured": launches * floor_ms / med,
                     "gb_per_s_of_the_floor_traffic": launches * E * n * n * BYTES_PER_NODE / (med * 1e-3) / 1e9})
    return {"sweeps_per_launch": K, "tile": H.RELAX_TILE, "hbm_peak_bytes_per_s": HBM_PEAK,
            "bytes_per_node_per_launch": BYTES_PER_NODE,
            "timing": "poisson.relax calls (output and workspace allocation from the caching allocator included), "
                      "%d back to back between two HIP events, median of alternating repeats" % calls,
            "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model_path", default=None, help="a checkpoint with model_state_dict; default: train here")
    ap.add_argument("--train-steps", type=int, default=1500)
    ap.add_argument("--train-batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--examples", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--target", type=int, default=640)
    ap.add_argument("--omega", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("relax_bench: no GPU (a timing needs one)")
    if a.model_path:
        from superresolution_for_pdes_amd.compare_methods import load_model
        model, how = load_model(a.model_path, "cuda"), {"source": os.path.basename(a.model_path)}
    else:
        model, how = TB.train(a)
    print(json.dumps({"model": how}), flush=True)
    E = a.examples
    levels, r = [], 40
    while r < a.target:
        r *= 2
        levels.append(r)
    np.random.seed(a.seed)
    data = S.solve_multi_resolution(E, 40, levels, solver="dst")
    study = cascade(model, data, 40, a.target, a.reps, a.omega)
    print(json.dumps(study), flush=True)
    alone = kernel_alone(data, a.target, a.reps, E, a.omega)
    result = {"tool": "tools/relax_bench.py", "device": torch.cuda.get_device_name(0), "examples": E, "seed": a.seed,
              "reps": a.reps, "tile": TB.TILE, "solver": "dst", "model": how,
              "timing": "HIP events around one upscale_cascade call of all examples, ms; median of alternating repeats "
                        "after warm-up, with min and max",
              "figures": "means over the examples; seam = jump_at_tile_lines - jump_elsewhere (mean |error jump| "
                         "across fine-grid lines at multiples of 40 against all other lines)",
              "cascade": study, "kernel_alone": alone}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
