"""What overlapping windows and ground-truth-free statistics do to the cascade (tiled_inference, csrc/tiled.hip).

    python tools/tiled_inference_bench.py [--model_path best_model.pth] [--out profiles/tiled_inference_bench.json]

E seeded fields of resolution_comparison_statistical.solve_multi_resolution, 40 -> 640, run through
tiled_inference.upscale_cascade at every combination of stride (20 = the disjoint tiles of the existing cascade, 10,
5), window (linear, flat) and statistics (truth = the reference's label leak, input = none needed).  Per combination:
  * MAE and RMSE against the 640^2 solution (hipops.field_metrics) and the residual RMS of the discrete equation
    (poisson.residual_metrics), means over the examples;
  * a seam figure: the mean |jump of the error| across the fine-grid lines at multiples of 40 (where the disjoint
    tiling pastes two outputs side by side) minus the same mean over all other lines;
  * the time per call: HIP events, median of ``--reps`` repeats in which the combinations take turns.
A size that is no multiple of the tile (50 -> 100) runs beside it, with the multi-level bilinear baseline of both
cases for scale.  Without --model_path the model is trained here for ``--train-steps`` online steps (sample stream,
sine-transform solver, theta ~ U(0.5, 2), seed and step count recorded): a short run, so the figures compare the
inference variants on one model and say nothing about what a fully trained model reaches.  A recorded observation,
not a pass criterion.  Needs a GPU: there is no fallback."""
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
from superresolution_for_pdes_amd import poisson as P  # noqa: E402
from superresolution_for_pdes_amd import resolution_comparison_statistical as S  # noqa: E402
from superresolution_for_pdes_amd import tiled_inference as T  # noqa: E402

TILE = 20
STRIDES = (20, 10, 5)
WINDOWS = ("linear", "flat")
STATS = ("truth", "input")


def train(args):
    """A seeded short online run (MSE, fused clip + AdamW, the defaults of train_enhanced) -> (model, record)."""
    from superresolution_for_pdes_amd import online as O
    from superresolution_for_pdes_amd.functional import MSELoss
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.optim import FusedAdamW
    torch.manual_seed(args.seed)
    stream = O.SampleStream(args.seed, args.train_batch, theta_range=(0.5, 2.0), solver="dst")
    model = UNet().to("cuda")
    model.apply(init_weights)
    model.train()
    crit = MSELoss()
    opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-4)
    seen = {}
    for step in range(args.train_steps):
        inputs, targets = stream.next_batch()
        opt.zero_grad()
        loss = crit(model(inputs), targets)
        loss.backward()
        opt.step(max_grad_norm=1.0)
        if step in (0, args.train_steps - 1):
            seen[step] = float(loss.detach())
    model.eval()
    return model, {"source": "trained here", "seed": args.seed, "steps": args.train_steps, "batch": args.train_batch,
                   "data": "online.SampleStream, solver dst, theta ~ U(0.5, 2), half standard / half subdomain",
                   "loss": "MSE", "optimizer": "FusedAdamW lr 2e-4 wd 1e-4, grad clip 1.0",
                   "train_loss_first": seen[0], "train_loss_last": seen[args.train_steps - 1]}


def seam_figure(pred, gt, period=2 * TILE):
    """mean |jump of the error| across the lines between fine rows / columns k - 1 and k with k a multiple of
    ``period``, minus the same mean over every other line; both axes, all examples.  -> (difference, seam mean,
    other mean)."""
    err = pred.double() - gt
    n = err.shape[-1]
    jumps = ((err[:, 1:, :] - err[:, :-1, :]).abs().mean(dim=(0, 2)),
             (err[:, :, 1:] - err[:, :, :-1]).abs().mean(dim=(0, 1)))
    at = (torch.arange(1, n, device=err.device) % period) == 0
    seam = float(torch.cat([j[at] for j in jumps]).mean())
    other = float(torch.cat([j[~at] for j in jumps]).mean())
    return seam - other, seam, other


def quality(pred, data, res):
    gt = data["u"][res]
    mt = H.field_metrics(pred.contiguous(), gt).mean(dim=0).tolist()
    rm = P.residual_metrics(pred, data["f"][res], data["theta"][res]).mean(dim=0).tolist()
    d, seam, other = seam_figure(pred, gt)
    return {"mae": mt[0], "rmse": mt[1], "max_error": mt[2], "residual_rms": rm[0], "seam": d,
            "jump_at_tile_lines": seam, "jump_elsewhere": other}


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def tiles_total(start, target, stride, E):
    n, r = 0, start
    while r < target:
        n += E * len(T.tile_starts(r, TILE, stride)) ** 2
        r *= 2
    return n


def study(model, data, start, target, strides, reps, E):
    """Every (stride, window, stats) combination from ``start`` to ``target``: quality, then alternating timings."""
    def run(stride, window, stats):
        return T.upscale_cascade(model, data["u"][start], data["f"], data["theta"], target, tile=TILE, stride=stride,
                                 window=window, stats=stats, u_truth=data["u"])
    combos = [(s, w, st) for s in strides for w in WINDOWS for st in STATS]
    rows = {}
    for c in combos:
        run(*c)                                  # warm-up: code objects, every shape's forward graph
        rows[c] = quality(run(*c), data, target)
    times = {c: [] for c in combos}
    for _ in range(reps):                        # the combinations take turns: drift hits all of them alike
        for c in combos:
            times[c].append(timed_ms(lambda: run(*c))[1])
    out = []
    for c in combos:
        ms = times[c]
        out.append({"stride": c[0], "window": c[1], "stats": c[2], "tiles": tiles_total(start, target, c[0], E),
                    **rows[c], "ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)})
    base = {r["stats"]: r["ms"] for r in out if r["stride"] == strides[0] and r["window"] == "linear"}
    for r in out:
        r["ms_over_stride_%d" % strides[0]] = r["ms"] / base[r["stats"]]
    bil = S.interpolate_batched(data["u"][start], target, "bilinear", True)
    return {"from": start, "to": target, "rows": out, "bilinear_multi_level": quality(bil, data, target)}


def kernels(data, S0, reps, E, calls=20):
    """The three new passes alone at the largest level (S0 -> 2 S0), per stride: ms per call (``calls`` back to
    back between two events, median of ``reps``) and the rate over the bytes each has to move -- every input read
    once, every output written once (the overlapping reads of the same field are left to the caches)."""
    u, f, th = data["u"][S0], data["f"][2 * S0], data["theta"][2 * S0]
    rows = []
    for stride in STRIDES:
        m = len(T.tile_starts(S0, TILE, stride))
        stats, _ = H.tiled_level_stats(u, f, th)
        x = H.tiled_assemble(u, f, th, stats, TILE, stride)
        y = x[:, 0:1].contiguous()
        fields = E * S0 * S0 * 8
        passes = {
            "stats": (lambda: H.tiled_level_stats(u, f, th), 9 * fields),
            "assemble": (lambda: H.tiled_assemble(u, f, th, stats, TILE, stride), 9 * fields + x.numel() * 4),
            "blend_linear": (lambda: H.tiled_blend_denorm(y, stats, E, S0, TILE, stride, "linear"),
                             y.numel() * 4 + 4 * fields),
            "blend_flat": (lambda: H.tiled_blend_denorm(y, stats, E, S0, TILE, stride, "flat"),
                           y.numel() * 4 + 4 * fields),
        }
        row = {"stride": stride, "S": S0, "tiles": E * m * m}
        for name, (fn, nbytes) in passes.items():
            fn()
            ms = []
            for _ in range(reps):
                ms.append(timed_ms(lambda: [fn() for _ in range(calls)])[1] / calls)
            med = statistics.median(ms)
            row[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "bytes": nbytes,
                         "gb_per_s": nbytes / (med * 1e-3) / 1e9}
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model_path", default=None, help="a checkpoint with model_state_dict; default: train here")
    ap.add_argument("--train-steps", type=int, default=1500)
    ap.add_argument("--train-batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--examples", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--target", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_inference_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tiled_inference_bench: no GPU (a timing needs one)")
    if a.model_path:
        from superresolution_for_pdes_amd.compare_methods import load_model
        model, how = load_model(a.model_path, "cuda"), {"source": os.path.basename(a.model_path)}
    else:
        model, how = train(a)
    print(json.dumps({"model": how}), flush=True)
    E = a.examples
    levels, r = [], 40
    while r < a.target:
        r *= 2
        levels.append(r)
    np.random.seed(a.seed)
    data = S.solve_multi_resolution(E, 40, levels, solver="dst")
    main_study = study(model, data, 40, a.target, STRIDES, a.reps, E)
    print(json.dumps(main_study), flush=True)
    np.random.seed(a.seed + 1)
    odd = S.solve_multi_resolution(E, 50, [100], solver="dst")
    odd_study = study(model, odd, 50, 100, (10, 5), a.reps, E)
    kernel_rows = kernels(data, a.target // 2, a.reps, E)
    result = {"tool": "tools/tiled_inference_bench.py", "device": torch.cuda.get_device_name(0), "examples": E,
              "seed": a.seed, "reps": a.reps, "tile": TILE, "solver": "dst", "model": how,
              "timing": "HIP events around one upscale_cascade call of all examples, ms; median of alternating "
                        "repeats after warm-up, with min and max",
              "figures": "means over the examples; seam = jump_at_tile_lines - jump_elsewhere (mean |error jump| "
                         "across fine-grid lines at multiples of 40 against all other lines)",
              "cascade": main_study, "not_a_multiple_of_the_tile": odd_study, "kernels_alone": kernel_rows}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
