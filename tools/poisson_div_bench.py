"""Time the divergence-form solver (poisson.solve_div: CG preconditioned by the sine-transform solve) beside the
pointwise solvers of the same box, its operator alone against its traffic floor, and one streamed batch.

    python tools/poisson_div_bench.py [--out profiles/poisson_div_bench.json] [--repeats 7]

(i)   Per (n, B): theta ~ U(0.5, 2) per pixel, f the project's forcing with k ~ U(0.5, 12) (rng 100).  solve_div in its
      default mode (chunks of 8 iterations, the done flags read between chunks) and in fixed mode (the smallest
      multiple of 8 that default mode ran, no host read), for both face means, with the iteration counts (min / max
      over the batch); beside them solve_batched(method="cg") and method="dst" on the same f and theta -- those solve
      the pointwise equation, another problem of the same size.  HIP-event time per call over a ~50 ms window of
      back-to-back calls, all variants alternating inside each repeat, the median of the repeats with min - max.
      ``per_iteration_ms`` is the fixed-mode time over its iteration count, ``dst_solves_equivalent`` that over the
      sine-transform solve: what one iteration costs in units of its preconditioner.
(ii)  apply_div alone at the same shapes against its traffic floor: u and theta read, y written, 24 B per node, over
      the HBM peak of --hbm-tbs (8 TB/s, MI355X).  Fields that fit the 256 MB Infinity Cache can beat that floor.
(iii) One SampleStream batch (next_batch) at --batch with theta ~ U(0.5, 2): form="pointwise" with the sine-transform
      solver against form="divergence" with each mean (30 fixed iterations), alternating.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from superresolution_for_pdes_amd import online as O  # noqa: E402
from superresolution_for_pdes_amd import poisson as P  # noqa: E402

SIZES = "40:1024,80:1024,640:4"


def timed_ms(fn, calls=1):
    """HIP-event milliseconds per call of ``calls`` back-to-back calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def window_calls(fn, target_ms=50.0, most=64):
    """Calls per timed window: enough for ~target_ms, so that a short call is not a timing of the clock."""
    return max(1, min(most, int(target_ms / max(timed_ms(fn), 1e-3))))


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def alternating(fns, repeats):
    """{name: summary of ms per call}: warm-up, window sizes, then the variants taking turns inside every repeat."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    calls = {k: window_calls(fn) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, calls[k]))
    return {k: dict(summary(v), calls_per_window=calls[k]) for k, v in ms.items()}


def bench_solves(n, B, rng, repeats):
    f = P.forcing_batched(rng.uniform(0.5, 12.0, (B, 2)), n)
    th = torch.from_numpy(rng.uniform(0.5, 2.0, (B, n, n))).cuda()
    P.dst_plan(n)
    row = {"n": n, "B": B, "theta": "U(0.5, 2) per pixel"}
    fns = {"pointwise_cg": lambda: P.solve_batched(f, th, method="cg"),
           "pointwise_dst": lambda: P.solve_batched(f, th, method="dst")}
    fixed = {}
    for mean in P.FACE_MEANS:
        u, iters, resid = P.solve_div(f, th, face_mean=mean, return_info=True)
        fixed[mean] = 8 * -(-int(iters.max()) // 8)
        m = P.residual_metrics(u, f, th, form="divergence", face_mean=mean)[:, 0]
        row[mean] = {"iters_min": int(iters.min()), "iters_max": int(iters.max()), "resid_max": float(resid.max()),
                     "fixed_iters": fixed[mean],
                     "residual_rms_over_rms_f_max": float((m / f.flatten(1).pow(2).mean(1).sqrt()).max())}
        fns[mean + "_default"] = lambda mean=mean: P.solve_div(f, th, face_mean=mean)
        fns[mean + "_fixed"] = lambda mean=mean: P.solve_div(f, th, face_mean=mean, maxit=fixed[mean],
                                                             check_every=0, check=False)
        fns[mean + "_apply"] = lambda mean=mean: P.apply_div(f, th, face_mean=mean)
    t = alternating(fns, repeats)
    row["pointwise_cg"], row["pointwise_dst"] = t["pointwise_cg"], t["pointwise_dst"]
    for mean in P.FACE_MEANS:
        per_it = t[mean + "_fixed"]["ms"] / fixed[mean]
        row[mean].update({"default": t[mean + "_default"], "fixed": t[mean + "_fixed"],
                          "per_iteration_ms": round(per_it, 5),
                          "dst_solves_equivalent": round(per_it / t["pointwise_dst"]["ms"], 2)})
    return row, {mean: t[mean + "_apply"] for mean in P.FACE_MEANS}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="n:B pairs")
    ap.add_argument("--batch", type=int, default=1024, help="the streamed batch of (iii)")
    ap.add_argument("--calib", type=int, default=256, help="calibration samples of the streams of (iii)")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak for the traffic floor, TB/s")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("poisson_div_bench: no GPU")
    rng = np.random.default_rng(100)
    solves, applies = [], []
    for n, B in [tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",") if s]:
        row, app = bench_solves(n, B, rng, args.repeats)
        solves.append(row)
        print(json.dumps(row), flush=True)
        nbytes = 24 * B * n * n
        floor_ms = nbytes / (args.hbm_tbs * 1e12) * 1e3
        arow = {"n": n, "B": B, "bytes": nbytes, "floor_ms": round(floor_ms, 5)}
        for mean, t in app.items():
            arow[mean] = dict(t, tbs=round(nbytes / (t["ms"] * 1e-3) / 1e12, 3), floor_over_ms=round(floor_ms / t["ms"], 3))
        applies.append(arow)
        print(json.dumps(arow), flush=True)
    kw = dict(theta_range=(0.5, 2.0), n_calib=args.calib)
    streams = {"pointwise_dst": O.SampleStream(42, args.batch, solver="dst", **kw)}
    for mean in P.FACE_MEANS:
        streams["divergence_" + mean] = O.SampleStream(42, args.batch, form="divergence", face_mean=mean, **kw)
    stream_row = {"batch": args.batch, "pcg_iters": streams["divergence_harmonic"].pcg_iters,
                  **alternating({k: s.next_batch for k, s in streams.items()}, args.repeats)}
    print(json.dumps(stream_row), flush=True)
    rec = {"tool": "tools/poisson_div_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around a ~50 ms window of back-to-back calls, per call; median of alternating repeats "
                     "after warm-up",
           "traffic_model": f"apply_div: 24 B per node (u, theta read, y written) over {args.hbm_tbs} TB/s",
           "solves": solves, "apply_div": applies, "stream_batch": stream_row}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
