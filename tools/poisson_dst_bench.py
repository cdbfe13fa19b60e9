"""Time poisson.solve_batched(method="cg") against method="dst" on the same box, at bench.py's Poisson sizes
(same draws: rng 100, k ~ U(0.5, 12), theta ~ U(0.5, 2)) plus 1280:1 for the direct solver alone (the CG takes
~4,200 iterations there; the size shows the direct solver beyond the usual range).

    python tools/poisson_dst_bench.py [--out profiles/poisson_dst_bench.json] [--repeats 7]

Per size: HIP-event time per call over a window of back-to-back calls (~50 ms; plans built, both methods
warmed up, the two methods alternating, the median of the repeats), the ratio cg / dst, the direct solver's
achieved fp64 rate (4 products x 2 n^3 flop per problem over its time: the algorithm's operations, not the
padded tiles'), and the relative L2 difference of the two solutions (worst problem).  Needs a GPU: there is
no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from superresolution_for_pdes_amd import poisson as P  # noqa: E402

SIZES = "40:1024,80:1024,160:64,320:16,640:4"
DST_ONLY = "1280:1"


def timed_ms(fn, calls=1):
    """HIP-event milliseconds per call of ``calls`` back-to-back calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def parse_sizes(text):
    return [tuple(int(v) for v in s.split(":")) for s in text.split(",") if s]


def dst_flop(B, n):
    return 4 * 2 * B * n ** 3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="n:B pairs timed with both methods")
    ap.add_argument("--dst-only", default=DST_ONLY, help="n:B pairs timed with the direct solver alone")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("poisson_dst_bench: no GPU")
    both = parse_sizes(args.sizes)
    rng = np.random.default_rng(100)
    rows = []
    for n, B in both + parse_sizes(args.dst_only):
        with_cg = (n, B) in both
        f = P.forcing_batched(rng.uniform(0.5, 12.0, (B, 2)), n)
        th = torch.from_numpy(rng.uniform(0.5, 2.0, (B, n, n))).cuda()
        P.dst_plan(n)
        methods = ("cg", "dst") if with_cg else ("dst",)
        sol = {m: P.solve_batched(f, th, method=m) for m in methods}          # warm-up
        torch.cuda.synchronize()
        # calls per timed window: enough for ~50 ms, so that a sub-millisecond solve is not a timing of the clock
        calls = {m: max(1, min(64, int(50.0 / max(timed_ms(lambda: P.solve_batched(f, th, method=m)), 1e-3))))
                 for m in methods}
        ms = {m: [] for m in methods}
        for _ in range(args.repeats):
            for m in methods:                                                 # alternating
                ms[m].append(timed_ms(lambda: P.solve_batched(f, th, method=m), calls[m]))
        med = {m: statistics.median(v) for m, v in ms.items()}
        row = {"n": n, "B": B, "dst_ms": round(med["dst"], 4), "dst_ms_min": round(min(ms["dst"]), 4),
               "dst_ms_max": round(max(ms["dst"]), 4), "calls_per_window": calls,
               "dst_fp64_tflops": round(dst_flop(B, n) / (med["dst"] * 1e-3) / 1e12, 3),
               "dst_path": "fused" if n <= int(P.query("srpde_poisson_dst_lds_max_n")) else "general"}
        if with_cg:
            d = (sol["dst"] - sol["cg"]).flatten(1).norm(dim=1) / sol["cg"].flatten(1).norm(dim=1)
            row.update({"cg_ms": round(med["cg"], 4), "cg_ms_min": round(min(ms["cg"]), 4),
                        "cg_ms_max": round(max(ms["cg"]), 4), "cg_over_dst": round(med["cg"] / med["dst"], 2),
                        "rel_l2_dst_vs_cg": float(d.max())})
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/poisson_dst_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around a ~50 ms window of solve_batched calls, per call; median of alternating repeats "
                     "after warm-up",
           "flop_model": "dst: 4 products x 2 n^3 per problem", "sizes": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
