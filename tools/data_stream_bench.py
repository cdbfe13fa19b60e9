"""Time the streamed-sample generator (online.SampleStream) on one GPU: what a freshly generated batch costs alone,
and what it costs inside the training step that consumes it.

    python tools/data_stream_bench.py [--out profiles/data_stream_bench.json] [--batch 1024] [--repeats 7]

(i)  One generated batch alone (``next_batch()``: draws, forcing, solves, window, normalised inputs) at the default mix
     of standard and subdomain samples, for theta = 1 and theta ~ U(0.5, 2), with the sine-transform solver and with
     the CG: HIP-event time per batch over a window of back-to-back batches, the four variants alternating, the median
     of the repeats with min - max.  Beside it the generator's kernels stand-alone: every C entry of one batch timed
     in a window of its own on preallocated buffers, and their sum (the batch with no host work between launches).
(ii) The training step of train_model (zero_grad, forward, MSE, backward, fused clip + AdamW) at the same batch size,
     fed by DeviceBatchLoader from a fixed device-resident set against the same step fed by OnlineBatchLoader, in the
     same process, alternating; the overhead is the difference of the medians.
(iii) Kernel times, from a profiler run of its own:
         rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ds -- \
             python tools/data_stream_bench.py --profile-batches 50
     runs nothing but 50 batches (plus the calibration set, sized like one batch, and one warm-up batch: 52 batches of
     identical launches), and ``--kernel-stats ones=DIR/.../ds_kernel_stats.csv`` folds that file's srpde kernels, per
     batch, into the record -- the generator's kernel time with no host in it.
Needs a GPU: there is no fallback."""
import argparse
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superresolution_for_pdes_amd import hipops as H  # noqa: E402
from superresolution_for_pdes_amd import online as O  # noqa: E402
from superresolution_for_pdes_amd import poisson as P  # noqa: E402

THETA = {"ones": None, "uniform": (0.5, 2.0)}


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


def alternating(fns, repeats, calls):
    """{name: [ms per call] * repeats}, the variants taking turns inside every repeat."""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, calls[k]))
    return ms


def kernel_stages(stream):
    """{stage: a call of one C entry of a batch on buffers made here} -- the launches of SampleStream._fields and
    _assemble, one by one."""
    s, dev = stream, stream.device
    nc, nf, nsf = s.n_coarse, s.n_fine, s.n_superfine
    B = s.batch_size
    n_std = O.n_standard(B, s.sub_fraction)
    n_sub = B - n_std
    k, _, th_f, th_c = H.stream_draw(s.seed, 0, n_std, s.k_std, s.theta_range, n=nf, theta_half=True, device=dev)
    ks, starts, th, _ = H.stream_draw(s.seed, n_std, n_sub, s.k_sub, s.theta_range, n=nsf, max_start=nsf - nf,
                                      device=dev)
    f_f, f_c, f = P.forcing_batched(k, nf, dev), P.forcing_batched(k, nc, dev), P.forcing_batched(ks, nsf, dev)
    u_f, u_c, u = s._solve(f_f, th_f), s._solve(f_c, th_c), s._solve(f, th)
    f32 = dict(dtype=torch.float32, device=dev)
    out = tuple(torch.empty(B, m, m, **f32) for m in (nf, nf, nf, nc))
    fields = dict(zip(("u_fine", "f_fine", "theta_fine", "u_coarse"), out))
    return {
        "draw_standard": lambda: H.stream_draw(s.seed, 0, n_std, s.k_std, s.theta_range, n=nf, theta_half=True,
                                               device=dev),
        "draw_subdomain": lambda: H.stream_draw(s.seed, n_std, n_sub, s.k_sub, s.theta_range, n=nsf,
                                                max_start=nsf - nf, device=dev),
        "forcing_fine": lambda: P.forcing_batched(k, nf, dev),
        "forcing_coarse": lambda: P.forcing_batched(k, nc, dev),
        "forcing_superfine": lambda: P.forcing_batched(ks, nsf, dev),
        "solve_fine": lambda: s._solve(f_f, th_f),
        "solve_coarse": lambda: s._solve(f_c, th_c),
        "solve_superfine": lambda: s._solve(f, th),
        "window_standard": lambda: H.stream_window(u_f, f_f, th_f, None, nf, u_coarse_in=u_c,
                                                   out=tuple(t[:n_std] for t in out)),
        "window_subdomain": lambda: H.stream_window(u, f, th, starts, nf, out=tuple(t[n_std:] for t in out)),
        "assemble": lambda: s._assemble(fields),
    }


def bench_generator(args):
    streams = {(t, m): O.SampleStream(42, args.batch, theta_range=THETA[t], solver=m, n_calib=args.calib)
               for t in THETA for m in P.SOLVERS}
    fns = {key: s.next_batch for key, s in streams.items()}
    for fn in fns.values():                                   # warm-up
        fn()
    torch.cuda.synchronize()
    calls = {key: window_calls(fn) for key, fn in fns.items()}
    ms = alternating(fns, args.repeats, calls)
    rows = []
    for (t, m), s in streams.items():
        stages = kernel_stages(s)
        for fn in stages.values():
            fn()
        torch.cuda.synchronize()
        scalls = {k: window_calls(fn, 20.0) for k, fn in stages.items()}
        sms = {k: statistics.median(v) for k, v in alternating(stages, args.repeats, scalls).items()}
        row = {"theta": t, "solver": m, "batch": args.batch, "standard": O.n_standard(args.batch, s.sub_fraction),
               "subdomain": args.batch - O.n_standard(args.batch, s.sub_fraction), "calls_per_window": calls[(t, m)],
               **{"batch_" + k: v for k, v in summary(ms[(t, m)]).items()},
               "stage_ms": {k: round(v, 4) for k, v in sms.items()}, "stage_sum_ms": round(sum(sms.values()), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def profile_batches(args):
    """Only batches, for a kernel trace: calibration (batch-sized), one warm-up batch and --profile-batches more."""
    s = O.SampleStream(42, args.batch, theta_range=THETA[args.profile_theta], solver=args.step_solver,
                       n_calib=args.batch)
    for _ in range(1 + args.profile_batches):
        s.next_batch()
    torch.cuda.synchronize()
    print(json.dumps({"profiled_batches": 2 + args.profile_batches, "theta": args.profile_theta,
                      "solver": args.step_solver, "batch": args.batch}))


def kernel_stats(path, batches):
    """The library's kernels of a rocprofv3 kernel_stats.csv, per batch."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "srpde::" in r["Name"]]
    ks = [{"kernel": r["Name"].split("(")[0].replace("void ", ""), "calls_per_batch": round(int(r["Calls"]) / batches, 3),
           "us_per_batch": round(float(r["TotalDurationNs"]) / 1e3 / batches, 3)}
          for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))]
    return {"batches": batches, "kernels": ks,
            "kernel_sum_ms": round(sum(k["us_per_batch"] for k in ks) / 1e3, 4)}


def bench_step(args):
    from superresolution_for_pdes_amd.functional import MSELoss
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.optim import FusedAdamW
    from superresolution_for_pdes_amd.train_enhanced import DeviceBatchLoader
    rows = []
    for t in THETA:
        torch.manual_seed(42)
        stream = O.SampleStream(42, args.batch, theta_range=THETA[t], solver=args.step_solver, n_calib=args.calib)
        fixed = DeviceBatchLoader(stream.frozen_set(2 * args.batch, O.CALIB_FIRST), args.batch, shuffle=True, seed=42)
        model = UNet().to("cuda")
        model.apply(init_weights)
        model.train()
        criterion = MSELoss()
        opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-4)
        acc = torch.zeros((), dtype=torch.float64, device="cuda")

        def feed(loader):
            while True:
                yield from loader
        sources = {"fixed": feed(fixed), "online": feed(O.OnlineBatchLoader(stream, args.steps))}

        def step_from(src):
            def step():
                inputs, targets = next(src)
                opt.zero_grad()
                loss = criterion(model(inputs), targets)
                loss.backward()
                opt.step(max_grad_norm=1.0)
                acc.add_(loss.detach())
            return step
        fns = {k: step_from(src) for k, src in sources.items()}
        for fn in itertools.chain.from_iterable([fns.values()] * args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = alternating(fns, args.repeats, {k: args.steps for k in fns})
        fx, on = summary(ms["fixed"]), summary(ms["online"])
        row = {"theta": t, "solver": args.step_solver, "batch": args.batch, "steps_per_window": args.steps,
               **{"step_fixed_" + k: v for k, v in fx.items()}, **{"step_online_" + k: v for k, v in on.items()},
               "online_overhead_ms": round(on["ms"] - fx["ms"], 4),
               "online_overhead_percent": round(100.0 * (on["ms"] - fx["ms"]) / fx["ms"], 3),
               "loss_finite": bool(torch.isfinite(acc))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed window")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per batch source")
    ap.add_argument("--calib", type=int, default=2048, help="calibration samples of the frozen statistics")
    ap.add_argument("--step-solver", choices=P.SOLVERS, default="dst", help="the stream's solver in part (ii)")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    ap.add_argument("--profile-batches", type=int, default=0, help="run only this many batches (for a kernel trace)")
    ap.add_argument("--profile-theta", choices=tuple(THETA), default="ones")
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="THETA=CSV",
                    help="rocprofv3 kernel_stats.csv files of --profile-batches runs, e.g. ones=DIR/ds_kernel_stats.csv")
    ap.add_argument("--kernel-stats-batches", type=int, default=52, help="batches in that run (2 + --profile-batches)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("data_stream_bench: no GPU")
    if args.profile_batches:
        return profile_batches(args)
    rec = {"tool": "tools/data_stream_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around a window of back-to-back calls, per call; median of alternating repeats after "
                     "warm-up, with min and max",
           "generated_batch": bench_generator(args), "training_step": bench_step(args)}
    if args.kernel_stats:
        rec["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats around --profile-batches runs (solver "
                                         f"{args.step_solver}); the library's kernels, per batch",
                               **{spec.split("=", 1)[0]: kernel_stats(spec.split("=", 1)[1], args.kernel_stats_batches)
                                  for spec in args.kernel_stats}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
